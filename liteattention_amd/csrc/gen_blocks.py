"""Shared by the body generators (gen_fwd_x64.py, gen_fwd_x64_fp8.py, gen_fwd_x64_m16.py): the blocks a body is made of wherever they
are the same text under a parameter - the out-of-line blocks of a step, the LDS-DMA issue, the loop skeleton and the common pieces of
the prologue. gen_asm.py is the assembler core and the ABI underneath; what differs in substance (every step() schedule, the forms of
P, the transposed state of the 16x16x32 body, the W2 step, the half-vote state machine) stays in its generator.

A block takes the registers it touches as arguments; `R` is the generator's register map (a namespace with T, QBS and the running
state MLOC, MTRUE, MREF, MTHR, NMS, ALPHA, L0, L1, NEGINF: lists are per q-block). Labels are numbered in call order (new_label):
a block asks for its labels where the code it replaced did.
"""
from gen_asm import *


# ---------------------------------------------------------------- out-of-line blocks of a step
def flush_block(flush_label, back_label, T, tail=None):
    """Out of line: doflags word |= domask by one lane; next word, domask = 0, bit = 1. Drains lgkmcnt (keeps counted waits valid);
    `tail` replaces the drain (half-vote form: the activity window's refill, which ends in its own)."""
    label(flush_label)
    flush_domask(T[4], T[5])
    emit(f"s_add_u32 {s(S_DOWORD)}, {s(S_DOWORD)}, 4")
    emit(f"s_mov_b32 {s(S_BIT)}, 1")
    if tail:
        tail()
    else:
        emit("s_waitcnt lgkmcnt(0)")
    emit(f"s_branch {back_label}")


def inval_block(lbl, back, R):
    """Out of line (last step of a walk): the tile max and -m_ref*c := -inf, so exp2(S*c - inf) = 0 for the tile that does not exist."""
    label(lbl)
    for qb in R.QBS:
        emit(f"v_mov_b32 {v(R.MLOC[qb])}, {v(R.NEGINF)}")
        emit(f"v_mov_b32 {v(R.NMS[qb])}, {v(R.NEGINF)}")
    emit(f"s_branch {back}")


def rescale_o_block(lbl, back, T, scaled, nops=2, tail=None):
    """Out of line (rare): O^T *= alpha (AGPR -> VGPR -> AGPR) after the PV MFMAs have drained (`nops` x 16 wait states).
    scaled: (alpha register, accumulator range) per q-block; tail: what else is rescaled with O."""
    label(lbl)
    for _ in range(nops):
        emit("s_nop 15")
    for alpha, acc in scaled:
        for base in acc[::8]:
            for k in range(8):
                emit(f"v_accvgpr_read_b32 {v(T[k])}, a{base + k}")
            for k in range(8):
                emit(f"v_mul_f32 {v(T[k])}, {v(T[k])}, {v(alpha)}")
            for k in range(8):
                emit(f"v_accvgpr_write_b32 a{base + k}, {v(T[k])}")
    if tail:
        tail()
    emit(f"s_mov_b32 {s(S_RESC)}, 0")
    emit("s_nop 7")
    emit(f"s_branch {back}")


def rare_rescale_block(rare_label, back_label, R, set_nms=None, l_in_vgprs=True):
    """Out of line: m_ref follows m_true; alpha = exp2((m_ref_old - m_true)*c); l *= alpha (where l lives in VGPRs); O rescale flagged.
    set_nms(qb): how -m_ref*c is set (default: NMS = -c * m_ref)."""
    label(rare_label)
    for qb in R.QBS:
        emit(f"v_sub_f32 {v(R.T[2 + qb])}, {v(R.MREF[qb])}, {v(R.MTRUE[qb])}")
    for qb in R.QBS:
        emit(f"v_mul_f32 {v(R.T[2 + qb])}, {s(S_C)}, {v(R.T[2 + qb])}")
    for qb in R.QBS:
        emit(f"v_exp_f32 {v(R.ALPHA[qb])}, {v(R.T[2 + qb])}")
    for qb in R.QBS:
        emit(f"v_mov_b32 {v(R.MREF[qb])}, {v(R.MTRUE[qb])}")
    for qb in R.QBS:
        if set_nms:
            set_nms(qb)
        else:
            emit(f"v_mul_f32 {v(R.NMS[qb])}, {s(S_NEGC)}, {v(R.MREF[qb])}")
        emit(f"v_add_f32 {v(R.MTHR[qb])}, {s(S_TAU)}, {v(R.MREF[qb])}")
    for qb in R.QBS if l_in_vgprs else ():
        emit(f"v_mul_f32 {v(R.L0[qb])}, {v(R.L0[qb])}, {v(R.ALPHA[qb])}")
        emit(f"v_mul_f32 {v(R.L1[qb])}, {v(R.L1[qb])}, {v(R.ALPHA[qb])}")
    emit(f"s_mov_b32 {s(S_RESC)}, 1")
    emit(f"s_branch {back_label}")


# ---------------------------------------------------------------- pieces of a step
def row_max_chains(scores, MLOC, MLOC2):
    """In-lane max of the scores of each q-block (scores[qb]: its registers) into MLOC[qb]: two max3 chains each, interleaved over
    the q-blocks."""
    per = []
    for regs, m, m2 in zip(scores, MLOC, MLOC2):
        ops = [f"    v_max_f32 {v(m)}, {v(regs[0])}, {v(regs[1])}", f"    v_max_f32 {v(m2)}, {v(regs[2])}, {v(regs[3])}"]
        for n_, i in enumerate(range(4, len(regs), 2)):
            ch = (m, m2)[n_ & 1]
            ops.append(f"    v_max3_f32 {v(ch)}, {v(ch)}, {v(regs[i])}, {v(regs[i + 1])}")
        ops.append(f"    v_max_f32 {v(m)}, {v(m)}, {v(m2)}")
        per.append(ops)
    return [x for pair in zip(*per) for x in pair]


def dma_issue(groups, policy=""):
    """LDS-DMA of K / V pieces. groups: (SGPR of the wave's LDS window, LDS offset, lane-offset VGPR per piece, SGPR pair of the global
    base) - one M0 per group, the piece index rides on the instruction offset (applied to both the global and the LDS address)."""
    o = []
    for window, lds_off, lanes, base in groups:
        o.append(f"    s_add_u32 m0, {s(window)}, {lds_off}")
        o += [f"    global_load_lds_dwordx4 {v(r)}, {sr(base)} offset:{1024 * j}{policy}" for j, r in enumerate(lanes)]
    return o


def emit_gaps(pre, mf, post):
    """One phase: per gap the pre items, the MFMA, the fillers."""
    for p, m, q in zip(pre, mf, post):
        out.extend(p + [m] + q)


# ---------------------------------------------------------------- loop skeleton
def loop_head(phase, align, pad4):
    """Code placement: where the loop head falls inside a 32-byte fetch window moves a body's throughput by up to 2-3 % (period 32
    bytes, profiles/r05_code_placement.md), so the head is pinned: .p2align 5, then `phase` / 4 s_nop (executed once per item) - per
    body the best measured phase. The option values `align` / `pad4` override it for experiments."""
    if align or pad4:
        if align:
            out.append(f".p2align {align}")
        for _ in range(int(pad4 or "0")):
            emit("s_nop 0")
    else:
        out.append(".p2align 5")
        for _ in range(phase // 4):
            emit("s_nop 0")


def unrolled_loop(step, end_test=True, before_copy=None):
    """The loop of two step copies (step(variant, done label)), each behind its end test; the out-of-line blocks; the `done` label."""
    loop, done = new_label("loop"), new_label("done")
    label(loop)
    for variant in (0, 1):
        if before_copy:
            before_copy(variant)
        if end_test:
            emit(f"s_cmp_lt_u32 {s(S_I)}, {s(S_NTILES)}")
            emit(f"s_cbranch_scc0 {done}")
        step(variant, done)
    emit(f"s_branch {loop}")
    for blk in deferred:
        blk()
    label(done)


def flush_last_vote_word(T, nops=2):
    """Behind the loop: flush the last (partial) vote word; then the last PV MFMAs have written the accumulators (`nops` x 16)."""
    emit("; ---- flush the last (partial) vote word")
    nofl = new_label("nolastflush")
    emit(f"s_cmp_eq_u32 {s(S_DOMASK)}, 0")
    emit(f"s_cbranch_scc1 {nofl}")
    flush_domask(T[4], T[5])
    label(nofl)
    for _ in range(nops):
        emit("s_nop 15")


# ---------------------------------------------------------------- prologue
def q_row_address(T, row):
    """v[T[4]:T[5]] = address of the lane's 16 bytes of Q row min(row, seqlen_q - 1): S_T1 = seqlen_q - 1, T[6] = byte offset in the row."""
    emit(f"v_min_i32 {v(T[3])}, {v(row)}, {s(S_T1)}")
    emit(f"v_mad_u64_u32 {vr(T[4], 2)}, {sr(S_T64)}, {v(T[3])}, {s(S_QRS)}, 0")
    emit(f"v_add_co_u32 {v(T[4])}, vcc, {v(T[4])}, {v(T[6])}")
    emit(f"v_addc_co_u32 {v(T[5])}, vcc, 0, {v(T[5])}, vcc")
    emit(f"v_add_co_u32 {v(T[4])}, vcc, {s(S_QBASE)}, {v(T[4])}")
    emit(f"v_mov_b32 {v(T[7])}, {s(S_QBASE + 1)}")
    emit(f"v_addc_co_u32 {v(T[5])}, vcc, {v(T[5])}, {v(T[7])}, vcc")


def q_rows_to_agprs(T, n_qb, n_frag, frag_bytes, q_a0, row_of, loaded=None):
    """Q fragments -> v[0 ...] -> AGPRs q_a0 ...: n_frag loads of 16 bytes, frag_bytes apart, per q-block; rows past seqlen_q are ZERO
    rows. row_of(qb, again) emits what sets the lane's row of q-block qb and returns its register (again: the second pass, behind
    the loads). T[0] = the lane's 16-byte group inside a fragment."""
    emit(f"v_lshlrev_b32 {v(T[6])}, 4, {v(T[0])}")
    for qb in range(n_qb):
        q_row_address(T, row_of(qb, False))
        for f in range(n_frag):
            emit(f"global_load_dwordx4 {vr(4 * n_frag * qb + 4 * f, 4)}, {vr(T[4], 2)}, off offset:{frag_bytes * f}")
    (loaded or (lambda: emit("s_waitcnt vmcnt(0)")))()
    for qb in range(n_qb):
        emit(f"v_cmp_gt_i32 vcc, {s(S_SEQLENQ)}, {v(row_of(qb, True))}")
        for r in range(4 * n_frag * qb, 4 * n_frag * (qb + 1)):
            emit(f"v_cndmask_b32 {v(r)}, 0, {v(r)}, vcc")
    for r in range(4 * n_frag * n_qb):
        emit(f"v_accvgpr_write_b32 a{q_a0 + r}, {v(r)}")


def zero_accumulators(regs):
    emit("; ---- state")
    for r in regs:
        emit(f"v_accvgpr_write_b32 a{r}, 0")


def read_tile_table(T, TABV):
    """The tile-address table entries of positions 1..3 -> T[8:13]; TABV = &tab[2] (what step 0 reads from)."""
    emit("; ---- tile addresses of positions 1..3 from the table; K(0) fragments -> AGPRs, S(0) = K(0) Q^T, then K(1) fragments")
    emit(f"v_mov_b32 {v(T[6])}, {s(S_TAB)}")
    emit(f"ds_read_b64 {vr(T[8], 2)}, {v(T[6])} offset:32")          # tab[2].k : K(2), staged by the prologue
    emit(f"ds_read_b64 {vr(T[10], 2)}, {v(T[6])} offset:48")         # tab[3].k : K(3), staged by step 0
    emit(f"ds_read_b64 {vr(T[12], 2)}, {v(T[6])} offset:24")         # tab[1].v : V(1), staged by step 0
    emit(f"v_add_u32 {v(TABV)}, 32, {v(T[6])}")                      # step 0 reads tab[2].v and tab[4].k


def k2_base(T):
    """Behind the K(0) fragment reads: drain (the table entries have arrived too), K(2)'s address -> the DMA base."""
    emit(("DRAIN",))
    emit(f"v_readfirstlane_b32 {s(TBS[0])}, {v(T[8])}")
    emit(f"v_readfirstlane_b32 {s(TBS[0] + 1)}, {v(T[9])}")


def stage_k2(k_ops, T):
    """Behind the prologue's barrier (every wave has read K(0) and K(1): both K buffers are free): K(2) -> K buffer 0 (k_ops: its DMA
    issue; an M0 write is never adjacent to its first use); then the bases of what step 0 stages, K(3) and V(1)."""
    for it in k_ops:
        out.append(it)
        if "m0" in it:
            emit("s_nop 0")
    for dst, src in ((TBS[0], T[10]), (TBS[0] + 1, T[11]), (VBS[0], T[12]), (VBS[0] + 1, T[13])):
        emit(f"v_readfirstlane_b32 {s(dst)}, {v(src)}")


def mask_ops(T, NEGINF, lane_key, keys):
    """seqlen-k mask (mask.h:44-78): columns >= tail_valid -> -inf. keys: (key of lane_key == 0, the score registers of that key)."""
    for key, regs in keys:
        emit(f"v_add_u32 {v(T[0])}, {key}, {v(lane_key)}")
        emit(f"v_cmp_gt_i32 vcc, {s(S_TAILVALID)}, {v(T[0])}")            # key < tail_valid -> keep
        for r in regs:
            emit(f"v_cndmask_b32 {v(r)}, {v(NEGINF)}, {v(r)}, vcc")


def first_tile_mask(T, NEGINF, lane_key, keys):
    """The mask of the first walked tile (only that one can be tile k_tiles - 1: mainloop...:1626), if it is and tail_valid < 64."""
    nomask = new_label("nomask")
    emit(f"s_cmp_eq_u32 {s(S_FIRSTLAST)}, 1")                # the first walked tile is tile k_tiles - 1 (C++ shell)
    emit(f"s_cbranch_scc0 {nomask}")
    emit(f"s_cmp_lt_i32 {s(S_TAILVALID)}, 64")
    emit(f"s_cbranch_scc0 {nomask}")
    mask_ops(T, NEGINF, lane_key, keys)
    label(nomask)
