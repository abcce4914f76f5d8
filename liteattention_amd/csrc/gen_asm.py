"""Shared by the body generators (gen_fwd_x64.py, gen_fwd_x64_fp8.py, gen_fwd_x64_m16.py), gen_blocks.py and gen_epilogue.py: the assembler
core, the SGPR map and the parameter block ABI (``from gen_asm import *``). What a body is made of sits on it: gen_blocks.py, gen_epilogue.py.

The body is built in ``out`` as a list of items: a str (one line of assembly), ("LDS", text, tag) (an LDS operation whose completion
a later wait may name), ("WAIT", tag) (a counted lgkmcnt wait for the youngest LDS operation of that tag) or ("DRAIN",). ``finalize``
turns the items into lines. Out-of-line blocks are callables in ``deferred``, emitted after the loop. Generators append to ``out`` and
``deferred`` in place and never rebind them.

Parameter block: the C++ shells (la_fwd_kernel_x64.hip, la_fwd_kernel_x64_fp8.hip) write 32 words to LDS, and the body receives its
address as %1. ``read_params`` loads words 0-22 into the SGPRs of ``PARAM_WORDS``, in the shell's order. Word 23 belongs to the
half-vote form (gen_fwd_x64.py ``S_HSTRIDE``), words 24-31 to the epilogue (gen_epilogue.py).
"""
import os

out = []
deferred = []
_uid = [0]
_label_prefix = [".L"]


def emit(x):
    out.append(x if isinstance(x, tuple) else "    " + x)


def label(name):
    out.append(name + ":")


def v(i):
    return f"v{i}"


def vr(a, n):
    return f"v[{a}:{a + n - 1}]"


def ar(a, n):
    return f"a[{a}:{a + n - 1}]"


def s(i):
    return f"s{i}"


def sr(a, n=2):
    return f"s[{a}:{a + n - 1}]"


def set_label_prefix(prefix):
    """The generator's label prefix (.LX / .LF / .LM)."""
    _label_prefix[0] = prefix


def new_label(name):
    _uid[0] += 1
    return f"{_label_prefix[0]}{name}_{_uid[0]}_%="


# ---------------------------------------------------------------- options
def options(var):
    """The option set of a generator: the comma-separated words of environment variable `var`."""
    return set(x for x in os.environ.get(var, "").split(",") if x)


def opt_val(opt, key, default):
    for o in opt:
        if o.startswith(key + ":"):
            return o[len(key) + 1:]
    return default


def option_tag(opt, schedule_only):
    """Options in `schedule_only` only move instructions: the body computes the same results bit for bit. Every other option drops
    work or changes the arithmetic (pricing experiments, tools/asm_variants.py). The tag says which kind went in; build.py refuses the
    latter for the product library and records both in la_build_info() for A/B builds (--out=)."""
    wrong = sorted(o for o in opt if o.split(":")[0] not in schedule_only)
    return (f"// la_body_options: {','.join(sorted(opt)) or '-'}; wrong_results={1 if wrong else 0}"
            + (f" (PRICING ONLY, results are wrong: {','.join(wrong)})" if wrong else ""))


# ---------------------------------------------------------------- output
def finalize(opt):
    """The lines of ``out``, with counted lgkmcnt waits: LDS operations of one wave return in order."""
    lines, q = [], []
    for it in out:
        if isinstance(it, str):
            lines.append(it)
        elif it[0] == "LDS":
            lines.append("    " + it[1])
            q.append(it[2])
        elif it[0] == "WAIT":
            if it[1] in q:
                idx = max(i for i, t in enumerate(q) if t == it[1])
                lines.append(f"    s_waitcnt lgkmcnt({min(len(q) - 1 - idx, 15)})")
                q = q[idx + 1:]
        elif it[0] == "DRAIN":
            lines.append("    s_waitcnt lgkmcnt(0)" if "nowaitvm" in opt else "    s_waitcnt vmcnt(0) lgkmcnt(0)")   # nowaitvm: pricing only
            q = []
    return lines


def write_body(path, header, tag, lines):
    """The generated file: header line, option tag, the body as a C++ raw string (the shell's asm statement includes it)."""
    text = "\n".join(lines)
    with open(path, "w") as f:
        f.write(header + "\n")
        f.write(tag + "\n")
        f.write('R"ASM(\n' + text + '\n)ASM"\n')
    print(f"wrote {path}: {len(lines)} lines, {text.count('v_mfma')} MFMAs")


# ---------------------------------------------------------------- filling the MFMA gaps
def weight(it):
    """Issue cost in quad-cycles as measured (PMC: SQ_ACTIVE_INST_VALU): a transcendental takes two slots, labels none."""
    if isinstance(it, str):
        if it.endswith(":"):
            return 0
        if "v_exp_f32" in it:
            return 2
    return 1


def n_fill(items):
    return sum(weight(it) for it in items)


def distribute(queue, post, start, cap=0, end=None):
    """Append the ops of `queue` (order kept) to post[start..end-1] (end: every gap), topping every gap up to `cap` fillers (0:
    balance evenly)."""
    end = len(post) if end is None else end
    q = list(queue)
    if cap <= 0:
        total = sum(n_fill(post[t]) for t in range(start, end)) + n_fill(q)
        cap = -(-total // (end - start))
    for t in range(start, end):
        while q and n_fill(post[t]) < cap:
            post[t].append(q.pop(0))
            while q and isinstance(q[0], str) and q[0].endswith(":"):      # a label sticks to the op before it
                post[t].append(q.pop(0))
    post[end - 1] += q


# ---------------------------------------------------------------- SGPR map (s32-s34 are ABI-reserved: unused)
S_KBASE, S_VBASE, S_QBASE = 36, 38, 40    # 64-bit
S_TB, S_VB, S_EXEC, S_T64, S_T64B = 42, 44, 46, 48, 50   # 64-bit temps
(S_KRS, S_VRS, S_LASTROW, S_NTILES, S_C, S_THR, S_TAILVALID, S_FIRSTLAST, S_TAB, S_DOFLAGS, S_WAVE, S_I, S_DOMASK,
 S_FREE0, S_FREE1, S_FREE2, S_LDS, S_T0, S_T1, S_T2, S_T3, S_NM1, S_QRS, S_QROW0, S_SEQLENQ, S_EXPORT, S_PARAM, S_DOWORD, S_NEGC,
 S_FREE3, S_DMAW, S_FREE4, S_TAU, S_RESC, S_FREE5) = range(52, 87)
S_FREE6, S_TB2, S_VB2, S_BIT = 87, 88, 90, 92     # second set of DMA bases (the loop is unrolled by two); the rotating vote bit
TBS, VBS = [S_TB, S_TB2], [S_VB, S_VB2]

# Parameter words 0-22, in the order the shells write param[i]
PARAM_WORDS = [
    S_KBASE, S_KBASE + 1,       # [0] [1]   K row 0 of this (batch, KV head): byte address
    S_VBASE, S_VBASE + 1,       # [2] [3]   V row 0 (fp8: the prepared V^T tiles)
    S_KRS, S_VRS,               # [4] [5]   K / V row stride in bytes
    S_LASTROW, S_NTILES,        # [6] [7]   seqlen_k - 1; tiles in the walk
    S_C, S_THR,                 # [8] [9]   c = softmax scale * log2 e (fp8: with the Q / K descales); skip threshold
    S_TAILVALID, S_FIRSTLAST,   # [10] [11] valid keys of the last tile; 1 if the walk starts at the last tile
    S_TAB, S_DOFLAGS,           # [12] [13] LDS address of the tile-address table; of the vote words
    S_QBASE, S_QBASE + 1,       # [14] [15] Q row 0 of this (batch, head): byte address
    S_QRS, S_QROW0, S_SEQLENQ,  # [16] [17] [18] Q row stride in bytes; first query row of the item; seqlen_q
    S_EXPORT,                   # [19]      half-vote form: LDS address of half 0's activity words, else 0
    S_LDS, S_NEGC, S_TAU,       # [20] [21] [22] LDS address of the K / V rings; -c; tau / c
]


def read_params(lane, tmp, extra=()):
    """Lane id -> v[lane]; wave index (%0) -> S_WAVE, parameter block address (%1) -> S_PARAM; words 0-22 -> PARAM_WORDS, words 23...
    -> `extra`. v0 .. v23 hold the words afterwards (fp8 reads c / -c from v8 / v21)."""
    emit("; ---- lane id, parameter block -> SGPRs")
    emit(f"v_mbcnt_lo_u32_b32 {v(lane)}, -1, 0")
    emit(f"v_mbcnt_hi_u32_b32 {v(lane)}, -1, {v(lane)}")
    emit(f"s_mov_b32 {s(S_WAVE)}, %0")
    emit(f"s_mov_b32 {s(S_PARAM)}, %1")
    emit(f"v_mov_b32 {v(tmp)}, {s(S_PARAM)}")
    for q in range(6):
        emit(f"ds_read_b128 {vr(4 * q, 4)}, {v(tmp)} offset:{16 * q}")
    emit("s_waitcnt lgkmcnt(0)")
    plist = PARAM_WORDS + list(extra)
    for idx, sg in enumerate(plist):
        emit(f"v_readfirstlane_b32 {s(sg)}, {v(idx)}")
    emit("s_nop 4")


def flush_domask(t0, t1):
    """Vote word |= S_DOMASK by one lane (t0, t1: two free VGPRs); S_DOMASK = 0."""
    emit(f"v_mov_b32 {v(t0)}, {s(S_DOWORD)}")
    emit(f"v_mov_b32 {v(t1)}, {s(S_DOMASK)}")
    emit(f"s_mov_b64 {sr(S_EXEC)}, exec")
    emit("s_mov_b64 exec, 1")
    emit(f"ds_or_b32 {v(t0)}, {v(t1)}")
    emit(f"s_mov_b64 exec, {sr(S_EXEC)}")
    emit(f"s_mov_b32 {s(S_DOMASK)}, 0")
