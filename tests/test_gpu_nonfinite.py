"""GPU: non-finite inputs stay in the results that depend on them - containment on every forward body.

Everywhere else in the suite the data a launch reads is finite (the poison of tests/test_gpu_layout_poison.py sits in rows the kernels
clamp, mask or never list). Here NaN, infinity and the largest finite value sit in rows the launch USES, and the results that do not
depend on them must not change by one bit. What could carry them over rests on `0 x finite = 0` or `exp2(finite - inf) = 0`, neither
of which holds for NaN or Inf: the step the software-pipelined walk runs past its end on whatever the K / V rings in LDS still hold
(gen_blocks.inval_block, read_tile_table, stage_k2), the rings and registers a persistent workgroup keeps from item to item and the early
start of the next item (kOverlap), the LDS a workgroup of the static map inherits, the masked keys and zeroed query rows of ragged tiles,
the wave-wide lazy rescale (rare_rescale_block), the caller's workspace (torch.empty: the e4m3 V tiles and the ticket counters), and the
row-by-row LSE merge (la_aux_kernels.hip: combine_kernel).

Inputs and expectations: tests/nonfinite_cases.py, proved on the CPU by tests/test_nonfinite_cases_cpu.py (the finite / non-finite masks
are those of the plain fp64 softmax on the same inputs). The bodies are the list of tests/test_gpu_score_range.py. There is no tolerance
of this file's own; every assertion is bit-identity with an unpoisoned launch (raw bits), finite / not finite, or the rule the existing
test of the body uses (`_tol` and the 1e-3 LSE bound of tests/test_gpu_head_dims.py at the ulps of tests/test_gpu_layout_poison.py;
test_gpu_fp8._tol with helpers.fp8_lse_tol(); test_gpu_parity._compare_lists), and every family holds its unpoisoned launch to the oracle.

A  A seeded half of the (batch, kv head) pairs has every element of K, of V or of both poisoned, or (separately) half of the (batch,
   head) pairs every element of Q; the twin launch has finite data there. GQA 4 on 2, two q-tiles (the second ragged), key lengths
   1 .. 560 (walks of 1, 1, 2, 3, 4, 5 and 9 tiles with ragged tails), every launch under the ticket queues and under the static map.
   Clean heads: out, lse and write-list rows are the twin's bits. Poisoned heads, NaN only: V alone gives a non-finite out and the twin's
   LSE bits, K or Q a non-finite out and LSE. B x H x 2 items are at least three times the workgroups resident on the device
   (flash_attn_interface.device_slots, read at run time) - asserted. That poisoned-then-clean successions then occur on many persistent
   workgroups is a property of the schedule; it cannot be observed or proved from here.
   One 16-bit and one e4m3 body per head-dim family also run read lists (the ranges of layout_cases, thr = -inf and -3) and a packed
   batch in which poisoned sequences of 560 keys alternate with clean ones of 13, 65 and 130: the long item fills every ring slot, the
   short one rewrites few of them.
B  Inside one item (B 2, H 4, Hk 2, Sq 300, Sk 203): three V elements (B1: only their three columns change, in every row of the two
   query heads on that kv head), three query rows (B2: only those rows; their neighbours within the tolerance - an Inf or huge row may
   trigger the wave-wide lazy rescale - other heads bit-identical), one NaN key row (B3: its kv head's query heads, nothing else); B1
   and B3 again through the host split (num_splits = 3, which resolves to two chunks of two tiles at 203 keys) and `fwd_combine` on one
   NaN LSE or one NaN partial-output element.
C  The workspace on entry does not matter: exactly la_fwd_workspace_bytes() bytes of 0x00 against 0x7F (the e4m3 NaN; a large ticket
   count) through the raw C-ABI give the same bits.

Measured on an MI355X: every body passed every CONTAINMENT assertion as it stood - no clean head, row, column or sequence differed from
its unpoisoned launch by a bit, under the ticket queues and under the static map, and no fill of the workspace showed in a result; no
kernel needed a fix. 191 cases: A 37 dense (per body 7 key lengths x 2 schedules x (twin + 4 targets x 3 kinds; e4m3: 2 kinds) = 182 /
126 launches) + 8 on lists + 8 packed; B 3 x 37 (+ the four listed variants); 12 host splits and 6 merges; C 5 + 4. The unpoisoned
launches against the oracle (largest error of the family over its cases, next to the bound it is held to there):

    family                      max |O - oracle|  bound      max |LSE - oracle|  bound
    x64 bf16 / fp16 (A)         7.8e-3 / 1.0e-3   2.5e-2 / 4.0e-3   1.4e-6       1e-3
    half-vote, 128-row (A)      7.8e-3 / 9.6e-4   2.5e-2 / 4.0e-3   1.4e-6       1e-3
    16-bit, B (clean, B2 rows)  3.8e-3 / 4.8e-4   5.7e-3 .. 9.5e-3 / 1.6e-3 .. 2.1e-3   9.5e-7   1e-3
    16-bit host split           4.9e-3 / 6.8e-4   6.4e-3 / 6.5e-3   9.5e-7       1e-3
    e4m3 reference (A / B)      4.6e-2 / 7.6e-2   2.5e-1 / 2.4e-1   1.1e-4       1e-3
    e4m3 mfma_rowsum            5.7e-2            2.5e-1            2.4e-2       6.2e-2
    e4m3 encoded                4.2e-2            2.5e-1            1.4e-2       1.19e-1
    16x16x32 variant, d128      passes the same cases (tests/test_gpu_m16.py)

Two findings about what a row with a NaN score RETURNS (MEASUREMENTS.md, section 7); neither moves anything into a clean result:

* Every body finalizes a row whose sum is NaN to LSE = -inf with out = acc x 0 = NaN. That is the reference's own rule (softmax.h:285-293:
  `sum == 0 | sum != sum`), restated by the generated epilogue, the 16x16x32 body, the 128-row template and the C oracle, so the
  non-finite LSE the cases ask for is -inf, never NaN. Through the host split the merge (like the reference's, and like
  oracle.attention_combine_ref) gives such a partial the weight 0: the merged out is NaN, the merged LSE is the FINITE LSE of the chunks
  without the NaN key, where the fp64 softmax over all keys says NaN. test_host_split_... pins this as it is (merged LSE against the
  oracle over the keys of the other chunk: 9.5e-7, e4m3 5.2e-6, bound 1e-3). Changing it means leaving the reference's finalize rule in
  all four places and in the pinned checker; it is recorded, not changed.
* The e4m3 bodies with the byte-encoded P (LA_FP8_P=encoded; not the default form) return FINITE results where the fp64 softmax is
  NaN, and the hardware decides it: v_cvt_pk_u8_f32 converts a NaN score to byte 0 (gen_fwd_x64_fp8.py), so the key is not there. A row
  or head whose every score is NaN returns out = 0 and LSE = -inf (K and V both NaN: out NaN, 0 x NaN); one NaN key row returns the
  attention over the other keys (against the oracle on the input without that key: |dO| 8.7e-2 at a bound of 2.4e-1, |dLSE| 5.1e-2 at
  1.19e-1). Asserted as observed for those five bodies (nonfinite_cases.a_expectation(encoded=True), B2, B3); the reference and
  mfma_rowsum forms return NaN / -inf like the 16-bit bodies.
"""
import ctypes

import pytest
import torch

import layout_cases as lc
import nonfinite_cases as nf
import test_gpu_fp8 as f8
import test_gpu_head_dims as hd
import test_gpu_score_range as sr
from helpers import fp8_lse_tol, fp8_p_round
from layout_cases import F8
from test_gpu_layout_poison import EXTRA as _EXTRA_LAYOUT
from test_gpu_parity import _compare_lists
from test_gpu_round2 import _raw_args

pytestmark = pytest.mark.gpu
BF, HF = torch.bfloat16, torch.float16
NEG_INF = float("-inf")
BODIES = sr.BODIES
EXTRA = [sr.BY_ID[b[0]] for b in _EXTRA_LAYOUT]              # one 16-bit and one e4m3 body per head-dim family
SPLIT_BODIES = sr.BODIES_16 + [b for b in EXTRA if b[1] == F8]
_ids = sr._ids


def _setenv(monkeypatch, body, static_env=False):
    sr._setenv(monkeypatch, body)
    monkeypatch.delenv("LA_SCHED", raising=False)
    if static_env:                                             # the packed route has no _static_sched argument: the host default
        monkeypatch.setenv("LA_SCHED", "static")


def _es(body):
    return 1 if body[1] == F8 else 2


def _encoded(body):
    """The e4m3 bodies whose P is a byte code (LA_FP8_P=encoded): a NaN score becomes byte 0 in the hardware conversion."""
    return body[3].get("LA_FP8_P") == "encoded"


def _dev(ds):
    return {n: t.cuda() for n, t in ds.items()}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else lc.raw(t)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _launch(q, k, v, ds, static=False, rd=None, thr=NEG_INF):
    """-> (out, lse, write list or None)"""
    from liteattention_amd.flash_attn_interface import mha_fwd
    kw, wr = {}, None
    if rd is not None:
        wr = torch.full_like(rd, -7)
        kw = dict(attn_read_list=rd, attn_write_list=wr, thr=thr)
    o, lse, *_ = mha_fwd(q, k, v, _static_sched=static, **ds, **kw)
    return o, lse, wr


def _oracle(body, q, k, v, ds, rd=None, thr=NEG_INF):
    """The C oracle in the body's form on CPU tensors -> (o, lse, write list, margins)."""
    import liteattention_amd as L
    from oracle import oracle as orc
    _, dtype, D, _ = body
    bm, bn = L.get_tile_sizes(D, _es(body))
    kw, wr, mg = {}, None, None
    if rd is not None:
        wr, mg = torch.zeros_like(rd), torch.empty(q.shape[0], q.shape[2], rd.shape[2], -(-k.shape[1] // bn))
        kw = dict(read_list=rd, write_list=wr, thr=thr, margins=mg)
    if dtype == F8:
        o, lse, _ = orc.qkskip_fwd(q.float(), k.float(), v.float(), block_m=bm, block_n=bn, p_round=fp8_p_round(), **ds, **kw)
    else:
        o, lse, _ = orc.qkskip_fwd(q, k, v, block_m=bm, block_n=bn, p_round="f16" if dtype == HF else True, **kw)
    return o, lse, wr, mg


def _tols(body, o_ref, listed):
    """The existing rule of the body (tests/test_gpu_layout_poison.py: 0.75 ulp dense, 1.0 on lists; e4m3: test_gpu_fp8._tol)."""
    if body[1] == F8:
        return f8._tol(o_ref), fp8_lse_tol()
    return hd._tol(o_ref, body[1], ulps=1.0 if listed else 0.75), 1e-3


def _within(body, what, out, lse, ref, rd=None, wr=None, thr=NEG_INF, rows=None):
    """`out` (B, Sq, H, D), `lse` (B, H, Sq) (CPU) against ``ref`` = _oracle(...); `rows`: bool (B, Sq, H), the rows that are compared."""
    from oracle import oracle as orc
    o_ref, lse_ref, wr_orc, mg = ref
    tol_o, tol_l = _tols(body, o_ref, rd is not None)
    d_o, d_l = (out.float() - o_ref).abs(), (lse - lse_ref).abs()
    if rows is not None:
        d_o, d_l = d_o[rows], d_l[rows.permute(0, 2, 1)]
    err_o, err_l = d_o.max().item(), d_l.max().item()
    print(f"nonfinite {body[0]} {what}: dO {err_o:.3e} (bound {tol_o:.3e}) dLSE {err_l:.3e} (bound {tol_l:.1e})")
    assert bool(torch.isfinite(d_o).all()) and bool(torch.isfinite(d_l).all()), (body[0], what)
    assert err_o <= tol_o, (body[0], what, err_o, tol_o)
    assert err_l <= tol_l, (body[0], what, err_l, tol_l)
    if rd is not None:
        bad, _ = _compare_lists(orc, rd, wr, wr_orc, mg, thr, rd.shape[0])
        assert bad == 0, (body[0], what, bad)


# ------------------------------------------------------------------------------------------------------------------- family A
_A_DEV, _A_CPU = {}, {}


def _a_geometry(body):
    """(rows of a workgroup item, Sq, batch): two q-tiles per (batch, head), and at least three times as many items as the device holds
    workgroups - the CONDITION of family A, asserted here."""
    from liteattention_amd.flash_attn_interface import device_slots, q_tiles_per_item
    _, dtype, D, _ = body
    rows = sr._tiles(body) * q_tiles_per_item(D, _es(body))
    cus, per = device_slots(D, _es(body))
    Sq = nf.a_seqlen_q(rows)
    q_tiles = -(-Sq // rows)
    B = -(-3 * cus * per // (nf.A_H * q_tiles))
    B += B % 2                                                 # (the packed batch alternates in pairs)
    assert q_tiles == 2 and Sq % rows != 0
    assert B * nf.A_H * q_tiles >= 3 * cus * per, (B, cus, per)
    return rows, Sq, B


def _a_base(body, B):
    """The twin on the device (all of it) and on the CPU (batch entries 0 and 1, for the oracle): ((q, k, v, ds), (q, k, v, ds))."""
    _, dtype, D, _ = body
    if (dtype, D, B) not in _A_DEV:
        for dt, (q, k, v, ds) in nf.a_base(D, B, [BF, HF, F8]).items():
            _A_DEV[(dt, D, B)] = (q.cuda(), k.cuda(), v.cuda(), _dev(ds))
            _A_CPU[(dt, D, B)] = (q[:2].clone(), k[:2].clone(), v[:2].clone(), {n: t[:2].clone() for n, t in ds.items()})
    return _A_DEV[(dtype, D, B)], _A_CPU[(dtype, D, B)]


def _head_diff(a, b):
    """bool (B, H): the heads in which two results differ by a bit. out (B, S, H, D); lse (B, H, S); write list (B, H, Qt, Kt + 1)."""
    d = _bits(a) != _bits(b)
    if a.dtype == torch.float32:
        return d.any(2)
    if a.dtype == torch.int32:
        return d.any(3).any(2)
    return d.any(3).any(1)


def _head_nonfinite(o, lse):
    """bool (B, H) x 2: every element of the head's out / lse is not finite."""
    return (~torch.isfinite(o.float())).all(3).all(1), (~torch.isfinite(lse)).all(2)


def _check_heads(tag, res, twin, heads, exp, lists):
    """One poisoned launch against its twin. heads: bool (B, H) on the device, the heads that depend on the poison."""
    o, lse, wr = res
    d_o, d_l = _head_diff(o, twin[0]), _head_diff(lse, twin[1])
    assert not bool((d_o & ~heads).any()), (tag, "out of a clean head differs from the twin", (d_o & ~heads).nonzero()[:4].tolist())
    assert not bool((d_l & ~heads).any()), (tag, "lse of a clean head differs from the twin", (d_l & ~heads).nonzero()[:4].tolist())
    if lists:
        d_w = _head_diff(wr, twin[2])
        assert not bool((d_w & ~heads).any()), (tag, "write list of a clean head differs from the twin", (d_w & ~heads).nonzero()[:4].tolist())
    assert bool(((d_o | d_l) & heads).any()), (tag, "vacuous: no poisoned head differs from the twin")      # (one key: out is V whatever K is)
    if exp is not None:
        bad_o, bad_l = _head_nonfinite(o, lse)
        if exp.out == "nonfinite":
            assert bool(bad_o[heads].all()), (tag, "out of a poisoned head is finite")
        else:                                                  # the byte-encoded P: every key dropped, the row of an item without keys
            assert bool((o.float() == 0).all(3).all(1)[heads].all()), (tag, "out of a head without a finite score is not 0")
        if exp.lse == "twin":
            assert not bool((d_l & heads).any()), (tag, "lse depends on V")
        elif exp.lse == "nonfinite":
            assert bool(bad_l[heads].all()), (tag, "lse of a poisoned head is finite")
        else:
            assert bool((lse == NEG_INF).all(2)[heads].all()), (tag, "lse of a head without a finite score is not -inf")


@pytest.mark.parametrize("body", BODIES, ids=_ids(BODIES))
def test_poisoned_heads_stay_in_their_items(monkeypatch, body):
    """Family A, dense fixed-length launches: every body, seven key lengths, K / V / K and V / Q, every poison kind of the type, ticket
    queues and static map. The twin of every key length is held to the oracle (batch entry 0)."""
    _setenv(monkeypatch, body)
    rows, Sq, B = _a_geometry(body)
    (q0, k0, v0, ds), (qc, kc, vc, dsc) = _a_base(body, B)
    q = q0[:, :Sq].contiguous()
    heads = {t: nf.a_poisoned_heads(t, B).cuda() for t in nf.A_TARGETS}
    one = {n: t[:1] for n, t in dsc.items()}
    for Sk in nf.A_KEY_LENS:
        k, v = k0[:, :Sk].contiguous(), v0[:, :Sk].contiguous()
        ref = _oracle(body, qc[:1, :Sq], kc[:1, :Sk], vc[:1, :Sk], one)
        for static in (False, True):
            twin = _launch(q, k, v, ds, static)
            _within(body, f"A dense Sk={Sk} static={static}", twin[0][:1].cpu(), twin[1][:1].cpu(), ref)
            for target in nf.A_TARGETS:
                for kind in nf.kinds(body[1]):
                    res = _launch(*nf.a_poison(q, k, v, target, kind), ds, static)
                    _check_heads((body[0], Sk, static, target, kind), res, twin, heads[target], nf.a_expectation(target, kind, _encoded(body)), False)


@pytest.mark.parametrize("static", [False, True], ids=["tickets", "static"])
@pytest.mark.parametrize("body", EXTRA, ids=_ids(EXTRA))
def test_poisoned_heads_stay_in_their_items_on_read_lists(monkeypatch, body, static):
    """Family A on hand-built read lists (600 keys; every q-tile: tiles 9 8 7 6 | 4 3 | 1 0) at thr = -inf and at thr = -3: also the
    write-list rows of the clean heads are the twin's. (Nothing is asked of a poisoned head's write list: a vote on NaN is another matter.)"""
    _setenv(monkeypatch, body)
    rows, Sq, B = _a_geometry(body)
    (q0, k, v, ds), (qc, kc, vc, dsc) = _a_base(body, B)
    q = q0[:, :Sq].contiguous()
    rd = lc.list_rows([lc.LIST_RANGES] * 2, B, nf.A_H)
    rd_d = rd.cuda()
    one = {n: t[:1] for n, t in dsc.items()}
    for thr in (NEG_INF, nf.FINITE_THR):
        twin = _launch(q, k, v, ds, static, rd_d, thr)
        _within(body, f"A lists thr={thr:g} static={static}", twin[0][:1].cpu(), twin[1][:1].cpu(),
                _oracle(body, qc[:1, :Sq], kc[:1], vc[:1], one, rd[:1].contiguous(), thr), rd[:1].contiguous(), twin[2][:1].cpu(), thr)
        for target in nf.A_TARGETS:
            heads = nf.a_poisoned_heads(target, B).cuda()
            for kind in nf.kinds(body[1]):
                res = _launch(*nf.a_poison(q, k, v, target, kind), ds, static, rd_d, thr)
                _check_heads((body[0], "lists", thr, static, target, kind), res, twin, heads, nf.a_expectation(target, kind), True)


@pytest.mark.parametrize("static", [False, True], ids=["tickets", "static"])
@pytest.mark.parametrize("body", EXTRA, ids=_ids(EXTRA))
def test_poisoned_sequences_of_a_packed_batch_stay_in_their_items(monkeypatch, body, static):
    """Family A as a packed batch (cu_seqlens): sequences of 560 keys whose every K / V row is poison alternate with clean ones of 13, 65
    and 130 keys; every sequence has two q-tiles. Clean sequences: the twin's bits. The twin's sequences 0 (560 keys) and 1 (13) are
    held to the oracle."""
    from liteattention_amd.flash_attn_interface import mha_fwd
    _setenv(monkeypatch, body, static_env=static)
    rows, Sq, B = _a_geometry(body)
    (q0, k0, v0, ds), (qc, kc, vc, dsc) = _a_base(body, B)
    lens, flags = nf.packed_lens(B)
    q, k, v = q0[:, :Sq].reshape(B * Sq, nf.A_H, body[2]), nf.pack(k0, lens), nf.pack(v0, lens)
    cu_q, cu_k = nf.cu([Sq] * B).cuda(), nf.cu(lens).cuda()
    k_rows = nf.packed_row_mask(lens, flags).cuda()
    q_rows = nf.packed_row_mask([Sq] * B, flags).cuda()

    def launch(k_, v_):
        o, lse, *_ = mha_fwd(q, k_, v_, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, max_seqlen_q=Sq, max_seqlen_k=nf.P_LONG, **ds)
        return o, lse                                          # (T, H, D), (H, T)

    twin = launch(k, v)
    for b in (0, 1):
        one = {n: t[b:b + 1] for n, t in dsc.items()}
        _within(body, f"A packed seq {b} static={static}", twin[0][b * Sq:(b + 1) * Sq][None].cpu(), twin[1][:, b * Sq:(b + 1) * Sq][None].cpu(),
                _oracle(body, qc[b:b + 1, :Sq], kc[b:b + 1, :lens[b]], vc[b:b + 1, :lens[b]], one))
    for target in ("k", "v", "kv"):
        for kind in nf.kinds(body[1]):
            o, lse = launch(nf.poison_packed_rows(k, k_rows, kind) if "k" in target else k,
                            nf.poison_packed_rows(v, k_rows, kind) if "v" in target else v)
            tag = (body[0], "packed", static, target, kind)
            assert _same(o[~q_rows], twin[0][~q_rows]), (tag, "out of a clean sequence differs from the twin")
            assert _same(lse[:, ~q_rows], twin[1][:, ~q_rows]), (tag, "lse of a clean sequence differs from the twin")
            assert not _same(o[q_rows], twin[0][q_rows]), (tag, "vacuous")
            exp = nf.a_expectation(target, kind)
            if exp is not None:
                assert not bool(torch.isfinite(o[q_rows].float()).any()), (tag, "out of a poisoned sequence is finite")
                if exp.lse == "twin":
                    assert _same(lse[:, q_rows], twin[1][:, q_rows]), (tag, "lse depends on V")
                else:
                    assert not bool(torch.isfinite(lse[:, q_rows]).any()), (tag, "lse of a poisoned sequence is finite")


# ------------------------------------------------------------------------------------------------------------------- family B
_B_CLEAN = {}


def _b_variants(body):
    return (False, True) if body in EXTRA else (False,)


def _b_clean(body, listed):
    """The clean launch of family B (dense, or on read lists at thr = -inf), held to the oracle once:
    (CPU inputs, device inputs, read list (CPU, device) or None, listed keys or None, (out, lse, write list), oracle result)."""
    key = (body[0], listed)
    if key not in _B_CLEAN:
        import liteattention_amd as L
        _, dtype, D, _ = body
        q, k, v, ds = nf.b_inputs(dtype, D)
        rd = keys = None
        if listed:
            bm, _ = L.get_tile_sizes(D, _es(body))
            rd = lc.list_rows([nf.B_LIST_RANGES] * -(-nf.B_SQ // bm), nf.B_B, nf.B_H, k_tiles=nf.walk_len(nf.B_SK))
            keys = nf.b_listed_keys()
        dev = (q.cuda(), k.cuda(), v.cuda(), _dev(ds))
        rd_d = None if rd is None else rd.cuda()
        res = _launch(*dev, False, rd_d)
        ref = _oracle(body, q, k, v, ds, rd)
        _within(body, f"B clean listed={listed}", res[0].cpu(), res[1].cpu(), ref, rd, None if rd is None else res[2].cpu())
        _B_CLEAN[key] = ((q, k, v, ds), dev, (rd, rd_d), keys, res, ref)
    return _B_CLEAN[key]


@pytest.mark.parametrize("body", BODIES, ids=_ids(BODIES))
def test_v_elements_reach_their_columns_only(monkeypatch, body):
    """B1: (key Sk - 1, column 0), (key 69, column D - 1), (key 0, column D / 2) of one kv head poisoned in one launch. Every other column
    of out and all of lse: the clean launch's bits, for every head; the three columns non-finite (NaN, inf) in every row of the query
    heads on that kv head; the write list at thr = -inf the clean launch's."""
    _setenv(monkeypatch, body)
    D = body[2]
    cols = torch.tensor([c for _, c in nf.b1_positions(D)])
    other = torch.ones(D, dtype=torch.bool).index_fill(0, cols, False).cuda()
    for listed in _b_variants(body):
        (q, k, v, ds), (qd, kd, vd, dsd), (rd, rd_d), keys, clean, _ = _b_clean(body, listed)
        for kind in nf.kinds(body[1]):
            tag = (body[0], "B1", listed, kind)
            vp = nf.b1_poison_v(v, kind)
            o, lse, wr = _launch(qd, kd, vp.cuda(), dsd, False, rd_d)
            assert _same(o[..., other], clean[0][..., other]), (tag, "a column without poison differs from the clean launch")
            assert _same(lse, clean[1]), (tag, "lse depends on V")
            assert wr is None or torch.equal(wr, clean[2]), tag
            bad_o, _ = nf.nonfinite_masks(q, k, vp, ds, keys=keys)
            assert bool(bad_o.any()) == (kind != "huge")
            assert not bool(torch.isfinite(o.float().cpu())[bad_o].any()), (tag, "a poisoned column is finite")
            assert not _same(o, clean[0]), (tag, "vacuous")


@pytest.mark.parametrize("body", BODIES, ids=_ids(BODIES))
def test_query_rows_stay_in_their_rows(monkeypatch, body):
    """B2: rows 0, 129 and Sq - 1 of one head poisoned, one launch per kind. NaN: those rows of out and lse are non-finite. Every other
    row of the head is finite and within the body's tolerance of the oracle on the CLEAN input (not bit-identical: an Inf or huge row may
    trigger the lazy rescale for the rows of its wave); every other head: the clean launch's bits; the write list the clean launch's."""
    _setenv(monkeypatch, body)
    head = torch.ones(nf.B_B, nf.B_H, dtype=torch.bool)
    head[nf.B_BATCH, nf.B_Q_HEAD] = False
    head = head.cuda()
    for listed in _b_variants(body):
        (q, k, v, ds), (qd, kd, vd, dsd), (rd, rd_d), keys, clean, ref = _b_clean(body, listed)
        for kind in nf.kinds(body[1]):
            tag = (body[0], "B2", listed, kind)
            qp = nf.b2_poison_q(q, kind)
            o, lse, wr = _launch(qp.cuda(), kd, vd, dsd, False, rd_d)
            assert not bool((_head_diff(o, clean[0]) & head).any()) and not bool((_head_diff(lse, clean[1]) & head).any()), (tag, "another head differs")
            assert wr is None or torch.equal(wr, clean[2]), tag
            rows = torch.ones(nf.B_B, nf.B_SQ, nf.B_H, dtype=torch.bool)
            rows[nf.B_BATCH, list(nf.B2_ROWS), nf.B_Q_HEAD] = False
            oc, lsec = o.cpu(), lse.cpu()
            _within(body, f"B2 listed={listed} {kind}", oc, lsec, ref, rows=rows)            # finite, and the oracle's on the clean input
            bad_o, bad_l = nf.nonfinite_masks(qp, k, v, ds, keys=keys)
            if kind == "nan":
                assert int(bad_l.sum()) == len(nf.B2_ROWS) and torch.equal(bad_l.permute(0, 2, 1), ~rows)
                if _encoded(body):                             # every score of the row NaN -> every byte 0: the row of an item without keys
                    assert bool((oc.float()[bad_o] == 0).all()) and bool((lsec[bad_l] == NEG_INF).all()), (tag, "a row without a finite score")
                else:
                    assert not bool(torch.isfinite(oc.float())[bad_o].any()), (tag, "out of a NaN row is finite")
                    assert not bool(torch.isfinite(lsec)[bad_l].any()), (tag, "lse of a NaN row is finite")


@pytest.mark.parametrize("body", BODIES, ids=_ids(BODIES))
def test_a_nan_key_row_reaches_its_kv_head_only(monkeypatch, body):
    """B3: one NaN key row (key 69 of one kv head): every row of the two query heads on that kv head is non-finite in out and lse; the
    other kv head's query heads, and the other batch entry: the clean launch's bits."""
    _setenv(monkeypatch, body)
    on_kv = nf.b_heads_on_kv().cuda()
    for listed in _b_variants(body):
        (q, k, v, ds), (qd, kd, vd, dsd), (rd, rd_d), keys, clean, _ = _b_clean(body, listed)
        tag = (body[0], "B3", listed)
        kp = nf.b3_poison_k(k)
        o, lse, wr = _launch(qd, kp.cuda(), vd, dsd, False, rd_d)
        assert not bool((_head_diff(o, clean[0]) & ~on_kv).any()) and not bool((_head_diff(lse, clean[1]) & ~on_kv).any()), (tag, "another head differs")
        bad_o, bad_l = nf.nonfinite_masks(q, kp, v, ds, keys=keys)
        assert torch.equal(bad_l.any(2), on_kv.cpu()) and torch.equal(bad_l.all(2), on_kv.cpu())
        if _encoded(body):
            # the hardware decides (MEASUREMENTS.md 7): the NaN score becomes byte 0, the key is not there - those heads are the attention
            # over the OTHER keys, under the body's tolerance against the oracle on the input without that key
            keep = torch.ones(nf.B_SK, dtype=torch.bool)
            keep[nf.B3_KEY] = False
            _within(body, "B3 without the key", o.cpu(), lse.cpu(), _oracle(body, q, k[:, keep].contiguous(), v[:, keep].contiguous(), ds),
                    rows=on_kv.cpu()[:, None, :].expand(nf.B_B, nf.B_SQ, nf.B_H))
            continue
        assert not bool(torch.isfinite(o.float().cpu())[bad_o].any()), (tag, "out of a row with a NaN score is finite")
        assert not bool(torch.isfinite(lse.cpu())[bad_l].any()), (tag, "lse of a row with a NaN score is finite")


# --------------------------------------------------------------------------------------------------------------- B4: the merge
def _split_tols(body, o_ref):
    """tests/test_gpu_joint_recipe.py test_split_kv_of_dense_launches_with_few_items (16-bit); e4m3: the rule of the body."""
    if body[1] == F8:
        return f8._tol(o_ref), fp8_lse_tol()
    return (2.0 ** -8 + 2.0 ** -9) * o_ref.abs().max().item() + 1e-3, 1e-3


@pytest.mark.parametrize("body", SPLIT_BODIES, ids=_ids(SPLIT_BODIES))
def test_host_split_shows_the_pattern_of_the_unsplit_launch(monkeypatch, body):
    """The B1 and B3 inputs through flash_attn_func(num_splits=3): partial launches over the key chunks and la_combine. The heads the
    poison should not touch are the clean split launch's bits and within the split path's tolerance of the oracle; the others show the
    pattern of the unsplit launch (B1: three non-finite columns, every other column and the LSE the clean split launch's bits)."""
    import liteattention_amd as L
    from liteattention_amd.flash_attn_interface import _num_splits
    _setenv(monkeypatch, body)
    D = body[2]
    q, k, v, ds = nf.b_inputs(body[1], D)
    qd, kd, vd, dsd = q.cuda(), k.cuda(), v.cuda(), _dev(ds)
    assert _num_splits(nf.B_B, nf.B_H, nf.B_SQ, nf.B_SK, D, _es(body), 3) > 1
    o_ref, lse_ref, _, _ = _oracle(body, q, k, v, ds)
    tol_o, tol_l = _split_tols(body, o_ref)
    on_kv = nf.b_heads_on_kv()

    def run(k_, v_, what):
        o, lse = L.flash_attn_func(qd, k_.cuda(), v_.cuda(), num_splits=3, return_softmax_lse=True, **dsd)
        oc, lsec = o.cpu(), lse.cpu()
        d_o = (oc.float() - o_ref).abs().permute(0, 2, 1, 3)[~on_kv]
        d_l = (lsec - lse_ref).abs()[~on_kv]
        print(f"nonfinite {body[0]} split {what}: dO {d_o.max().item():.3e} (bound {tol_o:.3e}) dLSE {d_l.max().item():.3e} (bound {tol_l:.1e})")
        assert d_o.max().item() <= tol_o and d_l.max().item() <= tol_l, (body[0], what)       # (NaN fails the comparison)
        return o, lse, oc, lsec

    clean = run(k, v, "clean")
    assert (clean[2].float() - o_ref).abs().max().item() <= tol_o and (clean[3] - lse_ref).abs().max().item() <= tol_l
    cols = torch.tensor([c for _, c in nf.b1_positions(D)])
    other = torch.ones(D, dtype=torch.bool).index_fill(0, cols, False).cuda()
    for kind in nf.kinds(body[1]):
        vp = nf.b1_poison_v(v, kind)
        o, lse, oc, _ = run(k, vp, f"B1 {kind}")
        assert _same(o[..., other], clean[0][..., other]) and _same(lse, clean[1]), (body[0], "B1", kind)
        bad_o, _ = nf.nonfinite_masks(q, k, vp, ds)
        assert not bool(torch.isfinite(oc.float())[bad_o].any()), (body[0], "B1", kind, "a poisoned column is finite")
    kp = nf.b3_poison_k(k)
    o, lse, oc, lsec = run(kp, v, "B3")
    assert not bool((_head_diff(o, clean[0]) & ~on_kv.cuda()).any()) and not bool((_head_diff(lse, clean[1]) & ~on_kv.cuda()).any())
    bad_o, bad_l = nf.nonfinite_masks(q, kp, v, ds)
    assert not bool(torch.isfinite(oc.float())[bad_o].any()), (body[0], "B3", "out of a row with a NaN score is finite")
    # The merged LSE of those rows is FINITE where the fp64 softmax over all keys is NaN, and by the reference's own arithmetic: a row sum
    # that is NaN finalizes to LSE = -inf (softmax.h:285-293, restated by every body, the 128-row template and the C oracle), and the merge
    # gives a partial with LSE = -inf the weight 0 (flash_fwd_combine_kernel.h; oracle.attention_combine_ref) - out stays NaN (0 x NaN),
    # the LSE is that of the chunk without the NaN key. Pinned as it is: the LSE over the keys of the other chunk, under the LSE bound.
    chunk = -(-nf.walk_len(nf.B_SK) // 3) * nf.BN
    assert -(-nf.B_SK // chunk) == 2 and nf.B3_KEY < chunk
    _, lse_rest, _, _ = _oracle(body, q, k[:, chunk:].contiguous(), v[:, chunk:].contiguous(), ds)
    d_l = (lsec - lse_rest).abs()[on_kv]
    print(f"nonfinite {body[0]} split B3: merged LSE against the LSE of keys {chunk}..: {d_l.max().item():.3e} (bound {tol_l:.1e})")
    assert d_l.max().item() <= tol_l, (body[0], "B3", "merged lse")


@pytest.mark.parametrize("which", ["lse", "out"])
@pytest.mark.parametrize("dtype", [torch.float32, BF, HF], ids=["fp32", "bf16", "fp16"])
def test_fwd_combine_keeps_one_nan_in_its_row(dtype, which):
    """torch.ops.lite_attention.fwd_combine on three partials with one NaN LSE, or one NaN partial-output element, in one split of one
    row: every other row is the merge of the clean partials, bit for bit; the row is non-finite where oracle.attention_combine_ref is.
    The clean merge is held to that reference under the rule of tests/test_gpu_round4.py."""
    import liteattention_amd  # noqa: F401  (registers the op)
    from oracle import oracle as orc
    o, lse = nf.combine_partials(dtype)
    od, lsed = o.cuda(), lse.cuda()
    assert lsed.stride(-2) == 1
    out, lse_m = torch.ops.lite_attention.fwd_combine(od, lsed, None, dtype)
    ref, lse_ref = orc.attention_combine_ref(o.float(), lse)
    out_pt = ref.to(dtype)
    assert torch.allclose(lse_m.cpu(), lse_ref, atol=1e-5, rtol=1e-5)
    assert ((out.cpu().float() - ref).abs().max().item() <= 2 * (out_pt.float() - ref).abs().max().item()) or torch.allclose(out.cpu(), out_pt, atol=1e-5, rtol=1e-5)
    op, lsep, (b, s, h) = nf.combine_poison(o, lse, which)
    outp, lse_mp = torch.ops.lite_attention.fwd_combine(op.cuda(), lsep.cuda(), None, dtype)
    refp, lse_refp = orc.attention_combine_ref(op.float(), lsep)
    row = torch.zeros(nf.C_B, nf.C_S, nf.C_H, dtype=torch.bool)
    row[b, s, h] = True
    assert _same(outp.cpu()[~row], out.cpu()[~row]) and _same(lse_mp.cpu()[~row], lse_m.cpu()[~row])
    bad_o, bad_l = ~torch.isfinite(refp), ~torch.isfinite(lse_refp)
    assert bool(bad_o.any()) == (which == "out") and bool(bad_l.any()) == (which == "lse")
    assert not bool(torch.isfinite(outp.cpu().float())[bad_o].any()) and not bool(torch.isfinite(lse_mp.cpu())[bad_l].any())


# ------------------------------------------------------------------------------------------------------------------- family C
C_BODIES = [(sr.BY_ID["e4m3-d64"], False), (sr.BY_ID["e4m3-d64"], True), (sr.BY_ID["e4m3-d192"], False), (sr.BY_ID["e4m3-d192"], True),
            (sr.BY_ID["bf16-d128"], True)]
C_IDS = [f"{b[0]}-{'lists' if l else 'dense'}" for b, l in C_BODIES]
C_LENS_Q, C_LENS_K = [300, 130, 172], [203, 13, 130]          # packed: the 13-key sequence leaves three tiles of its Kt_max row unwritten


def _c_run(body, q, k, v, fill, static, rd=None, cu=None):
    """One la_fwd through the raw C-ABI on a workspace of exactly la_fwd_workspace_bytes() bytes of `fill` -> (out, lse, write list)."""
    from liteattention_amd import _cabi
    lib = _cabi.load()
    _, dtype, D, _ = body
    packed = cu is not None
    H = q.shape[-2]
    out = torch.empty(q.shape, dtype=BF if dtype == F8 else dtype, device="cuda")
    lse = torch.empty((H, q.shape[0]) if packed else (q.shape[0], H, q.shape[1]), device="cuda")
    a = _raw_args(*((t[None] for t in (q, k, v, out)) if packed else (q, k, v, out)), lse)
    a.dtype = {BF: _cabi.LA_DTYPE_BF16, HF: _cabi.LA_DTYPE_FP16, F8: _cabi.LA_DTYPE_FP8_E4M3}[dtype]
    a.flags = _cabi.LA_FLAG_STATIC_SCHED if static else 0
    a.block_m, a.block_n = _cabi.get_tile_sizes(D, _es(body), 0)
    if packed:
        a.batch, a.seqlen_q, a.seqlen_k, a.total_q = len(C_LENS_Q), max(C_LENS_Q), max(C_LENS_K), q.shape[0]
        a.q_batch_stride = a.k_batch_stride = a.v_batch_stride = a.o_batch_stride = 0
        a.cu_seqlens_q, a.cu_seqlens_k = cu[0].data_ptr(), cu[1].data_ptr()
    wr = None
    if rd is not None:
        wr = torch.full_like(rd, -7)
        a.read_list, a.write_list, a.thr = rd.data_ptr(), wr.data_ptr(), NEG_INF
    need = int(lib.la_fwd_workspace_bytes(ctypes.byref(a)))
    assert need > 0 or (need == 0 and static and dtype != F8), need        # (16-bit under the static map: no counters, no workspace)
    if need:
        ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
    rc = lib.la_fwd(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _cabi.LA_OK, _cabi.status_string(rc)
    torch.cuda.synchronize()
    return out, lse, wr


def _c_compare(body, runs):
    first = runs[0]
    assert bool(torch.isfinite(first[0].float()).all()) and bool(torch.isfinite(first[1]).all())
    for i, r in enumerate(runs[1:]):
        assert _same(r[0], first[0]) and _same(r[1], first[1]), (body[0], i + 1, "the result depends on the workspace's contents on entry")
        assert (r[2] is None) == (first[2] is None) and (r[2] is None or torch.equal(r[2], first[2])), (body[0], i + 1)


@pytest.mark.parametrize("body,listed", C_BODIES, ids=C_IDS)
def test_workspace_contents_on_entry_do_not_matter(monkeypatch, body, listed):
    """Family C, fixed-length: 0x00 against 0x7F in every byte of the workspace (e4m3: the V tiles start as NaN; all: the ticket counters
    start at 0x7F7F7F7F), ticket queues and static map: out, lse and the write list are the same bits, and finite."""
    for name in sr.ENV_NAMES + ("LA_SCHED",):
        monkeypatch.delenv(name, raising=False)
    import liteattention_amd as L
    q, k, v, _ = nf.b_inputs(body[1], body[2])
    rd = None
    if listed:
        bm, _ = L.get_tile_sizes(body[2], _es(body))
        rd = lc.list_rows([nf.B_LIST_RANGES] * -(-nf.B_SQ // bm), nf.B_B, nf.B_H, k_tiles=nf.walk_len(nf.B_SK))
    qd, kd, vd, rd_d = q.cuda(), k.cuda(), v.cuda(), None if rd is None else rd.cuda()
    runs = [_c_run(body, qd, kd, vd, fill, static, rd_d) for static in (False, True) for fill in (0x00, 0x7F)]
    _c_compare(body, runs)
    _within(body, f"C listed={listed}", runs[0][0].cpu(), runs[0][1].cpu(), _oracle(body, q, k, v, {}, rd), rd, None if rd is None else runs[0][2].cpu())


@pytest.mark.parametrize("body,listed", C_BODIES[:4], ids=C_IDS[:4])
def test_workspace_contents_on_entry_do_not_matter_packed(monkeypatch, body, listed):
    """Family C, packed batch with key lengths 203, 13 and 130: the prepare pass writes each sequence's own tiles onto the [B, Hk, Kt_max]
    grid, so most of the short sequences' rows keep the fill. Sequence 0 is held to the oracle."""
    for name in sr.ENV_NAMES + ("LA_SCHED",):
        monkeypatch.delenv(name, raising=False)
    import liteattention_amd as L
    _, dtype, D, _ = body
    g = torch.Generator().manual_seed(D + 3)
    q = torch.randn(sum(C_LENS_Q), nf.B_H, D, generator=g).to(dtype)
    k, v = [torch.randn(sum(C_LENS_K), nf.B_HK, D, generator=g).to(dtype) for _ in range(2)]
    bm, bn = L.get_tile_sizes(D, _es(body))
    rd = None
    if listed:                                                  # every sequence: one range over its own tiles
        rd = torch.zeros(len(C_LENS_Q), nf.B_H, -(-max(C_LENS_Q) // bm), nf.walk_len(max(C_LENS_K)) + 1, dtype=torch.int32)
        for b, n in enumerate(C_LENS_K):
            rd[b, :, :, 0], rd[b, :, :, 1] = 2, nf.walk_len(n) - 1
    cu = (nf.cu(C_LENS_Q).cuda(), nf.cu(C_LENS_K).cuda())
    qd, kd, vd, rd_d = q.cuda(), k.cuda(), v.cuda(), None if rd is None else rd.cuda()
    runs = [_c_run(body, qd, kd, vd, fill, static, rd_d, cu) for static in (False, True) for fill in (0x00, 0x7F)]
    _c_compare(body, runs)
    n_q, n_k = C_LENS_Q[0], C_LENS_K[0]
    rd0 = None if rd is None else rd[:1].contiguous()
    _within(body, f"C packed listed={listed}", runs[0][0][:n_q][None].cpu(), runs[0][1][:, :n_q][None].cpu(),
            _oracle(body, q[:n_q][None], k[:n_k][None], v[:n_k][None], {}, rd0), rd0, None if rd is None else runs[0][2][:1].cpu())
