"""GPU: score staircases - the lazy O-rescale path of every forward body at the product's own tau.

Every hand-scheduled body keeps O and the row sums relative to a reference maximum that follows the running maximum only after growth by
more than tau log2 units (8 for bf16 / fp16, 2 for the e4m3 reference / mfma_rowsum forms, 32 for the encoded form). The code behind that
trigger is out of line and rare: gen_blocks.rare_rescale_block / rescale_o_block (the AGPR -> VGPR -> AGPR round trip under S_RESC), the
rescale of the matrix-pipe row sums, the transposed running state of gen_fwd_x64_m16.py, and the empty-start half of a half-vote
workgroup, which enters through that block from m_ref = -inf. randn inputs and helpers.fragmented_qkv never grow a row maximum by tau
after the first walked tile, so nothing else in the suite runs it below LA_FLAG_EXACT_RESCALE.

Inputs: tests/score_range_cases.py (Sq 300, Sk 792, H 2; per-head descales for e4m3). tests/test_score_range_cases_cpu.py proves on the
CPU, per (dtype, tau) and head dim, that the staircases deliver the events a - g listed there - every schedule delivers all of them for
its tau (s8: tau 8, and c d e f g at tau 0; s2: tau 2; s32: tau 32) - and that a body with a wrong rescale would miss the bounds below
ten times over. Per body (ten 16-bit x64 bodies, their six half-vote forms, the six 128-row template cases, fifteen e4m3 bodies):

* a dense launch;
* a list launch at thr = -inf on read lists with gaps (head 0: 12-10 8 6-3 1-0, a trigger on the first tile after a gap and at the last
  position; head 1: 12-11 8 5-3 1, a walk that ends with a lag; q-tile 1 of either head starts one position late: under LA_VOTE=half
  that is the second half of workgroup 0, which starts from the empty state on a tile that is a trigger step of the first half);
* the same lists at a finite thr (0.4 tau: the descending q-tile drops what it may, the rising ones keep their growing tiles);
* bf16 / fp16 x64 bodies: the three again under LA_FLAG_EXACT_RESCALE, whose write lists must equal the lazy launch's.

Compared with ``oracle.qkskip_fwd`` in the body's own form under the EXISTING rules - no tolerance of this file's own:
test_gpu_head_dims._tol(o_ref, dtype, ulps=1.0) lazily (the peaked-row bound of test_gpu_fragmented.py), ulps=0.5 under
LA_FLAG_EXACT_RESCALE, LSE 1e-3; e4m3: test_gpu_fp8._tol and helpers.fp8_lse_tol(); write lists through test_gpu_parity._compare_lists
with no bad and no borderline row (every oracle margin is 0.05 or more from thr: CPU test).

softmax_scale = 0 and 1e-30 (test_uniform_attention_*): every score is 0, so O = mean of V over the walked keys and LSE = ln of their
number, in closed form - one 16-bit and one e4m3 body per head-dim family dense and listed, and both half-vote dims with the
empty-start half.

Measured on an MI355X (largest error of the family over head dims and the three launches, next to the bound it is held to there; every body passed
as it stood - no body needed a fix for the staircases):

    family (cases)              max |O - oracle|  bound      max |LSE - oracle|  bound
    x64 bf16 (15)               1.91e-3           5.02e-3    3.1e-5              1e-3
    x64 fp16 (15)               2.42e-4           1.53e-3    3.1e-5              1e-3
    x64 bf16, exact (15)        1.91e-3           3.01e-3    3.1e-5              1e-3
    x64 fp16, exact (15)        2.42e-4           1.26e-3    3.1e-5              1e-3
    half-vote bf16 / fp16 (9+9) 1.91e-3 / 2.42e-4 5.02e-3 / 1.53e-3  3.1e-5      1e-3
    128-row template (9+9)      1.91e-3 / 2.36e-4 5.02e-3 / 1.50e-3  3.1e-5      1e-3
    e4m3 reference (15)         1.12e-2           3.80e-2    1.5e-5              1e-3
    e4m3 mfma_rowsum (15)       1.12e-2           3.80e-2    2.6e-2              6.2e-2
    e4m3 encoded (15)           4.7e-3            4.62e-2    1.8e-3              1.19e-1
    16x16x32 variant, d128      passes the same cases (tests/test_gpu_m16.py)
    scale 0 / 1e-30 (24)        4.7e-4            1.4e-3 ..  8.7e-7              1e-3

The oracle against the plain fp64 softmax on these inputs (CPU, worst head dim): bf16 |dO| 1.1e-3 at max|O| 0.69, |dLSE| 2.8e-5 at |LSE| up
to 153; fp16 1.8e-4, 2.7e-5; "fp8" 1.35e-2, 1.7e-5 (|LSE| up to 132); "fp8_lin" 2.2e-2, 5.2e-2 against the exact values (|LSE| up to 252).

softmax_scale = 0 did need a fix: the dense launch of every body tried returned NaN (c = 0 makes NaN of -inf * 0 for a masked key of the
ragged last tile - and, by reading, for the empty-start half's m_ref = -inf - and inf of tau / c). la_fwd now runs a zero scale at
c = 2^-100, where every exp2 is exactly 1 (la_api.hip), and the oracle masks by value (qkskip_oracle.c).
"""
import pytest
import torch

import score_range_cases as sc
import test_gpu_fp8 as f8
import test_gpu_head_dims as hd
from helpers import fp8_lse_tol, fp8_p_round
from score_range_cases import F8
from test_gpu_parity import _compare_lists

pytestmark = pytest.mark.gpu
BF, HF = torch.bfloat16, torch.float16
NEG_INF = float("-inf")
ENV_NAMES = ("LA_FWD_KERNEL", "LA_FP8_P", "LA_VOTE", "LA_RESCALE_TAU")

# (id, dtype, head_dim, environment)
BODIES_16 = [(f"{n}-d{D}", dt, D, {}) for D in (64, 96, 128, 192, 256) for n, dt in (("bf16", BF), ("fp16", HF))]
BODIES_HALF = [(f"half-{n}-d{D}", dt, D, {"LA_VOTE": "half"}) for D in (64, 96, 128) for n, dt in (("bf16", BF), ("fp16", HF))]
BODIES_V2 = [(f"v2-{n}-d{D}", dt, D, {"LA_FWD_KERNEL": "v2"}) for D in (64, 128, 256) for n, dt in (("bf16", BF), ("fp16", HF))]
BODIES_F8 = [(f"e4m3-d{D}" + (f"-{form}" if form else ""), F8, D, {"LA_FP8_P": form} if form else {})
             for D in (64, 96, 128, 192, 256) for form in ("", "mfma_rowsum", "encoded")]
BODIES = BODIES_16 + BODIES_HALF + BODIES_V2 + BODIES_F8
BY_ID = {b[0]: b for b in BODIES}


def _ids(bodies):
    return [b[0] for b in bodies]


def _setenv(monkeypatch, body):
    for name in ENV_NAMES:
        monkeypatch.delenv(name, raising=False)
    for name, val in body[3].items():
        monkeypatch.setenv(name, val)


def _schedule(body):
    return "s8" if body[1] != F8 else ("s32" if body[3].get("LA_FP8_P") == "encoded" else "s2")


def _tiles(body):
    import liteattention_amd as L
    bm, bn = L.get_tile_sizes(body[2], 1 if body[1] == F8 else 2)
    assert bn == sc.BN
    if body[3]:
        assert bm == (128 if (body[1] != F8 or body[2] > 128) else 256), (body[0], bm)       # the environment selected the body it names
    return bm


_DEV, _REF, _LAZY_LISTS = {}, {}, {}


def _device_inputs(dtype, D, schedule):
    key = (dtype, D, schedule)
    if key not in _DEV:
        q, k, v, ds = sc.staircase_qkv(dtype, D, schedule)
        _DEV[key] = ((q, k, v, ds), (q.cuda(), k.cuda(), v.cuda(), {n: t.cuda() for n, t in ds.items()}))
    return _DEV[key]


def _oracle(body, bm, thr):
    """The C oracle in the body's form: dense if thr is None, else on the read lists at `thr` -> (o, lse, read list, write list, margins).
    Computed once per (inputs, form, q-tile, thr) and shared by the lazy and the exact launch of every body with these."""
    from oracle import oracle as orc
    _, dtype, D, _ = body
    p_round = fp8_p_round() if dtype == F8 else ("f16" if dtype == HF else True)
    key = (dtype, D, _schedule(body), p_round, bm, thr)
    if key not in _REF:
        (q, k, v, ds), _ = _device_inputs(dtype, D, _schedule(body))
        qf, kf, vf = (q.float(), k.float(), v.float()) if dtype == F8 else (q, k, v)
        if thr is None:
            o, lse, _ = orc.qkskip_fwd(qf, kf, vf, block_m=bm, block_n=sc.BN, p_round=p_round, **ds)
            _REF[key] = (o, lse, None, None, None)
        else:
            rd = sc.read_lists(bm)
            wr, mg = torch.zeros_like(rd), torch.empty(1, sc.H, rd.shape[2], sc.KT)
            o, lse, _ = orc.qkskip_fwd(qf, kf, vf, block_m=bm, block_n=sc.BN, p_round=p_round, read_list=rd, write_list=wr, thr=thr, margins=mg, **ds)
            _REF[key] = (o, lse, rd, wr, mg)
    return _REF[key]


def _launch_and_check(body, thr, exact=False):
    """One launch (dense if thr is None) against the oracle; prints the errors next to their bounds; returns the write list (CPU)."""
    from liteattention_amd import _cabi
    from liteattention_amd.flash_attn_interface import mha_fwd
    from oracle import oracle as orc
    name, dtype, D, _ = body
    bm = _tiles(body)
    o_ref, lse_ref, rd, wr_orc, mg = _oracle(body, bm, thr)
    _, (qd, kd, vd, dsd) = _device_inputs(dtype, D, _schedule(body))
    kw = dict(_flags=_cabi.LA_FLAG_EXACT_RESCALE) if exact else {}
    wr = None
    if thr is not None:
        wr = torch.full_like(rd, -7).cuda()
        kw.update(attn_read_list=rd.cuda(), attn_write_list=wr, thr=thr)
    out, lse, *_ = mha_fwd(qd, kd, vd, **dsd, **kw)
    torch.cuda.synchronize()
    out, lse = out.float().cpu(), lse.cpu()
    err_o, err_l = (out - o_ref).abs().max().item(), (lse - lse_ref).abs().max().item()
    if dtype == F8:
        tol_o, tol_l = f8._tol(o_ref), fp8_lse_tol()
    else:
        tol_o, tol_l = hd._tol(o_ref, dtype, ulps=0.5 if exact else 1.0), 1e-3
    print(f"score_range {name}{' exact' if exact else ''} {'dense' if thr is None else f'thr={thr:g}'}: "
          f"dO {err_o:.3e} (bound {tol_o:.3e}) dLSE {err_l:.3e} (bound {tol_l:.1e})")
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all()), name
    assert err_o <= tol_o, (name, err_o, tol_o)
    assert err_l <= tol_l, (name, err_l, tol_l)
    if thr is None:
        return None
    wr = wr.cpu()
    bad, border = _compare_lists(orc, rd, wr, wr_orc, mg, thr, 1)
    assert bad == 0 and border == 0, (name, bad, border)
    return wr


def _thrs(body):
    return (None, NEG_INF, sc.finite_thr(_schedule(body)))


@pytest.mark.parametrize("body", BODIES, ids=_ids(BODIES))
def test_staircase_matches_oracle(monkeypatch, body):
    """Dense, listed at thr = -inf and listed at the finite thr, lazily rescaled (the product's tau)."""
    _setenv(monkeypatch, body)
    for thr in _thrs(body):
        wr = _launch_and_check(body, thr)
        if thr == NEG_INF:                                   # nothing is dropped: the write list is the read list
            rd = sc.read_lists(_tiles(body))
            for h in range(sc.H):
                for m in range(rd.shape[2]):
                    n = int(rd[0, h, m, 0])
                    assert torch.equal(wr[0, h, m, :n + 1], rd[0, h, m, :n + 1]), (h, m)
        if thr is not None:
            _LAZY_LISTS[(body[0], thr)] = wr


@pytest.mark.parametrize("body", BODIES_16, ids=_ids(BODIES_16))
def test_staircase_exact_rescale_matches_oracle_and_the_lazy_lists(monkeypatch, body):
    """LA_FLAG_EXACT_RESCALE (tau = 0: the blocks run on every growth) on every 16-bit x64 body: the half-ulp bound, and write lists that
    equal the lazy launch's - the skip vote uses m_true, so lists do not depend on tau."""
    _setenv(monkeypatch, body)
    for thr in _thrs(body):
        wr = _launch_and_check(body, thr, exact=True)
        if thr is not None:
            if (body[0], thr) not in _LAZY_LISTS:
                _LAZY_LISTS[(body[0], thr)] = _launch_and_check(body, thr)
            assert torch.equal(wr, _LAZY_LISTS[(body[0], thr)]), (body[0], thr)


# ------------------------------------------------------------------------------------------------------- softmax_scale = 0, 1e-30
UNIFORM = [BY_ID[i] for i in ("bf16-d128", "fp16-d256", "e4m3-d64", "e4m3-d192", "half-bf16-d128", "half-bf16-d64")]


@pytest.mark.parametrize("scale", [0.0, 1e-30], ids=["scale0", "scale1e-30"])
@pytest.mark.parametrize("body", UNIFORM, ids=_ids(UNIFORM))
def test_uniform_attention_at_zero_and_tiny_scale(monkeypatch, body, scale):
    """Closed form, dense and on the read lists (thr = -inf; under LA_VOTE=half q-tile 1 is the empty-start half: m_ref = -inf times a
    zero scale). The oracle is held to the same closed form."""
    from liteattention_amd.flash_attn_interface import mha_fwd
    from oracle import oracle as orc
    _setenv(monkeypatch, body)
    name, dtype, D, _ = body
    bm = _tiles(body)
    (q, k, v, ds), (qd, kd, vd, dsd) = _device_inputs(dtype, D, _schedule(body))
    qf, kf, vf = (q.float(), k.float(), v.float()) if dtype == F8 else (q, k, v)
    p_round = fp8_p_round() if dtype == F8 else ("f16" if dtype == HF else True)
    for listed in (False, True):
        o_ref, lse_ref = sc.uniform_reference(v, ds, bm, listed)
        rd = sc.read_lists(bm) if listed else None
        kw, okw = {}, {}
        if listed:
            wr = torch.full_like(rd, -7).cuda()
            kw = dict(attn_read_list=rd.cuda(), attn_write_list=wr, thr=NEG_INF)
            okw = dict(read_list=rd, write_list=torch.zeros_like(rd), thr=NEG_INF)
        tol_o = f8._tol(o_ref) if dtype == F8 else hd._tol(o_ref, dtype, ulps=0.5)
        tol_l = fp8_lse_tol() if dtype == F8 else 1e-3
        o_orc, lse_orc, _ = orc.qkskip_fwd(qf, kf, vf, block_m=bm, block_n=sc.BN, p_round=p_round, softmax_scale=scale, **ds, **okw)
        assert (o_orc.double() - o_ref).abs().max().item() <= tol_o and (lse_orc.double() - lse_ref).abs().max().item() <= tol_l
        out, lse, *_ = mha_fwd(qd, kd, vd, softmax_scale=scale, **dsd, **kw)
        torch.cuda.synchronize()
        err_o, err_l = (out.double().cpu() - o_ref).abs().max().item(), (lse.double().cpu() - lse_ref).abs().max().item()
        print(f"score_range uniform {name} scale={scale:g} {'listed' if listed else 'dense'}: dO {err_o:.3e} (bound {tol_o:.3e}) dLSE {err_l:.3e} (bound {tol_l:.1e})")
        assert err_o <= tol_o, (name, listed, err_o, tol_o)
        assert err_l <= tol_l, (name, listed, err_l, tol_l)
        if listed:
            wr = wr.cpu()
            for h in range(sc.H):
                for m in range(rd.shape[2]):
                    n = int(rd[0, h, m, 0])
                    assert torch.equal(wr[0, h, m, :n + 1], rd[0, h, m, :n + 1]), (h, m)
