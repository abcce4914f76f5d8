"""CPU: the score staircases of tests/score_range_cases.py really drive the lazy O-rescale path the way tests/test_gpu_score_range.py
relies on. Everything is read in fp64 from the CAST inputs and the descaled scores, with each tau taken from where the build takes it
(kRescaleTauBf16 in la_api.hip; LA_X64F8_TAU_<mode> of the generated la_fwd_x64_fp8*_consts.h), through ``lazy_walk`` - the fp64 model of
a wave's shared trigger - at both wave sizes (64 rows at head dims <= 128, 32 above). Per (dtype, tau) pair of a GPU case, per head dim
and head, some row shows

  a  a sub-tau step, then a second sub-tau step whose cumulative lag crosses tau          (not at tau = 0: no step is below it)
  b  a single step in (tau, tau + 1)                                                       (not at tau = 0)
  c  a step above 2 tau
  d  a step of at least 160 log2 units (alpha underflows to 0)
  e  a trigger at position 1 and a trigger at the last walked position
  f  flat rows in every 32-row group of the mixed rows, beside rows that trigger; the all-flat 64-row block never triggers
  g  descending rows whose later tiles give P = 0

and on the hand-built read lists: a trigger on the first tile after a gap, a trigger at the last position (head 0), a walk that ends
with a lag (head 1), and a q-tile that starts one position late on a tile that is a trigger step of the q-tile before it.

Sensitivity: the fp64 model with one injected fault (alpha not applied to O at the last trigger; alpha applied to l but never to O; the
LSE formed from m_true over sums kept relative to m_ref) misses the bound of the body by at least 10 x on one of the walks the GPU test
launches. A fault at an EARLY trigger cannot show in any output: what was accumulated before it weighs 2^-(growth after it), and the
staircase grows by hundreds of log2 units - which is why the lists end at different positions.

The C oracle alone stays within the existing bound of each body against the plain fp64 softmax (it is the reference of the GPU test), and
every oracle margin of the list launches is at least 0.05 away from the finite threshold (the list comparison allows 1e-3)."""
import glob
import os
import re

import pytest
import torch

import score_range_cases as sc
from score_range_cases import F8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "liteattention_amd", "csrc")
BF, HF = torch.bfloat16, torch.float16
DIMS = (64, 96, 128, 192, 256)


def _tau_16bit():
    with open(os.path.join(CSRC, "la_api.hip")) as f:
        return float(re.search(r"kRescaleTauBf16\s*=\s*([0-9.]+)f", f.read()).group(1))


def _tau_fp8():
    """{mode: tau} from the generated headers (mode 0: encoded; 1: mfma_rowsum; 2: the default, fp32 row sums)."""
    out = {}
    for path in glob.glob(os.path.join(CSRC, "la_fwd_x64_fp8*_consts.h")):
        with open(path) as f:
            for mode, val in re.findall(r"#define LA_X64F8_TAU_(\d) ([0-9.]+)f", f.read()):
                out[int(mode)] = float(val)
    return out


# (id, dtype, schedule, tau as the build has it, oracle p_round, fp8 form or None)
def _cases():
    t16, t8 = _tau_16bit(), _tau_fp8()
    assert sorted(t8) == [0, 1, 2], "the generated la_fwd_x64_fp8*_consts.h are missing: run the build"
    return [("bf16", BF, "s8", t16, True, None), ("fp16", HF, "s8", t16, "f16", None),
            ("bf16-exact", BF, "s8", 0.0, True, None), ("fp16-exact", HF, "s8", 0.0, "f16", None),
            ("e4m3", F8, "s2", t8[2], "fp8", "reference"), ("e4m3-mfma_rowsum", F8, "s2", t8[1], "fp8", "mfma_rowsum"),
            ("e4m3-encoded", F8, "s32", t8[0], "fp8_lin", "encoded")]


CASES = _cases()
_INPUTS = {}


def _inputs(dtype, D, schedule):
    key = (dtype, D, schedule)
    if key not in _INPUTS:
        q, k, v, ds = sc.staircase_qkv(dtype, D, schedule)
        _INPUTS[key] = (q, k, v, ds, [sc.scores_log2(q, k, ds, h) for h in range(sc.H)], [sc.v_f64(v, ds, h) for h in range(sc.H)])
    return _INPUTS[key]


def test_the_schedules_are_built_around_the_builds_taus():
    """A changed tau in the sources must fail here, not quietly turn the staircases into something else."""
    assert {c[3] for c in CASES} == {0.0, 2.0, 8.0, 32.0}
    for _, _, schedule, tau, _, _ in CASES:
        assert tau in (0.0, sc.TAUS[schedule])
    q, k, v, ds = sc.staircase_qkv(F8, 64, "s2")
    assert q.dtype == k.dtype == v.dtype == F8 and tuple(q.shape) == (1, sc.SQ, sc.H, 64) and tuple(k.shape) == (1, sc.SK, sc.H, 64)
    for n in ("q_descale", "k_descale", "v_descale"):
        assert tuple(ds[n].shape) == (1, sc.H) and ds[n].dtype == torch.float32 and float(ds[n][0, 0]) != float(ds[n][0, 1])
    assert sc.log2_scale(64, ds, 0) != sc.log2_scale(64, ds, 1)                   # tau / c differs per head
    assert sc.staircase_qkv(BF, 96, "s8")[3] == {} and all(bool(torch.isfinite(x.float()).all()) for x in (q, k, v))


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_dense_walk_shows_every_event(case, D):
    _, dtype, schedule, tau, _, _ = case
    q, k, v, ds, s2s, vs = _inputs(dtype, D, schedule)
    gains = sc.row_gains()
    for h in range(sc.H):
        for group in (32, 64):
            _, _, tr = sc.lazy_walk(s2s[h], vs[h], sc.DENSE_WALK, tau, group)
            ev = sc.events(tr, tau)
            want = [n for n in ev if tau > 0 or n not in ("a", "b")]
            assert all(ev[n] for n in want), (h, group, ev)
            # f: every 32-row group of the mixed rows holds gain-0 rows that never trigger on their own beside rows that do; the flat block never does
            own = torch.stack([t["own"] for t in tr[1:]]).any(dim=0)
            wave = torch.stack([t["wave"] for t in tr[1:]]).any(dim=0)
            for rows in sc.MIXED_ROWS:
                for g0 in range(rows.start, rows.stop, 32):
                    flat = [r for r in range(g0, g0 + 32) if gains[r] == 0.0]
                    assert flat and bool(own[g0:g0 + 32].any()) and bool(wave[flat].all())
                    assert tau == 0 or not bool(own[flat].any())
            if tau > 0:
                assert not bool(wave[sc.FLAT_ROWS].any()) and not bool(own[sc.FLAT_ROWS].any())
            # g: the descending rows never grow, and their last walked tiles lie more than 150 log2 units below the maximum: P = 0 in fp32
            grown = torch.stack([t["step"] for t in tr[1:]]).sum(dim=0)
            assert bool((grown[sc.DESC_ROWS] == 0).all())
            below = s2s[h][sc.DESC_ROWS, :sc.BN].max(dim=1).values - s2s[h][sc.DESC_ROWS].max(dim=1).values
            assert int((below < -150.0).sum()) >= 8 and bool((below < -30.0).all())


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_list_walks_trigger_after_gaps_at_the_end_and_end_with_a_lag(case, D):
    _, dtype, schedule, tau, _, _ = case
    q, k, v, ds, s2s, vs = _inputs(dtype, D, schedule)
    for group in (32, 64):
        w0, w1 = sc.walk_of(sc.LIST_H0), sc.walk_of(sc.LIST_H1)
        o, lse, tr = sc.lazy_walk(s2s[0], vs[0], w0, tau, group)
        after_gap = [p for p in range(1, len(w0)) if w0[p] != w0[p - 1] - 1]
        assert len(after_gap) == 3 and sum(bool(tr[p]["own"].any()) for p in after_gap) >= 2
        assert bool(tr[len(w0) - 1]["own"].any())                                     # ... and at the last walked position
        o, lse, tr = sc.lazy_walk(s2s[1], vs[1], w1, tau, group)
        last = tr[len(w1) - 1]
        if tau > 0:                                                                      # the walk of head 1 ends with a lag: no trigger, growth
            assert not bool(last["wave"][:128].any()) and float(last["step"][:128].max()) > 0.5 * tau
        # the late lists drop exactly the first position, and their first tile is a trigger step of the q-tile that started at position 0
        for h, (full, late) in enumerate(((sc.LIST_H0, sc.LIST_H0_LATE), (sc.LIST_H1, sc.LIST_H1_LATE))):
            assert sc.walk_of(late) == sc.walk_of(full)[1:]
            _, _, tr = sc.lazy_walk(s2s[h], vs[h], sc.walk_of(full), tau, group, rows=(0, 128))
            assert bool(tr[1]["own"].any())
    for bm in (128, 256):
        rd = sc.read_lists(bm)
        assert rd.shape == (1, sc.H, -(-sc.SQ // bm), sc.KT + 1) and rd.dtype == torch.int32
        assert rd[0, 0, 1, 1] == sc.KT - 2 and rd[0, 0, 0, 1] == sc.KT - 1


def _bound(case, o_ref, monkeypatch):
    """(bound on O, bound on the LSE) the GPU test holds the body to against the oracle."""
    import test_gpu_fp8 as f8
    import test_gpu_head_dims as hd
    from helpers import fp8_lse_tol
    _, dtype, _, tau, _, form = case
    if dtype == F8:
        monkeypatch.setenv("LA_FP8_P", "" if form == "reference" else form)
        return f8._tol(o_ref), fp8_lse_tol()
    return hd._tol(o_ref, dtype, ulps=0.5 if tau == 0 else 1.0), 1e-3


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_an_injected_fault_misses_the_bound_ten_times_over(case, D, monkeypatch):
    _, dtype, schedule, tau, _, _ = case
    q, k, v, ds, s2s, vs = _inputs(dtype, D, schedule)
    group = 64 if D <= 128 else 32
    w0, w1 = sc.walk_of(sc.LIST_H0), sc.walk_of(sc.LIST_H1)
    # the model without a fault is the plain softmax
    for h, walk in ((0, sc.DENSE_WALK), (0, w0), (1, w1)):
        o, lse, _ = sc.lazy_walk(s2s[h], vs[h], walk, tau, group)
        o64, lse64 = sc.dense_f64(s2s[h], vs[h], walk)
        assert float((o - o64).abs().max()) < 1e-12 and float((lse - lse64).abs().max()) < 1e-10
    o64, lse64 = sc.dense_f64(s2s[0], vs[0])
    tol_o, tol_lse = _bound(case, o64, monkeypatch)
    for fault in (("o_once", sc.KT - 1), ("o_never", None)):
        o, lse, _ = sc.lazy_walk(s2s[0], vs[0], sc.DENSE_WALK, tau, group, fault=fault)
        assert float((o - o64).abs().max()) >= 10.0 * tol_o, (fault, float((o - o64).abs().max()), tol_o)
    if tau > 0:        # (at tau = 0 m_ref is m_true: the fault does not exist)
        o64, lse64 = sc.dense_f64(s2s[1], vs[1], w1)
        _, lse, _ = sc.lazy_walk(s2s[1], vs[1], w1, tau, group, fault=("lse_true", None))
        assert float((lse - lse64).abs().max()) >= 10.0 * tol_lse, (float((lse - lse64).abs().max()), tol_lse)


_ORACLE = {}


def oracle_runs(dtype, D, schedule, p_round, bm, thr):
    """(o, lse) dense; (o, lse, write list, margins) on the read lists at `thr` - the C oracle in the body's own form."""
    from oracle import oracle as orc
    key = (dtype, D, schedule, p_round, bm, thr)
    if key not in _ORACLE:
        q, k, v, ds = _inputs(dtype, D, schedule)[:4]
        qf, kf, vf = (q.float(), k.float(), v.float()) if dtype == F8 else (q, k, v)
        dense = orc.qkskip_fwd(qf, kf, vf, block_m=bm, block_n=sc.BN, p_round=p_round, **ds)[:2]
        rd = sc.read_lists(bm)
        wr, mg = torch.zeros_like(rd), torch.empty(1, sc.H, rd.shape[2], sc.KT)
        o, lse, _ = orc.qkskip_fwd(qf, kf, vf, block_m=bm, block_n=sc.BN, p_round=p_round, read_list=rd, write_list=wr, thr=thr, margins=mg, **ds)
        _ORACLE[key] = (dense, (o, lse, wr, mg))
    return _ORACLE[key]


def _f64_reference(dtype, D, schedule, bm, listed):
    q, k, v, ds, s2s, vs = _inputs(dtype, D, schedule)
    o, lse = torch.empty(1, sc.SQ, sc.H, D, dtype=torch.float64), torch.empty(1, sc.H, sc.SQ, dtype=torch.float64)
    for h in range(sc.H):
        for m in range(-(-sc.SQ // bm)):
            rows = slice(m * bm, min((m + 1) * bm, sc.SQ))
            o[0, rows, h], lse[0, h, rows] = sc.dense_f64(s2s[h][rows], vs[h], sc.walk_of(sc.list_ranges(h, m)) if listed else None)
    return o, lse


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("case", [c for c in CASES if c[3] != 0.0], ids=[c[0] for c in CASES if c[3] != 0.0])
def test_the_oracle_carries_the_staircases(case, D, monkeypatch):
    """Dense and listed, at both q-tile sizes a body of this head dim can have: the C oracle against the fp64 softmax, inside the bound the
    bodies are held to against the oracle (the fp8 forms: the LSE against the EXACT values, helpers.fp8_lse_tol_vs_exact); finite; and
    every margin at least 0.05 from the finite threshold, with the descending q-tile dropping tiles and the rising ones keeping them."""
    from helpers import fp8_lse_tol_vs_exact
    _, dtype, schedule, tau, p_round, form = case
    thr = sc.finite_thr(schedule)
    for bm in ((128, 256) if D <= 128 else (128,)):
        dense, (o_l, lse_l, wr, mg) = oracle_runs(dtype, D, schedule, p_round, bm, thr)
        for (o, lse), listed in ((dense, False), ((o_l, lse_l), True)):
            o64, lse64 = _f64_reference(dtype, D, schedule, bm, listed)
            tol_o, tol_lse = _bound(case, o64, monkeypatch)
            if dtype == F8:
                tol_lse = fp8_lse_tol_vs_exact()
            assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse).all())
            assert float((o.double() - o64).abs().max()) <= tol_o and float((lse.double() - lse64).abs().max()) <= tol_lse
        m = mg[~torch.isnan(mg)]
        assert float((m - thr).abs().min()) >= 0.05
        for h in range(sc.H):
            walked = len(sc.walk_of(sc.list_ranges(h, 0)))
            assert int(wr[0, h, -1, 0]) == 2 and len(sc.walk_of(wr[0, h, -1, 1:3].tolist())) <= 2          # the descending q-tile: flagged everywhere
            kept = len(sc.walk_of(wr[0, h, 0, 1:1 + int(wr[0, h, 0, 0])].tolist()))
            assert 4 <= kept < walked                             # the rising q-tile keeps its growing tiles and drops the flat ones


@pytest.mark.parametrize("scale", [0.0, 1e-30])
@pytest.mark.parametrize("case", [c for c in CASES if c[3] != 0.0], ids=[c[0] for c in CASES if c[3] != 0.0])
def test_the_oracle_at_zero_and_tiny_scale_is_uniform_attention(case, scale, monkeypatch):
    """softmax_scale = 0: every score is 0 - O = mean of V over the walked keys, LSE = ln of their number; the masked keys of the ragged last
    tile keep P = 0 (-inf * 0 is NaN in fp32: the oracle masks by value, not by product)."""
    from oracle import oracle as orc
    _, dtype, schedule, tau, p_round, form = case
    for D, bm in ((64, 256), (192, 128), (128, 128)):
        q, k, v, ds = _inputs(dtype, D, schedule)[:4]
        qf, kf, vf = (q.float(), k.float(), v.float()) if dtype == F8 else (q, k, v)
        for listed in (False, True):
            rd = sc.read_lists(bm)
            kw = dict(read_list=rd, write_list=torch.zeros_like(rd), thr=float("-inf")) if listed else {}
            o, lse, _ = orc.qkskip_fwd(qf, kf, vf, block_m=bm, block_n=sc.BN, p_round=p_round, softmax_scale=scale, **ds, **kw)
            o_ref, lse_ref = sc.uniform_reference(v, ds, bm, listed)
            tol_o, tol_lse = _bound(case, o_ref, monkeypatch)
            assert float((o.double() - o_ref).abs().max()) <= min(tol_o, 1e-5) and float((lse.double() - lse_ref).abs().max()) <= min(tol_lse, 1e-5)
            if listed:
                assert torch.equal(kw["write_list"][..., :9], rd[..., :9])
