"""GPU: per-step threshold schedules, snapshot / restore and calibrate_error_schedule on the real kernels.

Workload, metric and bound rule: tests/error_schedule_common.py (fragmented_qkv(1, 1024, 2, 128, seed=3), 4 steps, tiles 256 x 64; bounds
from the constant -0.001 run, a baseline on code older than the calibrator). Bit-identity is asserted wherever two runs issue the same
launches on the same data (schedule against thresholds set by hand, calls after restore against calls after the snapshot). Lists
against the oracle follow tests/test_gpu_fragmented.py: at every step the oracle walks the list the kernel read, the written lists are
bit-equal except rows holding a tile whose decision margin is within 1e-3 of the threshold (test_gpu_parity._compare_lists)."""
import pytest
import torch

import error_schedule_common as C
from test_gpu_parity import _compare_lists

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn
SCHED = [-6.0, -3.0, -1.5, -0.5]


def _L():
    import liteattention_amd as L
    return L


def _inputs(kind, t, dev):
    if kind == "fp8":                      # the generator's fp32 values cast to e4m3, as tests/test_gpu_fragmented.py does
        from helpers import fragmented_qkv
        return [x.to(F8).to(dev) for x in fragmented_qkv(C.B, C.S, C.H, C.D, seed=C.SEED, step=t, steps=C.STEPS, dtype=torch.float32)]
    return [x.to(dev) for x in C.qkv_cpu(t)]


def _run(att, kind, dev, before_call):
    """STEPS calls; ``before_call(t)`` runs first. Returns per step (O, LSE, both list buffers, phase), cloned."""
    res = []
    for t in range(C.STEPS):
        before_call(t)
        out, lse = att(*_inputs(kind, t, dev), return_softmax_lse=True)
        res.append((out.clone(), lse.clone(), att._skip_list.clone(), att._phase))
    return res


def _same(a, b):
    for t, (x, y) in enumerate(zip(a, b)):
        # O of e4m3 inputs is bf16; compare bit patterns (NaN-proof) through the integer view
        assert torch.equal(x[0].view(torch.int16), y[0].view(torch.int16)), f"O differs at step {t}"
        assert torch.equal(x[1].view(torch.int32), y[1].view(torch.int32)), f"LSE differs at step {t}"
        assert torch.equal(x[2], y[2]) and x[3] == y[3], f"lists differ at step {t}"


@pytest.mark.parametrize("kind,list_dtype", [("bf16", torch.int32), ("fp8", torch.int32), ("bf16", torch.int16)])
def test_schedule_equals_thresholds_set_by_hand_before_each_call(kind, list_dtype):
    L, dev = _L(), torch.device("cuda", 0)
    sched = L.LiteAttention(threshold=-10.0, max_batch_size=C.B, list_dtype=list_dtype)
    sched.set_threshold_schedule(SCHED)
    a = _run(sched, kind, dev, lambda t: None)
    hand = L.LiteAttention(threshold=-10.0, max_batch_size=C.B, list_dtype=list_dtype)
    b = _run(hand, kind, dev, lambda t: setattr(hand, "threshold", SCHED[t]))
    _same(a, b)
    assert a[0][2].dtype == list_dtype
    const = L.LiteAttention(threshold=SCHED[1], max_batch_size=C.B, list_dtype=list_dtype)
    c = _run(const, kind, dev, lambda t: None)
    assert not torch.equal(c[-1][2], a[-1][2])                # and the schedule is not a no-op: a constant ends on other lists
    assert sched.get_skip_fraction() > const.get_skip_fraction() > 0.0


@pytest.mark.parametrize("list_dtype", [torch.int32, torch.int16])
def test_calls_after_restore_repeat_the_calls_after_the_snapshot(list_dtype):
    L, dev = _L(), torch.device("cuda", 0)
    att = L.LiteAttention(threshold=-10.0, max_batch_size=C.B, list_dtype=list_dtype)
    att.set_threshold_schedule(SCHED)
    for t in range(2):
        att(*_inputs("bf16", t, dev))
    snap = att.snapshot()
    ptr = att._skip_list.data_ptr()

    def two_more():
        res = []
        for t in (2, 3):
            out, lse = att(*_inputs("bf16", t, dev), return_softmax_lse=True)
            res.append((out.clone(), lse.clone(), att._skip_list.clone(), att._phase))
        return res

    first = two_more()
    assert not torch.equal(att._skip_list, snap["skip_list"])                     # the two steps did change the lists
    att.restore(snap)
    assert att._skip_list.data_ptr() == ptr and att._step == 2 and att.current_threshold() == SCHED[2]
    _same(first, two_more())
    assert snap["skip_list"].is_cuda and snap["skip_list"].dtype == list_dtype


@pytest.fixture(scope="module")
def gpu_case():
    """Computed once: dense outputs, the -0.001 baseline, the bounds, the calibrated schedule and the best constant of the grid."""
    from liteattention_amd.calibration import LiteAttentionBackend, calibrate_error_schedule
    dev = torch.device("cuda", 0)
    inputs = [_inputs("bf16", t, dev) for t in range(C.STEPS)]
    be = LiteAttentionBackend(lambda t: inputs[t], max_batch_size=C.B)
    e_hi, _, _ = C.run_thresholds(be, [C.HI_THR] * C.STEPS)
    bounds = C.bounds_from(e_hi)
    thresholds, trace = calibrate_error_schedule(lambda t: inputs[t], C.STEPS, bounds, max_batch_size=C.B)
    return dict(inputs=inputs, be=be, e_hi=e_hi, bounds=bounds, thresholds=thresholds, trace=trace, best=C.best_constant(be, bounds))


def test_calibrated_schedule_on_the_kernels_meets_every_bound_and_beats_the_best_constant(gpu_case):
    c = gpu_case
    thresholds, trace, bounds = c["thresholds"], c["trace"], c["bounds"]
    assert all(e > 0 for e in c["e_hi"][1:]), c["e_hi"]
    errs, skips, _ = C.run_thresholds(c["be"], thresholds)                         # replay from a fresh state
    print("schedule", thresholds, "errors", errs, "bounds", bounds, "skips", skips, "best constant", c["best"], "e_hi", c["e_hi"])
    assert all(e <= b for e, b in zip(errs, bounds)), (errs, bounds)
    assert all(tr["bound_met"] for tr in trace)
    assert all(thr != -20.0 for thr in thresholds) and thresholds[-1] == thresholds[-2]
    for t, tr in enumerate(trace):
        assert tr["threshold"] == thresholds[t] and tr["bound"] == bounds[t]
        assert tr["error"] == errs[t] and tr["skip_fraction"] == skips[t]          # same launches, same data: the same numbers
    assert c["best"] is not None, "no constant of the grid meets the bounds"
    assert skips[-1] > c["best"][1], (skips[-1], c["best"])


def test_replayed_schedule_errors_match_torch_and_lists_match_the_oracle(gpu_case):
    L, dev = _L(), torch.device("cuda", 0)
    from liteattention_amd.calibration import output_error
    from oracle import oracle as orc
    c = gpu_case
    att = L.LiteAttention(threshold=-10.0, max_batch_size=C.B)
    att.set_threshold_schedule(c["thresholds"])
    md = orc.expand_must_do_ref([0, 0], C.BN, C.KT + 1)
    margins = torch.empty(C.B, C.H, C.QT, C.KT)
    borderline = 0
    for t in range(C.STEPS):
        q, k, v = c["inputs"][t]
        dense = L.flash_attn_func(q, k, v)
        rd_idx = att._phase if att._skip_list is not None else 0
        out = att(q, k, v)
        # the device statistic against torch in fp64 on the same two tensors
        got = output_error(out, dense).rel_l1
        o64, d64 = out.double(), dense.double()
        want = (o64 - d64).abs().sum(dim=(1, 3)) / d64.abs().sum(dim=(1, 3))
        torch.testing.assert_close(got, want, rtol=1e-9, atol=0.0)
        assert float(got.max()) == c["trace"][t]["error"]                          # and it is the committed run's error
        # the lists against the oracle walking the same read list at this step's threshold
        rd, wr = att._skip_list[rd_idx].cpu(), att._skip_list[1 - rd_idx].cpu()
        wr_orc = torch.zeros_like(wr)
        orc.qkskip_fwd(q.cpu(), k.cpu(), v.cpu(), block_m=C.BM, block_n=C.BN, read_list=rd, write_list=wr_orc, must_do_list=md,
                       thr=c["thresholds"][t], margins=margins)
        bad, border = _compare_lists(orc, rd, wr, wr_orc, margins, c["thresholds"][t], C.B)
        assert bad == 0, f"step {t}: {bad} rows differ from the oracle with no borderline tile"
        borderline += border
    assert borderline <= 4
    assert att.get_skip_fraction() > 0.0
