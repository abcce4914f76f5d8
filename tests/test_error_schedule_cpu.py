"""CPU: error-bounded threshold schedules - the la_output_error boundary (symbol, argument checks without a device), the per-step
threshold host logic of LiteAttention (recorder in place of the kernel call, as tests/test_host_logic.py does) and
calibrate_error_schedule through a backend built on the CPU oracle (tests/error_schedule_common.py: workload and bound rule)."""
import ctypes
import os
import re

import pytest
import torch

import liteattention_amd as L
from liteattention_amd import _cabi
from liteattention_amd import lite_attention as la_mod
from liteattention_amd.calibration import calibrate_error_schedule

import error_schedule_common as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the boundary
def test_output_error_is_exported_declared_and_bound_under_abi_9():
    lib = _cabi.load()
    assert "la_output_error" in _cabi.EXPORTED_SYMBOLS and hasattr(lib, "la_output_error")
    assert lib.la_abi_version() == 9 == _cabi.LA_ABI_VERSION
    header = open(os.path.join(ROOT, "include", "lite_attention_amd.h")).read()
    assert re.search(r"^int la_output_error\(", header, flags=re.M)
    assert "#define LA_ABI_VERSION 9" in header and "#define LA_STAT_COUNT 6" in header
    assert len(lib.la_output_error.argtypes) == 17 and lib.la_output_error.restype is ctypes.c_int
    assert (_cabi.LA_STAT_ABS_DIFF, _cabi.LA_STAT_ABS_REF, _cabi.LA_STAT_SQ_DIFF, _cabi.LA_STAT_SQ_REF, _cabi.LA_STAT_MAX_ABS_DIFF,
            _cabi.LA_STAT_NONFINITE, _cabi.LA_STAT_COUNT) == (0, 1, 2, 3, 4, 5, 6)
    for i, name in enumerate(("ABS_DIFF", "ABS_REF", "SQ_DIFF", "SQ_REF", "MAX_ABS_DIFF", "NONFINITE")):
        assert re.search(rf"LA_STAT_{name} = {i}\b", header), name


def _call(out=0x1000, odt=_cabi.LA_DTYPE_BF16, ostr=(4096, 256, 128), ref=0x2000, rdt=_cabi.LA_DTYPE_BF16, rstr=(4096, 256, 128),
          shape=(1, 16, 2, 128), rpb=16, stats=0x3000):
    return _cabi.load().la_output_error(out, odt, *ostr, ref, rdt, *rstr, *shape, rpb, stats, None)


def test_output_error_argument_checks_need_no_device():
    """Every code of the header comment comes back before any HIP call (the pointers are never dereferenced)."""
    E = _cabi
    assert _call(out=None) == _call(ref=None) == _call(stats=None) == E.LA_ERR_NULL_ARG
    for bad in (E.LA_DTYPE_FP8_E4M3, 4, -1):
        assert _call(odt=bad) == _call(rdt=bad) == E.LA_ERR_DTYPE
    for i in range(4):
        for v in (0, -1):
            shape = [1, 16, 2, 128]
            shape[i] = v
            assert _call(shape=tuple(shape)) == E.LA_ERR_SHAPE, (i, v)
    assert _call(rpb=0) == _call(rpb=-3) == E.LA_ERR_SHAPE
    for d in (4, 12, 100, 129):
        assert _call(shape=(1, 16, 2, d)) == E.LA_ERR_HEAD_DIM, d
    for i in range(3):                                                     # a negative stride, of either operand
        s = [4096, 256, 128]
        s[i] = -s[i]
        assert _call(ostr=tuple(s)) == _call(rstr=tuple(s)) == E.LA_ERR_STRIDE, i
    # 16-bit elements: row starts every 8 elements; fp32: every 4
    assert _call(ostr=(4096, 260, 128)) == _call(rstr=(4096, 256, 132)) == E.LA_ERR_STRIDE
    assert _call(rdt=E.LA_DTYPE_FP32, rstr=(4096, 258, 128)) == _call(odt=E.LA_DTYPE_FP32, ostr=(4096, 256, 130)) == E.LA_ERR_STRIDE
    assert _call(odt=E.LA_DTYPE_FP16, ostr=(4096, 256, 124)) == E.LA_ERR_STRIDE
    assert _call(out=0x1008) == _call(ref=0x2004) == E.LA_ERR_STRIDE        # the first row itself
    assert _call(shape=(2, 16, 2, 128), ostr=(4100, 256, 128)) == E.LA_ERR_STRIDE      # the batch stride, once there is a second batch
    # one workgroup per stats row: more than 2^31 - 1 of them is refused, not truncated
    assert _call(shape=(2, 2 ** 31 - 1, 2, 8), rpb=1, ostr=(0, 8, 8), rstr=(0, 8, 8)) == E.LA_ERR_SHAPE
    # the order of the checks: NULL, dtype, shape, head_dim, stride
    assert _call(out=None, odt=9, shape=(0, 0, 0, 4)) == E.LA_ERR_NULL_ARG
    assert _call(odt=9, shape=(0, 16, 2, 4), ostr=(-1, -1, -1)) == E.LA_ERR_DTYPE
    assert _call(shape=(0, 16, 2, 4), ostr=(-1, -1, -1)) == E.LA_ERR_SHAPE
    assert _call(shape=(1, 16, 2, 4), ostr=(-1, -1, -1)) == E.LA_ERR_HEAD_DIM


# ---------------------------------------------------------------------------------------------------------------- host logic
class Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, q, k, v, softmax_scale=None, attn_read_list=None, attn_must_do_list=None,
                 attn_write_list=None, thr=None, return_softmax_lse=False, **kw):
        self.calls.append(dict(read=attn_read_list, write=attn_write_list, must_do=attn_must_do_list, thr=thr,
                               scale=softmax_scale, lse=return_softmax_lse, extra=kw))
        out = torch.zeros_like(q)
        return (out, torch.zeros(q.shape[0], q.shape[2], q.shape[1])) if return_softmax_lse else out


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(la_mod, "flash_attn_func", r)
    return r


Q1 = torch.zeros(1, 1000, 2, 128, dtype=torch.bfloat16)
Q2 = torch.zeros(1, 700, 2, 128, dtype=torch.bfloat16)
SCHED = [-9.0, -5.0, -2.5]


def test_schedule_gives_call_i_its_threshold_and_then_holds_the_last(rec):
    att = L.LiteAttention(threshold=-7.0)
    att.set_threshold_schedule(SCHED)
    n = len(SCHED)
    for i in range(n + 3):
        assert att.current_threshold() == SCHED[min(i, n - 1)]
        att(Q1, Q1, Q1)
    assert [c["thr"] for c in rec.calls] == [SCHED[min(i, n - 1)] for i in range(n + 3)]
    assert att.threshold == -7.0                                              # the constant is kept beside the schedule
    # read / write buffers still alternate as without a schedule
    assert [c["read"].data_ptr() for c in rec.calls[:4]] == [rec.calls[0]["read"].data_ptr(), rec.calls[0]["write"].data_ptr()] * 2


def test_dense_calls_do_not_advance_the_schedule(rec):
    att = L.LiteAttention(threshold=-7.0)
    att.set_threshold_schedule(SCHED)
    att(Q1, Q1, Q1)
    att.enable_skip_optimization(False)
    att(Q1, Q1, Q1)
    att(Q1, Q1, Q1)
    att.enable_skip_optimization(True)
    assert att.current_threshold() == SCHED[1]
    att(Q1, Q1, Q1)
    att(Q1, Q1, Q1)
    sparse = [c for c in rec.calls if c["read"] is not None]
    assert [c["thr"] for c in sparse] == SCHED
    assert len(rec.calls) == 5 and all(c["read"] is None and c["write"] is None for c in rec.calls[1:3])


def test_reset_and_shape_change_restart_the_schedule(rec):
    att = L.LiteAttention()
    att.set_threshold_schedule(SCHED)
    att(Q1, Q1, Q1)
    att(Q1, Q1, Q1)
    att.reset_skip_state()
    assert att.current_threshold() == SCHED[0]
    att(Q1, Q1, Q1)
    att(Q1, Q1, Q1)
    att(Q2, Q2, Q2)                                                           # another sequence length: the lists are rebuilt
    att(Q2, Q2, Q2)
    assert [c["thr"] for c in rec.calls] == [SCHED[0], SCHED[1], SCHED[0], SCHED[1], SCHED[0], SCHED[1]]


def test_call_windowed_follows_the_schedule(monkeypatch):
    from liteattention_amd import flash_attn_interface as fi
    seen = []

    def fake_mha_fwd(q, k, v, **kw):
        seen.append(kw["thr"])
        return torch.zeros_like(q), torch.zeros(q.shape[0], q.shape[2], q.shape[1])

    monkeypatch.setattr(fi, "mha_fwd", fake_mha_fwd)
    att = L.LiteAttention()
    att.set_threshold_schedule(SCHED)
    for _ in range(4):
        att.call_windowed(Q1, Q1, Q1, [(0, 2), (2, 2)])
    assert seen == SCHED + [SCHED[-1]]


def test_set_threshold_clears_the_schedule_and_entries_are_validated(rec, monkeypatch):
    monkeypatch.delenv("LITE_ATTENTION_DEBUG", raising=False)
    att = L.LiteAttention()
    att.set_threshold_schedule(SCHED)
    att(Q1, Q1, Q1)
    att.set_threshold(-4.0)
    assert att.current_threshold() == -4.0
    att(Q1, Q1, Q1)
    assert [c["thr"] for c in rec.calls] == [SCHED[0], -4.0]
    for bad in ([-3.0, 0.0], [0.5], [-1.0, -2.0, 1e-9]):
        with pytest.raises(ValueError):
            att.set_threshold_schedule(bad)
    with pytest.raises(ValueError):
        att.set_threshold_schedule([])
    assert att.current_threshold() == -4.0                                     # a refused schedule changes nothing
    att.set_threshold_schedule(SCHED)
    att.set_threshold_schedule(None)
    assert att.current_threshold() == -4.0
    monkeypatch.setenv("LITE_ATTENTION_DEBUG", "1")                            # as set_threshold: the debug switch admits thr >= 0
    att.set_threshold_schedule([-1.0, 0.25])
    assert att.current_threshold() in (-1.0, 0.25)


def test_without_a_schedule_the_recorded_call_is_the_one_of_before(rec):
    att = L.LiteAttention(threshold=-6.5)
    att(Q1, Q1, Q1)
    att(Q1, Q1, Q1, scale=0.25, return_softmax_lse=True)
    att.enable_skip_optimization(False)
    att(Q1, Q1, Q1)
    a, b, c = rec.calls
    assert a["thr"] == b["thr"] == c["thr"] == -6.5 == att.threshold == att.current_threshold()
    assert a["extra"] == {} and b["extra"] == {} and c["extra"] == {"num_splits": -1}       # the exact keyword set of the call
    assert (a["scale"], a["lse"], b["scale"], b["lse"]) == (None, False, 0.25, True)
    assert a["must_do"][:3].tolist() == [2, 0, 0] and c["must_do"] is None


def test_forwarders_hand_the_schedule_to_every_state(rec):
    from liteattention_amd.parallel import HeadShardedLiteAttention, RingSeqParallelLiteAttention, UlyssesLiteAttention
    sp = L.SeqParallelLiteAttention(3)
    sp.set_threshold_schedule(SCHED)
    assert all(la._threshold_schedule == tuple(SCHED) for la in sp.lite_attention)
    sp.set_threshold(-2.0)
    assert all(la._threshold_schedule is None and la.threshold == -2.0 for la in sp.lite_attention)
    hs, ul, ring = HeadShardedLiteAttention(2), UlyssesLiteAttention(2), RingSeqParallelLiteAttention()
    for obj, states in ((hs, [hs.local]), (ul, [ul.local]), (ring, ring.states.lite_attention)):
        obj.set_threshold_schedule(SCHED)
        assert all(la._threshold_schedule == tuple(SCHED) for la in states)
        obj.set_threshold_schedule(None)
        assert all(la._threshold_schedule is None for la in states)
    # every driver forwards every setter of its states (the head table: sliced to the rank's heads where heads are sharded)
    for obj in (sp, hs, ul, ring):
        for name in ("reset_skip_state", "set_threshold", "set_threshold_schedule", "set_head_thresholds"):
            assert callable(getattr(obj, name)), (type(obj).__name__, name)
    for obj, states in ((ul, [ul.local]), (ring, ring.states.lite_attention)):
        obj.set_head_thresholds([-1.0, -2.0])
        assert all(la._head_thresholds.tolist() == [-1.0, -2.0] for la in states)
        obj.set_threshold_schedule(SCHED)                  # the last setter wins, through the forwarders too
        assert all(la._head_thresholds is None for la in states)
    ul.inner.h0, ul.inner.h1 = 1, 2                        # the slice a second rank of two would own
    ul.set_head_thresholds([[-1.0, -2.0], [-3.0, -4.0]])
    assert ul.local._head_thresholds.tolist() == [[-2.0], [-4.0]]
    with pytest.raises(ValueError):
        ul.set_head_thresholds([-1.0, -2.0, -3.0])
    ul.set_head_thresholds(None)
    assert ul.local._head_thresholds is None


def test_state_dict_round_trip_keeps_schedule_and_step_and_old_states_load(rec):
    att = L.LiteAttention(threshold=-7.0)
    att.set_threshold_schedule(SCHED)
    att(Q1, Q1, Q1)
    att(Q1, Q1, Q1)
    state = att.state_dict()
    assert state["threshold_schedule"] == SCHED and state["step"] == 2
    other = L.LiteAttention()
    other.load_state_dict(state, device="cpu")
    assert other.current_threshold() == SCHED[2] and other._step == 2 and other._phase == att._phase
    assert torch.equal(other._skip_list, att._skip_list)
    other(Q1, Q1, Q1)
    assert rec.calls[-1]["thr"] == SCHED[2]
    old = {k: v for k, v in state.items() if k not in ("threshold_schedule", "step")}     # a state saved before schedules existed
    third = L.LiteAttention()
    third.set_threshold_schedule(SCHED)
    third.load_state_dict(old, device="cpu")
    assert third._threshold_schedule is None and third._step == 0 and third.current_threshold() == -7.0
    third(Q1, Q1, Q1)
    assert rec.calls[-1]["thr"] == -7.0


def test_snapshot_and_restore_bring_back_lists_phase_and_step(rec):
    att = L.LiteAttention()
    att.set_threshold_schedule(SCHED)
    att(Q1, Q1, Q1)
    att._skip_list[att._phase, 0, 0, 0, :3] = torch.tensor([2, 7, 3], dtype=torch.int32)
    snap = att.snapshot()
    kept, ptr = att._skip_list.clone(), att._skip_list.data_ptr()
    att(Q1, Q1, Q1)
    att._skip_list.zero_()
    att.restore(snap)
    assert torch.equal(att._skip_list, kept) and att._skip_list.data_ptr() == ptr         # overwritten in place
    assert (att._phase, att._step, att.current_threshold()) == (1, 1, SCHED[1])
    att._skip_list.zero_()
    assert torch.equal(snap["skip_list"], kept)                                           # the snapshot is a copy and stays one
    fresh = L.LiteAttention()
    empty = fresh.snapshot()
    fresh(Q1, Q1, Q1)
    fresh.restore(empty)
    assert fresh._skip_list is None and fresh._step == 0


# ---------------------------------------------------------------------------------------------------------------- the calibrator
@pytest.fixture(scope="module")
def oracle_case():
    """Computed once: the -0.001 baseline, the bounds derived from it, the calibrated schedule and the best constant of the grid."""
    be = C.OracleBackend()
    e_hi, _, _ = C.run_thresholds(be, [C.HI_THR] * C.STEPS)
    bounds = C.bounds_from(e_hi)
    thresholds, trace = calibrate_error_schedule(None, C.STEPS, bounds, backend=be)
    return dict(be=be, e_hi=e_hi, bounds=bounds, thresholds=thresholds, trace=trace, best=C.best_constant(be, bounds))


def test_calibrated_schedule_meets_every_bound_and_beats_the_best_constant(oracle_case):
    c = oracle_case
    thresholds, trace, bounds = c["thresholds"], c["trace"], c["bounds"]
    assert len(thresholds) == len(trace) == C.STEPS and thresholds[-1] == thresholds[-2]
    assert all(e > 0 for e in c["e_hi"][1:]), c["e_hi"]                            # the baseline does skip: the bounds bind
    errs, skips, _ = C.run_thresholds(c["be"], thresholds)                         # replay from a fresh state
    print("schedule", thresholds, "errors", errs, "bounds", bounds, "skips", skips, "best constant", c["best"])
    assert all(e <= b for e, b in zip(errs, bounds)), (errs, bounds)
    assert all(tr["bound_met"] for tr in trace)
    assert all(thr != -20.0 for thr in thresholds)
    for t, tr in enumerate(trace):                                                 # the trace is the replay
        assert tr["threshold"] == thresholds[t] and tr["bound"] == bounds[t]
        assert tr["error"] == errs[t] and tr["skip_fraction"] == skips[t]
    assert c["best"] is not None and c["best"][0] == -3.5                          # checked with the oracle when the test was written
    assert skips[-1] > c["best"][1], (skips[-1], c["best"])
    assert abs(skips[-1] - 0.406) < 5e-3 and abs(c["best"][1] - 0.305) < 5e-3
    assert thresholds == sorted(thresholds)                                        # stricter early, looser late: what the bounds ask


def test_every_kept_threshold_is_a_probed_value(oracle_case):
    """Bisection points of [-20, -0.001): k / 2^8 of the way for an odd-or-even k - never an interpolation between probes."""
    for thr in oracle_case["thresholds"]:
        x = (thr + 20.0) / (20.0 - 0.001) * 256
        assert abs(x - round(x)) < 1e-6 and 0 < round(x) < 256, thr


def test_zero_bounds_return_lo_throughout_and_never_raise():
    """A bound of 0 that no probe can meet: with lo = -3 every value of [lo, hi) drops tiles at every step of this workload, so every
    probe fails, lo is kept throughout, bound_met is False exactly where the error at lo is above 0 (step 0 reads the full list: its
    error is 0 and its bound is met), and nothing raises."""
    be = C.OracleBackend()
    thresholds, trace = calibrate_error_schedule(None, C.STEPS, [0.0] * C.STEPS, backend=be, lo=-3.0)
    assert thresholds == [-3.0] * C.STEPS
    errs, _, _ = C.run_thresholds(be, thresholds)
    assert errs[0] == 0.0 and all(e > 0 for e in errs[1:]), errs
    for t, tr in enumerate(trace):
        assert tr["error"] == errs[t] and tr["bound"] == 0.0
        assert tr["bound_met"] == (errs[t] <= 0.0)


def test_zero_bounds_from_the_default_lo_keep_probed_values_that_skip_nothing():
    """From the default lo = -20 a bound of 0 CAN be met on this workload: below about -6.2 no tile is dropped, the outputs equal the
    dense ones exactly, and the bisection keeps the highest probed value with error 0 - a value that met the bound, as always."""
    be = C.OracleBackend()
    thresholds, trace = calibrate_error_schedule(None, C.STEPS, [0.0] * C.STEPS, backend=be)
    errs, skips, _ = C.run_thresholds(be, thresholds)
    assert errs == [0.0] * C.STEPS and skips == [0.0] * C.STEPS
    assert all(tr["bound_met"] and tr["error"] == 0.0 for tr in trace)
    assert all(-20.0 < thr < -3.5 for thr in thresholds), thresholds


def test_calibrator_rejects_what_it_cannot_run():
    with pytest.raises(ValueError):
        calibrate_error_schedule(None, 1, [0.1], backend=C.OracleBackend())
    with pytest.raises(ValueError):
        calibrate_error_schedule(None, 4, [0.1] * 3, backend=C.OracleBackend())
