"""CPU: per-head vote thresholds - the two entry points (la_fwd_head_thr, la_skip_list_stats_heads) as the library exports, declares,
binds and documents them, their argument checks (all before any HIP call: no device is needed), what ``mha_fwd(_thr_head=...)`` hands
to the C ABI under the stand-ins of tests/host_calls.py, the semantics of ``LiteAttention.set_head_thresholds`` and the per-head
calibrator on a stand-in backend whose error is a known monotone function of the threshold."""
import ctypes
import os
import re

import pytest
import torch

import host_calls as hc
import liteattention_amd as L
from liteattention_amd import _cabi
from liteattention_amd import calibration as cal
from liteattention_amd import flash_attn_interface as fi
from liteattention_amd import lite_attention as la_mod

E = _cabi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("la_fwd_head_thr", "la_skip_list_stats_heads")


# ---------------------------------------------------------------------------------------------------------------- entry points
def test_entry_points_are_exported_declared_bound_and_documented_under_abi_9():
    lib = _cabi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lite_attention_amd.h")).read(), flags=re.S)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in _cabi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is ctypes.c_int
        assert re.search(r"\b" + name + r"\b", integration), name
    assert lib.la_abi_version() == 9 == _cabi.LA_ABI_VERSION
    for name in ("skip_list_stats_heads", "calibrate_head_thresholds"):
        import lite_attention
        assert hasattr(L, name) and name in L.__all__ and hasattr(lite_attention, name)


def test_la_fwd_args_is_the_block_the_golden_records():
    """The table travels beside the block, not in it: sizeof(la_fwd_args) is what tests/golden/host_calls.json recorded."""
    sizes = {c["args"]["struct_size"] for rec in hc.load_golden().values() for c in rec.get("calls", []) if c["call"] == "la_fwd"}
    assert sizes == {ctypes.sizeof(_cabi.LaFwdArgs)}


def _block(lists=True):
    H, D = 2, 128
    a = _cabi.LaFwdArgs()
    a.struct_size = ctypes.sizeof(_cabi.LaFwdArgs)
    a.dtype = E.LA_DTYPE_BF16
    a.q = a.k = a.v = a.o = a.lse = 0x10000
    a.batch, a.seqlen_q, a.seqlen_k, a.num_heads, a.num_heads_k, a.head_dim, a.head_dim_v = 1, 150, 150, H, H, D, D
    a.softmax_scale = D ** -0.5
    a.block_m, a.block_n = _cabi.get_tile_sizes(D, 2, 0)
    for n in "qkvo":
        setattr(a, f"{n}_batch_stride", 150 * H * D)
        setattr(a, f"{n}_row_stride", H * D)
        setattr(a, f"{n}_head_stride", D)
    if lists:
        a.read_list, a.write_list = 0x20000, 0x30000
    return a


def test_la_fwd_head_thr_checks_need_no_device():
    lib = _cabi.load()
    call = lib.la_fwd_head_thr
    assert call(None, 0x40000, 0, 1, None) == E.LA_ERR_NULL_ARG
    assert call(None, None, 0, 1, None) == E.LA_ERR_NULL_ARG
    # a valid dense block with a table
    assert call(ctypes.byref(_block(lists=False)), 0x40000, 0, 1, None) == E.LA_ERR_LISTS
    # a valid block with lists: the table's own checks
    assert call(ctypes.byref(_block()), 0x40000, -1, 1, None) == E.LA_ERR_STRIDE
    assert call(ctypes.byref(_block()), 0x40000, 0, -1, None) == E.LA_ERR_STRIDE
    assert call(ctypes.byref(_block()), 0x40002, 0, 1, None) == E.LA_ERR_STRIDE
    # la_fwd's own checks come first, in their order and codes, whatever the table is
    a = _block()
    a.write_list = None
    assert call(ctypes.byref(a), 0x40002, -1, -1, None) == E.LA_ERR_LISTS == lib.la_fwd(ctypes.byref(a), None)
    a = _block()
    a.q_row_stride += 4
    assert call(ctypes.byref(a), 0x40002, -1, -1, None) == E.LA_ERR_STRIDE
    a = _block()
    a.q_tile_begin = 1
    assert call(ctypes.byref(a), 0x40002, -1, -1, None) == E.LA_ERR_Q_WINDOW == lib.la_fwd(ctypes.byref(a), None)
    a = _block(lists=False)
    a.block_m += 1
    assert call(ctypes.byref(a), 0x40000, 0, 1, None) == E.LA_ERR_TILE_MISMATCH
    a = _block()
    a.struct_size -= 8
    assert call(ctypes.byref(a), 0x40000, 0, 1, None) == E.LA_ERR_STRUCT_SIZE


def test_la_skip_list_stats_heads_has_the_argument_errors_of_la_skip_list_stats_ex():
    lib = _cabi.load()
    heads, ex = lib.la_skip_list_stats_heads, lib.la_skip_list_stats_ex
    for args in ((None, 4, 1, 1, 1, 1, 0x1000, None), (0x1000, 4, 1, 1, 1, 1, None, None),      # NULL
                 (0x1000, 3, 1, 1, 1, 1, 0x1000, None), (0x1000, 8, 1, 1, 1, 1, 0x1000, None),  # element size
                 (0x1000, 4, 0, 1, 1, 1, 0x1000, None), (0x1000, 4, 1, 0, 1, 1, 0x1000, None),  # sizes
                 (0x1000, 4, 1, 1, 0, 1, 0x1000, None), (0x1000, 4, 1, 1, 1, 0, 0x1000, None),
                 (0x1000, 2, 1, 1, 1, 32767, 0x1000, None),                                      # an int16 row too long for int16
                 (0x1000, 4, 1 << 15, 1 << 15, 2, 1, 0x1000, None)):                             # more than 2^31 - 1 rows
        rc = heads(*args)
        assert rc < 0 and rc == ex(*args), args
    assert heads(None, 3, 0, 0, 0, 0, None, None) == E.LA_ERR_NULL_ARG
    assert heads(0x1000, 3, 0, 0, 0, 0, 0x1000, None) == E.LA_ERR_DTYPE
    assert heads(0x1000, 2, 1, 1, 1, 40000, 0x1000, None) == E.LA_ERR_SEQLEN


# ------------------------------------------------------------------------------------------------- the host path (stand-ins)
@pytest.fixture
def table_calls(monkeypatch):
    """tests/host_calls.py's library stand-in, taught the new entry: it records the block like ``la_fwd`` plus the table."""
    def la_fwd_head_thr(self, ref, table, bs, hs, stream):
        self._calls.append({"call": "la_fwd_head_thr", "args": hc._block(ref._obj, self._owners), "stream": hc._ptr(stream) or 0,
                            "thr_head": self._owners.resolve(hc._ptr(table)), "strides": [int(bs), int(hs)]})
        return self._rc
    monkeypatch.setattr(hc._Library, "la_fwd_head_thr", la_fwd_head_thr, raising=False)


def _run(monkeypatch, kw, env=None):
    monkeypatch.setitem(hc.CASES, "_head_thr_case", (env, lambda: kw))
    return hc.run_case("_head_thr_case")


@pytest.mark.parametrize("route", ["fixed", "windows", "int16_half", "packed", "e4m3"])
def test_with_a_table_the_new_entry_gets_the_block_la_fwd_would_have_got(route, table_calls, monkeypatch):
    env = None
    if route == "fixed":
        kw = hc.with_lists(hc.qkv(hc.BF, B=2, H=4, Hk=2), must="1d")
    elif route == "windows":
        kw = hc.upd(hc.with_lists(hc.qkv(hc.BF, B=2, H=4)), _q_windows=hc.WIN2, _static_sched="after_first")
    elif route == "int16_half":
        env = {"LA_VOTE": "half"}
        with hc.environment(env):
            kw = hc.with_lists(hc.qkv(hc.FH, B=2, H=4), dtype=hc.I16)
    elif route == "packed":
        kw = hc.with_lists(hc.packed(hc.BF, H=4))
    else:
        kw = hc.with_lists(hc.descales(hc.qkv(hc.F8, B=2, H=4, Hk=2)))
    B = 2
    base = torch.zeros(B, 8, dtype=torch.float32)
    for name, table, strides in (("rows", base[:, ::2], [8, 2]), ("one_row", base[1, 4:], [0, 1])):
        plain = _run(monkeypatch, dict(kw), env)
        with_table = _run(monkeypatch, dict(kw, _thr_head=table), env)
        assert "raises" not in plain and "raises" not in with_table, (plain.get("raises"), with_table.get("raises"))
        a = [c for c in plain["calls"] if c["call"] == "la_fwd"]
        b = [c for c in with_table["calls"] if c["call"] == "la_fwd_head_thr"]
        assert a and len(a) == len(b) and not [c for c in with_table["calls"] if c["call"] == "la_fwd"]
        for x, y in zip(a, b):
            assert x["args"] == y["args"] and x["stream"] == y["stream"]
            assert y["strides"] == strides
            assert y["thr_head"] == ["_thr_head", 0]
        assert plain["allocations"] == with_table["allocations"]
        others = lambda rec: [c for c in rec["calls"] if c["call"] not in ("la_fwd", "la_fwd_head_thr")]      # noqa: E731
        assert others(plain) == others(with_table)


def test_a_wrong_table_is_a_value_error_before_any_launch(table_calls, monkeypatch):
    kw = hc.with_lists(hc.qkv(hc.BF, B=2, H=4))
    for bad in (torch.zeros(3), torch.zeros(2, 3), torch.zeros(1, 4), torch.zeros(2, 4, 1), torch.zeros(4, dtype=torch.float64),
                torch.zeros(4, device="meta"), [-1.0] * 4):
        rec = _run(monkeypatch, dict(kw, _thr_head=bad))
        assert rec["raises"][0] == "ValueError", (bad, rec.get("raises"))
        assert not [c for c in rec["calls"] if c["call"].startswith("la_fwd") and c["call"] != "la_fwd_workspace_bytes"]
    rec = _run(monkeypatch, dict(hc.qkv(hc.BF, B=2, H=4), _thr_head=torch.zeros(4)))          # a dense call has no vote
    assert rec["raises"][0] == "ValueError" and not rec["calls"]


def test_flash_attn_func_and_the_registered_op_keep_the_reference_signature():
    import inspect
    assert "_thr_head" not in inspect.signature(fi.flash_attn_func).parameters
    assert "thr_head" not in fi._FWD_SCHEMA and "float thr = -3.0" in fi._FWD_SCHEMA
    assert "_thr_head" in inspect.signature(fi.mha_fwd).parameters


# --------------------------------------------------------------------------------------------- set_head_thresholds semantics
Q1 = torch.zeros(1, 1000, 4, 128, dtype=torch.bfloat16)
Q2 = torch.zeros(1, 700, 4, 128, dtype=torch.bfloat16)
TABLE = [[-9.0, -8.0, -7.0, -6.0], [-5.0, -4.0, -3.0, -2.0], [-1.0, -0.9, -0.8, -0.7]]


class Seen:
    def __init__(self):
        self.calls = []

    def mha_fwd(self, q, k, v, **kw):
        self.calls.append(kw)
        return torch.zeros_like(q), torch.zeros(q.shape[0], q.shape[2], q.shape[1])

    def flash_attn_func(self, q, k, v, **kw):
        self.calls.append(dict(kw, _via="flash_attn_func"))
        out = torch.zeros_like(q)
        return (out, torch.zeros(q.shape[0], q.shape[2], q.shape[1])) if kw.get("return_softmax_lse") else out

    def rows(self):
        return [None if c.get("_thr_head") is None else c["_thr_head"].tolist() for c in self.calls]


@pytest.fixture
def seen(monkeypatch):
    s = Seen()
    monkeypatch.setattr(fi, "mha_fwd", s.mha_fwd)
    monkeypatch.setattr(la_mod, "flash_attn_func", s.flash_attn_func)
    monkeypatch.delenv("LITE_ATTENTION_DEBUG", raising=False)
    return s


def _f32(rows):
    return torch.tensor(rows, dtype=torch.float32).tolist()


def test_step_i_takes_row_min_i_and_a_vector_is_constant(seen):
    att = L.LiteAttention(threshold=-7.0)
    att.set_head_thresholds(TABLE)
    for i in range(5):
        assert att.current_head_thresholds().tolist() == _f32(TABLE[min(i, 2)])
        att(Q1, Q1, Q1)
    assert seen.rows() == _f32([TABLE[0], TABLE[1], TABLE[2], TABLE[2], TABLE[2]])
    assert all(c["_must_do_is_1d"] and c["attn_read_list"] is not None for c in seen.calls)
    assert [c["attn_read_list"].data_ptr() for c in seen.calls[:4]] == \
        [seen.calls[0]["attn_read_list"].data_ptr(), seen.calls[0]["attn_write_list"].data_ptr()] * 2      # the ping-pong is the scalar's
    att.set_head_thresholds(torch.tensor(TABLE[1]))
    att(Q1, Q1, Q1)
    att(Q1, Q1, Q1)
    assert seen.rows()[-2:] == _f32([TABLE[1], TABLE[1]])
    assert att.threshold == -7.0


def test_dense_calls_reset_and_shape_changes_count_as_for_a_schedule(seen):
    att = L.LiteAttention()
    att.set_head_thresholds(TABLE)
    att(Q1, Q1, Q1)
    att.enable_skip_optimization(False)
    att(Q1, Q1, Q1)
    att(Q1, Q1, Q1)
    att.enable_skip_optimization(True)
    assert att.current_head_thresholds().tolist() == _f32(TABLE[1])
    att(Q1, Q1, Q1)
    dense = [c for c in seen.calls if c.get("_via") == "flash_attn_func"]
    assert len(dense) == 2 and all(c["attn_read_list"] is None and "_thr_head" not in c for c in dense)
    att.reset_skip_state()
    att(Q1, Q1, Q1)
    att(Q2, Q2, Q2)                                                           # another sequence length: the lists are rebuilt
    att(Q2, Q2, Q2)
    sparse = [r for r in seen.rows() if r is not None]
    assert sparse == _f32([TABLE[0], TABLE[1], TABLE[0], TABLE[0], TABLE[1]])


def test_windowed_and_prepared_v_routes_pass_the_row(seen):
    att = L.LiteAttention()
    att.set_head_thresholds(TABLE)
    for _ in range(2):
        att.call_windowed(Q1, Q1, Q1, [(0, 2), (2, 2)])
    assert seen.rows() == _f32(TABLE[:2]) and all(c["_q_windows"] == [(0, 2), (2, 2)] for c in seen.calls)

    class Tiles:                                                              # what LiteAttention asks of a PreparedV
        def check_call(self, *a, **k):
            pass

        def as_v(self):
            return Q1
    att(Q1, Q1, Tiles())
    assert seen.rows()[-1] == _f32(TABLE[2]) and seen.calls[-1]["_v_prepared"] is not None
    att.set_head_thresholds(None)
    att.call_windowed(Q1, Q1, Q1, [(0, 4)])
    att(Q1, Q1, Tiles())
    assert all("_thr_head" not in c for c in seen.calls[-2:])                 # without a table: the calls of before, key for key


def test_host_values_are_checked_and_a_mismatch_of_heads_raises(seen, monkeypatch):
    att = L.LiteAttention(threshold=-4.0)
    for bad in ([-3.0, 0.0, -1.0, -1.0], [[-1.0] * 4, [-1.0, -1.0, 0.5, -1.0]], torch.tensor([1e-9, -1.0, -1.0, -1.0]),
                [float("nan"), -1.0, -1.0, -1.0], [], [[[-1.0] * 4]]):
        with pytest.raises(ValueError):
            att.set_head_thresholds(bad)
    assert att.current_head_thresholds() is None                               # a refused table changes nothing
    att.set_head_thresholds([-1.0, -2.0])                                      # two heads, the query has four
    phase = att._phase
    with pytest.raises(ValueError):
        att(Q1, Q1, Q1)
    with pytest.raises(ValueError):
        att.call_windowed(Q1, Q1, Q1, [(0, 4)])
    assert att._step == 0 and att._phase == phase and not seen.calls           # ... and no step was taken
    mine = [-1.0, -2.0, -3.0, -4.0]
    att.set_head_thresholds(mine)
    mine[0] = -100.0                                                           # host values are copied
    assert att.current_head_thresholds().tolist() == [-1.0, -2.0, -3.0, -4.0]
    monkeypatch.setenv("LITE_ATTENTION_DEBUG", "1")
    att.set_head_thresholds([0.5, -1.0, -1.0, -1.0])


def test_the_last_setter_wins(seen):
    att = L.LiteAttention(threshold=-7.0)
    att.set_head_thresholds(TABLE)
    att(Q1, Q1, Q1)
    att.set_threshold(-4.0)
    assert att.current_head_thresholds() is None and att._head_thresholds is None
    att(Q1, Q1, Q1)
    assert seen.calls[-1]["_via"] == "flash_attn_func" and seen.calls[-1]["thr"] == -4.0
    att.set_head_thresholds(TABLE)
    att.set_threshold_schedule([-3.0, -2.0])
    assert att.current_head_thresholds() is None
    att(Q1, Q1, Q1)
    assert seen.calls[-1]["_via"] == "flash_attn_func" and seen.calls[-1]["thr"] == -2.0      # the third call that used the lists
    att.set_threshold_schedule([-3.0, -2.0])
    att.set_head_thresholds(TABLE[0])
    att(Q1, Q1, Q1)
    assert seen.rows()[-1] == _f32(TABLE[0])
    att.set_head_thresholds(None)
    att(Q1, Q1, Q1)
    assert seen.calls[-1]["_via"] == "flash_attn_func"


def test_state_dict_round_trip_and_the_dict_without_a_table(seen):
    att = L.LiteAttention(threshold=-7.0)
    keys_before = set(att.state_dict())
    assert keys_before == {"skip_list", "phase", "threshold", "enable_skipping", "max_batch_size", "shape_key", "device", "tile_sizes",
                           "list_dtype", "threshold_schedule", "step"}                     # the parent's keys, key for key
    att.set_head_thresholds(TABLE)
    att(Q1, Q1, Q1)
    att(Q1, Q1, Q1)
    state = att.state_dict()
    assert set(state) == keys_before | {"head_thresholds"} and state["head_thresholds"] == _f32(TABLE) and state["step"] == 2
    other = L.LiteAttention()
    other.load_state_dict(state, device="cpu")
    assert other.current_head_thresholds().tolist() == _f32(TABLE[2]) and torch.equal(other._skip_list, att._skip_list)
    other(Q1, Q1, Q1)
    assert seen.rows()[-1] == _f32(TABLE[2])
    att.set_head_thresholds(None)
    assert set(att.state_dict()) == keys_before
    other.load_state_dict(att.state_dict(), device="cpu")                      # a state without a table removes the one set
    assert other.current_head_thresholds() is None


def test_forwarders_hand_the_table_on(seen):
    from liteattention_amd.parallel import HeadShardedLiteAttention
    sp = L.SeqParallelLiteAttention(3)
    sp.set_head_thresholds(TABLE)
    assert all(la._head_thresholds.tolist() == _f32(TABLE) for la in sp.lite_attention)
    sp.set_threshold(-2.0)
    assert all(la._head_thresholds is None for la in sp.lite_attention)
    hs = HeadShardedLiteAttention(4)                                           # one rank: the whole table
    hs.set_head_thresholds(TABLE)
    assert hs.local._head_thresholds.tolist() == _f32(TABLE)
    hs.h0, hs.h1 = 1, 3                                                        # the slice a second rank of two would own
    hs.set_head_thresholds(TABLE)
    assert hs.local._head_thresholds.tolist() == _f32([r[1:3] for r in TABLE])
    hs.set_head_thresholds(TABLE[0])
    assert hs.local._head_thresholds.tolist() == _f32(TABLE[0][1:3])
    with pytest.raises(ValueError):
        hs.set_head_thresholds([-1.0, -2.0])
    hs.set_head_thresholds(None)
    assert hs.local._head_thresholds is None


# ------------------------------------------------------------------------------------------------ calibrator on a stand-in
class MonotoneBackend:
    """Per-head error of step t + 1 = 1 where the threshold head h ran step t with is above T[t][h], else 0 (monotone, a different
    crossing per head and step); step 0's own output is exact. Only the protocol of the calibrators, no attention."""
    H = 5

    def __init__(self, crossings):
        self.T = torch.tensor(crossings, dtype=torch.float64)      # (n_steps - 1, H)
        self.reset()

    def reset(self):
        self.prev, self.t_prev = None, -1

    def snapshot(self):
        return self.prev, self.t_prev

    def restore(self, snap):
        self.prev, self.t_prev = snap

    def step(self, t, thr):
        thr = thr.double() if isinstance(thr, torch.Tensor) else torch.full((self.H,), float(thr), dtype=torch.float64)
        err = torch.zeros(self.H, dtype=torch.float64)
        if self.prev is not None and self.t_prev == t - 1 and t - 1 < self.T.shape[0]:
            err = (self.prev > self.T[t - 1]).double()
        self.prev, self.t_prev = thr.clone(), t
        return err.view(1, 1, self.H, 1)                             # "the output": its error against dense (zeros)

    def dense(self, t):
        return torch.zeros(1, 1, self.H, 1, dtype=torch.float64)

    def error_heads(self, out, ref):
        return (out - ref).abs().amax(dim=(0, 1, 3))

    def error(self, out, ref):
        return float(self.error_heads(out, ref).max())

    def skip_fraction(self):
        return 0.0


def _grid_best(lo, hi, iters, crossing):
    """The largest point lo + j (hi - lo) / 2^iters, 0 < j < 2^iters, reachable by the bisection, that is <= crossing; else lo."""
    a, b, best = lo, hi, lo
    for _ in range(iters):
        mid = 0.5 * (a + b)
        if mid <= crossing:
            best = a = mid
        else:
            b = mid
    return best


@pytest.mark.parametrize("lo,hi,iters", [(-20.0, -1e-3, 8), (-16.0, -1.0, 5)])
def test_table_is_the_largest_grid_point_that_meets_the_bound_per_head(lo, hi, iters):
    crossings = [[-3.3, -7.9, -0.5, -15.99, -25.0], [-12.1, -1.01, -6.0, -2.5, -0.0001], [-4.0, -4.0, -15.5, -9.25, -8.0]]
    n = len(crossings) + 1
    be = MonotoneBackend(crossings)
    table, trace = cal.calibrate_head_thresholds(None, n, [0.5] * n, lo=lo, hi=hi, iters=iters, backend=be)
    assert table.dtype == torch.float32 and tuple(table.shape) == (n, be.H) and len(trace) == n
    for t in range(n - 1):
        for h in range(be.H):
            want = _grid_best(lo, hi, iters, crossings[t][h])
            assert table[t, h].item() == torch.tensor(want, dtype=torch.float32).item(), (t, h)
            j = (want - lo) / (hi - lo) * 2 ** iters
            assert abs(j - round(j)) < 1e-9 and 0 <= round(j) < 2 ** iters     # ... a point of the dyadic grid (j in fp64 rounding)
    assert torch.equal(table[-1], table[-2])
    for t in range(n):
        assert torch.equal(trace[t]["threshold"], table[t]) and tuple(trace[t]["error"].shape) == (be.H,)
        assert bool(trace[t]["bound_met"].all()) == bool((trace[t]["error"] <= 0.5).all())
    # a head whose crossing lies below lo keeps lo and misses its bound at the next step
    assert table[0, 4].item() == lo and not bool(trace[1]["bound_met"][4]) and bool(trace[1]["bound_met"][:4].all())
    # bounds per (step, head): a head with a bound nothing misses runs at the top of the grid
    loose = torch.full((n, be.H), 0.5)
    loose[:, 2] = 2.0
    table2, _ = cal.calibrate_head_thresholds(None, n, loose, lo=lo, hi=hi, iters=iters, backend=MonotoneBackend(crossings))
    top = torch.tensor(lo + (hi - lo) * (1 - 2.0 ** -iters), dtype=torch.float32)
    assert bool((table2[:, 2] == top).all()) and torch.equal(table2[:, [0, 1, 3, 4]], table[:, [0, 1, 3, 4]])
    # the scalar calibrator on the same backend, equal bounds: the minimum over the heads
    sched, _ = cal.calibrate_error_schedule(None, n, [0.5] * n, lo=lo, hi=hi, iters=iters, backend=MonotoneBackend(crossings))
    assert torch.tensor(sched, dtype=torch.float32).tolist() == table.min(dim=1).values.tolist()


def test_head_calibrator_rejects_what_it_cannot_run():
    be = MonotoneBackend([[-1.0] * 5])
    with pytest.raises(ValueError):
        cal.calibrate_head_thresholds(None, 1, [0.5], backend=be)
    with pytest.raises(ValueError):
        cal.calibrate_head_thresholds(None, 2, [0.5, 0.5], lo=-1.0, hi=-2.0, backend=be)
    with pytest.raises(ValueError):
        cal.calibrate_head_thresholds(None, 2, [0.5, 0.5, 0.5], backend=be)
    with pytest.raises(ValueError):
        cal.calibrate_head_thresholds(None, 2, torch.zeros(2, 4), backend=be)
