"""CPU recorder of what the Python host path (liteattention_amd/flash_attn_interface.py) hands to the C ABI.

``run_case(name)`` runs one named call of ``mha_fwd`` (or of a combine function) on CPU tensors under four stand-ins and returns a
JSON-able record of it: the library calls in order with every non-zero field of their argument blocks (pointers resolved to
``[owner, byte offset]``), the ``torch.empty`` allocations, the returned tensors and the exception, if any. Nothing is computed and no
device is needed: ``la_get_tile_sizes_ex`` and ``la_fwd_workspace_bytes`` are host code and run for real.

The stand-ins (all undone when the call is over):
  * ``torch.Tensor.is_cuda`` -> True;
  * ``_cabi.load()`` -> the real library, except that ``la_fwd`` / ``la_combine`` / ``la_combine_list`` record and return a chosen
    code (LA_OK), and ``la_fwd_workspace_bytes`` records and passes through;
  * ``torch.cuda.device`` -> a null context, ``torch.cuda.current_stream`` -> stream 0;
  * ``_cabi.device_slots`` -> (256, 1).

``python tests/host_calls.py --write`` regenerates tests/golden/host_calls.json (tests/test_host_calls_cpu.py compares against it);
``python tests/host_calls.py --time`` prints the host time per call of three calls under the stand-ins, and ``--time-against FILE``
times them against another copy of flash_attn_interface.py in the same process (profiles/host_path.md)."""
import contextlib
import ctypes
import json
import os
import statistics
import sys
import time
import types

import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from liteattention_amd import _cabi  # noqa: E402
from liteattention_amd import flash_attn_interface as fai  # noqa: E402
from liteattention_amd import skip_lists as sl  # noqa: E402

GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "host_calls.json")
ENV_SWITCHES = ("LA_FWD_KERNEL", "LA_VOTE", "LA_SCHED", "LA_RESCALE_TAU", "LA_FP8_P")      # what _cabi.default_flags() reads
BF, FH, F8 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
I32, I16 = torch.int32, torch.int16
EX, ROWSUM, ENC = _cabi.LA_FLAG_EXACT_RESCALE, _cabi.LA_FLAG_FP8_MFMA_ROWSUM, _cabi.LA_FLAG_FP8_ENCODED_P


# ---- the stand-ins ------------------------------------------------------------------------------------------------------------------
class _Owners:
    """Who owns an address: the caller's tensors by argument name, then ``alloc<i>`` = the i-th ``torch.empty`` of the call, then
    ``tmp<i>`` = another tensor the host path made (a padded copy, a replicated q, ...), numbered in the order in which the record
    first refers to them - so neither the names nor the number of torch's internal ops are part of the record. Everything is kept
    alive until the record is complete, so no address is used twice."""

    def __init__(self, named):
        self.entries = [(name, t) for name, t in named if t.untyped_storage().nbytes() > 0]
        self.storages = {t.untyped_storage().data_ptr() for _, t in self.entries}
        self.allocs, self.tmp_names = 0, {}

    def add_alloc(self, t):
        self.allocs += 1
        self._add(f"alloc{self.allocs - 1}", t)

    def add_tmp(self, t):
        if t.untyped_storage().nbytes() > 0 and t.untyped_storage().data_ptr() not in self.storages:
            self._add("tmp", t)

    def _add(self, name, t):
        if t.untyped_storage().nbytes() > 0:
            self.entries.append((name, t))
            self.storages.add(t.untyped_storage().data_ptr())

    def resolve(self, ptr):
        if not ptr:
            return None
        best = None
        for rank, (name, t) in enumerate(self.entries):
            s = t.untyped_storage()
            if s.data_ptr() <= ptr < s.data_ptr() + s.nbytes() and t.data_ptr() <= ptr:
                kind = 0 if not name.startswith(("alloc", "tmp")) else 1
                key = (kind, -t.data_ptr(), rank)      # the caller's tensors first; of several views of one storage the nearest below
                if best is None or key < best[0]:
                    best = (key, name, ptr - t.data_ptr())
        if best is None:
            return ["unknown", 0]
        _, name, offset = best
        if name == "tmp":
            name = self.tmp_names.setdefault(best[0][2], f"tmp{len(self.tmp_names)}")
        return [name, offset]


class _TrackNewTensors(TorchDispatchMode):
    def __init__(self, owners):
        super().__init__()
        self.owners = owners

    def __torch_dispatch__(self, func, types_, args=(), kwargs=None):
        res = func(*args, **(kwargs or {}))
        if func.overloadpacket.__name__ != "empty":               # torch.empty is counted by its own patch
            for t in (res if isinstance(res, (tuple, list)) else (res,)):
                if isinstance(t, torch.Tensor):
                    self.owners.add_tmp(t)
        return res


def _block(a, owners):
    """Every non-zero field of a LaFwdArgs."""
    d = {}
    for name, ctype in _cabi.LaFwdArgs._fields_:
        val = getattr(a, name)
        if not val:
            continue
        if ctype is ctypes.c_void_p:
            d[name] = owners.resolve(val)
        elif ctype is ctypes.c_float:
            d[name] = float(val).hex()
        else:
            d[name] = int(val)
    return d


def _ptr(x):
    return x.value if isinstance(x, ctypes.c_void_p) else x


class _Library:
    """The real library, but for the calls that would launch a kernel."""

    def __init__(self, real, calls, owners, rc, ws):
        self._real, self._calls, self._owners, self._rc, self._ws = real, calls, owners, rc, ws

    def __getattr__(self, name):
        return getattr(self._real, name)

    def la_fwd_workspace_bytes(self, ref):
        need = self._real.la_fwd_workspace_bytes(ref)
        if self._ws is not None:                                  # a case that asks how a route words the library's refusal
            need = self._ws
        if self._calls is not None:
            self._calls.append({"call": "la_fwd_workspace_bytes", "args": _block(ref._obj, self._owners), "returns": int(need)})
        return need

    def la_fwd(self, ref, stream):
        if self._calls is not None:
            self._calls.append({"call": "la_fwd", "args": _block(ref._obj, self._owners), "stream": _ptr(stream) or 0})
        return self._rc

    def la_combine(self, o_part, is16, lse_part, out, o_dtype, lse, ns, B, S, H, D, stream):
        if self._calls is not None:
            r = self._owners.resolve
            self._calls.append({"call": "la_combine", "o_partial": r(_ptr(o_part)), "partial_is_16bit": is16, "lse_partial": r(_ptr(lse_part)),
                                "o": r(_ptr(out)), "o_dtype": o_dtype, "lse": r(_ptr(lse)), "dims": [ns, B, S, H, D], "stream": _ptr(stream) or 0})
        return _cabi.LA_OK

    def la_combine_list(self, o_ptrs, is16, l_ptrs, out, o_dtype, lse, n, B, S, H, D, stream):
        if self._calls is not None:
            r = self._owners.resolve
            self._calls.append({"call": "la_combine_list", "o_partials": [r(o_ptrs[i]) for i in range(n)], "partial_is_16bit": is16,
                                "lse_partials": [r(l_ptrs[i]) for i in range(n)], "o": r(_ptr(out)), "o_dtype": o_dtype,
                                "lse": r(_ptr(lse)), "dims": [n, B, S, H, D], "stream": _ptr(stream) or 0})
        return _cabi.LA_OK


@contextlib.contextmanager
def stand_ins(named=(), calls=None, allocs=None, rc=_cabi.LA_OK, cuda=True, ws=None):
    """The four stand-ins. With ``calls`` / ``allocs`` lists the library calls and the ``torch.empty`` allocations are recorded into them
    (and every new tensor is tracked, so that pointers resolve); without, nothing but the stand-ins is in the way (timing)."""
    real = _cabi.load()
    record = calls is not None
    owners = _Owners(named) if record else None
    lib = _Library(real, calls, owners, rc, ws)
    saved = (_cabi.load, _cabi.device_slots, torch.cuda.device, torch.cuda.current_stream, torch.empty)
    real_empty = torch.empty

    def empty(*args, **kwargs):
        t = real_empty(*args, **kwargs)
        allocs.append([list(t.shape), str(t.dtype).replace("torch.", "")])
        owners.add_alloc(t)
        return t

    try:
        _cabi.load = lambda: lib
        _cabi.device_slots = lambda head_dim, element_size, flags=None: (256, 1)
        torch.cuda.device = lambda device: contextlib.nullcontext()
        torch.cuda.current_stream = lambda device=None: types.SimpleNamespace(cuda_stream=0)
        if cuda:
            torch.Tensor.is_cuda = property(lambda self: True)
        if record:
            torch.empty = empty
            with _TrackNewTensors(owners):
                yield owners
        else:
            yield None
    finally:
        _cabi.load, _cabi.device_slots, torch.cuda.device, torch.cuda.current_stream, torch.empty = saved
        if cuda:
            del torch.Tensor.is_cuda


@contextlib.contextmanager
def environment(env):
    """The switches of ``_cabi.default_flags()`` set to exactly ``env`` (a case is recorded the same whatever the caller's shell has)."""
    saved = {k: os.environ.pop(k, None) for k in ENV_SWITCHES}
    os.environ.update(env or {})
    try:
        yield
    finally:
        for k in ENV_SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _t(shape, dtype):
    if dtype == F8:
        return torch.zeros(shape, dtype=torch.uint8).view(F8)
    return torch.zeros(shape, dtype=dtype)


def qkv(dtype, B=1, Sq=300, Sk=520, H=2, Hk=None, D=128):
    Hk = Hk or H
    return dict(q=_t((B, Sq, H, D), dtype), k=_t((B, Sk, Hk, D), dtype), v=_t((B, Sk, Hk, D), dtype))


def descales(kw, B=None, names="qkv", shape=None, dtype=torch.float32):
    Bq, Hk = (kw["cu_seqlens_q"].numel() - 1 if "cu_seqlens_q" in kw else kw["q"].shape[0]), kw["k"].shape[-2]
    for n in names:
        kw[f"{n}_descale"] = torch.ones(shape or (B or Bq, Hk), dtype=dtype)
    return kw


def with_lists(kw, dtype=I32, batch=None, must=None, write=True):
    """Read / write lists of the project's own initialiser for this call's tiles; ``must``: None, "4d" or "1d"."""
    q = kw["q"]
    if "cu_seqlens_q" in kw:
        B, H, Sq, Sk = kw["cu_seqlens_q"].numel() - 1, q.shape[1], kw["max_seqlen_q"], kw["max_seqlen_k"]
    else:
        B, Sq, H, Sk = q.shape[0], q.shape[1], q.shape[2], kw["k"].shape[1]
    bm, bn = fai.get_tile_sizes(q.shape[-1], q.element_size())
    qt, kt = -(-Sq // bm), -(-Sk // bn)
    lists = sl.new_skip_lists(batch or B, H, qt, kt, "cpu", list_dtype=dtype)
    kw["attn_read_list"] = lists[0]
    if write:
        kw["attn_write_list"] = lists[1]
    if must == "4d":
        kw["attn_must_do_list"] = sl.new_skip_lists(batch or B, H, qt, kt, "cpu")[0]
    if must == "1d":
        kw["attn_must_do_list"] = sl.must_do_row([0, 0], bn, kt + 1, "cpu")
        kw["_must_do_is_1d"] = True
    return kw


def sliced(kw, pad_heads=1, pad_dim=32):
    """q / k / v as slices of wider tensors: head and row strides not packed, last dimension contiguous."""
    for n in "qkv":
        t = kw[n]
        B, S, H, D = t.shape
        kw[n] = _t((B, S, H + pad_heads, D + pad_dim), t.dtype)[:, :, :H, :D]
    return kw


def with_out(kw, dtype=None, strided=False, shape=None, D=None):
    q = kw["q"]
    dtype = dtype or (BF if q.dtype == F8 else q.dtype)
    shape = list(shape or q.shape)
    if strided:
        kw["out"] = _t(shape[:-2] + [shape[-2] + 1, shape[-1]], dtype)[..., :shape[-2], :]
    else:
        kw["out"] = _t(shape, dtype)
    return kw


def packed(dtype, seq_q=(100, 37), seq_k=(130, 200), H=2, Hk=None, D=128):
    Hk = Hk or H
    cu = lambda seqs: torch.tensor([sum(seqs[:i]) for i in range(len(seqs) + 1)], dtype=I32)      # noqa: E731
    return dict(q=_t((sum(seq_q), H, D), dtype), k=_t((sum(seq_k), Hk, D), dtype), v=_t((sum(seq_k), Hk, D), dtype),
                cu_seqlens_q=cu(seq_q), cu_seqlens_k=cu(seq_k), max_seqlen_q=max(seq_q), max_seqlen_k=max(seq_k))


def upd(kw, **more):
    kw.update(more)
    return kw


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
CASES = {}      # name -> (env, builder); a builder returns the kwargs of mha_fwd, or a dict with "kw" and options (see run_case)


def case(name, builder, env=None):
    assert name not in CASES, name
    CASES[name] = (env, builder)


WIN2 = [(0, 1), (1, 1)]      # two windows over the two 256-row q-tiles of Sq = 300

# fixed-length route: dtypes and head dims
case("fixed_bf16_d128", lambda: qkv(BF))
case("fixed_fp16_d64", lambda: qkv(FH, D=64))
case("fixed_e4m3_d128_descales", lambda: descales(qkv(F8, B=2, H=4, Hk=2)))
case("fixed_e4m3_d192", lambda: qkv(F8, D=192))
case("fixed_e4m3_d128_q_descale_only", lambda: descales(qkv(F8), names="q"))
# GQA, batch 2
case("fixed_bf16_gqa_b2", lambda: qkv(BF, B=2, H=4, Hk=2))
# layouts
case("fixed_bf16_sliced", lambda: sliced(qkv(BF, B=2)))
case("fixed_e4m3_sliced", lambda: sliced(qkv(F8, B=2)))
case("fixed_bf16_out", lambda: with_out(qkv(BF)))
case("fixed_bf16_out_head_strided", lambda: with_out(qkv(BF, B=2), strided=True))
case("fixed_bf16_scale_given", lambda: upd(qkv(BF), softmax_scale=0.125))
# padded head dim 80 -> 96
for _n, _dt in (("bf16", BF), ("e4m3", F8)):
    case(f"fixed_{_n}_d80", lambda dt=_dt: qkv(dt, D=80))
    case(f"fixed_{_n}_d80_out", lambda dt=_dt: with_out(qkv(dt, D=80)))
    case(f"fixed_{_n}_d80_out_strided", lambda dt=_dt: with_out(qkv(dt, D=80), strided=True))
case("fixed_bf16_d80_windows_hook", lambda: dict(kw=upd(qkv(BF, D=80), _q_windows=WIN2), hook=True))
case("fixed_e4m3_d80_windows_hook_out", lambda: dict(kw=upd(with_out(qkv(F8, D=80)), _q_windows=WIN2, _static_sched="after_first"), hook=True))
case("fixed_bf16_d80_lists", lambda: with_lists(qkv(BF, D=80), must="1d"))
case("fixed_bf16_d80_scale_given", lambda: upd(qkv(BF, D=80), softmax_scale=0.25))
# lists
case("fixed_bf16_lists_int32", lambda: with_lists(qkv(BF)))
case("fixed_bf16_lists_int16", lambda: with_lists(qkv(BF), dtype=I16))
case("fixed_bf16_lists_must4d", lambda: with_lists(qkv(BF), must="4d"))
case("fixed_bf16_lists_must1d", lambda: with_lists(qkv(BF), must="1d"))
case("fixed_bf16_lists_int16_must1d", lambda: with_lists(qkv(BF), dtype=I16, must="1d"))
case("fixed_bf16_lists_batch_larger", lambda: with_lists(qkv(BF), batch=3, must="4d"))
case("fixed_bf16_lists_thr", lambda: upd(with_lists(qkv(BF)), thr=-7.5))
case("fixed_e4m3_lists_must1d", lambda: with_lists(descales(qkv(F8)), must="1d"))
case("fixed_fp16_d64_lists_gqa", lambda: with_lists(qkv(FH, B=2, H=4, Hk=2, D=64), dtype=I16))
case("fixed_bf16_read_list_only", lambda: with_lists(qkv(BF), write=False))
case("fixed_bf16_must1d_without_lists", lambda: upd(qkv(BF), attn_must_do_list=torch.tensor([2, 0, 0], dtype=I32), _must_do_is_1d=True))
# windows
for _n, _dt in (("bf16", BF), ("e4m3", F8)):
    for _s in (False, True, "after_first"):
        case(f"fixed_{_n}_windows_static_{_s}", lambda dt=_dt, s=_s: dict(kw=upd(qkv(dt), _q_windows=WIN2, _static_sched=s), hook=True))
case("fixed_bf16_windows_lists", lambda: upd(with_lists(qkv(BF), must="1d"), _q_windows=WIN2))
case("fixed_bf16_static_no_windows", lambda: upd(qkv(BF), _static_sched=True))
case("fixed_bf16_static_after_first_no_windows", lambda: upd(qkv(BF), _static_sched="after_first"))
# extra flags
for _n, _f in (("exact_rescale", EX), ("mfma_rowsum", ROWSUM), ("encoded_p", ENC)):
    case(f"fixed_e4m3_flags_{_n}", lambda f=_f: upd(qkv(F8), _flags=f))
    case(f"fixed_bf16_flags_{_n}", lambda f=_f: upd(qkv(BF), _flags=f))
case("fixed_e4m3_scope_nested", lambda: dict(kw=qkv(F8), scope=[(EX | ENC, 0), (ROWSUM, ENC)]))
case("fixed_e4m3_scope_nested_reset", lambda: dict(kw=qkv(F8), scope=[(0, ENC | ROWSUM), (ENC, 0)]))
case("fixed_e4m3_flag_inside_clearing_scope", lambda: dict(kw=upd(qkv(F8), _flags=ENC), scope=[(0, ENC | ROWSUM)]))
case("fixed_e4m3_env_encoded_scope_clears", lambda: dict(kw=qkv(F8), scope=[(0, ENC | ROWSUM)]), env={"LA_FP8_P": "encoded"})
case("fixed_bf16_d80_scope", lambda: dict(kw=upd(qkv(BF, D=80), _flags=EX), scope=[(ROWSUM, EX)]))
# environment defaults
case("env_v2_bf16", lambda: qkv(BF), env={"LA_FWD_KERNEL": "v2"})
case("env_v2_bf16_lists", lambda: with_lists(qkv(BF), must="1d"), env={"LA_FWD_KERNEL": "v2"})
case("env_v2_bf16_d80", lambda: qkv(BF, D=80), env={"LA_FWD_KERNEL": "v2"})
case("env_v2_e4m3", lambda: qkv(F8), env={"LA_FWD_KERNEL": "v2"})
case("env_half_vote_lists_window", lambda: upd(with_lists(qkv(BF), must="1d"), _q_windows=[(0, 2), (2, 1)]), env={"LA_VOTE": "half"})
case("env_half_vote_split", lambda: upd(qkv(BF, Sk=4096), num_splits=-1), env={"LA_VOTE": "half"})
case("env_static_sched_bf16", lambda: qkv(BF), env={"LA_SCHED": "static"})
case("env_exact_rescale_bf16", lambda: qkv(BF), env={"LA_RESCALE_TAU": "0"})
for _p in ("reference", "mfma_rowsum", "encoded"):
    case(f"env_fp8_p_{_p}_e4m3", lambda: qkv(F8), env={"LA_FP8_P": _p})
    case(f"env_fp8_p_{_p}_bf16", lambda: qkv(BF), env={"LA_FP8_P": _p})
    case(f"env_fp8_p_{_p}_e4m3_split", lambda: upd(qkv(F8, Sk=800), num_splits=3), env={"LA_FP8_P": _p})
    case(f"env_fp8_p_{_p}_e4m3_packed", lambda: packed(F8), env={"LA_FP8_P": _p})

# split-KV route
case("split_e4m3_n3_exact", lambda: upd(qkv(F8, Sk=768), num_splits=3))
case("split_e4m3_n3_ragged", lambda: upd(qkv(F8, Sk=800), num_splits=3))
case("split_e4m3_auto", lambda: upd(qkv(F8, Sk=4096), num_splits=-1))
case("split_e4m3_descales", lambda: upd(descales(qkv(F8, Sk=800, H=4, Hk=2)), num_splits=3))
case("split_bf16_n3", lambda: upd(qkv(BF, Sk=800), num_splits=3))
case("split_bf16_auto", lambda: upd(qkv(BF, Sk=4096), num_splits=-1))
case("split_fp16_d64_sliced", lambda: upd(sliced(qkv(FH, Sk=800, D=64)), num_splits=3))
case("split_bf16_descale_raises", lambda: upd(descales(qkv(BF, Sk=800), names="k"), num_splits=3))
case("split_bf16_out", lambda: upd(with_out(qkv(BF, Sk=800)), num_splits=3))
case("split_bf16_out_strided", lambda: upd(with_out(qkv(BF, Sk=800), strided=True), num_splits=3))
case("split_bf16_out_wrong_dtype", lambda: upd(with_out(qkv(BF, Sk=800), dtype=FH), num_splits=3))
case("split_bf16_b2_packed_rows", lambda: upd(qkv(BF, B=2, Sk=800), num_splits=3))
case("split_bf16_b2_packed_rows_out", lambda: upd(with_out(qkv(BF, B=2, Sk=800)), num_splits=3))
case("split_e4m3_b2_packed_rows_descales", lambda: upd(descales(qkv(F8, B=2, Sk=800)), num_splits=3))
case("split_bf16_b2_padded_k_batch_stride",
     lambda: (lambda kw: upd(kw, k=_t((2, 808, 2, 128), BF)[:, :800], num_splits=3))(qkv(BF, B=2, Sk=800)))
case("split_bf16_d80", lambda: upd(qkv(BF, Sk=800, D=80), num_splits=3))
case("split_e4m3_d80_descales", lambda: upd(descales(qkv(F8, Sk=800, D=80)), num_splits=3))
case("split_short_keys_n1", lambda: upd(qkv(BF, Sk=64), num_splits=3))
case("split_auto_short_keys", lambda: upd(qkv(BF, Sk=520), num_splits=-1))
case("split_scope_flags_e4m3", lambda: dict(kw=upd(qkv(F8, Sk=800), num_splits=3), scope=[(EX | ENC, ROWSUM)]))
case("split_scope_flags_bf16", lambda: dict(kw=upd(qkv(BF, Sk=800), num_splits=3, _flags=EX, _static_sched=True), scope=[(ENC, 0)]))
case("split_bf16_env_v2", lambda: upd(qkv(BF, Sk=800), num_splits=3), env={"LA_FWD_KERNEL": "v2"})
case("split_n2_with_lists_raises", lambda: upd(with_lists(qkv(BF)), num_splits=2))
case("split_n2_with_windows_raises", lambda: upd(qkv(BF), num_splits=2, _q_windows=WIN2))
case("split_n2_with_cu_raises", lambda: upd(packed(BF), num_splits=2))
case("split_auto_with_lists_is_unsplit", lambda: upd(with_lists(qkv(BF, Sk=4096)), num_splits=-1))

# packed (cu_seqlens) route
case("packed_bf16", lambda: packed(BF))
case("packed_fp16_d64_gqa", lambda: packed(FH, H=4, Hk=2, D=64))
case("packed_e4m3", lambda: packed(F8))
case("packed_e4m3_descales", lambda: descales(packed(F8, H=4, Hk=2)))
case("packed_bf16_sliced", lambda: (lambda kw: upd(kw, q=_t((137, 3, 160), BF)[:, :2, :128], k=_t((330, 3, 160), BF)[:, :2, :128]))(packed(BF)))
case("packed_bf16_lists_int32", lambda: with_lists(packed(BF)))
case("packed_bf16_lists_int16", lambda: with_lists(packed(BF), dtype=I16))
case("packed_bf16_lists_must1d", lambda: upd(with_lists(packed(BF), must="1d"), thr=-5.0))
case("packed_bf16_lists_must4d", lambda: with_lists(packed(BF), must="4d", batch=3))
case("packed_e4m3_lists", lambda: with_lists(packed(F8), must="1d"))
case("packed_bf16_must1d_without_lists", lambda: upd(packed(BF), attn_must_do_list=torch.tensor([2, 0, 0], dtype=I32), _must_do_is_1d=True))
case("packed_bf16_d80", lambda: packed(BF, D=80))
case("packed_e4m3_d80_descales", lambda: descales(packed(F8, D=80)))
case("packed_bf16_d80_lists", lambda: with_lists(packed(BF, D=80)))
case("packed_bf16_out", lambda: with_out(packed(BF)))
case("packed_e4m3_out_strided", lambda: with_out(packed(F8), strided=True))
case("packed_bf16_d80_out", lambda: with_out(packed(BF, D=80)))
case("packed_bf16_scale_given", lambda: upd(packed(BF), softmax_scale=0.5))
case("packed_scope_flags_e4m3", lambda: dict(kw=packed(F8), scope=[(EX | ENC, ROWSUM)]))
case("packed_scope_flags_bf16", lambda: dict(kw=upd(packed(BF), _flags=EX), scope=[(ENC, 0)]))
case("packed_bf16_env_v2_static", lambda: packed(BF), env={"LA_FWD_KERNEL": "v2", "LA_SCHED": "static", "LA_RESCALE_TAU": "0"})
case("packed_e4m3_env_v2_static", lambda: packed(F8), env={"LA_FWD_KERNEL": "v2", "LA_SCHED": "static", "LA_RESCALE_TAU": "0"})
case("packed_empty_q", lambda: packed(BF, seq_q=(0, 0)))
case("packed_empty_q_out", lambda: with_out(packed(BF, seq_q=(0, 0))))
case("packed_max_seqlen_q_zero", lambda: upd(packed(BF), max_seqlen_q=0))
case("packed_empty_k", lambda: packed(BF, seq_k=(0, 0)))
case("packed_e4m3_empty_k", lambda: packed(F8, seq_k=(0, 0)))
case("packed_negative_max_seqlen_k", lambda: upd(packed(BF), max_seqlen_k=-1))

# what the library answers: each route's translation of a return code
for _rc_name, _rc in (("unsupported", _cabi.LA_ERR_UNSUPPORTED), ("launch", _cabi.LA_ERR_LAUNCH), ("seqlen", _cabi.LA_ERR_SEQLEN)):
    case(f"rc_{_rc_name}_fixed", lambda rc=_rc: dict(kw=qkv(BF), rc=rc))
    case(f"rc_{_rc_name}_split", lambda rc=_rc: dict(kw=upd(qkv(BF, Sk=800), num_splits=3), rc=rc))
    case(f"rc_{_rc_name}_packed", lambda rc=_rc: dict(kw=packed(BF), rc=rc))
case("rc_launch_fixed_second_window", lambda: dict(kw=upd(qkv(BF), _q_windows=WIN2), rc=_cabi.LA_ERR_LAUNCH, hook=True))
case("workspace_refused_fixed_e4m3_batch0", lambda: qkv(F8, B=0))
case("workspace_refused_fixed", lambda: dict(kw=qkv(BF), ws=_cabi.LA_ERR_SEQLEN))
case("workspace_refused_split", lambda: dict(kw=upd(qkv(F8, Sk=800), num_splits=3), ws=_cabi.LA_ERR_SEQLEN))
case("workspace_refused_packed", lambda: dict(kw=packed(F8), ws=_cabi.LA_ERR_SEQLEN))
case("workspace_refused_packed_lists", lambda: dict(kw=with_lists(packed(BF)), ws=_cabi.LA_ERR_SHAPE))

# refused calls, fixed-length route (one fault per call)
case("refuse_flags_geometry_bit", lambda: upd(qkv(BF), _flags=_cabi.LA_FLAG_KERNEL_128ROW))
case("refuse_flags_static_sched_bit", lambda: dict(kw=upd(qkv(BF), _flags=_cabi.LA_FLAG_STATIC_SCHED), scope=[(EX, 0)]))
case("refuse_cpu_tensor", lambda: dict(kw=qkv(BF), cuda=False))
case("refuse_dtype_fp32", lambda: qkv(torch.float32))
case("refuse_dtype_q_k_differ", lambda: upd(qkv(BF), k=_t((1, 520, 2, 128), FH)))
case("refuse_dtype_q_v_differ", lambda: upd(qkv(BF), v=_t((1, 520, 2, 128), FH)))
for _name in ("k_new", "v_new", "q_v", "cu_seqlens_k_new", "seqused_q", "seqused_k", "page_table", "kv_batch_idx", "leftpad_k",
              "rotary_cos", "rotary_sin", "seqlens_rotary", "scheduler_metadata"):
    case(f"refuse_arg_{_name}", lambda n=_name: upd(qkv(BF), **{n: torch.zeros(1, dtype=I32)}))
case("refuse_causal", lambda: upd(qkv(BF), is_causal=True))
case("refuse_window_left", lambda: upd(qkv(BF), window_size_left=0))
case("refuse_window_right", lambda: upd(qkv(BF), window_size_right=16))
case("refuse_attention_chunk", lambda: upd(qkv(BF), attention_chunk=4))
case("refuse_softcap", lambda: upd(qkv(BF), softcap=1.5))
case("refuse_num_splits_200", lambda: upd(qkv(BF), num_splits=200))
case("refuse_num_splits_minus2", lambda: upd(qkv(BF), num_splits=-2))
case("refuse_pack_gqa", lambda: upd(qkv(BF), pack_gqa=True))
case("refuse_rank", lambda: upd(qkv(BF), q=_t((300, 2, 128), BF)))
case("refuse_last_dim_strided", lambda: upd(qkv(BF), q=_t((1, 300, 2, 256), BF)[..., ::2]))
case("refuse_k_batch", lambda: upd(qkv(BF), k=_t((2, 520, 2, 128), BF)))
case("refuse_k_head_dim", lambda: upd(qkv(BF), k=_t((1, 520, 2, 64), BF)))
case("refuse_v_seqlen", lambda: upd(qkv(BF), v=_t((1, 519, 2, 128), BF)))
case("refuse_v_heads", lambda: upd(qkv(BF), v=_t((1, 520, 1, 128), BF)))
case("refuse_heads_not_divisible", lambda: qkv(BF, H=3, Hk=2))
case("refuse_head_size_not_multiple_of_8", lambda: qkv(BF, D=100))
case("refuse_head_size_not_multiple_of_16", lambda: qkv(F8, D=72))
case("refuse_head_size_above_256", lambda: qkv(BF, D=320))
case("refuse_descale_on_bf16", lambda: descales(qkv(BF), names="v"))
case("refuse_descale_shape", lambda: descales(qkv(F8, B=2), names="k", shape=(1, 2)))
case("refuse_descale_rank", lambda: descales(qkv(F8), names="q", shape=(2,)))
case("refuse_descale_dtype", lambda: descales(qkv(F8), names="v", dtype=torch.float64))
case("refuse_dv_differs", lambda: upd(qkv(BF), v=_t((1, 520, 2, 64), BF)))
case("refuse_out_dtype", lambda: with_out(qkv(BF), dtype=FH))
case("refuse_out_dtype_e4m3", lambda: with_out(qkv(F8), dtype=FH))
case("refuse_out_shape", lambda: with_out(qkv(BF), shape=(1, 300, 2, 64)))
case("refuse_out_last_dim_strided", lambda: upd(qkv(BF), out=_t((1, 300, 2, 256), BF)[..., ::2]))
case("refuse_out_dtype_padded", lambda: with_out(qkv(BF, D=80), dtype=FH))
case("refuse_out_shape_padded", lambda: with_out(qkv(BF, D=80), shape=(1, 300, 2, 96)))
case("refuse_out_dtype_padded_e4m3", lambda: with_out(qkv(F8, D=80), dtype=F8))
case("refuse_list_dtype", lambda: (lambda kw: upd(kw, attn_read_list=kw["attn_read_list"].long()))(with_lists(qkv(BF))))
case("refuse_write_list_dtype", lambda: (lambda kw: upd(kw, attn_write_list=kw["attn_write_list"].to(torch.uint8)))(with_lists(qkv(BF))))
case("refuse_list_dtypes_mixed", lambda: (lambda kw: upd(kw, attn_write_list=kw["attn_write_list"].to(I16)))(with_lists(qkv(BF))))
case("refuse_must_do_int16", lambda: (lambda kw: upd(kw, attn_must_do_list=kw["attn_must_do_list"].to(I16)))(with_lists(qkv(BF), must="4d")))
case("refuse_list_rank", lambda: (lambda kw: upd(kw, attn_read_list=kw["attn_read_list"][0]))(with_lists(qkv(BF))))
case("refuse_list_not_contiguous", lambda: (lambda kw: upd(kw, attn_write_list=kw["attn_write_list"].transpose(1, 2)))(with_lists(qkv(BF))))
case("refuse_list_shape", lambda: (lambda kw: upd(kw, attn_read_list=kw["attn_read_list"][..., :-1].contiguous()))(with_lists(qkv(BF))))
case("refuse_list_batch_too_small", lambda: with_lists(qkv(BF, B=2), batch=1))
case("refuse_must_do_4d_shape", lambda: (lambda kw: upd(kw, attn_must_do_list=kw["attn_must_do_list"][:, :1].contiguous()))(with_lists(qkv(BF), must="4d")))
case("refuse_must_do_1d_dtype", lambda: (lambda kw: upd(kw, attn_must_do_list=kw["attn_must_do_list"].long()))(with_lists(qkv(BF), must="1d")))
case("refuse_must_do_1d_rank", lambda: (lambda kw: upd(kw, attn_must_do_list=kw["attn_must_do_list"][None]))(with_lists(qkv(BF), must="1d")))
case("refuse_must_do_1d_strided", lambda: (lambda kw: upd(kw, attn_must_do_list=kw["attn_must_do_list"][::2]))(with_lists(qkv(BF), must="1d")))
case("refuse_must_do_1d_short", lambda: (lambda kw: upd(kw, attn_must_do_list=kw["attn_must_do_list"][:2]))(with_lists(qkv(BF), must="1d")))
case("refuse_windows_outside", lambda: upd(qkv(BF), _q_windows=[(0, 1), (1, 2)]))
case("refuse_windows_zero_count", lambda: upd(qkv(BF), _q_windows=[(0, 0)]))
case("refuse_windows_negative_begin", lambda: upd(qkv(BF), _q_windows=[(-1, 1)]))

# refused calls, packed route
case("refuse_packed_only_cu_q", lambda: (lambda kw: (kw.pop("cu_seqlens_k"), kw)[1])(packed(BF)))
case("refuse_packed_only_cu_k", lambda: (lambda kw: (kw.pop("cu_seqlens_q"), kw)[1])(packed(BF)))
case("refuse_packed_read_list_only", lambda: with_lists(packed(BF), write=False))
case("refuse_packed_write_list_only", lambda: (lambda kw: (kw.pop("attn_read_list"), kw)[1])(with_lists(packed(BF))))
case("refuse_packed_rank", lambda: upd(packed(BF), q=_t((1, 137, 2, 128), BF)))
case("refuse_packed_cu_dtype", lambda: (lambda kw: upd(kw, cu_seqlens_k=kw["cu_seqlens_k"].long()))(packed(BF)))
case("refuse_packed_cu_rank", lambda: (lambda kw: upd(kw, cu_seqlens_q=kw["cu_seqlens_q"][None]))(packed(BF)))
case("refuse_packed_cu_strided", lambda: (lambda kw: upd(kw, cu_seqlens_q=torch.zeros(6, dtype=I32)[::2]))(packed(BF)))
case("refuse_packed_cu_lengths_differ", lambda: upd(packed(BF), cu_seqlens_k=torch.tensor([0, 330], dtype=I32)))
case("refuse_packed_cu_single_entry", lambda: upd(packed(BF), cu_seqlens_q=torch.zeros(1, dtype=I32), cu_seqlens_k=torch.zeros(1, dtype=I32)))
case("refuse_packed_max_seqlen_q_missing", lambda: upd(packed(BF), max_seqlen_q=None))
case("refuse_packed_max_seqlen_k_missing", lambda: upd(packed(BF), max_seqlen_k=None))
case("refuse_packed_last_dim_strided", lambda: upd(packed(BF), k=_t((330, 2, 256), BF)[..., ::2]))
case("refuse_packed_k_head_dim", lambda: upd(packed(BF), k=_t((330, 2, 64), BF)))
case("refuse_packed_v_rows", lambda: upd(packed(BF), v=_t((329, 2, 128), BF)))
case("refuse_packed_heads_not_divisible", lambda: packed(BF, H=3, Hk=2))
case("refuse_packed_head_size_not_multiple_of_8", lambda: packed(BF, D=100))
case("refuse_packed_head_size_not_multiple_of_16", lambda: packed(F8, D=72))
case("refuse_packed_descale_on_bf16", lambda: descales(packed(BF), names="q"))
case("refuse_packed_descale_shape", lambda: descales(packed(F8), names="k", shape=(1, 2)))
case("refuse_packed_out_dtype", lambda: with_out(packed(BF), dtype=FH))
case("refuse_packed_out_shape", lambda: with_out(packed(BF), shape=(137, 2, 64)))
case("refuse_packed_out_dtype_padded", lambda: with_out(packed(BF, D=80), dtype=FH))
case("refuse_packed_out_shape_padded", lambda: with_out(packed(BF, D=80), shape=(137, 2, 96)))
case("refuse_packed_list_dtype", lambda: (lambda kw: upd(kw, attn_read_list=kw["attn_read_list"].long()))(with_lists(packed(BF))))
case("refuse_packed_list_dtypes_mixed", lambda: (lambda kw: upd(kw, attn_write_list=kw["attn_write_list"].to(I16)))(with_lists(packed(BF))))
case("refuse_packed_must_do_int16", lambda: (lambda kw: upd(kw, attn_must_do_list=kw["attn_must_do_list"].to(I16)))(with_lists(packed(BF), must="4d")))
case("refuse_packed_list_rank", lambda: (lambda kw: upd(kw, attn_write_list=kw["attn_write_list"][0]))(with_lists(packed(BF))))
case("refuse_packed_list_not_contiguous", lambda: upd(with_lists(packed(BF)), attn_read_list=torch.zeros(2, 2, 1, 10, dtype=I32)[..., ::2]))
case("refuse_packed_list_shape", lambda: (lambda kw: upd(kw, attn_write_list=kw["attn_write_list"][..., :-1].contiguous()))(with_lists(packed(BF))))
case("refuse_packed_list_batch_too_small", lambda: with_lists(packed(BF), batch=1))
case("refuse_packed_must_do_1d_dtype", lambda: (lambda kw: upd(kw, attn_must_do_list=kw["attn_must_do_list"].long()))(with_lists(packed(BF), must="1d")))
case("refuse_packed_must_do_1d_rank", lambda: (lambda kw: upd(kw, attn_must_do_list=kw["attn_must_do_list"][None]))(with_lists(packed(BF), must="1d")))
case("refuse_packed_must_do_1d_short", lambda: (lambda kw: upd(kw, attn_must_do_list=kw["attn_must_do_list"][:2]))(with_lists(packed(BF), must="1d")))


# the two merge entry points (they share the dtype code of the forward routes)
def _partials(dtype, n=3, B=2, S=40, H=2, D=64):
    return dict(out_partial=_t((n, B, S, H, D), dtype), lse_partial=torch.zeros(n, B, H, S).transpose(-1, -2))


for _n, _dt in (("bf16", BF), ("fp16", FH), ("fp32", torch.float32)):
    case(f"combine_{_n}", lambda dt=_dt: dict(fn="mha_combine", kw=_partials(dt)))
    case(f"combine_list_{_n}", lambda dt=_dt: dict(fn="combine_partials", kw=dict(outs=[_t((2, 40, 2, 64), dt) for _ in range(3)],
                                                                                   lses=[torch.zeros(2, 2, 40) for _ in range(3)])))
case("combine_fp32_into_bf16_out", lambda: dict(fn="mha_combine", kw=upd(_partials(torch.float32), out=_t((2, 40, 2, 64), BF), out_dtype=BF)))
case("combine_bf16_d60_padded", lambda: dict(fn="mha_combine", kw=_partials(BF, D=60)))
case("combine_list_fp32_into_fp16_no_lse", lambda: dict(fn="combine_partials", kw=dict(
    outs=[_t((2, 40, 2, 64), torch.float32) for _ in range(2)], lses=[torch.zeros(2, 2, 40) for _ in range(2)], out_dtype=FH, return_lse=False)))


# ---- running a case -----------------------------------------------------------------------------------------------------------------
def _named_tensors(kw):
    for name, val in kw.items():
        if isinstance(val, torch.Tensor):
            yield name, val
        elif isinstance(val, (list, tuple)):
            for i, t in enumerate(val):
                if isinstance(t, torch.Tensor):
                    yield f"{name}[{i}]", t


def _tensor_record(t, owners):
    return {"shape": list(t.shape), "dtype": str(t.dtype).replace("torch.", ""), "strides": list(t.stride()), "at": owners.resolve(t.data_ptr())}


def run_case(name):
    """Run the named case under the stand-ins; returns its record (see the module docstring)."""
    env, builder = CASES[name]
    with environment(env):
        spec = builder()
        if "kw" not in spec:
            spec = {"kw": spec}
        kw = dict(spec["kw"])
        fn = getattr(fai, spec.get("fn", "mha_fwd"))
        record = {"calls": [], "allocations": []}
        hooked = []
        if spec.get("hook"):
            kw["_window_hook"] = lambda i, o, r0, r1: hooked.append([i, list(o.shape), list(o.stride()), r0, r1])
            record["hook"] = hooked
        fai._SPLIT_CU.clear()
        with contextlib.ExitStack() as stack:
            owners = stack.enter_context(stand_ins(list(_named_tensors(kw)), record["calls"], record["allocations"],
                                                   rc=spec.get("rc", _cabi.LA_OK), cuda=spec.get("cuda", True), ws=spec.get("ws")))
            for flags, clear in spec.get("scope", ()):
                stack.enter_context(fai.fwd_flags(flags, clear))
            try:
                res = fn(**kw)
            except Exception as e:      # noqa: BLE001 - the type and the message are the record
                record["raises"] = [type(e).__name__, str(e)]
            else:
                res = res if isinstance(res, tuple) else (res,)
                record["returns"] = [None if t is None else _tensor_record(t, owners) for t in res]
                record["out_is_callers"] = kw.get("out") is not None and res[0] is kw["out"]
        fai._SPLIT_CU.clear()
    return record


def load_golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)


# ---- host time per call (profiles/host_path.md) -------------------------------------------------------------------------------------
TIMED = {"dense_bf16": "fixed_bf16_d128", "lists_must1d": "fixed_bf16_lists_must1d", "split_one_sequence": "split_bf16_n3"}


def time_calls(rounds=5, calls=2000):
    """Five medians of 2000 calls each, in microseconds, of three calls under the stand-ins (no recording: only the Python path and
    the two host functions of the library are timed)."""
    result = {}
    for label, name in TIMED.items():
        env, builder = CASES[name]
        with environment(env):
            kw = builder()
            with stand_ins():
                for _ in range(200):
                    fai.mha_fwd(**kw)
                medians = []
                for _ in range(rounds):
                    ts = []
                    for _ in range(calls):
                        t0 = time.perf_counter()
                        fai.mha_fwd(**kw)
                        ts.append(time.perf_counter() - t0)
                    medians.append(round(statistics.median(ts) * 1e6, 2))
        result[label] = medians
    return result


def _load_other(path):
    """Another copy of flash_attn_interface.py (the parent commit's, say) as a second module of the package; it must not register
    the ops a second time."""
    import importlib.util
    real, torch.library.Library = torch.library.Library, lambda *a, **k: types.SimpleNamespace(define=lambda *a, **k: None, impl=lambda *a, **k: None)
    try:
        spec = importlib.util.spec_from_file_location("liteattention_amd._other_flash_attn_interface", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        torch.library.Library = real
    return mod


def time_against(path, blocks=100, calls=100):
    """This tree's ``mha_fwd`` against the one in ``path``, in ONE process, in alternating blocks of 100 calls, so that both see the
    same machine state: per call the medians over the blocks' medians, and the median of the paired differences (this - other), in us."""
    other = _load_other(path)
    result = {}
    for label, name in TIMED.items():
        env, builder = CASES[name]
        with environment(env):
            kw = builder()
            with stand_ins():
                meds = {other: [], fai: []}
                for i in range(3 + blocks):
                    for mod in ((other, fai) if i % 2 else (fai, other)):      # neither is always the one that runs second
                        ts = []
                        for _ in range(calls):
                            t0 = time.perf_counter()
                            mod.mha_fwd(**kw)
                            ts.append(time.perf_counter() - t0)
                        meds[mod].append(statistics.median(ts) * 1e6)
        o, b = meds[other][3:], meds[fai][3:]      # (the first blocks warm up)
        result[label] = {"other": round(statistics.median(o), 2), "this": round(statistics.median(b), 2),
                         "paired_diff": round(statistics.median([y - x for x, y in zip(o, b)]), 2)}
    return result


if __name__ == "__main__":
    if "--time-against" in sys.argv:
        print(json.dumps(time_against(sys.argv[sys.argv.index("--time-against") + 1])))
    elif "--write" in sys.argv:
        with open(GOLDEN_PATH, "w") as f:
            json.dump({name: run_case(name) for name in CASES}, f, separators=(",", ":"), sort_keys=True)
            f.write("\n")
        print(f"{len(CASES)} cases -> {GOLDEN_PATH} ({os.path.getsize(GOLDEN_PATH)} bytes)")
    elif "--time" in sys.argv:
        print(json.dumps(time_calls()))
    else:
        for name in sys.argv[1:]:
            print(name, json.dumps(run_case(name), indent=1))
