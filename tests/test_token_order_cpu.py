"""CPU: token orders - `brick_order` against a brute-force sort, `TokenOrder.from_rows`, every validation rule of the three `_rows` entry
points (all of them answer before any HIP call, so no device is needed), the reference functions under a map, and the Python argument
checks, which run before anything launches."""
import ctypes
import itertools
import os
import re
import sys

import pytest
import torch

from liteattention_amd import _cabi

import test_qk_prep_cpu as unmapped

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lite_attention_amd.h")
BRICKS = ((1, 4, 4), (1, 2, 2))


# ---- brick_order ------------------------------------------------------------------------------------------------------------------------
def brute_force(grid, bricks):
    T, H, W = grid
    toks = list(itertools.product(range(T), range(H), range(W)))
    key = lambda p: tuple(c // b for lvl in bricks for c, b in zip(p, lvl)) + p                      # noqa: E731
    return [(t * H + y) * W + x for t, y, x in sorted(toks, key=key)]


@pytest.mark.parametrize("grid", [(2, 4, 4), (2, 5, 7)])
def test_brick_order_equals_a_brute_force_sort(grid):
    import liteattention_amd as L
    order = L.brick_order(grid, BRICKS)
    n = grid[0] * grid[1] * grid[2]
    assert order.grid == grid and order.bricks == BRICKS and order.src_seqlen == n == len(order)
    assert order.src_rows.dtype == order.dst_rows.dtype == torch.int32
    assert order.src_rows.tolist() == brute_force(grid, BRICKS)
    assert sorted(order.src_rows.tolist()) == list(range(n))                                       # a permutation, partial bricks or not
    assert torch.equal(order.dst_rows[order.src_rows.long()], torch.arange(n, dtype=torch.int32))
    assert L.brick_order(grid, BRICKS[:1]).src_rows.tolist() == brute_force(grid, BRICKS[:1])


def test_aligned_runs_are_bricks_on_the_dividing_grid():
    import liteattention_amd as L
    T, H, W = grid = (2, 4, 4)
    src = L.brick_order(grid, BRICKS).src_rows.long()
    t, y, x = src // (H * W), (src // W) % H, src % W
    inner = torch.stack((t, y // 2, x // 2), 1).view(-1, 4, 3)
    outer = torch.stack((t, y // 4, x // 4), 1).view(-1, 16, 3)
    assert (inner == inner[:, :1]).all() and len({tuple(r) for r in inner[:, 0].tolist()}) == inner.shape[0]
    assert (outer == outer[:, :1]).all() and len({tuple(r) for r in outer[:, 0].tolist()}) == outer.shape[0]


def test_frames_stay_contiguous_with_bt_1():
    import liteattention_amd as L
    src = L.brick_order((2, 5, 7), BRICKS).src_rows
    for f in range(2):
        assert sorted(src[35 * f:35 * f + 35].tolist()) == list(range(35 * f, 35 * f + 35))


def test_brick_order_argument_errors():
    import liteattention_amd as L
    for bad in (dict(grid=(2, 4)), dict(grid=(2, 0, 4)), dict(grid=(2, 4, 4), bricks=()), dict(grid=(2, 4, 4), bricks=((1, 0, 2),)),
                dict(grid=(2, 4, 4), bricks=((2, 2),))):
        with pytest.raises(ValueError):
            L.brick_order(**bad)


def test_from_rows():
    import liteattention_amd as L
    perm = torch.tensor([2, 0, 3, 1], dtype=torch.int32)
    order = L.TokenOrder.from_rows(perm, 4)
    assert torch.equal(order.dst_rows[perm.long()], torch.arange(4, dtype=torch.int32)) and order.grid is None
    pruned = L.TokenOrder.from_rows(torch.tensor([5, 1, 1], dtype=torch.int32), 6)                   # a selection: no inverse
    assert pruned.dst_rows is None and len(pruned) == 3 and pruned.src_seqlen == 6
    with pytest.raises(ValueError):
        pruned.restore_lse(torch.zeros(1, 1, 3))
    with pytest.raises(TypeError):
        L.TokenOrder.from_rows(perm.long(), 4)
    with pytest.raises(ValueError, match=r"src_rows\[2\] = 4"):
        L.TokenOrder.from_rows(torch.tensor([0, 1, 4, 2], dtype=torch.int32), 4)
    with pytest.raises(ValueError):
        L.TokenOrder.from_rows(torch.tensor([0, -1], dtype=torch.int32), 4)
    with pytest.raises(ValueError):
        L.TokenOrder.from_rows(perm.view(2, 2), 4)
    lse = torch.randn(2, 3, 4)
    assert torch.equal(order.restore_lse(lse[..., perm.long()]), lse)


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------------------
ENTRIES = (("la_qk_prep", _cabi.LaQkPrepArgs), ("la_qk_prep_fp8", _cabi.LaQkPrepFp8Args), ("la_qk_prep_smooth", _cabi.LaQkPrepSmoothArgs))


def test_the_three_entry_points_are_exported_declared_and_bound_under_abi_9():
    lib = _cabi.load()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert lib.la_abi_version() == _cabi.LA_ABI_VERSION == 9
    for name, struct in ENTRIES:
        fn = getattr(lib, name + "_rows")
        assert name + "_rows" in _cabi.EXPORTED_SYMBOLS
        assert re.search(r"\bint\s+" + name + r"_rows\s*\(\s*const\s+" + name + r"_args\s*\*\s*\w+\s*,\s*const\s+la_row_map\s*\*", src)
        assert fn.argtypes[0]._type_ is struct and fn.argtypes[1]._type_ is _cabi.LaRowMap
    info = _cabi.build_info()
    assert info["variant"] == "0" and info["wrong_results"] == "0"                                  # a product build, no new option
    import liteattention_amd
    import lite_attention
    for name in ("brick_order", "TokenOrder"):
        assert getattr(lite_attention, name) is getattr(liteattention_amd, name)


def test_row_map_layout_matches_header(tmp_path):
    import subprocess
    fields = [f[0] for f in _cabi.LaRowMap._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){", 'printf("%zu\\n", sizeof(la_row_map));']
    prog += [f'printf("%zu\\n", offsetof(la_row_map, {f}));' for f in fields] + ["return 0;}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(c)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(_cabi.LaRowMap)
    for f, off in zip(fields, out[1:]):
        assert getattr(_cabi.LaRowMap, f).offset == int(off), f


def _valid_map(seqlen=60, **changes):
    m = _cabi.LaRowMap()
    m.struct_size, m.src_seqlen = ctypes.sizeof(_cabi.LaRowMap), seqlen
    m.src_rows, m.positions, m.batch_stride = 0x50000, 0x60000, seqlen
    for k, v in changes.items():
        setattr(m, k, v)
    return m


def _valid_args(struct):
    """`test_qk_prep_cpu._valid_args` as any of the three argument structs (the shared fields have the same names)."""
    src = unmapped._valid_args()
    a = struct()
    for name, _ in _cabi.LaQkPrepArgs._fields_:
        if name != "out_dtype" or struct is _cabi.LaQkPrepArgs:
            setattr(a, name, getattr(src, name))
    a.struct_size = ctypes.sizeof(struct)
    if struct is not _cabi.LaQkPrepArgs:
        a.heads_per_scale = 1
    return a


def _first_failing_check(entry, struct, map_changes=None, null_map=False, **changes):
    """The code `entry`_rows answers for valid arguments and a valid map with the scalar fields of `changes` / `map_changes` replaced."""
    a = _valid_args(struct)
    for k, v in changes.items():
        setattr(a, k, v)
    m = _valid_map(**(map_changes or {}))
    return getattr(_cabi.load(), entry + "_rows")(ctypes.byref(a), None if null_map else ctypes.byref(m), None)


@pytest.mark.parametrize("entry,struct", ENTRIES)
def test_every_rule_of_the_map_answers_its_code_without_a_device(entry, struct):
    lib = _cabi.load()
    m = _valid_map()
    check = lambda **kw: _first_failing_check(entry, struct, **kw)                                  # noqa: E731
    assert getattr(lib, entry + "_rows")(None, ctypes.byref(m), None) == _cabi.LA_ERR_NULL_ARG
    assert check(null_map=True) == _cabi.LA_ERR_NULL_ARG
    assert check(map_changes=dict(struct_size=ctypes.sizeof(_cabi.LaRowMap) - 8)) == _cabi.LA_ERR_STRUCT_SIZE
    assert check(map_changes=dict(struct_size=0)) == _cabi.LA_ERR_STRUCT_SIZE
    assert check(struct_size=0, map_changes=dict(struct_size=0)) == _cabi.LA_ERR_STRUCT_SIZE
    assert check(map_changes=dict(src_seqlen=0)) == _cabi.LA_ERR_SHAPE
    assert check(map_changes=dict(src_seqlen=-3)) == _cabi.LA_ERR_SHAPE
    assert check(map_changes=dict(src_seqlen=59, src_rows=None)) == _cabi.LA_ERR_SHAPE                # the identity source needs 60 rows of x
    assert check(map_changes=dict(src_rows=0x50002)) == _cabi.LA_ERR_STRIDE
    assert check(map_changes=dict(positions=0x60001)) == _cabi.LA_ERR_STRIDE
    assert check(map_changes=dict(batch_stride=-1)) == _cabi.LA_ERR_STRIDE
    assert check(out=0x10000) == _cabi.LA_ERR_UNSUPPORTED                                             # out == x with src_rows: no in-place gather
    # positions == NULL: the bound of the unmapped call holds for pos_offset + src_seqlen (61 rows of x on 60 positions) ...
    wide = dict(src_seqlen=61, positions=None)
    assert check(map_changes=wide) == _cabi.LA_ERR_SHAPE
    assert check(map_changes=dict(src_seqlen=59, positions=None), pos_offset=2) == _cabi.LA_ERR_SHAPE
    # ... and with a table the positions are the table's, clamped by the kernel: 61 rows of x pass, and the complaint left is the one
    # planted BEHIND the position check (the e4m3 forms keep at most 1024 heads; la_qk_prep has no check behind it)
    if struct is not _cabi.LaQkPrepArgs:
        many = dict(norm_mode=_cabi.LA_NORM_HEAD, num_heads=1025, x_row_stride=1025 * 128, out_row_stride=1025 * 128,
                    x_batch_stride=61 * 1025 * 128, out_batch_stride=60 * 1025 * 128)
        assert check(map_changes=dict(src_seqlen=61), **many) == _cabi.LA_ERR_UNSUPPORTED
        assert check(map_changes=wide, **many) == _cabi.LA_ERR_SHAPE
    planted = dict(norm_mode=_cabi.LA_NORM_TOKEN, num_heads=65, head_dim=256, x_batch_stride=60 * 65 * 256, out_batch_stride=60 * 65 * 256,
                   x_row_stride=65 * 256, out_row_stride=65 * 256, x_head_stride=256, out_head_stride=256)
    assert check(**planted) == _cabi.LA_ERR_UNSUPPORTED                                               # (the unmapped rules still hold)


UNMAPPED_CASES = [dict(struct_size=0), dict(x=None), dict(out=None), dict(in_dtype=7), dict(in_dtype=_cabi.LA_DTYPE_FP8_E4M3),
                  dict(out_dtype=_cabi.LA_DTYPE_FP32), dict(norm_mode=3), dict(norm_mode=-1), dict(batch=0), dict(seqlen=-1),
                  dict(num_heads=0), dict(head_dim=0), dict(head_dim=100), dict(head_dim=264), dict(head_dim=4),
                  dict(x_row_stride=-512), dict(out_head_stride=-128), dict(x_batch_stride=-1), dict(x=0x10002), dict(out=0x20008),
                  dict(x_row_stride=516), dict(x_head_stride=132), dict(out_batch_stride=60 * 512 + 2), dict(weight=0x30004),
                  dict(pos_offset=-1), dict(pos_offset=1), dict(seqlen=61, x_batch_stride=61 * 512, out_batch_stride=61 * 512)]


@pytest.mark.parametrize("changes", UNMAPPED_CASES, ids=["-".join(f"{k}={v}" for k, v in c.items()) for c in UNMAPPED_CASES])
def test_a_map_with_both_tables_null_answers_as_the_unmapped_entry(changes):
    """The cases of tests/test_qk_prep_cpu.py (its `_first_failing_check`): la_qk_prep_rows with a both-NULL map of src_seqlen == seqlen
    gives the code la_qk_prep gives."""
    want = unmapped._first_failing_check(**changes)
    a = unmapped._valid_args()
    for k, v in changes.items():
        setattr(a, k, v)
    m = _valid_map(seqlen=a.seqlen, src_rows=None, positions=None, batch_stride=0)
    got = _cabi.load().la_qk_prep_rows(ctypes.byref(a), ctypes.byref(m), None)
    assert got == want != _cabi.LA_OK


def test_array_cases_of_the_unmapped_file_with_a_null_map():
    lib = _cabi.load()
    for field, i, v in (("rope_table", 1, 0x41004), ("axis_pairs", 1, -1), ("axis_pairs", 2, 22), ("rope_table", 1, None), ("axis_extent", 1, 0)):
        a = unmapped._valid_args()
        getattr(a, field)[i] = v
        m = _valid_map(src_rows=None, positions=None, batch_stride=0)
        assert lib.la_qk_prep_rows(ctypes.byref(a), ctypes.byref(m), None) == unmapped._rc(a) != _cabi.LA_OK


# ---- the reference functions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["token", "head", None])
def test_references_commute_with_the_order(norm):
    """ref(x[:, src], positions=src) == ref(x)[:, src] == ref(x, rows=src), exactly, for every output that has rows; the amax is
    order-free, and the column mean of the smooth reference (fp64, the same S terms in another order) to 2 S 2^-53 mean|y|."""
    import liteattention_amd as L
    torch.manual_seed(4)
    Bn, S, H, D = 2, 60, 2, 32
    x = torch.randn(Bn, S, H, D)
    w = 0.5 + torch.rand(H * D if norm == "token" else D)
    tabs = L.rope_tables((3, 4, 5), D)
    shared = torch.randperm(S)
    per_batch = torch.stack([torch.randperm(S) for _ in range(Bn)])
    descale, shift, vec = 0.01 + torch.rand(Bn, H), torch.randn(Bn, H, D), torch.randn(Bn, H, D)
    for src in (shared, per_batch, shared.int()):
        take = (lambda t, dim=1: t.index_select(dim, src.long())) if src.dim() == 1 else \
            (lambda t, dim=1: torch.stack([t[b].index_select(dim - 1, src[b]) for b in range(Bn)]))
        xs = take(x)
        want = take(L.qk_prep_reference(x, w, 1e-6, tabs, norm=norm))
        assert torch.equal(L.qk_prep_reference(xs, w, 1e-6, tabs, norm=norm, positions=src), want)
        assert torch.equal(L.qk_prep_reference(x, w, 1e-6, tabs, norm=norm, rows=src), want)
        assert not torch.equal(L.qk_prep_reference(xs, w, 1e-6, tabs, norm=norm), want)
        z0, a0 = L.qk_prep_fp8_reference(x, w, 1e-6, tabs, norm=norm, descale=descale)
        for kw, xin in ((dict(positions=src), xs), (dict(rows=src), x)):
            z1, a1 = L.qk_prep_fp8_reference(xin, w, 1e-6, tabs, norm=norm, descale=descale, **kw)
            assert torch.equal(z1, take(z0)) and torch.equal(a1, a0)
        z0, a0, m0, d0 = L.qk_prep_smooth_reference(x, w, 1e-6, tabs, norm=norm, shift=shift, descale=descale, dot_vec=vec)
        for kw, xin in ((dict(positions=src), xs), (dict(rows=src), x)):
            z1, a1, m1, d1 = L.qk_prep_smooth_reference(xin, w, 1e-6, tabs, norm=norm, shift=shift, descale=descale, dot_vec=vec, **kw)
            assert torch.equal(z1, take(z0)) and torch.equal(a1, a0) and torch.equal(d1, take(d0, 2))
            y_abs = L.qk_prep_reference(x, w, 1e-6, tabs, norm=norm).abs().mean(1)
            assert ((m1 - m0).abs() <= 2 * S * 2.0 ** -53 * y_abs).all()


def test_reference_refuses_what_the_kernel_would_clamp():
    import liteattention_amd as L
    x = torch.randn(1, 60, 2, 32)
    tabs = L.rope_tables((3, 4, 5), 32)
    with pytest.raises(ValueError):
        L.qk_prep_reference(x, None, 1e-6, tabs, rows=torch.tensor([0, 60]))
    with pytest.raises(ValueError):
        L.qk_prep_reference(x, None, 1e-6, tabs, positions=torch.arange(60) + 1)
    with pytest.raises(ValueError):
        L.qk_prep_reference(x, None, 1e-6, tabs, positions=torch.arange(59))
    with pytest.raises(ValueError):
        L.qk_prep_reference(x, None, 1e-6, tabs, positions=torch.arange(60).float())


# ---- Python argument errors: before any launch (these are CPU tensors on a machine without a GPU) ------------------------------------------
class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it lives on a GPU: the argument checks of the prologue calls run on it, a launch never happens."""
    is_cuda = True


def _fake(t):
    return t.as_subclass(_FakeCuda)


def test_python_argument_errors_surface_before_any_launch(monkeypatch):
    import liteattention_amd as L
    Q = sys.modules["liteattention_amd.qk_prep"]                                                      # (the package attribute is the function)
    launched = []
    monkeypatch.setattr(Q, "_call", lambda *a, **k: launched.append(a))
    x = _fake(torch.randn(2, 60, 3, 64).bfloat16())
    ok = torch.arange(60, dtype=torch.int32)
    for kw, exc in ((dict(rows=ok.long()), TypeError), (dict(positions=ok.float()), TypeError), (dict(rows=[0, 1]), TypeError),
                    (dict(rows=ok.view(3, 20)), ValueError),                                           # [3, S] for a batch of 2
                    (dict(positions=ok[:59]), ValueError),                                             # positions: one per row of the result
                    (dict(rows=ok[:30], positions=ok), ValueError),
                    (dict(rows=ok, positions=ok.expand(2, 60).contiguous()), ValueError),              # one batch stride for both
                    (dict(rows=torch.zeros(2, 120, dtype=torch.int32)[:, ::2]), ValueError),                                # last dimension not contiguous
                    (dict(rows=ok, out=x), ValueError)):                                               # a gather in place
        for fn in (L.qk_prep, L.qk_prep_fp8, L.qk_prep_amax, L.qk_prep_smooth, L.qk_prep_colmean):
            if "out" in kw and fn is not L.qk_prep:
                continue
            with pytest.raises(exc):
                fn(x, None, 1e-6, None, **kw)
    with pytest.raises(ValueError, match="gather"):
        L.E4m3Scales(tiles=True)(x, norm=None, rows=ok)
    with pytest.raises(TypeError):
        L.v_prep_tiles(x, rows=ok)                                                                     # takes no map: gather V first
    order = L.TokenOrder.from_rows(ok, 60)
    with pytest.raises(ValueError):
        order.gather(_fake(torch.zeros(2, 59, 3, 64).bfloat16()))
    with pytest.raises(ValueError):
        L.TokenOrder.from_rows(torch.tensor([3, 3], dtype=torch.int32), 4).restore(x)
    assert not launched
    # ... and a call that passes them reaches the launch with the _rows entry point and a map of the right shape
    out = torch.empty(2, 30, 3, 64, dtype=torch.bfloat16)
    L.qk_prep(x, None, 1e-6, None, rows=ok[:30], out=out)
    (entry, _, _, a, m), = launched
    assert entry == "la_qk_prep_rows" and a._obj.seqlen == 30 and m._obj.src_seqlen == 60 and m._obj.batch_stride == 0
    assert m._obj.src_rows == ok.data_ptr() and not m._obj.positions
