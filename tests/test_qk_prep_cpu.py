"""CPU: the q / k prologue (la_qk_prep) at the boundary - the symbol, the argument struct, every validation rule (all of them answer
before any HIP call, so no device is needed) - and the host side of it: the rope tables and the fp64 reference against the demo block's
own eager RMSNorm + rope_3d."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from liteattention_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lite_attention_amd.h")
sys.path.insert(0, os.path.join(ROOT, "examples"))


def test_la_qk_prep_is_exported_declared_and_bound_under_abi_9():
    lib = _cabi.load()
    assert "la_qk_prep" in _cabi.EXPORTED_SYMBOLS and hasattr(lib, "la_qk_prep")
    assert lib.la_abi_version() == _cabi.LA_ABI_VERSION == 9
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+la_qk_prep\s*\(\s*const\s+la_qk_prep_args\s*\*", src)
    assert re.search(r"#define\s+LA_ABI_VERSION\s+9\b", src)
    assert lib.la_qk_prep.argtypes[0]._type_ is _cabi.LaQkPrepArgs
    import liteattention_amd
    import lite_attention
    for name in ("qk_prep", "qk_prep_reference", "rope_tables"):
        assert getattr(lite_attention, name) is getattr(liteattention_amd, name)
    assert hasattr(torch.ops.lite_attention, "qk_prep") and hasattr(torch.ops.lite_attention, "fwd")


def test_qk_prep_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of la_qk_prep_args as gcc compiles the header == the ctypes mirror; the enum values too."""
    fields = [f[0] for f in _cabi.LaQkPrepArgs._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
            'printf("%zu\\n", sizeof(la_qk_prep_args));']
    prog += [f'printf("%zu\\n", offsetof(la_qk_prep_args, {f}));' for f in fields]
    prog += ['printf("%d %d %d\\n", (int)LA_NORM_NONE, (int)LA_NORM_TOKEN, (int)LA_NORM_HEAD);', "return 0;}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(c)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(_cabi.LaQkPrepArgs)
    for f, off in zip(fields, out[1:]):
        assert getattr(_cabi.LaQkPrepArgs, f).offset == int(off), f
    assert [int(v) for v in out[-3:]] == [_cabi.LA_NORM_NONE, _cabi.LA_NORM_TOKEN, _cabi.LA_NORM_HEAD]


def _valid_args(H=4, D=128, S=60, B=2, in_dtype=_cabi.LA_DTYPE_BF16, out_dtype=_cabi.LA_DTYPE_BF16):
    """Arguments that pass every check (grid (3, 4, 5), Wan's split of D = 128); pointers are never dereferenced on the host."""
    a = _cabi.LaQkPrepArgs()
    a.struct_size = ctypes.sizeof(_cabi.LaQkPrepArgs)
    a.in_dtype, a.out_dtype, a.norm_mode = in_dtype, out_dtype, _cabi.LA_NORM_TOKEN
    a.x, a.out, a.weight = 0x10000, 0x20000, 0x30000
    a.x_batch_stride = a.out_batch_stride = S * H * D
    a.x_row_stride = a.out_row_stride = H * D
    a.x_head_stride = a.out_head_stride = D
    a.batch, a.seqlen, a.num_heads, a.head_dim = B, S, H, D
    a.eps, a.pos_offset = 1e-6, 0
    for i, (e, n) in enumerate(zip((3, 4, 5), (22, 21, 21))):
        a.rope_table[i], a.axis_extent[i], a.axis_pairs[i] = 0x40000 + 0x1000 * i, e, n
    return a


def _rc(a):
    return _cabi.load().la_qk_prep(ctypes.byref(a), None)


def _first_failing_check(**changes):
    """The code la_qk_prep answers for valid arguments with the scalar fields of `changes` replaced."""
    a = _valid_args()
    for k, v in changes.items():
        setattr(a, k, v)
    return _rc(a)


def test_null_args_struct_size_and_null_tensors():
    lib = _cabi.load()
    assert lib.la_qk_prep(None, None) == _cabi.LA_ERR_NULL_ARG
    assert _first_failing_check(struct_size=ctypes.sizeof(_cabi.LaQkPrepArgs) - 4) == _cabi.LA_ERR_STRUCT_SIZE
    assert _first_failing_check(struct_size=0) == _cabi.LA_ERR_STRUCT_SIZE
    assert _first_failing_check(x=None) == _cabi.LA_ERR_NULL_ARG
    assert _first_failing_check(out=None) == _cabi.LA_ERR_NULL_ARG


def test_dtypes_and_norm_mode():
    assert _first_failing_check(in_dtype=_cabi.LA_DTYPE_FP8_E4M3) == _cabi.LA_ERR_DTYPE
    assert _first_failing_check(in_dtype=7) == _cabi.LA_ERR_DTYPE
    assert _first_failing_check(out_dtype=_cabi.LA_DTYPE_FP32) == _cabi.LA_ERR_DTYPE          # fp32 is an input type only
    assert _first_failing_check(out_dtype=_cabi.LA_DTYPE_FP8_E4M3) == _cabi.LA_ERR_DTYPE
    assert _first_failing_check(norm_mode=3) == _cabi.LA_ERR_UNSUPPORTED
    assert _first_failing_check(norm_mode=-1) == _cabi.LA_ERR_UNSUPPORTED


@pytest.mark.parametrize("field", ["batch", "seqlen", "num_heads", "head_dim"])
def test_non_positive_sizes(field):
    assert _first_failing_check(**{field: 0}) == _cabi.LA_ERR_SHAPE
    assert _first_failing_check(**{field: -1}) == _cabi.LA_ERR_SHAPE


def test_head_dim_rules():
    assert _first_failing_check(head_dim=100) == _cabi.LA_ERR_HEAD_DIM                         # % 8
    assert _first_failing_check(head_dim=264) == _cabi.LA_ERR_HEAD_DIM                         # > 256
    assert _first_failing_check(head_dim=4) == _cabi.LA_ERR_HEAD_DIM


def test_token_norm_limit_is_16384_elements():
    """H * D = 16384 passes the limit (the complaint is the one planted behind it), 16392 and 65 * 256 do not; head norm has no limit."""
    a = _valid_args(H=64, D=256)
    a.pos_offset = 1                                                 # 1 + 60 rows > 3 * 4 * 5 positions: the LAST check
    assert _rc(a) == _cabi.LA_ERR_SHAPE
    a = _valid_args(H=65, D=256)
    a.pos_offset = 1
    assert _rc(a) == _cabi.LA_ERR_UNSUPPORTED
    a = _valid_args(H=2049, D=8)                                     # H * D = 16392
    a.axis_pairs[0], a.axis_pairs[1], a.axis_pairs[2] = 2, 1, 1
    a.pos_offset = 1
    assert _rc(a) == _cabi.LA_ERR_UNSUPPORTED
    a.norm_mode = _cabi.LA_NORM_HEAD
    assert _rc(a) == _cabi.LA_ERR_SHAPE


def test_stride_rules():
    H, D = 4, 128
    assert _first_failing_check(x_row_stride=-H * D) == _cabi.LA_ERR_STRIDE
    assert _first_failing_check(out_head_stride=-D) == _cabi.LA_ERR_STRIDE
    assert _first_failing_check(x_batch_stride=-1) == _cabi.LA_ERR_STRIDE
    assert _first_failing_check(x=0x10002) == _cabi.LA_ERR_STRIDE                               # pointer off a 16-byte boundary
    assert _first_failing_check(out=0x20008) == _cabi.LA_ERR_STRIDE
    assert _first_failing_check(x_row_stride=H * D + 4) == _cabi.LA_ERR_STRIDE                  # bf16: rows must start every 8 elements
    assert _first_failing_check(x_head_stride=D + 4) == _cabi.LA_ERR_STRIDE
    assert _first_failing_check(out_batch_stride=60 * H * D + 2) == _cabi.LA_ERR_STRIDE
    assert _first_failing_check(weight=0x30004) == _cabi.LA_ERR_STRIDE
    a = _valid_args()
    a.rope_table[1] = 0x41004
    assert _rc(a) == _cabi.LA_ERR_STRIDE


def test_a_stride_valid_for_fp32_input_is_misaligned_for_bf16_output():
    """Row stride H * D + 4 elements: 16-byte rows for fp32 (4 elements), not for bf16 (8 elements)."""
    H, D = 4, 128
    a = _valid_args(in_dtype=_cabi.LA_DTYPE_FP32)
    a.x_row_stride = H * D + 4
    a.x_batch_stride = 60 * (H * D + 4)
    a.pos_offset = 1                                                 # accepted: the only complaint left is the one planted in the LAST check
    assert _rc(a) == _cabi.LA_ERR_SHAPE
    a = _valid_args(in_dtype=_cabi.LA_DTYPE_FP32)
    a.x_row_stride = a.out_row_stride = H * D + 4
    a.x_batch_stride = a.out_batch_stride = 60 * (H * D + 4)
    assert _rc(a) == _cabi.LA_ERR_STRIDE                             # the same stride on the bf16 output
    a.x_row_stride, a.x_batch_stride = H * D + 2, 60 * (H * D + 2)   # ... and 2 elements off is misaligned for fp32 too
    a.out_row_stride, a.out_batch_stride = H * D, 60 * H * D
    assert _rc(a) == _cabi.LA_ERR_STRIDE


def test_axis_pairs_rules():
    a = _valid_args()
    a.axis_pairs[1] = -1
    assert _rc(a) == _cabi.LA_ERR_SHAPE
    a = _valid_args()
    a.axis_pairs[2] = 22                                             # 22 + 21 + 22 = 65 > 128 / 2
    assert _rc(a) == _cabi.LA_ERR_SHAPE


def test_table_pointer_rules():
    a = _valid_args()
    a.rope_table[1] = None
    assert _rc(a) == _cabi.LA_ERR_NULL_ARG                           # axis 1 rotates 21 pairs and has no table
    a.pos_offset = 1
    assert _rc(a) == _cabi.LA_ERR_NULL_ARG                           # (checked before the positions)
    a.axis_pairs[1] = 0                                              # an axis that rotates nothing needs no table: the complaint left is
    assert _rc(a) == _cabi.LA_ERR_SHAPE                              # the one planted in the last check, 1 + 60 rows > 60 positions


def test_position_rules():
    assert _first_failing_check(pos_offset=-1) == _cabi.LA_ERR_SHAPE
    assert _first_failing_check(pos_offset=1) == _cabi.LA_ERR_SHAPE                             # 1 + 60 rows > 3 * 4 * 5 positions
    assert _first_failing_check(seqlen=61, x_batch_stride=61 * 512, out_batch_stride=61 * 512) == _cabi.LA_ERR_SHAPE
    a = _valid_args()
    a.axis_extent[1] = 0
    assert _rc(a) == _cabi.LA_ERR_SHAPE


# ---- the host side: tables and the reference against the demo's own eager code ------------------------------------------------------------
GRIDS = ((3, 4, 5), (1, 1, 61))
HEAD_DIMS = (40, 64, 96, 128, 256)


def _demo_angles(grid, D, theta=10000.0):
    """rope_3d's own angles: per axis the fp32 (S, d / 2) tensor `ang` of examples/wan_self_attention_demo.py, the same expressions."""
    F, Hh, W = grid
    parts = [D - 2 * (D // 3), D // 3, D // 3]
    parts = [p - (p % 2) for p in parts]
    parts[0] = D - parts[1] - parts[2]
    f = torch.arange(F).view(F, 1, 1).expand(F, Hh, W).reshape(-1)
    h = torch.arange(Hh).view(1, Hh, 1).expand(F, Hh, W).reshape(-1)
    w = torch.arange(W).view(1, 1, W).expand(F, Hh, W).reshape(-1)
    out = []
    for pos, d in zip((f, h, w), parts):
        freqs = 1.0 / theta ** (torch.arange(0, d, 2).float() / d)
        out.append((pos, d, pos.float()[:, None] * freqs[None]))
    return out


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("D", HEAD_DIMS)
def test_rope_tables_match_the_demo(grid, D):
    import liteattention_amd as L
    tables, pairs = L.rope_tables(grid, D)
    assert L.rope_tables(grid, D).tables[0] is tables[0]                    # cached
    angles = _demo_angles(grid, D)
    assert tuple(pairs) == tuple(d // 2 for _, d, _ in angles) and sum(pairs) == D // 2
    for t, extent, (pos, d, ang) in zip(tables, grid, angles):
        assert t.dtype == torch.float32 and tuple(t.shape) == (extent, d // 2, 2) and t.is_contiguous()
        got = t[pos].double()                                              # (S, d / 2, 2): the row of every token's coordinate
        assert (got[..., 0] - ang.double().cos()).abs().max().item() <= 2.0 ** -23
        assert (got[..., 1] - ang.double().sin()).abs().max().item() <= 2.0 ** -23


def test_rope_tables_one_axis_and_partial_rotary():
    import liteattention_amd as L
    tables, pairs = L.rope_tables((17, 1, 1), 64, parts=(64, 0, 0))
    assert tuple(pairs) == (32, 0, 0) and tuple(tables[0].shape) == (17, 32, 2) and tables[1].numel() == 0
    tables, pairs = L.rope_tables((3, 4, 5), 64, parts=(16, 16, 16))
    assert tuple(pairs) == (8, 8, 8)
    with pytest.raises(ValueError):
        L.rope_tables((3, 4, 5), 64, parts=(22, 22, 22))
    with pytest.raises(ValueError):
        L.rope_tables((3, 4, 5), 64, parts=(21, 21, 20))


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("D", HEAD_DIMS)
def test_reference_equals_the_demo_rmsnorm_then_rope_on_fp32(grid, D):
    """fp32 CPU tensors: the demo's RMSNorm (`.type_as` is a no-op) then rope_3d, against qk_prep_reference, to 1e-5 of the token's
    largest magnitude."""
    import liteattention_amd as L
    import wan_self_attention_demo as demo
    torch.manual_seed(D + grid[2])
    B, H, S = 2, 3, grid[0] * grid[1] * grid[2]
    x = torch.randn(B, S, H * D) * (0.25 + 3.75 * torch.rand(1, 1, H * D))
    norm = demo.RMSNorm(H * D)
    with torch.no_grad():
        norm.weight.copy_(0.5 + torch.rand(H * D))
        want = demo.rope_3d(norm(x).view(B, S, H, D), grid)
    got = L.qk_prep_reference(x.view(B, S, H, D), norm.weight.detach(), norm.eps, L.rope_tables(grid, D), norm="token")
    assert got.dtype == torch.float64 and got.shape == want.shape
    scale = want.abs().amax(dim=(2, 3), keepdim=True).double()
    assert ((got - want.double()).abs() / scale).max().item() <= 1e-5


def test_reference_modes_on_cpu():
    """Head norm, no norm, no tables, partial rotary and pos_offset of the reference, against direct expressions."""
    import liteattention_amd as L
    torch.manual_seed(3)
    B, S, H, D = 1, 60, 2, 32
    x = torch.randn(B, S, H, D)
    w = 0.5 + torch.rand(D)
    got = L.qk_prep_reference(x, w, 1e-6, None, norm="head")
    want = x.double() * torch.rsqrt(x.double().pow(2).mean(-1, keepdim=True) + float(torch.tensor(1e-6))) * w.double()
    assert torch.allclose(got, want, rtol=1e-12, atol=0)
    assert torch.equal(L.qk_prep_reference(x, w, 1e-6, None, norm=None), x.double())
    tabs = L.rope_tables((3, 4, 5), D, parts=(8, 4, 4))
    full = L.qk_prep_reference(x, None, 1e-6, tabs, norm=None)
    assert torch.equal(full[..., 16:], x.double()[..., 16:])                  # pairs behind the rotated ones pass through
    assert not torch.equal(full[:, 1:, :, :16], x.double()[:, 1:, :, :16])
    part = L.qk_prep_reference(x[:, 23:40], None, 1e-6, tabs, norm=None, pos_offset=23)
    assert torch.equal(part, full[:, 23:40])
    with pytest.raises(ValueError):
        L.qk_prep_reference(x, None, 1e-6, tabs, norm=None, pos_offset=1)
