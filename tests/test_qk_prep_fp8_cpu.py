"""CPU: the e4m3 q / k / v prologue (la_qk_prep_fp8) at the boundary - the symbol, the argument struct, every validation rule (all of
them answer before any HIP call, so no device is needed) - and the host side of it: the fp64 reference against hand values, the
descale formula, the bookkeeping of E4m3Scales on CPU tensors and the Meta op."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from liteattention_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lite_attention_amd.h")


def test_la_qk_prep_fp8_is_exported_declared_and_bound_under_abi_9():
    lib = _cabi.load()
    assert "la_qk_prep_fp8" in _cabi.EXPORTED_SYMBOLS and hasattr(lib, "la_qk_prep_fp8")
    assert lib.la_abi_version() == _cabi.LA_ABI_VERSION == 9
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+la_qk_prep_fp8\s*\(\s*const\s+la_qk_prep_fp8_args\s*\*", src)
    assert re.search(r"#define\s+LA_ABI_VERSION\s+9\b", src)
    assert lib.la_qk_prep_fp8.argtypes[0]._type_ is _cabi.LaQkPrepFp8Args
    import liteattention_amd
    import lite_attention
    for name in ("qk_prep_fp8", "qk_prep_amax", "descale_from_amax", "qk_prep_fp8_reference", "E4m3Scales"):
        assert getattr(lite_attention, name) is getattr(liteattention_amd, name)
    assert hasattr(torch.ops.lite_attention, "qk_prep_fp8") and hasattr(torch.ops.lite_attention, "qk_prep")


def test_qk_prep_fp8_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of la_qk_prep_fp8_args as gcc compiles the header == the ctypes mirror; la_qk_prep_args has every field of it
    but the scale fields, and out_dtype instead of heads_per_scale."""
    fields = [f[0] for f in _cabi.LaQkPrepFp8Args._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
            'printf("%zu\\n", sizeof(la_qk_prep_fp8_args));']
    prog += [f'printf("%zu\\n", offsetof(la_qk_prep_fp8_args, {f}));' for f in fields]
    prog += ["return 0;}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(c)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(_cabi.LaQkPrepFp8Args)
    for f, off in zip(fields, out[1:]):
        assert getattr(_cabi.LaQkPrepFp8Args, f).offset == int(off), f
    old = {f[0] for f in _cabi.LaQkPrepArgs._fields_}
    new = set(fields)
    assert old - new == {"out_dtype"}
    assert new - old == {"heads_per_scale", "descale", "descale_batch_stride", "descale_head_stride", "amax", "amax_batch_stride",
                         "amax_head_stride"}


def _valid_args(H=4, D=128, S=60, B=2, in_dtype=_cabi.LA_DTYPE_BF16, hps=1):
    """Arguments that pass every check (grid (3, 4, 5), Wan's split of D = 128); pointers are never dereferenced on the host."""
    a = _cabi.LaQkPrepFp8Args()
    a.struct_size = ctypes.sizeof(_cabi.LaQkPrepFp8Args)
    a.in_dtype, a.norm_mode, a.heads_per_scale = in_dtype, _cabi.LA_NORM_TOKEN, hps
    a.x, a.out, a.weight, a.descale, a.amax = 0x10000, 0x20008, 0x30000, 0x50004, 0x60004      # out on 8 bytes, the scales on 4
    a.x_batch_stride = a.out_batch_stride = S * H * D
    a.x_row_stride = a.out_row_stride = H * D
    a.x_head_stride = a.out_head_stride = D
    a.batch, a.seqlen, a.num_heads, a.head_dim = B, S, H, D
    a.eps, a.pos_offset = 1e-6, 0
    a.descale_batch_stride = a.amax_batch_stride = H // hps
    a.descale_head_stride = a.amax_head_stride = 1
    for i, (e, n) in enumerate(zip((3, 4, 5), (22, 21, 21))):
        a.rope_table[i], a.axis_extent[i], a.axis_pairs[i] = 0x40000 + 0x1000 * i, e, n
    return a


def _rc(a):
    return _cabi.load().la_qk_prep_fp8(ctypes.byref(a), None)


PLANTED = _cabi.LA_ERR_SHAPE      # pos_offset = 1: 1 + 60 rows > 3 * 4 * 5 positions, the LAST check - "accepted up to there"


def _first_failing_check(**changes):
    """The code la_qk_prep_fp8 answers for arguments that are valid but for the complaint planted in the last check and `changes`."""
    a = _valid_args()
    a.pos_offset = 1
    for k, v in changes.items():
        setattr(a, k, v)
    return _rc(a)


def test_the_valid_arguments_reach_the_last_check():
    assert _first_failing_check() == PLANTED
    assert _first_failing_check(pos_offset=-1) == _cabi.LA_ERR_SHAPE


def test_null_args_struct_size_and_null_tensors():
    lib = _cabi.load()
    assert lib.la_qk_prep_fp8(None, None) == _cabi.LA_ERR_NULL_ARG
    assert _first_failing_check(struct_size=ctypes.sizeof(_cabi.LaQkPrepFp8Args) - 8) == _cabi.LA_ERR_STRUCT_SIZE
    assert _first_failing_check(struct_size=ctypes.sizeof(_cabi.LaQkPrepArgs)) == _cabi.LA_ERR_STRUCT_SIZE
    assert _first_failing_check(x=None) == _cabi.LA_ERR_NULL_ARG
    assert _first_failing_check(out=None, amax=None) == _cabi.LA_ERR_NULL_ARG
    assert _first_failing_check(out=None) == PLANTED                     # the amax pass alone
    assert _first_failing_check(amax=None) == PLANTED                    # quantizing without an amax
    assert _first_failing_check(descale=None) == PLANTED                 # descale NULL reads as 1.0
    assert _first_failing_check(out=None, out_row_stride=3) == PLANTED   # ... and no out, no out rules


def test_dtype_and_norm_mode():
    assert _first_failing_check(in_dtype=_cabi.LA_DTYPE_FP8_E4M3) == _cabi.LA_ERR_DTYPE
    assert _first_failing_check(in_dtype=7) == _cabi.LA_ERR_DTYPE
    for dt in (_cabi.LA_DTYPE_FP16, _cabi.LA_DTYPE_FP32):
        assert _first_failing_check(in_dtype=dt) == PLANTED
    assert _first_failing_check(norm_mode=3) == _cabi.LA_ERR_UNSUPPORTED
    assert _first_failing_check(norm_mode=_cabi.LA_NORM_NONE) == PLANTED
    assert _first_failing_check(norm_mode=_cabi.LA_NORM_HEAD) == PLANTED


def test_la_qk_prep_itself_still_refuses_an_e4m3_out_dtype():
    a = _cabi.LaQkPrepArgs()
    a.struct_size = ctypes.sizeof(_cabi.LaQkPrepArgs)
    a.in_dtype, a.out_dtype, a.norm_mode = _cabi.LA_DTYPE_BF16, _cabi.LA_DTYPE_FP8_E4M3, _cabi.LA_NORM_TOKEN
    a.x, a.out = 0x10000, 0x20000
    assert _cabi.load().la_qk_prep(ctypes.byref(a), None) == _cabi.LA_ERR_DTYPE


@pytest.mark.parametrize("field", ["batch", "seqlen", "num_heads", "head_dim"])
def test_non_positive_sizes(field):
    assert _first_failing_check(**{field: 0}) == _cabi.LA_ERR_SHAPE
    assert _first_failing_check(**{field: -1}) == _cabi.LA_ERR_SHAPE


def test_head_dim_and_token_limit_rules_are_those_of_la_qk_prep():
    assert _first_failing_check(head_dim=100) == _cabi.LA_ERR_HEAD_DIM
    assert _first_failing_check(head_dim=264) == _cabi.LA_ERR_HEAD_DIM
    a = _valid_args(H=64, D=256)
    a.pos_offset = 1
    assert _rc(a) == PLANTED                                             # H * D = 16384 is accepted
    a = _valid_args(H=65, D=256)
    a.pos_offset = 1
    assert _rc(a) == _cabi.LA_ERR_UNSUPPORTED


def test_heads_per_scale_rules():
    for hps in (1, 2, 4):
        assert _first_failing_check(heads_per_scale=hps) == PLANTED
    for hps in (0, -1, 3, 8):                                            # below 1, not a divisor of the 4 heads
        assert _first_failing_check(heads_per_scale=hps) == _cabi.LA_ERR_SHAPE, hps
    a = _valid_args(H=6, hps=3)
    a.pos_offset = 1
    assert _rc(a) == PLANTED


def test_more_heads_than_a_workgroup_keeps_scales_for():
    """1024 heads is the limit (a workgroup keeps every head's scale and running maximum in LDS). The refusal comes BEHIND the checks
    shared with la_qk_prep, so the accepting side cannot be shown by a planted complaint here: tests/test_gpu_qk_prep_fp8.py launches
    it."""
    a = _valid_args(H=1025, D=8)
    a.norm_mode = _cabi.LA_NORM_HEAD
    a.axis_pairs[0], a.axis_pairs[1], a.axis_pairs[2] = 2, 1, 1
    assert _rc(a) == _cabi.LA_ERR_UNSUPPORTED
    a.pos_offset = 1
    assert _rc(a) == PLANTED                                             # (the common checks come first)


def test_out_alignment_is_eight_bytes():
    H, D = 4, 128
    assert _first_failing_check(out=0x20010) == PLANTED
    assert _first_failing_check(out=0x20004) == _cabi.LA_ERR_STRIDE       # pointer off an 8-byte boundary
    assert _first_failing_check(out_row_stride=H * D + 8) == PLANTED
    assert _first_failing_check(out_row_stride=H * D + 4) == _cabi.LA_ERR_STRIDE
    assert _first_failing_check(out_head_stride=D + 4) == _cabi.LA_ERR_STRIDE
    assert _first_failing_check(out_batch_stride=60 * H * D + 2) == _cabi.LA_ERR_STRIDE
    assert _first_failing_check(out_batch_stride=60 * H * D + 2, batch=1) == PLANTED           # an unused stride is free
    assert _first_failing_check(out_row_stride=-H * D) == _cabi.LA_ERR_STRIDE


def test_x_alignment_rules_are_unchanged():
    H, D = 4, 128
    assert _first_failing_check(x=0x10008) == _cabi.LA_ERR_STRIDE         # 16 bytes for x
    assert _first_failing_check(x_row_stride=H * D + 4) == _cabi.LA_ERR_STRIDE
    assert _first_failing_check(x_head_stride=D + 4) == _cabi.LA_ERR_STRIDE
    assert _first_failing_check(x_batch_stride=-1) == _cabi.LA_ERR_STRIDE
    assert _first_failing_check(in_dtype=_cabi.LA_DTYPE_FP32, x_row_stride=H * D + 4, x_batch_stride=60 * (H * D + 4)) == PLANTED
    assert _first_failing_check(weight=0x30004) == _cabi.LA_ERR_STRIDE
    a = _valid_args()
    a.rope_table[1] = 0x41004
    assert _rc(a) == _cabi.LA_ERR_STRIDE


@pytest.mark.parametrize("field", ["descale_batch_stride", "descale_head_stride", "amax_batch_stride", "amax_head_stride"])
def test_scale_strides(field):
    assert _first_failing_check(**{field: -1}) == _cabi.LA_ERR_STRIDE
    assert _first_failing_check(**{field: 0}) == PLANTED                 # a broadcast scale is a stride of 0
    assert _first_failing_check(**{field: 12345}) == PLANTED


def test_scale_pointers_are_fp32_aligned():
    assert _first_failing_check(descale=0x50002) == _cabi.LA_ERR_STRIDE
    assert _first_failing_check(amax=0x60001) == _cabi.LA_ERR_STRIDE


def test_table_and_position_rules():
    a = _valid_args()
    a.rope_table[1] = None
    assert _rc(a) == _cabi.LA_ERR_NULL_ARG
    a = _valid_args()
    a.axis_pairs[2] = 22
    assert _rc(a) == _cabi.LA_ERR_SHAPE
    a = _valid_args()
    a.axis_extent[1] = 0
    assert _rc(a) == _cabi.LA_ERR_SHAPE


# ---- the host side ----------------------------------------------------------------------------------------------------------------------
def test_reference_against_hand_values():
    """One token, two heads of 8, no norm, no tables: y = x. Head 0 holds 3 and -5, head 1 holds 0.5 and 2000."""
    import liteattention_amd as L
    x = torch.zeros(1, 1, 2, 8)
    x[0, 0, 0, 0], x[0, 0, 0, 3] = 3.0, -5.0
    x[0, 0, 1, 1], x[0, 0, 1, 7] = 0.5, 2000.0
    z, amax = L.qk_prep_fp8_reference(x, norm=None)
    assert z.dtype == torch.float64 and amax.dtype == torch.float64
    assert amax.tolist() == [[5.0, 2000.0]]
    assert z[0, 0, 0].tolist() == [3.0, 0, 0, -5.0, 0, 0, 0, 0] and z[0, 0, 1].tolist() == [0, 0.5, 0, 0, 0, 0, 0, 448.0]
    d = torch.tensor([[0.25, 8.0]])
    z, amax = L.qk_prep_fp8_reference(x, norm=None, descale=d)
    assert amax.tolist() == [[5.0, 2000.0]]                               # of the unscaled y
    assert z[0, 0, 0].tolist() == [12.0, 0, 0, -20.0, 0, 0, 0, 0] and z[0, 0, 1].tolist() == [0, 0.0625, 0, 0, 0, 0, 0, 250.0]
    z, amax = L.qk_prep_fp8_reference(x, norm=None, descale=torch.tensor([[2.0]]), heads_per_scale=2)
    assert amax.tolist() == [[2000.0]] and z[0, 0, 0, 3].item() == -2.5 and z[0, 0, 1, 7].item() == 448.0
    with pytest.raises(ValueError):
        L.qk_prep_fp8_reference(torch.zeros(1, 1, 3, 8), norm=None, heads_per_scale=2)
    x[0, 0, 1, 2] = float("nan")
    z, amax = L.qk_prep_fp8_reference(x, norm=None)
    assert amax[0, 0].item() == 5.0 and amax[0, 1].isnan() and z[0, 0, 1, 2].isnan() and z.isnan().sum().item() == 1


def test_reference_is_the_bf16_reference_scaled():
    import liteattention_amd as L
    torch.manual_seed(1)
    B, S, H, D = 2, 60, 4, 32
    x = torch.randn(B, S, H, D)
    w = 0.5 + torch.rand(H * D)
    tabs = L.rope_tables((3, 4, 5), D)
    d = 0.01 + torch.rand(B, 2)
    z, amax = L.qk_prep_fp8_reference(x, w, 1e-6, tabs, descale=d, heads_per_scale=2)
    y = L.qk_prep_reference(x, w, 1e-6, tabs)
    for b in range(B):
        for g in range(2):
            ys = y[b, :, 2 * g:2 * g + 2]
            assert amax[b, g].item() == ys.abs().max().item()
            assert torch.equal(z[b, :, 2 * g:2 * g + 2], (ys / d[b, g].double()).clamp(-448, 448))


def test_descale_from_amax():
    """`tiny` = 2^-100: an amax of 0 (an all-zero head) still gives a descale whose reciprocal, 448 x 2^100, is finite in fp32 - 0 times
    it is 0, not NaN."""
    import liteattention_amd as L
    tiny = 2.0 ** -100
    amax = torch.tensor([[448.0, 1.0, 0.0], [3.5, float("nan"), 1e-45]])
    d = L.descale_from_amax(amax)
    assert d.dtype == torch.float32 and d.shape == amax.shape
    assert d[0, 0].item() == 1.0 and d[0, 1].item() == torch.tensor(1.0).div(448.0).item()
    assert d[0, 2].item() == d[1, 2].item() == torch.tensor(tiny).div(448.0).item() and d[0, 2].item() > 0
    assert torch.isfinite(1.0 / d[0, 2]) and (0.0 * (1.0 / d[0, 2])).item() == 0.0
    assert d[1, 1].isnan()
    out = torch.empty_like(amax)
    d2 = L.descale_from_amax(amax, margin=1.25, out=out)
    assert d2.data_ptr() == out.data_ptr()
    assert torch.equal(out[0], amax[0].clamp_min(tiny) * 1.25 / 448.0)
    assert amax[0, 2].item() == 0.0                                       # the input is left alone


def _CpuScales(*args, **kwargs):
    """E4m3Scales with the two passes replaced by the fp64 reference on CPU tensors, and a log of what was called."""
    import liteattention_amd as L
    log = []

    def amax_pass(x, weight=None, eps=1e-6, tables=None, norm="token", pos_offset=0, *, amax_out, heads_per_scale=1):
        _, am = L.qk_prep_fp8_reference(x, weight, eps, tables, norm, pos_offset, heads_per_scale=heads_per_scale)
        amax_out.copy_(torch.maximum(amax_out, am.float()))
        log.append("amax")

    def quant_pass(x, weight=None, eps=1e-6, tables=None, norm="token", pos_offset=0, *, descale, amax_out, heads_per_scale, out):
        z, am = L.qk_prep_fp8_reference(x, weight, eps, tables, norm, pos_offset, descale=descale, heads_per_scale=heads_per_scale)
        out.copy_(z.float().to(torch.float8_e4m3fn))
        if amax_out is not None:
            amax_out.copy_(torch.maximum(amax_out, am.float()))
        log.append("quant+amax" if amax_out is not None else "quant")

    sub = type("CpuE4m3Scales", (L.E4m3Scales,), {"_amax_pass": staticmethod(amax_pass), "_quant_pass": staticmethod(quant_pass)})
    obj = sub(*args, **kwargs)
    obj.log = log
    return obj


def test_e4m3_scales_current_mode_bookkeeping():
    torch.manual_seed(0)
    s = _CpuScales(mode="current", margin=1.0)
    x0, x1 = torch.randn(2, 8, 4, 16), 7.0 * torch.randn(2, 8, 4, 16)
    out0, d0 = s(x0, norm=None)
    assert out0.dtype == torch.float8_e4m3fn and out0.shape == x0.shape and d0.shape == (2, 4)
    am0 = x0.abs().amax(dim=(1, 3))
    assert torch.equal(s.amax, am0) and torch.equal(d0, am0 / 448.0)
    assert out0.float().abs().amax(dim=(1, 3)).eq(448.0).all()           # the largest element of every (batch, head) lands on 448
    ptrs = (s.amax.data_ptr(), s.descale.data_ptr(), s.out.data_ptr())
    out1, d1 = s(x1, norm=None)
    assert (s.amax.data_ptr(), s.descale.data_ptr(), s.out.data_ptr()) == ptrs == (s.amax.data_ptr(), d1.data_ptr(), out1.data_ptr())
    assert torch.equal(d1, x1.abs().amax(dim=(1, 3)) / 448.0)             # a fresh amax every call, not a running one
    assert s.log == ["amax", "quant", "amax", "quant"] and s.calls == 2


def test_e4m3_scales_delayed_mode_uses_the_previous_steps_amax():
    torch.manual_seed(0)
    s = _CpuScales(mode="delayed", margin=1.25, heads_per_scale=2)
    base = torch.randn(1, 8, 4, 16)
    xs = [base * f for f in (4.0, 2.0, 3.0)]
    am = [x.abs().reshape(1, 8, 2, 32).amax(dim=(1, 3)) for x in xs]
    tiny = 2.0 ** -100
    want_d = [am[0], am[0], am[1]]                                        # step 0 has no history: its own amax
    for t, x in enumerate(xs):
        out, d = s(x, norm=None)
        assert d.shape == (1, 2)
        assert torch.equal(d, want_d[t].clamp_min(tiny) * 1.25 / 448.0), t
        assert torch.equal(s.amax, am[t]), t                              # this step's amax, for the next step
        z = (x.double() / d.double().repeat_interleave(2, 1)[:, None, :, None]).clamp(-448, 448)
        assert torch.equal(out.float(), z.float().to(torch.float8_e4m3fn).float()), t
    assert s.log == ["amax", "quant+amax", "quant+amax", "quant+amax"]
    assert out.float().abs().max().item() == 448.0                        # step 2 grew 1.5 x over step 1: above the margin, it saturates


def test_e4m3_scales_refuses_unknown_modes():
    import liteattention_amd as L
    with pytest.raises(ValueError):
        L.E4m3Scales(mode="static")
    with pytest.raises(ValueError):
        L.E4m3Scales(margin=0.0)


def test_the_functions_refuse_cpu_tensors_and_bad_groups():
    import liteattention_amd as L
    x = torch.zeros(1, 4, 4, 16)
    with pytest.raises(ValueError, match="GPU"):
        L.qk_prep_fp8(x)
    with pytest.raises(ValueError, match="GPU"):
        L.qk_prep_amax(x)


def test_meta_op_gives_shape_and_dtype_only():
    x = torch.empty(2, 60, 4, 128, dtype=torch.bfloat16, device="meta")
    got = torch.ops.lite_attention.qk_prep_fp8(x, None, 1e-6, None, None, "token", 0, None, None, 1, None)
    assert got.shape == x.shape and got.dtype == torch.float8_e4m3fn and got.device.type == "meta"
    out = torch.empty(2, 60, 4, 128, dtype=torch.float8_e4m3fn, device="meta")
    got = torch.ops.lite_attention.qk_prep_fp8(x, None, 1e-6, None, None, None, 0, None, None, 2, out)
    assert got.shape == out.shape and got.dtype == torch.float8_e4m3fn and got.device.type == "meta"
