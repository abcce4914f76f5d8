"""CPU: the K-smoothing prologue (la_qk_prep_smooth, la_qk_prep_smooth_parts, la_colsum_finish) at the boundary - the symbols, the
argument struct, every validation rule in the order the header states (all of them answer before any HIP call, so no device is needed) -
and the host side of it: identities of the fp64 reference, lse_unshift, the Meta op."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from liteattention_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lite_attention_amd.h")


def test_the_entry_points_are_exported_declared_and_bound_under_abi_9():
    lib = _cabi.load()
    for name in ("la_qk_prep_smooth", "la_qk_prep_smooth_parts", "la_qk_prep_smooth_part_rows", "la_colsum_finish"):
        assert name in _cabi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.la_abi_version() == _cabi.LA_ABI_VERSION == 9
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+la_qk_prep_smooth\s*\(\s*const\s+la_qk_prep_smooth_args\s*\*", src)
    assert re.search(r"\bint\s+la_qk_prep_smooth_parts\s*\(\s*int32_t\s+seqlen\s*,\s*int32_t\s+num_heads\s*,\s*int32_t\s+head_dim\s*\)", src)
    assert re.search(r"\bint\s+la_colsum_finish\s*\(\s*const\s+float\s*\*", src)
    assert lib.la_qk_prep_smooth.argtypes[0]._type_ is _cabi.LaQkPrepSmoothArgs
    import liteattention_amd
    import lite_attention
    for name in ("qk_prep_smooth", "qk_prep_colmean", "colsum_finish", "qk_prep_smooth_parts", "qk_prep_smooth_reference", "lse_unshift",
                 "SmoothedQK"):
        assert getattr(lite_attention, name) is getattr(liteattention_amd, name)
    assert hasattr(torch.ops.lite_attention, "qk_prep_smooth")


def test_struct_layout_matches_header_and_extends_the_fp8_struct(tmp_path):
    """sizeof / offsetof of la_qk_prep_smooth_args as gcc compiles the header == the ctypes mirror; its first fields are those of
    la_qk_prep_fp8_args at the same offsets, and that struct is unchanged."""
    fields = [f[0] for f in _cabi.LaQkPrepSmoothArgs._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
            'printf("%zu\\n", sizeof(la_qk_prep_smooth_args));', 'printf("%zu\\n", sizeof(la_qk_prep_fp8_args));']
    prog += [f'printf("%zu\\n", offsetof(la_qk_prep_smooth_args, {f}));' for f in fields]
    prog += ["return 0;}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(c)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(_cabi.LaQkPrepSmoothArgs)
    assert int(out[1]) == ctypes.sizeof(_cabi.LaQkPrepFp8Args) == 208
    for f, off in zip(fields, out[2:]):
        assert getattr(_cabi.LaQkPrepSmoothArgs, f).offset == int(off), f
    old = [f[0] for f in _cabi.LaQkPrepFp8Args._fields_]
    assert fields[:len(old)] == old
    for f in old:
        assert getattr(_cabi.LaQkPrepSmoothArgs, f).offset == getattr(_cabi.LaQkPrepFp8Args, f).offset, f
    assert fields[len(old):] == ["shift", "shift_batch_stride", "shift_head_stride", "colsum_part", "dot_vec", "dot_vec_batch_stride",
                                 "dot_vec_head_stride", "dot_out", "heads_per_dot", "reserved0"]


def _valid_args(H=4, D=128, S=60, B=2, in_dtype=_cabi.LA_DTYPE_BF16, hps=1, hpd=2):
    """Arguments that pass every check, everything asked for (grid (3, 4, 5), Wan's split of D = 128); no pointer is dereferenced."""
    a = _cabi.LaQkPrepSmoothArgs()
    a.struct_size = ctypes.sizeof(_cabi.LaQkPrepSmoothArgs)
    a.in_dtype, a.norm_mode, a.heads_per_scale, a.heads_per_dot = in_dtype, _cabi.LA_NORM_TOKEN, hps, hpd
    a.x, a.out, a.weight, a.descale, a.amax = 0x10000, 0x20008, 0x30000, 0x50004, 0x60004
    a.shift, a.colsum_part, a.dot_vec, a.dot_out = 0x70000, 0x80010, 0x90000, 0xa0004
    a.x_batch_stride = a.out_batch_stride = S * H * D
    a.x_row_stride = a.out_row_stride = H * D
    a.x_head_stride = a.out_head_stride = D
    a.batch, a.seqlen, a.num_heads, a.head_dim = B, S, H, D
    a.eps, a.pos_offset = 1e-6, 0
    a.descale_batch_stride = a.amax_batch_stride = H // hps
    a.descale_head_stride = a.amax_head_stride = 1
    a.shift_batch_stride, a.shift_head_stride = H * D, D
    a.dot_vec_batch_stride, a.dot_vec_head_stride = H // hpd * D, D
    for i, (e, n) in enumerate(zip((3, 4, 5), (22, 21, 21))):
        a.rope_table[i], a.axis_extent[i], a.axis_pairs[i] = 0x40000 + 0x1000 * i, e, n
    return a


def _rc(a):
    return _cabi.load().la_qk_prep_smooth(ctypes.byref(a), None)


PLANTED = _cabi.LA_ERR_SHAPE      # pos_offset = 1: 1 + 60 rows > 3 * 4 * 5 positions, the last of the checks shared with la_qk_prep


def _first_failing_check(**changes):
    """The code la_qk_prep_smooth answers for arguments that are valid but for the complaint planted in that check and `changes`."""
    a = _valid_args()
    a.pos_offset = 1
    for k, v in changes.items():
        setattr(a, k, v)
    return _rc(a)


def test_every_error_in_the_order_of_the_header():
    """Each line breaks one rule and, with it, every LATER rule that can be broken independently; the answer is the earlier one's."""
    E = _cabi
    size = ctypes.sizeof(_cabi.LaQkPrepSmoothArgs)
    assert _first_failing_check() == PLANTED
    assert _cabi.load().la_qk_prep_smooth(None, None) == E.LA_ERR_NULL_ARG
    assert _first_failing_check(struct_size=size - 8, x=None) == E.LA_ERR_STRUCT_SIZE
    assert _first_failing_check(struct_size=ctypes.sizeof(_cabi.LaQkPrepFp8Args)) == E.LA_ERR_STRUCT_SIZE
    assert _first_failing_check(x=None, in_dtype=7) == E.LA_ERR_NULL_ARG
    assert _first_failing_check(out=None, amax=None, colsum_part=None, dot_out=None, dot_vec=None, in_dtype=7) == E.LA_ERR_NULL_ARG
    assert _first_failing_check(dot_out=None, in_dtype=7) == E.LA_ERR_NULL_ARG            # dot_vec without dot_out
    assert _first_failing_check(dot_vec=None, in_dtype=7) == E.LA_ERR_NULL_ARG            # dot_out without dot_vec
    assert _first_failing_check(in_dtype=7, heads_per_scale=3) == E.LA_ERR_DTYPE
    assert _first_failing_check(in_dtype=E.LA_DTYPE_FP8_E4M3) == E.LA_ERR_DTYPE
    assert _first_failing_check(heads_per_scale=3, amax_head_stride=-1) == E.LA_ERR_SHAPE
    assert _first_failing_check(heads_per_scale=0) == E.LA_ERR_SHAPE
    assert _first_failing_check(heads_per_dot=3, amax_head_stride=-1) == E.LA_ERR_SHAPE
    assert _first_failing_check(heads_per_dot=0) == E.LA_ERR_SHAPE
    assert _first_failing_check(heads_per_dot=0, dot_vec=None, dot_out=None) == PLANTED   # ... only read with dot_vec
    for field in ("descale_batch_stride", "descale_head_stride", "amax_batch_stride", "amax_head_stride", "shift_batch_stride",
                  "shift_head_stride", "dot_vec_batch_stride", "dot_vec_head_stride"):
        assert _first_failing_check(**{field: -4}, norm_mode=3) == E.LA_ERR_STRIDE, field
    for field, ptr in (("descale", 0x50002), ("amax", 0x60001), ("dot_out", 0xa0002), ("shift", 0x70008), ("dot_vec", 0x90004),
                       ("colsum_part", 0x80008)):
        assert _first_failing_check(**{field: ptr}, norm_mode=3) == E.LA_ERR_STRIDE, field
    assert _first_failing_check(shift_head_stride=130) == E.LA_ERR_STRIDE                  # a shift row off 16 bytes
    assert _first_failing_check(shift_batch_stride=4 * 128 + 2) == E.LA_ERR_STRIDE
    assert _first_failing_check(shift_batch_stride=4 * 128 + 2, batch=1) == PLANTED        # an unused stride is free
    assert _first_failing_check(dot_vec_head_stride=130) == E.LA_ERR_STRIDE
    assert _first_failing_check(dot_vec_head_stride=130, heads_per_dot=4) == PLANTED       # one group: its stride is unused
    assert _first_failing_check(shift_head_stride=0, dot_vec_batch_stride=0) == PLANTED    # a broadcast vector is a stride of 0
    assert _first_failing_check(norm_mode=3, head_dim=100) == E.LA_ERR_UNSUPPORTED         # from here on: la_qk_prep_fp8's own order
    assert _first_failing_check(seqlen=0, head_dim=100) == E.LA_ERR_SHAPE
    assert _first_failing_check(head_dim=100) == E.LA_ERR_HEAD_DIM
    assert _first_failing_check(out=0x20004) == E.LA_ERR_STRIDE
    assert _first_failing_check(x_row_stride=4 * 128 + 4) == E.LA_ERR_STRIDE
    a = _valid_args()
    a.rope_table[1] = None
    assert _rc(a) == E.LA_ERR_NULL_ARG


def test_what_may_be_left_out():
    assert _first_failing_check(out=None) == PLANTED                                       # nothing stored: sums, dots and amax
    assert _first_failing_check(out=None, amax=None, dot_vec=None, dot_out=None) == PLANTED        # the sums-only pass
    assert _first_failing_check(out=None, amax=None, colsum_part=None) == PLANTED          # the dots-only pass
    assert _first_failing_check(out=None, colsum_part=None, dot_vec=None, dot_out=None, shift=None) == PLANTED     # the amax pass
    assert _first_failing_check(shift=None, colsum_part=None, dot_vec=None, dot_out=None) == PLANTED       # la_qk_prep_fp8 itself
    assert _first_failing_check(descale=None, amax=None) == PLANTED


def test_the_column_sums_have_a_limit_behind_the_shared_checks():
    """Token norm serves every H * D it accepts; the head kernel keeps sums for 16 * (64 / G) heads: 64 heads of 128, 32 of 256."""
    E = _cabi
    for H, D, mode, rc in ((64, 256, E.LA_NORM_TOKEN, E.LA_OK), (64, 128, E.LA_NORM_HEAD, E.LA_OK), (65, 128, E.LA_NORM_HEAD, E.LA_ERR_UNSUPPORTED),
                           (32, 256, E.LA_NORM_NONE, E.LA_OK), (33, 256, E.LA_NORM_NONE, E.LA_ERR_UNSUPPORTED)):
        a = _valid_args(H=H, D=D, hpd=1)
        a.norm_mode = mode
        if D == 256:
            a.axis_pairs[0], a.axis_pairs[1], a.axis_pairs[2] = 44, 42, 42
        a.pos_offset = 1
        assert _rc(a) == PLANTED, (H, D)                                               # the shared checks come first
        if rc != E.LA_OK:
            a.pos_offset = 0
            assert _rc(a) == rc, (H, D)
            a.colsum_part = None                                                       # without the sums the shape is served: the refusal
            a.pos_offset = 1                                                           # was about them
            assert _rc(a) == PLANTED
    a = _valid_args(H=1025, D=8)
    a.norm_mode = E.LA_NORM_HEAD
    a.heads_per_dot = 1
    a.dot_vec_batch_stride = 1025 * 8
    a.axis_pairs[0], a.axis_pairs[1], a.axis_pairs[2] = 2, 1, 1
    assert _rc(a) == E.LA_ERR_UNSUPPORTED                                              # more than 1024 heads


def test_parts_are_a_pure_function_of_the_shape():
    lib = _cabi.load()
    seen = {}
    for _ in range(2):
        for S in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 600, 16384, 16385, 75600, 2 ** 31 - 1):
            for H, D in ((1, 8), (40, 128), (64, 256)):
                n, r = lib.la_qk_prep_smooth_parts(S, H, D), lib.la_qk_prep_smooth_part_rows(S, H, D)
                assert seen.setdefault((S, H, D), (n, r)) == (n, r)
                assert n > 0 and n % 4 == 0 and r >= 1 and n * r >= S and (n - 4) * r < S     # covers S, no block of 4 parts to spare
    assert seen[(600, 40, 128)] == (40, 16) and seen[(75600, 40, 128)] == (1024, 74)
    for bad in ((0, 1, 8), (5, 0, 8), (5, 1, 0), (-1, 1, 8)):
        assert lib.la_qk_prep_smooth_parts(*bad) == _cabi.LA_ERR_SHAPE and lib.la_qk_prep_smooth_part_rows(*bad) == _cabi.LA_ERR_SHAPE
    import liteattention_amd as L
    assert L.qk_prep_smooth_parts(600, 40, 128) == (40, 16)


def test_colsum_finish_rules():
    lib, E = _cabi.load(), _cabi
    ok = [0x10000, 8, 2, 4, 128, 60, 0x20000, 4 * 128, 128, None]

    def rc(**ch):
        args = list(ok)
        for k, v in ch.items():
            args[["part", "n_parts", "batch", "num_heads", "head_dim", "seqlen", "mean", "bs", "hs"].index(k)] = v
        return lib.la_colsum_finish(*args)

    assert rc(part=None) == E.LA_ERR_NULL_ARG and rc(mean=None) == E.LA_ERR_NULL_ARG
    for k in ("n_parts", "batch", "num_heads", "head_dim", "seqlen"):
        assert rc(**{k: 0}) == E.LA_ERR_SHAPE, k
    assert rc(bs=-1) == E.LA_ERR_STRIDE and rc(hs=-1) == E.LA_ERR_STRIDE
    assert rc(part=0x10002) == E.LA_ERR_STRIDE and rc(mean=0x20001) == E.LA_ERR_STRIDE


# ---- the host side ----------------------------------------------------------------------------------------------------------------------
def _inputs():
    import liteattention_amd as L
    torch.manual_seed(3)
    B, S, H, D = 2, 60, 4, 32
    x = torch.randn(B, S, H, D) + 3.0 * torch.randn(1, 1, H, D)
    return x, 0.5 + torch.rand(H * D), L.rope_tables((3, 4, 5), D)


def test_reference_without_a_shift_is_the_fp8_reference():
    import liteattention_amd as L
    x, w, tabs = _inputs()
    d = 0.01 + torch.rand(2, 2)
    z0, a0 = L.qk_prep_fp8_reference(x, w, 1e-6, tabs, descale=d, heads_per_scale=2)
    for shift in (None, torch.zeros(2, 4, 32)):
        z, a, mean, dots = L.qk_prep_smooth_reference(x, w, 1e-6, tabs, shift=shift, descale=d, heads_per_scale=2)
        assert torch.equal(z, z0) and torch.equal(a, a0) and dots is None
        assert z.dtype == a.dtype == mean.dtype == torch.float64 and mean.shape == (2, 4, 32)


def test_reference_mean_of_the_shifted_values_is_zero_and_the_amax_is_theirs():
    import liteattention_amd as L
    x, w, tabs = _inputs()
    y = L.qk_prep_reference(x, w, 1e-6, tabs)
    _, _, mean, _ = L.qk_prep_smooth_reference(x, w, 1e-6, tabs)
    assert torch.allclose(mean, y.mean(1), rtol=0, atol=1e-15)
    z, amax, mean2, _ = L.qk_prep_smooth_reference(x, w, 1e-6, tabs, shift=mean)
    assert z.mean(1).abs().max().item() <= 1e-14                      # (the shift handed over in fp64: nothing but fp64 rounding)
    assert torch.equal(mean2, mean)                                   # the mean is of the UNSHIFTED y
    assert torch.equal(amax, (y - mean[:, None]).abs().amax(dim=(1, 3)))


def test_reference_dots_against_an_einsum_with_grouped_heads():
    import liteattention_amd as L
    x, w, tabs = _inputs()
    y = L.qk_prep_reference(x, w, 1e-6, tabs)
    c = torch.randn(2, 2, 32)
    _, _, _, dots = L.qk_prep_smooth_reference(x, w, 1e-6, tabs, dot_vec=c, heads_per_dot=2, shift=torch.randn(2, 4, 32))
    want = torch.einsum("bshd,bhd->bhs", y, c.double()[:, [0, 0, 1, 1]])
    assert dots.shape == (2, 4, 60) and torch.allclose(dots, want, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        L.qk_prep_smooth_reference(x, w, 1e-6, tabs, dot_vec=c, heads_per_dot=3)


def test_shifting_the_keys_moves_the_lse_by_the_dot_and_nothing_else():
    """The identity the feature rests on, in fp64: softmax(q (k - c)) = softmax(q k), and lse_unshift restores the LSE."""
    import liteattention_amd as L
    torch.manual_seed(5)
    q, k, v = (torch.randn(1, 40, 2, 16, dtype=torch.float64) for _ in range(3))
    c = 4.0 * torch.randn(1, 2, 16, dtype=torch.float64)
    scale = 0.25

    def attention(kk):
        s = torch.einsum("bqhd,bkhd->bhqk", q, kk) * scale
        return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v), torch.logsumexp(s, -1)

    o, lse = attention(k)
    o2, lse2 = attention(k - c[:, None])
    dot = torch.einsum("bshd,bhd->bhs", q, c)
    assert torch.allclose(o2, o, rtol=0, atol=1e-12)
    assert (lse2 - lse).abs().max().item() > 1.0
    assert torch.allclose(L.lse_unshift(lse2, dot, scale), lse, rtol=0, atol=1e-12)
    out = torch.empty_like(lse)
    assert L.lse_unshift(lse2, dot, scale, out=out).data_ptr() == out.data_ptr() and torch.allclose(out, lse, rtol=0, atol=1e-12)


def test_the_functions_refuse_cpu_tensors_and_bad_arguments():
    import liteattention_amd as L
    x = torch.zeros(1, 4, 4, 16)
    with pytest.raises(ValueError, match="GPU"):
        L.qk_prep_smooth(x)
    with pytest.raises(ValueError, match="GPU"):
        L.colsum_finish(torch.zeros(4, 1, 4, 16), 4)
    with pytest.raises(ValueError):
        L.qk_prep_smooth(x, quantize=False, out=torch.zeros(1, 4, 4, 16, dtype=torch.float8_e4m3fn))
    with pytest.raises(ValueError):
        L.SmoothedQK(mode="static")
    with pytest.raises(ValueError):
        L.SmoothedQK(margin=0.0)


def test_meta_op_gives_shape_and_dtype_only():
    x = torch.empty(2, 60, 4, 128, dtype=torch.bfloat16, device="meta")
    got = torch.ops.lite_attention.qk_prep_smooth(x)
    assert got.shape == x.shape and got.dtype == torch.float8_e4m3fn and got.device.type == "meta"
