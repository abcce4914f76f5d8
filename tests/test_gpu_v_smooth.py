"""GPU: V smoothing - la_v_colstats + la_v_colstats_finish against `v_colstats_reference` and, bit for bit, against the amax pass of
la_qk_prep_smooth; la_attn_unshift against `attn_unshift_reference`; and the whole path through the e4m3 forward.

Acceptance rules:

    min / max   exact (they are values of x).
    mean        |mean - mean64| <= (R + n_parts + 1) 2^-24 mean_s |x|  per column: a part adds R values in sequence, the finish n_parts
                partial sums, then one division - the bound of the two-level recursive sum.
    amax        the bits of qk_prep_smooth(x, norm=None, shift=mean, amax_out=zeros, quantize=False).
    unshift     fp32 out: within one fp32 ulp of the fp64 value. 16-bit out: the fp64 value rounded to the type, except where that value
                lies within one fp32 ulp of the midpoint of two neighbours of the type (the kernel rounds the fp32 sum).
    fused LSE   within one fp32 ulp of lse_unshift.
    end to end  the ratio (error with SmoothedV) / (error with E4m3Scales) of the relative rms error of O against fp64 is below
                min(1, 1.25 x the ratio of tests/v_smooth_emulation.py) at offset 16 and below 1.10 at offset 0; 25 % for the device's own
                exp and accumulation order, which the emulation does not model."""
import os
import sys

import pytest
import torch

import v_smooth_emulation as emu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
BF, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32


def bits(t):
    return t.contiguous().view(torch.int32)


def make_v(B, S, H, D, dtype=BF, seed=0):
    """N(0, 1) times a per-head scale in [0.25, 4] plus a per-column offset in [-8, 8]: a wrong row, head or column index shows."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, H, D, generator=g) * (0.25 + 3.75 * torch.rand(1, 1, H, 1, generator=g))
    x = x + 16.0 * (torch.rand(B, 1, H, D, generator=g) - 0.5)
    return x.to(dtype).cuda()


def ulp32(ref64):
    """The spacing of fp32 at |ref| (fp64 tensor)."""
    a = ref64.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


# ---- v_colstats ------------------------------------------------------------------------------------------------------------------------
def check_colstats(x, label=""):
    """Everything the module docstring asks of one launch; returns (mean, amax, stat_part)."""
    import liteattention_amd as L
    B, S, H, D = x.shape
    n_parts, R = L.v_colstats_parts(S, H, D)
    part = torch.full((n_parts, 3, B, H, D), float("nan"), device="cuda")
    mean, amax = L.v_colstats(x, stat_part=part)
    assert mean.shape == (B, H, D) and amax.shape == (B, H) and mean.dtype == amax.dtype == FP32
    assert not part.isnan().any(), label                                              # every element is written
    xf = x.float()
    pad = n_parts * R - S
    lo = torch.cat((xf, torch.full((B, pad, H, D), float("inf"), device="cuda")), 1).reshape(B, n_parts, R, H, D).amin(2)
    hi = torch.cat((xf, torch.full((B, pad, H, D), float("-inf"), device="cuda")), 1).reshape(B, n_parts, R, H, D).amax(2)
    assert torch.equal(part[:, 1], lo.transpose(0, 1)) and torch.equal(part[:, 2], hi.transpose(0, 1)), label
    mean64, amax64 = L.v_colstats_reference(x)
    bound = (R + n_parts + 1) * 2.0 ** -24 * x.double().abs().mean(dim=1)
    err = (mean.double() - mean64).abs()
    assert (err <= bound).all(), (label, (err / bound.clamp_min(1e-300)).max().item())
    want = torch.zeros(B, H, device="cuda")
    L.qk_prep_smooth(x, norm=None, shift=mean, amax_out=want, quantize=False)
    assert torch.equal(bits(amax), bits(want)), (label, amax, want)
    assert (amax.double() - amax64).abs().max().item() <= bound.max().item() + 2.0 ** -22 * amax64.max().item()      # (... of x - mean)
    part2 = torch.empty_like(part)
    mean2, amax2 = L.v_colstats(x, stat_part=part2)
    assert torch.equal(bits(part), bits(part2)) and torch.equal(bits(mean), bits(mean2)) and torch.equal(bits(amax), bits(amax2)), label
    return mean, amax, part


@pytest.mark.parametrize("S", [1, 63, 255, 256, 257, 600])
def test_colstats_row_counts_around_the_part_and_unroll_boundaries(S):
    check_colstats(make_v(1, S, 3, 64, seed=S), f"S={S}")


@pytest.mark.parametrize("dtype", [BF, FP16, FP32], ids=["bf16", "fp16", "fp32"])
def test_colstats_input_types_two_batches_odd_heads(dtype):
    check_colstats(make_v(2, 300, 5, 128, dtype, seed=1), str(dtype))


@pytest.mark.parametrize("shape", [(1, 70, 40, 128), (1, 90, 2, 256), (1, 90, 3, 40), (1, 3000, 40, 128)], ids=str)
def test_colstats_head_counts_and_head_dims(shape):
    """40 heads of 128 (the headline row), head_dim 256 and 40 (5 chunks: threads of a wave straddle heads), and 120 320 threads in
    470 workgroups (the kernel has no grid cap: one thread per (part, batch, head, chunk))."""
    check_colstats(make_v(*shape, seed=2), str(shape))


def test_colstats_of_the_v_slice_of_a_fused_projection_with_guard_bands():
    """x = qkv[:, :, 2] of a (B, S, 3, H, D) projection whose q and k slices hold NaN: the same bits as for a contiguous copy, and
    nothing but stat_part, mean and amax is written (NaN guard bands around each)."""
    import liteattention_amd as L
    B, S, H, D = 2, 100, 4, 128
    qkv = torch.full((B, S, 3, H, D), float("nan"), dtype=BF, device="cuda")
    v = make_v(B, S, H, D, seed=3)
    qkv[:, :, 2] = v
    n_parts, _ = L.v_colstats_parts(S, H, D)
    G = 64
    sizes = (n_parts * 3 * B * H * D, B * H * D, B * H)
    bufs = [torch.full((n + 2 * G,), float("nan"), device="cuda") for n in sizes]
    part, mean, amax = (b[G:G + n].view(shape) for b, n, shape in zip(bufs, sizes, ((n_parts, 3, B, H, D), (B, H, D), (B, H))))
    L.v_colstats(qkv[:, :, 2], stat_part=part, mean_out=mean, amax_out=amax)
    mean_c, amax_c, part_c = check_colstats(v, "contiguous")
    assert torch.equal(bits(part), bits(part_c)) and torch.equal(bits(mean), bits(mean_c)) and torch.equal(bits(amax), bits(amax_c))
    for b in bufs:
        assert b[:G].isnan().all() and b[-G:].isnan().all()
    assert qkv[:, :, :2].isnan().all() and torch.equal(qkv[:, :, 2], v)


def test_a_nan_marks_its_column_and_its_head_only():
    import liteattention_amd as L
    x = make_v(2, 100, 4, 128, seed=4)
    x[1, 37, 2, 5] = float("nan")
    mean, amax = L.v_colstats(x)
    assert mean[1, 2, 5].isnan() and mean.isnan().sum().item() == 1
    assert amax[1, 2].isnan() and amax.isnan().sum().item() == 1


def test_the_v_colstats_op_equals_the_function():
    import liteattention_amd as L
    x = make_v(1, 100, 4, 128, seed=5)
    mean, amax = L.v_colstats(x)
    got = torch.ops.lite_attention.v_colstats(x)
    assert torch.equal(bits(got[0]), bits(mean)) and torch.equal(bits(got[1]), bits(amax))
    m, a = torch.empty_like(mean), torch.empty_like(amax)
    got = torch.ops.lite_attention.v_colstats(x, None, m, a)
    assert got[0].data_ptr() == m.data_ptr() and torch.equal(bits(m), bits(mean)) and torch.equal(bits(a), bits(amax))


# ---- attn_unshift ----------------------------------------------------------------------------------------------------------------------
def make_o(B, S, H, D, dtype, hpv, seed=0):
    """o of order 1 and a shift in [-16, 16] per (batch, kv-head, column)."""
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(B, S, H, D, generator=g).to(dtype).cuda()
    shift = ((2.0 * torch.rand(B, H // hpv, D, generator=g) - 1.0) * 16.0).cuda()
    return o, shift


def assert_rounded(got, ref64, label=""):
    """`got` against the unrounded fp64 value, by the rule of the module docstring for its type."""
    if got.dtype == FP32:
        assert ((got.double() - ref64).abs() <= ulp32(ref64)).all(), label
        return
    want = ref64.to(got.dtype)
    off = got != want
    if off.any():
        mid = (got.double()[off] + want.double()[off]) / 2
        assert ((ref64[off] - mid).abs() <= ulp32(ref64[off])).all(), (label, off.sum().item())
        assert off.float().mean().item() < 1e-3, label                               # near-midpoints are rare


UNSHIFT_CASES = [((2, 130, 4, 128), hpv) for hpv in (1, 2, 4)] + [((1, 65, 6, 64), hpv) for hpv in (1, 2)]


@pytest.mark.parametrize("o_dtype", [BF, FP16], ids=["o_bf16", "o_fp16"])
@pytest.mark.parametrize("out_dtype", [BF, FP16, FP32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("shape,hpv", UNSHIFT_CASES, ids=lambda v: str(v))
def test_unshift_against_the_reference(shape, hpv, o_dtype, out_dtype):
    import liteattention_amd as L
    o, shift = make_o(*shape, o_dtype, hpv, seed=hpv)
    ref = L.attn_unshift_reference(o, shift)
    keep = o.clone()
    got = L.attn_unshift(o, shift, out_dtype=out_dtype)
    assert got.dtype == out_dtype and got.shape == o.shape and got.is_contiguous() and torch.equal(o, keep)
    assert_rounded(got, ref, "new tensor")
    cast = L.attn_unshift(o, out_dtype=out_dtype)                                     # shift=None: the cast alone
    assert torch.equal(cast, o.to(out_dtype))
    if out_dtype == o_dtype:
        same = L.attn_unshift(o, shift, out=o)                                        # in place
        assert same.data_ptr() == o.data_ptr() and torch.equal(o, got)


@pytest.mark.parametrize("shape,hpv", [((2, 130, 4, 128), 2), ((1, 65, 6, 64), 3)], ids=str)
def test_unshift_into_a_strided_view_of_the_projection_input(shape, hpv):
    """out = the (B, S, H, D) view of a (B, S, H * D + pad) fp32 buffer: the pad columns keep their sentinel; o itself is the k slice of
    a fused (B, S, 3, H, D) tensor."""
    import liteattention_amd as L
    B, S, H, D = shape
    o, shift = make_o(*shape, BF, hpv, seed=9)
    fused = torch.full((B, S, 3, H, D), float("nan"), dtype=BF, device="cuda")
    fused[:, :, 1] = o
    pad = 12
    buf = torch.full((B, S, H * D + pad), -7.0, device="cuda")
    view = buf[:, :, :H * D].view(B, S, H, D)
    got = L.attn_unshift(fused[:, :, 1], shift, out=view)
    assert got.data_ptr() == buf.data_ptr()
    assert_rounded(view, L.attn_unshift_reference(o, shift), "strided")
    assert (buf[:, :, H * D:] == -7.0).all()
    assert torch.equal(bits(view), bits(L.attn_unshift(o, shift, out_dtype=FP32)))


def test_unshift_empty_rows_nan_rows_and_the_fused_lse():
    import liteattention_amd as L
    B, S, H, D = 2, 130, 4, 128
    o, shift = make_o(B, S, H, D, BF, 2, seed=11)
    g = torch.Generator().manual_seed(12)
    lse = (4.0 * torch.randn(B, H, S, generator=g)).cuda()
    dot = (30.0 * torch.randn(B, H, S, generator=g)).cuda()
    lse[0, 1, 7], lse[1, 3, 129], lse[1, 0, 64] = float("inf"), float("-inf"), float("nan")
    scale = D ** -0.5
    ref_o, ref_lse = L.attn_unshift_reference(o, shift, lse=lse, lse_dot=dot, softmax_scale=scale)
    for out_dtype in (BF, FP32):
        got, lse_out = L.attn_unshift(o, shift, lse=lse, lse_dot=dot, softmax_scale=scale, out_dtype=out_dtype)
        assert (got[0, 7, 1] == 0).all() and (got[1, 129, 3] == 0).all()              # +inf and -inf rows: zeros ...
        assert lse_out[0, 1, 7] == float("inf") and lse_out[1, 3, 129] == float("-inf")      # ... and the lse unchanged
        assert lse_out[1, 0, 64].isnan() and not got[1, 64, 0].isnan().any() and (got[1, 64, 0] != 0).any()    # NaN: the normal path
        assert_rounded(got, ref_o, "with lse")
        fine = ~(lse.isinf() | lse.isnan())
        assert ((lse_out.double() - ref_lse)[fine].abs() <= ulp32(ref_lse[fine])).all()
        unfused = L.lse_unshift(lse, dot, scale)
        assert ((lse_out.double() - unfused.double())[fine].abs() <= ulp32(unfused.double()[fine])).all()
    only_o = L.attn_unshift(o, shift, lse=lse)                                        # lse without lse_dot: the empty-row rule alone
    assert (only_o[0, 7, 1] == 0).all() and torch.equal(only_o, L.attn_unshift(o, shift, lse=lse, lse_dot=dot, softmax_scale=scale)[0])
    no_rule = L.attn_unshift(o, shift)
    assert (no_rule[0, 7, 1] != 0).any()
    # in place, o and lse both
    o2, lse2 = o.clone(), lse.clone()
    got, lse_out = L.attn_unshift(o2, shift, lse=lse2, lse_dot=dot, softmax_scale=scale, out=o2, lse_out=lse2)
    assert got.data_ptr() == o2.data_ptr() and lse_out.data_ptr() == lse2.data_ptr()
    want_o, want_lse = L.attn_unshift(o, shift, lse=lse, lse_dot=dot, softmax_scale=scale)
    assert torch.equal(o2, want_o) and torch.equal(bits(lse2), bits(want_lse))


def test_the_attn_unshift_op_equals_the_function():
    import liteattention_amd as L
    o, shift = make_o(1, 65, 6, 64, FP16, 2, seed=13)
    lse, dot = torch.randn(1, 6, 65, device="cuda"), torch.randn(1, 6, 65, device="cuda")
    want, want_lse = L.attn_unshift(o, shift, lse=lse, lse_dot=dot, softmax_scale=0.3, out_dtype=FP32)
    lse_out = torch.empty_like(lse)
    got = torch.ops.lite_attention.attn_unshift(o, shift, lse, dot, 0.3, None, FP32, lse_out)
    assert got.dtype == FP32 and torch.equal(bits(got), bits(want)) and torch.equal(bits(lse_out), bits(want_lse))


# ---- end to end through the fp8 attention call ---------------------------------------------------------------------------------------
_DEV = {}


def _case(offset):
    """emu.case(offset) on the device: bf16 q / k / v with +-offset on 8 channels of every V head, the fp64 O and LSE; once."""
    if offset not in _DEV:
        _DEV[offset] = tuple(t.cuda() for t in emu.case(offset))
    return _DEV[offset]


def _qk(q, k):
    import liteattention_amd as L
    q8, dq = L.E4m3Scales()(q, norm=None)
    k8, dk = L.E4m3Scales()(k, norm=None)
    return q8, k8, dq, dk


def _dense_errors(offset, out_dtype):
    """(plain, smoothed) relative rms error of O against fp64 for E4m3Scales and for SmoothedV with finish(out_dtype)."""
    import liteattention_amd as L
    q, k, v, o64, _ = _case(offset)
    q8, k8, dq, dk = _qk(q, k)
    v8, dv = L.E4m3Scales()(v, norm=None)
    o_plain = L.flash_attn_func(q8, k8, v8, q_descale=dq, k_descale=dk, v_descale=dv)
    sv = L.SmoothedV()
    s8, sdv, shift = sv(v)
    o_s, lse = L.flash_attn_func(q8, k8, s8, q_descale=dq, k_descale=dk, v_descale=sdv, return_softmax_lse=True)
    o_smooth = sv.finish(o_s, lse=lse, out_dtype=out_dtype)
    assert o_smooth.dtype == out_dtype
    return emu.rel_rms(o_plain.to(out_dtype), o64), emu.rel_rms(o_smooth, o64)


@pytest.mark.parametrize("out_dtype", [BF, FP32], ids=["bf16", "fp32"])
def test_dense_fp8_attention_gains_from_v_smoothing_at_offset_16(out_dtype):
    """Device ratio below min(1, 1.25 x the emulation's), the emulation in the form of the default P (rounded, fp32 row sums of the
    unrounded P): 0.577 (bf16) and 0.302 (fp32), i.e. bounds 0.721 and 0.377."""
    ratio_emu, plain_emu, smooth_emu = emu.smoothing_ratio(16, out_dtype, True, False)
    plain, smooth = _dense_errors(16, out_dtype)
    print(f"offset 16, out {out_dtype}: O rel rms plain {plain:.5f}, smoothed {smooth:.5f} (ratio {smooth / plain:.3f}); emulation "
          f"plain {plain_emu:.5f}, smoothed {smooth_emu:.5f} (ratio {ratio_emu:.3f})")
    assert smooth / plain < min(1.0, 1.25 * ratio_emu)


def test_dense_fp8_attention_loses_nothing_without_an_offset():
    """Offset 0: the ratio is below 1.10 (the emulation gives 1.003)."""
    plain, smooth = _dense_errors(0, BF)
    print(f"offset 0: O rel rms plain {plain:.5f}, smoothed {smooth:.5f} (ratio {smooth / plain:.3f}); emulation "
          f"{emu.smoothing_ratio(0, BF, True, False)[0]:.4f}")
    assert smooth / plain < 1.10


def test_with_skip_lists_v_never_enters_the_vote_and_the_smoothed_run_is_no_worse():
    """Two LiteAttention steps at threshold -4 on the offset-16 input, the same q / k codes for both runs: the lists after each step
    are bit-equal (V is not part of the vote), the second step walks the first's lists, the smoothed O is no further from fp64."""
    import liteattention_amd as L
    q, k, v, o64, _ = _case(16)
    q8, k8, dq, dk = _qk(q, k)
    v8, dv = L.E4m3Scales()(v, norm=None)
    sv = L.SmoothedV()
    s8, sdv, shift = sv(v)
    lists, errs = [], []
    for vv, d_v, kw in ((v8, dv, {}), (s8, sdv, dict(v_shift=shift))):
        la = L.LiteAttention(threshold=-4.0)
        la(q8, k8, vv, q_descale=dq, k_descale=dk, v_descale=d_v, **kw)
        first = la.current_read_list().clone()
        listed = 1.0 - la.get_skip_fraction(batch=1)
        out = la(q8, k8, vv, q_descale=dq, k_descale=dk, v_descale=d_v, **kw)
        lists.append((first, la.current_read_list().clone(), listed))
        errs.append(emu.rel_rms(out, o64))
    print(f"threshold -4, step 2: listed fraction {lists[0][2]:.4f} / {lists[1][2]:.4f}; O rel rms plain {errs[0]:.5f}, smoothed {errs[1]:.5f}")
    assert torch.equal(lists[0][0], lists[1][0]) and torch.equal(lists[0][1], lists[1][1])
    assert errs[1] <= errs[0]


def test_gqa_and_a_split_kv_call():
    """H_q 4 on H_kv 2 (two q-heads per shift row), dense, once as one launch and once with num_splits=2 (the shift is added behind the
    merge of the splits): both within the e4m3 error of fp64, and closer than the unsmoothed call."""
    import liteattention_amd as L
    g = torch.Generator().manual_seed(21)
    q = torch.randn(1, 320, 4, 128, generator=g).bfloat16().cuda()
    k = torch.randn(1, 320, 2, 128, generator=g).bfloat16().cuda()
    v = (torch.randn(1, 320, 2, 128, generator=g) + emu.offset_vector(2, 128, 16.0, 3)[None, None]).bfloat16().cuda()
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double().repeat_interleave(2, dim=2)) * 128 ** -0.5
    o64 = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), v.double().repeat_interleave(2, dim=2))
    q8, dq = L.E4m3Scales(heads_per_scale=2)(q, norm=None)
    k8, dk = L.E4m3Scales()(k, norm=None)
    v8, dv = L.E4m3Scales()(v, norm=None)
    plain = emu.rel_rms(L.flash_attn_func(q8, k8, v8, q_descale=dq, k_descale=dk, v_descale=dv), o64)
    sv = L.SmoothedV()
    s8, sdv, shift = sv(v)
    assert shift.shape == (1, 2, 128)
    for splits in (1, 2):
        o, lse = L.flash_attn_func(q8, k8, s8, q_descale=dq, k_descale=dk, v_descale=sdv, return_softmax_lse=True, num_splits=splits)
        err = emu.rel_rms(sv.finish(o, lse=lse, out_dtype=FP32), o64)
        print(f"GQA 4 on 2, num_splits {splits}: O rel rms plain {plain:.5f}, smoothed {err:.5f}")
        assert err < plain


def test_a_call_without_keys_stays_zero():
    import liteattention_amd as L
    q, k, v, _, _ = _case(16)
    q8, _, dq, _ = _qk(q, k)
    sv = L.SmoothedV()
    _, _, shift = sv(v)
    empty = torch.zeros(1, 0, 2, 128, dtype=F8, device="cuda")
    o, lse = L.flash_attn_func(q8, empty, empty, return_softmax_lse=True)
    out = sv.finish(o, lse=lse, out_dtype=FP32)
    assert (out == 0).all() and (lse == float("inf")).all() and shift.abs().max().item() > 8
    la = L.LiteAttention(enable_skipping=False)
    assert (la(q8, empty, empty, v_shift=shift) == 0).all()


def test_k_and_v_smoothing_together_o_and_lse_from_one_finish():
    """SmoothedQK and SmoothedV on an input with offsets on both K and V: one finish restores O and the LSE; the LSE lands within the
    header's fp8 LSE bound (0.084) of fp64 and the raw one does not; LiteAttention(v_shift=, lse_shift=, out_dtype=) gives the same
    bits as the manual sequence."""
    import liteattention_amd as L
    q, k, v, _, _ = _case(16)
    k = (k.float() + emu.offset_vector(2, 128, 16.0, 5)[None, None].cuda()).bfloat16()
    scale = 128 ** -0.5
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * scale
    o64, lse64 = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), v.double()), torch.logsumexp(s, dim=-1)
    sq, sk, sdq, sdk, lse_shift = L.SmoothedQK().pair(q, k, norm=None)
    sv = L.SmoothedV()
    s8, sdv, shift = sv(v)
    kw = dict(q_descale=sdq, k_descale=sdk, v_descale=sdv)
    o_raw, lse_raw = L.flash_attn_func(sq, sk, s8, return_softmax_lse=True, **kw)
    raw_err = (lse_raw.double() - lse64).abs().max().item()
    o_keep, lse_keep = o_raw.clone(), lse_raw.clone()
    out, lse = sv.finish(o_raw, lse=lse_raw, lse_dot=lse_shift, softmax_scale=scale, out_dtype=FP32)
    lse_err = (lse.double() - lse64).abs().max().item()
    print(f"K and V smoothed: O rel rms {emu.rel_rms(out, o64):.5f}; max |LSE error| raw {raw_err:.4f}, restored {lse_err:.4f}")
    assert lse.data_ptr() == lse_raw.data_ptr() and lse_err <= 0.084 < raw_err
    assert emu.rel_rms(out, o64) < 0.01
    la = L.LiteAttention(enable_skipping=False)
    got, got_lse = la(sq, sk, s8, return_softmax_lse=True, v_shift=shift, lse_shift=lse_shift, out_dtype=FP32, **kw)
    assert got.dtype == FP32 and torch.equal(bits(got), bits(out)) and torch.equal(bits(got_lse), bits(lse))
    want_bf = L.attn_unshift(o_keep, shift, lse=lse_keep)
    assert torch.equal(la(sq, sk, s8, v_shift=shift, **kw), want_bf)                  # O alone, bf16, no LSE asked for
    sp = L.SeqParallelLiteAttention(2, enable_skipping=False)
    got, got_lse = sp(sq, sk, s8, 1, return_softmax_lse=True, v_shift=shift, lse_shift=lse_shift, out_dtype=FP32, **kw)
    assert torch.equal(bits(got), bits(out)) and torch.equal(bits(got_lse), bits(lse))


def test_delayed_mode_captures_into_a_hip_graph_and_replays():
    """Delayed mode: the first call (no history) eager, then sv(x) + finish captured once and replayed on two changing inputs; codes,
    descale, shift, the restored output and the state for the next step equal the eager object's bit for bit, and step t used step
    t - 1's mean."""
    import liteattention_amd as L
    x = make_v(1, 100, 4, 128, seed=30)
    o = torch.randn(1, 100, 8, 128, device="cuda").bfloat16()                         # stands for the attention output (8 q-heads on 4)
    eager, graphed = L.SmoothedV(mode="delayed", margin=1.25), L.SmoothedV(mode="delayed", margin=1.25)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for sv in (eager, graphed):
            sv(x)
            sv.finish(o, out_dtype=FP32)
    torch.cuda.current_stream().wait_stream(side)
    ptrs = [t.data_ptr() for t in (graphed.v8, graphed.shift, graphed.part, graphed.next_mean, graphed.out)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res_g = graphed(x)
        out_g = graphed.finish(o, out_dtype=FP32)
    assert ptrs == [t.data_ptr() for t in (graphed.v8, graphed.shift, graphed.part, graphed.next_mean, graphed.out)]
    for rep in range(2):
        x.copy_(make_v(1, 100, 4, 128, seed=40 + rep) * (1.0 + 0.1 * rep) + 2.0 * rep)
        mean_before = eager.next_mean.clone()
        g.replay()
        res_e = eager(x)
        out_e = eager.finish(o, out_dtype=FP32)
        torch.cuda.synchronize()
        for a, b in zip(res_g, res_e):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), rep
        assert torch.equal(bits(out_g), bits(out_e)), rep
        assert torch.equal(bits(graphed.next_mean), bits(eager.next_mean)) and torch.equal(bits(graphed.next_amax), bits(eager.next_amax))
        assert torch.equal(bits(res_e[2]), bits(mean_before)), rep                    # the shift used is the previous step's mean
        assert torch.equal(bits(eager.next_mean), bits(L.v_colstats(x)[0])), rep      # ... and the state now holds this step's own
    assert eager.calls == 3 and graphed.calls == 2                                    # (the capture ran the call once, the replays none)


def test_the_demo_block_with_smooth_v_is_as_close_to_the_bf16_block_as_the_plain_fp8_one():
    """`examples/wan_self_attention_demo.py --fp8 --smooth-v [--smooth-k]`: the same weights in a bf16 block, a plain fp8 block and the
    smoothed ones, skipping off. A random projection gives V no offset, so smoothing has nothing to gain: its rms error against the bf16
    block stays below 1.10 x the plain fp8 block's (the offset-0 bound above); the block returns fp32 through `out_dtype`."""
    import wan_self_attention_demo as demo
    torch.manual_seed(0)
    grid, heads = (3, 8, 10), 2
    x = torch.randn(1, 240, heads * 128, device="cuda")
    blocks = {name: demo.WanLikeSelfAttention(heads * 128, heads, enable_skipping=False, **kw).cuda()
              for name, kw in (("bf16", dict(fused_prep=True)), ("fp8", dict(fp8=True)), ("smooth_v", dict(fp8=True, smooth_v=True)),
                               ("smooth_kv", dict(fp8=True, smooth_k=True, smooth_v=True)))}
    for b in blocks.values():
        b.load_state_dict(blocks["bf16"].state_dict())
    with torch.no_grad():
        y = {name: b(x, grid) for name, b in blocks.items()}
    err = {name: (y[name] - y["bf16"]).pow(2).mean().sqrt().item() for name in ("fp8", "smooth_v", "smooth_kv")}
    print("demo block, rms error against the bf16 block:", err)
    assert y["smooth_v"].dtype == torch.float32 and y["smooth_v"].shape == x.shape
    assert err["smooth_v"] < 1.10 * err["fp8"]
    assert err["smooth_kv"] < 1.10 * 1.10 * err["fp8"]                                # (K smoothing's own offset-0 bound is 1.10 too)
