"""GPU: la_attn_unshift_fp8 / attn_out_fp8 - O restored (shift, empty rows, LSE) and row-scaled to e4m3 in one pass.

The expected bytes and descales come from tests/attn_out_fp8_emulation.py: the formula of the header step by step in torch fp32 on the
CPU, never from the code under test. The formula holds no sum that could be reassociated - an fp32 addition, a maximum of bit patterns,
two IEEE divisions, a product, a clamp and the e4m3 rounding - so bytes and descales are compared for EQUALITY. One bound is checked
besides, against the unrounded fp64 reference: |data * descale - y| <= max(|y| 2^-4, descale 2^-10) (1 + 2^-16), half an e4m3 step
or half the subnormal step, plus the fp32 product and reciprocal."""
import ctypes

import pytest
import torch

import attn_out_fp8_emulation as emu

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
BF16, FP16 = torch.bfloat16, torch.float16
TINY_DESCALE = torch.tensor(2.0 ** -100).div(448.0)       # fp32: what an all-zero group gets


def make_o(B, S, H, D, dtype=BF16, seed=0, decades=False):
    """N(0, 1) times a per-(token, head) scale in [0.25, 4] - with `decades` times a per-token power of two in [2^-15, 2^14] too."""
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(B, S, H, D, generator=g) * (0.25 + 3.75 * torch.rand(B, S, H, 1, generator=g))
    if decades:
        o = o * torch.exp2(torch.randint(-15, 15, (B, S, 1, 1), generator=g).float())
    return o.to(dtype).cuda()


def make_shift(B, Hkv, D, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    return (torch.randn(B, Hkv, D, generator=g) * 2.0).cuda()


def make_lse(B, H, S, seed=0, holes=True):
    """Finite values, and with `holes` a +inf, a -inf and a NaN sprinkled in (every 7th, 11th and 13th element)."""
    g = torch.Generator().manual_seed(200 + seed)
    lse = torch.randn(B, H, S, generator=g) * 3.0 + 5.0
    dot = torch.randn(B, H, S, generator=g)
    if holes:
        flat = lse.view(-1)
        flat[3::7], flat[5::11], flat[6::13] = float("inf"), float("-inf"), float("nan")
    return lse.cuda(), dot.cuda()


def same_bytes(got, want):
    return torch.equal(got.cpu().view(torch.uint8), want.cpu().view(torch.uint8))


def same_bits(got, want):
    return torch.equal(got.cpu().contiguous().view(torch.int32), want.cpu().contiguous().view(torch.int32))


def check(o, shift=None, lse=None, lse_dot=None, hps=None, scale=0.3, **kw):
    """One dynamic-mode call against the emulation: bytes and descales bit for bit; with lse_dot the LSE attn_unshift writes."""
    import liteattention_amd as L
    before = o.clone()
    res = L.attn_out_fp8(o, shift, lse=lse, lse_dot=lse_dot, softmax_scale=scale, heads_per_scale=hps, **kw)
    r = res[0] if lse_dot is not None else res
    assert isinstance(r, L.RowScaledE4m3) and r.data.dtype == F8 and r.data.shape == o.shape and r.descale.dtype == torch.float32
    data, d, _ = emu.emulate(o, shift, lse, hps)
    assert r.descale.shape == d.shape
    assert same_bits(r.descale, d), f"descale: {(r.descale.cpu() != d).sum().item()} of {d.numel()} differ"
    diff = (r.data.cpu().view(torch.uint8) != data.view(torch.uint8))
    assert not diff.any(), f"{diff.sum().item()} of {diff.numel()} bytes differ, the first at {diff.nonzero()[0].tolist()}"
    assert torch.equal(o, before)                                                  # o is read, never written
    if lse_dot is not None:
        _, want = L.attn_unshift(o, shift, lse=lse, lse_dot=lse_dot, softmax_scale=scale)
        assert same_bits(res[1], want)
    return r


# ---- bit equality over the shapes ----------------------------------------------------------------------------------------------------
SHAPES = [((2, 67, 5, 96), 1), ((2, 67, 5, 96), 5),                    # odd head count; S no multiple of 32 or 64; 60 chunks for 64 lanes
          ((1, 33, 40, 128), 40), ((1, 33, 40, 128), 8), ((1, 33, 40, 128), 1),      # H * D = 5120: 10 chunks a lane; 2; 16 lanes a unit
          ((1, 1, 1, 64), 1),                                          # fewer elements than lanes
          ((1, 40, 64, 256), 64)]                                      # the limit: 16384 elements, 32 chunks a lane


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("form", ["plain", "shift", "shift_lse", "shift_lse_dot", "lse_dot"])
@pytest.mark.parametrize("shape,hps", SHAPES, ids=[f"{'x'.join(map(str, s))}-hps{h}" for s, h in SHAPES])
def test_bytes_and_descales_equal_the_emulation(shape, hps, form, dtype):
    B, S, H, D = shape
    o = make_o(B, S, H, D, dtype, seed=hps)
    hkv = H // 2 if H % 2 == 0 else 1                                              # GQA: two query heads a shift row (five of H = 5)
    shift = make_shift(B, hkv, D) if "shift" in form else None
    lse, dot = make_lse(B, H, S) if "lse" in form else (None, None)
    check(o, shift, lse, dot if "dot" in form else None, hps)


def test_views_the_middle_of_a_fused_tensor_a_flat_out_and_a_padded_descale():
    B, S, H, D = 2, 70, 4, 128
    qkv = make_o(B, S, 3 * H, D, seed=9).view(B, S, 3, H, D)
    o = qkv[:, :, 1]
    flat = torch.empty(B, S, H * D, dtype=F8, device="cuda")
    pad = torch.full((B, S, 2 + 3), float("nan"), device="cuda")
    lse, dot = make_lse(B, H, S)
    r = check(o, make_shift(B, 2, D), lse, dot, 2, out=flat.view(B, S, H, D), descale_out=pad[..., :2])
    assert r.data.data_ptr() == flat.data_ptr() and r.descale.data_ptr() == pad.data_ptr()
    assert pad[..., 2:].isnan().all() and not pad[..., :2].isnan().any()
    r = check(o, make_shift(B, 2, D), lse, None, None, out=flat.view(B, S, H, D))
    m, s = r.as_matrix()                                                           # one scale per token: what a row-wise scaled GEMM takes
    assert m.shape == (B * S, H * D) and s.shape == (B * S, 1) and m.data_ptr() == flat.data_ptr()


# ---- the reduction covers its ends -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,hps", [((1, 33, 40, 128), 40), ((1, 33, 40, 128), 8), ((2, 67, 5, 96), 5), ((1, 40, 64, 256), 64),
                                       ((1, 33, 40, 128), 1)])
def test_the_largest_element_is_found_wherever_it_sits(shape, hps):
    """Rows of |o| <= 1 with ONE element of magnitude 3 - at element 0 of a group, at its last element, inside its last chunk, once
    negative: that element must land on +-448 and everything else on the emulation's bytes."""
    B, S, H, D = shape
    n = hps * D
    o = (make_o(B, S, H, D, seed=3).float().clamp(-1, 1)).to(BF16)
    places = [(0, 0, 0, 3.0), (1, 0, n - 1, 3.0), (2, H // hps - 1, n - 5, -3.0), (3, H // hps - 1, 0, -3.0), (4, 0, n - 8, 3.0),
              (5, H // hps - 1, n - 1, -3.0), (6, 0, n // 2 + 3, 3.0)]
    og = o.view(B, S, H // hps, n)
    for s, g, e, v in places:
        og[B - 1, s, g, e] = v
    r = check(o, None, None, None, hps)
    got = r.data.float().view(B, S, H // hps, n)
    for s, g, e, v in places:
        assert got[B - 1, s, g, e].item() == (448.0 if v > 0 else -448.0), (s, g, e)
        assert r.descale[B - 1, s, g].item() == torch.tensor(3.0).div(448.0).item()


# ---- dynamic range ----------------------------------------------------------------------------------------------------------------------
def test_rows_of_2_to_the_minus_30_and_plus_30_zeros_and_a_lone_large_value():
    B, S, H, D = 1, 33, 40, 128
    o = make_o(B, S, H, D, seed=4).float()
    o[0, 0] *= 2.0 ** -30
    o[0, 1] *= 2.0 ** 30
    o[0, 2] = 0.0
    o[0, 3] = 1e-3
    o[0, 3, 17, 5] = 1e4
    o[0, 4, :20] = 0.0                                                             # hps 8: groups 0 and 1 of this token are all zero
    o = o.to(BF16)
    for hps in (40, 8):
        r = check(o, None, None, None, hps)
        assert (r.descale[0, 2] == TINY_DESCALE.item()).all() and r.data[0, 2].view(torch.uint8).eq(0).all()
        big, small = r.data[0, 1].float().abs().max().item(), r.data[0, 0].float().abs().max().item()
        assert big == small == 448.0                                               # each row uses the whole range, whatever its magnitude
        row = r.data[0, 3].float()
        assert row[17, 5] == 448.0
        in_group = row.view(H // hps, -1)[17 // hps]
        assert in_group.abs().sum() == 448.0                                       # 1e-3 under a scale made for 1e4: 4.5e-5 rounds to zero
        if hps == 8:
            assert (r.descale[0, 4, :2] == TINY_DESCALE.item()).all() and (r.descale[0, 4, 3:] > 1e-4).all()
            other = row.view(H // hps, -1)[0]
            assert (other == 448.0).all()                                          # a group of equal values: all on the maximum
    # e4m3 subnormals: the largest value 1, then +-2^-j: 448 / 2^j runs through the normal codes, the subnormal ones (steps of 2^-9), and out
    o = torch.zeros(1, 1, 1, 64)
    o[0, 0, 0, 0] = 1.0
    for j in range(1, 24):
        o[0, 0, 0, j] = 2.0 ** -j * (1.0 if j % 2 else -1.0)
    r = check(o.to(BF16).cuda(), None, None, None, 1)
    vals = r.data.float()[0, 0, 0]
    step = 2.0 ** -9                                                               # 448 / 2^j = 7 * 2^(15 - j) steps (j = 16 is a tie: the emulation's)
    assert vals[0] == 448.0 and vals[15] == 7 * step and vals[17] == 2 * step and vals[18] == -step     # 1.75 -> 2, 0.875 -> 1
    assert vals[19:].abs().sum() == 0                                              # 0.4375 of a step and less: flushed to zero


# ---- empty rows -----------------------------------------------------------------------------------------------------------------------------
def test_empty_heads_are_zero_bytes_and_the_scale_comes_from_the_rest():
    B, S, H, D = 2, 67, 5, 96
    o = make_o(B, S, H, D, seed=5)
    shift = make_shift(B, 1, D)
    lse, _ = make_lse(B, H, S, holes=False)
    lse[1, 1, 40], lse[1, 3, 40] = float("inf"), float("inf")                      # two heads of one token
    lse[0, :, 7] = float("inf")                                                    # every head of a token
    lse[1, :, 66] = float("-inf")
    lse[1, 2, 66] = float("inf")
    r = check(o, shift, lse, None, None)
    y = emu.restored(o, shift)
    data = r.data.view(torch.uint8)
    assert data[1, 40, 1].eq(0).all() and data[1, 40, 3].eq(0).all() and not data[1, 40, 0].eq(0).all()
    want = y[1, 40, [0, 2, 4]].abs().max().clamp_min(emu.TINY) / 448.0
    assert r.descale[1, 40, 0].item() == want.item()
    for b, s in ((0, 7), (1, 66)):
        assert r.descale[b, s, 0].item() == TINY_DESCALE.item() and data[b, s].eq(0).all()
    r1 = check(o, shift, lse, None, 1)                                             # per head: the empty heads' own scales are the tiny one
    assert r1.descale[1, 40, 1].item() == r1.descale[1, 40, 3].item() == TINY_DESCALE.item()


# ---- NaN containment ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,hps", [((1, 33, 40, 128), 8), ((2, 67, 5, 96), 1)])
def test_a_nan_stays_in_its_group(shape, hps):
    import liteattention_amd as L
    B, S, H, D = shape
    o = make_o(B, S, H, D, seed=6)
    shift = make_shift(B, 1, D)
    clean = L.attn_out_fp8(o, shift, heads_per_scale=hps)
    clean_data, clean_ds = clean.data.clone(), clean.descale.clone()
    b, s, h = B - 1, S - 2, H - 2
    o[b, s, h, D - 3] = float("nan")
    r = L.attn_out_fp8(o, shift, heads_per_scale=hps)
    g = h // hps
    assert r.descale.isnan().sum() == 1 and r.descale[b, s, g].isnan()
    bad = torch.zeros(B, S, H, D, dtype=torch.bool, device="cuda")
    bad[b, s, g * hps:(g + 1) * hps] = True
    got = r.data.view(torch.uint8)
    assert ((got[bad] & 0x7f) == 0x7f).all()                                       # the group: e4m3 NaN, every byte
    assert torch.equal(got[~bad], clean_data.view(torch.uint8)[~bad])              # every other group and token: as without the NaN
    keep = ~r.descale.isnan()
    assert torch.equal(r.descale[keep].view(torch.int32), clean_ds[keep].view(torch.int32))
    data, d, _ = emu.emulate(o, shift, None, hps)                                  # ... and as the emulation
    assert torch.equal(got.cpu()[~bad.cpu()], data.view(torch.uint8)[~bad.cpu()]) and d.isnan().sum() == 1


# ---- the static mode ----------------------------------------------------------------------------------------------------------------------
def _direct_static_call(o, out, descale, row_descale):
    """The C entry point with BOTH descale_in and row_descale: the static mode must leave row_descale alone."""
    from liteattention_amd import _cabi
    a = _cabi.LaAttnUnshiftFp8Args()
    a.struct_size = ctypes.sizeof(_cabi.LaAttnUnshiftFp8Args)
    a.o_dtype, a.heads_per_vec, a.heads_per_scale = _cabi.LA_DTYPE_BF16, 1, o.shape[2]
    a.o, a.out = o.data_ptr(), out.data_ptr()
    a.o_batch_stride, a.o_row_stride, a.o_head_stride = o.stride()[:3]
    a.out_batch_stride, a.out_row_stride, a.out_head_stride = out.stride()[:3]
    a.batch, a.seqlen, a.num_heads, a.head_dim = o.shape
    a.row_descale = row_descale.data_ptr()
    a.row_descale_batch_stride, a.row_descale_row_stride, a.row_descale_group_stride = row_descale.stride()
    a.descale_in, a.descale_in_batch_stride = descale.data_ptr(), 1
    rc = _cabi.load().la_attn_unshift_fp8(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _cabi.LA_OK, _cabi.status_string(rc)


def test_static_mode_bytes_running_amax_and_an_untouched_row_descale():
    import liteattention_amd as L
    B, S, H, D = 2, 67, 5, 96
    o = make_o(B, S, H, D, seed=7)
    shift = make_shift(B, 1, D)
    lse, dot = make_lse(B, H, S)
    ds = torch.tensor([0.05, 0.004], device="cuda")                                # the second saturates part of its batch
    amax = torch.zeros(B, device="cuda")
    (r, lse_out) = L.attn_out_fp8(o, shift, lse=lse, lse_dot=dot, softmax_scale=0.3, descale=ds, amax_out=amax)
    data, _, y = emu.emulate(o, shift, lse, None, ds)
    assert r.descale is ds and same_bytes(r.data, data)
    assert (r.data[1].float().abs() == 448).any() and not r.data.float().isnan().any()
    assert same_bits(lse_out, L.attn_unshift(o, shift, lse=lse, lse_dot=dot, softmax_scale=0.3)[1])
    first = y.abs().amax(dim=(1, 2, 3))
    assert same_bits(amax, first)                                                  # the exact maximum of |y|
    o2 = make_o(B, S, H, D, seed=8)
    o2[0] *= 4.0
    o2[1] *= 0.25
    one = torch.tensor([0.05], device="cuda")                                      # one element for every batch
    r2 = L.attn_out_fp8(o2, shift, descale=one, amax_out=amax)
    data2, _, y2 = emu.emulate(o2, shift, None, None, one)
    assert same_bytes(r2.data, data2)
    both = torch.maximum(first, y2.abs().amax(dim=(1, 2, 3)))                      # positive floats: the unsigned maximum of the bits
    assert same_bits(amax, both) and amax[0].item() > first[0].item() and amax[1].item() == first[1].item()
    pattern = torch.full((B, S, 1), -123.25, device="cuda")
    out = torch.empty(B, S, H, D, dtype=F8, device="cuda")
    _direct_static_call(o, out, ds, pattern)
    assert (pattern == -123.25).all() and same_bytes(out, emu.emulate(o, None, None, None, ds)[0])


# ---- the error bound against fp64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hps", [1, 5])
def test_error_bound_against_the_fp64_reference_over_nine_decades(hps):
    import liteattention_amd as L
    B, S, H, D = 2, 67, 5, 96
    o = make_o(B, S, H, D, seed=11, decades=True)
    shift = make_shift(B, 1, D) * 0.01
    r = L.attn_out_fp8(o, shift, heads_per_scale=hps)
    y = L.attn_unshift_reference(o, shift)
    d = r.descale.double().repeat_interleave(hps, dim=2)[..., None]
    err = (r.data.double() * d - y).abs()
    bound = torch.maximum(y.abs() * 2.0 ** -4, d * 2.0 ** -10) * (1 + 2.0 ** -16)
    print(f"hps {hps}: max err / bound {(err / bound).max().item():.4f}")
    assert (err <= bound).all(), (err / bound).max().item()
    z, d64 = L.attn_out_fp8_reference(o, shift, heads_per_scale=hps)
    assert ((r.descale.double() - d64).abs() <= d64 * 2.0 ** -22).all()


# ---- nothing else is written ------------------------------------------------------------------------------------------------------------------
def test_poison_around_out_and_row_descale_is_intact():
    B, S, H, D = 2, 70, 4, 128
    o = make_o(B, S, H, D, seed=12)
    shift = make_shift(B, 2, D)
    lse, dot = make_lse(B, H, S)
    big = torch.full((B + 1, S + 3, H + 2, D + 8), 0x7f, dtype=torch.uint8, device="cuda")
    ds_big = torch.full((B + 1, S + 2, 2 + 1), float("nan"), device="cuda")
    lse_big = torch.full((B * H * S + 64,), float("nan"), device="cuda")
    out, ds_out = big.view(F8)[:B, :S, :H, :D], ds_big[:B, :S, :2]
    lse_out = lse_big[32:32 + B * H * S].view(B, H, S)
    check(o, shift, lse, dot, 2, out=out, descale_out=ds_out, lse_out=lse_out)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[:B, :S, :H, :D] = False
    assert big[mask].eq(0x7f).all()
    dmask = torch.ones_like(ds_big, dtype=torch.bool)
    dmask[:B, :S, :2] = False
    assert ds_big[dmask].isnan().all() and not ds_big[~dmask].isnan().any()
    assert lse_big[:32].isnan().all() and lse_big[32 + B * H * S:].isnan().all()


# ---- through the classes ------------------------------------------------------------------------------------------------------------------------
def _fp8_inputs(B=1, S=320, H=4, D=128, seed=13):
    g = torch.Generator().manual_seed(seed)
    q, k = [torch.randn(B, S, H, D, generator=g).to(F8).cuda() for _ in range(2)]
    xv = (torch.randn(B, S, H, D, generator=g) + 3.0).bfloat16().cuda()            # a V with a mean: what smoothing is for
    return q, k, xv


def test_lite_attention_out_fp8_equals_the_pass_on_the_same_calls_output():
    import liteattention_amd as L
    q, k, xv = _fp8_inputs()
    v8, dv, shift = L.SmoothedV()(xv)
    for cls in ("LiteAttention", "SeqParallelLiteAttention"):
        if cls == "LiteAttention":
            la = L.LiteAttention(enable_skipping=False)
            call = lambda **kw: la(q, k, v8, v_descale=dv, **kw)                   # noqa: E731
        else:
            sp = L.SeqParallelLiteAttention(2, enable_skipping=False)
            sp.exact_fp8_lse = False                                               # the same form of P with and without the LSE
            call = lambda **kw: sp(q, k, v8, 1, v_descale=dv, **kw)                # noqa: E731
        o, lse = call(return_softmax_lse=True)
        assert o.dtype == BF16
        want = L.attn_out_fp8(o, shift, lse=lse)
        got = call(v_shift=shift, out_fp8=True)
        assert isinstance(got, L.RowScaledE4m3) and same_bytes(got.data, want.data) and same_bits(got.descale, want.descale)
        want2 = L.attn_out_fp8(o, shift, lse=lse, heads_per_scale=2)
        got2, lse2 = call(v_shift=shift, out_fp8=dict(heads_per_scale=2), return_softmax_lse=True)
        assert same_bytes(got2.data, want2.data) and same_bits(got2.descale, want2.descale) and same_bits(lse2, lse)
        data, d, _ = emu.emulate(o, shift, lse, 2)                                 # and the pass itself: the emulation's bytes
        assert same_bytes(got2.data, data) and same_bits(got2.descale, d)


def test_smoothed_v_finish_fp8_keeps_its_buffers():
    import liteattention_amd as L
    q, k, xv = _fp8_inputs(seed=14)
    sv = L.SmoothedV()
    v8, dv, shift = sv(xv)
    o, lse = L.flash_attn_func(q, k, v8, v_descale=dv, return_softmax_lse=True)
    want = L.attn_out_fp8(o, shift, lse=lse)
    got = sv.finish(o, lse=lse, fp8=True)
    assert same_bytes(got.data, want.data) and same_bits(got.descale, want.descale)
    again = sv.finish(o, lse=lse, fp8=True)
    assert again.data.data_ptr() == got.data.data_ptr() == sv.out8.data_ptr() and again.descale.data_ptr() == sv.out_descale.data_ptr()
    ds = torch.tensor([0.02], device="cuda")
    st = sv.finish(o, lse=lse, fp8=True, descale=ds)
    assert st.descale is ds and same_bytes(st.data, emu.emulate(o, shift, lse, None, ds)[0])
    per_head = sv.finish(o, lse=lse, fp8=True, heads_per_scale=1)
    assert per_head.descale.shape == (1, 320, 4) and same_bits(per_head.descale, emu.emulate(o, shift, lse, 1)[1])


# ---- a HIP graph --------------------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay_give_the_eager_bytes():
    import liteattention_amd as L
    B, S, H, D = 1, 33, 40, 128
    o = make_o(B, S, H, D, seed=15)
    shift = make_shift(B, 20, D)
    lse, dot = make_lse(B, H, S)
    out = torch.empty(B, S, H, D, dtype=F8, device="cuda")
    ds = torch.empty(B, S, 1, device="cuda")
    lse_out = torch.empty(B, H, S, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        L.attn_out_fp8(o, shift, lse=lse, lse_dot=dot, out=out, descale_out=ds, lse_out=lse_out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r, l = L.attn_out_fp8(o, shift, lse=lse, lse_dot=dot, out=out, descale_out=ds, lse_out=lse_out)
    assert r.data.data_ptr() == out.data_ptr() and r.descale.data_ptr() == ds.data_ptr() and l.data_ptr() == lse_out.data_ptr()
    o.copy_(make_o(B, S, H, D, seed=16))
    out.view(torch.uint8).fill_(0x7f)
    ds.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    eager, lse_eager = L.attn_out_fp8(o, shift, lse=lse, lse_dot=dot)
    assert same_bytes(out, eager.data) and same_bits(ds, eager.descale) and same_bits(lse_out, lse_eager)
    data, d, _ = emu.emulate(o, shift, lse, None)
    assert same_bytes(out, data) and same_bits(ds, d)
