"""GPU: la_qk_prep_fp8 (RMSNorm + 3-axis RoPE + per-head scale + e4m3 cast, and the per-head amax, in one pass) against
`qk_prep_fp8_reference`, the same formula in torch fp64 from the same fp32 tables, weights and descales.

Acceptance rule, derived in the form of tests/test_gpu_qk_prep.py, with z = clamp(ref64 / d, +-448), got = float(out) and (a', b') the
normalised inputs of the element's pair:

    |got - z| <= 2^-4 |z| + 2^-10 + 2^-16 (|a'| + |b'|) / d + 1e-7

2^-4 |z| is the half-ulp of a 3-bit mantissa, 2^-10 half the subnormal spacing 2^-9, the third term the fp32 arithmetic bound the bf16
test uses. A wrong column, axis, scale group or an `fnuz` encoding is off by a factor of 2 or more and cannot pass. The amax:
|amax - amax64| <= 2^-16 (largest pair sum of the group) + 1e-7, and the amax pass alone reports the same bits."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

F8 = torch.float8_e4m3fn
GRID = (3, 4, 5)


def make_x(B, S, H, D, dtype=torch.bfloat16, seed=0):
    """N(0, 1) times a per-head scale in [0.25, 4]; the weight of a token norm in [0.5, 1.5] (as tests/test_gpu_qk_prep.py)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, H, D, generator=g) * (0.25 + 3.75 * torch.rand(1, 1, H, 1, generator=g))
    w = 0.5 + torch.rand(H * D, generator=g)
    return x.to(dtype).cuda(), w.cuda()


def make_descale(B, G, seed=0):
    """One value per (batch, group), log-uniform in [2^-6, 2^2]: a wrong index shows."""
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.exp2(-6.0 + 8.0 * torch.rand(B, G, generator=g)).cuda()


def tables_for(grid, D, parts=None):
    import liteattention_amd as L
    return L.rope_tables(grid, D, parts=parts, device="cuda")


def check(x, weight, tables, norm="token", pos_offset=0, hps=1, descale="draw", eps=1e-6, label="", seed=0):
    import liteattention_amd as L
    B, S, H, D = x.shape
    G = H // hps
    if isinstance(descale, str):
        descale = make_descale(B, G, seed)
    amax = torch.zeros(B, G, device="cuda")
    out = L.qk_prep_fp8(x, weight, eps, tables, norm=norm, pos_offset=pos_offset, descale=descale, amax_out=amax, heads_per_scale=hps)
    assert out.dtype == F8 and out.shape == x.shape and out.is_contiguous()
    z, amax64 = L.qk_prep_fp8_reference(x, weight, eps, tables, norm=norm, pos_offset=pos_offset, descale=descale, heads_per_scale=hps)
    y = L.qk_prep_reference(x, weight, eps, None, norm=norm)                           # the normalised inputs (a', b') of every pair
    pair_sum = y.abs().reshape(*y.shape[:-1], -1, 2).sum(-1, keepdim=True).expand(*y.shape[:-1], -1, 2).reshape(y.shape)
    d = torch.ones(B, G, device="cuda", dtype=torch.float64) if descale is None else descale.double()
    d_el = d.repeat_interleave(hps, dim=1)[:, None, :, None]
    bound = 2.0 ** -4 * z.abs() + 2.0 ** -10 + 2.0 ** -16 * pair_sum / d_el + 1e-7
    err = (out.double() - z).abs()
    a_bound = 2.0 ** -16 * pair_sum.reshape(B, S, G, hps * D).amax(dim=(1, 3)) + 1e-7
    a_err = (amax.double() - amax64).abs()
    only = L.qk_prep_amax(x, weight, eps, tables, norm=norm, pos_offset=pos_offset, heads_per_scale=hps)
    print(f"qk_prep_fp8 {label or tuple(x.shape)} {x.dtype} norm={norm} hps={hps}: max err / bound {(err / bound).max().item():.3f}, "
          f"amax err / bound {(a_err / a_bound).max().item():.3f}, saturated {(out.float().abs() == 448).sum().item()} of {out.numel()}")
    assert not out.float().isnan().any()
    assert (err <= bound).all(), (label, (err / bound).max().item())
    assert (a_err <= a_bound).all(), (label, (a_err / a_bound).max().item())
    assert torch.equal(only.view(torch.int32), amax.view(torch.int32)), label         # the amax pass alone: the same bits
    return out, amax


# ---- the cast: every bf16 bit pattern --------------------------------------------------------------------------------------------------
def test_every_bf16_code_casts_as_torch_does():
    """x = all 65 536 bf16 patterns, no norm, no tables, descale 1: on every finite input (and +-inf, which saturates) the VALUE of the
    output equals torch's CPU cast of the clamped input - all ties, the subnormals, saturation at +-448; all 254 finite codes occur.
    Zeros compare by value (the sign of -0 is counted and printed); a NaN input gives a NaN byte."""
    import liteattention_amd as L
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).reshape(1, 64, 8, 128)
    x = bits.cuda()
    for mode, descale in (("descale NULL", None), ("descale 1", torch.ones(1, 8, device="cuda"))):
        out = L.qk_prep_fp8(x, norm=None, descale=descale).cpu()
        nan_in = bits.float().isnan()
        want = bits.float().clamp(-448, 448).to(F8)
        got_b, want_b = out.view(torch.uint8), want.view(torch.uint8)
        assert ((got_b[nan_in] & 0x7f) == 0x7f).all()
        ok = ~nan_in
        assert torch.equal(out.float()[ok], want.float()[ok])
        zero = ok & (want.float() == 0)
        print(f"{mode}: {(got_b[zero] != want_b[zero]).sum().item()} of {zero.sum().item()} zeros differ from torch in the sign bit; "
              f"{(got_b[ok & ~zero] != want_b[ok & ~zero]).sum().item()} non-zero codes differ")
        assert torch.equal(got_b[ok & ~zero], want_b[ok & ~zero])
        assert len(set(got_b[ok].tolist())) >= 254                                   # every finite code (+-0 may be one or two)


def test_fp32_and_fp16_inputs_cast_the_same_values():
    import liteattention_amd as L
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).reshape(1, 64, 8, 128)
    x32 = bits.float().cuda()
    out = L.qk_prep_fp8(x32, norm=None).cpu()
    ok = ~bits.float().isnan()
    assert torch.equal(out.float()[ok], bits.float().clamp(-448, 448).to(F8).float()[ok])
    h = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16).reshape(1, 64, 8, 128)
    out = L.qk_prep_fp8(h.cuda(), norm=None).cpu()
    ok = ~h.float().isnan()
    assert torch.equal(out.float()[ok], h.float().clamp(-448, 448).to(F8).float()[ok])


# ---- the shapes of the bf16 suite -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [40, 64, 96, 128, 256])
def test_head_dims_with_wans_split(D):
    x, w = make_x(2, 60, 3, D, seed=D)
    check(x, w, tables_for(GRID, D), seed=D)


@pytest.mark.parametrize("H,D,grid", [(3, 64, GRID), (5, 128, GRID), (12, 128, (2, 3, 2)), (24, 128, (2, 3, 2)), (40, 128, (2, 2, 2)),
                                      (48, 128, (2, 2, 2)), (40, 256, (2, 2, 1)), (64, 256, (2, 2, 1))])
def test_token_sizes_on_every_register_form(H, D, grid):
    """The list of tests/test_gpu_qk_prep.py: H * D = 192 ... 5120 (one wave per token), 6144 / 10240 / 16384 (one workgroup)."""
    S = grid[0] * grid[1] * grid[2]
    x, w = make_x(1, S, H, D, seed=H)
    check(x, w, tables_for(grid, D), seed=H)


def test_token_counts_that_do_not_fill_a_workgroup():
    x, w = make_x(2, 61, 3, 128, seed=61)
    check(x, w, tables_for((1, 1, 61), 128))
    check(x, w[:128].contiguous(), tables_for((1, 1, 61), 128), norm="head")


def test_more_tokens_than_the_grid_holds():
    grid = (10, 25, 40)
    x, w = make_x(2, 10000, 1, 8, seed=8)
    check(x, w, tables_for(grid, 8), label="grid stride")
    check(x, w, tables_for(grid, 8), norm="head", label="grid stride, head kernel")


@pytest.mark.parametrize("in_dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_dtypes(in_dtype):
    x, w = make_x(2, 60, 3, 128, dtype=in_dtype, seed=5)
    check(x, w, tables_for(GRID, 128))
    check(x, w[:128].contiguous(), tables_for(GRID, 128), norm="head")
    check(x, None, None, norm=None, label="the V form")


@pytest.mark.parametrize("norm", ["token", "head", None])
@pytest.mark.parametrize("rotate", ["wan", "none", "partial", "one_axis"])
@pytest.mark.parametrize("D", [64, 96])
def test_modes(norm, rotate, D):
    H, S = 5, 60
    x, w = make_x(2, S, H, D, seed=D + len(rotate))
    tables = {"wan": lambda: tables_for(GRID, D), "none": lambda: None,
              "partial": lambda: tables_for(GRID, D, parts=(D - 16 - 2 * (D // 4), D // 4, D // 4)),
              "one_axis": lambda: tables_for((S, 1, 1), D, parts=(D, 0, 0))}[rotate]()
    weight = None if norm is None else (w if norm == "token" else w[:D].contiguous())
    check(x, weight, tables, norm=norm, label=f"{norm}/{rotate}/D{D}")
    check(x, None, tables, norm=norm, descale=None, label=f"{norm}/{rotate}/D{D}/no weight, no descale")


def test_the_largest_head_count():
    """1024 heads of 8: the most a workgroup keeps scales for (token norm: H * D = 8192; head norm too)."""
    x, w = make_x(1, 8, 1024, 8, seed=3)
    check(x, w, tables_for((2, 2, 2), 8), hps=4)
    check(x, w[:8].contiguous(), tables_for((2, 2, 2), 8), norm="head")


# ---- scale groups, strides, neighbours ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hps", [1, 2, 4, 8])
@pytest.mark.parametrize("norm", ["token", None])
def test_scale_groups_with_strided_scales_and_untouched_neighbours(hps, norm):
    """H = 8; descale and amax are slices of larger poisoned buffers, out a slice of a larger poisoned e4m3 buffer: every byte outside
    the addressed elements is unchanged."""
    import liteattention_amd as L
    B, S, H, D = 2, 60, 8, 64
    G = H // hps
    x, w = make_x(B, S, H, D, seed=hps)
    tables = tables_for(GRID, D)
    weight = w if norm == "token" else None
    d = make_descale(B, G, seed=hps)
    want, want_amax = check(x, weight, tables, norm=norm, hps=hps, descale=d)
    d_big = torch.full((B + 2, 3 * G + 1), float("nan"), device="cuda")
    d_big[1:B + 1, 1:3 * G:3] = d
    a_big = torch.full((B + 1, 2 * G + 3), -7.0, device="cuda")
    a_view = a_big[1:, 2:2 * G + 2:2]
    a_view.zero_()
    o_big = torch.zeros((B + 1, S + 3, H + 2, D + 8), dtype=torch.uint8, device="cuda").fill_(0x5b).view(F8)
    before_a, before_o = a_big.clone(), o_big.clone()
    out = o_big[1:, 2:S + 2, 1:H + 1, :D]
    got = L.qk_prep_fp8(x, weight, 1e-6, tables, norm=norm, descale=d_big[1:B + 1, 1:3 * G:3], amax_out=a_view, heads_per_scale=hps, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out.view(torch.uint8), want.view(torch.uint8))
    assert torch.equal(a_view.contiguous().view(torch.int32), want_amax.view(torch.int32))
    mask = torch.ones(o_big.shape, dtype=torch.bool, device="cuda")
    mask[1:, 2:S + 2, 1:H + 1, :D] = False
    assert torch.equal(o_big.view(torch.uint8)[mask], before_o.view(torch.uint8)[mask])
    amask = torch.ones_like(a_big, dtype=torch.bool)
    amask[1:, 2:2 * G + 2:2] = False
    assert torch.equal(a_big[amask], before_a[amask])


def test_strided_q_and_k_slices_of_a_fused_projection_are_read_in_place():
    import liteattention_amd as L
    B, S, H, D = 2, 60, 3, 128
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(B, S, 3, H, D, generator=g).bfloat16().cuda()
    w = (0.5 + torch.rand(H * D, generator=g)).cuda()
    tables, d = tables_for(GRID, D), make_descale(B, H, seed=7)
    for which in (0, 1, 2):
        x = qkv[:, :, which]
        assert not x.is_contiguous() and x.stride(1) == 3 * H * D
        norm, weight, tabs = ("token", w, tables) if which < 2 else (None, None, None)
        want, _ = check(x.contiguous(), weight, tabs, norm=norm, descale=d, label=f"qkv slice {which} (contiguous copy)")
        got = L.qk_prep_fp8(x, weight, 1e-6, tabs, norm=norm, descale=d)
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))


# ---- amax ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["token", "head"])
def test_amax_is_a_running_maximum_and_two_launches_agree(norm):
    import liteattention_amd as L
    tables = tables_for(GRID, 128)
    for H in (5, 48):                                                                  # one wave per token / one workgroup per token
        x, w = make_x(2, 60, H, 128, seed=9)
        w = w if norm == "token" else w[:128].contiguous()
        a1 = L.qk_prep_amax(x, w, 1e-6, tables, norm=norm)
        a2 = L.qk_prep_amax(x, w, 1e-6, tables, norm=norm)
        assert torch.equal(a1.view(torch.int32), a2.view(torch.int32)) and (a1 > 0).all()
        pre = a1.clone()
        pre[0] *= 2.0                                                                  # larger: kept
        pre[1] *= 0.5                                                                  # smaller: raised
        got = L.qk_prep_amax(x, w, 1e-6, tables, norm=norm, amax_out=pre.clone())
        assert torch.equal(got[0], a1[0] * 2.0) and torch.equal(got[1], a1[1])
        d = make_descale(2, H, seed=H)
        o1 = L.qk_prep_fp8(x, w, 1e-6, tables, norm=norm, descale=d)
        o2 = L.qk_prep_fp8(x, w, 1e-6, tables, norm=norm, descale=d)
        assert torch.equal(o1.view(torch.uint8), o2.view(torch.uint8))
        for b in range(2):                                                             # a batch alone: the same bits
            ob = L.qk_prep_fp8(x[b:b + 1], w, 1e-6, tables, norm=norm, descale=d[b:b + 1])
            assert torch.equal(ob.view(torch.uint8), o1[b:b + 1].view(torch.uint8))


@pytest.mark.parametrize("norm", ["head", None])
def test_a_nan_makes_its_group_nan_and_no_other(norm):
    """Head norm / no norm (under a token norm a NaN poisons its whole token by definition): NaN planted in head 2 of batch 1."""
    import liteattention_amd as L
    x, w = make_x(2, 60, 6, 128, seed=11)
    x[1, 17, 2, 5] = float("nan")
    amax = torch.zeros(2, 3, device="cuda")
    out = L.qk_prep_fp8(x, w[:128].contiguous(), 1e-6, tables_for(GRID, 128), norm=norm, amax_out=amax, heads_per_scale=2)
    assert amax[1, 1].isnan() and amax.isnan().sum().item() == 1
    nan_out = out.float().isnan()
    assert nan_out[1, 17, 2].any() and not nan_out[0].any() and not nan_out[1, :, :2].any() and not nan_out[1, :, 3:].any()
    assert ((out.view(torch.uint8)[nan_out] & 0x7f) == 0x7f).all()
    only = L.qk_prep_amax(x, w[:128].contiguous(), 1e-6, tables_for(GRID, 128), norm=norm, heads_per_scale=2)
    assert torch.equal(only.isnan(), amax.isnan())


@pytest.mark.parametrize("norm", ["token", "head"])
def test_an_all_zero_token_or_head_gives_zeros_and_no_nan(norm):
    import liteattention_amd as L
    x, w = make_x(1, 60, 3, 128, seed=1)
    x[0, 17] = 0
    x[0, :, 1] = 0
    amax = torch.zeros(1, 3, device="cuda")
    out = L.qk_prep_fp8(x, w if norm == "token" else w[:128].contiguous(), 1e-6, tables_for(GRID, 128), norm=norm,
                        descale=make_descale(1, 3), amax_out=amax)
    assert not out.float().isnan().any() and not amax.isnan().any()
    assert (out[0, 17].float() == 0).all() and (out[0, :, 1].float() == 0).all() and (out[0, 16, 0].float() != 0).any()
    assert amax[0, 1].item() == 0.0 and amax[0, 0].item() > 0
    s = L.E4m3Scales()                                                                 # ... and through the scales made from that amax
    x8, d = s(x, w if norm == "token" else w[:128].contiguous(), 1e-6, tables_for(GRID, 128), norm=norm)
    assert not x8.float().isnan().any() and (x8[0, :, 1].float() == 0).all() and torch.isfinite(d).all() and (d > 0).all()


def test_saturation_is_exact_and_local():
    """Head 1's descale 4 x too small: exactly +-448 where |z| >= 448, no NaN, the other heads' bytes as before."""
    import liteattention_amd as L
    x, w = make_x(2, 60, 3, 128, seed=13)
    tables = tables_for(GRID, 128)
    d = L.descale_from_amax(L.qk_prep_amax(x, w, 1e-6, tables), margin=1.01)           # the good heads stay below 448 / 1.01
    good = L.qk_prep_fp8(x, w, 1e-6, tables, descale=d)
    d_bad = d.clone()
    d_bad[:, 1] /= 4.0
    out, _ = check(x, w, tables, descale=d_bad, label="saturating")
    z, _ = L.qk_prep_fp8_reference(x, w, 1e-6, tables, descale=d_bad)
    sat = z.abs() >= 448
    assert sat[:, :, 1].any() and not sat[:, :, 0].any() and not sat[:, :, 2].any()
    assert torch.equal(out.float()[sat].double(), z[sat]) and not out.float().isnan().any()
    assert torch.equal(out[:, :, 0].view(torch.uint8), good[:, :, 0].view(torch.uint8))
    assert torch.equal(out[:, :, 2].view(torch.uint8), good[:, :, 2].view(torch.uint8))


def test_consistency_with_the_bf16_path_is_printed():
    """descale 1, y inside +-448: qk_prep_fp8(x) against qk_prep(x) -> bf16 -> e4m3; they may differ where double rounding does. The
    share is printed, not asserted; that both obey the rule against fp64 is (check)."""
    import liteattention_amd as L
    x, w = make_x(2, 60, 5, 128, seed=21)
    tables = tables_for(GRID, 128)
    out, _ = check(x, w, tables, descale=None)
    two_step = L.qk_prep(x, w, 1e-6, tables, out_dtype=torch.bfloat16).float().to(F8)
    differ = (out.view(torch.uint8) != two_step.view(torch.uint8)).sum().item()
    print(f"qk_prep_fp8 vs qk_prep -> bf16 -> e4m3: {differ} of {out.numel()} bytes differ ({differ / out.numel():.4%})")
    assert (out.float() - two_step.float()).abs().max().item() <= 32.0                  # at most one e4m3 step (the largest is 32)


# ---- other cases -----------------------------------------------------------------------------------------------------------------------
def test_pos_offset_equals_the_slice_of_the_full_run_bitwise():
    import liteattention_amd as L
    x, w = make_x(2, 60, 3, 128, seed=23)
    tables, d = tables_for(GRID, 128), make_descale(2, 3, seed=23)
    full = L.qk_prep_fp8(x, w, 1e-6, tables, descale=d)
    part = L.qk_prep_fp8(x[:, 23:40], w, 1e-6, tables, pos_offset=23, descale=d)
    assert torch.equal(part.view(torch.uint8), full[:, 23:40].view(torch.uint8))
    with pytest.raises(RuntimeError, match="la_qk_prep_fp8"):
        L.qk_prep_fp8(x, w, 1e-6, tables, pos_offset=1)


def test_the_op_equals_the_function():
    import liteattention_amd as L
    x, w = make_x(1, 60, 4, 128, seed=4)
    tables, d = tables_for(GRID, 128), make_descale(1, 2, seed=4)
    a_op, a_fn = torch.zeros(1, 2, device="cuda"), torch.zeros(1, 2, device="cuda")
    got = torch.ops.lite_attention.qk_prep_fp8(x, w, 1e-6, list(tables.tables), list(tables.axis_pairs), "token", 0, d, a_op, 2, None)
    want = L.qk_prep_fp8(x, w, 1e-6, tables, descale=d, amax_out=a_fn, heads_per_scale=2)
    assert got.dtype == F8 and torch.equal(got.view(torch.uint8), want.view(torch.uint8)) and torch.equal(a_op, a_fn) and (a_op > 0).all()


def test_current_scaling_captures_into_a_hip_graph_and_replays():
    """(amax pass, descale_from_amax, quantizing pass) for q and k on a single branch; tables built and a warm-up run before the
    capture; three replays on changing inputs equal the eager sequence bitwise."""
    import liteattention_amd as L
    tables = tables_for(GRID, 128)
    q, w_q = make_x(1, 60, 5, 128, seed=100)
    k, w_k = make_x(1, 60, 5, 128, seed=101)

    def sequence(x, w, amax, descale, out):
        amax.zero_()
        L.qk_prep_amax(x, w, 1e-6, tables, amax_out=amax)
        L.descale_from_amax(amax, 1.0, out=descale)
        return L.qk_prep_fp8(x, w, 1e-6, tables, descale=descale, out=out)

    def buffers():
        return torch.zeros(1, 5, device="cuda"), torch.zeros(1, 5, device="cuda"), torch.empty(1, 60, 5, 128, dtype=F8, device="cuda")

    gq_buf, gk_buf, eq_buf, ek_buf = buffers(), buffers(), buffers(), buffers()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        sequence(q, w_q, *eq_buf)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sequence(q, w_q, *gq_buf)
        sequence(k, w_k, *gk_buf)
    for rep in range(3):
        q.copy_(make_x(1, 60, 5, 128, seed=200 + rep)[0] * (rep + 1))
        k.copy_(make_x(1, 60, 5, 128, seed=300 + rep)[0])
        g.replay()
        sequence(q, w_q, *eq_buf)
        sequence(k, w_k, *ek_buf)
        torch.cuda.synchronize()
        for gb, eb in ((gq_buf, eq_buf), (gk_buf, ek_buf)):
            assert torch.equal(gb[2].view(torch.uint8), eb[2].view(torch.uint8)) and torch.equal(gb[1], eb[1]) and torch.equal(gb[0], eb[0]), rep
    assert gq_buf[2].float().abs().max().item() == 448.0


# ---- end to end: the demo block in fp8 -------------------------------------------------------------------------------------------------
def _block_fp64(blk, x, grid):
    """The demo's self-attention block evaluated in fp64 on the CPU from the module's own weights (as tests/test_gpu_qk_prep.py)."""
    import liteattention_amd as L
    n, d = blk.num_heads, blk.head_dim
    x = x.double().cpu()

    def lin(m, t):
        return t @ m.weight.detach().double().cpu().T + m.bias.detach().double().cpu()

    b, s = x.shape[:2]
    tables = L.rope_tables(grid, d)
    q = L.qk_prep_reference(lin(blk.q, x).view(b, s, n, d), blk.norm_q.weight.detach().cpu(), blk.norm_q.eps, tables)
    k = L.qk_prep_reference(lin(blk.k, x).view(b, s, n, d), blk.norm_k.weight.detach().cpu(), blk.norm_k.eps, tables)
    v = lin(blk.v, x).view(b, s, n, d)
    p = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k) * d ** -0.5, dim=-1)
    return lin(blk.o, torch.einsum("bhqk,bkhd->bqhd", p, v).reshape(b, s, n * d))


def _eager_fp8_block(blk, x, grid):
    """The yardstick: the demo's own eager lines (norm, rope), then per-head amax, scale, clamp, .to(float8) in eager torch, and the same
    descales into the same attention call."""
    import wan_self_attention_demo as demo
    b, s, n, d = *x.shape[:2], blk.num_heads, blk.head_dim
    q = demo.rope_3d(blk.norm_q(blk.q(x)).view(b, s, n, d), grid)
    k = demo.rope_3d(blk.norm_k(blk.k(x)).view(b, s, n, d), grid)
    v = blk.v(x).view(b, s, n, d)
    ops = []
    for t in (q, k, v):
        desc = t.float().abs().amax(dim=(1, 3)).clamp_min(2.0 ** -100) / 448.0
        ops += [(t.float() / desc[:, None, :, None]).clamp(-448, 448).to(F8), desc]
    out = blk.lite_attention(ops[0], ops[2], ops[4], q_descale=ops[1], k_descale=ops[3], v_descale=ops[5])
    return blk.o(out.float().flatten(2))


def test_demo_block_in_fp8_is_as_close_to_fp64_as_the_eager_fp8_block():
    """Frames 4, height 16, width 20, heads 3, threshold -60 (nothing skipped), current scaling: e_fused <= 2 e_eager + 1e-6 and
    e_eager < 0.05 max|ref| - the rule and the sanity bound of the bf16 test, for the same reason."""
    import wan_self_attention_demo as demo
    torch.manual_seed(0)
    heads, grid = 3, (4, 16, 20)
    dim, S = heads * 128, 4 * 16 * 20
    eager = demo.WanLikeSelfAttention(dim, heads, threshold=-60.0).cuda()
    eager.k.load_state_dict(eager.q.state_dict())
    with torch.no_grad():
        eager.norm_q.weight.copy_(0.5 + torch.rand(dim))
        eager.norm_k.weight.copy_(0.5 + torch.rand(dim))
    fused = demo.WanLikeSelfAttention(dim, heads, threshold=-60.0, fp8=True).cuda()
    fused.load_state_dict(eager.state_dict())
    x = torch.randn(1, 4, 1, dim).expand(1, 4, 16 * 20, dim).reshape(1, S, dim) * 2.0 + 0.5 * torch.randn(1, S, dim)
    x = x.cuda()
    with torch.no_grad():
        y_eager, y_fused = _eager_fp8_block(eager, x, grid), fused(x, grid)
        ref = _block_fp64(eager, x, grid)
    assert eager.lite_attention.get_skip_fraction(batch=1) == 0.0 and fused.lite_attention.get_skip_fraction(batch=1) == 0.0
    e_eager = (y_eager.double().cpu() - ref).abs().max().item()
    e_fused = (y_fused.double().cpu() - ref).abs().max().item()
    print(f"fp8 demo block vs fp64: eager {e_eager:.3e}, fused {e_fused:.3e} (|ref| max {ref.abs().max().item():.3f})")
    assert e_eager < 0.05 * ref.abs().max().item()                                     # the yardstick itself is sane
    assert e_fused <= 2.0 * e_eager + 1e-6


def test_demo_run_in_fp8_delayed_scaling_skips_as_current_scaling_does():
    """Threshold -6, 5 steps, margin 1.25 (the noise level falls: the amax does not outgrow it): finite output, a skip fraction that
    grows monotonically and stays within 0.05 absolute of the current-scaling run at every step."""
    import wan_self_attention_demo as demo
    cur = demo.run(frames=4, height=16, width=20, heads=3, steps=5, threshold=-6.0, verbose=False, fp8=True)
    dly = demo.run(frames=4, height=16, width=20, heads=3, steps=5, threshold=-6.0, verbose=False, fp8=True, fp8_mode="delayed",
                   fp8_margin=1.25)
    s_c, s_d = [r[1] for r in cur], [r[1] for r in dly]
    print("fp8 skip fractions current", [f"{v:.4f}" for v in s_c], "delayed", [f"{v:.4f}" for v in s_d], "errors", [f"{r[2]:.2e}" for r in dly])
    assert all(r[2] == r[2] and abs(r[2]) != float("inf") for r in dly)               # finite
    assert s_d == sorted(s_d)
    assert all(abs(a - b) <= 0.05 for a, b in zip(s_c, s_d))
