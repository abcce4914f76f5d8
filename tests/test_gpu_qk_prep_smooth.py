"""GPU: la_qk_prep_smooth (la_qk_prep_fp8 with a per-head shift of the keys, deterministic column sums and q . c row dots) against
`qk_prep_smooth_reference`, the same formula in torch fp64 from the same fp32 tables, weights, shifts and descales.

Acceptance rules, in the form tests/test_gpu_qk_prep_fp8.py derives its own. y64 is the fp64 value of the prologue, (a', b') the
normalised inputs of an element's rotation pair, pair_sum = |a'| + |b'|, d the descale, c the shift or the dot vector:

    quantized   z = clamp((y64 - shift) / d):  |got - z| <= 2^-4 |z| + 2^-10 + 2^-16 pair_sum / d + 2^-24 |shift| / d + 1e-7
                (half an ulp of a 3-bit mantissa, half the subnormal spacing, the fp32 arithmetic of y, the one fp32 subtraction)
    amax        |amax - amax64| <= 2^-16 max pair_sum + 2^-24 max |shift| + 1e-7
    mean        |mean - mean64| <= 2^-16 mean_s(pair_sum) + (rows_per_part + n_parts) 2^-24 mean_s |y| + 1e-7
                (every y is off by at most 2^-16 pair_sum; a part adds rows_per_part values in sequence, the finish n_parts)
    dots        |dot - dot64| <= sum_d (2^-16 pair_sum + D 2^-24 |y|) |c| + 1e-7

Shifts reach +-16 against y of order 1: a missed or doubled subtraction is off by many e4m3 ulps."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

F8 = torch.float8_e4m3fn
GRID = (3, 4, 5)


def grid_for(S):
    """GRID scaled along its first axis until it holds S positions."""
    return (max(3, -(-S // 20)), 4, 5)


def make_x(B, S, H, D, dtype=torch.bfloat16, seed=0):
    """N(0, 1) times a per-head scale in [0.25, 4]; the weight of a token norm in [0.5, 1.5] (as tests/test_gpu_qk_prep_fp8.py)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, H, D, generator=g) * (0.25 + 3.75 * torch.rand(1, 1, H, 1, generator=g))
    w = 0.5 + torch.rand(H * D, generator=g)
    return x.to(dtype).cuda(), w.cuda()


def make_vec(B, H, D, seed=0, span=16.0):
    """One value per (batch, head, column), uniform in [-span, span]: a wrong index shows."""
    g = torch.Generator().manual_seed(2000 + seed)
    return ((2.0 * torch.rand(B, H, D, generator=g) - 1.0) * span).cuda()


def tables_for(grid, D, parts=None):
    import liteattention_amd as L
    return L.rope_tables(grid, D, parts=parts, device="cuda")


def bits(t):
    return t.contiguous().view(torch.int32)


def check(x, weight, tables, norm="token", pos_offset=0, hps=1, hpd=1, eps=1e-6, label="", seed=0, sums=True, shift="draw", dots=True):
    """One quantizing launch with everything on, against the reference and the bounds of the module docstring; the part sums against
    a second launch and against the sums-only pass, bitwise. Returns (out, amax, mean, dots)."""
    import liteattention_amd as L
    B, S, H, D = x.shape
    G = H // hps
    if isinstance(shift, str):
        shift = make_vec(B, H, D, seed)
    c = make_vec(B, H // hpd, D, seed + 1) if dots else None
    kw = dict(norm=norm, pos_offset=pos_offset)
    z1, amax64, mean64, dots64 = L.qk_prep_smooth_reference(x, weight, eps, tables, shift=shift, heads_per_scale=hps, dot_vec=c,
                                                            heads_per_dot=hpd, **kw)
    g = torch.Generator().manual_seed(3000 + seed)
    descale = (amax64.clamp_min(1e-3) / 448.0 * (1.0 + 3.0 * torch.rand(B, G, generator=g).cuda().double())).float()
    z = (z1 / descale.double().repeat_interleave(hps, dim=1)[:, None, :, None]).clamp(-448, 448)
    n_parts, rows = L.qk_prep_smooth_parts(S, H, D)
    amax = torch.zeros(B, G, device="cuda")
    part = torch.full((n_parts, B, H, D), float("nan"), device="cuda") if sums else None
    dot_out = torch.full((B, H, S), float("nan"), device="cuda") if dots else None
    out = L.qk_prep_smooth(x, weight, eps, tables, shift=shift, descale=descale, amax_out=amax, heads_per_scale=hps, colsum_part=part,
                           dot_vec=c, heads_per_dot=hpd, dot_out=dot_out, **kw)
    assert out.dtype == F8 and out.shape == x.shape and out.is_contiguous()
    y = L.qk_prep_reference(x, weight, eps, None, norm=norm)                           # the normalised inputs (a', b') of every pair
    pair_sum = y.abs().reshape(*y.shape[:-1], -1, 2).sum(-1, keepdim=True).expand(*y.shape[:-1], -1, 2).reshape(y.shape)
    yr = L.qk_prep_reference(x, weight, eps, tables, norm=norm, pos_offset=pos_offset)
    d_el = descale.double().repeat_interleave(hps, dim=1)[:, None, :, None]
    sh = torch.zeros(B, H, D, device="cuda", dtype=torch.float64) if shift is None else shift.double()
    bound = 2.0 ** -4 * z.abs() + 2.0 ** -10 + 2.0 ** -16 * pair_sum / d_el + 2.0 ** -24 * sh.abs()[:, None] / d_el + 1e-7
    err = (out.double() - z).abs()
    a_bound = 2.0 ** -16 * pair_sum.reshape(B, S, G, hps * D).amax(dim=(1, 3)) + 2.0 ** -24 * sh.abs().reshape(B, G, hps * D).amax(2) + 1e-7
    a_err = (amax.double() - amax64).abs()
    msg = f"qk_prep_smooth {label or tuple(x.shape)} {x.dtype} norm={norm} hps={hps}: max err / bound {(err / bound).max().item():.3f}, " \
          f"amax {(a_err / a_bound).max().item():.3f}"
    assert not out.float().isnan().any()
    assert (err <= bound).all(), (label, (err / bound).max().item())
    assert (a_err <= a_bound).all(), (label, (a_err / a_bound).max().item())
    mean = None
    if sums:
        assert not part.isnan().any()                                                  # every element of every part is written
        mean = L.colsum_finish(part, S)
        m_bound = 2.0 ** -16 * pair_sum.mean(1) + (rows + n_parts) * 2.0 ** -24 * yr.abs().mean(1) + 1e-7
        m_err = (mean.double() - mean64).abs()
        msg += f", mean {(m_err / m_bound).max().item():.3f} ({n_parts} parts of {rows} rows)"
        assert (m_err <= m_bound).all(), (label, (m_err / m_bound).max().item())
        again = torch.full_like(part, float("nan"))
        L.qk_prep_smooth(x, weight, eps, tables, shift=shift, descale=descale, heads_per_scale=hps, colsum_part=again, **kw)
        assert torch.equal(bits(again), bits(part)), label                             # two launches: the same bits
        only = torch.full_like(part, float("nan"))
        assert L.qk_prep_smooth(x, weight, eps, tables, colsum_part=only, quantize=False, **kw) is None
        assert torch.equal(bits(only), bits(part)), label                              # the sums-only pass: the same bits
        assert torch.equal(bits(L.qk_prep_colmean(x, weight, eps, tables, **kw)), bits(mean)), label
    if dots:
        c_el = c.double().repeat_interleave(hpd, dim=1)[:, None].abs()
        d_bound = ((2.0 ** -16 * pair_sum + D * 2.0 ** -24 * yr.abs()) * c_el).sum(-1).permute(0, 2, 1) + 1e-7
        d_err = (dot_out.double() - dots64).abs()
        msg += f", dots {(d_err / d_bound).max().item():.3f}"
        assert not dot_out.isnan().any()
        assert (d_err <= d_bound).all(), (label, (d_err / d_bound).max().item())
        again = torch.full_like(dot_out, float("nan"))
        L.qk_prep_smooth(x, weight, eps, tables, dot_vec=c, heads_per_dot=hpd, dot_out=again, quantize=False, **kw)
        assert torch.equal(bits(again), bits(dot_out)), label                          # the dots-only pass: the same bits
    print(msg)
    return out, amax, mean, dot_out


def weight_for(w, norm, D):
    return None if norm is None else (w if norm == "token" else w[:D].contiguous())


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 63, 255, 256, 257, 600])
@pytest.mark.parametrize("norm", ["token", "head", None])
def test_row_counts_around_the_part_boundaries(S, norm):
    """Parts hold 16 rows at these lengths: 1 row, a last part of 15, exactly 16 parts, one row more, and 38 parts (10 blocks of 4)."""
    x, w = make_x(2, S, 3, 128, seed=S)
    check(x, weight_for(w, norm, 128), tables_for(grid_for(S), 128), norm=norm, seed=S)


@pytest.mark.parametrize("H,D,grid", [(3, 64, GRID), (5, 128, GRID), (12, 128, (2, 3, 2)), (24, 128, (2, 3, 2)), (40, 128, (2, 2, 2)),
                                      (48, 128, (2, 2, 2)), (40, 256, (2, 2, 1)), (64, 256, (2, 2, 1))])
def test_token_sizes_on_every_register_form(H, D, grid):
    """The list of tests/test_gpu_qk_prep_fp8.py: H * D = 192 ... 5120 (one wave per token), 6144 / 10240 / 16384 (one workgroup per
    token). The head kernel (head norm, no norm) serves the same shapes; it keeps column sums for at most 16 * (64 / G) heads and
    refuses the sums beyond (LA_ERR_UNSUPPORTED) while shift and dots still run."""
    import liteattention_amd as L
    S = grid[0] * grid[1] * grid[2]
    x, w = make_x(1, S, H, D, seed=H)
    tables = tables_for(grid, D)
    check(x, w, tables, seed=H)
    G = 1
    while 8 * G < D:
        G *= 2
    fits = H <= 16 * (64 // G)
    check(x, w[:D].contiguous(), tables, norm="head", seed=H, sums=fits)
    check(x, None, tables, norm=None, seed=H, sums=fits)
    if not fits:
        part = torch.zeros(L.qk_prep_smooth_parts(S, H, D)[0], 1, H, D, device="cuda")
        with pytest.raises(RuntimeError, match="outside the QK-Skip hot path"):
            L.qk_prep_smooth(x, None, 1e-6, tables, norm=None, colsum_part=part, quantize=False)
        assert (part == 0).all()


@pytest.mark.parametrize("D", [40, 64, 96, 128, 256])
@pytest.mark.parametrize("norm", ["token", "head", None])
def test_head_dims_with_wans_split(D, norm):
    x, w = make_x(2, 60, 3, D, seed=D)
    check(x, weight_for(w, norm, D), tables_for(GRID, D), norm=norm, seed=D)


@pytest.mark.parametrize("in_dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_dtypes(in_dtype):
    x, w = make_x(2, 60, 3, 128, dtype=in_dtype, seed=5)
    check(x, w, tables_for(GRID, 128))
    check(x, w[:128].contiguous(), tables_for(GRID, 128), norm="head")
    check(x, None, None, norm=None, label="no norm, no tables")


def test_more_blocks_than_the_grid_holds():
    """12 x 256 blocks of 4 parts of 16 rows against at most 2048 workgroups: the grid stride over blocks, both kernels."""
    grid = (164, 10, 10)
    x, w = make_x(12, 16384, 1, 8, seed=8)
    check(x, w, tables_for(grid, 8), label="grid stride")
    check(x, w, tables_for(grid, 8), norm="head", label="grid stride, head kernel")


# ---- GQA dots, strides, neighbours ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hpd", [1, 2, 4])
@pytest.mark.parametrize("norm", ["token", "head"])
def test_dots_of_grouped_query_heads(hpd, norm):
    """8 query heads, 8 / hpd dot vectors, each distinct (make_vec draws every row): a wrong group is off by its whole value."""
    x, w = make_x(2, 60, 8, 64, seed=hpd)
    check(x, weight_for(w, norm, 64), tables_for(GRID, 64), norm=norm, hps=hpd, hpd=hpd, seed=hpd)


@pytest.mark.parametrize("norm", ["token", None])
def test_strided_shift_and_untouched_neighbours(norm):
    """B = 2; shift and dot_vec are slices of larger buffers, the part sums and the dots sit inside larger poisoned buffers: the results
    are those of the contiguous call, bit for bit, and every word outside the addressed elements is unchanged."""
    import liteattention_amd as L
    B, S, H, D = 2, 60, 4, 64
    x, w = make_x(B, S, H, D, seed=31)
    tables, weight = tables_for(GRID, D), weight_for(w, norm, D)
    shift, c = make_vec(B, H, D, 31), make_vec(B, H // 2, D, 32)
    d = torch.full((B, H), 0.05, device="cuda")
    n_parts, _ = L.qk_prep_smooth_parts(S, H, D)
    want_part, want_dots = torch.empty(n_parts, B, H, D, device="cuda"), torch.empty(B, H, S, device="cuda")
    want = L.qk_prep_smooth(x, weight, 1e-6, tables, norm=norm, shift=shift, descale=d, colsum_part=want_part, dot_vec=c, heads_per_dot=2,
                            dot_out=want_dots)
    s_big = torch.full((B + 1, 2 * H + 1, D + 8), float("nan"), device="cuda")
    s_big[1:, 1:2 * H:2, 4:D + 4] = shift
    c_big = torch.full((B, H, 2 * D), float("nan"), device="cuda")
    c_big[:, 1::2, D:] = c
    p_big = torch.full((want_part.numel() + 32,), -7.0, device="cuda")
    t_big = torch.full((want_dots.numel() + 32,), -7.0, device="cuda")
    part, dots = p_big[16:-16].view(want_part.shape), t_big[16:-16].view(want_dots.shape)
    got = L.qk_prep_smooth(x, weight, 1e-6, tables, norm=norm, shift=s_big[1:, 1:2 * H:2, 4:D + 4], descale=d, colsum_part=part,
                           dot_vec=c_big[:, 1::2, D:], heads_per_dot=2, dot_out=dots)
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    assert torch.equal(bits(part), bits(want_part)) and torch.equal(bits(dots), bits(want_dots))
    for big in (p_big, t_big):
        assert (big[:16] == -7.0).all() and (big[-16:] == -7.0).all()
    with pytest.raises(RuntimeError, match="la_qk_prep_smooth"):                       # a shift row off a 16-byte boundary
        L.qk_prep_smooth(x, weight, 1e-6, tables, norm=norm, shift=s_big[1:, 1:2 * H:2, 2:D + 2])


def test_strided_q_and_k_slices_of_a_fused_projection_are_read_in_place():
    import liteattention_amd as L
    B, S, H, D = 2, 60, 3, 128
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(B, S, 3, H, D, generator=g).bfloat16().cuda()
    w = (0.5 + torch.rand(H * D, generator=g)).cuda()
    tables = tables_for(GRID, D)
    for which in (0, 1):
        x = qkv[:, :, which]
        assert not x.is_contiguous() and x.stride(1) == 3 * H * D
        want = check(x.contiguous(), w, tables, label=f"qkv slice {which} (contiguous copy)", seed=which)
        got = check(x, w, tables, label=f"qkv slice {which}", seed=which)
        for a, b in zip(want, got):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_pos_offset_equals_the_slice_of_the_full_run_bitwise():
    import liteattention_amd as L
    x, w = make_x(2, 60, 3, 128, seed=23)
    tables, shift, c = tables_for(GRID, 128), make_vec(2, 3, 128, 23), make_vec(2, 3, 128, 24)
    d = torch.full((2, 3), 0.05, device="cuda")
    full_dots = torch.empty(2, 3, 60, device="cuda")
    full = L.qk_prep_smooth(x, w, 1e-6, tables, shift=shift, descale=d, dot_vec=c, dot_out=full_dots)
    part_dots = torch.empty(2, 3, 17, device="cuda")
    part = L.qk_prep_smooth(x[:, 23:40], w, 1e-6, tables, pos_offset=23, shift=shift, descale=d, dot_vec=c, dot_out=part_dots)
    assert torch.equal(part.view(torch.uint8), full[:, 23:40].view(torch.uint8))
    assert torch.equal(bits(part_dots), bits(full_dots[:, :, 23:40]))
    check(x[:, 23:40], w, tables, pos_offset=23, label="pos_offset 23")
    with pytest.raises(RuntimeError, match="la_qk_prep_smooth"):
        L.qk_prep_smooth(x, w, 1e-6, tables, pos_offset=1, shift=shift)


# ---- nothing added, NaN -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["token", "head", None])
def test_without_extras_it_is_qk_prep_fp8_and_a_zero_shift_changes_no_bit(norm):
    import liteattention_amd as L
    for H in (5, 48):
        x, w = make_x(2, 60, H, 128, seed=H)
        tables, weight = tables_for(GRID, 128), weight_for(w, norm, 128)
        d = torch.full((2, H), 0.02, device="cuda")
        a0, a1, a2 = (torch.zeros(2, H, device="cuda") for _ in range(3))
        want = L.qk_prep_fp8(x, weight, 1e-6, tables, norm=norm, descale=d, amax_out=a0)
        got = L.qk_prep_smooth(x, weight, 1e-6, tables, norm=norm, descale=d, amax_out=a1)
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)) and torch.equal(bits(a0), bits(a1))
        zero = L.qk_prep_smooth(x, weight, 1e-6, tables, norm=norm, descale=d, amax_out=a2, shift=torch.zeros(2, H, 128, device="cuda"))
        assert torch.equal(zero.view(torch.uint8), want.view(torch.uint8)) and torch.equal(bits(a0), bits(a2))
        only = torch.zeros(2, H, device="cuda")
        assert L.qk_prep_smooth(x, weight, 1e-6, tables, norm=norm, amax_out=only, quantize=False) is None
        assert torch.equal(bits(only), bits(a0))


@pytest.mark.parametrize("norm", ["head", None])
def test_a_nan_makes_its_heads_mean_amax_and_dots_nan_and_no_others(norm):
    """Head norm / no norm (under a token norm a NaN poisons its whole token by definition): NaN planted in head 2 of batch 1, row 17."""
    import liteattention_amd as L
    x, w = make_x(2, 60, 6, 128, seed=11)
    x[1, 17, 2, 5] = float("nan")
    tables = tables_for(GRID, 128)
    amax, dots = torch.zeros(2, 6, device="cuda"), torch.empty(2, 6, 60, device="cuda")
    part = torch.empty(L.qk_prep_smooth_parts(60, 6, 128)[0], 2, 6, 128, device="cuda")
    L.qk_prep_smooth(x, w[:128].contiguous(), 1e-6, tables, norm=norm, shift=make_vec(2, 6, 128), amax_out=amax, colsum_part=part,
                     dot_vec=make_vec(2, 6, 128, 1), dot_out=dots)
    mean = L.colsum_finish(part, 60)
    assert amax[1, 2].isnan() and amax.isnan().sum().item() == 1
    assert dots[1, 2, 17].isnan() and dots.isnan().sum().item() == 1
    assert mean[1, 2, 5].isnan()
    mean[1, 2] = 0
    assert not mean.isnan().any()


# ---- SmoothedQK --------------------------------------------------------------------------------------------------------------------------
def code_order(t8):
    """e4m3 bytes as integers in value order (+-0 both 0): neighbouring codes differ by 1."""
    b = t8.view(torch.uint8).to(torch.int32)
    return torch.where(b >= 128, -(b - 128), b)


def offset_vector(H, D, size, seed):
    """+-size on 8 channels of every head, sign and channel drawn per head."""
    g = torch.Generator().manual_seed(seed)
    c = torch.zeros(H, D)
    for h in range(H):
        idx = torch.randperm(D, generator=g)[:8]
        c[h, idx] = size * (2.0 * torch.randint(0, 2, (8,), generator=g) - 1.0)
    return c


def test_current_mode_is_invariant_under_a_common_offset_of_the_keys():
    """fp32 input, norm=None, current mode: k against k + c with c = +-16 on 8 channels per head (seed 7). The codes differ in at most
    0.1 % of the elements and by one code step. The reference alone (fp64 formula on the two fp32 inputs, mean and amax in fp64, torch's
    e4m3 cast), for this seed: 1 of 163 840 codes differs, by one step - k + c rounds k's low bits away (an ulp of 2^-20 at 16), which
    can move a value across a rounding tie; the cap of 0.1 % is 163 codes. Measured on the device: 1 of 163 840, one step, equal
    descales."""
    import liteattention_amd as L
    B, S, H, D = 1, 320, 4, 128
    g = torch.Generator().manual_seed(7)
    k = torch.randn(B, S, H, D, generator=g)
    q = torch.randn(B, S, H, D, generator=g).cuda()
    k2 = k + offset_vector(H, D, 16.0, 7)[None, None]
    codes = []
    for kk in (k, k2):                                                                 # the reference alone, on the CPU
        _, _, mean64, _ = L.qk_prep_smooth_reference(kk, norm=None)
        z1, amax64, _, _ = L.qk_prep_smooth_reference(kk, norm=None, shift=mean64)
        codes.append(code_order((z1 / (amax64 / 448.0)[:, None, :, None]).float().to(F8)))
    ref_step = (codes[0] - codes[1]).abs()
    print(f"reference alone: {(ref_step > 0).sum().item()} of {ref_step.numel()} codes differ, largest step {ref_step.max().item()}")
    assert (ref_step > 0).float().mean().item() <= 1e-3 and ref_step.max().item() <= 1
    got = []
    for kk in (k, k2):
        s = L.SmoothedQK(mode="current")
        _, k8, _, dk, _ = s.pair(q, kk.cuda(), norm=None)
        got.append((code_order(k8), dk.clone()))
    step = (got[0][0] - got[1][0]).abs()
    print(f"device: {(step > 0).sum().item()} of {step.numel()} codes differ, largest step {step.max().item()}; descales differ by "
          f"{((got[0][1] - got[1][1]).abs() / got[0][1]).max().item():.2e} relative")
    assert (step > 0).float().mean().item() <= 1e-3 and step.max().item() <= 1


def test_delayed_mode_captures_into_a_hip_graph_and_replays():
    """Delayed mode, GQA (8 query heads on 4 key heads): the first call (no history) eager, then pair() captured once and replayed on
    three changing inputs; results, descales, LSE shifts and the state (mean, amaxes) equal the eager object's bit for bit."""
    import liteattention_amd as L
    tables = tables_for(GRID, 128)
    q, w_q = make_x(1, 60, 8, 128, seed=100)
    k, w_k = make_x(1, 60, 4, 128, seed=101)
    eager, graphed = L.SmoothedQK(mode="delayed", margin=1.25), L.SmoothedQK(mode="delayed", margin=1.25)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eager.pair(q, k, w_q, w_k, 1e-6, tables)
        graphed.pair(q, k, w_q, w_k, 1e-6, tables)
    torch.cuda.current_stream().wait_stream(s)
    ptrs = [t.data_ptr() for t in (graphed.q8, graphed.k8, graphed.mean, graphed.part)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g = graphed.pair(q, k, w_q, w_k, 1e-6, tables)
    assert ptrs == [t.data_ptr() for t in (graphed.q8, graphed.k8, graphed.mean, graphed.part)]
    for rep in range(3):
        q.copy_(make_x(1, 60, 8, 128, seed=200 + rep)[0] * (1.0 + 0.1 * rep))
        k.copy_(make_x(1, 60, 4, 128, seed=300 + rep)[0] + 2.0 * rep)
        mean_used = eager.mean.clone()
        g.replay()
        out_e = eager.pair(q, k, w_q, w_k, 1e-6, tables)
        torch.cuda.synchronize()
        for a, b in zip(out_g, out_e):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), rep
        for a, b in ((graphed.mean, eager.mean), (graphed.amax_k, eager.amax_k), (graphed.amax_q, eager.amax_q)):
            assert torch.equal(bits(a), bits(b)), rep
        # step t used step t - 1's mean: the LSE shift is q . that mean, and the state now holds this step's own mean
        _, _, mean64, dots64 = L.qk_prep_smooth_reference(q, w_q, 1e-6, tables, dot_vec=mean_used, heads_per_dot=2)
        assert (out_e[4].double() - dots64).abs().max().item() <= 1e-3 * (1.0 + dots64.abs().max().item())
        own = L.qk_prep_colmean(k, w_k, 1e-6, tables)
        assert torch.equal(bits(own), bits(eager.mean)), rep
    assert eager.calls == 4 and graphed.calls == 2                                     # (the capture ran pair() once, the replays none)


# ---- end to end through the fp8 attention call ---------------------------------------------------------------------------------------
def _attention_fp64(q, k, v, scale):
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * scale
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), v.double()), torch.logsumexp(s, dim=-1)


_CASES = {}


def _case(offset):
    """B = 1, S = 320, H = 2, D = 128, bf16 q / k / v, +-offset on 8 channels of every key head; the fp64 attention of those bf16
    values, computed once."""
    if offset not in _CASES:
        g = torch.Generator().manual_seed(0)
        q, k, v = (torch.randn(1, 320, 2, 128, generator=g) for _ in range(3))
        k = k + offset_vector(2, 128, float(offset), 1)[None, None]
        q, k, v = (t.bfloat16().cuda() for t in (q, k, v))
        _CASES[offset] = (q, k, v) + _attention_fp64(q, k, v, 128 ** -0.5)
    return _CASES[offset]


def _rel_rms(got, ref):
    return ((got.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


def _run_dense(offset):
    import liteattention_amd as L
    q, k, v, o64, lse64 = _case(offset)
    v8, dv = L.E4m3Scales()(v, norm=None)
    q8, dq = L.E4m3Scales()(q, norm=None)
    k8, dk = L.E4m3Scales()(k, norm=None)
    o_plain, lse_plain = L.flash_attn_func(q8, k8, v8, q_descale=dq, k_descale=dk, v_descale=dv, return_softmax_lse=True)
    sq, sk, sdq, sdk, lse_shift = L.SmoothedQK().pair(q, k, norm=None)
    o_smooth, lse_smooth = L.flash_attn_func(sq, sk, v8, q_descale=sdq, k_descale=sdk, v_descale=dv, return_softmax_lse=True)
    fixed = L.lse_unshift(lse_smooth, lse_shift, 128 ** -0.5)
    return (_rel_rms(o_plain, o64), _rel_rms(o_smooth, o64), (lse_plain.double() - lse64).abs().max().item(),
            (lse_smooth.double() - lse64).abs().max().item(), (fixed.double() - lse64).abs().max().item())


def test_dense_fp8_attention_gains_from_smoothing_when_the_keys_carry_an_offset():
    """Offset 16: the relative rms error of O against fp64 with SmoothedQK is at most 0.75 x the error with E4m3Scales (a CPU emulation
    with P kept in fp32 gives 0.42; an independent 0.04 for the device's e4m3 P gives about 0.53). The LSE after lse_unshift is within
    the fp8 LSE bound of the header, 0.084, and the uncorrected one is not: the correction matters on this input."""
    e_plain, e_smooth, l_plain, l_raw, l_fixed = _run_dense(16)
    print(f"offset 16: O rel rms plain {e_plain:.4f}, smoothed {e_smooth:.4f} (ratio {e_smooth / e_plain:.3f}); max |LSE error| plain "
          f"{l_plain:.4f}, smoothed uncorrected {l_raw:.4f}, after lse_unshift {l_fixed:.4f}")
    assert e_smooth <= 0.75 * e_plain
    assert l_fixed <= 0.084
    assert l_raw > 0.084


def test_dense_fp8_attention_loses_nothing_without_an_offset():
    """Offset 0: the smoothed error is at most 1.10 x the plain one (the emulation gives 0.98 - 1.01); the corrected LSE inside 0.084."""
    e_plain, e_smooth, l_plain, l_raw, l_fixed = _run_dense(0)
    print(f"offset 0: O rel rms plain {e_plain:.4f}, smoothed {e_smooth:.4f} (ratio {e_smooth / e_plain:.3f}); max |LSE error| plain "
          f"{l_plain:.4f}, smoothed uncorrected {l_raw:.4f}, after lse_unshift {l_fixed:.4f}")
    assert e_smooth <= 1.10 * e_plain
    assert l_fixed <= 0.084


def test_with_skip_lists_the_smoothed_run_is_no_further_from_dense_fp64():
    """Two LiteAttention steps at threshold -4 on the offset-16 input (the second walks the lists the first wrote); the listed fraction
    of both runs is printed."""
    import liteattention_amd as L
    q, k, v, o64, _ = _case(16)
    v8, dv = L.E4m3Scales()(v, norm=None)
    q8, dq = L.E4m3Scales()(q, norm=None)
    k8, dk = L.E4m3Scales()(k, norm=None)
    sq, sk, sdq, sdk, _ = L.SmoothedQK().pair(q, k, norm=None)
    errs, listed = [], []
    for qq, kk, d_q, d_k in ((q8, k8, dq, dk), (sq, sk, sdq, sdk)):
        la = L.LiteAttention(threshold=-4.0)
        la(qq, kk, v8, q_descale=d_q, k_descale=d_k, v_descale=dv)
        listed.append(1.0 - la.get_skip_fraction(batch=1))
        out = la(qq, kk, v8, q_descale=d_q, k_descale=d_k, v_descale=dv)
        errs.append(_rel_rms(out, o64))
    print(f"threshold -4, step 2: listed fraction plain {listed[0]:.4f}, smoothed {listed[1]:.4f}; O rel rms plain {errs[0]:.4f}, "
          f"smoothed {errs[1]:.4f}")
    assert errs[1] <= errs[0]


def test_the_op_equals_the_function():
    import liteattention_amd as L
    x, w = make_x(1, 60, 4, 128, seed=4)
    tables, shift, c = tables_for(GRID, 128), make_vec(1, 4, 128, 4), make_vec(1, 2, 128, 5)
    d = torch.full((1, 2), 0.05, device="cuda")
    a_op, a_fn = torch.zeros(1, 2, device="cuda"), torch.zeros(1, 2, device="cuda")
    t_op, t_fn = torch.empty(1, 4, 60, device="cuda"), torch.empty(1, 4, 60, device="cuda")
    got = torch.ops.lite_attention.qk_prep_smooth(x, w, 1e-6, list(tables.tables), list(tables.axis_pairs), "token", 0, shift, d, a_op, 2,
                                                  None, c, 2, t_op, None)
    want = L.qk_prep_smooth(x, w, 1e-6, tables, shift=shift, descale=d, amax_out=a_fn, heads_per_scale=2, dot_vec=c, heads_per_dot=2,
                            dot_out=t_fn)
    assert got.dtype == F8 and torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    assert torch.equal(a_op, a_fn) and (a_op > 0).all() and torch.equal(t_op, t_fn)
