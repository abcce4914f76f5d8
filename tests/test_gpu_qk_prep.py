"""GPU: la_qk_prep (RMSNorm + 3-axis RoPE + cast in one pass) against `qk_prep_reference`, the same formula in torch fp64 computed from
the same fp32 tables and weights.

Acceptance rule, derived, for the output element of a pair whose normalised inputs are (a', b'):

    |out - ref64| <= u |ref64| + 2^-16 (|a'| + |b'|) + 1e-7

u = 2^-8 (bf16) / 2^-11 (fp16) is the unit roundoff of the ONE rounding at the store; the second term bounds the fp32 arithmetic before
it (a serial sum of at most 256 squares per lane plus a handful of operations, about 100 * 2^-24) and is still 250 x (bf16) / 32 x (fp16)
below u: a wrong column, sign, axis or coordinate is an error of order |a'| + |b'| and cannot pass. Every case also prints how many
elements are not bit-equal to the rounded fp64 value (not asserted)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
GRID = (3, 4, 5)


def make_x(B, S, H, D, dtype=torch.bfloat16, seed=0):
    """N(0, 1) times a per-head scale in [0.25, 4]; the weight of a token norm in [0.5, 1.5]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, H, D, generator=g) * (0.25 + 3.75 * torch.rand(1, 1, H, 1, generator=g))
    w = 0.5 + torch.rand(H * D, generator=g)
    return x.to(dtype).cuda(), w.cuda()


def check(x, weight, tables, norm="token", pos_offset=0, out_dtype=torch.bfloat16, eps=1e-6, label=""):
    import liteattention_amd as L
    out = L.qk_prep(x, weight, eps, tables, norm=norm, pos_offset=pos_offset, out_dtype=out_dtype)
    assert out.dtype == out_dtype and out.shape == x.shape and out.is_contiguous()
    ref = L.qk_prep_reference(x, weight, eps, tables, norm=norm, pos_offset=pos_offset)
    y = L.qk_prep_reference(x, weight, eps, None, norm=norm)                           # the normalised inputs (a', b') of every pair
    pair_sum = y.abs().reshape(*y.shape[:-1], -1, 2).sum(-1, keepdim=True).expand(*y.shape[:-1], -1, 2).reshape(y.shape)
    bound = U[out_dtype] * ref.abs() + 2.0 ** -16 * pair_sum + 1e-7
    err = (out.double() - ref).abs()
    not_exact = (out != ref.to(out_dtype)).sum().item()
    print(f"qk_prep {label or tuple(x.shape)} {x.dtype}->{out_dtype} norm={norm}: max err / bound {(err / bound).max().item():.3f}, "
          f"{not_exact} of {out.numel()} elements not bit-equal to the rounded fp64 value")
    assert torch.isfinite(out.float()).all()
    assert (err <= bound).all(), (label, (err / bound).max().item())
    return out


def tables_for(grid, D, parts=None):
    import liteattention_amd as L
    return L.rope_tables(grid, D, parts=parts, device="cuda")


@pytest.mark.parametrize("D", [40, 64, 96, 128, 256])
def test_head_dims_with_wans_split(D):
    """Axis boundaries inside a lane's 16-byte chunk (D = 128: elements 44 and 86; D = 64: 24 and 44)."""
    x, w = make_x(2, 60, 3, D, seed=D)
    check(x, w, tables_for(GRID, D))


@pytest.mark.parametrize("H,D,grid", [(3, 64, GRID), (5, 128, GRID), (12, 128, (2, 3, 2)), (24, 128, (2, 3, 2)), (40, 128, (2, 2, 2)),
                                      (48, 128, (2, 2, 2)), (40, 256, (2, 2, 1)), (64, 256, (2, 2, 1))])
def test_token_sizes_on_every_register_form(H, D, grid):
    """H * D = 192 / 640 (a partial first / second pass of a wave's 512 elements), 1536, 3072, 5120 (the model's size: 10 chunks per lane,
    one wave per token), 6144 / 10240 / 16384 (one workgroup per token: 4 and 8 chunks per lane; 16384 is the largest accepted)."""
    S = grid[0] * grid[1] * grid[2]
    x, w = make_x(1, S, H, D, seed=H)
    check(x, w, tables_for(grid, D))


def test_token_norm_above_16384_elements_is_refused():
    import liteattention_amd as L
    x = torch.zeros(1, 4, 2049, 8, dtype=torch.bfloat16, device="cuda")                 # H * D = 16392
    with pytest.raises(RuntimeError, match="la_qk_prep"):
        L.qk_prep(x, None, norm="token")
    assert L.qk_prep(x, None, norm="head").shape == x.shape                             # the limit is the token norm's


def test_token_counts_that_do_not_fill_a_workgroup():
    x, w = make_x(2, 61, 3, 128, seed=61)
    check(x, w, tables_for((1, 1, 61), 128))


def test_more_tokens_than_the_grid_holds():
    """20 000 tokens of 8 elements: 2 048 workgroups of 4 tokens each run the grid-stride loop more than twice."""
    grid = (10, 25, 40)
    x, w = make_x(2, 10000, 1, 8, seed=8)
    check(x, w, tables_for(grid, 8), label="grid stride")
    check(x, w, tables_for(grid, 8), norm="head", label="grid stride, head kernel")


@pytest.mark.parametrize("in_dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16])
def test_dtypes(in_dtype, out_dtype):
    x, w = make_x(2, 60, 3, 128, dtype=in_dtype, seed=5)
    check(x, w, tables_for(GRID, 128), out_dtype=out_dtype)
    check(x, w[:128].contiguous(), tables_for(GRID, 128), norm="head", out_dtype=out_dtype)


@pytest.mark.parametrize("norm", ["token", "head", None])
@pytest.mark.parametrize("rotate", ["wan", "none", "partial", "one_axis"])
@pytest.mark.parametrize("D", [64, 96])
def test_modes(norm, rotate, D):
    """Token / head / no norm x Wan's split / no tables / partial rotary (parts summing to D - 16) / 1-D RoPE; with and without weight."""
    H, S = 5, 60
    x, w = make_x(2, S, H, D, seed=D + len(rotate))
    tables = {"wan": lambda: tables_for(GRID, D), "none": lambda: None,
              "partial": lambda: tables_for(GRID, D, parts=(D - 16 - 2 * (D // 4), D // 4, D // 4)),
              "one_axis": lambda: tables_for((S, 1, 1), D, parts=(D, 0, 0))}[rotate]()
    weight = None if norm is None else (w if norm == "token" else w[:D].contiguous())
    check(x, weight, tables, norm=norm, label=f"{norm}/{rotate}/D{D}")
    check(x, None, tables, norm=norm, label=f"{norm}/{rotate}/D{D}/no weight")


def test_strided_views_and_untouched_neighbours():
    """x = the q slice, then the k slice, of a fused (B, S, 3, H, D) projection; out = a slice of a larger poisoned buffer, of which every
    byte outside the addressed elements is unchanged (the method of tests/test_gpu_layout_poison.py)."""
    import liteattention_amd as L
    B, S, H, D = 2, 60, 3, 128
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(B, S, 3, H, D, generator=g).bfloat16().cuda()
    w = (0.5 + torch.rand(H * D, generator=g)).cuda()
    tables = tables_for(GRID, D)
    for which in (0, 1):
        x = qkv[:, :, which]
        assert not x.is_contiguous() and x.stride(1) == 3 * H * D
        want = check(x.contiguous(), w, tables, label=f"qkv slice {which} (contiguous copy)")
        big = torch.full((B + 1, S + 3, H + 2, D + 8), float("nan"), dtype=torch.bfloat16, device="cuda")
        big.view(torch.int16).fill_(0x7fa5)                                            # a NaN pattern no kernel writes
        before = big.clone()
        out = big[1:, 2:S + 2, 1:H + 1, :D]
        got = L.qk_prep(x, w, 1e-6, tables, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(out, want)
        mask = torch.ones_like(big, dtype=torch.bool)
        mask[1:, 2:S + 2, 1:H + 1, :D] = False
        assert torch.equal(big.view(torch.int16)[mask], before.view(torch.int16)[mask])


@pytest.mark.parametrize("norm", ["token", "head"])
def test_in_place_equals_out_of_place_bitwise(norm):
    import liteattention_amd as L
    tables = tables_for(GRID, 128)
    for H in (5, 48):                                                                  # one wave per token / one workgroup per token
        x, w = make_x(2, 60, H, 128, seed=9)
        w = w if norm == "token" else w[:128].contiguous()
        want = L.qk_prep(x, w, 1e-6, tables, norm=norm)
        buf = x.clone()
        got = L.qk_prep(buf, w, 1e-6, tables, norm=norm, out=buf)
        assert got.data_ptr() == buf.data_ptr() and torch.equal(buf, want)


def test_pos_offset_equals_the_slice_of_the_full_run_bitwise():
    import liteattention_amd as L
    x, w = make_x(2, 60, 3, 128, seed=23)
    tables = tables_for(GRID, 128)
    full = L.qk_prep(x, w, 1e-6, tables)
    part = L.qk_prep(x[:, 23:40], w, 1e-6, tables, pos_offset=23)
    assert torch.equal(part, full[:, 23:40])
    with pytest.raises(RuntimeError, match="la_qk_prep"):
        L.qk_prep(x, w, 1e-6, tables, pos_offset=1)                                    # 1 + 60 rows on 60 positions


def test_batches_and_launches_agree_bitwise():
    import liteattention_amd as L
    x, w = make_x(2, 60, 40, 128, seed=40)
    tables = tables_for(GRID, 128)
    both = L.qk_prep(x, w, 1e-6, tables)
    assert torch.equal(L.qk_prep(x, w, 1e-6, tables), both)                            # two launches of one call
    for b in range(2):
        assert torch.equal(L.qk_prep(x[b:b + 1], w, 1e-6, tables), both[b:b + 1])


@pytest.mark.parametrize("norm", ["token", "head"])
def test_an_all_zero_token_gives_zeros_and_no_nan(norm):
    import liteattention_amd as L
    x, w = make_x(1, 60, 3, 128, seed=1)
    x[0, 17] = 0
    x[0, 33, 1] = 0
    out = L.qk_prep(x, w if norm == "token" else w[:128].contiguous(), 1e-6, tables_for(GRID, 128), norm=norm)
    assert torch.isfinite(out.float()).all()
    assert (out[0, 17] == 0).all() and (out[0, 33, 1] == 0).all() and (out[0, 16] != 0).any()


def test_q_and_k_capture_into_a_hip_graph_and_replay():
    """The single-branch capture of tests/test_gpu_wan_block.py: tables built before the capture, warm-up on a side stream; three
    replays on changing inputs equal the eager pair bitwise."""
    import liteattention_amd as L
    tables = tables_for(GRID, 128)
    q, w_q = make_x(1, 60, 5, 128, seed=100)
    k, w_k = make_x(1, 60, 5, 128, seed=101)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        L.qk_prep(q, w_q, 1e-6, tables)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gq = L.qk_prep(q, w_q, 1e-6, tables)
        gk = L.qk_prep(k, w_k, 1e-6, tables)
    for rep in range(3):
        q.copy_(make_x(1, 60, 5, 128, seed=200 + rep)[0])
        k.copy_(make_x(1, 60, 5, 128, seed=300 + rep)[0])
        g.replay()
        eq, ek = L.qk_prep(q, w_q, 1e-6, tables), L.qk_prep(k, w_k, 1e-6, tables)
        torch.cuda.synchronize()
        assert torch.equal(gq, eq) and torch.equal(gk, ek), rep
    assert gq.abs().max().item() > 0


def test_the_op_is_registered_beside_fwd():
    import liteattention_amd as L
    x, w = make_x(1, 60, 3, 128, seed=4)
    tables = tables_for(GRID, 128)
    got = torch.ops.lite_attention.qk_prep(x, w, 1e-6, list(tables.tables), list(tables.axis_pairs), "token", 0, None, None)
    assert torch.equal(got, L.qk_prep(x, w, 1e-6, tables))
    meta = torch.ops.lite_attention.qk_prep(x.to("meta"), None, 1e-6, None, None, "token", 0, None, torch.float16)
    assert meta.shape == x.shape and meta.dtype == torch.float16 and meta.device.type == "meta"


# ---- end to end: the demo block with the fused prologue against the block as it was --------------------------------------------------
def _block_fp64(blk, x, grid):
    """The demo's self-attention block evaluated in fp64 on the CPU from the module's own weights (no bf16 anywhere)."""
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


def test_demo_block_with_fused_prologue_is_as_close_to_fp64_as_the_eager_block():
    """Frames 4, height 16, width 20, heads 3, threshold -60 (nothing skipped). The yardstick is the existing path: the fused block's
    max-abs error against fp64 is at most 2 x the eager block's own + 1e-6 (q and k each lose at most one rounding of difference, in
    either direction)."""
    import wan_self_attention_demo as demo
    torch.manual_seed(0)
    heads, grid = 3, (4, 16, 20)
    dim, S = heads * 128, 4 * 16 * 20
    eager = demo.WanLikeSelfAttention(dim, heads, threshold=-60.0).cuda()
    eager.k.load_state_dict(eager.q.state_dict())
    with torch.no_grad():
        eager.norm_q.weight.copy_(0.5 + torch.rand(dim))
        eager.norm_k.weight.copy_(0.5 + torch.rand(dim))
    fused = demo.WanLikeSelfAttention(dim, heads, threshold=-60.0, fused_prep=True).cuda()
    fused.load_state_dict(eager.state_dict())
    x = torch.randn(1, 4, 1, dim).expand(1, 4, 16 * 20, dim).reshape(1, S, dim) * 2.0 + 0.5 * torch.randn(1, S, dim)
    x = x.cuda()
    with torch.no_grad():
        y_eager, y_fused = eager(x, grid), fused(x, grid)
        ref = _block_fp64(eager, x, grid)
    assert eager.lite_attention.get_skip_fraction(batch=1) == 0.0 and fused.lite_attention.get_skip_fraction(batch=1) == 0.0
    e_eager = (y_eager.double().cpu() - ref).abs().max().item()
    e_fused = (y_fused.double().cpu() - ref).abs().max().item()
    print(f"demo block vs fp64: eager {e_eager:.3e}, fused {e_fused:.3e} (|ref| max {ref.abs().max().item():.3f})")
    assert e_eager < 0.05 * ref.abs().max().item()                                     # the yardstick itself is sane
    assert e_fused <= 2.0 * e_eager + 1e-6


def test_demo_run_skips_alike_with_and_without_the_fused_prologue():
    """Threshold -6, 5 steps: the fused block's skip fraction is within 0.05 absolute of the eager block's at every step and grows
    monotonically (lists need not be equal: the operands differ by a rounding)."""
    import wan_self_attention_demo as demo
    eager = demo.run(frames=4, height=16, width=20, heads=3, steps=5, threshold=-6.0, verbose=False)
    fused = demo.run(frames=4, height=16, width=20, heads=3, steps=5, threshold=-6.0, verbose=False, fused_prep=True)
    s_e, s_f = [r[1] for r in eager], [r[1] for r in fused]
    print("skip fractions eager", [f"{v:.4f}" for v in s_e], "fused", [f"{v:.4f}" for v in s_f])
    assert s_f == sorted(s_f)
    assert all(abs(a - b) <= 0.05 for a, b in zip(s_e, s_f))
    assert s_f[-1] > 0.05 and all(r[2] < 2e-2 for r in fused)


def test_cross_attention_block_with_fused_prologue():
    """The text cross-attention of the demo (no rope: norm + cast only, ragged prompts) with `fused_prep` against its own reference and
    against the eager block, the rule of tests/test_gpu_wan_block.py."""
    import wan_self_attention_demo as demo
    shims = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "compat_shims")
    sys.path.insert(0, shims)
    try:
        torch.manual_seed(0)
        eager = demo.WanLikeCrossAttention(3 * 128, 3).cuda()
        fused = demo.WanLikeCrossAttention(3 * 128, 3, fused_prep=True).cuda()
        fused.load_state_dict(eager.state_dict())
        x = torch.randn(2, 700, 3 * 128, device="cuda")
        ctx = torch.randn(2, 512, 3 * 128, device="cuda")
        lens = [77, 512]
        with torch.no_grad():
            y_fused, y_eager, y_ref = fused(x, ctx, lens), eager(x, ctx, lens), eager.reference(x, ctx, lens)
        scale = y_ref.abs().max().item()
        assert (y_fused - y_ref).abs().max().item() <= 2e-2 * scale
        assert (y_fused - y_eager).abs().max().item() <= 2.0 ** -7 * scale
    finally:
        sys.path.remove(shims)
        for n in [m for m in sys.modules if m == "flash_attn" or m.startswith("flash_attn.") or m == "flash_attn_interface"]:
            del sys.modules[n]
