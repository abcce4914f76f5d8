"""GPU: the prologue passes with a row map (la_qk_prep_rows, la_qk_prep_fp8_rows, la_qk_prep_smooth_rows) and `TokenOrder`.

The rule of every case but two is bit equality: a row of the mapped call is the row of the unmapped call it was made from, because
everything behind the load is the unmapped pass' own arithmetic in its own order. The two exceptions carry their derivation: the column
mean of the smooth form (the same S fp32 terms per column, added in another order) and the end-to-end attention (the reference's own
tolerance rule, tests/helpers.py). No case feeds an out-of-range table to the GPU: the clamp is a definition, `from_rows` the guard.

Shapes: (3,4,5) x 3 heads of 64 - base; (1,3,3) x 40 heads of 128 - H D = 5120, the top of the wave-per-token form, 9 rows leave spare
waves in the last round of 4; (1,3,3) x 64 heads of 128 - the workgroup-per-token form; (3,4,5) x 3 heads of 96 with norm "head" / None -
the head kernel (12 of 16 lanes of a head's group live)."""
import os
import re
import subprocess
import sys

import pytest
import torch

from helpers import ref_tolerance

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#        grid       H   D    norm
SHAPES = [((3, 4, 5), 3, 64, "token"), ((1, 3, 3), 40, 128, "token"), ((1, 3, 3), 64, 128, "token"), ((3, 4, 5), 3, 96, "head"),
          ((3, 4, 5), 3, 96, None)]
IDS = ["base", "wave_top", "workgroup", "head_norm", "no_norm"]
B = 2


def make_x(S, H, D, dtype=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, H, D, generator=g) * (0.25 + 3.75 * torch.rand(1, 1, H, 1, generator=g))
    w = 0.5 + torch.rand(H * D, generator=g)
    return x.to(dtype).cuda(), w.cuda()


def weight_for(w, norm, D):
    return w if norm == "token" else (w[:D].contiguous() if norm == "head" else None)


def make_src(S, shared, seed=0):
    """A seeded random permutation of the S rows: one for both batches ([S]) or one per batch ([B, S]), int32 on the device."""
    g = torch.Generator().manual_seed(1000 + seed)
    if shared:
        return torch.randperm(S, generator=g).int().cuda()
    return torch.stack([torch.randperm(S, generator=g) for _ in range(B)]).int().cuda()


def take(t, src, dim=1):
    """t with its dimension `dim` indexed by src ([S]: every batch alike; [B, S]: batch b by src[b])."""
    if src.dim() == 1:
        return t.index_select(dim, src.long())
    return torch.stack([t[b].index_select(dim - 1, src[b].long()) for b in range(t.shape[0])])


def tables_for(grid, D, parts=None):
    import liteattention_amd as L
    return L.rope_tables(grid, D, parts=parts, device="cuda")


def bits(t):
    return t.view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t


@pytest.mark.parametrize("shared", [True, False], ids=["shared_map", "per_batch_maps"])
@pytest.mark.parametrize("grid,H,D,norm", SHAPES, ids=IDS)
def test_gather_positions_and_identity(grid, H, D, norm, shared):
    """rows=src is the gathered unmapped result; positions=src on the gathered input is the same result; rows=arange is the unmapped call."""
    import liteattention_amd as L
    S = grid[0] * grid[1] * grid[2]
    x, w = make_x(S, H, D, seed=S + H)
    w, tables, src = weight_for(w, norm, D), tables_for(grid, D), make_src(S, shared, seed=H)
    plain = L.qk_prep(x, w, 1e-6, tables, norm=norm)
    want = take(plain, src)
    assert not torch.equal(want, plain)
    got = L.qk_prep(x, w, 1e-6, tables, norm=norm, rows=src)
    assert got.shape == x.shape and torch.equal(got, want)
    assert torch.equal(L.qk_prep(take(x, src).contiguous(), w, 1e-6, tables, norm=norm, positions=src), want)
    ident = torch.arange(S, dtype=torch.int32, device="cuda")
    ident = ident if shared else ident.expand(B, S).contiguous()
    assert torch.equal(L.qk_prep(x, w, 1e-6, tables, norm=norm, rows=ident), plain)
    assert torch.equal(L.qk_prep(x, w, 1e-6, tables, norm=norm, positions=ident), plain)


@pytest.mark.parametrize("in_dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16])
def test_gather_over_the_dtypes(in_dtype, out_dtype):
    import liteattention_amd as L
    x, w = make_x(60, 3, 64, in_dtype, seed=5)
    tables, src = tables_for((3, 4, 5), 64), make_src(60, False, seed=5)
    want = take(L.qk_prep(x, w, 1e-6, tables, out_dtype=out_dtype), src)
    got = L.qk_prep(x, w, 1e-6, tables, out_dtype=out_dtype, rows=src)
    assert got.dtype == out_dtype and torch.equal(got, want)


@pytest.mark.parametrize("rotate", ["wan", "partial", "none"])
@pytest.mark.parametrize("grid,H,D,norm", [SHAPES[0], SHAPES[3]], ids=["token_kernel", "head_kernel"])
def test_gather_over_the_rotations_with_a_pos_offset(grid, H, D, norm, rotate):
    """The tables of a (5, 4, 5) grid, the 60 rows at positions 20 ... 79: position = pos_offset + source row."""
    import liteattention_amd as L
    S, pos_offset = 60, 20
    x, w = make_x(S, H, D, seed=77)
    w, src = weight_for(w, norm, D), make_src(S, False, seed=77)
    tables = {"wan": lambda: tables_for((5, 4, 5), D), "partial": lambda: tables_for((5, 4, 5), D, parts=(16, 8, 8)), "none": lambda: None}[rotate]()
    plain = L.qk_prep(x, w, 1e-6, tables, norm=norm, pos_offset=pos_offset)
    if rotate != "none":
        assert not torch.equal(plain, L.qk_prep(x, w, 1e-6, tables, norm=norm))
    want = take(plain, src)
    assert torch.equal(L.qk_prep(x, w, 1e-6, tables, norm=norm, pos_offset=pos_offset, rows=src), want)
    assert torch.equal(L.qk_prep(take(x, src).contiguous(), w, 1e-6, tables, norm=norm, pos_offset=pos_offset, positions=src), want)


def test_rows_with_positions_of_their_own_and_a_shorter_result():
    """rows and positions together: the positions win over the source row; a table shorter than x selects (a pruned sequence)."""
    import liteattention_amd as L
    x, w = make_x(60, 3, 64, seed=8)
    tables = tables_for((3, 4, 5), 64)
    src, pos = make_src(60, True, seed=1), make_src(60, True, seed=2)
    want = L.qk_prep(take(x, src).contiguous(), w, 1e-6, tables, positions=pos)
    assert torch.equal(L.qk_prep(x, w, 1e-6, tables, rows=src, positions=pos), want)
    keep = src[:23].contiguous()
    got = L.qk_prep(x, w, 1e-6, tables, rows=keep)
    assert got.shape == (B, 23, 3, 64) and torch.equal(got, L.qk_prep(x, w, 1e-6, tables)[:, keep.long()])


@pytest.mark.parametrize("shared", [True, False], ids=["shared_map", "per_batch_maps"])
@pytest.mark.parametrize("grid,H,D,norm", SHAPES, ids=IDS)
def test_fp8_bytes_and_amax(grid, H, D, norm, shared):
    import liteattention_amd as L
    S = grid[0] * grid[1] * grid[2]
    x, w = make_x(S, H, D, seed=3 * S + H)
    w, tables, src = weight_for(w, norm, D), tables_for(grid, D), make_src(S, shared, seed=H + 1)
    amax = L.qk_prep_amax(x, w, 1e-6, tables, norm=norm)
    assert amax.min().item() > 0
    descale = L.descale_from_amax(amax.clone())
    a0 = torch.zeros_like(amax)
    plain = L.qk_prep_fp8(x, w, 1e-6, tables, norm=norm, descale=descale, amax_out=a0)
    assert torch.equal(a0, amax)
    for xin, kw in ((x, dict(rows=src)), (take(x, src).contiguous(), dict(positions=src))):
        assert torch.equal(L.qk_prep_amax(xin, w, 1e-6, tables, norm=norm, **kw), amax)
        a1 = torch.zeros_like(amax)
        got = L.qk_prep_fp8(xin, w, 1e-6, tables, norm=norm, descale=descale, amax_out=a1, **kw)
        assert torch.equal(bits(got), take(bits(plain), src)) and torch.equal(a1, amax)


@pytest.mark.parametrize("shared", [True, False], ids=["shared_map", "per_batch_maps"])
@pytest.mark.parametrize("grid,H,D,norm", SHAPES, ids=IDS)
def test_smooth_bytes_dots_and_column_mean(grid, H, D, norm, shared):
    """Given shift and descale. Bytes and row dots: bitwise. Column mean: the parts of the mapped call add the same S fp32 terms per
    column as those of the unmapped call, in another order; a sum of S fp32 terms in any order is within S 2^-24 sum|y| (first order) of
    the exact sum, so two orders differ by at most 2 S 2^-24 sum|y|, and the means (one division by S each, monotone) by
    2 S 2^-24 mean|y| per column - |y| the fp32 value the prologue makes before its cast, taken from the fp64 reference."""
    import liteattention_amd as L
    S = grid[0] * grid[1] * grid[2]
    x, w = make_x(S, H, D, seed=7 * S + H)
    w, tables, src = weight_for(w, norm, D), tables_for(grid, D), make_src(S, shared, seed=H + 2)
    g = torch.Generator().manual_seed(H)
    shift = (0.3 * torch.randn(B, H, D, generator=g)).cuda()
    vec = torch.randn(B, H, D, generator=g).cuda()
    descale = (0.01 + 0.02 * torch.rand(B, H, generator=g)).cuda()
    parts = L.qk_prep_smooth_parts(S, H, D)[0]

    def run(xin, **kw):
        part = torch.empty(parts, B, H, D, device="cuda")
        dots = torch.empty(B, H, S, device="cuda")
        am = torch.zeros(B, H, device="cuda")
        out = L.qk_prep_smooth(xin, w, 1e-6, tables, norm=norm, shift=shift, descale=descale, amax_out=am, colsum_part=part, dot_vec=vec,
                               dot_out=dots, **kw)
        return bits(out), dots, am, L.colsum_finish(part, S)

    o0, d0, a0, m0 = run(x)
    y_abs_mean = L.qk_prep_reference(x, w, 1e-6, tables, norm=norm).abs().mean(dim=1)            # (B, H, D) fp64
    bound = 2 * S * 2.0 ** -24 * y_abs_mean
    for xin, kw in ((x, dict(rows=src)), (take(x, src).contiguous(), dict(positions=src))):
        o1, d1, a1, m1 = run(xin, **kw)
        assert torch.equal(o1, take(o0, src))
        assert torch.equal(d1, take(d0, src, dim=2))
        assert torch.equal(a1, a0)
        err = (m1.double() - m0.double()).abs()
        print(f"smooth {list(kw)[0]}= {grid} H{H} D{D} norm={norm}: column mean err / bound {(err / bound).max().item():.3f}")
        assert (err <= bound).all()
        assert torch.equal(L.qk_prep_colmean(xin, w, 1e-6, tables, norm=norm, **kw), m1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_round_trip_of_gather_restore_and_restore_lse(dtype):
    import liteattention_amd as L
    order = L.brick_order((3, 4, 5), ((1, 2, 2),), device="cuda")
    x, _ = make_x(60, 3, 64, dtype, seed=11)
    g = order.gather(x)
    assert g.dtype == dtype and torch.equal(g, x[:, order.src_rows.long()]) and not torch.equal(g, x)
    assert torch.equal(order.restore(g), x)
    out = torch.empty_like(x)
    assert order.restore(g, out=out).data_ptr() == out.data_ptr() and torch.equal(out, x)
    x32 = x.float() * 1.001
    assert torch.equal(order.gather(x32), x32[:, order.src_rows.long()].bfloat16())
    lse = torch.randn(B, 3, 60, device="cuda")
    assert torch.equal(order.restore_lse(lse[..., order.src_rows.long()]), lse)
    custom = L.TokenOrder.from_rows(make_src(60, True, seed=4), 60)
    assert torch.equal(custom.restore(custom.gather(x)), x)
    with pytest.raises(ValueError):
        order.gather(x, out=x)
    with pytest.raises(ValueError):
        order.gather(x[:, :59])


def test_strided_out_keeps_its_untouched_neighbours():
    """x = a slice of a fused (B, S, 3, H, D) projection, out = a slice of a poisoned buffer: every byte outside the addressed elements
    is unchanged (the method of tests/test_gpu_qk_prep.py::test_strided_views_and_untouched_neighbours)."""
    import liteattention_amd as L
    S, H, D = 60, 3, 128
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(B, S, 3, H, D, generator=g).bfloat16().cuda()
    w = (0.5 + torch.rand(H * D, generator=g)).cuda()
    tables, src = tables_for((3, 4, 5), D), make_src(S, False, seed=6)
    for which in (0, 1):
        x = qkv[:, :, which]
        want = take(L.qk_prep(x.contiguous(), w, 1e-6, tables), src)
        big = torch.empty((B + 1, S + 3, H + 2, D + 8), dtype=torch.bfloat16, device="cuda")
        big.view(torch.int16).fill_(0x7fa5)                                            # a NaN pattern no kernel writes
        before = big.clone()
        out = big[1:, 2:S + 2, 1:H + 1, :D]
        got = L.qk_prep(x, w, 1e-6, tables, out=out, rows=src)
        assert got.data_ptr() == out.data_ptr() and torch.equal(out, want)
        mask = torch.ones_like(big, dtype=torch.bool)
        mask[1:, 2:S + 2, 1:H + 1, :D] = False
        assert torch.equal(big.view(torch.int16)[mask], before.view(torch.int16)[mask])


def test_a_mapped_q_and_k_pair_captures_into_a_hip_graph_and_replays():
    """The single-branch capture of tests/test_gpu_qk_prep.py with rows= on q and positions= on k: tables and maps built before the
    capture, warm-up on a side stream; three replays on changing inputs equal the eager pair bitwise."""
    import liteattention_amd as L
    tables = tables_for((3, 4, 5), 128)
    order = L.brick_order((3, 4, 5), ((1, 2, 2),), device="cuda")
    q, w_q = make_x(60, 5, 128, seed=100)
    k, w_k = make_x(60, 5, 128, seed=101)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        L.qk_prep(q, w_q, 1e-6, tables, rows=order)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gq = L.qk_prep(q, w_q, 1e-6, tables, rows=order)
        gk = L.qk_prep(k, w_k, 1e-6, tables, positions=order)
    for rep in range(3):
        q.copy_(make_x(60, 5, 128, seed=200 + rep)[0])
        k.copy_(make_x(60, 5, 128, seed=300 + rep)[0])
        g.replay()
        eq, ek = L.qk_prep(q, w_q, 1e-6, tables, rows=order), L.qk_prep(k, w_k, 1e-6, tables, positions=order)
        torch.cuda.synchronize()
        assert torch.equal(gq, eq) and torch.equal(gk, ek), rep
        assert torch.equal(gq, L.qk_prep(q, w_q, 1e-6, tables)[:, order.src_rows.long()])


def test_e4m3_scales_and_smoothed_qk_take_the_map():
    import liteattention_amd as L
    x, w = make_x(60, 4, 128, seed=31)
    tables = tables_for((3, 4, 5), 128)
    order = L.brick_order((3, 4, 5), ((1, 2, 2),), device="cuda")
    src = order.src_rows.long()
    x8, d = L.E4m3Scales()(x, w, 1e-6, tables)
    x8, d = bits(x8).clone(), d.clone()
    m8, md = L.E4m3Scales()(x, w, 1e-6, tables, rows=order)
    assert torch.equal(md, d) and torch.equal(bits(m8), x8[:, src])
    with pytest.raises(ValueError, match="gather"):
        L.E4m3Scales(tiles=True)(x, norm=None, rows=order)
    q8, k8, dq, dk, ls = [t.clone() for t in L.SmoothedQK().pair(x, x, w, w, 1e-6, tables)]
    g = take(x, order.src_rows).contiguous()
    mq, mk, mdq, mdk, mls = L.SmoothedQK().pair(g, g, w, w, 1e-6, tables, positions=order)
    # q is not shifted: its descale and bytes are order-free. The shift of k is the column mean, which the two orders round differently
    # (to 2 S 2^-24 mean|y|, far below a code step): a key may land one e4m3 code away - at most 32 descale, the spacing of the top
    # binade - and the descale itself may move by an ulp of fp32 (448 x 2^-23 descale, far below a step): two steps bound the sum
    assert torch.equal(mdq, dq)
    assert torch.equal(bits(mq), bits(q8)[:, src])
    step = dk.max().item() * 32
    assert ((mk.float() * mdk[:, None, :, None]) - (k8.float() * dk[:, None, :, None])[:, src]).abs().max().item() <= 2 * step


def test_attention_in_brick_order_end_to_end():
    """Grid (2,16,32), S = 1024: q and k from qk_prep(rows=order), v from order.gather; order.restore(out) and the raster-order output each
    against the fp32 torch reference under the reference's tolerance rule, the two LSEs to the 1e-3 of the dense parity tests."""
    import liteattention_amd as L
    grid, H, D = (2, 16, 32), 2, 128
    S = 1024
    g = torch.Generator().manual_seed(5)
    xq, xk = (torch.randn(1, S, H, D, generator=g).bfloat16().cuda() for _ in range(2))
    v = torch.randn(1, S, H, D, generator=g).bfloat16().cuda()
    w = (0.5 + torch.rand(H * D, generator=g)).cuda()
    tables = tables_for(grid, D)
    order = L.brick_order(grid, device="cuda")
    q, k = L.qk_prep(xq, w, 1e-6, tables), L.qk_prep(xk, w, 1e-6, tables)
    qo, ko, vo = L.qk_prep(xq, w, 1e-6, tables, rows=order), L.qk_prep(xk, w, 1e-6, tables, rows=order), order.gather(v)
    assert torch.equal(qo, q[:, order.src_rows.long()])
    out_r, lse_r = L.LiteAttention(enable_skipping=False)(q, k, v, return_softmax_lse=True)
    out_o, lse_o = L.LiteAttention(enable_skipping=False)(qo, ko, vo, return_softmax_lse=True)
    out_o, lse_o = order.restore(out_o), order.restore_lse(lse_o)
    scale = D ** -0.5
    s32 = torch.einsum("bqhd,bkhd->bhqk", q.float(), k.float()) * scale
    ref = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s32, -1), v.float())
    lse_ref = torch.logsumexp(s32, -1)
    pt = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k).float() * scale, -1).bfloat16(), v)
    tol = ref_tolerance(ref, (pt.float() - ref).abs().max().item())
    for name, o, l in (("raster", out_r, lse_r), ("bricks", out_o, lse_o)):
        err, lerr = (o.float() - ref).abs().max().item(), (l - lse_ref).abs().max().item()
        print(f"{name}: max |O - ref| {err:.3e} (tolerance {tol:.3e}), max |LSE - ref| {lerr:.3e}")
        assert err <= tol and lerr <= 1e-3


def test_demo_with_brick_order():
    """--brick-order on the demo's small configuration: exit 0, and the printed difference to the raster run inside the printed
    tolerance, which is the reference's rule (2 x the error of the bf16 torch attention + the fp32 roundoff term) on the demo's own q, k, v."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "wan_self_attention_demo.py"), "--brick-order", "1,8,8", "1,4,4",
                        "--frames", "2", "--steps", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"max abs difference to the raster run ([0-9.e+-]+) \(tolerance ([0-9.e+-]+)\)", r.stdout)
    assert m, r.stdout
    diff, tol = float(m.group(1)), float(m.group(2))
    assert 0 <= diff <= tol < 0.1, r.stdout
