"""CPU: the layout helpers of tests/layout_cases.py really build what tests/test_gpu_layout_poison.py relies on - views that equal their
source bit for bit, satisfy the library's stride rule (la_api.hip), and are surrounded by nothing but poison / canary - and the hand-built
read lists of the list launches are well formed and a fixed point of the oracle at thr = -inf."""
import pytest
import torch

import layout_cases as lc
from layout_cases import F8

DTYPES = [torch.bfloat16, torch.float16, F8]


def _src(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def _poisons(dtype):
    return [p for p in lc.POISONS if (dtype, p) in lc.POISON_BITS]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "e4m3"])
@pytest.mark.parametrize("layout,packed", [(l, False) for l in lc.IN_LAYOUTS] + [("wide_rows", True), ("bhsd", True)])   # packed (T, H, D) batches use these two
def test_input_views(layout, dtype, packed):
    lead, trail = 3, 70
    shape = (37, 2, 64) if packed else (2, 13, 2, 64)
    n = 3 if layout == "packed_qkv" else 1
    srcs = [_src(shape, dtype, seed=i) for i in range(n)]
    if layout == "batch0":
        srcs = [srcs[0][:1].expand(shape)]
    for poison in _poisons(dtype):
        buf, views = lc.embed(tuple(srcs) if n == 3 else srcs[0], layout, poison, lead, trail)
        views = views if n == 3 else (views,)
        for s, v in zip(srcs, views):
            assert v.dtype == dtype and tuple(v.shape) == shape
            assert torch.equal(lc.raw(v), lc.raw(s))
            assert lc.strides_ok(v, dtype == F8), v.stride()
            assert not v.is_contiguous() and (layout != "batch0" or v.stride(0) == 0)
        cov = lc.covered(shape, layout, lead, trail, n_views=n)
        assert int(cov.sum()) == n * srcs[0].numel() // (2 if layout == "batch0" else 1) and not bool(cov.all())
        even, odd = lc.poison_bits(dtype, poison)
        assert lc.untouched_outside(buf, cov, even, odd)
        outside = buf.reshape(-1)[~cov.reshape(-1)].float()
        if poison == "nan":
            assert bool(torch.isnan(outside).all())
        elif poison == "inf":
            assert bool(torch.isinf(outside).all()) and bool((outside > 0).any()) and bool((outside < 0).any())
        else:
            big = {torch.bfloat16: 3.3895313892515355e38, torch.float16: 65504.0, F8: 448.0}[dtype]
            assert bool((outside.abs() == big).all()) and bool((outside > 0).any()) and bool((outside < 0).any())
        # the check can fail: one flipped element outside the view is seen
        lc.raw(buf).view(-1)[int((~cov.reshape(-1)).nonzero()[0])] ^= 1
        assert not lc.untouched_outside(buf, cov, even, odd)


def test_layout_geometry():
    """What each layout promises about the neighbours of a row."""
    B, S, H, D, lead, trail = 2, 13, 2, 64, 3, 70
    x = _src((B, S, H, D), torch.bfloat16)
    _, w = lc.embed(x, "wide_rows", "nan", lead, trail)
    assert w.stride() == ((lead + S + trail) * H * 2 * D, H * 2 * D, 2 * D, 1) and w.stride(0) > S * w.stride(1)
    _, b = lc.embed(x, "bhsd", "nan", lead, trail)
    assert b.stride() == (H * (S + trail) * D, D, (S + trail) * D, 1) and b.stride(2) > b.stride(1)
    _, (q, k, v) = lc.embed((x, x, x), "packed_qkv", "nan", lead, trail)
    assert q.stride() == ((S + trail) * 3 * H * D, 3 * H * D, D, 1) and k.data_ptr() - q.data_ptr() == 2 * H * D == v.data_ptr() - k.data_ptr()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("layout", lc.OUT_LAYOUTS)
@pytest.mark.parametrize("packed", [False, True], ids=["bshd", "packed"])
def test_out_views(layout, dtype, packed):
    shape = (37, 4, 64) if packed else (2, 13, 4, 64)
    buf, view = lc.embed_out(shape, dtype, layout, "cpu", trail=5)
    assert tuple(view.shape) == shape and view.dtype == dtype and lc.strides_ok(view, False) and not view.is_contiguous()
    cov = lc.covered(shape, layout, 0, 5)
    assert int(cov.sum()) == view.numel() and not bool(cov.all())
    assert bool((lc.raw(buf) == lc.raw(buf).view(-1)[0]).all()) and bool(torch.isfinite(buf.float()).all())
    view.fill_(1.0)
    assert lc.canary_intact(buf, cov) and int((buf.float() == 1.0).sum()) == view.numel()
    lc.raw(buf).view(-1)[int((~cov.reshape(-1)).nonzero()[-1])] ^= 1
    assert not lc.canary_intact(buf, cov)


def test_poison_rows():
    x = _src((1, lc.LIST_S, 2, 64), F8)
    rows = [lc.tile_rows(t) for t in lc.SKIPPED_TILES]
    y = lc.poison_rows(x, rows, "huge")
    assert rows[0] == slice(128, 192) and lc.tile_rows(9) == slice(576, 600)
    keep = torch.ones(lc.LIST_S, dtype=torch.bool)
    for sl in rows:
        keep[sl] = False
    assert torch.equal(lc.raw(y)[:, keep], lc.raw(x)[:, keep])
    assert bool((y[:, ~keep].float().abs() == 448.0).all()) and y[:, ~keep].float().sum().item() == 0.0


@pytest.mark.parametrize("block_m", [256, 128])
@pytest.mark.parametrize("must_do", [False, True])
def test_read_lists_are_well_formed_and_a_fixed_point_of_the_oracle(block_m, must_do):
    from oracle import oracle as orc
    B, S, H, D = 1, lc.LIST_S, 2, 64
    Qt, Kt = -(-S // block_m), -(-S // 64)
    assert Kt == lc.LIST_KT and Qt in (3, 5)
    rd = lc.list_rows([lc.LIST_RANGES] * Qt, B, H)
    walked = orc.walk_tiles(rd[0, 0, 0].tolist())
    assert walked == [9, 8, 7, 6, 4, 3, 1, 0] and not set(walked) & set(lc.SKIPPED_TILES) and len(lc.LIST_RANGES) // 2 >= 3
    g = torch.Generator().manual_seed(1)
    q, k, v = [torch.randn(B, S, H, D, generator=g).bfloat16() for _ in range(3)]
    md = orc.expand_must_do_ref(lc.MUST_DO_KEYS, 64, Kt + 1) if must_do else None
    wr = torch.full_like(rd, -7)
    o, lse, n = orc.qkskip_fwd(q, k, v, block_m=block_m, block_n=64, read_list=rd, write_list=wr, must_do_list=md, thr=float("-inf"))
    assert n == B * H * Qt * len(walked) and bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse).all())
    L = len(lc.LIST_RANGES)
    assert torch.equal(wr[..., :L + 1], rd[..., :L + 1])
    # the skipped tiles are not read into the oracle's result either
    kp, vp = [lc.poison_rows(t, [lc.tile_rows(x) for x in lc.SKIPPED_TILES], "nan") for t in (k, v)]
    o2, lse2, _ = orc.qkskip_fwd(q, kp, vp, block_m=block_m, block_n=64, read_list=rd, write_list=torch.zeros_like(rd), thr=float("-inf"))
    assert torch.equal(o2, o) and torch.equal(lse2, lse)


def test_half_vote_lists_differ_in_one_tile_only():
    from oracle import oracle as orc
    rd = lc.list_rows([lc.HALF0_RANGES, lc.HALF1_RANGES] * 2, 1, 2)
    h0, h1 = orc.walk_tiles(rd[0, 0, 0].tolist()), orc.walk_tiles(rd[0, 0, 1].tolist())
    assert set(h0) - set(h1) == {lc.HALF_TILE} and not set(h1) - set(h0)
    g = torch.Generator().manual_seed(2)
    q = torch.randn(1, 512, 2, 64, generator=g).bfloat16()
    k, v = [torch.randn(1, lc.LIST_S, 2, 64, generator=g).bfloat16() for _ in range(2)]
    wr = torch.full_like(rd, -7)
    orc.qkskip_fwd(q, k, v, block_m=128, block_n=64, read_list=rd, write_list=wr, thr=float("-inf"))
    for m in range(4):
        n = int(rd[0, 0, m, 0])
        assert torch.equal(wr[:, :, m, :n + 1], rd[:, :, m, :n + 1])
