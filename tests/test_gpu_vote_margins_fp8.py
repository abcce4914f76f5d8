"""GPU: la_vote_margins_fp8 against the fp64 reference of the map - on a grid of e4m3 values where every fp32 score is exact (every
head dim, dense and listed walks), on plain e4m3 operands, against the list the e4m3 forward writes, and bit for bit between launches."""
import math

import pytest
import torch

from liteattention_amd import LiteAttention, _cabi, skip_list_stats_heads, vote_margins, vote_margins_reference
from test_gpu_vote_margins import drifting_qkv, fragmented_rows

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn
SENTINEL = 12345.0


def packed_qk(B, Sq, Sk, H, Hk, D, seed=0, exact=True):
    """e4m3 q and k as strided views of one packed buffer, and descales in [0.5, 2) per (batch, K/V head) as strided views of another.
    ``exact``: multiples of 1/4 below 4 - e4m3 values whose products are multiples of 2^-4 and whose sums over 256 terms stay below
    2^12, so every accumulation order and rounding mode gives the same fp32 score."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, max(Sq, Sk), H + Hk, D, generator=g)
    buf = ((x * 4).round().clamp(-15, 15) / 4 if exact else x).to(F8).cuda()
    ds = (0.5 + 1.5 * torch.rand(B, Hk, 2, generator=g)).cuda()
    return buf[:, :Sq, :H], buf[:, :Sk, H:], ds[..., 0], ds[..., 1]


def check_map(q, k, qd, kd, read_list=None, accumulation=0.0):
    """NaN exactly at the first walked tile and at unwalked tiles; elsewhere |m - ref| <= accumulation c 2 D 2^-23 A + 2^-21 |ref| with
    c = softmax_scale log2 e qd kd and A = max_ij sum_d |q_id| |k_jd| per (batch, head), in fp64. The second term: three fp32 roundings
    in c and one in the product (the subtraction of two fp32 maxima is exact or rounded once, inside the same 2^-24 steps); the first
    is zero on the exact grid and bounds round-to-nearest fp32 sums of D exact products, doubled for the two maxima, elsewhere."""
    D = q.shape[3]
    bm, bn = _cabi.get_tile_sizes(D, 1)
    ref = vote_margins_reference(q, k, read_list=read_list, block_m=bm, block_n=bn, q_descale=qd, k_descale=kd)
    out = torch.full(ref.shape, SENTINEL, dtype=torch.float32, device=q.device)
    got = vote_margins(q, k, read_list=read_list, out=out, q_descale=qd, k_descale=kd)
    assert got is out and torch.equal(torch.isnan(got), torch.isnan(ref))
    r = q.shape[2] // k.shape[2]
    A = torch.einsum("bqhd,bkhd->bhqk", q.double().abs(), k.double().abs().repeat_interleave(r, dim=2)).amax(dim=(2, 3), keepdim=True)
    c = D ** -0.5 * math.log2(math.e) * (qd.double() * kd.double()).repeat_interleave(r, dim=1)[:, :, None, None]
    first = c * 2 * D * 2.0 ** -23 * A
    walked = ~torch.isnan(ref)
    err = (got.double() - ref).abs()
    ratio = float(((err - 2.0 ** -21 * ref.abs()).clamp(min=0) / first)[walked].max())
    print(f"walked {int(walked.sum())} max err {float(err[walked].max()):.3e} largest (err - 2^-21 |ref|) / accumulation term {ratio:.3f}")
    assert bool((err <= accumulation * first + 2.0 ** -21 * ref.abs())[walked].all())
    return ref


@pytest.mark.parametrize("D", [64, 96, 128, 192, 256])
def test_map_against_the_fp64_reference_on_exact_scores(D):
    bm, _ = _cabi.get_tile_sizes(D, 1)
    check_map(*packed_qk(2, 2 * bm + 44, 5 * 64 + 17, 4, 2, D))               # ragged last q-tile, six key tiles, the last one masked


@pytest.mark.parametrize("list_dtype", [torch.int32, torch.int16], ids=["int32", "int16"])
@pytest.mark.parametrize("D", [128, 192])
def test_map_under_a_read_list(D, list_dtype):
    bm, _ = _cabi.get_tile_sizes(D, 1)
    read_list = fragmented_rows(4, list_dtype).view(1, 4, 1, 7).expand(3, 4, 3, 7).contiguous().cuda()      # B_alloc = 3 > B
    ref = check_map(*packed_qk(2, 2 * bm + 44, 5 * 64 + 17, 4, 2, D, seed=1), read_list)
    assert (~torch.isnan(ref[0, :, 0])).sum(dim=-1).tolist() == [2, 3, 3, 4]


def test_map_on_plain_e4m3_operands():
    check_map(*packed_qk(2, 2 * 256 + 44, 5 * 64 + 17, 4, 2, 128, seed=2, exact=False), accumulation=1.0)


def test_map_predicts_the_list_the_fp8_forward_writes():
    """test_gpu_vote_margins.test_map_predicts_the_list_the_forward_writes on the e4m3 pipeline: the drifting operands quantised per
    (batch, K/V head) with descale = amax / 448; the threshold lies in the widest gap of the central half of the sorted reference
    margins, and the gap exceeds twice the bound of the plain-operand case: no tile is borderline."""
    x = [t.cpu().float() for t in drifting_qkv(0)]
    ds = [t.abs().amax(dim=(1, 3)) / 448.0 for t in x]
    q, k, v = [(t / d[:, None, :, None]).to(F8).cuda() for t, d in zip(x, ds)]
    qd, kd, vd = [d.cuda() for d in ds]
    ref = vote_margins_reference(q, k, block_m=256, block_n=64, q_descale=qd, k_descale=kd)
    srt = ref[torch.isfinite(ref)].sort().values
    mid = srt[len(srt) // 4: 3 * len(srt) // 4 + 1]
    gaps = mid[1:] - mid[:-1]
    i = int(gaps.argmax())
    thr = float(0.5 * (mid[i] + mid[i + 1]))
    A = torch.einsum("bqhd,bkhd->bhqk", q.double().abs(), k.double().abs()).amax(dim=(2, 3))
    c = 128 ** -0.5 * math.log2(math.e) * qd.double() * kd.double()
    bound = float((c * 2 * 128 * 2.0 ** -23 * A).max()) + 2.0 ** -21 * float(srt.abs().max())
    print(f"thr {thr:.4f} gap {float(gaps[i]):.3e} bound {bound:.3e}")
    assert thr < 0 and float(gaps[i]) > 2 * bound
    margins = vote_margins(q, k, q_descale=qd, k_descale=kd)
    att = LiteAttention(threshold=thr, max_batch_size=2)
    att(q, k, v, q_descale=qd, k_descale=kd, v_descale=vd)
    listed = skip_list_stats_heads(att.current_read_list(), 2)
    keep = margins > thr
    keep[..., -1] = True                                                      # the first tile of the dense walk
    assert torch.equal(listed, keep.sum(dim=(2, 3)) + (keep[..., 1:] & ~keep[..., :-1]).sum(dim=(2, 3)))
    assert 0.2 < float((margins > thr).sum()) / float(torch.isfinite(margins).sum()) < 0.8


def test_two_launches_give_identical_bits():
    q, k, qd, kd = packed_qk(2, 2 * 256 + 44, 5 * 64 + 17, 4, 2, 128, seed=3, exact=False)
    read_list = fragmented_rows(4, torch.int32).view(1, 4, 1, 7).expand(2, 4, 3, 7).contiguous().cuda()
    for rl in (None, read_list):
        a, b = (vote_margins(q, k, read_list=rl, q_descale=qd, k_descale=kd) for _ in range(2))
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
