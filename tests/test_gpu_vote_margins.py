"""GPU: la_vote_margins against the fp64 reference of the map (dense and listed walks, every head dim, both dtypes and q-tile
geometries), against the list the forward writes, through calibrate_skip_schedule, and bit for bit between launches."""
import math

import pytest
import torch

from liteattention_amd import (LiteAttention, _cabi, skip_list_stats_heads, vote_margins,
                               vote_margins_reference)
from liteattention_amd.calibration import calibrate_skip_schedule

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0


def packed_qk(B, Sq, Sk, H, Hk, D, dtype, seed=0):
    """q and k as strided views of one packed buffer."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(B, max(Sq, Sk), H + Hk, D, generator=g).to(dtype).cuda()
    return buf[:, :Sq, :H], buf[:, :Sk, H:]


def check_map(q, k, flags, read_list=None):
    """NaN exactly at the first walked tile and at unwalked tiles; elsewhere |m - ref| <= c 2 D 2^-23 A + 2^-22 |ref|, c = softmax_scale
    log2 e, A = max_ij sum_d |q_id| |k_jd| in fp64. Products of 16-bit operands are exact in fp32, so the first term bounds any fp32
    accumulation order of D terms, doubled for the two maxima a margin subtracts; the second covers the fp32 subtraction, product and c."""
    D = q.shape[3]
    bm, bn = _cabi.get_tile_sizes(D, 2, flags)
    ref = vote_margins_reference(q, k, read_list=read_list, block_m=bm, block_n=bn)
    out = torch.full(ref.shape, SENTINEL, dtype=torch.float32, device=q.device)
    got = vote_margins(q, k, read_list=read_list, flags=flags, out=out)
    assert got is out and torch.equal(torch.isnan(got), torch.isnan(ref))
    A = torch.einsum("bqhd,bkhd->bhqk", q.double().abs(), k.double().abs().repeat_interleave(q.shape[2] // k.shape[2], dim=2)).max()
    bound = D ** -0.5 * math.log2(math.e) * 2 * D * 2.0 ** -23 * float(A) + 2.0 ** -22 * ref.abs()
    walked = ~torch.isnan(ref)
    err = (got.double() - ref).abs()
    print(f"walked {int(walked.sum())} max err {float(err[walked].max()):.3e} smallest bound {float(bound[walked].min()):.3e}")
    assert bool((err <= bound)[walked].all())
    return ref


# every head dim in the default geometry, and under the half vote where it changes the q-tile (d <= 128)
GEOMETRIES = [(D, 0) for D in (64, 96, 128, 192, 256)] + [(D, _cabi.LA_FLAG_HALF_VOTE) for D in (64, 96, 128)]


@pytest.mark.parametrize("D,flags", GEOMETRIES, ids=[f"d{D}-{'half' if f else 'default'}" for D, f in GEOMETRIES])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_map_against_the_fp64_reference(dtype, D, flags):
    bm, _ = _cabi.get_tile_sizes(D, 2, flags)
    q, k = packed_qk(2, 2 * bm + 44, 5 * 64 + 17, 4, 2, D, dtype)             # ragged last q-tile, six key tiles, the last one masked
    check_map(q, k, flags)


def fragmented_rows(H, list_dtype):
    """Three ranges per row, the first walked tile is not Kt - 1 = 5, rows differ per head."""
    rows = [[6, 4, 4, 2, 2, 0, 0], [6, 4, 3, 1, 1, 0, 0], [6, 3, 3, 2, 1, 0, 0], [6, 4, 2, 1, 1, 0, 0]]
    return torch.tensor(rows[:H], dtype=list_dtype)


@pytest.mark.parametrize("list_dtype", [torch.int32, torch.int16], ids=["int32", "int16"])
@pytest.mark.parametrize("D,flags", [(128, 0), (64, _cabi.LA_FLAG_HALF_VOTE), (192, 0)], ids=["d128", "d64-half", "d192"])
def test_map_under_a_read_list(D, flags, list_dtype):
    bm, _ = _cabi.get_tile_sizes(D, 2, flags)
    q, k = packed_qk(2, 2 * bm + 44, 5 * 64 + 17, 4, 2, D, torch.bfloat16, seed=1)
    read_list = fragmented_rows(4, list_dtype).view(1, 4, 1, 7).expand(3, 4, 3, 7).contiguous().cuda()      # B_alloc = 3 > B
    ref = check_map(q, k, flags, read_list)
    assert (~torch.isnan(ref[0, :, 0])).sum(dim=-1).tolist() == [2, 3, 3, 4]


def test_map_under_a_list_of_more_ranges_than_a_wave_has_lanes():
    Kt = 132                                                                  # 66 ranges of one tile: the expansion takes two passes
    q, k = packed_qk(1, 256, Kt * 64, 2, 1, 64, torch.bfloat16, seed=2)
    row = [Kt] + [t for n in range(Kt - 2, -1, -2) for t in (n, n)]
    read_list = torch.tensor(row, dtype=torch.int32).view(1, 1, 1, Kt + 1).expand(1, 2, 1, Kt + 1).contiguous().cuda()
    ref = check_map(q, k, 0, read_list)
    assert int((~torch.isnan(ref)).sum()) == 2 * 65


def drifting_qkv(t, B=2, S=512, Sk=1280, H=4, D=128):
    """Scores with a common component that falls along the descending key walk, so that the margins are negative and spread over several
    log2 units (a tile late in the walk seldom holds a row's maximum); q and k drift slowly with the step t."""
    g = torch.Generator().manual_seed(7)
    u = torch.nn.functional.normalize(torch.randn(1, 1, H, D, generator=g), dim=-1) * 6.0
    a = 1.0 + 0.2 * torch.randn(B, S, H, 1, generator=g)
    b = 1.0 + 2.0 * torch.arange(Sk).view(1, Sk, 1, 1) / Sk + 0.3 * torch.randn(B, Sk, H, 1, generator=g)
    nq, nk, dq, dk = (torch.randn(B, n, H, D, generator=g) for n in (S, Sk, S, Sk))
    q = a * u + 0.3 * nq + 0.05 * t * dq
    k = b * u + 0.3 * nk + 0.05 * t * dk
    return q.to(torch.bfloat16).cuda(), k.to(torch.bfloat16).cuda(), torch.randn(B, Sk, H, D, generator=g).to(torch.bfloat16).cuda()


def test_map_predicts_the_list_the_forward_writes():
    """Per (batch, head), over the dense walk: listed tiles of the written list = Qt (every row's first tile) + #{finite margins > thr}
    + #{tiles with margin <= thr right behind a kept tile} - the writer (and the oracle's: checked on the CPU) closes a range with the
    first DROPPED tile as its inclusive end, so that tile is named too. The threshold lies in the widest gap of the central half of
    the sorted margins, and the gap exceeds twice the bound of the map: no tile is borderline."""
    q, k, v = drifting_qkv(0)
    ref = vote_margins_reference(q, k, block_m=256, block_n=64)
    srt = ref[torch.isfinite(ref)].sort().values
    mid = srt[len(srt) // 4: 3 * len(srt) // 4 + 1]
    gaps = mid[1:] - mid[:-1]
    i = int(gaps.argmax())
    thr = float(0.5 * (mid[i] + mid[i + 1]))
    A = float(torch.einsum("bqhd,bkhd->bhqk", q.double().abs(), k.double().abs()).max())
    bound = 128 ** -0.5 * math.log2(math.e) * 2 * 128 * 2.0 ** -23 * A + 2.0 ** -22 * float(srt.abs().max())
    print(f"thr {thr:.4f} gap {float(gaps[i]):.3e} bound {bound:.3e}")
    assert thr < 0 and float(gaps[i]) > 2 * bound
    margins = vote_margins(q, k, flags=0)
    att = LiteAttention(threshold=thr, max_batch_size=2)
    att(q, k, v)
    listed = skip_list_stats_heads(att.current_read_list(), 2)
    keep = margins > thr
    keep[..., -1] = True                                                      # the first tile of the dense walk
    assert torch.equal(listed, keep.sum(dim=(2, 3)) + (keep[..., 1:] & ~keep[..., :-1]).sum(dim=(2, 3)))
    assert 0.2 < float((margins > thr).sum()) / float(torch.isfinite(margins).sum()) < 0.8


@pytest.mark.parametrize("per_head", [False, True], ids=["global", "per-head"])
def test_calibrate_skip_schedule_hits_its_targets(per_head):
    """Replayed on a fresh object, every step's written list keeps 1 - target of the tiles the step walked: to within one tile of the
    total (one threshold), or of every head's tiles over the batch (one threshold per head)."""
    targets = [0.3, 0.25, 0.2]
    thresholds, trace = calibrate_skip_schedule(drifting_qkv, 3, targets, per_head=per_head, max_batch_size=2)
    att = LiteAttention(threshold=-1.0, max_batch_size=2)
    if per_head:
        assert tuple(thresholds.shape) == (3, 4) and bool((thresholds < -1e-3).all())
        att.set_head_thresholds(thresholds)
    else:
        assert len(thresholds) == 3 and all(t < -1e-3 for t in thresholds)
        att.set_threshold_schedule(thresholds)
    walked = torch.full((4,), 2 * 2 * 20, dtype=torch.int64, device="cuda")                   # per head: B * Qt * Kt, every tile listed
    for t, target in enumerate(targets):
        att(*drifting_qkv(t))
        kept = skip_list_stats_heads(att.current_read_list(), 2).sum(dim=0)
        off = (kept - (1 - target) * walked).abs() if per_head else (kept.sum() - (1 - target) * walked.sum()).abs()
        print(f"step {t} walked {walked.tolist()} kept {kept.tolist()}")
        assert float(off.max()) <= 1.0
        assert float(torch.as_tensor(trace[t]["kept"]).sum()) == float(kept.sum())                # the replay is the calibration run
        walked = kept


def test_two_launches_give_identical_bits():
    q, k = packed_qk(2, 2 * 256 + 44, 5 * 64 + 17, 4, 2, 128, torch.bfloat16, seed=3)
    read_list = fragmented_rows(4, torch.int32).view(1, 4, 1, 7).expand(2, 4, 3, 7).contiguous().cuda()
    for rl in (None, read_list):
        a, b = vote_margins(q, k, read_list=rl, flags=0), vote_margins(q, k, read_list=rl, flags=0)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
