"""GPU: la_tile_mass against the fp64 reference of the map (dense and listed walks, every head dim, both dtypes and q-tile geometries),
its margins against la_vote_margins bit for bit, and calibrate_mass_schedule against the lists the forward writes."""
import math

import pytest
import torch

from liteattention_amd import (LiteAttention, _cabi, calibrate_mass_schedule, tile_mass, tile_mass_reference, vote_margins)
from liteattention_amd.calibration import _walk_of_row
from test_gpu_vote_margins import GEOMETRIES, drifting_qkv, fragmented_rows, packed_qk

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
EXP_REL = 2.0 ** -23              # v_exp_f32: one ulp
TINY = 2.0 ** -119                # 64 keys of a tile, each probability below 2^-126 flushed to zero, with room


def lse_of(q, k, scale):
    """The fp64 logsumexp of every row over all keys, rounded to fp32: what both sides are given."""
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double().repeat_interleave(q.shape[2] // k.shape[2], dim=2)) * scale
    return torch.logsumexp(s, dim=-1).float(), float(s.abs().max())


def map_eps(q, k, lse, smax, bm):
    """Relative bound of a mass. x = s c - L2 in log2 units, c = softmax_scale log2 e, L2 = lse log2 e: the fp32 accumulation of D exact
    16-bit products is off by at most c D 2^-23 A, A = max_ij sum_d |q_id| |k_jd| (any order); the roundings of c, of L2 and of the FMA by
    2^-22 (max|s c| + max|L2|). p = exp2(x) moves by ln 2 times that, relatively, plus the relative error of v_exp_f32; sums of
    non-negative terms - 64 keys, then up to block_m rows - add (64 + block_m) 2^-24. Nothing here comes from the kernel's output."""
    D = q.shape[3]
    A = float(torch.einsum("bqhd,bkhd->bhqk", q.double().abs(), k.double().abs().repeat_interleave(q.shape[2] // k.shape[2], dim=2)).max())
    c = D ** -0.5 * math.log2(math.e)
    l2 = float(lse[torch.isfinite(lse)].abs().max()) * math.log2(math.e)
    return math.log(2) * (c * D * 2.0 ** -23 * A + 2.0 ** -22 * (smax * math.log2(math.e) + l2)) + EXP_REL + (64 + bm) * 2.0 ** -24


def check_maps(q, k, lse, smax, flags, read_list=None):
    """NaN exactly at unwalked tiles of both maps; elsewhere |got - ref| <= eps ref + tiny (map_eps)."""
    bm, bn = _cabi.get_tile_sizes(q.shape[3], 2, flags)
    ref = tile_mass_reference(q, k, lse, read_list=read_list, block_m=bm, block_n=bn)
    shape = ref.mass_max.shape
    out = type(ref)(*(torch.full(shape, SENTINEL, dtype=torch.float32, device=q.device) for _ in range(2)))
    got = tile_mass(q, k, lse, read_list=read_list, flags=flags, out=out)
    eps = map_eps(q, k, lse, smax, bm)
    for name in ("mass_max", "mass_mean"):
        g, r = getattr(got, name), getattr(ref, name)
        assert g is getattr(out, name) and torch.equal(torch.isnan(g), torch.isnan(r))
        walked = ~torch.isnan(r)
        ratio = ((g.double() - r).abs() / (eps * r + TINY))[walked]
        print(f"{name}: walked {int(walked.sum())} eps {eps:.3e} worst ratio {float(ratio.max()):.3f}")
        assert bool((ratio <= 1.0).all())
    return ref


@pytest.mark.parametrize("D,flags", GEOMETRIES, ids=[f"d{D}-{'half' if f else 'default'}" for D, f in GEOMETRIES])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_maps_against_the_fp64_reference(dtype, D, flags):
    bm, _ = _cabi.get_tile_sizes(D, 2, flags)
    q, k = packed_qk(2, 2 * bm + 44, 5 * 64 + 17, 4, 2, D, dtype)             # ragged last q-tile, six key tiles, the last one masked
    lse, smax = lse_of(q, k, D ** -0.5)
    ref = check_maps(q, k, lse, smax, flags)
    assert torch.allclose(ref.mass_mean.sum(dim=-1), torch.ones_like(ref.mass_mean[..., 0]), rtol=0, atol=1e-5)      # the lse is the rows' own


@pytest.mark.parametrize("list_dtype", [torch.int32, torch.int16], ids=["int32", "int16"])
@pytest.mark.parametrize("D,flags", [(128, 0), (64, _cabi.LA_FLAG_HALF_VOTE), (192, 0)], ids=["d128", "d64-half", "d192"])
def test_maps_under_a_read_list(D, flags, list_dtype):
    bm, _ = _cabi.get_tile_sizes(D, 2, flags)
    q, k = packed_qk(2, 2 * bm + 44, 5 * 64 + 17, 4, 2, D, torch.bfloat16, seed=1)
    lse, smax = lse_of(q, k, D ** -0.5)
    lse[1, 2, bm + 3] = float("-inf")                                         # a row without keys: counts as 0
    read_list = fragmented_rows(4, list_dtype).view(1, 4, 1, 7).expand(3, 4, 3, 7).contiguous().cuda()      # B_alloc = 3 > B
    ref = check_maps(q, k, lse, smax, flags, read_list)
    assert (~torch.isnan(ref.mass_max[0, :, 0])).sum(dim=-1).tolist() == [3, 4, 4, 5]


def test_margins_are_la_vote_margins_own_and_launches_agree_bit_for_bit():
    q, k = packed_qk(2, 2 * 256 + 44, 5 * 64 + 17, 4, 2, 128, torch.bfloat16, seed=3)
    lse, _ = lse_of(q, k, 128 ** -0.5)
    read_list = fragmented_rows(4, torch.int32).view(1, 4, 1, 7).expand(2, 4, 3, 7).contiguous().cuda()
    for rl in (None, read_list):
        a, b = tile_mass(q, k, lse, read_list=rl, flags=0, margins=True), tile_mass(q, k, lse, read_list=rl, flags=0, margins=True)
        assert torch.equal(a.margins.view(torch.int32), vote_margins(q, k, read_list=rl, flags=0).view(torch.int32))
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        alone = tile_mass(q, k, lse, read_list=rl, flags=0)                   # the kernels without the margins: the same masses
        assert alone.margins is None and torch.equal(alone.mass_max.view(torch.int32), a.mass_max.view(torch.int32))


def listed_mask(lists, B, kt):
    """bool (B, H, Qt, Kt): the tiles each list row walks; None = all."""
    rows = lists[:B].cpu().tolist()
    mask = torch.zeros(B, len(rows[0]), len(rows[0][0]), kt, dtype=torch.bool)
    for b, per_b in enumerate(rows):
        for h, per_h in enumerate(per_b):
            for m, row in enumerate(per_h):
                mask[b, h, m, _walk_of_row(row, kt)] = True
    return mask.cuda()


def test_calibrate_mass_schedule_keeps_every_q_tile_inside_its_budget():
    """Replayed on a fresh object: at every step the list the forward writes drops only tiles of the predicted set {margin <= thr}, and
    the fp64 mass_max of what it dropped - under the fp64 LSE of the step's own sparse softmax - sums to at most the budget in every
    q-tile, to the relative bound of the map (the threshold was priced on fp32 masses). A q-tile is excused only when one of its fp64
    margins lies within the margin map's bound (test_gpu_vote_margins.check_map) of the threshold, and at most 5 % of them may be."""
    budgets = [0.05, 0.03, 0.02]
    thresholds, trace = calibrate_mass_schedule(drifting_qkv, 3, budgets, max_batch_size=2)
    assert len(thresholds) == 3 and all(t <= -1e-3 for t in thresholds)
    att = LiteAttention(threshold=-1.0, max_batch_size=2)
    att.set_threshold_schedule(thresholds)
    c, kt, excused, total, dropped_total = 128 ** -0.5 * math.log2(math.e), 20, 0, 0, 0
    for t, budget in enumerate(budgets):
        q, k, v = drifting_qkv(t)
        read = att.current_read_list()
        walked = torch.ones(2, 4, 2, kt, dtype=torch.bool, device="cuda") if read is None else listed_mask(read, 2, kt)
        s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * 128 ** -0.5
        keys = walked.repeat_interleave(256, dim=2).repeat_interleave(64, dim=3)
        lse = torch.logsumexp(s.masked_fill(~keys, float("-inf")), dim=-1).float()
        ref = tile_mass_reference(q, k, lse, read_list=read, margins=True)
        predicted = att.vote_margins(q, k) <= thresholds[t]
        att(q, k, v)
        dropped = walked & ~listed_mask(att.current_read_list(), 2, kt)
        assert not bool((dropped & ~predicted).any())
        mass = torch.where(dropped, ref.mass_max, torch.zeros_like(ref.mass_max)).sum(dim=-1)
        A = float(torch.einsum("bqhd,bkhd->bhqk", q.double().abs(), k.double().abs()).max())
        near = ((ref.margins - thresholds[t]).abs() <= c * 2 * 128 * 2.0 ** -23 * A + 2.0 ** -22 * ref.margins.abs()).any(dim=-1)
        over = mass > budget * (1 + map_eps(q, k, lse, float(s.abs().max()), 256)) + TINY
        print(f"step {t} thr {thresholds[t]:.4f} dropped {int(dropped.sum())} worst mass {float(mass.max()):.4e} budget {budget} "
              f"predicted {trace[t]['predicted_mass']:.4e} over {int(over.sum())}")
        assert not bool((over & ~near).any())
        excused, total, dropped_total = excused + int(over.sum()), total + over.numel(), dropped_total + int(dropped.sum())
    assert excused <= 0.05 * total and dropped_total > 0
