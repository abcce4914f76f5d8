"""CPU: la_vote_margins is exported, declared and bound and returns every code of its contract without a device; the fp64 reference of
the map equals the oracle's ``margins=``; ``threshold_for_skip`` hits its target on a hand-made tensor."""
import ctypes
import math
import os
import re

import pytest
import torch

from liteattention_amd import _cabi, threshold_for_skip, vote_margins_reference
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_declared_and_bound():
    lib = _cabi.load()
    header = open(os.path.join(ROOT, "include", "lite_attention_amd.h")).read()
    assert re.search(r"^int la_vote_margins\(const la_vote_margins_args\* args, void\* stream\);", header, flags=re.M)
    assert "la_vote_margins" in _cabi.EXPORTED_SYMBOLS and lib.la_vote_margins.argtypes[0]._type_ is _cabi.LaVoteMarginsArgs


def _args(**over):
    a = _cabi.LaVoteMarginsArgs()
    a.struct_size, a.dtype = ctypes.sizeof(_cabi.LaVoteMarginsArgs), _cabi.LA_DTYPE_BF16
    a.q, a.k, a.margins = 0x10000, 0x20000, 0x30000
    a.batch, a.seqlen_q, a.seqlen_k, a.num_heads, a.num_heads_k, a.head_dim = 2, 300, 500, 4, 2, 128
    a.q_batch_stride, a.q_row_stride, a.q_head_stride = 300 * 4 * 128, 4 * 128, 128
    a.k_batch_stride, a.k_row_stride, a.k_head_stride = 500 * 2 * 128, 2 * 128, 128
    a.softmax_scale = 128 ** -0.5
    for name, val in over.items():
        setattr(a, name, val)
    return a


@pytest.mark.parametrize("over,code", [
    (dict(struct_size=8), _cabi.LA_ERR_STRUCT_SIZE),
    (dict(dtype=_cabi.LA_DTYPE_FP8_E4M3), _cabi.LA_ERR_DTYPE), (dict(dtype=_cabi.LA_DTYPE_FP32), _cabi.LA_ERR_DTYPE),
    (dict(q=None), _cabi.LA_ERR_NULL_ARG), (dict(k=None), _cabi.LA_ERR_NULL_ARG), (dict(margins=None), _cabi.LA_ERR_NULL_ARG),
    (dict(batch=0), _cabi.LA_ERR_SHAPE), (dict(seqlen_k=0), _cabi.LA_ERR_SHAPE), (dict(num_heads_k=3), _cabi.LA_ERR_SHAPE),
    (dict(head_dim=80), _cabi.LA_ERR_HEAD_DIM), (dict(head_dim=100), _cabi.LA_ERR_HEAD_DIM),
    (dict(head_dim=96, flags=_cabi.LA_FLAG_KERNEL_128ROW), _cabi.LA_ERR_HEAD_DIM),
    (dict(q_row_stride=4 * 128 + 4), _cabi.LA_ERR_STRIDE), (dict(k_head_stride=-128), _cabi.LA_ERR_STRIDE),
    (dict(q=0x10008), _cabi.LA_ERR_STRIDE), (dict(margins=0x30002), _cabi.LA_ERR_STRIDE),
    (dict(read_list=0x40002), _cabi.LA_ERR_STRIDE),
    (dict(read_list=0x40000, flags=_cabi.LA_FLAG_LIST_INT16, seqlen_k=64 * 32767), _cabi.LA_ERR_SEQLEN),
    (dict(seqlen_k=64 * 40000), _cabi.LA_ERR_SEQLEN),                          # the walk storage of a workgroup
    (dict(batch=1 << 20, num_heads=1 << 12, num_heads_k=1 << 12), _cabi.LA_ERR_SHAPE),   # more workgroups than a grid holds
])
def test_every_error_code_is_returned_without_a_device(over, code):
    lib = _cabi.load()
    assert lib.la_vote_margins(None, None) == _cabi.LA_ERR_NULL_ARG
    assert lib.la_vote_margins(ctypes.byref(_args(**over)), None) == code


def _operands(Sq, Sk, H=2, D=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, Sq, H, D, generator=g).to(torch.bfloat16), torch.randn(1, Sk, H, D, generator=g).to(torch.bfloat16))


def margin_bound(q, k, scale, ref):
    """|m - ref| <= c 2 D 2^-23 A + 2^-22 |ref|, A = max_ij sum_d |q_id| |k_jd| in fp64: products of 16-bit operands are exact in
    fp32, so this bounds any fp32 accumulation order of D terms, doubled for the two maxima a margin subtracts."""
    A = torch.einsum("bqhd,bkhd->bhqk", q.double().abs(), k.double().abs().repeat_interleave(q.shape[2] // k.shape[2], dim=2)).max()
    return scale * math.log2(math.e) * 2 * q.shape[3] * 2.0 ** -23 * float(A) + 2.0 ** -22 * ref.abs()


@pytest.mark.parametrize("fragmented", [False, True], ids=["dense", "fragmented"])
def test_reference_equals_the_oracle_margins(fragmented):
    bm, bn, Sq, Sk = 128, 64, 128 + 44, 5 * 64 + 17                           # ragged Sq and Sk: zero rows vote, tile 5 is masked
    q, k = _operands(Sq, Sk)
    read_list = None
    if fragmented:                                                            # three ranges, the first tile walked is not Kt - 1
        read_list = torch.tensor([[6, 4, 4, 5, 5, 2, 0], [4, 3, 1, 5, 5, 0, 0]], dtype=torch.int32).repeat(2, 1).view(1, 2, 2, 7).contiguous()
    got = torch.empty(1, 2, 2, 6, dtype=torch.float32)
    orc.qkskip_fwd(q, k, k, block_m=bm, block_n=bn, read_list=read_list, margins=got)
    ref = vote_margins_reference(q, k, read_list=read_list, block_m=bm, block_n=bn)
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    walked = ~torch.isnan(ref)
    assert int(walked.sum()) == (4 * 5 if not fragmented else 2 * (4 + 3))
    assert bool(((got.double() - ref).abs() <= margin_bound(q, k, 64 ** -0.5, ref))[walked].all())


@pytest.mark.parametrize("per_head", [False, True], ids=["global", "per-head"])
@pytest.mark.parametrize("target", [0.0, 0.3, 0.5, 1.0])
def test_threshold_for_skip_hits_the_target_to_within_one_tile(per_head, target):
    g = torch.Generator().manual_seed(1)
    m = torch.randn(2, 3, 4, 9, generator=g) * torch.tensor([1.0, 3.0, 0.2]).view(1, 3, 1, 1) - 2.0
    m[..., 8] = float("nan")                                                  # first tiles
    m[0, 1, 2, :5] = float("nan")                                             # tiles not walked
    thr = threshold_for_skip(m, target, per_head=per_head)
    groups = [(m[:, h], float(thr[h])) for h in range(3)] if per_head else [(m, thr)]
    assert (tuple(thr.shape) == (3,) and thr.dtype == torch.float32) if per_head else isinstance(thr, float)
    for vals, t in groups:
        n = int(torch.isfinite(vals).sum())
        assert abs(int((vals <= t).sum()) - target * n) <= 1.0
