"""CPU: la_vote_margins_fp8 is exported, declared and bound and returns every code of its contract without a device; the fp64 reference
of the map on e4m3 operands with descales is the 16-bit reference on the (exact) bf16 casts with the descales folded into the scale."""
import ctypes
import os
import re

import pytest
import torch

from liteattention_amd import _cabi, vote_margins_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_declared_and_bound():
    lib = _cabi.load()
    header = open(os.path.join(ROOT, "include", "lite_attention_amd.h")).read()
    assert re.search(r"^int la_vote_margins_fp8\(const la_vote_margins_fp8_args\* args, void\* stream\);", header, flags=re.M)
    assert "la_vote_margins_fp8" in _cabi.EXPORTED_SYMBOLS and lib.la_vote_margins_fp8.argtypes[0]._type_ is _cabi.LaVoteMarginsFp8Args


def _args(**over):
    a = _cabi.LaVoteMarginsFp8Args()
    a.struct_size = ctypes.sizeof(_cabi.LaVoteMarginsFp8Args)
    a.q, a.k, a.margins, a.q_descale, a.k_descale = 0x10000, 0x20000, 0x30000, 0x50000, 0x60000
    a.batch, a.seqlen_q, a.seqlen_k, a.num_heads, a.num_heads_k, a.head_dim = 2, 300, 500, 4, 2, 128
    a.q_batch_stride, a.q_row_stride, a.q_head_stride = 300 * 4 * 128, 4 * 128, 128
    a.k_batch_stride, a.k_row_stride, a.k_head_stride = 500 * 2 * 128, 2 * 128, 128
    a.q_descale_batch_stride, a.q_descale_head_stride, a.k_descale_batch_stride, a.k_descale_head_stride = 2, 1, 2, 1
    a.softmax_scale = 128 ** -0.5
    for name, val in over.items():
        setattr(a, name, val)
    return a


@pytest.mark.parametrize("over,code", [
    (dict(struct_size=8), _cabi.LA_ERR_STRUCT_SIZE), (dict(struct_size=ctypes.sizeof(_cabi.LaVoteMarginsArgs)), _cabi.LA_ERR_STRUCT_SIZE),
    (dict(q=None), _cabi.LA_ERR_NULL_ARG), (dict(k=None), _cabi.LA_ERR_NULL_ARG), (dict(margins=None), _cabi.LA_ERR_NULL_ARG),
    (dict(batch=0), _cabi.LA_ERR_SHAPE), (dict(seqlen_k=0), _cabi.LA_ERR_SHAPE), (dict(num_heads_k=3), _cabi.LA_ERR_SHAPE),
    (dict(head_dim=80), _cabi.LA_ERR_HEAD_DIM), (dict(head_dim=100), _cabi.LA_ERR_HEAD_DIM),
    (dict(q_row_stride=4 * 128 + 8), _cabi.LA_ERR_STRIDE), (dict(k_head_stride=-128), _cabi.LA_ERR_STRIDE),
    (dict(q=0x10008), _cabi.LA_ERR_STRIDE), (dict(margins=0x30002), _cabi.LA_ERR_STRIDE),
    (dict(read_list=0x40002), _cabi.LA_ERR_STRIDE),
    (dict(q_descale=0x50002), _cabi.LA_ERR_STRIDE), (dict(k_descale=0x60001), _cabi.LA_ERR_STRIDE),
    (dict(q_descale_head_stride=-1), _cabi.LA_ERR_STRIDE), (dict(k_descale_batch_stride=-2), _cabi.LA_ERR_STRIDE),
    (dict(read_list=0x40000, flags=_cabi.LA_FLAG_LIST_INT16, seqlen_k=64 * 32767), _cabi.LA_ERR_SEQLEN),
    (dict(seqlen_k=64 * 40000), _cabi.LA_ERR_SEQLEN),                          # the walk storage of a workgroup
    (dict(batch=1 << 20, num_heads=1 << 12, num_heads_k=1 << 12), _cabi.LA_ERR_SHAPE),   # more workgroups than a grid holds
])
def test_every_error_code_is_returned_without_a_device(over, code):
    lib = _cabi.load()
    assert lib.la_vote_margins_fp8(None, None) == _cabi.LA_ERR_NULL_ARG
    assert lib.la_vote_margins_fp8(ctypes.byref(_args(**over)), None) == code


@pytest.mark.parametrize("fragmented", [False, True], ids=["dense", "fragmented"])
def test_reference_with_descales_is_the_16_bit_reference_at_the_folded_scale(fragmented):
    g = torch.Generator().manual_seed(0)
    Sq, Sk, D, qd, kd = 128 + 44, 5 * 64 + 17, 96, 1.375, 0.8125
    q, k = (torch.randn(1, S, 2, D, generator=g).to(torch.float8_e4m3fn) for S in (Sq, Sk))
    read_list = None
    if fragmented:
        read_list = torch.tensor([[6, 4, 4, 5, 5, 2, 0], [4, 3, 1, 5, 5, 0, 0]], dtype=torch.int32).repeat(2, 1).view(1, 2, 2, 7).contiguous()
    got = vote_margins_reference(q, k[:, :, :1], 0.11, read_list, block_m=128, q_descale=torch.tensor([[qd]]), k_descale=torch.tensor([[kd]]))
    ref = vote_margins_reference(q.bfloat16(), k[:, :, :1].bfloat16(), 0.11 * qd * kd, read_list, block_m=128)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and int((~torch.isnan(ref)).sum()) == (20 if not fragmented else 14)
    assert bool(((got - ref).abs() <= 2.0 ** -50 * ref.abs())[~torch.isnan(ref)].all())        # c is rounded in another order
