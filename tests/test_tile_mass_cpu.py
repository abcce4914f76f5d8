"""CPU: la_tile_mass is exported, declared and bound and returns every code of its contract without a device; the fp64 reference of the
map sums to 1 over a dense walk and is NaN exactly at unwalked tiles; ``threshold_for_mass`` on hand-made maps."""
import ctypes
import os
import re

import pytest
import torch

from liteattention_amd import _cabi, threshold_for_mass, tile_mass_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSE, MAX, MEAN = 0x50000, 0x60000, 0x70000


def test_symbol_is_exported_declared_and_bound():
    lib = _cabi.load()
    header = open(os.path.join(ROOT, "include", "lite_attention_amd.h")).read()
    assert re.search(r"^int la_tile_mass\(const la_vote_margins_args\* args, const float\* lse, float\* mass_max, float\* mass_mean, "
                     r"void\* stream\);", header, flags=re.M)
    assert "la_tile_mass" in _cabi.EXPORTED_SYMBOLS and lib.la_tile_mass.argtypes[0]._type_ is _cabi.LaVoteMarginsArgs
    assert lib.la_abi_version() == _cabi.LA_ABI_VERSION == 9


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


# in the order of the contract: a case that breaks two rules returns the code of the earlier one
@pytest.mark.parametrize("over,ptrs,code", [
    (dict(struct_size=8, dtype=_cabi.LA_DTYPE_FP32), (LSE, MAX, MEAN), _cabi.LA_ERR_STRUCT_SIZE),
    (dict(dtype=_cabi.LA_DTYPE_FP8_E4M3, q=None), (LSE, MAX, MEAN), _cabi.LA_ERR_DTYPE),
    (dict(q=None, batch=0), (LSE, MAX, MEAN), _cabi.LA_ERR_NULL_ARG),
    (dict(k=None), (LSE, MAX, MEAN), _cabi.LA_ERR_NULL_ARG),
    (dict(num_heads_k=3, head_dim=80), (LSE, MAX, MEAN), _cabi.LA_ERR_SHAPE),
    (dict(head_dim=80, q=0x10008), (LSE, MAX, MEAN), _cabi.LA_ERR_HEAD_DIM),
    (dict(head_dim=96, flags=_cabi.LA_FLAG_KERNEL_128ROW), (LSE, MAX, MEAN), _cabi.LA_ERR_HEAD_DIM),
    (dict(q_row_stride=4 * 128 + 4), (None, MAX, MEAN), _cabi.LA_ERR_STRIDE),
    (dict(margins=0x30002), (None, MAX, MEAN), _cabi.LA_ERR_STRIDE),
    (dict(read_list=0x40000, flags=_cabi.LA_FLAG_LIST_INT16, seqlen_k=64 * 32767), (None, MAX, MEAN), _cabi.LA_ERR_SEQLEN),
    (dict(batch=1 << 20, num_heads=1 << 12, num_heads_k=1 << 12), (None, MAX, MEAN), _cabi.LA_ERR_SHAPE),
    (dict(), (None, MAX + 2, MEAN), _cabi.LA_ERR_NULL_ARG),                   # NULL lse
    (dict(margins=None), (LSE + 2, None, None), _cabi.LA_ERR_NULL_ARG),       # no output at all
    (dict(), (LSE + 2, MAX, MEAN), _cabi.LA_ERR_STRIDE),
    (dict(), (LSE, MAX + 2, MEAN), _cabi.LA_ERR_STRIDE),
    (dict(seqlen_k=64 * 30332), (LSE, MAX, MEAN + 1), _cabi.LA_ERR_STRIDE),
    # head_dim 128: 30 332 key tiles fit la_vote_margins' 64-byte head and not the 128 bytes of three outputs (the test below)
    (dict(seqlen_k=64 * 30332), (LSE, MAX, MEAN), _cabi.LA_ERR_SEQLEN),
])
def test_every_error_code_is_returned_in_order_without_a_device(over, ptrs, code):
    lib = _cabi.load()
    assert lib.la_tile_mass(None, LSE, MAX, MEAN, None) == _cabi.LA_ERR_NULL_ARG
    assert lib.la_tile_mass(ctypes.byref(_args(**over)), *ptrs, None) == code


def test_lds_boundary_of_the_case_above():
    """What the last case of the table leans on, from the sizes the header states."""
    ring = 2 * 64 * (2 * 128 + 16)
    walk = lambda kt: 4 * ((kt + 3) & ~3) + 8 * ((kt + 31) // 32)       # noqa: E731
    assert ring + 64 + walk(30332) <= 160 * 1024 < ring + 128 + walk(30332)
    big = _args(seqlen_k=64 * 30332, batch=1 << 20, num_heads=1 << 12, num_heads_k=1 << 12)      # past la_vote_margins' LDS check: the next one
    assert _cabi.load().la_vote_margins(ctypes.byref(big), None) == _cabi.LA_ERR_SHAPE


def test_reference_sums_to_one_and_marks_unwalked_tiles():
    bm, bn, Sq, Sk, H = 128, 64, 128 + 44, 5 * 64 + 17, 2                     # ragged Sq and Sk
    g = torch.Generator().manual_seed(0)
    q, k = torch.randn(1, Sq, H, 64, generator=g).to(torch.bfloat16), torch.randn(1, Sk, H, 64, generator=g).to(torch.bfloat16)
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * 64 ** -0.5
    lse = torch.logsumexp(s, dim=-1)
    dense = tile_mass_reference(q, k, lse, block_m=bm, block_n=bn)
    assert dense.margins is None and not bool(torch.isnan(dense.mass_max).any())
    assert torch.allclose(dense.mass_mean.sum(dim=-1), torch.ones(1, H, 2, dtype=torch.float64), rtol=0, atol=1e-12)
    assert bool((dense.mass_max >= dense.mass_mean).all())
    # a row without a finite lse counts as 0: the mean of its q-tile loses exactly that row's share, 1 / rows
    lse[0, 1, 130] = float("-inf")
    holed = tile_mass_reference(q, k, lse.transpose(1, 2), block_m=bm, block_n=bn)          # the (B, Sq, H) view
    assert abs(float(holed.mass_mean[0, 1, 1].sum()) - 43 / 44) < 1e-12 and torch.equal(holed.mass_mean[0, 0], dense.mass_mean[0, 0])
    # three ranges, the first tile walked is not Kt - 1: NaN exactly off the walk, and the first walked tile has a mass
    read_list = torch.tensor([[6, 4, 4, 5, 5, 2, 0], [4, 3, 1, 5, 5, 0, 0]], dtype=torch.int32).repeat(2, 1).view(1, 2, 2, 7).contiguous()
    listed = tile_mass_reference(q, k, lse, read_list=read_list, block_m=bm, block_n=bn, margins=True)
    walked = torch.tensor([[1, 1, 1, 0, 1, 1], [0, 1, 1, 1, 0, 1]] * 2, dtype=torch.bool).view(1, 2, 2, 6)      # walks 4 5 2 1 0 and 3 2 1 5
    for got, full in ((listed.mass_max, holed.mass_max), (listed.mass_mean, holed.mass_mean)):
        assert torch.equal(~torch.isnan(got), walked) and torch.equal(got[walked], full[walked])
    first = torch.zeros_like(walked)
    first[0, :, 0, 4] = first[0, :, 1, 3] = True
    assert torch.equal(~torch.isnan(listed.margins), walked & ~first)


def test_threshold_for_mass_on_hand_made_maps():
    nan = float("nan")
    # (B 1, H 2, Qt 2, Kt 4); head 0 / q-tile 0 breaks a budget of 0.25 at margin -2 (0.1 + 0.1 + 0.2), q-tile 1 never does
    margins = torch.tensor([[[[-4.0, -3.0, -2.0, nan], [-5.0, -1.0, nan, nan]],
                             [[-8.0, -6.0, -7.0, nan], [-9.0, -2.5, -0.5, nan]]]])
    mass = torch.tensor([[[[0.1, 0.1, 0.2, 0.6], [0.05, 0.05, nan, 0.9]],
                          [[0.2, 0.2, 0.01, 0.59], [0.01, 0.02, 0.03, 0.94]]]])
    assert threshold_for_mass(margins, mass, 0.25) == pytest.approx(-6.5)               # head 1 breaks first, at -6 (0.2 + 0.01 + 0.2)
    per_head = threshold_for_mass(margins, mass, 0.25, per_head=True)
    assert per_head.dtype == torch.float32 and per_head.tolist() == [-2.5, -6.5]        # midpoints: (-3, -2) and (-7, -6)
    assert threshold_for_mass(margins, mass, 1.0) == pytest.approx(-1e-3)               # nothing breaks: one above the largest, capped
    assert threshold_for_mass(margins, mass, 1.0, hi=-3.5) == pytest.approx(-3.5)
    assert threshold_for_mass(margins, mass, 0.0) == pytest.approx(-10.0)               # nothing fits: one below the smallest
    # mean over the 4 q-tiles of the summed mass, in margin order: .0025 .0525 .055 (-7) .105 (-6) ... .1725 (-2.5) .2225 (-2) ...
    assert threshold_for_mass(margins, mass, 0.21, reduce="mean") == pytest.approx(-2.25)
    assert threshold_for_mass(margins, mass, 0.1, reduce="mean") == pytest.approx(-6.5)
    # per head, over its 2 q-tiles: head 0 .025 (-5) .075 (-4); head 1 .005 (-9) .105 (-8)
    assert threshold_for_mass(margins, mass, 0.06, reduce="mean", per_head=True).tolist() == [-4.5, -8.5]
