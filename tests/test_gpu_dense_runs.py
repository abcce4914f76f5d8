"""GPU: a long dense key range cut into runs (la_api.hip: fwd_dense_runs) at a shape with more than one batch, head and K/V head.

The other tests of the split (test_gpu_head_dims.py::test_longest_key_sequence, test_gpu_fp8_head_dims.py::
test_dense_key_range_beyond_one_launchs_walk) use batch 1, one head and a contiguous ``out``: every batch and head stride of the runs'
partial O / LSE and of the merge is multiplied by zero there. Here: B = 2, H = 4 on Hk = 2 (GQA), 131 query rows (the partial LSE of a
run is no multiple of 16 bytes), ``out`` a view with padded rows, and the shortest key range that takes two runs with a ragged last
tile: the pinned bound of one launch (tests/golden/walk_bounds.json) + 64 + 37 keys - bf16 at head_dim 256 (102 757 keys) and e4m3 at
head_dim 64 (413 477), the smallest lengths at which each path can go wrong. Reference: fp32 torch on the same inputs, per K/V head.
Tolerances: those of the two tests named above (a split result has two 16-bit roundings: partials, merge)."""
import json
import os

import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu
BOUNDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "walk_bounds.json")
B, H, HK, SQ, PAD, SENTINEL = 2, 4, 2, 131, 64, -7.0


def _reference(q, k, v):
    """fp32 softmax(q k^T / sqrt(D)) v and its log-sum-exp, one K/V head (two query heads) at a time: (B, Sq, H, D), (B, H, Sq)."""
    D, r = q.shape[-1], H // HK
    o, lse = torch.empty(B, SQ, H, D, device=q.device), torch.empty(B, H, SQ, device=q.device)
    for b in range(B):
        for hk in range(HK):
            qh = q[b, :, hk * r:(hk + 1) * r].float().transpose(0, 1).reshape(r * SQ, D)
            sc = qh @ k[b, :, hk].float().T / D ** 0.5
            l = torch.logsumexp(sc, -1)
            o[b, :, hk * r:(hk + 1) * r] = (torch.exp(sc - l[:, None]) @ v[b, :, hk].float()).view(r, SQ, D).transpose(0, 1)
            lse[b, hk * r:(hk + 1) * r] = l.view(r, SQ)
    return o, lse


@pytest.mark.parametrize("dtype,D", [("bf16", 256), ("e4m3", 64)])
def test_two_runs_with_gqa_batches_and_a_strided_out(dtype, D, monkeypatch):
    import liteattention_amd as L
    monkeypatch.delenv("LA_FP8_P", raising=False)                      # e4m3: the default form of P (the reference's arithmetic)
    Sk = json.load(open(BOUNDS))[dtype][str(D)] + 64 + 37
    tdtype = torch.bfloat16 if dtype == "bf16" else torch.float8_e4m3fn
    g = torch.Generator(device="cuda").manual_seed(D)
    q = torch.randn(B, SQ, H, D, device="cuda", generator=g).to(tdtype)
    k = torch.randn(B, Sk, HK, D, device="cuda", generator=g).to(tdtype)
    v = torch.randn(B, Sk, HK, D, device="cuda", generator=g).to(tdtype)
    buf = torch.full((B, SQ, H * D + PAD), SENTINEL, dtype=torch.bfloat16, device="cuda")
    out_view = buf[..., :H * D].view(B, SQ, H, D)                      # rows of H * D + 64 elements
    assert not out_view.is_contiguous()
    from liteattention_amd.flash_attn_interface import mha_fwd
    out, lse, *_ = mha_fwd(q, k, v, out=out_view, softmax_scale=D ** -0.5)
    out2, lse2 = L.flash_attn_func(q, k, v, return_softmax_lse=True)
    ref, ref_lse = _reference(q, k, v)
    assert out.data_ptr() == out_view.data_ptr() and bool(torch.isfinite(out.float()).all())
    err, lse_err = (out.float() - ref).abs().max().item(), (lse - ref_lse).abs().max().item()
    err2, lse_err2 = (out2.float() - ref).abs().max().item(), (lse2 - ref_lse).abs().max().item()
    print(f"{dtype} d{D} Sk={Sk}: |O - ref| {err:.3e} / {err2:.3e} (max|ref| {ref.abs().max().item():.3e}), |LSE - ref| {lse_err:.3e} / {lse_err2:.3e}")
    if dtype == "bf16":
        o_tol, lse_tol = 2.0 ** -7 * ref.abs().max().item() + 1e-3, 1e-3
    else:
        o_tol, lse_tol = 0.05 * ref.abs().max().item() + 2e-3, helpers.fp8_lse_tol_vs_exact()
    assert err <= o_tol and err2 <= o_tol
    assert lse_err <= lse_tol and lse_err2 <= lse_tol
    assert torch.equal(out, out2) and torch.equal(lse, lse2)           # the same runs and the same merge, whatever the strides of out
    assert bool((buf[..., H * D:] == SENTINEL).all())                  # the padding of the strided out is untouched
