#!/usr/bin/env python
"""A Wan2.x-style self-attention block running on `from lite_attention import LiteAttention` — the integration recipe of the
reference's README (README.md:268-323) applied to a self-contained stand-in for `WanSelfAttention` (Wan2.1
wan/modules/model.py): q/k/v projections, RMSNorm on q and k, 3-axis RoPE over the (frames, height, width) latent grid,
q/k/v cast to bf16, ONE `self.lite_attention(q, k, v)` call, result back to fp32, output projection. Random weights (no
checkpoints here); what it demonstrates is the drop-in at the module boundary: shapes, dtypes, one LiteAttention instance
per layer, the skip state carried across denoising steps.

    python examples/wan_self_attention_demo.py [--frames 5 --height 16 --width 16 --heads 4 --steps 6 --threshold -6] [--fused-prep]

`--fused-prep` (`fused_prep=True` on the modules): RMSNorm, RoPE and the bf16 cast of q and k run as ONE pass each (`qk_prep`) instead of
the eager lines below. `--fp8 --smooth-k`: each key head's mean over the tokens is subtracted before the e4m3 cast (`SmoothedQK`); the
output needs no correction. `--fp8 --smooth-v` (combinable with `--smooth-k`): the same for V (`SmoothedV`); the mean is added back to
the attention output by the restoring pass, which also replaces the block's `.float()` (`out_dtype=torch.float32`).
`--fp8 [--smooth-v] --v-tiles`: V is quantized straight into the V^T tiles the e4m3 forward stages (`v_prep_tiles`) and handed to the
attention call as a `PreparedV`: the same codes, no e4m3 V tensor. (The block with skipping disabled is then never split over the
keys; with a tensor V it is above 704 keys, so its rows agree with those of the tensor route to rounding there, bit for bit below.)

`--brick-order [BT,BH,BW ...]` (with the fused prologue; default bricks 1,16,16 1,8,8): the block runs on the tokens in brick order
(`brick_order`) - the hidden states are gathered ONCE on entry, q and k are rotated as the positions the rows have
(`qk_prep(positions=order)`), v and the output need nothing, and the result is restored at the exit. Prints the largest difference of
the attention output to the raster run, beside the reference's tolerance rule for it.

Prints, per denoising step, the fraction of tiles skipped and the error against the same block with skipping disabled.
"""
import argparse
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lite_attention import LiteAttention  # noqa: E402  (same import line as the reference recipe)
from lite_attention import qk_prep, rope_tables  # noqa: E402  (the fused q / k prologue: fused_prep=True)
from lite_attention import E4m3Scales  # noqa: E402  (its e4m3 form with per-head scales: fp8=True)
from lite_attention import SmoothedQK  # noqa: E402  (... with the keys mean-shifted before they are quantized: smooth_k=True)
from lite_attention import SmoothedV  # noqa: E402  (... and V: smooth_v=True; the attention call adds the mean back to its output)
from lite_attention import attn_out_fp8, attn_unshift  # noqa: E402  (O restored as row-scaled e4m3 for an fp8 output projection: fp8_oproj=True)
from lite_attention import brick_order  # noqa: E402  (token orders: the block on 3-D bricks of the latent grid instead of raster stripes)


class RMSNorm(nn.Module):
    def __init__(self, dim, eps=1e-6):
        super().__init__()
        self.eps, self.weight = eps, nn.Parameter(torch.ones(dim))

    def forward(self, x):
        return (x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + self.eps)).type_as(x) * self.weight


def rope_3d(x, grid, theta=10000.0):
    """x (B, S, H, D) with S = F*Hh*W tokens in (f, h, w) order; the head dim is split over the three axes as Wan does
    (d - 2*(d//3), d//3, d//3), each part rotated by its own coordinate."""
    B, S, H, D = x.shape
    F, Hh, W = grid
    parts = [D - 2 * (D // 3), D // 3, D // 3]
    parts = [p - (p % 2) for p in parts]
    parts[0] = D - parts[1] - parts[2]
    f = torch.arange(F, device=x.device).view(F, 1, 1).expand(F, Hh, W).reshape(-1)
    h = torch.arange(Hh, device=x.device).view(1, Hh, 1).expand(F, Hh, W).reshape(-1)
    w = torch.arange(W, device=x.device).view(1, 1, W).expand(F, Hh, W).reshape(-1)
    out, off = [], 0
    for pos, d in zip((f, h, w), parts):
        freqs = 1.0 / theta ** (torch.arange(0, d, 2, device=x.device).float() / d)
        ang = pos.float()[:, None] * freqs[None]                       # (S, d/2)
        cos, sin = ang.cos()[None, :, None], ang.sin()[None, :, None]
        xs = x[..., off:off + d].float().reshape(B, S, H, d // 2, 2)
        a, b = xs[..., 0], xs[..., 1]
        out.append(torch.stack((a * cos - b * sin, a * sin + b * cos), dim=-1).reshape(B, S, H, d))
        off += d
    return torch.cat(out, dim=-1).type_as(x)


def fp8_linear(r, linear):
    """`linear` on a RowScaledE4m3 activation (one scale per token), its weight quantized per OUTPUT channel in torch:
    `torch._scaled_mm` with row-wise scales where this torch / ROCm accepts the call, else the two operands dequantised and a
    matmul. Returns (y fp32, which of the two ran)."""
    a, sa = r.as_matrix()                                           # (B * S, H * D) e4m3, (B * S, 1) fp32
    w = linear.weight.float()                                       # (out, in)
    sw = w.abs().amax(dim=1, keepdim=True).clamp_min(2.0 ** -100) / 448.0
    w8 = (w / sw).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    try:
        y = torch._scaled_mm(a, w8.t(), scale_a=sa, scale_b=sw.t().contiguous(), out_dtype=torch.bfloat16).float()
        how = "torch._scaled_mm with row-wise scales"
    except Exception as e:                                          # this build has no row-wise form: the same product, dequantised
        y = (a.float() * sa) @ (w8.float() * sw).t()
        how = f"dequantise + matmul (torch._scaled_mm refused: {type(e).__name__})"
    if linear.bias is not None:
        y = y + linear.bias.float()
    return y.view(*r.data.shape[:2], -1), how


class WanLikeSelfAttention(nn.Module):
    def __init__(self, dim, num_heads, threshold=-10.0, enable_skipping=True, max_batch_size=1, fused_prep=False, *, fp8=False,
                 fp8_mode="current", fp8_margin=1.0, smooth_k=False, smooth_v=False, v_tiles=False, fp8_oproj=False):
        super().__init__()
        assert dim % num_heads == 0
        self.num_heads, self.head_dim, self.fused_prep = num_heads, dim // num_heads, fused_prep
        # fp8: q, k and v are produced in e4m3 by qk_prep_fp8, each with the per-head scales of its own E4m3Scales
        self.fp8 = fp8
        # v_tiles: v is quantized straight into the V^T tiles of the e4m3 forward (a PreparedV): no e4m3 V tensor, no prepare pass
        assert fp8 or not v_tiles, "v_tiles is a form of the fp8 path"
        self.scales = [E4m3Scales(mode=fp8_mode, margin=fp8_margin, tiles=v_tiles and i == 2) for i in range(3)] if fp8 else None
        # smooth_k: q and k go through one SmoothedQK instead (k first, q with the dots that would restore the LSE); v as before
        assert fp8 or not smooth_k, "smooth_k is a form of the fp8 path"
        self.smoothed = SmoothedQK(mode=fp8_mode, margin=fp8_margin) if smooth_k else None
        # smooth_v: v goes through a SmoothedV; the attention call restores O (v_shift) and hands it on in fp32 (out_dtype)
        assert fp8 or not smooth_v, "smooth_v is a form of the fp8 path"
        self.smoothed_v = SmoothedV(mode=fp8_mode, margin=fp8_margin, tiles=v_tiles) if smooth_v else None
        # fp8_oproj: the restoring pass writes row-scaled e4m3 (attn_out_fp8) and the output projection runs on it (fp8_linear)
        assert fp8 or not fp8_oproj, "fp8_oproj is a form of the fp8 path"
        self.fp8_oproj, self.oproj_how, self.oproj_error = fp8_oproj, None, None
        self.q, self.k, self.v, self.o = (nn.Linear(dim, dim) for _ in range(4))
        self.norm_q, self.norm_k = RMSNorm(dim), RMSNorm(dim)
        # the recipe: ONE LiteAttention per attention layer (its skip lists are that layer's state)
        self.lite_attention = LiteAttention(enable_skipping=enable_skipping, threshold=threshold, max_batch_size=max_batch_size)
        self.keep_last, self.last = False, None                     # keep_last: (q, k, v, o) of the fused-prep path stay for inspection

    def forward(self, x, grid, order=None):
        """order: a TokenOrder the rows of x are ALREADY in (gathered at the model boundary): q and k are rotated as the positions
        the rows have; v, the attention call and the output projection are per row and need nothing (fused_prep only)."""
        b, s, n, d = *x.shape[:2], self.num_heads, self.head_dim
        assert order is None or (self.fused_prep and not self.fp8), "a token order runs through the fused prologue"
        if self.fp8:                                                # norm + rope + scale + e4m3 cast of q and k, scale + cast of v
            tables = rope_tables(grid, d, device=x.device)
            if self.smoothed is not None:
                q, k, dq, dk, _ = self.smoothed.pair(self.q(x).view(b, s, n, d), self.k(x).view(b, s, n, d), self.norm_q.weight,
                                                     self.norm_k.weight, self.norm_q.eps, tables)
            else:
                q, dq = self.scales[0](self.q(x).view(b, s, n, d), self.norm_q.weight, self.norm_q.eps, tables)
                k, dk = self.scales[1](self.k(x).view(b, s, n, d), self.norm_k.weight, self.norm_k.eps, tables)
            if self.fp8_oproj:
                v_shift = None
                if self.smoothed_v is not None:
                    v, dv, v_shift = self.smoothed_v(self.v(x).view(b, s, n, d))
                else:
                    v, dv = self.scales[2](self.v(x).view(b, s, n, d), norm=None)
                o, lse = self.lite_attention(q, k, v, q_descale=dq, k_descale=dk, v_descale=dv, return_softmax_lse=True)
                y, self.oproj_how = fp8_linear(attn_out_fp8(o, v_shift, lse=lse), self.o)       # one scale per token
                y16 = self.o(attn_unshift(o, v_shift, lse=lse).float().flatten(2))             # the bf16 path, for the comparison
                self.oproj_error = ((y - y16).abs().max() / y16.abs().max()).item()
                return y
            if self.smoothed_v is not None:                         # the block's .float() becomes the restoring pass' out_dtype
                v, dv, v_shift = self.smoothed_v(self.v(x).view(b, s, n, d))
                return self.o(self.lite_attention(q, k, v, q_descale=dq, k_descale=dk, v_descale=dv, v_shift=v_shift,
                                                  out_dtype=torch.float32).flatten(2))
            v, dv = self.scales[2](self.v(x).view(b, s, n, d), norm=None)
            return self.o(self.lite_attention(q, k, v, q_descale=dq, k_descale=dk, v_descale=dv).float().flatten(2))
        if self.fused_prep:                                         # norm + rope + cast of q and of k: one pass each
            tables = rope_tables(grid, d, device=x.device)
            q = qk_prep(self.q(x).view(b, s, n, d), self.norm_q.weight, self.norm_q.eps, tables, out_dtype=torch.bfloat16, positions=order)
            k = qk_prep(self.k(x).view(b, s, n, d), self.norm_k.weight, self.norm_k.eps, tables, out_dtype=torch.bfloat16, positions=order)
            v = self.v(x).view(b, s, n, d).bfloat16()
            o = self.lite_attention(q, k, v)
            if self.keep_last:
                self.last = (q, k, v, o)
            return self.o(o.float().flatten(2))
        q = self.norm_q(self.q(x)).view(b, s, n, d)
        k = self.norm_k(self.k(x)).view(b, s, n, d)
        v = self.v(x).view(b, s, n, d)
        q_rope, k_rope = rope_3d(q, grid), rope_3d(k, grid)
        x = self.lite_attention(q_rope.bfloat16(), k_rope.bfloat16(), v.bfloat16())       # (B, S, H, D) bf16
        return self.o(x.float().flatten(2))


class WanLikeCrossAttention(nn.Module):
    """The text-conditioning attention of a Wan2.x block as the stock pipeline writes it: its `flash_attention()` wrapper imports
    `flash_attn` / `flash_attn_interface` and calls `flash_attn_varlen_func` on packed (total, H, D) tensors with `cu_seqlens`
    because the prompts of a batch have different lengths. With `compat_shims/` on the path those imports resolve to the gfx950
    kernel: one dense launch for the whole ragged batch, no host sync."""

    def __init__(self, dim, num_heads, fused_prep=False):
        super().__init__()
        self.num_heads, self.head_dim, self.fused_prep = num_heads, dim // num_heads, fused_prep
        self.q, self.k, self.v, self.o = (nn.Linear(dim, dim) for _ in range(4))
        self.norm_q, self.norm_k = RMSNorm(dim), RMSNorm(dim)

    def forward(self, x, context, context_lens):
        import flash_attn_interface                                 # FA3 name, served by compat_shims/flash_attn_interface.py
        b, s, n, d = *x.shape[:2], self.num_heads, self.head_dim
        lens = [int(l) for l in context_lens]
        if self.fused_prep:                                         # no rope on the text side: norm + cast, one pass each
            q = qk_prep(self.q(x).view(b, s, n, d), self.norm_q.weight, self.norm_q.eps, out_dtype=torch.bfloat16).view(b * s, n, d)
            k_all = torch.cat([self.k(context[i, :l]) for i, l in enumerate(lens)]).view(1, -1, n, d)
            k = qk_prep(k_all, self.norm_k.weight, self.norm_k.eps, out_dtype=torch.bfloat16).view(-1, n, d)
        else:
            q = self.norm_q(self.q(x)).view(b * s, n, d).bfloat16()
            k = torch.cat([self.norm_k(self.k(context[i, :l])) for i, l in enumerate(lens)]).view(-1, n, d).bfloat16()
        v = torch.cat([self.v(context[i, :l]) for i, l in enumerate(lens)]).view(-1, n, d).bfloat16()
        cu_q = torch.arange(0, (b + 1) * s, s, dtype=torch.int32, device=x.device)
        cu_k = torch.tensor([0] + lens, device=x.device).cumsum(0).to(torch.int32)
        out = flash_attn_interface.flash_attn_varlen_func(q, k, v, cu_q, cu_k, s, max(lens))
        return self.o(out.view(b, s, n * d).float())

    def reference(self, x, context, context_lens):
        b, s, n, d = *x.shape[:2], self.num_heads, self.head_dim
        q = self.norm_q(self.q(x)).view(b, s, n, d).bfloat16().float()
        outs = []
        for i, l in enumerate(int(l) for l in context_lens):
            k = self.norm_k(self.k(context[i, :l])).view(l, n, d).bfloat16().float()
            v = self.v(context[i, :l]).view(l, n, d).bfloat16().float()
            p = torch.softmax(torch.einsum("qhd,khd->hqk", q[i], k) * d ** -0.5, -1)
            outs.append(torch.einsum("hqk,khd->qhd", p, v).reshape(s, n * d))
        return self.o(torch.stack(outs))


def run(frames=5, height=16, width=16, heads=4, steps=6, threshold=-6.0, seed=0, device="cuda", verbose=True, fused_prep=False, *,
        fp8=False, fp8_mode="current", fp8_margin=1.0, smooth_k=False, smooth_v=False, v_tiles=False, bricks=None, fp8_oproj=False):
    """bricks: None (raster order), or the brick levels of `brick_order` - the blocks then run in that order (fused prologue) and the
    rows gain a fourth entry, the largest difference of the dense block's attention output to its raster run."""
    torch.manual_seed(seed)
    dim, grid = heads * 128, (frames, height, width)
    S = frames * height * width
    order = None
    if bricks is not None:
        assert not fp8, "--brick-order runs the bf16 block"
        fused_prep, order = True, brick_order(grid, bricks, device=device)
    kw = dict(fp8=fp8, fp8_mode=fp8_mode, fp8_margin=fp8_margin, smooth_k=smooth_k, smooth_v=smooth_v, v_tiles=v_tiles,
              fp8_oproj=fp8_oproj)
    sparse = WanLikeSelfAttention(dim, heads, threshold=threshold, fused_prep=fused_prep, **kw).to(device)
    # random q and k projections give unstructured scores (nothing to skip); tie them, as a stand-in for trained weights
    # under which tokens of the same frame attend to each other
    sparse.k.load_state_dict(sparse.q.state_dict())
    dense = WanLikeSelfAttention(dim, heads, enable_skipping=False, fused_prep=fused_prep, **kw).to(device)
    dense.load_state_dict(sparse.state_dict())
    dense.keep_last = order is not None
    # a latent with frame-to-frame structure, denoised over `steps` steps (noise level 0.5 -> 0.05)
    base = torch.randn(1, frames, 1, dim, device=device).expand(1, frames, height * width, dim).reshape(1, S, dim) * 2.0
    base = base + 0.5 * torch.randn(1, S, dim, device=device)
    rows = []
    with torch.no_grad():
        for t in range(steps):
            sigma = 0.5 + (0.05 - 0.5) * t / max(1, steps - 1)
            x = (1 - sigma ** 2) ** 0.5 * base + sigma * torch.randn(1, S, dim, device=device)
            if order is not None:
                # the model boundary: the hidden states (bf16 here, so that the gather is an exact copy) go into the order ONCE ...
                x = x.bfloat16()
                xo = order.gather(x.view(1, S, heads, 128)).view(1, S, dim).float()
                y, y_ref = sparse(xo, grid, order), dense(xo, grid, order)
                o_bricks = order.restore(dense.last[3])             # ... and come back at the exit (here: the attention output)
                dense(x.float(), grid)                              # the same block on the same tokens in raster order
                q, k, v, o_raster = dense.last
                diff, tol = (o_bricks.float() - o_raster.float()).abs().max().item(), attention_tolerance(q, k, v)
            else:
                y, y_ref = sparse(x, grid), dense(x, grid)
            skipped = sparse.lite_attention.get_skip_fraction(batch=1)
            err = (y - y_ref).abs().max().item() / y_ref.abs().max().item()
            rows.append((t, skipped, err) if order is None else (t, skipped, err, diff))
            if verbose:
                print(f"step {t}: tiles skipped by the NEXT step {skipped:6.1%}   max rel. error vs dense block {err:.2e}")
                if fp8_oproj:
                    print(f"step {t}: fp8 output projection ({dense.oproj_how}): max rel. error vs the bf16 path {dense.oproj_error:.2e}")
                if order is not None:
                    print(f"step {t}: brick order {order.bricks}: max abs difference to the raster run {diff:.3e} (tolerance {tol:.3e})")
    return rows


def attention_tolerance(q, k, v):
    """The reference's acceptance rule for an attention output (its tests/test_flash_attn.py): twice the error of the same attention in
    torch bf16 against torch fp32, plus twice the fp32 roundoff at the magnitude of the output."""
    scale = q.shape[-1] ** -0.5
    ref = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q.float(), k.float()) * scale, -1), v.float())
    low = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k).float() * scale, -1).to(v.dtype), v)
    return 2 * (low.float() - ref).abs().max().item() + 2 * (ref + 0.3 - 0.3 - ref).abs().max().item()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    for name, default in (("frames", 5), ("height", 16), ("width", 16), ("heads", 4), ("steps", 6)):
        ap.add_argument(f"--{name}", type=int, default=default)
    ap.add_argument("--threshold", type=float, default=-6.0)
    ap.add_argument("--fused-prep", action="store_true", help="norm + rope + cast of q and k in one pass each (qk_prep)")
    ap.add_argument("--fp8", action="store_true", help="q, k and v in e4m3 with per-head scales (qk_prep_fp8 through E4m3Scales)")
    ap.add_argument("--fp8-mode", choices=("current", "delayed"), default="current")
    ap.add_argument("--fp8-margin", type=float, default=1.0)
    ap.add_argument("--smooth-k", action="store_true", help="with --fp8: subtract each key head's mean before the e4m3 cast (SmoothedQK)")
    ap.add_argument("--smooth-v", action="store_true", help="with --fp8: subtract each V head's mean before the e4m3 cast (SmoothedV); "
                    "the attention call adds it back and returns fp32")
    ap.add_argument("--v-tiles", action="store_true", help="with --fp8: quantize V straight into the V^T tiles the e4m3 forward stages "
                    "(v_prep_tiles through E4m3Scales / SmoothedV with tiles=True): no e4m3 V tensor, no prepare pass in the call")
    ap.add_argument("--fp8-oproj", action="store_true", help="with --fp8: the attention output restored and row-scaled to e4m3 in one "
                    "pass (attn_out_fp8) and the output projection on it, its weight quantized per output channel in torch")
    ap.add_argument("--brick-order", nargs="*", metavar="BT,BH,BW", default=None, help="run the block on the tokens in brick order "
                    "(brick levels, outermost first; none given: 1,16,16 1,8,8): gather once on entry, positions= in the fused prologue, "
                    "restore at the exit; prints the difference to the raster run")
    a = ap.parse_args()
    bricks = None
    if a.brick_order is not None:
        if a.fp8:
            ap.error("--brick-order runs the bf16 block (the e4m3 forms take positions= alike: INTEGRATION.md 1h)")
        bricks = tuple(tuple(int(v) for v in level.split(",")) for level in a.brick_order) or ((1, 16, 16), (1, 8, 8))
    if (a.smooth_k or a.smooth_v or a.v_tiles or a.fp8_oproj) and not a.fp8:
        ap.error("--smooth-k, --smooth-v, --v-tiles and --fp8-oproj need --fp8")
    run(a.frames, a.height, a.width, a.heads, a.steps, a.threshold, fused_prep=a.fused_prep, fp8=a.fp8, fp8_mode=a.fp8_mode,
        fp8_margin=a.fp8_margin, smooth_k=a.smooth_k, smooth_v=a.smooth_v, v_tiles=a.v_tiles, bricks=bricks,
        fp8_oproj=a.fp8_oproj)
