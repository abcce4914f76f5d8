#!/usr/bin/env python
"""Head rotation in the e4m3 prologue, one process: the quantizing pass and the amax pass of q and k at (1, 75 600, 40, 128) on the grid
(21, 45, 80), bf16 in, e4m3 out, token RMSNorm + Wan's 3-axis RoPE, without and with `rotate=head_rotation(128)`. The two forms are
timed ALTERNATELY, launch by launch, so that whatever else the machine does falls on both: HIP events, 5 warm-up + 30 timed launches of
each, median (min, max). Two A/B libraries join the same loop when they are given (`python -m liteattention_amd.build -D... --out=...`):
`--same-flags-lib` (-DLA_QK_PREP_SAME_FLAGS=1: the UNROTATED kernels under the compile flags of the rotated unit, so that the cost of the
butterflies stands apart from the registers those flags save) and `--lds-lib` (-DLA_QK_ROT_LDS=1: the rotated kernels with the three
low cross-lane stages transposed through LDS instead of DPP + ds_swizzle; its bytes must equal the product's). Then the accuracy table: the rms error of O of the dense e4m3 forward against fp64 attention on the unquantized
operands, (1, 512, 2, D), without and with rotation, on the two inputs of tests/test_gpu_qk_rotate.py. Writes `profiles/qk_rotate.md`.

    python tools/qk_rotate_bench.py [--grid 21 45 80 --heads 40 --head-dim 128] [--same-flags-lib build_variants/qk_same_flags.so]
                                    [--lds-lib build_variants/qk_rot_lds.so] [--out profiles/qk_rotate]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import liteattention_amd as L                                      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, nargs=3, default=[21, 45, 80])
ap.add_argument("--heads", type=int, default=40)
ap.add_argument("--head-dim", type=int, default=128)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--same-flags-lib", default=None)
ap.add_argument("--lds-lib", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qk_rotate"), help="path without extension: .md is written")
a = ap.parse_args()
dev = torch.device("cuda", 0)
grid = tuple(a.grid)
S, H, D = grid[0] * grid[1] * grid[2], a.heads, a.head_dim
shape = (1, S, H, D)


def timed_pair(fns):
    """Median (min, max) ms of each of `fns`, their launches interleaved."""
    for _ in range(a.warmup):
        for fn in fns:
            fn()
    times = [[] for _ in fns]
    for _ in range(a.iters):
        for fn, ts in zip(fns, times):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
    return [(statistics.median(ts), min(ts), max(ts)) for ts in times]


def on(path, fn):
    """`fn` with the prologue entry points of the A/B library at `path` (None: the product's)."""
    if path is None:
        return fn
    lib = ctypes.CDLL(os.path.abspath(path))

    def run():
        saved, L._cabi._lib = L._cabi.load(), lib
        try:
            return fn()
        finally:
            L._cabi._lib = saved
    return run


g = torch.Generator(device=dev).manual_seed(0)
weight = 0.5 + torch.rand(H * D, device=dev, generator=g)
tables = L.rope_tables(grid, D, device=dev)
rot = L.head_rotation(D, device=dev)
FORMS = [("unrotated", None, None), ("unrotated, rotated unit's flags", a.same_flags_lib, None), ("rotated (DPP + ds_swizzle)", None, rot),
         ("rotated, LDS transpose", a.lds_lib, rot)]
FORMS = [f for f in FORMS if f[1] is not None or not f[0].endswith(("flags", "transpose"))]
lines = ["# Head rotation in the e4m3 prologue: `la_qk_prep_fp8_rot`", "",
         f"Written by `tools/qk_rotate_bench.py` on {torch.cuda.get_device_name(0)} (library src {L._cabi.build_info().get('src')}), one "
         f"process. Pass times: {shape} on the grid {grid}, bf16 in, e4m3 out, token RMSNorm + 3-axis RoPE; the forms of a row "
         f"alternate launch by launch, HIP events, {a.warmup} warm-up + {a.iters} timed of each, median (min, max) ms.", "",
         "| tensor, pass | " + " | ".join(f[0] for f in FORMS) + " |", "|---|" + "---|" * len(FORMS)]
notes = []
for tensor in ("q", "k"):
    x = (torch.randn(shape, device=dev, generator=g) * 2.0).bfloat16()
    amax, descale = torch.zeros(1, H, device=dev), torch.ones(1, H, device=dev)
    outs = [torch.empty(shape, dtype=torch.float8_e4m3fn, device=dev) for _ in FORMS]
    args = (x, weight, 1e-6, tables, "token")
    quant = [on(lib, lambda r=r, o=o: L.qk_prep_fp8(*args, descale=descale, amax_out=amax, out=o, rotate=r)) for (_, lib, r), o in zip(FORMS, outs)]
    amaxp = [on(lib, lambda r=r: L.qk_prep_amax(*args, amax_out=amax, rotate=r)) for _, lib, r in FORMS]
    for name, fns in (("quantizing pass", quant), ("amax pass", amaxp)):
        lines.append(f"| {tensor}, {name} | " + " | ".join(f"{m:.4f} ({lo:.4f}, {hi:.4f})" for m, lo, hi in timed_pair(fns)) + " |")
        print(lines[-1], flush=True)
    for (name, _, r), o in zip(FORMS, outs):                     # the LDS form computes the product's bytes: the same additions
        differ = (o.view(torch.uint8) != outs[[f[2] is r for f in FORMS].index(True)].view(torch.uint8)).sum().item()
        assert differ == 0 or r is None, (name, differ)
        notes.append(f"{tensor}, {name}: {differ} of {o.numel()} bytes differ from the product form")
    del x, outs
lines += [""] + [n + "." for n in notes if "product" in n and not n.split(":")[0].endswith(("unrotated", "swizzle)"))] + [
          "(Without the packed forms the compiler contracts other multiply-add pairs of the norm and the rope into FMAs, so the unrotated "
          "bytes may differ in the last code step; the LDS form runs the product's own additions and must not differ.)", "",
          "The rotated unit is compiled without the packed fp32 forms (`_buildinfo.SOURCE_FLAGS`), which costs the butterflies nothing and "
          "saves registers (the headline quantizing form: 279 -> 227 VGPRs, one wave per SIMD -> two); the unrotated product kernels "
          "keep the flags, and the instructions, they had before. The second column is the unrotated pass under the same flags: the "
          "difference between it and the third is what the rotation itself costs."]


def attention_fp64(q, k, v, scale):
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * scale
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), v.double())


lines += ["", "## Accuracy", "",
          "Rms error of O of the dense e4m3 forward against fp64 attention on the unquantized q, k, v: (1, 512, 2, D), softmax_scale "
          "1 / (8 sqrt(D)), q and k from `qk_prep_fp8` (one descale per head, current scaling) without and with `rotate`, V quantized "
          "unrotated in both. Concentrated: N(0, 1) with q += 24, k += 40 in column 5 and q -= 16, k += 30 in column D - 3.", "",
          "| D | input | unrotated | rotated | unrotated / rotated |", "|---|---|---|---|---|"]
for Dh in (128, 64):
    for concentrated in (True, False):
        gc = torch.Generator().manual_seed(Dh)
        q, k, v = (torch.randn(1, 512, 2, Dh, generator=gc) for _ in range(3))
        if concentrated:
            q[..., 5] += 24
            k[..., 5] += 40
            q[..., Dh - 3] -= 16
            k[..., Dh - 3] += 30
        q, k, v = (t.bfloat16().to(dev) for t in (q, k, v))
        scale = 1.0 / (8.0 * Dh ** 0.5)
        o64 = attention_fp64(q, k, v, scale)
        v8, dv = L.E4m3Scales()(v, norm=None)
        errs = []
        for r in (None, L.head_rotation(Dh, device=dev)):
            (q8, dq), (k8, dk) = (L.E4m3Scales()(t, norm=None, rotate=r) for t in (q, k))
            o = L.flash_attn_func(q8, k8, v8, softmax_scale=scale, q_descale=dq, k_descale=dk, v_descale=dv)
            errs.append((o.double() - o64).pow(2).mean().sqrt().item())
        lines.append(f"| {Dh} | {'concentrated' if concentrated else 'N(0, 1)'} | {errs[0]:.3e} | {errs[1]:.3e} | {errs[0] / errs[1]:.2f} |")
        print(lines[-1], flush=True)

lines += ["", "## The cross-lane stages", "",
          "The product: the exchanges with lanes ^1 and ^2 are DPP `quad_perm` operands of the addition itself (`v_add_f32_dpp`, no "
          "instruction of their own), those with ^4, ^8 and ^16 one `ds_swizzle_b32` in bit mode each (the LDS crossbar; no LDS memory); "
          "the sign of \"own\" and the eight signs of `s` are lane masks in scalar registers, applied by one `v_cndmask` with a negated "
          "source each. At head_dim 128: 16 swizzles, 32 DPP additions and 24 in-lane additions per chunk of 8 elements.",
          "The alternative (`-DLA_QK_ROT_LDS=1`, the last column above): the three low lane bits are transposed against the three "
          "register bits through an 8 x 8 tile of the wave's own LDS per group of 8 lanes (two 16-byte writes, eight 4-byte reads, "
          "bank-conflict free, wavefront fences only), their 24 additions run in-lane, and the tile is transposed back; ^8 and ^16 stay "
          "`ds_swizzle`. It moves 128 bytes per lane and chunk through LDS where the product's one swizzle stage it replaces moves 32. "
          "The choice is the faster column of the table above."]
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out + ".md", "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", a.out + ".md")
