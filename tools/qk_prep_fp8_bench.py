#!/usr/bin/env python
"""The e4m3 prologue at the headline shape, one process, one session: for each of q, k (token RMSNorm + Wan's 3-axis RoPE) and v (no
norm, no rope) of (1, 75 600, 40, 128) on the grid (21, 45, 80), bf16 and fp32 input:
  * the amax pass (`qk_prep_amax`), the quantizing pass (`qk_prep_fp8` with a descale, collecting the amax) and both together with
    `descale_from_amax` between them (current scaling);
  * `qk_prep` to bf16 on the same tensor (`la_qk_prep`: by bytes the quantizing pass moves 3/4 of it from bf16, 5/6 from fp32);
  * the eager recipe: `qk_prep` to bf16, per-head `amax`, scale, `clamp`, `.to(float8_e4m3fn)`;
  * the e4m3 attention call the three tensors feed (dense, per-head descales).
HIP events, 3 warm-up + 20 timed launches, median (min, max). Writes `profiles/qk_prep_fp8.json` and `profiles/qk_prep_fp8.md`.

    python tools/qk_prep_fp8_bench.py [--grid 21 45 80 --heads 40 --head-dim 128] [--out profiles/qk_prep_fp8]
"""
import argparse
import json
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
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--no-attention", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qk_prep_fp8"), help="path without extension: .json and .md are written")
a = ap.parse_args()
dev = torch.device("cuda", 0)
grid = tuple(a.grid)
S, H, D = grid[0] * grid[1] * grid[2], a.heads, a.head_dim
shape = (1, S, H, D)
F8 = torch.float8_e4m3fn


def timed(fn):
    for _ in range(a.warmup):
        fn()
    times = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"ms": round(statistics.median(times), 4), "ms_min_max": [round(min(times), 4), round(max(times), 4)]}


def with_bytes(t, nbytes):
    t["bytes"], t["TBps"] = nbytes, round(nbytes / t["ms"] / 1e9, 3)
    return t


g = torch.Generator(device=dev).manual_seed(0)
weight = 0.5 + torch.rand(H * D, device=dev, generator=g)
tables = L.rope_tables(grid, D, device=dev)
res = {"shape": list(shape), "grid": list(grid), "timing": f"HIP events, {a.warmup} warm-up + {a.iters} timed, median (min, max)",
       "device": torch.cuda.get_device_name(0), "build": L._cabi.build_info().get("src"), "cases": {}}
outs = {}
for tensor in ("q", "k", "v"):
    x32 = torch.randn(shape, device=dev, generator=g) * 2.0
    args = (weight, 1e-6, tables, "token") if tensor != "v" else (None, 1e-6, None, None)
    for in_name, x in (("bf16", x32.bfloat16()), ("fp32", x32)):
        amax, descale = torch.zeros(1, H, device=dev), torch.ones(1, H, device=dev)
        out8, out16 = torch.empty(shape, dtype=F8, device=dev), torch.empty(shape, dtype=torch.bfloat16, device=dev)
        n_in, n = x.numel() * x.element_size(), x.numel()

        def amax_pass():
            amax.zero_()
            L.qk_prep_amax(x, *args, amax_out=amax)

        def quant_pass():
            L.qk_prep_fp8(x, *args, descale=descale, amax_out=amax, out=out8)

        def current():
            amax_pass()
            L.descale_from_amax(amax, out=descale)
            L.qk_prep_fp8(x, *args, descale=descale, out=out8)

        def eager():
            y = L.qk_prep(x, *args, out=out16)
            d = y.float().abs().amax(dim=(1, 3)).clamp_min(2.0 ** -100) / 448.0
            return (y.float() / d[:, None, :, None]).clamp(-448, 448).to(F8), d

        case = {"amax_pass": with_bytes(timed(amax_pass), n_in),
                "quantizing_pass": with_bytes(timed(quant_pass), n_in + n),
                "current_scaling": with_bytes(timed(current), 2 * n_in + n),
                "la_qk_prep_to_bf16": with_bytes(timed(lambda: L.qk_prep(x, *args, out=out16)), n_in + 2 * n)}
        try:
            case["eager_recipe"] = timed(eager)
            e8, ed = eager()
            current()
            case["eager_recipe"]["bytes_differing_from_current_scaling"] = (e8.view(torch.uint8) != out8.view(torch.uint8)).sum().item()
            del e8, ed
        except torch.cuda.OutOfMemoryError as exc:
            case["eager_recipe"] = {"error": f"out of memory: {exc}"}
        q_ms, b_ms = case["quantizing_pass"]["ms"], case["la_qk_prep_to_bf16"]["ms"]
        case["quantizing_over_la_qk_prep"] = round(q_ms / b_ms, 3)
        case["bytes_ratio"] = round((n_in + n) / (n_in + 2 * n), 3)
        res["cases"][f"{tensor}_{in_name}"] = case
        print(tensor, in_name, json.dumps(case), flush=True)
        if in_name == "bf16":
            current()
            outs[tensor] = (out8, descale)
        torch.cuda.empty_cache()

if not a.no_attention:
    (q8, dq), (k8, dk), (v8, dv) = outs["q"], outs["k"], outs["v"]
    att = L.LiteAttention(enable_skipping=False, max_batch_size=1)
    res["e4m3_attention_dense"] = timed(lambda: att(q8, k8, v8, q_descale=dq, k_descale=dk, v_descale=dv))
    print("attention", json.dumps(res["e4m3_attention_dense"]), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out + ".json", "w") as fh:
    json.dump(res, fh, indent=1)

lines = ["# The e4m3 prologue in one pass: `la_qk_prep_fp8`", "",
         f"Written by `tools/qk_prep_fp8_bench.py` on {res['device']} (library src {res['build']}), one process: {tuple(shape)} on the grid "
         f"{grid}, q and k with a token RMSNorm and Wan's 3-axis RoPE, v with neither. {res['timing']}. TB/s = bytes read once + bytes "
         "written once over the median.", "",
         "| tensor, input | amax pass ms (TB/s) | quantizing pass ms (TB/s) | both + descale (current scaling) ms | `la_qk_prep` to bf16 ms (TB/s) "
         "| quantizing / `la_qk_prep` (bytes ratio) | eager recipe ms |", "|---|---|---|---|---|---|---|"]
slower = []
for name, c in res["cases"].items():
    lines.append(f"| {name.replace('_', ', ')} | {c['amax_pass']['ms']} ({c['amax_pass']['TBps']}) | {c['quantizing_pass']['ms']} "
                 f"({c['quantizing_pass']['TBps']}) | {c['current_scaling']['ms']} | {c['la_qk_prep_to_bf16']['ms']} "
                 f"({c['la_qk_prep_to_bf16']['TBps']}) | {c['quantizing_over_la_qk_prep']} ({c['bytes_ratio']}) | "
                 f"{c['eager_recipe'].get('ms', 'out of memory')} |")
    if c["quantizing_over_la_qk_prep"] > 1.0:
        slower.append(name)
lines += ["", "The quantizing pass is " + ("at least as fast as `la_qk_prep` on the same input in every case." if not slower else
                                           "SLOWER than `la_qk_prep` on the same input for: " + ", ".join(slower) + " (see below).")]
if "e4m3_attention_dense" in res:
    t = res["e4m3_attention_dense"]["ms"]
    cur = sum(res["cases"][f"{n}_bf16"]["current_scaling"]["ms"] for n in "qkv")
    dly = sum(res["cases"][f"{n}_bf16"]["quantizing_pass"]["ms"] for n in "qkv")
    egr = sum(res["cases"][f"{n}_bf16"]["eager_recipe"].get("ms", float("nan")) for n in "qkv")
    lines += ["", f"The dense e4m3 attention call these feed: {t} ms. q + k + v from bf16: current scaling {cur:.3f} ms ({cur / t:.1%} of it), "
              f"delayed scaling (the quantizing pass alone) {dly:.3f} ms ({dly / t:.1%}), the eager recipe {egr:.3f} ms ({egr / t:.1%})."]
with open(a.out + ".md", "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", a.out + ".json", a.out + ".md")
