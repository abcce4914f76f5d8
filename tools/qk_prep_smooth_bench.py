#!/usr/bin/env python
"""The K-smoothing prologue (`la_qk_prep_smooth`) at the headline shape, one process: k and q of (1, 75 600, 40, 128) on the grid
(21, 45, 80), bf16 in, token RMSNorm + Wan's 3-axis RoPE. Every new pass is timed INTERLEAVED with the plain pass of the same reads and
writes (`qk_prep_amax` / `qk_prep_fp8`): one launch of each per iteration, alternating, HIP events around each launch, medians; the
whole set is run twice and the two ratios of a pair give the session's own run-to-run spread. Beside each measured ratio stands the
one expected from the byte counts: the extra traffic is n_parts B H D 4 bytes written for the part sums, B H D 4 read for a shift or a
dot vector, B H S 4 written for the row dots. Then `SmoothedQK.pair` against two `E4m3Scales` in both modes, the finish kernel alone,
and the end-to-end error of the dense e4m3 attention call with and without smoothing on the input of tests/test_gpu_qk_prep_smooth.py.
Writes `profiles/qk_prep_smooth.json` and `profiles/qk_prep_smooth.md`.

    python tools/qk_prep_smooth_bench.py [--grid 21 45 80 --heads 40 --head-dim 128] [--out profiles/qk_prep_smooth] [--render-only]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, nargs=3, default=[21, 45, 80])
ap.add_argument("--heads", type=int, default=40)
ap.add_argument("--head-dim", type=int, default=128)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--render-only", action="store_true", help="write the .md again from the saved .json (no device needed)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qk_prep_smooth"), help="path without extension: .json and .md are written")
a = ap.parse_args()
grid = tuple(a.grid)
S, H, D = grid[0] * grid[1] * grid[2], a.heads, a.head_dim
shape = (1, S, H, D)
F8 = torch.float8_e4m3fn


def measure():
    import liteattention_amd as L
    dev = torch.device("cuda", 0)

    def interleaved(new, plain):
        """Medians (ms) of `new` and `plain`, one launch of each per iteration, alternating."""
        for _ in range(a.warmup):
            new()
            plain()
        times = ([], [])
        for _ in range(a.iters):
            for fn, acc in ((new, times[0]), (plain, times[1])):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                acc.append(e0.elapsed_time(e1))
        return statistics.median(times[0]), statistics.median(times[1])

    g = torch.Generator(device=dev).manual_seed(0)
    weight = 0.5 + torch.rand(H * D, device=dev, generator=g)
    tables = L.rope_tables(grid, D, device=dev)
    args = (weight, 1e-6, tables, "token")
    xk = (torch.randn(shape, device=dev, generator=g) * 2.0).bfloat16()
    xq = (torch.randn(shape, device=dev, generator=g) * 2.0).bfloat16()
    n_parts, part_rows = L.qk_prep_smooth_parts(S, H, D)
    part = torch.empty(n_parts, 1, H, D, device=dev)
    mean = L.qk_prep_colmean(xk, *args, colsum_part=part)
    amax, descale = torch.zeros(1, H, device=dev), torch.ones(1, H, device=dev)
    L.qk_prep_amax(xk, *args, amax_out=amax)
    L.descale_from_amax(amax, 1.25, out=descale)                       # headroom: the timed passes quantize the same tensor
    out8, dots = torch.empty(shape, dtype=F8, device=dev), torch.empty(1, H, S, device=dev)
    n_in, n = xk.numel() * 2, xk.numel()
    vec, part_bytes, dot_bytes = H * D * 4, n_parts * H * D * 4, H * S * 4

    pairs = {      # name: (new pass, plain pass, bytes of the plain pass, extra bytes of the new one)
        "k sums-only pass vs qk_prep_amax": (
            lambda: L.qk_prep_smooth(xk, *args, colsum_part=part, quantize=False),
            lambda: L.qk_prep_amax(xk, *args, amax_out=amax), n_in, part_bytes),
        "k amax pass with shift vs qk_prep_amax": (
            lambda: L.qk_prep_smooth(xk, *args, shift=mean, amax_out=amax, quantize=False),
            lambda: L.qk_prep_amax(xk, *args, amax_out=amax), n_in, vec),
        "k quantizing pass with shift vs qk_prep_fp8": (
            lambda: L.qk_prep_smooth(xk, *args, shift=mean, descale=descale, out=out8),
            lambda: L.qk_prep_fp8(xk, *args, descale=descale, out=out8), n_in + n, vec),
        "k delayed pass (shift + amax + sums) vs qk_prep_fp8 with amax": (
            lambda: L.qk_prep_smooth(xk, *args, shift=mean, descale=descale, amax_out=amax, colsum_part=part, out=out8),
            lambda: L.qk_prep_fp8(xk, *args, descale=descale, amax_out=amax, out=out8), n_in + n, vec + part_bytes),
        "q quantizing pass with dots vs qk_prep_fp8": (
            lambda: L.qk_prep_smooth(xq, *args, descale=descale, dot_vec=mean, dot_out=dots, out=out8),
            lambda: L.qk_prep_fp8(xq, *args, descale=descale, out=out8), n_in + n, vec + dot_bytes),
        "q delayed pass (amax + dots) vs qk_prep_fp8 with amax": (
            lambda: L.qk_prep_smooth(xq, *args, descale=descale, amax_out=amax, dot_vec=mean, dot_out=dots, out=out8),
            lambda: L.qk_prep_fp8(xq, *args, descale=descale, amax_out=amax, out=out8), n_in + n, vec + dot_bytes),
    }
    res = {"shape": list(shape), "grid": list(grid), "n_parts": n_parts, "rows_per_part": part_rows,
           "bytes": {"vector": vec, "part_sums": part_bytes, "row_dots": dot_bytes},
           "timing": f"HIP events around single launches, new and plain pass alternating, {a.warmup} warm-up + {a.iters} timed of each, medians; "
                     "the whole set twice (run 1, run 2)",
           "device": torch.cuda.get_device_name(0), "build": L._cabi.build_info().get("src"), "passes": {}}
    for name in pairs:
        res["passes"][name] = {"runs": []}
    for run in range(2):
        for name, (new, plain, base, extra) in pairs.items():
            t_new, t_plain = interleaved(new, plain)
            rec = res["passes"][name]
            rec["runs"].append({"new_ms": round(t_new, 4), "plain_ms": round(t_plain, 4), "ratio": round(t_new / t_plain, 4)})
            rec["plain_bytes"], rec["extra_bytes"], rec["expected_ratio"] = base, extra, round((base + extra) / base, 4)
            print(run, name, json.dumps(rec["runs"][-1]), "expected", rec["expected_ratio"], flush=True)

    # the finish kernel alone, and whole pairs: SmoothedQK against two E4m3Scales
    t_fin, _ = interleaved(lambda: L.colsum_finish(part, S, out=mean), lambda: None)
    res["colsum_finish_ms"] = round(t_fin, 4)
    for mode in ("current", "delayed"):
        sm, sq, sk = L.SmoothedQK(mode=mode, margin=1.25), L.E4m3Scales(mode=mode, margin=1.25), L.E4m3Scales(mode=mode, margin=1.25)
        sm.pair(xq, xk, weight, weight, 1e-6, tables)                  # first calls: allocation, history
        sq(xq, *args)
        sk(xk, *args)

        def plain_pair():
            sq(xq, *args)
            sk(xk, *args)

        t_new, t_plain = interleaved(lambda: sm.pair(xq, xk, weight, weight, 1e-6, tables), plain_pair)
        res[f"pair_{mode}"] = {"smoothed_ms": round(t_new, 4), "e4m3scales_ms": round(t_plain, 4), "ratio": round(t_new / t_plain, 4)}
        print(mode, json.dumps(res[f"pair_{mode}"]), flush=True)
        del sm, sq, sk
        torch.cuda.empty_cache()

    # the error end to end: B = 1, S = 320, H = 2, D = 128, +-offset on 8 channels of every key head (tests/test_gpu_qk_prep_smooth.py)
    def offset_vector(heads, dim, size, seed):
        gg = torch.Generator().manual_seed(seed)
        c = torch.zeros(heads, dim)
        for h in range(heads):
            idx = torch.randperm(dim, generator=gg)[:8]
            c[h, idx] = size * (2.0 * torch.randint(0, 2, (8,), generator=gg) - 1.0)
        return c

    def rel_rms(got, ref):
        return ((got.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()

    res["dense_attention_error"] = {}
    for offset in (0, 8, 16):
        gg = torch.Generator().manual_seed(0)
        q, k, v = (torch.randn(1, 320, 2, 128, generator=gg) for _ in range(3))
        k = k + offset_vector(2, 128, float(offset), 1)[None, None]
        q, k, v = (t.bfloat16().to(dev) for t in (q, k, v))
        s64 = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * 128 ** -0.5
        o64, lse64 = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s64, -1), v.double()), torch.logsumexp(s64, -1)
        v8, dv = L.E4m3Scales()(v, norm=None)
        q8, dq = L.E4m3Scales()(q, norm=None)
        k8, dk = L.E4m3Scales()(k, norm=None)
        o_p, lse_p = L.flash_attn_func(q8, k8, v8, q_descale=dq, k_descale=dk, v_descale=dv, return_softmax_lse=True)
        sq8, sk8, sdq, sdk, shift = L.SmoothedQK().pair(q, k, norm=None)
        o_s, lse_s = L.flash_attn_func(sq8, sk8, v8, q_descale=sdq, k_descale=sdk, v_descale=dv, return_softmax_lse=True)
        rec = {"o_rel_rms_plain": round(rel_rms(o_p, o64), 5), "o_rel_rms_smoothed": round(rel_rms(o_s, o64), 5),
               "lse_max_err_plain": round((lse_p.double() - lse64).abs().max().item(), 5),
               "lse_max_err_smoothed_uncorrected": round((lse_s.double() - lse64).abs().max().item(), 5),
               "lse_max_err_after_lse_unshift": round((L.lse_unshift(lse_s, shift, 128 ** -0.5).double() - lse64).abs().max().item(), 5)}
        rec["o_ratio"] = round(rec["o_rel_rms_smoothed"] / rec["o_rel_rms_plain"], 4)
        res["dense_attention_error"][str(offset)] = rec
        print("offset", offset, json.dumps(rec), flush=True)

    return res


if a.render_only:                                                  # the tables again from a saved run: no device needed
    res = json.load(open(a.out + ".json"))
else:
    res = measure()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
n_parts, part_rows = res["n_parts"], res["rows_per_part"]
vec, part_bytes, dot_bytes = res["bytes"]["vector"], res["bytes"]["part_sums"], res["bytes"]["row_dots"]
shape, grid = tuple(res["shape"]), tuple(res["grid"])

lines = ["# K smoothing in the prologue: `la_qk_prep_smooth`", "",
         f"Written by `tools/qk_prep_smooth_bench.py` on {res['device']} (library src {res['build']}), one process: {tuple(shape)} on the "
         f"grid {grid}, bf16 in, token RMSNorm + Wan's 3-axis RoPE; {n_parts} parts of {part_rows} rows. {res['timing']}.", "",
         "Expected ratio = (bytes of the plain pass + extra bytes) / bytes of the plain pass; extra = the part sums written "
         f"({part_bytes} B), a shift or dot vector read ({vec} B), the row dots written ({dot_bytes} B).", "",
         "| new pass vs plain pass | plain ms (run 1, run 2) | new ms (run 1, run 2) | measured ratio (run 1, run 2) | expected ratio | "
         "excess over expected beyond the spread |", "|---|---|---|---|---|---|"]
for name, rec in res["passes"].items():
    r1, r2 = rec["runs"]
    spread = abs(r1["ratio"] - r2["ratio"])
    excess = max(r1["ratio"], r2["ratio"]) - rec["expected_ratio"] - spread
    rec["spread"], rec["excess"] = round(spread, 4), round(excess, 4)
    lines.append(f"| {name} | {r1['plain_ms']}, {r2['plain_ms']} | {r1['new_ms']}, {r2['new_ms']} | {r1['ratio']}, {r2['ratio']} | "
                 f"{rec['expected_ratio']} | {'none' if excess <= 0 else f'{excess:.3f}'} |")
c, d = res["pair_current"], res["pair_delayed"]
lines += ["", f"`la_colsum_finish` alone: {res['colsum_finish_ms']} ms. `SmoothedQK.pair` (q and k) against two `E4m3Scales` calls, same "
          f"interleaving: current {c['smoothed_ms']} vs {c['e4m3scales_ms']} ms (ratio {c['ratio']}; 5 reads of a tensor against 4), delayed "
          f"{d['smoothed_ms']} vs {d['e4m3scales_ms']} ms (ratio {d['ratio']}; 2 reads against 2, plus the finish kernel and torch's small ops).",
          "", "## Error of the dense e4m3 attention call, against fp64 attention of the same bf16 inputs", "",
          "B = 1, S = 320, H = 2, D = 128, +-offset on 8 channels of every key head (the input of tests/test_gpu_qk_prep_smooth.py): "
          "relative rms error of O, largest |LSE error|.", "",
          "| offset | O plain (`E4m3Scales`) | O smoothed (`SmoothedQK`) | ratio | LSE plain | LSE smoothed, uncorrected | LSE after `lse_unshift` |",
          "|---|---|---|---|---|---|---|"]
for off, rec in res["dense_attention_error"].items():
    lines.append(f"| {off} | {rec['o_rel_rms_plain']} | {rec['o_rel_rms_smoothed']} | {rec['o_ratio']} | {rec['lse_max_err_plain']} | "
                 f"{rec['lse_max_err_smoothed_uncorrected']} | {rec['lse_max_err_after_lse_unshift']} |")
resources = os.path.join(ROOT, "profiles", "qk_prep_smooth_resources.json")
if os.path.exists(resources):
    kern = json.load(open(resources))
    lines += ["", "## Resource usage (the compiler's kernel-resource-usage remark)", "", kern["source"] + ".", "",
              "| kernel | VGPRs | AGPRs | scratch B/lane | static LDS B | waves/SIMD |", "|---|---|---|---|---|---|"]
    for name, r in kern["kernels"].items():
        if "bf16" in name:
            lines.append(f"| {name} | {r['vgprs']} | {r['agprs']} | {r['scratch_bytes_per_lane']} | {r['static_lds_bytes']} | "
                         f"{r['occupancy_waves_per_simd']} |")
notes = os.path.join(ROOT, "profiles", "qk_prep_smooth_notes.md")      # the interpretation, kept apart from the numbers
if os.path.exists(notes):
    lines += ["", open(notes).read().rstrip()]
with open(a.out + ".json", "w") as fh:
    json.dump(res, fh, indent=1)
with open(a.out + ".md", "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", a.out + ".json", a.out + ".md")
