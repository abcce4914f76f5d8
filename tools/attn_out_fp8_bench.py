#!/usr/bin/env python
"""`attn_out_fp8` (`la_attn_unshift_fp8`) at the headline shape, one process: O of (1, 75 600, 40, 128) bf16 with a V shift, the LSE
and the K-smoothing row dots. Four candidates on the same inputs, one call of each per iteration in turn, HIP events around each:

  * the pass in its dynamic mode (one scale per token) and in its static mode (a given scale, the running amax collected);
  * `attn_unshift` bf16 -> bf16 into a second buffer: what the pass reads, twice what it writes - the criterion: the pass's median
    is to be no more than this call's, with this call's own run-to-run spread of this session as the margin;
  * the unfused composition a caller runs today: `attn_unshift` to bf16, then torch `abs().amax()`, a divide, a clamp and
    `.to(float8_e4m3fn)`.

The set is repeated `--runs` times; per candidate the median over all samples, the medians of the runs and their spread (largest
minus smallest run median over the median) are recorded. The pass's bytes are compared with the emulation of
tests/attn_out_fp8_emulation.py on the first and the last 1024 rows. Writes `<out>.json` and `<out>.md` (default
`profiles/attn_out_fp8`).

    python tools/attn_out_fp8_bench.py [--seqlen 75600 --heads 40 --head-dim 128] [--out profiles/attn_out_fp8] [--render-only]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--seqlen", type=int, default=75600)
ap.add_argument("--heads", type=int, default=40)
ap.add_argument("--head-dim", type=int, default=128)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--render-only", action="store_true", help="write the .md again from the saved .json (no device needed)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_out_fp8"), help="path without extension: .json and .md are written")
a = ap.parse_args()
S, H, D = a.seqlen, a.heads, a.head_dim
F8 = torch.float8_e4m3fn


def measure():
    import attn_out_fp8_emulation as emu
    import liteattention_amd as L
    from liteattention_amd import _cabi
    if not torch.cuda.is_available():
        raise SystemExit("attn_out_fp8_bench.py measures on the GPU: none found (--render-only rewrites the .md from a saved .json)")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    o = torch.randn((1, S, H, D), device=dev, generator=g).bfloat16()
    shift = 4.0 * torch.randn(1, H, D, device=dev, generator=g)
    lse = torch.randn(1, H, S, device=dev, generator=g) * 3.0 + 5.0
    lse[0, :, 100], lse[0, 3, 200] = float("inf"), float("inf")                    # an empty token, an empty head
    dot = torch.randn(1, H, S, device=dev, generator=g)
    scale = D ** -0.5
    out8 = torch.empty((1, S, H, D), dtype=F8, device=dev)
    ds = torch.empty(1, S, 1, device=dev)
    lse_out = torch.empty_like(lse)
    out16 = torch.empty_like(o)
    static_ds = torch.full((1,), 0.08, device=dev)
    amax = torch.zeros(1, device=dev)

    def new_dynamic():
        return L.attn_out_fp8(o, shift, lse=lse, lse_dot=dot, softmax_scale=scale, out=out8, descale_out=ds, lse_out=lse_out)

    def new_static():
        return L.attn_out_fp8(o, shift, lse=lse, lse_dot=dot, softmax_scale=scale, descale=static_ds, amax_out=amax, out=out8, lse_out=lse_out)

    def parent():
        return L.attn_unshift(o, shift, lse=lse, lse_dot=dot, softmax_scale=scale, out=out16, lse_out=lse_out)

    def unfused():
        ob, _ = parent()
        flat = ob.view(1, S, H * D)
        d = flat.abs().amax(dim=-1, keepdim=True).float().clamp_min(2.0 ** -100) / 448.0
        return (flat.float() / d).clamp(-448.0, 448.0).to(F8), d

    cands = {"attn_out_fp8, dynamic (one scale per token)": new_dynamic, "attn_out_fp8, static (given scale, running amax)": new_static,
             "attn_unshift bf16 -> bf16 (the criterion)": parent,
             "unfused: attn_unshift to bf16 + torch amax / div / clamp / cast": unfused}
    o_bytes, lse_bytes = o.numel() * 2, lse.numel() * 4
    nbytes = {"attn_out_fp8, dynamic (one scale per token)": o_bytes + o_bytes // 2 + 3 * lse_bytes + S * 4,
              "attn_out_fp8, static (given scale, running amax)": o_bytes + o_bytes // 2 + 3 * lse_bytes,
              "attn_unshift bf16 -> bf16 (the criterion)": 2 * o_bytes + 3 * lse_bytes}
    for fn in cands.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    samples = {name: [[] for _ in range(a.runs)] for name in cands}
    for run in range(a.runs):
        for _ in range(a.iters):
            for name, fn in cands.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                samples[name][run].append(e0.elapsed_time(e1))
    res = {"shape": [1, S, H, D], "device": torch.cuda.get_device_name(0), "build": _cabi.build_info().get("src"),
           "timing": f"HIP events around each call, the four candidates in turn, {a.warmup} warm-up calls of each, then {a.runs} runs of "
                     f"{a.iters} timed calls of each", "candidates": {}}
    for name, runs in samples.items():
        every = [t for r in runs for t in r]
        med, run_meds = statistics.median(every), [statistics.median(r) for r in runs]
        rec = {"median_ms": round(med, 4), "run_medians_ms": [round(m, 4) for m in run_meds], "min_ms": round(min(every), 4),
               "max_ms": round(max(every), 4), "spread_of_run_medians": round((max(run_meds) - min(run_meds)) / med, 4)}
        if name in nbytes:
            rec["bytes"] = nbytes[name]
            rec["TBps"] = round(nbytes[name] / med / 1e9, 3)
        res["candidates"][name] = rec
        print(name, json.dumps(rec), flush=True)
    c = res["candidates"]
    crit = c["attn_unshift bf16 -> bf16 (the criterion)"]
    for key, name in (("dynamic", "attn_out_fp8, dynamic (one scale per token)"), ("static", "attn_out_fp8, static (given scale, running amax)")):
        ratio = c[name]["median_ms"] / crit["median_ms"]
        res[key + "_over_criterion"] = round(ratio, 4)
        res[key + "_meets_criterion"] = bool(ratio <= 1.0 + crit["spread_of_run_medians"])
        res[key + "_over_unfused"] = round(c[name]["median_ms"] / c["unfused: attn_unshift to bf16 + torch amax / div / clamp / cast"]["median_ms"], 4)
    # the bytes at this size: the first and the last 1024 rows against the emulation (CPU, fp32 step by step)
    r, _ = new_dynamic()
    torch.cuda.synchronize()
    ok = True
    for rows in (slice(0, min(S, 1024)), slice(max(0, S - 1024), S)):
        data, d, _ = emu.emulate(o[:, rows], shift, lse[:, :, rows])
        ok = ok and torch.equal(r.data[:, rows].cpu().view(torch.uint8), data.view(torch.uint8)) and \
            torch.equal(r.descale[:, rows].cpu().view(torch.int32), d.view(torch.int32))
    res["first_and_last_1024_rows_equal_the_emulation"] = bool(ok)
    return res


if a.render_only:
    res = json.load(open(a.out + ".json"))
else:
    res = measure()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

crit = res["candidates"]["attn_unshift bf16 -> bf16 (the criterion)"]
lines = ["# `attn_out_fp8`: O restored and row-scaled to e4m3 in one pass", "",
         f"Written by `tools/attn_out_fp8_bench.py` on {res['device']} (library src {res['build']}), one process: O of {tuple(res['shape'])} "
         f"bf16 with a V shift, the LSE and the row dots. {res['timing']}. Spread = (largest - smallest run median) / median.", "",
         "| candidate | median ms | run medians ms | min .. max ms | spread | algorithmic TB/s |", "|---|---|---|---|---|---|"]
for name, rec in res["candidates"].items():
    lines.append(f"| {name} | {rec['median_ms']} | {', '.join(str(m) for m in rec['run_medians_ms'])} | {rec['min_ms']} .. {rec['max_ms']} | "
                 f"{rec['spread_of_run_medians']} | {rec.get('TBps', '-')} |")
lines += ["", f"Criterion: the pass's median is no more than `attn_unshift` bf16 -> bf16's ({crit['median_ms']} ms), with that call's spread "
          f"of this session ({crit['spread_of_run_medians']}) as the margin. Dynamic mode: {res['dynamic_over_criterion']} of it - "
          f"{'met' if res['dynamic_meets_criterion'] else 'NOT met'}; static mode: {res['static_over_criterion']} - "
          f"{'met' if res['static_meets_criterion'] else 'NOT met'}. Against the unfused composition a caller runs today the dynamic mode "
          f"takes {res['dynamic_over_unfused']} of the time, the static one {res['static_over_unfused']}.", "",
          f"Bytes and descales of the first and the last 1024 rows equal the emulation of `tests/attn_out_fp8_emulation.py`: "
          f"{res['first_and_last_1024_rows_equal_the_emulation']}."]
notes = os.path.join(ROOT, "profiles", "attn_out_fp8_notes.md")        # the interpretation, kept apart from the numbers
if os.path.exists(notes):
    lines += ["", open(notes).read().rstrip()]
with open(a.out + ".json", "w") as fh:
    json.dump(res, fh, indent=1)
with open(a.out + ".md", "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", a.out + ".json", a.out + ".md")
