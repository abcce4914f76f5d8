#!/usr/bin/env python
"""la_vote_margins beside la_fwd, and calibrate_skip_schedule beside calibrate_threshold, in one process -> profiles/vote_margins.md.

(1) Headline shape (1, 75 600, 40, 128, bf16), dense and under an imposed banded list (default 42 % sparsity): device-event time of one
margin pass and of one la_fwd call over the SAME walk, alternated, `--reps` timed calls each after warm-up; median, min - max spread and
the ratio of the medians. Operations from shapes: the pass does 2 S_q S_k D H per listed tile pair (Q K^T), the forward twice that.
(2) `--steps` steps of tools.selfcheck.DenoiseWorkload: wall time (host clock around work that ends in a synchronise) of
calibrate_skip_schedule (one margin pass + one forward per step) and of calibrate_threshold at its default iters, and their forward calls.
    python tools/vote_margins_bench.py [--reps 6] [--steps 3] [--sparsity 0.42] [--out profiles/vote_margins.md]
`--fp8` -> profiles/vote_margins_fp8.md: the same shape in e4m3 with per-head descales. Three calls over the SAME walk, alternated: the
la_vote_margins_fp8 pass; what a caller without it runs - q and k up-converted to bf16 in torch, then la_vote_margins, the conversion inside
the timing; and the e4m3 la_fwd. Then registers, LDS and resident workgroups of every instantiation of the new kernel, from a compile
of its source with the build's flags (`-Rpass-analysis=kernel-resource-usage`; no device involved)."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import liteattention_amd as L                                    # noqa: E402
from liteattention_amd.calibration import calibrate_skip_schedule, calibrate_threshold      # noqa: E402
from tools.selfcheck import DenoiseWorkload, banded_rows, executed_flops, impose_lists      # noqa: E402


def timed_pair(fns, reps):
    """Device-event milliseconds of each function, alternated call by call after two warm-up rounds."""
    for _ in range(2):
        for fn in fns:
            fn()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return ms


def row(name, ms, flops):
    med = statistics.median(ms)
    return f"| {name} | {med:.2f} | {min(ms):.2f} - {max(ms):.2f} | {flops / med / 1e9:.0f} |", med


def resource_rows(k_tiles):
    """Per head dim of la_vote_margins_fp8.hip: VGPRs, scratch, the dynamic LDS of a walk of `k_tiles` (vote_margins_fp8_lds_bytes) and the
    workgroups a compute unit holds (four waves per workgroup, one per SIMD: waves per SIMD by registers, 160 KiB by LDS)."""
    from liteattention_amd.build import CSRC, INCLUDE, _hipcc
    src = os.path.join(CSRC, "la_vote_margins_fp8.hip")
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", INCLUDE, "-I", CSRC, "-c", src, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    rows = []
    for m in re.finditer(r"fp8_kernelILi(\d+)ELi(\d)E.*?VGPRs: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?VGPRs Spill: (\d+)", r.stderr, flags=re.S):
        D, nq, vgpr, occ, spill = (int(x) for x in m.groups())
        lds = 2 * 64 * ((D + 63) // 64 * 64 + 16) + 64 + 4 * ((k_tiles + 3) & ~3) + 8 * ((k_tiles + 31) // 32)
        rows.append(f"| {D} | {128 * nq} x 64 | {8 * nq * ((D + 63) // 64)} | {vgpr} | {spill} | {lds} | {min(occ, 160 * 1024 // lds)} |")
    return rows


def main_fp8(a):
    """la_vote_margins_fp8 beside the up-convert route and the e4m3 la_fwd -> a.out."""
    dev, S, H, D, F8 = torch.device("cuda"), a.seqlen, a.heads, 128, torch.float8_e4m3fn
    g = torch.Generator(device=dev).manual_seed(1234)
    q, k, v = [torch.randn(1, S, H, D, device=dev, generator=g).to(F8) for _ in range(3)]
    ds = dict(zip(("q_descale", "k_descale", "v_descale"), (0.5 + 1.5 * torch.rand(3, 1, H, device=dev, generator=g)).unbind(0)))
    qk_ds = {n: d for n, d in ds.items() if n != "v_descale"}
    bm, bn = L.get_tile_sizes(D, 1)
    qt, kt = -(-S // bm), -(-S // bn)
    lines = ["# la_vote_margins_fp8 beside the up-convert route and the e4m3 la_fwd", "",
             f"`tools/vote_margins_bench.py --fp8 --reps {a.reps} --sparsity {a.sparsity}` on {torch.cuda.get_device_name()}; shape (1, {S}, {H}, "
             f"{D}) e4m3 with descales per head, q-tile {bm} x {bn}. Device events around single calls, the three calls alternated, {a.reps} "
             "timed calls each after 2 warm-up rounds. `bf16 route`: `q.bfloat16()`, `k.bfloat16()` (two new tensors) and la_vote_margins, "
             "all inside the events - the descales then go into `softmax_scale` per head, which one call cannot do: the route is timed, "
             "not its result. TFLOP/s: operations from shapes over the median (the pass: half the forward's).", "",
             "| walk | call | median ms | min - max ms | TFLOP/s |", "|---|---|---|---|---|"]
    att = L.LiteAttention(threshold=-10.0, max_batch_size=1)
    att.threshold = float("-inf")                                 # the forward flags nothing: the imposed list is a fixed point
    att._get_read_write_lists(q, k)
    att._phase = 0
    ratios = []
    for name, s_ in (("dense", 0.0), (f"imposed {a.sparsity:.0%}", a.sparsity)):
        rows = banded_rows(qt, kt, bm, bn, s_)
        impose_lists(att, rows)
        fwd_flops = executed_flops(rows, H, 1, S, S, bm, bn, D)
        walk = None if s_ == 0.0 else att.current_read_list()
        fwd = (lambda: L.flash_attn_func(q, k, v, **ds)) if s_ == 0.0 else (lambda: att(q, k, v, **ds))
        ms = timed_pair([lambda: L.vote_margins(q, k, read_list=walk, **qk_ds),
                         lambda: L.vote_margins(q.bfloat16(), k.bfloat16(), read_list=walk, flags=0), fwd], a.reps)
        meds = []
        for call, m, fl in zip(("la_vote_margins_fp8", "bf16 route", "la_fwd e4m3"), ms, (fwd_flops / 2, fwd_flops / 2, fwd_flops)):
            line, med = row(call, m, fl)
            lines.append(f"| {name} " + line)
            meds.append(med)
        ratios.append(f"{name}: pass / la_fwd **{meds[0] / meds[2]:.3f}**, pass / bf16 route **{meds[0] / meds[1]:.3f}**")
    lines += ["", "Ratios of medians - " + "; ".join(ratios) + ".", "",
              f"## Resources of la_vote_margins_fp8_kernel (compile for gfx950; LDS for the {kt} key tiles of this shape)", "",
              "| head_dim | q-tile | Q registers | VGPRs | spilled | LDS bytes | workgroups / CU |", "|---|---|---|---|---|---|---|"] + resource_rows(kt) + [""]
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--sparsity", type=float, default=0.42)
    ap.add_argument("--seqlen", type=int, default=75600)
    ap.add_argument("--heads", type=int, default=40)
    ap.add_argument("--fp8", action="store_true", help="the e4m3 pass beside the up-convert route and the e4m3 forward")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "vote_margins_fp8.md" if a.fp8 else "vote_margins.md")
    if not torch.cuda.is_available():
        sys.exit("vote_margins_bench needs a GPU: nothing here is measured on a CPU")
    if a.fp8:
        return main_fp8(a)
    dev, S, H, D = torch.device("cuda"), a.seqlen, a.heads, 128
    g = torch.Generator(device=dev).manual_seed(1234)
    q, k, v = [torch.randn(1, S, H, D, device=dev, generator=g).bfloat16() for _ in range(3)]
    bm, bn = L.get_tile_sizes(D, 2)
    qt, kt = -(-S // bm), -(-S // bn)
    lines = ["# la_vote_margins beside la_fwd", "",
             f"`tools/vote_margins_bench.py --reps {a.reps} --steps {a.steps} --sparsity {a.sparsity}` on {torch.cuda.get_device_name()}; "
             f"shape (1, {S}, {H}, {D}) bf16, q-tile {bm} x {bn}. Device events around single calls, the two kernels alternated, "
             f"{a.reps} timed calls each after 2 warm-up rounds. TFLOP/s: operations from shapes (listed tiles x 2 rows cols D for the "
             "pass, x 4 for the forward) over the median.", "",
             "| walk | call | median ms | min - max ms | TFLOP/s |", "|---|---|---|---|---|"]
    att = L.LiteAttention(threshold=-10.0, max_batch_size=1)
    att.threshold = float("-inf")                                 # the forward flags nothing: the imposed list is a fixed point
    att._get_read_write_lists(q, k)
    att._phase = 0
    ratios = {}
    for name, s_ in (("dense", 0.0), (f"imposed {a.sparsity:.0%}", a.sparsity)):
        rows = banded_rows(qt, kt, bm, bn, s_)
        impose_lists(att, rows)
        fwd_flops = executed_flops(rows, H, 1, S, S, bm, bn, D)
        walk = None if s_ == 0.0 else att.current_read_list()
        fwd = (lambda: L.flash_attn_func(q, k, v)) if s_ == 0.0 else (lambda: att(q, k, v))
        ms_m, ms_f = timed_pair([lambda: L.vote_margins(q, k, read_list=walk), fwd], a.reps)
        (lm, med_m), (lf, med_f) = row("la_vote_margins", ms_m, fwd_flops / 2), row("la_fwd", ms_f, fwd_flops)
        lines += [f"| {name} " + lm, f"| {name} " + lf]
        ratios[name] = med_m / med_f
    lines += ["", "Ratio la_vote_margins / la_fwd (medians): " + ", ".join(f"{n}: **{r:.3f}**" for n, r in ratios.items()) + ".", ""]
    del q, k, v, att

    w = DenoiseWorkload(H, dev, steps=50)
    calls = {"n": 0}

    def qkv_at(t):
        calls["n"] += 1
        return w.qkv(t)

    res = {}
    for name, fn in (("calibrate_skip_schedule", lambda: calibrate_skip_schedule(qkv_at, a.steps, [a.sparsity / a.steps * (t + 1) for t in range(a.steps)])),
                     ("calibrate_threshold", lambda: calibrate_threshold(qkv_at, a.steps, a.sparsity))):
        calls["n"] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        res[name] = (time.perf_counter() - t0, calls["n"], out)
    sk, th = res["calibrate_skip_schedule"], res["calibrate_threshold"]
    lines += [f"## Calibration on {a.steps} steps of DenoiseWorkload (S = {w.S}, H = {H})", "",
              "Host clock around the whole call, ending in a device synchronise; the workload's own generation of q, k, v (one call of "
              "`qkv(t)` per forward) is inside both. One run each: no spread was measured for these two numbers.", "",
              "| calibrator | wall s | forward calls | result |", "|---|---|---|---|",
              f"| calibrate_skip_schedule (targets rising to {a.sparsity:.0%}) | {sk[0]:.2f} | {sk[1]} | thresholds "
              f"{[round(x, 3) for x in sk[2][0]]}, kept / walked {[round(e['kept'] / e['walked'], 3) for e in sk[2][1]]} |",
              f"| calibrate_threshold (target {a.sparsity:.0%}, iters 10, tol 0.01) | {th[0]:.2f} | {th[1]} | threshold {th[2][0]:.3f}, "
              f"skip fractions {[round(x, 3) for x in th[2][1]]} |", "",
              f"Wall-time ratio calibrate_skip_schedule / calibrate_threshold: **{sk[0] / th[0]:.3f}**.", ""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
