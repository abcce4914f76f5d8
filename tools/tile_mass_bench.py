#!/usr/bin/env python
"""la_tile_mass beside la_vote_margins and la_fwd, and calibrate_mass_schedule beside calibrate_error_schedule, in one process ->
profiles/tile_mass.md.

(1) Headline shape (1, 75 600, 40, 128, bf16), dense and under an imposed banded list (default 42 % sparsity): device-event time of one
la_tile_mass pass with all three outputs, of the pass without the margins, of one la_vote_margins pass and of one la_fwd call over the
SAME walk, alternated, `--reps` timed calls each after warm-up; median, min - max spread and the ratios of the medians. The lse given to
the pass is the forward's own. Operations from shapes: a pass does 2 S_q S_k D H per listed tile pair (Q K^T), the forward twice that.
(2) `--steps` steps of tools.selfcheck.DenoiseWorkload: wall time and forward calls (LiteAttention calls, and dense flash_attn_func
calls of the error calibrator) of calibrate_mass_schedule and of calibrate_error_schedule at its default iters.
(3) Registers, LDS and resident workgroups of every instantiation of la_tile_mass_kernel, from a compile of its source with the build's
flags (`-Rpass-analysis=kernel-resource-usage`; no device involved).
    python tools/tile_mass_bench.py [--reps 6] [--steps 3] [--sparsity 0.42] [--out profiles/tile_mass.md]"""
import argparse
import os
import re
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import liteattention_amd as L                                    # noqa: E402
from liteattention_amd import flash_attn_interface, lite_attention      # noqa: E402
from liteattention_amd.calibration import calibrate_error_schedule, calibrate_mass_schedule      # noqa: E402
from tools.selfcheck import DenoiseWorkload, banded_rows, executed_flops, impose_lists      # noqa: E402
from tools.vote_margins_bench import row, timed_pair             # noqa: E402


def resource_rows(k_tiles):
    """Per instantiation of la_tile_mass.hip (bf16; the fp16 ones differ in the MFMA opcode alone): VGPRs, spills, the dynamic LDS of a
    walk of `k_tiles` (tile_mass_lds_bytes) and the workgroups a compute unit holds (four waves per workgroup, one per SIMD: waves per
    SIMD by registers, 160 KiB by LDS)."""
    from liteattention_amd.build import CSRC, INCLUDE, _hipcc
    src = os.path.join(CSRC, "la_tile_mass.hip")
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", INCLUDE, "-I", CSRC, "-c", src, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    rows = []
    for m in re.finditer(r"tile_mass_kernelILb0ELi(\d+)ELi(\d)ELb([01])E.*?VGPRs: (\d+).*?AGPRs: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                         r"VGPRs Spill: (\d+)", r.stderr, flags=re.S):
        D, nq, margins, vgpr, agpr, occ, spill = (int(x) for x in m.groups())
        lds = 2 * 64 * (2 * D + 16) + 128 + 4 * ((k_tiles + 3) & ~3) + 8 * ((k_tiles + 31) // 32)
        rows.append((D, -nq, margins, f"| {D} | {128 * nq} x 64 | {'yes' if margins else 'no'} | {4 * nq * D // 16} | {vgpr} | {agpr} | {spill} | "
                                      f"{lds} | {min(occ, 160 * 1024 // lds)} |"))
    return [r[3] for r in sorted(rows)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--sparsity", type=float, default=0.42)
    ap.add_argument("--seqlen", type=int, default=75600)
    ap.add_argument("--heads", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_mass.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tile_mass_bench needs a GPU: nothing here is measured on a CPU")
    dev, S, H, D = torch.device("cuda"), a.seqlen, a.heads, 128
    g = torch.Generator(device=dev).manual_seed(1234)
    q, k, v = [torch.randn(1, S, H, D, device=dev, generator=g).bfloat16() for _ in range(3)]
    bm, bn = L.get_tile_sizes(D, 2)
    qt, kt = -(-S // bm), -(-S // bn)
    lines = ["# la_tile_mass beside la_vote_margins and la_fwd", "",
             f"`tools/tile_mass_bench.py --reps {a.reps} --steps {a.steps} --sparsity {a.sparsity}` on {torch.cuda.get_device_name()}; "
             f"shape (1, {S}, {H}, {D}) bf16, q-tile {bm} x {bn}. Device events around single calls, the four calls alternated, "
             f"{a.reps} timed calls each after 2 warm-up rounds. TFLOP/s: operations from shapes (listed tiles x 2 rows cols D for a "
             "pass, x 4 for the forward) over the median; the exponentials of the mass pass are not counted.", "",
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
        fwd = (lambda: L.flash_attn_func(q, k, v)) if s_ == 0.0 else (lambda: att(q, k, v))
        lse = (L.flash_attn_func(q, k, v, return_softmax_lse=True) if s_ == 0.0 else att(q, k, v, return_softmax_lse=True))[1]
        ms = timed_pair([lambda: L.tile_mass(q, k, lse, read_list=walk, margins=True), lambda: L.tile_mass(q, k, lse, read_list=walk),
                         lambda: L.vote_margins(q, k, read_list=walk), fwd], a.reps)
        meds = []
        for call, m, fl in zip(("la_tile_mass + margins", "la_tile_mass", "la_vote_margins", "la_fwd"), ms,
                               (fwd_flops / 2, fwd_flops / 2, fwd_flops / 2, fwd_flops)):
            line, med = row(call, m, fl)
            lines.append(f"| {name} " + line)
            meds.append(med)
        ratios.append(f"{name}: mass + margins / la_vote_margins **{meds[0] / meds[2]:.3f}**, mass + margins / la_fwd **{meds[0] / meds[3]:.3f}**"
                      + (" (the pass is SLOWER than the forward)" if meds[0] > meds[3] else ""))
    lines += ["", "Ratios of medians - " + "; ".join(ratios) + ".", ""]
    del q, k, v, att, lse

    w = DenoiseWorkload(H, dev, steps=50)
    calls = {"sparse": 0, "dense": 0}
    att_call, dense_call = lite_attention.LiteAttention.__call__, flash_attn_interface.flash_attn_func

    def counted_att(self, *args, **kw):
        calls["sparse"] += 1
        return att_call(self, *args, **kw)

    def counted_dense(*args, **kw):
        calls["dense"] += 1
        return dense_call(*args, **kw)

    lite_attention.LiteAttention.__call__, flash_attn_interface.flash_attn_func = counted_att, counted_dense
    res = {}
    for name, fn in (("calibrate_mass_schedule", lambda: calibrate_mass_schedule(w.qkv, a.steps, [0.02] * a.steps)),
                     ("calibrate_error_schedule", lambda: calibrate_error_schedule(w.qkv, a.steps, [0.02] * a.steps))):
        calls.update(sparse=0, dense=0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        res[name] = (time.perf_counter() - t0, dict(calls), out)
    lite_attention.LiteAttention.__call__, flash_attn_interface.flash_attn_func = att_call, dense_call
    ms_, er = res["calibrate_mass_schedule"], res["calibrate_error_schedule"]
    lines += [f"## Calibration on {a.steps} steps of DenoiseWorkload (S = {w.S}, H = {H})", "",
              "Host clock around the whole call, ending in a device synchronise; the workload's own generation of q, k, v is inside both. "
              "One run each: no spread was measured for these two numbers. The two calibrators bound different things (a mass budget of "
              "0.02 per step against the step's own softmax; a rel_l1 bound of 0.02 against the dense output): the thresholds are not "
              "comparable, the launch counts are.", "",
              "| calibrator | wall s | LiteAttention calls | dense calls | map passes | result |", "|---|---|---|---|---|---|",
              f"| calibrate_mass_schedule (budget 0.02, max) | {ms_[0]:.2f} | {ms_[1]['sparse']} | {ms_[1]['dense']} | {a.steps} | thresholds "
              f"{[round(x, 3) for x in ms_[2][0]]}, predicted mass {[round(e['predicted_mass'], 4) for e in ms_[2][1]]} |",
              f"| calibrate_error_schedule (rel_l1 0.02, iters 8) | {er[0]:.2f} | {er[1]['sparse']} | {er[1]['dense']} | 0 | thresholds "
              f"{[round(x, 3) for x in er[2][0]]}, errors {[round(e['error'], 4) for e in er[2][1]]} |", "",
              f"Wall-time ratio calibrate_mass_schedule / calibrate_error_schedule: **{ms_[0] / er[0]:.3f}**.", "",
              f"## Resources of la_tile_mass_kernel (compile for gfx950, bf16; LDS for the {kt} key tiles of the headline shape)", "",
              "| head_dim | q-tile | margins | Q registers | VGPRs | AGPRs | spilled | LDS bytes | workgroups / CU |",
              "|---|---|---|---|---|---|---|---|---|"] + resource_rows(kt) + [""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
