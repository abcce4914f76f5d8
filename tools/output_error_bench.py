#!/usr/bin/env python
"""`la_output_error` (liteattention_amd.calibration.output_error) at the headline output shape (1, 75 600, 40, 128) against the torch
expression that yields the same six numbers per head on the same tensors: bf16 against bf16 and bf16 against fp32, rows_per_bin 256.
HIP events, 3 warm-up + 20 timed launches, median. Bytes / time is the ALGORITHMIC rate (each operand read once).

    python tools/output_error_bench.py [--seqlen 75600 --heads 40] [--out profiles/output_error_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from liteattention_amd.calibration import output_error            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seqlen", type=int, default=75600)
ap.add_argument("--heads", type=int, default=40)
ap.add_argument("--head-dim", type=int, default=128)
ap.add_argument("--rows-per-bin", type=int, default=256)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "output_error_bench.json"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
shape = (1, a.seqlen, a.heads, a.head_dim)


def torch_six(out, ref):
    """The same six numbers per (batch, head) from torch ops (fp32 temporaries; the sums accumulate in fp32 there)."""
    o, r = out.float(), ref.float()
    fin = torch.isfinite(o) & torch.isfinite(r)
    d = torch.where(fin, o - r, 0.0)
    r = torch.where(fin, r, 0.0)
    return torch.stack([d.abs().sum(dim=(1, 3)), r.abs().sum(dim=(1, 3)), (d * d).sum(dim=(1, 3)), (r * r).sum(dim=(1, 3)),
                        d.abs().amax(dim=(1, 3)), (~fin).sum(dim=(1, 3)).float()], dim=-1)


def median_ms(fn):
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
    return statistics.median(times), min(times), max(times)


g = torch.Generator(device=dev).manual_seed(0)
ref32 = torch.randn(shape, device=dev, generator=g)
out = (ref32 + 0.01 * torch.randn(shape, device=dev, generator=g)).bfloat16()
res = {"shape": list(shape), "rows_per_bin": a.rows_per_bin, "timing": f"HIP events, {a.warmup} warm-up + {a.iters} timed, median (min, max)", "cases": {}}
for name, ref in (("bf16_vs_bf16", ref32.bfloat16()), ("bf16_vs_fp32", ref32)):
    nbytes = out.numel() * out.element_size() + ref.numel() * ref.element_size()
    k = median_ms(lambda: output_error(out, ref, rows_per_bin=a.rows_per_bin))
    k_head = median_ms(lambda: output_error(out, ref, rows_per_bin=a.seqlen))
    t = median_ms(lambda: torch_six(out, ref))
    es = output_error(out, ref, rows_per_bin=a.rows_per_bin)
    six = torch.stack([es.stats[..., i].sum(-1) for i in range(4)] + [es.max_abs, es.nonfinite.double()], dim=-1)
    rel = ((six - torch_six(out, ref).double()).abs() / six.abs().clamp_min(1e-300)).amax().item()
    res["cases"][name] = {
        "bytes": nbytes, "kernel_ms": round(k[0], 4), "kernel_ms_min_max": [round(k[1], 4), round(k[2], 4)],
        "kernel_TBps": round(nbytes / k[0] / 1e9, 3), "kernel_one_bin_per_head_ms": round(k_head[0], 4),
        "torch_ms": round(t[0], 4), "torch_ms_min_max": [round(t[1], 4), round(t[2], 4)], "torch_over_kernel": round(t[0] / k[0], 2),
        "fraction_of_la_combine_5.0_5.2_TBps": [round(nbytes / k[0] / 1e9 / x, 3) for x in (5.0, 5.2)],
        "fraction_of_streaming_read_6.0_6.3_TBps": [round(nbytes / k[0] / 1e9 / x, 3) for x in (6.0, 6.3)],
        "max_rel_diff_of_the_six_numbers_kernel_fp64_vs_torch_fp32": rel}
    print(name, json.dumps(res["cases"][name]), flush=True)
    del ref
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    json.dump(res, fh, indent=1)
print("wrote", a.out)
