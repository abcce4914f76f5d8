#!/usr/bin/env python
"""The q / k prologue at the headline shape, one process, one session: `qk_prep` (`la_qk_prep`: token RMSNorm + Wan's 3-axis RoPE + cast)
on q and k of (1, 75 600, 40, 128) on the grid (21, 45, 80), bf16 -> bf16 and fp32 -> bf16, against
  * `la_combine` at the same output shape (two bf16 partials -> bf16: existing code that also reads and writes a stream), the yardstick
    of the algorithmic TB/s (bytes read once + bytes written once);
  * the demo block's eager prologue (`RMSNorm` + `rope_3d` + `.bfloat16()`, examples/wan_self_attention_demo.py) on the same tensors;
  * one `LiteAttention` step on the imposed 42 % list, whose share of time the two prologues are reported as.
HIP events, 3 warm-up + 20 timed launches, median (min, max).

    python tools/qk_prep_bench.py [--grid 21 45 80 --heads 40 --head-dim 128] [--out profiles/qk_prep.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import liteattention_amd as L                                      # noqa: E402
import wan_self_attention_demo as demo                             # noqa: E402
from selfcheck import banded_rows, impose_lists                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, nargs=3, default=[21, 45, 80])
ap.add_argument("--heads", type=int, default=40)
ap.add_argument("--head-dim", type=int, default=128)
ap.add_argument("--sparsity", type=float, default=0.42)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--no-attention", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qk_prep.json"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
grid = tuple(a.grid)
S, H, D = grid[0] * grid[1] * grid[2], a.heads, a.head_dim
shape = (1, S, H, D)


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


g = torch.Generator(device=dev).manual_seed(0)
q32 = torch.randn(shape, device=dev, generator=g) * 2.0
k32 = torch.randn(shape, device=dev, generator=g) * 2.0
norm_q, norm_k = demo.RMSNorm(H * D).to(dev), demo.RMSNorm(H * D).to(dev)
with torch.no_grad():
    norm_q.weight.copy_(0.5 + torch.rand(H * D, device=dev, generator=g))
    norm_k.weight.copy_(0.5 + torch.rand(H * D, device=dev, generator=g))
wq, wk = norm_q.weight.detach(), norm_k.weight.detach()
tables = L.rope_tables(grid, D, device=dev)
res = {"shape": list(shape), "grid": list(grid), "timing": f"HIP events, {a.warmup} warm-up + {a.iters} timed, median (min, max)",
       "device": torch.cuda.get_device_name(0), "build": L._cabi.build_info().get("src"), "cases": {}}

# la_combine at the same output shape: two bf16 partials + their LSE in, one bf16 output + LSE out
part = torch.randn((2,) + shape, device=dev, generator=g).bfloat16()
lse_part = torch.randn(2, 1, H, S, device=dev, generator=g)
o_comb = torch.empty(shape, dtype=torch.bfloat16, device=dev)
comb = timed(lambda: L.flash_attn_combine(part, lse_part, out=o_comb))
comb_bytes = part.numel() * 2 + lse_part.numel() * 4 + o_comb.numel() * 2 + H * S * 4
comb["bytes"], comb["TBps"] = comb_bytes, round(comb_bytes / comb["ms"] / 1e9, 3)
res["la_combine"] = comb
print("la_combine", json.dumps(comb), flush=True)
del part, lse_part, o_comb


def eager_prologue(x, norm):
    """The demo block's lines between the projection and the attention call, for one of q / k."""
    with torch.no_grad():
        return demo.rope_3d(norm(x.view(1, S, H * D)).view(shape), grid).bfloat16()


for name, q_in, k_in in (("bf16_to_bf16", q32.bfloat16(), k32.bfloat16()), ("fp32_to_bf16", q32, k32)):
    oq, ok = torch.empty(shape, dtype=torch.bfloat16, device=dev), torch.empty(shape, dtype=torch.bfloat16, device=dev)

    def fused():
        L.qk_prep(q_in, wq, norm_q.eps, tables, out=oq)
        L.qk_prep(k_in, wk, norm_k.eps, tables, out=ok)

    def eager():
        return eager_prologue(q_in, norm_q), eager_prologue(k_in, norm_k)

    f = timed(fused)
    nbytes = 2 * (q_in.numel() * q_in.element_size() + oq.numel() * 2)
    f["bytes"], f["TBps"] = nbytes, round(nbytes / f["ms"] / 1e9, 3)
    f["TBps_over_la_combine"] = round(f["TBps"] / comb["TBps"], 3)
    try:
        e = timed(eager)
        eq, _ = eager()
        ref = L.qk_prep_reference(q_in[:, :4096], wq, norm_q.eps, tables)
        e["max_abs_err_vs_fp64_first_4096_rows"] = (eq[:, :4096].double() - ref).abs().max().item()
        f["max_abs_err_vs_fp64_first_4096_rows"] = (oq[:, :4096].double() - ref).abs().max().item()
        e["over_qk_prep"] = round(e["ms"] / f["ms"], 2)
        del eq, ref
    except torch.cuda.OutOfMemoryError as exc:                     # report it; the caller reruns with a smaller --grid and says so
        e = {"error": f"out of memory: {exc}"}
    res["cases"][name] = {"qk_prep_q_and_k": f, "eager_q_and_k": e}
    print(name, json.dumps(res["cases"][name]), flush=True)
    torch.cuda.empty_cache()

if not a.no_attention:
    q, k = oq, ok
    v = torch.randn(shape, device=dev, generator=g).bfloat16()
    bm, bn = L.get_tile_sizes(D, 2)
    att = L.LiteAttention(threshold=-10.0, max_batch_size=1)
    att.threshold = float("-inf")
    att._get_read_write_lists(q, k)
    att._phase = 0
    impose_lists(att, banded_rows(-(-S // bm), -(-S // bn), bm, bn, a.sparsity))
    t = timed(lambda: att(q, k, v))
    t["imposed_sparsity"] = a.sparsity
    res["attention_step"] = t
    for case in res["cases"].values():
        for side in ("qk_prep_q_and_k", "eager_q_and_k"):
            if "ms" in case[side]:
                case[side]["share_of_attention_step"] = round(case[side]["ms"] / t["ms"], 4)
    print("attention", json.dumps(t), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
print("wrote", a.out)
