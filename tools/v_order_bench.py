"""What a token order costs on the V side and on the O side of a layer: each fused pass (v_prep_tiles_rows, `rows=` on v_colstats /
attn_unshift / attn_out_fp8) against the route it replaces (TokenOrder.gather or restore + restore_lse around the unmapped pass) and
against the unmapped pass alone, which is the floor: the fused pass moves the same bytes. -> profiles/v_order.md.

    python tools/v_order_bench.py [--grid 21 45 80] [--heads 40] [--head-dim 128] [--repeats 30] [--out FILE.json]

Method: every variant is warmed up, then the variants of a group run interleaved `--repeats` times, each timed by a pair of events on
the launch stream; median and min / max per variant (the spread to read a difference against). All buffers are allocated before the
loop. The fused results are checked against the routes they replace, bit for bit, at the size that is timed."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import liteattention_amd as L                                      # noqa: E402
from liteattention_amd import _cabi                                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, nargs=3, default=[21, 45, 80])
ap.add_argument("--heads", type=int, default=40)
ap.add_argument("--head-dim", type=int, default=128)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeats", type=int, default=30)
ap.add_argument("--out", default=None, help="also write the JSON result here")
a = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU: there is no CPU path"
dev = torch.device("cuda", 0)
grid = tuple(a.grid)
S, H, D = grid[0] * grid[1] * grid[2], a.heads, a.head_dim
order = L.brick_order(grid, device=dev)
dst = order.dst_rows
g = torch.Generator(device=dev).manual_seed(0)
f32 = dict(dtype=torch.float32, device=dev)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(variants):
    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
    times = {name: [] for name in variants}
    for _ in range(a.repeats):
        for name, fn in variants.items():
            times[name].append(event_ms(fn))
    return {name: {"ms": round(statistics.median(t), 4), "ms_min_max": [round(min(t), 4), round(max(t), 4)]} for name, t in times.items()}


res = {"shape": [1, S, H, D], "grid": list(grid), "bricks": [list(b) for b in order.bricks], "device": torch.cuda.get_device_name(0),
       "build": _cabi.build_info().get("src"), "repeats": a.repeats}

# ---- V: statistics + tiles ------------------------------------------------------------------------------------------------------------------
v = (torch.randn((1, S, H, D), device=dev, generator=g) * 2.0 + 0.3).bfloat16()
vg = torch.empty_like(v)
part = torch.empty((L.v_colstats_parts(S, H, D)[0], 3, 1, H, D), **f32)
mean, amax, mean2, amax2 = torch.empty((1, H, D), **f32), torch.empty((1, H), **f32), torch.empty((1, H, D), **f32), torch.empty((1, H), **f32)
dv = torch.full((1, H), 0.02, **f32)
pv = L.v_prep_tiles(v, descale=dv, shift=mean)
pv2 = L.v_prep_tiles(v, descale=dv, shift=mean)


def v_route(x, out, m, am, rows=None):
    L.v_colstats(x, stat_part=part, mean_out=m, amax_out=am, rows=rows)
    if rows is None:
        L.v_prep_tiles(x, descale=dv, shift=m, out=out)
    else:
        L.v_prep_tiles_rows(x, rows, descale=dv, shift=m, out=out)


res["v"] = measure({"gather + v_colstats + v_prep_tiles": lambda: v_route(order.gather(v, out=vg), pv, mean, amax),
                    "v_colstats(rows=) + v_prep_tiles_rows": lambda: v_route(v, pv2, mean2, amax2, rows=order),
                    "v_colstats + v_prep_tiles (no order)": lambda: v_route(v, pv2, mean2, amax2)})
v_route(order.gather(v, out=vg), pv, mean, amax)
v_route(v, pv2, mean2, amax2, rows=order)
n = L.v_tiles_bytes(1, H, S, D)[0]
assert torch.equal(pv.workspace[:n], pv2.workspace[:n]) and torch.equal(mean, mean2) and torch.equal(amax, amax2)
print(json.dumps(res["v"], indent=1), flush=True)
del v, vg, pv, pv2
torch.cuda.empty_cache()

# ---- O: restored to raster order, as bf16 and as row-scaled e4m3 ------------------------------------------------------------------------------
o = torch.randn((1, S, H, D), device=dev, generator=g).bfloat16()
lse = torch.randn((1, H, S), device=dev, generator=g)
shift = torch.randn((1, H, D), device=dev, generator=g)
tmp, out, out2 = torch.empty_like(o), torch.empty_like(o), torch.empty_like(o)
lse2 = torch.empty_like(lse)
o8, o8b = torch.empty(o.shape, dtype=torch.float8_e4m3fn, device=dev), torch.empty(o.shape, dtype=torch.float8_e4m3fn, device=dev)
ds, dsb = torch.empty((1, S, 1), **f32), torch.empty((1, S, 1), **f32)
res["o_bf16"] = measure({
    "attn_unshift + restore + restore_lse": lambda: (L.attn_unshift(o, shift, lse=lse, out=tmp), order.restore(tmp, out=out), order.restore_lse(lse)),
    "attn_unshift(rows=dst_rows)": lambda: L.attn_unshift(o, shift, lse=lse, out=out2, lse_out=lse2, rows=dst),
    "attn_unshift (no order)": lambda: L.attn_unshift(o, shift, lse=lse, out=out2)})
L.attn_unshift(o, shift, lse=lse, out=tmp)
order.restore(tmp, out=out)
L.attn_unshift(o, shift, lse=lse, out=out2, lse_out=lse2, rows=dst)
assert torch.equal(out, out2) and torch.equal(lse2, order.restore_lse(lse))
res["o_fp8"] = measure({
    "restore + restore_lse + attn_out_fp8": lambda: L.attn_out_fp8(order.restore(o, out=tmp), shift, lse=order.restore_lse(lse), out=o8, descale_out=ds),
    "attn_out_fp8(rows=dst_rows)": lambda: L.attn_out_fp8(o, shift, lse=lse, out=o8b, descale_out=dsb, lse_out=lse2, rows=dst),
    "attn_out_fp8 (no order)": lambda: L.attn_out_fp8(o, shift, lse=lse, out=o8b, descale_out=dsb)})
L.attn_out_fp8(order.restore(o, out=tmp), shift, lse=order.restore_lse(lse), out=o8, descale_out=ds)
L.attn_out_fp8(o, shift, lse=lse, out=o8b, descale_out=dsb, lse_out=lse2, rows=dst)
assert torch.equal(o8.view(torch.uint8), o8b.view(torch.uint8)) and torch.equal(ds, dsb)
print(json.dumps({k: res[k] for k in ("o_bf16", "o_fp8")}, indent=1), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
