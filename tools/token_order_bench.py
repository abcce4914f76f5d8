#!/usr/bin/env python
"""Token orders at the headline shape, one process, one session -> profiles/token_order.md (+ .json).

(a) What the row map costs. `qk_prep` (token RMSNorm + Wan's 3-axis RoPE + cast, bf16 -> bf16) of (1, 75 600, 40, 128) on the grid
    (21, 45, 80): unmapped, `rows=order` (the gather fused into the pass) and `positions=order` (input already in the order), and
    `TokenOrder.gather` against `torch.index_select` on a tensor of the same shape. All variants in this process, INTERLEAVED: repeat r
    times (every variant once); HIP events around each call; median and min - max per variant. With `--parent-lib` the unmapped
    `la_qk_prep` of that library (the parent commit, `python -m liteattention_amd.build --out=build_variants/parent.so` in a worktree
    of it) runs in the same loop on the same tensors, called through the C-ABI as this tree's is.
(b) What an order does to the vote, on a SYNTHETIC field - no model. Per head and channel a smooth random field over the grid,
        f[s, h, c] = sqrt(2 / J) sum_j cos(2 pi u[h, j] . p_s + phi[h, c, j]),   p_s = (t / T, y / H, x / W),   J = 6,
    u[h, j] integer frequencies drawn uniformly from {0..2} x {0..3} x {0..4} (not all zero), phi uniform in [0, 2 pi): unit variance,
    correlation length a third of the grid and more. q = k = sqrt(alpha / sqrt(D)) (f + 0.1 n), n ~ N(0, 1), so that the score of a
    token with itself is about alpha and with a far token about alpha N(0, 1 / D); v ~ N(0, 1). The same tokens in raster order and in
    two brick orders (`TokenOrder.gather`), `LiteAttention` at equal thresholds: step 0 builds the list, step 1 reads it. Reported per
    (alpha, threshold, order): the skipped-tile fraction of that list, the `la_output_error` statistics of step 1 against the dense
    result in the same order, ms of step 1 (median of `--iters` replays from a snapshot of the list). Reported, not gated.

    python tools/token_order_bench.py [--grid 21 45 80 --heads 40 --head-dim 128] [--parent-lib build_variants/parent.so]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import liteattention_amd as L                                      # noqa: E402
from liteattention_amd import _cabi                                # noqa: E402

Q = sys.modules["liteattention_amd.qk_prep"]

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, nargs=3, default=[21, 45, 80])
ap.add_argument("--heads", type=int, default=40)
ap.add_argument("--head-dim", type=int, default=128)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeats", type=int, default=30, help="(a): interleaved repeats")
ap.add_argument("--iters", type=int, default=5, help="(b): timed replays of step 1")
ap.add_argument("--alphas", type=float, nargs="*", default=[10.0, 14.0, 20.0])
ap.add_argument("--thresholds", type=float, nargs="*", default=[-8.0, -6.0, -2.0])
ap.add_argument("--parent-lib", default=None, help="the parent commit's library: its unmapped la_qk_prep joins the loop of (a)")
ap.add_argument("--skip-sparsity", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_order"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
grid = tuple(a.grid)
S, H, D = grid[0] * grid[1] * grid[2], a.heads, a.head_dim
shape = (1, S, H, D)
BRICKS = {"bricks (2,16,8)/(1,8,8)": ((2, 16, 8), (1, 8, 8)), "bricks (1,16,16)/(1,8,8)": ((1, 16, 16), (1, 8, 8))}
res = {"shape": list(shape), "grid": list(grid), "device": torch.cuda.get_device_name(0), "build": _cabi.build_info().get("src")}


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(times):
    return {"ms": round(statistics.median(times), 4), "ms_min_max": [round(min(times), 4), round(max(times), 4)]}


# ---- (a) the cost of the map --------------------------------------------------------------------------------------------------------------
g = torch.Generator(device=dev).manual_seed(0)
x = (torch.randn(shape, device=dev, generator=g) * 2.0).bfloat16()
w = 0.5 + torch.rand(H * D, device=dev, generator=g)
tables = L.rope_tables(grid, D, device=dev)
order = L.brick_order(grid, BRICKS["bricks (1,16,16)/(1,8,8)"], device=dev)
idx64 = order.src_rows.long()
xg = order.gather(x)
out, out2 = torch.empty_like(x), torch.empty_like(x)
tabs, pairs = Q._unpack_tables(tables, D)
args = Q._prep_args(_cabi.LaQkPrepArgs, x, out, _cabi.LA_NORM_TOKEN, w, 1e-6, 0, tabs, pairs)
args.out_dtype = _cabi.LA_DTYPE_BF16
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def c_call(lib):
    def run():
        rc = lib.la_qk_prep(ctypes.byref(args), stream)
        assert rc == _cabi.LA_OK, rc
    return run


variants = {"qk_prep unmapped (this tree, C-ABI)": c_call(_cabi.load()),
            "qk_prep unmapped (this tree, Python)": lambda: L.qk_prep(x, w, 1e-6, tables, out=out),
            "qk_prep rows=order (fused gather)": lambda: L.qk_prep(x, w, 1e-6, tables, out=out2, rows=order),
            "qk_prep positions=order (input in the order)": lambda: L.qk_prep(xg, w, 1e-6, tables, out=out2, positions=order),
            "TokenOrder.gather": lambda: order.gather(x, out=out2),
            "torch.index_select(x, 1, rows)": lambda: torch.index_select(x, 1, idx64, out=out2)}
if a.parent_lib:
    parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
    parent.la_qk_prep.argtypes, parent.la_qk_prep.restype = [ctypes.POINTER(_cabi.LaQkPrepArgs), ctypes.c_void_p], ctypes.c_int
    parent.la_build_info.restype = ctypes.c_char_p
    res["parent_build"] = parent.la_build_info().decode()
    variants["qk_prep unmapped (parent commit, C-ABI)"] = c_call(parent)
for _ in range(a.warmup):
    for fn in variants.values():
        fn()
times = {name: [] for name in variants}
for _ in range(a.repeats):
    for name, fn in variants.items():
        times[name].append(event_ms(fn))
nbytes = 2 * x.numel() * 2
res["cost"] = {name: dict(summary(t), TBps=round(nbytes / statistics.median(t) / 1e9, 3)) for name, t in times.items()}
assert torch.equal(L.qk_prep(x, w, 1e-6, tables, rows=order), L.qk_prep(x, w, 1e-6, tables)[:, idx64])
assert torch.equal(order.gather(x), torch.index_select(x, 1, idx64))
print(json.dumps(res["cost"], indent=1), flush=True)
del x, xg, out, out2
torch.cuda.empty_cache()


# ---- (b) the vote on a synthetic field with 3-D locality ----------------------------------------------------------------------------------
def synthetic_field(seed, J=6):
    """(1, S, H, D) fp32: f + 0.1 n of the docstring, head by head."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    T, Hh, W = grid
    t = torch.arange(T, device=dev).view(T, 1, 1).expand(T, Hh, W).reshape(-1).float() / T
    y = torch.arange(Hh, device=dev).view(1, Hh, 1).expand(T, Hh, W).reshape(-1).float() / Hh
    xx = torch.arange(W, device=dev).view(1, 1, W).expand(T, Hh, W).reshape(-1).float() / W
    p = torch.stack((t, y, xx), 1)                                                      # (S, 3)
    f = torch.empty(S, H, D, device=dev)
    for h in range(H):
        u = torch.zeros(J, 3, device=dev)
        while (u.abs().sum(1) == 0).any():
            u = torch.stack([torch.randint(0, hi + 1, (J,), device=dev, generator=gen) for hi in (2, 3, 4)], 1).float()
        phi = 2 * math.pi * torch.rand(1, J, D, device=dev, generator=gen)
        ang = 2 * math.pi * (p @ u.t())                                                 # (S, J)
        f[:, h] = math.sqrt(2.0 / J) * torch.cos(ang[:, :, None] + phi).sum(1)
    return (f + 0.1 * torch.randn(S, H, D, device=dev, generator=gen))[None]


if not a.skip_sparsity:
    field = synthetic_field(1)
    v = torch.randn(shape, device=dev, generator=g).bfloat16()
    orders = {"raster": None}
    orders.update({name: L.brick_order(grid, b, device=dev) for name, b in BRICKS.items()})
    rows = []
    for alpha in a.alphas:
        qk = (math.sqrt(alpha / math.sqrt(D)) * field).bfloat16()
        for name, o in orders.items():
            q = qk if o is None else o.gather(qk)
            vv = v if o is None else o.gather(v)
            dense = L.flash_attn_func(q, q, vv)
            for thr in a.thresholds:
                att = L.LiteAttention(threshold=thr, max_batch_size=1)
                att(q, q, vv)                                                            # step 0: every tile, writes the list
                snap = att.snapshot()
                skipped = att.get_skip_fraction(batch=1)
                ms = []
                for _ in range(a.iters):
                    att.restore(snap)
                    o1 = [None]
                    ms.append(event_ms(lambda: o1.__setitem__(0, att(q, q, vv))))
                err = L.output_error(o1[0], dense)
                row = {"alpha": alpha, "threshold": thr, "order": name, "skipped": round(skipped, 4), "listed": round(1 - skipped, 4),
                       "rel_l1_mean": float(err.rel_l1.mean()), "rel_l1_max": float(err.rel_l1.max()),
                       "max_abs": float(err.max_abs.max()), **summary(ms)}
                rows.append(row)
                print(json.dumps(row), flush=True)
            del q, vv, dense
        del qk
    res["sparsity"] = rows

# ---- the report ---------------------------------------------------------------------------------------------------------------------------
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out + ".json", "w") as fh:
    json.dump(res, fh, indent=1)
md = [f"# Token orders at {shape} bf16 on the grid {grid} ({res['device']})", "",
      "Written by `tools/token_order_bench.py` (its docstring states the method); raw numbers in `token_order.json`.", "",
      f"## (a) The cost of the row map: one process, {a.repeats} interleaved repeats, HIP events, median (min - max)", "",
      "| call | ms | min - max | TB/s of 2 x 774 MB |", "|---|---|---|---|"]
for name, c in res["cost"].items():
    md.append(f"| {name} | {c['ms']:.4f} | {c['ms_min_max'][0]:.4f} - {c['ms_min_max'][1]:.4f} | {c['TBps']:.2f} |")
md += ["", "The mapped calls and the gathered unmapped result are bit-equal (asserted in the run)."
       + (f" Parent library: `{res['parent_build']}`." if a.parent_lib else " No parent library was given: the parent row is missing."), ""]
if "sparsity" in res:
    md += ["## (b) SYNTHETIC: the vote on a smooth random 3-D field, raster order against two brick orders", "",
           "A generator, not a model: **no real-model gain has been measured.** q = k = sqrt(alpha / sqrt(D)) (f + 0.1 n) with f a sum of "
           "6 random low-frequency 3-D cosines per head and channel (formula in the tool's docstring), v ~ N(0, 1). Step 0 builds the list "
           "at the threshold, step 1 reads it; error of step 1 against the dense result in the same order (`la_output_error`, over heads).", "",
           "| alpha | threshold | order | tiles skipped | tiles listed | rel. L1 mean | rel. L1 max | max abs | ms step 1 (min - max) |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in res["sparsity"]:
        md.append(f"| {r['alpha']:g} | {r['threshold']:g} | {r['order']} | {r['skipped']:.3f} | {r['listed']:.3f} | {r['rel_l1_mean']:.2e} | "
                  f"{r['rel_l1_max']:.2e} | {r['max_abs']:.2e} | {r['ms']:.2f} ({r['ms_min_max'][0]:.2f} - {r['ms_min_max'][1]:.2f}) |")
    md.append("")
with open(a.out + ".md", "w") as fh:
    fh.write("\n".join(md))
print("wrote", a.out + ".md")
