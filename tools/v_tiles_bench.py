#!/usr/bin/env python
"""fp8 V in one pass (`la_v_prep_tiles`) at the headline shape, one process: V of (1, 75 600, 40, 128), bf16.

  (a) what the pass replaces: the quantizing pass `qk_prep_smooth(v, norm=None, shift=, descale=)` plus `la_fwd`'s prepare pass over its
      e4m3 result. The prepare time is the difference of one raw e4m3 `la_fwd` (256 query rows against all the keys, so that the
      forward itself is small) without and with LA_FLAG_V_PREPARED on the same inputs and the same workspace;
  (b) the fused pass `v_prep_tiles` with the same shift and descale;
  (c) one `SmoothedV` + e4m3 attention call end to end (S x S, the restoring pass included) with `tiles` off and on.

Timing: HIP events around WINDOWS of back-to-back calls, each window at least `--window` seconds long (the call count comes from a
calibration window), windows of the two routes of a pair alternating, medians of `--rounds` windows; the whole set is run twice in the
process (run 1, run 2) and the difference of the two is the session's own spread. GB/s is against the bytes a route must move.
Writes `profiles/v_tiles.json` and `profiles/v_tiles.md`.

    python tools/v_tiles_bench.py [--seqlen 75600 --heads 40 --head-dim 128] [--out profiles/v_tiles] [--render-only]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--seqlen", type=int, default=75600)
ap.add_argument("--heads", type=int, default=40)
ap.add_argument("--head-dim", type=int, default=128)
ap.add_argument("--window", type=float, default=0.3, help="least length of a timed window, seconds")
ap.add_argument("--rounds", type=int, default=3, help="windows per route and run")
ap.add_argument("--render-only", action="store_true", help="write the .md again from the saved .json (no device needed)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "v_tiles"), help="path without extension: .json and .md are written")
a = ap.parse_args()
S, H, D = a.seqlen, a.heads, a.head_dim
F8 = torch.float8_e4m3fn


def measure():
    import liteattention_amd as L
    from liteattention_amd import _cabi
    from liteattention_amd import flash_attn_interface as fai
    dev = torch.device("cuda", 0)
    lib = _cabi.load()

    def window(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n                                 # ms per call

    def calls_per_window(fn):
        fn()
        fn()                                                           # warm-up
        return max(2, int(a.window * 1e3 / window(fn, 4)) + 1)

    def alternating(f_old, f_new):
        """Medians (ms per call) of `rounds` windows of each route, the windows alternating."""
        n_old, n_new = calls_per_window(f_old), calls_per_window(f_new)
        t_old, t_new = [], []
        for _ in range(a.rounds):
            t_old.append(window(f_old, n_old))
            t_new.append(window(f_new, n_new))
        return statistics.median(t_old), statistics.median(t_new), n_old, n_new

    g = torch.Generator(device=dev).manual_seed(0)
    xv = (torch.randn((1, S, H, D), device=dev, generator=g) + 4.0 * torch.randn(1, 1, H, D, device=dev, generator=g)).bfloat16()
    mean, amax = L.v_colstats(xv)
    dv = L.descale_from_amax(amax, 1.25)
    v8 = torch.empty((1, S, H, D), dtype=F8, device=dev)
    tiles, ws = L.v_tiles_bytes(1, H, S, D)
    pv = L.PreparedV(torch.empty(ws, dtype=torch.uint8, device=dev), (1, S, H, D))

    def quantize():
        L.qk_prep_smooth(xv, norm=None, shift=mean, descale=dv, out=v8)

    def fused():
        L.v_prep_tiles(xv, shift=mean, descale=dv, out=pv)

    # the raw forward of (a): 256 query rows, all the keys, its own workspace; only the flag differs between the two
    q_s = torch.randn((1, 256, H, D), device=dev, generator=g).to(F8)
    k8 = torch.randn((1, S, H, D), device=dev, generator=g).to(F8)
    o_s = torch.empty((1, 256, H, D), dtype=torch.bfloat16, device=dev)
    lse_s = torch.empty((1, H, 256), dtype=torch.float32, device=dev)
    quantize()
    bm, bn = _cabi.get_tile_sizes(D, 1)
    args = fai._fwd_args(q_s, k8, v8, o_s, lse_s, (None, None, dv), 1, 256, S, D ** -0.5, bm, bn)
    need = lib.la_fwd_workspace_bytes(ctypes.byref(args))
    assert need == ws, (need, ws)
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    args.workspace, args.workspace_bytes = work.data_ptr(), need
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd(flags):
        args.flags = flags
        rc = lib.la_fwd(ctypes.byref(args), stream)
        assert rc == 0, _cabi.status_string(rc)

    fwd(0)
    fused()
    torch.cuda.synchronize()
    same = bool(torch.equal(work[:tiles], pv.workspace[:tiles]))

    # (c): the whole call
    q8 = torch.randn((1, S, H, D), device=dev, generator=g).to(F8)
    sv = {False: L.SmoothedV(margin=1.25), True: L.SmoothedV(margin=1.25, tiles=True)}

    def end_to_end(tiles_on):
        v, d, shift = sv[tiles_on](xv)
        o, lse = L.flash_attn_func(q8, k8, v, v_descale=d, return_softmax_lse=True)
        return sv[tiles_on].finish(o, lse=lse, out_dtype=torch.float32)

    o_off = end_to_end(False).clone()
    same_o = bool(torch.equal(o_off, end_to_end(True)))
    del o_off

    x_bytes, c_bytes = xv.numel() * 2, xv.numel()
    res = {"shape": [1, S, H, D], "device": torch.cuda.get_device_name(0), "build": _cabi.build_info().get("src"),
           "timing": f"HIP events around windows of back-to-back calls, each at least {a.window} s, windows of the two routes alternating, "
                     f"medians of {a.rounds} windows; the whole set twice in one process (run 1, run 2)",
           "tile_bytes": tiles, "tiles_bit_equal": same, "end_to_end_o_bit_equal": same_o,
           "bytes": {"two_passes": x_bytes + 2 * c_bytes + tiles, "fused": x_bytes + tiles}, "runs": []}
    for run in range(2):
        t_q, t_f, n_q, n_f = alternating(quantize, fused)
        t_plain, t_prep, n_plain, n_prep = alternating(lambda: fwd(0), lambda: fwd(_cabi.LA_FLAG_V_PREPARED))
        t_off, t_on, n_off, n_on = alternating(lambda: end_to_end(False), lambda: end_to_end(True))
        rec = {"quantize_ms": round(t_q, 4), "fused_ms": round(t_f, 4), "fwd_ms": round(t_plain, 4), "fwd_prepared_ms": round(t_prep, 4),
               "prepare_ms": round(t_plain - t_prep, 4), "two_passes_ms": round(t_q + t_plain - t_prep, 4),
               "end_to_end_off_ms": round(t_off, 4), "end_to_end_on_ms": round(t_on, 4),
               "calls_per_window": [n_q, n_f, n_plain, n_prep, n_off, n_on]}
        res["runs"].append(rec)
        print(run, json.dumps(rec), flush=True)
    return res


if a.render_only:
    res = json.load(open(a.out + ".json"))
else:
    res = measure()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

r1, r2 = res["runs"]
b2, b1 = res["bytes"]["two_passes"], res["bytes"]["fused"]


def pair(key, digits=4):
    return f"{r1[key]:.{digits}f}, {r2[key]:.{digits}f}"


def gbps(nbytes, key):
    return f"{nbytes / r1[key] / 1e6:.0f}, {nbytes / r2[key] / 1e6:.0f}"


spread_a, spread_b = abs(r1["two_passes_ms"] - r2["two_passes_ms"]), abs(r1["fused_ms"] - r2["fused_ms"])
gain = min(r1["two_passes_ms"], r2["two_passes_ms"]) - max(r1["fused_ms"], r2["fused_ms"])
lines = ["# fp8 V in one pass: `la_v_prep_tiles`", "",
         f"Written by `tools/v_tiles_bench.py` on {res['device']} (library src {res['build']}), one process: V of {tuple(res['shape'])}, bf16, "
         f"shift = its mean, descale from its amax. {res['timing']}.", "",
         f"Tile region: {res['tile_bytes']} bytes. The fused pass left the bytes of the two passes there: {res['tiles_bit_equal']}; the "
         f"end-to-end O of the two routes is bit-equal: {res['end_to_end_o_bit_equal']}.", "",
         "| | ms (run 1, run 2) | bytes it must move | GB/s (run 1, run 2) |", "|---|---|---|---|",
         f"| quantizing pass (`qk_prep_smooth`, norm=None): read bf16, write e4m3 | {pair('quantize_ms')} | | |",
         f"| `la_fwd` 256 rows x all keys, prepare pass inside | {pair('fwd_ms')} | | |",
         f"| the same under LA_FLAG_V_PREPARED | {pair('fwd_prepared_ms')} | | |",
         f"| prepare pass = their difference: read e4m3, write tiles | {pair('prepare_ms')} | | |",
         f"| (a) quantize + prepare | {pair('two_passes_ms')} | {b2} | {gbps(b2, 'two_passes_ms')} |",
         f"| (b) `v_prep_tiles`: read bf16, write tiles | {pair('fused_ms')} | {b1} | {gbps(b1, 'fused_ms')} |",
         f"| (c) `SmoothedV` + attention + restore, `tiles=False` | {pair('end_to_end_off_ms', 3)} | | |",
         f"| (c) the same, `tiles=True` | {pair('end_to_end_on_ms', 3)} | | |", "",
         f"Spread between the two runs: (a) {spread_a:.4f} ms, (b) {spread_b:.4f} ms. The slower run of (b) is "
         f"{abs(gain):.4f} ms {'below' if gain > 0 else 'ABOVE'} the faster run of (a)"
         + (": more than either spread." if gain > max(spread_a, spread_b) else ": NOT more than the spread."),
         f"End to end the call changes by {r1['end_to_end_off_ms'] - r1['end_to_end_on_ms']:.3f} / "
         f"{r2['end_to_end_off_ms'] - r2['end_to_end_on_ms']:.3f} ms (off - on; run 1 / run 2), against a spread of "
         f"{abs(r1['end_to_end_off_ms'] - r2['end_to_end_off_ms']):.3f} ms (off) and {abs(r1['end_to_end_on_ms'] - r2['end_to_end_on_ms']):.3f} ms "
         "(on) between the runs.",
         f"Memory: the route with `tiles=True` never allocates the e4m3 V ({res['shape'][1] * res['shape'][2] * res['shape'][3]} bytes) and the "
         f"attention call allocates no workspace ({res['tile_bytes'] + 1024} bytes per call otherwise); it runs one kernel fewer."]
notes = os.path.join(ROOT, "profiles", "v_tiles_notes.md")            # the interpretation, kept apart from the numbers
if os.path.exists(notes):
    lines += ["", open(notes).read().rstrip()]
with open(a.out + ".json", "w") as fh:
    json.dump(res, fh, indent=1)
with open(a.out + ".md", "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", a.out + ".json", a.out + ".md")
