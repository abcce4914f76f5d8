#!/usr/bin/env python
"""V smoothing (`la_v_colstats`, `la_v_colstats_finish`, `la_attn_unshift`) at the headline shape, one process: V and O of
(1, 75 600, 40, 128), bf16. Every new pass is timed INTERLEAVED with what it replaces - one launch sequence of each per iteration,
alternating, HIP events around each, medians; the whole set is run twice and the two ratios of a pair give the session's own spread:

  * `v_colstats` (statistics + finish) against the two passes it replaces: `qk_prep_colmean(norm=None)` plus the amax pass with shift;
  * `SmoothedV` current / delayed against `E4m3Scales` on V in the same mode;
  * `attn_unshift` - bf16 in place, fp32 out, each with and without the LSE - against the eager `(o.float() + shift).to(dtype)` plus
    `lse_unshift`, and its algorithmic bytes/s against `la_combine`'s (two bf16 partials -> bf16), the project's HBM yardstick.

Then the accuracy of the dense e4m3 attention call with and without V smoothing at offsets 0 / 4 / 16 on the input of
tests/test_gpu_v_smooth.py, for the three forms of P the device has, beside the emulation's (tests/v_smooth_emulation.py).
Writes `profiles/v_smooth.json` and `profiles/v_smooth.md` (`profiles/v_smooth_notes.md`, when present, is appended).

    python tools/v_smooth_bench.py [--seqlen 75600 --heads 40 --head-dim 128] [--out profiles/v_smooth] [--render-only]
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
ap.add_argument("--render-only", action="store_true", help="write the .md again from the saved .json (no device needed)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "v_smooth"), help="path without extension: .json and .md are written")
a = ap.parse_args()
S, H, D = a.seqlen, a.heads, a.head_dim
shape = (1, S, H, D)
BF, FP32 = torch.bfloat16, torch.float32


def measure():
    import liteattention_amd as L
    import v_smooth_emulation as emu
    from liteattention_amd import _cabi
    from liteattention_amd.flash_attn_interface import fwd_flags
    dev = torch.device("cuda", 0)

    def interleaved(new, old):
        """Medians (ms) of `new` and `old`, one call of each per iteration, alternating."""
        for _ in range(a.warmup):
            new()
            old()
        times = ([], [])
        for _ in range(a.iters):
            for fn, acc in ((new, times[0]), (old, times[1])):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                acc.append(e0.elapsed_time(e1))
        return statistics.median(times[0]), statistics.median(times[1])

    g = torch.Generator(device=dev).manual_seed(0)
    xv = (torch.randn(shape, device=dev, generator=g) + 4.0 * torch.randn(1, 1, H, D, device=dev, generator=g)).bfloat16()
    n_parts, part_rows = L.v_colstats_parts(S, H, D)
    stat = torch.empty(n_parts, 3, 1, H, D, device=dev)
    mean, amax = torch.empty(1, H, D, device=dev), torch.empty(1, H, device=dev)
    k_parts = L.qk_prep_smooth_parts(S, H, D)[0]
    colsum, mean_old, amax_old = torch.empty(k_parts, 1, H, D, device=dev), torch.empty(1, H, D, device=dev), torch.zeros(1, H, device=dev)

    def old_stats():
        L.qk_prep_colmean(xv, norm=None, colsum_part=colsum, out=mean_old)
        amax_old.zero_()
        L.qk_prep_smooth(xv, norm=None, shift=mean_old, amax_out=amax_old, quantize=False)

    res = {"shape": list(shape), "n_parts": n_parts, "rows_per_part": part_rows,
           "timing": f"HIP events around each call sequence, new and old alternating, {a.warmup} warm-up + {a.iters} timed of each, medians; "
                     "the whole set twice (run 1, run 2)",
           "device": torch.cuda.get_device_name(0), "build": _cabi.build_info().get("src"), "pairs": {}}
    v_bytes = xv.numel() * 2

    # la_combine at the same output shape: two bf16 partials + their LSE in, one bf16 output + LSE out
    part2 = torch.randn((2,) + shape, device=dev, generator=g).bfloat16()
    lse2 = torch.randn(2, 1, H, S, device=dev, generator=g)
    o_comb = torch.empty(shape, dtype=BF, device=dev)
    t_comb, _ = interleaved(lambda: L.flash_attn_combine(part2, lse2, out=o_comb), lambda: None)
    comb_bytes = part2.numel() * 2 + lse2.numel() * 4 + o_comb.numel() * 2 + H * S * 4
    res["la_combine"] = {"ms": round(t_comb, 4), "bytes": comb_bytes, "TBps": round(comb_bytes / t_comb / 1e9, 3)}
    print("la_combine", json.dumps(res["la_combine"]), flush=True)
    del part2, lse2, o_comb
    torch.cuda.empty_cache()

    sv = {m: L.SmoothedV(mode=m, margin=1.25) for m in ("current", "delayed")}
    es = {m: L.E4m3Scales(mode=m, margin=1.25) for m in ("current", "delayed")}
    for m in sv:                                                       # first calls: allocation, history
        sv[m](xv)
        es[m](xv, norm=None)

    o = torch.randn(shape, device=dev, generator=g).bfloat16()
    o_work = o.clone()
    out32 = torch.empty(shape, dtype=FP32, device=dev)
    shift = mean
    lse = torch.randn(1, H, S, device=dev, generator=g)
    dot = torch.randn(1, H, S, device=dev, generator=g)
    lse_work = lse.clone()
    scale = D ** -0.5
    o_bytes, lse_bytes = o.numel() * 2, lse.numel() * 4

    def eager(dtype, with_lse):
        r = (o.float() + shift[:, None]).to(dtype)
        return (r, L.lse_unshift(lse, dot, scale)) if with_lse else r

    pairs = {      # name: (new, old, algorithmic bytes of the new one)
        "v_colstats + finish vs qk_prep_colmean(norm=None) + amax pass with shift": (
            lambda: L.v_colstats(xv, stat_part=stat, mean_out=mean, amax_out=amax), old_stats, v_bytes),
        "SmoothedV current vs E4m3Scales current": (lambda: sv["current"](xv), lambda: es["current"](xv, norm=None), 2 * v_bytes + v_bytes // 2),
        "SmoothedV delayed vs E4m3Scales delayed": (lambda: sv["delayed"](xv), lambda: es["delayed"](xv, norm=None), 2 * v_bytes + v_bytes // 2),
        "attn_unshift bf16 in place vs eager": (lambda: L.attn_unshift(o_work, shift, out=o_work), lambda: eager(BF, False), 2 * o_bytes),
        "attn_unshift bf16 in place with LSE vs eager + lse_unshift": (
            lambda: L.attn_unshift(o_work, shift, lse=lse_work, lse_dot=dot, softmax_scale=scale, out=o_work, lse_out=lse_work),
            lambda: eager(BF, True), 2 * o_bytes + 3 * lse_bytes),
        "attn_unshift fp32 out vs eager": (lambda: L.attn_unshift(o, shift, out=out32), lambda: eager(FP32, False), 3 * o_bytes),
        "attn_unshift fp32 out with LSE vs eager + lse_unshift": (
            lambda: L.attn_unshift(o, shift, lse=lse, lse_dot=dot, softmax_scale=scale, out=out32, lse_out=lse_work),
            lambda: eager(FP32, True), 3 * o_bytes + 3 * lse_bytes),
    }
    for name in pairs:
        res["pairs"][name] = {"runs": []}
    for run in range(2):
        for name, (new, old, nbytes) in pairs.items():
            lse_work.copy_(lse)                                        # (an LSE restored in place over and over would run away)
            t_new, t_old = interleaved(new, old)
            rec = res["pairs"][name]
            rec["runs"].append({"new_ms": round(t_new, 4), "old_ms": round(t_old, 4), "ratio": round(t_new / t_old, 4)})
            rec["bytes"] = nbytes
            rec["TBps"] = round(nbytes / min(r["new_ms"] for r in rec["runs"]) / 1e9, 3)
            rec["TBps_over_la_combine"] = round(rec["TBps"] / res["la_combine"]["TBps"], 3)
            print(run, name, json.dumps(rec["runs"][-1]), "TB/s", rec["TBps"], flush=True)
    t_stat, _ = interleaved(lambda: L.v_colstats(xv, stat_part=stat, mean_out=mean, amax_out=amax), lambda: None)
    res["v_colstats_ms"] = round(t_stat, 4)
    # the two kernels of v_colstats apart: the finish alone, on the parts the launch above left
    lib = _cabi.load()
    import ctypes

    def finish_only():
        lib.la_v_colstats_finish(stat.data_ptr(), n_parts, 1, H, D, S, mean.data_ptr(), mean.stride(0), mean.stride(1), amax.data_ptr(),
                                 amax.stride(0), amax.stride(1), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    t_fin, _ = interleaved(finish_only, lambda: None)
    res["v_colstats_finish_ms"] = round(t_fin, 4)
    want = torch.zeros(1, H, device=dev)
    L.qk_prep_smooth(xv, norm=None, shift=mean, amax_out=want, quantize=False)
    res["amax_bit_equal_to_the_amax_pass"] = bool(torch.equal(amax.view(torch.int32), want.view(torch.int32)))
    del xv, o, o_work, out32, stat, colsum, sv, es
    torch.cuda.empty_cache()

    # accuracy end to end: B = 1, S = 320, H = 2, D = 128, +-offset on 8 channels of every V head (tests/test_gpu_v_smooth.py)
    forms = {"default (rounded P, fp32 row sums of the unrounded P)": 0, "mfma_rowsum (row sums of the rounded P)": _cabi.LA_FLAG_FP8_MFMA_ROWSUM,
             "encoded (block-scaled log-linear P)": _cabi.LA_FLAG_FP8_ENCODED_P}
    res["accuracy"] = {"device": {}, "emulation": {}}
    for offset in (0, 4, 16):
        q, k, v, o64, _ = (t.to(dev) for t in emu.case(offset))
        q8, dq = L.E4m3Scales()(q, norm=None)
        k8, dk = L.E4m3Scales()(k, norm=None)
        v8, dv = L.E4m3Scales()(v, norm=None)
        s = L.SmoothedV()
        s8, sdv, _ = s(v)
        for form, flag in forms.items():
            with fwd_flags(flag, clear=(_cabi.LA_FLAG_FP8_MFMA_ROWSUM | _cabi.LA_FLAG_FP8_ENCODED_P) & ~flag):
                o_p = L.flash_attn_func(q8, k8, v8, q_descale=dq, k_descale=dk, v_descale=dv)
                o_s, lse_s = L.flash_attn_func(q8, k8, s8, q_descale=dq, k_descale=dk, v_descale=sdv, return_softmax_lse=True)
            rec = {"plain": round(emu.rel_rms(o_p, o64), 5)}
            rec["smoothed_fp32"] = round(emu.rel_rms(s.finish(o_s, lse=lse_s, out_dtype=FP32), o64), 5)
            rec["smoothed_bf16"] = round(emu.rel_rms(s.finish(o_s, lse=lse_s), o64), 5)          # (in place: last)
            rec["ratio_bf16"], rec["ratio_fp32"] = round(rec["smoothed_bf16"] / rec["plain"], 4), round(rec["smoothed_fp32"] / rec["plain"], 4)
            res["accuracy"]["device"].setdefault(str(offset), {})[form] = rec
            print("offset", offset, form, json.dumps(rec), flush=True)
        for form, (rp, rs) in (("P in fp32", (False, False)), ("rounded P, fp32 row sums of the unrounded P", (True, False)),
                               ("rounded P, row sums of the rounded P", (True, True))):
            rb, plain, sb = emu.smoothing_ratio(offset, BF, rp, rs)
            rf, _, sf = emu.smoothing_ratio(offset, FP32, rp, rs)
            res["accuracy"]["emulation"].setdefault(str(offset), {})[form] = {
                "plain": round(plain, 5), "smoothed_bf16": round(sb, 5), "smoothed_fp32": round(sf, 5), "ratio_bf16": round(rb, 4),
                "ratio_fp32": round(rf, 4)}
    return res


if a.render_only:                                                  # the tables again from a saved run: no device needed
    res = json.load(open(a.out + ".json"))
else:
    res = measure()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

comb = res["la_combine"]
lines = ["# V smoothing: `la_v_colstats`, `la_attn_unshift`", "",
         f"Written by `tools/v_smooth_bench.py` on {res['device']} (library src {res['build']}), one process: V and O of {tuple(res['shape'])}, "
         f"bf16; {res['n_parts']} parts of {res['rows_per_part']} rows. {res['timing']}.", "",
         f"`la_combine` at the same output shape (two bf16 partials -> bf16), the HBM yardstick: {comb['ms']} ms, {comb['TBps']} TB/s of "
         "algorithmic bytes. Bytes of a new pass = what the algorithm must move (V read once for the statistics; read twice and the codes "
         "written for `SmoothedV`; O read and the result written, the LSE read twice and written, for `attn_unshift`).", "",
         "| new vs old | old ms (run 1, run 2) | new ms (run 1, run 2) | new / old (run 1, run 2) | new: TB/s | over `la_combine` |",
         "|---|---|---|---|---|---|"]
for name, rec in res["pairs"].items():
    r1, r2 = rec["runs"]
    lines.append(f"| {name} | {r1['old_ms']}, {r2['old_ms']} | {r1['new_ms']}, {r2['new_ms']} | {r1['ratio']}, {r2['ratio']} | {rec['TBps']} | "
                 f"{rec['TBps_over_la_combine']} |")
lines += ["", f"`v_colstats` alone (both kernels): {res['v_colstats_ms']} ms; `la_v_colstats_finish` alone: {res['v_colstats_finish_ms']} ms. Its "
          f"amax equals the amax pass with shift bit for bit on this input: {res['amax_bit_equal_to_the_amax_pass']}.", "",
          "## Error of the dense e4m3 attention call, against fp64 attention of the same bf16 inputs", "",
          "B = 1, S = 320, H = 2, D = 128, +-offset on 8 channels of every V head (the input of tests/test_gpu_v_smooth.py): relative rms "
          "error of O with `E4m3Scales` on V (plain) and with `SmoothedV`, the result handed on in bf16 or in fp32.", "",
          "| offset | where | form of P | plain | smoothed, bf16 | smoothed, fp32 | ratio bf16 | ratio fp32 |", "|---|---|---|---|---|---|---|---|"]
for where in ("device", "emulation"):
    for off, forms in res["accuracy"][where].items():
        for form, rec in forms.items():
            lines.append(f"| {off} | {where} | {form} | {rec['plain']} | {rec['smoothed_bf16']} | {rec['smoothed_fp32']} | {rec['ratio_bf16']} | "
                         f"{rec['ratio_fp32']} |")
notes = os.path.join(ROOT, "profiles", "v_smooth_notes.md")           # the interpretation, kept apart from the numbers
if os.path.exists(notes):
    lines += ["", open(notes).read().rstrip()]
with open(a.out + ".json", "w") as fh:
    json.dump(res, fh, indent=1)
with open(a.out + ".md", "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", a.out + ".json", a.out + ".md")
