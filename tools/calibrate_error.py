#!/usr/bin/env python
"""Error-bounded threshold schedule on tools.selfcheck.DenoiseWorkload: `calibrate_error_schedule` (liteattention_amd/calibration.py)
against the best CONSTANT threshold of a stated grid under the same per-step bounds.

Bounds (the rule of tests/error_schedule_common.py, scaled to any number of steps): e_hi[t] = relative L1 error (worst head, against
the dense output of the same step, `output_error` on the device) of the constant threshold --hi-thr (default -0.001, which drops
about all that can be dropped) at step t; bounds[t] = f(t) * e_hi[t] with f rising linearly from --f-first (0.1) at step 1 to
--f-last (0.5) at the last step: stricter early, looser late, as the reference's README asks ("stricter bounds for earlier
timesteps"). Step 0 reads the list of all tiles: bounds[0] = 2^-7 (one bf16 ulp per element).

    python tools/calibrate_error.py [--frames 3 --per 1200 --heads 8 --steps 6] [--headline] [--out profiles/error_schedule.json]

Default size: S = 3 600, 8 heads, 6 steps - seconds on the GPU. --headline: the Wan2.1 shape (S = 75 600, 40 heads), minutes.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import liteattention_amd as L                                                                  # noqa: E402
from liteattention_amd.calibration import LiteAttentionBackend, calibrate_error_schedule        # noqa: E402
from tools.selfcheck import DenoiseWorkload                                                     # noqa: E402

GRID = (-6.0, -5.0, -4.5, -4.0, -3.5, -3.0, -2.5, -2.0)

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=3)
ap.add_argument("--per", type=int, default=1200, help="tokens per frame")
ap.add_argument("--heads", type=int, default=8)
ap.add_argument("--steps", type=int, default=6)
ap.add_argument("--headline", action="store_true", help="21 frames x 3 600 tokens, 40 heads (the Wan2.1 shape)")
ap.add_argument("--hi-thr", type=float, default=-1e-3)
ap.add_argument("--f-first", type=float, default=0.1)
ap.add_argument("--f-last", type=float, default=0.5)
ap.add_argument("--iters", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "error_schedule.json"))
a = ap.parse_args()
if a.headline:
    a.frames, a.per, a.heads = 21, 3600, 40
if a.steps < 2:
    ap.error("--steps: at least 2")

dev = torch.device("cuda", 0)
Workload = type("Workload", (DenoiseWorkload,), {"FRAMES": a.frames, "PER": a.per})            # the generator at another size
wl = Workload(a.heads, dev, steps=a.steps, sink=min(640, a.per // 2))
be = LiteAttentionBackend(wl.qkv)
t0 = time.time()


def run(thresholds):
    """Every step at thresholds[t] from a fresh state: errors against dense, skip fraction of the list each step read."""
    be.reset()
    errs, skips = [], []
    for t in range(a.steps):
        skips.append(be.skip_fraction())
        errs.append(be.error(be.step(t, thresholds[t]), be.dense(t)))
    return errs, skips


e_hi, skip_hi = run([a.hi_thr] * a.steps)
f = [a.f_first + (a.f_last - a.f_first) * (t - 1) / max(1, a.steps - 2) for t in range(1, a.steps)]
bounds = [2.0 ** -7] + [fi * e for fi, e in zip(f, e_hi[1:])]
thresholds, trace = calibrate_error_schedule(wl.qkv, a.steps, bounds, iters=a.iters, backend=be)
t_cal = time.time() - t0
errs, skips = run(thresholds)
constants = []
for thr in GRID:
    ce, cs = run([thr] * a.steps)
    constants.append({"thr": thr, "meets_all_bounds": all(e <= b for e, b in zip(ce, bounds)), "errors": ce, "skip_last_read_list": cs[-1]})
ok = [c for c in constants if c["meets_all_bounds"]]
best = max(ok, key=lambda c: c["skip_last_read_list"]) if ok else None
res = {
    "what": f"calibrate_error_schedule on DenoiseWorkload (anchored), S = {wl.S}, H = {a.heads}, {a.steps} steps, tiles {L.get_tile_sizes(128, 2)}; "
            "metric rel_l1 per head against the dense output of the step, worst head",
    "bound_rule": f"bounds[0] = 2^-7; bounds[t] = f(t) * e_hi[t], f linear {a.f_first} -> {a.f_last}, e_hi = the errors of constant thr {a.hi_thr}",
    "e_hi": e_hi, "skip_hi": skip_hi, "bounds": bounds, "schedule": thresholds, "trace": trace,
    "replay": {"errors": errs, "skip_read_list": skips, "meets_all_bounds": all(e <= b for e, b in zip(errs, bounds))},
    "constant_grid": constants, "best_constant": best,
    "skip_last_read_list": {"schedule": skips[-1], "best_constant": None if best is None else best["skip_last_read_list"]},
    "seconds": {"calibration": round(t_cal, 1), "total": round(time.time() - t0, 1)},
}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps({k: res[k] for k in ("schedule", "bounds", "replay", "best_constant", "skip_last_read_list", "seconds")}))
print("wrote", a.out)
