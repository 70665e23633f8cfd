#!/usr/bin/env python3
"""What tracking a moving setpoint costs the fused rollout, and what a reference per env costs on top: launches of the SAME build on
the same objects, alternating over the sides, the median of each side's timed launches -> profiles/tracking_rate.json.
    python tools/tracking_rate.py [--envs 65536] [--steps 500] [--launches 7] [--precision fp32] [--out profiles/tracking_rate.json]
                                  [--single-only] [--parent FILE ...] [--repeat FILE ...]
The sides: untracked; tracked (vector.rollout(..., reference=ref), one figure-eight over the whole episode,
raptor_amd.tracking.lissajous: lanes of a wave are at different rows as soon as episodes end at different steps, which is the
per-lane load the kernel pays for); and, unless --single-only, a ReferenceBank of M = 1, of M = 16 with the ids dealt per lane
(neighbouring lanes read different tables) and of M = 16 with the ids sorted by wave (a wave reads one table).  The 16 tables are
figure-eights of 16 periods.
--single-only is also what measures ANOTHER build's single-reference rollout in the same session (RAPTOR_QUAD_LIB=<its library>
RAPTOR_QUAD_ABI_ANY=1): --parent takes the files such runs of the parent commit's build wrote, --repeat those of repeated runs of
this build, and the record then holds this build's tracked launch against the parent's with the spread between the parent's own
repeated measurements as the margin.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raptor_amd.l2f as l2f                       # noqa: E402
from raptor_amd import _lib, build, tracking             # noqa: E402
from bench import Shard                            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--launches", type=int, default=7)
ap.add_argument("--precision", default="fp32")
ap.add_argument("--single-only", action="store_true")
ap.add_argument("--parent", nargs="*", default=[])
ap.add_argument("--repeat", nargs="*", default=[])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracking_rate.json"))
args = ap.parse_args()
M = 16

device = l2f.Device()
sh = Shard(device, args.envs, 0, precision=args.precision)
v = sh.vector
limit = int(sh.env.config.episode_step_limit)
dt = float(sh.env.config.dt)
eight = tracking.lissajous(limit, dt, amplitude=(0.3, 0.15, 0.0), period=5.0)
ref = l2f.Reference(device, eight)
sides = {"untracked": {}, "tracked": dict(reference=ref)}
if not args.single_only:
    many = l2f.ReferenceBank(device, [tracking.lissajous(limit, dt, amplitude=(0.3, 0.15, 0.0), period=4.0 + 0.5 * k) for k in range(M)])
    per_lane = tracking.spread_reference_ids(args.envs, M)
    sides["bank_1"] = dict(reference=l2f.ReferenceBank(device, [eight]), reference_ids=np.zeros(args.envs, np.uint32))
    sides["bank_16_per_lane"] = dict(reference=many, reference_ids=per_lane)
    sides["bank_16_by_wave"] = dict(reference=many, reference_ids=np.ascontiguousarray((np.arange(args.envs) // 64 % M).astype(np.uint32)))


def launch(side):
    # a one-step launch first, outside the timer: the sides share the env, whose per-env first rows are built for ONE (bank, ids) at a
    # time - the timed launch then finds them in place, as a loop of rollouts with one assignment does (every side pays the step alike)
    v.rollout(device, sh.env, sh.params, sh.state, sh.policy, sh.rng, 1, "fused", autoreset=True, **sides[side])
    device.timer_start()
    v.rollout(device, sh.env, sh.params, sh.state, sh.policy, sh.rng, args.steps, "fused", autoreset=True, **sides[side])
    return device.timer_stop()


for _ in range(6):                                 # clocks, every kernel's code loaded
    for side in sides:
        launch(side)
ms = {side: [] for side in sides}
for _ in range(args.launches):                     # alternating: a drift of the clock meets every side alike
    for side in sides:
        ms[side].append(launch(side))
work = args.envs * args.steps
med = {k: statistics.median(x) for k, x in ms.items()}
rec = {"envs": args.envs, "steps": args.steps, "launches_per_side": args.launches, "precision": args.precision,
       "timer": "HIP events around one launch on the engine's stream (Device.timer_start / timer_stop)",
       "untracked_ms": [round(x, 4) for x in ms["untracked"]], "tracked_ms": [round(x, 4) for x in ms["tracked"]],
       "untracked_env_steps_per_s": work / (med["untracked"] * 1e-3), "tracked_env_steps_per_s": work / (med["tracked"] * 1e-3),
       "untracked_us_per_step": med["untracked"] * 1e3 / args.steps, "tracked_us_per_step": med["tracked"] * 1e3 / args.steps,
       "tracked_over_untracked_time": med["tracked"] / med["untracked"],
       "tracking_rmse_quantiles_m": [float(q) for q in np.nanquantile(sh.env.tracking_rmse(), [0.5, 0.9, 0.99])]}
for side in sides:
    if side.startswith("bank"):
        rec[side + "_ms"] = [round(x, 4) for x in ms[side]]
        rec[side + "_over_tracked_time"] = med[side] / med["tracked"]
if args.parent:
    runs = {k: [statistics.median(json.load(open(f))["tracked_ms"]) for f in files] for k, files in (("parent", args.parent), ("this", args.repeat))}
    runs["this"].append(med["tracked"])
    rec["single_reference_against_parent"] = {
        "what": "median tracked launch (ms) of each run, the parent commit's build and this one alternating in one session",
        "parent_runs_ms": [round(x, 4) for x in runs["parent"]], "this_runs_ms": [round(x, 4) for x in runs["this"]],
        "parent_spread_ms": round(max(runs["parent"]) - min(runs["parent"]), 4),
        "this_median_minus_parent_median_ms": round(statistics.median(runs["this"]) - statistics.median(runs["parent"]), 4)}
rec["library_sha256"] = build.library_sha256(_lib.LIB_PATH)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec))
