#!/usr/bin/env python3
"""What tracking a moving setpoint costs the fused rollout: tracked (vector.rollout(..., reference=ref)) against untracked launches of
the SAME build on the same objects, alternating, the median of each side's timed launches -> profiles/tracking_rate.json.
    python tools/tracking_rate.py [--envs 65536] [--steps 500] [--launches 5] [--precision fp32] [--out profiles/tracking_rate.json]
The reference is a figure-eight over the whole episode (raptor_amd.tracking.lissajous): lanes of a wave are at different rows as
soon as episodes end at different steps, which is the per-lane load the kernel pays for.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raptor_amd.l2f as l2f                       # noqa: E402
from raptor_amd import build, tracking             # noqa: E402
from bench import Shard                            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--launches", type=int, default=5)
ap.add_argument("--precision", default="fp32")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracking_rate.json"))
args = ap.parse_args()

device = l2f.Device()
sh = Shard(device, args.envs, 0, precision=args.precision)
v = sh.vector
limit = int(sh.env.config.episode_step_limit)
ref = l2f.Reference(device, tracking.lissajous(limit, float(sh.env.config.dt), amplitude=(0.3, 0.15, 0.0), period=5.0))


def launch(tracked):
    device.timer_start()
    v.rollout(device, sh.env, sh.params, sh.state, sh.policy, sh.rng, args.steps, "fused", autoreset=True,
              reference=ref if tracked else None)
    return device.timer_stop()


for _ in range(6):                                 # clocks, and both kernels' code loaded
    launch(False)
    launch(True)
ms = {False: [], True: []}
for _ in range(args.launches):                     # alternating: a drift of the clock meets both sides alike
    for tracked in (False, True):
        ms[tracked].append(launch(tracked))
work = args.envs * args.steps
med = {k: statistics.median(x) for k, x in ms.items()}
rec = {"envs": args.envs, "steps": args.steps, "launches_per_side": args.launches, "precision": args.precision,
       "timer": "HIP events around one launch on the engine's stream (Device.timer_start / timer_stop)",
       "untracked_ms": [round(x, 4) for x in ms[False]], "tracked_ms": [round(x, 4) for x in ms[True]],
       "untracked_env_steps_per_s": work / (med[False] * 1e-3), "tracked_env_steps_per_s": work / (med[True] * 1e-3),
       "untracked_us_per_step": med[False] * 1e3 / args.steps, "tracked_us_per_step": med[True] * 1e3 / args.steps,
       "tracked_over_untracked_time": med[True] / med[False],
       "tracking_rmse_quantiles_m": [float(q) for q in __import__("numpy").nanquantile(sh.env.tracking_rmse(), [0.5, 0.9, 0.99])],
       "library_sha256": build.library_sha256()}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec))
