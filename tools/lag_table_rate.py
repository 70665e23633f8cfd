#!/usr/bin/env python3
"""Time of the lagged-gain table of one recording (raptor_amd.probing.lag_gains, csrc/rq_lag_table.inc), beside the feedback-gain
table of the same recording on the same GPU:
(a) lag_gains at --lags lags: the state-saving forward and one reverse sweep, one wave per 16 envs, sum [K, 4, 16, N] and count
    [K, N] in device memory;
(b) feedback_gains with one bucket: lag 0 alone, one forward walk, one wave per 64 envs.
Per 16 envs and step (a) issues 30 MFMAs of recompute and 48 (2 K - 1) of adjoint products, (b) 30 + 48: the file records the ratio
these counts predict beside the measured one and assumes neither.  The student is the shipped policy with perturbed weights.

Each timed region is bracketed by a device synchronise (torch's and the engine's) with the host's perf_counter in between; the two
calls alternate for --rounds rounds after one warm-up each; medians are reported, every round is kept.

    python tools/lag_table_rate.py [--envs 65536] [--steps 500] [--lags 16] [--rounds 5] [--json profiles/lag_table_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                                   # noqa: E402
from bench import Shard                                        # noqa: E402
from raptor_amd import probing                                 # noqa: E402
from raptor_amd.build import LIB, library_sha256               # noqa: E402
from raptor_amd.foundation_policy import Raptor                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--lags", type=int, default=16)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()
N, T, K = args.envs, args.steps, args.lags

device = l2f.Device()


def sync():
    torch.cuda.synchronize()
    device.synchronize()


def measure(fn):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return (time.perf_counter() - t0) * 1e3, out


sh = Shard(device, N, 0)
traj = sh.vector.Trajectory(sh.env, T)
sh.vector.rollout(device, sh.env, sh.params, sh.state, sh.policy, sh.rng, T, "fused", autoreset=True, trajectory=traj)
w = sh.policy.weights
w = (w + np.random.default_rng(0).standard_normal(w.size).astype(np.float32) * 0.02).astype(np.float32)
student = Raptor(device, weights=w)
student.reset()


def lag_path():
    return probing.lag_gains(traj, student, n_lags=K)


def gain_path():
    return probing.feedback_gains(traj, student)


lag_path(), gain_path()                                        # warm-up: code objects, workspaces, the allocator's blocks
rows = []
for r in range(args.rounds):
    a, lag = measure(lag_path)
    b, gain = measure(gain_path)
    rows.append(dict(round=r, lag_gains_ms=a, feedback_gains_ms=b))
    print(f"round {r}: lag_gains {a:.2f} ms; feedback_gains {b:.2f} ms", flush=True)
med = {k: float(np.median([x[k] for x in rows])) for k in rows[0] if k != "round"}
g_lag, g_gain = lag.by_lag().cpu().numpy()[0], gain.by_age().cpu().numpy()[0]
live_steps = int(lag.count[0].sum())
instantiation = 4 if K <= 4 else 8 if K <= 8 else 16
res = dict(gpu=torch.cuda.get_device_name(0), library_sha256=library_sha256(LIB),
           clock="host time.perf_counter between device synchronisations (torch.cuda.synchronize and the engine's stream)",
           envs=N, steps=T, lags=K, instantiation=instantiation, rounds=rows,
           lag_gains_ms_median=med["lag_gains_ms"], feedback_gains_ms_median=med["feedback_gains_ms"],
           ratio_lag_gains_over_feedback_gains=med["lag_gains_ms"] / med["feedback_gains_ms"],
           ratio_expected_from_mfma_counts=(30 + 48 * (2 * K - 1)) / (30 + 48),
           env_steps_per_second_at_median=N * T / (med["lag_gains_ms"] * 1e-3),
           adjoint_tflops_at_median=live_steps * 48 * (2 * K - 1) * 2048 / 16 / (med["lag_gains_ms"] * 1e-3) / 1e12,
           counts_at_lag_0_equal=bool(torch.equal(lag.count[0], gain.count[0])),
           lag_0_max_relative_difference_to_feedback_gains=float(np.abs(g_lag - g_gain).max() / np.abs(g_gain).max()))
print(json.dumps(res))
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
