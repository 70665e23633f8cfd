#!/usr/bin/env python3
"""Sampled quadrotors fly a figure-eight, entirely on the device: the foundation policy is a position controller, so it tracks a
moving setpoint when it is shown position and velocity relative to it - ``vector.rollout(..., reference=ref)`` does that inside the
fused kernel, each env reading the row of its own episode step count.
    python examples/track_figure_eight.py [--envs 4096] [--period 5.0] [--amplitude 0.3]
Prints the quantiles of the per-env RMS distance to the setpoint over one 500-step episode, beside what hovering at the origin
would score (the RMS of |p_ref|).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                       # noqa: E402
from raptor_amd import tracking                    # noqa: E402
from raptor_amd.foundation_policy import Raptor    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--period", type=float, default=5.0)
ap.add_argument("--amplitude", type=float, default=0.3)
args = ap.parse_args()

device = l2f.Device()
vector = l2f.vector(args.envs)
rng, env = vector.VectorRng(), vector.VectorEnvironment()
params, state = vector.VectorParameters(), vector.VectorState()
vector.initialize_rng(device, rng, 0)
vector.initialize_environment(device, env)
cfg = env.config
cfg.init_guidance = 1.0                            # every quadrotor starts in hover at the origin, where the path starts
env.config = cfg
vector.sample_initial_parameters(device, env, params, rng)      # domain-randomised quadrotors
vector.sample_initial_state(device, env, params, state, rng)
policy = Raptor(device)
policy.reset()

steps = int(cfg.episode_step_limit)
table = tracking.lissajous(steps, float(cfg.dt), amplitude=(args.amplitude, args.amplitude / 2, 0.0), period=args.period)
assert np.abs(table[:, :3]).max() < cfg.termination_position, "termination looks at the absolute position: keep the path inside"
ref = l2f.Reference(device, table)
vector.rollout(device, env, params, state, policy, rng, steps, mode="fused", autoreset=False, reference=ref)

rmse = env.tracking_rmse()
flew = env.finished_terminated() == 0
hover = float(np.sqrt((table[:, :3].astype(np.float64) ** 2).sum(axis=1).mean()))
q = np.quantile(rmse[flew], [0.1, 0.5, 0.9, 0.99])
print(f"{args.envs} quadrotors, figure-eight {args.amplitude} m x {args.amplitude / 2} m, period {args.period} s, {steps} steps")
print(f"  completed the episode: {flew.mean():.3f}")
print(f"  RMS distance to the setpoint [m]  p10 {q[0]:.3f}  median {q[1]:.3f}  p90 {q[2]:.3f}  p99 {q[3]:.3f}")
print(f"  hovering at the origin would score {hover:.3f} m")
