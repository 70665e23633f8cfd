#!/usr/bin/env python3
"""The foundation policy at a flight controller's rate.  It was trained at 100 Hz; the reference's deployment notes run it at 400 Hz
and let its recurrent state move on every 4th step only.  Here the same sampled quadrotors (same seed) fly 5 s three ways:
    100 Hz, native interval 1        the rate of training
    400 Hz, native interval 4        the deployment mode (dt = 0.0025, episode_step_limit = 2000)
    400 Hz, native interval 1        the mistake: the recurrence advances four times too fast
    python examples/deployment_rate.py [--envs 4096] [--figure-eight]
Prints the share terminated, the mean episode length in seconds and the final position error of each; with --figure-eight the
quadrotors follow a setpoint (raptor_amd.tracking.lissajous sampled at the simulated dt) and the tracking RMSE is printed too.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                       # noqa: E402
from raptor_amd import tracking                    # noqa: E402
from raptor_amd.foundation_policy import Raptor    # noqa: E402

WAYS = (("100 Hz, R = 1", 0.01, 1), ("400 Hz, R = 4", 0.0025, 4), ("400 Hz, R = 1 (the mistake)", 0.0025, 1))


def fly(device, n_envs, dt, interval, seconds=5.0, figure_eight=False, seed=0):
    """One episode of `seconds` for n_envs domain-randomised quadrotors -> the statistics as a dict."""
    steps = int(round(seconds / dt))
    vector = l2f.vector(n_envs)
    rng, env = vector.VectorRng(), vector.VectorEnvironment()
    params, state = vector.VectorParameters(), vector.VectorState()
    vector.initialize_rng(device, rng, seed)
    vector.initialize_environment(device, env)
    cfg = env.config
    cfg.dt, cfg.episode_step_limit = dt, steps
    if figure_eight:
        cfg.init_guidance = 1.0                    # hover at the origin, where the path starts
    env.config = cfg
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    policy = Raptor(device, native_interval=interval)
    policy.reset()
    ref = table = None
    if figure_eight:
        table = tracking.lissajous(steps, dt, amplitude=(0.3, 0.15, 0.0), period=5.0)
        ref = l2f.Reference(device, table)
    vector.rollout(device, env, params, state, policy, rng, steps, mode="fused", autoreset=False, reference=ref)
    target = table[-1, :3] if figure_eight else np.zeros(3, np.float32)
    flew = env.finished_terminated() == 0
    out = {"dt": dt, "native_interval": interval, "steps": steps, "envs": n_envs,
           "terminated": float(1.0 - flew.mean()),
           "mean_episode_seconds": float(env.finished_lengths().mean() * dt),
           "final_position_error_m": float(np.linalg.norm(state.numpy()[flew, :3] - target, axis=1).mean()) if flew.any() else None}
    if figure_eight:
        out["tracking_rmse_m"] = float(np.median(env.tracking_rmse()[flew])) if flew.any() else None
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--figure-eight", action="store_true")
    args = ap.parse_args()
    device = l2f.Device()
    print(f"{args.envs} sampled quadrotors, 5 s" + (", figure-eight 0.3 m x 0.15 m, period 5 s" if args.figure_eight else ", holding the origin"))
    for name, dt, interval in WAYS:
        r = fly(device, args.envs, dt, interval, figure_eight=args.figure_eight)
        err = "-" if r["final_position_error_m"] is None else f"{r['final_position_error_m']:.4f} m"
        line = f"  {name:28s} terminated {r['terminated']:.3f}  mean episode {r['mean_episode_seconds']:.3f} s  final position error {err}"
        if args.figure_eight and r["tracking_rmse_m"] is not None:
            line += f"  tracking RMSE (median) {r['tracking_rmse_m']:.4f} m"
        print(line)
