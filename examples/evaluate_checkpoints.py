#!/usr/bin/env python3
"""Fly a bank of student checkpoints - one per wave, 64 quadrotors each - for one episode length in ONE fused launch and print every
policy's closed-loop record: what a checkpoint of a post-training run is picked by (return, episode length, share terminated).

    python examples/evaluate_checkpoints.py [--policies 1000] [--blocks 1] [--checkpoints DIR] [--sigma 0.05] [--show 10] [--mode fused|chained]
                                            [--native-interval R [R ...]] [--dt SECONDS] [--figure-eight | --suite]

At deployment conditions: --dt 0.0025 --native-interval 4 flies every checkpoint at 400 Hz with its hidden state moving every 4th step
(the episode stays 5 s: 2 000 steps); several values of R are dealt to the policies in turn (policy k: R[k % len(R)]), which sweeps the
interval when the policies are copies of one checkpoint (--sigma 0).  --figure-eight: the bank tracks the 0.3 m x 0.15 m figure-eight
of examples/track_figure_eight.py from hover at the origin, and the table gains every policy's RMS distance to the setpoint.
--suite: the same ONE launch flies every policy on the setpoints of raptor_amd.tracking.suite (hover, the figure-eight at two speeds, a
circle, a position step), dealt evenly over each policy's envs, and prints the [P, M] table of RMS distances: policy p on setpoint r.

Without --checkpoints the bank holds the shipped policy (policy 0) and perturbed copies of it, weights + sigma * N(0, 1): the further a
copy strays, the worse it flies.  --blocks: 64-env blocks per policy (more envs, tighter means).
"""
import argparse
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                                                           # noqa: E402
from raptor_amd import tracking                                                        # noqa: E402
from raptor_amd.foundation_policy import load_weights                                  # noqa: E402
from raptor_amd.policy_bank import PolicyBank, block_policy_assignment                 # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", type=int, default=1000)
    ap.add_argument("--blocks", type=int, default=1)
    ap.add_argument("--checkpoints", default=None, help="directory of policy checkpoints (*.h5), one policy per file")
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--show", type=int, default=10)
    ap.add_argument("--mode", default="fused", choices=["fused", "chained"])
    ap.add_argument("--native-interval", type=int, nargs="+", default=[1], metavar="R",
                    help="native interval of the policies, 1 .. 64; several: dealt to the policies in turn")
    ap.add_argument("--dt", type=float, default=None, help="control interval in seconds (default: the env's 0.01); the episode stays as long")
    ap.add_argument("--figure-eight", action="store_true", help="track a figure-eight instead of holding the origin")
    ap.add_argument("--suite", action="store_true", help="track a suite of setpoints, a reference per env: the RMSE table is [P, M]")
    args = ap.parse_args()
    if args.figure_eight and args.suite:
        ap.error("--figure-eight and --suite do not combine: the suite holds the figure-eight")

    device = l2f.Device()
    names = None
    if args.checkpoints:
        names = sorted(glob.glob(os.path.join(args.checkpoints, "*.h5")))
        bank = PolicyBank.from_checkpoints(device, names)
    else:
        w0 = load_weights()
        W = np.stack([w0] + [w0 + np.float32(args.sigma) * np.random.default_rng(100 + k).standard_normal(w0.size).astype(np.float32)
                             for k in range(1, args.policies)])
        bank = PolicyBank(device, W.astype(np.float32))
    intervals = np.resize(np.asarray(args.native_interval, np.uint32), bank.n_policies)
    bank.native_interval = intervals
    n = bank.n_policies * 64 * args.blocks
    vector = l2f.vector(n)
    rng, env = vector.VectorRng(), vector.VectorEnvironment()
    params, state = vector.VectorParameters(), vector.VectorState()
    vector.initialize_rng(device, rng, 0)
    vector.initialize_environment(device, env)
    cfg = env.config
    if args.dt is not None:                        # the same seconds per episode at another control rate
        cfg.episode_step_limit = int(round(cfg.episode_step_limit * float(cfg.dt) / args.dt))
        cfg.dt = args.dt
    if args.figure_eight or args.suite:
        cfg.init_guidance = 1.0                    # hover at the origin, where the path starts
    env.config = cfg
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    ids = block_policy_assignment(n, bank.n_policies)
    steps = int(cfg.episode_step_limit)
    ref, ref_ids, suite = None, None, None
    if args.figure_eight:
        ref = l2f.Reference(device, tracking.lissajous(steps, float(cfg.dt), amplitude=(0.3, 0.15, 0.0), period=5.0))
    if args.suite:
        suite = tracking.suite(steps, float(cfg.dt))
        ref = l2f.ReferenceBank(device, list(suite.values()))
        ref_ids = tracking.spread_reference_ids(n, len(suite), ids)
    device.timer_start()
    tab = bank.evaluate(vector, device, env, params, state, rng, steps, ids, mode=args.mode, reference=ref, reference_ids=ref_ids)
    ms = device.timer_stop()
    print(f"{bank.n_policies} policies x {64 * args.blocks} envs = {n} envs, {steps} steps of {float(cfg.dt):g} s ({args.mode}"
          f"{', figure-eight' if args.figure_eight else ', suite of ' + str(len(suite)) if suite else ''}): {ms:.1f} ms on the device, {int(tab['episodes'].sum())} episodes finished")
    rmse = tab.get("tracking_rmse")
    if suite:                                      # [P, M]: a column per setpoint
        print(f"{'policy':>8} {'R':>3} {'mean return':>12} {'terminated':>11}" + "".join(f" {name:>11}" for name in suite) + "   RMSE [m] per setpoint")
        order = np.argsort(np.nan_to_num(rmse.mean(axis=1), nan=np.inf))
        for k in order[:args.show]:
            print(f"{k:8d} {intervals[k]:3d} {tab['mean_return'][k]:12.3f} {tab['termination_share'][k]:11.3f}" +
                  "".join(f" {x:11.4f}" for x in rmse[k]) + (f"  {os.path.basename(names[k])}" if names else ""))
        best = int(order[0])
        print(f"best by mean RMSE over the suite: policy {best}" + (f" ({names[best]})" if names else "") +
              f", {rmse[best].mean():.4f} m; worst setpoint for it: {list(suite)[int(np.nanargmax(rmse[best]))]}")
        return
    print(f"{'policy':>8} {'R':>3} {'envs':>6} {'episodes':>9} {'mean return':>12} {'std':>9} {'mean length':>12} {'terminated':>11}" +
          (f" {'RMSE [m]':>9}" if rmse is not None else ""))
    order = np.argsort(-np.nan_to_num(tab["mean_return"], nan=-np.inf))
    for k in order[:args.show]:
        print(f"{k:8d} {intervals[k]:3d} {tab['envs'][k]:6d} {tab['episodes'][k]:9d} {tab['mean_return'][k]:12.3f} {tab['std_return'][k]:9.3f} "
              f"{tab['mean_length'][k]:12.1f} {tab['termination_share'][k]:11.3f}" + (f" {rmse[k]:9.4f}" if rmse is not None else "") +
              (f"  {os.path.basename(names[k])}" if names else ""))
    best = int(order[0])
    print(f"best by return: policy {best}" + (f" ({names[best]})" if names else "") +
          f", mean return {tab['mean_return'][best]:.3f}, mean length {tab['mean_length'][best]:.1f}, "
          f"terminated {tab['termination_share'][best]:.3f}")


if __name__ == "__main__":
    main()
