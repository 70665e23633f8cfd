#!/usr/bin/env python3
"""Rank student checkpoints by how they reject disturbances: P checkpoints x M scheduled wrenches (raptor_amd.disturbances.suite:
nothing, a lateral gust, a poke, a wind that builds up, a payload that hangs on, a roll kick) on the hover setpoint, in ONE fused
launch, and print the [P, M] table of RMS distances to the setpoint.

    python examples/disturbance_rejection.py [--policies 16] [--blocks 2] [--checkpoints DIR] [--sigma 0.05] [--show 10] [--mode fused|chained]

Every 64-env block is flown by one policy; inside every policy's envs the scenarios are dealt evenly (tracking.spread_reference_ids),
each env reading the row of its own episode step count of its own table.  Without --checkpoints the bank holds the shipped policy
(policy 0) and perturbed copies of it, weights + sigma * N(0, 1).
"""
import argparse
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                                                           # noqa: E402
from raptor_amd import disturbances, tracking                                          # noqa: E402
from raptor_amd.foundation_policy import load_weights                                  # noqa: E402
from raptor_amd.policy_bank import PolicyBank, block_policy_assignment                 # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--checkpoints", default=None, help="directory of policy checkpoints (*.h5), one policy per file")
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--show", type=int, default=10)
    ap.add_argument("--mode", default="fused", choices=["fused", "chained"])
    args = ap.parse_args()

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
    n = bank.n_policies * 64 * args.blocks
    vector = l2f.vector(n)
    rng, env = vector.VectorRng(), vector.VectorEnvironment()
    params, state = vector.VectorParameters(), vector.VectorState()
    vector.initialize_rng(device, rng, 0)
    vector.initialize_environment(device, env)
    cfg = env.config
    cfg.init_guidance = 1.0                        # hover at the origin, the setpoint that is held
    env.config = cfg
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    steps = int(cfg.episode_step_limit)
    suite = disturbances.suite(steps, float(cfg.dt))
    ids = block_policy_assignment(n, bank.n_policies)
    scenario = tracking.spread_reference_ids(n, len(suite), ids)
    env.set_wrench_schedule(l2f.WrenchBank(device, list(suite.values())), scenario)       # relative units: multiples of m g, m g arm
    hold = l2f.Reference(device, tracking.hold(steps))
    device.timer_start()
    tab = bank.evaluate(vector, device, env, params, state, rng, steps, ids, mode=args.mode, reference=hold, wrench_ids=scenario)
    ms = device.timer_stop()
    rmse = tab["tracking_rmse"]                    # [P, M]: policy p under scenario r
    print(f"{bank.n_policies} policies x {64 * args.blocks} envs = {n} envs, {steps} steps, {len(suite)} disturbance scenarios ({args.mode}): "
          f"{ms:.1f} ms on the device, {int(tab['episodes'].sum())} episodes finished")
    print(f"{'policy':>8} {'mean return':>12} {'terminated':>11}" + "".join(f" {name:>11}" for name in suite) + "   RMSE [m] per scenario")
    order = np.argsort(np.nan_to_num(rmse.mean(axis=1), nan=np.inf))
    for k in order[:args.show]:
        print(f"{k:8d} {tab['mean_return'][k]:12.3f} {tab['termination_share'][k]:11.3f}" + "".join(f" {x:11.4f}" for x in rmse[k]) +
              (f"  {os.path.basename(names[k])}" if names else ""))
    best = int(order[0])
    print(f"best by mean RMSE over the scenarios: policy {best}" + (f" ({names[best]})" if names else "") +
          f", {rmse[best].mean():.4f} m; hardest scenario for it: {list(suite)[int(np.nanargmax(rmse[best]))]}")
    env.clear_wrench_schedule()


if __name__ == "__main__":
    main()
