#!/usr/bin/env python3
"""What does the GRU state know about the quadrotor it flies, and after how many steps?  Domain-randomised quadrotors fly with the
shipped policy; a linear read-out of the hidden state is fitted per bucket of episode age on one recording and scored on a second
one, of other quadrotors (the next parameter epoch of the same RNG).
    python examples/probe_hidden_state.py [--envs 16384] [--steps 500] [--buckets 10] [--json profiles/probe_curve.json]
Prints held-out R^2 per age bucket and target.  The device computes the second moments of [1, h_t, y] in one pass over each recording
(raptor_amd.probing.HiddenProbe.moments); fit and score are 17 x 17 algebra on the host.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                       # noqa: E402
from raptor_amd import probing                     # noqa: E402
from raptor_amd.foundation_policy import Raptor    # noqa: E402

NAMES = ["log_mass", "thrust_to_weight", "log_jxx", "log_jzz", "tau_rise", "torque_const", "hover_action"]


def record(device, vector, env, params, state, rng, policy, steps):
    """New quadrotors (the RNG's next parameter epoch), new initial states, `steps` recorded steps -> (trajectory, params [N, 26])"""
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    env.reset_statistics()
    traj = vector.Trajectory(env, steps)
    policy.reset()
    vector.rollout(device, env, params, state, policy, rng, steps, mode="fused", autoreset=True, trajectory=traj)
    return traj, params.numpy()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--buckets", type=int, default=10)
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "probe_curve.json"))
    args = ap.parse_args()
    device = l2f.Device()
    vector = l2f.vector(args.envs)
    rng, env = vector.VectorRng(), vector.VectorEnvironment()
    params, state = vector.VectorParameters(), vector.VectorState()
    vector.initialize_rng(device, rng, 0)
    vector.initialize_environment(device, env)
    cfg = env.config
    cfg.domain_randomization = 1
    env.config = cfg
    policy = Raptor(device)
    edges = probing.log_age_edges(min(args.steps, int(cfg.episode_step_limit)), args.buckets)

    traj_fit, p_fit = record(device, vector, env, params, state, rng, policy, args.steps)
    y_fit, names = probing.targets_from_params(p_fit, cfg, NAMES)
    y_fit, mean, std = probing.standardise(y_fit)
    fit_probe = probing.HiddenProbe(policy, y_fit, names, edges)
    m_fit = fit_probe.moments(traj_fit)
    W = fit_probe.fit(m_fit)
    r2_fit = fit_probe.r2(m_fit, W)
    del traj_fit

    traj_held, p_held = record(device, vector, env, params, state, rng, policy, args.steps)
    y_held, _ = probing.targets_from_params(p_held, cfg, NAMES)
    y_held = ((y_held - mean) / std).astype(np.float32)              # the fit's units
    held_probe = probing.HiddenProbe(policy, y_held, names, edges)
    m_held = held_probe.moments(traj_held)
    r2_held = held_probe.r2(m_held, W)

    print(f"{args.envs} domain-randomised quadrotors x {args.steps} steps, fitted on one recording, scored on another; held-out R^2")
    print("  age [from, to)     samples  " + "  ".join(f"{n:>16s}" for n in names))
    for b in range(len(edges) - 1):
        print(f"  [{edges[b]:4d}, {edges[b + 1]:4d})  {int(m_held.counts[b]):10d}  " + "  ".join(f"{v:16.4f}" for v in r2_held[b]))
    out = dict(envs=args.envs, steps=args.steps, targets=names, age_edges=[int(e) for e in edges],
               samples_fit=[int(c) for c in m_fit.counts], samples_held_out=[int(c) for c in m_held.counts],
               r2_fit=[[None if not np.isfinite(v) else float(v) for v in row] for row in r2_fit],
               r2_held_out=[[None if not np.isfinite(v) else float(v) for v in row] for row in r2_held],
               note="linear read-out of the hidden state entering a step, per bucket of episode age; fitted on one recording, scored "
                    "on a second one of other quadrotors; targets standardised with the fit recording's mean and deviation")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote", args.json)
