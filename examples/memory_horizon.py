#!/usr/bin/env python3
"""How far back does the policy's memory reach - and does that reach shrink once it has identified the quadrotor it flies?  The
lagged gain G^(k) = da_t/dobs_(t-k) [4, 22] is how much of the command at step t answers what was seen k steps earlier: the
linearised impulse response of the control law along the flown trajectory, through the GRU's recurrence.  Fly domain-randomised
quadrotors, record, then read the gains off the recording on the device (raptor_amd.probing.lag_gains) twice: seeded by the steps
of episode age < 20 - the policy is still finding out what it flies - and by those of age >= 100.

Printed: the Frobenius norm of the mean gain per observation block at every lag, early and late.

    python examples/memory_horizon.py [--envs 16384] [--steps 500] [--lags 16] [--json profiles/memory_horizon.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                                    # noqa: E402
from raptor_amd import probing                                  # noqa: E402
from raptor_amd.foundation_policy import Raptor                 # noqa: E402

EARLY, LATE = 20, 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--lags", type=int, default=probing.MAX_LAGS)
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "memory_horizon.json"))
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
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    policy = Raptor(device)
    policy.reset()
    traj = vector.Trajectory(env, args.steps)
    vector.rollout(device, env, params, state, policy, rng, args.steps, "fused", autoreset=True, trajectory=traj)
    device.synchronize()

    done = traj.numpy()["done"]
    age = probing.episode_steps(done)
    windows = {f"age < {EARLY}": age < EARLY, f"age >= {LATE}": age >= LATE}
    out = dict(envs=int(env.N_ENVIRONMENTS), steps=args.steps, lags=args.lags, windows={},
               note="Frobenius norm of the mean lagged gain da_t/dobs_(t-k) [4, 22] per observation block; a step of age a counts at "
                    "lags 0 .. a only")
    print(f"{env.N_ENVIRONMENTS} domain-randomised quadrotors x {args.steps} steps, {args.lags} lags")
    for name, select in windows.items():
        table = probing.lag_gains(traj, policy, n_lags=args.lags, select=select)
        norms = table.norm_by_lag()
        counts = np.asarray(table.count.cpu() if hasattr(table.count, "data_ptr") else table.count, np.int64).sum(1)
        print(f"\nseeded by the steps of {name}")
        print("lag      steps  " + "  ".join(f"{b:>16s}" for b in norms))
        for k in range(args.lags):
            print(f"{k:3d}  {int(counts[k]):9d}  " + "  ".join(f"{norms[b][k]:16.5f}" for b in norms))
        out["windows"][name] = dict(steps_by_lag=[int(c) for c in counts],
                                    gain_norm_by_lag={b: [None if np.isnan(v) else float(v) for v in norms[b]] for b in norms})
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.json)


if __name__ == "__main__":
    main()
