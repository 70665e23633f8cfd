#!/usr/bin/env python3
"""What does the policy DO with what it knows about the quadrotor it flies?  A control engineer reads a controller off its feedback
gains: G = da/dobs [4, 22], the local Jacobian of the four motor commands with respect to the observation, at the state the GRU is
in.  Fly domain-randomised quadrotors, then read the gains off the recording in ONE pass on the device
(raptor_amd.probing.feedback_gains): per env and bucket of episode age, nothing of the recording's Jacobians stored.

Two readings: how the collective gains on z position and z velocity (the mean over the four motors: the stiffness and the damping of
the height loop) settle over the first steps of an episode, and how the settled stiffness scales with thrust-to-weight and mass
across the fleet.  G is the instantaneous gain at fixed hidden state; the path of an observation into later actions through the
recurrence is not part of it.

    python examples/feedback_gains.py [--envs 16384] [--steps 500] [--buckets 10] [--json profiles/feedback_gains.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                                    # noqa: E402
from raptor_amd import probing                                  # noqa: E402
from raptor_amd.foundation_policy import Raptor                 # noqa: E402

Z_POSITION, Z_VELOCITY = 2, 14          # columns of the observation


def host(x):
    return np.asarray(x.cpu() if hasattr(x, "data_ptr") else x, np.float64)


def correlation(a, b):
    ok = np.isfinite(a) & np.isfinite(b)
    a, b = a[ok] - a[ok].mean(), b[ok] - b[ok].mean()
    d = np.sqrt((a * a).sum() * (b * b).sum())
    return float((a * b).sum() / d) if d > 0 else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--buckets", type=int, default=10)
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "feedback_gains.json"))
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

    edges = probing.log_age_edges(min(args.steps, int(cfg.episode_step_limit)), args.buckets)
    probing.feedback_gains(traj, policy, edges=edges)                          # code objects, workspaces
    device.synchronize()
    t0 = time.perf_counter()
    table = probing.feedback_gains(traj, policy, edges=edges)
    device.synchronize()
    ms = (time.perf_counter() - t0) * 1e3

    by_age = host(table.by_age())                                              # [B, 4, 22]
    counts = host(table.count).sum(1)
    kz, dz = by_age[:, :, Z_POSITION].mean(1), by_age[:, :, Z_VELOCITY].mean(1)
    last = args.buckets - 1
    settled = host(table.per_env(last))                                        # [4, 22, N]
    kz_env = settled[:, Z_POSITION, :].mean(0)
    y, names = probing.targets_from_params(params.numpy(), cfg, ["thrust_to_weight", "log_mass"])
    corr = {n: correlation(kz_env, y[:, i].astype(np.float64)) for i, n in enumerate(names)}
    norms = {name: float(np.sqrt((probing.GainTable.block(by_age[last], name) ** 2).sum())) for name in probing.OBSERVATION_BLOCKS}

    print(f"{env.N_ENVIRONMENTS} domain-randomised quadrotors x {args.steps} steps: the table in {ms:.2f} ms")
    print("age bucket        steps   collective gain on z   on z velocity")
    for b in range(args.buckets):
        print(f"[{int(edges[b]):4d}, {int(edges[b + 1]):4d})  {int(counts[b]):9d}  {kz[b]:+.5f}              {dz[b]:+.5f}")
    print(f"across envs, the settled (last bucket) collective z-position gain against the quadrotor's parameters: "
          + ", ".join(f"corr with {n} {v:+.3f}" for n, v in corr.items()))
    print("Frobenius norm of the settled mean gain by observation block: " + ", ".join(f"{k} {v:.3f}" for k, v in norms.items()))
    out = dict(envs=int(env.N_ENVIRONMENTS), steps=args.steps, age_edges=[int(e) for e in edges], table_ms=ms,
               steps_per_bucket=[int(v) for v in counts], collective_z_position_gain_by_age=[float(v) for v in kz],
               collective_z_velocity_gain_by_age=[float(v) for v in dz],
               correlation_of_settled_z_position_gain=corr, settled_gain_norm_by_block=norms,
               mean_gain_last_bucket=[[float(v) for v in row] for row in by_age[last]],
               note="G = da/dobs at fixed hidden state (the instantaneous gain); collective = the mean over the four motor commands; "
                    "settled = the last age bucket")
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.json)


if __name__ == "__main__":
    main()
