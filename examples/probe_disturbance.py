#!/usr/bin/env python3
"""Does the GRU state know what is pushing on the vehicle right now, and how many steps after the onset does it know?
Domain-randomised quadrotors hold the origin with the shipped policy under a wrench schedule: every env flies one of --tables gusts,
a constant force from step --onset for --length steps whose direction and strength differ per table - so that the target varies
between the envs of one age bucket.  A linear read-out of the hidden state is fitted per bucket of episode age on one recording and
scored on a second one, of other quadrotors (the next parameter epoch of the same RNG).
    python examples/probe_disturbance.py [--envs 16384] [--steps 300] [--onset 100] [--length 100] [--json profiles/probe_disturbance.json]
The targets are the scheduled force of every step in multiples of m g, rebuilt on the device from the recording's done codes
(Trajectory.wrench_targets): they never exist on the host.  The device also computes the second moments of [1, h_t, y_t] in one pass
over each recording (HiddenProbe.moments(traj, targets=...)); fit and score are 17 x 17 algebra on the host.
Buckets before the onset and after the gust's end hold a constant target (zero): there is no variance to explain and their R^2 is
NaN (null in the file), not a bad score.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                       # noqa: E402
from raptor_amd import disturbances, probing       # noqa: E402
from raptor_amd.foundation_policy import Raptor    # noqa: E402

FORCE = probing.WRENCH_NAMES[:3]


def gust_tables(n_tables, rows, dt, onset, length):
    """Gusts of one timing: directions spread over the sphere (a golden-angle spiral), strengths 0.1 .. 0.4 m g"""
    tables = []
    for j in range(n_tables):
        z = 1.0 - 2.0 * (j + 0.5) / n_tables
        phi = j * np.pi * (3.0 - np.sqrt(5.0))
        direction = np.array([np.sqrt(1.0 - z * z) * np.cos(phi), np.sqrt(1.0 - z * z) * np.sin(phi), z])
        strength = 0.1 + 0.3 * ((j * 7) % n_tables) / max(n_tables - 1, 1)
        tables.append(disturbances.gust(rows, dt, strength * direction, (onset - 0.5) * dt, length * dt))
    return np.stack(tables)


def onset_edges(onset, length, steps):
    """Linear age edges around the onset: two buckets before it, two steps wide right after it, wider later, two after the end"""
    e = [onset - 20, onset - 10] + [onset + d for d in (0, 2, 4, 6, 8, 10, 15, 20, 40, 70)] + [onset + length, onset + length + 10,
                                                                                               onset + length + 30]
    e = sorted({int(v) for v in e if 0 <= v <= steps})
    return np.asarray(e, np.uint32)


def record(device, vector, env, params, state, rng, policy, steps):
    """New quadrotors (the RNG's next parameter epoch), new initial states, `steps` recorded steps -> (trajectory, start steps)"""
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    env.reset_statistics()
    start = env.episode_steps()                     # zeros after reset_statistics: read, not assumed
    traj = vector.Trajectory(env, steps)
    policy.reset()
    vector.rollout(device, env, params, state, policy, rng, steps, mode="fused", autoreset=True, trajectory=traj)
    return traj, start


def force_moments(probe, traj, bank, ids, params, start):
    y = traj.wrench_targets(bank, ids, params, start, units="relative", device=True)       # [T, 6, ld] on the device
    return probe.moments(traj, targets=y[:, :3].contiguous(), device=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--tables", type=int, default=16)
    ap.add_argument("--onset", type=int, default=100)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "probe_disturbance.json"))
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
    tables = gust_tables(args.tables, int(cfg.episode_step_limit), float(cfg.dt), args.onset, args.length)
    assert (tables[:, args.onset - 1] == 0).all() and (tables[:, args.onset, :3] != 0).any(axis=1).all()
    bank = l2f.WrenchBank(device, tables, units="relative")
    ids = (np.arange(args.envs) % args.tables).astype(np.uint32)
    env.set_wrench_schedule(bank, ids)
    edges = onset_edges(args.onset, args.length, min(args.steps, int(cfg.episode_step_limit)))
    probe = probing.HiddenProbe(policy, None, FORCE, edges)

    traj_fit, start = record(device, vector, env, params, state, rng, policy, args.steps)
    m_fit = force_moments(probe, traj_fit, bank, ids, params, start)
    W = probe.fit(m_fit)
    r2_fit = probe.r2(m_fit, W)
    del traj_fit

    traj_held, start = record(device, vector, env, params, state, rng, policy, args.steps)
    m_held = force_moments(probe, traj_held, bank, ids, params, start)
    r2_held = probe.r2(m_held, W)

    print(f"{args.envs} domain-randomised quadrotors x {args.steps} steps, {args.tables} gusts from episode step {args.onset} for "
          f"{args.length} steps; fitted on one recording, scored on another; held-out R^2 of the force read-out (multiples of m g)")
    print("  age [from, to)     samples  " + "  ".join(f"{n:>10s}" for n in FORCE))
    for b in range(len(edges) - 1):
        print(f"  [{edges[b]:4d}, {edges[b + 1]:4d})  {int(m_held.counts[b]):10d}  " + "  ".join(f"{v:10.4f}" for v in r2_held[b]))
    print("  (nan: the bucket lies before the onset or after the gust's end - the target is constant, there is nothing to explain)")
    out = dict(envs=args.envs, steps=args.steps, tables=args.tables, onset_step=args.onset, gust_steps=args.length,
               units="multiples of m g", targets=FORCE, age_edges=[int(e) for e in edges],
               samples_fit=[int(c) for c in m_fit.counts], samples_held_out=[int(c) for c in m_held.counts],
               r2_fit=[[None if not np.isfinite(v) else float(v) for v in row] for row in r2_fit],
               r2_held_out=[[None if not np.isfinite(v) else float(v) for v in row] for row in r2_held],
               note="linear read-out of the hidden state entering a step, per bucket of episode age, of the scheduled force applied at "
                    "that step; fitted on one recording, scored on a second one of other quadrotors; null: the target is constant "
                    "in the bucket (before the onset, after the gust's end) or the bucket holds fewer than 18 samples")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote", args.json)
