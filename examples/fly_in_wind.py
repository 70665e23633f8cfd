#!/usr/bin/env python3
"""How far does a steady wind push the shipped policy off its setpoint, how much does it lean, and does the GRU state know the wind?
Domain-randomised quadrotors hold the origin (tracking.hold) with the shipped policy under a wind schedule: every env flies one
scenario - calm air, still air that only drags, steady winds of several speeds along x, and turbulence around a mean - and the wind
sets in at episode step --at (before it the air is at rest, with the same drag).
    python examples/fly_in_wind.py [--envs 16384] [--steps 300] [--at 100] [--json profiles/fly_in_wind.json]
Per scenario it prints the deviation from the setpoint and the tilt by time since the onset (probing.flight_table(...).by_group), and
per bucket of episode age the held-out R^2 of a linear read-out of the air velocity (x, y) from the hidden state: the targets are the
schedule's own rows gathered on the host along the recording's episode step counts (probing.table_targets), the moments of
[1, h_t, y_t] are made on the device (HiddenProbe.moments(traj, targets=...)), fitted on one recording and scored on a second one of
other quadrotors.  Before the onset the air velocity is zero in every scenario: the target is constant and the R^2 undefined (null).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                       # noqa: E402
from raptor_amd import build as rq_build           # noqa: E402
from raptor_amd import probing, tracking, winds    # noqa: E402
from raptor_amd.foundation_policy import Raptor    # noqa: E402

SPEEDS = (2.0, 5.0, 8.0)                           # m/s, along +x


def scenarios(rows, dt, at, drag):
    """name -> table [rows, 4]: the air at rest until step `at`, then the scenario's wind; the drag holds throughout"""
    start = at * dt
    out = {"calm": winds.calm(rows), "still_air": winds.still_air(rows, drag)}
    for v in SPEEDS:
        out[f"steady_{v:g}"] = winds.ramp(rows, dt, (v, 0.0, 0.0), start, 0.0, drag)
    turb = winds.turbulence(rows, dt, (3.0, 0.0, 0.0), 1.5, 1.0, drag, 0)
    turb[:at, 0:3] = 0.0
    out["turbulence"] = turb
    return out


def onset_edges(at, steps):
    """Linear age edges around the onset: two buckets before it, narrow ones right after it, wider later"""
    e = [at - 20, at - 10] + [at + d for d in (0, 5, 10, 20, 30, 50, 75, 100, 150, 200)]
    return np.asarray(sorted({int(v) for v in e if 0 <= v <= steps}), np.uint32)


def record(device, vector, env, params, state, rng, policy, steps, hold):
    """New quadrotors (the RNG's next parameter epoch), new initial states, `steps` recorded steps -> (trajectory, start steps)"""
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    env.reset_statistics()
    start = env.episode_steps()                     # zeros after reset_statistics: read, not assumed
    traj = vector.Trajectory(env, steps)
    policy.reset()
    vector.rollout(device, env, params, state, policy, rng, steps, mode="fused", autoreset=True, trajectory=traj, reference=hold)
    return traj, start


def wind_moments(probe, traj, tables, ids, start):
    k = probing.episode_steps(traj.numpy()["done"], start)
    y = probing.table_targets(tables[:, :, 0:2], k, ids).astype(np.float32)
    y[k < 0] = 0.0                                  # frozen steps (none under auto-reset) carry no target
    return probe.moments(traj, targets=y)


def _clean(a):
    return [[None if not np.isfinite(v) else float(v) for v in row] for row in np.asarray(a, np.float64)]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--at", type=int, default=100)
    ap.add_argument("--drag", type=float, default=winds.DEFAULT_DRAG)
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fly_in_wind.json"))
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
    limit = int(cfg.episode_step_limit)
    suite = scenarios(limit, float(cfg.dt), args.at, args.drag)
    names, tables = list(suite), np.stack(list(suite.values()))
    M = len(names)
    bank = l2f.WindBank(device, tables)
    ids = (np.arange(args.envs) % M).astype(np.uint32)
    env.set_wind_schedule(bank, ids)
    hold = l2f.Reference(device, tracking.hold(limit))
    edges = onset_edges(args.at, min(args.steps, limit))
    onset = int(np.flatnonzero(edges == args.at)[0])
    probe = probing.HiddenProbe(policy, None, ["wind_x", "wind_y"], edges)

    traj_fit, start = record(device, vector, env, params, state, rng, policy, args.steps, hold)
    m_fit = wind_moments(probe, traj_fit, tables, ids, start)
    W = probe.fit(m_fit)
    r2_fit = probe.r2(m_fit, W)
    del traj_fit

    traj_held, start = record(device, vector, env, params, state, rng, policy, args.steps, hold)
    m_held = wind_moments(probe, traj_held, tables, ids, start)
    r2_held = probe.r2(m_held, W)
    ft = probing.flight_table(traj_held, edges=edges, start_steps=start, device=False)
    curves = ft.by_group(ids, M)
    rms, tilt = np.asarray(curves["rms_position"], np.float64), np.asarray(curves["mean_tilt"], np.float64)

    print(f"{args.envs} domain-randomised quadrotors x {args.steps} steps on tracking.hold, drag {args.drag} / s, the wind sets in at "
          f"episode step {args.at}")
    for title, table in (("rms deviation from the setpoint [m]", rms), ("mean tilt 1 - R22", tilt)):
        print(f"  {title} by episode age")
        print("  age [from, to)    " + "  ".join(f"{n:>12s}" for n in names))
        for b in range(len(edges) - 1):
            print(f"  [{edges[b]:4d}, {edges[b + 1]:4d})  " + "  ".join(f"{table[g, b]:12.4f}" for g in range(M)))
    print("  held-out R^2 of the air velocity (x, y) read off the hidden state, by episode age")
    for b in range(len(edges) - 1):
        print(f"  [{edges[b]:4d}, {edges[b + 1]:4d})  {int(m_held.counts[b]):10d} samples  {r2_held[b, 0]:8.4f}  {r2_held[b, 1]:8.4f}")
    out = dict(library_sha256=rq_build.library_sha256(), envs=args.envs, steps=args.steps, onset_step=args.at, drag=args.drag,
               scenarios=names, columns=list(winds.WIND_NAMES), targets=["wind_x", "wind_y"], onset_bucket=onset,
               age_edges=[int(e) for e in edges], rms_position=_clean(rms), mean_tilt=_clean(tilt),
               samples_fit=[int(c) for c in m_fit.counts], samples_held_out=[int(c) for c in m_held.counts],
               r2_fit=_clean(r2_fit), r2_held_out=_clean(r2_held),
               note="rms_position / mean_tilt: [scenario][bucket] over the scenario's envs, buckets of episode age; R^2: [bucket][target], "
                    "linear read-out of the hidden state entering a step of the air velocity at that step, fitted on one recording, "
                    "scored on a second one of other quadrotors; null: the target is constant in the bucket")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print("wrote", args.json)
