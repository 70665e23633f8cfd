#!/usr/bin/env python3
"""How many steps after a payload pick-up does the GRU state know the new mass, and how far does the vehicle sag meanwhile?
Domain-randomised quadrotors hold the origin (tracking.hold) with the shipped policy under a vehicle schedule: every env flies one
scenario of vehicles.suite - nothing, a payload picked up, a payload dropped, a sagging battery, slow motors - and the vehicle changes
at episode step --at.
    python examples/payload_pickup.py [--envs 16384] [--steps 300] [--at 100] [--json profiles/payload_pickup.json]
Per scenario it prints the deviation from the setpoint and the tilt by time since the change (probing.flight_table(...).by_group,
peak_by_group, FlightTable.recovery), and per bucket of episode age the held-out R^2 of a linear read-out of log(mass factor) from
the hidden state: the targets are the schedule's own rows gathered on the host along the recording's episode step counts
(probing.table_targets), the moments of [1, h_t, y_t] are made on the device (HiddenProbe.moments(traj, targets=...)), fitted on one
recording and scored on a second one of other quadrotors.  Before the change every scenario but the dropped payload has the factor
1: with two values in a bucket the read-out separates the payload that will be dropped from the rest.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                       # noqa: E402
from raptor_amd import probing, tracking, vehicles  # noqa: E402
from raptor_amd.foundation_policy import Raptor    # noqa: E402


def change_edges(at, steps):
    """Linear age edges around the change: two buckets before it, narrow ones right after it, wider later"""
    e = [at - 20, at - 10] + [at + d for d in (0, 2, 4, 6, 8, 10, 15, 20, 30, 50, 80, 120, 180)]
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


def mass_moments(probe, traj, tables, ids, start):
    k = probing.episode_steps(traj.numpy()["done"], start)
    factor = probing.table_targets(tables[:, :, vehicles.MASS:vehicles.MASS + 1], k, ids).astype(np.float64)
    factor[k < 0] = 1.0                             # frozen steps (none under auto-reset) carry no target
    y = np.log(factor).astype(np.float32)
    return probe.moments(traj, targets=y)


def _clean(a):
    return [[None if not np.isfinite(v) else float(v) for v in row] for row in np.asarray(a, np.float64)]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--at", type=int, default=100)
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "payload_pickup.json"))
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
    suite = vehicles.suite(limit, step=args.at)
    names, tables = list(suite), np.stack(list(suite.values()))
    M = len(names)
    bank = l2f.VehicleBank(device, tables)
    ids = (np.arange(args.envs) % M).astype(np.uint32)
    env.set_vehicle_schedule(bank, ids)
    hold = l2f.Reference(device, tracking.hold(limit))
    edges = change_edges(args.at, min(args.steps, limit))
    onset = int(np.flatnonzero(edges == args.at)[0])
    probe = probing.HiddenProbe(policy, None, ["log_mass_factor"], edges)

    traj_fit, start = record(device, vector, env, params, state, rng, policy, args.steps, hold)
    m_fit = mass_moments(probe, traj_fit, tables, ids, start)
    W = probe.fit(m_fit)
    r2_fit = probe.r2(m_fit, W)
    del traj_fit

    traj_held, start = record(device, vector, env, params, state, rng, policy, args.steps, hold)
    m_held = mass_moments(probe, traj_held, tables, ids, start)
    r2_held = probe.r2(m_held, W)
    ft = probing.flight_table(traj_held, edges=edges, start_steps=start, device=False)
    curves = ft.by_group(ids, M)
    peaks = np.asarray(ft.peak_by_group(ids, M), np.float64)
    rms, tilt = np.asarray(curves["rms_position"], np.float64), np.asarray(curves["mean_tilt"], np.float64)
    level = 1.25 * rms[:, max(onset - 1, 0)]           # "recovered": back within a quarter above the bucket before the change
    recovered = [probing.FlightTable.recovery(rms[g], onset, level[g]) for g in range(M)]

    print(f"{args.envs} domain-randomised quadrotors x {args.steps} steps on tracking.hold, the vehicle changes at episode step {args.at}")
    print("  rms deviation from the setpoint [m] by episode age")
    print("  age [from, to)    " + "  ".join(f"{n:>14s}" for n in names))
    for b in range(len(edges) - 1):
        print(f"  [{edges[b]:4d}, {edges[b + 1]:4d})  " + "  ".join(f"{rms[g, b]:14.4f}" for g in range(M)))
    print("  peak deviation [m] " + "  ".join(f"{np.sqrt(np.nanmax(peaks[g, onset:, 0])):14.4f}" for g in range(M)))
    print("  peak tilt 1 - R22  " + "  ".join(f"{np.nanmax(peaks[g, onset:, 1]):14.4f}" for g in range(M)))
    print("  recovered from     " + "  ".join(f"{('age %d' % edges[r]) if r >= 0 else 'not':>14s}" for r in recovered))
    print("  held-out R^2 of log(mass factor) read off the hidden state, by episode age")
    for b in range(len(edges) - 1):
        print(f"  [{edges[b]:4d}, {edges[b + 1]:4d})  {int(m_held.counts[b]):10d} samples  {r2_held[b, 0]:8.4f}")
    out = dict(envs=args.envs, steps=args.steps, change_step=args.at, scenarios=names, columns=list(vehicles.VEHICLE_NAMES),
               age_edges=[int(e) for e in edges], rms_position=_clean(rms), mean_tilt=_clean(tilt),
               peak_position=[float(np.sqrt(np.nanmax(peaks[g, onset:, 0]))) for g in range(M)],
               peak_tilt=[float(np.nanmax(peaks[g, onset:, 1])) for g in range(M)],
               recovered_from_age=[int(edges[r]) if r >= 0 else None for r in recovered],
               samples_fit=[int(c) for c in m_fit.counts], samples_held_out=[int(c) for c in m_held.counts],
               r2_fit=_clean(r2_fit), r2_held_out=_clean(r2_held),
               note="rms_position / mean_tilt: [scenario][bucket] over the scenario's envs; peaks over the buckets from the change on; "
                    "recovered: the first bucket from which the rms deviation stays within 1.25 x the bucket before the change; R^2: "
                    "linear read-out of the hidden state entering a step of log(mass factor) at that step, fitted on one recording, "
                    "scored on a second one of other quadrotors; null: the target is constant in the bucket")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote", args.json)
