#!/usr/bin/env python3
"""The step response of the fleet, read off a recording: fly the disturbance suite (raptor_amd.disturbances.suite: nothing, a
lateral gust, a poke, a wind that builds up, a payload that hangs on, a roll kick) on the hover setpoint, the scenarios dealt over
the envs, record, and take the flight table (raptor_amd.probing.flight_table) in buckets of episode age around the onsets - the age
is the row of the wrench schedule, so a bucket of age is "time since the poke".  Per scenario: how far the vehicles were thrown (the
peak deviation), the share of the fleet outside the tolerance by age, the bucket from which the RMS deviation is back within
--back of what it was before the onset, and how often the commands sat at their limits.

    python examples/step_response.py [--envs 4096] [--lo 90] [--hi 410] [--buckets 32] [--tolerance 0.05] [--back 1.5]
                                     [--teachers K] [--json profiles/step_response.json]

--teachers K flies a TeacherBank of K MLP teachers (random weights unless --checkpoints DIR) instead of the shipped policy, each env
by its own teacher: what the student's recovery stands against.
"""
import argparse
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                                                           # noqa: E402
from raptor_amd import disturbances, probing, tracking                                 # noqa: E402
from raptor_amd.foundation_policy import Raptor                                        # noqa: E402


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--lo", type=int, default=90)
    ap.add_argument("--hi", type=int, default=410)
    ap.add_argument("--buckets", type=int, default=32)
    ap.add_argument("--tolerance", type=float, default=0.05)
    ap.add_argument("--back", type=float, default=1.5, help="recovered: the RMS deviation stays within this multiple of its value before the onset")
    ap.add_argument("--teachers", type=int, default=0)
    ap.add_argument("--checkpoints", default=None, help="directory of teacher checkpoints (*.h5), with --teachers")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    device = l2f.Device()
    vector = l2f.vector(args.envs)
    n = vector.N_ENVIRONMENTS
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
    names = list(suite)
    onsets = {"calm": None, "gust": steps // 4, "poke": steps // 4, "ramp": steps // 4, "payload": steps // 2, "torque_kick": steps // 4}
    scenario = tracking.spread_reference_ids(n, len(suite))
    env.set_wrench_schedule(l2f.WrenchBank(device, list(suite.values())), scenario)       # relative units: multiples of m g, m g arm
    hold = l2f.Reference(device, tracking.hold(steps))
    start = env.episode_steps()
    traj = vector.Trajectory(env, steps)
    if args.teachers:
        from raptor_amd.teachers import TeacherBank, balanced_teacher_assignment, parameter_count
        if args.checkpoints:
            bank = TeacherBank.from_checkpoints(device, sorted(glob.glob(os.path.join(args.checkpoints, "*.h5"))))
        else:
            w = np.random.default_rng(1).standard_normal((args.teachers, parameter_count(22, 64, 64))) * 0.1
            bank = TeacherBank(device, w.astype(np.float32), 22, 64, 64, "relu", "tanh")
        who = f"{bank.n_teachers} teachers"
        # (a teacher bank flies a wrench schedule in the chained mode)
        bank.fly(vector, device, env, params, state, rng, steps, balanced_teacher_assignment(n, bank.n_teachers), mode="chained",
                 autoreset=True, trajectory=traj, reference=hold)
    else:
        policy = Raptor(device)
        policy.reset()
        who = "the shipped policy"
        vector.rollout(device, env, params, state, policy, rng, steps, "fused", autoreset=True, trajectory=traj, reference=hold)

    edges = probing.linear_age_edges(args.lo, args.hi, args.buckets)
    width = int(edges[1] - edges[0])
    probing.flight_table(traj, edges=edges, start_steps=start, tolerance=args.tolerance)     # code objects, workspaces, torch's start
    device.timer_start()
    table = probing.flight_table(traj, edges=edges, start_steps=start, tolerance=args.tolerance)
    ms = device.timer_stop()
    curves = {k: host(v) for k, v in table.by_group(scenario, len(suite)).items()}          # [M, B] each
    peaks = host(table.peak_by_group(scenario, len(suite)))                                 # [M, B, 3]
    print(f"{who}, {n} envs x {steps} steps, {len(suite)} scenarios, {args.buckets} buckets of {width} steps from age {int(edges[0])}: "
          f"flight table in {ms:.2f} ms on the device")
    print(f"{'scenario':>12} {'onset':>6} {'peak dev [m]':>13} {'at age':>7} {'worst share outside':>20} {'recovered at age':>17} {'saturated':>10}")
    out = dict(policy=who, envs=n, steps=steps, tolerance=args.tolerance, age_edges=[int(x) for x in edges], back=args.back,
               flight_table_ms=ms, scenarios={})
    for g, name in enumerate(names):
        onset = onsets.get(name)
        ob = 0 if onset is None else min(max((onset - int(edges[0])) // width, 0), args.buckets - 1)
        rms, outside = curves["rms_position"][g], curves["share_outside"][g]
        before = float(np.nanmean(rms[:max(ob, 1)]))
        rec = probing.FlightTable.recovery(rms, ob, args.back * before)
        dev2 = peaks[g, :, 0]
        worst = int(np.nanargmax(dev2)) if np.isfinite(dev2).any() else 0
        sat = float(np.nanmean(curves["share_saturated"][g]))
        print(f"{name:>12} {'-' if onset is None else onset:>6} {float(np.sqrt(dev2[worst])):13.4f} {int(edges[worst]):7d} "
              f"{float(np.nanmax(outside)):20.3f} {'never' if rec < 0 else int(edges[rec]):>17} {sat:10.4f}")
        out["scenarios"][name] = dict(onset=onset, onset_bucket=ob, peak_deviation_m=float(np.sqrt(dev2[worst])), peak_at_age=int(edges[worst]),
                                      rms_before_onset_m=before, recovery_bucket=int(rec), recovered_at_age=None if rec < 0 else int(edges[rec]),
                                      share_saturated=sat, rms_position_m=[float(x) for x in rms], share_outside=[float(x) for x in outside],
                                      share_saturated_by_age=[float(x) for x in curves["share_saturated"][g]],
                                      mean_tilt=[float(x) for x in curves["mean_tilt"][g]])
    env.clear_wrench_schedule()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
