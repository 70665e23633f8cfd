#!/usr/bin/env python3
"""Which latency hurts a checkpoint more: the sensor's or the command's?  P checkpoints x delays of 0 .. 8 steps hold the origin
(tracking.hold) and are poked sideways (disturbances.poke) at episode step --at - once with the delays on the sensor side (a sensor
schedule: the policy sees the state of d steps ago) and once with the same delays on the command side (a delay schedule: the rotors
get the command of d steps ago), at 100 Hz and at 400 Hz with the policy at native interval 4 (a step of delay is 10 ms there and
2.5 ms here).
    python examples/sensor_latency.py [--policies 4] [--blocks 1] [--sigma 0.05] [--at 100] [--json profiles/sensor_latency.json]
Every 64-env block is flown by one policy; inside every policy's envs the delays are dealt evenly (tracking.spread_reference_ids).
Either schedule beside a wrench schedule flies chained.  Per rate, side, checkpoint and delay it writes the rms deviation from the
setpoint after the poke, the share of envs that terminated, and the bucket of episode age from which the deviation stays within
--level of the setpoint (FlightTable.recovery; -1: never).  Without --checkpoints the bank holds the shipped policy (policy 0) and
perturbed copies of it.  Nothing here says how a checkpoint SHOULD degrade: the table is the measurement.
"""
import argparse
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                                                           # noqa: E402
from raptor_amd import build as rq_build                                               # noqa: E402
from raptor_amd import delays, disturbances, probing, sensors, tracking                # noqa: E402
from raptor_amd.foundation_policy import load_weights                                  # noqa: E402
from raptor_amd.policy_bank import PolicyBank, block_policy_assignment                 # noqa: E402

DELAYS = tuple(range(9))                           # steps
SIDES = ("sensor", "command")


def _clean(a):
    """NaN (a group without a live step after the poke: every env had terminated) -> null"""
    return [[None if not np.isfinite(v) else float(v) for v in row] for row in np.asarray(a, np.float64)]


def fly(device, W, names, blocks, dt, interval, at, steps, level, side):
    """one rate and one side: the bank at `interval`, the env at `dt`; the poke lasts 50 ms from `at` (in steps of this rate) on"""
    bank = PolicyBank.from_checkpoints(device, names) if names else PolicyBank(device, W)
    bank.native_interval = interval
    P, M = bank.n_policies, len(DELAYS)
    n = P * 64 * blocks
    vector = l2f.vector(n)
    rng, env = vector.VectorRng(), vector.VectorEnvironment()
    params, state = vector.VectorParameters(), vector.VectorState()
    vector.initialize_rng(device, rng, 0)
    vector.initialize_environment(device, env)
    cfg = env.config
    cfg.init_guidance = 1.0                        # hover at the origin, the setpoint that is held
    cfg.dt, cfg.episode_step_limit = dt, steps
    env.config = cfg
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    pids = block_policy_assignment(n, P)
    dids = tracking.spread_reference_ids(n, M, pids)
    poke = disturbances.poke(steps, (0.5, 0.0, 0.0), at, steps=max(1, int(round(0.05 / dt))))      # half the weight, sideways
    env.set_wrench_schedule(l2f.WrenchBank(device, [poke]))
    if side == "sensor":
        env.set_sensor_schedule(l2f.SensorBank(device, [sensors.constant(steps, d) for d in DELAYS]), dids)
    else:
        env.set_delay_schedule(l2f.DelayBank(device, [delays.constant(steps, d) for d in DELAYS]), dids)
    hold = l2f.Reference(device, tracking.hold(steps))
    env.reset_statistics()
    bank.reset()
    traj = vector.Trajectory(env, steps)
    bank.fly(vector, device, env, params, state, rng, steps, pids, mode="chained", autoreset=False, trajectory=traj, reference=hold)
    # (the flight table reads the recorded observation: what the policy saw.  Under a sensor schedule that is the delivered position,
    # d steps old, so the deviation is taken from the env's own tracking error, which stays on the true position, per env)
    width = max(1, int(round(0.1 / dt)))           # buckets of 100 ms from the poke on
    edges = np.arange(at, steps + 1, width, dtype=np.uint32)
    group = (pids.astype(np.int64) * M + dids).astype(np.int64)
    rec = traj.numpy()
    done = rec["done"]
    terminated = np.array([[(done[:, group == p * M + m] == 1).any(axis=0).mean() for m in range(M)] for p in range(P)])
    out = dict(dt=dt, native_interval=interval, envs=n, steps=steps, poke_step=at, delay_ms=[d * dt * 1e3 for d in DELAYS],
               age_edges=[int(e) for e in edges], share_terminated=_clean(terminated))
    sq, cnt = env.tracking_error()                 # true position against the held setpoint, over the whole flight
    rmse = np.array([[np.sqrt(sq[group == p * M + m].astype(np.float64).sum() / max(1, int(cnt[group == p * M + m].sum())))
                      for m in range(M)] for p in range(P)])
    out["tracking_rmse"] = _clean(rmse)
    if side == "command":                          # the recorded position is the true one: the poke's aftermath by episode age
        ft = probing.flight_table(traj, edges=edges, device=False)
        rms = np.asarray(ft.by_group(group, P * M)["rms_position"], np.float64).reshape(P, M, -1)
        out["rms_after_poke"] = _clean(np.sqrt(np.nanmean(rms ** 2, axis=2)))
        out["recovery_bucket"] = [[int(probing.FlightTable.recovery(rms[p, m], 0, level)) for m in range(M)] for p in range(P)]
    else:                                          # the recorded position is d steps old: shifted back onto its own step, per group
        pos = rec["obs"][:, :, 0:3].astype(np.float64)
        live = done != 4
        rms_after = np.full((P, M), np.nan)
        recovery = [[-1] * M for _ in range(P)]
        for p in range(P):
            for m, d in enumerate(DELAYS):
                sel = group == p * M + m
                true_pos = pos[d:, sel] if d else pos[:, sel]                # what was seen at step t + d is the position of step t
                ok = live[d:, sel] if d else live[:, sel]
                dev2 = np.where(ok, (true_pos ** 2).sum(axis=2), np.nan)
                buckets = [np.sqrt(np.nanmean(dev2[lo:hi])) if np.isfinite(dev2[lo:hi]).any() else np.nan
                           for lo, hi in zip(edges[:-1], edges[1:]) if lo < len(dev2)]
                if buckets:
                    b = np.asarray(buckets)
                    rms_after[p, m] = np.sqrt(np.nanmean(b ** 2)) if np.isfinite(b).any() else np.nan
                    recovery[p][m] = int(probing.FlightTable.recovery(b, 0, level))
        out["rms_after_poke"] = _clean(rms_after)
        out["recovery_bucket"] = recovery
    env.clear_wrench_schedule()
    env.clear_sensor_schedule()
    env.clear_delay_schedule()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", type=int, default=4)
    ap.add_argument("--blocks", type=int, default=1)
    ap.add_argument("--checkpoints", default=None, help="directory of policy checkpoints (*.h5), one policy per file")
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--at", type=int, default=100, help="the poke's episode step at 100 Hz")
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--level", type=float, default=0.05, help="recovered: rms deviation within this many metres")
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sensor_latency.json"))
    args = ap.parse_args()
    device = l2f.Device()
    names, W = None, None
    if args.checkpoints:
        names = sorted(glob.glob(os.path.join(args.checkpoints, "*.h5")))
    else:
        w0 = load_weights()
        W = np.stack([w0] + [w0 + np.float32(args.sigma) * np.random.default_rng(100 + k).standard_normal(w0.size).astype(np.float32)
                             for k in range(1, args.policies)]).astype(np.float32)
    out = dict(library_sha256=rq_build.library_sha256(), delays_steps=list(DELAYS), level=args.level, rates={})
    for label, dt, interval in (("100Hz", 0.01, 1), ("400Hz_interval4", 0.0025, 4)):
        scale = int(round(0.01 / dt))
        out["rates"][label] = {}
        for side in SIDES:
            r = fly(device, W, names, args.blocks, dt, interval, args.at * scale, int(round(args.seconds / dt)), args.level, side)
            out["rates"][label][side] = r
            print(f"{label}, latency on the {side} side: {r['envs']} envs x {r['steps']} steps (chained), poke at step {r['poke_step']}; rms "
                  f"deviation after the poke [m] | whole-flight tracking rmse [m] | share terminated | recovery bucket, by delay in steps")
            for p in range(len(r["rms_after_poke"])):
                print(f"  policy {p}" + (f" ({os.path.basename(names[p])})" if names else ""))
                for m, d in enumerate(DELAYS):
                    rms, whole = r["rms_after_poke"][p][m], r["tracking_rmse"][p][m]
                    print(f"    d = {d} ({r['delay_ms'][m]:5.1f} ms)  {float('nan') if rms is None else rms:8.4f}  "
                          f"{float('nan') if whole is None else whole:8.4f}  {r['share_terminated'][p][m]:6.3f}  {r['recovery_bucket'][p][m]:3d}")
    out["note"] = ("[rate][side][policy][delay]; side 'sensor': a sensor schedule (the policy sees the state of d steps ago), 'command': a "
                   "delay schedule (the rotors get the command of d steps ago); rms_after_poke: true position over the live steps from the "
                   "poke on; tracking_rmse: true position over the whole flight (env.tracking_error); recovery_bucket: the first 100 ms "
                   "bucket after the poke from which the rms deviation stays within `level`, -1: never")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print("wrote", args.json)


if __name__ == "__main__":
    main()
