#!/usr/bin/env python3
"""What a wind schedule costs the fused fp32 rollout -> profiles/wind_rate.json.
    python tools/wind_rate.py [--envs 65536] [--steps 500] [--rounds 5]
Four launches of the same shape in one process on one build, alternating, each timed with HIP events on the device's stream; medians:
  plain    k_rollout_fused: the shipped policy, no schedule;
  wrench   k_rollout_fused_wrench: the shipped policy on an env that carries a wrench schedule of zeros (same bits as `plain`);
  vehicle  k_rollout_fused_vehicle: the shipped policy on an env that carries a vehicle schedule of ones (same bits as `plain`);
  wind     k_rollout_fused_wind: the shipped policy on an env that carries a wind schedule without drag (same bits as `plain`).
wind / plain is what a user pays who attaches one - a 16-byte row, a product for m d, three differences, three products and three
sums per step of the lone wave, and the disturbance folded anew; wind / wrench and wind / vehicle stand it beside the other
schedules' kernels, built from the same text.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raptor_amd.l2f as l2f                       # noqa: E402
from raptor_amd import build as rq_build           # noqa: E402
from raptor_amd import disturbances, vehicles, winds   # noqa: E402
from raptor_amd.foundation_policy import Raptor    # noqa: E402


def _world(device, n):
    vector = l2f.VectorModule(n, 0)
    rng, env = vector.VectorRng(), vector.VectorEnvironment()
    params, state = vector.VectorParameters(), vector.VectorState()
    vector.initialize_rng(device, rng, 0)
    vector.initialize_environment(device, env)
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    return vector, env, params, state, rng


def rate(device, n, steps, rounds):
    sides = ("plain", "wrench", "vehicle", "wind")
    worlds = {s: _world(device, n) for s in sides}
    policy = {s: Raptor(device) for s in sides}
    for p in policy.values():
        p.reset()
    limit = int(worlds["plain"][1].config.episode_step_limit)
    worlds["wrench"][1].set_wrench_schedule(l2f.WrenchBank(device, [disturbances.calm(limit)]))
    worlds["vehicle"][1].set_vehicle_schedule(l2f.VehicleBank(device, [vehicles.nominal(limit)]))
    worlds["wind"][1].set_wind_schedule(l2f.WindBank(device, [winds.steady(limit, (5.0, 0.0, 0.0), 0.0)]))

    def launch(side):
        vector, env, params, state, rng = worlds[side]
        device.timer_start()
        vector.rollout(device, env, params, state, policy[side], rng, steps, mode="fused", autoreset=True)
        return device.timer_stop()

    for side in sides + sides:                     # warm-up: code objects loaded, clocks up
        launch(side)
    ms = {s: [] for s in sides}
    for _ in range(rounds):
        for side in sides:
            ms[side].append(launch(side))
    device.synchronize()
    plain = worlds["plain"][3].numpy().view(np.uint32)
    same = {s: bool(np.array_equal(plain, worlds[s][3].numpy().view(np.uint32))) for s in ("wrench", "vehicle", "wind")}
    med = {s: statistics.median(v) for s, v in ms.items()}
    return {"envs": n, "steps": steps, "rounds": rounds, "precision": "fp32", "autoreset": True, "table_rows": limit,
            "ms": ms, "median_ms": med, "env_steps_per_s": {s: n * steps / (med[s] * 1e-3) for s in sides},
            "wind_over_plain_time": med["wind"] / med["plain"], "wind_over_wrench_time": med["wind"] / med["wrench"],
            "wind_over_vehicle_time": med["wind"] / med["vehicle"], "vehicle_over_plain_time": med["vehicle"] / med["plain"],
            "wrench_over_plain_time": med["wrench"] / med["plain"], "identity_state_equals_plain": same}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wind_rate.json"))
    args = ap.parse_args()
    device = l2f.Device()
    out = {"library_sha256": rq_build.library_sha256(), "fused_fp32": rate(device, args.envs, args.steps, args.rounds)}
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    f = out["fused_fp32"]
    print(f"fused fp32, {f['envs']} envs x {f['steps']} steps: plain {f['median_ms']['plain']:.3f} ms, zero-table wrench schedule "
          f"{f['median_ms']['wrench']:.3f} ms, all-ones vehicle schedule {f['median_ms']['vehicle']:.3f} ms, drag-free wind schedule "
          f"{f['median_ms']['wind']:.3f} ms; wind / plain {f['wind_over_plain_time']:.4f}, wind / wrench "
          f"{f['wind_over_wrench_time']:.4f}, wind / vehicle {f['wind_over_vehicle_time']:.4f}; same bits as plain: "
          f"{f['identity_state_equals_plain']}")
