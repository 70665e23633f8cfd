#!/usr/bin/env python3
"""What a wrench schedule costs the fused fp32 rollout -> profiles/wrench_rate.json.
    python tools/wrench_rate.py [--envs 65536] [--steps 500] [--rounds 7]
Three launches of the same shape in one process, alternating, each timed with HIP events on the device's stream; medians:
  plain   k_rollout_fused: the shipped policy, no schedule;
  rate1   the RATE text at interval 1 with nothing attached.  A single policy at interval 1 is launched as k_rollout_fused, so the
          RATE text at interval 1 is reached through its bank twin, k_rollout_fused_bank_rate - the kernel whose text the
          schedule's kernel is: a bank of two copies of the shipped policy with intervals (1, 2), every block flown by copy 0;
  wrench  k_rollout_fused_wrench: the shipped policy on an env that carries a schedule of zeros (same bits as `plain`).
wrench / rate1 is what the schedule's loads and arithmetic cost; wrench / plain what a user pays who attaches one.
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
from raptor_amd import disturbances                # noqa: E402
from raptor_amd.foundation_policy import Raptor    # noqa: E402
from raptor_amd.policy_bank import PolicyBank      # noqa: E402


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
    sides = ("plain", "rate1", "wrench")
    worlds = {s: _world(device, n) for s in sides}
    policy = {s: Raptor(device) for s in ("plain", "wrench")}
    for p in policy.values():
        p.reset()
    weights = policy["plain"].weights
    bank = PolicyBank(device, np.stack([weights, weights]), native_interval=[1, 2])
    ids = np.zeros(n, np.uint32)
    limit = int(worlds["wrench"][1].config.episode_step_limit)
    zeros = l2f.WrenchBank(device, [disturbances.calm(limit)])
    worlds["wrench"][1].set_wrench_schedule(zeros)

    def launch(side):
        vector, env, params, state, rng = worlds[side]
        device.timer_start()
        if side == "rate1":
            bank.fly(vector, device, env, params, state, rng, steps, ids, "fused", True)
        else:
            vector.rollout(device, env, params, state, policy[side], rng, steps, mode="fused", autoreset=True)
        return device.timer_stop()

    for side in sides + sides:                     # warm-up: code objects loaded, clocks up
        launch(side)
    ms = {s: [] for s in sides}
    for _ in range(rounds):
        for side in sides:
            ms[side].append(launch(side))
    device.synchronize()
    same = np.array_equal(worlds["plain"][3].numpy().view(np.uint32), worlds["wrench"][3].numpy().view(np.uint32))
    med = {s: statistics.median(v) for s, v in ms.items()}
    return {"envs": n, "steps": steps, "rounds": rounds, "precision": "fp32", "autoreset": True, "table_rows": limit,
            "ms": ms, "median_ms": med, "env_steps_per_s": {s: n * steps / (med[s] * 1e-3) for s in sides},
            "wrench_over_plain_time": med["wrench"] / med["plain"], "wrench_over_rate1_time": med["wrench"] / med["rate1"],
            "rate1_over_plain_time": med["rate1"] / med["plain"], "zero_table_state_equals_plain": bool(same)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wrench_rate.json"))
    args = ap.parse_args()
    device = l2f.Device()
    out = {"library_sha256": rq_build.library_sha256(), "fused_fp32": rate(device, args.envs, args.steps, args.rounds)}
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    f = out["fused_fp32"]
    print(f"fused fp32, {f['envs']} envs x {f['steps']} steps: plain {f['median_ms']['plain']:.3f} ms, RATE text at interval 1 "
          f"{f['median_ms']['rate1']:.3f} ms, zero-table schedule {f['median_ms']['wrench']:.3f} ms; wrench / plain "
          f"{f['wrench_over_plain_time']:.4f}, wrench / rate1 {f['wrench_over_rate1_time']:.4f}; same bits as plain: "
          f"{f['zero_table_state_equals_plain']}")
