#!/usr/bin/env python3
"""What a delay schedule costs the fused fp32 rollout -> profiles/delay_rate.json.
    python tools/delay_rate.py [--envs 65536] [--steps 500] [--rounds 5]
Four launches of the same shape in one process on one build, alternating, each timed with HIP events on the device's stream; medians:
  plain    k_rollout_fused: the shipped policy, no schedule;
  wind     k_rollout_fused_wind: the shipped policy on an env that carries a wind schedule without drag (same bits as `plain`);
  zeros    k_rollout_fused_delay: the shipped policy on an env that carries a delay schedule of zeros (same bits as `plain`): the
           byte of delay per step and the four stores of the command into the env's history, no read of it;
  four     k_rollout_fused_delay on a constant delay of four steps (10 ms at 400 Hz): the four loads out of the history too.
four / plain is what a user pays who attaches one; four / wind stands it beside the wind schedule's kernel, built from the same
text; four / zeros is the history's read.
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
from raptor_amd import delays, winds               # noqa: E402
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
    sides = ("plain", "wind", "zeros", "four")
    worlds = {s: _world(device, n) for s in sides}
    policy = {s: Raptor(device) for s in sides}
    for p in policy.values():
        p.reset()
    limit = int(worlds["plain"][1].config.episode_step_limit)
    worlds["wind"][1].set_wind_schedule(l2f.WindBank(device, [winds.steady(limit, (5.0, 0.0, 0.0), 0.0)]))
    worlds["zeros"][1].set_delay_schedule(l2f.DelayBank(device, [delays.none(limit)]))
    worlds["four"][1].set_delay_schedule(l2f.DelayBank(device, [delays.constant(limit, 4)]))

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
    same = {s: bool(np.array_equal(plain, worlds[s][3].numpy().view(np.uint32))) for s in ("wind", "zeros", "four")}
    med = {s: statistics.median(v) for s, v in ms.items()}
    return {"envs": n, "steps": steps, "rounds": rounds, "precision": "fp32", "autoreset": True, "table_rows": limit,
            "ms": ms, "median_ms": med, "env_steps_per_s": {s: n * steps / (med[s] * 1e-3) for s in sides},
            "four_over_plain_time": med["four"] / med["plain"], "zeros_over_plain_time": med["zeros"] / med["plain"],
            "four_over_wind_time": med["four"] / med["wind"], "four_over_zeros_time": med["four"] / med["zeros"],
            "wind_over_plain_time": med["wind"] / med["plain"], "state_equals_plain": same}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delay_rate.json"))
    args = ap.parse_args()
    device = l2f.Device()
    out = {"library_sha256": rq_build.library_sha256(), "fused_fp32": rate(device, args.envs, args.steps, args.rounds)}
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    f = out["fused_fp32"]
    print(f"fused fp32, {f['envs']} envs x {f['steps']} steps: plain {f['median_ms']['plain']:.3f} ms, drag-free wind schedule "
          f"{f['median_ms']['wind']:.3f} ms, delay schedule of zeros {f['median_ms']['zeros']:.3f} ms, of four steps "
          f"{f['median_ms']['four']:.3f} ms; four / plain {f['four_over_plain_time']:.4f}, zeros / plain "
          f"{f['zeros_over_plain_time']:.4f}, four / wind {f['four_over_wind_time']:.4f}; same bits as plain: "
          f"{f['state_equals_plain']} (four: expected False)")
