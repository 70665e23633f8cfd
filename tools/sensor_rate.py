#!/usr/bin/env python3
"""What a sensor schedule costs a rollout -> profiles/sensor_rate.json.
    python tools/sensor_rate.py [--envs 65536] [--steps 500] [--rounds 5]
Six launches of the same shape in one process on one build, alternating, each timed with HIP events on the device's stream; medians:
  fused    plain    k_rollout_fused: the shipped policy, no schedule;
           zeros    k_rollout_fused_sensor on a sensor schedule of zeros (same bits as `plain`): the byte of delay per step and the
                    18 stores of the reading into the env's ring, no read of it;
           four     k_rollout_fused_sensor on a constant delay of four steps (10 ms at 400 Hz): the 18 loads out of the ring too;
           delay4   k_rollout_fused_delay on a constant command delay of four steps: the other side of the loop, 16 + 16 B per
                    env-step against this one's 72 + 72 B;
  chained  plain    the chained launch (a replayed graph of actor and step kernels), no schedule;
           four     the same with k_sensor_apply as a third node per step, on a constant delay of four steps.
four / plain is what a user pays who attaches one; fused four / chained four is the condition the fused kernel was built under: it
must take less time than the chained launch with the same schedule.
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
from raptor_amd import delays, sensors             # noqa: E402
from raptor_amd.foundation_policy import Raptor    # noqa: E402

SIDES = (("fused", "plain"), ("fused", "zeros"), ("fused", "four"), ("fused", "delay4"), ("chained", "plain"), ("chained", "four"))


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
    worlds = {s: _world(device, n) for s in SIDES}
    policy = {s: Raptor(device) for s in SIDES}
    for p in policy.values():
        p.reset()
    limit = int(worlds[SIDES[0]][1].config.episode_step_limit)
    worlds[("fused", "zeros")][1].set_sensor_schedule(l2f.SensorBank(device, [sensors.none(limit)]))
    four = l2f.SensorBank(device, [sensors.constant(limit, 4)])
    worlds[("fused", "four")][1].set_sensor_schedule(four)
    worlds[("chained", "four")][1].set_sensor_schedule(four)
    worlds[("fused", "delay4")][1].set_delay_schedule(l2f.DelayBank(device, [delays.constant(limit, 4)]))

    def launch(side):
        vector, env, params, state, rng = worlds[side]
        device.timer_start()
        vector.rollout(device, env, params, state, policy[side], rng, steps, mode=side[0], autoreset=True)
        return device.timer_stop()

    for side in SIDES + SIDES:                     # warm-up: code objects loaded, graphs built, clocks up
        launch(side)
    ms = {s: [] for s in SIDES}
    for _ in range(rounds):
        for side in SIDES:
            ms[side].append(launch(side))
    device.synchronize()
    state = {s: worlds[s][3].numpy().view(np.uint32) for s in SIDES}
    med = {s: statistics.median(v) for s, v in ms.items()}
    name = {s: f"{s[0]}_{s[1]}" for s in SIDES}
    fp, fz, f4, fd, cp, c4 = (med[s] for s in SIDES)
    return {"envs": n, "steps": steps, "rounds": rounds, "precision": "fp32", "autoreset": True, "table_rows": limit,
            "ms": {name[s]: ms[s] for s in SIDES}, "median_ms": {name[s]: med[s] for s in SIDES},
            "env_steps_per_s": {name[s]: n * steps / (med[s] * 1e-3) for s in SIDES},
            "fused_four_over_plain_time": f4 / fp, "fused_zeros_over_plain_time": fz / fp, "fused_four_over_zeros_time": f4 / fz,
            "fused_four_over_delay4_time": f4 / fd, "fused_delay4_over_plain_time": fd / fp,
            "chained_four_over_plain_time": c4 / cp, "fused_four_over_chained_four_time": f4 / c4,
            "fused_four_is_faster_than_chained_four": bool(f4 < c4),
            "state_equals": {"fused_zeros_fused_plain": bool(np.array_equal(state[("fused", "zeros")], state[("fused", "plain")])),
                             "chained_plain_fused_plain": bool(np.array_equal(state[("chained", "plain")], state[("fused", "plain")])),
                             "chained_four_fused_four": bool(np.array_equal(state[("chained", "four")], state[("fused", "four")])),
                             "fused_four_fused_plain": bool(np.array_equal(state[("fused", "four")], state[("fused", "plain")]))}}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensor_rate.json"))
    args = ap.parse_args()
    device = l2f.Device()
    out = {"library_sha256": rq_build.library_sha256(), "fp32": rate(device, args.envs, args.steps, args.rounds)}
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    f = out["fp32"]
    m = f["median_ms"]
    print(f"fp32, {f['envs']} envs x {f['steps']} steps: fused plain {m['fused_plain']:.3f} ms, sensor schedule of zeros "
          f"{m['fused_zeros']:.3f} ms, of four steps {m['fused_four']:.3f} ms, delay schedule of four steps {m['fused_delay4']:.3f} ms; "
          f"chained plain {m['chained_plain']:.3f} ms, sensor schedule of four steps {m['chained_four']:.3f} ms; fused four / plain "
          f"{f['fused_four_over_plain_time']:.4f}, zeros / plain {f['fused_zeros_over_plain_time']:.4f}, chained four / plain "
          f"{f['chained_four_over_plain_time']:.4f}, fused four / chained four {f['fused_four_over_chained_four_time']:.4f}; "
          f"same bits: {f['state_equals']} (fused_four_fused_plain: expected False)")
