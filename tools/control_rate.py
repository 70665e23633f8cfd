#!/usr/bin/env python3
"""What the native interval costs and what it changes -> profiles/control_rate.json.
    python tools/control_rate.py [--envs 65536] [--steps 500] [--pairs 7]
Rate: the fused fp32 rollout of a policy with native interval 4 (k_rollout_fused_rate) against the plain kernel's (k_rollout_fused,
interval 1) in the same process at the same shape, launches alternating, each timed with HIP events on the device's stream; medians.
Statistics: the three rows of examples/deployment_rate.py (100 Hz R = 1, 400 Hz R = 4, 400 Hz R = 1), and the nominal Crazyflie
from hover at 400 Hz with both intervals (what tests/test_gpu_control_rate.py prints).
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raptor_amd.l2f as l2f                       # noqa: E402
from raptor_amd import build as rq_build           # noqa: E402
from raptor_amd.foundation_policy import Raptor    # noqa: E402


def _example():
    spec = importlib.util.spec_from_file_location("deployment_rate", os.path.join(ROOT, "examples", "deployment_rate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _world(device, n, interval, **cfg_over):
    vector = l2f.vector(n)
    rng, env = vector.VectorRng(), vector.VectorEnvironment()
    params, state = vector.VectorParameters(), vector.VectorState()
    vector.initialize_rng(device, rng, 0)
    vector.initialize_environment(device, env)
    cfg = env.config
    for k, v in cfg_over.items():
        setattr(cfg, k, v)
    env.config = cfg
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    policy = Raptor(device, native_interval=interval)
    policy.reset()
    return vector, env, params, state, policy, rng


def rate(device, n, steps, pairs):
    worlds = {r: _world(device, n, r) for r in (1, 4)}

    def launch(r):
        vector, env, params, state, policy, rng = worlds[r]
        device.timer_start()
        vector.rollout(device, env, params, state, policy, rng, steps, mode="fused", autoreset=True)
        return device.timer_stop()

    for r in (1, 4, 1, 4):                        # warm-up: code objects loaded, clocks up
        launch(r)
    ms = {1: [], 4: []}
    for _ in range(pairs):
        for r in (1, 4):
            ms[r].append(launch(r))
    med = {r: statistics.median(v) for r, v in ms.items()}
    return {"envs": n, "steps": steps, "pairs": pairs, "precision": "fp32", "autoreset": True,
            "plain_ms": ms[1], "rate_ms": ms[4], "plain_median_ms": med[1], "rate_median_ms": med[4],
            "plain_env_steps_per_s": n * steps / (med[1] * 1e-3), "rate_env_steps_per_s": n * steps / (med[4] * 1e-3),
            "rate_over_plain_time": med[4] / med[1]}


def nominal(device, interval):
    vector, env, params, state, policy, rng = _world(device, 64, interval, domain_randomization=0, init_guidance=1.0, dt=0.0025,
                                                     episode_step_limit=2000)
    vector.rollout(device, env, params, state, policy, rng, 2000, mode="fused", autoreset=False)
    return {"native_interval": interval, "dt": 0.0025, "envs": 64, "terminated": float(env.finished_terminated().mean()),
            "final_position_error_m": float(np.linalg.norm(state.numpy()[:, :3], axis=1).mean())}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "control_rate.json"))
    args = ap.parse_args()
    device = l2f.Device()
    ex = _example()
    out = {"library_sha256": rq_build.library_sha256(),
           "fused_fp32": rate(device, args.envs, args.steps, args.pairs),
           "deployment_rate": [dict(name=name, **ex.fly(device, 4096, dt, r)) for name, dt, r in ex.WAYS],
           "deployment_rate_figure_eight": [dict(name=name, **ex.fly(device, 4096, dt, r, figure_eight=True)) for name, dt, r in ex.WAYS],
           "nominal_hover_400hz": [nominal(device, 4), nominal(device, 1)]}
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    f = out["fused_fp32"]
    print(f"fused fp32, {f['envs']} envs x {f['steps']} steps: plain {f['plain_median_ms']:.3f} ms, native interval 4 "
          f"{f['rate_median_ms']:.3f} ms, ratio {f['rate_over_plain_time']:.4f}")
    for row in out["deployment_rate"] + out["deployment_rate_figure_eight"] + out["nominal_hover_400hz"]:
        print(row)
