#!/usr/bin/env python3
"""What one policy per wave costs -> profiles/policy_bank_rate.json.
    python tools/policy_bank_rate.py [--envs 65536] [--steps 500] [--policies 1024] [--rounds 7]
The fused fp32 rollout (no observation noise, auto-reset) three ways in one process at one shape, launches alternating, each timed
with HIP events on the device's stream; medians:
    single    rq_rollout with one policy (k_rollout_fused: every wave loads the same, L2-resident 18 KB image)
    distinct  rq_rollout_policies with `policies` distinct policies dealt round-robin (k_rollout_fused_bank: 18 KB per wave from HBM)
    one_id    rq_rollout_policies with one id everywhere (the bank kernel reading one image: what the table look-up itself costs)
The single-policy time of the same run is the yardstick; nothing is gated on a number.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raptor_amd.l2f as l2f                                              # noqa: E402
from raptor_amd import build as rq_build                                  # noqa: E402
from raptor_amd.foundation_policy import Raptor, load_weights             # noqa: E402
from raptor_amd.policy_bank import PolicyBank, block_policy_assignment    # noqa: E402


def _world(device, n):
    vector = l2f.vector(n)
    rng, env = vector.VectorRng(), vector.VectorEnvironment()
    params, state = vector.VectorParameters(), vector.VectorState()
    vector.initialize_rng(device, rng, 0)
    vector.initialize_environment(device, env)
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    return vector, env, params, state, rng


def rate(device, n, steps, n_policies, rounds):
    w0 = load_weights()
    # small perturbations: every policy keeps its quadrotors flying, so the three ways step the same mix of episodes
    W = np.stack([w0 + np.float32(1e-3) * np.random.default_rng(100 + k).standard_normal(w0.size).astype(np.float32)
                  for k in range(n_policies)]).astype(np.float32)
    actors = {"single": (Raptor(device, weights=W[0]), None),
              "distinct": (PolicyBank(device, W), block_policy_assignment(n, n_policies)),
              "one_id": (PolicyBank(device, W), np.zeros(n, np.uint32))}
    worlds = {k: _world(device, n) for k in actors}

    def launch(k):
        vector, env, params, state, rng = worlds[k]
        actor, ids = actors[k]
        device.timer_start()
        vector.rollout(device, env, params, state, actor, rng, steps, mode="fused", autoreset=True, policy_ids=ids)
        return device.timer_stop()

    for k in list(actors) * 2:                    # warm-up: code objects loaded, id tables uploaded, clocks up
        launch(k)
    ms = {k: [] for k in actors}
    for _ in range(rounds):
        for k in actors:
            ms[k].append(launch(k))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"envs": n, "steps": steps, "policies": n_policies, "rounds": rounds, "precision": "fp32", "noise": False, "autoreset": True}
    for k in actors:
        out[k + "_ms"] = ms[k]
        out[k + "_median_ms"] = med[k]
        out[k + "_env_steps_per_s"] = n * steps / (med[k] * 1e-3)
    out["distinct_over_single_time"] = med["distinct"] / med["single"]
    out["one_id_over_single_time"] = med["one_id"] / med["single"]
    out["distinct_over_one_id_time"] = med["distinct"] / med["one_id"]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--policies", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_bank_rate.json"))
    args = ap.parse_args()
    device = l2f.Device()
    out = {"library_sha256": rq_build.library_sha256(), "fused_fp32": rate(device, args.envs, args.steps, args.policies, args.rounds)}
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    f = out["fused_fp32"]
    print(f"fused fp32, {f['envs']} envs x {f['steps']} steps: single {f['single_median_ms']:.3f} ms, {f['policies']} distinct policies "
          f"{f['distinct_median_ms']:.3f} ms (x{f['distinct_over_single_time']:.4f}), one id everywhere {f['one_id_median_ms']:.3f} ms "
          f"(x{f['one_id_over_single_time']:.4f})")
