#!/usr/bin/env python3
"""What flying a bank at deployment conditions costs -> profiles/bank_rate.json.
    python tools/bank_rate.py [--envs 65536] [--steps 500] [--pairs 7] [--policies 1024]
The fused fp32 rollout of a policy bank on a moving setpoint with native interval 4 (k_rollout_fused_bank_rate: image and interval
chosen per wave, one policy per 64-env block by default) against the single-policy kernel at the same conditions
(k_rollout_fused_rate: one Raptor, native interval 4, the same reference) in the same process at the same shape, launches
alternating, each timed with HIP events on the device's stream; medians (tools/control_rate.py's protocol).  Both fly from the same
seed, so the envs are the same; the bank's policies are copies of the shipped one, so the flights are the same too and the two
kernels do the same work - what differs is where the image and the interval come from.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raptor_amd.l2f as l2f                                            # noqa: E402
from raptor_amd import build as rq_build, tracking                      # noqa: E402
from raptor_amd.foundation_policy import Raptor, load_weights           # noqa: E402
from raptor_amd.policy_bank import PolicyBank, block_policy_assignment  # noqa: E402

INTERVAL, DT = 4, 0.0025


def _world(device, n, steps):
    vector = l2f.vector(n)
    rng, env = vector.VectorRng(), vector.VectorEnvironment()
    params, state = vector.VectorParameters(), vector.VectorState()
    vector.initialize_rng(device, rng, 0)
    vector.initialize_environment(device, env)
    cfg = env.config
    cfg.dt, cfg.episode_step_limit = DT, steps
    env.config = cfg
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    return vector, env, params, state, rng


def rate(device, n, steps, pairs, n_policies):
    ref = l2f.Reference(device, tracking.lissajous(steps, DT, amplitude=(0.3, 0.15, 0.0), period=5.0))
    n_policies = min(n_policies, (n + 63) // 64)
    bank = PolicyBank(device, np.tile(load_weights(), (n_policies, 1)), native_interval=INTERVAL)
    ids = block_policy_assignment(n, n_policies)
    policy = Raptor(device, native_interval=INTERVAL)
    policy.reset()
    worlds = {"bank": _world(device, n, steps), "policy": _world(device, n, steps)}

    def launch(who):
        vector, env, params, state, rng = worlds[who]
        device.timer_start()
        if who == "bank":
            bank.fly(vector, device, env, params, state, rng, steps, ids, mode="fused", autoreset=True, reference=ref)
        else:
            vector.rollout(device, env, params, state, policy, rng, steps, mode="fused", autoreset=True, reference=ref)
        return device.timer_stop()

    order = ("policy", "bank")
    for who in order * 2:                         # warm-up: code objects loaded, the id table uploaded, clocks up
        launch(who)
    same = bool(np.array_equal(worlds["bank"][3].numpy(), worlds["policy"][3].numpy()))
    ms = {who: [] for who in order}
    for _ in range(pairs):
        for who in order:
            ms[who].append(launch(who))
    med = {who: statistics.median(v) for who, v in ms.items()}
    return {"envs": n, "steps": steps, "pairs": pairs, "policies": n_policies, "precision": "fp32", "autoreset": True, "tracked": True,
            "native_interval": INTERVAL, "dt": DT, "states_equal_after_warm_up": same,
            "policy_kernel": "k_rollout_fused_rate", "bank_kernel": "k_rollout_fused_bank_rate",
            "policy_ms": ms["policy"], "bank_ms": ms["bank"], "policy_median_ms": med["policy"], "bank_median_ms": med["bank"],
            "policy_env_steps_per_s": n * steps / (med["policy"] * 1e-3), "bank_env_steps_per_s": n * steps / (med["bank"] * 1e-3),
            "bank_over_policy_time": med["bank"] / med["policy"]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--policies", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bank_rate.json"))
    args = ap.parse_args()
    device = l2f.Device()
    out = {"library_sha256": rq_build.library_sha256(), "fused_fp32": rate(device, args.envs, args.steps, args.pairs, args.policies)}
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    f = out["fused_fp32"]
    print(f"fused fp32, tracked, native interval {INTERVAL}, {f['envs']} envs x {f['steps']} steps: one policy "
          f"{f['policy_median_ms']:.3f} ms, a bank of {f['policies']} {f['bank_median_ms']:.3f} ms, ratio {f['bank_over_policy_time']:.4f}")
