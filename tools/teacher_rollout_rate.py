#!/usr/bin/env python3
"""Rate of teacher rollouts (rq_rollout_teachers): a bank of 22-64-64-4 MLP teachers flying 65 536 envs for 100 steps, fused
(k_rollout_teachers, one launch) against chained (observe -> the bank's relabel kernel at T = 1 -> step, per step), the two
alternating round by round, each round timed on the host around the call + a device synchronise after a warm-up.  Beside them the
student's fused rollout (k_rollout_fused) on the same envs for scale.  The matrix-core fraction is the teachers' model FLOP per
env-step (2 (in h1 + h1 h2 + 4 h2)) x env-steps / time / 157.3 TFLOP/s (the f32 MFMA peak).

    python tools/teacher_rollout_rate.py [--envs 65536] [--steps 100] [--rounds 5] [--json profiles/teacher_rollout_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                                                     # noqa: E402
from raptor_amd import build                                                     # noqa: E402
from raptor_amd.foundation_policy import Raptor                                  # noqa: E402
from raptor_amd.teachers import TeacherBank, balanced_teacher_assignment, parameter_count    # noqa: E402

F32_PEAK = 157.3e12

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()

device = l2f.Device()
vector = l2f.vector(args.envs)
rng, env = vector.VectorRng(), vector.VectorEnvironment()
params, state = vector.VectorParameters(), vector.VectorState()
vector.initialize_rng(device, rng, 0)
vector.initialize_environment(device, env)
vector.sample_initial_parameters(device, env, params, rng)
vector.sample_initial_state(device, env, params, state, rng)
n, T = env.N_ENVIRONMENTS, args.steps
flop = 2 * (22 * 64 + 64 * 64 + 4 * 64)


def timed(fn):
    device.synchronize()
    t0 = time.perf_counter()
    fn()
    device.synchronize()
    return time.perf_counter() - t0


out = dict(envs=n, steps=T, rounds=args.rounds, teacher="22-64-64-4 relu/tanh fp32", flop_per_env_step=flop,
           f32_mfma_peak_flops=F32_PEAK, library_sha256=build.library_sha256(), configs=[])
for n_teachers in (1000, 64):
    w = np.random.default_rng(n_teachers).standard_normal((n_teachers, parameter_count(22, 64, 64))) * 0.1
    bank = TeacherBank(device, w.astype(np.float32), 22, 64, 64, "relu", "tanh")
    ids = balanced_teacher_assignment(n, n_teachers)
    runs = {m: (lambda m=m: vector.rollout(device, env, params, state, bank, rng, T, m, True, teacher_ids=ids)) for m in ("fused", "chained")}
    for m in runs:                               # warm-up: code objects, tile list upload, scratch
        timed(runs[m])
    times = {"fused": [], "chained": []}
    for _ in range(args.rounds):
        for m in ("fused", "chained"):
            times[m].append(timed(runs[m]))
    rec = dict(teachers=n_teachers)
    for m, ts in times.items():
        med = float(np.median(ts))
        rec[m] = dict(seconds=[round(t, 6) for t in ts], median_s=round(med, 6), env_steps_per_s=n * T / med,
                      matrix_core_fraction=flop * n * T / med / F32_PEAK)
    rec["fused_over_chained_speedup"] = rec["chained"]["median_s"] / rec["fused"]["median_s"]
    out["configs"].append(rec)
    print(json.dumps(rec), flush=True)

student = Raptor(device)
student.reset()
run = lambda: vector.rollout(device, env, params, state, student, rng, T, "fused", True)      # noqa: E731
timed(run)
ts = [timed(run) for _ in range(args.rounds)]
med = float(np.median(ts))
out["student_fused"] = dict(seconds=[round(t, 6) for t in ts], median_s=round(med, 6), env_steps_per_s=n * T / med)
print(json.dumps(out["student_fused"]), flush=True)
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
