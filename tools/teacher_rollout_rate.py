#!/usr/bin/env python3
"""Rate of teacher rollouts (rq_rollout_teachers): a bank of 22-64-64-4 MLP teachers flying 65 536 envs for 100 steps, fused
(k_rollout_teachers, one launch) against chained (observe -> the bank's relabel kernel at T = 1 -> step, per step), the two
alternating round by round, each round timed on the host around the call + a device synchronise after a warm-up.  Beside them the
student's fused rollout (k_rollout_fused) on the same envs for scale.  The matrix-core fraction is the teachers' model FLOP per
env-step (2 (in h1 + h1 h2 + 4 h2)) x env-steps / time / 157.3 TFLOP/s (the f32 MFMA peak).

--track single | bank16: the same two launches on a moving setpoint (TeacherBank.fly with one figure-eight, or with a bank of 16
figure-eights of different periods, ids dealt inside every teacher's envs) timed in the SAME alternating rounds, and the ratios
tracked / untracked recorded.  --parent-json FILE: a result of this tool made with another build of the library (RAPTOR_QUAD_LIB,
same box, same call: tools/ab_run.sh) - this build's untracked fused median is recorded beside that build's median and the spread of
its rounds, with whether it lies outside that spread on the slow side.

    python tools/teacher_rollout_rate.py [--envs 65536] [--steps 100] [--rounds 5] [--track none] [--parent-json FILE]
                                         [--json profiles/teacher_rollout_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                                                     # noqa: E402
from raptor_amd import build, tracking                                           # noqa: E402
from raptor_amd.foundation_policy import Raptor                                  # noqa: E402
from raptor_amd.teachers import TeacherBank, balanced_teacher_assignment, parameter_count    # noqa: E402

F32_PEAK = 157.3e12

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--json", default=None)
ap.add_argument("--track", choices=("none", "single", "bank16"), default="none")
ap.add_argument("--parent-json", default=None)
args = ap.parse_args()
parent = json.load(open(args.parent_json)) if args.parent_json else None

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


# the setpoints: figure-eights inside termination_position, tables as long as an episode
reference = None
if args.track != "none":
    cfg = env.config
    rows, dt = int(cfg.episode_step_limit), float(cfg.dt)
    eight = lambda period: tracking.lissajous(rows, dt, amplitude=(0.3, 0.15, 0.0), period=period)      # noqa: E731
    reference = l2f.Reference(device, eight(5.0)) if args.track == "single" else \
        l2f.ReferenceBank(device, [eight(4.0 + 0.5 * r) for r in range(16)])

out = dict(envs=n, steps=T, rounds=args.rounds, teacher="22-64-64-4 relu/tanh fp32", flop_per_env_step=flop,
           f32_mfma_peak_flops=F32_PEAK, library_sha256=build.library_sha256(os.environ.get("RAPTOR_QUAD_LIB") or build.LIB),
           track=args.track, configs=[])
for n_teachers in (1000, 64):
    w = np.random.default_rng(n_teachers).standard_normal((n_teachers, parameter_count(22, 64, 64))) * 0.1
    bank = TeacherBank(device, w.astype(np.float32), 22, 64, 64, "relu", "tanh")
    ids = balanced_teacher_assignment(n, n_teachers)
    runs = {m: (lambda m=m: vector.rollout(device, env, params, state, bank, rng, T, m, True, teacher_ids=ids)) for m in ("fused", "chained")}
    if reference is not None:
        ref_ids = tracking.spread_reference_ids(n, 16, ids) if args.track == "bank16" else None
        for m in ("fused", "chained"):
            runs[m + "_tracked"] = lambda m=m: bank.fly(vector, device, env, params, state, rng, T, ids, m, True, reference=reference,
                                                        reference_ids=ref_ids)
    for m in runs:                               # warm-up: code objects, tile list upload, scratch
        timed(runs[m])
    times = {m: [] for m in runs}
    for _ in range(args.rounds):
        for m in runs:
            times[m].append(timed(runs[m]))
    rec = dict(teachers=n_teachers)
    for m, ts in times.items():
        med = float(np.median(ts))
        rec[m] = dict(seconds=[round(t, 6) for t in ts], median_s=round(med, 6), env_steps_per_s=n * T / med,
                      matrix_core_fraction=flop * n * T / med / F32_PEAK)
    rec["fused_over_chained_speedup"] = rec["chained"]["median_s"] / rec["fused"]["median_s"]
    if reference is not None:
        rec["tracked_over_untracked"] = {m: rec[m + "_tracked"]["median_s"] / rec[m]["median_s"] for m in ("fused", "chained")}
    if parent is not None:       # this build's untracked launches against the other build's median and the spread of its rounds
        theirs = next(c for c in parent["configs"] if c["teachers"] == n_teachers)
        rec["untracked_against_parent"] = {}
        for m in ("fused", "chained"):
            lo, hi = min(theirs[m]["seconds"]), max(theirs[m]["seconds"])
            rec["untracked_against_parent"][m] = dict(parent_median_s=theirs[m]["median_s"], parent_min_s=lo, parent_max_s=hi,
                                                      this_median_s=rec[m]["median_s"], ratio=rec[m]["median_s"] / theirs[m]["median_s"],
                                                      outside_parent_spread_on_the_slow_side=rec[m]["median_s"] > hi)
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
if parent is not None:
    out["parent"] = dict(library_sha256=parent.get("library_sha256"), configs=parent["configs"], student_fused=parent.get("student_fused"))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
