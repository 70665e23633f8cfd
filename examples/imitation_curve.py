#!/usr/bin/env python3
"""Which teachers does the student imitate badly, and how does its error fall with episode age?  Fly the student with auto-reset,
relabel what it visited with a bank of MLP teachers - one teacher per group of quadrotors -, and score the student against those
labels per env and bucket of episode age in ONE forward pass on the device (raptor_amd.training.imitation_error): no backward, no
action tensor, no pass over the done codes on the host.  Everything below the call is small algebra on the [buckets, envs] table.

Random 22-64-64-4 teachers stand in for trained ones, each with its own output scale so that they differ in how far they are from
the student; the figures say how the table is read, not how good a policy is.

    python examples/imitation_curve.py [--envs 16384] [--steps 500] [--teachers 64] [--buckets 10] [--json profiles/imitation_curve.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                                    # noqa: E402
from raptor_amd import probing                                  # noqa: E402
from raptor_amd.foundation_policy import Raptor                 # noqa: E402
from raptor_amd.teachers import TeacherBank, balanced_teacher_assignment, parameter_count    # noqa: E402
from raptor_amd.training import imitation_error                 # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--teachers", type=int, default=64)
    ap.add_argument("--buckets", type=int, default=10)
    ap.add_argument("--json", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "imitation_curve.json"))
    args = ap.parse_args()

    device = l2f.Device()
    vector = l2f.vector(args.envs)
    rng, env = vector.VectorRng(), vector.VectorEnvironment()
    params, state = vector.VectorParameters(), vector.VectorState()
    vector.initialize_rng(device, rng, 0)
    vector.initialize_environment(device, env)
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    student = Raptor(device)
    student.reset()

    traj = vector.Trajectory(env, args.steps)
    vector.rollout(device, env, params, state, student, rng, args.steps, "fused", autoreset=True, trajectory=traj)
    K = args.teachers
    weights = np.random.default_rng(1).standard_normal((K, parameter_count(22, 64, 64))).astype(np.float32) * 0.1
    weights *= np.linspace(0.2, 2.0, K, dtype=np.float32)[np.random.default_rng(2).permutation(K), None]
    bank = TeacherBank(device, weights, 22, 64, 64, "relu", "tanh")
    teacher_of = balanced_teacher_assignment(env.N_ENVIRONMENTS, K)
    traj.relabel_teachers(bank, teacher_of, overwrite=True, fetch=False)      # the stored actions are the teachers' now
    device.synchronize()

    edges = probing.log_age_edges(min(args.steps, int(env.config.episode_step_limit)), args.buckets)
    imitation_error(traj, student, edges=edges)                               # code objects, workspaces
    device.synchronize()
    t0 = time.perf_counter()
    table = imitation_error(traj, student, edges=edges)                       # target=None: the stored actions
    device.synchronize()
    ms = (time.perf_counter() - t0) * 1e3

    def host(x):
        return np.asarray(x.cpu() if hasattr(x, "data_ptr") else x, np.float64)

    by_age, per_teacher = host(table.by_age()), host(table.by_group(teacher_of, K))        # [B], [K, B]
    counts = host(table.count).sum(1)
    s, c = host(table.sse), host(table.count)
    teacher_mse = np.asarray([s[:, teacher_of == k].sum() / (4 * max(c[:, teacher_of == k].sum(), 1)) for k in range(K)])
    worst = np.argsort(-teacher_mse)[:5]
    print(f"{env.N_ENVIRONMENTS} envs x {args.steps} steps, {K} teachers: the table in {ms:.2f} ms; loss {float(table.loss()):.5f}")
    print("age bucket        steps      mse")
    for b in range(args.buckets):
        print(f"[{int(edges[b]):4d}, {int(edges[b + 1]):4d})  {int(counts[b]):9d}  {by_age[b]:.5f}")
    print("the five teachers the student imitates worst (mse over all ages; by age bucket):")
    for k in worst:
        print(f"  teacher {int(k):3d}: {teacher_mse[k]:.5f}   " + " ".join(f"{v:.3f}" for v in per_teacher[k]))
    out = dict(envs=int(env.N_ENVIRONMENTS), steps=args.steps, teachers=K, age_edges=[int(e) for e in edges],
               table_ms=ms, loss=float(table.loss()), steps_per_bucket=[int(v) for v in counts], mse_by_age=[float(v) for v in by_age],
               teacher_mse=[float(v) for v in teacher_mse], worst_teachers=[int(k) for k in worst],
               worst_teachers_mse_by_age=[[float(v) for v in per_teacher[k]] for k in worst],
               note="random MLP teachers with output scales 0.2 .. 2.0 stand in for trained ones: the figures show how the table is "
                    "read, not how good a policy is")
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.json)


if __name__ == "__main__":
    main()
