#!/usr/bin/env python3
"""Fly every teacher of a bank on its own quadrotors for one episode length and print its closed-loop record: the first check after
pre-training (per-teacher return and termination share).

    python examples/evaluate_teachers.py [--envs 16384] [--teachers 64] [--checkpoints DIR] [--worst 10] [--mode fused|chained]

Without --checkpoints the bank holds random stand-in teachers (the trained ones are not in the reference tree): expect them to crash.
"""
import argparse
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                                                           # noqa: E402
from raptor_amd.teachers import (TeacherBank, balanced_teacher_assignment, parameter_count,  # noqa: E402
                                 teacher_episode_table)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--teachers", type=int, default=64)
    ap.add_argument("--checkpoints", default=None, help="directory of teacher checkpoints (*.h5) in the reference's layout")
    ap.add_argument("--worst", type=int, default=10)
    ap.add_argument("--mode", default="fused", choices=["fused", "chained"])
    args = ap.parse_args()

    device = l2f.Device()
    vector = l2f.vector(args.envs)
    rng, env = vector.VectorRng(), vector.VectorEnvironment()
    params, state = vector.VectorParameters(), vector.VectorState()
    vector.initialize_rng(device, rng, 0)
    vector.initialize_environment(device, env)
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    if args.checkpoints:
        bank = TeacherBank.from_checkpoints(device, sorted(glob.glob(os.path.join(args.checkpoints, "*.h5"))))
    else:
        w = np.random.default_rng(1).standard_normal((args.teachers, parameter_count(22, 64, 64))) * 0.1
        bank = TeacherBank(device, w.astype(np.float32), 22, 64, 64, "relu", "tanh")
    ids = balanced_teacher_assignment(env.N_ENVIRONMENTS, bank.n_teachers)
    steps = env.config.episode_step_limit
    env.reset_statistics()
    vector.rollout(device, env, params, state, bank, rng, steps, args.mode, autoreset=True, teacher_ids=ids)
    tab = teacher_episode_table(env, ids, bank.n_teachers)
    print(f"{bank.n_teachers} teachers x {env.N_ENVIRONMENTS} envs, {steps} steps ({args.mode}): "
          f"{int(tab['episodes'].sum())} episodes finished, mean return {np.nanmean(tab['mean_return']):.3f}, "
          f"termination share {np.nansum(tab['termination_share'] * tab['episodes']) / max(1, tab['episodes'].sum()):.3f}")
    print(f"{'teacher':>8} {'envs':>6} {'episodes':>9} {'mean return':>12} {'mean length':>12} {'terminated':>11}")
    order = np.argsort(np.nan_to_num(tab["mean_return"], nan=-np.inf))
    for k in order[:args.worst]:
        print(f"{k:8d} {tab['envs'][k]:6d} {tab['episodes'][k]:9d} {tab['mean_return'][k]:12.3f} {tab['mean_length'][k]:12.1f} "
              f"{tab['termination_share'][k]:11.3f}")


if __name__ == "__main__":
    main()
