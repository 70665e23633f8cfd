#!/usr/bin/env python3
"""Fly every teacher of a bank on its own quadrotors for one episode length and print its closed-loop record: the first check after
pre-training (per-teacher return and termination share).

    python examples/evaluate_teachers.py [--envs 16384] [--teachers 64] [--checkpoints DIR] [--worst 10] [--mode fused|chained]
                                         [--figure-eight | --suite]

--figure-eight: every teacher tracks the 0.3 m x 0.15 m figure-eight of examples/track_figure_eight.py from hover at the origin, and
the table gains its RMS distance to the setpoint - what a student's tracking error stands against.  --suite: the same ONE launch
flies every teacher on the setpoints of raptor_amd.tracking.suite, dealt evenly inside every teacher's envs: a column per setpoint.
Without --checkpoints the bank holds random stand-in teachers (the trained ones are not in the reference tree): expect them to crash.
"""
import argparse
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                                                           # noqa: E402
from raptor_amd import tracking                                                        # noqa: E402
from raptor_amd.teachers import TeacherBank, balanced_teacher_assignment, parameter_count    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--teachers", type=int, default=64)
    ap.add_argument("--checkpoints", default=None, help="directory of teacher checkpoints (*.h5) in the reference's layout")
    ap.add_argument("--worst", type=int, default=10)
    ap.add_argument("--mode", default="fused", choices=["fused", "chained"])
    ap.add_argument("--figure-eight", action="store_true", help="track a figure-eight instead of holding the origin")
    ap.add_argument("--suite", action="store_true", help="track a suite of setpoints, a reference per env: the RMSE table is [K, M]")
    args = ap.parse_args()
    if args.figure_eight and args.suite:
        ap.error("--figure-eight and --suite do not combine: the suite holds the figure-eight")

    device = l2f.Device()
    vector = l2f.vector(args.envs)
    rng, env = vector.VectorRng(), vector.VectorEnvironment()
    params, state = vector.VectorParameters(), vector.VectorState()
    vector.initialize_rng(device, rng, 0)
    vector.initialize_environment(device, env)
    cfg = env.config
    if args.figure_eight or args.suite:
        cfg.init_guidance = 1.0                    # hover at the origin, where the path starts
        env.config = cfg
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    if args.checkpoints:
        bank = TeacherBank.from_checkpoints(device, sorted(glob.glob(os.path.join(args.checkpoints, "*.h5"))))
    else:
        w = np.random.default_rng(1).standard_normal((args.teachers, parameter_count(22, 64, 64))) * 0.1
        bank = TeacherBank(device, w.astype(np.float32), 22, 64, 64, "relu", "tanh")
    ids = balanced_teacher_assignment(env.N_ENVIRONMENTS, bank.n_teachers)
    steps = int(cfg.episode_step_limit)
    ref, ref_ids, suite = None, None, None
    if args.figure_eight:
        ref = l2f.Reference(device, tracking.lissajous(steps, float(cfg.dt), amplitude=(0.3, 0.15, 0.0), period=5.0))
    if args.suite:
        suite = tracking.suite(steps, float(cfg.dt))
        ref = l2f.ReferenceBank(device, list(suite.values()))
        ref_ids = tracking.spread_reference_ids(env.N_ENVIRONMENTS, len(suite), ids)
    tab = bank.closed_loop(vector, device, env, params, state, rng, steps, ids, mode=args.mode, reference=ref, reference_ids=ref_ids)
    print(f"{bank.n_teachers} teachers x {env.N_ENVIRONMENTS} envs, {steps} steps ({args.mode}"
          f"{', figure-eight' if args.figure_eight else ', suite of ' + str(len(suite)) if suite else ''}): "
          f"{int(tab['episodes'].sum())} episodes finished, mean return {np.nanmean(tab['mean_return']):.3f}, "
          f"termination share {np.nansum(tab['termination_share'] * tab['episodes']) / max(1, tab['episodes'].sum()):.3f}")
    rmse = tab.get("tracking_rmse")
    extra = "" if rmse is None else "".join(f" {name:>11}" for name in suite) + "   RMSE [m] per setpoint" if suite else f" {'RMSE [m]':>9}"
    print(f"{'teacher':>8} {'envs':>6} {'episodes':>9} {'mean return':>12} {'mean length':>12} {'terminated':>11}" + extra)
    order = np.argsort(np.nan_to_num(tab["mean_return"], nan=-np.inf))
    for k in order[:args.worst]:
        tail = "" if rmse is None else "".join(f" {e:11.4f}" for e in rmse[k]) if suite else f" {rmse[k]:9.4f}"
        print(f"{k:8d} {tab['envs'][k]:6d} {tab['episodes'][k]:9d} {tab['mean_return'][k]:12.3f} {tab['mean_length'][k]:12.1f} "
              f"{tab['termination_share'][k]:11.3f}" + tail)


if __name__ == "__main__":
    main()
