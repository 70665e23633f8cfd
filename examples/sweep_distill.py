#!/usr/bin/env python3
"""A learning-rate sweep of distillation, the whole population at once: P perturbed copies of the student, each with its own
learning rate, fly 64 quadrotors each in ONE rollout (the policy bank), the recording is labelled by the shipped policy as the
teacher, and ONE call per epoch takes K Adam steps of every policy on its own envs (raptor_amd.training.BankDistiller).  Fly,
distil, fly again never leaves the device; the launch count is one student's.  At the end the bank is evaluated closed loop and the
table printed, best return first.

    python examples/sweep_distill.py [--policies 64] [--steps 100] [--epochs 3] [--adam-steps 10] [--lr-min 1e-4] [--lr-max 1e-2]
                                     [--sigma 0.05] [--show 10]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                                                           # noqa: E402
from raptor_amd.foundation_policy import Raptor, load_weights                          # noqa: E402
from raptor_amd.policy_bank import PolicyBank, block_policy_assignment                 # noqa: E402
from raptor_amd.training import BankDistiller                                          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--adam-steps", type=int, default=10)
    ap.add_argument("--lr-min", type=float, default=1e-4)
    ap.add_argument("--lr-max", type=float, default=1e-2)
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--show", type=int, default=10)
    args = ap.parse_args()

    P, T = args.policies, args.steps
    device = l2f.Device()
    n = P * 64
    vector = l2f.vector(n)
    rng, env = vector.VectorRng(), vector.VectorEnvironment()
    params, state = vector.VectorParameters(), vector.VectorState()
    vector.initialize_rng(device, rng, 0)
    vector.initialize_environment(device, env)
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)

    # every policy starts from the SAME perturbed student: what tells them apart afterwards is the learning rate
    w0 = load_weights()
    start = (w0 + np.float32(args.sigma) * np.random.default_rng(1).standard_normal(w0.size).astype(np.float32)).astype(np.float32)
    bank = PolicyBank(device, np.tile(start, (P, 1)))
    rates = np.geomspace(args.lr_min, args.lr_max, P)
    sweep = BankDistiller(bank, lr=rates)
    teacher = Raptor(device)                            # the shipped policy labels what the students saw
    ids = block_policy_assignment(n, P)
    traj = vector.Trajectory(env, T)

    for epoch in range(args.epochs):
        traj.reset()
        bank.reset()
        vector.rollout(device, env, params, state, bank, rng, T, "fused", autoreset=True, trajectory=traj, policy_ids=ids)
        teacher.reset()
        traj.relabel(teacher, overwrite=True, fetch=False)                             # stored actions <- the teacher's labels
        device.synchronize()
        t0 = time.perf_counter()
        losses = np.asarray(sweep.step(traj, ids, updates=args.adam_steps).tolist())   # [K, P]; the bank is updated in place
        dt = time.perf_counter() - t0
        print(f"epoch {epoch}: {args.adam_steps} updates of {P} policies on {n} envs x {T} steps in {dt * 1e3:.1f} ms; masked MSE "
              f"before the first / the last update: median {np.median(losses[0]):.5f} / {np.median(losses[-1]):.5f}, "
              f"best {losses[0].min():.5f} / {losses[-1].min():.5f}", flush=True)

    vector.sample_initial_state(device, env, params, state, rng)
    tab = bank.evaluate(vector, device, env, params, state, rng, env.config.episode_step_limit, ids)
    print(f"{'policy':>8} {'lr':>10} {'last loss':>10} {'episodes':>9} {'mean return':>12} {'std':>9} {'mean length':>12} {'terminated':>11}")
    order = np.argsort(-np.nan_to_num(tab["mean_return"], nan=-np.inf))
    for k in order[:args.show]:
        print(f"{k:8d} {rates[k]:10.2e} {losses[-1][k]:10.5f} {tab['episodes'][k]:9d} {tab['mean_return'][k]:12.3f} "
              f"{tab['std_return'][k]:9.3f} {tab['mean_length'][k]:12.1f} {tab['termination_share'][k]:11.3f}")
    best = int(order[0])
    print(f"best by return: policy {best}, lr {rates[best]:.2e}, mean return {tab['mean_return'][best]:.3f}")


if __name__ == "__main__":
    main()
