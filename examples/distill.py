#!/usr/bin/env python3
"""The distillation loop of post-training (README.md:208-216) on the device: collect with the student (auto-reset, recorded),
label the recorded observations with a bank of MLP teachers, take K Adam steps on the MSE between the student's actions over the
recording and the labels (masked by done != 4), push the new weights into the student, collect again.

The K updates of a collection are ONE call (raptor_amd.training.Distiller.step): forward, loss-seeded backward, Adam and the rebuilt
operand images are HIP launches enqueued back to back, and nothing of the recording's size or the weights visits the host.
--torch-optimizer keeps the earlier loop instead - trajectory_actions + masked_mse + torch.optim.Adam + set_weights, the way any
other loss than the masked MSE still goes - and prints the same lines.

--figure-eight / --suite: every collection - the teachers' epochs (--teacher-epochs K) and the student's alike - flies the
figure-eight of examples/track_figure_eight.py, or the setpoints of raptor_amd.tracking.suite dealt evenly inside every teacher's
envs, so behaviour cloning starts on the paths the student is ranked on (examples/evaluate_checkpoints.py --suite).

    python examples/distill.py [--envs 16384] [--steps 100] [--epochs 3] [--adam-steps 10] [--lr 1e-3] [--torch-optimizer]
                               [--teacher-epochs K] [--figure-eight | --suite]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                       # noqa: E402
from raptor_amd import tracking                    # noqa: E402
from raptor_amd.foundation_policy import Raptor    # noqa: E402
from raptor_amd.teachers import TeacherBank, balanced_teacher_assignment, parameter_count    # noqa: E402
from raptor_amd.training import Distiller, masked_mse, trajectory_actions  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--adam-steps", type=int, default=10)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--teachers", type=int, default=64)
    ap.add_argument("--teacher-epochs", type=int, default=0,
                    help="the first K epochs collect with the teachers flying the envs (behaviour cloning), then the student acts")
    ap.add_argument("--torch-optimizer", action="store_true",
                    help="the loss and Adam in torch (trajectory_actions + masked_mse) instead of Distiller.step")
    ap.add_argument("--figure-eight", action="store_true", help="every collection tracks a figure-eight")
    ap.add_argument("--suite", action="store_true", help="every collection tracks a suite of setpoints, a reference per env")
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
        cfg.init_guidance = 1.0                    # hover at the origin, where the paths start
        env.config = cfg
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    n, T = env.N_ENVIRONMENTS, args.steps

    student = Raptor(device)
    # stand-in teachers (the trained ones are not in the reference tree): 22-64-64-4 MLPs, one per group of quadrotors
    bank = TeacherBank(device, (np.random.default_rng(1).standard_normal((args.teachers, parameter_count(22, 64, 64))) * 0.1)
                       .astype(np.float32), 22, 64, 64, "relu", "tanh")
    ids = balanced_teacher_assignment(n, args.teachers)
    # the setpoint both kinds of epoch fly: a row per step of an episode (the env reads the row of its own episode step count)
    ref, ref_ids = None, None
    rows = int(cfg.episode_step_limit)
    if args.figure_eight:
        ref = l2f.Reference(device, tracking.lissajous(rows, float(cfg.dt), amplitude=(0.3, 0.15, 0.0), period=5.0))
    if args.suite:
        ref = l2f.ReferenceBank(device, list(tracking.suite(rows, float(cfg.dt)).values()))
        ref_ids = tracking.spread_reference_ids(n, ref.n_references, ids)
    if args.torch_optimizer:
        weights = torch.tensor(student.weights, device="cuda", requires_grad=True)
        opt = torch.optim.Adam([weights], lr=args.lr)
    else:
        distiller = Distiller(student, lr=args.lr)
    traj = vector.Trajectory(env, T)

    for epoch in range(args.epochs):
        traj.reset()
        student.reset()
        if epoch < args.teacher_epochs:     # the teachers act: the recorded actions ARE their labels
            bank.fly(vector, device, env, params, state, rng, T, ids, "fused", autoreset=True, trajectory=traj, reference=ref,
                     reference_ids=ref_ids)
        else:
            vector.rollout(device, env, params, state, student, rng, T, "fused", autoreset=True, trajectory=traj, reference=ref,
                           reference_ids=ref_ids)
            traj.relabel_teachers(bank, ids, overwrite=True, fetch=False)      # stored actions <- the teachers' labels
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if args.torch_optimizer:
            rec = traj.tensors()
            labels = rec["act"][:, :, :n].clone()
            live = (rec["done"][:, :n] != 4)[:, None, :].expand(T, 4, n)       # frozen steps carry no label
            losses = []
            for k in range(args.adam_steps):
                opt.zero_grad()
                act = trajectory_actions(traj, student, weights)[:, :, :n]
                loss = masked_mse(act, labels, live)    # masks the inputs: frozen steps may hold NaN
                loss.backward()
                opt.step()
                losses.append(loss.item())
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            student.set_weights(weights)                # the next collection runs the updated student
        else:
            # the labels are the trajectory's stored actions, frozen steps are masked in the kernel; the student is updated in place
            losses = distiller.step(traj, updates=args.adam_steps).tolist()
            dt = time.perf_counter() - t0
        for k, loss in enumerate(losses):
            print(f"epoch {epoch} step {k}: masked MSE {loss:.5f}", flush=True)
        print(f"epoch {epoch}: {args.adam_steps} gradient passes over {n} envs x {T} steps in {dt * 1e3:.1f} ms "
              f"({args.adam_steps / dt:.1f} passes/s, {args.adam_steps * n * T / dt:.3g} env-steps/s)", flush=True)


if __name__ == "__main__":
    main()
