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

--holdout F: a fraction F of the envs is held out of every update (training.holdout_weights, the same split every epoch) and the
loss on them - a validation loss - is printed beside the training loss each epoch: one more loss_and_grad over the same recording
with the complementary mask, no copy of it.  --teacher-weights: every env's entries are weighted by how well its teacher flies,
w_k = max(0, 1 - 2 x termination share of teacher k) from one closed-loop run of the bank before the first epoch
(TeacherBank.closed_loop): a teacher that never crashes counts fully, one that crashes half its episodes or more not at all, one
that finished no episode (NaN) not at all either.  Both are weights inside the device's loss (Distiller.step(weight=...)); with
--torch-optimizer the same loss is training.weighted_mse.

    python examples/distill.py [--envs 16384] [--steps 100] [--epochs 3] [--adam-steps 10] [--lr 1e-3] [--torch-optimizer]
                               [--teacher-epochs K] [--figure-eight | --suite] [--holdout 0.1] [--teacher-weights]
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
from raptor_amd.training import Distiller, holdout_weights, masked_mse, trajectory_actions, weighted_mse  # noqa: E402


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
    ap.add_argument("--holdout", type=float, default=0.0, help="fraction of the envs held out of the updates; their loss is printed")
    ap.add_argument("--teacher-weights", action="store_true", help="weight every env by its teacher's closed-loop survival")
    args = ap.parse_args()
    if not 0.0 <= args.holdout < 1.0:
        ap.error("--holdout is a fraction in [0, 1)")
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
    # the loss's weights, one per env: None = every live entry counts the same (the unweighted call)
    weight, held_out = None, None
    if args.teacher_weights:
        table = bank.closed_loop(vector, device, env, params, state, rng, rows, ids, reference=ref, reference_ids=ref_ids)
        per_teacher = np.nan_to_num(np.maximum(0.0, 1.0 - 2.0 * table["termination_share"]), nan=0.0).astype(np.float32)
        print(f"teacher weights: {int((per_teacher > 0).sum())} of {args.teachers} teachers count, mean weight {per_teacher.mean():.3f}",
              flush=True)
        if per_teacher.any():
            weight = per_teacher[ids]
        else:                               # (the random stand-in teachers above crash every episode: nothing would be left to learn from)
            print("no teacher survives half its episodes: every weight would be 0 and the loss with it; the envs stay unweighted", flush=True)
        vector.sample_initial_state(device, env, params, state, rng)
    if args.holdout > 0.0:
        train, held_out = holdout_weights(n, args.holdout, seed=0)
        weight = train if weight is None else weight * train
    if weight is not None:
        weight_t = torch.tensor(weight, device="cuda")          # uploaded once, not every epoch
        held_out_t = None if held_out is None else torch.tensor(held_out, device="cuda")

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
                # both mask the inputs: frozen steps may hold NaN
                loss = masked_mse(act, labels, live) if weight is None else weighted_mse(act, labels, live, weight_t[None, None, :])
                loss.backward()
                opt.step()
                losses.append(loss.item())
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            student.set_weights(weights)                # the next collection runs the updated student
            if held_out is not None:
                with torch.no_grad():
                    val = weighted_mse(trajectory_actions(traj, student, weights)[:, :, :n], labels, live, held_out_t[None, None, :]).item()
        else:
            # the labels are the trajectory's stored actions, frozen steps are masked in the kernel; the student is updated in place
            losses = distiller.step(traj, updates=args.adam_steps, weight=None if weight is None else weight_t).tolist()
            dt = time.perf_counter() - t0
            if held_out is not None:                    # the loss of the updated student on the envs it was not trained on
                val = float(distiller.loss_and_grad(traj, weight=held_out_t)[0])
        for k, loss in enumerate(losses):
            print(f"epoch {epoch} step {k}: masked MSE {loss:.5f}", flush=True)
        if held_out is not None:
            print(f"epoch {epoch}: training loss {losses[-1]:.5f} (before the last update), held-out loss {val:.5f} "
                  f"({int(held_out.sum())} of {n} envs)", flush=True)
        print(f"epoch {epoch}: {args.adam_steps} gradient passes over {n} envs x {T} steps in {dt * 1e3:.1f} ms "
              f"({args.adam_steps / dt:.1f} passes/s, {args.adam_steps * n * T / dt:.3g} env-steps/s)", flush=True)


if __name__ == "__main__":
    main()
