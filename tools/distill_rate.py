#!/usr/bin/env python3
"""Time and peak device memory of the K distillation updates of one collection, two ways on the same recording and the same GPU:
(a) the torch loop - trajectory_actions + masked_mse + torch.optim.Adam per update, set_weights at the end (examples/distill.py
--torch-optimizer) - and (b) Distiller.step(traj, updates=K), everything on the device (rq_trajectory_distill).  At each shape the
two alternate for --rounds rounds after one warm-up each; every timed region is bracketed by a device synchronise (torch's and the
engine's), wall clock in between.  No speed-up is assumed: the file records what was measured.

    python tools/distill_rate.py [--shapes 16384x100,65536x500] [--updates 10] [--rounds 5] [--json profiles/distill_step_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                       # noqa: E402
from bench import Shard                            # noqa: E402
from raptor_amd.build import LIB, library_sha256   # noqa: E402
from raptor_amd.foundation_policy import Raptor    # noqa: E402
from raptor_amd.training import Distiller, masked_mse, trajectory_actions    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="16384x100,65536x500")
ap.add_argument("--updates", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--lr", type=float, default=1e-3)
ap.add_argument("--json", default=None)
args = ap.parse_args()

device = l2f.Device()


def sync():
    torch.cuda.synchronize()
    device.synchronize()


def measure(fn):
    sync()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    last_loss = fn()
    sync()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, torch.cuda.max_memory_allocated(), last_loss


results = []
for shape in args.shapes.split(","):
    n, T = (int(x) for x in shape.split("x"))
    sh = Shard(device, n, 0)
    traj = sh.vector.Trajectory(sh.env, T)
    sh.policy.reset()
    sh.vector.rollout(device, sh.env, sh.params, sh.state, sh.policy, sh.rng, T, "fused", autoreset=True, trajectory=traj)
    teacher = Raptor(device, weights=sh.policy.weights * np.float32(0.98))
    teacher.reset()
    traj.relabel(teacher, overwrite=True, fetch=False)          # the stored actions: the labels
    rec = traj.tensors()
    start = sh.policy.weights.copy()

    def torch_path():
        student = Raptor(device, weights=start)
        w = torch.tensor(start, device="cuda", requires_grad=True)
        opt = torch.optim.Adam([w], lr=args.lr)
        labels = rec["act"][:, :, :n].clone()
        live = (rec["done"][:, :n] != 4)[:, None, :].expand(T, 4, n)
        for _ in range(args.updates):
            opt.zero_grad()
            loss = masked_mse(trajectory_actions(traj, student, w)[:, :, :n], labels, live)
            loss.backward()
            opt.step()
        student.set_weights(w)
        return float(loss.detach())

    def device_path():
        student = Raptor(device, weights=start)
        losses = Distiller(student, lr=args.lr).step(traj, updates=args.updates)
        return float(losses[-1])

    torch_path(); device_path()                          # warm-up: allocations, first launches
    rows = []
    for r in range(args.rounds):
        a_ms, a_peak, a_loss = measure(torch_path)
        b_ms, b_peak, b_loss = measure(device_path)
        rows.append(dict(round=r, torch_ms=a_ms, device_ms=b_ms, torch_peak_bytes=a_peak, device_torch_peak_bytes=b_peak,
                         torch_last_loss=a_loss, device_last_loss=b_loss))
        print(f"{n} x {T} round {r}: torch loop {a_ms:.1f} ms (peak {a_peak / 2**20:.0f} MiB of torch tensors), "
              f"Distiller.step {b_ms:.1f} ms (peak {b_peak / 2**20:.0f} MiB)", flush=True)
    a = float(np.median([x["torch_ms"] for x in rows]))
    b = float(np.median([x["device_ms"] for x in rows]))
    results.append(dict(envs=n, steps=T, updates=args.updates, torch_ms_median=a, device_ms_median=b,
                        torch_ms_per_update=a / args.updates, device_ms_per_update=b / args.updates, ratio=a / b,
                        torch_peak_bytes=max(x["torch_peak_bytes"] for x in rows),
                        device_peak_bytes=max(x["device_torch_peak_bytes"] for x in rows),
                        recording_bytes=int(sum(v.numel() * v.element_size() for v in rec.values())), rounds=rows))
    del traj, sh, rec
    torch.cuda.empty_cache()

res = dict(gpu=torch.cuda.get_device_name(0), library_sha256=library_sha256(LIB), lr=args.lr,
           peak_bytes_note="torch.cuda.max_memory_allocated over the region: the temporaries of the update (the engine's own workspace, "
                           "64 B per env-step of saved state + 8 KB per wave, is the same on both paths and not in it)",
           shapes=results)
print(json.dumps(res))
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
