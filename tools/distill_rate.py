#!/usr/bin/env python3
"""Time and peak device memory of the K distillation updates of one collection, two ways on the same recording and the same GPU:
(a) the torch loop - trajectory_actions + masked_mse + torch.optim.Adam per update, set_weights at the end (examples/distill.py
--torch-optimizer) - and (b) Distiller.step(traj, updates=K), everything on the device (rq_trajectory_distill).  At each shape the
two alternate for --rounds rounds after one warm-up each; every timed region is bracketed by a device synchronise (torch's and the
engine's), wall clock in between.  No speed-up is assumed: the file records what was measured.

    python tools/distill_rate.py [--shapes 16384x100,65536x500] [--updates 10] [--rounds 5] [--json profiles/distill_step_rate.json]

--weighted times something else: Distiller.step(traj, updates=K) without a weight against the same call with a weight per env and
with a weight per env and step (rq_trajectory_distill_weighted), on one recording in one run, the three alternating for --rounds
rounds after a warm-up each.  The weights are device tensors made beforehand, uniform in (0.5, 1.5) with a tenth of the envs held
out (0): what a hold-out split or a teacher ranking passes.  The result becomes key "weighted" of the JSON file, whose other keys
are kept.

    python tools/distill_rate.py --weighted [--shapes 65536x500] [--updates 10] [--rounds 5] [--json profiles/distill_rate.json]
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
ap.add_argument("--shapes", default=None, help="ENVSxSTEPS,... (16384x100,65536x500; --weighted: 65536x500)")
ap.add_argument("--weighted", action="store_true", help="time the weighted update against the unweighted one instead")
ap.add_argument("--updates", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--lr", type=float, default=1e-3)
ap.add_argument("--json", default=None)
args = ap.parse_args()
if args.shapes is None:
    args.shapes = "65536x500" if args.weighted else "16384x100,65536x500"
if args.weighted and args.json is None:
    args.json = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "distill_rate.json")

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


def weighted_rates():
    """-> the "weighted" entry: per shape the medians of the three updates and the two ratios to the unweighted one"""
    from raptor_amd.training import holdout_weights
    out = []
    for shape in args.shapes.split(","):
        n, T = (int(x) for x in shape.split("x"))
        sh = Shard(device, n, 0)
        traj = sh.vector.Trajectory(sh.env, T)
        sh.policy.reset()
        sh.vector.rollout(device, sh.env, sh.params, sh.state, sh.policy, sh.rng, T, "fused", autoreset=True, trajectory=traj)
        teacher = Raptor(device, weights=sh.policy.weights * np.float32(0.98))
        teacher.reset()
        traj.relabel(teacher, overwrite=True, fetch=False)          # the stored actions: the labels
        start = sh.policy.weights.copy()
        gen = torch.Generator("cuda").manual_seed(0)
        train = torch.tensor(holdout_weights(n, 0.1, 0)[0], device="cuda")
        per_env = (0.5 + torch.rand(n, device="cuda", generator=gen)) * train
        per_step = (0.5 + torch.rand((T, n), device="cuda", generator=gen)) * train[None, :]
        forms = dict(unweighted=None, per_env=per_env, per_step=per_step)

        def update(weight):
            student = Raptor(device, weights=start)
            return float(Distiller(student, lr=args.lr).step(traj, updates=args.updates, weight=weight)[-1])

        for w in forms.values():
            update(w)                                        # warm-up: allocations, first launches
        rows = []
        for r in range(args.rounds):
            row = dict(round=r)
            for name, w in forms.items():
                row[name + "_ms"], _, row[name + "_last_loss"] = measure(lambda: update(w))
            rows.append(row)
            print(f"{n} x {T} round {r}: " + ", ".join(f"{k} {row[k + '_ms']:.1f} ms" for k in forms), flush=True)
        med = {k: float(np.median([x[k + "_ms"] for x in rows])) for k in forms}
        out.append(dict(envs=n, steps=T, updates=args.updates, **{k + "_ms_median": v for k, v in med.items()},
                        per_env_over_unweighted=med["per_env"] / med["unweighted"],
                        per_step_over_unweighted=med["per_step"] / med["unweighted"], rounds=rows))
        del traj, sh
        torch.cuda.empty_cache()
    return dict(gpu=torch.cuda.get_device_name(0), library_sha256=library_sha256(LIB), lr=args.lr, shapes=out)


if args.weighted:
    entry = weighted_rates()
    print(json.dumps(dict(weighted=entry)))
    doc = {}
    if os.path.exists(args.json):
        with open(args.json) as f:
            doc = json.load(f)
    doc["weighted"] = entry
    with open(args.json, "w") as f:
        json.dump(doc, f, indent=1)
    sys.exit(0)

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
