#!/usr/bin/env python3
"""Time of the imitation error table of one recording (raptor_amd.training.imitation_error, csrc/rq_grad_forward.inc under
RQ_GRAD_ERROR_TABLE), against the two ways the same numbers cost before it, on the same GPU and the same recording:
(a) imitation_error: one launch, sse and count [B, N] in device memory;
(b) Distiller.loss_and_grad: forward, loss-seeded backward, reduction - what a held-out loss costs today, for one scalar;
(c) the torch route: trajectory_actions under no_grad (rq_trajectory_policy_forward into a [T, 4, ld] tensor; timed on its own too,
    as forward_ms) plus the bucket sums - the done codes fetched, probing.episode_steps on the host, the bucket index uploaded, one
    masked sum per bucket.
The target is the trajectory's stored actions in all three; the student is the shipped policy with perturbed weights.

Each timed region is bracketed by a device synchronise (torch's and the engine's) with the host's perf_counter in between; the three
ways alternate for --rounds rounds after one warm-up each; medians are reported, every round is kept.  No ratio is assumed: the file
records what was measured and how far the results are apart.

    python tools/error_table_rate.py [--envs 65536] [--steps 500] [--buckets 10] [--rounds 5] [--json profiles/error_table_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                                   # noqa: E402
from bench import Shard                                        # noqa: E402
from raptor_amd import probing                                 # noqa: E402
from raptor_amd.build import LIB, library_sha256               # noqa: E402
from raptor_amd.foundation_policy import Raptor                # noqa: E402
from raptor_amd.training import Distiller, imitation_error, trajectory_actions      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--buckets", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()
N, T, B = args.envs, args.steps, args.buckets

device = l2f.Device()


def sync():
    torch.cuda.synchronize()
    device.synchronize()


def measure(fn):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return (time.perf_counter() - t0) * 1e3, out


sh = Shard(device, N, 0)
traj = sh.vector.Trajectory(sh.env, T)
sh.vector.rollout(device, sh.env, sh.params, sh.state, sh.policy, sh.rng, T, "fused", autoreset=True, trajectory=traj)
w = sh.policy.weights
w = (w + np.random.default_rng(0).standard_normal(w.size).astype(np.float32) * 0.02).astype(np.float32)
student = Raptor(device, weights=w)
student.reset()
distiller = Distiller(student)
edges = probing.log_age_edges(min(T, int(sh.env.config.episode_step_limit)), B)
dev = traj.tensors()["done"].device
w_dev = torch.tensor(w, device=dev)
edges_host = edges.astype(np.int64)


def table_path():
    return imitation_error(traj, student, edges=edges)


def loss_path():
    return distiller.loss_and_grad(traj)


def forward_path():
    with torch.no_grad():
        return trajectory_actions(traj, student, w_dev)


def sums_path(act):
    """act [T, 4, ld] -> (sse [B, N] fp32, count [B, N]) in torch, the ages from probing.episode_steps on the host"""
    t = traj.tensors()
    done = t["done"][:, :N].cpu().numpy()
    k = probing.episode_steps(done)
    b = np.searchsorted(edges_host, k, side="right") - 1
    b[(k < edges_host[0]) | (k >= edges_host[-1])] = -1
    bucket = torch.from_numpy(b).to(dev)
    d = act[:, :, :N] - t["act"][:, :, :N]
    zero = torch.zeros((), device=dev)
    e = torch.where((bucket >= 0)[:, None, :], d, zero).square().sum(1)            # a select: NaN outside the buckets goes nowhere
    sse = torch.stack([torch.where(bucket == j, e, zero).sum(0) for j in range(B)])
    count = torch.stack([(bucket == j).sum(0) for j in range(B)])
    return sse, count


def torch_path():
    return sums_path(forward_path())


table_path(), loss_path(), torch_path()                       # warm-up: code objects, workspaces, the allocator's blocks
rows = []
for r in range(args.rounds):
    a, tab = measure(table_path)
    b, (loss, _) = measure(loss_path)
    f, act = measure(forward_path)
    s, (sse_t, count_t) = measure(lambda: sums_path(act))
    del act
    rows.append(dict(round=r, imitation_error_ms=a, loss_and_grad_ms=b, forward_ms=f, bucket_sums_ms=s, torch_route_ms=f + s))
    print(f"round {r}: imitation_error {a:.2f} ms; loss_and_grad {b:.2f} ms; torch route {f + s:.2f} ms (forward {f:.2f} + sums {s:.2f})",
          flush=True)
med = {k: float(np.median([x[k] for x in rows])) for k in rows[0] if k != "round"}
sse_k, count_k = tab.sse.double().cpu().numpy(), tab.count.cpu().numpy().astype(np.int64)
sse_t64 = sse_t.double().cpu().numpy()
ld = int(traj.tensors()["done"].shape[1])
read_bytes = int(T) * ld * (22 * 4 + 4 * 4 + 1)
res = dict(gpu=torch.cuda.get_device_name(0), library_sha256=library_sha256(LIB),
           clock="host time.perf_counter between device synchronisations (torch.cuda.synchronize and the engine's stream)",
           envs=N, steps=T, buckets=B, age_edges=[int(x) for x in edges], rounds=rows,
           imitation_error_ms_median=med["imitation_error_ms"], loss_and_grad_ms_median=med["loss_and_grad_ms"],
           forward_ms_median=med["forward_ms"], bucket_sums_ms_median=med["bucket_sums_ms"], torch_route_ms_median=med["torch_route_ms"],
           ratio_loss_and_grad_over_imitation_error=med["loss_and_grad_ms"] / med["imitation_error_ms"],
           ratio_torch_route_over_imitation_error=med["torch_route_ms"] / med["imitation_error_ms"],
           ratio_imitation_error_over_forward=med["imitation_error_ms"] / med["forward_ms"],
           bytes_read=read_bytes, read_GBps_at_median=read_bytes / (med["imitation_error_ms"] * 1e-3) / 1e9,
           counts_equal=bool(np.array_equal(count_k, count_t.cpu().numpy())),
           sse_max_relative_difference_to_torch=float((np.abs(sse_k - sse_t64) / np.maximum(np.abs(sse_t64), 1e-30)).max()),
           table_loss=float(tab.loss()), loss_and_grad_loss=float(loss),
           forward="rq_trajectory_policy_forward through trajectory_actions under no_grad: k_policy_grad_forward, which also stores the "
                   "saved state and the actions; the error table's kernel is the same pass without those stores")
print(json.dumps(res))
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
