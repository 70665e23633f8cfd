#!/usr/bin/env python3
"""Time of the feedback-gain table of one recording (raptor_amd.probing.feedback_gains, csrc/rq_gain_table.inc), beside two other
passes over the same recording on the same GPU:
(a) feedback_gains: one launch, sum [B, 4, 16, N] and count [B, N] in device memory;
(b) imitation_error: the error table (csrc/rq_grad_forward.inc under RQ_GRAD_ERROR_TABLE) - the forward alone, 30 MFMAs per
    tile-step where the gain table issues 30 + 48;
(c) the torch route: the states entering every step from traj.hidden(policy, device=True), the recorded observations, A = da/dp0
    from the closed formula in torch float32 (chunks of --chunk steps, so that no [T, N, 64] array exists), bucket sums by index_add;
    the ages from probing.episode_steps on the host, as a user would.
The student is the shipped policy with perturbed weights.

Each timed region is bracketed by a device synchronise (torch's and the engine's) with the host's perf_counter in between; the three
ways alternate for --rounds rounds after one warm-up each; medians are reported, every round is kept.  No ratio is assumed: the file
records what was measured and how far the results are apart.

    python tools/gain_table_rate.py [--envs 65536] [--steps 500] [--buckets 10] [--rounds 5] [--json profiles/gain_table_rate.json]
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
from raptor_amd.training import imitation_error                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--buckets", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--chunk", type=int, default=25)
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
edges = probing.log_age_edges(min(T, int(sh.env.config.episode_step_limit)), B)
dev = traj.tensors()["done"].device
edges_host = edges.astype(np.int64)
wt = torch.tensor(w, device=dev)
W0, b0 = wt[0:352].reshape(16, 22), wt[352:368]
Wi, Wh = wt[368:1136].reshape(48, 16), wt[1136:1904].reshape(48, 16)
bi, bh, W2 = wt[1904:1952], wt[1952:2000], wt[2016:2080].reshape(4, 16)


def table_path():
    return probing.feedback_gains(traj, student, edges=edges)


def error_path():
    return imitation_error(traj, student, edges=edges)


def torch_path():
    """-> (sum [B, 4, 16, N] fp32, count [B, N]) in torch"""
    t = traj.tensors()
    hidden = traj.hidden(student, device=True)                  # [T, N, 16]
    done = t["done"][:, :N].cpu().numpy()
    k = probing.episode_steps(done)
    b = np.searchsorted(edges_host, k, side="right") - 1
    b[(k < edges_host[0]) | (k >= edges_host[-1])] = -1
    bucket = torch.from_numpy(b).to(dev)                        # [T, N]
    env = torch.arange(N, device=dev)
    total = torch.zeros((B * N, 64), dtype=torch.float32, device=dev)
    count = torch.zeros(B * N, dtype=torch.int64, device=dev)
    for s in range(0, T, args.chunk):
        e = min(s + args.chunk, T)
        x = t["obs"][s:e, :, :N].permute(0, 2, 1).reshape(-1, 22)
        h = hidden[s:e].reshape(-1, 16)
        bk = bucket[s:e].reshape(-1)
        at = bk >= 0
        x, h = x[at], h[at]                                     # a select: NaN on frozen steps goes nowhere
        key = bk[at] * N + env.repeat(e - s)[at]
        p0 = x @ W0.T + b0
        y0 = torch.relu(p0)
        gi, gh = y0 @ Wi.T + bi, h @ Wh.T + bh
        r, z = torch.sigmoid(gi[:, :16] + gh[:, :16]), torch.sigmoid(gi[:, 16:32] + gh[:, 16:32])
        c = gh[:, 32:]
        n = torch.tanh(gi[:, 32:] + r * c)
        fn = (1 - z) * (1 - n * n)
        fr = fn * c * r * (1 - r)
        fz = (h - n) * z * (1 - z)
        m = (p0 > 0).to(torch.float32)
        A = torch.stack([((fn * W2[i]) @ Wi[32:48] + (fr * W2[i]) @ Wi[0:16] + (fz * W2[i]) @ Wi[16:32]) * m for i in range(4)], dim=1)
        total.index_add_(0, key, A.reshape(-1, 64))
        count.index_add_(0, key, torch.ones_like(key))
    return total.reshape(B, N, 4, 16).permute(0, 2, 3, 1), count.reshape(B, N)


table_path(), error_path(), torch_path()                      # warm-up: code objects, workspaces, the allocator's blocks
rows = []
for r in range(args.rounds):
    a, tab = measure(table_path)
    b, _ = measure(error_path)
    c, (sum_t, count_t) = measure(torch_path)
    rows.append(dict(round=r, feedback_gains_ms=a, imitation_error_ms=b, torch_route_ms=c))
    print(f"round {r}: feedback_gains {a:.2f} ms; imitation_error {b:.2f} ms; torch route {c:.2f} ms", flush=True)
    if r + 1 < args.rounds:
        del sum_t, count_t
med = {k: float(np.median([x[k] for x in rows])) for k in rows[0] if k != "round"}
g_k = tab.by_age().cpu().numpy()
W064 = W0.double()
c_t = count_t.double().sum(1)
g_t = (torch.einsum("bik,kf->bif", sum_t.double().sum(3), W064) / c_t[:, None, None]).cpu().numpy()
ld = int(traj.tensors()["done"].shape[1])
read_bytes = int(T) * ld * (22 * 4 + 1)
res = dict(gpu=torch.cuda.get_device_name(0), library_sha256=library_sha256(LIB),
           clock="host time.perf_counter between device synchronisations (torch.cuda.synchronize and the engine's stream)",
           envs=N, steps=T, buckets=B, age_edges=[int(x) for x in edges], torch_chunk_steps=args.chunk, rounds=rows,
           feedback_gains_ms_median=med["feedback_gains_ms"], imitation_error_ms_median=med["imitation_error_ms"],
           torch_route_ms_median=med["torch_route_ms"],
           ratio_feedback_gains_over_imitation_error=med["feedback_gains_ms"] / med["imitation_error_ms"],
           ratio_expected_from_mfma_counts=(30 + 48) / 30,
           ratio_torch_route_over_feedback_gains=med["torch_route_ms"] / med["feedback_gains_ms"],
           env_steps_per_second_at_median=N * T / (med["feedback_gains_ms"] * 1e-3),
           bytes_read=read_bytes, read_GBps_at_median=read_bytes / (med["feedback_gains_ms"] * 1e-3) / 1e9,
           counts_equal=bool(np.array_equal(tab.count.cpu().numpy().astype(np.int64), count_t.cpu().numpy())),
           by_age_max_relative_difference_to_torch=float((np.abs(g_k - g_t).max(axis=(1, 2)) / np.abs(g_t).max(axis=(1, 2))).max()))
print(json.dumps(res))
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
