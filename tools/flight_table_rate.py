#!/usr/bin/env python3
"""Time of the flight table of one recording (raptor_amd.probing.flight_table, csrc/rq_flight_table.inc), against two things on
the same GPU and the same recording:
(a) flight_table: one launch, sum [B, 9, N], peak [B, 3, N] and count [B, N] in device memory;
(b) the torch route: the same nine values per step as elementwise float32 statistics of ``traj.tensors()``, the done codes fetched,
    ``probing.episode_steps`` on the host for the buckets, the bucket index uploaded, one ``index_add`` per table and an ``amax``
    for the peaks;
(c) ``traj.wrench_targets(..., device=True)``: k_probe_wrench_targets' pass over the same recording - a lane per env walking the
    done codes and WRITING 24 B per env-step -, a streaming yardstick of the same shape.
The recording is flown under the disturbance suite, the scenarios dealt over the envs; it is made twice per bucket count, with 10
doubling and with 32 linear buckets.

Each timed region is bracketed by a device synchronise (torch's and the engine's) with the host's perf_counter in between; the three
ways alternate for --rounds rounds after one warm-up each; medians are reported, every round is kept.  No ratio is assumed: the file
records what was measured.  The table reads 77 B per env-step (19 dword rows and one byte row).

    python tools/flight_table_rate.py [--envs 65536] [--steps 500] [--buckets 10 32] [--rounds 5] [--json profiles/flight_table_rate.json]
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
from raptor_amd import disturbances, probing                   # noqa: E402
from raptor_amd.build import LIB, library_sha256               # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--buckets", type=int, nargs="+", default=[10, 32])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--tolerance", type=float, default=0.05)
ap.add_argument("--json", default=None)
args = ap.parse_args()
N, T = args.envs, args.steps

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
cfg = sh.env.config
limit = int(cfg.episode_step_limit)
bank = l2f.WrenchBank(device, list(disturbances.suite(limit, float(cfg.dt)).values()))
ids = (np.arange(N) % bank.n_tables).astype(np.uint32)
sh.env.set_wrench_schedule(bank, ids)
start = sh.env.episode_steps()
traj = sh.vector.Trajectory(sh.env, T)
sh.vector.rollout(device, sh.env, sh.params, sh.state, sh.policy, sh.rng, T, "fused", autoreset=True, trajectory=traj)
dev = traj.tensors()["done"].device
ld = int(traj.tensors()["done"].shape[1])
tol2 = float(np.float32(args.tolerance) * np.float32(args.tolerance))


def edges_of(B):
    return probing.log_age_edges(min(T, limit), B) if B <= 10 else probing.linear_age_edges(0, min(T, limit), B)


def torch_path(edges):
    """-> (sum [B, 9, N] fp32, peak [B, 3, N], count [B, N]) in torch, the ages from probing.episode_steps on the host"""
    t = traj.tensors()
    B = len(edges) - 1
    done = t["done"][:, :N].cpu().numpy()
    k = probing.episode_steps(done, start)
    e = edges.astype(np.int64)
    b = np.searchsorted(e, k, side="right") - 1
    b[(k < e[0]) | (k >= e[-1])] = B                                  # a bucket of its own for what is counted nowhere
    x, a, r = t["obs"][:, :, :N], t["act"][:, :, :N], t["rew"][:, :N]
    d = a - x[:, 18:22]
    pos2 = x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]
    omega2 = x[:, 15] * x[:, 15] + x[:, 16] * x[:, 16] + x[:, 17] * x[:, 17]
    tilt = 1.0 - x[:, 11]
    v = torch.stack([pos2, x[:, 12] * x[:, 12] + x[:, 13] * x[:, 13] + x[:, 14] * x[:, 14], omega2, tilt, (a * a).sum(1), (d * d).sum(1),
                     (a.abs() >= 1.0).sum(1).float(), (pos2 > tol2).float(), r], 1)          # [T, 9, N]
    cell = torch.from_numpy(b).to(dev) * N + torch.arange(N, device=dev)          # [T, N] -> the cell of (bucket, env)
    live = cell.reshape(-1) < B * N
    flat = torch.where(live, cell.reshape(-1), torch.zeros((), dtype=cell.dtype, device=dev))
    vv = torch.where(live[:, None], v.permute(0, 2, 1).reshape(-1, 9), torch.zeros((), device=dev))     # a select: NaN goes nowhere
    total = torch.zeros((B * N, 9), device=dev).index_add(0, flat, vv)
    count = torch.zeros(B * N, device=dev).index_add(0, flat, live.float())
    peak = torch.zeros((B * N, 3), device=dev).scatter_reduce(0, flat[:, None].expand(-1, 3), vv[:, [0, 3, 2]], "amax", include_self=True)
    return total.reshape(B, N, 9).permute(0, 2, 1), peak.reshape(B, N, 3).permute(0, 2, 1), count.reshape(B, N)


def targets_path():
    return traj.wrench_targets(bank, ids, sh.params, start, units="relative", device=True)


results = []
for B in args.buckets:
    edges = edges_of(B)

    def table_path():
        return probing.flight_table(traj, edges=edges, start_steps=start, tolerance=args.tolerance, device=True)

    table_path(), torch_path(edges), targets_path()                  # warm-up: code objects, workspaces, the allocator's blocks
    rows = []
    for r in range(args.rounds):
        a, tab = measure(table_path)
        b, (sum_t, peak_t, count_t) = measure(lambda: torch_path(edges))
        c, y = measure(targets_path)
        del y
        rows.append(dict(round=r, flight_table_ms=a, torch_route_ms=b, wrench_targets_ms=c))
        print(f"B={B} round {r}: flight_table {a:.3f} ms; torch route {b:.2f} ms; wrench_targets {c:.3f} ms", flush=True)
    med = {k: float(np.median([x[k] for x in rows])) for k in rows[0] if k != "round"}
    s_k, s_t = tab.sum.double().cpu().numpy(), sum_t.double().cpu().numpy()
    read_bytes = int(T) * N * 77
    results.append(dict(buckets=B, age_edges=[int(x) for x in edges], rounds=rows,
                        flight_table_ms_median=med["flight_table_ms"], torch_route_ms_median=med["torch_route_ms"],
                        wrench_targets_ms_median=med["wrench_targets_ms"],
                        ratio_torch_route_over_flight_table=med["torch_route_ms"] / med["flight_table_ms"],
                        ratio_flight_table_over_wrench_targets=med["flight_table_ms"] / med["wrench_targets_ms"],
                        bytes_read=read_bytes, read_GBps_at_median=read_bytes / (med["flight_table_ms"] * 1e-3) / 1e9,
                        wrench_targets_bytes=int(T) * N * 25,
                        wrench_targets_GBps_at_median=int(T) * N * 25 / (med["wrench_targets_ms"] * 1e-3) / 1e9,
                        counts_equal=bool(np.array_equal(tab.count.cpu().numpy(), count_t.cpu().numpy().astype(np.int64))),
                        peaks_equal=bool(np.array_equal(tab.peak.cpu().numpy(), peak_t.cpu().numpy())),
                        sum_max_relative_difference_to_torch=float((np.abs(s_k - s_t) / np.maximum(np.abs(s_t), 1e-30)).max())))
res = dict(gpu=torch.cuda.get_device_name(0), library_sha256=library_sha256(LIB),
           clock="host time.perf_counter between device synchronisations (torch.cuda.synchronize and the engine's stream)",
           envs=N, steps=T, ld=ld, tolerance=args.tolerance, bytes_per_env_step=77, results=results,
           note="flight_table includes the call's host side (the start steps compared with the call before, one launch); wrench_targets "
                "reads one byte and writes 24 per env-step")
print(json.dumps(res))
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
