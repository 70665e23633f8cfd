#!/usr/bin/env python3
"""Time of the probe moments of one recording (raptor_amd.probing, csrc/rq_probe.hip), two ways on the same GPU:
(a) rq_trajectory_probe_moments on the saved state of a forward that has already run (the forward is excluded: the first, untimed
    call runs it and every timed call reuses its state), everything in device memory;
(b) the same moments in torch on the same device from Trajectory.hidden(policy, device=True) [T, N, 16] and the done codes: ages by
    a resetting cumulative sum, buckets by torch.bucketize, then one masked matrix product per bucket in fp32.  Fetching the hidden
    tensor (the [T, N, 16] copy in the learner layout) is timed on its own and is NOT part of (b).

Each timed region is bracketed by a device synchronise (torch's and the engine's) with the host's perf_counter in between; the two
ways alternate for --rounds rounds after one warm-up each; medians are reported, every round is kept.  No ratio is assumed: the file
records what was measured, and how far the two results are apart.

    python tools/probe_rate.py [--envs 65536] [--steps 500] [--buckets 10] [--targets 7] [--rounds 5] [--json profiles/probe_rate.json]

--timed: targets per step instead (rq_trajectory_probe_moments_timed, M = 6: the scheduled wrench of a recording flown under
raptor_amd.disturbances.suite, generated on the device by rq_trajectory_wrench_targets).  Timed, alternating, --rounds rounds
(7 by default here) after one warm-up each, medians reported, every round kept:
(a) the timed moments, (b) the untimed kernel at the same M on the same recording (per-env targets: the wrench of one step),
(c) the generation of the target tensor on its own, (d) the same moments in torch from the hidden tensor and the target tensor.
The forward is excluded as above.  With --json the figures go under the key "timed" of that file; what else it holds is kept.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                       # noqa: E402
from bench import Shard                            # noqa: E402
from raptor_amd import _lib, probing               # noqa: E402
from raptor_amd.build import LIB, library_sha256   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--buckets", type=int, default=10)
ap.add_argument("--targets", type=int, default=7)
ap.add_argument("--rounds", type=int, default=None)
ap.add_argument("--json", default=None)
ap.add_argument("--timed", action="store_true")
args = ap.parse_args()
if args.rounds is None:
    args.rounds = 7 if args.timed else 5
if args.timed:
    args.targets = 6
N, T, B, M = args.envs, args.steps, args.buckets, args.targets

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
if args.timed:                                                         # the recording is flown under a wrench schedule
    from raptor_amd import disturbances
    cfg = sh.env.config
    bank = l2f.WrenchBank(device, list(disturbances.suite(int(cfg.episode_step_limit), float(cfg.dt)).values()))
    ids = (np.arange(N) % bank.n_tables).astype(np.uint32)
    sh.env.set_wrench_schedule(bank, ids)
    start = sh.env.episode_steps()
traj = sh.vector.Trajectory(sh.env, T)
sh.vector.rollout(device, sh.env, sh.params, sh.state, sh.policy, sh.rng, T, "fused", autoreset=True, trajectory=traj)
if args.timed:
    names = list(probing.WRENCH_NAMES)
    Y_dev = traj.wrench_targets(bank, ids, sh.params, start, units="relative", device=True)       # [T, 6, ld]
    y = np.ascontiguousarray(Y_dev[T // 3, :, :N].cpu().numpy().T)     # [N, 6]: the untimed kernel's targets, one step's wrench
else:
    names = ["log_mass", "thrust_to_weight", "log_jxx", "log_jzz", "tau_rise", "torque_const", "hover_action"][:M]
    y, names = probing.targets_from_params(sh.params.numpy(), sh.env.config, names)
    y, _, _ = probing.standardise(y)
edges = probing.log_age_edges(min(T, int(sh.env.config.episode_step_limit)), B)
dev = traj.tensors()["done"].device
y_dev = torch.from_numpy(np.ascontiguousarray(y.T)).to(dev)            # [M, N]
S_dev = torch.empty((B, 32, 32), dtype=torch.float64, device=dev)
counts_dev = torch.empty(B, dtype=torch.int64, device=dev)
edges_dev = torch.from_numpy(edges.astype(np.int64)).to(dev)
pol, h_traj = sh.policy._handle(device), traj._require("trajectory")


def kernel_path():
    _lib.call("rq_trajectory_probe_moments", h_traj, pol, C.c_void_p(y_dev.data_ptr()), N, len(names), edges.ctypes.data, B,
              C.c_void_p(S_dev.data_ptr()), C.c_void_p(counts_dev.data_ptr()), 1)


def torch_path(hidden, done, dtype=torch.float32, targets=None):
    """hidden [T, N, 16], done [T, ld] uint8 -> (S [B, K, K] in `dtype` with K = 17 + M, counts [B]); targets [T, M, ld]: per step"""
    d = done[:, :N]
    live = d != 4
    ended = live & ((d == 1) | (d == 2))
    seen = torch.cumsum(live, dim=0)                                   # live steps up to and including t
    base = torch.cummax(torch.where(ended, seen, torch.zeros_like(seen)), dim=0).values
    age = (seen - live.long()) - torch.cat([torch.zeros_like(base[:1]), base[:-1]])
    bucket = torch.bucketize(age, edges_dev, right=True) - 1
    bucket = torch.where(live & (age >= edges_dev[0]) & (age < edges_dev[-1]), bucket, torch.full_like(bucket, -1))
    yz = y_dev.t().expand(T, N, len(names)) if targets is None else targets[:, :, :N].permute(0, 2, 1)
    z = torch.cat([torch.ones((T, N, 1), device=dev), hidden, yz], dim=2).reshape(T * N, -1).to(dtype)
    zero = torch.zeros((), device=dev, dtype=dtype)
    S, counts = [], []
    for b in range(B):
        m = (bucket == b).reshape(T * N, 1)
        zb = torch.where(m, z, zero)                                   # a select: NaN outside the bucket goes nowhere
        S.append(zb.t() @ zb)
        counts.append(m.sum())
    return torch.stack(S), torch.stack(counts)


def timed_path():
    _lib.call("rq_trajectory_probe_moments_timed", h_traj, pol, C.c_void_p(Y_dev.data_ptr()), int(Y_dev.shape[2]), 6,
              edges.ctypes.data, B, C.c_void_p(S_dev.data_ptr()), C.c_void_p(counts_dev.data_ptr()), 1)


def generate_path():
    _lib.call("rq_trajectory_wrench_targets", h_traj, bank._h, ids.ctypes.data, sh.params._require("VectorParameters"),
              start.ctypes.data, 0, C.c_void_p(Y_gen.data_ptr()), int(Y_gen.shape[2]), 1)


def run_timed():
    kernel_path()                                                      # runs the forward and tags its state; allocations
    timed_path()
    generate_path()
    fetch_ms, hidden = measure(lambda: traj.hidden(sh.policy, device=True))
    done = traj.tensors()["done"]
    torch_path(hidden, done, targets=Y_dev)                            # warm-up: code objects, the allocator's blocks
    rows = []
    for r in range(args.rounds):
        a, _ = measure(timed_path)
        S_k, c_k = S_dev.cpu().numpy(), counts_dev.cpu().numpy()
        u, _ = measure(kernel_path)
        g, _ = measure(generate_path)
        b, (S_t, c_t) = measure(lambda: torch_path(hidden, done, targets=Y_dev))
        rows.append(dict(round=r, timed_moments_ms=a, untimed_moments_ms=u, wrench_targets_ms=g, torch_ms=b))
        print(f"round {r}: timed moments {a:.2f} ms; untimed at M = 6 {u:.2f} ms; wrench targets {g:.2f} ms; torch {b:.2f} ms", flush=True)
    S_t32 = S_t.double().cpu().numpy()
    del S_t
    S_64 = torch_path(hidden, done, torch.float64, targets=Y_dev)[0].cpu().numpy()       # untimed: what both are measured against
    scale = np.sqrt(np.einsum("bii,bjj->bij", S_64, S_64))
    scale = np.where(scale > 0, scale, 1.0)
    med = {k: float(np.median([x[k] for x in rows])) for k in ("timed_moments_ms", "untimed_moments_ms", "wrench_targets_ms", "torch_ms")}
    ld = int(done.shape[1])
    read_bytes = int(T) * (16 + 6) * ld * 4
    K = 17 + 6
    res = dict(gpu=torch.cuda.get_device_name(0), library_sha256=library_sha256(LIB),
               clock="host time.perf_counter between device synchronisations (torch.cuda.synchronize and the engine's stream)",
               envs=N, steps=T, buckets=B, targets=names, age_edges=[int(e) for e in edges], rounds=rows,
               timed_moments_ms_median=med["timed_moments_ms"], untimed_moments_ms_median=med["untimed_moments_ms"],
               wrench_targets_ms_median=med["wrench_targets_ms"], torch_ms_median=med["torch_ms"],
               ratio_timed_over_untimed=med["timed_moments_ms"] / med["untimed_moments_ms"],
               ratio_expected_from_traffic=(64 + 4 * 6) / 64,
               ratio_torch_over_timed=med["torch_ms"] / med["timed_moments_ms"],
               hidden_fetch_ms=fetch_ms, state_and_target_bytes=read_bytes,
               state_and_target_read_GBps_at_median=read_bytes / (med["timed_moments_ms"] * 1e-3) / 1e9,
               target_bytes_written=int(T) * 6 * ld * 4,
               target_write_GBps_at_median=int(T) * 6 * ld * 4 / (med["wrench_targets_ms"] * 1e-3) / 1e9,
               generated_equals_timed_input=bool(torch.equal(Y_gen, Y_dev)),
               counts_equal=bool(np.array_equal(c_k, c_t.cpu().numpy())),
               error_measure="max over buckets and elements of |S - S64| / sqrt(S64_ii S64_jj), S64 = the same torch code in float64",
               timed_moments_error=float((np.abs(S_k[:, :K, :K] - S_64) / scale).max()),
               torch_fp32_error=float((np.abs(S_t32 - S_64) / scale).max()),
               excluded="the forward that saves the state (run once, before the timed rounds); the torch path also excludes the "
                        "fetch of the [T, N, 16] hidden tensor (hidden_fetch_ms) and the generation of the targets")
    print(json.dumps(res))
    if args.json:
        old = json.load(open(args.json)) if os.path.exists(args.json) else {}
        old["timed"] = res
        with open(args.json, "w") as f:
            json.dump(old, f, indent=1)


if args.timed:
    Y_gen = torch.zeros_like(Y_dev)
    run_timed()
    sys.exit(0)

kernel_path()                                                          # runs the forward and tags its state; allocations
fetch_ms, hidden = measure(lambda: traj.hidden(sh.policy, device=True))
done = traj.tensors()["done"]
torch_path(hidden, done)                                               # warm-up: code objects, the allocator's blocks
rows = []
for r in range(args.rounds):
    a, _ = measure(kernel_path)
    b, (S_t, c_t) = measure(lambda: torch_path(hidden, done))
    rows.append(dict(round=r, probe_moments_ms=a, torch_ms=b))
    print(f"round {r}: rq_trajectory_probe_moments {a:.2f} ms; torch on the same tensors {b:.2f} ms", flush=True)
K = 17 + len(names)
S_k, c_k = S_dev.cpu().numpy(), counts_dev.cpu().numpy()
S_t32 = S_t.double().cpu().numpy()
S_64 = torch_path(hidden, done, torch.float64)[0].cpu().numpy()       # untimed: what both are measured against
scale = np.sqrt(np.einsum("bii,bjj->bij", S_64, S_64))
scale = np.where(scale > 0, scale, 1.0)
a = float(np.median([x["probe_moments_ms"] for x in rows]))
b = float(np.median([x["torch_ms"] for x in rows]))
res = dict(gpu=torch.cuda.get_device_name(0), library_sha256=library_sha256(LIB),
           clock="host time.perf_counter between device synchronisations (torch.cuda.synchronize and the engine's stream)",
           envs=N, steps=T, buckets=B, targets=names, age_edges=[int(e) for e in edges], rounds=rows,
           probe_moments_ms_median=a, torch_ms_median=b, ratio_torch_over_probe_moments=b / a,
           hidden_fetch_ms=fetch_ms,
           saved_state_bytes=int(T) * 16 * int(traj.tensors()["done"].shape[1]) * 4,
           saved_state_read_GBps_at_median=int(T) * 16 * int(traj.tensors()["done"].shape[1]) * 4 / (a * 1e-3) / 1e9,
           counts_equal=bool(np.array_equal(c_k, c_t.cpu().numpy())),
           error_measure="max over buckets and elements of |S - S64| / sqrt(S64_ii S64_jj), S64 = the same torch code in float64",
           probe_moments_error=float((np.abs(S_k[:, :K, :K] - S_64) / scale).max()),
           torch_fp32_error=float((np.abs(S_t32 - S_64) / scale).max()),
           excluded="(a) excludes the forward that saves the state (run once, before the timed rounds); (b) excludes the fetch of the "
                    "[T, N, 16] hidden tensor, reported as hidden_fetch_ms (one untimed-warm call, forward already run)")
print(json.dumps(res))
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
