#!/usr/bin/env python3
"""Time of K distillation updates of a population of P students, 64 envs each, T recorded steps, two ways on the same GPU:
(a) BankDistiller.step(updates=K) on one recording of P x 64 envs - the whole bank in one call (rq_trajectory_policies_distill) - and
(b) what the same work took before a bank could learn: one Distiller.step(updates=K) per student on a 64-env recording of the same T.
(b) is timed for at most --singles students (each with its own policy, optimizer and recording, the calls issued back to back) and
scaled linearly to P: that figure is an EXTRAPOLATION and is labelled so.  It leaves out what (b) needs on top, copying every weight
vector into a bank before the evaluation rollout.

Each timed region is bracketed by a device synchronise (torch's and the engine's) with the host's perf_counter in between; the two
ways alternate for --rounds rounds after one warm-up each; medians are reported, every round is kept.  No ratio is assumed: the file
records what was measured.

    python tools/bank_distill_rate.py [--policies 1000] [--steps 500] [--updates 10] [--singles 32] [--rounds 5]
                                      [--json profiles/bank_distill_rate.json]
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
from raptor_amd.policy_bank import PolicyBank, block_policy_assignment    # noqa: E402
from raptor_amd.training import BankDistiller, Distiller                  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--policies", type=int, default=1000)
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--updates", type=int, default=10)
ap.add_argument("--singles", type=int, default=32)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--lr", type=float, default=1e-3)
ap.add_argument("--json", default=None)
args = ap.parse_args()
P, T, K = args.policies, args.steps, args.updates
S = min(args.singles, 32, P)

device = l2f.Device()


def sync():
    torch.cuda.synchronize()
    device.synchronize()


def measure(fn):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def recording(n, seed_offset):
    """n envs flown T steps by the shipped policy, the stored actions replaced by a slightly different teacher's labels"""
    sh = Shard(device, n, seed_offset)
    traj = sh.vector.Trajectory(sh.env, T)
    sh.policy.reset()
    sh.vector.rollout(device, sh.env, sh.params, sh.state, sh.policy, sh.rng, T, "fused", autoreset=True, trajectory=traj)
    teacher = Raptor(device, weights=sh.policy.weights * np.float32(0.98))
    teacher.reset()
    traj.relabel(teacher, overwrite=True, fetch=False)
    return sh, traj


big, big_traj = recording(P * 64, 0)
start = big.policy.weights.copy()
ids = block_policy_assignment(P * 64, P)
singles = [recording(64, 64 * k) for k in range(S)]


def bank_path():
    bank = PolicyBank(device, np.tile(start, (P, 1)))
    sweep = BankDistiller(bank, lr=args.lr)
    sync()
    return bank, sweep, measure(lambda: sweep.step(big_traj, ids, updates=K, wait=False))


def single_path():
    pairs = [(Raptor(device, weights=start), traj) for _, traj in singles]
    dist = [Distiller(pol, lr=args.lr) for pol, _ in pairs]
    for pol, _ in pairs:
        pol._handle(device)
    sync()

    def run():
        for d, (_, traj) in zip(dist, pairs):
            d.step(traj, updates=K, wait=False)
    return measure(run)


bank_path(); single_path()                               # warm-up: allocations, code objects, first launches
rows = []
for r in range(args.rounds):
    _, _, a = bank_path()
    b = single_path()
    rows.append(dict(round=r, bank_ms=a, singles_ms=b))
    print(f"round {r}: BankDistiller.step, {P} policies x 64 envs x {T} steps x {K} updates: {a:.1f} ms; {S} single Distiller.step calls: "
          f"{b:.1f} ms = {b / S:.2f} ms each", flush=True)
a = float(np.median([x["bank_ms"] for x in rows]))
b = float(np.median([x["singles_ms"] for x in rows]))
res = dict(gpu=torch.cuda.get_device_name(0), library_sha256=library_sha256(LIB), lr=args.lr,
           clock="host time.perf_counter between device synchronisations (torch.cuda.synchronize and the engine's stream); the work of a "
                 "region is enqueued back to back with no synchronisation inside it",
           policies=P, envs_per_policy=64, steps=T, updates=K, rounds=rows,
           bank_ms_median=a, bank_ms_per_update=a / K,
           singles_timed=S, singles_ms_median=b, single_ms_per_policy=b / S,
           singles_extrapolated_to_policies_ms=b / S * P,
           extrapolation_note=f"{S} single-policy Distiller.step calls were timed and scaled linearly to {P} policies: an extrapolation, "
                              "not a measurement of the whole population",
           ratio_extrapolated_singles_over_bank=b / S * P / a)
print(json.dumps(res))
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
