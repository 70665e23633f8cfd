#!/usr/bin/env python3
"""Time of the learner's gradient pass over a recorded trajectory: rq_trajectory_policy_forward + rq_trajectory_policy_backward
(device pointers, asynchronous, the engine's stream) against a torch restatement of the same student and episode rules on the same
GPU (Dense + nn.GRUCell stepped through time in Python, torch autograd), the two alternating, each round timed with events around
the forward + backward pair after warm-up.  The torch restatement runs on --torch-envs envs (its time scales with the launches,
not the envs, until the GPU fills) and is reported per env-step as well.

    python tools/grad_rate.py [--envs 65536] [--steps 500] [--rounds 3] [--torch-envs 65536] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raptor_amd.l2f as l2f                       # noqa: E402
from bench import Shard                            # noqa: E402
from raptor_amd import _lib                        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--torch-envs", type=int, default=65536)
ap.add_argument("--json", default=None)
args = ap.parse_args()

device = l2f.Device()
sh = Shard(device, args.envs, 0)
traj = sh.vector.Trajectory(sh.env, args.steps)
sh.policy.reset()
sh.vector.rollout(device, sh.env, sh.params, sh.state, sh.policy, sh.rng, args.steps, "fused", autoreset=True, trajectory=traj)
ten = traj.tensors()
T, ld, n = args.steps, ten["act"].shape[2], args.envs
act = torch.empty((T, 4, ld), device="cuda")
gact = torch.randn((T, 4, ld), device="cuda")
gw = torch.empty(2084, device="cuda")
sp = C.c_void_p()
_lib.call("rq_device_stream", device._h, C.byref(sp))
stream = torch.cuda.ExternalStream(sp.value)           # the engine's own stream: the events go where its launches are
h = traj._require("trajectory")
pol = sh.policy._handle()


def engine_pass():
    _lib.call("rq_trajectory_policy_forward", h, pol, 1, C.c_void_p(act.data_ptr()), ld, 2)
    _lib.call("rq_trajectory_policy_backward", h, pol, C.c_void_p(gact.data_ptr()), ld, C.c_void_p(gw.data_ptr()), None, 2)


def time_engine():
    engine_pass()
    _lib.call("rq_device_synchronize", device._h)
    with torch.cuda.stream(stream):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(stream)
        engine_pass()
        e.record(stream)
    e.synchronize()
    return s.elapsed_time(e)


# the torch restatement: the same parameters, observations and episode rules
w = torch.tensor(sh.policy.weights, device="cuda")
nt = min(args.torch_envs, n)
obs_t = ten["obs"][:, :, :nt].permute(0, 2, 1).contiguous()       # [T, n, 22]
done_t = ten["done"][:, :nt].long()
cell = torch.nn.GRUCell(16, 16).cuda()
W0 = w[0:352].view(16, 22).clone().requires_grad_()
b0 = w[352:368].clone().requires_grad_()
h0 = w[2000:2016].clone().requires_grad_()
W2 = w[2016:2080].view(4, 16).clone().requires_grad_()
b2 = w[2080:2084].clone().requires_grad_()
with torch.no_grad():
    cell.weight_ih.copy_(w[368:1136].view(48, 16)); cell.weight_hh.copy_(w[1136:1904].view(48, 16))
    cell.bias_ih.copy_(w[1904:1952]); cell.bias_hh.copy_(w[1952:2000])
g_t = gact[:, :, :nt].permute(0, 2, 1).contiguous()


def torch_pass():
    hh = h0.expand(nt, 16)
    total = 0
    for t in range(T):
        y = torch.relu(obs_t[t] @ W0.T + b0)
        hn = cell(y, hh)
        total = total + ((hn @ W2.T + b2) * g_t[t]).sum()
        d = done_t[t][:, None]
        hh = torch.where(d == 4, hh, hn)
        hh = torch.where((d == 1) | (d == 2), h0.expand(nt, 16), hh)
    total.backward()


def time_torch():
    torch_pass()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    torch_pass()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


rows = []
for r in range(args.rounds):
    te = time_engine()
    tt = time_torch()
    rows.append(dict(round=r, engine_ms=te, torch_ms=tt))
    print(f"round {r}: engine forward+backward {te:.2f} ms ({n} envs x {T} steps); torch GRUCell loop {tt:.1f} ms ({nt} envs)",
          flush=True)
eng = float(np.median([x["engine_ms"] for x in rows]))
tor = float(np.median([x["torch_ms"] for x in rows]))
res = dict(envs=n, steps=T, torch_envs=nt, engine_ms_median=eng, torch_ms_median=tor,
           engine_ns_per_env_step=eng * 1e6 / (n * T), torch_ns_per_env_step=tor * 1e6 / (nt * T),
           speedup_per_env_step=(tor / (nt * T)) / (eng / (n * T)), rounds=rows,
           gpu=torch.cuda.get_device_name(0))
print(json.dumps(res))
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
