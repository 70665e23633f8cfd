"""A numpy float64 reference of the probe moments (raptor_amd/csrc/rq_probe.hip, rq_trajectory_probe_moments), written from the
rule in include/raptor_quad.h and sharing nothing with the kernel.

Age: 0 at t = 0; a step is live when its done code is not 4; a live step contributes (h entering step t, age); after a live step
with code 1 or 2 the age is 0 again, after any other live step one more; a frozen step changes nothing and contributes nothing.
A sample of age a belongs to bucket b when edges[b] <= a < edges[b + 1]; any other sample is dropped."""
import numpy as np

DIM = 32


def ages(done):
    """done [T, N] -> (age [T, N] int64, -1 where the step is not live; live [T, N] bool)"""
    done = np.asarray(done)
    T, N = done.shape
    age = np.zeros(N, np.int64)
    out = np.full((T, N), -1, np.int64)
    live = done != 4
    for t in range(T):
        out[t, live[t]] = age[live[t]]
        ended = live[t] & ((done[t] == 1) | (done[t] == 2))
        age = np.where(ended, 0, np.where(live[t], age + 1, age))
    return out, live


def buckets(age, edges):
    """age [T, N] (-1: not live) -> bucket [T, N] int64, -1 for no sample (not live, or an age outside the edges)"""
    e = np.asarray(edges, np.int64)
    b = np.searchsorted(e, age, side="right") - 1
    return np.where((age >= e[0]) & (age < e[-1]), b, -1)


def samples(hidden, targets):
    """hidden [T, N, 16], targets [N, M] -> z [T, N, 32] float64 = [1, h, y, 0 ...]"""
    h = np.asarray(hidden, np.float64)
    y = np.asarray(targets, np.float64)
    T, N, _ = h.shape
    z = np.zeros((T, N, DIM))
    z[:, :, 0] = 1.0
    z[:, :, 1:17] = h
    z[:, :, 17:17 + y.shape[1]] = y[None]
    return z


def moments(hidden, done, targets, edges):
    """-> dict(age [T, N], bucket [T, N], counts [B] uint64, S [B, 32, 32] = sum z z^T, A [B, 32, 32] = sum |z| |z|^T), float64"""
    age, _ = ages(done)
    bucket = buckets(age, edges)
    z = samples(hidden, targets)
    B = len(edges) - 1
    S, A, counts = np.zeros((B, DIM, DIM)), np.zeros((B, DIM, DIM)), np.zeros(B, np.uint64)
    for b in range(B):
        zb = z[bucket == b]                   # NaN in a row that is not selected goes nowhere
        counts[b] = zb.shape[0]
        S[b] = zb.T @ zb
        A[b] = np.abs(zb).T @ np.abs(zb)
    return dict(age=age, bucket=bucket, counts=counts, S=S, A=A)
