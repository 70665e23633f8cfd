"""The imitation error table restated in NumPy float32 (rq_trajectory_policy_error_table, csrc/rq_grad_forward.inc under
RQ_GRAD_ERROR_TABLE): ages, buckets, the per-step error and the sequential sums exactly as include/raptor_quad.h defines them, so
that the kernel's sse and count can be held to it bit for bit.

Age: 0 at the first recorded step; a step is live when its done code is not 4; after a live step with code 1 or 2 the age is 0
again, after any other live step one more; frozen steps neither count nor age.  A live step of age k belongs to bucket b when
edges[b] <= k < edges[b + 1]; outside every bucket it is counted nowhere.  e = ((d0 d0 + d1 d1) + d2 d2) + d3 d3 with d = a - y,
every operation rounded to float32 on its own; sse[b][i] is the sum of e in time order, float32, from 0."""
import numpy as np


def ages(done):
    """done [T, N] codes -> k [T, N] int64: the age of every step, -1 on a frozen one.  Written env by env, step by step - the
    rule as it is stated, not probing.episode_steps' vectorised form."""
    done = np.asarray(done)
    T, N = done.shape
    out = np.full((T, N), -1, np.int64)
    for i in range(N):
        age = 0
        for t in range(T):
            d = int(done[t, i])
            if d == 4:
                continue
            out[t, i] = age
            age = 0 if d in (1, 2) else age + 1
    return out


def buckets(k, edges):
    """k [T, N] ages (-1: frozen), edges [B + 1] strictly ascending -> b [T, N] int64: the bucket of every step, -1 where the step
    is frozen or its age lies outside every bucket."""
    k = np.asarray(k, np.int64)
    e = np.asarray(edges).astype(np.int64)
    assert e.ndim == 1 and e.size >= 2 and (e[1:] > e[:-1]).all() and e[0] >= 0
    b = np.full(k.shape, -1, np.int64)
    for j in range(e.size - 1):
        b[(k >= e[j]) & (k < e[j + 1])] = j
    return b


def step_error(act, target):
    """act, target [T, 4, N] float32 -> e [T, N] float32, every operation rounded once (NaN where an input is NaN: the caller selects)"""
    a, y = np.asarray(act, np.float32), np.asarray(target, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (a - y).astype(np.float32)
        sq = (d * d).astype(np.float32)
        return (((sq[:, 0] + sq[:, 1]).astype(np.float32) + sq[:, 2]).astype(np.float32) + sq[:, 3]).astype(np.float32)


def error_table(act, target, done, edges):
    """act, target [T, 4, >= N] float32, done [T, N], edges [B + 1] -> (sse [B, N] float32, count [B, N] uint32).  What is frozen or
    outside the buckets is selected away before it meets a sum: NaN there goes nowhere."""
    done = np.asarray(done)
    T, N = done.shape
    b = buckets(ages(done), edges)
    e = step_error(np.asarray(act)[:, :, :N], np.asarray(target)[:, :, :N])
    B = len(edges) - 1
    sse, count = np.zeros((B, N), np.float32), np.zeros((B, N), np.uint32)
    cols = np.arange(N)
    for t in range(T):                       # time order; within a step every env adds to one cell of its own
        at = b[t] >= 0
        i, bi = cols[at], b[t][at]
        sse[bi, i] = (sse[bi, i] + e[t][at]).astype(np.float32)
        count[bi, i] += np.uint32(1)
    return sse, count
