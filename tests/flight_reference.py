"""The flight table restated in NumPy float32 (rq_trajectory_flight_table, csrc/rq_flight_table.inc), written env by env from the
rule in include/raptor_quad.h ("Flight table") and sharing nothing with the kernel, so that sum, peak and count can be held to it
bit for bit.

Age: start_steps[i] at the first recorded step (None: 0); a step is live when its done code is not 4; after a live step with code 1
or 2 the age is 0, after any other live step one more; a frozen step changes nothing and contributes nothing.  A live step of age k
belongs to bucket b when edges[b] <= k < edges[b + 1]; outside every bucket it is counted nowhere.  Per counted step nine values,
every operation rounded to float32 on its own, summed s = s + v in time order from 0; three peaks from 0 by p = v > p ? v : p."""
import numpy as np

F = np.float32
SUMS = ["pos2", "vel2", "omega2", "tilt", "act2", "dact2", "saturated", "outside", "reward"]
PEAKS = ["pos2", "tilt", "omega2"]          # the sum columns 0, 3, 2


def ages(done, start_steps=None):
    """done [T, N] codes -> k [T, N] int64: the age of every step, -1 on a frozen one - env by env, step by step, as stated"""
    done = np.asarray(done)
    T, N = done.shape
    out = np.full((T, N), -1, np.int64)
    for i in range(N):
        age = 0 if start_steps is None else int(start_steps[i])
        for t in range(T):
            d = int(done[t, i])
            if d == 4:
                continue
            out[t, i] = age
            age = 0 if d in (1, 2) else age + 1
    return out


def bucket_of(k, edges):
    """one age and edges [B + 1] -> its bucket, or -1"""
    for b in range(len(edges) - 1):
        if int(edges[b]) <= k < int(edges[b + 1]):
            return b
    return -1


def _sq3(p, q, s):
    return ((p * p).astype(F) + (q * q).astype(F)).astype(F) + (s * s).astype(F)


def step_values(x, a, r, tol2):
    """x [..., 22], a [..., 4], r [...] float32 -> the nine values of every step, float32 [..., 9]; float32 arrays throughout, so
    every operation is rounded once (NaN where an input is NaN: the caller never looks at what it does not count)"""
    x, a, r = np.asarray(x, F), np.asarray(a, F), np.asarray(r, F)
    pos2 = _sq3(x[..., 0], x[..., 1], x[..., 2]).astype(F)
    vel2 = _sq3(x[..., 12], x[..., 13], x[..., 14]).astype(F)
    omega2 = _sq3(x[..., 15], x[..., 16], x[..., 17]).astype(F)
    tilt = (F(1.0) - x[..., 11]).astype(F)
    act2 = (_sq3(a[..., 0], a[..., 1], a[..., 2]).astype(F) + (a[..., 3] * a[..., 3]).astype(F)).astype(F)
    d = (a - x[..., 18:22]).astype(F)
    dact2 = (_sq3(d[..., 0], d[..., 1], d[..., 2]).astype(F) + (d[..., 3] * d[..., 3]).astype(F)).astype(F)
    saturated = (np.abs(a) >= F(1.0)).sum(-1).astype(F)
    outside = (pos2 > tol2).astype(F)
    return np.stack([pos2, vel2, omega2, tilt, act2, dact2, saturated, outside, r], axis=-1).astype(F)


def flight_table(obs, act, rew, done, edges, start_steps=None, tolerance=0.05):
    """obs [T, N, 22], act [T, N, 4], rew [T, N] float32, done [T, N] (``Trajectory.numpy()``), edges [B + 1] ->
    (sum [B, 9, N] float32, peak [B, 3, N] float32, count [B, N] uint32).  What is frozen or outside the buckets is selected away
    before it meets a sum: NaN there goes nowhere."""
    done = np.asarray(done)
    T, N = done.shape
    B = len(edges) - 1
    tol2 = F(F(tolerance) * F(tolerance))
    k = ages(done, start_steps)
    with np.errstate(invalid="ignore", over="ignore"):
        v = step_values(obs, act, rew, tol2)                 # [T, N, 9]
        total, peak, count = np.zeros((B, 9, N), F), np.zeros((B, 3, N), F), np.zeros((B, N), np.uint32)
        for i in range(N):
            for t in range(T):
                if k[t, i] < 0:
                    continue
                b = bucket_of(int(k[t, i]), edges)
                if b < 0:
                    continue
                total[b, :, i] = (total[b, :, i] + v[t, i]).astype(F)
                for j, c in enumerate((0, 3, 2)):
                    if v[t, i, c] > peak[b, j, i]:
                        peak[b, j, i] = v[t, i, c]
                count[b, i] += np.uint32(1)
    return total, peak, count
