"""A numpy reference of the timed probe moments (rq_trajectory_probe_moments_timed) and of the wrench targets
(rq_trajectory_wrench_targets), written from the rule in include/raptor_quad.h and sharing nothing with the kernels.  The age rule
and the buckets are tests/probe_reference.py's.

Timed moments: the sample of a live step t of env i is z = [1, h_t (16), targets[t, i, 0 .. M-1], 0 ...]; everything else is the
untimed rule.  Float64.

Wrench targets: per env k = start[i]; at step t with done code d: d == 4 gives six 0.0f and leaves k; otherwise the row is
table[id[i]][min(k, rows - 1)], as it is (relative output) or scaled to N and N m (absolute output of a relative bank: fs row[0..2],
ts row[3..5], one float32 product each); then k = 0 if d is 1 or 2, else k + 1.  The scaling follows
raptor_amd.disturbances.compose operation for operation in float32."""
import numpy as np

import probe_reference as R

DIM = R.DIM
RELATIVE, ABSOLUTE = "relative", "absolute"


def samples_timed(hidden, targets):
    """hidden [T, N, 16], targets [T, N, M] -> z [T, N, 32] float64 = [1, h_t, y_t, 0 ...]"""
    h = np.asarray(hidden, np.float64)
    y = np.asarray(targets, np.float64)
    T, N, _ = h.shape
    assert y.shape[:2] == (T, N) and y.shape[2] <= DIM - 17
    z = np.zeros((T, N, DIM))
    z[:, :, 0] = 1.0
    z[:, :, 1:17] = h
    z[:, :, 17:17 + y.shape[2]] = y
    return z


def moments_timed(hidden, done, targets, edges):
    """-> dict(age [T, N], bucket [T, N], counts [B] uint64, S [B, 32, 32] = sum z z^T, A [B, 32, 32] = sum |z| |z|^T), float64"""
    age, _ = R.ages(done)
    bucket = R.buckets(age, edges)
    z = samples_timed(hidden, targets)
    B = len(edges) - 1
    S, A, counts = np.zeros((B, DIM, DIM)), np.zeros((B, DIM, DIM)), np.zeros(B, np.uint64)
    for b in range(B):
        zb = z[bucket == b]                   # NaN in a row that is not selected goes nowhere
        counts[b] = zb.shape[0]
        S[b] = zb.T @ zb
        A[b] = np.abs(zb).T @ np.abs(zb)
    return dict(age=age, bucket=bucket, counts=counts, S=S, A=A)


def episode_steps(done, start=None):
    """done [T, N], start [N] (None: 0) -> (k [T, N] int64, -1 on code 4; k_end [N]: the count after the last step)"""
    done = np.asarray(done)
    T, N = done.shape
    k = [0] * N if start is None else [int(v) for v in start]
    out = np.full((T, N), -1, np.int64)
    for i in range(N):                        # env by env, step by step: the rule as it is written
        for t in range(T):
            d = int(done[t, i])
            if d == 4:
                continue
            out[t, i] = k[i]
            k[i] = 0 if d in (1, 2) else k[i] + 1
    return out, np.asarray(k, np.int64)


def wrench_scales(mass, gravity, rotor_xy):
    """fs = m g, ts = (m g) arm with arm = sqrt(x0 x0 + y0 y0): every operation one float32 operation (disturbances.compose)"""
    f32 = np.float32
    m = np.asarray(mass, f32)
    xy = np.asarray(rotor_xy, f32)
    x0, y0 = xy[..., 0], xy[..., 1]
    mg = (m * f32(gravity)).astype(f32)
    arm = np.sqrt(((x0 * x0).astype(f32) + (y0 * y0).astype(f32)).astype(f32)).astype(f32)
    return mg, (mg * arm).astype(f32)


def wrench_targets(done, start, tables, ids, mass, gravity, rotor_xy, bank_units=RELATIVE, units_out=RELATIVE):
    """done [T, N], start [N] or None, tables [M, rows, 6], ids [N] or None, mass [N], rotor_xy [N, 2] -> float32 [T, N, 6]"""
    if units_out == RELATIVE and bank_units == ABSOLUTE:
        raise ValueError("relative output from an absolute bank")
    f32 = np.float32
    tab = np.asarray(tables, f32)
    done = np.asarray(done)
    T, N = done.shape
    ids = np.zeros(N, np.int64) if ids is None else np.asarray(ids, np.int64)
    k, _ = episode_steps(done, start)
    rows = tab[ids[None, :], np.minimum(np.maximum(k, 0), tab.shape[1] - 1)]          # [T, N, 6]
    out = rows.copy()
    if units_out == ABSOLUTE and bank_units == RELATIVE:
        fs, ts = wrench_scales(mass, gravity, rotor_xy)
        out[..., 0:3] = (fs[None, :, None] * rows[..., 0:3]).astype(f32)
        out[..., 3:6] = (ts[None, :, None] * rows[..., 3:6]).astype(f32)
    out[k < 0] = f32(0.0)
    return out
