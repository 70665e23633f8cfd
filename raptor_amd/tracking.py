"""Reference tables for tracked rollouts (``vector.rollout(..., reference=l2f.Reference(device, table))``), suites of them for a
reference bank (``l2f.ReferenceBank(device, tables)`` with one ``reference_ids`` entry per env) and the per-reference error table.

A table is float32 ``[rows, 6]``: columns 0..2 the target position, columns 3..5 the target linear velocity, world frame (FLU), one
row per env step.  An env reads the row of its own episode step count, so ``rows`` must be at least the env's ``episode_step_limit``
and ``dt`` its step (0.01 s by default).  Positions and velocities are computed in float64 - the velocities analytically, not by
differencing - and rounded once.  The path must stay inside ``termination_position``: termination looks at the absolute position.
"""
import numpy as np

__all__ = ["lissajous", "lissajous64", "hold", "circle", "circle64", "step_setpoint", "suite", "spread_reference_ids",
           "check_reference_ids", "reference_tracking_table"]


def _rows(rows):
    if int(rows) != rows or rows < 1:
        raise ValueError("rows must be a positive integer")
    return int(rows)


def hold(rows):
    """The origin, at rest, for ``rows`` steps: tracking it is regulating to the origin (the untracked rollout)."""
    return np.zeros((_rows(rows), 6), np.float32)


def lissajous(rows, dt, amplitude, period, ratio=(1, 2, 0)):
    """The float32 table of ``lissajous64``: p_i(t) = amplitude_i sin(ratio_i 2 pi t / period), t = k dt for row k, with v = dp/dt.  The default ratio (1, 2, 0) with
    amplitudes (a, a / 2, 0) is the figure-eight in the horizontal plane the policy is usually shown flying; every axis starts
    at the origin.  ``amplitude``: a scalar or one value per axis (metres); ``period`` (seconds) is that of a ratio-1 axis."""
    return lissajous64(rows, dt, amplitude, period, ratio).astype(np.float32)


def lissajous64(rows, dt, amplitude, period, ratio=(1, 2, 0)):
    """``lissajous`` before it is rounded: the float64 positions and analytic velocities, [rows, 6]."""
    rows = _rows(rows)
    if not (np.isfinite(dt) and dt > 0 and np.isfinite(period) and period > 0):
        raise ValueError("dt and period must be positive")
    a = np.broadcast_to(np.asarray(amplitude, np.float64), (3,))
    r = np.asarray(ratio, np.float64)
    if r.shape != (3,) or not (np.isfinite(a).all() and np.isfinite(r).all()):
        raise ValueError("amplitude: a scalar or three values; ratio: three values")
    w = 2.0 * np.pi * r / float(period)                      # rad/s per axis
    t = np.arange(rows, dtype=np.float64)[:, None] * float(dt)
    table = np.empty((rows, 6), np.float64)
    table[:, 0:3] = a * np.sin(w * t)
    table[:, 3:6] = a * w * np.cos(w * t)
    return table


def circle(rows, dt, radius, period):
    """The float32 table of ``circle64``: a horizontal circle flown once per ``period`` seconds that STARTS AT THE ORIGIN - its centre
    is at (radius, 0, 0), p(t) = (radius (1 - cos wt), radius sin wt, 0), w = 2 pi / period - so every episode starts on the path."""
    return circle64(rows, dt, radius, period).astype(np.float32)


def circle64(rows, dt, radius, period):
    """``circle`` before it is rounded: the float64 positions and analytic velocities, [rows, 6]."""
    rows = _rows(rows)
    if not (np.isfinite(dt) and dt > 0 and np.isfinite(period) and period > 0 and np.isfinite(radius)):
        raise ValueError("dt and period must be positive, radius finite")
    w = 2.0 * np.pi / float(period)
    t = np.arange(rows, dtype=np.float64) * float(dt)
    table = np.zeros((rows, 6), np.float64)
    table[:, 0] = radius * (1.0 - np.cos(w * t))
    table[:, 1] = radius * np.sin(w * t)
    table[:, 3] = radius * w * np.sin(w * t)
    table[:, 4] = radius * w * np.cos(w * t)
    return table


def step_setpoint(rows, dt, offset, at_step):
    """A position step: the origin for the rows before ``at_step``, ``offset`` (three values, metres) from that row on, at rest
    throughout (the target velocity is zero: the jump is the policy's to fly).  ``dt`` is taken, and checked, as every generator takes
    it; the table does not depend on it."""
    rows = _rows(rows)
    if not (np.isfinite(dt) and dt > 0):
        raise ValueError("dt must be positive")
    o = np.asarray(offset, np.float64)
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError("offset: three finite values")
    if int(at_step) != at_step or at_step < 0:
        raise ValueError("at_step must be a non-negative integer")
    table = np.zeros((rows, 6), np.float64)
    table[int(at_step):, 0:3] = o
    return table.astype(np.float32)


def suite(rows, dt):
    """A small named suite of setpoints for checkpoint selection, every table ``[rows, 6]`` float32 and within 0.3 m of the origin
    on every axis - well inside the default ``termination_position`` of 1 m: a hover, the figure-eight at two speeds, a circle and a
    position step.  ``l2f.ReferenceBank(device, list(suite(rows, dt).values()))`` flies them side by side."""
    return {
        "hold": hold(rows),
        "eight_slow": lissajous(rows, dt, amplitude=(0.3, 0.15, 0.0), period=10.0),
        "eight_fast": lissajous(rows, dt, amplitude=(0.3, 0.15, 0.0), period=5.0),
        "circle": circle(rows, dt, radius=0.15, period=5.0),
        "step": step_setpoint(rows, dt, offset=(0.2, 0.0, 0.1), at_step=_rows(rows) // 4),
    }


def check_reference_ids(ids, n_references, n_envs=None):
    """The host-side validator of ``reference_ids`` (no GPU): an integer array, one id per env (``n_envs`` given: exactly that many),
    each in [0, n_references); ids are free per env.  -> the ids as a contiguous uint32 array; ValueError otherwise."""
    a = np.asarray(ids)
    if a.ndim != 1 or a.size == 0:
        raise ValueError("reference_ids must be a non-empty one-dimensional array: one id per env")
    if n_envs is not None and a.size != int(n_envs):
        raise ValueError(f"reference_ids must hold one id per env: {a.size} ids for {int(n_envs)} envs")
    if a.dtype == bool or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("reference_ids must be integers")
    a = a.astype(np.int64)
    bad = np.flatnonzero((a < 0) | (a >= int(n_references)))
    if bad.size:
        raise ValueError(f"reference id out of range: env {int(bad[0])} names reference {int(a[bad[0]])} of a bank of {int(n_references)}")
    return np.ascontiguousarray(a.astype(np.uint32))


def spread_reference_ids(n_envs, n_references, policy_ids=None):
    """reference id of every env (uint32 [n_envs]), the references dealt evenly: env i -> i % n_references, or, with ``policy_ids``
    ([n_envs]), the j-th env of every policy -> j % n_references, so that every policy flies every reference equally often (counts
    differ by at most one)."""
    n_envs, n_references = int(n_envs), int(n_references)
    if n_envs <= 0 or n_references <= 0:
        raise ValueError("n_envs and n_references must be positive")
    rank = np.arange(n_envs, dtype=np.int64)
    if policy_ids is not None:
        p = np.asarray(policy_ids, np.int64).ravel()
        if p.shape != (n_envs,):
            raise ValueError("policy_ids must hold one id per env")
        order = np.argsort(p, kind="stable")
        sorted_p = p[order]
        first = np.flatnonzero(np.r_[True, sorted_p[1:] != sorted_p[:-1]])             # where each policy's envs start
        start = first[np.cumsum(np.r_[False, sorted_p[1:] != sorted_p[:-1]])]
        rank = np.empty(n_envs, np.int64)
        rank[order] = np.arange(n_envs, dtype=np.int64) - start
    return np.ascontiguousarray((rank % n_references).astype(np.uint32))


def reference_tracking_table(sum_sq, steps, reference_ids, n_references, policy_ids=None, n_policies=None):
    """Per-reference tracking error from the per-env sums ``env.tracking_error()`` returns, as ``policy_tracking_table`` groups them by
    policy: ``tracking_rmse`` float64 [n_references] = sqrt(sum of the reference's sums / sum of its counts), the mean over STEPS, NaN
    for a cell without a counted step.  With ``policy_ids`` and ``n_policies``: [n_policies, n_references], cell (p, r) over the envs
    policy p flew on reference r."""
    ids = np.asarray(reference_ids, np.int64).ravel()
    sq = np.asarray(sum_sq, np.float64).ravel()
    cnt = np.asarray(steps, np.float64).ravel()
    if not (ids.shape == sq.shape == cnt.shape):
        raise ValueError("sum_sq, steps and reference_ids must hold one entry per env")
    m = int(n_references)
    shape = (m,)
    if (policy_ids is None) != (n_policies is None):
        raise ValueError("policy_ids and n_policies go together")
    if policy_ids is not None:
        p = np.asarray(policy_ids, np.int64).ravel()
        if p.shape != ids.shape:
            raise ValueError("policy_ids must hold one entry per env")
        ids = p * m + ids
        shape = (int(n_policies), m)
    cells = shape[0] * (shape[1] if len(shape) == 2 else 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(np.bincount(ids, weights=sq, minlength=cells) / np.bincount(ids, weights=cnt, minlength=cells)).reshape(shape)
