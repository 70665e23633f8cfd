"""Reference tables for tracked rollouts (``vector.rollout(..., reference=l2f.Reference(device, table))``).

A table is float32 ``[rows, 6]``: columns 0..2 the target position, columns 3..5 the target linear velocity, world frame (FLU), one
row per env step.  An env reads the row of its own episode step count, so ``rows`` must be at least the env's ``episode_step_limit``
and ``dt`` its step (0.01 s by default).  Positions and velocities are computed in float64 - the velocities analytically, not by
differencing - and rounded once.  The path must stay inside ``termination_position``: termination looks at the absolute position.
"""
import numpy as np

__all__ = ["lissajous", "lissajous64", "hold"]


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
