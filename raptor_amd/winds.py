"""Wind schedules: the tables ``l2f.WindBank(device, tables)`` holds and ``env.set_wind_schedule(bank, ids)`` attaches.

A table is ``[rows, 4]`` float32: columns 0..2 the air velocity in the world frame (m/s), column 3 the specific drag ``d`` (1/s, >= 0):
the drag force per unit mass and unit air speed.  Row k holds for the transition an env takes at episode step count k: the force the
transition is computed with gains ``mass * d * (w - v)``, ``v`` the vehicle's velocity entering the step, held across the step's RK4
stages.  A wrench schedule pushes whatever the vehicle does; this force depends on the vehicle's motion through the air: a steady wind
is leant into, drifting with the wind costs nothing, still air (``w = 0``, ``d > 0``) damps every motion.  Ids are dealt with
``tracking.spread_reference_ids`` and the ``[P, M]`` table comes from ``tracking.reference_tracking_table``, as for the other
schedules.  ``compose`` is the definition every kernel computes (include/raptor_quad.h "Wind schedule"), in NumPy float32."""
import numpy as np

WIND_NAMES = ("wx", "wy", "wz", "drag")       # the four columns
DRAG = 3
DEFAULT_DRAG = 0.35                           # 1/s: rotor drag of a small multirotor, a few tenths


def _rows(rows):
    if int(rows) != rows or int(rows) < 1:
        raise ValueError("rows must be a positive integer")
    return int(rows)


def _vec3(v, what):
    a = np.asarray(v, np.float64)
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError(f"{what} is three finite numbers")
    return a


def _dt(dt):
    if not np.isfinite(dt) or dt <= 0:
        raise ValueError("dt must be positive")
    return float(dt)


def _drag(drag):
    if not np.isfinite(drag) or drag < 0:
        raise ValueError(f"drag is a finite number >= 0 (1/s); got {drag!r}")
    return float(drag)


def _table(rows, velocity, drag):
    """velocity [rows, 3] or [3] float64, one drag -> [rows, 4] float32"""
    table = np.zeros((rows, 4), np.float64)
    table[:, 0:3] = velocity
    table[:, DRAG] = drag
    return table.astype(np.float32)


def calm(rows):
    """No wind and no drag: zeros (the unscheduled transition)."""
    return np.zeros((_rows(rows), 4), np.float32)


def still_air(rows, drag):
    """Air at rest that drags: ``w = 0``, damping only."""
    return _table(_rows(rows), 0.0, _drag(drag))


def steady(rows, velocity, drag):
    """A constant air ``velocity`` (3 numbers, world frame, m/s)."""
    return _table(_rows(rows), _vec3(velocity, "velocity"), _drag(drag))


def gust(rows, dt, velocity, start_s, duration_s, drag):
    """Air at ``velocity`` on the steps k with start_s <= k dt < start_s + duration_s, at rest otherwise; the drag holds throughout."""
    rows, dt, v, d = _rows(rows), _dt(dt), _vec3(velocity, "velocity"), _drag(drag)
    if not (np.isfinite(start_s) and np.isfinite(duration_s)) or start_s < 0 or duration_s < 0:
        raise ValueError("start_s and duration_s must be non-negative")
    t = np.arange(rows, dtype=np.float64) * dt
    on = ((t >= start_s) & (t < start_s + duration_s)).astype(np.float64)
    return _table(rows, on[:, None] * v, d)


def ramp(rows, dt, velocity, start_s, rise_s, drag):
    """A wind that builds up: velocity * clip((k dt - start_s) / rise_s, 0, 1) (``rise_s`` 0: a step at ``start_s``)."""
    rows, dt, v, d = _rows(rows), _dt(dt), _vec3(velocity, "velocity"), _drag(drag)
    if not (np.isfinite(start_s) and np.isfinite(rise_s)) or start_s < 0 or rise_s < 0:
        raise ValueError("start_s and rise_s must be non-negative")
    t = np.arange(rows, dtype=np.float64) * dt
    gain = (t >= start_s).astype(np.float64) if rise_s == 0 else np.clip((t - start_s) / rise_s, 0.0, 1.0)
    return _table(rows, gain[:, None] * v, d)


def turbulence(rows, dt, mean, sigma, tau_s, drag, seed):
    """An Ornstein-Uhlenbeck air velocity around ``mean``: per axis x_0 ~ N(0, sigma^2), x_{k+1} = a x_k + sigma sqrt(1 - a^2) n_k with
    a = exp(-dt / tau_s) and n_k standard normal (the exact discretisation: stationary standard deviation ``sigma``, correlation time
    ``tau_s``), computed in float64 from ``numpy.random.default_rng(seed)``: the same table for the same arguments."""
    rows, dt, m, d = _rows(rows), _dt(dt), _vec3(mean, "mean"), _drag(drag)
    if not (np.isfinite(sigma) and np.isfinite(tau_s)) or sigma < 0 or tau_s <= 0:
        raise ValueError("sigma must be non-negative and tau_s positive")
    if int(seed) != seed or int(seed) < 0:
        raise ValueError("seed must be a non-negative integer")
    g = np.random.default_rng(int(seed))
    noise = g.standard_normal((rows, 3))
    a = np.exp(-dt / float(tau_s))
    x = np.empty((rows, 3), np.float64)
    x[0] = float(sigma) * noise[0]
    kick = float(sigma) * np.sqrt(1.0 - a * a)
    for k in range(1, rows):
        x[k] = a * x[k - 1] + kick * noise[k]
    return _table(rows, m + x, d)


def suite(rows, dt):
    """A small named suite of wind scenarios, every table ``[rows, 4]`` float32, drag ``DEFAULT_DRAG``: calm air without drag, still
    air, steady winds of 2, 5 and 8 m/s along x, a 5 m/s cross gust over the second quarter of the table, a wind that builds up to
    5 m/s, and turbulence of 1.5 m/s around a 3 m/s mean.  ``l2f.WindBank(device, list(suite(rows, dt).values()))`` holds them."""
    rows, dt = _rows(rows), _dt(dt)
    quarter = rows // 4
    d = DEFAULT_DRAG
    return {
        "calm": calm(rows),
        "still_air": still_air(rows, d),
        "steady_2": steady(rows, (2.0, 0.0, 0.0), d),
        "steady_5": steady(rows, (5.0, 0.0, 0.0), d),
        "steady_8": steady(rows, (8.0, 0.0, 0.0), d),
        "gust": gust(rows, dt, (0.0, 5.0, 0.0), quarter * dt, quarter * dt, d),
        "ramp": ramp(rows, dt, (5.0, 0.0, 0.0), quarter * dt, quarter * dt, d),
        "turbulence": turbulence(rows, dt, (3.0, 0.0, 0.0), 1.5, 1.0, d, 0),
    }


def check_tables(tables):
    """The tables of a ``WindBank`` as the C layer takes them, or ValueError: float32 [M >= 1, rows >= 1, 4], every entry finite, the
    drag column >= 0, contiguous; a list of M ``[rows, 4]`` tables of equal length is stacked."""
    from . import schedules
    return schedules.check_tables(schedules.WIND, tables)


def check_wind_ids(ids, n_tables, n_envs):
    """One table id per env, each in [0, n_tables) -> contiguous uint32; ValueError otherwise."""
    from . import schedules
    return schedules.check_ids(schedules.WIND, ids, n_tables, n_envs)


def compose(base6, mass, velocity3, row4):
    """The wrench of one transition, as every kernel computes it: ``base6`` [..., 6] the force | torque the step would use without the
    wind (the state's per-episode one, or ``disturbances.compose`` of it), ``mass`` [...] the step's mass, ``velocity3`` [..., 3] the
    linear velocity of the state before the step, ``row4`` [..., 4] the schedule's row -> float32 [..., 6].
    md = mass * row[3]; u = row[0:3] - v; force = base + (md * u); the torque is the base's.  Every product, difference and sum is ONE
    float32 operation, in this order; nothing is fused."""
    f32 = np.float32
    base = np.asarray(base6, f32)
    m = np.asarray(mass, f32)
    v = np.asarray(velocity3, f32)
    r = np.asarray(row4, f32)
    if base.shape[-1] != 6 or v.shape[-1] != 3 or r.shape[-1] != 4:
        raise ValueError(f"compose takes base [..., 6], velocity [..., 3] and row [..., 4]; got {base.shape}, {v.shape} and {r.shape}")
    md = (m * r[..., DRAG]).astype(f32)
    u = (r[..., 0:3] - v).astype(f32)
    drag = (md[..., None] * u).astype(f32)
    out = np.broadcast_to(base, np.broadcast_shapes(base.shape[:-1], drag.shape[:-1]) + (6,)).astype(f32, copy=True)
    out[..., 0:3] = (out[..., 0:3] + drag).astype(f32)
    return out
