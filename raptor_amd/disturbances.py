"""Wrench schedules: the tables ``l2f.WrenchBank(device, tables, units)`` holds and ``env.set_wrench_schedule(bank, ids)`` attaches.

A table is ``[rows, 6]`` float32: columns 0..2 a force in the world frame, 3..5 a torque in the body frame, row k applied at the
transition an env takes at episode step count k.  In relative units (the default) a force is in multiples of ``m g`` and a torque in
multiples of ``m g arm`` - the units of the config's ``disturbance_force_std`` / ``disturbance_torque_std``.  Ids are dealt with
``tracking.spread_reference_ids`` and the ``[P, M]`` table comes from ``tracking.reference_tracking_table``: both are generic over ids.
``compose`` is the definition every kernel computes (include/raptor_quad.h "Wrench schedule"), in NumPy float32."""
import numpy as np

RELATIVE, ABSOLUTE = "relative", "absolute"
UNITS = {RELATIVE: 0, ABSOLUTE: 1}          # rq_wrench_units


def _rows(rows):
    if int(rows) != rows or int(rows) < 1:
        raise ValueError("rows must be a positive integer")
    return int(rows)


def _step(at_step, what="at_step"):
    if int(at_step) != at_step or int(at_step) < 0:
        raise ValueError(f"{what} must be a non-negative integer")
    return int(at_step)


def _vec3(v, what):
    a = np.asarray(v, np.float64)
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError(f"{what} is three finite numbers")
    return a


def _dt(dt):
    if not np.isfinite(dt) or dt <= 0:
        raise ValueError("dt must be positive")
    return float(dt)


def calm(rows):
    """No scheduled wrench: zeros."""
    return np.zeros((_rows(rows), 6), np.float32)


def gust(rows, dt, force, start_s, duration_s):
    """A constant ``force`` (3 numbers, world frame) on the steps k with start_s <= k dt < start_s + duration_s."""
    rows, dt, f = _rows(rows), _dt(dt), _vec3(force, "force")
    if not (np.isfinite(start_s) and np.isfinite(duration_s)) or start_s < 0 or duration_s < 0:
        raise ValueError("start_s and duration_s must be non-negative")
    t = np.arange(rows, dtype=np.float64) * dt
    table = np.zeros((rows, 6), np.float64)
    table[(t >= start_s) & (t < start_s + duration_s), 0:3] = f
    return table.astype(np.float32)


def poke(rows, force, at_step, steps=1):
    """``force`` on the steps at_step .. at_step + steps - 1."""
    rows, f, k, n = _rows(rows), _vec3(force, "force"), _step(at_step), _step(steps, "steps")
    table = np.zeros((rows, 6), np.float64)
    table[k:k + n, 0:3] = f
    return table.astype(np.float32)


def ramp(rows, dt, force, start_s, rise_s):
    """A force that rises linearly from 0 at ``start_s`` to ``force`` at ``start_s + rise_s`` and stays: force * clip((k dt -
    start_s) / rise_s, 0, 1) (``rise_s`` 0: a step at ``start_s``)."""
    rows, dt, f = _rows(rows), _dt(dt), _vec3(force, "force")
    if not (np.isfinite(start_s) and np.isfinite(rise_s)) or start_s < 0 or rise_s < 0:
        raise ValueError("start_s and rise_s must be non-negative")
    t = np.arange(rows, dtype=np.float64) * dt
    gain = (t >= start_s).astype(np.float64) if rise_s == 0 else np.clip((t - start_s) / rise_s, 0.0, 1.0)
    table = np.zeros((rows, 6), np.float64)
    table[:, 0:3] = gain[:, None] * f
    return table.astype(np.float32)


def payload(rows, fraction, at_step):
    """A payload of ``fraction`` of the vehicle's weight (relative units) that hangs on from ``at_step``: ``-fraction`` on z."""
    rows, k = _rows(rows), _step(at_step)
    if not np.isfinite(fraction):
        raise ValueError("fraction must be finite")
    table = np.zeros((rows, 6), np.float64)
    table[k:, 2] = -float(fraction)
    return table.astype(np.float32)


def torque_kick(rows, torque, at_step, steps=1):
    """``torque`` (3 numbers, body frame) on the steps at_step .. at_step + steps - 1."""
    rows, tq, k, n = _rows(rows), _vec3(torque, "torque"), _step(at_step), _step(steps, "steps")
    table = np.zeros((rows, 6), np.float64)
    table[k:k + n, 3:6] = tq
    return table.astype(np.float32)


def suite(rows, dt):
    """A small named suite of disturbance scenarios in RELATIVE units, every table ``[rows, 6]`` float32: nothing, a lateral gust of
    0.3 m g over the second quarter of the episode, a 5-step poke of 1 m g, a wind that builds up to 0.2 m g, a payload of a fifth of
    the weight from the middle, and a 5-step roll kick.  ``l2f.WrenchBank(device, list(suite(rows, dt).values()))`` holds them."""
    rows, dt = _rows(rows), _dt(dt)
    quarter = rows // 4
    return {
        "calm": calm(rows),
        "gust": gust(rows, dt, (0.3, 0.0, 0.0), quarter * dt, quarter * dt),
        "poke": poke(rows, (0.0, 1.0, 0.0), quarter, steps=5),
        "ramp": ramp(rows, dt, (0.2, 0.0, 0.0), quarter * dt, quarter * dt),
        "payload": payload(rows, 0.2, rows // 2),
        "torque_kick": torque_kick(rows, (0.05, 0.0, 0.0), quarter, steps=5),
    }


def check_tables(tables):
    """The tables of a ``WrenchBank`` as the C layer takes them, or ValueError: float32 [M >= 1, rows >= 1, 6], finite, contiguous;
    a list of M ``[rows, 6]`` tables of equal length is stacked."""
    from . import schedules
    return schedules.check_tables(schedules.WRENCH, tables)


def check_units(units):
    if units not in UNITS:
        raise ValueError(f"units must be 'relative' or 'absolute'; got {units!r}")
    return UNITS[units]


def check_wrench_ids(ids, n_tables, n_envs):
    """One table id per env, each in [0, n_tables) -> contiguous uint32; ValueError otherwise."""
    from . import schedules
    return schedules.check_ids(schedules.WRENCH, ids, n_tables, n_envs)


def compose(base6, mass, gravity, rotor_xy, row, units=RELATIVE):
    """The wrench of one transition, as every kernel computes it: ``base6`` [..., 6] the state's per-episode force | torque, ``row``
    [..., 6] the schedule's row, ``mass`` [...] and ``rotor_xy`` [..., 2] (x, y of rotor 0) from the parameters -> float32 [..., 6].
    Every product, sum and square root is ONE float32 operation, in the order of include/raptor_quad.h; nothing is fused."""
    f32 = np.float32
    relative = check_units(units) == 0
    base = np.asarray(base6, f32)
    r = np.asarray(row, f32)
    m = np.asarray(mass, f32)
    xy = np.asarray(rotor_xy, f32)
    x0, y0 = xy[..., 0], xy[..., 1]
    mg = (m * f32(gravity)).astype(f32)
    arm = np.sqrt(((x0 * x0).astype(f32) + (y0 * y0).astype(f32)).astype(f32)).astype(f32)
    one = np.ones_like(mg)
    fs = mg if relative else one
    ts = (mg * arm).astype(f32) if relative else one
    out = np.empty(np.broadcast(base, r).shape, f32)
    out[..., 0:3] = base[..., 0:3] + (fs[..., None] * r[..., 0:3]).astype(f32)
    out[..., 3:6] = base[..., 3:6] + (ts[..., None] * r[..., 3:6]).astype(f32)
    return out
