"""Vehicle schedules: the tables ``l2f.VehicleBank(device, tables)`` holds and ``env.set_vehicle_schedule(bank, ids)`` attaches.

A table is ``[rows, 4]`` float32, every entry a positive factor: column 0 scales the mass, column 1 the inertia (all three axes),
column 2 the thrust curve (``c0``, ``c1``, ``c2`` alike: battery sag, a damaged propeller set) and column 3 the motor time constant
(rise and fall alike).  Row k holds for the transition an env takes at episode step count k.  A wrench schedule pushes on the
vehicle; this one changes what the dynamics divide and multiply by.  Ids are dealt with ``tracking.spread_reference_ids`` and the
``[P, M]`` table comes from ``tracking.reference_tracking_table``, as for a wrench schedule.  ``compose`` is the definition every
kernel computes (include/raptor_quad.h "Vehicle schedule"), in NumPy float32."""
import numpy as np

VEHICLE_NAMES = ("mass", "inertia", "thrust", "motor_tau")       # the four columns
MASS, INERTIA, THRUST, MOTOR_TAU = range(4)

# RQ_P_* (include/raptor_quad.h): which parameter fields each column scales
SCALED_FIELDS = {MASS: (0,), INERTIA: (1, 2, 3), THRUST: (16, 17, 18), MOTOR_TAU: (20, 21)}
_PARAM_DIM = 26


def _rows(rows):
    if int(rows) != rows or int(rows) < 1:
        raise ValueError("rows must be a positive integer")
    return int(rows)


def _step(step, what="step"):
    if int(step) != step or int(step) < 0:
        raise ValueError(f"{what} must be a non-negative integer")
    return int(step)


def _factor(x, what):
    if not np.isfinite(x) or x <= 0:
        raise ValueError(f"{what} is a positive finite factor; got {x!r}")
    return float(x)


def nominal(rows):
    """The vehicle as its parameters describe it: ones."""
    return np.ones((_rows(rows), 4), np.float32)


def payload_pickup(rows, step, mass, inertia=1.0):
    """From ``step`` on the vehicle carries a payload: mass x ``mass``, inertia x ``inertia`` (a point mass at the centre: 1)."""
    rows, k, m, j = _rows(rows), _step(step), _factor(mass, "mass"), _factor(inertia, "inertia")
    table = np.ones((rows, 4), np.float64)
    table[k:, MASS] = m
    table[k:, INERTIA] = j
    return table.astype(np.float32)


def payload_drop(rows, step, mass, inertia=1.0):
    """The vehicle starts with a payload (mass x ``mass``, inertia x ``inertia``) and lets go of it at ``step``."""
    rows, k, m, j = _rows(rows), _step(step), _factor(mass, "mass"), _factor(inertia, "inertia")
    table = np.ones((rows, 4), np.float64)
    table[:k, MASS] = m
    table[:k, INERTIA] = j
    return table.astype(np.float32)


def battery_sag(rows, start, end, thrust):
    """The thrust factor falls linearly from 1 at step ``start`` to ``thrust`` at step ``end`` and stays (``end == start``: a step)."""
    rows, a, b, f = _rows(rows), _step(start, "start"), _step(end, "end"), _factor(thrust, "thrust")
    if b < a:
        raise ValueError("end must not lie before start")
    k = np.arange(rows, dtype=np.float64)
    gain = (k >= a).astype(np.float64) if b == a else np.clip((k - a) / (b - a), 0.0, 1.0)
    table = np.ones((rows, 4), np.float64)
    table[:, THRUST] = 1.0 + gain * (f - 1.0)
    return table.astype(np.float32)


def slow_motors(rows, step, factor):
    """From ``step`` on the motors answer with ``factor`` times their time constant."""
    rows, k, f = _rows(rows), _step(step), _factor(factor, "factor")
    table = np.ones((rows, 4), np.float64)
    table[k:, MOTOR_TAU] = f
    return table.astype(np.float32)


def suite(rows, step=None):
    """A small named suite of vehicle scenarios, every table ``[rows, 4]`` float32, the change at ``step`` (default: a fifth of the
    table): nothing, a payload of 30 % of the mass picked up, the same payload dropped, a battery that sags to 85 % of the thrust
    over a fifth of the table, and motors twice as slow.  ``l2f.VehicleBank(device, list(suite(rows).values()))`` holds them."""
    rows = _rows(rows)
    k = rows // 5 if step is None else _step(step)
    return {
        "nominal": nominal(rows),
        "payload_pickup": payload_pickup(rows, k, 1.3, 1.1),
        "payload_drop": payload_drop(rows, k, 1.3, 1.1),
        "battery_sag": battery_sag(rows, k, min(rows - 1, k + max(1, rows // 5)), 0.85),
        "slow_motors": slow_motors(rows, k, 2.0),
    }


def check_tables(tables):
    """The tables of a ``VehicleBank`` as the C layer takes them, or ValueError: float32 [M >= 1, rows >= 1, 4], every entry finite
    and > 0, contiguous; a list of M ``[rows, 4]`` tables of equal length is stacked."""
    from . import schedules
    return schedules.check_tables(schedules.VEHICLE, tables)


def check_vehicle_ids(ids, n_tables, n_envs):
    """One table id per env, each in [0, n_tables) -> contiguous uint32; ValueError otherwise."""
    from . import schedules
    return schedules.check_ids(schedules.VEHICLE, ids, n_tables, n_envs)


def compose(params, row):
    """The effective parameters of one transition, as every kernel computes them: ``params`` [..., 26] the base fields, ``row``
    [..., 4] the schedule's row -> float32 [..., 26].  mass x row[0]; Jxx, Jyy, Jzz x row[1]; c0, c1, c2 x row[2]; tau_rise,
    tau_fall x row[3]; every other field the base value.  Each product is ONE float32 multiplication."""
    f32 = np.float32
    p = np.asarray(params, f32)
    r = np.asarray(row, f32)
    if p.shape[-1] != _PARAM_DIM or r.shape[-1] != 4:
        raise ValueError(f"compose takes params [..., {_PARAM_DIM}] and row [..., 4]; got {p.shape} and {r.shape}")
    out = np.broadcast_to(p, np.broadcast_shapes(p.shape[:-1], r.shape[:-1]) + (_PARAM_DIM,)).astype(f32, copy=True)
    for column, fields in SCALED_FIELDS.items():
        for f in fields:
            out[..., f] = (p[..., f] * r[..., column]).astype(f32)
    return out
