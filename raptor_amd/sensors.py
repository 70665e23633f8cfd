"""Sensor schedules: the tables ``l2f.SensorBank(device, tables)`` holds and ``env.set_sensor_schedule(bank, ids)`` attaches.

A table is ``[rows]`` uint8: the observation latency in steps, ``0 <= d <= MAX_STEPS``.  Row k holds for the observation assembled
for an env at episode step count k: the policy sees, in columns 0..17 (position, rotation matrix, linear and angular velocity), the
reading taken ``d' = min(d, k)`` steps earlier in the same episode - the stored bits, observation noise included, before any setpoint
row is subtracted; an episode younger than the delay sees its first reading held.  Columns from 18 on (the controller's own last
command, the rotor tail of ``vector.observe``) are today's.  State and env step are unchanged; a recording holds what the policy
saw.  ``raptor_amd.delays`` is the same on the command side.  Ids are dealt with ``tracking.spread_reference_ids`` and the ``[P, M]``
table comes from ``tracking.reference_tracking_table``, as for the other schedules.  ``delivered`` is the definition every kernel
computes (include/raptor_quad.h "Sensor schedule"), in NumPy."""
import numpy as np

MAX_STEPS = 16                                # RQ_SENSOR_MAX_STEPS: 160 ms at dt = 10 ms, 40 ms at 2.5 ms
READING_COLUMNS = 18                          # position 0..2, rotation matrix 3..11, linear velocity 12..14, angular velocity 15..17


def _rows(rows):
    if int(rows) != rows or int(rows) < 1:
        raise ValueError("rows must be a positive integer")
    return int(rows)


def _steps(d, what="d"):
    if int(d) != d or not 0 <= int(d) <= MAX_STEPS:
        raise ValueError(f"{what} is a whole number of steps in [0, {MAX_STEPS}]; got {d!r}")
    return int(d)


def _row(k, rows, what):
    if int(k) != k or int(k) < 0:
        raise ValueError(f"{what} is a non-negative step count")
    return min(int(k), rows)


def steps_for(seconds, dt):
    """The delay in steps that stands for ``seconds`` of latency at control period ``dt``: rounded to the nearest step (0.5 rounds
    up); ValueError above ``MAX_STEPS``."""
    if not (np.isfinite(seconds) and np.isfinite(dt)) or seconds < 0 or dt <= 0:
        raise ValueError("seconds must be non-negative and dt positive")
    d = int(np.floor(float(seconds) / float(dt) + 0.5))
    if d > MAX_STEPS:
        raise ValueError(f"{seconds} s at dt = {dt} s are {d} steps: a sensor schedule holds at most {MAX_STEPS}")
    return d


def none(rows):
    """No latency: zeros (the unscheduled observation, bit for bit)."""
    return np.zeros(_rows(rows), np.uint8)


def constant(rows, d):
    """The same latency at every step."""
    return np.full(_rows(rows), _steps(d), np.uint8)


def jitter(rows, lo, hi, seed):
    """A latency drawn per step, uniform on the whole numbers ``lo .. hi``, from ``numpy.random.default_rng(seed)``: the same table
    for the same arguments."""
    rows, lo, hi = _rows(rows), _steps(lo, "lo"), _steps(hi, "hi")
    if lo > hi:
        raise ValueError("lo must not exceed hi")
    if int(seed) != seed or int(seed) < 0:
        raise ValueError("seed must be a non-negative integer")
    return np.random.default_rng(int(seed)).integers(lo, hi + 1, rows).astype(np.uint8)


def low_rate(rows, period):
    """A sensor that refreshes every ``period``-th step and is held between: d = k mod period (an estimator at 1 / period of the
    control rate)."""
    rows = _rows(rows)
    if int(period) != period or not 1 <= int(period) <= MAX_STEPS + 1:
        raise ValueError(f"period is a whole number of steps in [1, {MAX_STEPS + 1}]; got {period!r}")
    return (np.arange(rows) % int(period)).astype(np.uint8)


def dropout(rows, start, length):
    """A link that drops ``length`` readings from step ``start`` on and holds the last one it got: d = 0 before, then 0, 1, 2, ...,
    ``length`` (the reading of step ``start`` is seen on), then back to 0."""
    rows, length = _rows(rows), _steps(length, "length")
    start = _row(start, rows, "start")
    t = np.zeros(rows, np.uint8)
    ramp = np.arange(length + 1, dtype=np.uint8)
    n = min(length + 1, rows - start)
    t[start:start + n] = ramp[:n]
    return t


def onset(rows, start, d):
    """No latency before step ``start``, ``d`` steps from it on."""
    rows, d = _rows(rows), _steps(d)
    t = np.zeros(rows, np.uint8)
    t[_row(start, rows, "start"):] = d
    return t


def suite(rows):
    """A small named suite of sensor scenarios, every table ``[rows]`` uint8: none, constant delays of 1, 2, 4 and 8 steps, a jitter
    of 0 .. 3 steps, a sensor at a quarter of the control rate, a dropout of 8 readings and an onset of 4 steps, the last two at a
    quarter of the table.  ``l2f.SensorBank(device, list(suite(rows).values()))`` holds them."""
    rows = _rows(rows)
    quarter = rows // 4
    return {
        "none": none(rows),
        "constant_1": constant(rows, 1),
        "constant_2": constant(rows, 2),
        "constant_4": constant(rows, 4),
        "constant_8": constant(rows, 8),
        "jitter_0_3": jitter(rows, 0, 3, 0),
        "low_rate_4": low_rate(rows, 4),
        "dropout_8": dropout(rows, quarter, 8),
        "onset_4": onset(rows, quarter, 4),
    }


def check_table(table):
    """One ``[rows]`` table as the C layer takes it, or ValueError: uint8, [rows >= 1], every entry at most ``MAX_STEPS``."""
    if not isinstance(table, np.ndarray) or table.dtype != np.uint8:
        raise ValueError("a sensor table is a uint8 NumPy array [rows] (raptor_amd.sensors builds them)")
    if table.ndim != 1 or table.shape[0] < 1:
        raise ValueError(f"a sensor table has shape [rows >= 1]: the delay in steps; got {table.shape}")
    return np.ascontiguousarray(table)


def check_tables(tables):
    """The tables of a ``SensorBank`` as the C layer takes them, or ValueError: uint8 [M >= 1, rows >= 1], every entry at most
    ``MAX_STEPS``, contiguous; a list of M ``[rows]`` tables of equal length is stacked."""
    if isinstance(tables, (list, tuple)):
        if not tables:
            raise ValueError("a sensor bank holds at least one table")
        rows = [check_table(t) for t in tables]
        if len({t.shape[0] for t in rows}) != 1:
            raise ValueError("the tables of a sensor bank have the same number of rows; got " + ", ".join(str(t.shape[0]) for t in rows))
        tables = np.stack(rows)
    if not isinstance(tables, np.ndarray) or tables.dtype != np.uint8:
        raise ValueError("a sensor bank is a uint8 NumPy array [M, rows] or a list of M [rows] tables")
    if tables.ndim != 2 or tables.shape[0] < 1 or tables.shape[1] < 1:
        raise ValueError(f"a sensor bank has shape [M >= 1, rows >= 1]; got {tables.shape}")
    bad = np.argwhere(tables > MAX_STEPS)
    if bad.size:
        t, r = (int(x) for x in bad[0])
        raise ValueError(f"a sensor table holds a delay above {MAX_STEPS} steps: table {t}, row {r} ({int(tables[t, r])})")
    if tables.shape[0] * tables.shape[1] >= 1 << 28:
        raise ValueError("a sensor bank holds fewer than 2^28 rows in all")
    return np.ascontiguousarray(tables)


def check_sensor_ids(ids, n_tables, n_envs):
    """One table id per env, each in [0, n_tables) -> contiguous uint32; ValueError otherwise."""
    from . import schedules
    return schedules.check_ids(schedules.SENSOR, ids, n_tables, n_envs)


def delivered(readings, delay_of_step):
    """The observations the policy sees, as every kernel computes them: ``readings`` [K, ..., C >= 18] the observations assembled
    for ONE episode without the schedule (before any setpoint row is subtracted), index k its episode step count from 0;
    ``delay_of_step`` [K, ...] whole numbers, the table's row of every step -> [K, ..., C] of the readings' dtype with columns 0..17
    of step k those of step ``k - min(d, k)`` - an episode younger than the delay sees its first reading held - and the columns from
    18 on passed through.  A copy of bits: nothing is computed."""
    z = np.asarray(readings)
    d = np.asarray(delay_of_step)
    if z.ndim < 2 or z.shape[-1] < READING_COLUMNS or d.shape != z.shape[:-1]:
        raise ValueError(f"delivered takes readings [K, ..., C >= {READING_COLUMNS}] and a delay per step [K, ...]; got {z.shape} and {d.shape}")
    if d.dtype == bool or not np.issubdtype(d.dtype, np.integer) or (d.astype(np.int64) < 0).any():
        raise ValueError("a delay is a non-negative whole number of steps")
    k = np.arange(z.shape[0], dtype=np.int64).reshape((-1,) + (1,) * (d.ndim - 1))
    src = k - np.minimum(d.astype(np.int64), k)
    out = z.copy()
    head = z[..., :READING_COLUMNS]
    out[..., :READING_COLUMNS] = np.take_along_axis(head, np.broadcast_to(src[..., None], head.shape), axis=0)
    return out
