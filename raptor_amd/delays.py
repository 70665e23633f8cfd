"""Delay schedules: the tables ``l2f.DelayBank(device, tables)`` holds and ``env.set_delay_schedule(bank, ids)`` attaches.

A table is ``[rows]`` uint8: the control latency in steps, ``0 <= d <= MAX_STEPS``.  Row k holds for the transition an env takes at
episode step count k: the transition is computed from the command the actor gave d steps earlier, ``u_k = a_{k-d}``, or from four
zeros where the episode is younger than the delay (the zero ``sample_initial_state`` leaves in the action history).  The next state's
last-action columns keep the actor's own command: a controller sees what it sent, not what arrived, and so do recordings, relabelling
and distillation.  The wrench, vehicle and wind schedules change the force and the plant; this one changes the loop.  Ids are dealt
with ``tracking.spread_reference_ids`` and the ``[P, M]`` table comes from ``tracking.reference_tracking_table``, as for the other
schedules.  ``applied`` is the definition every kernel computes (include/raptor_quad.h "Delay schedule"), in NumPy."""
import numpy as np

MAX_STEPS = 16                                # RQ_DELAY_MAX_STEPS: 160 ms at dt = 10 ms, 40 ms at 2.5 ms


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
        raise ValueError(f"{seconds} s at dt = {dt} s are {d} steps: a delay schedule holds at most {MAX_STEPS}")
    return d


def none(rows):
    """No latency: zeros (the unscheduled transition, bit for bit)."""
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


def dropout(rows, start, length):
    """A link that drops ``length`` commands from step ``start`` on and holds the last one it got: d = 0 before, then 0, 1, 2, ...,
    ``length`` (the command of step ``start`` acts on), then back to 0."""
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
    """A small named suite of latency scenarios, every table ``[rows]`` uint8: none, constant delays of 1, 2, 4 and 8 steps, a jitter
    of 0 .. 3 steps, a dropout of 8 commands and an onset of 4 steps, the last two at a quarter of the table.
    ``l2f.DelayBank(device, list(suite(rows).values()))`` holds them."""
    rows = _rows(rows)
    quarter = rows // 4
    return {
        "none": none(rows),
        "constant_1": constant(rows, 1),
        "constant_2": constant(rows, 2),
        "constant_4": constant(rows, 4),
        "constant_8": constant(rows, 8),
        "jitter_0_3": jitter(rows, 0, 3, 0),
        "dropout_8": dropout(rows, quarter, 8),
        "onset_4": onset(rows, quarter, 4),
    }


def check_table(table):
    """One ``[rows]`` table as the C layer takes it, or ValueError: uint8, [rows >= 1], every entry at most ``MAX_STEPS``."""
    if not isinstance(table, np.ndarray) or table.dtype != np.uint8:
        raise ValueError("a delay table is a uint8 NumPy array [rows] (raptor_amd.delays builds them)")
    if table.ndim != 1 or table.shape[0] < 1:
        raise ValueError(f"a delay table has shape [rows >= 1]: the delay in steps; got {table.shape}")
    return np.ascontiguousarray(table)


def check_tables(tables):
    """The tables of a ``DelayBank`` as the C layer takes them, or ValueError: uint8 [M >= 1, rows >= 1], every entry at most
    ``MAX_STEPS``, contiguous; a list of M ``[rows]`` tables of equal length is stacked."""
    if isinstance(tables, (list, tuple)):
        if not tables:
            raise ValueError("a delay bank holds at least one table")
        rows = [check_table(t) for t in tables]
        if len({t.shape[0] for t in rows}) != 1:
            raise ValueError("the tables of a delay bank have the same number of rows; got " + ", ".join(str(t.shape[0]) for t in rows))
        tables = np.stack(rows)
    if not isinstance(tables, np.ndarray) or tables.dtype != np.uint8:
        raise ValueError("a delay bank is a uint8 NumPy array [M, rows] or a list of M [rows] tables")
    if tables.ndim != 2 or tables.shape[0] < 1 or tables.shape[1] < 1:
        raise ValueError(f"a delay bank has shape [M >= 1, rows >= 1]; got {tables.shape}")
    bad = np.argwhere(tables > MAX_STEPS)
    if bad.size:
        t, r = (int(x) for x in bad[0])
        raise ValueError(f"a delay table holds a delay above {MAX_STEPS} steps: table {t}, row {r} ({int(tables[t, r])})")
    if tables.shape[0] * tables.shape[1] >= 1 << 28:
        raise ValueError("a delay bank holds fewer than 2^28 rows in all")
    return np.ascontiguousarray(tables)


def check_delay_ids(ids, n_tables, n_envs):
    """One table id per env, each in [0, n_tables) -> contiguous uint32; ValueError otherwise."""
    from . import schedules
    return schedules.check_ids(schedules.DELAY, ids, n_tables, n_envs)


def applied(actions, delay_of_step):
    """The commands that act, as every kernel computes them: ``actions`` [K, ..., 4] the actor's commands of ONE episode, index k
    its episode step count from 0; ``delay_of_step`` [K, ...] whole numbers, the table's row of every step -> u [K, ..., 4] of the
    actions' dtype with u[k] = actions[k - d] where d <= k and +0.0 where the episode is younger than the delay.  A copy of bits:
    nothing is computed."""
    a = np.asarray(actions)
    d = np.asarray(delay_of_step)
    if a.ndim < 2 or a.shape[-1] != 4 or d.shape != a.shape[:-1]:
        raise ValueError(f"applied takes actions [K, ..., 4] and a delay per step [K, ...]; got {a.shape} and {d.shape}")
    if d.dtype == bool or not np.issubdtype(d.dtype, np.integer) or (d.astype(np.int64) < 0).any():
        raise ValueError("a delay is a non-negative whole number of steps")
    k = np.arange(a.shape[0], dtype=np.int64).reshape((-1,) + (1,) * (d.ndim - 1))
    src = k - d.astype(np.int64)
    reaches = src >= 0
    u = np.take_along_axis(a, np.broadcast_to(np.where(reaches, src, 0)[..., None], a.shape), axis=0)
    return np.where(reaches[..., None], u, np.zeros((), a.dtype))


def applied_actions(traj, tables, ids=None, start_steps=None):
    """What the rotors got in a recording: ``traj`` the dict of ``Trajectory.numpy()`` (``act`` [T, N, 4] the actor's own commands,
    ``done`` [T, N]), ``tables`` [M, rows] (or one [rows] table) and ``ids`` [N] what ``env.set_delay_schedule`` was given,
    ``start_steps`` [N] what ``env.episode_steps()`` answered right before the rollout (None: 0) -> u [T, N, 4] float32, rebuilt on
    the host along ``probing.episode_steps``: the command of d steps earlier in the same episode, zeros where the episode is younger
    than the delay and on frozen steps, NaN where the command was given before the recording began."""
    from .probing import episode_steps
    act = np.asarray(traj["act"], np.float32)
    tab = np.asarray(tables)
    if tab.ndim == 1:
        tab = tab[None]
    T, N = act.shape[:2]
    which = np.zeros(N, np.int64) if ids is None else np.asarray(ids).astype(np.int64)
    k = episode_steps(traj["done"], start_steps)                     # [T, N], -1 on a frozen step
    live = k >= 0
    d = tab[which[None, :], np.clip(k, 0, tab.shape[1] - 1)].astype(np.int64)
    reaches = live & (d <= k)
    src = np.arange(T, dtype=np.int64)[:, None] - d                    # a live episode's steps stand one after another in a recording
    u = np.take_along_axis(act, np.broadcast_to(np.clip(src, 0, T - 1)[..., None], act.shape), axis=0)
    u = np.where(reaches[..., None], u, np.float32(0.0))
    u[reaches & (src < 0)] = np.nan
    return u
