"""What the kinds of row tables share on the Python side: the wrench, vehicle, wind, delay and sensor schedules (``raptor_amd.disturbances``,
``raptor_amd.vehicles``, ``raptor_amd.winds``, ``raptor_amd.delays``, ``raptor_amd.sensors`` build their tables; ``l2f.WrenchBank`` / ``VehicleBank`` /
``WindBank`` / ``DelayBank`` / ``SensorBank`` hold them; ``env.set_*_schedule`` attaches them) and the moving setpoints of ``l2f.Reference`` / ``ReferenceBank``.  A kind is one ``Kind``
record; the checks of tables and ids, the banks and the env's attach / clear / property are written once and driven by it.  What a
row means is each builder module's ``compose``."""
from typing import Callable, NamedTuple, Optional

import numpy as np

from .vehicles import VEHICLE_NAMES
from .winds import DRAG, WIND_NAMES


def _finite(kind, tables):
    """Every entry finite; the entry is not named."""
    if not np.isfinite(tables).all():
        return f"a {kind.noun} table holds finite entries only"


def _positive_factors(kind, tables):
    bad = np.argwhere(~(np.isfinite(tables) & (tables > 0)))
    if bad.size:
        t, r, c = (int(x) for x in bad[0])
        return f"a {kind.noun} table holds positive finite factors only: table {t}, row {r}, column {c} ({kind.names[c]})"


def _finite_drag_not_negative(kind, tables):
    bad = np.argwhere(~np.isfinite(tables))
    if bad.size:
        t, r, c = (int(x) for x in bad[0])
        return f"a {kind.noun} table holds a non-finite entry: table {t}, row {r}, column {c} ({kind.names[c]})"
    bad = np.argwhere(tables[:, :, DRAG] < 0)
    if bad.size:
        t, r = (int(x) for x in bad[0])
        return f"a {kind.noun} table holds a negative drag: table {t}, row {r}, column {DRAG} ({kind.names[DRAG]})"


class Kind(NamedTuple):
    noun: str                   # "wrench": the bank class, the env's methods and the C entry points are named after it
    cols: int
    columns: str                # what the columns are, as the shape message lists them
    names: Optional[tuple]      # one name per column, for the rules that name an entry's column
    builder: str                # the module that builds such tables
    rule: Callable              # (kind, tables [M, rows, cols]) -> the message of the first bad entry, or None
    # ``<noun>_ids`` of ``PolicyBank.evaluate`` / ``TeacherBank.closed_loop``: what they group the tracking error by, and the
    # sentence that refuses them beside the ids of a kind before this one
    scenario: str = ""
    beside: str = ""


WRENCH = Kind("wrench", 6, "force, torque", None, "raptor_amd.disturbances", _finite, "disturbance")
VEHICLE = Kind("vehicle", 4, ", ".join(VEHICLE_NAMES), VEHICLE_NAMES, "raptor_amd.vehicles", _positive_factors, "vehicle",
               "vehicle_ids group the tracking error by vehicle scenario and wrench_ids by disturbance: give one of them")
WIND = Kind("wind", 4, ", ".join(WIND_NAMES), WIND_NAMES, "raptor_amd.winds", _finite_drag_not_negative, "wind",
            "wind_ids group the tracking error by wind scenario, wrench_ids by disturbance and vehicle_ids by vehicle scenario: "
            "give one of them")
# (a delay table is [rows] bytes, not [rows, cols] floats: raptor_amd.delays checks its tables itself; ids and the env's methods are
# the kind's)
DELAY = Kind("delay", 1, "delay in steps", None, "raptor_amd.delays", _finite, "latency",
             "delay_ids group the tracking error by latency scenario, wrench_ids by disturbance, vehicle_ids by vehicle scenario and "
             "wind_ids by wind scenario: give one of them")
# (a sensor table likewise: raptor_amd.sensors)
SENSOR = Kind("sensor", 1, "delay in steps", None, "raptor_amd.sensors", _finite, "sensor",
              "sensor_ids group the tracking error by sensor scenario, wrench_ids by disturbance, vehicle_ids by vehicle scenario, "
              "wind_ids by wind scenario and delay_ids by latency scenario: give one of them")
REFERENCE = Kind("reference", 6, "target position, target velocity", None, "raptor_amd.tracking", _finite)
KINDS = (WRENCH, VEHICLE, WIND, DELAY, SENSOR)       # the schedules, in the order the C layer walks them


def check_table(kind, table, entries=True):
    """One ``[rows, cols]`` table as the C layer takes it, or ValueError: float32, C-contiguous, [rows >= 1, cols]; ``entries``:
    checked by the kind's rule too."""
    if not isinstance(table, np.ndarray) or table.dtype != np.float32:
        raise ValueError(f"a {kind.noun} table is a float32 NumPy array [rows, {kind.cols}] ({kind.builder} builds them)")
    if table.ndim != 2 or table.shape[1] != kind.cols or table.shape[0] < 1:
        raise ValueError(f"a {kind.noun} table has shape [rows >= 1, {kind.cols}]: {kind.columns}; got {table.shape}")
    bad = kind.rule(kind, table[None]) if entries else None
    if bad:
        raise ValueError(bad)
    return np.ascontiguousarray(table)


def check_tables(kind, tables):
    """The tables of a bank as the C layer takes them, or ValueError: float32 [M >= 1, rows >= 1, cols], every entry as the kind's
    rule has it, contiguous; a list of M ``[rows, cols]`` tables of equal length is stacked."""
    if isinstance(tables, (list, tuple)):
        if not tables:
            raise ValueError(f"a {kind.noun} bank holds at least one table")
        # (a rule that names no entry is checked table by table; one that names table, row and column, on the stack below)
        rows = [check_table(kind, t, entries=kind.names is None) for t in tables]
        if len({t.shape[0] for t in rows}) != 1:
            raise ValueError(f"the tables of a {kind.noun} bank have the same number of rows; got " + ", ".join(str(t.shape[0]) for t in rows))
        tables = np.stack(rows)
    if not isinstance(tables, np.ndarray) or tables.dtype != np.float32:
        raise ValueError(f"a {kind.noun} bank is a float32 NumPy array [M, rows, {kind.cols}] or a list of M [rows, {kind.cols}] tables")
    if tables.ndim != 3 or tables.shape[2] != kind.cols or tables.shape[0] < 1 or tables.shape[1] < 1:
        raise ValueError(f"a {kind.noun} bank has shape [M >= 1, rows >= 1, {kind.cols}]; got {tables.shape}")
    bad = kind.rule(kind, tables)
    if bad:
        raise ValueError(bad)
    if tables.shape[0] * tables.shape[1] >= 1 << 28:
        raise ValueError(f"a {kind.noun} bank holds fewer than 2^28 rows in all")
    return np.ascontiguousarray(tables)


def check_ids(kind, ids, n_tables, n_envs):
    """One table id per env, each in [0, n_tables) -> contiguous uint32; ValueError otherwise."""
    a = np.asarray(ids)
    if a.ndim != 1 or a.size != int(n_envs):
        raise ValueError(f"{kind.noun} ids must hold one id per env: {a.size if a.ndim == 1 else a.shape} ids for {int(n_envs)} envs")
    if a.dtype == bool or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{kind.noun} ids must be integers")
    a = a.astype(np.int64)
    bad = np.flatnonzero((a < 0) | (a >= int(n_tables)))
    if bad.size:
        raise ValueError(f"{kind.noun} id out of range: env {int(bad[0])} names table {int(a[bad[0]])} of a bank of {int(n_tables)}")
    return np.ascontiguousarray(a.astype(np.uint32))


class ScheduleIds(NamedTuple):
    """The ids a closed-loop evaluation was given for the env's schedule of ``kind``: ``bank`` the attached bank, ``ids`` uint32."""
    kind: Kind
    bank: object
    ids: np.ndarray

    def attach(self, env):
        getattr(env, f"set_{self.kind.noun}_schedule")(self.bank, self.ids)


def checked_schedule_ids(env, given, ref_ids, n_envs):
    """What the ``wrench_ids`` / ``vehicle_ids`` / ``wind_ids`` / ``delay_ids`` / ``sensor_ids`` of ``PolicyBank.evaluate`` / ``TeacherBank.closed_loop`` must be,
    before any library call.  ``given``: ``{kind: ids or None}`` of the kinds the caller takes, in the order of ``KINDS`` ->
    ``ScheduleIds`` of the one that was given, or None (none was); ValueError otherwise."""
    found = None
    for kind, ids in given.items():
        if ids is None:
            continue
        name = f"{kind.noun}_ids"
        schedule = getattr(env, f"{kind.noun}_schedule", None)
        if schedule is None:
            raise ValueError(f"{name} name tables of the env's {kind.noun} schedule: attach one first (env.set_{kind.noun}_schedule(bank))")
        if found is not None:
            raise ValueError(kind.beside)
        if ref_ids is not None:
            raise ValueError(f"{name} group the tracking error by {kind.scenario} scenario and reference_ids by setpoint: give one of them "
                             f"(a single l2f.Reference goes with {name})")
        found = ScheduleIds(kind, schedule[0], check_ids(kind, ids, schedule[0].n_tables, n_envs))
    return found
