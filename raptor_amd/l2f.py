"""Drop-in for the ``l2f`` Python surface used by the rollout loop of rl-tools/raptor.

The names, argument order and in-place semantics follow /root/reference/README.md:41-101:

    import raptor_amd.l2f as l2f
    from raptor_amd.l2f import vector8 as vector      # or: vector = l2f.vector(65536)
    device = l2f.Device(); rng = vector.VectorRng(); env = vector.VectorEnvironment()
    params = vector.VectorParameters(); state = vector.VectorState(); next_state = vector.VectorState()
    observation = np.zeros((env.N_ENVIRONMENTS, env.OBSERVATION_DIM), dtype=np.float32)
    vector.initialize_rng(device, rng, 0)
    vector.initialize_environment(device, env)
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    vector.observe(device, env, params, state, observation, rng)
    dts = vector.step(device, env, params, state, action, next_state, rng)
    state.assign(next_state)

Differences that are deliberate (DESIGN.md "Boundary"):
  * the batch size is a runtime value: ``l2f.vector(N)`` builds the module-like object the
    reference pre-compiles as ``vector1 ... vectorN``; ``vector8`` is ``vector(8)``;
  * passing ``None`` for ``observation`` / ``action`` keeps the data in HBM (zero PCIe
    traffic); ``vector.rollout`` runs the whole loop body on the device;
  * everything executes on an MI355X through libraptor_quad.so — no CPU path exists here.

The UI / JSON message helpers of l2f (``set_ui_message``, ``set_parameters_message``,
``set_state_action_message``, README.md:63-92) are emitted by the host side here (plain JSON from device
snapshots); their schema beyond ``namespace`` / ``channel`` / ``data[i]`` is not in the reference tree
[UPSTREAM-UNVERIFIED], see the functions.
"""
import ctypes as C
import json
import weakref

import numpy as np

from . import _lib, schedules
from ._lib import (ACTION_DIM, OBSERVATION_DIM, PARAM_DIM, STATE_DIM, ROLLOUT_AUTORESET, ROLLOUT_CHAINED,
                   ROLLOUT_FUSED, EnvConfig, RaptorQuadError)

__all__ = ["Device", "Reference", "WrenchBank", "VehicleBank", "WindBank", "DelayBank", "SensorBank", "UI", "vector", "vector8", "EnvConfig", "RaptorQuadError"]


class UI:
    """``l2f.UI()`` (README.md:52): carries the namespace the ui-server hands out in its handshake
    (``ui.ns = handshake["data"]["namespace"]``, README.md:82-85)."""

    def __init__(self, ns=""):
        self.ns = ns


class Device:
    """``l2f.Device()`` (README.md:49): one HIP device + one stream."""

    def __init__(self, ordinal=0):
        h = C.c_void_p()
        _lib.call("rq_device_create", int(ordinal), C.byref(h))
        self._h = h
        self.ordinal = int(ordinal)
        self._fin = weakref.finalize(self, _lib.load().rq_device_destroy, h)

    def synchronize(self):
        _lib.call("rq_device_synchronize", self._h)

    def timer_start(self):
        """HIP-event stopwatch on this device's stream."""
        _lib.call("rq_device_timer_start", self._h)

    def timer_stop(self):
        ms = C.c_float()
        _lib.call("rq_device_timer_stop", self._h, C.byref(ms))
        return float(ms.value)

    def set_rollout_timing(self, enable):
        """Kernel-level timing of fused rollouts: every wave records the wall-clock ticks at which it came in and went out."""
        _lib.call("rq_device_set_rollout_timing", self._h, 1 if enable else 0)

    def last_rollout_ms(self):
        """Duration (ms) of the most recent fused rollout kernel launched while ``set_rollout_timing(True)``."""
        ms = C.c_float()
        _lib.call("rq_device_last_rollout_ms", self._h, C.byref(ms))
        return float(ms.value)

    def last_rollout_waves(self):
        """(t_in, t_out, xcd, t_first_step, t_last_step_done) per wave of the most recent timed fused rollout; 100 MHz
        ticks, comparable within a die."""
        n = C.c_uint32()
        _lib.call("rq_device_last_rollout_waves", self._h, None, 0, C.byref(n))
        rec = np.zeros((n.value, 4), np.uint64)
        _lib.call("rq_device_last_rollout_waves", self._h, rec.ctypes.data, n.value, C.byref(n))
        mask = np.uint64(0x0FFFFFFFFFFFFFFF)
        return (rec[:, 0] & mask, rec[:, 1] & mask, (rec[:, 1] >> np.uint64(60)).astype(np.int64) & 7,
                rec[:, 2] & mask, rec[:, 3] & mask)

    def last_rollout_clock_ghz(self):
        """Core clock (GHz) the most recent timed fused rollout ran its steps at (median wave: shader-clock cycles over
        constant-rate ticks between its first step's start and its last step's end)."""
        ghz = C.c_float()
        _lib.call("rq_device_last_rollout_clock", self._h, C.byref(ghz))
        return float(ghz.value)

    def launch_floor(self, n, reps=200):
        """Average us per launch of back-to-back near-empty kernels on an n-thread grid (diagnostic)."""
        us = C.c_float()
        _lib.call("rq_device_launch_floor", self._h, int(n), int(reps), C.byref(us))
        return float(us.value)

    def set_speculation(self, enable):
        """The small-batch loop's speculative policy step (rq_device_set_speculation, include/raptor_quad.h): off / on
        for this device.  Left on, the device suspends it by itself after four speculated steps in a row nobody took."""
        _lib.call("rq_device_set_speculation", self._h, 1 if enable else 0)

    def speculation(self):
        """-> {"enabled", "suspended", "consecutive_misses"}"""
        e, s, m = C.c_int(), C.c_int(), C.c_uint32()
        _lib.call("rq_device_get_speculation", self._h, C.byref(e), C.byref(s), C.byref(m))
        return {"enabled": bool(e.value), "suspended": bool(s.value), "consecutive_misses": int(m.value)}

    def set_resident(self, enable):
        """The small-batch loop's resident executor (rq_device_set_resident, include/raptor_quad.h): off / on for this device."""
        _lib.call("rq_device_set_resident", self._h, 1 if enable else 0)

    def resident(self):
        """-> {"enabled", "running", "starts", "commands", "replays"}: is a resident kernel on the device now; kernels started,
        commands posted to them, commands replayed as launches since the device was created."""
        e, r = C.c_int(), C.c_int()
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _lib.call("rq_device_get_resident", self._h, C.byref(e), C.byref(r), C.byref(a), C.byref(b), C.byref(c))
        return {"enabled": bool(e.value), "running": bool(r.value), "starts": int(a.value), "commands": int(b.value), "replays": int(c.value)}

    def resident_timing_us(self):
        """Device-side timeline of the last command the resident kernel finished, in microseconds from the moment it saw the command:
        {"rows_read", "stepped", "first_flag", "acted", "done"} (rq_device_get_resident_timing)."""
        t = (C.c_uint64 * 6)()
        _lib.call("rq_device_get_resident_timing", self._h, t)
        return {k: (int(t[i + 1]) - int(t[0])) / 100.0 for i, k in enumerate(("rows_read", "stepped", "first_flag", "acted", "done"))}

    @property
    def stream(self):
        s = C.c_void_p()
        _lib.call("rq_device_stream", self._h, C.byref(s))
        return s.value

    @staticmethod
    def count():
        n = C.c_int()
        lib = _lib.load()
        lib.rq_device_count(C.byref(n))
        return n.value


class Reference:
    """A moving setpoint for ``vector.rollout(..., reference=ref)``: ``table`` [rows, 6] float32, columns 0..2 the target position and
    3..5 the target linear velocity in the world frame (``raptor_amd.tracking.lissajous`` / ``hold``).  An env reads the row of its
    own episode step count, so ``rows`` must cover ``episode_step_limit``.  The table is copied to ``device`` once, here."""

    def __init__(self, device, table):
        t = schedules.check_table(schedules.REFERENCE, table)    # refused before the device is touched
        h = C.c_void_p()
        _lib.call("rq_reference_create", device._h, _lib.fptr(t), int(t.shape[0]), C.byref(h))
        self._h = h
        self._device = device
        self.rows = int(t.shape[0])
        self._fin = weakref.finalize(self, _lib.load().rq_reference_destroy, h)


class ReferenceBank:
    """M moving setpoints of the same length for ``vector.rollout(..., reference=bank, reference_ids=ids)`` and
    ``PolicyBank.fly(..., reference=bank, reference_ids=ids)``: ``tables`` float32 [M, rows, 6] (or a list of M [rows, 6] tables),
    columns as in ``Reference``.  Env i flies table ``ids[i]`` - ids are free per env - and computes, bit for bit, what it computes
    with ``Reference(tables[ids[i]])``.  The tables are copied to ``device`` once, here (``raptor_amd.tracking.suite`` makes some)."""

    def __init__(self, device, tables):
        t = schedules.check_tables(schedules.REFERENCE, tables)      # refused before the device is touched
        h = C.c_void_p()
        _lib.call("rq_reference_bank_create", device._h, _lib.fptr(t), int(t.shape[0]), int(t.shape[1]), C.byref(h))
        self._h = h
        self._device = device
        self.n_references = int(t.shape[0])
        self.rows = int(t.shape[1])
        self._fin = weakref.finalize(self, _lib.load().rq_reference_bank_destroy, h)


class _ScheduleBank:
    """M tables of one kind of schedule on ``device``: checked (``schedules.check_tables``), copied once, destroyed with the object.
    A subclass names its ``_kind`` and may add arguments to the library's create call (``_create_arguments``)."""
    _kind = None

    def __init__(self, device, tables):
        t = schedules.check_tables(self._kind, tables)          # refused before the device is touched
        extra = self._create_arguments()
        h = C.c_void_p()
        _lib.call(f"rq_{self._kind.noun}_bank_create", device._h, _lib.fptr(t), int(t.shape[0]), int(t.shape[1]), *extra, C.byref(h))
        self._h = h
        self._device = device
        self.n_tables = int(t.shape[0])
        self.rows = int(t.shape[1])
        # (the library refuses to destroy a bank that is still attached to a live env; the envs hold their bank, so it outlives them)
        self._fin = weakref.finalize(self, getattr(_lib.load(), f"rq_{self._kind.noun}_bank_destroy"), h)

    def _create_arguments(self):
        return ()


class WrenchBank(_ScheduleBank):
    """M wrench tables of the same length for ``env.set_wrench_schedule(bank, ids)``: ``tables`` float32 [M, rows, 6] (or a list of M
    [rows, 6] tables; ``raptor_amd.disturbances`` builds them), columns 0..2 a force in the world frame and 3..5 a torque in the body
    frame.  ``units``: "relative" (multiples of m g and of m g arm, the default) or "absolute" (N and N m).  While the bank is
    attached to an env, every transition of env i adds the row of its own episode step count of table ``ids[i]`` to the per-episode
    disturbance (include/raptor_quad.h "Wrench schedule").  The tables are copied to ``device`` once, here."""
    _kind = schedules.WRENCH

    def __init__(self, device, tables, units="relative"):
        self.units = units
        super().__init__(device, tables)

    def _create_arguments(self):
        from .disturbances import check_units
        return (check_units(self.units),)


class VehicleBank(_ScheduleBank):
    """M vehicle tables of the same length for ``env.set_vehicle_schedule(bank, ids)``: ``tables`` float32 [M, rows, 4] (or a list of
    M [rows, 4] tables; ``raptor_amd.vehicles`` builds them), positive factors on the mass, the inertia, the thrust curve and the
    motor time constant.  While the bank is attached to an env, every transition of env i is computed from its parameters times
    the row of its own episode step count of table ``ids[i]`` (include/raptor_quad.h "Vehicle schedule").  The tables are copied
    to ``device`` once, here."""
    _kind = schedules.VEHICLE


class WindBank(_ScheduleBank):
    """M wind tables of the same length for ``env.set_wind_schedule(bank, ids)``: ``tables`` float32 [M, rows, 4] (or a list of M
    [rows, 4] tables; ``raptor_amd.winds`` builds them), the air velocity in the world frame (m/s) and the specific drag (1/s).
    While the bank is attached to an env, every transition of env i is computed with the linear drag against the air of the row of
    its own episode step count of table ``ids[i]`` (include/raptor_quad.h "Wind schedule").  The tables are copied to ``device``
    once, here."""
    _kind = schedules.WIND


class DelayBank(_ScheduleBank):
    """M delay tables of the same length for ``env.set_delay_schedule(bank, ids)``: ``tables`` uint8 [M, rows] (or a list of M [rows]
    tables; ``raptor_amd.delays`` builds them), the control latency in steps, at most ``delays.MAX_STEPS``.  While the bank is
    attached to an env, every transition of env i is computed from the command its actor gave as many steps ago as the row of its
    own episode step count of table ``ids[i]`` says (include/raptor_quad.h "Delay schedule").  The tables are copied to ``device``
    once, here."""
    _kind = schedules.DELAY

    def __init__(self, device, tables):
        from . import delays
        t = delays.check_tables(tables)                          # refused before the device is touched
        h = C.c_void_p()
        _lib.call("rq_delay_bank_create", device._h, t.ctypes.data, int(t.shape[0]), int(t.shape[1]), C.byref(h))
        self._h = h
        self._device = device
        self.n_tables = int(t.shape[0])
        self.rows = int(t.shape[1])
        self._fin = weakref.finalize(self, _lib.load().rq_delay_bank_destroy, h)


class SensorBank(_ScheduleBank):
    """M sensor tables of the same length for ``env.set_sensor_schedule(bank, ids)``: ``tables`` uint8 [M, rows] (or a list of M
    [rows] tables; ``raptor_amd.sensors`` builds them), the observation latency in steps, at most ``sensors.MAX_STEPS``.  While the
    bank is attached to an env, every observation assembled for env i carries in columns 0..17 the reading taken as many steps ago as
    the row of its own episode step count of table ``ids[i]`` says, the first reading of the episode where it is younger
    (include/raptor_quad.h "Sensor schedule").  The tables are copied to ``device`` once, here."""
    _kind = schedules.SENSOR

    def __init__(self, device, tables):
        from . import sensors
        t = sensors.check_tables(tables)                         # refused before the device is touched
        h = C.c_void_p()
        _lib.call("rq_sensor_bank_create", device._h, t.ctypes.data, int(t.shape[0]), int(t.shape[1]), C.byref(h))
        self._h = h
        self._device = device
        self.n_tables = int(t.shape[0])
        self.rows = int(t.shape[1])
        self._fin = weakref.finalize(self, _lib.load().rq_sensor_bank_destroy, h)


_BANKS = {schedules.WRENCH: WrenchBank, schedules.VEHICLE: VehicleBank, schedules.WIND: WindBank, schedules.DELAY: DelayBank,
          schedules.SENSOR: SensorBank}


def _checked_reference(reference, reference_ids, n_envs):
    """What a rollout's ``reference`` / ``reference_ids`` pair must be, before any library call -> the ids as uint32 (a
    ``ReferenceBank``) or None (a ``Reference``, or no reference); ValueError otherwise."""
    if isinstance(reference, ReferenceBank):
        if reference_ids is None:
            raise ValueError("a ReferenceBank flies the envs by reference_ids: one reference id per env is required")
        from .tracking import check_reference_ids
        return check_reference_ids(reference_ids, reference.n_references, n_envs)
    if reference_ids is not None:
        raise ValueError("reference_ids belong to a ReferenceBank: a Reference is every env's table")
    if reference is not None and not isinstance(reference, Reference):
        raise ValueError("reference must be an l2f.Reference or an l2f.ReferenceBank")
    return None


_MODES = {"fused": ROLLOUT_FUSED, "chained": ROLLOUT_CHAINED}


def _rollout_call(entry, device, env, params, state, actor_handle, ids, rng, n_steps, mode, autoreset, trajectory, reference, ref_ids):
    """The one library call of every rollout.  ``entry``: "rq_rollout" (``ids`` None), "rq_rollout_policies" or
    "rq_rollout_teachers" (``ids``: the actor's id per env); ``mode``: ``_MODES[...]``; ``reference`` / ``ref_ids`` as ``_checked_reference`` left them pick the
    entry point itself, its ``_track`` or its ``_track_refs`` twin.  The untracked single-policy call has two names: with a
    ``trajectory`` it is ``rq_rollout_record``."""
    args = (device._h, env._require("environment"), params._require("VectorParameters"), state._require("VectorState"), actor_handle)
    if ids is not None:
        args += (ids.ctypes.data,)
    args += (rng._require("rng"), int(n_steps), mode, ROLLOUT_AUTORESET if autoreset else 0)
    traj = trajectory._require("trajectory") if trajectory is not None else None
    if reference is not None:
        args += (traj, reference._h)
        if ref_ids is None:
            return _lib.call(entry + "_track", *args)
        return _lib.call(entry + "_track_refs", *args, ref_ids.ctypes.data)
    if entry != "rq_rollout":
        return _lib.call(entry, *args, traj)
    if traj is None:
        return _lib.call(entry, *args)
    return _lib.call("rq_rollout_record", *args, traj)


def tracking_rmse(env, reference, ref_ids, schedule_ids, actor_ids, n_actors):
    """``tracking_rmse`` of a bank's closed-loop table, from ``env.tracking_error()`` grouped by actor (policy or teacher): [n_actors,
    M] over the scenarios of a schedule (``schedule_ids``: what ``schedules.checked_schedule_ids`` answered - disturbances, vehicles, winds, latencies or sensors)
    or the setpoints (``ref_ids`` of a ``ReferenceBank``), [n_actors] on a single ``Reference``."""
    from .tracking import reference_tracking_table
    sum_sq, steps = env.tracking_error()
    if schedule_ids is not None:
        return reference_tracking_table(sum_sq, steps, schedule_ids.ids, schedule_ids.bank.n_tables, actor_ids, n_actors)
    if ref_ids is not None:
        return reference_tracking_table(sum_sq, steps, ref_ids, reference.n_references, actor_ids, n_actors)
    from .policy_bank import policy_tracking_table
    return policy_tracking_table(sum_sq, steps, actor_ids, n_actors)


class _Handle:
    """Lazily created C object (the reference's constructors take no device argument)."""
    _destroy = None

    def __init__(self):
        self._h = None
        self._fin = None

    def _adopt(self, h):
        self._h = h
        self._fin = weakref.finalize(self, getattr(_lib.load(), self._destroy), h)

    def _require(self, what):
        if self._h is None:
            raise RaptorQuadError(-6, f"{what} is not initialised yet")
        return self._h


class _DeviceArray:
    """A device buffer of the engine described by ``__cuda_array_interface__`` (version 3): PyTorch (and CuPy,
    Numba) wrap it WITHOUT a copy - ``torch.as_tensor(x, device="cuda")`` - so a learner reads rollouts where
    the engine wrote them.  ``owner`` keeps the C object alive as long as a tensor made from this exists."""

    def __init__(self, ptr, shape, typestr, owner):
        self._owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(int(d) for d in shape), "typestr": typestr,
                                         "data": (int(ptr), False), "version": 3, "strides": None}


def _ordinal_of(owner):
    """HIP device ordinal of the engine object a buffer belongs to (env, container or trajectory)."""
    for obj in (owner, getattr(owner, "_env", None)):
        dev = getattr(obj, "_device", None)
        if dev is not None:
            return dev.ordinal
    raise RaptorQuadError(-6, "the object is not bound to a device yet")


def _as_torch(ptr, shape, typestr, owner):
    """Zero-copy torch view of an engine buffer ON THE ENGINE'S DEVICE (not torch's current one: as_tensor with a
    bare "cuda" would silently copy to the current device and the view would be a detached copy)."""
    import torch
    t = torch.as_tensor(_DeviceArray(ptr, shape, typestr, owner), device=f"cuda:{_ordinal_of(owner)}")
    if t.data_ptr() != int(ptr):
        raise RaptorQuadError(-3, "torch copied the buffer instead of wrapping it (device mismatch)")
    return t


class _StateView:
    """One element of ``VectorState.states`` (README.md:73-75): a host-side snapshot."""
    __slots__ = ("_row",)

    def __init__(self, row):
        self._row = row

    position = property(lambda s: s._row[0:3])
    orientation = property(lambda s: s._row[3:7])
    linear_velocity = property(lambda s: s._row[7:10])
    angular_velocity = property(lambda s: s._row[10:13])
    rpm = property(lambda s: s._row[13:17])
    last_action = property(lambda s: s._row[17:21])
    force = property(lambda s: s._row[21:24])
    torque = property(lambda s: s._row[24:27])


class VectorModule:
    """What ``from l2f import vector8 as vector`` gives, for a runtime batch size.

    ``global_env_offset``: global id of env 0 when one logical batch is sharded over several
    devices/processes — the RNG is keyed by global id, so results do not depend on sharding.
    """

    def __init__(self, n_environments, global_env_offset=0):
        if n_environments <= 0:
            raise ValueError("n_environments must be positive")
        self.N_ENVIRONMENTS = int(n_environments)
        self.OBSERVATION_DIM = OBSERVATION_DIM
        self.ACTION_DIM = ACTION_DIM
        self.global_env_offset = int(global_env_offset)
        mod = self

        class VectorRng(_Handle):
            _destroy = "rq_rng_destroy"

            def _ensure(self, device):
                if self._h is None:
                    h = C.c_void_p()
                    _lib.call("rq_rng_create", device._h, C.byref(h))
                    self._adopt(h)
                    self._device = device
                return self._h

            @property
            def epoch(self):
                e = C.c_uint32()
                _lib.call("rq_rng_get", self._require("rng"), None, C.byref(e))
                return e.value

            @property
            def seed(self):
                s = C.c_uint64()
                _lib.call("rq_rng_get", self._require("rng"), C.byref(s), None)
                return s.value

        class VectorEnvironment(_Handle):
            _destroy = "rq_env_destroy"
            N_ENVIRONMENTS = mod.N_ENVIRONMENTS
            OBSERVATION_DIM = OBSERVATION_DIM
            ACTION_DIM = ACTION_DIM

            def _ensure(self, device):
                if self._h is None:
                    h = C.c_void_p()
                    _lib.call("rq_env_create", device._h, mod.N_ENVIRONMENTS, mod.global_env_offset, C.byref(h))
                    self._adopt(h)
                    self._device = device
                return self._h

            # --- configuration (the MDP constants initialize_environment fills) ---
            @property
            def config(self):
                cfg = _lib.env_config_type()()
                _lib.call("rq_env_get_config", self._require("environment"), C.byref(cfg))
                return cfg

            @config.setter
            def config(self, cfg):
                _lib.call("rq_env_set_config", self._require("environment"), C.byref(cfg))
                self._dt = None

            def _step_dt(self):
                """dt of the configuration in force (what ``step`` returns per env), asked of the library once per configuration."""
                dt = getattr(self, "_dt", None)
                if dt is None:
                    dt = self._dt = float(self.config.dt)
                return dt

            # --- device-resident observation / action buffers ---
            def observation(self):
                out = np.empty((mod.N_ENVIRONMENTS, OBSERVATION_DIM), np.float32)
                _lib.call("rq_env_get_observation", self._require("environment"), _lib.fptr(out))
                return out

            def action(self):
                out = np.empty((mod.N_ENVIRONMENTS, ACTION_DIM), np.float32)
                _lib.call("rq_env_get_action", self._require("environment"), _lib.fptr(out))
                return out

            def _ld(self):
                ld = C.c_uint32()
                _lib.call("rq_env_leading_dim", self._require("environment"), C.byref(ld))
                return ld.value

            def observation_tensor(self):
                """The env's device observation buffer as a torch tensor view, field-major [OBSERVATION_DIM, ld]
                (env i = column i < N_ENVIRONMENTS); zero copy.  Order your torch work behind the engine's stream
                (``device.synchronize()`` or an event on ``device.stream``)."""
                p = C.c_void_p()
                _lib.call("rq_env_observation_device_ptr", self._require("environment"), C.byref(p))
                return _as_torch(p.value, (OBSERVATION_DIM, self._ld()), "<f4", self)

            def action_tensor(self):
                """The env's device action buffer, field-major [4, ld]; zero copy (a learner may write it)."""
                p = C.c_void_p()
                _lib.call("rq_env_action_device_ptr", self._require("environment"), C.byref(p))
                return _as_torch(p.value, (ACTION_DIM, self._ld()), "<f4", self)

            def set_action(self, action):
                a = np.ascontiguousarray(action, np.float32)
                assert a.shape == (mod.N_ENVIRONMENTS, ACTION_DIM)
                _lib.call("rq_env_set_action", self._require("environment"), _lib.fptr(a))

            # --- episode statistics ---
            def _stat(self, fn, dtype, out=None, wait=True):
                h = self._require("environment")
                if out is not None:   # a torch tensor on the same HIP device; wait=False: only enqueued on
                    import torch                                                     # the engine's stream
                    want = {np.float32: torch.float32, np.uint32: torch.int32, np.uint8: torch.uint8}[dtype]
                    if (not out.is_cuda or out.device.index != self._device.ordinal or not out.is_contiguous() or
                            out.numel() != mod.N_ENVIRONMENTS or (out.dtype != want and not
                                                                 (dtype is np.uint32 and out.dtype == getattr(torch, "uint32", None)))):
                        raise ValueError(f"out must be a contiguous {want} tensor of {mod.N_ENVIRONMENTS} elements on "
                                         f"cuda:{self._device.ordinal}")
                    _lib.call(fn, h, C.c_void_p(out.data_ptr()), 1 if wait else 2)
                    return out
                a = np.empty(mod.N_ENVIRONMENTS, dtype)
                _lib.call(fn, h, a.ctypes.data, 0)
                return a

            def rewards(self, out=None): return self._stat("rq_env_get_rewards", np.float32, out)
            def terminated(self, out=None): return self._stat("rq_env_get_terminated", np.uint8, out)
            def done_codes(self, out=None): return self._stat("rq_env_get_done_codes", np.uint8, out)
            def frozen(self, out=None): return self._stat("rq_env_get_frozen", np.uint8, out)
            def episode_index(self, out=None): return self._stat("rq_env_get_episode_index", np.uint32, out)
            def returns(self, out=None): return self._stat("rq_env_get_returns", np.float32, out)
            def episode_steps(self, out=None): return self._stat("rq_env_get_episode_steps", np.uint32, out)
            def finished_returns(self, out=None, wait=True):
                return self._stat("rq_env_get_finished_returns", np.float32, out, wait)
            def finished_lengths(self, out=None): return self._stat("rq_env_get_finished_lengths", np.uint32, out)
            def finished_counts(self, out=None): return self._stat("rq_env_get_finished_counts", np.uint32, out)
            def finished_terminated(self, out=None): return self._stat("rq_env_get_finished_terminated", np.uint32, out)

            def reset_statistics(self):
                _lib.call("rq_env_reset_statistics", self._require("environment"))

            # --- the schedules: wrench (scheduled gusts, pokes, payloads: raptor_amd.disturbances), vehicle (payloads, battery sag,
            # slow motors: raptor_amd.vehicles), wind (air that moves and drags: raptor_amd.winds), delay (control latency:
            # raptor_amd.delays), sensor (observation latency: raptor_amd.sensors).  One implementation; what is attached of a kind is kept as (bank, ids) under _<noun>. ---
            _wrench = _vehicle = _wind = _delay = _sensor = None

            def _set_schedule(self, kind, bank, ids):
                if not isinstance(bank, _BANKS[kind]):
                    raise ValueError(f"bank must be an l2f.{_BANKS[kind].__name__} (clear_{kind.noun}_schedule() detaches)")
                a = (np.zeros(mod.N_ENVIRONMENTS, np.uint32) if ids is None
                     else schedules.check_ids(kind, ids, bank.n_tables, mod.N_ENVIRONMENTS))
                _lib.call(f"rq_env_set_{kind.noun}_schedule", self._require("environment"), bank._h, a.ctypes.data)
                setattr(self, "_" + kind.noun, (bank, a.copy()))

            def _clear_schedule(self, kind):
                if self._h is not None:
                    _lib.call(f"rq_env_set_{kind.noun}_schedule", self._h, None, None)
                setattr(self, "_" + kind.noun, None)

            def _schedule(self, kind):
                attached = getattr(self, "_" + kind.noun)
                return None if attached is None else (attached[0], attached[1].copy())

            def set_wrench_schedule(self, bank, ids=None):
                """Attach ``bank`` (an ``l2f.WrenchBank``): from now on every transition of env i, in every call that steps this
                env, is computed with the row of its episode step count of table ``ids[i]`` ([N] integers, free per env; None:
                table 0 for every env) added to its per-episode disturbance.  The tables must cover ``episode_step_limit``."""
                self._set_schedule(schedules.WRENCH, bank, ids)

            def set_vehicle_schedule(self, bank, ids=None):
                """Attach ``bank`` (an ``l2f.VehicleBank``): from now on every transition of env i, in every call that steps this
                env, is computed from its parameters times the row of its episode step count of table ``ids[i]`` ([N] integers,
                free per env; None: table 0 for every env).  The tables must cover ``episode_step_limit``."""
                self._set_schedule(schedules.VEHICLE, bank, ids)

            def set_wind_schedule(self, bank, ids=None):
                """Attach ``bank`` (an ``l2f.WindBank``): from now on every transition of env i, in every call that steps this env,
                is computed with the drag against the air of the row of its episode step count of table ``ids[i]`` ([N] integers,
                free per env; None: table 0 for every env).  The tables must cover ``episode_step_limit``."""
                self._set_schedule(schedules.WIND, bank, ids)

            def set_delay_schedule(self, bank, ids=None):
                """Attach ``bank`` (an ``l2f.DelayBank``): from now on every transition of env i, in every call that steps this
                env, is computed from the command its actor gave d steps ago, d the row of its episode step count of table
                ``ids[i]`` ([N] integers, free per env; None: table 0 for every env); the state's last-action columns and a
                recording keep the actor's own command.  Attaching zeroes the env's command history.  A table shorter than
                ``episode_step_limit`` holds its last row."""
                self._set_schedule(schedules.DELAY, bank, ids)

            def set_sensor_schedule(self, bank, ids=None):
                """Attach ``bank`` (an ``l2f.SensorBank``): from now on every observation assembled for env i - ``vector.observe``
                and every rollout - carries in columns 0..17 the reading taken d steps ago, d the row of its episode step count of
                table ``ids[i]`` ([N] integers, free per env; None: table 0 for every env), the episode's first reading where the
                episode is younger; the state and the env step are unchanged and a recording holds what the policy saw.
                Attaching zeroes the env's readings.  A table shorter than ``episode_step_limit`` holds its last row."""
                self._set_schedule(schedules.SENSOR, bank, ids)

            def clear_wrench_schedule(self): self._clear_schedule(schedules.WRENCH)
            def clear_vehicle_schedule(self): self._clear_schedule(schedules.VEHICLE)
            def clear_wind_schedule(self): self._clear_schedule(schedules.WIND)
            def clear_delay_schedule(self): self._clear_schedule(schedules.DELAY)
            def clear_sensor_schedule(self): self._clear_schedule(schedules.SENSOR)

            @property
            def wrench_schedule(self):
                """(bank, ids) of the attached schedule, or None."""
                return self._schedule(schedules.WRENCH)

            @property
            def vehicle_schedule(self):
                """(bank, ids) of the attached schedule, or None."""
                return self._schedule(schedules.VEHICLE)

            @property
            def wind_schedule(self):
                """(bank, ids) of the attached schedule, or None."""
                return self._schedule(schedules.WIND)

            @property
            def delay_schedule(self):
                """(bank, ids) of the attached schedule, or None."""
                return self._schedule(schedules.DELAY)

            @property
            def sensor_schedule(self):
                """(bank, ids) of the attached schedule, or None."""
                return self._schedule(schedules.SENSOR)

            def tracking_error(self):
                """-> (sum_sq [N] float32, steps [N] uint32): per env, the running sum of |p - p_ref|^2 over the steps it took in
                tracked rollouts (``rollout(..., reference=ref)``; true position, at observe time) and their count.
                ``reset_statistics`` zeroes both."""
                sq, steps = np.empty(mod.N_ENVIRONMENTS, np.float32), np.empty(mod.N_ENVIRONMENTS, np.uint32)
                _lib.call("rq_env_get_tracking_error", self._require("environment"), sq.ctypes.data, steps.ctypes.data, 0)
                return sq, steps

            def tracking_rmse(self):
                """Root mean square distance to the setpoint per env, float64 [N] (NaN for an env that took no tracked step)."""
                sq, steps = self.tracking_error()
                with np.errstate(invalid="ignore", divide="ignore"):
                    return np.sqrt(sq.astype(np.float64) / steps)

        class _Container(_Handle):
            _create = None
            _get = None
            _set = None
            _dim = 0

            def _ensure(self, env):
                if self._h is None:
                    h = C.c_void_p()
                    _lib.call(self._create, env._require("environment"), C.byref(h))
                    self._adopt(h)
                    self._env = env
                return self._h

            def numpy(self):
                out = np.empty((mod.N_ENVIRONMENTS, self._dim), np.float32)
                _lib.call(self._get, self._require(type(self).__name__), _lib.fptr(out))
                return out

            def set(self, array):
                a = np.ascontiguousarray(array, np.float32)
                assert a.shape == (mod.N_ENVIRONMENTS, self._dim), a.shape
                _lib.call(self._set, self._require(type(self).__name__), _lib.fptr(a))

            def tensor(self):
                """The container's device buffer as a torch tensor view, field-major [dim, ld]; zero copy."""
                p = C.c_void_p()
                _lib.call(self._ptr, self._require(type(self).__name__), C.byref(p))
                return _as_torch(p.value, (self._dim, self._env._ld()), "<f4", self)

        class VectorParameters(_Container):
            _destroy, _create, _get, _set, _dim = ("rq_params_destroy", "rq_params_create", "rq_params_get",
                                                   "rq_params_set", PARAM_DIM)
            _ptr = "rq_params_device_ptr"

        class VectorState(_Container):
            _destroy, _create, _get, _set, _dim = ("rq_state_destroy", "rq_state_create", "rq_state_get",
                                                   "rq_state_set", STATE_DIM)
            _ptr = "rq_state_device_ptr"

            _mirror = None      # host copy handed out by ``.states``; written back before the next device use

            def _flush(self):
                m, self._mirror = self._mirror, None
                if m is not None and self._h is not None:
                    _lib.call(self._set, self._h, _lib.fptr(m))

            def _require(self, what):
                if self._mirror is not None:
                    self._flush()
                return super()._require(what)

            def _ensure(self, env):
                if self._mirror is not None:
                    self._flush()
                return super()._ensure(env)

            def assign(self, other):
                """``state.assign(next_state)`` (README.md:99)."""
                if self._h is None:
                    self._ensure(other._env)
                self._mirror = None                       # overwritten anyway
                fast = _lib.fast
                if fast is not None and other._mirror is None:
                    status = fast.assign(_lib.fn_addr("rq_state_assign"), self._h, other._h)
                    if status == 0:
                        return
                    if status != 1:
                        _lib.check(status)
                _lib.call("rq_state_assign", self._h, other._require("VectorState"))

            @property
            def states(self):
                """One view per env (``.position`` etc., README.md:73-75).  Like the reference's, the views are
                writable - ``s.position[0] += 0.1`` (README.md:74) changes this VectorState: they alias a host
                copy that is written back to the device before the next call that uses the state (views kept
                beyond that call are stale)."""
                self._mirror = m = self.numpy()
                return [_StateView(r) for r in m]

            def __copy__(self):
                c = VectorState()
                if self._h is not None:
                    c._ensure(self._env)
                    c.assign(self)
                return c

        class Trajectory(_Handle):
            """Rollout recording buffer: ``vector.rollout(..., trajectory=t)``
            appends per step and env the 22 policy inputs, the raw action, the reward and a done
            code (0 running, 1 terminated, 2 step limit, 4 frozen/not stepped)."""
            _destroy = "rq_trajectory_destroy"

            def __init__(self, env, capacity_steps):
                super().__init__()
                h = C.c_void_p()
                _lib.call("rq_trajectory_create", env._require("environment"), int(capacity_steps), C.byref(h))
                self._adopt(h)
                self._env = env

            def __len__(self):
                n = C.c_uint32()
                _lib.call("rq_trajectory_length", self._h, C.byref(n), None)
                return n.value

            def reset(self):
                _lib.call("rq_trajectory_reset", self._h)

            def numpy(self):
                """-> dict(obs [T,N,22], act [T,N,4], rew [T,N], done [T,N] uint8)"""
                T, N = len(self), mod.N_ENVIRONMENTS
                out = dict(obs=np.empty((T, N, 22), np.float32), act=np.empty((T, N, 4), np.float32),
                           rew=np.empty((T, N), np.float32), done=np.empty((T, N), np.uint8))
                _lib.call("rq_trajectory_get", self._h, _lib.fptr(out["obs"]), _lib.fptr(out["act"]),
                          _lib.fptr(out["rew"]), out["done"].ctypes.data)
                return out

            def tensors(self):
                """The recorded steps as torch tensor VIEWS of the device buffers (zero copy), in the device layout:
                obs [T, 22, ld], act [T, 4, ld], rew [T, ld], done [T, ld] uint8 - env i is index i < N of the
                last axis.  ``obs.permute(0, 2, 1)[:, :N]`` is the learner layout [T, N, 22].
                What the engine has enqueued is waited for first: rollouts return before they have run, the engine's stream
                does not order itself against torch's, and a view read too early shows the buffer's previous contents."""
                _lib.call("rq_device_synchronize", self._env._device._h)
                o, a, r, d, ld = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32()
                _lib.call("rq_trajectory_device_ptrs", self._require("trajectory"), C.byref(o), C.byref(a), C.byref(r),
                          C.byref(d), C.byref(ld))
                T, L = len(self), ld.value
                return dict(obs=_as_torch(o.value, (T, 22, L), "<f4", self), act=_as_torch(a.value, (T, 4, L), "<f4", self),
                            rew=_as_torch(r.value, (T, L), "<f4", self), done=_as_torch(d.value, (T, L), "|u1", self))

            def relabel(self, policy, overwrite=False, fetch=True):
                """Actions of ``policy`` (a teacher, a newer student, ...) on the recorded observations, following
                the recorded episode structure (GRU state reset after episode ends, held on frozen steps; it
                starts from the policy's current hidden state: ``policy.reset()`` for episode starts).
                -> [T, N, 4] (``fetch=False``: only on the device); ``overwrite=True`` also replaces the stored
                actions.  With the policy that recorded the trajectory the result equals the stored actions."""
                T, N = len(self), mod.N_ENVIRONMENTS
                out = np.empty((T, N, 4), np.float32) if fetch else None
                _lib.call("rq_trajectory_relabel", self._h, policy._handle(self._env._device),
                          _lib.fptr(out) if fetch else None, 1 if overwrite else 0)
                return out

            def hidden(self, policy, device=False):
                """The GRU state of ``policy`` ENTERING every recorded step, [T, N, 16] float32: its forward over the
                recorded observations from the learned initial state (back to it after done codes 1 and 2, held on code
                4) - what ``raptor_amd.probing`` reads.  NumPy, or with ``device=True`` a torch tensor on the engine's
                device.  The policy's own hidden state is not changed."""
                T, N = len(self), mod.N_ENVIRONMENTS
                pol = policy._handle(self._env._device)
                self._learner_forwards = getattr(self, "_learner_forwards", 0) + 1     # the saved state may be this call's now
                if not device:
                    out = np.empty((T, N, 16), np.float32)
                    _lib.call("rq_trajectory_get_hidden", self._require("trajectory"), pol, _lib.fptr(out), 0)
                    return out
                import torch
                dev = torch.device(f"cuda:{_ordinal_of(self)}")
                out = torch.empty((T, N, 16), dtype=torch.float32, device=dev)
                torch.cuda.current_stream(dev).synchronize()          # the engine runs on its own stream
                _lib.call("rq_trajectory_get_hidden", self._require("trajectory"), pol, out.data_ptr(), 1)
                return out

            def wrench_targets(self, bank, ids, params, start_steps=None, units="relative", device=False):
                """The scheduled wrench every env was flown with at every recorded step, rebuilt on the device
                (rq_trajectory_wrench_targets): ``bank`` an ``l2f.WrenchBank`` and ``ids`` [N] its table per env (None: table
                0) - what ``env.set_wrench_schedule`` was given -, ``params`` the VectorParameters flown, ``start_steps`` [N] what
                ``env.episode_steps()`` returned right before the rollout that recorded step 0 (None: 0).  ``units``: "relative"
                (the rows themselves) or "absolute" (N and N m).  -> NumPy [T, N, 6] (columns ``probing.WRENCH_NAMES``), zeros on
                frozen steps; with ``device=True`` a torch tensor [T, 6, ld] on the engine's device, the layout
                ``HiddenProbe.moments(traj, targets=..., device=True)`` takes.  The per-episode base disturbance is not part of it."""
                from .disturbances import check_units, check_wrench_ids
                if not isinstance(bank, WrenchBank):
                    raise ValueError("bank must be an l2f.WrenchBank")
                T, N = len(self), mod.N_ENVIRONMENTS
                u = check_units(units)
                a = None if ids is None else check_wrench_ids(ids, bank.n_tables, N)
                k = None
                if start_steps is not None:
                    k = np.asarray(start_steps)
                    if k.shape != (N,) or k.dtype == bool or not np.issubdtype(k.dtype, np.integer) or (k < 0).any():
                        raise ValueError(f"start_steps must be {N} non-negative integers (env.episode_steps())")
                    k = np.ascontiguousarray(k.astype(np.uint32))
                h, p = self._require("trajectory"), params._require("VectorParameters")
                ia, ka = (None if a is None else a.ctypes.data), (None if k is None else k.ctypes.data)
                if not device:
                    out = np.empty((T, 6, N), np.float32)
                    _lib.call("rq_trajectory_wrench_targets", h, bank._h, ia, p, ka, u, _lib.fptr(out), N, 0)
                    return np.ascontiguousarray(out.transpose(0, 2, 1))
                import torch
                dev = torch.device(f"cuda:{_ordinal_of(self)}")
                ld = self._env._ld()
                out = torch.zeros((T, 6, ld), dtype=torch.float32, device=dev)
                torch.cuda.current_stream(dev).synchronize()          # the engine runs on its own stream
                _lib.call("rq_trajectory_wrench_targets", h, bank._h, ia, p, ka, u, out.data_ptr(), ld, 1)
                return out

            def relabel_teachers(self, bank, teacher_ids, overwrite=False, fetch=True):
                """Actions of MLP teacher ``teacher_ids[i]`` of ``bank`` (raptor_amd.teachers.TeacherBank) on every
                recorded step of env i, in one launch on the matrix cores -> [T, N, 4] (``fetch=False``: only on
                the device); ``overwrite=True`` replaces the stored actions with the teachers' (the regression
                targets of the distillation step, README.md:208-216)."""
                T, N = len(self), mod.N_ENVIRONMENTS
                from .teachers import check_teacher_ids
                ids = check_teacher_ids(teacher_ids, N)
                out = np.empty((T, N, 4), np.float32) if fetch else None
                _lib.call("rq_trajectory_relabel_teachers", self._h, bank._h, ids.ctypes.data,
                          _lib.fptr(out) if fetch else None, 1 if overwrite else 0)
                return out

        self.Trajectory = Trajectory
        self.VectorRng = VectorRng
        self.VectorEnvironment = VectorEnvironment
        self.VectorParameters = VectorParameters
        self.VectorState = VectorState

    # ------------------------------------------------------------------ l2f vector:: functions
    def initialize_rng(self, device, rng, seed):
        """README.md:58"""
        _lib.call("rq_initialize_rng", device._h, rng._ensure(device), int(seed))

    def initialize_environment(self, device, env):
        """README.md:59 — default MDP configuration."""
        _lib.call("rq_initialize_environment", device._h, env._ensure(device))
        env._dt = None

    def sample_initial_parameters(self, device, env, params, rng):
        """README.md:60 — per-env dynamics parameters (domain randomisation)."""
        _lib.call("rq_sample_initial_parameters", device._h, env._require("environment"), params._ensure(env),
                  rng._require("rng"))

    def sample_initial_state(self, device, env, params, state, rng):
        """README.md:61"""
        _lib.call("rq_sample_initial_state", device._h, env._require("environment"),
                  params._require("VectorParameters"), state._ensure(env), rng._require("rng"))

    def observe(self, device, env, params, state, observation, rng):
        """README.md:96 — fills ``observation`` [N, OBSERVATION_DIM] float32 in place
        (``None``: keep it in the env's device buffer)."""
        fast = _lib.fast
        if fast is not None and observation is not None and state._mirror is None:      # the README loop's call: no ctypes in between
            # (csrc/rq_pyfast.c; a state with views handed out goes the ordinary way, which writes them back first)
            status = fast.observe(_lib.fn_addr("rq_observe"), device._h, env._h, params._h, state._h, observation, rng._h,
                                  self.N_ENVIRONMENTS, OBSERVATION_DIM)
            if status == 0:
                return
            if status != 1:
                _lib.check(status)
        ptr = None
        if observation is not None:
            if (observation.dtype != np.float32 or not observation.flags.c_contiguous or
                    observation.shape != (self.N_ENVIRONMENTS, OBSERVATION_DIM)):
                raise ValueError("observation must be C-contiguous float32 [N_ENVIRONMENTS, OBSERVATION_DIM]")
            ptr = _lib.fptr_cached(observation)
        _lib.call("rq_observe", device._h, env._require("environment"), params._require("VectorParameters"),
                  state._require("VectorState"), ptr, rng._require("rng"))

    def step(self, device, env, params, state, action, next_state, rng):
        """README.md:98 — returns the list of per-env dt in seconds.
        ``action`` [N,4] (``None``: the env's device action buffer, e.g. written by
        ``Raptor.evaluate_step_device``)."""
        fast = _lib.fast
        if fast is not None and action is not None and next_state._h is not None and state._mirror is None and next_state._mirror is None:
            status = fast.step(_lib.fn_addr("rq_step"), device._h, env._h, params._h, state._h, action, next_state._h, rng._h,
                               self.N_ENVIRONMENTS)
            if status == 0:
                return [env._step_dt()] * self.N_ENVIRONMENTS
            if status != 1:
                _lib.check(status)
        aptr = None
        if action is not None:
            a = np.ascontiguousarray(action, np.float32)
            if a.shape != (self.N_ENVIRONMENTS, ACTION_DIM):
                raise ValueError("action must be [N_ENVIRONMENTS, 4]")
            aptr = _lib.fptr(a)
        _lib.call("rq_step", device._h, env._require("environment"), params._require("VectorParameters"),
                  state._require("VectorState"), aptr, next_state._ensure(env), rng._require("rng"), None)
        # every env advances by the configured dt (rq_step's dts output is that constant N times); turning 65 536
        # float32 into Python floats one by one took longer than the step itself (numpy tolist: ~1 ms)
        # (the dt itself is remembered per env: asking the library for the whole configuration cost the README loop 2 us per step)
        return [env._step_dt()] * self.N_ENVIRONMENTS

    def step_device(self, device, env, params, state, next_state, rng):
        """``step`` without host traffic: action from the env's device buffer, no dt list."""
        _lib.call("rq_step", device._h, env._require("environment"), params._require("VectorParameters"),
                  state._require("VectorState"), None, next_state._ensure(env), rng._require("rng"), None)

    def rollout(self, device, env, params, state, policy, rng, n_steps, mode="fused", autoreset=False,
                trajectory=None, teacher_ids=None, reference=None, policy_ids=None, reference_ids=None):
        """The loop body README.md:95-99, ``n_steps`` times, entirely on the device; with
        ``trajectory`` every transition is also appended to that buffer.  ``policy`` is a ``Raptor`` or a
        ``raptor_amd.teachers.TeacherBank``; with a bank, ``teacher_ids`` ([N] integers) names the teacher that flies
        each env (``mode="fused"``: fp32 banks of two hidden layers of 16 / 32 / 64 units; ``"chained"``: every bank).
        ``reference`` (a ``Reference``): the policy tracks that moving setpoint - it sees position and linear velocity relative to
        the row of each env's own episode step count; everything else (state, reward, termination, statistics) stays absolute, a
        ``trajectory`` records what the policy saw, and ``env.tracking_error()`` accumulates.  ``Raptor`` policies only here: a
        ``TeacherBank``'s tracked rollout is ``TeacherBank.fly(..., reference=ref)``.
        ``reference`` may also be a ``ReferenceBank`` with ``reference_ids`` ([N] integers, free per env): env i tracks table
        ``reference_ids[i]`` and computes what it computes with that table as its ``Reference``.
        ``policy`` may also be a ``raptor_amd.policy_bank.PolicyBank``: ``policy_ids`` ([N] integers, constant on every aligned
        block of 64 envs) names the student policy that flies each env, both modes, every policy at the bank's native interval for
        it.  A bank does not take ``reference`` here: ``PolicyBank.fly(..., reference=ref)`` is the bank's tracked rollout."""
        if reference is not None and teacher_ids is not None:
            raise ValueError("reference and teacher_ids do not combine here: a teacher bank's tracked rollout is its own call, "
                             "TeacherBank.fly(..., teacher_ids, reference=ref)")
        ref_ids = _checked_reference(reference, reference_ids, self.N_ENVIRONMENTS)
        m = _MODES[mode]
        entry, handle, ids = "rq_rollout", None, None
        from .policy_bank import PolicyBank, check_policy_ids
        from .teachers import TeacherBank, check_teacher_ids
        if isinstance(policy, PolicyBank):
            if reference is not None:
                raise ValueError("a PolicyBank rollout does not track a reference")
            if teacher_ids is not None:
                raise ValueError("teacher_ids belong to a TeacherBank rollout; a PolicyBank flies the envs by policy_ids")
            if policy_ids is None:
                raise ValueError("a PolicyBank flies the envs by policy_ids: one policy id per env is required")
            ids = check_policy_ids(policy_ids, policy.n_policies, self.N_ENVIRONMENTS)
            entry, handle = "rq_rollout_policies", policy._h
        elif policy_ids is not None:
            raise ValueError("policy_ids belong to a PolicyBank rollout; a Raptor policy flies every env itself and a TeacherBank "
                             "takes teacher_ids")
        elif isinstance(policy, TeacherBank):
            if reference is not None:
                raise ValueError("a TeacherBank does not take reference here: TeacherBank.fly(..., reference=ref) is its tracked rollout")
            if teacher_ids is None:
                raise ValueError("a TeacherBank flies the envs by teacher_ids: one teacher id per env is required")
            ids = check_teacher_ids(teacher_ids, self.N_ENVIRONMENTS)
            entry, handle = "rq_rollout_teachers", policy._h
        elif teacher_ids is not None:
            raise ValueError("teacher_ids belong to a TeacherBank rollout; a Raptor policy flies every env itself")
        else:
            handle = policy._handle(device)
            fast = _lib.fast
            if fast is not None and reference is None and trajectory is None and state._mirror is None and hasattr(fast, "rollout"):
                status = fast.rollout(_lib.fn_addr("rq_rollout"), device._h, env._h, params._h, state._h, handle, rng._h,
                                      int(n_steps), m, ROLLOUT_AUTORESET if autoreset else 0)
                if status == 0:
                    return
                if status != 1:
                    _lib.check(status)
        _rollout_call(entry, device, env, params, state, handle, ids, rng, n_steps, m, autoreset, trajectory, reference, ref_ids)


    # ------------------------------------------------------------------ ui-server messages (README.md:63-92)
    # Only three things about the wire format are visible in the reference tree: every message is a JSON object
    # with "namespace" (from the handshake) and "channel", and the parameters message carries "data", a list with
    # one entry per env that a client may extend (README.md:63-70 adds d["ui"] = {"model", "name"}).  Channel
    # names and the field names inside data[i] follow the l2f parameter / state structure as recalled
    # [UPSTREAM-UNVERIFIED: no file in /root/reference states them]; they are here so that GPU rollouts can be
    # inspected with a ui-server-like client, not as a parity claim.
    @staticmethod
    def _num(v):
        """JSON has no NaN / Infinity (a browser's JSON.parse rejects the tokens Python would emit): null instead."""
        v = float(v)
        return v if np.isfinite(v) else None

    def set_ui_message(self, device, env, ui):
        """README.md:86 - announces what is going to be rendered: N quadrotors."""
        return json.dumps({"namespace": ui.ns, "channel": "setUI",
                           "data": {"type": "l2f-vector", "n_environments": self.N_ENVIRONMENTS}})

    def set_parameters_message(self, device, env, params, ui):
        """README.md:87 - one entry of dynamics parameters per env in ``data``."""
        P = params.numpy()
        data = []
        for p in P:
            data.append({"dynamics": {
                "mass": float(p[0]), "J": [[float(p[1]), 0.0, 0.0], [0.0, float(p[2]), 0.0], [0.0, 0.0, float(p[3])]],
                "rotor_positions": [[float(v) for v in p[4 + 3 * i:7 + 3 * i]] for i in range(4)],
                "rotor_thrust_directions": [[0.0, 0.0, 1.0]] * 4,
                "rotor_torque_directions": [[0.0, 0.0, d] for d in (-1.0, 1.0, -1.0, 1.0)],
                "rotor_thrust_coefficients": [[float(p[16]), float(p[17]), float(p[18])]] * 4,
                "rotor_torque_constants": [float(p[19])] * 4,
                "rotor_time_constants_rising": [float(p[20])] * 4, "rotor_time_constants_falling": [float(p[21])] * 4,
                "action_limit": {"min": float(p[22]), "max": float(p[23])}, "hovering_rpm": float(p[24])}})
        return json.dumps({"namespace": ui.ns, "channel": "setParameters", "data": data}, allow_nan=False)

    def set_state_action_message(self, device, env, params, ui, state, action):
        """README.md:76 - the states (a ``copy(state)`` whose ``.states[i].position`` was shifted works, README.md:73-75)
        and the actions about to be applied, one entry per env."""
        S = state.numpy()
        A = np.asarray(action, np.float32).reshape(self.N_ENVIRONMENTS, ACTION_DIM)
        f = self._num
        data = [{"state": {"position": [f(v) for v in s[0:3]], "orientation": [f(v) for v in s[3:7]],
                           "linear_velocity": [f(v) for v in s[7:10]], "angular_velocity": [f(v) for v in s[10:13]],
                           "rpm": [f(v) for v in s[13:17]]},
                 "action": [f(v) for v in a]} for s, a in zip(S, A)]
        return json.dumps({"namespace": ui.ns, "channel": "setStateAction", "data": data}, allow_nan=False)


_modules = {}


def vector(n_environments, global_env_offset=0):
    """Runtime-sized equivalent of the reference's ``l2f.vectorN`` modules."""
    key = (int(n_environments), int(global_env_offset))
    if key not in _modules:
        _modules[key] = VectorModule(*key)
    return _modules[key]


vector8 = vector(8)   # README.md:45


def __getattr__(name):
    """``from l2f import vectorN`` for any N (the reference ships a fixed set of pre-compiled ``vectorN`` modules, README.md:45
    imports ``vector8``; here N is a run-time value, so every positive N resolves)."""
    if name.startswith("vector") and name[6:].isdigit() and int(name[6:]) > 0 and not name[6:].startswith("0"):
        return vector(int(name[6:]))
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
