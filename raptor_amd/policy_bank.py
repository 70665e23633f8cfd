"""Policy bank: many student policies flown in one rollout, one policy per wave.

Post-training of rl-tools/raptor writes a checkpoint and an ``evaluation/*`` record every epoch, and its users pick the student by
closed-loop return, episode length and share terminated; hyper-parameter sweeps and seed populations of ``training.Distiller`` ask
the same question of many weight vectors - and ``training.BankDistiller`` is their learner: it updates every policy of a bank on
its own blocks of a recording in one go, on the device, so the bank flies again with the new weights.  ``PolicyBank`` holds P policies of the ``Raptor`` topology on the device (fp32) and
``vector.rollout(..., bank, ..., policy_ids=ids)`` flies env ``i`` with policy ``ids[i]`` - in ONE launch: a 64-env block is one
wave of the fused kernel and the weights are that wave's matrix operands, so the granularity is the block: ``ids`` must be
constant on every aligned block of 64 env indices (``block_policy_assignment`` deals blocks round-robin).  What an env computes
is, bit for bit, what ``Raptor(weights=W[ids[i]])`` computes for it in a rollout of its own.
"""
import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._lib import POLICY_HIDDEN_DIM, POLICY_NUM_WEIGHTS

BLOCK = 64      # envs per wave: the granularity of an assignment


def block_policy_assignment(n_envs, n_policies):
    """policy id of every env (uint32 [n_envs]): the blocks of 64 envs dealt round-robin, block g -> policy g % n_policies (the
    ragged last block is one block).  1 000 policies x 64 envs: ``block_policy_assignment(64000, 1000)``."""
    n_envs, n_policies = int(n_envs), int(n_policies)
    if n_envs <= 0 or n_policies <= 0:
        raise ValueError("n_envs and n_policies must be positive")
    return np.ascontiguousarray(((np.arange(n_envs) // BLOCK) % n_policies).astype(np.uint32))


def check_policy_ids(ids, n_policies, n_envs=None):
    """The host-side validator of an assignment (no GPU): integers, one per env (``n_envs`` given: exactly that many), each in
    [0, n_policies), constant on every aligned block of 64.  -> the ids as a contiguous uint32 array; ValueError otherwise."""
    a = np.asarray(ids)
    if a.ndim != 1 or a.size == 0:
        raise ValueError("policy_ids must be a non-empty one-dimensional array: one id per env")
    if n_envs is not None and a.size != int(n_envs):
        raise ValueError(f"policy_ids must hold one id per env: {a.size} ids for {int(n_envs)} envs")
    if not (np.issubdtype(a.dtype, np.integer) or (np.issubdtype(a.dtype, np.floating) and np.all(a == np.floor(a)))):
        raise ValueError("policy_ids must be integers")
    a = a.astype(np.int64)
    if a.min() < 0 or a.max() >= int(n_policies):
        bad = int(np.flatnonzero((a < 0) | (a >= int(n_policies)))[0])
        raise ValueError(f"policy id out of range: env {bad} names policy {int(a[bad])} of a bank of {int(n_policies)}")
    first = a[(np.arange(a.size) // BLOCK) * BLOCK]
    if not np.array_equal(a, first):
        bad = int(np.flatnonzero(a != first)[0])
        raise ValueError(f"policy ids differ inside a 64-env block: env {bad} names policy {int(a[bad])}, env {bad // BLOCK * BLOCK} "
                         f"policy {int(first[bad])} (a policy flies whole blocks of 64 envs)")
    return np.ascontiguousarray(a.astype(np.uint32))


def policy_episode_table(env, policy_ids, n_policies):
    """Per-policy closed-loop summary of the env's finished episodes - what a checkpoint is picked by.

    Reads the env's finished-episode records (``env.finished_*``: per env, the number of finished episodes, how many of them
    terminated, and the return / length of the last one) and groups them by ``policy_ids``.  -> dict of [n_policies] arrays:
    ``envs`` (envs flown), ``episodes`` (finished), ``mean_return`` / ``std_return`` / ``mean_length`` (over the envs' last finished
    episodes, NaN for a policy without one) and ``termination_share`` (terminated / finished, NaN without episodes)."""
    ids = np.asarray(policy_ids, np.int64).ravel()
    counts = np.asarray(env.finished_counts(), np.float64)
    done = counts > 0
    ret = np.where(done, np.asarray(env.finished_returns(), np.float64), 0.0)
    length = np.where(done, np.asarray(env.finished_lengths(), np.float64), 0.0)
    term = np.asarray(env.finished_terminated(), np.float64)
    k = int(n_policies)
    envs = np.bincount(ids, minlength=k)
    with_episode = np.bincount(ids, weights=done.astype(np.float64), minlength=k)
    episodes = np.bincount(ids, weights=counts, minlength=k)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_return = np.bincount(ids, weights=ret, minlength=k) / with_episode
        dev = np.where(done, ret - mean_return[ids], 0.0)
        std_return = np.sqrt(np.bincount(ids, weights=dev * dev, minlength=k) / with_episode)
        mean_length = np.bincount(ids, weights=length, minlength=k) / with_episode
        termination_share = np.bincount(ids, weights=term, minlength=k) / episodes
    return dict(envs=envs, episodes=episodes.astype(np.int64), mean_return=mean_return, std_return=std_return,
                mean_length=mean_length, termination_share=termination_share)


def policy_tracking_table(sum_sq, steps, policy_ids, n_policies):
    """Per-policy tracking error from the per-env sums ``env.tracking_error()`` returns: ``sum_sq`` [N] (sum of |p - p_ref|^2 over
    the counted steps) and ``steps`` [N] (how many), grouped by ``policy_ids`` -> ``tracking_rmse`` [n_policies] (float64):
    sqrt(sum of the policy's sums / sum of its counts), NaN for a policy without a counted step."""
    ids = np.asarray(policy_ids, np.int64).ravel()
    sq = np.asarray(sum_sq, np.float64).ravel()
    cnt = np.asarray(steps, np.float64).ravel()
    if not (ids.shape == sq.shape == cnt.shape):
        raise ValueError("sum_sq, steps and policy_ids must hold one entry per env")
    k = int(n_policies)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(np.bincount(ids, weights=sq, minlength=k) / np.bincount(ids, weights=cnt, minlength=k))


MAX_NATIVE_INTERVAL = 64      # RQ_POLICY_MAX_NATIVE_INTERVAL


class PolicyBank:
    """``weights`` [P, 2084] float32, each row in the checkpoint order ``Raptor`` takes.  fp32 only; no Standardize or
    SampleAndSquash stage.  ``native_interval``: R, 1 to 64, a scalar or one per policy - policy p's hidden state moves on every
    R[p]-th step of an episode only, as ``Raptor(native_interval=R)``'s does (flown at ``dt = 0.01 / R``); policies of different
    intervals fly side by side in one rollout.  The learner (``training.BankDistiller``) takes a bank at interval 1 only."""

    def __init__(self, device, weights, native_interval=1):
        w = np.ascontiguousarray(weights, np.float32)
        if w.ndim != 2 or w.shape[0] == 0 or w.shape[1] != POLICY_NUM_WEIGHTS:
            raise ValueError(f"weights must be [n_policies, {POLICY_NUM_WEIGHTS}]")
        self.n_policies = int(w.shape[0])
        intervals = self._checked_intervals(native_interval)
        self._weights = w.copy()
        self._weights_on_device = False      # training.BankDistiller.step: the device's weights are newer than _weights
        self._device = device
        h = C.c_void_p()
        _lib.call("rq_policy_bank_create", device._h, _lib.fptr(w), self.n_policies, C.byref(h))
        self._h = h
        self._fin = weakref.finalize(self, _lib.load().rq_policy_bank_destroy, h)
        self._intervals = np.ones(self.n_policies, np.uint32)
        if (intervals != 1).any():
            self.native_interval = intervals

    def _checked_intervals(self, interval):
        """a scalar or a length-P sequence of integers in 1 .. 64 -> uint32 [P]; ValueError otherwise (no library call)"""
        a = np.asarray(interval)
        if a.ndim > 1 or (a.ndim == 1 and a.size != self.n_policies):
            raise ValueError(f"native_interval must be a scalar or one interval per policy: {a.size} for a bank of {self.n_policies}")
        if a.dtype == bool or not (np.issubdtype(a.dtype, np.integer) or (np.issubdtype(a.dtype, np.floating) and np.all(a == np.floor(a)))):
            raise ValueError("native_interval must be integers")
        a = np.broadcast_to(a.astype(np.int64), (self.n_policies,))
        bad = np.flatnonzero((a < 1) | (a > MAX_NATIVE_INTERVAL))
        if bad.size:
            raise ValueError(f"native_interval must be 1 .. {MAX_NATIVE_INTERVAL}: policy {int(bad[0])} is given {int(a[bad[0]])}")
        return np.ascontiguousarray(a.astype(np.uint32))

    @property
    def native_interval(self):
        """[P] uint32: policy p's native interval (a copy)."""
        return self._intervals.copy()

    @native_interval.setter
    def native_interval(self, interval):
        a = self._checked_intervals(interval)
        _lib.call("rq_policy_bank_set_native_interval", self._h, a.ctypes.data, a.size)
        self._intervals = a

    @classmethod
    def from_checkpoints(cls, device, paths, check_observation=True):
        """One policy per file, each an rl-tools policy checkpoint (``checkpoint.h5`` or the C++ export, as
        ``Raptor.from_checkpoint`` reads them).  A file whose ``/actor@meta`` names another observation layout than this
        engine's ``observe`` assembles is refused, as ``Raptor`` refuses it.  -> PolicyBank, policy k = paths[k]."""
        from . import checkpoint as ck
        paths = list(paths)
        if not paths:
            raise ValueError("no checkpoint files")
        rows = []
        for path in paths:
            w, _, meta = ck.load_checkpoint(path, with_meta=True)
            if check_observation:
                ck.check_observation(meta, path)
            rows.append(np.asarray(w, np.float32))
        return cls(device, np.stack(rows))

    @property
    def weights(self):
        if self._weights_on_device:          # updated on the device (training.BankDistiller.step): fetched once, when first asked for
            w = np.empty((self.n_policies, POLICY_NUM_WEIGHTS), np.float32)
            _lib.call("rq_policy_bank_get_weights", self._h, _lib.fptr(w))
            self._weights, self._weights_on_device = w, False
        return self._weights

    def set_weights(self, index, weights):
        """New parameters for policy ``index``: its slot is repacked in place; the hidden state stays."""
        w = np.array(weights, dtype=np.float32, copy=True).reshape(-1)
        if w.size != POLICY_NUM_WEIGHTS:
            raise ValueError(f"expected {POLICY_NUM_WEIGHTS} weights")
        if not 0 <= int(index) < self.n_policies:
            raise ValueError(f"policy index {index} is outside a bank of {self.n_policies}")
        _lib.call("rq_policy_bank_set_weights", self._h, int(index), _lib.fptr(w))
        self.weights[int(index)] = w         # (the other rows fetched first, should an update have left the host copy behind)

    def reset(self):
        """hidden state <- every env's own policy's initial_hidden_state (applied by the next use that knows the assignment)."""
        _lib.call("rq_policy_bank_reset", self._h)

    def hidden(self, batch):
        """The hidden state [batch, 16] of the envs the bank last flew."""
        out = np.empty((int(batch), POLICY_HIDDEN_DIM), np.float32)
        _lib.call("rq_policy_bank_get_hidden", self._h, _lib.fptr(out), int(batch))
        return out

    def fly(self, vector, device, env, params, state, rng, n_steps, policy_ids, mode="fused", autoreset=False, trajectory=None,
            reference=None, reference_ids=None):
        """The bank's own rollout call: ``vector.rollout(..., bank, ..., policy_ids=ids)`` - every policy at its native interval -
        and, with ``reference`` (an ``l2f.Reference``), on that moving setpoint: each env sees position and linear velocity relative
        to the row of its own episode step count, a ``trajectory`` records what the policy saw and ``env.tracking_error()``
        accumulates, as in a ``Raptor`` policy's tracked rollout.  With an ``l2f.ReferenceBank`` and ``reference_ids`` ([N] integers,
        free per env, also inside a block) env i tracks table ``reference_ids[i]``: one rollout flies P policies on M setpoints."""
        from .l2f import _MODES, _checked_reference, _rollout_call
        ids = check_policy_ids(policy_ids, self.n_policies, vector.N_ENVIRONMENTS)
        ref_ids = _checked_reference(reference, reference_ids, vector.N_ENVIRONMENTS)
        m = _MODES[mode]
        _rollout_call("rq_rollout_policies", device, env, params, state, self._h, ids, rng, n_steps, m, autoreset, trajectory,
                      reference, ref_ids)

    def evaluate(self, vector, device, env, params, state, rng, n_steps, policy_ids=None, mode="fused", autoreset=True,
                 reference=None, reference_ids=None, wrench_ids=None, vehicle_ids=None, wind_ids=None, delay_ids=None,
                 sensor_ids=None):
        """The closed-loop evaluation of the whole bank: statistics and hidden state start afresh, one rollout of ``n_steps`` flies
        env i with policy ``policy_ids[i]`` (default: blocks dealt round-robin) at its native interval ->
        ``policy_episode_table`` of what it finished.  With ``reference`` the bank tracks that moving setpoint and the table gains
        ``tracking_rmse`` [P] (``policy_tracking_table`` of ``env.tracking_error()``, which starts afresh too).  With an
        ``l2f.ReferenceBank`` and ``reference_ids`` (``tracking.spread_reference_ids(N, M, policy_ids)`` deals them evenly inside
        every policy's envs) ``tracking_rmse`` is [P, M]: policy p on setpoint r (``tracking.reference_tracking_table``).
        ``wrench_ids`` ([N] integers; the env carries a wrench schedule, ``env.set_wrench_schedule(bank)``): env i flies
        disturbance scenario ``wrench_ids[i]`` of the attached bank (dealt like reference ids) and, on an ``l2f.Reference`` such as
        ``tracking.hold``, ``tracking_rmse`` is [P, M] over the scenarios: P checkpoints x M disturbances in one launch.
        ``vehicle_ids`` likewise name the tables of the env's vehicle schedule (``env.set_vehicle_schedule(bank)``): [P, M] over the
        vehicle scenarios, and ``wind_ids`` those of its wind schedule (``env.set_wind_schedule(bank)``): [P, M] over the wind
        scenarios, and ``delay_ids`` those of its delay schedule (``env.set_delay_schedule(bank)``): [P, M] over the latency
        scenarios, and ``sensor_ids`` those of its sensor schedule (``env.set_sensor_schedule(bank)``): [P, M] over the sensor
        scenarios.  At most one of ``wrench_ids``, ``vehicle_ids``, ``wind_ids``, ``delay_ids`` and ``sensor_ids``: two together are
        refused."""
        ids = block_policy_assignment(vector.N_ENVIRONMENTS, self.n_policies) if policy_ids is None else policy_ids
        from . import schedules
        from .l2f import _checked_reference, tracking_rmse
        ref_ids = _checked_reference(reference, reference_ids, vector.N_ENVIRONMENTS)       # before the statistics are reset
        given = {schedules.WRENCH: wrench_ids, schedules.VEHICLE: vehicle_ids, schedules.WIND: wind_ids, schedules.DELAY: delay_ids,
                 schedules.SENSOR: sensor_ids}
        s_ids = schedules.checked_schedule_ids(env, given, ref_ids, vector.N_ENVIRONMENTS)
        if s_ids is not None:
            s_ids.attach(env)
        env.reset_statistics()
        self.reset()
        self.fly(vector, device, env, params, state, rng, n_steps, ids, mode=mode, autoreset=autoreset, reference=reference,
                 reference_ids=reference_ids)
        table = policy_episode_table(env, ids, self.n_policies)
        if reference is not None:
            table["tracking_rmse"] = tracking_rmse(env, reference, ref_ids, s_ids, ids, self.n_policies)
        return table
