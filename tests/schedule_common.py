"""What the GPU suites of the three kinds of schedule share (tests/test_gpu_wrench.py, test_gpu_vehicle.py, test_gpu_wind.py): the
rollouts' shape, ids that mix the tables inside every wave, and fresh worlds flown with a schedule attached - by their own policy or
by a policy bank, tracked or not.  A suite makes one ``Flights`` for its kind and keeps its tests."""
import numpy as np

from gpu_common import World
from rollout_common import bank_weights, bits, ids_of, roll, snapshot, world_snapshot

N, LAUNCHES = 200, (20, 20)                  # four blocks, the last ragged; 40 steps as two launches cross episode ends
BLOCK_IDS = [2, 0, 2, 1]                     # the policy bank's blocks: non-monotone, policy 2 twice
S_WRENCH = slice(21, 27)                     # RQ_S_FORCE, RQ_S_TORQUE


def mixed_ids(n, m, shift=0):
    """every wave holds all m ids and neighbouring lanes differ"""
    return ((np.arange(n) * 7 + 1 + shift) % m).astype(np.uint32)


def reference_kw(setpoints, kind, n=N):
    """setpoints: (tables, an l2f.Reference, an l2f.ReferenceBank of three); kind: "none", "single" or "bank" """
    _, single, many = setpoints
    return {"none": {}, "single": dict(reference=single), "bank": dict(reference=many, reference_ids=mixed_ids(n, 3, 2))}[kind]


def teachers(device, K=5):
    from raptor_amd.teachers import TeacherBank, layers_parameter_count
    g = np.random.default_rng(2)
    widths = [32, 16]
    W = np.empty((K, layers_parameter_count(22, widths)), np.float32)
    for k in range(K):
        parts, prev = [], 22
        for h in widths + [4]:
            parts += [g.standard_normal(h * prev) * 0.2 / np.sqrt(prev), g.standard_normal(h) * 0.1]
            prev = h
        W[k] = np.concatenate(parts).astype(np.float32)
    return TeacherBank.from_layers(device, W, 22, widths, "tanh", "identity", "fp32")


class Flights:
    """kind: "wrench", "vehicle" or "wind" - the env's setter; kw: the suite's env configuration; rates: the policy bank's native
    intervals (None: every policy at 1); nonzero_base_force: a world flown by its own policy must have sampled a base force that is
    neither 0 nor -0 (the wind suite's identity, b + (0 * u) = b, holds for those)."""

    def __init__(self, kind, kw, rates=None, nonzero_base_force=False):
        self.setter, self.kw, self.rates, self.nonzero_base_force = f"set_{kind}_schedule", kw, rates, nonzero_base_force

    def _attach(self, w, schedule):
        if schedule is not None:
            getattr(w.env, self.setter)(*schedule)

    def fly_policy(self, device, oracle, schedule, mode, autoreset, record, ref_kw, interval=1, n=N, launches=LAUNCHES, kw=None):
        """a fresh world flown by its own policy -> world, snapshot, recording; schedule: (bank, ids) or None"""
        w = World(device, oracle, n, **(self.kw if kw is None else kw))
        w.policy.native_interval = interval
        if self.nonzero_base_force:
            base = w.state.numpy()[:, S_WRENCH]
            assert (base != 0).all() and not (bits(base) == 0x80000000).any()          # a nonzero base force, and no -0
        self._attach(w, schedule)
        tr = w.vector.Trajectory(w.env, sum(launches)) if record else None
        for c in launches:
            roll(w, c, mode, autoreset, trajectory=tr, **ref_kw)
        return w, world_snapshot(w), tr.numpy() if record else None

    def fly_policy_bank(self, device, oracle, weights, schedule, mode, autoreset, record, ref_kw, launches=LAUNCHES):
        from raptor_amd.policy_bank import PolicyBank
        w = World(device, oracle, N, **self.kw)
        pb = PolicyBank(device, bank_weights(weights, 3), **({} if self.rates is None else dict(native_interval=self.rates)))
        pids = ids_of(BLOCK_IDS, N)
        self._attach(w, schedule)
        tr = w.vector.Trajectory(w.env, sum(launches)) if record else None
        for c in launches:
            pb.fly(w.vector, device, w.env, w.params, w.state, w.rng, c, pids, mode, autoreset, trajectory=tr, **ref_kw)
        return w, snapshot(w, pb.hidden(N)), tr.numpy() if record else None

    def fly(self, device, oracle, weights, setpoints, call, schedule, mode, autoreset, launches=LAUNCHES):
        """call: "rollout", "track_refs", "policy_bank" or "policy_bank_refs"; recorded"""
        if call.startswith("policy_bank"):
            ref_kw = reference_kw(setpoints, "bank") if call.endswith("refs") else {}
            return self.fly_policy_bank(device, oracle, weights, schedule, mode, autoreset, True, ref_kw, launches)
        ref_kw = reference_kw(setpoints, "bank") if call == "track_refs" else {}
        return self.fly_policy(device, oracle, schedule, mode, autoreset, True, ref_kw, launches=launches)
