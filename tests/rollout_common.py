"""Shared by the tests/test_gpu_*.py modules that hold one rollout path to another bit for bit: the snapshot of everything a
rollout leaves behind, the two comparisons (snapshots, recordings), and the policy-bank batch with its slice-by-slice reference.

Every comparison is on the bits, no tolerance: -0.0 is not +0.0 and a NaN equals only the NaN with its payload.  The comparisons
are tested by themselves in tests/test_rollout_common_cpu.py; this module imports NumPy alone until a function needs the GPU."""
import numpy as np

NOISE = dict(noise_position=0.01, noise_orientation=0.005, noise_linear_velocity=0.02, noise_angular_velocity=0.01)
# the policy-bank batches (Batch, fly_bank, fly_slice)
OFFSET = 1000                  # global id of the bank batch's env 0
LIMIT = 16                     # episode_step_limit: 40 steps cross two episode ends per env
STEPS = 40


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def bank_weights(weights, n_policies):
    """policy k = the shipped weights + 0.05 * default_rng(100 + k).standard_normal(2084), float32"""
    return np.stack([weights + np.float32(0.05) * np.random.default_rng(100 + k).standard_normal(2084).astype(np.float32)
                     for k in range(n_policies)]).astype(np.float32)


def ids_of(block_ids, n):
    """block g's id for each of its 64 envs, the last block cut at n"""
    return np.ascontiguousarray(np.repeat(np.asarray(block_ids, np.uint32), 64)[:n])


def random_table(rows, seed=1):
    """A setpoint table with entries of order 0.1 m and 0.1 m/s, different in every row."""
    g = np.random.default_rng(seed)
    t = (0.1 * g.uniform(-1.0, 1.0, (rows, 6))).astype(np.float32)
    assert len({r.tobytes() for r in t}) == rows
    return t


def roll(w, n_steps, mode="fused", autoreset=True, **kw):
    w.vector.rollout(w.device, w.env, w.params, w.state, w.policy, w.rng, n_steps, mode, autoreset, **kw)


def push(w, which):
    """a third of the envs (which, which + 3, ...) goes outside termination_position: it terminates at its next step and flies its
    following episodes out of phase with the rest"""
    s = w.state.numpy()
    s[which::3, 0] = 0.7
    w.state.set(s)


def snapshot(w, hidden=None):
    """Everything a rollout leaves behind in `w` (anything with .env .state .rng .n), every entry with n rows; `hidden`: the
    actor's hidden state [n, 16], where there is one"""
    e = w.env
    sq, cnt = e.tracking_error()
    snap = dict(state=w.state.numpy(), returns=e.returns(), steps=e.episode_steps(), rewards=e.rewards(), terminated=e.terminated(),
                done=e.done_codes(), frozen=e.frozen(), episode=e.episode_index(), fin_returns=e.finished_returns(),
                fin_lengths=e.finished_lengths(), fin_counts=e.finished_counts(), fin_terminated=e.finished_terminated(),
                track_sq=sq, track_steps=cnt, epoch=np.full(w.n, w.rng.epoch, np.uint32))
    if hidden is not None:
        snap["hidden"] = hidden
    return snap


def world_snapshot(w):
    """snapshot of a World flown by its own policy"""
    return snapshot(w, w.policy.hidden_state(w.n))


def assert_same(a, b, *, rows=slice(None), skip=(), what=""):
    """Two snapshots hold the same keys, and under every key but those of `skip` the same shape and, on `rows`, the same bits."""
    assert a.keys() == b.keys(), f"{what}: keys differ: {sorted(a.keys() ^ b.keys())}"
    for k in a:
        if k in skip:
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: {k} is {x.dtype}{x.shape} against {y.dtype}{y.shape}"
        assert np.array_equal(bits(x[rows]), bits(y[rows])), f"{what}: {k} differs"


def assert_same_recording(ra, rb, what="", frozen_too=False):
    """Two recordings (Trajectory.numpy()) hold the same done codes everywhere and the same bits in obs / act / rew wherever a
    transition was taken (done code != 4: the steps an env sat out frozen are never written by the fused kernel) - with
    `frozen_too`, on every entry."""
    assert ra["done"].shape == rb["done"].shape and np.array_equal(ra["done"], rb["done"]), f"{what}: done codes"
    live = np.ones(ra["done"].shape, bool) if frozen_too else ra["done"] != 4
    for k in ("obs", "act", "rew"):
        assert ra[k].shape == rb[k].shape and ra[k].dtype == rb[k].dtype, f"{what}: {k} shape"
        assert np.array_equal(bits(ra[k][live]), bits(rb[k][live])), f"{what}: {k} differs"


def join(slices):
    """slices' (snapshot, recording) in block order -> the batch's"""
    snaps, recs = zip(*slices)
    snap = {k: np.concatenate([s[k] for s in snaps]) for k in snaps[0]}
    rec = None if recs[0] is None else {k: np.concatenate([r[k] for r in recs], axis=1) for k in recs[0]}
    return snap, rec


class Batch:
    """The l2f-shaped objects of one batch on the GPU: domain randomisation on, seed 3.  `via`: how a bank flies it - "rollout":
    vector.rollout(..., policy_ids=), "fly": PolicyBank.fly."""

    def __init__(self, device, n, offset=OFFSET, limit=LIMIT, noise=False, via="rollout"):
        import raptor_amd.l2f as l2f
        assert via in ("rollout", "fly")
        self.device, self.n, self.via = device, n, via
        self.vector = v = l2f.VectorModule(n, offset)
        self.rng, self.env, self.params, self.state = v.VectorRng(), v.VectorEnvironment(), v.VectorParameters(), v.VectorState()
        v.initialize_rng(device, self.rng, 3)
        v.initialize_environment(device, self.env)
        cfg = self.env.config
        cfg.episode_step_limit = limit
        cfg.domain_randomization = 1
        for k, val in (NOISE if noise else {}).items():
            setattr(cfg, k, val)
        self.env.config = cfg
        v.sample_initial_parameters(device, self.env, self.params, self.rng)
        v.sample_initial_state(device, self.env, self.params, self.state, self.rng)

    def fly(self, actor, steps, mode="fused", autoreset=True, record=False, ids=None, ref=None):
        """`steps`: a number or a list of launches; `ids`: the policy ids, `actor` a bank.  -> the recording (dict) or None"""
        launches = list(steps) if isinstance(steps, (list, tuple)) else [steps]
        tr = self.vector.Trajectory(self.env, sum(launches)) if record else None
        for s in launches:
            if ids is not None and self.via == "fly":
                actor.fly(self.vector, self.device, self.env, self.params, self.state, self.rng, s, ids, mode, autoreset, trajectory=tr,
                          reference=ref)
            else:
                self.vector.rollout(self.device, self.env, self.params, self.state, actor, self.rng, s, mode, autoreset, trajectory=tr,
                                    reference=ref, policy_ids=ids)
        return tr.numpy() if record else None


def fly_bank(device, W, n, ids, rates=None, ref=None, steps=STEPS, mode="fused", autoreset=True, noise=False, record=False,
             limit=LIMIT, bank=None, via="rollout"):
    """A fresh batch flown by PolicyBank(W) - at the native intervals `rates`, where given - or by `bank`.
    -> the batch, its snapshot, the recording"""
    from raptor_amd.policy_bank import PolicyBank
    if bank is None and rates is None:
        bank = PolicyBank(device, W)
    elif bank is None:
        bank = PolicyBank(device, W, native_interval=list(rates))
        assert np.array_equal(bank.native_interval, np.asarray(rates, np.uint32))
    b = Batch(device, n, limit=limit, noise=noise, via=via)
    rec = b.fly(bank, steps, mode, autoreset, record, ids=ids, ref=ref)
    return b, snapshot(b, bank.hidden(n)), rec


def fly_slice(device, w, n, offset, rate=None, ref=None, steps=STEPS, mode="fused", autoreset=True, noise=False, record=False,
              limit=LIMIT):
    """The n envs from global id `offset` on, as a batch of their own, flown by Raptor(w) through the single-policy rollout.
    -> its snapshot, the recording"""
    from raptor_amd.foundation_policy import Raptor
    pol = Raptor(device, weights=w) if rate is None else Raptor(device, weights=w, native_interval=int(rate))
    b = Batch(device, n, offset=offset, limit=limit, noise=noise)
    rec = b.fly(pol, steps, mode, autoreset, record, ref=ref)
    return snapshot(b, pol.hidden_state(n)), rec
