"""A reference per env (rq_rollout_track_refs, rq_rollout_policies_track_refs): M setpoint tables in one rollout, env i on table
reference_ids[i].  The yardstick is the project's own single-reference path: the same world, seed and pushes flown with
``Reference(tables[r])`` gives, on the envs with ``ids == r``, every bit the bank rollout gives - state, hidden state, statistics,
finished-episode records, done codes, tracking sums and counts, the recording.  No tolerance anywhere: the kernels are the same,
only the table an env's row is read from is its own."""
import ctypes as C

import numpy as np
import pytest

import raptor_amd.l2f as l2f
from raptor_amd import _lib
from raptor_amd._lib import RaptorQuadError
from gpu_common import World
from rollout_common import (assert_same, assert_same_recording, bank_weights, bits, push, random_table, roll, snapshot,
                            world_snapshot)

pytestmark = pytest.mark.gpu

LIMIT = 9           # episode_step_limit: episodes end and restart inside every rollout
CHUNKS = (7, 12)
M = 3
KW = dict(seed=5, episode_step_limit=LIMIT, termination_position=0.6)


def _ids(n, shift=0):
    """every wave holds all three ids and neighbouring lanes differ"""
    return ((np.arange(n) * 7 + 1 + shift) % M).astype(np.uint32)


@pytest.fixture(scope="module")
def tables():
    t = np.stack([random_table(LIMIT, 11 + r) for r in range(M)])
    assert len({r.tobytes() for r in t.reshape(-1, 6)}) == M * LIMIT
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def bank(device, tables):
    b = l2f.ReferenceBank(device, tables)
    assert (b.n_references, b.rows) == (M, LIMIT)
    return b


@pytest.fixture(scope="module")
def refs(device, tables):
    return [l2f.Reference(device, np.array(tables[r])) for r in range(M)]


def _fly(w, launch, chunks=CHUNKS, pushes=True):
    """the launches of every world of this file: a push before each of the first two (the same in every world)"""
    for j, chunk in enumerate(chunks):
        if pushes and j < 2:
            push(w, j)
        launch(w, chunk)


def _ragged(w, ids):
    """at this launch boundary the first wave holds at least three distinct episode step counts and all M ids: the per-lane table
    base met per-lane rows"""
    k = w.env.episode_steps()[:64]
    return len(np.unique(k)) >= 3 and len(np.unique(ids[:64])) == M


_singles = {}


def _single_reference_worlds(device, oracle, refs, n, precision, autoreset, noise, interval=1, chunks=CHUNKS):
    """the M worlds b_r flown fused with Reference(tables[r]) -> their snapshots; computed once per case and left alone (fused ==
    chained for a single reference is tests/test_gpu_tracking.py's and test_gpu_control_rate.py's business)"""
    key = (n, precision, autoreset, noise, interval, tuple(chunks))
    if key not in _singles:
        out = []
        for r in range(M):
            b = World(device, oracle, n, noise_position=noise, **KW)
            b.policy.set_precision(precision)
            b.policy.native_interval = interval
            _fly(b, lambda w, c: roll(w, c, "fused", autoreset, reference=refs[r]), chunks)
            out.append(world_snapshot(b))
        _singles[key] = out
    return _singles[key]


def _assert_slices(snap, singles, ids, what=""):
    for r in range(M):
        if (ids == r).any():
            assert_same(snap, singles[r], rows=ids == r, what=f"{what} reference {r}")


# ------------------------------------------------------------------ 1 -----
SHAPES = [(n, p) for p in ("fp32", "bf16", "f16x2") for n in (1, 65, 130)] + [(4097, "fp32"), (70001, "fp32")]


@pytest.mark.parametrize("noise", [0.0, 0.01])
@pytest.mark.parametrize("autoreset", [True, False])
@pytest.mark.parametrize("n,precision", SHAPES)
def test_slices_equal_single_references(device, oracle, bank, refs, n, precision, autoreset, noise):
    ids = _ids(n)
    singles = _single_reference_worlds(device, oracle, refs, n, precision, autoreset, noise)
    for mode in ("fused", "chained"):
        a = World(device, oracle, n, noise_position=noise, **KW)
        a.policy.set_precision(precision)
        _fly(a, lambda w, c: roll(w, c, mode, autoreset, reference=bank, reference_ids=ids))
        snap = world_snapshot(a)
        _assert_slices(snap, singles, ids, f"{mode} n={n} {precision} autoreset={autoreset} noise={noise}")
        assert snap["fin_counts"].min() >= 1
        assert snap["epoch"][0] == sum(CHUNKS)
        if autoreset:
            assert np.array_equal(snap["track_steps"], np.full(n, sum(CHUNKS), np.uint32))
            if n >= 64:
                assert _ragged(a, ids), "the per-lane base was not exercised"
        else:           # an env flies its one episode and then sits still: a frozen env accumulates nothing
            assert snap["frozen"].all() and np.array_equal(snap["track_steps"], snap["fin_lengths"])
    # not vacuous: the three tables give three different flights (every env, from the first step on)
    if n >= 3:
        assert not np.array_equal(singles[0]["track_sq"], singles[1]["track_sq"])
        assert not np.array_equal(singles[1]["state"], singles[2]["state"])


# ------------------------------------------------------------------ 2 -----
@pytest.mark.parametrize("mode", ["fused", "chained"])
def test_one_table_is_the_reference(device, oracle, tables, refs, mode):
    n = 65
    one = l2f.ReferenceBank(device, [np.array(tables[1])])           # the list form
    assert (one.n_references, one.rows) == (1, LIMIT)
    a, b = World(device, oracle, n, **KW), World(device, oracle, n, **KW)
    _fly(a, lambda w, c: roll(w, c, mode, reference=one, reference_ids=np.zeros(n, np.int64)))
    _fly(b, lambda w, c: roll(w, c, mode, reference=refs[1]))
    assert_same(world_snapshot(a), world_snapshot(b), what=mode)
    assert a.env.finished_counts().min() >= 1


# ------------------------------------------------------------------ 3 -----
def test_recording_and_distiller(device, oracle, bank, refs):
    """The recording of the bank rollout is the per-reference recordings joined by id, bit for bit; and it goes through
    Distiller.step as it is: the loss equals, bit for bit, the loss of a recording JOINED on the device from the per-reference
    recordings (their columns copied into one trajectory through its tensor views)."""
    import torch
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.training import Distiller
    n, T = 65, sum(CHUNKS)
    ids = _ids(n)
    for mode in ("fused", "chained"):
        a = World(device, oracle, n, **KW)
        ta = a.vector.Trajectory(a.env, T)
        _fly(a, lambda w, c: roll(w, c, mode, trajectory=ta, reference=bank, reference_ids=ids))
        ra = ta.numpy()
        singles, trajs = [], []
        for r in range(M):
            b = World(device, oracle, n, **KW)
            tb = b.vector.Trajectory(b.env, T)
            _fly(b, lambda w, c: roll(w, c, mode, trajectory=tb, reference=refs[r]))
            rb = tb.numpy()
            own = ids == r
            assert_same_recording({k: v[:, own] for k, v in ra.items()}, {k: v[:, own] for k, v in rb.items()},
                                  f"{mode} reference {r}", frozen_too=True)
            singles.append(world_snapshot(b))
            trajs.append((b, tb))
        _assert_slices(world_snapshot(a), singles, ids, mode)
        assert (ra["done"] == 1).any() and (ra["done"] == 2).any()
        # the joined recording, made in trajectory 0 from the others' columns
        joined = trajs[0][1]
        views = joined.tensors()
        for r in (1, 2):
            cols = torch.tensor(np.flatnonzero(ids == r), device=views["obs"].device)
            src = trajs[r][1].tensors()
            for k in views:
                views[k].index_copy_(views[k].dim() - 1, cols, src[k].index_select(src[k].dim() - 1, cols))
        torch.cuda.synchronize()
        assert_same_recording(joined.numpy(), ra, what=f"{mode} joined", frozen_too=True)
        target = torch.zeros((T, 4, n), dtype=torch.float32, device=views["obs"].device)
        loss_a = Distiller(Raptor(device), lr=1e-3).step(ta, target=target)
        loss_j = Distiller(Raptor(device), lr=1e-3).step(joined, target=target)
        la, lj = np.asarray(loss_a.cpu()), np.asarray(loss_j.cpu())
        assert np.isfinite(la).all() and la[0] > 0 and np.array_equal(bits(la), bits(lj)), (mode, la, lj)


# ------------------------------------------------------------------ 4 -----
@pytest.mark.parametrize("n", [65, 70001])
def test_native_interval(device, oracle, bank, refs, n):
    ids = _ids(n)
    singles = _single_reference_worlds(device, oracle, refs, n, "fp32", True, 0.0, interval=4)
    for mode in ("fused", "chained"):
        a = World(device, oracle, n, **KW)
        a.policy.native_interval = 4
        _fly(a, lambda w, c: roll(w, c, mode, reference=bank, reference_ids=ids))
        _assert_slices(world_snapshot(a), singles, ids, f"{mode} n={n} interval 4")
    plain = _single_reference_worlds(device, oracle, refs, n, "fp32", True, 0.0)
    assert not np.array_equal(plain[0]["hidden"], singles[0]["hidden"])           # the interval is not a no-op


# ------------------------------------------------------------------ 5 -----
def test_policy_bank(device, oracle, weights, bank, refs):
    """192 envs, three blocks, two policies at intervals (1, 4), reference ids per lane"""
    from raptor_amd.policy_bank import PolicyBank
    from raptor_amd.tracking import reference_tracking_table
    n, P = 192, 2
    W = bank_weights(weights, P)
    pids = np.repeat(np.array([1, 0, 1], np.uint32), 64)
    ids = _ids(n)

    def fly(mode, **kw):
        w = World(device, oracle, n, **KW)
        pb = PolicyBank(device, W, native_interval=[1, 4])
        _fly(w, lambda w_, c: pb.fly(w_.vector, device, w_.env, w_.params, w_.state, w_.rng, c, pids, mode, True, **kw))
        return w, snapshot(w, pb.hidden(n))

    for mode in ("fused", "chained"):
        singles = [fly(mode, reference=refs[r])[1] for r in range(M)]
        a, snap = fly(mode, reference=bank, reference_ids=ids)
        _assert_slices(snap, singles, ids, f"policy bank {mode}")
        assert snap["fin_counts"].min() >= 1 and _ragged(a, ids)
    # evaluate: tracking_rmse [P, M] = the per-reference table of the single-reference evaluations joined
    def evaluate(**kw):
        w = World(device, oracle, n, **KW)
        pb = PolicyBank(device, W, native_interval=[1, 4])
        table = pb.evaluate(w.vector, device, w.env, w.params, w.state, w.rng, sum(CHUNKS), pids, **kw)
        return table, w.env.tracking_error()

    table, _ = evaluate(reference=bank, reference_ids=ids)
    assert table["tracking_rmse"].shape == (P, M) and table["tracking_rmse"].dtype == np.float64
    sq, steps = np.zeros(n, np.float32), np.zeros(n, np.uint32)
    for r in range(M):
        one, (sq_r, steps_r) = evaluate(reference=refs[r])
        assert one["tracking_rmse"].shape == (P,)
        sq[ids == r], steps[ids == r] = sq_r[ids == r], steps_r[ids == r]
    want = reference_tracking_table(sq, steps, ids, M, pids, P)
    assert np.isfinite(want).all() and (want > 0).all()
    assert np.array_equal(table["tracking_rmse"], want)


# ------------------------------------------------------------------ 6 -----
def test_graph_replay_follows_the_ids(device, oracle, tables):
    """From 25 steps on the chained mode replays a cached hipGraph: the same bank with other ids must not fly the old ones"""
    n, limit = 65, 30
    kw = dict(seed=6, episode_step_limit=limit, termination_position=0.6)
    big = l2f.ReferenceBank(device, np.stack([random_table(limit, 21 + r) for r in range(M)]))
    a = World(device, oracle, n, **kw)
    fresh = World(device, oracle, n, **kw)              # the same history, launch for launch, never through a graph
    for shift in (0, 1, 0):
        ids = _ids(n, shift)
        roll(a, 27, "chained", reference=big, reference_ids=ids)
        roll(fresh, 27, "fused", reference=big, reference_ids=ids)
        assert_same(world_snapshot(a), world_snapshot(fresh), what=f"shift {shift}")
    assert a.env.finished_counts().min() >= 1
    # not vacuous: the second run with the first run's ids is another flight
    stale = World(device, oracle, n, **kw)
    for shift in (0, 0, 0):
        roll(stale, 27, "fused", reference=big, reference_ids=_ids(n, shift))
    assert not np.array_equal(world_snapshot(stale)["state"], world_snapshot(a)["state"])


# ------------------------------------------------------------------ 7 -----
def test_refusals_enqueue_nothing(device, oracle, weights, tables, bank):
    from raptor_amd.policy_bank import PolicyBank
    n = 128
    ids = _ids(n)
    a = World(device, oracle, n, **KW)
    roll(a, 3, "fused", reference=bank, reference_ids=ids)
    tr = a.vector.Trajectory(a.env, 10)
    roll(a, 2, "fused", trajectory=tr, reference=bank, reference_ids=ids)
    pb = PolicyBank(device, bank_weights(weights, 2))
    pids = np.repeat(np.array([1, 0], np.uint32), 64)
    pb.fly(a.vector, device, a.env, a.params, a.state, a.rng, 2, pids, reference=bank, reference_ids=ids)

    def look():
        return dict(world_snapshot(a), bank_hidden=pb.hidden(n), recorded=np.full(n, len(tr)), recording=tr.numpy()["obs"].transpose(1, 0, 2))

    before, epoch = look(), a.rng.epoch
    assert epoch == 7 and len(tr) == 2

    def call(name, *args):
        with pytest.raises(RaptorQuadError) as e:
            _lib.call(name, *args)
        return e.value

    def attempt(who, mode, refs_h=bank._h, id_ptr=ids.ctypes.data, n_steps=5, flags=_lib.ROLLOUT_AUTORESET, traj=None, policy_ids=pids):
        if who == "policy":
            return call("rq_rollout_track_refs", device._h, a.env._h, a.params._h, a.state._h, a.policy._handle(device), a.rng._h,
                        n_steps, mode, flags, traj, refs_h, id_ptr)
        return call("rq_rollout_policies_track_refs", device._h, a.env._h, a.params._h, a.state._h, pb._h, policy_ids.ctypes.data,
                    a.rng._h, n_steps, mode, flags, traj, refs_h, id_ptr)

    short = l2f.ReferenceBank(device, np.array(tables[:, :LIMIT - 1]))
    other = l2f.ReferenceBank(l2f.Device(0), np.array(tables))
    far = ids.copy()
    far[77] = M
    mixed = pids.copy()
    mixed[5] = 0
    cases = []
    for who in ("policy", "policy bank"):
        for mode in (_lib.ROLLOUT_FUSED, _lib.ROLLOUT_CHAINED):
            cases += [("null bank", dict(refs_h=None), -1, "null reference bank"),
                      ("null ids", dict(id_ptr=None), -1, "null reference_id"),
                      ("fewer rows", dict(refs_h=short._h), -1, "fewer rows than episode_step_limit"),
                      ("another device", dict(refs_h=other._h), -5, "reference bank lives on another device"),
                      ("id out of range", dict(id_ptr=far.ctypes.data), -1, "env 77 names reference 3 of a bank of 3"),
                      ("no room in the recording", dict(traj=tr._h, n_steps=9), -1, "trajectory buffer too small"),
                      ("unknown flag", dict(flags=8), -1, "unknown flags")]
            cases = [c if len(c) == 6 else (who, mode) + c for c in cases]
        cases.append((who, 7, "unknown mode", {}, -1, "unknown mode"))
    cases.append(("policy bank", 0, "policy ids differ inside a block", dict(policy_ids=mixed), -1, "differ inside a 64-env block"))
    for who, mode, what, kw, status, words in cases:
        err = attempt(who, mode, **kw)
        assert err.status == status, (who, mode, what, err)
        assert words in str(err), (who, mode, what, err)
        assert_same(look(), before, what=f"{who} {mode} {what}")
        assert a.rng.epoch == epoch, what
    a.policy.set_sample_and_squash("mean")
    for mode in (_lib.ROLLOUT_FUSED, _lib.ROLLOUT_CHAINED):
        assert "SampleAndSquash" in str(attempt("policy", mode))
        assert_same(look(), before, what="SampleAndSquash")
    a.policy.set_sample_and_squash("off")
    # creation: refused before the device is touched
    h = C.c_void_p()
    bad = np.array(tables)
    bad[2, 4, 1] = np.inf
    with pytest.raises(ValueError):
        l2f.ReferenceBank(device, bad)
    for arr, m, rows, words in ((bad, M, LIMIT, "non-finite entry: table 2, row 4"), (np.array(tables), 0, LIMIT, "at least one table"),
                                (np.array(tables), M, 0, "at least one row"), (np.array(tables), 1 << 14, 1 << 14, "2^28")):
        assert words in str(call("rq_reference_bank_create", device._h, _lib.fptr(arr), m, rows, C.byref(h)))
        assert not h.value
    # a teacher bank still does not track (the Python surface says so before any call)
    with pytest.raises(ValueError, match="teacher_ids"):
        a.vector.rollout(device, a.env, a.params, a.state, a.policy, a.rng, 5, reference=bank, reference_ids=ids, teacher_ids=ids)
    assert_same(look(), before, what="after everything")
    assert a.rng.epoch == epoch
    roll(a, 3, "fused", reference=bank, reference_ids=ids)          # and it still flies
    assert a.rng.epoch == epoch + 3


# ------------------------------------------------------------------ 8 -----
@pytest.mark.parametrize("mode", ["fused", "chained"])
def test_two_launches_join(device, oracle, bank, mode):
    """7 + 12 against one launch of 19 (no pushes in between): the per-env base is loaded from memory by every launch, not carried"""
    n = 130
    ids = _ids(n)
    a, b = World(device, oracle, n, **KW), World(device, oracle, n, **KW)
    for w in (a, b):
        push(w, 0)
    _fly(a, lambda w, c: roll(w, c, mode, reference=bank, reference_ids=ids), pushes=False)
    _fly(b, lambda w, c: roll(w, c, mode, reference=bank, reference_ids=ids), chunks=(sum(CHUNKS),), pushes=False)
    assert_same(world_snapshot(a), world_snapshot(b), what=mode)
    assert a.env.finished_counts().min() >= 1 and len(np.unique(a.env.episode_steps()[:64])) >= 2
