"""The flight table on the GPU (rq_trajectory_flight_table; csrc/rq_flight_table.inc; raptor_amd.probing.flight_table).

The reference for every bit is the NumPy float32 restatement (tests/flight_reference.py) of ``traj.numpy()``.  Beside it: a recording
of one step and one whose tail is frozen for every env, output strides and memory modes, NaN written over everything the table
must not look at, the counts against ``probing.episode_steps``, the Python route, and the refusals.  The recordings are those of
tests/test_gpu_error_table.py (episode limit 9, terminations, step limits, frozen stretches, a bucket met again)."""
import ctypes as C

import numpy as np
import pytest

import flight_reference as FR
from distill_common import ASYNC, DEVICE, HOST, _lib, _record, same

pytestmark = pytest.mark.gpu

T = 40
SIZES = [1, 64, 65, 130]          # one env; a full wave; a wave and one env; three waves, the last ragged
SENTINEL = np.float32(-777.25)
COUNT_SENTINEL = np.uint32(0xABCD1234)
ALL_AGES = np.asarray([0, 2 ** 32 - 1], np.uint32)
EDGES = {"doubling": np.asarray([0, 1, 2, 4, 9], np.uint32),     # to the recordings' episode limit
         "no_age_0": np.asarray([1, 3, 9], np.uint32),           # age 0 is counted nowhere
         "short": np.asarray([0, 2, 5], np.uint32),              # ages 5 .. 8 are counted nowhere
         "all": ALL_AGES,
         "units": np.arange(33, dtype=np.uint32)}                # 32 unit buckets


def flight(traj, edges, start=None, tolerance=0.05, ld_out=None, memory=HOST):
    """-> (sum [B, 9, ld_out], peak [B, 3, ld_out], count [B, ld_out]), pre-filled with the sentinels; NumPy for HOST, fetched from
    torch tensors otherwise"""
    L = _lib()
    n = int(traj._env.N_ENVIRONMENTS)
    e = np.ascontiguousarray(edges, np.uint32)
    B, ld_out = e.size - 1, ld_out or n
    total, peak = np.full((B, 9, ld_out), SENTINEL, np.float32), np.full((B, 3, ld_out), SENTINEL, np.float32)
    count = np.full((B, ld_out), COUNT_SENTINEL, np.uint32)
    k = None if start is None else np.ascontiguousarray(start, np.uint32)
    ka = None if k is None else k.ctypes.data
    if memory == HOST:
        L.call("rq_trajectory_flight_table", traj._require("trajectory"), ka, tolerance, e.ctypes.data, B, L.fptr(total), L.fptr(peak),
               count.ctypes.data, ld_out, HOST)
        return total, peak, count
    import torch
    d = [torch.tensor(total, device="cuda"), torch.tensor(peak, device="cuda"), torch.tensor(count.view(np.int32), device="cuda")]
    torch.cuda.synchronize()
    L.call("rq_trajectory_flight_table", traj._require("trajectory"), ka, tolerance, e.ctypes.data, B, *(C.c_void_p(x.data_ptr()) for x in d),
           ld_out, memory)
    L.call("rq_device_synchronize", traj._env._device._h)
    return d[0].cpu().numpy(), d[1].cpu().numpy(), d[2].cpu().numpy().view(np.uint32)


def all_same(a, b):
    return all(same(x, y) for x, y in zip(a, b))


class Case:
    """One recording of n envs with every done code, fetched once, and a start count per env"""

    def __init__(self, device, oracle, n):
        self.n = n
        self.world, self.traj = _record(device, oracle, n, T, seed=500 + n, frozen=True)
        self.rec = self.traj.numpy()
        self.done = self.rec["done"]
        self.start = np.random.default_rng(n).integers(0, 9, n).astype(np.uint32)
        self._ref = {}

    def ref(self, which, started, tolerance):
        key = (which, started, tolerance)
        if key not in self._ref:
            r = self.rec
            self._ref[key] = FR.flight_table(r["obs"], r["act"], r["rew"], r["done"], EDGES[which], self.start if started else None, tolerance)
        return self._ref[key]


_cases = {}


@pytest.fixture(scope="module")
def cases(device, oracle):
    def get(n):
        if n not in _cases:
            _cases[n] = Case(device, oracle, n)
        return _cases[n]
    yield get
    _cases.clear()


# ------------------------------------------------------------------------------ 1. bit for bit against the restatement -
@pytest.mark.parametrize("tolerance", [0.0, 0.05])
@pytest.mark.parametrize("started", [False, True])
@pytest.mark.parametrize("which", sorted(EDGES))
@pytest.mark.parametrize("n", SIZES)
def test_the_table_is_the_restatement_bit_for_bit(cases, n, which, started, tolerance):
    c, edges = cases(n), EDGES[which]
    if n >= 64:          # the recording has what the table must get right: frozen steps, both kinds of end, a bucket met again
        k = FR.ages(c.done)
        assert (c.done == 4).any() and (c.done == 1).any() and (c.done == 2).any() and k.max() == 8
        assert (((c.done == 1) | (c.done == 2)).sum(0) >= 2).any()
    total, peak, count = flight(c.traj, edges, c.start if started else None, tolerance)
    ref = c.ref(which, started, tolerance)
    assert same(count, ref[2])
    assert same(peak, ref[1]), np.abs(peak - ref[1]).max()
    assert same(total, ref[0]), np.abs(total - ref[0]).max()
    assert np.isfinite(total).all() and np.isfinite(peak).all()
    if not started or which == "all":
        assert total[:, 0].any() and peak.any() and count.any()
    if tolerance == 0.0:          # every counted step off the setpoint is outside
        assert np.array_equal(total[:, 7] > 0, (total[:, 0] > 0))
    live = int((c.done != 4).sum())
    if which in ("all", "units") or (which == "doubling" and not started):
        assert int(count.sum()) == live
    elif n >= 64 and not started:
        assert int(count.sum()) < live          # these edges leave live steps out: age 0, or ages 5 .. 8


# ------------------------------------------------------------------------------ 2. one step; a tail frozen for every env -
def test_a_recording_of_one_step_and_one_whose_tail_is_frozen_for_every_env(device, oracle):
    from gpu_common import World
    n = 65
    w, traj = _record(device, oracle, n, 1, seed=9, frozen=True)
    assert len(traj) == 1
    r = traj.numpy()
    for which in ("doubling", "no_age_0", "all"):
        got = flight(traj, EDGES[which], None, 0.05)
        assert all_same(got, FR.flight_table(r["obs"], r["act"], r["rew"], r["done"], EDGES[which]))
    start = np.arange(n, dtype=np.uint32) % 5
    assert all_same(flight(traj, EDGES["short"], start, 0.05), FR.flight_table(r["obs"], r["act"], r["rew"], r["done"], EDGES["short"], start))
    # wholly without auto-reset: every env is frozen from its first episode end (step limit 9) to the end
    w = World(device, oracle, 130, seed=12, episode_step_limit=9, termination_position=0.6, domain_randomization=1)
    traj = w.vector.Trajectory(w.env, 20)
    w.policy.reset()
    w.vector.rollout(device, w.env, w.params, w.state, w.policy, w.rng, 20, "fused", autoreset=False, trajectory=traj)
    r = traj.numpy()
    assert (r["done"][10:] == 4).all() and (r["done"][0] != 4).all()
    for which in ("doubling", "units", "all"):
        got = flight(traj, EDGES[which], None, 0.05)
        assert all_same(got, FR.flight_table(r["obs"], r["act"], r["rew"], r["done"], EDGES[which]))
        assert int(got[2].sum()) == int((r["done"] != 4).sum())


# ------------------------------------------------------------------------------ 3. strides, memory modes, twice -
@pytest.mark.parametrize("n", [65, 130])
def test_strides_and_memory_modes_keep_the_bits_and_leave_the_columns_beyond_n(cases, n):
    c, edges = cases(n), EDGES["doubling"]
    want = flight(c.traj, edges, c.start, 0.05)
    assert all_same(want, c.ref("doubling", True, 0.05))
    for memory in (HOST, DEVICE, ASYNC):
        total, peak, count = flight(c.traj, edges, c.start, 0.05, ld_out=n + 7, memory=memory)
        assert same(total[:, :, :n], want[0]) and same(peak[:, :, :n], want[1]) and same(count[:, :n], want[2]), memory
        assert (total[:, :, n:] == SENTINEL).all() and (peak[:, :, n:] == SENTINEL).all() and (count[:, n:] == COUNT_SENTINEL).all(), memory
        assert all_same(flight(c.traj, edges, c.start, 0.05, memory=memory), want), memory
    assert all_same(flight(c.traj, edges, c.start, 0.05), want)                       # twice: the same bits
    assert not all_same(flight(c.traj, edges, None, 0.05), want)                      # other starts: another table
    assert all_same(flight(c.traj, edges, c.start, 0.05), want)                       # and the starts of before again


# ------------------------------------------------------------------------------ 4. what is not counted may hold anything -
def test_nan_on_frozen_steps_and_padding_columns_changes_no_bit(device, oracle):
    import torch
    n = 130
    w, traj = _record(device, oracle, n, T, seed=77, frozen=True)
    start = np.random.default_rng(5).integers(0, 9, n).astype(np.uint32)
    before = {which: flight(traj, EDGES[which], start, 0.05) for which in ("doubling", "short", "all")}
    t = traj.tensors()
    frozen = t["done"] == 4
    assert frozen[:, :n].any() and t["done"].shape[1] > n
    nan = float("nan")
    t["obs"][frozen[:, None, :].expand_as(t["obs"])] = nan
    t["act"][frozen[:, None, :].expand_as(t["act"])] = nan
    t["rew"][frozen] = nan
    t["obs"][:, :, n:], t["act"][:, :, n:], t["rew"][:, n:] = nan, nan, nan
    torch.cuda.synchronize()
    for which, want in before.items():
        got = flight(traj, EDGES[which], start, 0.05)
        assert all_same(got, want), which
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    # a live NaN stays in its own env's cells
    live = (~frozen[:, :n]).nonzero()[7]
    t["obs"][live[0], 0, live[1]] = nan
    torch.cuda.synchronize()
    got = flight(traj, ALL_AGES, start, 0.05)
    others = np.arange(n) != int(live[1])
    assert np.isnan(got[0][0, 0, int(live[1])]) and np.isfinite(got[1]).all()
    assert same(got[0][:, :, others], before["all"][0][:, :, others]) and same(got[1][:, :, others], before["all"][1][:, :, others])


# ------------------------------------------------------------------------------ 5. the counts -
@pytest.mark.parametrize("n", SIZES)
def test_counts_are_the_bucket_counts_of_episode_steps(cases, n):
    from raptor_amd import probing
    c = cases(n)
    for started in (False, True):
        k = probing.episode_steps(c.done, c.start if started else None)
        for which, edges in EDGES.items():
            count = flight(c.traj, edges, c.start if started else None, 0.05)[2]
            for b in range(len(edges) - 1):
                assert np.array_equal(count[b], ((k >= int(edges[b])) & (k < int(edges[b + 1]))).sum(0)), (which, b)


# ------------------------------------------------------------------------------ 6. through Python -
def test_flight_table_returns_the_c_abis_bits_as_numpy_or_tensors(cases):
    from raptor_amd import probing
    c, n, edges = cases(130), 130, EDGES["doubling"]
    want = flight(c.traj, edges, c.start, 0.05)
    tab = probing.flight_table(c.traj, edges=edges, start_steps=c.start, tolerance=0.05, device=False)
    assert isinstance(tab.sum, np.ndarray) and all_same((tab.sum, tab.peak, tab.count), want)
    dev = probing.flight_table(c.traj, edges=edges, start_steps=c.start, tolerance=0.05, device=True)
    assert dev.sum.is_cuda and dev.peak.is_cuda and dev.count.is_cuda and tuple(dev.sum.shape) == (4, 9, n)
    assert all_same((dev.sum.cpu().numpy(), dev.peak.cpu().numpy(), dev.count.cpu().numpy().view(np.uint32)), want)
    whole = probing.flight_table(c.traj)                    # edges=None: one bucket for every age; tensors when torch is present
    assert tuple(whole.sum.shape) == (1, 9, n) and same(whole.sum.cpu().numpy(), flight(c.traj, ALL_AGES)[0])
    groups = np.arange(n) % 5
    s64, c64 = want[0].astype(np.float64), want[2].astype(np.float64)
    for table in (tab, dev):
        got = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in table.by_group(groups, 5).items()}
        peaks = table.peak_by_group(groups, 5)
        peaks = peaks.cpu().numpy() if hasattr(peaks, "cpu") else peaks
        for g in range(5):
            m = groups == g
            cnt = c64[:, m].sum(1)
            assert np.allclose(got["rms_position"][g], np.sqrt(s64[:, 0, m].sum(1) / cnt), rtol=1e-14, atol=0)
            assert np.allclose(got["mean_tilt"][g], s64[:, 3, m].sum(1) / cnt, rtol=1e-12, atol=0)
            assert np.allclose(got["share_saturated"][g], s64[:, 6, m].sum(1) / (4 * cnt), rtol=1e-14, atol=0)
            assert np.allclose(got["mean_reward"][g], s64[:, 8, m].sum(1) / cnt, rtol=1e-12, atol=0)
            assert np.array_equal(peaks[g], want[1][:, :, m].max(2).astype(np.float64))
        age = table.by_age()["share_outside"]
        age = age.cpu().numpy() if hasattr(age, "cpu") else age
        assert np.allclose(age, s64[:, 7].sum(1) / c64.sum(1), rtol=1e-14, atol=0)


# ------------------------------------------------------------------------------ 7. the refusals -
def test_refusals_through_the_c_abi(cases, device):
    from raptor_amd._lib import RaptorQuadError
    L = _lib()
    c, n, good = cases(65), 65, EDGES["doubling"]
    tp = c.traj._require("trajectory")

    def refused(words, edges=good, n_buckets=None, ld_out=n, tolerance=0.05, memory=HOST, traj=tp, null=None):
        e = np.ascontiguousarray(edges, np.uint32)
        B = e.size - 1 if n_buckets is None else n_buckets
        rows = max(B, 1)
        total, peak = np.full((rows, 9, n), SENTINEL, np.float32), np.full((rows, 3, n), SENTINEL, np.float32)
        count = np.full((rows, n), COUNT_SENTINEL, np.uint32)
        args = [traj, c.start.ctypes.data, tolerance, e.ctypes.data, B, L.fptr(total), L.fptr(peak), count.ctypes.data, ld_out, memory]
        if null is not None:
            args[null] = None
        with pytest.raises(RaptorQuadError) as err:
            L.call("rq_trajectory_flight_table", *args)
        assert words in str(err.value) and err.value.status < 0, str(err.value)
        assert (total == SENTINEL).all() and (peak == SENTINEL).all() and (count == COUNT_SENTINEL).all(), words

    refused("null argument: trajectory", null=0)
    refused("null argument: age_edges", null=3)
    refused("null argument: sum", null=5)
    refused("null argument: peak", null=6)
    refused("null argument: count", null=7)
    empty = c.world.vector.Trajectory(c.world.env, 4)
    refused("the trajectory is empty", traj=empty._require("trajectory"))
    refused("ld_out", ld_out=n - 1)
    refused("n_buckets must be 1 .. 32, not 0", n_buckets=0)
    refused("n_buckets must be 1 .. 32, not 33", edges=np.arange(34), n_buckets=33)
    refused("age_edges must ascend strictly (age_edges[2] does not)", edges=[0, 2, 2, 5])
    refused("age_edges must ascend strictly (age_edges[1] does not)", edges=[3, 1])
    refused("tolerance must be finite and not negative", tolerance=-0.01)
    refused("tolerance must be finite and not negative", tolerance=float("nan"))
    refused("tolerance must be finite and not negative", tolerance=float("inf"))
    refused("memory must be 0, 1 or 2", memory=3)
    for memory in (DEVICE, ASYNC):          # device memory announced, host arrays given
        refused("sum lives on another device", memory=memory)
    # after all that the call works
    assert all_same(flight(c.traj, good, c.start, 0.05), c.ref("doubling", True, 0.05))
