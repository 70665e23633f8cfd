"""rq_trajectory_get_hidden / rq_trajectory_probe_moments on the GPU (raptor_amd/csrc/rq_probe.hip) against the numpy float64
reference of tests/probe_reference.py.

Recordings: episode_step_limit 7, T = 23, domain randomisation, termination_position 0.3 m against initial positions up to 0.5 m -
episodes end by termination and by the step limit at different steps inside a wave; one recording per env count with auto-reset and
one without (envs freeze: code 4).  The CPU oracle flies the same env: with seed 0 it shows codes 1, 2 and 4 at every env count
below and live lanes of different ages in one wave at every count from 63 up (test_preconditions asserts it on the GPU's own
recordings).

The bound of check 4, per element and bucket, against float64 moments of the GPU's own hidden bits:
    |S - S64| <= (2 * 64 * T + 2) * 2^-24 * A,   A = sum |z_i| |z_j|
one wave adds at most 64 T fp32 products to an element in some fixed order, each product and each add rounds at most once, flushes
at most double the number of adds, and the sum across waves is float64.  Derived, not measured; the largest error / bound seen is
printed per case (pytest -s) and, with RQ_PROBE_MOMENTS_JSON=<path> in the environment, written there: profiles/probe_moments.json
is such a file."""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import probe_reference as R
from gpu_common import World

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 130)
T = 23
HOST, DEVICE, ASYNC = 0, 1, 2
CURRENT, INITIAL = 0, 1
EDGES = (0, 1, 2, 4, 7)                      # ages run 0 .. 6 under the step limit of 7
SENTINEL = -12345.0
_RATIOS = []


def _lib():
    from raptor_amd import _lib as L
    return L


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _world(device, oracle, n):
    return World(device, oracle, n, seed=0, episode_step_limit=7, termination_position=0.3, domain_randomization=1)


def _recording(device, oracle, n, steps, autoreset):
    w = _world(device, oracle, n)
    traj = w.vector.Trajectory(w.env, steps)
    w.policy.reset()
    w.vector.rollout(device, w.env, w.params, w.state, w.policy, w.rng, steps, "fused", autoreset=autoreset, trajectory=traj)
    return SimpleNamespace(w=w, traj=traj, n=n, pol=w.policy, done=traj.numpy()["done"])


def hidden(traj, pol, n, memory=HOST):
    L = _lib()
    steps = len(traj)
    if memory == HOST:
        out = np.full((steps, n, 16), SENTINEL, np.float32)
        L.call("rq_trajectory_get_hidden", traj._require("trajectory"), pol._handle(), L.fptr(out), HOST)
        return out
    import torch
    out = torch.full((steps, n, 16), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    L.call("rq_trajectory_get_hidden", traj._require("trajectory"), pol._handle(), C.c_void_p(out.data_ptr()), memory)
    return out.cpu().numpy()


def int_targets(n, M, ld=None):
    """[M, ld] float32: integers with |y| <= 8 - every product and every sum of the y block is exact in fp32"""
    ld = ld or n
    env, m = np.meshgrid(np.arange(ld), np.arange(M))
    return ((env * 7 + m) % 17 - 8).astype(np.float32)


def probe(traj, pol, y, edges, memory=HOST):
    """y [M, ld_targets] -> (S [B, 32, 32] float64, counts [B] uint64) through the C ABI"""
    L = _lib()
    y = np.ascontiguousarray(y, np.float32)
    e = np.ascontiguousarray(edges, np.uint32)
    B = e.size - 1
    if memory == HOST:
        S, counts = np.full((B, 32, 32), SENTINEL), np.full(B, 77, np.uint64)
        L.call("rq_trajectory_probe_moments", traj._require("trajectory"), pol._handle(), L.fptr(y), y.shape[1], y.shape[0],
               e.ctypes.data, B, S.ctypes.data, counts.ctypes.data, HOST)
        return S, counts
    import torch
    yd = torch.from_numpy(y).cuda()
    S = torch.full((B, 32, 32), SENTINEL, dtype=torch.float64, device="cuda")
    counts = torch.full((B,), 77, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L.call("rq_trajectory_probe_moments", traj._require("trajectory"), pol._handle(), C.c_void_p(yd.data_ptr()), y.shape[1], y.shape[0],
           e.ctypes.data, B, C.c_void_p(S.data_ptr()), C.c_void_p(counts.data_ptr()), memory)
    if memory == ASYNC:
        _lib().call("rq_device_synchronize", traj._env._device._h)
    return S.cpu().numpy(), counts.cpu().numpy().astype(np.uint64)


def check_against_reference(case, h, y, edges, S, counts, what, steps=None):
    """checks 2, 3 and 4: counts and the integer block exactly, every element within the derived bound"""
    n, M = case.n, y.shape[0]
    steps = steps or len(case.traj)
    ref = R.moments(h, case.done, y[:, :n].T, edges)
    assert counts.dtype == np.uint64 and np.array_equal(counts, ref["counts"]), (what, counts, ref["counts"])
    assert np.array_equal(S[:, 0, 0], counts.astype(np.float64)), what
    assert np.array_equal(S, np.transpose(S, (0, 2, 1))), what              # the full symmetric matrix
    assert (S[:, 17 + M:, :] == 0).all(), what                              # the zero padding of z
    if np.array_equal(y, np.round(y)) and np.abs(y).max() <= 8:
        assert np.abs(ref["S"][:, 17:, 17:]).max() < 2 ** 24
        assert np.array_equal(S[:, 17:, 17:], ref["S"][:, 17:, 17:]), what  # the y-y block
        assert np.array_equal(S[:, 0, 17:], ref["S"][:, 0, 17:]), what      # the row sum y
    err = np.abs(S - ref["S"])
    bound = (2 * 64 * steps + 2) * 2.0 ** -24 * ref["A"]
    assert (err[bound == 0] == 0).all(), what
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"probe moments {what}: n={n} T={steps} M={M} buckets={len(edges) - 1} max error/bound = {ratio:.3e}")
    _RATIOS.append(dict(what=what, n=int(n), T=int(steps), M=int(M), buckets=len(edges) - 1, max_error_over_bound=ratio))
    assert (err <= bound).all(), (what, ratio)
    return ref


@pytest.fixture(scope="module")
def cases(device, oracle):
    """(n, autoreset) -> the recording, with the GPU's own hidden bits; made once, never changed"""
    out = {}
    for n in NS:
        for auto in (True, False):
            c = _recording(device, oracle, n, T, auto)
            c.h = hidden(c.traj, c.pol, n)
            out[n, auto] = c
    yield out
    path = os.environ.get("RQ_PROBE_MOMENTS_JSON")             # where a run that refreshes profiles/probe_moments.json wants the figures
    if path and _RATIOS:
        worst = max(r["max_error_over_bound"] for r in _RATIOS)
        json.dump(dict(bound="|S - S64| <= (2 * 64 * T + 2) * 2^-24 * sum |z_i| |z_j|, per element and bucket",
                       largest_error_over_bound=worst, cases=_RATIOS), open(path, "w"), indent=1)


@pytest.mark.parametrize("n", NS)
def test_preconditions(cases, n):
    """no test below passes vacuously: the recordings hold every done code and waves whose live lanes differ in age"""
    auto, frozen = cases[n, True], cases[n, False]
    codes = set(np.unique(auto.done)) | set(np.unique(frozen.done))
    assert {1, 2, 4} <= codes, codes
    assert (frozen.done == 4).any()
    assert frozen.done.shape == (T, n)
    if n >= 63:
        age, _ = R.ages(auto.done)
        mixed = [t for t in range(T) for w0 in range(0, n, 64) if len(set(age[t, w0:w0 + 64][age[t, w0:w0 + 64] >= 0])) > 1]
        assert mixed, "no step at which two live lanes of one wave have different ages"


@pytest.mark.parametrize("n", NS)
def test_get_hidden(cases, oracle, weights, n):
    from distill_common import forward
    h0 = weights[2000:2016]
    for auto in (True, False):
        c = cases[n, auto]
        h, done = c.h, c.done
        assert h.shape == (T, n, 16) and same(h[0], np.broadcast_to(h0, (n, 16)))
        ended = (done[:-1] == 1) | (done[:-1] == 2)
        assert same(h[1:][ended], np.broadcast_to(h0, (int(ended.sum()), 16)))
        frozen = done[:-1] == 4
        assert same(h[1:][frozen], h[:-1][frozen])
        # the state after a step that neither ends nor is frozen is the GRU's: the CPU oracle's step from the same bits
        t = 0 if auto else int(np.argmax((done[:-1] == 0).any(axis=1)))
        rec = c.traj.numpy()
        nxt = h[t].copy()
        oracle.actor_batch_step(weights, np.ascontiguousarray(rec["obs"][t]), nxt)
        run = done[t] == 0
        assert run.any() or n == 1
        assert np.abs(nxt[run] - h[t + 1][run]).max(initial=0.0) < 2e-5
        # the saved state is the forward's own: its actions are what they were before the call, and the call gives the same bits
        # whether it reuses that forward's state or ran its own
        a0 = forward(c.traj, c.pol, INITIAL)[:, :, :n]              # (the call writes the envs' columns only)
        assert same(hidden(c.traj, c.pol, n), h)
        assert same(forward(c.traj, c.pol, INITIAL)[:, :, :n], a0)
        assert same(hidden(c.traj, c.pol, n, DEVICE), h)


@pytest.mark.parametrize("auto", (True, False))
@pytest.mark.parametrize("n", NS)
def test_counts_exact_block_and_bound(cases, n, auto):
    c = cases[n, auto]
    ld_t = n + 3 if n in (1, 65) else n                          # ld_targets > n_envs
    y = int_targets(n, 5, ld_t)
    S, counts = probe(c.traj, c.pol, y, EDGES)
    ref = check_against_reference(c, c.h, y, EDGES, S, counts, f"shipped policy, autoreset={auto}")
    live = int((c.done != 4).sum())
    assert int(counts.sum()) == live and live > 0                # the edges cover every age a step limit of 7 allows
    if n >= 63:
        assert (ref["counts"] > 0).all()
    # real-valued targets: the bound holds for them as it does for the integers
    yr = np.random.default_rng(n).standard_normal((3, n)).astype(np.float32)
    S, counts = probe(c.traj, c.pol, yr, EDGES)
    check_against_reference(c, c.h, yr, EDGES, S, counts, f"real targets, autoreset={auto}")


EDGE_CASES = {
    "one bucket": ([0, 2 ** 31], 4),
    "one bucket per age": (list(range(8)), 4),
    "32 buckets": (list(range(33)), 4),
    "dropped ages": ([2, 5], 4),
    "first edge above 0, gaps to the right": ([1, 3, 6], 4),
    "M = 1": (list(EDGES), 1),
    "M = 15": (list(EDGES), 15),
}


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_bucket_and_target_edges(cases, name):
    edges, M = EDGE_CASES[name]
    for n, auto in ((130, True), (65, False)):
        c = cases[n, auto]
        y = int_targets(n, M)
        S, counts = probe(c.traj, c.pol, y, edges)
        ref = check_against_reference(c, c.h, y, edges, S, counts, name)
        if name == "one bucket":
            assert int(counts[0]) == int((c.done != 4).sum())
        if name == "32 buckets":
            assert (counts[7:] == 0).all() and (S[7:] == 0).all() and (counts[:7] > 0).all()
        if name == "dropped ages":
            assert 0 < int(counts[0]) < int((c.done != 4).sum())
        assert (ref["counts"] > 0).any()


def test_one_step(device, oracle):
    c = _recording(device, oracle, 65, 1, True)
    h = hidden(c.traj, c.pol, 65)
    assert h.shape == (1, 65, 16)
    y = int_targets(65, 4)
    for edges in ([0, 1], [0, 1, 2], [1, 2]):
        S, counts = probe(c.traj, c.pol, y, edges)
        check_against_reference(c, h, y, edges, S, counts, "T = 1", steps=1)
        assert counts.tolist() == ([65] + [0] * (len(edges) - 2) if edges[0] == 0 else [0])


def test_garbage_outside_the_live_set(cases):
    """NaN in the target columns >= n_envs, device memory: the moments are finite and the same bits"""
    for n, auto in ((65, True), (65, False), (1, True)):
        c = cases[n, auto]
        clean = int_targets(n, 5)
        dirty = np.full((5, 128), np.nan, np.float32)
        dirty[:, :n] = clean
        S0, c0 = probe(c.traj, c.pol, clean, EDGES)
        for memory in (DEVICE, ASYNC):
            S1, c1 = probe(c.traj, c.pol, dirty, EDGES, memory)
            assert np.isfinite(S1).all() and same(S1, S0) and np.array_equal(c1, c0)


def test_determinism(cases):
    from distill_common import loss_grad
    for n, auto in ((130, True), (130, False)):
        c = cases[n, auto]
        y = np.random.default_rng(5).standard_normal((6, n)).astype(np.float32)
        S0, c0 = probe(c.traj, c.pol, y, EDGES)
        S1, c1 = probe(c.traj, c.pol, y, EDGES)
        assert same(S0, S1) and np.array_equal(c0, c1)
        target = np.zeros((T, 4, n), np.float32)
        for start in (CURRENT, INITIAL):          # the first replaces the saved state (the probe redoes the forward), the second leaves one to reuse
            c.pol.reset()
            loss_grad(c.traj, c.pol, target, start)
            S2, c2 = probe(c.traj, c.pol, y, EDGES)
            assert same(S0, S2) and np.array_equal(c0, c2)
            assert same(hidden(c.traj, c.pol, n), c.h)


def test_refusals(cases, device):
    import raptor_amd.l2f as l2f
    from raptor_amd._lib import RaptorQuadError
    from raptor_amd.foundation_policy import Raptor
    L = _lib()
    c = cases[65, True]
    n, traj = 65, c.traj
    pol = Raptor(device)
    pol.reset()
    y = int_targets(n, 3)
    e = np.asarray(EDGES, np.uint32)
    S, counts = np.full((4, 32, 32), SENTINEL), np.full(4, 77, np.uint64)
    out = np.full((T, n, 16), SENTINEL, np.float32)

    def moments(y=y, ld=n, M=3, edges=e, B=4, S=S, counts=counts, pol=pol, traj=traj, memory=HOST):
        L.call("rq_trajectory_probe_moments", traj._require("trajectory") if traj is not None else None,
               pol._handle() if pol is not None else None, None if y is None else L.fptr(y), ld, M,
               None if edges is None else edges.ctypes.data, B, None if S is None else S.ctypes.data,
               None if counts is None else counts.ctypes.data, memory)

    def get(pol=pol, traj=traj, out=out, memory=HOST):
        L.call("rq_trajectory_get_hidden", traj._require("trajectory") if traj is not None else None,
               pol._handle() if pol is not None else None, None if out is None else L.fptr(out), memory)

    def refused(fn, words):
        with pytest.raises(RaptorQuadError) as err:
            fn()
        assert words in str(err.value), str(err.value)
        assert (S == SENTINEL).all() and (counts == 77).all() and (out == SENTINEL).all()      # the outputs are untouched

    for prec in ("bf16", "f16x2"):
        pol.set_precision(prec)
        refused(moments, "fp32 policy only")
        refused(get, "fp32 policy only")
    pol.set_precision("fp32")
    pol.set_standardize(np.zeros(22, np.float32), np.ones(22, np.float32))
    refused(moments, "Standardize")
    refused(get, "Standardize")
    pol.set_standardize(None)
    pol.set_squash(True)
    refused(moments, "SampleAndSquash")
    refused(get, "SampleAndSquash")
    pol.set_squash(False)
    pol.native_interval = 4
    refused(moments, "native interval")
    refused(get, "native interval")
    pol.native_interval = 1
    foreign = Raptor(l2f.Device(0))                              # another engine device object (same GPU)
    foreign.reset()
    foreign._handle()
    refused(lambda: moments(pol=foreign), "another device")
    refused(lambda: get(pol=foreign), "another device")
    for M in (0, 16):
        refused(lambda: moments(M=M), "n_targets")
    for B in (0, 33):
        refused(lambda: moments(B=B, edges=np.arange(40, dtype=np.uint32)), "n_buckets")
    for bad in ([0, 1, 1, 4, 7], [0, 2, 1, 4, 7], [7, 4, 2, 1, 0]):
        refused(lambda: moments(edges=np.asarray(bad, np.uint32)), "age_edges")
    refused(lambda: moments(ld=n - 1), "ld_targets")
    nan = y.copy()
    nan[2, n - 1] = np.nan
    refused(lambda: moments(y=nan), "finite")
    refused(lambda: moments(y=None), "targets")
    refused(lambda: moments(edges=None), "age_edges")
    refused(lambda: moments(S=None), "moments")
    refused(lambda: moments(counts=None), "counts")
    refused(lambda: moments(pol=None), "null")
    refused(lambda: moments(traj=None), "null")
    refused(lambda: get(out=None), "out")
    refused(lambda: get(pol=None), "null")
    refused(lambda: moments(memory=3), "memory")
    refused(lambda: get(memory=-1), "memory")
    # device memory is announced, host memory is given
    refused(lambda: moments(memory=DEVICE), "another device")
    refused(lambda: get(memory=DEVICE), "another device")
    empty = c.w.vector.Trajectory(c.w.env, 4)
    refused(lambda: moments(traj=empty), "empty")
    refused(lambda: get(traj=empty), "empty")
    moments()                                                    # and after all that it works, to the same bits as the recording's policy
    get()
    S_ref, c_ref = probe(traj, c.pol, y, EDGES)
    assert same(S, S_ref) and np.array_equal(counts, c_ref) and same(out, c.h)


def test_new_weights_rerun_the_forward(device, oracle, weights):
    from distill_common import _perturbed
    c = _recording(device, oracle, 130, T, True)
    y = int_targets(130, 5)
    h0 = hidden(c.traj, c.pol, 130)
    S0, c0 = probe(c.traj, c.pol, y, EDGES)
    check_against_reference(c, h0, y, EDGES, S0, c0, "before set_weights")
    c.pol.set_weights(_perturbed(weights, 3))
    S1, c1 = probe(c.traj, c.pol, y, EDGES)                      # no get_hidden in between: this call must notice the new weights
    h1 = hidden(c.traj, c.pol, 130)
    assert not same(h1, h0) and np.array_equal(c1, c0) and not same(S1, S0)
    assert same(h1[0], np.broadcast_to(c.pol.weights[2000:2016], (130, 16)))
    check_against_reference(c, h1, y, EDGES, S1, c1, "after set_weights")


@pytest.mark.parametrize("n", (65, 130))
def test_random_weights_meet_the_bound(cases, device, n):
    """the bound does not depend on the checkpoint: weights drawn at random, hidden states spread over (-1, 1)"""
    from raptor_amd.foundation_policy import Raptor
    rng = np.random.default_rng(40 + n)
    w = (rng.standard_normal(2084) * 0.5).astype(np.float32)
    w[2000:2016] = rng.uniform(-0.9, 0.9, 16).astype(np.float32)
    pol = Raptor(device, weights=w)
    pol.reset()
    for auto in (True, False):
        c = cases[n, auto]
        h = hidden(c.traj, pol, n)
        assert np.isfinite(h).all() and np.abs(h).max() <= 1.0 and h.std() > 0.2
        for y in (int_targets(n, 15), rng.standard_normal((7, n)).astype(np.float32)):
            S, counts = probe(c.traj, pol, y, EDGES)
            check_against_reference(c, h, y, EDGES, S, counts, f"random weights, autoreset={auto}")
        assert same(hidden(c.traj, c.pol, n), c.h)               # and the recording's own policy gets its own state back
