"""rq_trajectory_probe_moments_timed / rq_trajectory_wrench_targets on the GPU (raptor_amd/csrc/rq_probe.hip) against the numpy
references of tests/probe_timed_reference.py.

Recordings: those of tests/test_gpu_probe.py - episode_step_limit 7, T = 23, termination_position 0.3, domain randomisation, seed 0,
one auto-reset and one freezing recording per env count (test_preconditions asserts on the GPU's own recordings that codes 1, 2 and 4
occur and that one wave holds live lanes of different ages from 63 envs up).

The bound of check 1, per element and bucket, against float64 moments of the GPU's own hidden bits, is the untimed one:
    |S - S64| <= (2 * 64 * T + 2) * 2^-24 * A,   A = sum |z_i| |z_j|
one wave adds at most 64 T fp32 products to an element in some fixed order, each product and each add rounds at most once, flushes
at most double the number of adds, and the sum across waves is float64; a target that changes per step changes no count of
roundings.  The largest error / bound is printed per case (pytest -s).  The wrench targets are compared bit for bit."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import probe_reference as R
import probe_timed_reference as RT
from gpu_common import World

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 130)
T = 23
HOST, DEVICE, ASYNC = 0, 1, 2
CURRENT, INITIAL = 0, 1
RELATIVE, ABSOLUTE = 0, 1
EDGES = (0, 1, 2, 4, 7)                      # ages run 0 .. 6 under the step limit of 7
SENTINEL = -12345.0
P_MASS, P_ROTOR_X = 0, 4                     # rq_param_field


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


def _record(w, device, steps, autoreset):
    traj = w.vector.Trajectory(w.env, steps)
    w.vector.rollout(device, w.env, w.params, w.state, w.policy, w.rng, steps, "fused", autoreset=autoreset, trajectory=traj)
    return traj


def _recording(device, oracle, n, steps, autoreset):
    w = _world(device, oracle, n)
    w.policy.reset()
    traj = _record(w, device, steps, autoreset)
    return SimpleNamespace(w=w, traj=traj, n=n, pol=w.policy, done=traj.numpy()["done"])


def hidden(traj, pol, n):
    L = _lib()
    out = np.full((len(traj), n, 16), SENTINEL, np.float32)
    L.call("rq_trajectory_get_hidden", traj._require("trajectory"), pol._handle(), L.fptr(out), HOST)
    return out


def int_targets(n, M, ld=None, steps=T):
    """[T, M, ld] float32: ((5 t + 7 env + m) mod 17) - 8 - integers with |y| <= 8, every product and sum of the y block exact"""
    ld = ld or n
    t, m, env = np.meshgrid(np.arange(steps), np.arange(M), np.arange(ld), indexing="ij")
    return ((5 * t + 7 * env + m) % 17 - 8).astype(np.float32)


def _moments_call(name, traj, pol, y, ld, M, edges, memory):
    L = _lib()
    y = np.ascontiguousarray(y, np.float32)
    e = np.ascontiguousarray(edges, np.uint32)
    B = e.size - 1
    if memory == HOST:
        S, counts = np.full((B, 32, 32), SENTINEL), np.full(B, 77, np.uint64)
        L.call(name, traj._require("trajectory"), pol._handle(), L.fptr(y), ld, M, e.ctypes.data, B, S.ctypes.data, counts.ctypes.data, HOST)
        return S, counts
    import torch
    yd = torch.from_numpy(y).cuda()
    S = torch.full((B, 32, 32), SENTINEL, dtype=torch.float64, device="cuda")
    counts = torch.full((B,), 77, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L.call(name, traj._require("trajectory"), pol._handle(), C.c_void_p(yd.data_ptr()), ld, M, e.ctypes.data, B,
           C.c_void_p(S.data_ptr()), C.c_void_p(counts.data_ptr()), memory)
    if memory == ASYNC:
        L.call("rq_device_synchronize", traj._env._device._h)
    return S.cpu().numpy(), counts.cpu().numpy().astype(np.uint64)


def probe_timed(traj, pol, y, edges, memory=HOST):
    """y [T, M, ld_targets] -> (S [B, 32, 32] float64, counts [B] uint64) through the C ABI"""
    return _moments_call("rq_trajectory_probe_moments_timed", traj, pol, y, y.shape[2], y.shape[1], edges, memory)


def probe_untimed(traj, pol, y, edges, memory=HOST):
    """y [M, ld_targets]: rq_trajectory_probe_moments"""
    return _moments_call("rq_trajectory_probe_moments", traj, pol, y, y.shape[1], y.shape[0], edges, memory)


def check_against_reference(case, h, y, edges, S, counts, what, steps=None):
    """counts and the integer block exactly, every element within the derived bound"""
    n, M = case.n, y.shape[1]
    steps = steps or len(case.traj)
    ref = RT.moments_timed(h, case.done, y[:, :, :n].transpose(0, 2, 1), edges)
    assert counts.dtype == np.uint64 and np.array_equal(counts, ref["counts"]), (what, counts, ref["counts"])
    assert np.array_equal(S[:, 0, 0], counts.astype(np.float64)), what
    assert np.array_equal(S, np.transpose(S, (0, 2, 1))), what              # the full symmetric matrix
    assert (S[:, 17 + M:, :] == 0).all(), what                              # the zero padding of z
    if np.array_equal(y, np.round(y)) and np.abs(y).max() <= 8:
        assert np.abs(ref["S"][:, 17:, 17:]).max() < 2 ** 24
        assert np.array_equal(S[:, 17:, 17:], ref["S"][:, 17:, 17:]), what  # the y-y block
        assert np.array_equal(S[:, 0, 17:], ref["S"][:, 0, 17:]), what      # the row sums of y
    err = np.abs(S - ref["S"])
    bound = (2 * 64 * steps + 2) * 2.0 ** -24 * ref["A"]
    assert (err[bound == 0] == 0).all(), what
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"timed probe moments {what}: n={n} T={steps} M={M} buckets={len(edges) - 1} max error/bound = {ratio:.3e}")
    assert (err <= bound).all(), (what, ratio)
    return ref


@pytest.fixture(scope="module")
def cases(device, oracle):
    """(n, autoreset) -> the recording, with the GPU's own hidden bits; made once, never changed"""
    lib = _lib().load()
    assert hasattr(lib, "rq_trajectory_probe_moments_timed") and hasattr(lib, "rq_trajectory_wrench_targets")
    out = {}
    for n in NS:
        for auto in (True, False):
            c = _recording(device, oracle, n, T, auto)
            c.h = hidden(c.traj, c.pol, n)
            out[n, auto] = c
    return out


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


# ------------------------------------------------------------------------------ 1: against float64 --
@pytest.mark.parametrize("auto", (True, False))
@pytest.mark.parametrize("n", NS)
def test_counts_exact_block_and_bound(cases, n, auto):
    c = cases[n, auto]
    ld_t = n + 3 if n in (1, 65) else n                          # ld_targets > n_envs
    y = int_targets(n, 5, ld_t)
    assert not np.array_equal(y[0], y[1])                        # the targets do change over time
    S, counts = probe_timed(c.traj, c.pol, y, EDGES)
    ref = check_against_reference(c, c.h, y, EDGES, S, counts, f"integer targets, autoreset={auto}")
    live = int((c.done != 4).sum())
    assert int(counts.sum()) == live and live > 0                # the edges cover every age a step limit of 7 allows
    if n >= 63:
        assert (ref["counts"] > 0).all()
    yr = np.random.default_rng(n).standard_normal((T, 3, n)).astype(np.float32)
    S, counts = probe_timed(c.traj, c.pol, yr, EDGES)
    check_against_reference(c, c.h, yr, EDGES, S, counts, f"real targets, autoreset={auto}")


# ------------------------------------------------------------------------------ 2: constant in time = the untimed call --
@pytest.mark.parametrize("auto", (True, False))
@pytest.mark.parametrize("n", NS)
def test_constant_targets_give_the_untimed_bits(cases, n, auto):
    c = cases[n, auto]
    y = np.random.default_rng(100 + n).standard_normal((6, n)).astype(np.float32)
    yt = np.ascontiguousarray(np.broadcast_to(y, (T, 6, n)))
    for memory in (HOST, DEVICE):
        S0, c0 = probe_untimed(c.traj, c.pol, y, EDGES, memory)
        S1, c1 = probe_timed(c.traj, c.pol, yt, EDGES, memory)
        assert same(S0, S1) and np.array_equal(c0, c1), (n, auto, memory)
    assert (c0 > 0).any()


# ------------------------------------------------------------------------------ 3: edges --
EDGE_CASES = {
    "M = 1": (list(EDGES), 1),
    "M = 15": (list(EDGES), 15),
    "one bucket": ([0, 2 ** 31], 4),
    "32 buckets": (list(range(33)), 4),
    "dropped ages": ([2, 5], 4),
    "first edge above 0": ([1, 3, 6], 4),
}


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_bucket_and_target_edges(cases, name):
    edges, M = EDGE_CASES[name]
    for n, auto in ((130, True), (65, False)):
        c = cases[n, auto]
        y = int_targets(n, M)
        S, counts = probe_timed(c.traj, c.pol, y, edges)
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
    y = int_targets(65, 4, steps=1)
    for edges in ([0, 1], [0, 1, 2], [1, 2]):
        S, counts = probe_timed(c.traj, c.pol, y, edges)
        check_against_reference(c, h, y, edges, S, counts, "T = 1", steps=1)
        assert counts.tolist() == ([65] + [0] * (len(edges) - 2) if edges[0] == 0 else [0])


# ------------------------------------------------------------------------------ 4: garbage --
def test_garbage_outside_the_live_set(cases):
    """NaN in device memory where no sample is - the columns >= n_envs, every frozen step, every step whose age is dropped -
    gives the bits of clean targets and a finite result"""
    from raptor_amd._lib import RaptorQuadError
    seen_frozen = seen_dropped = False
    for n, auto in ((65, True), (65, False), (130, False), (1, True)):
        c = cases[n, auto]
        age, live = R.ages(c.done)
        for edges in (EDGES, (2, 5)):
            clean = int_targets(n, 5)
            S0, c0 = probe_timed(c.traj, c.pol, clean, edges)
            assert np.isfinite(S0).all()
            dirty = np.full((T, 5, 128 if n <= 128 else 192), np.nan, np.float32)             # columns >= n
            dirty[:, :, :n] = clean
            nowhere = ~live | (R.buckets(age, edges) < 0)                                     # frozen steps, dropped ages
            dirty[:, :, :n][np.broadcast_to(nowhere[:, None, :], (T, 5, n))] = np.nan
            seen_frozen |= bool((~live).any())
            seen_dropped |= bool((live & nowhere).any())
            for memory in (DEVICE, ASYNC):
                S1, c1 = probe_timed(c.traj, c.pol, dirty, edges, memory)
                assert np.isfinite(S1).all() and same(S1, S0) and np.array_equal(c1, c0), (n, auto, edges, memory)
    assert seen_frozen and seen_dropped
    # host memory: a NaN in an env's column is refused, at a frozen step too
    c = cases[65, False]
    t, i = np.argwhere(c.done == 4)[-1]
    y = int_targets(65, 5)
    y[t, 3, i] = np.nan
    with pytest.raises(RaptorQuadError) as err:
        probe_timed(c.traj, c.pol, y, EDGES)
    msg = str(err.value)
    assert "finite" in msg and f"step {t}" in msg and "target 3" in msg and f"env {i}" in msg, msg


# ------------------------------------------------------------------------------ 5: determinism --
def test_determinism(cases):
    from distill_common import loss_grad
    for n, auto in ((130, True), (130, False)):
        c = cases[n, auto]
        y = np.random.default_rng(5).standard_normal((T, 6, n)).astype(np.float32)
        S0, c0 = probe_timed(c.traj, c.pol, y, EDGES)
        S1, c1 = probe_timed(c.traj, c.pol, y, EDGES)
        assert same(S0, S1) and np.array_equal(c0, c1)
        target = np.zeros((T, 4, n), np.float32)
        for start in (CURRENT, INITIAL):          # the first replaces the saved state (the probe redoes the forward), the second leaves one to reuse
            c.pol.reset()
            loss_grad(c.traj, c.pol, target, start)
            S2, c2 = probe_timed(c.traj, c.pol, y, EDGES)
            assert same(S0, S2) and np.array_equal(c0, c2)
            assert same(hidden(c.traj, c.pol, n), c.h)


# ------------------------------------------------------------------------------ 7: wrench targets --
def wrench_tables(units_scale=1.0):
    """3 tables of 7 rows, distinct non-zero entries in all six columns, |entry| <= 0.05"""
    v = (np.arange(3 * 7 * 6, dtype=np.float32).reshape(3, 7, 6) + 1.0) / np.float32(3 * 7 * 6) * np.float32(0.05)
    v[:, :, 1::2] *= -1.0
    assert len(np.unique(v)) == v.size and (v != 0).all() and np.abs(v).max() <= 0.05
    return (v * np.float32(units_scale)).astype(np.float32)


def index_tables():
    """one table whose row k holds k in column 0"""
    t = np.zeros((1, 7, 6), np.float32)
    t[0, :, 0] = np.arange(7)
    return t


def wrench_call(traj, bank, ids, params, start, units, n, ld=None, memory=HOST):
    """-> out [T, 6, ld] as the C ABI leaves it in an array full of sentinels"""
    L = _lib()
    ld = ld or n
    steps = len(traj)
    ia = None if ids is None else np.ascontiguousarray(ids, np.uint32)
    ka = None if start is None else np.ascontiguousarray(start, np.uint32)
    args = (traj._require("trajectory"), bank._h, None if ia is None else ia.ctypes.data, params._require("VectorParameters"),
            None if ka is None else ka.ctypes.data, units)
    if memory == HOST:
        out = np.full((steps, 6, ld), SENTINEL, np.float32)
        L.call("rq_trajectory_wrench_targets", *args, L.fptr(out), ld, HOST)
        return out
    import torch
    out = torch.full((steps, 6, ld), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    L.call("rq_trajectory_wrench_targets", *args, C.c_void_p(out.data_ptr()), ld, memory)
    if memory == ASYNC:
        L.call("rq_device_synchronize", traj._env._device._h)
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def flights(device, oracle):
    """n -> a world flown under a relative wrench schedule (ids = env mod 3): an unrecorded 3-step rollout, then an auto-reset
    recording; a second world with a freezing recording and, begun on the envs it left frozen, an auto-reset one.  Every recording
    comes with the episode step counts the engine reported right before and right after it."""
    import raptor_amd.l2f as l2f
    out = {}
    for n in (65, 130):
        ids = (np.arange(n) % 3).astype(np.uint32)
        recs = {}
        for kind in ("auto", "freezing"):
            w = _world(device, oracle, n)
            bank = l2f.WrenchBank(device, wrench_tables())
            w.env.set_wrench_schedule(bank, ids)
            w.policy.reset()
            w.vector.rollout(device, w.env, w.params, w.state, w.policy, w.rng, 3, "fused", autoreset=True)
            start = w.env.episode_steps()
            traj = _record(w, device, T, kind == "auto")
            recs[kind] = SimpleNamespace(w=w, traj=traj, n=n, pol=w.policy, done=traj.numpy()["done"], start=start,
                                         end=w.env.episode_steps(), bank=bank, ids=ids)
            if kind == "freezing":
                start2 = w.env.episode_steps()
                traj2 = _record(w, device, T, True)
                recs["thawed"] = SimpleNamespace(w=w, traj=traj2, n=n, pol=w.policy, done=traj2.numpy()["done"], start=start2,
                                                 end=w.env.episode_steps(), bank=bank, ids=ids)
        out[n] = recs
    return out


def _reference_wrench(f, tables, bank_units, units_out, ids="own"):
    P = f.w.params.numpy()
    return RT.wrench_targets(f.done, f.start, tables, f.ids if isinstance(ids, str) else ids, P[:, P_MASS], f.w.env.config.gravity,
                             P[:, P_ROTOR_X:P_ROTOR_X + 2], bank_units, units_out)


@pytest.mark.parametrize("n", (65, 130))
def test_wrench_targets_are_the_reference_bit_for_bit(flights, device, n):
    import raptor_amd.l2f as l2f
    from raptor_amd._lib import RaptorQuadError
    absolute_tables = wrench_tables(3.0)
    absolute_bank = l2f.WrenchBank(device, absolute_tables, units="absolute")
    for kind in ("auto", "freezing"):
        f = flights[n][kind]
        assert (f.start > 0).any() and (f.start < 7).all()                      # not all 0: the 3 unrecorded steps
        assert {1, 2} <= set(np.unique(f.done))
        if kind == "freezing":
            assert (f.done == 4).any()
        first = True
        for units, name in ((RELATIVE, "relative"), (ABSOLUTE, "absolute")):
            ref = _reference_wrench(f, wrench_tables(), "relative", name)       # [T, n, 6]
            assert (ref[f.done == 4] == 0).all() and (ref[f.done != 4] != 0).all()
            for memory in (HOST, DEVICE):
                ld = n + 3 if first else n                                      # ld_out > n_envs, once
                first = False
                out = wrench_call(f.traj, f.bank, f.ids, f.w.params, f.start, units, n, ld, memory)
                assert same(out[:, :, :n].transpose(0, 2, 1), ref), (kind, name, memory)
                assert (out[:, :, n:] == SENTINEL).all()                        # columns >= n_envs are not written
        if kind == "auto":
            rel, ab = _reference_wrench(f, wrench_tables(), "relative", "relative"), _reference_wrench(f, wrench_tables(), "relative", "absolute")
            assert not same(rel, ab)                                            # the scales do something
        # (b) an absolute bank: absolute output is the row, relative output is refused
        ref = _reference_wrench(f, absolute_tables, "absolute", "absolute")
        k, _ = RT.episode_steps(f.done, f.start)
        live = k >= 0
        rows = absolute_tables[f.ids[None, :].astype(np.int64), np.minimum(np.maximum(k, 0), 6)]
        assert same(ref[live], rows[live])
        for memory in (HOST, DEVICE):
            out = wrench_call(f.traj, absolute_bank, f.ids, f.w.params, f.start, ABSOLUTE, n, memory=memory)
            assert same(out.transpose(0, 2, 1), ref)
        with pytest.raises(RaptorQuadError) as err:
            wrench_call(f.traj, absolute_bank, f.ids, f.w.params, f.start, RELATIVE, n)
        assert "absolute bank" in str(err.value)
    # NULL ids and NULL start steps: table 0 and 0
    f = flights[n]["auto"]
    out = wrench_call(f.traj, f.bank, None, f.w.params, None, RELATIVE, n)
    P = f.w.params.numpy()
    ref = RT.wrench_targets(f.done, None, wrench_tables(), None, P[:, P_MASS], f.w.env.config.gravity, P[:, P_ROTOR_X:P_ROTOR_X + 2])
    assert same(out.transpose(0, 2, 1), ref)


@pytest.mark.parametrize("n", (65, 130))
def test_the_rule_is_the_engines(flights, device, n):
    """(c): an index bank (row k holds k) makes the generator print k; it is the reference's episode_steps, and k after the last
    step is what the engine itself reports - also for a recording begun on envs a freezing rollout left frozen"""
    import raptor_amd.l2f as l2f
    from raptor_amd import probing
    index = l2f.WrenchBank(device, index_tables())
    for kind in ("auto", "freezing", "thawed"):
        f = flights[n][kind]
        out = wrench_call(f.traj, index, None, f.w.params, f.start, RELATIVE, n)
        k, k_end = RT.episode_steps(f.done, f.start)
        assert (f.start < 7).all()
        got = out[:, 0, :].astype(np.int64)
        assert np.array_equal(got[k >= 0], k[k >= 0]), kind
        assert (out[:, :, :].transpose(0, 2, 1)[k < 0] == 0).all()
        assert (k[k >= 0] <= 6).all()                                           # the step limit of 7: no clamping hides a miscount
        assert np.array_equal(k_end, f.end.astype(np.int64)), (kind, np.flatnonzero(k_end != f.end)[:8])
        assert np.array_equal(probing.episode_steps(f.done, f.start), k)
    th = flights[n]["thawed"]
    assert (flights[n]["freezing"].done[-1] == 4).all() and (th.start == 0).all() and (th.done[0] != 4).all()


@pytest.mark.parametrize("n", (65, 130))
def test_generator_then_moments_on_the_stream(flights, n):
    """(d): both calls RQ_DST_DEVICE_ASYNC, one rq_device_synchronize at the end = the same targets fetched and passed from the host"""
    import torch
    L = _lib()
    for kind in ("auto", "freezing"):
        f = flights[n][kind]
        ld = n + 3
        e = np.ascontiguousarray(EDGES, np.uint32)
        B = e.size - 1
        y = torch.full((T, 6, ld), float("nan"), dtype=torch.float32, device="cuda")        # columns >= n stay NaN: never read into a sum
        S = torch.full((B, 32, 32), SENTINEL, dtype=torch.float64, device="cuda")
        counts = torch.full((B,), 77, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ids, start = np.ascontiguousarray(f.ids, np.uint32), np.ascontiguousarray(f.start, np.uint32)
        h, pol = f.traj._require("trajectory"), f.pol._handle()
        hidden(f.traj, f.pol, n)                                                            # the saved state exists: nothing below waits
        L.call("rq_trajectory_wrench_targets", h, f.bank._h, ids.ctypes.data, f.w.params._require("VectorParameters"),
               start.ctypes.data, ABSOLUTE, C.c_void_p(y.data_ptr()), ld, ASYNC)
        L.call("rq_trajectory_probe_moments_timed", h, pol, C.c_void_p(y.data_ptr()), ld, 6, e.ctypes.data, B,
               C.c_void_p(S.data_ptr()), C.c_void_p(counts.data_ptr()), ASYNC)
        L.call("rq_device_synchronize", f.traj._env._device._h)
        S, counts = S.cpu().numpy(), counts.cpu().numpy().astype(np.uint64)
        yh = wrench_call(f.traj, f.bank, f.ids, f.w.params, f.start, ABSOLUTE, n)
        S0, c0 = probe_timed(f.traj, f.pol, yh, EDGES)
        assert np.isfinite(S).all() and same(S, S0) and np.array_equal(counts, c0)
        assert (S0[:, 17:23, 17:23] != 0).any()


# ------------------------------------------------------------------------------ 6: refusals --
def test_refusals(cases, flights, device):
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
    out = np.full((T, 6, n), SENTINEL, np.float32)
    f = flights[65]["auto"]
    ids, start = np.ascontiguousarray(f.ids, np.uint32), np.ascontiguousarray(f.start, np.uint32)

    def moments(y=y, ld=n, M=3, edges=e, B=4, S=S, counts=counts, pol=pol, traj=traj, memory=HOST):
        L.call("rq_trajectory_probe_moments_timed", traj._require("trajectory") if traj is not None else None,
               pol._handle() if pol is not None else None, None if y is None else L.fptr(y), ld, M,
               None if edges is None else edges.ctypes.data, B, None if S is None else S.ctypes.data,
               None if counts is None else counts.ctypes.data, memory)

    def wrench(traj=f.traj, bank=f.bank, ids=ids, params=f.w.params, start=start, units=RELATIVE, out=out, ld=n, memory=HOST):
        L.call("rq_trajectory_wrench_targets", traj._require("trajectory") if traj is not None else None,
               bank._h if bank is not None else None, None if ids is None else ids.ctypes.data,
               params._require("VectorParameters") if params is not None else None, None if start is None else start.ctypes.data,
               units, None if out is None else L.fptr(out), ld, memory)

    def refused(fn, words):
        with pytest.raises(RaptorQuadError) as err:
            fn()
        assert words in str(err.value), str(err.value)
        assert (S == SENTINEL).all() and (counts == 77).all() and (out == SENTINEL).all()      # the outputs are untouched

    # everything the untimed call refuses
    for prec in ("bf16", "f16x2"):
        pol.set_precision(prec)
        refused(moments, "fp32 policy only")
    pol.set_precision("fp32")
    pol.set_standardize(np.zeros(22, np.float32), np.ones(22, np.float32))
    refused(moments, "Standardize")
    pol.set_standardize(None)
    pol.set_squash(True)
    refused(moments, "SampleAndSquash")
    pol.set_squash(False)
    pol.native_interval = 4
    refused(moments, "native interval")
    pol.native_interval = 1
    other_device = l2f.Device(0)                                 # another engine device object (same GPU)
    foreign = Raptor(other_device)
    foreign.reset()
    foreign._handle()
    refused(lambda: moments(pol=foreign), "another device")
    for M in (0, 16):
        refused(lambda: moments(M=M), "n_targets")
    for B in (0, 33):
        refused(lambda: moments(B=B, edges=np.arange(40, dtype=np.uint32)), "n_buckets")
    for bad in ([0, 1, 1, 4, 7], [0, 2, 1, 4, 7], [7, 4, 2, 1, 0]):
        refused(lambda: moments(edges=np.asarray(bad, np.uint32)), "age_edges")
    refused(lambda: moments(ld=n - 1), "ld_targets")
    nan = y.copy()
    nan[T - 1, 2, n - 1] = np.nan
    refused(lambda: moments(y=nan), "finite")
    refused(lambda: moments(y=nan), f"step {T - 1}, target 2, env {n - 1}")
    refused(lambda: moments(y=None), "targets")
    refused(lambda: moments(edges=None), "age_edges")
    refused(lambda: moments(S=None), "moments")
    refused(lambda: moments(counts=None), "counts")
    refused(lambda: moments(pol=None), "null")
    refused(lambda: moments(traj=None), "null")
    refused(lambda: moments(memory=3), "memory")
    refused(lambda: moments(memory=DEVICE), "another device")    # device memory is announced, host memory is given
    empty = c.w.vector.Trajectory(c.w.env, 4)
    refused(lambda: moments(traj=empty), "empty")

    # the wrench targets' own
    refused(lambda: wrench(out=None), "out")
    refused(lambda: wrench(bank=None), "bank")
    refused(lambda: wrench(params=None), "params")
    refused(lambda: wrench(traj=None), "null")
    refused(lambda: wrench(bank=l2f.WrenchBank(other_device, wrench_tables())), "another device")
    refused(lambda: wrench(params=c.w.params), "another env")
    refused(lambda: wrench(ld=n - 1), "ld_out")
    bad_ids = ids.copy()
    bad_ids[40] = 3
    refused(lambda: wrench(ids=bad_ids), "env 40")
    bad_start = start.copy()
    bad_start[17] = 7
    refused(lambda: wrench(start=bad_start), "env 17")
    refused(lambda: wrench(bank=l2f.WrenchBank(device, wrench_tables()[:, :6])), "episode_step_limit")
    for units in (-1, 2):
        refused(lambda: wrench(units=units), "units")
    refused(lambda: wrench(bank=l2f.WrenchBank(device, wrench_tables(), units="absolute")), "absolute bank")
    refused(lambda: wrench(traj=f.w.vector.Trajectory(f.w.env, 4)), "empty")
    refused(lambda: wrench(memory=3), "memory")
    refused(lambda: wrench(memory=DEVICE), "another device")

    moments()                                                    # and after all that it works, to the bits of check 1
    wrench()
    S_ref, c_ref = probe_timed(traj, c.pol, y, EDGES)
    assert same(S, S_ref) and np.array_equal(counts, c_ref)
    check_against_reference(c, c.h, y, EDGES, S, counts, "after the refusals")
    assert same(out.transpose(0, 2, 1), _reference_wrench(f, wrench_tables(), "relative", "relative"))


# ------------------------------------------------------------------------------ 8: Python --
def test_python_layer(cases, flights, device):
    import torch
    from raptor_amd import probing
    c = cases[130, True]
    n = 130
    Y = np.ascontiguousarray(int_targets(n, 5).transpose(0, 2, 1))               # [T, N, M]
    probe = probing.HiddenProbe(c.pol, None, list("abcde"), EDGES)
    S0, c0 = probe_timed(c.traj, c.pol, np.ascontiguousarray(Y.transpose(0, 2, 1)), EDGES)
    m = probe.moments(c.traj, targets=Y)
    assert same(m.S, S0) and np.array_equal(m.counts, c0)
    ld = 192
    Yd = torch.full((T, 5, ld), float("nan"), dtype=torch.float32, device="cuda")
    Yd[:, :, :n] = torch.from_numpy(np.ascontiguousarray(Y.transpose(0, 2, 1))).cuda()
    md = probe.moments(c.traj, targets=Yd, device=True)
    assert same(md.S, S0) and np.array_equal(md.counts, c0)
    with pytest.raises(ValueError):
        probe.moments(c.traj, targets=Yd[:, :4].contiguous(), device=True)
    with pytest.raises(ValueError):
        probe.moments(c.traj, targets=Yd.cpu(), device=True)
    # a probe built the old way gives what it gave
    y = np.random.default_rng(3).standard_normal((n, 4)).astype(np.float32)
    old = probing.HiddenProbe(c.pol, y, list("abcd"), EDGES)
    S1, c1 = probe_untimed(c.traj, c.pol, np.ascontiguousarray(y.T), EDGES)
    for dev in (False, True):
        mo = old.moments(c.traj, device=dev)
        assert same(mo.S, S1) and np.array_equal(mo.counts, c1)
    # traj.wrench_targets = the C call, in both layouts
    f = flights[130]["auto"]
    for units, u in (("relative", RELATIVE), ("absolute", ABSOLUTE)):
        want = wrench_call(f.traj, f.bank, f.ids, f.w.params, f.start, u, n)     # [T, 6, n]
        got = f.traj.wrench_targets(f.bank, f.ids, f.w.params, f.start, units=units)
        assert got.shape == (T, n, 6) and same(got, want.transpose(0, 2, 1))
        gd = f.traj.wrench_targets(f.bank, f.ids, f.w.params, f.start, units=units, device=True)
        assert gd.shape[:2] == (T, 6) and gd.shape[2] >= n and same(gd[:, :, :n].cpu().numpy(), want)
        assert (gd[:, :, n:] == 0).all()
    mw = probing.HiddenProbe(f.pol, None, probing.WRENCH_NAMES, EDGES).moments(f.traj, targets=gd, device=True)
    S2, c2 = probe_timed(f.traj, f.pol, want, EDGES)
    assert same(mw.S, S2) and np.array_equal(mw.counts, c2)
    assert np.array_equal(probing.table_targets(wrench_tables(), probing.episode_steps(f.done, f.start), f.ids),
                          f.traj.wrench_targets(f.bank, f.ids, f.w.params, f.start))
