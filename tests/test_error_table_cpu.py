"""The imitation error table without a GPU: the header's declarations of the two entry points against raptor_amd/_lib.py and the
built library, the NumPy restatement (tests/error_table_reference.py) against ``probing.episode_steps`` and against sums done by
hand, ``training.ErrorTable``'s algebra in float64, and the refusals Python makes itself - before the library is touched, so stubs do."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import error_table_reference as ER
from conftest import ROOT
from raptor_amd.training import ErrorTable, imitation_error      # noqa: F401  (what this module is about: without them nothing here runs)

CALLS = ["rq_trajectory_policy_error_table", "rq_trajectory_policies_error_table"]
N, T, P = 130, 12, 3


def test_the_header_declares_the_two_calls_as_bound_and_the_library_exports_them():
    from raptor_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "raptor_quad.h")).read()
    words = {}
    for name in CALLS:
        assert name in _lib._SIGNATURES and name in _lib.EXPORTED_SYMBOLS, name
        m = re.search(r"RQ_API int %s\(([^;]*)\);" % name, hdr, re.S)
        assert m, f"{name} is bound by raptor_amd/_lib.py but not declared in include/raptor_quad.h"
        args = m.group(1).split(",")
        assert len(args) == len(_lib._SIGNATURES[name]), name
        words[name] = [a.split()[-1].lstrip("*") for a in args]
        assert _lib._SIGNATURES[name][-1] is C.c_int and _lib._SIGNATURES[name][-2] is C.c_uint32      # ld_out, memory
        assert hasattr(C.CDLL(_lib.LIB_PATH), name), f"{_lib.LIB_PATH} does not export {name}"
    assert words[CALLS[0]] == ["t", "policy", "target", "ld_target", "age_edges", "n_buckets", "start", "sse", "count", "ld_out", "memory"]
    # the bank's call: the single policy's with the bank and its ids in the policy's place
    assert words[CALLS[1]] == ["t", "bank", "policy_id"] + words[CALLS[0]][2:]
    assert int(re.search(r"#define RQ_ABI_VERSION (\d+)", hdr).group(1)) == 5 == _lib.ABI_VERSION


# ---- the restatement ----
# four envs by hand.  env 0: an episode of 5 steps ending in a step limit (2), then one of 3 ending in a termination (1), then 4 more
# steps; env 1: frozen from step 3 to step 6, then it goes on where it was; env 2: never ends - its age passes every edge used below;
# env 3: ends at once, is frozen, thaws.
DONE = np.array([[0, 0, 0, 1],
                 [0, 0, 0, 4],
                 [0, 0, 0, 4],
                 [0, 4, 0, 0],
                 [2, 4, 0, 0],
                 [0, 4, 0, 2],
                 [0, 4, 0, 0],
                 [1, 0, 0, 0],
                 [0, 0, 0, 0],
                 [0, 1, 0, 0],
                 [0, 0, 0, 4],
                 [0, 0, 0, 0]], np.uint8)
AGES = np.array([[0, 0, 0, 0],
                 [1, 1, 1, -1],
                 [2, 2, 2, -1],
                 [3, -1, 3, 0],
                 [4, -1, 4, 1],
                 [0, -1, 5, 2],
                 [1, -1, 6, 0],
                 [2, 3, 7, 1],
                 [0, 4, 8, 2],
                 [1, 5, 9, 3],
                 [2, 0, 10, -1],
                 [3, 1, 11, 4]], np.int64)


def test_the_restated_ages_are_the_probes():
    from raptor_amd import probing
    assert set(np.unique(DONE)) == {0, 1, 2, 4}
    assert np.array_equal(ER.ages(DONE), AGES)
    assert np.array_equal(ER.ages(DONE), probing.episode_steps(DONE))
    rng = np.random.default_rng(0)
    for _ in range(5):
        done = rng.choice(np.asarray([0, 0, 0, 1, 2, 4, 4], np.uint8), size=(40, 9))
        assert np.array_equal(ER.ages(done), probing.episode_steps(done))


@pytest.mark.parametrize("edges", [(0, 1, 2, 4, 9), (1, 3), (0, 2, 5), (2, 3, 100), (0, 2 ** 32 - 1)])
def test_the_dropped_steps_are_exactly_those_outside_the_edges(edges):
    b = ER.buckets(AGES, edges)
    inside = (AGES >= edges[0]) & (AGES < edges[-1])
    assert np.array_equal(b >= 0, inside)
    for j in range(len(edges) - 1):
        assert np.array_equal(b == j, (AGES >= edges[j]) & (AGES < edges[j + 1]))
    rng = np.random.default_rng(1)
    act, y = rng.standard_normal((12, 4, 4)).astype(np.float32), rng.standard_normal((12, 4, 4)).astype(np.float32)
    sse, count = ER.error_table(act, y, DONE, edges)
    assert sse.dtype == np.float32 and count.dtype == np.uint32 and sse.shape == count.shape == (len(edges) - 1, 4)
    assert int(count.sum()) == int(inside.sum())
    for j in range(len(edges) - 1):
        assert np.array_equal(count[j], (b == j).sum(0))


def test_the_sums_are_sequential_float32_and_go_on_when_an_env_returns_to_a_bucket():
    rng = np.random.default_rng(2)
    act = (rng.standard_normal((12, 4, 4)) * 3).astype(np.float32)
    y = rng.standard_normal((12, 4, 4)).astype(np.float32)
    edges = (0, 2, 4)                       # env 0 is in bucket 0 at steps 0, 1 and again at 5, 6, 8, 9: three episodes
    sse, count = ER.error_table(act, y, DONE, edges)
    f = np.float32
    for i in range(4):
        for j in range(2):
            acc, cnt = f(0.0), 0
            for t in range(12):
                if edges[j] <= AGES[t, i] < edges[j + 1]:
                    d = [f(act[t, k, i] - y[t, k, i]) for k in range(4)]
                    e = f(f(f(f(d[0] * d[0]) + f(d[1] * d[1])) + f(d[2] * d[2])) + f(d[3] * d[3]))
                    acc, cnt = f(acc + e), cnt + 1
            assert sse[j, i].tobytes() == acc.tobytes() and count[j, i] == cnt, (i, j)
    assert count[0, 0] == 6 and count[1, 0] == 5
    # what is frozen or dropped goes nowhere, whatever it holds
    act2, y2 = act.copy(), y.copy()
    out = np.broadcast_to((ER.buckets(AGES, edges) < 0)[:, None, :], act.shape)
    act2[out], y2[out] = np.inf, np.nan
    sse2, count2 = ER.error_table(act2, y2, DONE, edges)
    assert sse2.tobytes() == sse.tobytes() and np.array_equal(count2, count) and np.isfinite(sse2).all()


# ---- ErrorTable ----
def _table(seed=0, B=4, n=10, kind=np.asarray):
    from raptor_amd.training import ErrorTable
    rng = np.random.default_rng(seed)
    count = rng.integers(1, 5, (B, n)).astype(np.uint32)
    count[1] = 0                                            # a bucket nobody met
    count[:, 3] = 0                                         # an env that never counted
    sse = np.where(count > 0, rng.random((B, n)) * 3, 0.0).astype(np.float32)
    return ErrorTable(kind(sse), kind(count), [0, 1, 2, 4, 9]), sse.astype(np.float64), count.astype(np.float64)


def _check_algebra(tab, sse, count, as_numpy):
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(as_numpy(tab.mse()), sse / (4 * count), equal_nan=True)
        assert np.isnan(as_numpy(tab.mse())[1]).all() and np.isnan(as_numpy(tab.mse())[:, 3]).all()
        assert np.allclose(as_numpy(tab.per_env()), sse.sum(0) / (4 * count.sum(0)), rtol=1e-15, atol=0, equal_nan=True)
        assert np.isnan(as_numpy(tab.per_env())[3]) and np.isfinite(np.delete(as_numpy(tab.per_env()), 3)).all()
        assert np.allclose(as_numpy(tab.by_age()), sse.sum(1) / (4 * count.sum(1)), rtol=1e-15, atol=0, equal_nan=True)
        assert np.isnan(as_numpy(tab.by_age())[1]) and tab.by_age().shape == (4,)
        assert abs(float(tab.loss()) - sse.sum() / (4 * count.sum())) <= 1e-15 * sse.sum()
        ids = np.asarray([2, 0, 0, 4, 2, 2, 0, 4, 4, 2])    # group 1 has no env, group 3 none either
        got = as_numpy(tab.by_group(ids, 5))
        assert got.shape == (5, 4)
        for g in range(5):
            want = sse[:, ids == g].sum(1) / (4 * count[:, ids == g].sum(1))
            assert np.allclose(got[g], want, rtol=1e-15, atol=0, equal_nan=True), g
        assert np.isnan(got[1]).all() and np.isnan(got[3]).all() and np.isnan(got[:, 1]).all() and np.isfinite(got[0, [0, 2, 3]]).all()
    for bad in (ids[:-1], ids + 1, ids.astype(np.float64), -ids):
        with pytest.raises(ValueError):
            tab.by_group(bad, 5)


def test_error_table_algebra_in_float64_with_nan_where_nothing_counts():
    from raptor_amd.training import ErrorTable
    tab, sse, count = _table()
    _check_algebra(tab, sse, count, np.asarray)
    assert tab.mse().dtype == np.float64 and tab.edges.dtype == np.uint32
    nothing = ErrorTable(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.uint32), [0, 1, 2])
    assert np.isnan(nothing.loss()) and np.isnan(nothing.by_age()).all() and np.isnan(nothing.per_env()).all()
    for bad in ((np.zeros((2, 3)), np.zeros((2, 4)), [0, 1, 2]), (np.zeros((2, 3)), np.zeros((2, 3)), [0, 1]), (np.zeros(3), np.zeros(3), [0, 1])):
        with pytest.raises(ValueError):
            ErrorTable(*bad)


def test_error_table_algebra_on_torch_tensors():
    torch = pytest.importorskip("torch")
    tab, sse, count = _table(kind=lambda a: torch.tensor(a.astype(np.int32) if a.dtype == np.uint32 else a))
    _check_algebra(tab, sse, count, lambda t: t.numpy())
    assert tab.mse().dtype == torch.float64


# ---- Python's refusals: stubs record every library call ----
class _Recorder:
    def __init__(self, monkeypatch):
        from raptor_amd import _lib, training
        self.names = []
        monkeypatch.setattr(_lib, "call", lambda name, *a: self.names.append(name) or 0)
        monkeypatch.setattr(_lib, "load", lambda: self.names.append("load") or types.SimpleNamespace())
        monkeypatch.setattr(training.Distiller, "_torch_device", staticmethod(lambda traj: None))      # the NumPy path, no device


def _stubs():
    env = types.SimpleNamespace(N_ENVIRONMENTS=N, _device=object())
    handles = []

    class Traj:
        _env = env

        def __len__(self):
            return T

        def _require(self, what):
            return 1

    def handle(device=None):
        handles.append(device)
        return 2

    return Traj(), types.SimpleNamespace(_handle=handle), types.SimpleNamespace(n_policies=P, _h=3), handles


def _ids():
    return np.repeat(np.asarray((2, 0, 2), np.uint32), 64)[:N]


BAD_EDGES = [(), (0,), (0, 0), (0, 2, 2), (3, 2), (0, 1.5), (-1, 2), (0, 2 ** 32), tuple(range(34)), ((0, 1), (2, 3)), ("a", "b")]


@pytest.mark.parametrize("edges", BAD_EDGES)
def test_bad_edges_are_refused_before_the_library_is_touched(monkeypatch, edges):
    from raptor_amd.training import imitation_error
    rec = _Recorder(monkeypatch)
    traj, policy, bank, handles = _stubs()
    with pytest.raises((ValueError, TypeError)):
        imitation_error(traj, policy, edges=edges)
    with pytest.raises((ValueError, TypeError)):
        imitation_error(traj, bank, edges=edges, policy_ids=_ids())
    assert rec.names == [] and handles == []


@pytest.mark.parametrize("shape", [(T, 4), (T + 1, 4, N), (T - 1, 4, N), (T, 3, N), (T, 4, N - 1), (T, 4, 0), (1, T, 4, N)])
def test_a_wrong_target_shape_is_refused_before_the_library_is_touched(monkeypatch, shape):
    from raptor_amd.training import imitation_error
    rec = _Recorder(monkeypatch)
    traj, policy, bank, handles = _stubs()
    with pytest.raises(ValueError, match="target"):
        imitation_error(traj, policy, target=np.zeros(shape, np.float32))
    with pytest.raises(ValueError, match="target"):
        imitation_error(traj, bank, target=np.zeros(shape, np.float32), policy_ids=_ids())
    assert rec.names == [] and handles == []


def test_a_bank_without_ids_and_ids_without_a_bank_are_refused_before_the_library_is_touched(monkeypatch):
    from raptor_amd.training import imitation_error
    rec = _Recorder(monkeypatch)
    traj, policy, bank, handles = _stubs()
    with pytest.raises(ValueError, match="policy_ids"):
        imitation_error(traj, bank)
    with pytest.raises(ValueError, match="policy_ids"):
        imitation_error(traj, policy, policy_ids=_ids())
    split = _ids()
    split[70] = 1
    for ids, words in ((split, "differ inside a 64-env block"), (_ids()[:-1], "one id per env"), (_ids() + 1, "out of range")):
        with pytest.raises(ValueError, match=words):
            imitation_error(traj, bank, policy_ids=ids)
    with pytest.raises(ValueError, match="start"):
        imitation_error(traj, policy, start="now")
    assert rec.names == [] and handles == []


def test_the_calls_that_are_made(monkeypatch):
    from raptor_amd import _lib
    from raptor_amd.training import imitation_error
    rec = _Recorder(monkeypatch)
    traj, policy, bank, handles = _stubs()
    seen = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: seen.append((name, a)) or 0)
    y = np.zeros((T, 4, N + 2), np.float32)
    tab = imitation_error(traj, policy)                                      # one bucket for every age, the stored actions
    assert tab.sse.shape == tab.count.shape == (1, N) and tab.edges.tolist() == [0, 2 ** 32 - 1]
    assert tab.sse.dtype == np.float32 and tab.count.dtype == np.uint32
    tab = imitation_error(traj, bank, edges=(0, 1, 2, 4, 9), target=y, start="current", policy_ids=_ids())
    assert tab.sse.shape == (4, N) and tab.edges.tolist() == [0, 1, 2, 4, 9]
    (n0, a0), (n1, a1) = seen
    assert (n0, n1) == tuple(CALLS) and len(a0) == len(_lib._SIGNATURES[n0]) and len(a1) == len(_lib._SIGNATURES[n1])
    # t, policy, target, ld_target, edges, B, start, sse, count, ld_out, memory
    assert a0[:4] == (1, 2, None, 0) and a0[5:7] == (1, 1) and a0[9:] == (N, 0)
    assert a1[:2] == (1, 3) and a1[4] == N + 2 and a1[6:8] == (4, 0) and a1[10:] == (N, 0)
    assert not hasattr(traj, "_learner_forwards")        # the trajectory's saved state is not this call's: a pending backward stays valid
    assert rec.names == []
