"""Targets per step, without a GPU: the declarations of the two entry points, the episode-step rule of the reference the GPU tests
compare against (tests/probe_timed_reference.py) and of raptor_amd.probing.episode_steps, the ValueErrors of
HiddenProbe.moments(traj, targets=...), and fit / R^2 on moments of a relation that changes over time."""
import os
import re

import numpy as np
import pytest

import probe_timed_reference as RT
from conftest import ROOT
from raptor_amd import _lib, probing


# ------------------------------------------------------------------------------ declarations --
def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "raptor_quad.h")).read()
    assert re.search(r"#define\s+RQ_ABI_VERSION\s+5\b", header)
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    assert ("RQ_API int rq_trajectory_probe_moments_timed(rq_trajectory* t, rq_policy* policy, const float* targets, uint32_t ld_targets, "
            "uint32_t n_targets, const uint32_t* age_edges, uint32_t n_buckets, double* moments, uint64_t* counts, int memory);") in flat
    assert ("RQ_API int rq_trajectory_wrench_targets(rq_trajectory* t, const rq_wrench_bank* bank, const uint32_t* wrench_id , "
            "const rq_params* params, const uint32_t* start_steps , int units_out , float* out, uint32_t ld_out, int memory);") in flat
    assert len(_lib._SIGNATURES["rq_trajectory_probe_moments_timed"]) == 10
    assert len(_lib._SIGNATURES["rq_trajectory_wrench_targets"]) == 9
    assert {"rq_trajectory_probe_moments_timed", "rq_trajectory_wrench_targets"} <= set(_lib.EXPORTED_SYMBOLS)
    lib = _lib.load()                                  # binds every listed symbol or raises
    assert lib.rq_abi_version() == 5
    assert probing.WRENCH_NAMES == ["fx", "fy", "fz", "tx", "ty", "tz"]


# ------------------------------------------------------------------------------ the k rule --
# columns: a start above 0 running on; code 1 then code 2; code 4 at the first step; code 4 in the middle; an episode that ends
# at the last step
DONE = np.array([[0, 0, 4, 0, 0],
                 [0, 1, 4, 0, 0],
                 [0, 0, 0, 4, 0],
                 [2, 0, 0, 4, 0],
                 [0, 2, 1, 0, 0],
                 [0, 0, 0, 0, 1]], np.uint8)
START = np.array([3, 0, 5, 1, 2], np.uint32)
K = np.array([[3, 0, -1, 1, 2],
              [4, 1, -1, 2, 3],
              [5, 0, 5, -1, 4],
              [6, 1, 6, -1, 5],
              [0, 2, 7, 3, 6],
              [1, 0, 0, 4, 7]], np.int64)
K_END = [2, 1, 1, 5, 0]


def test_episode_step_rule_on_hand_written_columns():
    k, end = RT.episode_steps(DONE, START)
    assert k.tolist() == K.tolist()
    assert end.tolist() == K_END
    k0, end0 = RT.episode_steps(DONE)                           # start None: all 0
    assert k0[:, 0].tolist() == [0, 1, 2, 3, 0, 1] and k0[:, 2].tolist() == [-1, -1, 0, 1, 2, 0]
    assert end0.tolist() == [2, 1, 1, 4, 0]
    assert k.shape == DONE.shape                               # every column ends at T
    assert probing.episode_steps(DONE, START).tolist() == K.tolist()          # and the package's helper says the same


def test_probing_episode_steps_is_the_reference():
    rng = np.random.default_rng(0)
    done = rng.choice(np.array([0, 0, 0, 1, 2, 4], np.uint8), size=(40, 33))
    start = rng.integers(0, 9, 33).astype(np.uint32)
    k = probing.episode_steps(done, start)
    assert k.dtype == np.int64 and np.array_equal(k, RT.episode_steps(done, start)[0])
    assert np.array_equal(probing.episode_steps(done), RT.episode_steps(done)[0])
    with pytest.raises(ValueError):
        probing.episode_steps(done, start[:-1])
    with pytest.raises(ValueError):
        probing.episode_steps(done[0])


def test_wrench_targets_reference_and_table_targets():
    rng = np.random.default_rng(1)
    tables = rng.uniform(-0.05, 0.05, (3, 7, 6)).astype(np.float32)
    ids = np.arange(5) % 3
    mass = rng.uniform(0.02, 0.1, 5).astype(np.float32)
    xy = rng.uniform(0.02, 0.06, (5, 2)).astype(np.float32)
    rel = RT.wrench_targets(DONE, START, tables, ids, mass, 9.81, xy)
    assert rel.dtype == np.float32 and rel.shape == (6, 5, 6)
    assert (rel[K < 0] == 0).all()
    assert np.array_equal(rel[0, 0], tables[0, 3]) and np.array_equal(rel[3, 0], tables[0, 6])
    assert np.array_equal(rel[4, 2], tables[2, 6])             # k = 7 is clamped to the last row
    assert np.array_equal(rel[5, 2], tables[2, 0])
    assert np.array_equal(probing.table_targets(tables, K, ids), rel)
    assert np.array_equal(probing.table_targets(tables[1], K[:, 1:2]), rel[:, 1:2])
    # the scaling is disturbances.compose's on a zero base
    from raptor_amd import disturbances
    ab = RT.wrench_targets(DONE, START, tables, ids, mass, 9.81, xy, units_out="absolute")
    want = disturbances.compose(np.zeros(6, np.float32), mass[None, :], 9.81, xy[None, :, :], rel)
    live = K >= 0
    assert np.array_equal(ab[live].view(np.uint32), want[live].view(np.uint32))
    assert (ab[~live] == 0).all()
    same = RT.wrench_targets(DONE, START, tables, ids, mass, 9.81, xy, bank_units="absolute", units_out="absolute")
    assert np.array_equal(same, rel)
    with pytest.raises(ValueError):
        RT.wrench_targets(DONE, START, tables, ids, mass, 9.81, xy, bank_units="absolute", units_out="relative")
    with pytest.raises(ValueError):
        probing.table_targets(tables, K, np.arange(5))         # an id outside the bank


# ------------------------------------------------------------------------------ ValueErrors before any library call --
class _NoPolicy:
    def _handle(self, device=None):
        raise AssertionError("the library was reached")


class _FakeEnv:
    N_ENVIRONMENTS = 4
    _device = None


class _FakeTraj:
    _env = _FakeEnv()

    def __len__(self):
        return 3

    def _require(self, what):
        raise AssertionError("the library was reached")


def test_value_errors_before_any_library_call():
    probe = probing.HiddenProbe(_NoPolicy(), None, ["a", "b"], [0, 2, 5])
    assert probe.n_targets == 2 and probe.n_buckets == 2
    assert probing.HiddenProbe(_NoPolicy(), names=["a"], age_edges=[0, 1]).n_targets == 1
    traj = _FakeTraj()
    good = np.zeros((3, 4, 2), np.float32)
    for bad in (np.zeros((2, 4, 2), np.float32),               # T
                np.zeros((3, 5, 2), np.float32),               # N
                np.zeros((3, 4, 3), np.float32),               # M
                np.zeros((3, 4), np.float32),
                good.astype(np.float64),                       # dtype
                np.where(np.arange(24).reshape(3, 4, 2) == 7, np.nan, good).astype(np.float32),
                np.where(np.arange(24).reshape(3, 4, 2) == 9, np.inf, good).astype(np.float32)):
        with pytest.raises(ValueError):
            probe.moments(traj, targets=bad)
    with pytest.raises(ValueError):
        probe.moments(traj)                                    # a probe without targets of its own needs the recording's
    with pytest.raises(ValueError):
        probing.HiddenProbe(_NoPolicy(), None, [], [0, 1])
    with pytest.raises(ValueError):
        probing.HiddenProbe(_NoPolicy(), None, ["a"] * 16, [0, 1])
    with pytest.raises(AssertionError):                        # and a good array does go on to the library
        probe.moments(traj, targets=good)


# ------------------------------------------------------------------------------ fit / r2 on timed moments --
def test_fit_recovers_an_exact_time_varying_linear_relation():
    """y_t = W0 + h_t W, with h_t and therefore y_t different at every step: moments_timed carries it, fit finds it, R^2 = 1"""
    rng = np.random.default_rng(7)
    T, n, M = 6, 150, 3
    Wt = rng.standard_normal((17, M))
    h = rng.uniform(-1, 1, (T, n, 16))
    y = Wt[0] + h @ Wt[1:]
    assert np.abs(y[0] - y[1]).min() > 0                       # it does change over time
    done = np.zeros((T, n), np.uint8)
    done[2, ::3] = 1
    done[4, 1::5] = 2
    edges = [0, 2, 6]
    ref = RT.moments_timed(h, done, y, edges)
    assert ref["counts"].sum() == T * n and (ref["counts"] > 17).all()
    m = probing.ProbeMoments(ref["S"], ref["counts"])
    probe = probing.HiddenProbe(_NoPolicy(), None, ["a", "b", "c"], edges)
    W = probe.fit(m, ridge=0.0)
    assert W.shape == (2, 17, M)
    for b in range(2):
        np.testing.assert_allclose(W[b], Wt, rtol=0, atol=1e-8)
    assert np.abs(probe.r2(m, W) - 1.0).max() < 1e-9
    # the untimed moments of the first step's targets are another matrix: the relation does not hold for them
    import probe_reference as R
    stale = R.moments(h, done, y[0], edges)
    assert np.abs(stale["S"] - ref["S"]).max() > 1.0
    # targets constant over time: the two references agree to the last bit
    const = np.broadcast_to(y[0], (T, n, M))
    assert np.array_equal(RT.moments_timed(h, done, const, edges)["S"], stale["S"])
