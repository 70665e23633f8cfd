"""The probes' host side without a GPU: the age rule of the reference the GPU tests compare against (tests/probe_reference.py), the
float64 algebra of raptor_amd/probing.py (fit, R^2 from moments alone), the targets, and the declarations of the two entry points."""
import os
import re

import numpy as np
import pytest

import probe_reference as R
from conftest import ROOT
from raptor_amd import _lib, probing


# ------------------------------------------------------------------------------ the age rule --
def test_age_resets_after_codes_1_and_2():
    done = np.array([[0, 0], [1, 0], [0, 2], [0, 0], [0, 0]], np.uint8)
    age, live = R.ages(done)
    assert live.all()
    assert age[:, 0].tolist() == [0, 1, 0, 1, 2]          # the ending step itself still has its age; the next one starts at 0
    assert age[:, 1].tolist() == [0, 1, 2, 0, 1]


def test_age_holds_across_code_4():
    done = np.array([[0], [0], [4], [4], [0], [2], [4], [0]], np.uint8)
    age, live = R.ages(done)
    assert live[:, 0].tolist() == [True, True, False, False, True, True, False, True]
    assert age[:, 0].tolist() == [0, 1, -1, -1, 2, 3, -1, 0]    # frozen steps neither count nor age; the reset survives a freeze


def test_age_code_4_at_the_first_step():
    done = np.array([[4, 0], [4, 1], [0, 4], [0, 0]], np.uint8)
    age, _ = R.ages(done)
    assert age[:, 0].tolist() == [-1, -1, 0, 1]
    assert age[:, 1].tolist() == [0, 1, -1, 0]


def test_dropped_ages():
    age = np.array([[0, 1, 2, 3, 4, 5, 6, -1]]).T
    assert R.buckets(age, [2, 5])[:, 0].tolist() == [-1, -1, 0, 0, 0, -1, -1, -1]
    assert R.buckets(age, [0, 1, 2, 4])[:, 0].tolist() == [0, 1, 2, 2, -1, -1, -1, -1]
    done = np.zeros((7, 1), np.uint8)
    h = np.arange(7 * 16, dtype=np.float64).reshape(7, 1, 16) / 100
    ref = R.moments(h, done, np.ones((1, 1)), [2, 5])
    assert ref["counts"].tolist() == [3]
    assert ref["S"][0, 0, 0] == 3 and np.isclose(ref["S"][0, 0, 1], h[2:5, 0, 0].sum())
    assert ref["S"][0, 0, 17] == 3 and ref["S"][0, 18:, :].max() == 0


def test_samples_outside_the_live_set_do_not_reach_a_sum():
    done = np.array([[0], [4], [0]], np.uint8)
    h = np.ones((3, 1, 16))
    h[1] = np.nan
    ref = R.moments(h, done, np.ones((1, 2)), [0, 8])
    assert np.isfinite(ref["S"]).all() and ref["counts"].tolist() == [2]


# ------------------------------------------------------------------------------ fit / r2 --
class _NoPolicy:
    pass


def _synthetic(seed, n, M=3, noise=0.0, w_seed=100):
    """y = Wt[0] + h Wt[1:] + noise; the relation comes from ``w_seed``, inputs and noise from ``seed``"""
    Wt = np.random.default_rng(w_seed).standard_normal((17, M))
    rng = np.random.default_rng(seed)
    h = rng.uniform(-1, 1, (1, n, 16))
    y = Wt[0] + h[0] @ Wt[1:] + noise * rng.standard_normal((n, M))
    return h, y, Wt


def _moments(h, y, edges):
    T, n, _ = h.shape
    ref = R.moments(h, np.zeros((T, n), np.uint8), y, edges)
    return probing.ProbeMoments(ref["S"], ref["counts"])


def test_fit_recovers_an_exact_linear_relation():
    h, y, Wt = _synthetic(0, 400)
    probe = probing.HiddenProbe(_NoPolicy(), y, ["a", "b", "c"], [0, 1])
    m = _moments(h, y, [0, 1])
    X = np.concatenate([np.ones((400, 1)), h[0]], axis=1)
    lstsq = np.linalg.lstsq(X, y, rcond=None)[0]
    W0 = probe.fit(m, ridge=0.0)
    assert W0.shape == (1, 17, 3)
    np.testing.assert_allclose(W0[0], lstsq, rtol=0, atol=1e-9)
    np.testing.assert_allclose(W0[0], Wt, rtol=0, atol=1e-9)
    W = probe.fit(m)                                           # the default ridge moves the solution by its relative size
    np.testing.assert_allclose(W[0], lstsq, rtol=0, atol=1e-4)
    for w in (W0, W):
        r2 = probe.r2(m, w)
        assert r2.shape == (1, 3) and np.abs(r2 - 1.0).max() < 1e-9, r2


def test_held_out_r2_from_moments_equals_r2_from_residuals():
    h, y, _ = _synthetic(1, 600, noise=0.5)
    h2, y2, _ = _synthetic(2, 500, noise=0.5)                  # the same relation on other inputs, other noise
    probe = probing.HiddenProbe(_NoPolicy(), y, ["a", "b", "c"], [0, 1])
    W = probe.fit(_moments(h, y, [0, 1]))
    r2 = probe.r2(_moments(h2, y2, [0, 1]), W)
    X2 = np.concatenate([np.ones((500, 1)), h2[0]], axis=1)
    res = y2 - X2 @ W[0]
    direct = 1.0 - (res ** 2).sum(axis=0) / ((y2 - y2.mean(axis=0)) ** 2).sum(axis=0)
    np.testing.assert_allclose(r2[0], direct, rtol=0, atol=1e-10)
    assert (r2[0] > 0.3).all() and (r2[0] < 0.999).all()       # noisy: a real fit, not a perfect one


def test_undersized_buckets_give_nan():
    rng = np.random.default_rng(2)
    T, n = 3, 17                                               # bucket 0 and 1: 17 samples each (< 18), bucket 2 none; [0, 3): 51
    h = rng.uniform(-1, 1, (T, n, 16))
    y = rng.standard_normal((n, 2))
    ref = R.moments(h, np.zeros((T, n), np.uint8), y, [0, 1, 2, 2 + 5])
    ref2 = R.moments(h, np.zeros((T, n), np.uint8), y, [0, 3, 4, 5])
    probe = probing.HiddenProbe(_NoPolicy(), y, ["a", "b"], [0, 1, 2, 7])
    m = probing.ProbeMoments(ref["S"], ref["counts"])
    assert m.counts.tolist() == [17, 17, 17]
    W = probe.fit(m)
    assert np.isnan(W).all() and np.isnan(probe.r2(m, W)).all()
    m2 = probing.ProbeMoments(ref2["S"], ref2["counts"])
    assert m2.counts.tolist() == [51, 0, 0]
    W2 = probe.fit(m2)
    assert np.isfinite(W2[0]).all() and np.isnan(W2[1:]).all()
    r2 = probe.r2(m2, W2)
    assert np.isfinite(r2[0]).all() and np.isnan(r2[1:]).all()


def test_moments_add():
    h, y, _ = _synthetic(3, 100)
    a, b = _moments(h[:, :60], y[:60], [0, 1]), _moments(h[:, 60:], y[60:], [0, 1])
    both = _moments(h, y, [0, 1])
    s = a + b
    np.testing.assert_allclose(s.S, both.S, rtol=1e-13, atol=1e-12)
    assert s.counts.tolist() == both.counts.tolist() == [100]
    assert sum([a, b]).counts.tolist() == [100]


def test_helpers():
    assert probing.log_age_edges(500, 10).tolist() == [0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 500]
    assert probing.log_age_edges(7, 1).tolist() == [0, 7]
    assert probing.log_age_edges(500, 10).dtype == np.uint32
    with pytest.raises(ValueError):
        probing.log_age_edges(4, 4)                 # 0 1 2 4 4: not ascending
    with pytest.raises(ValueError):
        probing.log_age_edges(500, 33)
    y = np.random.default_rng(4).standard_normal((50, 2)) * [3.0, 0.1] + [100.0, -5.0]
    ys, mean, std = probing.standardise(y)
    assert ys.dtype == np.float32 and np.abs(ys.mean(axis=0)).max() < 1e-6 and np.abs(ys.std(axis=0) - 1).max() < 1e-6
    np.testing.assert_allclose(ys * std + mean, y, atol=1e-4)
    with pytest.raises(ValueError):
        probing.HiddenProbe(_NoPolicy(), np.zeros((4, 1)), ["a"], [0, 2, 2])
    with pytest.raises(ValueError):
        probing.HiddenProbe(_NoPolicy(), np.zeros((4, 16)), ["a"] * 16, [0, 2])
    with pytest.raises(ValueError):
        probing.HiddenProbe(_NoPolicy(), np.full((4, 1), np.nan), ["a"], [0, 2])


# ------------------------------------------------------------------------------ targets --
def test_targets_of_the_nominal_crazyflie(oracle):
    cfg = oracle.default_config()
    cfg.domain_randomization = 0
    P = oracle.sample_initial_parameters(cfg, 0, 0, 0, 3)
    assert P.shape == (3, 26)
    names = ["log_mass", "thrust_to_weight", "log_jxx", "log_jzz", "tau_rise", "tau_fall", "torque_const", "hover_action"]
    y, out_names = probing.targets_from_params(P, cfg, names)
    assert out_names == names and y.shape == (3, 8) and y.dtype == np.float32
    rpm = 21702.0
    t2w = 4 * 3.16e-10 * rpm * rpm / (0.027 * cfg.gravity)
    hover = 2 * np.sqrt(0.027 * cfg.gravity / 4 / 3.16e-10) / rpm - 1
    want = [np.log(0.027), t2w, np.log(3.85e-6), np.log(5.9675e-6), 0.15, 0.15, 0.005964552, hover]
    np.testing.assert_allclose(y[0], want, rtol=2e-6)
    assert 2.2 < t2w < 2.3
    assert (y == y[0]).all()
    y2, _ = probing.targets_from_params(P, float(cfg.gravity), ["thrust_to_weight"])
    assert y2[0, 0] == y[0, 1]
    with pytest.raises(ValueError):
        probing.targets_from_params(P, cfg, ["mass_in_stone"])
    with pytest.raises(ValueError):
        probing.targets_from_params(P[:, :25], cfg, ["log_mass"])


# ------------------------------------------------------------------------------ declarations --
def test_entry_points_are_declared_and_the_abi_is_still_5():
    header = open(os.path.join(ROOT, "include", "raptor_quad.h")).read()
    assert re.search(r"#define\s+RQ_ABI_VERSION\s+5\b", header)
    assert _lib.ABI_VERSION == 5
    flat = re.sub(r"\s+", " ", header)
    assert "RQ_API int rq_trajectory_get_hidden(rq_trajectory* t, rq_policy* policy, float* out, int memory);" in flat
    assert ("RQ_API int rq_trajectory_probe_moments(rq_trajectory* t, rq_policy* policy, const float* targets, uint32_t ld_targets, "
            "uint32_t n_targets, const uint32_t* age_edges, uint32_t n_buckets, double* moments, uint64_t* counts, int memory);") in flat
    assert len(_lib._SIGNATURES["rq_trajectory_get_hidden"]) == 4
    assert len(_lib._SIGNATURES["rq_trajectory_probe_moments"]) == 10
    assert {"rq_trajectory_get_hidden", "rq_trajectory_probe_moments"} <= set(_lib.EXPORTED_SYMBOLS)
    lib = _lib.load()                                  # binds every listed symbol or raises
    assert lib.rq_abi_version() == 5
