"""tests/rate_grad_reference.py checked on the CPU: at interval 1 it is tests/policy_grad_reference.py, and at intervals 2, 3 and 4
its gradient is the derivative of its forward (central differences)."""
import numpy as np
import pytest

import policy_grad_reference as R
import rate_grad_reference as RR

T, N, SEED = 12, 5, 3


def _case():
    """12 steps x 5 envs, every done code, non-zero start steps, random weights; the seed keeps every layer_0 pre-activation away
    from the ReLU kink, where a central difference straddles it"""
    rng = np.random.default_rng(SEED)
    w = 0.3 * rng.standard_normal(2084)
    obs = rng.standard_normal((T, N, 22))
    done = rng.choice(np.array([0, 0, 0, 0, 1, 2, 4], np.uint8), size=(T, N))
    assert {0, 1, 2, 4} == set(np.unique(done).tolist())
    start_steps = np.array([1, 2, 3, 5, 7])
    h_start = rng.uniform(-0.7, 0.7, (N, 16))
    dact = rng.standard_normal((T, N, 4))
    return w, obs, done, start_steps, h_start, dact


def test_at_interval_one_it_is_the_native_rate_reference():
    w, obs, done, start_steps, h_start, dact = _case()
    for start in ("initial", "current"):
        act, cache = RR.forward(w, obs, done, 1, start_steps, start, h_start)
        act0, cache0 = R.forward(w, obs, done, start, h_start)
        assert np.array_equal(act, act0)
        for got, want in zip(RR.backward(cache, dact) + RR.bound(cache, dact, 1), R.backward(cache0, dact) + R.bound(cache0, dact, 1)):
            assert (got is None and want is None) or np.array_equal(got, want)


@pytest.mark.parametrize("interval", [2, 3, 4])
def test_gradient_is_the_derivative_of_the_forward(interval):
    """L = sum(a * dact).  Tolerance: a central difference of step e = 1e-6 has a truncation error of e^2 |L'''| / 6 ~ 1e-12 and a
    cancellation error of 2^-53 |L| / e ~ 1e-9 at |L| ~ 10: 1e-5 relative plus 1e-9 covers both in float64 and is no tuned number."""
    w, obs, done, start_steps, h_start, dact = _case()
    eps, rng = 1e-6, np.random.default_rng(SEED + interval)
    for start in ("initial", "current"):
        loss = lambda wv, h: float((RR.forward(wv, obs, done, interval, start_steps, start, h)[0] * dact).sum())
        _, cache = RR.forward(w, obs, done, interval, start_steps, start, h_start)
        assert min(np.abs(s["pre0"]).min() for s in cache["steps"]) >= 1e-3
        assert any((s["hold"] & (s["d"] != 4)).any() for s in cache["steps"])          # steps are held
        g, gh = RR.backward(cache, dact)
        assert (gh is None) == (start == "initial")
        for _ in range(10):
            v = rng.standard_normal(2084)
            v /= np.linalg.norm(v)
            fd, an = (loss(w + eps * v, h_start) - loss(w - eps * v, h_start)) / (2 * eps), float(g @ v)
            assert abs(fd - an) <= 1e-5 * abs(an) + 1e-9, (start, fd, an)
            if gh is not None:
                u = rng.standard_normal((N, 16))
                u /= np.linalg.norm(u)
                fd, an = (loss(w, h_start + eps * u) - loss(w, h_start - eps * u)) / (2 * eps), float((gh * u).sum())
                assert abs(fd - an) <= 1e-5 * abs(an) + 1e-9, (start, "h_start", fd, an)
