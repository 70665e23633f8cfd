"""The weighted distillation loss without a GPU: the header's declarations of the four *_weighted calls, that ``weight=None`` reaches
the calls of before and nothing else, the refusals Python makes itself - before an optimizer exists, so stubs do -,
``training.holdout_weights``, and the float64 restatement (tests/weighted_distill_reference.py) against the unweighted one."""
import os
import re
import types

import numpy as np
import pytest

import distill_reference as D
import weighted_distill_reference as WR
from conftest import ROOT

N, T, P = 300, 20, 3
WEIGHTED = ["rq_trajectory_policy_loss_grad_weighted", "rq_trajectory_distill_weighted", "rq_trajectory_policies_loss_grad_weighted",
            "rq_trajectory_policies_distill_weighted"]


def test_the_header_declares_the_four_weighted_calls_as_bound():
    from raptor_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "raptor_quad.h")).read()
    for name in WEIGHTED:
        assert name in _lib._SIGNATURES and name in _lib.EXPORTED_SYMBOLS, name
        m = re.search(r"RQ_API int %s\(([^;]*)\);" % name, hdr, re.S)
        assert m, f"{name} is bound by raptor_amd/_lib.py but not declared in include/raptor_quad.h"
        args = m.group(1).split(",")
        assert len(args) == len(_lib._SIGNATURES[name]), name
        # the sibling's arguments with weight, ld_weight, weight_steps behind ld_target
        sib = re.search(r"RQ_API int %s\(([^;]*)\);" % name[:-len("_weighted")], hdr, re.S).group(1).split(",")
        words = [a.split()[-1].lstrip("*") for a in args]
        at = words.index("ld_target")
        assert words[at + 1:at + 4] == ["weight", "ld_weight", "weight_steps"], words
        assert words[:at + 1] + words[at + 4:] == [a.split()[-1].lstrip("*") for a in sib], name
        assert len(_lib._SIGNATURES[name]) == len(_lib._SIGNATURES[name[:-len("_weighted")]]) + 3
    assert int(re.search(r"#define RQ_ABI_VERSION (\d+)", hdr).group(1)) == 5 == _lib.ABI_VERSION


# ---- stubs: a library that records the names it is called by, a trajectory and a policy / bank that are handles only ----
class _Recorder:
    def __init__(self, monkeypatch):
        from raptor_amd import _lib, training
        self.names = []
        monkeypatch.setattr(_lib, "call", lambda name, *a: self.names.append(name) or 0)
        monkeypatch.setattr(_lib, "load", lambda: types.SimpleNamespace(rq_optimizer_destroy=lambda h: 0, rq_bank_optimizer_destroy=lambda h: 0))
        monkeypatch.setattr(training.Distiller, "_torch_device", staticmethod(lambda traj: None))      # the NumPy path, no device


def _stubs(n=N, steps=T):
    env = types.SimpleNamespace(N_ENVIRONMENTS=n, _device=object())

    class Traj:
        _env = env

        def __len__(self):
            return steps

        def _require(self, what):
            return 1

    policy = types.SimpleNamespace(_handle=lambda device=None: 2, _weights_on_device=False)
    bank = types.SimpleNamespace(n_policies=P, _h=3, _weights_on_device=False)
    return Traj(), policy, bank


def _ids():
    return np.repeat(np.asarray((2, 0, 2, 1, 0), np.uint32), 64)[:N]


def test_without_a_weight_only_the_calls_of_before_are_made(monkeypatch):
    from raptor_amd.training import BankDistiller, Distiller
    rec = _Recorder(monkeypatch)
    traj, policy, bank = _stubs()
    y = np.zeros((T, 4, N), np.float32)
    d, b = Distiller(policy), BankDistiller(bank)
    for kw in (dict(), dict(weight=None)):
        d.loss_and_grad(traj, target=y, **kw)
        d.step(traj, target=y, updates=2, **kw)
        b.loss_and_grad(traj, _ids(), target=y, **kw)
        b.step(traj, _ids(), target=y, updates=2, **kw)
    assert set(rec.names) == {"rq_trajectory_policy_loss_grad", "rq_optimizer_create", "rq_trajectory_distill",
                              "rq_trajectory_policies_loss_grad", "rq_bank_optimizer_create", "rq_trajectory_policies_distill"}
    # and with one, the siblings - the same stubs tell the two apart
    rec.names.clear()
    w = np.ones(N, np.float32)
    d.loss_and_grad(traj, target=y, weight=w)
    d.step(traj, target=y, weight=w)
    b.loss_and_grad(traj, _ids(), target=y, weight=np.ones((T, N + 2), np.float32))
    b.step(traj, _ids(), target=y, weight=w[None])
    assert rec.names == WEIGHTED


BAD = [(np.ones(N, np.float64), "float32"), (np.ones(N, np.int32), "float32"), (np.ones((1, 1, N), np.float32), "float32"),
       (np.float32(1.0), "float32"), (np.ones(N - 1, np.float32), "columns"), (np.ones((T, N - 1), np.float32), "columns"),
       (np.ones((2, N), np.float32), "rows"), (np.ones((T + 1, N), np.float32), "rows"), (np.ones((0, N), np.float32), "rows")]


@pytest.mark.parametrize("weight,words", BAD)
def test_a_misshapen_weight_is_refused_before_the_library_is_touched(monkeypatch, weight, words):
    from raptor_amd.training import BankDistiller, Distiller
    rec = _Recorder(monkeypatch)
    traj, policy, bank = _stubs()
    d, b = Distiller(policy), BankDistiller(bank)
    for call in (lambda: d.loss_and_grad(traj, weight=weight), lambda: d.step(traj, weight=weight),
                 lambda: b.loss_and_grad(traj, _ids(), weight=weight), lambda: b.step(traj, _ids(), weight=weight)):
        with pytest.raises(ValueError, match=words):
            call()
    assert d._h is None and b._h is None and rec.names == []


@pytest.mark.parametrize("value", [-1.0, -0.0 - 1e-30, np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("steps", [1, T])
def test_a_numpy_weight_must_be_finite_and_non_negative_on_the_envs_columns(monkeypatch, value, steps):
    from raptor_amd.training import BankDistiller, Distiller
    rec = _Recorder(monkeypatch)
    traj, policy, bank = _stubs()
    d, b = Distiller(policy), BankDistiller(bank)
    w = np.ones((steps, N + 4), np.float32)
    w[steps - 1, 17] = value
    for call in (lambda: d.loss_and_grad(traj, weight=w), lambda: d.step(traj, weight=w),
                 lambda: b.loss_and_grad(traj, _ids(), weight=w), lambda: b.step(traj, _ids(), weight=w)):
        with pytest.raises(ValueError, match=f"step {steps - 1}, env 17"):
            call()
    assert d._h is None and b._h is None and rec.names == []
    # the padding columns are nobody's: whatever they hold, the call is made
    w[steps - 1, 17] = 1.0
    w[:, N:] = value
    d.loss_and_grad(traj, weight=w)
    assert rec.names == ["rq_trajectory_policy_loss_grad_weighted"]


def test_holdout_weights():
    from raptor_amd.training import holdout_weights
    for n, fraction in ((300, 0.1), (7, 0.5), (1, 0.4), (1000, 0.123), (65, 1 / 3), (10, 0.0), (10, 1.0), (0, 0.5)):
        train, held = holdout_weights(n, fraction, seed=3)
        assert train.dtype == held.dtype == np.float32 and train.shape == held.shape == (n,)
        assert set(np.unique(held)) <= {0.0, 1.0} and np.array_equal(train + held, np.ones(n, np.float32))
        assert int(held.sum()) == int(round(fraction * n)), (n, fraction)
        again = holdout_weights(n, fraction, seed=3)
        assert np.array_equal(again[0], train) and np.array_equal(again[1], held)
    a, b = holdout_weights(300, 0.5, seed=1)[1], holdout_weights(300, 0.5, seed=2)[1]
    assert not np.array_equal(a, b)
    assert not holdout_weights(10, 0.0, 0)[1].any() and holdout_weights(10, 1.0, 0)[1].all()
    with pytest.raises(ValueError):
        holdout_weights(10, 1.5, 0)


def _random_case(seed=0, shape=(12, 4, 37)):
    rng = np.random.default_rng(seed)
    act, y = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    live = np.broadcast_to(rng.random((shape[0], 1, shape[2])) < 0.8, shape)
    return rng, act, y, live


def test_with_ones_the_reference_is_the_unweighted_reference_exactly():
    rng, act, y, live = _random_case()
    l0, s0, t0 = D.masked_mse(act, y, live)
    for w in (np.ones(37, np.float32), np.ones((12, 1, 37), np.float32), np.float32(1.0)):
        loss, seed, terms, W4 = WR.weighted_mse(act, y, live, w)
        assert loss == l0 and np.array_equal(seed, s0) and np.array_equal(terms, t0) and W4 == live.sum()
    # the bound differs from the unweighted one by the float64 fraction only
    M = int(live.sum())
    assert D.loss_bound(t0, M) <= WR.loss_bound(t0, float(M), M) <= D.loss_bound(t0, M) * (1 + 1e-6)
    # every weight c: the loss and its gradient do not change but for the rounding of c
    loss, seed, _, W4 = WR.weighted_mse(act, y, live, np.float32(4.0))
    assert loss == l0 and np.array_equal(seed, s0) and W4 == 4.0 * M
    # nothing counts
    loss, seed, terms, W4 = WR.weighted_mse(act, y, live, np.zeros(37, np.float32))
    assert loss == 0.0 and W4 == 0.0 and not seed.any() and not terms.any()


def test_what_does_not_count_goes_nowhere_whatever_it_holds():
    rng, act, y, live = _random_case(1)
    w = rng.uniform(0.0, 2.0, (12, 1, 37)).astype(np.float32)
    drop = rng.integers(0, 4, w.shape)
    w[drop == 1] = 0.0
    w[drop == 2] = -1.5
    w[(drop == 3) & (rng.random(w.shape) < 0.3)] = np.nan
    counts, _ = WR.counting(live, w)
    assert counts.any() and (~counts & live).any() and (~live).any()
    clean = WR.weighted_mse(act, y, live, w)
    y2, act2 = y.copy(), act.copy()
    y2[~counts] = np.nan
    act2[~counts] = np.inf
    dirty = WR.weighted_mse(act2, y2, live, w)
    assert np.isfinite(dirty[0]) and np.isfinite(dirty[1]).all() and np.isfinite(dirty[2]).all()
    assert dirty[0] == clean[0] and np.array_equal(dirty[1], clean[1]) and dirty[3] == clean[3]
    assert not dirty[1][~counts].any()
    # the same by hand: a plain weighted mean over the counting entries
    e = (act.astype(np.float64) - y)[counts]
    ww = np.broadcast_to(w, act.shape).astype(np.float64)[counts]
    assert abs(clean[0] - (ww * e * e).sum() / ww.sum()) <= 1e-12 * clean[0]


def test_the_torch_statement_is_the_reference():
    torch = pytest.importorskip("torch")
    from raptor_amd.training import masked_mse, weighted_mse
    rng, act, y, live = _random_case(2)
    w = rng.uniform(0.0, 2.0, (12, 1, 37)).astype(np.float32)
    w[rng.random(w.shape) < 0.25] = 0.0
    w[0, 0, :3] = (-1.0, np.nan, 0.0)
    counts, _ = WR.counting(live, w)
    y2 = y.copy()
    y2[~counts] = np.nan
    a = torch.tensor(act, dtype=torch.float64, requires_grad=True)
    loss = weighted_mse(a, torch.tensor(y2, dtype=torch.float64), torch.tensor(live.copy()), torch.tensor(w))
    loss.backward()
    ref = WR.weighted_mse(act, y2, live, w)
    assert abs(float(loss.detach()) - ref[0]) <= 1e-12 * ref[0]
    assert np.isfinite(a.grad.numpy()).all() and np.abs(a.grad.numpy() - ref[1]).max() <= 1e-12 * np.abs(ref[1]).max()
    # ones: masked_mse; nothing counts: 0 and a zero gradient
    ones = weighted_mse(a, torch.tensor(y, dtype=torch.float64), torch.tensor(live.copy()), torch.ones(37))
    assert float(ones.detach()) == float(masked_mse(a, torch.tensor(y, dtype=torch.float64), torch.tensor(live.copy())).detach())
    a.grad = None
    none = weighted_mse(a, torch.tensor(y2, dtype=torch.float64), torch.tensor(live.copy()), torch.zeros(37))
    none.backward()
    assert float(none.detach()) == 0.0 and not a.grad.numpy().any()
