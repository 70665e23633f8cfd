"""CPU checks of the learner's float64 reference (tests/policy_grad_reference.py) and of the learner's C ABI surface.

The reference is what the GPU tests (tests/test_gpu_policy_grad.py) hold the fp32 kernels to, so it is checked here against two
independent statements of the same derivative: central finite differences of its own float64 forward, and torch's autograd through
a float64 nn.GRUCell loop.  Its forward must meet the checkpoint's known-answer vectors."""
import os
import re

import numpy as np
import pytest

import policy_grad_reference as R
from conftest import ROOT


def _case(seed, T, N, scale=0.4):
    g = np.random.default_rng(seed)
    w = g.standard_normal(2084) * scale
    w[R.OFF["H0"]:R.OFF["W2"]] = g.uniform(-0.5, 0.5, 16)       # a non-zero initial state makes the resets visible
    obs = g.standard_normal((T, N, 22))
    done = g.choice(np.array([0, 0, 0, 1, 2, 4], np.uint8), size=(T, N))
    dact = g.standard_normal((T, N, 4))
    h_start = g.uniform(-0.8, 0.8, (N, 16))
    return w, obs, done, dact, h_start


@pytest.mark.parametrize("start", ["initial", "current"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_gradient_matches_central_differences(start, seed):
    T, N = 7, 5
    w, obs, done, dact, h_start = _case(seed, T, N)
    assert {0, 1, 2, 4} <= set(np.unique(done).tolist())
    loss = lambda ww, hh=h_start: float((R.forward(ww, obs, done, start, hh)[0] * dact).sum())
    _, cache = R.forward(w, obs, done, start, h_start)
    g, gh = R.backward(cache, dact)
    eps = 1e-6
    fd = np.empty(2084)
    for k in range(2084):
        e = np.zeros(2084)
        e[k] = eps
        fd[k] = (loss(w + e) - loss(w - e)) / (2 * eps)
    scale = np.abs(fd).max()
    assert np.abs(g - fd).max() < 1e-6 * scale, np.abs(g - fd).max() / scale
    if start == "initial":
        assert gh is None and np.abs(g[R.OFF["H0"]:R.OFF["W2"]]).max() > 0
    else:
        fdh = np.empty((N, 16))
        for i in range(N):
            for k in range(16):
                e = np.zeros((N, 16))
                e[i, k] = eps
                fdh[i, k] = (loss(w, h_start + e) - loss(w, h_start - e)) / (2 * eps)
        assert np.abs(gh - fdh).max() < 1e-6 * max(np.abs(fdh).max(), 1.0)


def test_reference_gradient_matches_torch_autograd_on_a_grucell_loop():
    torch = pytest.importorskip("torch")
    T, N = 9, 6
    for start in ("initial", "current"):
        w, obs, done, dact, h_start = _case(7, T, N)
        p = R.unpack(w)
        prm = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
        cell = torch.nn.GRUCell(16, 16).double()
        with torch.no_grad():
            cell.weight_ih.copy_(prm["Wi"]); cell.weight_hh.copy_(prm["Wh"])
            cell.bias_ih.copy_(prm["bi"]); cell.bias_hh.copy_(prm["bh"])
        hs = torch.tensor(h_start, dtype=torch.float64, requires_grad=True)
        h = prm["h0"].expand(N, 16) if start == "initial" else hs
        x = torch.tensor(obs)
        d = torch.tensor(done.astype(np.int64))
        total = 0
        for t in range(T):
            y = torch.relu(x[t] @ prm["W0"].T + prm["b0"])
            hn = cell(y, h)
            a = hn @ prm["W2"].T + prm["b2"]
            total = total + (a * torch.tensor(dact[t])).sum()
            h = torch.where((d[t] == 4)[:, None], h, hn)
            h = torch.where(((d[t] == 1) | (d[t] == 2))[:, None], prm["h0"].expand(N, 16), h)
        total.backward()
        # the cell's own parameters carry the GRU's gradient
        got = dict(W0=prm["W0"].grad, b0=prm["b0"].grad, Wi=cell.weight_ih.grad, Wh=cell.weight_hh.grad, bi=cell.bias_ih.grad,
                   bh=cell.bias_hh.grad, h0=prm["h0"].grad, W2=prm["W2"].grad, b2=prm["b2"].grad)
        flat = R.pack({k: (v.numpy() if v is not None else np.zeros_like(p[k])) for k, v in got.items()})
        _, cache = R.forward(w, obs, done, start, h_start)
        g, gh = R.backward(cache, dact)
        assert np.abs(g - flat).max() < 1e-12 * max(1.0, np.abs(flat).max()), start
        if start == "current":
            assert np.abs(gh - hs.grad.numpy()).max() < 1e-12 * max(1.0, np.abs(gh).max())


def test_reference_forward_meets_the_checkpoint_known_answers(weights, kat):
    x, y = kat
    act, _ = R.forward(weights, x, np.zeros(x.shape[:2], np.uint8), "initial")
    assert np.abs(act - y).max() < 1e-5


def test_the_bound_is_finite_and_rejects_wrong_episode_rules():
    """The bound is meant to separate rounding from mistakes: gradients computed under slightly wrong episode rules (a frozen step
    treated as a running one; an episode end that does not cut the recurrence) must fall outside it."""
    T, N = 30, 40
    w, obs, done, dact, _ = _case(11, T, N, scale=0.3)
    w32 = w.astype(np.float32).astype(np.float64)
    _, cache = R.forward(w32, obs, done, "initial")
    g, _ = R.backward(cache, dact)
    b, _ = R.bound(cache, dact, waves=1)
    assert np.isfinite(b).all() and (b > 0).all()
    assert np.abs(g).max() > 0 and (b < 0.1 * np.abs(g).max()).all()
    for wrong in (np.where(done == 4, 0, done), np.where((done == 1) | (done == 2), 0, done)):
        _, c2 = R.forward(w32, obs, wrong.astype(np.uint8), "initial")
        g2, _ = R.backward(c2, dact)
        assert (np.abs(g2 - g) > b).any()


def test_learner_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "raptor_quad.h")).read()
    for name in ("rq_policy_set_weights", "rq_trajectory_policy_forward", "rq_trajectory_policy_backward"):
        assert re.search(r"^RQ_API\s+int\s+" + name + r"\(", hdr, flags=re.M), name
    assert re.search(r"enum rq_grad_start \{ RQ_GRAD_START_CURRENT = 0, RQ_GRAD_START_INITIAL = 1 \}", hdr)
    from raptor_amd import _lib
    lib = _lib.load()
    for name in ("rq_policy_set_weights", "rq_trajectory_policy_forward", "rq_trajectory_policy_backward"):
        assert hasattr(lib, name), name
    assert lib.rq_abi_version() == 5
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.training import trajectory_actions          # noqa: F401
    assert callable(Raptor.set_weights)


def test_set_weights_and_the_learner_fail_loudly_without_a_device():
    import ctypes
    from raptor_amd import _lib
    lib = _lib.load()
    w = np.zeros(2084, np.float32)
    assert lib.rq_policy_set_weights(None, w.ctypes.data, 2084) != 0
    assert lib.rq_trajectory_policy_forward(None, None, 0, None, 0, 0) != 0
    assert lib.rq_trajectory_policy_backward(None, None, None, 0, None, None, 0) != 0
    assert b"null" in ctypes.string_at(lib.rq_last_error())


def test_masked_mse_gives_masked_entries_no_gradient_even_when_they_are_nan():
    """The loss the distillation loop uses masks its inputs: NaN actions or labels outside the mask (frozen steps of a recording)
    must not reach dL/da.  Masking the output instead does let them through - the reason the helper exists."""
    torch = pytest.importorskip("torch")
    from raptor_amd.training import masked_mse
    act = torch.tensor([1.0, float("nan"), 3.0, float("inf")], requires_grad=True)
    target = torch.tensor([0.5, 2.0, float("nan"), 1.0])
    live = torch.tensor([True, False, False, False])
    loss = masked_mse(act, target, live)
    loss.backward()
    assert float(loss) == 0.25 and act.grad.tolist() == [1.0, 0.0, 0.0, 0.0]
    act.grad = None
    torch.where(live, (act - target) ** 2, 0.0).sum().backward()
    assert torch.isnan(act.grad[1:3]).all()
