"""The learner on the GPU (rq_trajectory_policy_forward / _backward, csrc/rq_grad.hpp; Raptor.set_weights; raptor_amd.training):
forward parity with rq_trajectory_relabel, the gradient against the float64 reference and its bound (tests/policy_grad_reference.py),
determinism, the refusals, set_weights against a freshly created policy, torch autograd and a short distillation run.

Slack of each accuracy case: ``pytest tests/test_gpu_policy_grad.py -m gpu -v -s``."""
import numpy as np
import pytest

import policy_grad_reference as R
from gpu_common import World

pytestmark = pytest.mark.gpu

CURRENT, INITIAL = 0, 1


def _lib():
    from raptor_amd import _lib as L
    return L


def _record(device, oracle, n, T, seed, frozen=True, finite=True):
    """A recording with episode ends (terminations and step limits), auto-resets, frozen stretches and domain randomisation:
    the first part without auto-reset (envs freeze when their episode ends), the rest with it (they thaw).  The observations of
    frozen steps are unspecified (a wave whose envs are all frozen stops writing them); ``finite`` replaces them by N(0, 1) draws,
    so that the actions there - which the gradient differentiates too - are defined."""
    w = World(device, oracle, n, seed=seed, episode_step_limit=9, termination_position=0.6, domain_randomization=1)
    traj = w.vector.Trajectory(w.env, T)
    w.policy.reset()
    T1 = T // 2 if frozen and T >= 4 else 0
    if T1:
        w.vector.rollout(device, w.env, w.params, w.state, w.policy, w.rng, T1, "fused", autoreset=False, trajectory=traj)
    w.vector.rollout(device, w.env, w.params, w.state, w.policy, w.rng, T - T1, "fused", autoreset=True, trajectory=traj)
    # terminations (code 1) are rare in a short recording of the shipped policy; for the policy codes 1 and 2 are the same event
    # (an episode end), so every other step-limit end is relabelled a termination in place
    import torch
    done = traj.tensors()["done"]
    ends = (done == 2).nonzero()
    done[ends[::2, 0], ends[::2, 1]] = 1
    if finite:
        obs = traj.tensors()["obs"]
        draw = torch.randn(obs.shape, device=obs.device, generator=torch.Generator(obs.device).manual_seed(seed))
        obs.copy_(torch.where((done == 4)[:, None, :], draw, obs))
    torch.cuda.synchronize()            # the engine's stream does not order itself against torch's: traj.numpy() must see these writes
    return w, traj


def _ld(traj):
    return traj.tensors()["act"].shape[2]


def forward(traj, pol, start, ld=None):
    L = _lib()
    T, ld = len(traj), ld or _ld(traj)
    act = np.empty((T, 4, ld), np.float32)
    L.call("rq_trajectory_policy_forward", traj._require("trajectory"), pol._handle(), start, L.fptr(act), ld, 0)
    return act


def backward(traj, pol, dact, want_h=False, ld=None):
    L = _lib()
    ld = ld or _ld(traj)
    g = np.empty(2084, np.float32)
    gh = np.empty((16, ld), np.float32) if want_h else None
    L.call("rq_trajectory_policy_backward", traj._require("trajectory"), pol._handle(), L.fptr(np.ascontiguousarray(dact)), ld,
           L.fptr(g), L.fptr(gh) if want_h else None, 0)
    return g, gh


def _perturbed(weights, seed, scale=0.05):
    w = (weights + np.random.default_rng(seed).standard_normal(weights.size).astype(np.float32) * scale).astype(np.float32)
    w[2000:2016] = np.random.default_rng(seed + 1).uniform(-0.3, 0.3, 16).astype(np.float32)
    return w


def _dact(T, n, ld, seed):
    d = np.full((T, 4, ld), np.nan, np.float32)                 # padding columns: NaN, they must not matter
    d[:, :, :n] = np.random.default_rng(seed).standard_normal((T, 4, n)).astype(np.float32)
    return d


@pytest.mark.parametrize("n", [1000, 70000])
def test_forward_equals_relabel_bit_for_bit(device, oracle, weights, n):
    from raptor_amd.foundation_policy import Raptor
    w, traj = _record(device, oracle, n, 40, seed=41, finite=False)
    rec = traj.numpy()
    assert {0, 1, 2, 4} <= set(np.unique(rec["done"]).tolist())
    w2 = _perturbed(weights, 3)
    teacher, student = Raptor(device, weights=w2), Raptor(device, weights=w2)
    teacher.reset()
    ref = traj.relabel(teacher)                                 # [T, N, 4]
    student.reset()
    h_before = student.hidden_state(n)
    got = forward(traj, student, CURRENT)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)      # frozen steps may hold NaN: compare the bits
    assert np.array_equal(bits(got[:, :, :n].transpose(0, 2, 1)), bits(ref))
    assert np.array_equal(student.hidden_state(n), h_before)     # the policy's state is left alone
    assert np.array_equal(bits(forward(traj, student, INITIAL)[:, :, :n]), bits(got[:, :, :n]))   # after reset(): h0


CASES = [(1, 1), (2, 15), (37, 16), (500, 17), (2, 63), (37, 64), (1, 65), (500, 1000), (37, 65536), (2, 65536)]


@pytest.mark.parametrize("T,n", CASES)
def test_gradient_within_the_float64_bound(device, oracle, weights, T, n):
    from raptor_amd.foundation_policy import Raptor
    w, traj = _record(device, oracle, n, T, seed=50 + T + n)
    ld = _ld(traj)
    obs = traj.tensors()["obs"]
    obs[:, :, n:] = float("nan")                                # padding columns of the recording: NaN as well
    import torch
    torch.cuda.synchronize()                                    # before the engine's stream reads them (as in _record)
    rec = traj.numpy()
    wts = _perturbed(weights, 5)
    pol = Raptor(device, weights=wts)
    pol.reset()
    for start in (INITIAL, CURRENT):
        if start == CURRENT:                                    # a non-trivial current state
            pol.set_hidden_state(np.random.default_rng(9).uniform(-0.7, 0.7, (n, 16)).astype(np.float32))
        h_start = pol.hidden_state(n)
        act = forward(traj, pol, start)
        dact = _dact(T, n, ld, seed=T + n + start)
        g, gh = backward(traj, pol, dact, want_h=start == CURRENT)
        a_ref, cache = R.forward(wts.astype(np.float64), rec["obs"], rec["done"], "initial" if start else "current", h_start)
        assert np.abs(act[:, :, :n].transpose(0, 2, 1) - a_ref).max() < 1e-4
        g_ref, gh_ref = R.backward(cache, dact[:, :, :n].transpose(0, 2, 1))
        b, bh = R.bound(cache, dact[:, :, :n].transpose(0, 2, 1), waves=(n + 63) // 64)
        err = np.abs(g - g_ref)
        assert np.isfinite(g).all()
        print(f"T={T} n={n} start={start}: max err/bound {np.max(err / b):.3g}, max |g| {np.abs(g_ref).max():.3g}")
        assert (err <= b).all(), (np.argmax(err / b), np.max(err / b))
        if start == CURRENT:
            assert np.isfinite(gh).all() and not gh[:, n:].any()
            assert (np.abs(gh[:, :n].T - gh_ref) <= bh).all()


def test_gradient_is_deterministic_zero_and_linear(device, oracle, weights):
    from raptor_amd.foundation_policy import Raptor
    n, T = 1000, 120
    w, traj = _record(device, oracle, n, T, seed=61)
    ld = _ld(traj)
    pol = Raptor(device, weights=_perturbed(weights, 7))
    pol.reset()
    forward(traj, pol, INITIAL)
    d1, d2 = _dact(T, n, ld, 1), _dact(T, n, ld, 2)
    g1, _ = backward(traj, pol, d1)
    g1b, _ = backward(traj, pol, d1)
    assert np.array_equal(g1.view(np.uint32), g1b.view(np.uint32))
    forward(traj, pol, INITIAL)
    assert np.array_equal(backward(traj, pol, d1)[0].view(np.uint32), g1.view(np.uint32))
    zero = np.zeros_like(d1)
    zero[:, :, n:] = np.nan
    assert not backward(traj, pol, zero)[0].any()               # exact zeros
    assert np.array_equal(backward(traj, pol, 2 * d1)[0], 2 * g1)    # scaling by 2 is exact in every operation
    g2, _ = backward(traj, pol, d2)
    g12, _ = backward(traj, pol, d1 + d2)
    rec = traj.numpy()
    _, cache = R.forward(pol.weights.astype(np.float64), rec["obs"], rec["done"], "initial")
    tol = sum(R.bound(cache, d[:, :, :n].transpose(0, 2, 1), 16)[0] for d in (d1, d2, d1 + d2))
    assert (np.abs(g12 - (g1.astype(np.float64) + g2)) <= tol).all()


def test_h0_slice(device, oracle, weights):
    """START_CURRENT without episode ends: the initial state never enters, its gradient is exactly 0.  With ends (and with
    START_INITIAL) it is what the reference gives - covered by the bound test; here against the reference once more."""
    from raptor_amd.foundation_policy import Raptor
    n, T = 300, 30
    w, traj = _record(device, oracle, n, T, seed=71)
    done = traj.tensors()["done"]
    saved = done.clone()
    done.zero_()
    pol = Raptor(device, weights=_perturbed(weights, 8))
    pol.reset()
    forward(traj, pol, CURRENT)
    g, _ = backward(traj, pol, _dact(T, n, _ld(traj), 3))
    assert not g[2000:2016].any() and g[:2000].any()
    done.copy_(saved)
    rec = traj.numpy()
    assert ((rec["done"] == 1) | (rec["done"] == 2)).any()
    forward(traj, pol, CURRENT)
    d = _dact(T, n, _ld(traj), 4)
    g, _ = backward(traj, pol, d)
    _, cache = R.forward(pol.weights.astype(np.float64), rec["obs"], rec["done"], "current", pol.hidden_state(n))
    g_ref, _ = R.backward(cache, d[:, :, :n].transpose(0, 2, 1))
    b, _ = R.bound(cache, d[:, :, :n].transpose(0, 2, 1), 5)
    assert np.abs(g_ref[2000:2016]).max() > 0
    assert (np.abs(g - g_ref)[2000:2016] <= b[2000:2016]).all()


def test_refusals(device, oracle, weights):
    import raptor_amd.l2f as l2f
    from raptor_amd._lib import RaptorQuadError
    from raptor_amd.foundation_policy import Raptor
    n, T = 128, 10
    w, traj = _record(device, oracle, n, T, seed=81)
    ld = _ld(traj)
    d = _dact(T, n, ld, 5)
    pol = Raptor(device)
    pol.reset()

    def refused(fn, words):
        with pytest.raises(RaptorQuadError) as e:
            fn()
        assert words in str(e.value), str(e.value)

    refused(lambda: backward(traj, pol, d), "no matching forward")
    forward(traj, pol, INITIAL)
    other = Raptor(device)
    refused(lambda: backward(traj, other, d), "no matching forward")
    refused(lambda: backward(traj, pol, d, want_h=True), "RQ_GRAD_START_CURRENT only")
    pol.set_weights(weights)                                    # same values, but new weights as far as the engine knows
    refused(lambda: backward(traj, pol, d), "weights changed")
    forward(traj, pol, INITIAL)
    backward(traj, pol, d)
    for prec in ("bf16", "f16x2"):
        pol.set_precision(prec)
        refused(lambda: backward(traj, pol, d), "fp32 policy only")
        refused(lambda: forward(traj, pol, INITIAL), "fp32 policy only")
    pol.set_precision("fp32")
    pol.set_standardize(np.zeros(22, np.float32), np.ones(22, np.float32))
    refused(lambda: backward(traj, pol, d), "Standardize")
    pol.set_standardize(None)
    pol.set_squash(True)
    refused(lambda: backward(traj, pol, d), "SampleAndSquash")
    pol.set_squash(False)
    foreign = Raptor(l2f.Device(0))                             # another engine device object (same GPU)
    foreign.reset()
    foreign._handle()
    refused(lambda: forward(traj, foreign, INITIAL), "another device")
    refused(lambda: backward(traj, foreign, d), "another device")
    traj.reset()
    refused(lambda: forward(traj, pol, INITIAL, ld=ld), "empty")
    refused(lambda: backward(traj, pol, d, ld=ld), "empty")


def test_set_weights_gives_the_bits_of_a_fresh_policy_and_keeps_the_state(device, oracle, weights):
    import torch
    from raptor_amd.foundation_policy import Raptor
    n, T = 256, 24
    w2 = _perturbed(weights, 11)
    rng = np.random.default_rng(12)
    obs = rng.standard_normal((3, n, 22)).astype(np.float32)
    a = Raptor(device)
    a.reset()
    a.evaluate_step(obs[0])
    h = a.hidden_state(n)
    a.set_weights(torch.tensor(w2, device="cuda"))              # any torch tensor (numpy below)
    assert np.array_equal(a.hidden_state(n), h)
    b = Raptor(device, weights=w2)
    b.reset()
    b.set_hidden_state(h)
    assert np.array_equal(a.evaluate_step(obs[1]), b.evaluate_step(obs[1]))
    assert np.array_equal(a.evaluate_sequence(obs), b.evaluate_sequence(obs))
    # relabel and the fused rollout, from reset
    wa, traj = _record(device, oracle, n, T, seed=91)
    a.reset(); b.reset()
    assert np.array_equal(traj.relabel(a), traj.relabel(b))
    worlds = [World(device, oracle, n, seed=93, episode_step_limit=9) for _ in range(2)]
    for wd, pol in zip(worlds, (a, b)):
        pol.reset()
        wd.vector.rollout(device, wd.env, wd.params, wd.state, pol, wd.rng, T, "fused", autoreset=True)
    assert np.array_equal(worlds[0].state.numpy(), worlds[1].state.numpy())
    assert np.array_equal(a.hidden_state(n), b.hidden_state(n))
    a.set_weights(weights)                                      # numpy, and back
    c = Raptor(device)
    a.reset(); c.reset()
    assert np.array_equal(a.evaluate_step(obs[2]), c.evaluate_step(obs[2]))


def test_autograd_directional_derivatives(device, oracle, weights):
    import torch
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.training import trajectory_actions
    n, T = 512, 30
    w, traj = _record(device, oracle, n, T, seed=101)
    pol = Raptor(device, weights=_perturbed(weights, 13))
    target = torch.randn((T, 4, n), device="cuda", generator=torch.Generator("cuda").manual_seed(0))

    def loss(wt):
        return ((trajectory_actions(traj, pol, wt)[:, :, :n] - target) ** 2).mean()

    wt = torch.tensor(pol.weights, device="cuda", requires_grad=True)
    L = loss(wt)
    L.backward()
    grad = wt.grad.double()
    gen = torch.Generator("cuda").manual_seed(1)
    for _ in range(3):
        v = torch.randn(2084, device="cuda", generator=gen)
        v = v / v.norm()
        eps = 1e-2
        with torch.no_grad():
            fd = (loss(wt + eps * v).double() - loss(wt - eps * v).double()) / (2 * eps)
        an = (grad * v.double()).sum()
        assert abs(float(fd - an)) <= 2e-2 * abs(float(an)) + 1e-5, (float(fd), float(an))


def test_twenty_adam_steps_halve_the_distillation_loss(device, oracle, weights):
    """Distil a perturbed student toward the shipped policy's labels: 4 096 envs x 100 steps, MSE masked by done != 4
    (raptor_amd.training.masked_mse).  The observations of frozen steps are unspecified; here they are made NaN on purpose, so
    that the actions and labels there are NaN: the masked loss must give them no gradient, and every step must stay finite."""
    import torch
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.training import masked_mse, trajectory_actions
    torch.manual_seed(0)
    n, T = 4096, 100
    w, traj = _record(device, oracle, n, T, seed=111, finite=False)
    frozen = traj.tensors()["done"] == 4
    assert frozen[:, :n].any()
    obs = traj.tensors()["obs"]
    obs.copy_(torch.where(frozen[:, None, :], float("nan"), obs))
    teacher = Raptor(device)
    teacher.reset()
    labels = torch.tensor(traj.relabel(teacher).transpose(0, 2, 1).copy(), device="cuda")    # [T, 4, N]
    live = (~frozen[:, :n])[:, None, :].expand(T, 4, n)
    assert torch.isnan(labels[~live]).all()
    student = Raptor(device, weights=_perturbed(weights, 17, scale=0.02))
    wt = torch.tensor(student.weights, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([wt], lr=2e-3)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        act = trajectory_actions(traj, student, wt)[:, :, :n]
        loss = masked_mse(act, labels, live)
        loss.backward()
        assert torch.isfinite(wt.grad).all()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        act = trajectory_actions(traj, student, wt)[:, :, :n]
        final = float(masked_mse(act, labels, live))
    print("distillation MSE:", [f"{x:.3g}" for x in losses], f"final {final:.3g}")
    assert final <= 0.5 * losses[0]


@pytest.mark.parametrize("n", [64, 1000])
def test_gradient_over_one_500_step_episode(device, oracle, weights, n):
    """Back-propagation through a recurrent chain as long as the recording: 500 steps, no episode end, no frozen step.  The bound
    is an outer one at this horizon (its A grows like the product of |J| over the episode, see the reference's docstring): the case
    checks that the long recursion stays finite and inside it, and prints the relative error against the float64 reference."""
    from raptor_amd.foundation_policy import Raptor
    T = 500
    w, traj = _record(device, oracle, n, T, seed=121)
    traj.tensors()["done"].zero_()
    rec = traj.numpy()
    ld = _ld(traj)
    wts = _perturbed(weights, 19)
    pol = Raptor(device, weights=wts)
    pol.reset()
    forward(traj, pol, INITIAL)
    dact = _dact(T, n, ld, seed=7)
    g, _ = backward(traj, pol, dact)
    _, cache = R.forward(wts.astype(np.float64), rec["obs"], rec["done"], "initial")
    g_ref, _ = R.backward(cache, dact[:, :, :n].transpose(0, 2, 1))
    b, _ = R.bound(cache, dact[:, :, :n].transpose(0, 2, 1), waves=(n + 63) // 64)
    rel = np.abs(g - g_ref).max() / np.abs(g_ref).max()
    print(f"one 500-step episode, n={n}: max |g - g_ref| / max |g_ref| = {rel:.3g}, max |g_ref| {np.abs(g_ref).max():.3g}")
    assert np.isfinite(g).all() and (np.abs(g - g_ref) <= b).all()


def test_other_strides_and_asynchronous_device_memory(device, oracle, weights):
    """ld_action / ld_grad other than the trajectory's ld, host and device memory, synchronous and RQ_DST_DEVICE_ASYNC: the same
    bits as the default call."""
    import ctypes as C
    import torch
    from raptor_amd.foundation_policy import Raptor
    L = _lib()
    n, T = 100, 20
    w, traj = _record(device, oracle, n, T, seed=131)
    ld = _ld(traj)
    assert ld == 128
    pol = Raptor(device, weights=_perturbed(weights, 23))
    pol.reset()
    h = traj._require("trajectory")
    ref = forward(traj, pol, INITIAL)[:, :, :n]
    wide = np.full((T, 4, ld + 7), -1.0, np.float32)
    L.call("rq_trajectory_policy_forward", h, pol._handle(), INITIAL, L.fptr(wide), ld + 7, 0)
    assert np.array_equal(wide[:, :, :n], ref)
    assert (wide[:, :, n:] == -1.0).all()                        # the caller's other columns are left alone
    for memory in (1, 2):
        narrow = torch.full((T, 4, n), -1.0, device="cuda")
        torch.cuda.synchronize()
        L.call("rq_trajectory_policy_forward", h, pol._handle(), INITIAL, C.c_void_p(narrow.data_ptr()), n, memory)
        L.call("rq_device_synchronize", device._h)
        assert np.array_equal(narrow.cpu().numpy(), ref)
    d = _dact(T, n, ld, 11)
    g_ref, _ = backward(traj, pol, d)
    dw = np.full((T, 4, ld + 5), np.nan, np.float32)
    dw[:, :, :ld] = d
    g = np.empty(2084, np.float32)
    L.call("rq_trajectory_policy_backward", h, pol._handle(), L.fptr(dw), ld + 5, L.fptr(g), None, 0)
    assert np.array_equal(g.view(np.uint32), g_ref.view(np.uint32))
    dn = torch.tensor(np.ascontiguousarray(d[:, :, :n]), device="cuda")
    gd = torch.empty(2084, device="cuda")
    for memory in (1, 2):
        gd.fill_(np.nan)
        torch.cuda.synchronize()
        L.call("rq_trajectory_policy_backward", h, pol._handle(), C.c_void_p(dn.data_ptr()), n, C.c_void_p(gd.data_ptr()), None,
               memory)
        L.call("rq_device_synchronize", device._h)
        assert np.array_equal(gd.cpu().numpy().view(np.uint32), g_ref.view(np.uint32))


def test_autograd_refuses_a_backward_whose_forward_was_replaced(device, oracle, weights):
    """The trajectory holds the saved state of its latest forward only: an earlier forward's backward must raise, not use it."""
    import torch
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.training import trajectory_actions
    n, T = 128, 10
    w, traj = _record(device, oracle, n, T, seed=141)
    pol = Raptor(device, weights=_perturbed(weights, 29))
    pol.reset()
    wt = torch.tensor(pol.weights, device="cuda", requires_grad=True)
    first = trajectory_actions(traj, pol, wt, start="initial")
    second = trajectory_actions(traj, pol, wt, start="current")
    with pytest.raises(RuntimeError, match="earlier forward"):
        first[:, :, :n].sum().backward()
    wt.grad = None
    second[:, :, :n].sum().backward()
    assert torch.isfinite(wt.grad).all() and wt.grad.abs().max() > 0
