"""The distillation update on the GPU (rq_trajectory_policy_loss_grad, rq_optimizer_*, rq_trajectory_distill, rq_policy_get_weights;
csrc/rq_grad.hpp; raptor_amd.training.Distiller): loss and gradient against float64 and their bounds, determinism, the masks, Adam's
arithmetic, the device-side repack against a policy packed on the host, ordering and staleness, the refusals, and ten updates
against today's torch path.

Slack of each accuracy case: ``pytest tests/test_gpu_distill.py -m gpu -v -s``."""
import ctypes as C

import numpy as np
import pytest

import distill_reference as D
import policy_grad_reference as R
from distill_common import (ASYNC, DEVICE, HOST, INITIAL, Opt, _bits, _ld, _lib, _perturbed, _record, _targets, distill, forward,
                            get_weights, loss_grad, opt_state)
from gpu_common import World

pytestmark = pytest.mark.gpu

# Roundings the loss seed adds on a path from dL/da to a gradient element, beyond policy_grad_reference.K_paths, counted from the
# kernels: the fp32 subtract a - y in k_policy_loss_backward, and the one rounding to fp32 of acc * (2 / M) in k_policy_loss_reduce.
# That product is formed in float64 (1 / M, 2 x, the product: three roundings of 2^-53 each, together below 2^-27 of one fp32
# rounding), carried as the fraction.
C_SEED = 2 + 2.0 ** -27


CASES = [(1, 1), (37, 16), (2, 63), (1, 65), (500, 1000), (37, 65536)]


@pytest.mark.parametrize("T,n", CASES)
def test_loss_and_gradient_within_the_float64_bounds(device, oracle, weights, T, n):
    from raptor_amd.foundation_policy import Raptor
    w, traj = _record(device, oracle, n, T, seed=50 + T + n)
    traj.tensors()["obs"][:, :, n:] = float("nan")               # padding columns of the recording: NaN
    rec = traj.numpy()
    wts = _perturbed(weights, 5)
    pol = Raptor(device, weights=wts)
    pol.reset()
    y = _targets(traj, n, seed=T + n)
    act = forward(traj, pol, INITIAL)                            # the device's own fp32 actions
    loss, g = loss_grad(traj, pol, y)
    live = np.broadcast_to((rec["done"] != 4)[:, None, :], (T, 4, n))
    M = int(live.sum())
    ref_loss, seed, terms = D.masked_mse(act[:, :, :n], y[:, :, :n], live)
    lb = D.loss_bound(terms, M)
    print(f"T={T} n={n}: M {M}, loss {loss:.6g}, |loss - ref| / bound {abs(loss - ref_loss) / lb:.3g}")
    assert np.isfinite(loss) and abs(loss - ref_loss) <= lb
    _, cache = R.forward(wts.astype(np.float64), rec["obs"], rec["done"], "initial")
    dact = seed.transpose(0, 2, 1)                               # [T, N, 4], 2 (a_dev - y) / M on live entries
    g_ref, _ = R.backward(cache, dact)
    waves = (n + 63) // 64
    K = R.K_paths(T, waves)
    b = R.bound(cache, dact, waves)[0] * (K + C_SEED) / K
    err = np.abs(g - g_ref)
    assert np.isfinite(g).all()
    print(f"T={T} n={n}: max err/bound {np.max(err / b):.3g}, max |g| {np.abs(g_ref).max():.3g}")
    assert (err <= b).all(), (np.argmax(err / b), np.max(err / b))


def test_deterministic_masked_and_indifferent_to_the_targets_stride(device, oracle, weights):
    import torch
    from raptor_amd.foundation_policy import Raptor
    L = _lib()
    n, T = 1000, 60
    w, traj = _record(device, oracle, n, T, seed=61)
    ld = _ld(traj)
    pol = Raptor(device, weights=_perturbed(weights, 7))
    pol.reset()
    y = _targets(traj, n, seed=1)
    l1, g1 = loss_grad(traj, pol, y)
    l2, g2 = loss_grad(traj, pol, y)
    assert _bits(g1).tolist() == _bits(g2).tolist() and _bits(l1) == _bits(l2) and g1.any()
    # another ld_target: the same bits
    wide = np.full((T, 4, ld + 5), np.nan, np.float32)
    wide[:, :, :ld] = y
    l3, g3 = loss_grad(traj, pol, wide)
    assert np.array_equal(_bits(g3), _bits(g1)) and _bits(l3) == _bits(l1)
    l3, g3 = loss_grad(traj, pol, np.ascontiguousarray(y[:, :, :n]))
    assert np.array_equal(_bits(g3), _bits(g1)) and _bits(l3) == _bits(l1)
    # target = None: the stored actions
    stored = traj.tensors()["act"]
    stored.copy_(torch.tensor(y, device=stored.device))
    l4, g4 = loss_grad(traj, pol, None)
    assert np.array_equal(_bits(g4), _bits(g1)) and _bits(l4) == _bits(l1)
    # device memory, synchronous and enqueued only
    yd = torch.tensor(y, device="cuda")
    for memory in (DEVICE, ASYNC):
        ld_, gd = torch.full((1,), np.nan, device="cuda"), torch.full((2084,), np.nan, device="cuda")
        torch.cuda.synchronize()
        L.call("rq_trajectory_policy_loss_grad", traj._require("trajectory"), pol._handle(), C.c_void_p(yd.data_ptr()), ld, INITIAL,
               C.c_void_p(ld_.data_ptr()), C.c_void_p(gd.data_ptr()), memory)
        L.call("rq_device_synchronize", device._h)
        assert np.array_equal(_bits(gd.cpu().numpy()), _bits(g1)) and _bits(ld_.cpu().numpy()) == _bits(l1)
    # what the observations of frozen steps hold does not matter: NaN there, the same bits
    obs = traj.tensors()["obs"]
    frozen = traj.tensors()["done"] == 4
    assert frozen[:, :n].any()
    obs.copy_(torch.where(frozen[:, None, :], float("nan"), obs))
    l5, g5 = loss_grad(traj, pol, y)
    assert np.array_equal(_bits(g5), _bits(g1)) and _bits(l5) == _bits(l1)
    # every step frozen: M = 0, loss 0, gradient 0 - not NaN
    traj.tensors()["done"].fill_(4)
    l6, g6 = loss_grad(traj, pol, y)
    assert l6 == 0.0 and not g6.any()


def test_one_update_is_adam_in_float64_to_a_rounding(device, oracle, weights):
    """rq_trajectory_distill(n_updates = 1), twice, against float64 Adam applied to the fp32 inputs: the gradient fetched with
    loss_grad beforehand, the weights read back, and the moments, step count and running powers read through
    rq_optimizer_get_state.  k_adam_repack forms m', v' and w' in float64 from the fp32 inputs and rounds each to fp32 ONCE, so
      update 1 (m = v = 0, exact inputs): |w1 - ref| <= u |ref|   (+ the float64 roundings of the expression, < 2^-48 relative),
        against tests/distill_reference.Adam; m1 and v1 within one rounding of its moments;
      update 2: w1, m1, v1 (the device's own bits, read back) and g2 are exact inputs, so w2, m2 and v2 lie within the one-rounding
        bound of tests/adam_reference.py - no propagation term.  An error of the gradient does not enter."""
    import adam_reference as A
    from raptor_amd.foundation_policy import Raptor
    n, T = 300, 30
    lr, b1, b2, eps = 3e-3, 0.9, 0.999, 1e-8
    cfg = (lr, b1, b2, eps, 0.0)
    w, traj = _record(device, oracle, n, T, seed=71)
    pol = Raptor(device, weights=_perturbed(weights, 8))
    pol.reset()
    y = _targets(traj, n, seed=2)
    opt = Opt(pol, lr=lr, betas=(b1, b2), eps=eps)
    w0 = get_weights(pol)
    assert np.array_equal(w0, pol.weights)
    m0, v0, step0, p0 = opt_state(opt)
    assert not m0.any() and not v0.any() and step0 == 0 and p0.tolist() == [1.0, 1.0]
    loss0, g1 = loss_grad(traj, pol, y)
    losses = distill(traj, pol, opt, 1, y)
    assert _bits(losses[0]) == _bits(loss0)
    w1 = get_weights(pol)
    m1, v1, step1, p1 = opt_state(opt)
    ref = D.Adam(w0, lr=lr, betas=(b1, b2), eps=eps)
    r1 = ref.step(g1)
    slack = 1.0 + 2.0 ** -20
    e1 = np.abs(w1 - r1)
    print("update 1: max |w - ref| / (u |ref|)", np.max(e1 / (D.U * np.abs(r1) + 2.0 ** -150)))
    assert (e1 <= slack * D.U * np.abs(r1) + 2.0 ** -150).all() and np.abs(w1 - w0).max() > 0.5 * lr
    assert (np.abs(m1 - ref.m) <= slack * D.U * np.abs(ref.m) + 2.0 ** -126).all() and m1.any()
    assert (np.abs(v1 - ref.v) <= slack * D.U * np.abs(ref.v) + 2.0 ** -126).all() and v1.any()
    assert step1 == 1 and p1.tolist() == [b1, b2]
    _, g2 = loss_grad(traj, pol, y)
    distill(traj, pol, opt, 1, y)
    w2 = get_weights(pol)
    m2, v2, step2, p2 = opt_state(opt)
    r2 = A.adam_exact(w1, m1, v1, g2, cfg, p1)                   # from the exact inputs of the second update
    bound = A.bound(w1, m1, v1, g2, cfg, p1)
    for name, got, r, b in zip(("w", "m", "v"), (w2, m2, v2), r2, bound):
        ok, ratio = A.agrees(got, r, b)
        print(f"update 2: max |{name} - ref| / bound", ratio.max())
        assert ok.all(), (name, int(np.argmax(ratio)), ratio.max())
    assert step2 == 2 and p2.tolist() == [b1 * b1, b2 * b2]
    opt.close()


def _same_everywhere(device, oracle, a, b, traj, y, n):
    """policies a and b compute the same bits: evaluate_step, the learner's forward, loss_grad (the transposed image), a rollout"""
    obs = np.random.default_rng(12).standard_normal((n, 22)).astype(np.float32)
    a.reset(); b.reset()
    assert np.array_equal(_bits(a.evaluate_step(obs)), _bits(b.evaluate_step(obs)))
    assert np.array_equal(_bits(forward(traj, a, INITIAL)[:, :, :n]), _bits(forward(traj, b, INITIAL)[:, :, :n]))
    la, ga = loss_grad(traj, a, y)
    lb, gb = loss_grad(traj, b, y)
    assert np.array_equal(_bits(ga), _bits(gb)) and _bits(la) == _bits(lb)
    worlds = [World(device, oracle, n, seed=93, episode_step_limit=9) for _ in range(2)]
    for wd, pol in zip(worlds, (a, b)):
        pol.reset()
        wd.vector.rollout(device, wd.env, wd.params, wd.state, pol, wd.rng, 20, "fused", autoreset=True)
    assert np.array_equal(worlds[0].state.numpy(), worlds[1].state.numpy())
    assert np.array_equal(a.hidden_state(n), b.hidden_state(n))


@pytest.mark.parametrize("k", [1, 7])
def test_the_device_repack_equals_a_policy_packed_on_the_host(device, oracle, weights, k):
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.training import Distiller
    n, T = 256, 24
    w, traj = _record(device, oracle, n, T, seed=91)
    y = _targets(traj, n, seed=3)
    pol = Raptor(device, weights=_perturbed(weights, 11))
    pol.reset()
    before = pol.weights.copy()
    Distiller(pol, lr=2e-3).step(traj, target=y, updates=k)
    fresh = Raptor(device, weights=pol.weights)                  # the updated weights, packed on the host
    assert np.abs(fresh.weights - before).max() > 1e-3
    _same_everywhere(device, oracle, pol, fresh, traj, y, n)


def test_five_updates_in_one_call_are_five_calls(device, oracle, weights):
    from raptor_amd.foundation_policy import Raptor
    n, T = 200, 20
    w, traj = _record(device, oracle, n, T, seed=95)
    y = _targets(traj, n, seed=4)
    out = []
    for calls in ((5,), (1, 1, 1, 1, 1)):
        pol = Raptor(device, weights=_perturbed(weights, 12))
        pol.reset()
        opt = Opt(pol, lr=2e-3, wd=0.01)
        losses = np.concatenate([distill(traj, pol, opt, c, y) for c in calls])
        out.append((losses, get_weights(pol)))
        opt.close()
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0])) and np.array_equal(_bits(out[0][1]), _bits(out[1][1]))
    assert len(set(out[0][0].tolist())) == 5


def test_ten_updates_follow_todays_torch_path(device, oracle, weights):
    """trajectory_actions + masked_mse + torch.optim.Adam + set_weights against Distiller.step, ten updates from the same start.
    Both gradients lie within R.bound of the float64 gradient, but Adam's early steps move every weight by about lr whatever the
    gradient's size, so where the sign of a tiny gradient element differs the weights part by up to 2 lr per step: the WEIGHTS are
    not compared.  The losses are: after k updates the two weight vectors differ by at most 2 lr k per element, so the losses by at
    most 2 lr k ||grad L||_1 to first order, with ||grad L||_1 taken from the float64 reference at the start (the loss falls, the
    gradient with it; the factor 2 below covers the second order)."""
    import torch
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.training import Distiller, masked_mse, trajectory_actions
    n, T, lr, updates = 512, 40, 1e-3, 10
    w, traj = _record(device, oracle, n, T, seed=111)
    rec = traj.numpy()
    teacher = Raptor(device)
    teacher.reset()
    labels = torch.tensor(traj.relabel(teacher).transpose(0, 2, 1).copy(), device="cuda")       # [T, 4, N]
    live = torch.tensor(rec["done"] != 4, device="cuda")[:, None, :].expand(T, 4, n)
    w0 = _perturbed(weights, 17, scale=0.02)
    # today's path
    student = Raptor(device, weights=w0)
    wt = torch.tensor(w0, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([wt], lr=lr)
    torch_losses = []
    for _ in range(updates):
        opt.zero_grad()
        loss = masked_mse(trajectory_actions(traj, student, wt)[:, :, :n], labels, live)
        loss.backward()
        opt.step()
        torch_losses.append(float(loss.detach()))
    # the device's
    pol = Raptor(device, weights=w0)
    dist = Distiller(pol, lr=lr)
    losses = dist.step(traj, target=labels, updates=updates).cpu().numpy()
    final, _ = dist.loss_and_grad(traj, target=labels)
    # float64: the gradient at the start
    a64, cache = R.forward(w0.astype(np.float64), rec["obs"], rec["done"], "initial")
    lv = np.broadcast_to((rec["done"] != 4)[:, :, None], (T, n, 4))
    _, seed, _ = D.masked_mse(a64, labels.cpu().numpy().transpose(0, 2, 1), lv)
    g64, _ = R.backward(cache, seed)
    l1 = np.abs(g64).sum()
    print("torch :", [f"{x:.4g}" for x in torch_losses])
    print("device:", [f"{x:.4g}" for x in losses], f"final {float(final):.4g}; lr ||g||_1 = {lr * l1:.3g}")
    with torch.no_grad():
        torch_final = float(masked_mse(trajectory_actions(traj, student, wt)[:, :, :n], labels, live))
    for k in range(updates):
        tol = 2 * (2 * lr * k * l1) + 1e-6 * torch_losses[k]
        print(f"update {k}: |device - torch| {abs(losses[k] - torch_losses[k]):.3g}, drift tolerance {tol:.3g} = {tol / torch_losses[k]:.3g} x loss")
        assert abs(losses[k] - torch_losses[k]) <= tol, k
    assert float(final) < losses[0] and (np.diff(losses) < 0).all()
    # The drift tolerance is loose by construction (||g||_1 over 2 084 elements).  What bites: the two paths make the same progress.
    # Where they can part at all is in elements whose gradient is at the fp32 rounding level, which carry none of the fall; a
    # different update rule (no bias correction, another epsilon placement) changes the early step sizes severalfold.  So the
    # losses after the ten updates agree within a tenth of the fall, and the first losses - the same weights - to fp32 summation.
    fall = losses[0] - float(final)
    print(f"final: device {float(final):.6g}, torch {torch_final:.6g}, fall {fall:.3g}")
    assert abs(float(final) - torch_final) <= 0.1 * fall
    assert abs(losses[0] - torch_losses[0]) <= 1e-5 * torch_losses[0]


def test_ordering_and_staleness(device, oracle, weights):
    import torch
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.training import Distiller
    n, T = 256, 24
    w, traj = _record(device, oracle, n, T, seed=131)
    y = torch.tensor(_targets(traj, n, seed=5), device="cuda")
    pol = Raptor(device, weights=_perturbed(weights, 13))
    pol.reset()
    dist = Distiller(pol, lr=2e-3)
    # an enqueued-only update, a rollout right behind it on the engine's stream: it flies the new weights
    world = World(device, oracle, n, seed=97, episode_step_limit=9)
    dist.step(traj, target=y, updates=3, wait=False)
    pol.reset()
    world.vector.rollout(device, world.env, world.params, world.state, pol, world.rng, 20, "fused", autoreset=True)
    new = pol.weights                                            # fetched from the device now
    assert np.abs(new - _perturbed(weights, 13)).max() > 1e-3
    fresh = Raptor(device, weights=new)
    other = World(device, oracle, n, seed=97, episode_step_limit=9)
    fresh.reset()
    other.vector.rollout(device, other.env, other.params, other.state, fresh, other.rng, 20, "fused", autoreset=True)
    assert np.array_equal(world.state.numpy(), other.state.numpy())
    assert np.array_equal(pol.hidden_state(n), fresh.hidden_state(n))
    # a 16-bit precision selected after an update packs from the updated weights
    dist.step(traj, target=y, updates=1)
    obs = np.random.default_rng(14).standard_normal((n, 22)).astype(np.float32)
    for prec in ("bf16", "f16x2"):
        pol.set_precision(prec)
        ref = Raptor(device, weights=pol.weights, precision=prec)
        pol.reset(); ref.reset()
        assert np.array_equal(_bits(pol.evaluate_step(obs)), _bits(ref.evaluate_step(obs)))
    pol.set_precision("fp32")
    # the resident executor (the policy alone at 8 rows, called in a row) is retired by an update; the next step has the new weights
    small = obs[:8]
    pol.reset()
    for _ in range(6):
        pol.evaluate_step(small)
    h = pol.hidden_state(8)
    for _ in range(6):
        pol.evaluate_step(small)
    pol.set_hidden_state(h)
    dist.step(traj, target=y, updates=1)
    got = pol.evaluate_step(small)
    ref = Raptor(device, weights=pol.weights)
    ref.reset()
    ref.set_hidden_state(h)
    assert np.array_equal(_bits(got), _bits(ref.evaluate_step(small)))
    # set_lr: in stream order, and a rate of 0 leaves the weights alone
    before = pol.weights.copy()
    dist.set_lr(0.0)
    dist.step(traj, target=y, updates=2)
    assert np.array_equal(_bits(pol.weights), _bits(before))


def test_refusals(device, oracle, weights):
    import torch
    import raptor_amd.l2f as l2f
    from raptor_amd._lib import RaptorQuadError
    from raptor_amd.foundation_policy import Raptor
    L = _lib()
    n, T = 128, 10
    w, traj = _record(device, oracle, n, T, seed=81)
    ld = _ld(traj)
    y = _targets(traj, n, seed=6)
    pol = Raptor(device)
    pol.reset()
    opt = Opt(pol)

    def refused(fn, words):
        with pytest.raises(RaptorQuadError) as e:
            fn()
        assert words in str(e.value), str(e.value)

    both = (lambda: loss_grad(traj, pol, y), lambda: distill(traj, pol, opt, 1, y))
    for prec in ("bf16", "f16x2"):
        pol.set_precision(prec)
        for fn in both:
            refused(fn, "fp32 policy only")
    pol.set_precision("fp32")
    pol.set_standardize(np.zeros(22, np.float32), np.ones(22, np.float32))
    for fn in both:
        refused(fn, "Standardize")
    pol.set_standardize(None)
    pol.set_squash(True)
    for fn in both:
        refused(fn, "SampleAndSquash")
    pol.set_squash(False)
    for fn in (lambda: loss_grad(traj, pol, y[:, :, :n - 1]), lambda: distill(traj, pol, opt, 1, y[:, :, :n - 1])):
        refused(fn, "ld_target")
    # device memory is announced, host memory is given: not a target on the trajectory's device
    loss_d, g_d = torch.empty(1, device="cuda"), torch.empty(2084, device="cuda")
    refused(lambda: L.call("rq_trajectory_policy_loss_grad", traj._require("trajectory"), pol._handle(), L.fptr(y), ld, INITIAL,
                           C.c_void_p(loss_d.data_ptr()), C.c_void_p(g_d.data_ptr()), DEVICE), "another device")
    other = Raptor(device)
    other.reset()
    refused(lambda: distill(traj, other, opt, 1, y), "another policy")
    foreign = Raptor(l2f.Device(0))                              # another engine device object (same GPU)
    foreign.reset()
    foreign._handle()
    refused(lambda: loss_grad(traj, foreign, y), "another device")
    refused(lambda: L.call("rq_trajectory_distill", traj._require("trajectory"), pol._handle(), opt.h, None, 0, INITIAL, 0,
                           L.fptr(np.empty(1, np.float32)), HOST), "n_updates")
    distill(traj, pol, opt, 1, y)                                # and after all that it works
    traj.reset()
    for fn in both:
        refused(fn, "empty")
    opt.close()
