"""What the distillation GPU tests share (tests/test_gpu_distill.py, tests/test_gpu_bank_distill.py): recordings with every done
code, made the way tests/test_gpu_policy_grad.py makes its own (the functions are restated here so that the two suites' cases do
not move together), perturbed weights, labels, and the single-policy learner through the C ABI: forward, loss and gradient, the
optimizer, updates, the weights read back."""
import ctypes as C

import numpy as np

from gpu_common import World


CURRENT, INITIAL = 0, 1          # where the forward starts: the policy's current hidden state, its initial one
HOST, DEVICE, ASYNC = 0, 1, 2    # where the results go


def _lib():
    from raptor_amd import _lib as L
    return L


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


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


def _perturbed(weights, seed, scale=0.05):
    w = (weights + np.random.default_rng(seed).standard_normal(weights.size).astype(np.float32) * scale).astype(np.float32)
    w[2000:2016] = np.random.default_rng(seed + 1).uniform(-0.3, 0.3, 16).astype(np.float32)
    return w


def _targets(traj, n, seed, nan_frozen=True):
    """[T, 4, ld] float32: N(0, 1) labels; NaN in the padding columns and on frozen steps"""
    rec = traj.numpy()
    T, ld = len(traj), _ld(traj)
    y = np.full((T, 4, ld), np.nan, np.float32)
    y[:, :, :n] = np.random.default_rng(seed).standard_normal((T, 4, n)).astype(np.float32)
    if nan_frozen:
        y[:, :, :n][np.broadcast_to((rec["done"] == 4)[:, None, :], (T, 4, n))] = np.nan
    return y


def _adam(cfg):
    return _lib().AdamConfig(cfg["lr"], cfg["betas"][0], cfg["betas"][1], cfg["eps"], cfg["wd"])


def loss_grad(traj, pol, target=None, start=INITIAL, ld=None):
    L = _lib()
    loss, g = np.empty(1, np.float32), np.empty(2084, np.float32)
    t = None if target is None else np.ascontiguousarray(target, np.float32)
    L.call("rq_trajectory_policy_loss_grad", traj._require("trajectory"), pol._handle(), None if t is None else L.fptr(t),
           0 if t is None else (ld or t.shape[2]), start, L.fptr(loss), L.fptr(g), HOST)
    return loss[0], g


class Opt:
    def __init__(self, pol, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.0):
        self.cfg, self.h = _adam(dict(lr=lr, betas=betas, eps=eps, wd=wd)), C.c_void_p()
        _lib().call("rq_optimizer_create", pol._handle(), C.byref(self.cfg), C.byref(self.h))

    def close(self):
        _lib().call("rq_optimizer_destroy", self.h)


def opt_state(opt, slots=None, name="rq_optimizer_get_state"):
    """-> (m, v, step, powers) of an Opt; ``slots``: a bank optimizer's P ([P, 2084], [P], [P, 2])"""
    L = _lib()
    shape = (2084,) if slots is None else (slots, 2084)
    m, v = np.full(shape, np.nan, np.float32), np.full(shape, np.nan, np.float32)
    step, powers = np.zeros(slots or 1, np.uint32), np.full((slots or 1, 2), np.nan, np.float64)
    L.call(name, opt.h, L.fptr(m), L.fptr(v), step.ctypes.data, powers.ctypes.data)
    return (m, v, int(step[0]), powers[0]) if slots is None else (m, v, step, powers)


def opt_set_state(opt, m, v, step, powers):
    L = _lib()
    m, v, powers = np.ascontiguousarray(m, np.float32), np.ascontiguousarray(v, np.float32), np.ascontiguousarray(powers, np.float64)
    L.call("rq_optimizer_set_state", opt.h, L.fptr(m), L.fptr(v), int(step), powers.ctypes.data)


def opt_apply(opt, grad):
    L = _lib()
    g = np.ascontiguousarray(grad, np.float32)
    L.call("rq_optimizer_apply", opt.h, L.fptr(g), HOST)


def distill(traj, pol, opt, n_updates, target=None, start=INITIAL):
    L = _lib()
    losses = np.empty(n_updates, np.float32)
    t = None if target is None else np.ascontiguousarray(target, np.float32)
    L.call("rq_trajectory_distill", traj._require("trajectory"), pol._handle(), opt.h, None if t is None else L.fptr(t),
           0 if t is None else t.shape[2], start, n_updates, L.fptr(losses), HOST)
    return losses


def get_weights(pol):
    L = _lib()
    w = np.empty(2084, np.float32)
    L.call("rq_policy_get_weights", pol._handle(), L.fptr(w))
    return w
