"""What the distillation GPU tests share (tests/test_gpu_distill.py): recordings with every done code, made the way
tests/test_gpu_policy_grad.py makes its own (the functions are restated here so that the two suites' cases do not move together),
perturbed weights, and the learner's forward through the C ABI."""
import numpy as np

from gpu_common import World


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
    done = traj.tensors()["done"]
    ends = (done == 2).nonzero()
    done[ends[::2, 0], ends[::2, 1]] = 1
    if finite:
        import torch
        obs = traj.tensors()["obs"]
        draw = torch.randn(obs.shape, device=obs.device, generator=torch.Generator(obs.device).manual_seed(seed))
        obs.copy_(torch.where((done == 4)[:, None, :], draw, obs))
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
