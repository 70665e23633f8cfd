"""The learner half of distillation (README.md:208-216): the student's actions over a recorded trajectory as a differentiable
torch function, so that collect -> relabel -> loss -> gradient -> update stays on the device.

    from raptor_amd.training import masked_mse, trajectory_actions
    w = torch.tensor(policy.weights, device="cuda", requires_grad=True)
    act = trajectory_actions(traj, policy, w)              # [T, 4, ld], the layout of traj.tensors()["act"]
    loss = masked_mse(act, target, live)                  # live: [T, 4, ld] bool: done != 4 on the envs' columns, False on padding
    loss.backward()                                         # w.grad: dL/dtheta, 2 084 floats in the checkpoint order

The forward is one HIP launch, the backward two (rq_trajectory_policy_forward / _backward, csrc/rq_grad.hpp); the optimiser is
torch's.  Only the fp32 policy without Standardize / SampleAndSquash stages has a gradient here.
"""
import ctypes as C

import numpy as np

from . import _lib

START = {"current": 0, "initial": 1}


def _device_ptr(t):
    return C.c_void_p(t.data_ptr())


def trajectory_actions(traj, policy, weights, start="initial"):
    """The actions of ``policy`` with parameters ``weights`` on every recorded step of ``traj`` (rq_trajectory_relabel's episode
    rules) -> a [T, 4, ld] float32 device tensor laid out like ``traj.tensors()["act"]`` (env i at index i < N of the last axis;
    the padding columns hold nothing defined and receive no gradient).

    ``weights``: a [2084] float32 tensor on the trajectory's device, usually a leaf with ``requires_grad``; when its values differ
    from the policy's they are pushed into it first (``Raptor.set_weights``).  ``start``: "initial" - every env starts from the
    learned initial state, whose gradient counts - or "current" - from the policy's current hidden state, a constant.  The
    backward returns ``dL/dweights``.  Both directions order themselves against torch's current stream as
    ``Raptor.evaluate_sequence`` does.

    The trajectory keeps the state saved by its LAST forward only: a backward whose forward is no longer the trajectory's latest
    (another ``trajectory_actions`` call on the same trajectory in between, even under ``torch.no_grad``) raises instead of
    differentiating the other forward.  A loss with two terms over one trajectory (e.g. both start modes) takes one backward per
    term, each right after its forward."""
    return _TrajectoryActions.apply(weights, traj, policy, start)


def masked_mse(act, target, live):
    """Mean of (act - target)^2 over the entries where ``live`` is True (e.g. ``done != 4`` broadcast over the 4 actions).

    The mask is applied to the loss's INPUTS: outside ``live`` both act and target are replaced by 0 before the difference, so
    dL/dact is exactly 0 there even when act or target hold NaN or infinity - as they may on frozen steps, whose observations a
    recording leaves unspecified.  Masking the output instead (``torch.where(live, (act - target) ** 2, 0)`` or a 0/1 factor)
    does not: the square's backward multiplies the zero upstream gradient by 2 (act - target), and 0 x NaN is NaN."""
    import torch
    zero = torch.zeros((), dtype=act.dtype, device=act.device)
    a = torch.where(live, act, zero)
    t = torch.where(live, target, zero)
    return ((a - t) ** 2).sum() / live.sum()


def _sync_weights(policy, weights):
    host = weights.detach().to("cpu").numpy()
    if host.shape != (_lib.POLICY_NUM_WEIGHTS,) or host.dtype != np.float32:
        raise ValueError(f"weights must be a float32 tensor of {_lib.POLICY_NUM_WEIGHTS} values")
    if not np.array_equal(host.view(np.uint32), policy.weights.view(np.uint32)):
        policy.set_weights(host)


try:
    import torch

    class _TrajectoryActions(torch.autograd.Function):
        @staticmethod
        def forward(ctx, weights, traj, policy, start):
            if start not in START:
                raise ValueError('start must be "initial" or "current"')
            dev = traj.tensors()["act"].device
            if weights.device != dev:
                raise ValueError(f"weights must live on the trajectory's device ({dev})")
            _sync_weights(policy, weights)
            T = len(traj)
            ld = traj.tensors()["act"].shape[2]
            act = torch.empty((T, _lib.POLICY_OUTPUT_DIM, ld), dtype=torch.float32, device=dev)
            torch.cuda.current_stream(dev).synchronize()          # the engine runs on its own stream
            _lib.call("rq_trajectory_policy_forward", traj._require("trajectory"), policy._handle(traj._env._device),
                      START[start], _device_ptr(act), ld, 1)
            traj._learner_forwards = getattr(traj, "_learner_forwards", 0) + 1     # what the trajectory's saved state belongs to
            ctx.traj, ctx.policy, ctx.ld, ctx.start, ctx.forward_id = traj, policy, ld, start, traj._learner_forwards
            return act

        @staticmethod
        def backward(ctx, grad_act):
            if getattr(ctx.traj, "_learner_forwards", 0) != ctx.forward_id:
                raise RuntimeError(f'trajectory_actions: this backward belongs to an earlier forward (start="{ctx.start}") '
                                   "than the trajectory's latest, whose saved state has replaced it; run the backward right "
                                   "after its forward")
            g = grad_act.contiguous()
            if g.dtype != torch.float32:
                g = g.float()
            grad_w = torch.empty(_lib.POLICY_NUM_WEIGHTS, dtype=torch.float32, device=g.device)
            torch.cuda.current_stream(g.device).synchronize()
            _lib.call("rq_trajectory_policy_backward", ctx.traj._require("trajectory"), ctx.policy._handle(), _device_ptr(g),
                      ctx.ld, _device_ptr(grad_w), None, 1)
            return grad_w, None, None, None

except ImportError:        # the engine itself does not need torch; only this module's autograd function does
    _TrajectoryActions = None
