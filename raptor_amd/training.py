"""The learner half of distillation (README.md:208-216): the student's actions over a recorded trajectory as a differentiable
torch function, so that collect -> relabel -> loss -> gradient -> update stays on the device.

    from raptor_amd.training import masked_mse, trajectory_actions
    w = torch.tensor(policy.weights, device="cuda", requires_grad=True)
    act = trajectory_actions(traj, policy, w)              # [T, 4, ld], the layout of traj.tensors()["act"]
    loss = masked_mse(act, target, live)                  # live: [T, 4, ld] bool: done != 4 on the envs' columns, False on padding
    loss.backward()                                         # w.grad: dL/dtheta, 2 084 floats in the checkpoint order

The forward is one HIP launch, the backward two (rq_trajectory_policy_forward / _backward, csrc/rq_grad.hpp); the optimiser is
torch's.  Only the fp32 policy without Standardize / SampleAndSquash stages has a gradient here.

For the distillation loss itself - the masked MSE against the labels - the whole update stays on the device, torch not needed:

    distiller = Distiller(policy, lr=1e-3)
    losses = distiller.step(traj, updates=10)               # 10 x (forward, loss-seeded backward, Adam, repack), one enqueue
    loss, grad = distiller.loss_and_grad(traj)              # the same loss and its gradient, no update

Entries can be weighted, per env or per env and step, without leaving that path (rq_trajectory_*_weighted):

    train, held_out = holdout_weights(N, 0.1, seed=0)       # two 0/1 masks over the envs
    distiller.step(traj, weight=train, updates=10)          # trains on nine tenths of the recording
    val, _ = distiller.loss_and_grad(traj, weight=held_out) # the loss on the rest: a validation loss, no second recording

``weighted_mse`` is the same loss in torch, for the first way; any loss beyond that goes the first way too.

How well the student imitates - per env and per bucket of episode age - is one forward pass, no backward (rq_trajectory_policy_error_table):

    table = imitation_error(traj, policy, edges=probing.log_age_edges(500, 10), target=labels)   # sse, count [B, N]
    table.by_age()                                          # the in-context adaptation curve, [B]
    table.by_group(teacher_of, n_teachers)                  # which teachers the student imitates badly, [G, B]
    table.loss()                                            # the masked MSE: a held-out loss without a backward

A sweep or a seed population is distilled in one go: ``BankDistiller`` runs that update for every policy of a
``policy_bank.PolicyBank`` at once, each on the 64-env blocks of the recording that ``policy_ids`` deals it, with its own
hyper-parameters - one student's launch count for the whole bank, and the bank flies its next rollout with the updated weights:

    bank = PolicyBank(device, W)                              # [P, 2084]
    sweep = BankDistiller(bank, lr=np.geomspace(1e-4, 1e-2, P))
    losses = sweep.step(traj, ids, target=labels, updates=10) # [10, P]
    table = bank.evaluate(vector, device, env, params, state, rng, 500, ids)
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


def weighted_mse(act, target, live, weight):
    """``masked_mse`` with a weight on every entry: sum(w (act - target)^2) / sum(w) over the entries that COUNT - ``live`` and
    ``weight > 0`` - the loss of ``Distiller.step(..., weight=...)`` stated in torch.  ``weight`` broadcasts against ``act``
    (``w[None, None, :]`` for one weight per env of a [T, 4, N] tensor, ``w[:, None, :]`` for one per step and env).

    As in ``masked_mse`` the selection is applied to the INPUTS: where an entry does not count - a frozen step, a weight that is 0,
    negative or NaN - act, target and weight are replaced by 0 before any arithmetic, so NaN there goes nowhere, in the loss or in
    its gradient.  Nothing counts: 0, with a zero gradient."""
    import torch
    zero = torch.zeros((), dtype=act.dtype, device=act.device)
    w = torch.broadcast_to(weight.to(act.dtype), act.shape)
    counts = live & (w > 0)
    a = torch.where(counts, act, zero)
    t = torch.where(counts, target, zero)
    w = torch.where(counts, w, zero)
    total = w.sum()
    return (w * (a - t) ** 2).sum() / torch.where(total > 0, total, torch.ones_like(total))


def holdout_weights(n_envs, fraction, seed):
    """-> (train, held_out): two complementary float32 [n_envs] arrays of 0 and 1 for ``weight=``; exactly
    ``round(fraction * n_envs)`` envs, drawn without replacement, are held out.  A pure function of its arguments
    (``numpy.random.default_rng(seed)``'s permutation): the same split every epoch and every run."""
    n_envs = int(n_envs)
    if n_envs < 0 or not 0.0 <= fraction <= 1.0:
        raise ValueError("n_envs must be non-negative and fraction in [0, 1]")
    held = np.zeros(n_envs, np.float32)
    held[np.random.default_rng(seed).permutation(n_envs)[:int(round(fraction * n_envs))]] = 1.0
    return (1.0 - held).astype(np.float32), held


def _loss_weight(traj, weight):
    """The refusals Python makes itself for ``weight=``, before the library does anything for the call -> (w, ld_weight,
    weight_steps): ``w`` a contiguous float32 NumPy array or device tensor, [weight_steps, ld_weight]."""
    what = "weight must be float32, [>= N] (one per env) or [1 or T, >= N] (one per step and env)"
    tensor = hasattr(weight, "data_ptr")
    if tensor:
        import torch
        if weight.dtype != torch.float32 or weight.dim() not in (1, 2):
            raise ValueError(f"{what}, not {weight.dtype} {tuple(weight.shape)}")
        if not weight.is_cuda:
            raise ValueError("a tensor weight must live on the trajectory's device (a host weight is passed as a NumPy array)")
        w = weight.contiguous()
    else:
        w = np.asarray(weight)
        if w.dtype != np.float32 or w.ndim not in (1, 2):
            raise ValueError(f"{what}, not {w.dtype} {w.shape}")
        w = np.ascontiguousarray(w)
    w = w.reshape(1, -1) if len(w.shape) == 1 else w
    N = int(traj._env.N_ENVIRONMENTS)
    if w.shape[1] < N:
        raise ValueError(f"{what}: {w.shape[1]} columns for {N} envs")
    if not tensor:
        cols = w[:, :N]
        if not np.isfinite(cols).all() or (cols < 0).any():
            s, i = np.argwhere(~(np.isfinite(cols) & (cols >= 0)))[0]
            raise ValueError(f"weight must be finite and non-negative: step {s}, env {i} holds {cols[s, i]}")
    if w.shape[0] != 1 and w.shape[0] != len(traj):
        raise ValueError(f"{what}: {w.shape[0]} rows for a trajectory of {len(traj)} steps")
    return w, int(w.shape[1]), int(w.shape[0])


def _weight_pointer(w, dev):
    """a checked weight where the call wants it - device memory of ``dev``, or the host for ``dev`` None -> (pointer, keep-alive)"""
    tensor = hasattr(w, "data_ptr")
    if dev is None:
        w = w.cpu().numpy() if tensor else w
        return C.c_void_p(w.ctypes.data), w
    if not tensor:
        import torch
        w = torch.from_numpy(w).to(dev)            # a hold-out mask need not be a tensor: uploaded here
    return _device_ptr(w), w


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


class Distiller:
    """Adam on the masked mean squared error between ``policy``'s actions over a recording and a target, entirely on the device
    (rq_trajectory_distill: forward, loss-seeded backward, reduction, Adam and the rebuilt operand images are enqueued back to
    back; no action or gradient tensor the size of the recording exists, and the weights do not visit the host).

    The loss is ``masked_mse(trajectory_actions(traj, policy, w)[:, :, :N], target[:, :, :N], live)`` with ``live`` = done code
    != 4: a loss other than this (weighted) masked MSE still goes through ``trajectory_actions`` and torch.  The update is
    ``torch.optim.Adam``'s with these hyper-parameters (``weight_decay`` decoupled as in ``AdamW``; 0 = none).  ``policy`` must be
    the fp32 policy without Standardize / SampleAndSquash stages; its weights are updated in place - the next rollout, relabel or
    ``evaluate_step`` runs the updated policy, ``policy.weights`` fetches them when first read.

    ``target``: None - the trajectory's own stored actions (what ``relabel_teachers(..., overwrite=True)`` or a teacher-acting
    rollout left there) - or a [T, 4, ld_target] float32 array with ld_target >= N: a torch tensor on the trajectory's device, or
    (``loss_and_grad`` only needs it) a NumPy array.  ``start`` as in ``trajectory_actions``.

    ``weight``: None - every live entry counts the same, the calls above - or float32 weights, [>= N] (one per env) or [1 or T,
    >= N] (one per step and env), NumPy or a tensor on the trajectory's device: the loss becomes ``weighted_mse`` - sum(w (a - y)^2)
    / sum(w) over the live entries with w > 0; a weight of 0 drops its entries, NaN in their targets included
    (rq_trajectory_distill_weighted).  A NumPy weight must be finite and non-negative; beside a device target it is uploaded."""

    def __init__(self, policy, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.policy = policy
        self._cfg = _lib.AdamConfig(float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay))
        self._h = None
        self._fin = None
        self._target_in_flight = None      # the target an enqueued-only step may still be reading (a contiguous copy, perhaps)
        self._weight_in_flight = None      # and the weight (an uploaded copy, perhaps)

    def _handle(self, traj=None):
        pol = self.policy._handle(None if traj is None else traj._env._device)
        if self._h is None:
            import weakref
            h = C.c_void_p()
            _lib.call("rq_optimizer_create", pol, C.byref(self._cfg), C.byref(h))
            self._h = h
            self._fin = weakref.finalize(self, _lib.load().rq_optimizer_destroy, h)
        return pol, self._h

    def set_lr(self, lr):
        """A new learning rate for the updates enqueued from now on (schedules)."""
        self._cfg.lr = float(lr)
        if self._h is not None:
            _lib.call("rq_optimizer_set_lr", self._h, float(lr))

    def state(self):
        """Adam's state behind everything enqueued (rq_optimizer_get_state) -> a dict of NumPy arrays: ``m``, ``v`` [2084] float32,
        ``step`` (uint32 scalar, the updates made) and ``beta_powers`` [2] float64 - (beta1^step, beta2^step) as the device carries
        them.  Together with ``policy.weights`` that is a checkpoint of the run; the hyper-parameters are the constructor's."""
        _, opt = self._handle()
        m, v = np.empty(_lib.POLICY_NUM_WEIGHTS, np.float32), np.empty(_lib.POLICY_NUM_WEIGHTS, np.float32)
        step, powers = np.zeros(1, np.uint32), np.empty(2, np.float64)
        _lib.call("rq_optimizer_get_state", opt, _lib.fptr(m), _lib.fptr(v), step.ctypes.data, powers.ctypes.data)
        return {"m": m, "v": v, "step": step[0], "beta_powers": powers}

    def set_state(self, m, v, step, beta_powers):
        """The reverse (rq_optimizer_set_state): ``Distiller(policy, same hyper-parameters).set_state(**other.state())`` on a policy
        holding ``other``'s weights continues ``other``'s run bit for bit."""
        m, v, powers = _state_arrays(m, v, beta_powers, (_lib.POLICY_NUM_WEIGHTS,), (2,))
        _, opt = self._handle()
        _lib.call("rq_optimizer_set_state", opt, _lib.fptr(m), _lib.fptr(v), int(step), powers.ctypes.data)

    def apply(self, grad, wait=True):
        """One Adam update of the policy from ``grad`` [2084] float32 in the checkpoint order (rq_optimizer_apply): a NumPy array, or
        a tensor on the policy's device (``wait=False``: enqueued only).  ``loss_and_grad`` followed by ``apply`` of its gradient is
        one ``step``; a gradient from torch (``trajectory_actions`` and any loss) takes the same update without leaving the device."""
        if hasattr(grad, "data_ptr"):
            import torch
            g = grad.detach().contiguous()
            if g.dtype != torch.float32 or tuple(g.shape) != (_lib.POLICY_NUM_WEIGHTS,) or not g.is_cuda:
                raise ValueError(f"grad must be a float32 device tensor of {_lib.POLICY_NUM_WEIGHTS} values (or a NumPy array)")
            _, opt = self._handle()
            torch.cuda.current_stream(g.device).synchronize()     # the engine runs on its own stream
            _lib.call("rq_optimizer_apply", opt, _device_ptr(g), 1 if wait else 2)
            self._target_in_flight = g                            # an enqueued-only update may still be reading it
        else:
            g = np.ascontiguousarray(grad, np.float32)
            if g.shape != (_lib.POLICY_NUM_WEIGHTS,):
                raise ValueError(f"grad must hold {_lib.POLICY_NUM_WEIGHTS} values")
            _, opt = self._handle()
            _lib.call("rq_optimizer_apply", opt, _lib.fptr(g), 0)
        self.policy._weights_on_device = True

    @staticmethod
    def _target(traj, target):
        """-> (pointer or None, ld_target, on_device, keep-alive)"""
        if target is None:
            return None, 0, None, None
        T = len(traj)
        if hasattr(target, "data_ptr"):
            import torch
            t = target
            if t.dim() != 3 or t.shape[0] != T or t.shape[1] != _lib.POLICY_OUTPUT_DIM or t.dtype != torch.float32 or not t.is_cuda:
                raise ValueError(f"target must be a float32 device tensor [{T}, 4, >= N]")
            t = t.contiguous()
            return _device_ptr(t), t.shape[2], True, t
        t = np.ascontiguousarray(target, np.float32)
        if t.ndim != 3 or t.shape[0] != T or t.shape[1] != _lib.POLICY_OUTPUT_DIM:
            raise ValueError(f"target must be [{T}, 4, >= N]")
        return C.c_void_p(t.ctypes.data), t.shape[2], False, t

    @staticmethod
    def _torch_device(traj):
        try:
            import torch  # noqa: F401
        except ImportError:
            return None
        return traj.tensors()["act"].device

    def loss_and_grad(self, traj, target=None, start="initial", weight=None):
        """-> (loss, dloss/dweights [2084]): device tensors when torch is present, NumPy otherwise (or with a NumPy target)."""
        if start not in START:
            raise ValueError('start must be "initial" or "current"')
        suffix, pol, args, dev, _ = _loss_call(traj, target, weight, start, lambda: self.policy._handle(traj._env._device), False)
        name = "rq_trajectory_policy_loss_grad" + suffix
        if dev is None:
            loss, grad = np.empty(1, np.float32), np.empty(_lib.POLICY_NUM_WEIGHTS, np.float32)
            _lib.call(name, traj._require("trajectory"), pol, *args, _lib.fptr(loss), _lib.fptr(grad), 0)
            return loss[0], grad
        import torch
        loss = torch.empty((), dtype=torch.float32, device=dev)
        grad = torch.empty(_lib.POLICY_NUM_WEIGHTS, dtype=torch.float32, device=dev)
        torch.cuda.current_stream(dev).synchronize()          # the engine runs on its own stream
        _lib.call(name, traj._require("trajectory"), pol, *args, _device_ptr(loss), _device_ptr(grad), 1)
        return loss, grad

    def step(self, traj, target=None, start="initial", updates=1, wait=True, weight=None):
        """``updates`` Adam steps on the recording, enqueued in one call -> the loss before each of them, [updates] (a device
        tensor when torch is present, NumPy otherwise).  ``wait=False`` (torch only) returns once the work is enqueued on the
        engine's stream: what the engine is asked to do next is ordered behind it; read the losses after ``device.synchronize()``."""
        if start not in START:
            raise ValueError('start must be "initial" or "current"')
        updates = int(updates)
        if updates < 1:
            raise ValueError("updates must be at least 1")
        suffix, (pol, opt), args, dev, keep = _loss_call(traj, target, weight, start, lambda: self._handle(traj), True)
        name = "rq_trajectory_distill" + suffix
        if dev is None:
            losses = np.empty(updates, np.float32)
            _lib.call(name, traj._require("trajectory"), pol, opt, *args, updates, _lib.fptr(losses), 0)
        else:
            import torch
            losses = torch.empty(updates, dtype=torch.float32, device=dev)
            torch.cuda.current_stream(dev).synchronize()      # once per call, not per update
            _lib.call(name, traj._require("trajectory"), pol, opt, *args, updates, _device_ptr(losses), 1 if wait else 2)
        # until the next step: with wait=False the engine's stream may not have read the target or the weight yet
        self._target_in_flight, self._weight_in_flight = keep
        self.policy._weights_on_device = True
        return losses


def _state_arrays(m, v, beta_powers, shape, powers_shape):
    """the refusals Python makes itself for an optimizer state -> contiguous (m, v float32 ``shape``, powers float64)"""
    m, v = np.ascontiguousarray(m), np.ascontiguousarray(v)
    if m.dtype != np.float32 or v.dtype != np.float32 or m.shape != shape or v.shape != shape:
        raise ValueError(f"m and v must be float32 {list(shape)} (their bits are copied)")
    powers = np.ascontiguousarray(beta_powers, np.float64)
    if powers.shape != powers_shape:
        raise ValueError(f"beta_powers must be {list(powers_shape)}")
    return m, v, powers


def _loss_call(traj, target, weight, start, handles, host_ok):
    """What the four loss calls prepare alike, in the order they always did.  First the refusals Python makes itself for ``weight``
    and ``target``; then ``handles()``, the caller's library handles - an optimizer is created there, so a call Python refuses
    leaves the library untouched; then the device, the trajectory's ``_learner_forwards`` (its saved state is this call's now) and
    the weight where the call wants it.  ``host_ok``: whether a device target may go on without torch (else it is refused).
    -> (suffix of the entry point, what ``handles()`` gave, the arguments from ``target`` to ``start`` - the weight's three among
    them with the suffix "_weighted" -, the torch device or None for the NumPy path, (target, weight) to keep alive)"""
    w = None if weight is None else _loss_weight(traj, weight)
    ptr, ld_t, on_device, keep = Distiller._target(traj, target)
    h = handles()
    dev = Distiller._torch_device(traj) if on_device is not False else None
    traj._learner_forwards = getattr(traj, "_learner_forwards", 0) + 1
    suffix, wargs, wkeep = "", (), None
    if w is not None:
        wptr, wkeep = _weight_pointer(w[0], dev)
        suffix, wargs = "_weighted", (wptr, w[1], w[2])
    if dev is None and on_device and not host_ok:
        raise ValueError("a device target needs torch")
    return suffix, h, (ptr, ld_t, *wargs, START[start]), dev, (keep, wkeep)


MAX_BUCKETS = 32              # rq::kErrorTableMaxBuckets, the probes' limit


class ErrorTable:
    """What ``imitation_error`` returns: ``sse`` [B, N] float32 - per age bucket and env the sum over its live steps of the squared
    imitation error (a - y)^2 summed over the four actions -, ``count`` [B, N] - the number of those steps - and ``edges`` [B + 1]
    (uint32, NumPy).  The arrays are NumPy or torch tensors, as the call made them; every method below works in float64 on whatever
    they are and returns the same kind.  A mean over nothing is NaN."""

    def __init__(self, sse, count, edges):
        self.sse, self.count = sse, count
        self.edges = np.asarray(edges, np.uint32)
        if len(sse.shape) != 2 or tuple(sse.shape) != tuple(count.shape) or self.edges.shape != (sse.shape[0] + 1,):
            raise ValueError("sse and count must be [B, N] and edges [B + 1]")

    def _f64(self):
        if hasattr(self.sse, "data_ptr"):
            import torch
            return self.sse.to(torch.float64), self.count.to(torch.float64)
        return np.asarray(self.sse, np.float64), np.asarray(self.count, np.float64)

    @staticmethod
    def _mean(s, c):
        """s / (4 c) where c > 0, NaN elsewhere"""
        if hasattr(s, "data_ptr"):
            import torch
            return torch.where(c > 0, s / (4.0 * torch.clamp(c, min=1.0)), torch.full_like(s, float("nan")))
        return np.where(c > 0, s / (4.0 * np.maximum(c, 1.0)), np.nan)

    def mse(self):
        """-> [B, N]: the mean squared error per action of env i at the ages of bucket b"""
        return self._mean(*self._f64())

    def per_env(self):
        """-> [N]: every env's error over all buckets - with ``edges=None`` its error over the whole recording"""
        s, c = self._f64()
        return self._mean(s.sum(0), c.sum(0))

    def by_age(self):
        """-> [B]: the error of all envs by age bucket, the in-context adaptation curve"""
        s, c = self._f64()
        return self._mean(s.sum(1), c.sum(1))

    def by_group(self, ids, n_groups):
        """``ids`` [N] integers below ``n_groups`` - the teacher, reference, wrench scenario or policy of every env -> [G, B]: the
        error of each group's envs by age bucket."""
        s, c = self._f64()
        G, N = int(n_groups), int(s.shape[1])
        g = np.asarray(ids.cpu() if hasattr(ids, "data_ptr") else ids)
        if g.shape != (N,) or not np.issubdtype(g.dtype, np.integer) or (N and (g.min() < 0 or g.max() >= G)):
            raise ValueError(f"ids must be [{N}] integers below {G}")
        if hasattr(s, "data_ptr"):
            import torch
            at = torch.as_tensor(g.astype(np.int64), device=s.device)
            zero = torch.zeros((G, s.shape[0]), dtype=torch.float64, device=s.device)
            return self._mean(zero.index_add(0, at, s.T), zero.index_add(0, at, c.T))
        gs, gc = np.zeros((G, s.shape[0])), np.zeros((G, s.shape[0]))
        np.add.at(gs, g, s.T)
        np.add.at(gc, g, c.T)
        return self._mean(gs, gc)

    def loss(self):
        """-> the masked MSE over everything the table counts: sum(sse) / (4 sum(count)).  With ``edges=None`` that is the loss of
        ``Distiller.loss_and_grad`` on the same recording and target, summed in another order."""
        s, c = self._f64()
        return self._mean(s.sum(), c.sum())


def _age_edges(edges):
    """The refusals Python makes itself for ``edges=`` -> uint32 [B + 1]; None: one bucket for every age."""
    if edges is None:
        return np.asarray([0, 2 ** 32 - 1], np.uint32)
    e = np.asarray(edges)
    if e.ndim != 1 or not 2 <= e.size <= MAX_BUCKETS + 1 or not (np.issubdtype(e.dtype, np.integer) or np.all(e == np.floor(e))):
        raise ValueError(f"edges must be 2 .. {MAX_BUCKETS + 1} strictly ascending uint32 values")
    e = e.astype(np.int64) if not np.issubdtype(e.dtype, np.unsignedinteger) else e.astype(np.uint64)
    if (e[1:] <= e[:-1]).any() or e[0] < 0 or e[-1] >= 1 << 32:
        raise ValueError(f"edges must be 2 .. {MAX_BUCKETS + 1} strictly ascending uint32 values")
    return np.ascontiguousarray(e.astype(np.uint32))


def imitation_error(traj, policy, edges=None, target=None, start="initial", policy_ids=None):
    """How well ``policy`` imitates ``target`` on the recording, per env and bucket of episode age -> ``ErrorTable``.  One forward
    pass on the device (rq_trajectory_policy_error_table): no backward, no action tensor, no pass over the done codes on the host.

    ``policy``: a ``Raptor`` (fp32, no Standardize / SampleAndSquash stage, native rate), or a ``PolicyBank`` together with
    ``policy_ids`` - one id per env, constant on every aligned block of 64 -, each env scored under its own policy.  ``edges``:
    [B + 1] strictly ascending episode ages, B <= 32 (``probing.log_age_edges``); a live step of age k falls in bucket b when
    ``edges[b] <= k < edges[b + 1]`` and is counted nowhere outside them; None: one bucket for every age, the per-env error.  Age is
    the probes': 0 at the first recorded step and after an episode end, one more after every other live step; frozen steps neither
    count nor age.  ``target`` and ``start`` as for ``Distiller``.

    The table's arrays are device tensors when torch is present and the target is not NumPy, NumPy otherwise; the call orders itself
    against torch's current stream as ``Distiller.loss_and_grad`` does.  The trajectory's saved state is not touched: a pending
    ``trajectory_actions`` backward stays valid."""
    if start not in START:
        raise ValueError('start must be "initial" or "current"')
    e = _age_edges(edges)
    N = int(traj._env.N_ENVIRONMENTS)
    bank = hasattr(policy, "n_policies")
    if bank and policy_ids is None:
        raise ValueError("a PolicyBank needs policy_ids: one id per env, constant on every aligned block of 64")
    if not bank and policy_ids is not None:
        raise ValueError("policy_ids belong to a PolicyBank")
    ids = None
    if bank:
        from .policy_bank import check_policy_ids
        ids = check_policy_ids(policy_ids, policy.n_policies, N)
    ptr, ld_t, on_device, keep = Distiller._target(traj, target)
    if target is not None and ld_t < N:
        raise ValueError(f"target must be [{len(traj)}, 4, >= N]: {ld_t} columns for {N} envs")
    head = (policy._h, ids.ctypes.data) if bank else (policy._handle(traj._env._device),)
    name = "rq_trajectory_policies_error_table" if bank else "rq_trajectory_policy_error_table"
    dev = Distiller._torch_device(traj) if on_device is not False else None
    if dev is None and on_device:
        raise ValueError("a device target needs torch")
    B = e.size - 1
    if dev is None:
        sse, count = np.empty((B, N), np.float32), np.empty((B, N), np.uint32)
        _lib.call(name, traj._require("trajectory"), *head, ptr, ld_t, e.ctypes.data, B, START[start], _lib.fptr(sse), count.ctypes.data, N, 0)
        return ErrorTable(sse, count, e)
    import torch
    sse = torch.empty((B, N), dtype=torch.float32, device=dev)
    count = torch.empty((B, N), dtype=torch.int32, device=dev)          # the engine's uint32; a recording has fewer than 2^31 steps
    torch.cuda.current_stream(dev).synchronize()          # the engine runs on its own stream
    _lib.call(name, traj._require("trajectory"), *head, ptr, ld_t, e.ctypes.data, B, START[start], _device_ptr(sse), _device_ptr(count), N, 1)
    del keep
    return ErrorTable(sse, count, e)


def _per_policy(name, value, n_policies):
    """a hyper-parameter given as a scalar or as one value per policy -> float64 [n_policies]"""
    a = np.asarray(value, np.float64)
    if a.ndim == 0:
        return np.full(n_policies, float(a))
    if a.ndim != 1 or a.size not in (1, n_policies):
        raise ValueError(f"{name} must be a scalar or hold one value per policy ({n_policies}), not {a.shape}")
    return np.full(n_policies, a[0]) if a.size == 1 else np.ascontiguousarray(a)


class BankDistiller:
    """``Distiller`` for every policy of a ``PolicyBank`` at once (rq_trajectory_policies_distill): policy p is updated on the
    64-env blocks of the recording that ``policy_ids`` names it for - its loss is the masked MSE over those envs alone - with
    its own Adam state and hyper-parameters.  ``lr``, ``betas[0]``, ``betas[1]``, ``eps`` and ``weight_decay`` are each a scalar or
    a length-P sequence: that is the sweep.  What policy p gets is, bit for bit, what a ``Distiller`` of its own gets on a
    recording of its blocks; the cost is one student's launches.  The bank's weights are updated in place on the device: its next
    rollout flies them, ``bank.weights`` fetches them when first read.  A policy that owns no block is left alone (loss NaN).

    ``policy_ids``: one id per env of the trajectory, constant on every aligned block of 64 (``check_policy_ids``).  ``target``,
    ``start`` and ``weight`` as for ``Distiller``; ``start="current"`` reads the bank's hidden state.  With a ``weight`` policy p's
    loss is normalised by the weights of ITS blocks; a policy none of whose entries counts gets loss 0 and a zero gradient."""

    def __init__(self, bank, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        P = int(bank.n_policies)
        if len(betas) != 2:
            raise ValueError("betas must be a pair")
        cols = [_per_policy("lr", lr, P), _per_policy("betas[0]", betas[0], P), _per_policy("betas[1]", betas[1], P),
                _per_policy("eps", eps, P), _per_policy("weight_decay", weight_decay, P)]
        self.bank = bank
        self._cfg = (_lib.AdamConfig * P)(*[_lib.AdamConfig(*(float(c[p]) for c in cols)) for p in range(P)])
        self._h = None
        self._fin = None
        self._target_in_flight = None
        self._weight_in_flight = None

    def _handle(self):
        if self._h is None:
            import weakref
            h = C.c_void_p()
            _lib.call("rq_bank_optimizer_create", self.bank._h, self._cfg, len(self._cfg), C.byref(h))
            self._h = h
            self._fin = weakref.finalize(self, _lib.load().rq_bank_optimizer_destroy, h)
        return self._h

    def set_lr(self, lr):
        """New learning rates (a scalar or one per policy) for the updates enqueued from now on."""
        rates = _per_policy("lr", lr, len(self._cfg))
        for c, r in zip(self._cfg, rates):
            c.lr = float(r)
        if self._h is not None:
            _lib.call("rq_bank_optimizer_set_lr", self._h, rates.ctypes.data, rates.size)

    def state(self):
        """Every policy's Adam state behind everything enqueued (rq_bank_optimizer_get_state) -> a dict of NumPy arrays: ``m``,
        ``v`` [P, 2084] float32, ``step`` [P] uint32, ``beta_powers`` [P, 2] float64.  As ``Distiller.state``."""
        P, opt = int(self.bank.n_policies), self._handle()
        m, v = np.empty((P, _lib.POLICY_NUM_WEIGHTS), np.float32), np.empty((P, _lib.POLICY_NUM_WEIGHTS), np.float32)
        step, powers = np.zeros(P, np.uint32), np.empty((P, 2), np.float64)
        _lib.call("rq_bank_optimizer_get_state", opt, _lib.fptr(m), _lib.fptr(v), step.ctypes.data, powers.ctypes.data)
        return {"m": m, "v": v, "step": step, "beta_powers": powers}

    def set_state(self, m, v, step, beta_powers):
        """The reverse (rq_bank_optimizer_set_state); a restored bank run continues bit for bit."""
        P = int(self.bank.n_policies)
        m, v, powers = _state_arrays(m, v, beta_powers, (P, _lib.POLICY_NUM_WEIGHTS), (P, 2))
        step = np.ascontiguousarray(step, np.uint32)
        if step.shape != (P,):
            raise ValueError(f"step must hold one count per policy ({P})")
        _lib.call("rq_bank_optimizer_set_state", self._handle(), _lib.fptr(m), _lib.fptr(v), step.ctypes.data, powers.ctypes.data)

    def _check(self, traj, policy_ids, start, updates=1):
        """the refusals Python makes itself, before any library call -> (ids, updates)"""
        from .policy_bank import check_policy_ids
        if start not in START:
            raise ValueError('start must be "initial" or "current"')
        updates = int(updates)
        if updates < 1:
            raise ValueError("updates must be at least 1")
        return check_policy_ids(policy_ids, self.bank.n_policies, traj._env.N_ENVIRONMENTS), updates

    def loss_and_grad(self, traj, policy_ids, target=None, start="initial", weight=None):
        """-> (loss [P], dloss/dweights [P, 2084]), every policy's over its own blocks; no update.  Device tensors when torch is
        present, NumPy otherwise (or with a NumPy target).  A policy that owns no block: loss NaN, its gradient row zero."""
        ids, _ = self._check(traj, policy_ids, start)
        P = int(self.bank.n_policies)
        suffix, _, args, dev, _ = _loss_call(traj, target, weight, start, lambda: None, False)
        name = "rq_trajectory_policies_loss_grad" + suffix
        if dev is None:
            loss, grad = np.empty(P, np.float32), np.zeros((P, _lib.POLICY_NUM_WEIGHTS), np.float32)
            _lib.call(name, traj._require("trajectory"), self.bank._h, ids.ctypes.data, *args, _lib.fptr(loss), _lib.fptr(grad), 0)
            return loss, grad
        import torch
        loss = torch.empty(P, dtype=torch.float32, device=dev)
        grad = torch.zeros((P, _lib.POLICY_NUM_WEIGHTS), dtype=torch.float32, device=dev)
        torch.cuda.current_stream(dev).synchronize()          # the engine runs on its own stream
        _lib.call(name, traj._require("trajectory"), self.bank._h, ids.ctypes.data, *args, _device_ptr(loss), _device_ptr(grad), 1)
        return loss, grad

    def step(self, traj, policy_ids, target=None, start="initial", updates=1, wait=True, weight=None):
        """``updates`` Adam steps of every policy on its blocks of the recording, enqueued in one call -> the losses before each
        of them, [updates, P] (a device tensor when torch is present, NumPy otherwise).  ``wait=False`` (torch only) returns once
        the work is enqueued on the engine's stream: a rollout of the bank asked for next flies the updated weights."""
        ids, updates = self._check(traj, policy_ids, start, updates)
        P = int(self.bank.n_policies)
        suffix, opt, args, dev, keep = _loss_call(traj, target, weight, start, self._handle, True)
        name = "rq_trajectory_policies_distill" + suffix
        if dev is None:
            losses = np.empty((updates, P), np.float32)
            _lib.call(name, traj._require("trajectory"), self.bank._h, opt, ids.ctypes.data, *args, updates, _lib.fptr(losses), 0)
        else:
            import torch
            losses = torch.empty((updates, P), dtype=torch.float32, device=dev)
            torch.cuda.current_stream(dev).synchronize()      # once per call, not per update
            _lib.call(name, traj._require("trajectory"), self.bank._h, opt, ids.ctypes.data, *args, updates, _device_ptr(losses),
                      1 if wait else 2)
        # until the next step: with wait=False the engine's stream may not have read the target or the weight yet
        self._target_in_flight, self._weight_in_flight = keep
        self.bank._weights_on_device = True
        return losses
