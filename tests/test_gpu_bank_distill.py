"""Distilling a policy bank on the GPU (rq_trajectory_policies_loss_grad, rq_bank_optimizer_*, rq_trajectory_policies_distill,
rq_policy_bank_get_weights; csrc/rq_grad_bank.hpp; raptor_amd.training.BankDistiller).

The reference for everything is the project's own single-policy path: what policy p of a bank gets on the blocks dealt to it is,
as bits, what `Raptor(weights=W[p])` gets from rq_trajectory_policy_loss_grad / rq_trajectory_distill on a recording that holds
p's columns alone, in order.  Beside that: the float64 bounds of tests/test_gpu_distill.py per policy (the per-wave arithmetic is
that of the single policy, so the bound is too), per-policy hyper-parameters, a policy without a block, the device-side repack
against a bank packed on the host, ordering against a rollout, and the refusals.

Slack of the accuracy case: ``pytest tests/test_gpu_bank_distill.py -m gpu -v -s``."""
import ctypes as C

import numpy as np
import pytest

import distill_reference as D
import policy_grad_reference as R
from distill_common import (DEVICE, HOST, INITIAL, Opt, _adam, _ld, _lib, _perturbed, _record, _targets, distill, forward, get_weights,
                            loss_grad, opt_state, same)
from gpu_common import World
from rollout_common import ids_of

pytestmark = pytest.mark.gpu

NW = 2084
# Roundings the loss seed adds on a path from dL/da to a gradient element beyond policy_grad_reference.K_paths (as defined in
# tests/test_gpu_distill.py, restated): the fp32 subtract a - y in the seeded backward and the one rounding to fp32 of acc * (2 / M)
# in the reduction, whose float64 product adds three roundings of 2^-53, together below 2^-27 of one fp32 rounding.
C_SEED = 2 + 2.0 ** -27

# the shared case: five blocks, the last ragged with 44 envs; non-monotone ids, and the ragged block shares policy 0 with a full one
N, T, P = 300, 20, 3
BLOCK_IDS = [2, 0, 2, 1, 0]
CFG = [dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.0), dict(lr=1e-3, betas=(0.8, 0.99), eps=1e-7, wd=0.01),
       dict(lr=5e-4, betas=(0.95, 0.9995), eps=1e-8, wd=0.0)]


# ---- the bank's calls ----
def bank_loss_grad(traj, bank, ids, target, start=INITIAL, ld=None, memory=HOST, fill=np.nan):
    L = _lib()
    loss, g = np.full(bank.n_policies, fill, np.float32), np.full((bank.n_policies, NW), fill, np.float32)
    t = None if target is None else np.ascontiguousarray(target, np.float32)
    ids = np.ascontiguousarray(ids, np.uint32)
    L.call("rq_trajectory_policies_loss_grad", traj._require("trajectory"), bank._h, ids.ctypes.data, None if t is None else L.fptr(t),
           0 if t is None else (ld or t.shape[2]), start, L.fptr(loss), L.fptr(g), memory)
    return loss, g


class BankOpt:
    def __init__(self, bank, cfgs):
        cfgs = cfgs if isinstance(cfgs, (list, tuple)) else [cfgs]
        self.cfg, self.h = (_lib().AdamConfig * len(cfgs))(*[_adam(c) for c in cfgs]), C.c_void_p()
        _lib().call("rq_bank_optimizer_create", bank._h, self.cfg, len(cfgs), C.byref(self.h))

    def close(self):
        _lib().call("rq_bank_optimizer_destroy", self.h)


def bank_distill(traj, bank, opt, ids, n_updates, target, start=INITIAL, ld=None, memory=HOST):
    L = _lib()
    losses = np.empty((max(n_updates, 1), bank.n_policies), np.float32)
    t = None if target is None else np.ascontiguousarray(target, np.float32)
    ids = np.ascontiguousarray(ids, np.uint32)
    L.call("rq_trajectory_policies_distill", traj._require("trajectory"), bank._h, opt.h, ids.ctypes.data,
           None if t is None else L.fptr(t), 0 if t is None else (ld or t.shape[2]), start, n_updates, L.fptr(losses), memory)
    return losses


def bank_weights(bank):
    L = _lib()
    w = np.empty((bank.n_policies, NW), np.float32)
    L.call("rq_policy_bank_get_weights", bank._h, L.fptr(w))
    return w


def has_ends_and_frozen(done, ids, n_policies):
    """policies in whose envs the recording holds both an episode end (code 1 or 2) and a frozen step (code 4)"""
    return [p for p in range(n_policies) if ((done[:, ids == p] == 1) | (done[:, ids == p] == 2)).any() and (done[:, ids == p] == 4).any()]


class Case:
    """The shared recording (N envs, T steps, every done code), its labels, four perturbed weight vectors, and - computed once
    per set of columns - the recording that holds those columns alone."""

    def __init__(self, device, oracle, weights):
        self.device, self.oracle = device, oracle
        self.world, self.traj = _record(device, oracle, N, T, seed=211, frozen=True)
        self.ids = ids_of(BLOCK_IDS, N)
        self.y = _targets(self.traj, N, seed=9)
        self.W = np.stack([_perturbed(weights, 30 + k) for k in range(4)])
        self.rec = self.traj.numpy()
        assert len(has_ends_and_frozen(self.rec["done"], self.ids, P)) >= 2
        self._subs = {}

    def columns(self, ids, p):
        return np.flatnonzero(np.asarray(ids) == p)

    def sub(self, cols):
        """-> (trajectory of len(cols) envs holding the shared recording's columns `cols` in order, its labels)"""
        import torch
        key = tuple(int(c) for c in cols)
        if key not in self._subs:
            n = len(key)
            w = World(self.device, self.oracle, n, seed=5, episode_step_limit=9)
            traj = w.vector.Trajectory(w.env, T)
            w.vector.rollout(self.device, w.env, w.params, w.state, w.policy, w.rng, T, "fused", autoreset=True, trajectory=traj)   # sizes it
            src, dst = self.traj.tensors(), traj.tensors()
            idx = torch.tensor(np.asarray(key), device=src["obs"].device)
            for k in ("obs", "act"):
                dst[k][:, :, :n] = src[k][:, :, idx]
            dst["done"][:, :n] = src["done"][:, idx]
            torch.cuda.synchronize()
            y = np.full((T, 4, _ld(traj)), np.nan, np.float32)
            y[:, :, :n] = self.y[:, :, np.asarray(key)]
            self._subs[key] = (w, traj, y)
        return self._subs[key][1], self._subs[key][2]


@pytest.fixture(scope="module")
def case(device, oracle, weights):
    return Case(device, oracle, weights)


# ------------------------------------------------------------------------------ 1. a bank of one is the Distiller -
@pytest.mark.parametrize("steps,n", [(5, 1), (37, 200)])
def test_a_bank_of_one_is_the_distiller(device, oracle, weights, steps, n):
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.policy_bank import PolicyBank
    w, traj = _record(device, oracle, n, steps, seed=300 + n, frozen=True)
    ids = np.zeros(n, np.uint32)
    if n > 1:
        assert has_ends_and_frozen(traj.numpy()["done"], ids, 1) == [0]
    y = _targets(traj, n, seed=steps)
    w0 = _perturbed(weights, 21)
    cfg = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.01)
    pol = Raptor(device, weights=w0)
    pol.reset()
    bank = PolicyBank(device, w0[None])
    l_ref, g_ref = loss_grad(traj, pol, y)
    l_bank, g_bank = bank_loss_grad(traj, bank, ids, y)
    assert same(l_bank[0], l_ref) and same(g_bank[0], g_ref) and g_ref.any()
    opt, bopt = Opt(pol, **cfg), BankOpt(bank, cfg)
    ref_losses = distill(traj, pol, opt, 3, y)
    losses = bank_distill(traj, bank, bopt, ids, 3, y)
    assert losses.shape == (3, 1) and same(losses[:, 0], ref_losses)
    assert same(bank_weights(bank)[0], get_weights(pol)) and not same(get_weights(pol), w0)
    opt.close(); bopt.close()


# ------------------------------------------------------------------------------ 2. each policy == a Distiller of its own -
def _single_reference(case, w, cfg, cols, updates):
    """Raptor(weights=w) on the recording of `cols` alone: loss_grad, then `updates` x rq_trajectory_distill(1) -> (loss, grad, losses, weights)"""
    from raptor_amd.foundation_policy import Raptor
    traj, y = case.sub(cols)
    pol = Raptor(case.device, weights=w)
    pol.reset()
    loss, g = loss_grad(traj, pol, y)
    opt = Opt(pol, **cfg)
    losses = np.concatenate([distill(traj, pol, opt, 1, y) for _ in range(updates)])
    out = (loss, g, losses, get_weights(pol))
    opt.close()
    return out


def test_each_policy_gets_what_a_distiller_of_its_own_gets(case):
    from raptor_amd.policy_bank import PolicyBank
    bank = PolicyBank(case.device, case.W[:P])
    L0, G0 = bank_loss_grad(case.traj, bank, case.ids, case.y)
    bopt = BankOpt(bank, CFG)
    losses = bank_distill(case.traj, bank, bopt, case.ids, 2, case.y)
    Wn = bank_weights(bank)
    assert losses.shape == (2, P)
    for p in range(P):
        loss, g, ls, w = _single_reference(case, case.W[p], CFG[p], case.columns(case.ids, p), 2)
        assert same(L0[p], loss) and same(G0[p], g), p
        assert same(losses[:, p], ls), (p, losses[:, p], ls)
        assert same(Wn[p], w), p
        assert not same(w, case.W[p]) and g.any() and ls[0] != ls[1]
    bopt.close()


# ------------------------------------------------------------------------------ 3. float64 bounds per policy -
def test_float64_bounds_per_policy(case):
    import torch
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.policy_bank import PolicyBank
    bank = PolicyBank(case.device, case.W[:P])
    loss, g = bank_loss_grad(case.traj, bank, case.ids, case.y)
    rec = case.rec
    for p in range(P):
        cols = case.columns(case.ids, p)
        n_p, waves_p = len(cols), BLOCK_IDS.count(p)
        pol = Raptor(case.device, weights=case.W[p])
        pol.reset()
        act = forward(case.traj, pol, INITIAL)[:, :, cols]                    # the device's own fp32 actions of p on its envs
        y = case.y[:, :, cols]
        live = np.broadcast_to((rec["done"][:, cols] != 4)[:, None, :], (T, 4, n_p))
        M = int(live.sum())
        ref_loss, seed, terms = D.masked_mse(act, y, live)
        lb = D.loss_bound(terms, M)
        print(f"policy {p}: {n_p} envs, {waves_p} waves, M {M}, loss {loss[p]:.6g}, |loss - ref| / bound {abs(loss[p] - ref_loss) / lb:.3g}")
        assert M > 0 and np.isfinite(loss[p]) and abs(loss[p] - ref_loss) <= lb
        _, cache = R.forward(case.W[p].astype(np.float64), rec["obs"][:, cols], rec["done"][:, cols], "initial")
        dact = seed.transpose(0, 2, 1)
        g_ref, _ = R.backward(cache, dact)
        K = R.K_paths(T, waves_p)
        b = R.bound(cache, dact, waves_p)[0] * (K + C_SEED) / K
        err = np.abs(g[p] - g_ref)
        print(f"policy {p}: max err/bound {np.max(err / b):.3g}, max |g| {np.abs(g_ref).max():.3g}")
        assert np.isfinite(g[p]).all() and (err <= b).all(), (p, np.argmax(err / b), np.max(err / b))
    # padding columns and the observations of frozen steps: NaN there, the same bits
    obs, done = case.traj.tensors()["obs"], case.traj.tensors()["done"]
    keep = obs.clone()
    try:
        assert (done[:, :N] == 4).any() and obs.shape[2] > N
        obs[:, :, N:] = float("nan")
        obs.copy_(torch.where((done == 4)[:, None, :], float("nan"), obs))
        torch.cuda.synchronize()
        loss2, g2 = bank_loss_grad(case.traj, bank, case.ids, case.y)
        assert same(loss2, loss) and same(g2, g)
    finally:
        obs.copy_(keep)
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------ 4. per-policy hyper-parameters -
def test_per_policy_learning_rates(case):
    from raptor_amd.policy_bank import PolicyBank
    from raptor_amd.training import BankDistiller
    lr = [2e-3, 0.0, 5e-4]
    bank = PolicyBank(case.device, case.W[:P])
    sweep = BankDistiller(bank, lr=lr)
    losses = sweep.step(case.traj, case.ids, target=case.y, updates=2)
    assert tuple(losses.shape) == (2, P)
    Wn = bank.weights.copy()
    assert same(Wn[1], case.W[1])
    for p in (0, 2):
        assert np.abs(Wn[p] - case.W[p]).max() > 0.5 * lr[p], p
    sweep.set_lr([0.0, 0.0, 0.0])
    sweep.step(case.traj, case.ids, target=case.y, updates=2)
    assert same(bank.weights, Wn)
    sweep.set_lr(1e-3)                                               # one rate for all: everyone moves again
    sweep.step(case.traj, case.ids, target=case.y, updates=1)
    assert all(not same(bank.weights[p], Wn[p]) for p in range(P))


# ------------------------------------------------------------------------------ 5. a policy that owns no block -
def test_a_policy_without_a_block_is_left_alone(case):
    from raptor_amd.policy_bank import PolicyBank
    cfg = CFG[1]
    bank = PolicyBank(case.device, case.W)                           # P = 4, the ids name 0 .. 2 only
    bopt = BankOpt(bank, cfg)
    state = lambda: opt_state(bopt, slots=4, name="rq_bank_optimizer_get_state")
    loss, g = bank_loss_grad(case.traj, bank, case.ids, case.y, fill=7.0)
    assert np.isnan(loss[3]) and np.isfinite(loss[:3]).all() and (g[3] == 7.0).all()        # its gradient row: not written
    losses = bank_distill(case.traj, bank, bopt, case.ids, 2, case.y)
    Wn = bank_weights(bank)
    assert np.isnan(losses[:, 3]).all() and np.isfinite(losses[:, :3]).all()
    assert same(Wn[3], case.W[3]) and all(not same(Wn[p], case.W[p]) for p in range(3))
    # and so are its moments, step count and running powers: those of creation, while the others' have moved twice
    m, v, step, powers = state()
    assert not m[3].any() and not v[3].any() and step.tolist() == [2, 2, 2, 0] and powers[3].tolist() == [1.0, 1.0]
    assert all(m[p].any() and v[p].any() for p in range(3))
    b1, b2 = cfg["betas"]
    assert all(powers[p].tolist() == [b1 * b1, b2 * b2] for p in range(3))
    # later it gets blocks, same optimizer: its first update is update 1 of a fresh Distiller - step count and moments untouched
    ids2 = ids_of([3, 0, 3, 1, 0], N)
    losses2 = bank_distill(case.traj, bank, bopt, ids2, 1, case.y)
    ref_loss, _, ref_losses, ref_w = _single_reference(case, case.W[3], cfg, case.columns(ids2, 3), 1)
    assert same(losses2[0, 3], ref_losses[0]) and same(ref_losses[0], ref_loss)
    assert same(bank_weights(bank)[3], ref_w) and not same(ref_w, case.W[3])
    assert np.isnan(losses2[0, 2]) and same(bank_weights(bank)[2], Wn[2])      # and policy 2 sat this one out
    m2, v2, step2, powers2 = state()
    assert same(m2[2], m[2]) and same(v2[2], v[2]) and same(powers2[2].view(np.uint32), powers[2].view(np.uint32))
    assert step2.tolist() == [3, 3, 2, 1] and powers2[3].tolist() == [b1, b2]
    bopt.close()


# ------------------------------------------------------------------------------ 6. five updates in one call are five calls -
def test_five_updates_in_one_call_are_five_calls(case):
    from raptor_amd.policy_bank import PolicyBank
    out = []
    for calls in ((5,), (1, 1, 1, 1, 1)):
        bank = PolicyBank(case.device, case.W[:P])
        bopt = BankOpt(bank, CFG)
        losses = np.concatenate([bank_distill(case.traj, bank, bopt, case.ids, c, case.y) for c in calls])
        out.append((losses, bank_weights(bank)))
        bopt.close()
    assert out[0][0].shape == (5, P)
    assert same(out[0][0], out[1][0]) and same(out[0][1], out[1][1])
    for p in range(P):
        assert len(set(out[0][0][:, p].tolist())) == 5, p


# ------------------------------------------------------------------------------ 7. the device repack == a bank packed on the host -
def _fly(case, bank, ids):
    w = World(case.device, case.oracle, N, seed=93, episode_step_limit=9)
    bank.reset()
    w.vector.rollout(case.device, w.env, w.params, w.state, bank, w.rng, 20, "fused", autoreset=True, policy_ids=ids)
    return w.state.numpy(), bank.hidden(N)


def test_the_device_repack_equals_a_bank_packed_on_the_host(case):
    from raptor_amd.policy_bank import PolicyBank
    from raptor_amd.training import BankDistiller
    bank = PolicyBank(case.device, case.W[:P])
    sweep = BankDistiller(bank, lr=[2e-3, 1e-3, 5e-4])
    sweep.step(case.traj, case.ids, target=case.y, updates=3)
    Wn = bank.weights.copy()
    assert all(np.abs(Wn[p] - case.W[p]).max() > 1e-4 for p in range(P))
    fresh = PolicyBank(case.device, Wn)                              # the updated weights, packed on the host
    s_a, h_a = _fly(case, bank, case.ids)
    s_b, h_b = _fly(case, fresh, case.ids)
    assert same(s_a, s_b) and same(h_a, h_b)
    la, ga = bank_loss_grad(case.traj, bank, case.ids, case.y)       # the transposed images
    lb, gb = bank_loss_grad(case.traj, fresh, case.ids, case.y)
    assert same(la, lb) and same(ga, gb) and ga.any()
    # set_weights after an update also refreshes the slot's transposed image
    bank.set_weights(1, case.W[3])
    assert same(bank.weights[1], case.W[3]) and same(bank.weights[0], Wn[0]) and same(bank_weights(bank), bank.weights)
    fresh2 = PolicyBank(case.device, bank.weights)
    la, ga = bank_loss_grad(case.traj, bank, case.ids, case.y)
    l2, g2 = bank_loss_grad(case.traj, fresh2, case.ids, case.y)
    assert same(la, l2) and same(ga, g2) and not same(ga[1], gb[1])


# ------------------------------------------------------------------------------ 8. ordering -
def test_a_rollout_behind_an_enqueued_update_flies_the_new_weights(case):
    import torch
    from raptor_amd.policy_bank import PolicyBank
    from raptor_amd.training import BankDistiller
    bank = PolicyBank(case.device, case.W[:P])
    sweep = BankDistiller(bank, lr=2e-3)
    y = torch.tensor(case.y, device="cuda")
    w = World(case.device, case.oracle, N, seed=93, episode_step_limit=9)
    bank.reset()
    sweep.step(case.traj, case.ids, target=y, updates=3, wait=False)
    w.vector.rollout(case.device, w.env, w.params, w.state, bank, w.rng, 20, "fused", autoreset=True, policy_ids=case.ids)
    s_a, h_a = w.state.numpy(), bank.hidden(N)
    Wn = bank.weights                                                # fetched from the device now
    assert all(np.abs(Wn[p] - case.W[p]).max() > 1e-3 for p in range(P))
    s_b, h_b = _fly(case, PolicyBank(case.device, Wn), case.ids)
    assert same(s_a, s_b) and same(h_a, h_b)


# ------------------------------------------------------------------------------ 9. refusals -
def test_refusals_enqueue_nothing(case):
    import torch
    import raptor_amd.l2f as l2f
    from raptor_amd._lib import RaptorQuadError
    from raptor_amd.policy_bank import PolicyBank
    L = _lib()
    bank = PolicyBank(case.device, case.W[:P])
    other = PolicyBank(case.device, case.W[:P])
    foreign = PolicyBank(l2f.Device(0), case.W[:P])                  # another engine device object (same GPU)
    bopt, other_opt, foreign_opt = BankOpt(bank, CFG), BankOpt(other, CFG), BankOpt(foreign, CFG)
    traj, ids, y, ld = case.traj, case.ids, case.y, _ld(case.traj)
    bank_distill(traj, bank, bopt, ids, 1, y)                        # some history
    before = bank_weights(bank)

    def refused(fn, words):
        with pytest.raises(RaptorQuadError) as e:
            fn()
        assert words in str(e.value), str(e.value)
        assert same(bank_weights(bank), before), words

    def both(words, opt=bopt, **kw):
        a = dict(dict(traj=traj, bank=bank, ids=ids, target=y), **kw)
        refused(lambda: bank_loss_grad(a["traj"], a["bank"], a["ids"], a["target"]), words)
        refused(lambda: bank_distill(a["traj"], a["bank"], opt, a["ids"], 1, a["target"]), words)

    split, too_big = ids.copy(), ids.copy()
    split[100] = 1
    too_big[64:128] = P
    both("differ inside a 64-env block", ids=split)
    both("out of range", ids=too_big)
    refused(lambda: bank_distill(traj, bank, other_opt, ids, 1, y), "another bank")
    both("another device", opt=foreign_opt, bank=foreign)
    refused(lambda: bank_distill(traj, bank, bopt, ids, 0, y), "n_updates")
    empty = case.world.vector.Trajectory(case.world.env, 4)
    both("empty", traj=empty)
    both("ld_target", target=y[:, :, :N - 1])
    loss_d, g_d = torch.empty(P, device="cuda"), torch.empty((P, NW), device="cuda")
    refused(lambda: L.call("rq_trajectory_policies_loss_grad", traj._require("trajectory"), bank._h, ids.ctypes.data, L.fptr(y), ld,
                           INITIAL, C.c_void_p(loss_d.data_ptr()), C.c_void_p(g_d.data_ptr()), DEVICE), "another device")
    refused(lambda: L.call("rq_trajectory_policies_distill", traj._require("trajectory"), bank._h, bopt.h, ids.ctypes.data, L.fptr(y), ld,
                           INITIAL, 1, C.c_void_p(loss_d.data_ptr()), DEVICE), "another device")
    for n_cfg in (0, 2, P + 1):
        cfgs, h = (L.AdamConfig * (P + 1))(*[_adam(CFG[0])] * (P + 1)), C.c_void_p()
        refused(lambda: L.call("rq_bank_optimizer_create", bank._h, cfgs, n_cfg, C.byref(h)), "n_cfg")
        assert not h.value
    losses = bank_distill(traj, bank, bopt, ids, 1, y)               # and after all that it works
    assert np.isfinite(losses).all() and not same(bank_weights(bank), before)
    for o in (bopt, other_opt, foreign_opt):
        o.close()
