"""The weighted distillation loss on the GPU (rq_trajectory_policy_loss_grad_weighted, rq_trajectory_distill_weighted,
rq_trajectory_policies_loss_grad_weighted, rq_trajectory_policies_distill_weighted; csrc/rq_grad_backward.inc under RQ_GRAD_WEIGHTED;
raptor_amd.training.Distiller / BankDistiller with ``weight=``).

 1. every weight 1.0f: the bits of the unweighted calls - loss, gradient, updated weights;
 2. random weights, dropped entries among them, against float64 (tests/weighted_distill_reference.py) within counted bounds;
 3. a 0/1 mask over whole blocks is the unweighted call on a recording that holds those blocks alone;
 4. a bank's policy gets what a single policy gets from the weighted calls on its columns and its weights' columns;
 5. determinism, the three memory modes, NaN wherever an entry does not count, every weight 0, ordering behind an enqueued update;
 6. the refusals; and both distillers through raptor_amd.training.

Slack of each accuracy case: ``pytest tests/test_gpu_weighted_distill.py -m gpu -v -s``."""
import ctypes as C

import numpy as np
import pytest

import policy_grad_reference as R
import weighted_distill_reference as WR
from distill_common import (ASYNC, DEVICE, HOST, INITIAL, Opt, _adam, _bits, _ld, _lib, _perturbed, _record, _targets, distill, forward,
                            get_weights, loss_grad, same)
from gpu_common import World
from rollout_common import ids_of

pytestmark = pytest.mark.gpu

NW = 2084
FILL = 7.0


def c_seed_w(n_counting):
    """Roundings the weighted loss seed adds on a path from dL/da to a gradient element, beyond policy_grad_reference.K_paths,
    counted from the kernels as C_SEED is in tests/test_gpu_distill.py: in the seeded backward the fp32 subtract err = a - y and the
    fp32 product daB = wt * err (rq_grad_backward.inc under RQ_GRAD_WEIGHTED), and in k_policy_loss_reduce_weighted the one rounding
    to fp32 of acc * (2 / W4): 3.  That product is formed in float64 from a float64 W4: W4's sum of n_counting positive weights (at most
    n_counting - 1 roundings of 2^-53 relative), 1 / W4, 2 x (exact) and the product (one each) - (n_counting + 1) 2^-53 =
    (n_counting + 1) 2^-29 of one fp32 rounding, and as much again for the float64 restatement's own W4: the fraction."""
    return 3 + (n_counting + 1) * 2.0 ** -28


# ---- the weighted calls through the C ABI, in any memory mode -----------------------------------------------------------------
def _w2(w):
    w = np.ascontiguousarray(w, np.float32)
    return w[None] if w.ndim == 1 else w


def call_weighted(name, device, traj, head, y, w, start, mid, outs, memory=HOST):
    """name(traj, *head, target, ld_target, weight, ld_weight, weight_steps, start, *mid, *outs, memory); outs: NumPy arrays, filled
    in place (in the device modes: uploaded with what they hold, the call, a wait for the engine's stream, copied back)."""
    L = _lib()
    y = None if y is None else np.ascontiguousarray(y, np.float32)
    w = None if w is None else _w2(w)
    ld_t = 0 if y is None else y.shape[2]
    ld_w, steps = (0, 1) if w is None else (w.shape[1], w.shape[0])
    if memory == HOST:
        L.call(name, traj._require("trajectory"), *head, None if y is None else L.fptr(y), ld_t, None if w is None else L.fptr(w), ld_w,
               steps, start, *mid, *[L.fptr(o) for o in outs], HOST)
        return
    import torch
    yd = None if y is None else torch.tensor(y, device="cuda")
    wd = None if w is None else torch.tensor(w, device="cuda")
    od = [torch.tensor(o, device="cuda") for o in outs]
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    try:
        L.call(name, traj._require("trajectory"), *head, ptr(yd), ld_t, ptr(wd), ld_w, steps, start, *mid, *[ptr(o) for o in od], memory)
    finally:
        L.call("rq_device_synchronize", device._h)
        for o, d in zip(outs, od):
            o[...] = d.cpu().numpy()


def wloss_grad(device, traj, pol, y, w, memory=HOST, start=INITIAL):
    loss, g = np.full(1, FILL, np.float32), np.full(NW, FILL, np.float32)
    call_weighted("rq_trajectory_policy_loss_grad_weighted", device, traj, (pol._handle(),), y, w, start, (), (loss, g), memory)
    return loss[0], g


def wdistill(device, traj, pol, opt, n_updates, y, w, memory=HOST, start=INITIAL):
    losses = np.full(max(n_updates, 1), FILL, np.float32)
    call_weighted("rq_trajectory_distill_weighted", device, traj, (pol._handle(), opt.h), y, w, start, (n_updates,), (losses,), memory)
    return losses


def wbank_loss_grad(device, traj, bank, ids, y, w, memory=HOST, start=INITIAL):
    loss, g = np.full(bank.n_policies, FILL, np.float32), np.full((bank.n_policies, NW), FILL, np.float32)
    ids = np.ascontiguousarray(ids, np.uint32)
    call_weighted("rq_trajectory_policies_loss_grad_weighted", device, traj, (bank._h, ids.ctypes.data), y, w, start, (), (loss, g), memory)
    return loss, g


def wbank_distill(device, traj, bank, opt, ids, n_updates, y, w, memory=HOST, start=INITIAL):
    losses = np.full((max(n_updates, 1), bank.n_policies), FILL, np.float32)
    ids = np.ascontiguousarray(ids, np.uint32)
    call_weighted("rq_trajectory_policies_distill_weighted", device, traj, (bank._h, opt.h, ids.ctypes.data), y, w, start, (n_updates,),
                  (losses,), memory)
    return losses


class BankOpt:
    def __init__(self, bank, cfgs):
        self.cfg, self.h = (_lib().AdamConfig * len(cfgs))(*[_adam(c) for c in cfgs]), C.c_void_p()
        _lib().call("rq_bank_optimizer_create", bank._h, self.cfg, len(cfgs), C.byref(self.h))

    def close(self):
        _lib().call("rq_bank_optimizer_destroy", self.h)


def bank_loss_grad(traj, bank, ids, y):
    L = _lib()
    loss, g = np.full(bank.n_policies, FILL, np.float32), np.full((bank.n_policies, NW), FILL, np.float32)
    ids = np.ascontiguousarray(ids, np.uint32)
    L.call("rq_trajectory_policies_loss_grad", traj._require("trajectory"), bank._h, ids.ctypes.data, L.fptr(y), y.shape[2], INITIAL,
           L.fptr(loss), L.fptr(g), HOST)
    return loss, g


def bank_distill(traj, bank, opt, ids, n_updates, y):
    L = _lib()
    losses = np.empty((n_updates, bank.n_policies), np.float32)
    ids = np.ascontiguousarray(ids, np.uint32)
    L.call("rq_trajectory_policies_distill", traj._require("trajectory"), bank._h, opt.h, ids.ctypes.data, L.fptr(y), y.shape[2], INITIAL,
           n_updates, L.fptr(losses), HOST)
    return losses


def bank_weights(bank):
    L = _lib()
    w = np.empty((bank.n_policies, NW), np.float32)
    L.call("rq_policy_bank_get_weights", bank._h, L.fptr(w))
    return w


# ---- the recordings, made once per shape and left as they are --------------------------------------------------------------
class Recordings:
    def __init__(self, device, oracle, weights):
        self.device, self.oracle, self.weights, self._made = device, oracle, weights, {}

    def get(self, T, n):
        """-> dict(world, traj, y [T, 4, ld] with NaN on frozen steps and padding, rec, wts, ld); NaN in the padding observations"""
        if (T, n) not in self._made:
            world, traj = _record(self.device, self.oracle, n, T, seed=400 + T + n)
            traj.tensors()["obs"][:, :, n:] = float("nan")
            self._made[(T, n)] = dict(world=world, traj=traj, y=_targets(traj, n, seed=T + n), rec=traj.numpy(),
                                      wts=_perturbed(self.weights, 41), ld=_ld(traj))
        return self._made[(T, n)]

    def cache(self, T, n):
        """the float64 forward of `wts` over the recording, once"""
        c = self.get(T, n)
        if "cache" not in c:
            c["cache"] = R.forward(c["wts"].astype(np.float64), c["rec"]["obs"], c["rec"]["done"], "initial")[1]
        return c["cache"]


@pytest.fixture(scope="module")
def recs(device, oracle, weights):
    return Recordings(device, oracle, weights)


def _policy(device, wts):
    from raptor_amd.foundation_policy import Raptor
    pol = Raptor(device, weights=wts)
    pol.reset()
    return pol


def random_weights(T, n, form, seed, ld_w, dirty, zero_wave=False):
    """[1 or T, ld_w] float32 in [0, 2): about a quarter exactly 0; `dirty`: a few negative or NaN (to be dropped); NaN in the
    padding columns; `zero_wave`: envs 64 .. 127 all zero.  Env 0 keeps a positive weight on every step."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.0, 2.0, (1 if form == "env" else T, ld_w)).astype(np.float32)
    r = rng.random(w.shape)
    w[r < 0.25] = 0.0
    if dirty:
        w[(r >= 0.25) & (r < 0.29)] *= -1.0
        w[(r >= 0.29) & (r < 0.32)] = np.nan
    w[:, 0] = rng.uniform(0.5, 2.0, w.shape[0]).astype(np.float32)
    if zero_wave:
        w[:, 64:128] = 0.0
    w[:, n:] = np.nan
    return w


FORMS = ["env", "step"]


# ------------------------------------------------------------------------------ 1. ones are the unweighted bits -
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("T,n", [(1, 1), (2, 63), (1, 65), (20, 130)])
def test_ones_give_the_unweighted_bits(device, recs, T, n, form):
    c = recs.get(T, n)
    traj, y = c["traj"], c["y"]
    ones = np.ones((1 if form == "env" else T, n + 2), np.float32)
    ones[:, n:] = np.nan
    pol = _policy(device, c["wts"])
    l0, g0 = loss_grad(traj, pol, y)
    l1, g1 = wloss_grad(device, traj, pol, y, ones)
    assert same(l1, l0) and same(g1, g0) and g0.any()
    out = []
    for weighted in (False, True):
        pol = _policy(device, c["wts"])
        opt = Opt(pol, lr=2e-3, wd=0.01)
        losses = wdistill(device, traj, pol, opt, 3, y, ones) if weighted else distill(traj, pol, opt, 3, y)
        out.append((losses, get_weights(pol)))
        opt.close()
    assert same(out[0][0], out[1][0]) and same(out[0][1], out[1][1]) and not same(out[0][1], c["wts"])


# ------------------------------------------------------------------------------ the shared bank case -
N, T_BANK, P = 300, 20, 3
BLOCK_IDS = [2, 0, 2, 1, 0]
CFG = [dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.0), dict(lr=1e-3, betas=(0.8, 0.99), eps=1e-7, wd=0.01),
       dict(lr=5e-4, betas=(0.95, 0.9995), eps=1e-8, wd=0.0)]


class BankCase:
    """tests/test_gpu_bank_distill.py's shared case, restated: the recording, its labels, the weights of three policies, and - once
    per set of columns - the recording that holds those columns alone, in order."""

    def __init__(self, recs):
        self.recs, self.device, self.oracle = recs, recs.device, recs.oracle
        c = recs.get(T_BANK, N)
        self.traj, self.y, self.rec = c["traj"], c["y"], c["rec"]
        self.ids = ids_of(BLOCK_IDS, N)
        self.W = np.stack([_perturbed(recs.weights, 30 + k) for k in range(P)])
        self._subs = {}

    def sub(self, cols):
        import torch
        key = tuple(int(k) for k in cols)
        if key not in self._subs:
            n = len(key)
            w = World(self.device, self.oracle, n, seed=5, episode_step_limit=9)
            traj = w.vector.Trajectory(w.env, T_BANK)
            w.vector.rollout(self.device, w.env, w.params, w.state, w.policy, w.rng, T_BANK, "fused", autoreset=True, trajectory=traj)   # sizes it
            src, dst = self.traj.tensors(), traj.tensors()
            idx = torch.tensor(np.asarray(key), device=src["obs"].device)
            for k in ("obs", "act"):
                dst[k][:, :, :n] = src[k][:, :, idx]
            dst["done"][:, :n] = src["done"][:, idx]
            torch.cuda.synchronize()
            y = np.full((T_BANK, 4, _ld(traj)), np.nan, np.float32)
            y[:, :, :n] = self.y[:, :, np.asarray(key)]
            self._subs[key] = (w, traj, y)
        return self._subs[key][1], self._subs[key][2]


@pytest.fixture(scope="module")
def bank_case(recs):
    return BankCase(recs)


@pytest.mark.parametrize("form", FORMS)
def test_ones_give_the_unweighted_bits_for_a_bank(device, bank_case, form):
    from raptor_amd.policy_bank import PolicyBank
    c = bank_case
    ones = np.ones((1 if form == "env" else T_BANK, N), np.float32)
    bank = PolicyBank(device, c.W)
    l0, g0 = bank_loss_grad(c.traj, bank, c.ids, c.y)
    l1, g1 = wbank_loss_grad(device, c.traj, bank, c.ids, c.y, ones)
    assert same(l1, l0) and same(g1, g0) and g0.any()
    out = []
    for weighted in (False, True):
        bank = PolicyBank(device, c.W)
        opt = BankOpt(bank, CFG)
        losses = wbank_distill(device, c.traj, bank, opt, c.ids, 3, c.y, ones) if weighted else bank_distill(c.traj, bank, opt, c.ids, 3, c.y)
        out.append((losses, bank_weights(bank)))
        opt.close()
    assert out[0][0].shape == (3, P) and same(out[0][0], out[1][0]) and same(out[0][1], out[1][1])
    assert all(not same(out[0][1][p], c.W[p]) for p in range(P))


# ------------------------------------------------------------------------------ 2. float64 bounds -
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("T,n", [(1, 1), (37, 16), (2, 63), (1, 65), (20, 130), (60, 300)])
def test_loss_and_gradient_within_the_float64_bounds(device, recs, T, n, form):
    c = recs.get(T, n)
    traj, y, rec, wts = c["traj"], c["y"], c["rec"], c["wts"]
    ld_w = n + 3                                                 # not the trajectory's leading dimension
    assert ld_w != c["ld"]
    w = random_weights(T, n, form, seed=7 * T + n, ld_w=ld_w, dirty=True, zero_wave=n >= 130)
    pol = _policy(device, wts)
    act = forward(traj, pol, INITIAL)                            # the device's own fp32 actions
    loss, g = wloss_grad(device, traj, pol, y, w, memory=DEVICE)  # (a host weight with negative or NaN entries is refused)
    live = np.broadcast_to((rec["done"] != 4)[:, None, :], (T, 4, n))
    wb = w[:, None, :n]
    counts, _ = WR.counting(live, wb)
    nc = int(counts.sum())
    assert nc > 0 and (nc < live.sum() or n * T == 1)
    ref_loss, seed, terms, W4 = WR.weighted_mse(act[:, :, :n], y[:, :, :n], live, wb)
    lb = WR.loss_bound(terms, W4, nc)
    print(f"T={T} n={n} {form}: counting {nc} of {int(live.sum())} live, W4 {W4:.6g}, loss {loss:.6g}, "
          f"|loss - ref| / bound {abs(loss - ref_loss) / lb:.3g}")
    assert np.isfinite(loss) and abs(loss - ref_loss) <= lb
    cache = recs.cache(T, n)
    dact = seed.transpose(0, 2, 1)                               # [T, N, 4], 2 w (a_dev - y) / W4 on counting entries
    g_ref, _ = R.backward(cache, dact)
    waves = (n + 63) // 64
    K = R.K_paths(T, waves)
    b = R.bound(cache, dact, waves)[0] * (K + c_seed_w(nc)) / K
    err = np.abs(g - g_ref)
    assert np.isfinite(g).all()
    print(f"T={T} n={n} {form}: max err/bound {np.max(err / b):.3g}, max |g| {np.abs(g_ref).max():.3g}")
    assert (err <= b).all(), (np.argmax(err / b), np.max(err / b))


# ------------------------------------------------------------------------------ 3. a block mask is a smaller recording -
def test_a_block_mask_is_the_unweighted_call_on_those_blocks_alone(device, bank_case):
    c = bank_case
    mask = np.isin(np.arange(N) // 64, (0, 2, 4)).astype(np.float32)          # block 4 is the ragged one (44 envs)
    cols = np.flatnonzero(mask)
    assert len(cols) == 64 + 64 + 44
    sub_traj, sub_y = c.sub(cols)
    wts = c.W[0]
    l_ref, g_ref = loss_grad(sub_traj, _policy(device, wts), sub_y)
    for w in (mask, np.repeat(mask[None], T_BANK, 0)):
        loss, g = wloss_grad(device, c.traj, _policy(device, wts), c.y, w)
        # numeric equality: a wave of zero weights adds +0.0 to every sum
        assert np.array_equal(loss, l_ref) and np.array_equal(g, g_ref) and g_ref.any()


# ------------------------------------------------------------------------------ 4. bank equals single -
def test_each_policy_of_a_bank_gets_what_the_single_weighted_calls_give(device, bank_case):
    from raptor_amd.policy_bank import PolicyBank
    from raptor_amd.training import BankDistiller
    c = bank_case
    w = random_weights(T_BANK, N, "step", seed=77, ld_w=N, dirty=False)
    bank = PolicyBank(device, c.W)
    L0, G0 = wbank_loss_grad(device, c.traj, bank, c.ids, c.y, w)
    # the same through raptor_amd.training, a NumPy weight and a NumPy target
    L1, G1 = BankDistiller(bank).loss_and_grad(c.traj, c.ids, target=c.y, weight=w)
    assert same(np.asarray(L1), L0) and same(np.asarray(G1), G0)
    bopt = BankOpt(bank, CFG)
    losses = wbank_distill(device, c.traj, bank, bopt, c.ids, 3, c.y, w)
    Wn = bank_weights(bank)
    bopt.close()
    for p in range(P):
        cols = np.flatnonzero(c.ids == p)
        traj, y = c.sub(cols)
        wp = np.ascontiguousarray(w[:, cols])
        pol = _policy(device, c.W[p])
        loss, g = wloss_grad(device, traj, pol, y, wp)
        opt = Opt(pol, **CFG[p])
        ls = wdistill(device, traj, pol, opt, 3, y, wp)
        assert same(L0[p], loss) and same(G0[p], g) and g.any(), p
        assert same(losses[:, p], ls) and len(set(ls.tolist())) == 3, (p, losses[:, p], ls)
        assert same(Wn[p], get_weights(pol)) and not same(Wn[p], c.W[p]), p
        opt.close()
    # none of policy 2's entries counts (its configuration has no weight decay): loss 0, Adam on a zero gradient, weights as they were
    w0 = random_weights(T_BANK, N, "env", seed=78, ld_w=N, dirty=False)
    w0[:, c.ids == 2] = 0.0
    bank = PolicyBank(device, c.W)
    bopt = BankOpt(bank, CFG)
    L2, G2 = wbank_loss_grad(device, c.traj, bank, c.ids, c.y, w0)
    losses = wbank_distill(device, c.traj, bank, bopt, c.ids, 3, c.y, w0)
    Wn = bank_weights(bank)
    bopt.close()
    assert L2[2] == 0.0 and not G2[2].any() and (losses[:, 2] == 0.0).all() and same(Wn[2], c.W[2])
    assert all(L2[p] > 0 and G2[p].any() and not same(Wn[p], c.W[p]) for p in (0, 1))


# ------------------------------------------------------------------------------ 5. masks, memory, determinism -
def test_deterministic_in_every_memory_mode_and_blind_to_what_does_not_count(device, recs):
    import torch
    T, n = 20, 130
    c = recs.get(T, n)
    traj, y, rec, wts = c["traj"], c["y"], c["rec"], c["wts"]
    pol = _policy(device, wts)
    for form in FORMS:
        w = random_weights(T, n, form, seed=91, ld_w=n + 1, dirty=False)
        l1, g1 = wloss_grad(device, traj, pol, y, w)
        l2, g2 = wloss_grad(device, traj, pol, y, w)
        assert same(l1, l2) and same(g1, g2) and g1.any() and l1 > 0
        for memory in (DEVICE, ASYNC):
            lm, gm = wloss_grad(device, traj, pol, y, w, memory=memory)
            assert same(lm, l1) and same(gm, g1), memory
        # three updates: the same bits from host and device memory
        out = []
        for memory in (HOST, DEVICE, ASYNC):
            p = _policy(device, wts)
            opt = Opt(p, lr=2e-3)
            out.append((wdistill(device, traj, p, opt, 3, y, w, memory=memory), get_weights(p)))
            opt.close()
        assert all(same(o[0], out[0][0]) and same(o[1], out[0][1]) for o in out[1:]) and not same(out[0][1], wts)
        # NaN in the targets wherever the entry does not count, and in the observations of frozen steps: the same bits
        live = np.broadcast_to((rec["done"] != 4)[:, None, :], (T, 4, n))
        counts, _ = WR.counting(live, w[:, None, :n])
        assert (live & ~counts).any()
        y2 = y.copy()
        y2[:, :, :n][~counts] = np.nan
        obs, done = traj.tensors()["obs"], traj.tensors()["done"]
        keep = obs.clone()
        try:
            assert (done[:, :n] == 4).any()
            obs.copy_(torch.where((done == 4)[:, None, :], float("nan"), obs))
            torch.cuda.synchronize()
            l3, g3 = wloss_grad(device, traj, pol, y2, w)
        finally:
            obs.copy_(keep)
            torch.cuda.synchronize()
        assert same(l3, l1) and same(g3, g1)
        # the weight's own dropped values: 0, a negative weight and NaN are one and the same (device memory: the host refuses two of them)
        w2 = w.copy()
        zero = np.argwhere(w2[:, :n] == 0.0)
        assert len(zero) >= 2
        w2[tuple(zero[0])], w2[tuple(zero[1])] = -3.0, np.nan
        l4, g4 = wloss_grad(device, traj, pol, y2, w2, memory=DEVICE)
        assert same(l4, l1) and same(g4, g1)
    # every weight 0: loss 0 and a zero gradient, not NaN
    for w in (np.zeros(n, np.float32), np.zeros((T, n), np.float32)):
        l0, g0 = wloss_grad(device, traj, pol, y, w)
        assert l0 == 0.0 and not g0.any()


def test_a_rollout_behind_an_enqueued_weighted_update_flies_the_new_weights(device, oracle, recs):
    import torch
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.training import Distiller, holdout_weights
    T, n = 20, 130
    c = recs.get(T, n)
    traj, wts = c["traj"], c["wts"]
    y = torch.tensor(c["y"], device="cuda")
    train, _ = holdout_weights(n, 0.25, seed=1)
    pol = _policy(device, wts)
    dist = Distiller(pol, lr=2e-3)
    world = World(device, oracle, n, seed=97, episode_step_limit=9)
    dist.step(traj, target=y, updates=3, wait=False, weight=train)         # a NumPy weight beside a device target: uploaded, kept alive
    assert dist._weight_in_flight is not None and dist._weight_in_flight.is_cuda
    pol.reset()
    world.vector.rollout(device, world.env, world.params, world.state, pol, world.rng, 20, "fused", autoreset=True)
    new = pol.weights                                                      # fetched from the device now
    assert np.abs(new - wts).max() > 1e-3
    fresh = Raptor(device, weights=new)
    other = World(device, oracle, n, seed=97, episode_step_limit=9)
    fresh.reset()
    other.vector.rollout(device, other.env, other.params, other.state, fresh, other.rng, 20, "fused", autoreset=True)
    assert np.array_equal(world.state.numpy(), other.state.numpy())
    assert np.array_equal(pol.hidden_state(n), fresh.hidden_state(n))
    # and they are the weights of three weighted updates through the C ABI
    ref = _policy(device, wts)
    opt = Opt(ref, lr=2e-3)
    wdistill(device, traj, ref, opt, 3, c["y"], train)
    assert same(get_weights(ref), new)
    opt.close()


# ------------------------------------------------------------------------------ 6. refusals -
def test_refusals_enqueue_nothing_and_leave_the_outputs_alone(device, bank_case):
    import torch
    from raptor_amd._lib import RaptorQuadError
    from raptor_amd.policy_bank import PolicyBank
    c = bank_case
    traj, y, ids = c.traj, c.y, c.ids
    L = _lib()
    pol, other = _policy(device, c.W[0]), _policy(device, c.W[1])
    bank = PolicyBank(device, c.W)
    opt, other_opt, bopt = Opt(pol), Opt(other), BankOpt(bank, CFG)
    good = np.ones((1, N), np.float32)
    before, bank_before = get_weights(pol), bank_weights(bank)

    def calls(y=y, w=good, memory=HOST, opt=opt, n_updates=1, ids=ids):
        """the four weighted calls -> [(name, thunk returning its outputs)]"""
        return [("loss_grad", lambda: wloss_grad(device, traj, pol, y, w, memory)),
                ("distill", lambda: (wdistill(device, traj, pol, opt, n_updates, y, w, memory),)),
                ("policies_loss_grad", lambda: wbank_loss_grad(device, traj, bank, ids, y, w, memory)),
                ("policies_distill", lambda: (wbank_distill(device, traj, bank, bopt, ids, n_updates, y, w, memory),))]

    def refused(thunks, words, only=None):
        for name, fn in thunks:
            if only and name not in only:
                continue
            with pytest.raises(RaptorQuadError) as e:
                fn()
            assert words in str(e.value) and e.value.status < 0, (name, str(e.value))
            assert same(get_weights(pol), before) and same(bank_weights(bank), bank_before), (name, words)

    # (call_weighted fills the outputs with FILL and hands them over; a raise leaves no array to look at, so the outputs are checked
    # through one call made by hand below)
    refused(calls(w=None), "weight is null")
    for steps in (2, T_BANK - 1, T_BANK + 1):
        refused(calls(w=np.ones((steps, N), np.float32)), "weight_steps")
    refused(calls(w=np.ones((1, N - 1), np.float32)), "ld_weight")
    refused(calls(w=np.ones((T_BANK, N - 1), np.float32)), "ld_weight")
    for value in (-0.5, np.nan, np.inf):
        for steps, at in ((1, (0, 131)), (T_BANK, (7, 299))):
            w = np.ones((steps, N + 2), np.float32)
            w[at] = value
            refused(calls(w=w), f"weight of step {at[0]}, env {at[1]}")
    padded = np.ones((1, N + 2), np.float32)
    padded[:, N:] = np.nan                                       # the padding columns are nobody's
    for name, fn in calls(w=padded):
        fn()
    before, bank_before = get_weights(pol), bank_weights(bank)
    # device memory is announced, a host weight is given
    yd = torch.tensor(y, device="cuda")
    outs = [torch.full((P * NW,), FILL, device="cuda"), torch.full((P,), FILL, device="cuda")]
    torch.cuda.synchronize()
    tp, pp = traj._require("trajectory"), C.c_void_p
    by_hand = [
        ("rq_trajectory_policy_loss_grad_weighted", (pol._handle(),), (), 2),
        ("rq_trajectory_distill_weighted", (pol._handle(), opt.h), (1,), 1),
        ("rq_trajectory_policies_loss_grad_weighted", (bank._h, ids.ctypes.data), (), 2),
        ("rq_trajectory_policies_distill_weighted", (bank._h, bopt.h, ids.ctypes.data), (1,), 1)]
    for name, head, mid, n_out in by_hand:
        o = [pp(outs[1].data_ptr()), pp(outs[0].data_ptr())][:n_out]
        with pytest.raises(RaptorQuadError) as e:
            L.call(name, tp, *head, pp(yd.data_ptr()), yd.shape[2], L.fptr(good), N, 1, INITIAL, *mid, *o, DEVICE)
        assert "the weight lives on another device" in str(e.value), str(e.value)
        # and the outputs of a refused call hold what they held: host arrays, a weight_steps the recording does not have
        loss, g = np.full(P, FILL, np.float32), np.full((P, NW), FILL, np.float32)
        o = [L.fptr(loss), L.fptr(g)][:n_out]
        with pytest.raises(RaptorQuadError) as e:
            L.call(name, tp, *head, L.fptr(y), y.shape[2], L.fptr(good), N, 3, INITIAL, *mid, *o, HOST)
        assert "weight_steps" in str(e.value) and name in str(e.value)
        assert (loss == FILL).all() and (g == FILL).all()
    L.call("rq_device_synchronize", device._h)
    assert (outs[0] == FILL).all() and (outs[1] == FILL).all()
    # the siblings' refusals, through the weighted names
    refused(calls(y=y[:, :, :N - 1]), "ld_target")
    refused(calls(n_updates=0), "n_updates", only=("distill", "policies_distill"))
    refused(calls(opt=other_opt), "another policy", only=("distill",))
    split = ids.copy()
    split[100] = 1
    refused(calls(ids=split), "differ inside a 64-env block", only=("policies_loss_grad", "policies_distill"))
    pol.set_precision("bf16")
    refused(calls(), "fp32 policy only", only=("loss_grad", "distill"))
    pol.set_precision("fp32")
    for name, fn in calls():                                     # and after all that they work
        assert all(np.isfinite(o).all() and not (np.asarray(o) == FILL).any() for o in fn()), name
    assert not same(get_weights(pol), before) and not same(bank_weights(bank), bank_before)
    for o in (opt, other_opt, bopt):
        o.close()


# ------------------------------------------------------------------------------ through raptor_amd.training -
def test_distiller_step_with_a_weight_is_five_c_calls(device, recs):
    from raptor_amd.training import Distiller, holdout_weights
    T, n = 20, 130
    c = recs.get(T, n)
    traj, y, wts = c["traj"], c["y"], c["wts"]
    train, held = holdout_weights(n, 0.3, seed=5)
    assert held.sum() == 39
    pol = _policy(device, wts)
    dist = Distiller(pol, lr=2e-3)
    losses = np.asarray(dist.step(traj, target=y, weight=train, updates=5))
    ref = _policy(device, wts)
    opt = Opt(ref, lr=2e-3)
    ref_losses = np.concatenate([wdistill(device, traj, ref, opt, 1, y, train) for _ in range(5)])
    assert same(losses, ref_losses) and len(set(losses.tolist())) == 5
    assert same(pol.weights, get_weights(ref)) and not same(pol.weights, wts)
    opt.close()


def test_the_held_out_loss_agrees_with_the_torch_statement(device, recs):
    """loss_and_grad(traj, weight=held_out) against training.weighted_mse on trajectory_actions' output - the same fp32 actions,
    bit for bit, so both are fp32 evaluations of one sum and each is held to the float64 loss bound of the reference file: torch's
    (a - y) ** 2 times w is the same four roundings per term, its fp32 sum is at most N - 1 more in any order, its normaliser - a sum
    of 0/1 weights below 2^24 - is exact, and its division rounds once."""
    import torch
    from raptor_amd.training import Distiller, holdout_weights, trajectory_actions, weighted_mse
    T, n = 20, 130
    c = recs.get(T, n)
    traj, rec, wts = c["traj"], c["rec"], c["wts"]
    _, held = holdout_weights(n, 0.3, seed=5)
    pol = _policy(device, wts)
    y = torch.tensor(np.nan_to_num(c["y"][:, :, :n], nan=0.0), device="cuda")      # (torch reads every entry: finite labels)
    live = torch.tensor(rec["done"] != 4, device="cuda")[:, None, :].expand(T, 4, n)
    for w in (held, np.repeat(held[None], T, 0) * np.linspace(1.0, 2.0, T, dtype=np.float32)[:, None]):
        wt = torch.tensor(w, device="cuda")
        wt = wt[None, None, :] if w.ndim == 1 else wt[:, None, :]
        integer = w.ndim == 1
        with torch.no_grad():
            act = trajectory_actions(traj, pol, torch.tensor(wts, device="cuda"))[:, :, :n]
            torch_loss = float(weighted_mse(act, y, live, wt))
        loss, grad = Distiller(pol).loss_and_grad(traj, target=y, weight=w)
        loss = float(loss)
        lv = np.broadcast_to((rec["done"] != 4)[:, None, :], (T, 4, n))
        wb = w[None, None, :] if w.ndim == 1 else w[:, None, :]
        counts, _ = WR.counting(lv, wb)
        nc = int(counts.sum())
        ref, _, terms, W4 = WR.weighted_mse(act.cpu().numpy(), y.cpu().numpy(), lv, wb)
        lb = WR.loss_bound(terms, W4, nc)
        # torch sums the weights in fp32: exact for the 0/1 mask; for the graded weights nc - 1 more roundings of the normaliser
        tb = lb if integer else lb + (nc - 1) * WR.U * ref
        print(f"rows {wb.shape[0]}: counting {nc}, loss {loss:.6g}; |device - ref| / bound {abs(loss - ref) / lb:.3g}, "
              f"|torch - ref| / bound {abs(torch_loss - ref) / tb:.3g}")
        assert nc > 0 and abs(loss - ref) <= lb and abs(torch_loss - ref) <= tb
        assert np.isfinite(grad.cpu().numpy()).all() and grad.cpu().numpy().any()
