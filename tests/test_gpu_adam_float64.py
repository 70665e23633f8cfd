"""k_adam_repack / k_adam_repack_bank (csrc/rq_adam_repack.inc) against float64 on ARBITRARY state and gradients, through the
optimizer's state seam (rq_optimizer_get_state / _set_state / _apply, rq_bank_optimizer_get_state / _set_state): exact inputs at
every update, so the bound is one rounding to fp32 however long the run.  Reference, bound and design: tests/adam_reference.py
(tests/test_adam_bound_cpu.py shows that the bound admits the kernel as it is and rejects nine subtly wrong ones).

What is held: w', m', v' of one update on the design input for every row of the hyper-parameter grid and every step count; a free
run of 300 updates, each from the device's own previous bits; save / restore / continue; distill == loss_grad + apply, and the
repack behind apply; set_lr in stream order; the bank's kernel tied to the single one, its skipped policy and its set_lr; the
refusals of the five entry points.

MEASURED on an MI355X (``pytest tests/test_gpu_adam_float64.py -m gpu -v -s``), largest |got - ref| / bound; 17 tests, under a second
beside the recordings.  The figures are the first run's; no constant of the bound or of the design was changed after it (the one change
after the first run: the design's w_cancel weight where the update is 0 - the lr = 0 row - became +0 instead of the update's own -0,
because x = -0 - -0 is +0 in IEEE arithmetic, in the reference as on the device, and the test compares the weights' bits there).
  one update on the design, over the six step counts         w'       m'       v'
    row 0  (3e-3, .9, .999, 1e-8, 0)                          0.9866   0.9968   0.9903
    row 1  (1e-3, .8, .99, 1e-7, .01)                         0.9828   0.9752   0.9469
    row 2  (1e-3, 0, .999, 1e-8, 0)                           0.9889   0        0.9903      (beta1 = 0: m' = g exactly)
    row 3  (1e-3, .9, 0, 1e-8, 0)                             0.9992   0.9968   0.9864
    row 4  (0, .9, .999, 1e-8, .01)                           0        0.9968   0.9903      (lr = 0: w' = w exactly)
    row 5  (1, .9, .999, 1, .5)                               0.9884   0.9968   0.9903
    row 6  (1e-3, .9, .999, 0, 0)                             0.9855   0.9968   0.9903
  the free run, over 300 updates                              0.9993   0.9994   0.9991
  set_lr between two enqueued applies, the switched reference 0.9876   0.9981   0.9664
  the bank after set_lr, worst of 3 policies x 2 settings     0.9932   0.9991   0.9895
Every ratio is a little under 1 because the bound IS one rounding to fp32 and some element always uses nearly all of it; the CPU
emulation (tests/test_adam_bound_cpu.py) reaches 0.9992 / 0.9968 / 0.9903 on the same design.  Denormal results are KEPT by the
device's float64 -> fp32 conversion (m = 1e-38, g = 0 gives m' = 8.999999e-39 on every row with 0 < beta1 < 1), not flushed.
Not measured: the seam on a second device of one process (DeviceScope is the same code as the other optimizer calls'), a bank
larger than 3 policies through the state calls, RQ_DST_DEVICE_ASYNC of rq_optimizer_apply from another stream than torch's default.
"""
import ctypes as C

import numpy as np
import pytest

import adam_reference as A
from distill_common import (ASYNC, DEVICE, HOST, INITIAL, Opt, _bits, _ld, _lib, _perturbed, _record, _targets, distill, get_weights,
                            loss_grad, opt_apply, opt_set_state, opt_state, same)
from gpu_common import World
from rollout_common import ids_of
from test_gpu_bank_distill import CFG, BankOpt, bank_distill, bank_loss_grad, bank_weights
from test_gpu_weighted_distill import wdistill, wloss_grad

pytestmark = pytest.mark.gpu

NW = A.NW
SPECIAL = [*A.NAN_AT, *(i for i, _ in A.INF_AT)]


def _opt(pol, cfg):
    lr, b1, b2, eps, wd = cfg
    return Opt(pol, lr=lr, betas=(b1, b2), eps=eps, wd=wd)


def _cfg_tuple(c):
    return (c["lr"], c["betas"][0], c["betas"][1], c["eps"], c["wd"])


def _policy(device, w):
    from raptor_amd.foundation_policy import Raptor
    pol = Raptor(device, weights=w)
    pol.reset()
    return pol


def _inside(got, inputs, cfg, powers):
    """(w', m', v') of the device against the float64 reference from `inputs` -> the three largest ratios; asserts the bound"""
    ref = A.adam_exact(*inputs, cfg, powers)
    b = A.bound(*inputs, cfg, powers)
    worst = []
    for k, name in enumerate(("w'", "m'", "v'")):
        ok, ratio = A.agrees(got[k], ref[k], b[k])
        assert ok.all(), (name, cfg, int(np.argmax(ratio)), float(np.max(ratio)), got[k][np.argmax(ratio)], ref[k][np.argmax(ratio)])
        worst.append(float(ratio.max()))
    return worst


def _outside(got_w, inputs, cfg, powers):
    ref = A.adam_exact(*inputs, cfg, powers)
    return not A.agrees(got_w, ref[0], A.bound(*inputs, cfg, powers)[0])[0].all()


def _update(pol, opt, w, m, v, g, step, powers):
    """weights and state injected, one apply -> (w', m', v', step', powers')"""
    pol.set_weights(w)
    opt_set_state(opt, m, v, step, powers)
    opt_apply(opt, g)
    m1, v1, s1, p1 = opt_state(opt)
    return get_weights(pol), m1, v1, s1, p1


# ------------------------------------------------------------------------------ 1. the kernel against float64, directly -
@pytest.mark.parametrize("row", range(len(A.GRID)))
def test_one_update_on_the_design_lies_inside_the_bound(device, row):
    cfg = A.GRID[row]
    lr, b1, b2, eps, wd = cfg
    pol = _policy(device, np.zeros(NW, np.float32))
    opt = _opt(pol, cfg)
    worst = np.zeros(3)
    for step in A.STEPS:
        powers = A.powers_of(cfg, step)
        w, m, v, g = A.check_design(cfg, powers)
        w1, m1, v1, s1, p1 = _update(pol, opt, w, m, v, g, step, powers)
        worst = np.maximum(worst, _inside((w1, m1, v1), (w, m, v, g), cfg, powers))
        assert s1 == step + 1
        for k, beta in enumerate((b1, b2)):
            assert abs(p1[k] - powers[k] * beta) <= 2.0 ** -52 * abs(powers[k] * beta), (step, k)
        # a NaN or an infinite gradient element touches its own element only
        g0 = g.copy()
        g0[SPECIAL] = 0.0
        w2, m2, v2, _, _ = _update(pol, opt, w, m, v, g0, step, powers)
        others = np.delete(np.arange(NW), SPECIAL)
        assert same(w1[others], w2[others]) and same(m1[others], m2[others]) and same(v1[others], v2[others])
        assert np.isnan(w1[SPECIAL]).all() and np.isnan(m1[list(A.NAN_AT)]).all() and np.isfinite(w2[SPECIAL]).all()
        if lr == 0.0:                        # the weights' bits stay on every element whose gradient is finite; the moments move
            assert same(w1[others], w[others]) and not same(m1[others], m[others]) and not same(v1[others], v[others])
        if eps == 0.0:                       # 0 / (sqrt(0) + 0): NaN, as the reference (and torch), element for element
            z = A.family_index("g0_mv0")
            assert np.isnan(w1[z]).all() and np.isnan(A.adam_exact(w, m, v, g, cfg, powers)[0][z]).all()
            assert not m1[z].any() and not v1[z].any()
        d = A.family_index("denormal_out")
        if step == 0 and 0 < b1 < 1:
            kept = bool((m1[d] != 0).all())
            print(f"row {row}: denormal m' {'kept' if kept else 'flushed'} ({m1[d][0]!r} from m = {m[d][0]!r})")
    print(f"row {row} {cfg}: largest |got - ref| / bound over {len(A.STEPS)} step counts: w' {worst[0]:.4f}  m' {worst[1]:.4f}  v' {worst[2]:.4f}")
    opt.close()


# ------------------------------------------------------------------------------ 2. a free run with exact inputs at every step -
def test_a_free_run_of_300_updates_is_one_rounding_from_its_own_bits_every_time(device):
    cfg = A.GRID[1]
    rng = np.random.default_rng(21)
    w = (0.3 * rng.standard_normal(NW)).astype(np.float32)
    g0 = (0.1 * rng.standard_normal(NW)).astype(np.float32)
    scale = (1.0, -1.0, 1e-3, 0.0, 37.0)
    pol = _policy(device, w)
    opt = _opt(pol, cfg)
    m, v, step, powers = opt_state(opt)
    assert not m.any() and not v.any() and step == 0 and powers.tolist() == [1.0, 1.0]
    worst = np.zeros(3)
    for k in range(300):
        g = (g0 * np.float32(scale[k % 5])).astype(np.float32)
        opt_apply(opt, g)
        m1, v1, s1, p1 = opt_state(opt)
        w1 = get_weights(pol)
        worst = np.maximum(worst, _inside((w1, m1, v1), (w, m, v, g), cfg, powers))
        assert s1 == k + 1
        w, m, v, powers = w1, m1, v1, p1
    for k, beta in enumerate(cfg[1:3]):
        assert abs(powers[k] - beta ** 300) <= 300 * 2.0 ** -52 * beta ** 300
    print(f"free run: largest |got - ref| / bound over 300 updates: w' {worst[0]:.4f}  m' {worst[1]:.4f}  v' {worst[2]:.4f}")
    opt.close()


# ------------------------------------------------------------------------------ 3. save, restore, continue -
@pytest.fixture(scope="module")
def rec65(device, oracle):
    w, traj = _record(device, oracle, 65, 3, seed=401)
    return w, traj, _targets(traj, 65, seed=41)


def _all_bits(pol, opt):
    m, v, step, powers = opt_state(opt)
    return (_bits(get_weights(pol)).tolist(), _bits(m).tolist(), _bits(v).tolist(), step, powers.view(np.uint64).tolist())


def test_a_restored_run_continues_bit_for_bit(device, weights, rec65):
    _, traj, y = rec65
    cfg = A.GRID[1]
    w0 = _perturbed(weights, 51)
    a = _policy(device, w0)
    oa = _opt(a, cfg)
    la = np.concatenate([distill(traj, a, oa, 1, y) for _ in range(7)])
    b = _policy(device, w0)
    ob = _opt(b, cfg)
    lb = np.concatenate([distill(traj, b, ob, 1, y) for _ in range(3)])
    m, v, step, powers = opt_state(ob)
    assert step == 3 and m.any() and v.any()
    c = _policy(device, get_weights(b))
    oc = _opt(c, cfg)
    opt_set_state(oc, m, v, step, powers)
    lc = np.concatenate([distill(traj, c, oc, 1, y) for _ in range(4)])
    assert same(la[:3], lb) and same(la[3:], lc) and len(set(la.tolist())) == 7
    assert _all_bits(a, oa) == _all_bits(c, oc) and opt_state(oa)[2] == 7
    for o in (oa, ob, oc):
        o.close()


# ------------------------------------------------------------------------------ 4. distill is loss_grad then apply -
@pytest.mark.parametrize("weighted", [False, True])
def test_distill_is_loss_grad_then_apply_and_the_repack_behind_apply(device, weights, rec65, weighted):
    _, traj, y = rec65
    n, cfg = 65, A.GRID[1]
    w0 = _perturbed(weights, 52)
    wt = np.random.default_rng(53).uniform(0.0, 2.0, (3, _ld(traj))).astype(np.float32)
    a, b = _policy(device, w0), _policy(device, w0)
    oa, ob = _opt(a, cfg), _opt(b, cfg)
    if weighted:
        la = wdistill(device, traj, a, oa, 1, y, wt)
        lb, g = wloss_grad(device, traj, b, y, wt)
    else:
        la = distill(traj, a, oa, 1, y)
        lb, g = loss_grad(traj, b, y)
    opt_apply(ob, g)
    assert _bits(la[0]) == _bits(lb) and g.any()
    assert _all_bits(a, oa) == _all_bits(b, ob) and not same(get_weights(b), w0)
    # the images apply rebuilt, and the 16-bit ones it made stale: those of a policy packed on the host from the same weights
    fresh = _policy(device, get_weights(b))
    obs = np.random.default_rng(54).standard_normal((n, 22)).astype(np.float32)
    b.reset()
    assert same(b.evaluate_step(obs), fresh.evaluate_step(obs))
    l1, g1 = loss_grad(traj, b, y)
    l2, g2 = loss_grad(traj, fresh, y)
    assert same(g1, g2) and _bits(l1) == _bits(l2) and not same(g1, g)
    b.set_precision("bf16"); fresh.set_precision("bf16")
    b.reset(); fresh.reset()
    assert same(b.evaluate_step(obs), fresh.evaluate_step(obs))
    oa.close(); ob.close()


def test_the_python_wrappers_are_the_c_calls(device, weights, rec65, bank_case):
    import torch
    from raptor_amd.training import BankDistiller, Distiller
    _, traj, y = rec65
    lr, b1, b2, eps, wd = cfg = A.GRID[1]
    w0 = _perturbed(weights, 55)
    a, b = _policy(device, w0), _policy(device, w0)
    oa = _opt(a, cfg)
    d = Distiller(b, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for numpy_grad in (False, True):
        _, g = loss_grad(traj, a, y)
        opt_apply(oa, g)
        _, gd = d.loss_and_grad(traj, target=y if numpy_grad else torch.tensor(y, device="cuda"))
        assert isinstance(gd, np.ndarray) == numpy_grad
        d.apply(gd)
    st = d.state()
    m, v, step, powers = opt_state(oa)
    assert same(st["m"], m) and same(st["v"], v) and st["step"] == step == 2 and st["beta_powers"].tolist() == powers.tolist()
    assert same(b.weights, get_weights(a)) and not same(b.weights, w0)
    c = _policy(device, b.weights)
    d2 = Distiller(c, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    d2.set_state(**st)
    l1, l2 = distill(traj, a, oa, 1, y), d2.step(traj, target=y)
    assert _bits(l1[0]) == _bits(np.float32(l2[0])) and same(c.weights, get_weights(a)) and same(d2.state()["m"], opt_state(oa)[0])
    oa.close()
    bank, bopt = bank_case.bank()
    from raptor_amd.policy_bank import PolicyBank
    sweep = BankDistiller(PolicyBank(device, bank_case.W), lr=[c_["lr"] for c_ in CFG])
    zero = sweep.state()
    assert not zero["m"].any() and zero["step"].tolist() == [0] * P and zero["beta_powers"].tolist() == [[1.0, 1.0]] * P
    m, v, step, powers = opt_state(bopt, slots=P, name="rq_bank_optimizer_get_state")
    sweep.set_state(m, v, step, powers)
    got = sweep.state()
    assert same(got["m"], m) and same(got["v"], v) and got["step"].tolist() == step.tolist() and got["beta_powers"].tolist() == powers.tolist()
    bopt.close()


# ------------------------------------------------------------------------------ 5. stream order -
def test_set_lr_between_two_enqueued_applies_holds_for_the_second_only(device):
    import torch
    L = _lib()
    cfg = A.GRID[0]
    lr1, lr2 = cfg[0], 5.0 * cfg[0]
    rng = np.random.default_rng(61)
    w, m = (0.3 * rng.standard_normal(NW)).astype(np.float32), (0.1 * rng.standard_normal(NW)).astype(np.float32)
    v, g = ((0.1 * rng.standard_normal(NW)) ** 2).astype(np.float32), (0.1 * rng.standard_normal(NW)).astype(np.float32)
    g2 = (0.1 * rng.standard_normal(NW)).astype(np.float32)
    step, powers = 9, A.powers_of(cfg, 9)
    pol = _policy(device, w)
    opt = _opt(pol, cfg)
    opt_set_state(opt, m, v, step, powers)
    gd, g2d = torch.tensor(g, device="cuda"), torch.tensor(g2, device="cuda")
    torch.cuda.synchronize()
    L.call("rq_optimizer_apply", opt.h, C.c_void_p(gd.data_ptr()), ASYNC)
    L.call("rq_optimizer_set_lr", opt.h, lr2)
    L.call("rq_optimizer_apply", opt.h, C.c_void_p(g2d.data_ptr()), ASYNC)
    m2, v2, s2, p2 = opt_state(opt)                  # behind everything enqueued
    w2 = get_weights(pol)
    assert s2 == step + 2
    # the first update's own bits, from a run of it alone at each rate (the kernel is deterministic)
    first = {}
    for lr in (lr1, lr2):
        c = (lr, *cfg[1:])
        p = _policy(device, w)
        o = _opt(p, c)
        first[lr] = _update(p, o, w, m, v, g, step, powers)
        _inside(first[lr][:3], (w, m, v, g), c, powers)
        o.close()
    w1, m1, v1, _, p1 = first[lr1]
    switched = (lr2, *cfg[1:])
    print("switched:", _inside((w2, m2, v2), (w1, m1, v1, g2), switched, p1))
    assert _outside(w2, (w1, m1, v1, g2), cfg, p1)                                       # lr1 throughout
    wb, mb, vb, _, pb = first[lr2]
    assert _outside(w2, (wb, mb, vb, g2), switched, pb)                                  # lr2 throughout
    # the device-memory mode that waits
    L.call("rq_optimizer_apply", opt.h, C.c_void_p(gd.data_ptr()), DEVICE)
    assert opt_state(opt)[2] == step + 3
    opt.close()


# ------------------------------------------------------------------------------ 6. the bank -
P = 3


def _injected(p):
    """a different (m, v, step, powers) per policy"""
    r = np.random.default_rng(70 + p)
    cfg = _cfg_tuple(CFG[p])
    step = (0, 5, 999)[p]
    return ((0.01 * r.standard_normal(NW)).astype(np.float32), ((0.01 * r.standard_normal(NW)) ** 2).astype(np.float32), step,
            A.powers_of(cfg, step))


class BankCase:
    def __init__(self, device, oracle, weights):
        import torch
        self.device, self.n, self.T = device, 192, 3
        self.world, self.traj = _record(device, oracle, self.n, self.T, seed=402)
        self.y = _targets(self.traj, self.n, seed=42)
        self.W = np.stack([_perturbed(weights, 80 + p) for p in range(P)])
        self.ids = ids_of([0, 1, 2], self.n)
        self.state = [_injected(p) for p in range(P)]
        # block p alone: a 64-env recording holding the shared one's columns
        self.subs = []
        for p in range(P):
            cols = np.flatnonzero(self.ids == p)
            w = World(device, oracle, 64, seed=5, episode_step_limit=9)
            traj = w.vector.Trajectory(w.env, self.T)
            w.vector.rollout(device, w.env, w.params, w.state, w.policy, w.rng, self.T, "fused", autoreset=True, trajectory=traj)
            src, dst = self.traj.tensors(), traj.tensors()
            idx = torch.tensor(cols, device=src["obs"].device)
            for k in ("obs", "act"):
                dst[k][:, :, :64] = src[k][:, :, idx]
            dst["done"][:, :64] = src["done"][:, idx]
            torch.cuda.synchronize()
            y = np.full((self.T, 4, _ld(traj)), np.nan, np.float32)
            y[:, :, :64] = self.y[:, :, cols]
            self.subs.append((w, traj, y))

    def bank(self):
        """a fresh bank and its optimizer with the per-policy state injected"""
        from raptor_amd.policy_bank import PolicyBank
        L = _lib()
        bank = PolicyBank(self.device, self.W)
        bopt = BankOpt(bank, CFG)
        m, v = np.stack([s[0] for s in self.state]), np.stack([s[1] for s in self.state])
        step, powers = np.array([s[2] for s in self.state], np.uint32), np.stack([s[3] for s in self.state])
        L.call("rq_bank_optimizer_set_state", bopt.h, L.fptr(m), L.fptr(v), step.ctypes.data, powers.ctypes.data)
        return bank, bopt

    @staticmethod
    def read(bank, bopt):
        m, v, step, powers = opt_state(bopt, slots=P, name="rq_bank_optimizer_get_state")
        return bank_weights(bank), m, v, step, powers


@pytest.fixture(scope="module")
def bank_case(device, oracle, weights):
    return BankCase(device, oracle, weights)


def _slot_bits(read, p):
    w, m, v, step, powers = read
    return (_bits(w[p]).tolist(), _bits(m[p]).tolist(), _bits(v[p]).tolist(), int(step[p]), powers[p].view(np.uint64).tolist())


def test_each_policy_of_a_bank_gets_the_single_optimizers_bits_from_its_injected_state(bank_case):
    case = bank_case
    bank, bopt = case.bank()
    before = case.read(bank, bopt)
    for p in range(P):                               # set_state then get_state: the bits given
        assert _slot_bits(before, p) == _slot_bits((case.W, *[np.stack([s[k] for s in case.state]) for k in (0, 1)],
                                                    [s[2] for s in case.state], np.stack([s[3] for s in case.state])), p)
    losses = bank_distill(case.traj, bank, bopt, case.ids, 1, case.y)
    after = case.read(bank, bopt)
    for p in range(P):
        _, traj, y = case.subs[p]
        pol = _policy(case.device, case.W[p])
        opt = _opt(pol, _cfg_tuple(CFG[p]))
        opt_set_state(opt, *case.state[p])
        ls = distill(traj, pol, opt, 1, y)
        assert _bits(ls[0]) == _bits(losses[0, p]), p
        assert _slot_bits(after, p) == _all_bits(pol, opt), p
        assert after[3][p] == case.state[p][2] + 1 and not same(after[0][p], case.W[p])
        opt.close()
    bopt.close()


def test_a_skipped_policy_keeps_weights_moments_step_and_powers(bank_case):
    case = bank_case
    bank, bopt = case.bank()
    before = case.read(bank, bopt)
    losses = bank_distill(case.traj, bank, bopt, ids_of([0, 2, 2], case.n), 2, case.y)
    after = case.read(bank, bopt)
    assert np.isnan(losses[:, 1]).all() and np.isfinite(losses[:, [0, 2]]).all()
    assert _slot_bits(after, 1) == _slot_bits(before, 1)
    for p in (0, 2):
        assert after[3][p] == before[3][p] + 2 and not same(after[0][p], before[0][p]) and not same(after[1][p], before[1][p])
        assert not same(after[2][p], before[2][p]) and (after[4][p] != before[4][p]).all()
    bopt.close()


def test_bank_set_lr_changes_the_rate_of_the_next_update_and_nothing_else(bank_case):
    case = bank_case
    L = _lib()
    bank, bopt = case.bank()
    for rates in ([4e-3, 0.0, 2e-4], [7e-4]):
        before = case.read(bank, bopt)
        r = np.asarray(rates, np.float64)
        L.call("rq_bank_optimizer_set_lr", bopt.h, r.ctypes.data, r.size)
        assert all(_slot_bits(case.read(bank, bopt), p) == _slot_bits(before, p) for p in range(P))
        _, G = bank_loss_grad(case.traj, bank, case.ids, case.y)       # the gradient the update is about to use
        bank_distill(case.traj, bank, bopt, case.ids, 1, case.y)
        after = case.read(bank, bopt)
        for p in range(P):
            old = _cfg_tuple(CFG[p])
            new = (float(r[p % r.size]), *old[1:])
            inputs = (before[0][p], before[1][p], before[2][p], G[p])
            print(f"rates {rates}, policy {p}:", _inside((after[0][p], after[1][p], after[2][p]), inputs, new, before[4][p]))
            assert after[3][p] == before[3][p] + 1
            for k in (0, 1):
                assert abs(after[4][p][k] - before[4][p][k] * old[1 + k]) <= 2.0 ** -52 * before[4][p][k] * old[1 + k]
            if new[0] != old[0] and rates == [4e-3, 0.0, 2e-4]:
                assert _outside(after[0][p], inputs, old, before[4][p]), p          # not the rate it was created with
    bopt.close()


# ------------------------------------------------------------------------------ 7. refusals -
def test_refusals_leave_weights_state_and_outputs_alone(device, bank_case):
    from raptor_amd._lib import RaptorQuadError
    L = _lib()
    rng = np.random.default_rng(91)
    w = (0.3 * rng.standard_normal(NW)).astype(np.float32)
    g = (0.1 * rng.standard_normal(NW)).astype(np.float32)
    pol = _policy(device, w)
    opt = _opt(pol, A.GRID[1])
    opt_apply(opt, g)                                # some history
    before = _all_bits(pol, opt)
    bank, bopt = bank_case.bank()
    bank_before = [_slot_bits(bank_case.read(bank, bopt), p) for p in range(P)]

    def refused(fn, words):
        with pytest.raises(RaptorQuadError) as e:
            fn()
        assert words in str(e.value), str(e.value)
        assert _all_bits(pol, opt) == before, words
        assert [_slot_bits(bank_case.read(bank, bopt), p) for p in range(P)] == bank_before, words

    def outs(slots):
        return [np.full((slots, NW), 7.0, np.float32), np.full((slots, NW), 7.0, np.float32), np.full(slots, 7, np.uint32),
                np.full((slots, 2), 7.0, np.float64)]

    ptr = lambda a: a.ctypes.data
    for name, h, slots in (("rq_optimizer_get_state", opt.h, 1), ("rq_bank_optimizer_get_state", bopt.h, P)):
        for missing in range(-1, 4):
            o = outs(slots)
            args = [None if k == missing else ptr(a) for k, a in enumerate(o)]
            refused(lambda: L.call(name, None if missing < 0 else h, *args), "null argument")
            assert all((a == 7).all() for a in o), (name, missing)
    m, v, powers = np.zeros((P, NW), np.float32), np.ones((P, NW), np.float32), np.full((P, 2), 0.5)
    steps = np.full(P, 3, np.uint32)
    single = [ptr(m), ptr(v), 3, ptr(powers)]
    for missing in (-1, 0, 1, 3):
        args = [None if k == missing else a for k, a in enumerate(single)]
        refused(lambda: L.call("rq_optimizer_set_state", None if missing < 0 else opt.h, *args), "null argument")
    many = [ptr(m), ptr(v), ptr(steps), ptr(powers)]
    for missing in range(-1, 4):
        args = [None if k == missing else a for k, a in enumerate(many)]
        refused(lambda: L.call("rq_bank_optimizer_set_state", None if missing < 0 else bopt.h, *args), "null argument")
    refused(lambda: L.call("rq_optimizer_apply", None, L.fptr(g), HOST), "null argument")
    refused(lambda: L.call("rq_optimizer_apply", opt.h, None, HOST), "null argument")
    for memory in (-1, 3):
        refused(lambda: L.call("rq_optimizer_apply", opt.h, L.fptr(g), memory), "memory must be 0, 1 or 2")
    refused(lambda: L.call("rq_optimizer_apply", opt.h, L.fptr(g), DEVICE), "another device")          # host memory announced as device
    pol.set_precision("bf16")
    refused(lambda: opt_apply(opt, g), "fp32 policy only")
    pol.set_precision("fp32")
    opt_apply(opt, g)                                # and after all that it works
    assert _all_bits(pol, opt) != before
    # an optimizer that outlives its policy, or its bank: refused by name, nothing followed
    pol._fin.detach()
    L.call("rq_policy_destroy", pol._h)
    pol._h = None
    o = outs(1)
    for fn in (lambda: opt_apply(opt, g), lambda: opt_set_state(opt, m[0], v[0], 3, powers[0]),
               lambda: L.call("rq_optimizer_get_state", opt.h, *[ptr(a) for a in o])):
        with pytest.raises(RaptorQuadError) as e:
            fn()
        assert "policy was destroyed" in str(e.value), str(e.value)
    assert all((a == 7).all() for a in o)
    bank._fin.detach()
    L.call("rq_policy_bank_destroy", bank._h)
    bank._h = None
    o = outs(P)
    for fn in (lambda: L.call("rq_bank_optimizer_get_state", bopt.h, *[ptr(a) for a in o]),
               lambda: L.call("rq_bank_optimizer_set_state", bopt.h, *many)):
        with pytest.raises(RaptorQuadError) as e:
            fn()
        assert "bank was destroyed" in str(e.value), str(e.value)
    assert all((a == 7).all() for a in o)
    opt.close(); bopt.close()
