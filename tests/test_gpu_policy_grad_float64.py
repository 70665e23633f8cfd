"""The learner's backward held to float64 beyond the shipped checkpoint: k_policy_grad_backward, its four loss-seeded siblings, the two
reductions and the gain table on every weight family x input family of tests/actor_reference.py, over short teacher-forced windows
(T <= 3) whose observations, done codes and entering states the test writes into the recording.  The bound is
``policy_grad_window.window_bound`` (an error carried beside every value; proved on the CPU in tests/test_policy_grad_bound_cpu.py),
x (1 + 2^-20); ``policy_grad_reference.bound`` does not hold on these weights.  Envs with a step near a ReLU kink get dL/da = 0
(at most 2 % of a case, asserted on the CPU).

Largest |got - ref| / bound on an MI355X per weight family, over every input family, n in {1, 17, 64, 65, 130}, T in {1, 3} and both
starts (``pytest -s`` prints them per input family too); no constant of the bound or of the model was changed after the first GPU
run, and no kernel:

                  shipped perturbed fresh  sat8   sat64  tiny   signed_pos signed_neg
    unseeded      0.128   0.171     0.157  0.178  0.192  0.207  0.268      0.164
    seed's grad.  -       -         0.048  0.046  0.152  -      0.176      -
    gain table    0.030   0.026     0.036  0.018  0.078  0.045  0.161      0.036

"unseeded" is rq_trajectory_policy_backward (g and dL/dh_start); "seed's grad." the unseeded kernel on gact = fl(a - y), to which
rq_trajectory_policy_loss_grad is tied bit for bit (x 2 / M, one rounding) in every case - the bits never differed, so C_SEED is
not needed; its loss peaks at 0.023 of ``distill_reference.loss_bound``.  The gain table left no env-bucket out for a kink.  The
largest unseeded ratios per input family: normal 0.227, small 0.230, large 0.207, exact_h 0.268, wide_h 0.232, strided 0.247.  The
NumPy float32 emulation of the kernel peaks at 0.23 on the same cases.  The GPU's gradient against the reference of weights with
the r and z rows exchanged leaves the bound in 2 075 of 2 084 entries, by up to 5e3 x.
"""
import numpy as np
import pytest

import actor_reference as AR
import distill_reference as D
import policy_grad_window as PW
from distill_common import CURRENT, INITIAL, _ld, forward, loss_grad, same
from gpu_common import World
from rollout_common import ids_of
from test_gpu_policy_grad import backward

pytestmark = pytest.mark.gpu

BAR = 1.0 + 2.0 ** -20
SIZES = (1, 17, 64, 65, 130)      # one env; a tile and one; a full wave; a wave and one; three waves, the last ragged
START = {INITIAL: "initial", CURRENT: "current"}


class Windows:
    """One recording per (n, T), flown once to give the Trajectory its length; a case's observations and done codes are written over
    it (the padding columns of the observations stay NaN)."""

    def __init__(self, device, oracle):
        self.device, self.oracle, self._made = device, oracle, {}

    def traj(self, n, T):
        if (n, T) not in self._made:
            w = World(self.device, self.oracle, n, seed=900 + n, episode_step_limit=9)
            traj = w.vector.Trajectory(w.env, T)
            w.policy.reset()
            w.vector.rollout(self.device, w.env, w.params, w.state, w.policy, w.rng, T, "fused", autoreset=True, trajectory=traj)
            self._made[(n, T)] = (w, traj)
        return self._made[(n, T)][1]

    def write(self, n, T, obs, done):
        """obs [T, n, 22], done [T, n] -> the recording holding them"""
        import torch
        traj = self.traj(n, T)
        t = traj.tensors()
        o = np.full(tuple(t["obs"].shape), np.nan, np.float32)
        o[:, :, :n] = obs.transpose(0, 2, 1)
        d = np.zeros(tuple(t["done"].shape), np.uint8)
        d[:, :n] = done
        t["obs"].copy_(torch.tensor(o, device=t["obs"].device))
        t["done"].copy_(torch.tensor(d, device=t["done"].device))
        torch.cuda.synchronize()        # the engine's stream does not order itself against torch's
        return traj


@pytest.fixture(scope="module")
def windows(device, oracle):
    return Windows(device, oracle)


def _policy(device, w):
    from raptor_amd.foundation_policy import Raptor
    pol = Raptor(device, weights=w)
    pol.reset()
    return pol


def _padded(a, ld, fill=np.nan):
    """[T, n, 4] -> [T, 4, ld] float32 with ``fill`` in the padding columns"""
    T, n = a.shape[:2]
    out = np.full((T, 4, ld), fill, np.float32)
    out[:, :, :n] = a.transpose(0, 2, 1)
    return out


def _gradient(traj, pol, c, start, dact=None):
    """forward + unseeded backward from ``start`` -> (g, gh [n, 16] or None, act [T, 4, ld])"""
    n = c["done"].shape[1]
    pol.reset()
    if start == CURRENT:
        pol.set_hidden_state(c["h"])
    act = forward(traj, pol, start)
    g, gh = backward(traj, pol, _padded(c["dact"], _ld(traj)) if dact is None else dact, want_h=start == CURRENT)
    if start == CURRENT:
        assert np.isfinite(gh).all() and not gh[:, n:].any()               # exact zeros beyond n
        gh = np.ascontiguousarray(gh[:, :n].T)
    return g, gh, act


def _held(g, gh, c, start, label, dact=None):
    """the window bound on one gradient -> the largest error / bound"""
    n = c["done"].shape[1]
    ref, ref_h, b, bh = PW.window_bound(c["w"], c["obs"], c["done"], c["dact"] if dact is None else dact, START[start],
                                        c["h"] if start == CURRENT else None, (n + 63) // 64)
    assert np.isfinite(g).all() and np.isfinite(b).all(), label
    r = AR.ratio(g, ref, b)
    worst = float(r.max())
    assert worst <= BAR, (label, worst, int(np.argmax(r)))
    if start == CURRENT:
        rh = AR.ratio(gh, ref_h, bh)
        assert rh.max() <= BAR, (label, "gh", float(rh.max()))
        worst = max(worst, float(rh.max()))
    return worst


# ------------------------------------------------------------------------------ 1. the unseeded gradient -
@pytest.mark.parametrize("wf", AR.WEIGHT_FAMILIES)
def test_unseeded_gradient_lies_inside_the_window_bound(device, windows, wf):
    per_family = {}
    for n in SIZES:
        pol = _policy(device, AR.weights(wf))
        for xf in AR.INPUT_FAMILIES:
            for T in (1, 3):
                c = PW.case(wf, xf, n, T)
                traj = windows.write(n, T, c["obs"], c["done"])
                for start in (INITIAL, CURRENT):
                    g, gh, _ = _gradient(traj, pol, c, start)
                    r = _held(g, gh, c, start, (wf, xf, n, T, START[start]))
                    per_family[xf] = max(per_family.get(xf, 0.0), r)
    print(f"[grad float64] unseeded {wf}: max err / bound {max(per_family.values()):.3f}  (" +
          ", ".join(f"{k} {v:.3f}" for k, v in per_family.items()) + ")")


def test_the_bound_rejects_the_gradient_of_exchanged_gate_rows(device, windows):
    """the test can fail: the GPU's gradient against the reference of weights whose r and z rows are exchanged"""
    n, T = 65, 3
    c = PW.case("fresh", "normal", n, T)
    traj = windows.write(n, T, c["obs"], c["done"])
    pol = _policy(device, c["w"])
    for start in (INITIAL, CURRENT):
        g, gh, _ = _gradient(traj, pol, c, start)
        wrong, _, b, _ = PW.window_bound(AR.altered(c["w"], "rows_rz_exchanged"), c["obs"], c["done"], c["dact"], START[start],
                                         c["h"] if start == CURRENT else None, 2)
        r = AR.ratio(g, wrong, b)
        print(f"[grad float64] exchanged rows, {START[start]}: {int((r > BAR).sum())} of 2084 entries outside, the farthest by {r.max():.3g} x")
        assert (r > BAR).sum() > 1000


# ------------------------------------------------------------------------------ 2. the seeded gradient -
def _seeded_case(wf, xf, n, T, act, start):
    """labels for the window: N(0, 1); the device's own action on the envs quieted for a kink (their seed a - y is then an exact
    0, as the unseeded tests' dact); NaN on frozen steps and in the padding -> (y [T, 4, ld], live [T, 4, n], gact [T, 4, ld])"""
    c = PW.case(wf, xf, n, T)
    ld = act.shape[2]
    y = np.full((T, 4, ld), np.nan, np.float32)
    y[:, :, :n] = np.random.default_rng([7, n, T]).standard_normal((T, 4, n)).astype(np.float32)
    y[:, :, :n][:, :, c["quieted"]] = act[:, :, :n][:, :, c["quieted"]]
    live = np.broadcast_to((c["done"] != 4)[:, None, :], (T, 4, n))
    gact = np.full((T, 4, ld), np.nan, np.float32)
    gact[:, :, :n] = np.where(live, (act[:, :, :n] - y[:, :, :n]).astype(np.float32), np.float32(0))
    y[:, :, :n][~live] = np.nan
    return c, y, live, gact


@pytest.mark.parametrize("wf", ["fresh", "sat8", "sat64", "signed_pos"])
def test_seeded_gradient_is_the_unseeded_one_scaled_once_bit_for_bit(device, windows, wf):
    """k_policy_loss_backward is k_policy_grad_backward's text with dL/da = a - y formed in the kernel, and both reductions add the
    waves in ascending order; k_policy_loss_reduce then applies 2 / M once, the product in float64 (rq_loss_reduce.inc:93).  So the
    seeded gradient is float32(float64(unseeded gradient of gact = fl(a - y)) * (2.0 * (1.0 / M))), and that unseeded gradient lies
    inside the window bound."""
    T, worst, worst_loss = 3, 0.0, 0.0
    for n in (17, 65, 130):
        pol = _policy(device, AR.weights(wf))
        for xf in ("normal", "large"):
            for start in (INITIAL, CURRENT):
                c0 = PW.case(wf, xf, n, T)
                traj = windows.write(n, T, c0["obs"], c0["done"])
                pol.reset()
                if start == CURRENT:
                    pol.set_hidden_state(c0["h"])
                act = forward(traj, pol, start)
                c, y, live, gact = _seeded_case(wf, xf, n, T, act, start)
                label = (wf, xf, n, START[start])
                loss, g = loss_grad(traj, pol, y, start=start)
                M = int(live.sum())
                ref_loss, _, terms = D.masked_mse(act[:, :, :n], y[:, :, :n], live)
                lb = D.loss_bound(terms, M)
                assert np.isfinite(loss) and abs(loss - ref_loss) <= lb, (label, loss, ref_loss, lb)
                worst_loss = max(worst_loss, abs(loss - ref_loss) / lb)
                g_un, gh, _ = _gradient(traj, pol, c, start, dact=gact)
                want = (g_un.astype(np.float64) * (2.0 * (1.0 / M))).astype(np.float32)
                assert same(g, want) and g.any(), (label, int((g.view(np.uint32) != want.view(np.uint32)).sum()))
                worst = max(worst, _held(g_un, gh, c, start, label, dact=gact[:, :, :n].transpose(0, 2, 1)))
    print(f"[grad float64] seeded {wf}: the unseeded bits x 2 / M in every case; its seed's gradient max err / bound {worst:.3f}, "
          f"loss max err / bound {worst_loss:.3f}")


# ------------------------------------------------------------------------------ 3. bank and weighted variants -
@pytest.mark.parametrize("wf", ["fresh", "sat8"])
def test_bank_and_weighted_variants_give_the_single_policys_bits(device, windows, wf):
    """what tests/test_gpu_bank_distill.py and tests/test_gpu_weighted_distill.py assert on perturbed weights: a bank's policy gets
    the bits of the single-policy call on its own blocks, and a weight of 1.0f the unweighted bits"""
    from raptor_amd.policy_bank import PolicyBank
    from test_gpu_bank_distill import bank_loss_grad
    from test_gpu_weighted_distill import wbank_loss_grad, wloss_grad
    n, T = 130, 3
    blocks = [1, 0, 1]                                       # policy 1 owns the first block and the ragged last one
    ids = ids_of(blocks, n)
    W = np.stack([AR.weights(wf, seed=p) for p in range(2)])
    assert not np.array_equal(W[0], W[1])
    c = PW.case(wf, "normal", n, T)
    ld = _ld(windows.traj(n, T))
    y = np.full((T, 4, ld), np.nan, np.float32)
    y[:, :, :n] = np.random.default_rng(11).standard_normal((T, 4, n)).astype(np.float32)
    singles = []
    for p in range(2):                                       # a recording that holds p's columns alone, in order
        cols = np.flatnonzero(ids == p)
        sub = windows.write(len(cols), T, c["obs"][:, cols], c["done"][:, cols])
        ys = np.full((T, 4, _ld(sub)), np.nan, np.float32)
        ys[:, :, :len(cols)] = y[:, :, cols]
        pol = _policy(device, W[p])
        l0, g0 = loss_grad(sub, pol, ys)
        ones = np.ones((1, len(cols)), np.float32)
        l1, g1 = wloss_grad(device, sub, pol, ys, ones)
        assert same(l1, l0) and same(g1, g0) and g0.any() and np.isfinite(g0).all() and np.isfinite(l0), (wf, p)
        singles.append((l0, g0))
    assert not same(singles[0][1], singles[1][1])
    traj = windows.write(n, T, c["obs"], c["done"])
    bank = PolicyBank(device, W)
    lb, gb = bank_loss_grad(traj, bank, ids, y)
    ones = np.ones((T, n), np.float32)
    lw, gw = wbank_loss_grad(device, traj, bank, ids, y, ones)
    for p in range(2):
        assert same(lb[p], singles[p][0]) and same(gb[p], singles[p][1]), (wf, p)
        assert same(lw[p], lb[p]) and same(gw[p], gb[p]), (wf, p)


# ------------------------------------------------------------------------------ 4. the gain table -
@pytest.mark.parametrize("wf", AR.WEIGHT_FAMILIES)
def test_gain_table_lies_inside_its_float64_bound(device, windows, wf):
    from test_gpu_gain_table import held_to_float64, table
    edges = np.asarray([0, 2 ** 32 - 1], np.uint32)
    per_family = {}
    for n in (1, 65, 130):
        pol = _policy(device, AR.weights(wf))
        for xf in AR.INPUT_FAMILIES:
            c = PW.case(wf, xf, n, 1)
            traj = windows.write(n, 1, c["obs"], c["done"])
            pol.reset()
            pol.set_hidden_state(c["h"])
            total, count = table(traj, pol, edges, CURRENT)
            assert int(count.sum()) == int((c["done"] != 4).sum())
            r = held_to_float64(total, count, c["w"], c["obs"], c["h"][None], c["done"], edges, f"{wf} {xf} n={n}")
            per_family[xf] = max(per_family.get(xf, 0.0), r)
            assert np.array_equal(pol.hidden_state(n), c["h"])
    print(f"[grad float64] gain table {wf}: max err / bound {max(per_family.values()):.3f}  (" +
          ", ".join(f"{k} {v:.3f}" for k, v in per_family.items()) + ")")
