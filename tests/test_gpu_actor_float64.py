"""The student actor held to float64 beyond the shipped checkpoint: ONE teacher-forced policy step of ``evaluate_step`` and
``evaluate_sequence`` inside the element-wise bound of tests/actor_reference.py (proved on the CPU in
tests/test_actor_reference.py) for every weight family x input family x precision, and every other actor kernel tied to those
two bit for bit on the new weights.  No recurrence-long comparison: a step is forced from a hidden state the test sets, so no
error is amplified.

Largest |got - ref| / bound of ``evaluate_step`` on an MI355X, per precision x weight family (``pytest -s`` prints them, per
input family too); no constant of the model was changed after the first GPU run:

            shipped perturbed fresh  sat8   sat64  tiny   signed_pos signed_neg
    fp32    0.265   0.368     0.394  0.865  0.801  0.234  0.928      0.386
    bf16    1.000   1.000     0.904  1.000  1.000  0.814  0.965      0.932
    f16x2   0.263   0.363     0.370  0.860  0.793  0.710  0.928      0.383

bf16's 1.000 is the ``large`` inputs (observations x 2^10): the bound on a gate's argument then spans the gate's whole range
and a value at the rail sits exactly on it; without them bf16 peaks at 0.901.  ``evaluate_sequence`` peaks at 0.488 (fp32,
f16x2) and 0.728 (bf16), Standardize + squash at 0.302 / 0.408 / 0.301.
"""
import numpy as np
import pytest

import actor_reference as AR
from rollout_common import Batch, assert_same, assert_same_recording, random_table, snapshot

pytestmark = pytest.mark.gpu

BAR = 1.0 + 2.0 ** -20
BATCHES = (1, 16, 17, 63, 64, 65, 1000, 1100)     # the wave tail, the resident policy's 16 rows, the mailbox's 1024
GPU_PRECISIONS = ("fp32", "bf16", "f16x2")
LINK_FAMILIES = ("perturbed", "fresh", "sat8")


def _policy(device, w, precision, **kw):
    from raptor_amd.foundation_policy import Raptor
    return Raptor(device, weights=w, precision=precision, **kw)


def _forced_step(pol, x, h):
    """evaluate_step from the hidden state h: -> (action, new state)"""
    pol.reset()
    pol.evaluate_step(x[:, :22])                   # sizes the policy
    pol.set_hidden_state(h)
    act = pol.evaluate_step(x[:, :22])             # (rows of 26: a strided view, columns >= 22 never read)
    return act, pol.hidden_state(len(x))


def _inside(act, hid, ref, label):
    """both finite and inside bound x (1 + 2^-20) element by element -> the largest err / bound"""
    ra, rh, ba, bh = ref
    assert np.isfinite(act).all() and np.isfinite(hid).all(), label
    assert np.isfinite(ba).all() and np.isfinite(bh).all(), label
    qa, qh = AR.ratio(act, ra, ba), AR.ratio(hid, rh, bh)
    worst = float(max(qa.max(), qh.max()))
    assert worst <= BAR, (label, worst, np.argwhere(qa > BAR)[:3].tolist(), np.argwhere(qh > BAR)[:3].tolist())
    return worst


@pytest.mark.parametrize("wf", AR.WEIGHT_FAMILIES)
@pytest.mark.parametrize("precision", GPU_PRECISIONS)
def test_one_teacher_forced_step_lies_inside_the_float64_bound(device, precision, wf):
    w = AR.weights(wf)
    pol = _policy(device, w, precision)
    worst, per_family = 0.0, {}
    for xf in AR.INPUT_FAMILIES:
        for n in BATCHES:
            x, h = AR.inputs(xf, n)
            act, hid = _forced_step(pol, x, h)
            r = _inside(act, hid, AR.step_bound(w, x, h, precision), (precision, wf, xf, n))
            worst, per_family[xf] = max(worst, r), max(per_family.get(xf, 0.0), r)
    # k_actor_step_rate: call 0 of an interval of 3 commits the state, call 1 acts from it and leaves it
    rated = _policy(device, w, precision, native_interval=3)
    for n in (17, 1100):
        x, h = AR.inputs("normal", n, seed=1)
        ref = AR.step_bound(w, x, h, precision)
        rated.reset()
        rated.evaluate_step(x)
        rated.set_hidden_state(h)
        rated.native_interval = 3                  # the call counter starts again: the next call is native
        act0 = rated.evaluate_step(x)
        worst = max(worst, _inside(act0, rated.hidden_state(n), ref, (precision, wf, "rate call 0", n)))
        rated.set_hidden_state(h)
        act1 = rated.evaluate_step(x)              # call 1: the same step, not committed
        assert np.array_equal(act1.view(np.uint32), act0.view(np.uint32))
        assert np.array_equal(rated.hidden_state(n).view(np.uint32), h.view(np.uint32)), (precision, wf, "rate call 1", n)
    # (observations x 2^10 in bf16: the bound on a gate's argument spans the gate's whole range, a value at the rail is 1.000)
    print(f"[actor float64] evaluate_step {precision} {wf}: max err / bound {worst:.3f}  (" +
          ", ".join(f"{k} {v:.3f}" for k, v in per_family.items()) + ")")


def _sequence_case(device, w, precision, n, on_device, seed=0):
    """T = 2 from a set state: step 1 against the reference forced with h, step 2 against the one forced with the kernel's own
    state after step 1 (what a T = 1 call leaves) -> the largest err / bound"""
    import torch
    pol = _policy(device, w, precision)
    x0, h = AR.inputs("normal", n, seed=seed)
    x1, _ = AR.inputs("wide_h", n, seed=seed + 1)
    X = np.stack([x0, x1])
    arg = (lambda a: torch.from_numpy(a).to("cuda:0")) if on_device else (lambda a: a)
    out = (lambda a: a.cpu().numpy()) if on_device else (lambda a: a)
    pol.reset()
    pol.set_hidden_state(h)
    a1 = out(pol.evaluate_sequence(arg(X[:1])))[0]
    h1 = pol.hidden_state(n)
    pol.set_hidden_state(h)
    A = out(pol.evaluate_sequence(arg(X)))
    h2 = pol.hidden_state(n)
    assert np.array_equal(A[0].view(np.uint32), a1.view(np.uint32))
    worst = _inside(a1, h1, AR.step_bound(w, x0, h, precision), (precision, n, "sequence step 1"))
    return max(worst, _inside(A[1], h2, AR.step_bound(w, x1, h1, precision), (precision, n, "sequence step 2")))


@pytest.mark.parametrize("wf", AR.WEIGHT_FAMILIES)
@pytest.mark.parametrize("precision", GPU_PRECISIONS)
def test_evaluate_sequence_lies_inside_the_float64_bound(device, precision, wf):
    w = AR.weights(wf)
    worst = max(_sequence_case(device, w, precision, 65, on_device=False), _sequence_case(device, w, precision, 1000, on_device=True))
    print(f"[actor float64] evaluate_sequence {precision} {wf}: max err / bound {worst:.3f}")


def test_evaluate_sequence_two_waves_per_simd_lies_inside_the_float64_bound(device):
    """70 001 rows: the fp32 sequence kernel's 256-register build (two waves per SIMD)"""
    worst = _sequence_case(device, AR.weights("fresh"), "fp32", 70001, on_device=True, seed=5)
    print(f"[actor float64] evaluate_sequence fp32 fresh 70001 rows: max err / bound {worst:.3f}")


@pytest.mark.parametrize("precision", GPU_PRECISIONS)
def test_standardize_and_squash_lie_inside_the_float64_bound(device, precision):
    """Standardize folded into layer 0 on the host and tanh on the action ("mean"): the fold's roundings enter the bound
    through ``fold_bound``, the tanh costs tau."""
    w = AR.weights("fresh")
    rng = np.random.default_rng(17)
    mean = rng.standard_normal(22).astype(np.float32)
    std = rng.uniform(0.5, 2.0, 22).astype(np.float32)
    pol = _policy(device, w, precision)
    pol.set_standardize(mean, std)
    pol.set_squash(True)
    worst = 0.0
    for xf, n in (("normal", 65), ("large", 130), ("small", 1000)):
        x, h = AR.inputs(xf, n, seed=2)
        act, hid = _forced_step(pol, x, h)
        xs, e_z0 = AR.fold_bound(w, mean, std, x, precision)
        worst = max(worst, _inside(act, hid, AR.step_bound(w, xs, h, precision, e_z0=e_z0, squash=True), (precision, xf, n)))
        assert np.abs(act).max() <= 1.0
    print(f"[actor float64] standardize + squash {precision} fresh: max err / bound {worst:.3f}")


@pytest.mark.parametrize("precision", GPU_PRECISIONS)
def test_a_reference_of_exchanged_gate_rows_lies_outside_the_bound(device, precision):
    """The test can fail: the kernel against the float64 reference of weights whose r and z rows are exchanged."""
    w = AR.weights("fresh")
    x, h = AR.inputs("normal", 65)
    act, hid = _forced_step(_policy(device, w, precision), x, h)
    _inside(act, hid, AR.step_bound(w, x, h, precision), (precision, "true weights"))
    ra, rh, ba, bh = AR.step_bound(AR.altered(w, "rows_rz_exchanged"), x, h, precision)
    worst = float(max(AR.ratio(act, ra, ba).max(), AR.ratio(hid, rh, bh).max()))
    print(f"[actor float64] {precision} against exchanged r / z rows: max err / bound {worst:.3g}")
    assert worst > BAR


# ------------------------------------------------------------------------------ bit-for-bit links ---
def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("wf", LINK_FAMILIES)
@pytest.mark.parametrize("precision", GPU_PRECISIONS)
def test_every_other_actor_kernel_equals_the_step_bit_for_bit(device, precision, wf, n):
    """evaluate_sequence == T x evaluate_step; a recording's relabel == evaluate_sequence of its observations == its actions;
    fused == chained with recording and auto-reset at episode_step_limit = 5, also at a native interval of 3 and on a moving
    setpoint."""
    import raptor_amd.l2f as l2f
    T = 12
    w = AR.weights(wf)
    X = np.random.default_rng(n).standard_normal((T, n, 22)).astype(np.float32)
    p, q = _policy(device, w, precision), _policy(device, w, precision)
    p.reset(); q.reset()
    seq = p.evaluate_sequence(X)
    steps = np.stack([q.evaluate_step(X[t]) for t in range(T)])
    assert np.array_equal(_u32(seq), _u32(steps)) and np.array_equal(_u32(p.hidden_state(n)), _u32(q.hidden_state(n)))
    # a recording without an episode end: its actions are evaluate_sequence of its observations, and its relabel
    b = Batch(device, n, limit=40)
    cfg = b.env.config
    cfg.termination_enabled = 0
    b.env.config = cfg
    pol = _policy(device, w, precision)
    pol.reset()
    rec = b.fly(pol, T, "fused", True, record=True)
    assert not rec["done"].any()
    fresh = _policy(device, w, precision)
    fresh.reset()
    assert np.array_equal(_u32(fresh.evaluate_sequence(rec["obs"])), _u32(rec["act"]))
    assert np.array_equal(_u32(fresh.hidden_state(n)), _u32(pol.hidden_state(n)))
    # fused == chained, episodes ending every 5 steps; relabel reproduces the recording across the resets
    for kw in (dict(), dict(interval=3), dict(ref=True)):
        runs = []
        for mode in ("fused", "chained"):
            bb = Batch(device, n, limit=5)
            pp = _policy(device, w, precision, native_interval=kw.get("interval", 1))
            pp.reset()
            ref = l2f.Reference(device, random_table(5, seed=4)) if kw.get("ref") else None
            tr = bb.vector.Trajectory(bb.env, T)
            bb.vector.rollout(device, bb.env, bb.params, bb.state, pp, bb.rng, T, mode, True, trajectory=tr, reference=ref)
            runs.append((snapshot(bb, pp.hidden_state(n)), tr.numpy(), tr))
        assert_same(runs[0][0], runs[1][0], what=f"{precision} {wf} {kw}")
        assert_same_recording(runs[0][1], runs[1][1], what=f"{precision} {wf} {kw}")
        assert (runs[0][1]["done"] != 0).any()
        if not kw:
            teacher = _policy(device, w, precision)
            teacher.reset()
            assert np.array_equal(_u32(runs[0][2].relabel(teacher)), _u32(runs[0][1]["act"]))


# ------------------------------------------------------------------------------ the f16x2 range ---
def test_f16x2_refuses_weights_outside_its_range_and_leaves_the_policy_as_it_was(device):
    """A weight whose operand reaches 65 520 after the pre-scale has no hi / lo split (hi = inf, lo = -inf: NaN on the matrix
    pipe).  f16x2 refuses it at creation, at set_weights and at set_precision, names the weight, and the policy then computes
    exactly what it computed before; fp32 and bf16 carry the weight."""
    from raptor_amd import _lib
    w = AR.weights("fresh")
    index = 1136 + 40 * 16 + 3                                  # an n row of W_h: pre-scaled by -2 log2 e
    bad = w.copy()
    bad[index] = np.float32(2.3e4)
    assert abs(float(AR.K_TANH * bad[index])) >= 65520.0 > abs(float(bad[index]))
    x, h = AR.inputs("normal", 65)
    # creation
    with pytest.raises(_lib.RaptorQuadError, match=f"weight {index} ") as e:
        _policy(device, bad, "f16x2").reset()
    assert e.value.status == -1
    # set_precision: refused, the policy stays fp32 and answers the same bits; bf16 is taken
    pol = _policy(device, bad, "fp32")
    before = _forced_step(pol, x, h)
    assert np.isfinite(before[0]).all()
    with pytest.raises(_lib.RaptorQuadError, match=f"weight {index} "):
        pol.set_precision("f16x2")
    assert pol.precision == "fp32"
    after = _forced_step(pol, x, h)
    assert np.array_equal(_u32(before[0]), _u32(after[0])) and np.array_equal(_u32(before[1]), _u32(after[1]))
    pol.set_precision("bf16")
    assert np.isfinite(_forced_step(pol, x, h)[0]).all()
    # set_weights on an f16x2 policy: refused, weights and results stay
    pol = _policy(device, w, "f16x2")
    before = _forced_step(pol, x, h)
    with pytest.raises(_lib.RaptorQuadError, match=f"weight {index} "):
        pol.set_weights(bad)
    assert np.array_equal(pol.weights, w) and pol.precision == "f16x2"
    got = np.empty(2084, np.float32)
    _lib.call("rq_policy_get_weights", pol._handle(), _lib.fptr(got))
    assert np.array_equal(_u32(got), _u32(w))
    after = _forced_step(pol, x, h)
    assert np.array_equal(_u32(before[0]), _u32(after[0])) and np.array_equal(_u32(before[1]), _u32(after[1]))
    _inside(after[0], after[1], AR.step_bound(w, x, h, "f16x2"), "f16x2 after a refused set_weights")
    # just inside the range the weight is held and the step meets the bound
    ok = w.copy()
    ok[index] = np.float32(65000.0 / 2.8853900817779268)
    pol.set_weights(ok)
    act, hid = _forced_step(pol, x, h)
    _inside(act, hid, AR.step_bound(ok, x, h, "f16x2"), "f16x2 at a weight of 65 000 after the pre-scale")
