"""The learner's window bound without a GPU (tests/policy_grad_window.py): proved on a NumPy float32 emulation of the backward
kernel for every weight family x input family x T in {1, 3} x both starts, shown to reject seven deliberate mistakes and two wrong
episode rules, and the share of envs it has to leave out near a ReLU kink capped for every case the GPU suite
(tests/test_gpu_policy_grad_float64.py) uses.  ``pytest -s`` prints how tight the bound is per weight block.

The fp32 model of ``actor_reference`` never declares a forward bound infinite (only the f16x2 build has a range), so no cell is
skipped: every bound must be finite."""
import numpy as np
import pytest

import actor_reference as AR
import policy_grad_reference as R
import policy_grad_window as PW

N = 65                                     # a wave and one env: two partials, a ragged tile
GPU_SIZES = (1, 17, 64, 65, 130)           # tests/test_gpu_policy_grad_float64.py


def _run(c, T, start, alter=None):
    h = c["h"] if start == "current" else None
    return PW.emulate_backward(c["w"], c["obs"][:T], c["done"][:T], c["dact"][:T], start, h, alter=alter)


def _bound(c, T, start):
    n = c["done"].shape[1]
    return PW.window_bound(c["w"], c["obs"][:T], c["done"][:T], c["dact"][:T], start, c["h"] if start == "current" else None,
                           (n + 63) // 64)


@pytest.mark.parametrize("xf", AR.INPUT_FAMILIES)
@pytest.mark.parametrize("wf", AR.WEIGHT_FAMILIES)
def test_the_float32_emulation_lies_inside_the_window_bound(wf, xf):
    for T in (1, 3):
        c = PW.case(wf, xf, N, T)
        assert {0, 1, 2, 4} <= set(c["done"][0, :16].tolist())            # every code inside one 16-env tile
        assert c["quieted"].mean() <= PW.MAX_QUIETED, (wf, xf, T, c["quieted"].mean())
        for start in ("initial", "current"):
            g, gh, b, bh = _bound(c, T, start)
            got, got_h = _run(c, T, start)
            label = (wf, xf, T, start)
            assert np.isfinite(b).all() and (b > 0).all() and np.isfinite(got).all(), label
            # consistency: the gradient is policy_grad_reference's, exactly
            _, cache = R.forward(c["w"].astype(np.float64), c["obs"][:T], c["done"][:T], start, c["h"] if start == "current" else None)
            g_ref, gh_ref = R.backward(cache, c["dact"][:T])
            assert np.array_equal(g, g_ref), label
            r = AR.ratio(got, g, b)
            assert r.max() <= 1.0, (label, float(r.max()), int(np.argmax(r)))
            if start == "current":
                assert np.array_equal(gh, gh_ref) and np.isfinite(bh).all(), label
                rh = AR.ratio(got_h, gh, bh)
                assert rh.max() <= 1.0, (label, float(rh.max()))
                assert not got_h[c["quieted"]].any() and not gh[c["quieted"]].any(), label
            else:
                assert gh is None and bh is None and got_h is None
            assert wf == "tiny" or np.abs(g).max() > 0


@pytest.mark.parametrize("wf", AR.WEIGHT_FAMILIES)
def test_few_envs_are_quieted_for_a_kink_in_every_case_the_gpu_suite_uses(wf):
    worst = 0.0
    for xf in AR.INPUT_FAMILIES:
        for n in GPU_SIZES:
            for T in (1, 3):
                q = PW.case(wf, xf, n, T)["quieted"]
                assert q.mean() <= PW.MAX_QUIETED, (wf, xf, n, T, int(q.sum()))
                if n <= 17:
                    assert not q.any(), (wf, xf, n, T)
                worst = max(worst, float(q.mean()))
    print(f"[window bound] {wf}: at most {100 * worst:.2f} % of a case's envs quieted for a ReLU kink")


@pytest.mark.parametrize("wf", ["fresh", "perturbed", "sat8"])
def test_every_alteration_and_both_wrong_episode_rules_leave_the_bound(wf):
    T = 3
    c = PW.case(wf, "normal", N, T)
    for start in ("initial", "current"):
        g, gh, b, bh = _bound(c, T, start)
        for alter in PW.ALTERATIONS:
            got, _ = _run(c, T, start, alter=alter)
            r = AR.ratio(got, g, b)
            assert r.max() > 1.0, (wf, start, alter, float(r.max()))
            print(f"[window bound] {wf} {start} {alter}: {int((r > 1).sum())} of 2084 entries outside, the farthest by {r.max():.3g} x")
        # the float64 gradient under slightly wrong episode rules (tests/test_policy_grad_reference.py)
        done = c["done"][:T]
        for wrong in (np.where(done == 4, 0, done), np.where((done == 1) | (done == 2), 0, done)):
            _, c2 = R.forward(c["w"].astype(np.float64), c["obs"][:T], wrong.astype(np.uint8), start, c["h"] if start == "current" else None)
            g2, _ = R.backward(c2, c["dact"][:T])
            assert (np.abs(g2 - g) > b).any(), (wf, start)
        # r / z rows exchanged in the weights (the GPU suite's own "can fail" case)
        _, c3 = R.forward(AR.altered(c["w"], "rows_rz_exchanged").astype(np.float64), c["obs"][:T], done, start,
                          c["h"] if start == "current" else None)
        g3, _ = R.backward(c3, c["dact"][:T])
        assert (np.abs(g3 - g) > b).any(), (wf, start)


@pytest.mark.parametrize("wf", AR.WEIGHT_FAMILIES)
def test_print_how_tight_the_bound_is_per_weight_block(wf):
    """No number is fixed here: the alterations test is the condition.  bound / max |g| of the block, median and largest entry,
    over the input families at T = 3, start = current."""
    rows = {}
    for xf in AR.INPUT_FAMILIES:
        c = PW.case(wf, xf, N, 3)
        g, _, b, _ = _bound(c, 3, "current")
        for name, (a, z) in AR.BLOCKS.items():
            scale = np.abs(g[a:z]).max()
            if scale > 0:
                rel = b[a:z] / scale
                rows.setdefault(name, []).append((float(np.median(rel)), float(rel.max())))
    print(f"[window bound] {wf}: bound / max |g| per block, median | largest over the input families: " +
          ", ".join(f"{k} {max(m for m, _ in v):.2g} | {max(x for _, x in v):.2g}" for k, v in rows.items()))
    assert rows or wf == "tiny"


def test_the_emulation_is_the_float64_gradient_to_rounding_and_its_zeros_are_exact():
    """the emulation computes the right thing (so that the soundness test is about rounding), quieted envs and padding contribute
    exact zeros, and an all-zero dact gives an all-zero gradient"""
    c = PW.case("fresh", "normal", N, 3)
    g, gh, _, _ = _bound(c, 3, "current")
    got, got_h = _run(c, 3, "current")
    assert np.abs(got - g).max() <= 1e-5 * np.abs(g).max() and np.abs(got_h - gh).max() <= 1e-5 * np.abs(gh).max()
    z = dict(c, dact=np.zeros_like(c["dact"]))
    got, got_h = _run(z, 3, "current")
    assert not got.any() and not got_h.any()
