"""The Adam bound of tests/adam_reference.py, tested without a GPU: the emulation of k_adam_repack as it is lies inside the bound
on the whole design x grid x step counts, every deliberately wrong kernel leaves it, and the reference is tied to
tests/distill_reference.Adam (which tests/test_distill_reference.py ties to torch).

Measured here (``pytest tests/test_adam_bound_cpu.py -s``), all 42 (row, step) cases, 2 084 elements each.
  The correct emulation, largest |got - ref| / bound:  w' 0.9992   m' 0.9968   v' 0.9903   (one rounding to fp32 uses the bound up).
  Each mistake: its largest ratio per output over the cases, and the cases (of 42) and grid rows in which it leaves the bound:
    round_moments        w' 8.8e+08  m' 0.997    v' 0.99      36 cases, rows 0 1 2 3 5 6   (not lr = 0: the moments themselves are right)
    l2_decay             w' 1.1e+14  m' 4.0e+36  v' 1.9e+34   18 cases, rows 1 4 5         (the rows with weight_decay > 0)
    decay_after          w' 6.0e+13  m' 0.997    v' 0.99      12 cases, rows 1 5           (weight_decay > 0 and lr > 0)
    eps_in_sqrt          w' 2.6e+13  m' 0.997    v' 0.99      30 cases, rows 0 1 2 3 5     (not lr = 0, not eps = 0)
    no_bias_correction   w' 3.2e+14  m' 0.997    v' 0.99      29 cases, rows 0 1 2 3 5 6   (not lr = 0; not where both powers are 0)
    previous_power       w' inf      m' 0.997    v' 0.99      30 cases, every row          (step 0: 1 - beta^0 = 0)
    all_fp32             w' 9.8e+08  m' 301      v' 218       42 cases, every row
    abs_g                w' 2.8e+21  m' 0.997    v' inf       42 cases, every row
    beta2_for_both       w' 1.7e+16  m' 2.2e+37  v' 0.99      42 cases, every row
  No mistake is undetectable: each leaves the bound on at least one row, and all_fp32 leaves it on m' and v' as well as on w'.
No constant of the bound was set from these figures."""
import numpy as np
import pytest

import adam_reference as A
import distill_reference as D

CASES = [(r, s) for r in range(len(A.GRID)) for s in A.STEPS]


def _case(row, step):
    cfg = A.GRID[row]
    powers = A.powers_of(cfg, step)
    return cfg, powers, A.check_design(cfg, powers)


def _ratios(cfg, powers, inputs, mistake=None):
    """-> (largest ratio of w', m', v'; inf where a class differs)"""
    ref = A.adam_exact(*inputs, cfg, powers)
    b = A.bound(*inputs, cfg, powers)
    got = A.emulate(*inputs, cfg, powers, mistake)
    return [float(np.max(A.agrees(got[k], ref[k], b[k])[1])) for k in range(3)]


def test_the_design_puts_every_family_into_every_trip():
    assert np.gcd(A.PERIOD, 1024) == 1 and len(set(A.FAMILIES.values())) == len(A.FAMILIES) and max(A.FAMILIES.values()) < A.PERIOD
    for row, step in CASES:
        _case(row, step)                     # check_design asserts
    # the isolated elements are ordinary ones, and every element belongs to exactly one family
    counts = np.zeros(A.NW, int)
    for name in [*A.FAMILIES, "ordinary"]:
        counts[A.family_index(name)] += 1
    special = [*A.NAN_AT, *(i for i, _ in A.INF_AT)]
    assert (np.delete(counts, special) == 1).all() and (counts[special] == 0).all()


def test_the_kernel_as_it_is_lies_inside_the_bound():
    worst = np.zeros(3)
    for row, step in CASES:
        cfg, powers, inputs = _case(row, step)
        r = _ratios(cfg, powers, inputs)
        assert max(r) <= 1.0, (row, step, r)
        worst = np.maximum(worst, r)
    print(f"correct emulation, largest |got - ref| / bound: w' {worst[0]:.4f}  m' {worst[1]:.4f}  v' {worst[2]:.4f}")
    assert (worst > 0.5).all()               # the bound is one rounding, and a rounding uses it


def test_eps_zero_on_a_zero_gradient_with_zero_moments_is_nan_as_in_torch():
    """rq_adam_config.eps = 0 is accepted; with v' = 0 the update is 0 / 0.  The reference, the emulation and torch agree."""
    import torch
    cfg = A.GRID[6]
    assert cfg[3] == 0.0
    powers, idx = A.powers_of(cfg, 0), A.family_index("g0_mv0")
    w, m, v, g = (a[idx] for a in A.design(cfg, powers))
    x = A.adam_exact(w, m, v, g, cfg, powers)[0]
    assert np.isnan(x).all() and np.isnan(A.emulate(w, m, v, g, cfg, powers)[0]).all()
    wt = torch.tensor(w.astype(np.float64), requires_grad=True)
    opt = torch.optim.Adam([wt], lr=cfg[0], betas=(cfg[1], cfg[2]), eps=0.0)
    wt.grad = torch.zeros_like(wt)
    opt.step()
    assert torch.isnan(wt.detach()).all()


@pytest.mark.parametrize("mistake", A.MISTAKES)
def test_every_mistake_leaves_the_bound(mistake):
    out, worst = 0, np.zeros(3)
    rows = set()
    for row, step in CASES:
        cfg, powers, inputs = _case(row, step)
        r = np.array(_ratios(cfg, powers, inputs, mistake))
        worst = np.maximum(worst, r)
        if r.max() > 1.0:
            out += 1
            rows.add(row)
    print(f"{mistake:20s} largest ratio w' {worst[0]:.3g}  m' {worst[1]:.3g}  v' {worst[2]:.3g}; outside in {out} of {len(CASES)} cases, rows {sorted(rows)}")
    assert out >= 1, mistake
    if mistake == "all_fp32":                # wherever the update is far below u |w| it cannot show in w'; in the moments it must
        assert worst[1] > 1.0 and worst[2] > 1.0


def test_the_reference_iterated_without_rounding_is_the_torch_tied_adam():
    """``update64`` iterated on float64 state equals distill_reference.Adam over 20 steps.  The two differ in the powers alone - a
    running product against beta ** t, at most t roundings apart - which enter through 1 - beta^t, amplified by at most
    beta^t / (1 - beta^t) <= 1000 (beta2 at t = 1).  Per step that is within the bound's own count for w' (c_w <= 1100 on this
    row); a difference carried in m, v or w is passed on at most once per later step, so over 20 steps
    |w - w_ref| <= 20^2 * 2 * 1100 e (|w| + |U|), U <= lr * 10 (an update is at most a few lr)."""
    cfg = A.GRID[1]
    lr, b1, b2, eps, wd = cfg
    rng = np.random.default_rng(5)
    w = rng.standard_normal(A.NW)
    ref = D.Adam(w, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    m, v, powers = np.zeros(A.NW), np.zeros(A.NW), np.ones(2)
    for k in range(20):
        g = rng.standard_normal(A.NW) * 10.0 ** rng.integers(-6, 2)
        w, m, v, powers, _ = A.update64(w, m, v, g, cfg, powers)
        r = ref.step(g)
        tol = 20 ** 2 * 2 * 1100 * A.E * (np.abs(r) + 10 * lr)
        assert (np.abs(w - r) <= tol).all(), (k, np.max(np.abs(w - r) / tol))
        assert abs(powers[0] - b1 ** (k + 1)) <= (k + 1) * 2.0 ** -52 * b1 ** (k + 1)
