"""Float64 restatement of ONE Adam update as k_adam_repack makes it (csrc/rq_adam_repack.inc), the bound its three fp32 outputs are
held to, an fp32/float64 NumPy emulation of the kernel with deliberate mistakes selectable by name, and the design input - 2 084
elements of (w, m, v, g) that put every edge family into every trip of the kernel's 1024-thread loop.

The kernel, per element, from the fp32 inputs w, m, v, g and the float64 state (line numbers of rq_adam_repack.inc):
    41   b1t = beta1_t * beta1, b2t = beta2_t * beta2
    45   mm = beta1 * m + (1 - beta1) * g
    46   vv = beta2 * v + (1 - beta2) * g * g
    47   mhat = mm / (1 - b1t), vhat = vv / (1 - b2t)
    49   x = w * (1 - lr * wd) - lr * mhat / (sqrt(vhat) + eps)
    50-53  w' = (float)x, m' = (float)mm, v' = (float)vv           - ONE rounding to fp32 each, of the unrounded float64 values
``adam_exact`` is that text in NumPy float64, operation for operation, so infinities and NaN arise where the kernel's do.

THE BOUND (``bound``), per element, every term derived and none measured.  u = 2^-24, e = 2^-53.
    |got - ref| <= u |ref| (1 + 2^-20) + C e S + 2^-126
  * u |ref|: the one rounding to fp32; (1 + 2^-20) covers |fl(x)| against |x| in that product and the second-order terms.
  * 2^-126: the smallest normal fp32.  Where the rounded value is a denormal its spacing is 2^-149, not u |ref|, and a device that
    flushes denormal results to zero errs by less than 2^-126.  (Measured on the MI355X: the conversion KEEPS denormals -
    tests/test_gpu_adam_float64.py reads m' = 8.999999e-39 back from m = 1e-38, g = 0 - so the term is used as the denormal
    spacing only; it stays as derived.)
  * C e S: the float64 roundings of the expression, counted below from the kernel's lines, against the magnitude S they act on.
    Device and reference each make them (the compiler may contract a multiply-add, which removes roundings, never adds one), so
    the difference of the two is bounded by twice the count: C = 2 c.
    m' (line 45): beta1 m, 1 - beta1, its product with g, the sum: |err| <= e (|beta1 m| + 2 |(1 - beta1) g| + |mm|), which is
        c_m e |ref| with c_m = 4 where the two terms do not cancel; the bound uses the sum itself, S_m, so that it holds where they do.
    v' (line 46): beta2 v, 1 - beta2, two products, the sum; every term is non-negative: c_v = 5, S = |ref|.
    w' (lines 41, 45-49): relative to the update U = lr mhat / (sqrt(vhat) + eps):
        mm             k_m = S_m / |mm|                     (4 without cancellation)
        1 - b1t        k_1 = 1 + b1t / (1 - b1t)            (b1t's rounding, amplified by the subtraction, and the subtraction's)
        mm / (1 - b1t) 1
        sqrt(vhat)+eps (c_v + k_2 + 1) / 2 + 2              (vv, 1 - b2t as k_1, the division: halved by the root; the root, the sum)
        lr *, the division                                  2
      and relative to |w|: lr wd, 1 - lr wd (lr wd <= 1/2 on the grid: no amplification), the product: 3; the final subtraction
      rounds once relative to |x| <= |w| + |U|.  Together |err| <= e (4 |w| + (c_U + 1) |U|) <= c_w e (|w| + |U|) with
        c_w = max(4, k_m + k_1 + 1 + (c_v + k_2 + 1) / 2 + 2 + 2 + 1)   - per element (k_m) and per row and step (k_1, k_2).
      This is the term that matters where w' cancels to near zero: there u |ref| is far below e |w|.
  * Where fp32(ref) is infinite or NaN - ref itself, or a finite float64 value beyond fp32's range - the device must hold the
    same class, and the same sign for an infinity (``agrees``).
"""
import numpy as np

U = 2.0 ** -24
E = 2.0 ** -53
NW = 2084
TINY = 2.0 ** -126

# (lr, beta1, beta2, eps, weight_decay)
GRID = [(3e-3, .9, .999, 1e-8, 0.0), (1e-3, .8, .99, 1e-7, .01), (1e-3, 0.0, .999, 1e-8, 0.0), (1e-3, .9, 0.0, 1e-8, 0.0),
        (0.0, .9, .999, 1e-8, .01), (1.0, .9, .999, 1.0, .5), (1e-3, .9, .999, 0.0, 0.0)]
STEPS = [0, 1, 2, 9, 999, 10 ** 6]          # the step count BEFORE the update

MISTAKES = ["round_moments", "l2_decay", "decay_after", "eps_in_sqrt", "no_bias_correction", "previous_power", "all_fp32", "abs_g",
            "beta2_for_both"]


def powers_of(cfg, step):
    """(beta1^step, beta2^step) as Python floats: what a run of `step` updates carries, to a rounding per update"""
    return np.array([cfg[1] ** step, cfg[2] ** step], np.float64)


def update64(w, m, v, g, cfg, powers):
    """the kernel's expression on float64 arrays as they are -> (w', m', v', new powers, U), nothing rounded to fp32"""
    lr, b1, b2, eps, wd = (np.float64(c) for c in cfg)
    with np.errstate(all="ignore"):
        b1t, b2t = np.float64(powers[0]) * b1, np.float64(powers[1]) * b2
        mm = b1 * m + (1.0 - b1) * g
        vv = b2 * v + (1.0 - b2) * g * g
        mhat, vhat = mm / (1.0 - b1t), vv / (1.0 - b2t)
        upd = lr * mhat / (np.sqrt(vhat) + eps)
        x = w * (1.0 - lr * wd) - upd
    return x, mm, vv, np.array([b1t, b2t]), upd


def adam_exact(w, m, v, g, cfg, powers):
    """One update from fp32 inputs in float64, in the kernel's expression order -> (w', m', v', new powers, U): w', m', v' UNROUNDED
    (w' from the unrounded m', v'), the new powers beta^t, and U = lr mhat / (sqrt(vhat) + eps), the update itself."""
    return update64(*(np.asarray(a, np.float32).astype(np.float64) for a in (w, m, v, g)), cfg, powers)


def emulate(w, m, v, g, cfg, powers, mistake=None):
    """The kernel in NumPy: float64 arithmetic on fp32 inputs, one rounding to fp32 per output -> (w', m', v') float32.
    ``mistake``: None - the kernel as it is - or one of MISTAKES, a kernel that is subtly wrong in that way."""
    assert mistake is None or mistake in MISTAKES, mistake
    T = np.float32 if mistake == "all_fp32" else np.float64
    lr, b1, b2, eps, wd = (T(c) for c in cfg)
    w, m, v, g = (np.asarray(a, np.float32).astype(T) for a in (w, m, v, g))
    one = T(1.0)
    with np.errstate(all="ignore"):
        p1, p2 = T(powers[0]), T(powers[1])
        b1t, b2t = p1 * b1, p2 * b2
        if mistake == "l2_decay":
            g = g + wd * w
        bm = b2 if mistake == "beta2_for_both" else b1
        mm = bm * m + (one - bm) * g
        vv = b2 * v + (one - b2) * (np.abs(g) if mistake == "abs_g" else g * g)
        m_out, v_out = mm.astype(np.float32), vv.astype(np.float32)
        if mistake == "round_moments":
            mm, vv = m_out.astype(T), v_out.astype(T)
        if mistake == "no_bias_correction":
            mhat, vhat = mm, vv
        elif mistake == "previous_power":
            mhat, vhat = mm / (one - p1), vv / (one - p2)
        else:
            mhat, vhat = mm / (one - b1t), vv / (one - b2t)
        den = np.sqrt(vhat + eps) if mistake == "eps_in_sqrt" else np.sqrt(vhat) + eps
        upd = lr * mhat / den
        if mistake == "l2_decay":
            x = w - upd
        elif mistake == "decay_after":
            x = (w - upd) * (one - lr * wd)
        else:
            x = w * (one - lr * wd) - upd
    return x.astype(np.float32), m_out, v_out


def _amplified(power):
    """k of 1 - power: the power's own rounding amplified by the subtraction, and the subtraction's"""
    return 1.0 + abs(power) / abs(1.0 - power) if power != 1.0 else 1.0


def bound(w, m, v, g, cfg, powers):
    """-> (bound of w', of m', of v'), float64 [n] each, for the references ``adam_exact`` returns from the same arguments; the
    module docstring derives every term.  Where a reference is not finite the bound is inf there: ``agrees`` judges those."""
    lr, b1, b2, eps, wd = (np.float64(c) for c in cfg)
    x, mm, vv, new, upd = adam_exact(w, m, v, g, cfg, powers)
    w, m, g = (np.asarray(a, np.float32).astype(np.float64) for a in (w, m, g))
    with np.errstate(all="ignore"):
        s_m = np.abs(b1 * m) + 2.0 * np.abs((1.0 - b1) * g) + np.abs(mm)
        c_v = 5.0
        k_m = np.where(mm != 0.0, s_m / np.abs(mm), 4.0)
        k_1, k_2 = _amplified(new[0]), _amplified(new[1])
        c_w = np.maximum(4.0, k_m + k_1 + 1.0 + (c_v + k_2 + 1.0) / 2.0 + 2.0 + 2.0 + 1.0)
        bw = U * np.abs(x) * (1.0 + 2.0 ** -20) + 2.0 * c_w * E * (np.abs(w) + np.abs(upd)) + TINY
        bm = U * np.abs(mm) * (1.0 + 2.0 ** -20) + 2.0 * E * s_m + TINY
        bv = U * np.abs(vv) * (1.0 + 2.0 ** -20) + 2.0 * c_v * E * np.abs(vv) + TINY
    return tuple(np.where(np.isfinite(b), b, np.inf) for b in (bw, bm, bv))


def agrees(got, ref, b):
    """got float32 [n] against the float64 reference and its bound -> (ok bool [n], ratio float64 [n]): where fp32(ref) is finite,
    |got - ref| <= b and the ratio is |got - ref| / b; where it is an infinity or NaN, got must be the same class (and sign): ratio
    0 when it is, inf when not."""
    got = np.asarray(got, np.float32)
    with np.errstate(all="ignore"):
        ref32 = np.asarray(ref, np.float64).astype(np.float32)
        special = ~np.isfinite(ref32)
        same_class = np.where(np.isnan(ref32), np.isnan(got), np.isinf(got) & (np.sign(got) == np.sign(ref32)))
        err = np.abs(got.astype(np.float64) - np.asarray(ref, np.float64))
        ratio = np.where(special, np.where(same_class, 0.0, np.inf), np.where(np.isfinite(got), err / b, np.inf))
    return ratio <= 1.0, ratio


# ---- the design input ----
PERIOD = 13                 # coprime to 1024: every residue falls into every trip of the kernel's loop over 2 084 elements
FAMILIES = {"g0_mv0": 1, "g0_mv": 2, "g_tiny": 3, "g_huge": 4, "v_inf": 5, "w0": 6, "w_cancel": 7, "w_tiny": 8, "denormal_out": 9}
NAN_AT = (39, 1027, 2054)                   # ordinary elements (residue 0), one per trip: g = NaN
INF_AT = ((530, np.inf), (1311, -np.inf))   # ordinary elements (residues 10, 11): g = +-inf
TRIPS = ((0, 1024), (1024, 2048), (2048, NW))


def family_index(name):
    """the elements of a family (``ordinary``: what no family and no isolated NaN / inf claims)"""
    idx = np.arange(NW)
    special = {*NAN_AT, *(i for i, _ in INF_AT)}
    if name == "ordinary":
        keep = ~np.isin(idx % PERIOD, list(FAMILIES.values()))
        return np.array([i for i in idx[keep] if i not in special])
    return idx[idx % PERIOD == FAMILIES[name]]


def design(cfg, powers, seed=0):
    """-> (w, m, v, g) float32 [2084].  Ordinary elements are N(0, 1)-scaled draws (v >= 0); the families, tiled with PERIOD:
      g0_mv0  g = 0, m = v = 0                    g0_mv   g = 0, m, v != 0           g_tiny  |g| = 1e-30: g g underflows fp32
      g_huge  |g| = 1e25: v' rounds to fp32 inf   v_inf   v = inf from an earlier step
      w0      w = 0                               w_tiny  |w| = 1e-30
      w_cancel  w = fp32(U / (1 - lr wd)): w' cancels to within 2^-20 |w| (U from this cfg and these powers; where U = 0, w = 0)
      denormal_out  g = 0, m = 1e-38, v = 1e-38: m', v' (beta < 1) are fp32 denormals - what tells a flushing device from one that keeps them
    and, isolated, g = NaN at NAN_AT and g = +-inf at INF_AT.  The same (m, v, g) for every cfg; only w_cancel's w follows it."""
    r = np.random.default_rng(seed)
    w = (0.3 * r.standard_normal(NW)).astype(np.float32)
    m = (0.1 * r.standard_normal(NW)).astype(np.float32)
    v = ((0.1 * r.standard_normal(NW)) ** 2).astype(np.float32)
    g = (0.1 * r.standard_normal(NW)).astype(np.float32)
    sign = np.where(r.integers(0, 2, NW) == 1, np.float32(1), np.float32(-1))
    f = family_index
    g[f("g0_mv0")] = 0; m[f("g0_mv0")] = 0; v[f("g0_mv0")] = 0
    g[f("g0_mv")] = 0
    g[f("g_tiny")] = np.float32(1e-30) * sign[f("g_tiny")]
    g[f("g_huge")] = np.float32(1e25) * sign[f("g_huge")]
    v[f("v_inf")] = np.inf
    w[f("w0")] = 0
    w[f("w_tiny")] = np.float32(1e-30) * sign[f("w_tiny")]
    d = f("denormal_out")
    g[d] = 0; m[d] = np.float32(1e-38) * sign[d]; v[d] = np.float32(1e-38)
    c = f("w_cancel")
    _, _, _, _, upd = adam_exact(w[c], m[c], v[c], g[c], cfg, powers)
    with np.errstate(all="ignore"):
        w[c] = (upd / (1.0 - cfg[0] * cfg[4])).astype(np.float32)
    w[c] = np.where(w[c] == 0, np.float32(0.0), w[c])      # lr = 0: +0, never -0 (x = -0 - -0 is +0 in IEEE arithmetic: the sign would move)
    for i in NAN_AT:
        g[i] = np.nan
    for i, x in INF_AT:
        g[i] = x
    return w, m, v, g


def check_design(cfg, powers):
    """the properties the design promises, asserted: every family in every trip, and what each family's name says"""
    w, m, v, g = design(cfg, powers)
    for name in [*FAMILIES, "ordinary"]:
        idx = family_index(name)
        for lo, hi in TRIPS:
            assert ((idx >= lo) & (idx < hi)).any(), (name, lo)
    for k, i in enumerate(NAN_AT):
        assert TRIPS[k][0] <= i < TRIPS[k][1] and np.isnan(g[i])
    assert all(np.isinf(g[i]) and np.sign(g[i]) == np.sign(x) for i, x in INF_AT)
    special = [*NAN_AT, *(i for i, _ in INF_AT)]
    assert np.isfinite(np.delete(g, special)).all() and np.isfinite(w).all() and np.isfinite(m).all()
    f = family_index
    with np.errstate(all="ignore"):
        assert ((g[f("g_tiny")] * g[f("g_tiny")]) == 0).all() and (g[f("g_tiny")] != 0).all()            # fp32 product: underflows
        x, mm, vv, _, upd = adam_exact(w, m, v, g, cfg, powers)
        assert np.isinf(vv[f("g_huge")].astype(np.float32)).all() and np.isfinite(vv[f("g_huge")]).all()
        c = f("w_cancel")
        moved = upd[c] != 0
        assert (np.abs(x[c][moved]) <= 2.0 ** -20 * np.abs(w[c][moved])).all() and (w[c][~moved] == 0).all()
        d = f("denormal_out")
        if 0 < cfg[1] < 1:
            assert ((np.abs(mm[d]) < TINY) & (mm[d] != 0)).all()
        if 0 < cfg[2] < 1:
            assert ((vv[d] < TINY) & (vv[d] != 0)).all()
    return w, m, v, g
