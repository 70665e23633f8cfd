"""Float64 reference of the lagged-gain table (rq_trajectory_policy_lag_table, csrc/rq_lag_table.inc; raptor_amd.probing.lag_gains)
with an element-wise error bound for the fp32 kernel and a NumPy float32 restatement of the kernel's chain.

The quantity, with the gain table's names (tests/gain_reference.py) at every live step s, h the state entering it:

    E_s[u, j] = dh'_u/dp0_j = m_j ((1 - z_u)(1 - n_u^2)(Win[u, j] + c_u r_u (1 - r_u) Wir[u, j]) + (h_u - n_u) z_u (1 - z_u) Wiz[u, j])
    D_s[u, v] = dh'_u/dh_v  = z_u [u == v] + (1 - z_u)(1 - n_u^2)(r_u Whn[u, v] + c_u r_u (1 - r_u) Whr[u, v]) + (h_u - n_u) z_u (1 - z_u) Whz[u, v]
    A^(k)_t = W2 D_t D_(s_1) .. D_(s_(k-1)) E_(s_k),  s_1, s_2, .. the live steps before t in its episode, back in time

``lag_table`` forms D and E as matrices and multiplies them out in float64.

The bound.  The kernel carries, per lag slot and seed, a row dh~ within e_dh of the float64 row (W2 D_t .. D_(s_(k-1)))[i] (lag 0: W2[i],
exact).  At step s it forms dn, dz, dhd, du, dPr, dPz, dGnh from it and the step's gate factors (``_factors``: the forward half of
``gain_reference.gain_bound``, each factor with its own error): sixteen elementary fp32 operations, each charged by
``gain_reference._mul`` / ``_sub`` at its worst.  Then two fp32 MFMA chains of K = 48 products, dp0 = Wi^T [dPr; dPz; du] opened by zero
and dh_next = Wh^T [dPr; dPz; dGnh] opened by dhd: ``_chain`` charges 49 addends, g = 49 u / (1 - 49 u), on the absolute-value product
|W|^T (|delta| + e_delta) + |opening| + e_opening and carries the operand errors through |W|^T e_delta + e_opening.  e_dh_next is the
next slot's e_dh: the absolute-value products are carried through every lag.  The ReLU mask selects; a cell whose chains meet a step
near a kink (``gain_reference.near_kink``) anywhere is left out.  A running fp32 sum of ``count`` terms: as
``gain_reference.table_bound``, whatever the order of the terms.  Nothing here is fitted to an observed error.
"""
import numpy as np

import gain_reference as GR
from actor_reference import K_SIG, _dense, _sigma, _step_of, blocks
from gain_reference import PRECISION, TAU_S, TAU_T, _mul, _sub
from teacher_reference import K_TANH, U

G49 = 49 * U / (1.0 - 49 * U)


def _factors(w, x, h):
    """x [M, 22], h [M, 16] -> the gate factors of M steps as (value, error) pairs, and the float64 ReLU mask: the forward half of
    ``gain_reference.gain_bound``, term for term"""
    B = blocks(w)
    x, h = np.asarray(x, np.float64)[:, :22], np.asarray(h, np.float64)
    zero_h = np.zeros_like(h)
    p0, E0 = _dense(B["W0"], B["b0"], x, np.zeros_like(x), PRECISION, first=True)
    relu = lambda v: np.maximum(v, 0.0)
    y0, ey = relu(p0), _step_of(relu, p0, E0, 1.0)
    v, ev = np.concatenate([y0, h], axis=1), np.concatenate([ey, zero_h], axis=1)
    gate = []
    for m in range(2):
        rows = slice(16 * m, 16 * m + 16)
        W = np.concatenate([B["Wi"][rows], B["Wh"][rows]], axis=1)
        b = B["bi"][rows].astype(np.float64) + B["bh"][rows].astype(np.float64)
        s, E = _dense(W, b, v, ev, PRECISION, scaled=True, scale=float(-K_SIG), bias_sum=True)
        gate.append((_sigma(s), _step_of(_sigma, s, E, 0.25) + TAU_S))
    (r, er), (z, ez) = gate
    rows = slice(32, 48)
    p, Ep = _dense(B["Wi"][rows], B["bi"][rows], y0, ey, PRECISION, scaled=True, scale=float(-K_TANH))
    c, Eq = _dense(B["Wh"][rows], B["bh"][rows], h, zero_h, PRECISION, scaled=True, scale=float(-K_TANH))
    arg = p + r * c
    Ea = Ep + (np.abs(r) + er) * Eq + er * np.abs(c)
    Ea = Ea + U * (np.abs(arg) + Ea)
    n, en = np.tanh(arg), _step_of(np.tanh, arg, Ea, 1.0) + TAU_T
    one = np.ones_like(z)
    omz = _sub(one, 0.0, z, ez)
    f = {"r": (r, er), "z": (z, ez), "c": (c, Eq + 4 * U * (np.abs(c) + Eq)), "omz": omz, "hmn": _sub(h, 0.0, n, en),
         "omn": _sub(one, 0.0, *_mul(n, en, n, en)), "rr1": _mul(r, er, *_sub(one, 0.0, r, er)), "zz1": _mul(z, ez, *omz)}
    return f, p0 > 0.0, (h, n)


def step_matrices(w, x, h):
    """-> (D [M, 16, 16], E [M, 16, 16]) float64, the module docstring's dh'/dh and dh'/dp0 of M steps"""
    B = blocks(w, np.float64)
    f, mask, (h, n) = _factors(w, x, h)
    r, z, c = f["r"][0], f["z"][0], f["c"][0]
    fn = (1.0 - z) * (1.0 - n * n)
    fr, fz = fn * c * r * (1.0 - r), (h - n) * z * (1.0 - z)
    Wi, Wh = B["Wi"], B["Wh"]
    E = fn[:, :, None] * Wi[32:48] + fr[:, :, None] * Wi[0:16] + fz[:, :, None] * Wi[16:32]
    D = (fn * r)[:, :, None] * Wh[32:48] + fr[:, :, None] * Wh[0:16] + fz[:, :, None] * Wh[16:32] + z[:, :, None] * np.eye(16)
    return D, E * mask[:, None, :]


def _chain(WT, d, ed, c0, ec0):
    """one fp32 MFMA chain WT [16, 48] over d [..., 48] opened by c0 -> (value, bound): 49 addends"""
    A = np.abs(WT).T
    mag = (np.abs(d) + ed) @ A + np.abs(c0) + ec0
    return d @ WT.T + c0, ed @ A + ec0 + G49 * mag


def _step_bound(f, WiT, WhT, dh, e_dh):
    """dh, e_dh [N, 4, 16] and one step's factors [N, 16] -> ((dp0, E), (dh_next, e_next)) before the ReLU mask"""
    F = {k: (v[:, None, :], e[:, None, :]) for k, (v, e) in f.items()}
    dn = _mul(dh, e_dh, *F["omz"])
    dz = _mul(dh, e_dh, *F["hmn"])
    dhd = _mul(dh, e_dh, *F["z"])
    du = _mul(*dn, *F["omn"])
    dPr = _mul(*_mul(*du, *F["c"]), *F["rr1"])
    dPz = _mul(*dz, *F["zz1"])
    dGnh = _mul(*du, *F["r"])
    cat = lambda last: tuple(np.concatenate([dPr[i], dPz[i], last[i]], axis=-1) for i in range(2))
    return _chain(WiT, *cat(du), 0.0, 0.0), _chain(WhT, *cat(dGnh), *dhd)


def _walk(done, select, K, start, step):
    """The episode rules of the table, walked back in time over done [T, N].  ``start()`` -> the seed slot's state, ``step(s, k, state)``
    -> (term or None, the state one step back).  Yields (s, k, on [N], term): the envs that count step-slot (s, k)."""
    T, N = done.shape
    sel = np.ones((T, N), bool) if select is None else np.asarray(select) != 0
    bits = np.zeros((K, N), bool)                       # slot k holds the chain of a selected seed of this episode
    slots = [None] * K
    for s in range(T - 1, -1, -1):
        live, ended = done[s] != 4, (done[s] == 1) | (done[s] == 2)
        cur = np.concatenate([(sel[s] & live)[None], bits[1:] & ~ended & live], axis=0)
        slots[0] = start()
        nxt = [None] * K
        for k in range(K - 1, -1, -1):
            if slots[k] is None:
                continue
            term, back = step(s, k, slots[k])
            yield s, k, cur[k], term
            if k + 1 < K:       # a frozen env keeps what its slot held
                old = slots[k + 1] if slots[k + 1] is not None else back
                nxt[k + 1] = tuple(np.where(live.reshape((N,) + (1,) * (b.ndim - 1)), b, o) for b, o in zip(back, old))
        slots = nxt
        bits[1:] = np.where(live, cur[:-1], bits[1:])


def lag_table(w, obs, hid, done, n_lags, select=None):
    """obs [T, N, 22], hid [T, N, 16] (the state entering every step), done [T, N], select [T, N] or None
    -> (sum [K, 4, 16, N] float64, count [K, N] uint32, bound [K, 4, 16, N], left_out [K, N] bool)"""
    T, N = done.shape
    K = int(n_lags)
    B = blocks(w, np.float64)
    x, h = obs.reshape(T * N, 22), hid.reshape(T * N, 16)
    D, E = (m.reshape(T, N, 16, 16) for m in step_matrices(w, x, h))
    f, mask, _ = _factors(w, x, h)
    f = {k: (v.reshape(T, N, 16), e.reshape(T, N, 16)) for k, (v, e) in f.items()}
    mask = mask.reshape(T, N, 16)
    kink = GR.near_kink(w, x).reshape(T, N)
    with np.errstate(invalid="ignore", over="ignore"):          # what a frozen step holds reaches no cell
        for a in (D, E):
            a[done == 4] = 0.0
    WiT, WhT = np.ascontiguousarray(B["Wi"].T), np.ascontiguousarray(B["Wh"].T)
    W2 = np.broadcast_to(B["W2"], (N, 4, 16))
    total, esum, mag = (np.zeros((K, 4, 16, N)) for _ in range(3))
    count, left_out = np.zeros((K, N), np.uint32), np.zeros((K, N), bool)

    def step(s, k, state):
        P, v, e, met = state                            # the float64 product; the bound's value and error; a kink met on the chain
        fs = {key: (val[s], err[s]) for key, (val, err) in f.items()}
        (_, Ek), (vn, en) = _step_bound(fs, WiT, WhT, v, e)
        met = met | kink[s]
        return (P @ E[s], Ek * mask[s][:, None, :], met), (P @ D[s], vn, en, met)

    live_safe = lambda a, on: np.where(on[:, None, None], a, 0.0)
    for s, k, on, (A, EA, met) in _walk(done, select, K, lambda: (W2, W2, np.zeros((N, 4, 16)), np.zeros(N, bool)), step):
        with np.errstate(invalid="ignore"):
            A, EA = live_safe(A, on), live_safe(EA, on)
        total[k] += A.transpose(1, 2, 0)
        esum[k] += EA.transpose(1, 2, 0)
        mag[k] += (np.abs(A) + EA).transpose(1, 2, 0)
        count[k] += on.astype(np.uint32)
        left_out[k] |= on & met
    c = np.maximum(count.astype(np.float64) - 1.0, 0.0)[:, None, None, :]
    return total, count, esum + c * U / (1.0 - c * U) * mag, left_out


# ---------------------------------------------------------------------------- the kernel's chain in NumPy float32 ---
_f32 = np.float32


def emulate_table(w, obs, hid, done, n_lags, select=None, order=0, untransposed=None):
    """A plain float32 restatement of the kernel: the step in float32, the adjoint products in one of two contraction orders
    (``order`` 0: one 48-term product; 1: the three gates' 16-term products, added last to first), the sums in the walk's order
    -> sum [K, 4, 16, N] float32.  ``untransposed``: the name of one 16x16 block ("Whr", "Wiz", ..) used as it lies - a fault."""
    T, N = done.shape
    K = int(n_lags)
    B = blocks(w)
    Wi, Wh = B["Wi"].copy(), B["Wh"].copy()
    if untransposed:
        M, g = (Wi if untransposed[1] == "i" else Wh), 16 * "rzn".index(untransposed[2])
        M[g:g + 16] = M[g:g + 16].T.copy()
    one = _f32(1)
    sig = lambda v: (one / (one + np.exp(-v))).astype(_f32)
    total = np.zeros((K, 4, 16, N), _f32)
    W2 = np.broadcast_to(B["W2"], (N, 4, 16)).astype(_f32)

    def prod(M, d):                                      # M^T over the 48 gate rows
        if order == 0:
            return d @ M
        return (d[..., 32:] @ M[32:] + d[..., 16:32] @ M[16:32]) + d[..., :16] @ M[:16]

    def step(s, k, state):
        (dh,) = state
        x, h = obs[s].astype(_f32), hid[s].astype(_f32)
        with np.errstate(invalid="ignore", over="ignore"):
            p0 = x @ B["W0"].T + B["b0"]
            y0 = np.maximum(p0, _f32(0))
            gi, gh = y0 @ B["Wi"].T + B["bi"], h @ B["Wh"].T + B["bh"]
            r, z, c = sig(gi[:, :16] + gh[:, :16]), sig(gi[:, 16:32] + gh[:, 16:32]), gh[:, 32:]
            n = np.tanh(gi[:, 32:] + r * c).astype(_f32)
            e = lambda a: a[:, None, :]
            dn, dz, dhd = dh * e(one - z), dh * e(h - n), dh * e(z)
            du = dn * e(one - n * n)
            dPr, dPz, dGnh = du * e(c) * e(r * (one - r)), dz * e(z * (one - z)), du * e(r)
            dp0 = np.where(e(p0 > 0), prod(Wi, np.concatenate([dPr, dPz, du], axis=-1)), _f32(0))
            back = prod(Wh, np.concatenate([dPr, dPz, dGnh], axis=-1)) + dhd
        return dp0.astype(_f32), (back.astype(_f32),)

    for s, k, on, A in _walk(done, select, K, lambda: (W2,), step):
        total[k] = np.where(on, total[k] + A.transpose(1, 2, 0), total[k])
    return total
