"""Float64 reference of the feedback-gain table (rq_trajectory_policy_gain_table, csrc/rq_gain_table.inc;
raptor_amd.probing.feedback_gains) with an element-wise error bound for the fp32 kernel, a NumPy float32 emulation of the kernel's
chain, and the table's bucket sums.

The quantity, with the checkpoint's names, at the observation x (22) and the state h (16) entering the step:

    p0 = W0 x + b0,  y0 = relu(p0),  m_k = [p0_k > 0]  (ReLU'(0) = 0)
    r = s(Wir y0 + bir + Whr h + bhr),  z = s(Wiz y0 + biz + Whz h + bhz),  c = Whn h + bhn,  n = tanh(Win y0 + bin + r c)
    A[i, k] = m_k sum_u W2[i, u] ((1 - z_u)(1 - n_u^2)(Win[u, k] + c_u r_u (1 - r_u) Wir[u, k]) + (h_u - n_u) z_u (1 - z_u) Wiz[u, k])
    G = A W0  [4, 22]

``gain_bound``.  The forward half is ``actor_reference.step_bound``'s model of the fp32 build, restated here because the bound needs
the intermediates r, z, n and c = W_hn h + b_hn with their errors (the same ``_dense`` contractions, the same tau constants:
tau_sigma = 5 u + 2^-44, tau_tanh = 11 u).  The kernel un-scales the pre-scaled chain, c~ = fl(gnh~ kInvT~): kInvT~ is a float
constant formed from a rounded literal by a rounded division and the packer's k is rounded too, so k~ kInvT~ = 1 + d with
|d| < 3 u, and the product rounds once: e_c = E_q + 4 u (|c| + E_q).

The backward half is elementary fp32 arithmetic on values that carry an error each.  With a~ within e_a of a and b~ within e_b of b:

    fl(a~ b~)  is within  |a| e_b + |b| e_a + e_a e_b =: e  of a b,  plus the rounding  u (|a b| + e)
    fl(a~ - b~)  is within  e_a + e_b =: e  of a - b,  plus  u (|a - b| + e)

Per seed i and hidden unit u the kernel forms, in this order (rq_gain_table.inc),
    dn = W2[i, u] (1 - z),  dz = W2[i, u] (h - n),  du = dn (1 - n n),  dPr = (du c) (r (1 - r)),  dPz = dz (z (1 - z)),  dGni = du:
13 such operations, each charged as above (a compiler that contracts a product and a sum into one fma rounds once where two
roundings are charged: the bound covers both).  W2 and h are exact fp32 operands.  Then dy0 = Wi^T [dPr; dPz; dGni] is ONE fp32
MFMA chain of K = 48 products opened by zero with the unscaled weights as they are: ``_dense`` with 49 addends, no operand
rounding, the absolute-value product |Wi|^T (|delta| + e_delta).  The mask m_k multiplies nothing: it selects, and it is the
float64 mask away from a kink (``near_kink``).  So the bound on one A is E_A[i, k] = m_k E_dy0[i, k], and it has the shape
|W2| . |gate factors| . |Wi| throughout.

A running fp32 sum of ``count`` terms in step order: every addition rounds once, so a term passes through at most count - 1
roundings; with g = (count - 1) u / (1 - (count - 1) u) the sum is within  sum_t E_A,t + g sum_t (|A_t| + E_A,t)  of the float64
sum.  ``gain_bound`` returns E_A and the term's share E_A + g (|A| + E_A); a cell's bound is the sum of the shares of its steps.

Nothing here is fitted to an observed error.
"""
import numpy as np

from actor_reference import K_SIG, TAU_SIGMA, TAU_TANH, _chain_f32, _dense, _fma, _sigma, _step_of, blocks
from error_table_reference import ages, buckets
from teacher_reference import K_TANH, U

PRECISION = "fp32"
TAU_S = TAU_SIGMA.get(PRECISION, 5 * U + 2.0 ** -44)
TAU_T = TAU_TANH.get(PRECISION, 11 * U)
KINK_FACTOR = 32 * 2.0 ** -24


# ---------------------------------------------------------------------------- float64 ---
def _forward64(B, x, h):
    W0, b0 = B["W0"].astype(np.float64), B["b0"].astype(np.float64)
    Wi, Wh = B["Wi"].astype(np.float64), B["Wh"].astype(np.float64)
    bi, bh = B["bi"].astype(np.float64), B["bh"].astype(np.float64)
    p0 = x @ W0.T + b0
    y0 = np.maximum(p0, 0.0)
    gi, gh = y0 @ Wi.T + bi, h @ Wh.T + bh
    r, z = _sigma(gi[:, :16] + gh[:, :16]), _sigma(gi[:, 16:32] + gh[:, 16:32])
    c = gh[:, 32:]
    n = np.tanh(gi[:, 32:] + r * c)
    return p0, y0, r, z, c, n


def step64(w, x, h):
    """-> (a [N, 4], h' [N, 16]) float64: one step, the map the gain differentiates"""
    B = blocks(w)
    x, h = np.asarray(x, np.float64)[:, :22], np.asarray(h, np.float64)
    _, _, r, z, c, n = _forward64(B, x, h)
    hn = (1.0 - z) * n + z * h
    return hn @ B["W2"].astype(np.float64).T + B["b2"].astype(np.float64), hn


def gain_A(w, x, h):
    """w [2084], x [N, 22], h [N, 16] -> A [N, 4, 16] float64, da/dp0 from the formula"""
    B = blocks(w)
    x, h = np.asarray(x, np.float64)[:, :22], np.asarray(h, np.float64)
    p0, _, r, z, c, n = _forward64(B, x, h)
    Wi, W2 = B["Wi"].astype(np.float64), B["W2"].astype(np.float64)
    Wir, Wiz, Win = Wi[0:16], Wi[16:32], Wi[32:48]
    fn = (1.0 - z) * (1.0 - n * n)                     # [N, u]
    fr = fn * c * r * (1.0 - r)
    fz = (h - n) * z * (1.0 - z)
    # inner[N, u, k]
    inner = fn[:, :, None] * Win[None] + fr[:, :, None] * Wir[None] + fz[:, :, None] * Wiz[None]
    A = np.einsum("iu,nuk->nik", W2, inner)
    return A * (p0 > 0.0)[:, None, :]


def jacobian(w, x, h):
    """-> G [N, 4, 22] float64 = A W0: the instantaneous gain da/dx at fixed h"""
    return gain_A(w, x, h) @ blocks(w)["W0"].astype(np.float64)


def near_kink(w, x):
    """-> [N] bool: some |p0_k| in float64 lies below 32 . 2^-24 (sum_f |W0[k, f] x_f| + |b0_k|) - the forward error of a 23-term fp32
    dot product with margin; there the fp32 mask may legitimately differ from the float64 one"""
    B = blocks(w)
    x = np.asarray(x, np.float64)[:, :22]
    W0, b0 = B["W0"].astype(np.float64), B["b0"].astype(np.float64)
    p0 = x @ W0.T + b0
    mag = np.abs(x) @ np.abs(W0).T + np.abs(b0)
    return (np.abs(p0) < KINK_FACTOR * mag).any(axis=1)


# ---------------------------------------------------------------------------- the bound ---
def _mul(a, ea, b, eb):
    v = a * b
    e = np.abs(a) * eb + np.abs(b) * ea + ea * eb
    return v, e + U * (np.abs(v) + e)


def _sub(a, ea, b, eb):
    v = a - b
    e = ea + eb
    return v, e + U * (np.abs(v) + e)


def gain_bound(w, x, h, count=1):
    """-> (A [N, 4, 16] float64, E_A, share): E_A bounds |fp32 A - A| element-wise, share = E_A + g (|A| + E_A) with
    g = (count - 1) u / (1 - (count - 1) u) is the step's part of the bound of a running fp32 sum of ``count`` terms (module
    docstring).  ``count`` is a scalar or broadcasts against [N, 1, 1]."""
    B = blocks(w)
    x, h = np.asarray(x, np.float64)[:, :22], np.asarray(h, np.float64)
    zero_h = np.zeros_like(h)
    # ---- forward, as actor_reference.step_bound ----
    p0, E0 = _dense(B["W0"], B["b0"], x, np.zeros_like(x), PRECISION, first=True)
    relu = lambda v: np.maximum(v, 0.0)
    y0, ey = relu(p0), _step_of(relu, p0, E0, 1.0)
    v, ev = np.concatenate([y0, h], axis=1), np.concatenate([ey, zero_h], axis=1)
    gate, eg = [], []
    for m in range(2):
        rows = slice(16 * m, 16 * m + 16)
        W = np.concatenate([B["Wi"][rows], B["Wh"][rows]], axis=1)
        b = B["bi"][rows].astype(np.float64) + B["bh"][rows].astype(np.float64)
        s, E = _dense(W, b, v, ev, PRECISION, scaled=True, scale=float(-K_SIG), bias_sum=True)
        gate.append(_sigma(s))
        eg.append(_step_of(_sigma, s, E, 0.25) + TAU_S)
    (r, z), (er, ez) = gate, eg
    rows = slice(32, 48)
    p, Ep = _dense(B["Wi"][rows], B["bi"][rows], y0, ey, PRECISION, scaled=True, scale=float(-K_TANH))
    c, Eq = _dense(B["Wh"][rows], B["bh"][rows], h, zero_h, PRECISION, scaled=True, scale=float(-K_TANH))
    arg = p + r * c
    Ea = Ep + (np.abs(r) + er) * Eq + er * np.abs(c)
    Ea = Ea + U * (np.abs(arg) + Ea)
    n, en = np.tanh(arg), _step_of(np.tanh, arg, Ea, 1.0) + TAU_T
    ec = Eq + 4 * U * (np.abs(c) + Eq)
    # ---- the gate factors, shared by the four seeds up to W2[i, u] ----
    one = np.ones_like(z)
    omz, e_omz = _sub(one, 0.0, z, ez)
    hmn, e_hmn = _sub(h, 0.0, n, en)
    nsq, e_nsq = _mul(n, en, n, en)
    omn, e_omn = _sub(one, 0.0, nsq, e_nsq)
    omr, e_omr = _sub(one, 0.0, r, er)
    rr1, e_rr1 = _mul(r, er, omr, e_omr)
    zz1, e_zz1 = _mul(z, ez, omz, e_omz)
    W2 = B["W2"].astype(np.float64)
    WiT = np.ascontiguousarray(B["Wi"].T)              # [16 (k), 48 (gate row)]: dy0 = WiT [dPr; dPz; dGni]
    A = np.empty((x.shape[0], 4, 16))
    EA = np.empty_like(A)
    mask = p0 > 0.0
    for i in range(4):
        dh = W2[i][None, :]
        dn, e_dn = _mul(dh, 0.0, omz, e_omz)
        dz, e_dz = _mul(dh, 0.0, hmn, e_hmn)
        du, e_du = _mul(dn, e_dn, omn, e_omn)
        t, e_t = _mul(du, e_du, c, ec)
        dPr, e_dPr = _mul(t, e_t, rr1, e_rr1)
        dPz, e_dPz = _mul(dz, e_dz, zz1, e_zz1)
        d = np.concatenate([dPr, dPz, du], axis=1)
        ed = np.concatenate([e_dPr, e_dPz, e_du], axis=1)
        dy0, E = _dense(WiT, np.zeros(16, np.float32), d, ed, PRECISION)
        A[:, i] = np.where(mask, dy0, 0.0)
        EA[:, i] = np.where(mask, E, 0.0)
    cnt = np.asarray(count, np.float64)
    g = (cnt - 1.0) * U / (1.0 - (cnt - 1.0) * U)
    return A, EA, EA + g * (np.abs(A) + EA)


# ---------------------------------------------------------------------------- the kernel's chain in NumPy float32 ---
_f32, _f64 = np.float32, np.float64


def emulate_A(w, x, h):
    """What k_policy_gain_table computes for one step, operation by operation in float32 (MFMA chains add one K-step of four
    products at a time; the elementary operations round once each) -> A [N, 4, 16] float32"""
    B = blocks(w)
    x = np.ascontiguousarray(np.asarray(x, _f32)[:, :22])
    h = np.asarray(h, _f32)
    N = x.shape[0]
    kS, kT = K_SIG, K_TANH
    k = np.concatenate([np.full(32, kS, _f32), np.full(16, kT, _f32)])
    Wi, Wh = (k[:, None] * B["Wi"]).astype(_f32), (k[:, None] * B["Wh"]).astype(_f32)
    br = (kS * (B["bi"][0:16] + B["bh"][0:16]).astype(_f32)).astype(_f32)
    bz = (kS * (B["bi"][16:32] + B["bh"][16:32]).astype(_f32)).astype(_f32)
    bni, bnh = (kT * B["bi"][32:]).astype(_f32), (kT * B["bh"][32:]).astype(_f32)
    x24 = np.concatenate([x, np.ones((N, 1), _f32), np.zeros((N, 1), _f32)], axis=1)
    W24 = np.concatenate([B["W0"], B["b0"][:, None], np.zeros((16, 1), _f32)], axis=1)
    p0 = _chain_f32(W24, x24, np.zeros(16, _f32), [list(range(4 * s, 4 * s + 4)) for s in range(6)])
    y0 = np.maximum(p0, _f32(0))
    gk = [[s, 4 + s, 8 + s, 12 + s] for s in range(4)]
    hy, both = np.concatenate([h, y0], axis=1), gk + [[16 + i for i in g] for g in gk]
    gr = _chain_f32(np.concatenate([Wh[0:16], Wi[0:16]], axis=1), hy, br, both)
    gz = _chain_f32(np.concatenate([Wh[16:32], Wi[16:32]], axis=1), hy, bz, both)
    gni, gnh = _chain_f32(Wi[32:], y0, bni, gk), _chain_f32(Wh[32:], h, bnh, gk)
    one, two = _f32(1.0), _f32(2.0)
    with np.errstate(over="ignore", invalid="ignore"):
        rr = (one / (one + np.exp2(gr))).astype(_f32)
        zz = (one / (one + np.exp2(gz))).astype(_f32)
        arg = _fma(rr, gnh, gni)
        nn = _fma(np.full_like(arg, two), (one / (one + np.exp2(arg))).astype(_f32), np.full_like(arg, -one))
    kInvT = _f32(one / _f32(-2.8853900817779268))
    cc = (gnh * kInvT).astype(_f32)
    WiT = np.ascontiguousarray(B["Wi"].T)              # unscaled, [16, 48]
    groups = [[16 * g + 4 * q + r for q in range(4)] for g in range(3) for r in range(4)]
    A = np.empty((N, 4, 16), _f32)
    for i in range(4):
        dh = B["W2"][i][None, :]
        dn = (dh * (one - zz)).astype(_f32)
        dz = (dh * (h - nn)).astype(_f32)
        du = (dn * (one - (nn * nn).astype(_f32))).astype(_f32)
        dPr = ((du * cc).astype(_f32) * (rr * (one - rr)).astype(_f32)).astype(_f32)
        dPz = (dz * (zz * (one - zz)).astype(_f32)).astype(_f32)
        dy0 = _chain_f32(WiT, np.concatenate([dPr, dPz, du], axis=1), np.zeros(16, _f32), groups)
        A[:, i] = np.where(y0 > 0, dy0, _f32(0))
    return A


# ---------------------------------------------------------------------------- the table ---
def gain_table(A_steps, done, edges, dtype=np.float64):
    """A_steps [T, N, 4, 16], done [T, N], edges [B + 1] -> (sum [B, 4, 16, N] of ``dtype`` in step order, count [B, N] uint32), ages
    as in ``error_table_reference.ages``.  What is frozen or outside the buckets is selected away before it meets a sum."""
    done = np.asarray(done)
    T, N = done.shape
    b = buckets(ages(done), edges)
    nb = len(edges) - 1
    total, count = np.zeros((nb, 4, 16, N), dtype), np.zeros((nb, N), np.uint32)
    cols = np.arange(N)
    for t in range(T):
        at = b[t] >= 0
        i, bi = cols[at], b[t][at]
        total[bi, :, :, i] = (total[bi, :, :, i] + np.asarray(A_steps[t], dtype)[at]).astype(dtype)
        count[bi, i] += np.uint32(1)
    return total, count


def table_bound(A_steps, E_steps, done, edges):
    """A_steps, E_steps [T, N, 4, 16] float64 (``gain_bound``'s A and E_A per step) -> [B, 4, 16, N]: the bound of every cell, the
    sum over its steps of E_A + g (|A| + E_A) with g from the cell's own count"""
    total, count = gain_table(np.abs(A_steps) + E_steps, done, edges)
    esum, _ = gain_table(E_steps, done, edges)
    c = count.astype(np.float64)[:, None, None, :]
    g = np.maximum(c - 1.0, 0.0) * U / (1.0 - np.maximum(c - 1.0, 0.0) * U)
    return esum + g * total
