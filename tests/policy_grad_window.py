"""A sound element-wise bound for the learner's gradient over a SHORT teacher-forced window (T <= 3) on arbitrary weights, and a
NumPy float32 emulation of the backward kernel (csrc/rq_grad_backward.inc, k_policy_grad_reduce in csrc/rq_grad.hpp).

``policy_grad_reference.bound`` is 2 u K A with A the recursion on magnitudes: it charges every derivative factor relative to the
factor's own size.  The kernel forms 1 - z, 1 - n^2, r (1 - r), h - n from ROUNDED gates, so each factor carries an absolute error
of the order of u times its operands however small it is itself; on saturated or signed weights and on large observations the
true error leaves that bound by orders of magnitude.  ``window_bound`` instead carries an error beside every value, as
``gain_reference.gain_bound`` does for the gain table - the delta chain is the same six expressions.

Forward, per step (``_forward``; the constants are ``actor_reference``'s and ``gain_reference``'s, fp32 build): y0, r, z,
c = fl(gnh kInvT), n carry the ``e`` of ``gain_reference.gain_bound``, now with an entering state h that is within e_h of the float64
one: e_h joins the operand errors of the r / z chain (K = 32) and of the W_hn chain (K = 16).  h' = fma(z, h - n, n) with the
difference rounded first (rq_grad_backward.inc:143): with h~ = h + dh, n~ = n + dn, z~ = z + dz, d~ = (h~ - n~)(1 + e1),
    n~ + z~ d~ - h' = dn (1 - z) + z dh + z e1 (h~ - n~) + dz d~,
so with D = |h - n| + e_n + e_h the error before the fma's own rounding is T = e_n |1 - z| + |z| e_h + (u |z| + e_z (1 + u)) D and
e_h' = T + u (|h'| + T) (``actor_reference.step_bound`` with e_h = 0).  The state entering step 0 is the fp32 number the kernel reads
(e_h = 0); after a step with done code 1 or 2 it is h0, exact again; a step with code 4 leaves state and error as they were
(rq_grad_forward.inc; policy_grad_reference.forward).

Delta chain (rq_grad_backward.inc:192-204), every operation by ``gain_reference._mul`` / ``_sub``:
    dh   = W2^T da + din           ONE K = 4 MFMA chain opened by din (:192): ``_dense`` with 5 addends, the opener's own error e_din
                                   passed through and subject to the chain's roundings
    dn   = dh (1 - z)   dz = dh (h - n)   dhd = dh z   du = dn (1 - n n)
    dPr  = (du c) (r (1 - r))   dPz = dz (z (1 - z))   dGni = du   dGnh = du r
(a compiler that contracts 1 - n n into one fma rounds once where two roundings are charged).  da is the caller's fp32 number, exact.
Then dy0 = W_i^T [dPr; dPz; dGni] (:212-228) is one K = 48 chain opened by zero and dhp = W_h^T [dPr; dPz; dGnh] one opened by dhd,
on the unscaled weights (rq_pack.cpp pack_policy_grad_t).  The ReLU mask selects (:232): it is the float64 mask wherever no step
of the env lies near a kink (``gain_reference.near_kink``); envs that do are given dact = 0 by the tests and contribute exact zeros
to kernel and reference alike.  The carry is dc = dhp + pass (:233): pass is zero unless the step is frozen, so the addition rounds
only there.  Code 1 / 2: the carry goes to h0's lane sum and is cut (:178); code 4: it passes and din = 0 (:179-180).

Every fp32 result is also charged 2^-126, the smallest normal number: a result that is flushed or subnormal lies within that of
the exact one, whatever the denormal mode of the instruction.

Accumulation.  With n additions a term passes through at most n roundings: g(n) = n u / (1 - n u) (``gain_reference``'s table sums):
  * weight blocks W0 | b0, Wi, Wh, W2: per wave one MFMA accumulator per element, opened by zero, over 4 tiles x T steps x 16 envs on
    K (:259-275): 64 T products, g(64 T); a product of two values that carry errors each, a b with |a| e_b + |b| e_a + e_a e_b (the
    MFMA forms the product exactly).  b0 rides the constant-1 feature 22 of the observation (:87, :303).
  * b_i, b_h, h0, b2: lane (q, j) adds its four tiles' deltas over the T steps (:234-239; h0 also at the start, :285): g(4 T), h0
    g(4 T + 4); then 16 lanes are folded from zero (:317): g(16).
  * the waves' partials are added from zero in ascending order (k_policy_grad_reduce): g(waves).
dL/dh_start is the carry after step 0 as it stands (:286).  Nothing here is fitted to an observed error.

``emulate_backward`` is the kernel's arithmetic in NumPy float32 up to the order inside one MFMA (a K-step's four products are
added exactly and rounded once, ``actor_reference._chain_f32``): sigma as 1 / (1 + exp2(a)) on the pre-scaled accumulator, c through
kInvT, the expressions in the kernel's order, the accumulators in the kernel's order (step descending, tile, K-step; lanes folded
j ascending; waves ascending).  ``alter`` makes one deliberate mistake (``ALTERATIONS``).
"""
import numpy as np

import gain_reference as GR
import policy_grad_reference as R
from actor_reference import K_SIG, _chain_f32, _dense, _fma, _sigma, _step_of, blocks
from gain_reference import PRECISION, TAU_S, TAU_T
from teacher_reference import K_TANH, U, _constants

FLOOR = 2.0 ** -126
ALTERATIONS = ("rz_exchanged", "kinvt_halved", "dgnh_without_r", "one_minus_n", "relu_mask_dropped", "end_keeps_carry",
               "frozen_runs")


def g_of(n_add):
    """a term of a running fp32 sum of n_add additions is rounded at most n_add times"""
    return n_add * U / (1.0 - n_add * U)


def _mul(a, ea, b, eb):
    v, e = GR._mul(a, ea, b, eb)
    return v, e + FLOOR


def _sub(a, ea, b, eb):
    v, e = GR._sub(a, ea, b, eb)
    return v, e + FLOOR


def _opened(W32, c, ec, v, ev):
    """one fp32 MFMA chain s = c + W v whose opener c [N, out] is itself within ec: ``_dense`` on (c, v, ev), plus ec passed
    through and rounded with the running sum"""
    s, E = _dense(W32, c, v, ev, PRECISION)
    _, g_acc, _, _ = _constants(PRECISION, np.asarray(W32).shape[1], False, False)
    return s, E + ec * (1.0 + g_acc / (1.0 - g_acc)) + FLOOR


def _forward(B, x, h, eh):
    """one step in float64 with the error of the fp32 kernel's value beside every intermediate (module docstring)"""
    p0, E0 = _dense(B["W0"], B["b0"], x, np.zeros_like(x), PRECISION, first=True)
    relu = lambda v: np.maximum(v, 0.0)
    y0, ey = relu(p0), _step_of(relu, p0, E0, 1.0)
    v, ev = np.concatenate([y0, h], axis=1), np.concatenate([ey, eh], axis=1)
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
    c, Eq = _dense(B["Wh"][rows], B["bh"][rows], h, eh, PRECISION, scaled=True, scale=float(-K_TANH))
    arg = p + r * c
    Ea = Ep + (np.abs(r) + er) * Eq + er * np.abs(c)
    Ea = Ea + U * (np.abs(arg) + Ea)
    n, en = np.tanh(arg), _step_of(np.tanh, arg, Ea, 1.0) + TAU_T
    ec = Eq + 4 * U * (np.abs(c) + Eq) + FLOOR
    hn = n + z * (h - n)
    D = np.abs(h - n) + en + eh
    T = en * np.abs(1.0 - z) + np.abs(z) * eh + (U * np.abs(z) + ez * (1.0 + U)) * D
    ehn = T + U * (np.abs(hn) + T) + FLOOR
    return dict(p0=p0, y0=y0, ey=ey, r=r, er=er, z=z, ez=ez, c=c, ec=ec, n=n, en=en, hn=hn, ehn=ehn)


def _pad(a, npad):
    out = np.zeros((npad,) + a.shape[1:])
    out[:a.shape[0]] = a
    return out


def _sum_levels(V, E, adds):
    """V, E [L1, L2, ..., rows]: nested running fp32 sums, innermost level first (axis 0), each level a sum of ``adds[k]`` additions
    -> (sum, bound)"""
    for n_add in adds:
        g = g_of(n_add)
        V, E = V.sum(axis=0), E.sum(axis=0) + g * (np.abs(V) + E).sum(axis=0)
    return V, E


def window_bound(w32, obs, done, dact, start, h_start, waves):
    """w32 [2084] float32, obs [T, N, 22], done [T, N], dact [T, N, 4] (float32 values), start "initial" | "current", h_start [N, 16]
    (current), waves = ceil(N / 64) -> (g [2084], gh [N, 16] or None, bound_g, bound_gh), float64: the gradient of
    ``policy_grad_reference.backward`` and an element-wise bound on what k_policy_grad_backward + k_policy_grad_reduce may differ
    from it by (module docstring).  T <= 3."""
    w32 = np.asarray(w32, np.float32)
    obs, done, dact = np.asarray(obs, np.float64)[:, :, :22], np.asarray(done), np.asarray(dact, np.float64)
    T, N = done.shape
    assert T <= 3 and waves == (N + 63) // 64, (T, N, waves)
    _, cache = R.forward(w32.astype(np.float64), obs, done, start, h_start)
    g, gh = R.backward(cache, dact)
    B = blocks(w32)
    W2T = np.ascontiguousarray(B["W2"].T)              # [16, 4]
    WiT = np.ascontiguousarray(B["Wi"].T)              # [16, 48]
    WhT = np.ascontiguousarray(B["Wh"].T)
    h0 = B["h0"].astype(np.float64)
    # ---- forward: the values and errors of every step ----
    h = np.tile(h0, (N, 1)) if start == "initial" else np.asarray(h_start, np.float64).reshape(N, 16)
    eh = np.zeros_like(h)
    F = []
    for t in range(T):
        f = _forward(B, obs[t], h, eh)
        f["h"], f["eh"] = h, eh
        F.append(f)
        ended, frozen = ((done[t] == 1) | (done[t] == 2))[:, None], (done[t] == 4)[:, None]
        h, eh = np.where(frozen, h, f["hn"]), np.where(frozen, eh, f["ehn"])
        h, eh = np.where(ended, h0, h), np.where(ended, 0.0, eh)
    # ---- backward ----
    npad = 64 * waves
    acc = {k: [np.zeros(s) for _ in range(3)] for k, s in (("W0", (waves, 16, 23)), ("Wi", (waves, 48, 16)), ("Wh", (waves, 48, 16)),
                                                             ("W2", (waves, 4, 16)))}          # sum, error terms, magnitudes

    def outer(name, d, ed, v, ev):
        d, ed, v, ev = (_pad(a, npad).reshape(waves, 64, -1) for a in (d, ed, v, ev))
        S, E, M = acc[name]
        S += np.einsum("wer,wec->wrc", d, v)
        E += np.einsum("wer,wec->wrc", np.abs(d), ev) + np.einsum("wer,wec->wrc", ed, np.abs(v) + ev)
        M += np.einsum("wer,wec->wrc", np.abs(d), np.abs(v))

    lanes = {k: ([], []) for k in ("br", "bz", "bni", "bnh", "b2", "h0")}

    def lane(name, v, e):
        lanes[name][0].append(_pad(v, npad))
        lanes[name][1].append(_pad(e, npad))

    carry, ecarry = np.zeros((N, 16)), np.zeros((N, 16))
    zero16 = np.zeros((N, 16))
    for t in range(T - 1, -1, -1):
        f = F[t]
        ended, frozen = ((done[t] == 1) | (done[t] == 2))[:, None], (done[t] == 4)[:, None]
        lane("h0", np.where(ended, carry, 0.0), np.where(ended, ecarry, 0.0))
        carry, ecarry = np.where(ended, 0.0, carry), np.where(ended, 0.0, ecarry)
        din, edin = np.where(frozen, 0.0, carry), np.where(frozen, 0.0, ecarry)
        pas, epas = np.where(frozen, carry, 0.0), np.where(frozen, ecarry, 0.0)
        da = dact[t]
        dh, edh = _opened(W2T, din, edin, da, np.zeros_like(da))
        one = np.ones_like(f["z"])
        omz, e_omz = _sub(one, 0.0, f["z"], f["ez"])
        hmn, e_hmn = _sub(f["h"], f["eh"], f["n"], f["en"])
        nsq, e_nsq = _mul(f["n"], f["en"], f["n"], f["en"])
        omn, e_omn = _sub(one, 0.0, nsq, e_nsq)
        omr, e_omr = _sub(one, 0.0, f["r"], f["er"])
        rr1, e_rr1 = _mul(f["r"], f["er"], omr, e_omr)
        zz1, e_zz1 = _mul(f["z"], f["ez"], omz, e_omz)
        dn, e_dn = _mul(dh, edh, omz, e_omz)
        dz, e_dz = _mul(dh, edh, hmn, e_hmn)
        dhd, e_dhd = _mul(dh, edh, f["z"], f["ez"])
        du, e_du = _mul(dn, e_dn, omn, e_omn)
        tt, e_tt = _mul(du, e_du, f["c"], f["ec"])
        dPr, e_dPr = _mul(tt, e_tt, rr1, e_rr1)
        dPz, e_dPz = _mul(dz, e_dz, zz1, e_zz1)
        dGnh, e_dGnh = _mul(du, e_du, f["r"], f["er"])
        # an env that receives nothing at this step contributes exact zeros in the kernel (:186-210) as in float64
        quiet = ~(da.any(axis=1) | din.any(axis=1) | (edin > 0).any(axis=1))[:, None]
        di, edi = np.concatenate([dPr, dPz, du], axis=1), np.concatenate([e_dPr, e_dPz, e_du], axis=1)
        dhh, edhh = np.concatenate([dPr, dPz, dGnh], axis=1), np.concatenate([e_dPr, e_dPz, e_dGnh], axis=1)
        edi, edhh, e_dhd = np.where(quiet, 0.0, edi), np.where(quiet, 0.0, edhh), np.where(quiet, 0.0, e_dhd)
        dy0, Ey = _dense(WiT, np.zeros(16, np.float32), di, edi, PRECISION)
        dhp, Eh = _opened(WhT, dhd, e_dhd, dhh, edhh)
        Ey, Eh = np.where(quiet, 0.0, Ey + FLOOR), np.where(quiet, 0.0, Eh)
        mask = f["p0"] > 0.0
        dp0, edp0 = np.where(mask, dy0, 0.0), np.where(mask, Ey, 0.0)
        x1 = np.concatenate([obs[t], np.ones((N, 1))], axis=1)
        outer("W0", dp0, edp0, x1, np.zeros_like(x1))
        outer("Wi", di, edi, f["y0"], f["ey"])
        outer("Wh", dhh, edhh, f["h"], f["eh"])
        outer("W2", da, np.zeros_like(da), f["hn"], f["ehn"])
        lane("br", dPr, edi[:, 0:16]); lane("bz", dPz, edi[:, 16:32]); lane("bni", du, edi[:, 32:48]); lane("bnh", dGnh, edhh[:, 32:48])
        lane("b2", da, np.zeros_like(da))
        carry = dhp + pas
        e = Eh + epas
        ecarry = np.where(frozen, e + U * (np.abs(carry) + e) + FLOOR, e)
    if start == "initial":
        lane("h0", carry, ecarry)
    # ---- the accumulators ----
    bound = np.zeros(2084)
    g_mfma, g_waves = g_of(64 * T), g_of(waves)

    def block(name):
        S, E, M = acc[name]
        Ew = E + g_mfma * (M + E)
        return Ew.sum(axis=0) + g_waves * (np.abs(S) + Ew).sum(axis=0)

    w0 = block("W0")
    bound[R.OFF["W0"]:R.OFF["B0"]], bound[R.OFF["B0"]:R.OFF["WI"]] = w0[:, :22].ravel(), w0[:, 22]
    bound[R.OFF["WI"]:R.OFF["WH"]], bound[R.OFF["WH"]:R.OFF["BI"]] = block("Wi").ravel(), block("Wh").ravel()
    bound[R.OFF["W2"]:R.OFF["B2"]] = block("W2").ravel()

    def lanes_of(name, first):
        V, E = (np.stack(a) for a in lanes[name])                     # [steps, npad, rows]
        rows = V.shape[2]
        shape = (V.shape[0], waves, 4, 16, rows)                       # env = 64 w + 16 tile + j
        V, E = (a.reshape(shape).transpose(0, 2, 3, 1, 4).reshape(V.shape[0] * 4, 16, waves, rows) for a in (V, E))
        return _sum_levels(V, E, (first, 16, waves))[1]

    br, bz = lanes_of("br", 4 * T), lanes_of("bz", 4 * T)
    bound[R.OFF["BI"]:R.OFF["BH"]] = np.concatenate([br, bz, lanes_of("bni", 4 * T)])
    bound[R.OFF["BH"]:R.OFF["H0"]] = np.concatenate([br, bz, lanes_of("bnh", 4 * T)])
    bound[R.OFF["H0"]:R.OFF["W2"]] = lanes_of("h0", 4 * T + 4)
    bound[R.OFF["B2"]:R.OFF["END"]] = lanes_of("b2", 4 * T)
    return g, gh, bound + FLOOR, (None if start == "initial" else ecarry + FLOOR)


# ---------------------------------------------------------------------------- the kernel's arithmetic in NumPy float32 ---
_f32, _f64 = np.float32, np.float64
_GK = [[s, 4 + s, 8 + s, 12 + s] for s in range(4)]                       # the GRU chains' K-steps (actor_reference.emulate_step)
_GT = [[16 * g + 4 * q + r for q in range(4)] for g in range(3) for r in range(4)]   # the transposed chains' (rq_pack.cpp:66-77)


class _Images:
    """the fp32 operand image as rq_pack.cpp packs it (gate rows pre-scaled) and the transposed, unscaled one"""

    def __init__(self, w32):
        B = blocks(w32)
        k = np.concatenate([np.full(32, K_SIG, _f32), np.full(16, K_TANH, _f32)])
        self.B = B
        self.Wi, self.Wh = (k[:, None] * B["Wi"]).astype(_f32), (k[:, None] * B["Wh"]).astype(_f32)
        self.br = (K_SIG * (B["bi"][0:16] + B["bh"][0:16]).astype(_f32)).astype(_f32)
        self.bz = (K_SIG * (B["bi"][16:32] + B["bh"][16:32]).astype(_f32)).astype(_f32)
        self.bni, self.bnh = (K_TANH * B["bi"][32:]).astype(_f32), (K_TANH * B["bh"][32:]).astype(_f32)
        self.W24 = np.concatenate([B["W0"], B["b0"][:, None], np.zeros((16, 1), _f32)], axis=1)
        self.W2T, self.WiT, self.WhT = (np.ascontiguousarray(B[k].T) for k in ("W2", "Wi", "Wh"))


def _recompute(I, x24, h, exchange=False):
    """layer_0, the gates' chains and the gates (rq_grad_backward.inc:116-144) -> y0, rr, zz, nn, gnh, hn"""
    y0 = np.maximum(_chain_f32(I.W24, x24, np.zeros(16, _f32), [list(range(4 * s, 4 * s + 4)) for s in range(6)]), _f32(0))
    hy, both = np.concatenate([h, y0], axis=1), _GK + [[16 + i for i in g] for g in _GK]
    gr = _chain_f32(np.concatenate([I.Wh[0:16], I.Wi[0:16]], axis=1), hy, I.br, both)
    gz = _chain_f32(np.concatenate([I.Wh[16:32], I.Wi[16:32]], axis=1), hy, I.bz, both)
    gni, gnh = _chain_f32(I.Wi[32:], y0, I.bni, _GK), _chain_f32(I.Wh[32:], h, I.bnh, _GK)
    if exchange:
        gr, gz = gz, gr
    one, two = _f32(1.0), _f32(2.0)
    with np.errstate(over="ignore", invalid="ignore"):
        rr = (one / (one + np.exp2(gr))).astype(_f32)
        zz = (one / (one + np.exp2(gz))).astype(_f32)
        arg = _fma(rr, gnh, gni)
        nn = _fma(np.full_like(arg, two), (one / (one + np.exp2(arg))).astype(_f32), np.full_like(arg, -one))
    hn = _fma(zz, (h - nn).astype(_f32), nn)
    return y0, rr, zz, nn, gnh, hn


def emulate_backward(w32, obs, done, dact, start, h_start, alter=None):
    """-> (g [2084] float32, gh [N, 16] float32 or None): k_policy_grad_forward's saved states, k_policy_grad_backward and
    k_policy_grad_reduce operation by operation (module docstring).  ``alter``: one of ``ALTERATIONS``, a deliberate mistake in the
    backward - r and z rows exchanged, kInvT halved, dGnh = du without r, 1 - n for 1 - n^2, the ReLU mask dropped, an episode end
    that does not cut the carry, a frozen step treated as a running one."""
    assert alter is None or alter in ALTERATIONS, alter
    I = _Images(np.asarray(w32, _f32))
    obs, done, dact = np.asarray(obs, _f32)[:, :, :22], np.asarray(done), np.asarray(dact, _f32)
    T, N = done.shape
    waves = (N + 63) // 64
    npad = 64 * waves
    live = np.arange(npad) < N

    def padded(a):
        out = np.zeros((npad,) + a.shape[1:], _f32)
        out[:N] = a
        return out

    h = np.tile(I.B["h0"], (N, 1)) if start == "initial" else np.asarray(h_start, _f32).reshape(N, 16)
    saved, x24s = [], []
    for t in range(T):                                                     # the forward: the state entering every step
        x24 = np.concatenate([obs[t], np.ones((N, 1), _f32), np.zeros((N, 1), _f32)], axis=1)
        hn = _recompute(I, x24, h)[5]
        saved.append(h)
        x24s.append(x24)
        ended, frozen = ((done[t] == 1) | (done[t] == 2))[:, None], (done[t] == 4)[:, None]
        h = np.where(ended, I.B["h0"], np.where(frozen, h, hn)).astype(_f32)
    one = _f32(1.0)
    kInvT = _f32(one / _f32(-2.8853900817779268))
    if alter == "kinvt_halved":
        kInvT = _f32(kInvT * _f32(0.5))
    aWi, aWh = np.zeros((waves, 48, 16), _f32), np.zeros((waves, 48, 16), _f32)
    aW0, aW2 = np.zeros((waves, 16, 24), _f32), np.zeros((waves, 4, 16), _f32)
    names = ("br", "bz", "bni", "bnh", "h0")
    lanes = {k: np.zeros((waves, 16, 16), _f32) for k in names}           # [wave, j, row]
    lane_b2 = np.zeros((waves, 16, 4), _f32)
    dc = np.zeros((npad, 16), _f32)
    tiles = lambda a: a.reshape(waves, 4, 16, -1)                           # env = 64 w + 16 tile + j

    def mfma_outer(accu, a, b, t, u):
        a4, b4 = tiles(a)[:, t, 4 * u:4 * u + 4].astype(_f64), tiles(b)[:, t, 4 * u:4 * u + 4].astype(_f64)
        return (accu.astype(_f64) + np.einsum("wer,wec->wrc", a4, b4)).astype(_f32)

    for s in range(T - 1, -1, -1):
        x24, hp = padded(x24s[s]), padded(saved[s])
        y0, rr, zz, nn, gnh, hn = _recompute(I, x24, hp, exchange=alter == "rz_exchanged")
        d = np.zeros(npad, np.uint8)
        d[:N] = done[s]
        ended, frozen = ((d == 1) | (d == 2))[:, None], (d == 4)[:, None]
        if alter == "end_keeps_carry":
            ended = np.zeros_like(ended)
        if alter == "frozen_runs":
            frozen = np.zeros_like(frozen)
        da = padded(dact[s])
        to_h0 = np.where(ended, dc, _f32(0))
        dc = np.where(ended, _f32(0), dc)
        din, pas = np.where(frozen, _f32(0), dc), np.where(frozen, dc, _f32(0))
        quiet = ~((da != 0).any(axis=1) | (din != 0).any(axis=1))[:, None] | ~live[:, None]
        dh = _chain_f32(I.W2T, da, din, [[0, 1, 2, 3]])
        dn = (dh * (one - zz)).astype(_f32)
        dz = (dh * (hp - nn).astype(_f32)).astype(_f32)
        dhd = (dh * zz).astype(_f32)
        fac = (one - nn).astype(_f32) if alter == "one_minus_n" else (one - (nn * nn).astype(_f32)).astype(_f32)
        du = (dn * fac).astype(_f32)
        dPr = ((du * (gnh * kInvT).astype(_f32)).astype(_f32) * (rr * (one - rr).astype(_f32)).astype(_f32)).astype(_f32)
        dPz = (dz * (zz * (one - zz).astype(_f32)).astype(_f32)).astype(_f32)
        dGni = du
        dGnh = du if alter == "dgnh_without_r" else (du * rr).astype(_f32)
        z16 = _f32(0)
        dPr, dPz, dGni, dGnh, dhd = (np.where(quiet, z16, a) for a in (dPr, dPz, dGni, dGnh, dhd))
        y0, hp, hn, x24 = (np.where(quiet, z16, a) for a in (y0, hp, hn, x24))
        di, dhh = np.concatenate([dPr, dPz, dGni], axis=1), np.concatenate([dPr, dPz, dGnh], axis=1)
        dy0 = _chain_f32(I.WiT, di, np.zeros(16, _f32), _GT)
        dhp = _chain_f32(I.WhT, dhh, dhd, _GT)
        dp0 = dy0 if alter == "relu_mask_dropped" else np.where(y0 > 0, dy0, z16)
        dc = (dhp + pas).astype(_f32)
        for t in range(4):                                                 # the kernel's order: step, tile, K-step
            for k, v in (("h0", to_h0), ("br", dPr), ("bz", dPz), ("bni", dGni), ("bnh", dGnh)):
                lanes[k] = (lanes[k] + tiles(v)[:, t]).astype(_f32)
            lane_b2 = (lane_b2 + tiles(da)[:, t]).astype(_f32)
            for u in range(4):
                aWi, aWh = mfma_outer(aWi, di, y0, t, u), mfma_outer(aWh, dhh, hp, t, u)
                aW0, aW2 = mfma_outer(aW0, dp0, x24, t, u), mfma_outer(aW2, da, hn, t, u)
    gh = None
    if start == "initial":
        for t in range(4):
            lanes["h0"] = (lanes["h0"] + tiles(dc)[:, t]).astype(_f32)
    else:
        gh = dc[:N]

    def fold(a):                                                           # [wave, j, rows]: lanes j ascending, then waves ascending
        out = np.zeros((waves, a.shape[2]), _f32)
        for j in range(16):
            out = (out + a[:, j]).astype(_f32)
        return reduce_waves(out)

    def reduce_waves(p):
        out = np.zeros(p.shape[1:], _f32)
        for w in range(waves):
            out = (out + p[w]).astype(_f32)
        return out

    g = np.zeros(2084, _f32)
    w0 = reduce_waves(aW0)
    g[R.OFF["W0"]:R.OFF["B0"]], g[R.OFF["B0"]:R.OFF["WI"]] = w0[:, :22].ravel(), w0[:, 22]
    g[R.OFF["WI"]:R.OFF["WH"]], g[R.OFF["WH"]:R.OFF["BI"]] = reduce_waves(aWi).ravel(), reduce_waves(aWh).ravel()
    br, bz = fold(lanes["br"]), fold(lanes["bz"])
    g[R.OFF["BI"]:R.OFF["BH"]] = np.concatenate([br, bz, fold(lanes["bni"])])
    g[R.OFF["BH"]:R.OFF["H0"]] = np.concatenate([br, bz, fold(lanes["bnh"])])
    g[R.OFF["H0"]:R.OFF["W2"]] = fold(lanes["h0"])
    g[R.OFF["W2"]:R.OFF["B2"]] = reduce_waves(aW2).ravel()
    g[R.OFF["B2"]:R.OFF["END"]] = fold(lane_b2)
    return g, gh


# ---------------------------------------------------------------------------- the synthetic cases ---
_CODES = np.asarray([0, 1, 2, 4, 0, 0, 4, 0, 2, 0, 0, 1, 0, 4, 0, 0], np.uint8)
MAX_QUIETED = 0.02


def case(wf, xf, n, T, seed=0):
    """One window of the weight family ``wf`` on the input family ``xf`` -> dict(w [2084] f32, obs [T, n, 22] f32, h [n, 16] f32,
    done [T, n] u8, dact [T, n, 4] f32, quieted [n] bool).  Step t's observations are ``actor_reference.inputs(xf, n, seed + t)``'s,
    the entering state is that of step 0; every 16-env tile holds the done codes 0, 1, 2 and 4 at every step, and an env moves
    through them from step to step; dact is N(0, 1) and 0 on every step of an env some step of which lies near a ReLU kink
    (``quieted``; ``gain_reference.near_kink``), so that kernel and reference agree on the mask everywhere else."""
    import actor_reference as AR
    assert T <= 3 and 0 <= seed and seed + T <= 3, "the kink cap is checked for seeds 0 .. 2"
    w = AR.weights(wf)
    xs = [AR.inputs(xf, n, seed + t) for t in range(T)]
    obs = np.stack([np.ascontiguousarray(x[:, :22]) for x, _ in xs])
    h = xs[0][1]
    e = np.arange(n)
    done = np.stack([_CODES[(e + 5 * t) % 16] for t in range(T)])
    rng = np.random.default_rng([seed, n, T])
    dact = rng.standard_normal((T, n, 4)).astype(np.float32)
    quieted = np.zeros(n, bool)
    for t in range(T):
        quieted |= GR.near_kink(w, obs[t])
    dact[:, quieted] = 0.0
    return dict(w=w, obs=obs, h=h, done=done, dact=dact, quieted=quieted)
