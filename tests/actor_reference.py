"""Float64 reference of ONE step of the student actor (Dense 22 -> 16 ReLU, GRU 16, Dense 16 -> 4) with an element-wise
error bound per kernel precision, NumPy emulations of the three operand images, and the weight / input families the
actor is held to beyond the shipped checkpoint.

``step_bound`` evaluates the step in float64 from the float32 weights, teacher-forced from the hidden state it is given,
and carries next to every activation a bound ``e`` on how far the chosen implementation's value may lie from it, exactly
as ``teacher_reference.forward_bound`` does for the teacher bank.  For a contraction s = W v + b with K inputs whose
operands lie within e of v:

    E_s = |W| e + g_op (|W| (|v| + e) + |b| [bias rounded]) + g (|W| (|v| + e) + |b|)
          + alpha (sum_k |W_ik| + sum_k (|v_k| + e_k))

g_op, g_acc, alpha and [bias rounded] are ``teacher_reference._constants`` (derived in that module's docstring: u = 2^-24;
one rounding of the running sum per addend; gate rows pre-scaled by k in fp32, 2 u; bf16 operands 2^-8 + 2^-17 per
product; the f16 hi / lo split 3 * 2^-22 relative and 2^-25 absolute with three products per weight), and
g = g_acc / (1 - g_acc) (n roundings compound to at most n u / (1 - n u)).  What the actor adds to the teacher model, with
the code line that sets each constant (rq_device_math.hpp unless named otherwise):

* Layer 0 (K = 22, ReLU).  The bias rides K-slot 22 against the constant 1 in all three images (rq_pack.cpp:38, :112,
  :184; the constant: ActorF32T::load_impl ``wr[22] = 1.0f``, ActorBF16::run / ActorF16X2::step ``f1 == 22 ? 1.0f``):
  ``first = True`` - in bf16 and f16x2 it is rounded like a weight, and it is one of the K + 1 addends.
* r and z gates.  s = W_i y0 + W_h h + (b_i + b_h): ONE accumulator chain of 32 products opened by the bias as the C
  operand (recurrent_tile / run: "bias, W_h h (k = 0..15), W_i y0 (k = 0..15)"; bf16 / f16x2: one K = 32 MFMA per piece on
  the tuple [y0 | h]), so K = 32 with 33 addends (f16x2: 97).  The packers form k * (b_i + b_h) (rq_pack.cpp:52-53, :128,
  :197): the sum is rounded once in fp32 (u |b_i + b_h|) before the scaling, whose 2 u the pre-scale term carries.  The
  rows are scaled BEFORE the bf16 / f16 rounding (rq_pack.cpp:118, :187): g_op and alpha apply to the scaled weight, which
  in unscaled units is the same relative error and an absolute floor shrunk by |k| > 1.  The biases stay fp32 C operands.
* sigma.  gru_gates_prescaled (:643-644) forms rcp(1 + exp2(a)) on the accumulator a.  v_exp_f32 and v_rcp_f32 are
  accurate to 1 ulp (2 u relative) and the add rounds once (u): t = exp2(a) is within 2 u, the denominator 1 + t within
  2 u t / (1 + t) + u <= 3 u, the reciprocal adds 2 u: 5 u relative to sigma <= 1, tau_sigma = 5 u absolute (second-order
  terms below 2^-44; an overflowing t gives rcp(inf) = 0 and a flushed one gives 1, both within 2^-126 of the truth).
  The oracle calls 1 / (1 + expf(-s)) (raptor_oracle.c:127): glibc's expf is within 1 ulp (2 u), the add and the division
  round once each: tau_sigma = 4 u.  The gate's error is max(sigma(s + E) - sigma(s), sigma(s) - sigma(s - E)) <= E / 4
  plus tau_sigma.
* n gate.  p = W_i,n y0 + b_i,n and q = W_h,n h + b_h,n are chains of their own (K = 16, 17 addends; f16x2: 49), the
  argument is fma(r, q, p) (:645; raptor_oracle.c:149), one rounding: with E_a = E_p + (|r| + e_r) E_q + e_r |q|,
  E_arg = E_a + u (|arg| + E_a).  tanh costs tau = 11 u on the device (2 rcp(1 + exp2) - 1, :646, derived in
  teacher_reference) and 2^-22 in the oracle (tanhf).
* State update.  h' = fma(z, h - n, n) with the difference rounded first (:647; raptor_oracle.c:150).  With the computed
  n~ = n + dn, z~ = z + dz and d~ = (h - n~)(1 + e1):  n~ + z~ d~ - h' = dn (1 - z) + z e1 (h - n~) + dz d~, so with
  D = |h - n| + e_n the error before the fma's own rounding is T = e_n |1 - z| + (u |z| + e_z (1 + u)) D, and
  e_h' = T + u (|h'| + T).  The hidden state enters the blend as the fp32 number it is in every build (hQ).
* Output layer (K = 16, identity).  b2 is an fp32 C operand / the opening addend (rq_pack.cpp:57, :133, :202).  The fp32
  build adds its 17 addends as four chains of four packed fmas and two levels of adds (ActorF32T::run layer_2: at most
  six roundings on any addend, covered by the 17 of the sequential model); the 16-bit builds round or split h' as the
  B operand (ActorBF16::run ``pk(hQ...)``, ActorF16X2::step ``split2(hQ...)``).
* f16x2 range.  Observations and layer 0's output are clamped to +-65 504 before the split (split2_sat, clampf in
  ActorF16X2::step): an operand beyond that makes the bound infinite (the kernel is finite there, not accurate).
* "oracle".  Sequential fmaf opened by the bias (K roundings, no pre-scale, ``_constants(\"oracle\", ...)``); the r / z
  pre-activation is gi + gh, two chains of 16 and one add (17 roundings on any addend <= the 32 charged).
* The optional stages.  Standardize is folded into layer 0 on the host (rq_capi_policy.cpp policy_upload):
  ``fold_bound`` derives what that costs.  The squash is fmaf(2, rcp(1 + exp2(k a)), -1) (squash_action): the product
  k a costs 2 u |a| on the argument (k's own rounding and the product's), the tanh tau = 11 u.

Nothing here is fitted to an observed error.
"""
import os

import numpy as np

from teacher_reference import F16_MAX, K_TANH, U, _constants, split_f16, to_bf16

K_SIG = np.float32(-1.4426950408889634)           # -log2 e, as the packers write it (rq_pack.cpp:42)
N_WEIGHTS = 2084
BLOCKS = {"W0": (0, 352), "b0": (352, 368), "Wi": (368, 1136), "Wh": (1136, 1904), "bi": (1904, 1952), "bh": (1952, 2000),
          "h0": (2000, 2016), "W2": (2016, 2080), "b2": (2080, 2084)}
PRECISIONS = ("oracle", "fp32", "bf16", "f16x2")
TAU_TANH = {"oracle": 2.0 ** -22}
TAU_SIGMA = {"oracle": 4 * U + 2.0 ** -44}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def blocks(w, dtype=np.float32):
    """flat [2084] -> dict of the nine blocks, matrices as [out, in]"""
    w = np.asarray(w, dtype)
    assert w.shape == (N_WEIGHTS,), w.shape
    b = {k: w[a:z] for k, (a, z) in BLOCKS.items()}
    b["W0"], b["Wi"], b["Wh"], b["W2"] = b["W0"].reshape(16, 22), b["Wi"].reshape(48, 16), b["Wh"].reshape(48, 16), b["W2"].reshape(4, 16)
    return b


def _sigma(v):
    return 0.5 * (1.0 + np.tanh(0.5 * v))


def _step_of(f, z, E, lipschitz):
    """error of the monotone f at a pre-activation within E of z: the larger of the two steps, at most lipschitz * E"""
    v = f(z)
    with np.errstate(invalid="ignore"):
        step = np.maximum(f(z + E) - v, v - f(z - E))
    return np.where(np.isinf(E), np.inf, np.minimum(step, lipschitz * E))


def _dense(W32, b32, v, e, precision, first=False, scaled=False, scale=1.0, bias_sum=False):
    """s = W v + b in float64 and its bound E (module docstring).  ``scale``: |k| of the rows' pre-scale (the f16 range is
    checked on the scaled weight); ``bias_sum``: b is a sum the packer rounds once."""
    W, b = np.asarray(W32, np.float64), np.asarray(b32, np.float64)
    K = W.shape[1]
    g_op, g_acc, alpha, bias_rounded = _constants(precision, K, first, scaled)
    g = g_acc / (1.0 - g_acc)
    A, vp = np.abs(W), np.abs(v) + e
    s = v @ W.T + b
    mag = vp @ A.T
    E = e @ A.T + g_op * (mag + (np.abs(b) if bias_rounded else 0.0)) + g * (mag + np.abs(b))
    if bias_sum:
        E = E + U * np.abs(b)
    if alpha:
        E = E + alpha * (A.sum(axis=1) + vp.sum(axis=1, keepdims=True) + (1.0 if bias_rounded else 0.0)) + (K + 1) * 2.0 ** -48
    if precision == "f16x2":
        out = (vp > F16_MAX).any(axis=1, keepdims=True)
        big = (A * scale > F16_MAX).any(axis=1) | ((np.abs(b) * scale > F16_MAX) & bias_rounded)
        E = np.where(out | big[None, :], np.inf, E)
    return s, E


def step_bound(w32, x32, h32, precision, e_x=None, e_z0=None, squash=False):
    """One teacher-forced step: w32 [2084], x32 [N, 22], h32 [N, 16] (None: the weights' initial hidden state)
    -> (act [N, 4], hid [N, 16], bound_act, bound_hid), all float64.  ``e_x`` [N, 22]: a bound on the input's own error,
    ``e_z0`` [N, 16]: one added to layer 0's pre-activation (``fold_bound``); ``squash``: tanh on the action."""
    assert precision in PRECISIONS, precision
    B = blocks(w32)
    x = np.asarray(x32, np.float64)[:, :22]
    n = x.shape[0]
    h = np.tile(B["h0"].astype(np.float64), (n, 1)) if h32 is None else np.asarray(h32, np.float64)
    ex = np.zeros_like(x) if e_x is None else np.asarray(e_x, np.float64)
    tau_t = TAU_TANH.get(precision, 11 * U)
    tau_s = TAU_SIGMA.get(precision, 5 * U + 2.0 ** -44)
    # layer 0
    z0, E0 = _dense(B["W0"], B["b0"], x, ex, precision, first=True)
    if e_z0 is not None:
        E0 = E0 + e_z0
    relu = lambda v: np.maximum(v, 0.0)
    y0, ey = relu(z0), _step_of(relu, z0, E0, 1.0)
    # r and z: one chain over [y0 | h]
    v, ev = np.concatenate([y0, h], axis=1), np.concatenate([ey, np.zeros_like(h)], axis=1)
    gate, eg = [], []
    for m in range(2):
        rows = slice(16 * m, 16 * m + 16)
        W = np.concatenate([B["Wi"][rows], B["Wh"][rows]], axis=1)
        b = B["bi"][rows].astype(np.float64) + B["bh"][rows].astype(np.float64)
        s, E = _dense(W, b, v, ev, precision, scaled=precision != "oracle", scale=float(-K_SIG), bias_sum=True)
        gate.append(_sigma(s))
        eg.append(_step_of(_sigma, s, E, 0.25) + tau_s)
    (r, z), (er, ez) = gate, eg
    # n
    rows = slice(32, 48)
    p, Ep = _dense(B["Wi"][rows], B["bi"][rows], y0, ey, precision, scaled=precision != "oracle", scale=float(-K_TANH))
    q, Eq = _dense(B["Wh"][rows], B["bh"][rows], h, np.zeros_like(h), precision, scaled=precision != "oracle", scale=float(-K_TANH))
    arg = p + r * q
    Ea = Ep + (np.abs(r) + er) * Eq + er * np.abs(q)
    Ea = Ea + U * (np.abs(arg) + Ea)
    nn, en = np.tanh(arg), _step_of(np.tanh, arg, Ea, 1.0) + tau_t
    # h' = fma(z, h - n, n)
    hid = nn + z * (h - nn)
    D = np.abs(h - nn) + en
    T = en * np.abs(1.0 - z) + (U * np.abs(z) + ez * (1.0 + U)) * D
    eh = T + U * (np.abs(hid) + T)
    # output
    act, Eo = _dense(B["W2"], B["b2"], hid, eh, precision)
    if squash:
        Eo = Eo + 2 * U * (np.abs(act) + Eo)
        act, Eo = np.tanh(act), _step_of(np.tanh, act, Eo, 1.0) + tau_t
    return act, hid, Eo, eh


def fold_bound(w32, mean, std, x32, precision):
    """The Standardize stage as policy_upload folds it into layer 0 (rq_capi_policy.cpp: std_inv = 1 / std in
    rq_policy_set_standardize; w' = W0 * std_inv, shift += w' * mean over k, b0' = b0 - shift):
    -> (x_std [N, 22] float64 = (x - mean) / std, e_z0 [N, 16]) for ``step_bound(w32, x_std, ..., e_z0=e_z0)``.
    The kernel contracts w' with the RAW observation and adds b0', so its roundings are relative to |w'| |x| and |b0'|,
    not to the standardised magnitudes step_bound sees:
      * w'_k = W0_k / std_k (1 + d), |d| <= 2 u + u^2 < 3 u (the reciprocal and the product round once each);
      * shift: 22 products and 22 additions, any addend passes through at most 23 roundings: g_23 sum_k |w'_k mean_k|;
        the subtraction rounds once more: u |b0'|;
      * the kernel's own operand, accumulation and floor terms on the folded operands: (g_op + g) (sum |w'_k| |x_k| + |b0'|)
        + alpha (sum |w'_k| + sum |x_k| + 1), the constants of layer 0 in ``step_bound`` (which charges them once more on
        the standardised magnitudes: a looser bound, still one)."""
    B = blocks(w32)
    W0, b0 = B["W0"].astype(np.float64), B["b0"].astype(np.float64)
    m, s = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    x = np.asarray(x32, np.float64)[:, :22]
    Wf = np.abs(W0) / s
    sh = Wf @ np.abs(m)
    b0f = np.abs(b0) + sh                                     # >= |b0'|
    g23 = 23 * U / (1 - 23 * U)
    fold = 3 * U * (np.abs(x) @ Wf.T + sh) + g23 * sh + U * b0f
    g_op, g_acc, alpha, _ = _constants(precision, 22, True, False)
    g = g_acc / (1 - g_acc)
    own = (g_op + g) * (np.abs(x) @ Wf.T * (1 + 3 * U) + b0f)
    if alpha:
        own = own + alpha * (Wf.sum(axis=1) * (1 + 3 * U) + np.abs(x).sum(axis=1, keepdims=True) + 1.0) + 23 * 2.0 ** -48
    if precision == "f16x2":
        own = np.where((np.abs(x) > F16_MAX).any(axis=1, keepdims=True) | (Wf > F16_MAX).any(axis=1)[None, :] | (b0f > F16_MAX)[None, :], np.inf, own)
    return (x - m) / s, fold + own


def ratio(got, ref, bound):
    """|got - ref| / bound element-wise: 0 where both are 0, inf for a non-finite value, a zero or an infinite bound"""
    g = np.asarray(got, np.float64)
    d = np.abs(g - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / bound)
    return np.where(np.isfinite(g) & np.isfinite(bound) & ~np.isnan(r), r, np.inf)


# ---------------------------------------------------------------------------- emulations (NumPy) ---
def _bf16(x):
    """round-to-nearest-even fp32 -> bf16 -> fp32 (numpy)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32)


def _actor_bf16_model(w, x, h):
    """The bf16 kernel's arithmetic in numpy: operands rounded to bf16, fp32 accumulate, fp32 gates."""
    W0, b0 = w[0:352].reshape(16, 22), w[352:368]
    Wi, Wh = w[368:1136].reshape(48, 16), w[1136:1904].reshape(48, 16)
    bi, bh, W2, b2 = w[1904:1952], w[1952:2000], w[2016:2080].reshape(4, 16), w[2080:2084]
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    y0 = np.maximum(_bf16(x[:, :22]) @ _bf16(W0).T + _bf16(b0), 0).astype(np.float32)
    # the gate rows are pre-scaled (r, z by -log2 e, n by -2 log2 e) BEFORE they are rounded to bf16 (pack_policy_bf16)
    k = np.concatenate([np.full(32, -1.4426950408889634, np.float32), np.full(16, -2.8853900817779268, np.float32)])[:, None]
    gi, gh = (_bf16(y0) @ _bf16(k * Wi).T) / k.T, (_bf16(h) @ _bf16(k * Wh).T) / k.T
    r = sig(gi[:, :16] + gh[:, :16] + bi[:16] + bh[:16])
    z = sig(gi[:, 16:32] + gh[:, 16:32] + bi[16:32] + bh[16:32])
    n = np.tanh(gi[:, 32:] + bi[32:] + r * (gh[:, 32:] + bh[32:]))
    hn = ((1 - z) * n + z * h).astype(np.float32)
    return (_bf16(hn) @ _bf16(W2).T + b2).astype(np.float32), hn


_f32, _f64 = np.float32, np.float64


def _fma(a, b, c):
    return (a.astype(_f64) * b.astype(_f64) + c.astype(_f64)).astype(_f32)


def _chain_f32(Ws, X, c, groups):
    """an fp32 MFMA chain: the accumulator opens with c and takes one K-step (four products) at a time"""
    acc = np.broadcast_to(np.asarray(c, _f32), (X.shape[0], Ws.shape[0])).astype(_f32)
    for g in groups:
        acc = (acc.astype(_f64) + X[:, g].astype(_f64) @ Ws[:, g].astype(_f64).T).astype(_f32)
    return acc


def _contract16(Ws, X, c, precision, drop_lo_hi, saturate):
    """one K <= 32 contraction of a 16-bit build: operands rounded (bf16) or split (f16x2: hi.hi + hi(W) lo(x) + lo(W) hi(x)),
    exact products, one rounding to fp32"""
    if precision == "bf16":
        s = to_bf16(X).astype(_f64) @ to_bf16(Ws).astype(_f64).T
    else:
        xh, xl = split_f16(X, saturate=saturate)
        wh, wl = split_f16(Ws)
        with np.errstate(invalid="ignore", over="ignore"):
            s = xh @ wh.T + xl @ wh.T
            if not drop_lo_hi:
                s = s + xh @ wl.T
    with np.errstate(invalid="ignore", over="ignore"):
        return (s + np.asarray(c, _f64)).astype(_f32)


def _gates(gr, gz, gni, gnh, h):
    """gru_gates_prescaled in fp32, operation by operation"""
    one, two = _f32(1.0), _f32(2.0)
    with np.errstate(over="ignore", invalid="ignore"):
        rr = (one / (one + np.exp2(gr))).astype(_f32)
        zz = (one / (one + np.exp2(gz))).astype(_f32)
        arg = _fma(rr, gnh, gni)
        nn = _fma(np.full_like(arg, two), (one / (one + np.exp2(arg))).astype(_f32), np.full_like(arg, -one))
        return _fma(zz, (h - nn).astype(_f32), nn)


def emulate_step(w32, x32, h32, precision, drop_lo_hi=False):
    """What the kernel of ``precision`` ("fp32", "bf16", "f16x2") does with its operands, as rq_pack.cpp packs and
    rq_device_math.hpp contracts them -> (act [N, 4], hid [N, 16]) float32.  fp32 adds in MFMA order (K in groups of
    four: layer 0 features 4 s .. 4 s + 3, the GRU chains features {s, 4 + s, 8 + s, 12 + s}, W_h h before W_i y0).
    ``drop_lo_hi``: the f16x2 build without its lo(W) hi(x) product (a fault)."""
    B = blocks(w32)
    x = np.ascontiguousarray(np.asarray(x32, _f32)[:, :22])
    n = x.shape[0]
    h = np.tile(B["h0"], (n, 1)) if h32 is None else np.asarray(h32, _f32)
    kS, kT = K_SIG, K_TANH
    k = np.concatenate([np.full(32, kS, _f32), np.full(16, kT, _f32)])
    Wi, Wh = (k[:, None] * B["Wi"]).astype(_f32), (k[:, None] * B["Wh"]).astype(_f32)
    br = (kS * (B["bi"][0:16] + B["bh"][0:16]).astype(_f32)).astype(_f32)
    bz = (kS * (B["bi"][16:32] + B["bh"][16:32]).astype(_f32)).astype(_f32)
    bni, bnh = (kT * B["bi"][32:]).astype(_f32), (kT * B["bh"][32:]).astype(_f32)
    x1 = np.concatenate([x, np.ones((n, 1), _f32)], axis=1)
    W01 = np.concatenate([B["W0"], B["b0"][:, None]], axis=1)
    if precision == "fp32":
        x24, W24 = np.concatenate([x1, np.zeros((n, 1), _f32)], axis=1), np.concatenate([W01, np.zeros((16, 1), _f32)], axis=1)
        y0 = np.maximum(_chain_f32(W24, x24, np.zeros(16, _f32), [list(range(4 * s, 4 * s + 4)) for s in range(6)]), _f32(0))
        gk = [[s, 4 + s, 8 + s, 12 + s] for s in range(4)]
        hy, both = np.concatenate([h, y0], axis=1), gk + [[16 + i for i in g] for g in gk]
        gr = _chain_f32(np.concatenate([Wh[0:16], Wi[0:16]], axis=1), hy, br, both)
        gz = _chain_f32(np.concatenate([Wh[16:32], Wi[16:32]], axis=1), hy, bz, both)
        gni, gnh = _chain_f32(Wi[32:], y0, bni, gk), _chain_f32(Wh[32:], h, bnh, gk)
        hid = _gates(gr, gz, gni, gnh, h)
        parts = []
        for q in range(4):                                    # lane group q: b2 (q == 0) and its four features, packed fmas
            p = np.broadcast_to(B["b2"] if q == 0 else np.zeros(4, _f32), (n, 4)).astype(_f32)
            for r in range(4):
                p = _fma(np.broadcast_to(B["W2"][:, 4 * q + r], (n, 4)), hid[:, 4 * q + r:4 * q + r + 1], p)
            parts.append(p)
        act = ((parts[0] + parts[1]).astype(_f32) + (parts[2] + parts[3]).astype(_f32)).astype(_f32)
        return act, hid
    assert precision in ("bf16", "f16x2"), precision
    con = lambda Ws, X, c, sat=False: _contract16(Ws, X, c, precision, drop_lo_hi, sat)
    z0 = con(W01, x1, 0.0, sat=True)
    if precision == "bf16":
        y0 = np.maximum(to_bf16(z0), _f32(0))                 # rounded, then max(., 0) on the packed pairs: the same value
    else:
        y0 = np.where(np.isnan(z0), _f32(0), np.clip(z0, 0.0, F16_MAX)).astype(_f32)
    yh = np.concatenate([y0, h], axis=1)
    gr = con(np.concatenate([Wi[0:16], Wh[0:16]], axis=1), yh, br)
    gz = con(np.concatenate([Wi[16:32], Wh[16:32]], axis=1), yh, bz)
    gni, gnh = con(Wi[32:], y0, bni), con(Wh[32:], h, bnh)
    hid = _gates(gr, gz, gni, gnh, h)
    return con(B["W2"], hid, B["b2"]), hid


# ---------------------------------------------------------------------------- weights and inputs ---
def shipped():
    w = np.fromfile(os.path.join(ROOT, "raptor_amd", "data", "raptor_policy.bin"), "<f4")
    assert w.size == N_WEIGHTS
    return np.ascontiguousarray(w, np.float32)


def _fresh(rng):
    w = np.zeros(N_WEIGHTS, np.float64)
    for name, fan_in in (("W0", 22), ("Wi", 16), ("Wh", 16), ("W2", 16)):
        a, z = BLOCKS[name]
        w[a:z] = rng.uniform(-1, 1, z - a) / np.sqrt(fan_in)
    for name in ("b0", "bi", "bh", "b2"):
        a, z = BLOCKS[name]
        w[a:z] = rng.uniform(-0.2, 0.2, z - a)
    w[2000:2016] = rng.uniform(-0.3, 0.3, 16)
    return w.astype(np.float32)


WEIGHT_FAMILIES = ("shipped", "perturbed", "fresh", "sat8", "sat64", "tiny", "signed_pos", "signed_neg")


def weights(family, seed=0):
    """One weight vector [2084] float32 of ``family`` (the same for the same seed):
    shipped; perturbed = shipped + N(0, 0.05) with a fresh h0; fresh = uniform +-1 / sqrt(fan_in), biases +-0.2, h0 +-0.3;
    sat8 / sat64 = fresh with the GRU rows and biases x 8 / x 64 (gates deep in saturation: exp2 overflows, rcp(inf));
    tiny = fresh x 2^-10 (f16 lo pieces subnormal); signed_pos / signed_neg = fresh with the three gate-bias blocks of b_i
    at +6 / -6 (r, z and n at either rail)."""
    rng = np.random.default_rng([seed, WEIGHT_FAMILIES.index(family)])
    if family == "shipped":
        return shipped()
    if family == "perturbed":
        w = shipped().astype(np.float64) + rng.normal(0, 0.05, N_WEIGHTS)
        w[2000:2016] = rng.uniform(-0.3, 0.3, 16)
        return w.astype(np.float32)
    w = _fresh(rng)
    if family in ("sat8", "sat64"):
        w[368:2000] *= np.float32(8 if family == "sat8" else 64)
    elif family == "tiny":
        w *= np.float32(2.0 ** -10)
    elif family in ("signed_pos", "signed_neg"):
        w[1904:1952] = 6.0 if family == "signed_pos" else -6.0
    else:
        assert family == "fresh", family
    return w


INPUT_FAMILIES = ("normal", "small", "large", "exact_h", "wide_h", "strided")


def inputs(family, n, seed=0):
    """-> (x [n, 22] or [n, 26] float32, h [n, 16] float32).  normal: N(0, 1), h uniform in (-1, 1); small / large: the
    observation x 2^-10 / x 2^10; exact_h: hidden entries drawn from {0, 1, -1, a uniform one}; wide_h: hidden entries up to
    +-1.5; strided: rows of 26 with NaN in the columns >= 22 (a kernel that reads them poisons its row)."""
    rng = np.random.default_rng([seed, n, INPUT_FAMILIES.index(family)])
    x = rng.standard_normal((n, 22)).astype(np.float32)
    h = rng.uniform(-1, 1, (n, 16)).astype(np.float32)
    if family == "small":
        x *= np.float32(2.0 ** -10)
    elif family == "large":
        x *= np.float32(2.0 ** 10)
    elif family == "exact_h":
        pick = rng.integers(0, 4, (n, 16))
        h = np.choose(pick, [np.zeros_like(h), np.ones_like(h), -np.ones_like(h), h]).astype(np.float32)
    elif family == "wide_h":
        h = rng.uniform(-1.5, 1.5, (n, 16)).astype(np.float32)
    elif family == "strided":
        wide = np.full((n, 26), np.nan, np.float32)
        wide[:, :22] = x
        x = wide
    else:
        assert family in ("normal",), family
    return x, h


ALTERATIONS = tuple(f"swap_{b}" for b in BLOCKS) + ("bias_n_exchanged", "rows_rz_exchanged", "n_prescale_halved")
STRUCTURAL = ALTERATIONS[-3:]


def altered(w32, kind):
    """The weights a subtly wrong packer or kernel would be computing with -> [2084] float32:
    swap_<block>: two neighbouring elements of the block exchanged (the first pair whose values differ by more than a
    thousandth of the block's largest); bias_n_exchanged: b_i,n <-> b_h,n; rows_rz_exchanged: the r and z rows of W_i, W_h,
    b_i, b_h exchanged (two gate images swapped); n_prescale_halved: the n rows and biases x 1/2 (-log2 e where -2 log2 e
    belongs)."""
    w = np.array(w32, np.float32, copy=True)
    if kind.startswith("swap_"):
        a, z = BLOCKS[kind[5:]]
        blk = w[a:z]
        d = np.abs(np.diff(blk))
        i = int(np.argmax(d > 1e-3 * np.abs(blk).max()))
        assert d[i] > 0, kind
        blk[i], blk[i + 1] = blk[i + 1], blk[i]
        return w
    if kind == "bias_n_exchanged":
        w[1936:1952], w[1984:2000] = w32[1984:2000], w32[1936:1952]
        return w
    if kind == "rows_rz_exchanged":
        for base, per in ((368, 16), (1136, 16), (1904, 1), (1952, 1)):
            w[base:base + 16 * per], w[base + 16 * per:base + 32 * per] = w32[base + 16 * per:base + 32 * per], w32[base:base + 16 * per]
        return w
    if kind == "n_prescale_halved":
        for base, per in ((368, 16), (1136, 16), (1904, 1), (1952, 1)):
            w[base + 32 * per:base + 48 * per] *= np.float32(0.5)
        return w
    raise ValueError(kind)
