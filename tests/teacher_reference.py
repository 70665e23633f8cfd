"""Float64 reference of the teacher bank with an element-wise error bound per kernel precision.

``forward_bound`` evaluates a dense stack in float64 from its float32 weights and carries, next to every activation, a bound
``e`` on how far the chosen implementation's value may lie from it.  For a layer z = W h + b with K inputs, where the
implementation's operands lie within e of h:

    E_z = |W| e + g_op (|W| (|h| + e) + |b| [bias rounded]) + g_acc (|W| (|h| + e) + |b|) + alpha (sum_k |W_ik| + sum_k (|h_k| + e_k))
    e'  = max(f(z + E_z) - f(z), f(z) - f(z - E_z)) + tau_act       (f monotone and 1-Lipschitz: e' <= E_z + tau_act)

The constants come from how each implementation handles its operands (rq_teacher.hip header, pack_teacher_f32 /
pack_teacher_16 / pack_teacher_layers in rq_pack.cpp), not from observed errors:

* u = 2^-24, the unit roundoff of fp32 round-to-nearest.
* Accumulation (g_acc): every product or bias added to an fp32 accumulator is taken as one rounding of the running sum
  (the sequential fma model, the worst case of any summation order that rounds once per addition), so n addends cost
  n * u times the sum of their magnitudes.  The kernels add K products + the bias; the split-f16 kernel adds three
  products per weight (hi.hi, hi.lo, lo.hi), 3 K + 1 addends.
* tanh rows are pre-scaled by k = -2 log2 e in fp32 before any other rounding: k itself and k * w each cost one rounding
  (2 u relative on every term, bias included).  The kernel then works in scaled units; the bound is stated in unscaled
  ones, which only loosens the absolute floor below by |k| > 1.
* Layer 1's bias rides in K-slot in_dim with the constant 1 as its B operand: in bf16 and f16x2 it is rounded like a
  weight ([bias rounded]).  The other biases are fp32 C operands.
* bf16 (g_op): both operands rounded to bf16 with RNE, 2^-9 relative each: (1 + 2^-9)^2 - 1 < 2^-8 + 2^-17 per product.
  bf16 shares fp32's exponent range, so there is no absolute floor at the magnitudes tested.
* f16x2 (g_op, alpha): v = hi + lo + d with hi = f16(v), lo = f16(v - hi) (the residual is exact in fp32); |v - hi| <= 2^-11 |v|
  and, lo being f16, |d| <= 2^-22 |v| + 2^-25 (2^-25 = half the f16 subnormal spacing: below |v| ~ 2^-3 the lo piece is
  subnormal).  The product drops lo_v lo_w (|lo| <= 2^-11 |v| + 2^-25) and carries d_v w + v d_w: 3 * 2^-22 relative plus
  2^-25 (|v| + |w|) absolute, second-order terms below 2^-34 relative and 2^-35 absolute.  Valid while every operand lies
  inside the f16 range (|v| <= 65 504); beyond it the bound is infinite (the kernel saturates there: finite, not accurate).
* tanh (tau): the kernel forms 2 rcp(1 + 2^x) - 1.  v_exp_f32 and v_rcp_f32 are accurate to 1 ulp (2^-23 relative) and
  the add is one rounding (2^-24): rcp is within 5 * 2^-24 relative of 1 / (1 + 2^x) <= 1, so 2 rcp is within 10 * 2^-24
  absolute; the subtraction of 1 cancels (no relative bound near 0) and the fma rounds once more (2^-24 |tanh| <= 2^-24):
  tau = 11 * 2^-24 absolute.  The C oracle calls tanhf (glibc: at most 2 ulp): tau = 2^-22.
* The reference's own float64 sums cost (K + 1) * 2^-53 relative, added to g_acc.
"""
import numpy as np

U = 2.0 ** -24
K_TANH = np.float32(-2.8853900817779268)          # -2 log2 e, as the packers write it
F16_MAX = 65504.0
ACT_CODE = {"identity": 0, "relu": 1, "tanh": 2}
PRECISIONS = ("oracle", "fp32", "bf16", "f16x2")


def unpack(block, in_dim, widths):
    """One teacher's flat [W1 | b1 | ... | W_out | b_out] (float32) -> [(W [out, in], b [out])] as float32."""
    layers, at, prev = [], 0, int(in_dim)
    for h in list(widths) + [4]:
        W = np.asarray(block[at:at + h * prev], np.float32).reshape(h, prev)
        at += h * prev
        b = np.asarray(block[at:at + h], np.float32)
        at += h
        layers.append((W, b))
        prev = h
    assert at == len(block), (at, len(block))
    return layers


def _constants(precision, K, first, tanh_row):
    """-> (g_op, g_acc, alpha, bias_rounded) of one layer with K inputs (see the module docstring)."""
    prescale = 2 * U if tanh_row else 0.0
    ref64 = (K + 1) * 2.0 ** -53
    if precision == "oracle":                       # acc = b; acc = fma(W, x, acc) K times: K roundings, no pre-scale
        return 0.0, K * U + ref64, 0.0, False
    n_add = K + 1                                   # K products + the bias (layer 1: the bias slot's product)
    if precision == "fp32":
        return 0.0, n_add * U + prescale + ref64, 0.0, first
    if precision == "bf16":
        return 2.0 ** -8 + 2.0 ** -17, n_add * U + prescale + ref64, 0.0, first
    if precision == "f16x2":
        n_add = 3 * K + 1 + (2 if first else 0)     # three products per weight; layer 1's bias slot is a split weight
        return 3 * 2.0 ** -22 + 2.0 ** -34, n_add * U + prescale + ref64, 2.0 ** -25 + 2.0 ** -35, first
    raise ValueError(precision)


def forward_bound(layers, act, out_act, x, precision):
    """layers [(W, b)] float32, x [N, in_dim] (float32 values) -> (ref [N, 4] float64, bound [N, 4] float64)."""
    h = np.asarray(x, np.float64)
    e = np.zeros_like(h)
    tau = {"oracle": 2.0 ** -22}.get(precision, 11 * U)
    n_layers = len(layers)
    for li, (W32, b32) in enumerate(layers):
        last = li == n_layers - 1
        a = out_act if last else act
        W, b = W32.astype(np.float64), b32.astype(np.float64)
        K = W.shape[1]
        g_op, g_acc, alpha, bias_rounded = _constants(precision, K, li == 0, a == "tanh")
        A = np.abs(W)
        hp = np.abs(h) + e
        z = h @ W.T + b
        mag = hp @ A.T                                                    # sum_k |W_ik| (|h_k| + e_k)
        E = e @ A.T + g_op * (mag + (np.abs(b) if bias_rounded else 0.0)) + g_acc * (mag + np.abs(b))
        if alpha:
            # the bias slot: a split weight against the exact constant 1 (hi = 1, lo = 0), so only the weight's floor, times 1
            E = E + alpha * (A.sum(axis=1) + hp.sum(axis=1, keepdims=True) + (1.0 if bias_rounded else 0.0))
            E = E + (K + 1) * 2.0 ** -48                                  # products of two f16 floors (< 2^-50 each)
        if precision == "f16x2":
            # an operand outside the f16 range leaves the model: the kernel saturates it (finite, not accurate)
            out_of_range = (hp > F16_MAX).any(axis=1, keepdims=True)
            scale = float(np.abs(K_TANH)) if a == "tanh" else 1.0
            big = (A * scale > F16_MAX).any(axis=1) | ((np.abs(b) * scale > F16_MAX) & bias_rounded)
            out_of_range = out_of_range | big[None, :]
            E = np.where(out_of_range, np.inf, E)
        if a == "identity":
            h, e = z, E
            continue
        # a monotone activation of a pre-activation anywhere in [z - E, z + E] lies in [f(z - E), f(z + E)]: its error
        # is at most the larger of the two steps (<= E, both being 1-Lipschitz; far less where tanh saturates or ReLU
        # clips).  An infinite E (out of the f16 model) stays infinite.
        f = (lambda v: np.maximum(v, 0.0)) if a == "relu" else np.tanh
        h = f(z)
        with np.errstate(invalid="ignore"):
            step = np.maximum(f(z + E) - h, h - f(z - E))
        e = np.where(np.isinf(E), np.inf, np.minimum(step, E)) + (tau if a == "tanh" else 0.0)
    return h, e


def hidden_peak(layers, act, x):
    """the largest hidden activation |h| of each hidden layer over the samples of the float64 reference:
    x [N, in_dim] -> [n_hidden]"""
    h = np.asarray(x, np.float64)
    peaks = []
    for W, b in layers[:-1]:
        z = h @ W.astype(np.float64).T + b.astype(np.float64)
        h = np.maximum(z, 0.0) if act == "relu" else np.tanh(z)
        peaks.append(float(np.abs(h).max()))
    return np.array(peaks)


def relabel_bound(weights, in_dim, widths, act, out_act, obs, ids, precision):
    """The bank's labels in float64 and their bounds: weights [n_teachers, P] float32, obs [T, n, 22], ids [n]
    -> (ref [T, n, 4], bound [T, n, 4]).  Vectorised per teacher group."""
    T, n, _ = obs.shape
    ref = np.zeros((T, n, 4))
    bound = np.zeros((T, n, 4))
    ids = np.asarray(ids)
    for k in np.unique(ids):
        envs = np.nonzero(ids == k)[0]
        x = obs[:, envs, :in_dim].reshape(-1, in_dim)
        r, e = forward_bound(unpack(weights[k], in_dim, widths), act, out_act, x, precision)
        ref[:, envs] = r.reshape(T, len(envs), 4)
        bound[:, envs] = e.reshape(T, len(envs), 4)
    return ref, bound


def slack(got, ref, bound):
    """|got - ref| / bound element-wise (0 where both are 0; inf where the bound is 0 and the value is not; NaN labels
    count as inf)."""
    d = np.abs(np.asarray(got, np.float64) - ref)
    d = np.where(np.isnan(d), np.inf, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / bound)
    return np.where(np.isnan(r), np.inf, r)


def within(got, ref, bound, factor=2.0):
    """True where the label meets the bound: |got - ref| <= factor * bound (a NaN label never does)."""
    d = np.abs(np.asarray(got, np.float64) - ref)
    return d <= factor * bound


def assert_within(got, ref, bound, label, factor=2.0, mask=None, finite=True):
    """Assert |got - ref| <= factor * bound element by element (on ``mask`` if given) and print the largest ratio, how
    many labels have no finite bound (an operand outside the f16 model: nothing is claimed there, so a ratio of 0 from
    them is no slack) and the median bound relative to the label.  ``finite``: every bound must be finite."""
    ok = within(got, ref, bound, factor)
    r = slack(got, ref, bound)
    b, a = np.asarray(bound), np.abs(ref)
    if mask is not None:
        ok, r, b, a = ok[mask], r[mask], b[mask], a[mask]
    n_inf = int(np.isinf(b).sum())
    fin = np.isfinite(r) & np.isfinite(b)
    worst = float(r[np.isfinite(b)].max()) if np.isfinite(b).any() else float("nan")
    rel = float(np.median(b[fin] / np.maximum(a[fin], 1e-30))) if fin.any() else float("nan")
    print(f"[teacher bound] {label}: max |got - ref| / e = {worst:.3f} (bar {factor}); median e / |ref| = {rel:.2e}; "
          f"{n_inf} of {b.size} labels without a finite bound")
    if finite and n_inf:
        raise AssertionError(f"{label}: {n_inf} of {b.size} labels have no finite bound (an operand outside the f16 model)")
    if not ok.all():
        bad = np.argwhere(~ok)[:5]
        raise AssertionError(f"{label}: {int((~ok).sum())} labels outside {factor} x the float64 bound "
                             f"(max ratio {float(r.max()):.3g}; first at {bad.tolist()})")
    return worst


# ---------------------------------------------------------------------------- emulations (NumPy) ---
# What the 16-bit kernels do with their operands, step by step as rq_pack.cpp and rq_teacher.hip do it; the sums are
# taken in float64 (one rounding to fp32 per layer), which the accumulation term of the bound covers.
def to_bf16(x):
    """float32 -> nearest bf16 (ties to even), returned as float32; what to_bf16_rne and the device conversion do."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split_f16(x, saturate=False):
    """float32 -> (hi, lo) f16 pieces as float64: hi = f16(v), lo = f16(v - hi).  ``saturate`` clamps to +-65 504 first
    (a NaN becomes -65 504, as v_med3_f32 does); without it |v| >= 65 520 gives hi = inf and lo = -inf."""
    v = np.asarray(x, np.float32)
    if saturate:
        v = np.where(np.isnan(v), np.float32(-F16_MAX), np.clip(v, -F16_MAX, F16_MAX)).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def _tanh_kernel(z32):
    with np.errstate(over="ignore"):
        return (np.float32(2.0) / (np.float32(1.0) + np.exp2(z32)) - np.float32(1.0)).astype(np.float32)


def emulate(layers, act, out_act, x, precision, saturate=True, drop_hi_lo=False):
    """The bf16 or f16x2 kernel on x [N, in_dim] float32 -> labels [N, 4] float32.  ``saturate=False`` splits
    observations and ReLU activations unclamped; ``drop_hi_lo`` leaves out the hi(W) lo(h) products (both: faults)."""
    h = np.asarray(x, np.float32)
    n_layers = len(layers)
    for li, (W, b) in enumerate(layers):
        a = out_act if li == n_layers - 1 else act
        k = K_TANH if a == "tanh" else np.float32(1.0)
        Ws = (k * W).astype(np.float32)
        bs = (k * b).astype(np.float32)
        c = np.zeros(W.shape[0], np.float64)
        if li == 0:                                       # the bias rides in slot in_dim against the constant 1
            Ws = np.concatenate([Ws, bs[:, None]], axis=1)
            h = np.concatenate([h, np.ones((h.shape[0], 1), np.float32)], axis=1)
        else:
            c = bs.astype(np.float64)                     # fp32 C operand
        if precision == "bf16":
            z = to_bf16(h).astype(np.float64) @ to_bf16(Ws).astype(np.float64).T
        elif precision == "f16x2":
            sat_h = saturate and (li == 0 or act == "relu")
            hh, hl = split_f16(h, saturate=sat_h)
            wh, wl = split_f16(Ws)                        # the host packer: no clamp (it refuses what does not fit)
            with np.errstate(invalid="ignore", over="ignore"):
                z = hh @ wh.T
                if not drop_hi_lo:
                    z = z + hl @ wh.T
                z = z + hh @ wl.T
        else:
            raise ValueError(precision)
        with np.errstate(invalid="ignore", over="ignore"):
            z32 = (z + c).astype(np.float32)
        if a == "relu":
            h = np.maximum(z32, np.float32(0.0))
        elif a == "tanh":
            h = _tanh_kernel(z32)
        else:
            h = z32
    return h
