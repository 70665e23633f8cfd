"""Float64 reference of the student's forward and back-propagation through time over a recorded trajectory, with an element-wise
error bound for the fp32 kernels (csrc/rq_grad.hpp, compiled inside rq_kernels.hip).

The student is Dense 22->16 ReLU -> GRU 16 -> Dense 16->4 (PyTorch's GRUCell formulation):

    y  = relu(W0 x + b0)
    r  = sigma(Wi_r y + bi_r + Wh_r h + bh_r),  z = sigma(Wi_z y + bi_z + Wh_z h + bh_z)
    n  = tanh(Wi_n y + bi_n + r (Wh_n h + bh_n)),  h' = (1 - z) n + z h,  a = W2 h' + b2

over a trajectory with done codes: after a step with code 1 or 2 the state returns to the learned initial state h0 (weights
[2000:2016]); a step with code 4 computes its action from h' but the state is not advanced.  ``start`` = "initial" starts every
env from h0, "current" from a given state (a constant).  The loss's gradient dL/da is an input; ``backward`` returns dL/dtheta in
the flat weight order and dL/dh_start.

Error bound (``bound``).  A first-order forward error analysis (Higham, Accuracy and Stability of Numerical Algorithms, 3.1-3.5):
every value the kernel computes is a chain of fp32 operations, each of which rounds once with relative error at most u = 2^-24
(v_exp_f32 and v_rcp_f32: 1 ulp = 2 u, counted as two roundings).  To first order the error of a result is then at most u times
the sum, over every path from a rounding to the result, of (roundings on that path) x |path's product of partial derivatives x
value rounded|, which is at most u * K * A where

* A is the same computation carried out on absolute values (``backward(..., absolute=True)``): every product of absolute values,
  every sum a sum of magnitudes.  It bounds the magnitude of every path's contribution, so it is at least |g| element-wise.
* K bounds the number of roundings on any path:
  - accumulation: a weight's gradient is one fp32 sum per wave of 64 envs x T steps of products (the MFMA accumulators, one
    fma each), then a sum over the W waves: 64 T + W;
  - the reverse recursion: per step a path crosses W2^T (4 fmas), the gate deltas (at most 6 VALU roundings), W_i^T or W_h^T
    (48 fmas) and reads forward values recomputed from the saved state: layer_0 (24 fmas), the gate chains (32 fmas + the
    pre-scaling of their operands, 2), exp2, rcp, an add and three fmas for a gate (9 with the transcendentals counted twice):
    4 + 6 + 48 + 24 + 34 + 9 = 125 < 200 per step, so 200 T, plus 200 for the final step's forward values.
* The factor 2 covers the first-order model: the forward values enter the gradient through derivative factors (r (1 - r),
  z (1 - z), 1 - n^2, h - n, gnh) that are Lipschitz in their arguments with constants at most 1 (|sigma''| < 0.1,
  |(tanh')'| < 0.77), so an error in a forward value moves the factor by at most that much and is already counted once on its
  path; the second-order remainder is below (K u)^2 relative, < 1e-4 at K u <= 0.01 (T = 500).

    bound = 2 u K A + 2^-120 (an absolute floor: subnormal products)

Where it holds.  The Lipschitz remark bounds a factor's error by the error of its argument, an ABSOLUTE quantity of order u times
the gate chain's operands, while A charges the factor RELATIVE to its own size: 2 u K |dh| (1 - z) shrinks with 1 - z, and the
kernel's 1 - z~, formed from a rounded gate (rq_grad_backward.inc:197-204), is off by u-sized amounts however small it is.  The
bound therefore holds where the derivative factors are of order one and the observations of order one - the shipped checkpoint, its
perturbations, the recordings it flies - and not on saturated or signed gates or observations x 2^10, where a plain float32
evaluation of these very formulas leaves it by up to five orders of magnitude.  There ``policy_grad_window.window_bound`` is the
bound to use: it carries an absolute error beside every value (short windows, T <= 3); tests/test_gpu_policy_grad_float64.py holds
the kernels to it on every weight and input family of tests/actor_reference.py.

What the bound is good for: A propagates |J| - the Jacobians with every sign dropped - so it grows along an episode by about the
spectral radius of |J| per step (~1.7 for the shipped policy: A / max |g| is ~0.4 after 9 recurrent steps, ~1e3 after 24, ~1e20
after 100), while the signed products the gradient itself is made of stay bounded.  It is therefore a useful check over the short
episodes of the auto-reset recordings the tests use and only an outer bound over long ones; the GPU tests print the relative error
of a 500-step episode beside it.  The reference's own float64 error (K * 2^-53 relative) is below the bound's resolution.  Columns of padding envs are not part of
the reference: the kernel must give them no weight at all, which the GPU tests check with NaN there.
"""
import numpy as np

U = 2.0 ** -24
OFF = dict(W0=0, B0=352, WI=368, WH=1136, BI=1904, BH=1952, H0=2000, W2=2016, B2=2080, END=2084)


def unpack(w):
    """flat [2084] -> dict of float64 arrays in the checkpoint's shapes"""
    w = np.asarray(w, np.float64)
    assert w.shape == (2084,)
    return dict(W0=w[0:352].reshape(16, 22), b0=w[352:368], Wi=w[368:1136].reshape(48, 16), Wh=w[1136:1904].reshape(48, 16),
                bi=w[1904:1952], bh=w[1952:2000], h0=w[2000:2016], W2=w[2016:2080].reshape(4, 16), b2=w[2080:2084])


def pack(p):
    return np.concatenate([p["W0"].ravel(), p["b0"], p["Wi"].ravel(), p["Wh"].ravel(), p["bi"], p["bh"], p["h0"],
                           p["W2"].ravel(), p["b2"]])


def _sigmoid(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def forward(w, obs, done, start="initial", h_start=None):
    """obs [T, N, 22], done [T, N] -> (act [T, N, 4], cache).  ``h_start`` [N, 16] for start = "current"."""
    p = unpack(w)
    obs = np.asarray(obs, np.float64)
    T, N = obs.shape[:2]
    h = np.tile(p["h0"], (N, 1)) if start == "initial" else np.array(h_start, np.float64).reshape(N, 16)
    act = np.empty((T, N, 4))
    steps = []
    for t in range(T):
        x = obs[t]
        pre0 = x @ p["W0"].T + p["b0"]
        y0 = np.maximum(pre0, 0.0)
        gi = y0 @ p["Wi"].T + p["bi"]
        gh = h @ p["Wh"].T + p["bh"]
        r = _sigmoid(gi[:, :16] + gh[:, :16])
        z = _sigmoid(gi[:, 16:32] + gh[:, 16:32])
        gnh = gh[:, 32:]
        n = np.tanh(gi[:, 32:] + r * gnh)
        hn = (1.0 - z) * n + z * h
        act[t] = hn @ p["W2"].T + p["b2"]
        d = np.asarray(done[t])
        steps.append(dict(x=x, pre0=pre0, y0=y0, hp=h, r=r, z=z, n=n, gnh=gnh, hn=hn, d=d))
        h = np.where((d == 4)[:, None], h, hn)
        h = np.where(((d == 1) | (d == 2))[:, None], p["h0"], h)
    return act, dict(p=p, steps=steps, start=start)


def backward(cache, dact, absolute=False):
    """dact [T, N, 4] -> (dL/dtheta [2084], dL/dh_start [N, 16] or None).  absolute=True: the same recursion on magnitudes (the
    A of the bound)."""
    p, steps = cache["p"], cache["steps"]
    ab = np.abs if absolute else (lambda v: v)
    W0, Wi, Wh, W2 = ab(p["W0"]), ab(p["Wi"]), ab(p["Wh"]), ab(p["W2"])
    g = {k: np.zeros_like(v) for k, v in p.items()}
    dact = np.asarray(dact, np.float64)
    N = dact.shape[1]
    carry = np.zeros((N, 16))
    for t in range(len(steps) - 1, -1, -1):
        s = steps[t]
        ended = (s["d"] == 1) | (s["d"] == 2)
        frozen = s["d"] == 4
        g["h0"] += carry[ended].sum(0)
        carry = np.where(ended[:, None], 0.0, carry)
        din = np.where(frozen[:, None], 0.0, carry)
        pas = np.where(frozen[:, None], carry, 0.0)
        da = ab(dact[t])
        hn, hp, y0, x = ab(s["hn"]), ab(s["hp"]), ab(s["y0"]), ab(s["x"])
        r, z, n, gnh = s["r"], s["z"], s["n"], s["gnh"]
        dh = da @ W2 + din
        g["W2"] += da.T @ hn
        g["b2"] += da.sum(0)
        dn = dh * (1.0 - z)
        dz = dh * ab(s["hp"] - n)
        du = dn * (1.0 - n * n)
        dPr = du * ab(gnh) * r * (1.0 - r)
        dPz = dz * z * (1.0 - z)
        di = np.concatenate([dPr, dPz, du], 1)
        dhh = np.concatenate([dPr, dPz, du * r], 1)
        g["Wi"] += di.T @ y0
        g["bi"] += di.sum(0)
        g["Wh"] += dhh.T @ hp
        g["bh"] += dhh.sum(0)
        dp0 = (di @ Wi) * (s["pre0"] > 0)
        g["W0"] += dp0.T @ x
        g["b0"] += dp0.sum(0)
        carry = dhh @ Wh + dh * z + pas
    dh_start = None
    if cache["start"] == "initial":
        g["h0"] += carry.sum(0)
    else:
        dh_start = carry
    return pack(g), dh_start


def K_paths(T, waves):
    """the rounding count K of the module docstring"""
    return 64 * T + waves + 200 * T + 200


def bound(cache, dact, waves):
    """element-wise bound on |fp32 kernel - float64| for dL/dtheta and dL/dh_start (module docstring)"""
    A, A_h = backward(cache, dact, absolute=True)
    K = K_paths(len(cache["steps"]), waves)
    floor = 2.0 ** -120
    return 2 * U * K * A + floor, (None if A_h is None else 2 * U * K * A_h + floor)
