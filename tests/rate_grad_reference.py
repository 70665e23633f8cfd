"""tests/policy_grad_reference.py's float64 statement of the student's forward and back-propagation through time at a deployment
control rate (``Raptor(native_interval=R)``; csrc/rq_grad_forward.inc and rq_grad_backward.inc under RQ_GRAD_RATE).  Per env, k is
the episode step count of the step (``start_steps`` at the first one) and c the committed state: h' = GRU(relu(W0 x + b0), c) and
a = W2 h' + b2 at every step; c <- h' where k % R == 0 and the step is not frozen; done code 1 or 2: c <- h0, k <- 0; code 4: nothing
moves, k included; any other code: k <- k + 1.  Backward: a held step (not native, not frozen) treats the recurrence exactly as a
frozen step does - its own dL/da goes through h' into c - so ``backward`` is the native-rate recursion over a cache whose held steps
carry the frozen code.  At R = 1 nothing is held and the functions return that reference's arrays.  The bound has its form, 2 u K A +
2^-120, with the same K = K_paths(T, waves) - a held step adds selects to the kernel and no rounding - and A from the rated recursion
on magnitudes."""
import numpy as np

import policy_grad_reference as R


def forward(w, obs, done, interval, start_steps, start="initial", h_start=None):
    """obs [T, N, 22], done [T, N], start_steps [N] -> (act [T, N, 4], cache).  ``h_start`` [N, 16] for start = "current"."""
    p = R.unpack(w)
    obs = np.asarray(obs, np.float64)
    T, N = obs.shape[:2]
    c = np.tile(p["h0"], (N, 1)) if start == "initial" else np.array(h_start, np.float64).reshape(N, 16)
    k = np.asarray(start_steps).astype(np.int64).copy()
    assert k.shape == (N,) and interval >= 1
    act = np.empty((T, N, 4))
    steps = []
    for t in range(T):
        x = obs[t]
        pre0 = x @ p["W0"].T + p["b0"]
        y0 = np.maximum(pre0, 0.0)
        gi = y0 @ p["Wi"].T + p["bi"]
        gh = c @ p["Wh"].T + p["bh"]
        r = R._sigmoid(gi[:, :16] + gh[:, :16])
        z = R._sigmoid(gi[:, 16:32] + gh[:, 16:32])
        gnh = gh[:, 32:]
        n = np.tanh(gi[:, 32:] + r * gnh)
        hn = (1.0 - z) * n + z * c
        act[t] = hn @ p["W2"].T + p["b2"]
        d = np.asarray(done[t])
        frozen, ended = d == 4, (d == 1) | (d == 2)
        hold = frozen | (k % interval != 0)
        steps.append(dict(x=x, pre0=pre0, y0=y0, hp=c, r=r, z=z, n=n, gnh=gnh, hn=hn, d=d, hold=hold))
        c = np.where(hold[:, None], c, hn)
        c = np.where(ended[:, None], p["h0"], c)
        k = np.where(ended, 0, np.where(frozen, k, k + 1))
    return act, dict(p=p, steps=steps, start=start)


def _as_native(cache):
    """the cache the native-rate recursion takes: a held step that does not end an episode carries the frozen code"""
    steps = [dict(s, d=np.where(s["hold"] & (s["d"] != 1) & (s["d"] != 2), 4, s["d"])) for s in cache["steps"]]
    return dict(cache, steps=steps)


def backward(cache, dact, absolute=False):
    """dact [T, N, 4] -> (dL/dtheta [2084], dL/dh_start [N, 16] or None); absolute=True: the recursion on magnitudes"""
    return R.backward(_as_native(cache), dact, absolute)


def bound(cache, dact, waves):
    """element-wise bound on |fp32 kernel - float64| for dL/dtheta and dL/dh_start (module docstring)"""
    return R.bound(_as_native(cache), dact, waves)
