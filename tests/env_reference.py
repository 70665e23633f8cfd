"""Float64 statement of ONE env transition and of the noise-free observation, the element-wise bound a float32
evaluation of the specification is held to, references with one deliberate mistake each, and the input families that put the
edges of the randomised fleet into one batch.  NumPy only; nothing is imported from oracle/ and nothing here uses a device.

TWO TEXTS.  ``step64`` / ``observe64`` state the physics with objects: a rotation matrix R(q), the Hamilton product, cross products
of rotor arms and thrusts, an inertia J and its inverse - not the component formulas the kernels and the C restatement share.
``step_bound`` / ``observe_bound`` walk the specification's float32 operations one by one (they must, to count them) on pairs
(value, error); the value they carry is asserted to agree with ``step64`` to float64 rounding (2^-20 of the bound), so a term
lost or a sign flipped in either text shows as a disagreement of the two before any kernel is looked at.  What a kernel is compared
with is always ``step64``.

THE BOUND, by running-error analysis, u = 2^-24.  Inputs (params, state, action, config, schedule rows) are float32 and exact.
Every float32 operation of the specification - ``+``, ``x``, a one-rounding ``fma``, ``1/x``, ``/``, ``sqrt`` - on operands with
values a, b and error bounds ea, eb gives
      value  the exact result on the values
      error  the propagated input error in absolute values (|a| eb + |b| ea + ea eb for a product, ea / (|a| (|a| - ea)) for a
             reciprocal, ...)  +  u (|value| + that propagated error)            <- the one rounding of the computed result
  * min, max and the clamps are 1-Lipschitz: the error passes through;  a product with a power of two is exact (0.5 dt, 2 x, 0.5 x).
  * 1/m, 1/J, 1/tau, dt/6 and dt/3 are operations and round once each; so do the products of a vehicle row and the wrench scales.
  * No slack factor and no fitted constant: the only number besides u is the 2^-20 above, which covers float64 rounding of the
    reference itself (2^-53 per operation against 2^-24: a few hundred operations stay below 2^-20 of the bound).
  * Underflow is not modelled: the families keep every intermediate above 2^-126 or exactly zero.
DISCONTINUITIES.  A rotor whose set-point and speed at an RK4 stage differ by no more than their own error bounds may take either
time constant in float32: that stage's derivative gains (|sp - r| + error) |1/tau_rise - 1/tau_fall|.  A termination comparison is
UNDECIDED where the reference lies within its bound of the threshold: ``step_bound`` returns the mask, the flag and the reward of
those envs are not asserted (the state is), and the tests cap their share at 1 % per family - a cap, not a tolerance.

THE 1/|q| SERIES (``series_table``).  The specification pulls the quaternion back with s(e) = 1 + e (1/2 + 3 e / 8), e = 1 - |q|^2
clamped to +-0.5, not with 1 / |q|.  One RK4 step of a rotation at rate |w| from a unit quaternion leaves e ~ (|w| dt)^6 / 4600;
the relative distance of s(e) from 1 / sqrt(1 - e) is 5 e^3 / 16 + O(e^4), below one float32 ulp of 1 (2^-23) while |e| <= 7.2e-3.
Measured by ``series_table`` (the CPU test prints it): | |q'| - 1 | stays within one ulp for |w| dt <= 1.8 (0.77 ulp there: 180 rad/s
at dt = 10 ms, 90 rad/s at 20 ms), is 4.7 ulps at |w| dt = 2 and 0.05 % at 3; from |w| dt = 5 the clamp is active and |q'| is RK4's
own polynomial times 0.84 - off 1 by a third at |w| dt = 5, |q'| = 18 at 10, 220 at 18: finite, no rotation any more.  A state set with |q| in [0.8, 1.2] (``off_unit``) is pulled to within 2.4 % of unit length in
one step and 3.2e-5 in two.
"""
import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
SPIN = np.array([-1.0, 1.0, -1.0, 1.0])          # yaw reaction of rotors FR, BR, BL, FL
LARGEST_SCALE = 9.0
DTS = (0.0025, 0.01, 0.02)
RELATIVE, ABSOLUTE = "relative", "absolute"

MISTAKES = ["no_gyroscopic", "stage3_full_step", "weights_exchanged", "tau_exchanged", "yaw_reaction_flipped", "no_renormalisation",
            "series_first_order", "reward_on_entering_state", "wind_refreshed_per_stage", "vehicle_inertia_not_inverted",
            "wrench_arm_without_sqrt2"]
# what a mistake needs to show at all: a schedule row of that kind, or rotors that rise and fall at different rates
NEEDS = {"wind_refreshed_per_stage": "wind", "vehicle_inertia_not_inverted": "vehicle", "wrench_arm_without_sqrt2": "wrench",
         "tau_exchanged": "tau_differ"}


def _f64(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.astype(np.float64)


def _cfg(cfg):
    """the config's float32 fields as Python floats (exact)"""
    names = ("dt gravity reward_scale reward_constant reward_termination_penalty reward_position reward_orientation "
             "reward_linear_velocity reward_angular_velocity reward_action termination_position termination_linear_velocity "
             "termination_angular_velocity").split()
    c = {k: float(np.float32(getattr(cfg, k))) for k in names}
    c["termination_enabled"] = int(cfg.termination_enabled)
    c["action_history_raw"] = int(cfg.action_history_raw)
    return c


# ------------------------------------------------------------------ 1. the statement -----
def rotation(q):
    """R(q) [n, 3, 3], body -> world, of q = (w, v): I + 2 w K + 2 K K with K = [v]x, Rodrigues' form.  q is taken as it is: for
    |q| != 1 this is the polynomial the specification evaluates (it does not divide by |q|^2)."""
    w, v = q[:, 0], q[:, 1:4]
    K = np.zeros((q.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2] = -v[:, 2], v[:, 1]
    K[:, 1, 0], K[:, 1, 2] = v[:, 2], -v[:, 0]
    K[:, 2, 0], K[:, 2, 1] = -v[:, 1], v[:, 0]
    return np.eye(3)[None] + 2.0 * w[:, None, None] * K + 2.0 * (K @ K)


def qmul(a, b):
    """Hamilton product [n, 4]: (a0 b0 - av.bv, a0 bv + b0 av + av x bv)"""
    a0, av, b0, bv = a[:, 0:1], a[:, 1:4], b[:, 0:1], b[:, 1:4]
    return np.concatenate([a0 * b0 - (av * bv).sum(1, keepdims=True), a0 * bv + b0 * av + np.cross(av, bv)], axis=1)


class Vehicle:
    """The constants of one transition in float64: the params' fields, a vehicle row's factors applied, the wrench of the state with
    the wrench and wind rows added - as physics."""

    def __init__(self, c, P, S, wrench_row, vehicle_row, wind_row, units, mistake):
        P, S = _f64(P), _f64(S)
        n = P.shape[0]
        f = np.ones((n, 4)) if vehicle_row is None else _f64(vehicle_row)
        self.g = c["gravity"]
        self.m = P[:, 0] * f[:, 0]
        self.J = P[:, 1:4] * f[:, 1:2]                               # a diagonal inertia
        self.Jinv = 1.0 / (P[:, 1:4] if mistake == "vehicle_inertia_not_inverted" else self.J)
        self.arms = P[:, 4:16].reshape(n, 4, 3)
        self.c = P[:, 16:19] * f[:, 2:3]
        self.kq = -P[:, 19] if mistake == "yaw_reaction_flipped" else P[:, 19]
        tau = P[:, 20:22] * f[:, 3:4]
        self.tau_rise, self.tau_fall = (tau[:, 1], tau[:, 0]) if mistake == "tau_exchanged" else (tau[:, 0], tau[:, 1])
        self.rpm_min, self.rpm_max = P[:, 22], P[:, 23]
        self.hover_action = P[:, 25]
        force, torque = S[:, 21:24].copy(), S[:, 24:27].copy()
        if wrench_row is not None:
            row = _f64(wrench_row)
            if units == RELATIVE:
                mg = self.m * self.g
                arm = np.abs(P[:, 4]) if mistake == "wrench_arm_without_sqrt2" else np.hypot(P[:, 4], P[:, 5])
                force += mg[:, None] * row[:, 0:3]
                torque += (mg * arm)[:, None] * row[:, 3:6]
            else:
                assert units == ABSOLUTE, units
                force += row[:, 0:3]
                torque += row[:, 3:6]
        self.force, self.torque = force, torque
        self.air = None
        if wind_row is not None:
            row = _f64(wind_row)
            self.air, self.md = row[:, 0:3], self.m * row[:, 3]
            self.v_in = S[:, 7:10]
            self.refresh = mistake == "wind_refreshed_per_stage"
        self.gyroscopic = mistake != "no_gyroscopic"

    def ode(self, y, sp):
        """dy/dt of y = (p, q, v, w, rotors) [n, 17] at the rotor set-points sp [n, 4]"""
        n = y.shape[0]
        q, v, w, r = y[:, 3:7], y[:, 7:10], y[:, 10:13], y[:, 13:17]
        T = self.c[:, 0:1] + self.c[:, 1:2] * r + self.c[:, 2:3] * r * r
        thrusts = np.zeros((n, 4, 3))
        thrusts[:, :, 2] = T
        torque = np.cross(self.arms, thrusts).sum(axis=1) + self.torque
        torque[:, 2] += self.kq * (T @ SPIN)
        force = self.force
        if self.air is not None:
            force = force + self.md[:, None] * (self.air - (v if self.refresh else self.v_in))
        dv = (np.einsum("nij,nj->ni", rotation(q), thrusts.sum(axis=1)) + force) / self.m[:, None]
        dv[:, 2] -= self.g
        Jw = self.J * w
        dw = self.Jinv * (torque - np.cross(w, Jw) if self.gyroscopic else torque)
        dq = 0.5 * qmul(q, np.concatenate([np.zeros((n, 1)), w], axis=1))
        dr = (sp - r) / np.where(sp >= r, self.tau_rise[:, None], self.tau_fall[:, None])
        return np.concatenate([v, dq, dv, dw, dr], axis=1)


def _reward_and_termination(c, veh, y, ac, y_for_reward):
    term = np.zeros(y.shape[0], bool)
    if c["termination_enabled"]:
        with np.errstate(invalid="ignore"):
            term |= (np.abs(y[:, 0:3]) > c["termination_position"]).any(1)
            term |= (np.abs(y[:, 7:10]) > c["termination_linear_velocity"]).any(1)
            term |= (np.abs(y[:, 10:13]) > c["termination_angular_velocity"]).any(1)
            term |= ~np.isfinite(y).all(1)
    z = y_for_reward
    cost = (c["reward_position"] * (z[:, 0:3] ** 2).sum(1) + c["reward_orientation"] * (1.0 - z[:, 3] ** 2) +
            c["reward_linear_velocity"] * (z[:, 7:10] ** 2).sum(1) + c["reward_angular_velocity"] * (z[:, 10:13] ** 2).sum(1) +
            c["reward_action"] * ((ac - veh.hover_action[:, None]) ** 2).sum(1))
    reward = np.where(term, c["reward_termination_penalty"], c["reward_constant"] - c["reward_scale"] * cost)
    return reward, term


def step64(cfg, P, S, A, wrench_row=None, vehicle_row=None, wind_row=None, units=RELATIVE, mistake=None, dt=None):
    """One transition in float64 from float32 inputs -> (next state [n, 27], reward [n], terminated [n] bool).  ``mistake``: one of
    MISTAKES (``altered`` binds it); ``dt``: instead of the config's (the quarter steps of the integration test)."""
    assert mistake is None or mistake in MISTAKES, mistake
    c = _cfg(cfg)
    h = c["dt"] if dt is None else float(dt)
    veh = Vehicle(c, P, S, wrench_row, vehicle_row, wind_row, units, mistake)
    S64, A64 = _f64(S), _f64(A)
    ac = np.clip(A64, -1.0, 1.0)
    sp = veh.rpm_min[:, None] + (ac + 1.0) / 2.0 * (veh.rpm_max - veh.rpm_min)[:, None]
    y0 = S64[:, :17]
    k1 = veh.ode(y0, sp)
    k2 = veh.ode(y0 + h / 2 * k1, sp)
    k3 = veh.ode(y0 + (h if mistake == "stage3_full_step" else h / 2) * k2, sp)
    k4 = veh.ode(y0 + h * k3, sp)
    outer, inner = (h / 3, h / 6) if mistake == "weights_exchanged" else (h / 6, h / 3)
    y = y0 + outer * (k1 + k4) + inner * (k2 + k3)
    if mistake != "no_renormalisation":
        e = np.clip(1.0 - (y[:, 3:7] ** 2).sum(1), -0.5, 0.5)
        y[:, 3:7] *= (1.0 + e * (0.5 if mistake == "series_first_order" else 0.5 + 3.0 * e / 8.0))[:, None]
    y[:, 13:17] = np.clip(y[:, 13:17], veh.rpm_min[:, None], veh.rpm_max[:, None])
    ns = S64.copy()
    ns[:, :17] = y
    ns[:, 17:21] = A64 if c["action_history_raw"] else ac
    reward, term = _reward_and_termination(c, veh, y, ac, S64[:, :17] if mistake == "reward_on_entering_state" else y)
    return ns, reward, term


def altered(name):
    """``step64`` with one mistake: the reference of a kernel that is wrong in that way"""
    assert name in MISTAKES, name
    return lambda *a, **kw: step64(*a, mistake=name, **kw)


def exact_unit(q):
    """q / |q| [n, 4]: what the series approximates"""
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def observe64(P, S):
    """The 26 noise-free observation columns in float64: position, R(q) row-major, linear velocity, body rates, the previous action,
    the rotor speeds mapped to [-1, 1]."""
    P, S = _f64(P), _f64(S)
    n = S.shape[0]
    rotors = 2.0 * (S[:, 13:17] - P[:, 22:23]) / (P[:, 23:24] - P[:, 22:23]) - 1.0
    return np.concatenate([S[:, 0:3], rotation(S[:, 3:7]).reshape(n, 9), S[:, 7:10], S[:, 10:13], S[:, 17:21], rotors], axis=1)


# ------------------------------------------------------------------ 2. the running error -----
class V:
    """a float32 quantity of the specification: its exact-arithmetic value x (float64) and a bound e on |float32 value - x|"""
    __slots__ = ("x", "e")

    def __init__(self, x, e=None):
        self.x = np.asarray(x, np.float64)
        self.e = np.zeros_like(self.x) if e is None else np.asarray(e, np.float64)


def _v(a):
    return a if isinstance(a, V) else V(a)


def _rounded(x, propagated):
    with np.errstate(all="ignore"):
        return V(x, propagated + U * (np.abs(x) + propagated))


def add(a, b):
    a, b = _v(a), _v(b)
    return _rounded(a.x + b.x, a.e + b.e)


def sub(a, b):
    a, b = _v(a), _v(b)
    return _rounded(a.x - b.x, a.e + b.e)


def _product_error(a, b):
    with np.errstate(all="ignore"):
        return np.abs(a.x) * b.e + np.abs(b.x) * a.e + a.e * b.e


def mul(a, b):
    a, b = _v(a), _v(b)
    with np.errstate(all="ignore"):
        return _rounded(a.x * b.x, _product_error(a, b))


def fma(a, b, c):
    a, b, c = _v(a), _v(b), _v(c)
    with np.errstate(all="ignore"):
        return _rounded(a.x * b.x + c.x, _product_error(a, b) + c.e)


def rcp(a):
    a = _v(a)
    with np.errstate(all="ignore"):
        ax = np.abs(a.x)
        return _rounded(1.0 / a.x, np.where(a.e > 0, a.e / (ax * (ax - a.e)), 0.0))


def div(a, b):
    a, b = _v(a), _v(b)
    with np.errstate(all="ignore"):
        x = a.x / b.x
        return _rounded(x, (a.e + np.abs(x) * b.e) / (np.abs(b.x) - b.e))


def root(a):
    a = _v(a)
    with np.errstate(all="ignore"):
        return _rounded(np.sqrt(a.x), a.e / (np.sqrt(np.maximum(a.x - a.e, 0.0)) + np.sqrt(a.x)))


def scaled(a, k):
    """a product with +-2^j: exact"""
    a = _v(a)
    return V(a.x * k, a.e * abs(k))


def neg(a):
    return scaled(a, -1.0)


def clamp(a, lo, hi):
    return V(np.minimum(np.maximum(a.x, lo), hi), a.e)


class _Consts:
    pass


def _constants(c, P, S, wrench_row, vehicle_row, wind_row, units):
    """the per-env constants of a transition as the specification makes them, operation by operation"""
    P, S = _f64(P), _f64(S)
    k = _Consts()
    m, J, cc, tau = V(P[:, 0]), [V(P[:, 1 + i]) for i in range(3)], [V(P[:, 16 + i]) for i in range(3)], [V(P[:, 20]), V(P[:, 21])]
    if vehicle_row is not None:
        f = _f64(vehicle_row)
        m = mul(m, f[:, 0])
        J = [mul(j, f[:, 1]) for j in J]
        cc = [mul(x, f[:, 2]) for x in cc]
        tau = [mul(t, f[:, 3]) for t in tau]
    force, torque = [V(S[:, 21 + i]) for i in range(3)], [V(S[:, 24 + i]) for i in range(3)]
    if wrench_row is not None:
        row = _f64(wrench_row)
        if units == RELATIVE:
            mg = mul(m, c["gravity"])
            arm = root(add(mul(P[:, 4], P[:, 4]), mul(P[:, 5], P[:, 5])))
            fs, ts = mg, mul(mg, arm)
            force = [add(force[i], mul(fs, row[:, i])) for i in range(3)]
            torque = [add(torque[i], mul(ts, row[:, 3 + i])) for i in range(3)]
        else:
            force = [add(force[i], row[:, i]) for i in range(3)]           # 1.0f * row is row
            torque = [add(torque[i], row[:, 3 + i]) for i in range(3)]
    if wind_row is not None:
        row = _f64(wind_row)
        md = mul(m, row[:, 3])
        force = [add(force[i], mul(md, sub(row[:, i], S[:, 7 + i]))) for i in range(3)]
    k.inv_m = rcp(m)
    k.J, k.iJ = J, [rcp(j) for j in J]
    k.px, k.py = [V(P[:, 4 + 3 * i]) for i in range(4)], [V(P[:, 5 + 3 * i]) for i in range(4)]
    k.c0, k.c1, k.c2 = cc
    k.kq = V(P[:, 19])
    k.itr, k.itf = rcp(tau[0]), rcp(tau[1])
    k.ad = [mul(force[0], k.inv_m), mul(force[1], k.inv_m), fma(force[2], k.inv_m, -c["gravity"])]
    k.td = torque
    return k


def _dynamics(k, y, sp):
    """the stage derivative, the specification's operations in their order, on (value, error) pairs"""
    qw, qx, qy, qz = y[3:7]
    wx, wy, wz = y[10:13]
    T = [fma(fma(k.c2, y[13 + i], k.c1), y[13 + i], k.c0) for i in range(4)]
    u02, u13 = add(T[0], T[2]), add(T[1], T[3])
    tsum = add(u02, u13)
    tx, ty = k.td[0], k.td[1]
    for i in range(4):
        tx = fma(k.py[i], T[i], tx)
        ty = fma(neg(k.px[i]), T[i], ty)
    tz = fma(k.kq, sub(u13, u02), k.td[2])
    d = [None] * 17
    d[0], d[1], d[2] = y[7], y[8], y[9]
    d[3] = scaled(fma(neg(qy), wy, fma(neg(qx), wx, neg(mul(qz, wz)))), 0.5)
    d[4] = scaled(fma(qy, wz, fma(neg(qz), wy, mul(qw, wx))), 0.5)
    d[5] = scaled(fma(neg(qx), wz, fma(qz, wx, mul(qw, wy))), 0.5)
    d[6] = scaled(fma(neg(qy), wx, fma(qx, wy, mul(qw, wz))), 0.5)
    r02 = scaled(fma(qx, qz, mul(qw, qy)), 2.0)
    r12 = scaled(fma(qy, qz, neg(mul(qw, qx))), 2.0)
    r22 = fma(-2.0, fma(qx, qx, mul(qy, qy)), 1.0)
    acc = mul(tsum, k.inv_m)
    d[7], d[8], d[9] = fma(r02, acc, k.ad[0]), fma(r12, acc, k.ad[1]), fma(r22, acc, k.ad[2])
    jwx, jwy, jwz = mul(k.J[0], wx), mul(k.J[1], wy), mul(k.J[2], wz)
    cx = fma(neg(wz), jwy, mul(wy, jwz))
    cy = fma(wz, jwx, neg(mul(wx, jwz)))
    cz = fma(wx, jwy, neg(mul(wy, jwx)))
    d[10], d[11], d[12] = mul(sub(tx, cx), k.iJ[0]), mul(sub(ty, cy), k.iJ[1]), mul(sub(tz, cz), k.iJ[2])
    for i in range(4):
        r = y[13 + i]
        e = sub(sp[i], r)
        rise = sp[i].x >= r.x
        out = mul(e, V(np.where(rise, k.itr.x, k.itf.x), np.where(rise, k.itr.e, k.itf.e)))
        # either branch: the comparison is made on float32 values that lie within their bounds of these
        either = np.abs(sp[i].x - r.x) <= sp[i].e + r.e
        gap = np.abs(k.itr.x - k.itf.x) + k.itr.e + k.itf.e
        d[13 + i] = V(out.x, out.e + np.where(either, (np.abs(e.x) + e.e) * gap, 0.0))
    return d


def _quadratic(c, items):
    """c0 x0 + sum fma: the specification's nested fma sum of squares, innermost first"""
    acc = mul(items[0], items[0])
    for x in items[1:]:
        acc = fma(x, x, acc)
    return acc


def step_bound(cfg, P, S, A, wrench_row=None, vehicle_row=None, wind_row=None, units=RELATIVE):
    """-> (next state [n, 27], reward [n], terminated [n]) of ``step64``, the bounds (state [n, 27], reward [n]) on
    |float32 result - reference|, and the mask [n] of envs whose termination is undecided."""
    c = _cfg(cfg)
    ref_ns, ref_r, ref_t = step64(cfg, P, S, A, wrench_row, vehicle_row, wind_row, units)
    k = _constants(c, P, S, wrench_row, vehicle_row, wind_row, units)
    P64, S64, A64 = _f64(P), _f64(S), _f64(A)
    rmin, rmax = P64[:, 22], P64[:, 23]
    half = scaled(sub(rmax, rmin), 0.5)
    mid = add(rmin, half)
    ac = [V(np.clip(A64[:, i], -1.0, 1.0)) for i in range(4)]
    sp = [fma(ac[i], half, mid) for i in range(4)]
    dt = V(np.float64(c["dt"]))
    hdt, dt6, dt3 = scaled(dt, 0.5), div(c["dt"], 6.0), div(c["dt"], 3.0)
    y0 = [V(S64[:, i]) for i in range(17)]
    kk = _dynamics(k, y0, sp)
    acc = [fma(dt6, kk[i], y0[i]) for i in range(17)]
    yt = [fma(hdt, kk[i], y0[i]) for i in range(17)]
    kk = _dynamics(k, yt, sp)
    acc = [fma(dt3, kk[i], acc[i]) for i in range(17)]
    yt = [fma(hdt, kk[i], y0[i]) for i in range(17)]
    kk = _dynamics(k, yt, sp)
    acc = [fma(dt3, kk[i], acc[i]) for i in range(17)]
    yt = [fma(dt, kk[i], y0[i]) for i in range(17)]
    kk = _dynamics(k, yt, sp)
    y = [fma(dt6, kk[i], acc[i]) for i in range(17)]
    sq = add(fma(y[4], y[4], mul(y[3], y[3])), fma(y[5], y[5], mul(y[6], y[6])))
    eq = clamp(sub(1.0, sq), -0.5, 0.5)
    inq = fma(eq, fma(0.375, eq, 0.5), 1.0)
    for i in range(3, 7):
        y[i] = mul(y[i], inq)
    for i in range(13, 17):
        y[i] = clamp(y[i], rmin, rmax)
    # termination: decided where the reference is further from the threshold than its bound
    undecided = np.zeros(S64.shape[0], bool)
    if c["termination_enabled"]:
        for idx, thr in (((0, 1, 2), c["termination_position"]), ((7, 8, 9), c["termination_linear_velocity"]),
                         ((10, 11, 12), c["termination_angular_velocity"])):
            for i in idx:
                with np.errstate(invalid="ignore"):
                    undecided |= np.abs(np.abs(y[i].x) - thr) <= y[i].e
    pc = fma(y[2], y[2], fma(y[1], y[1], mul(y[0], y[0])))
    oc = fma(neg(y[3]), y[3], 1.0)
    vc = fma(y[9], y[9], fma(y[8], y[8], mul(y[7], y[7])))
    wc = fma(y[12], y[12], fma(y[11], y[11], mul(y[10], y[10])))
    dev = [sub(ac[i], P64[:, 25]) for i in range(4)]
    acst = fma(dev[3], dev[3], fma(dev[2], dev[2], fma(dev[1], dev[1], mul(dev[0], dev[0]))))
    cost = fma(c["reward_action"], acst, fma(c["reward_angular_velocity"], wc, fma(c["reward_linear_velocity"], vc,
               fma(c["reward_orientation"], oc, mul(c["reward_position"], pc)))))
    reward = fma(-c["reward_scale"], cost, c["reward_constant"])
    bound_ns = np.zeros_like(ref_ns)
    value = ref_ns.copy()
    for i in range(17):
        bound_ns[:, i], value[:, i] = y[i].e, y[i].x
    bound_r = np.where(ref_t, 0.0, reward.e)
    value_r = np.where(ref_t, c["reward_termination_penalty"], reward.x)
    # the two texts agree to float64 rounding
    with np.errstate(invalid="ignore"):
        finite = np.isfinite(ref_ns).all(1) & np.isfinite(bound_ns).all(1)
        assert (np.abs(value - ref_ns)[finite] <= 2.0 ** -20 * bound_ns[finite]).all(), "step64 and the operation walk disagree (state)"
        ok = finite & ~undecided
        assert (np.abs(value_r - ref_r)[ok] <= 2.0 ** -20 * bound_r[ok]).all(), "step64 and the operation walk disagree (reward)"
    return (ref_ns, ref_r, ref_t), (bound_ns, bound_r), undecided


def observe_bound(P, S):
    """-> (observe64's [n, 26], the bound [n, 26])"""
    ref = observe64(P, S)
    P64, S64 = _f64(P), _f64(S)
    w, x, y, z = (V(S64[:, 3 + i]) for i in range(4))
    xx, yy, zz, xy, xz, yz = mul(x, x), mul(y, y), mul(z, z), mul(x, y), mul(x, z), mul(y, z)
    wx, wy, wz = mul(w, x), mul(w, y), mul(w, z)
    R = [fma(-2.0, add(yy, zz), 1.0), scaled(sub(xy, wz), 2.0), scaled(add(xz, wy), 2.0),
         scaled(add(xy, wz), 2.0), fma(-2.0, add(xx, zz), 1.0), scaled(sub(yz, wx), 2.0),
         scaled(sub(xz, wy), 2.0), scaled(add(yz, wx), 2.0), fma(-2.0, add(xx, yy), 1.0)]
    inv = div(2.0, sub(P64[:, 23], P64[:, 22]))
    rot = [fma(sub(S64[:, 13 + i], P64[:, 22]), inv, -1.0) for i in range(4)]
    bound, value = np.zeros_like(ref), ref.copy()
    for j, v in list(enumerate(R, 3)) + list(enumerate(rot, 22)):
        bound[:, j], value[:, j] = v.e, v.x
    assert (np.abs(value - ref) <= 2.0 ** -20 * bound).all(), "observe64 and the operation walk disagree"
    return ref, bound


def ratio(got, ref, bound):
    """|got - ref| / (bound (1 + 2^-20)), element-wise; 0 where both the error and the bound are 0, inf where got is not finite or the
    error is positive on a bound of 0"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64) * SLACK
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        r = np.where(err == 0, 0.0, err / bound)
    return np.where(np.isfinite(got) & np.isfinite(r), r, np.inf)


# ------------------------------------------------------------------ 3. the families -----
PARAM_FAMILIES = ["nominal", "sampled", "smallest", "largest", "fast_motors", "composed"]
STATE_FAMILIES = ["initial", "hover", "tumbling", "fast", "near_edge", "off_unit", "rotor_rails"]
ACTION_FAMILIES = ["inside", "clipped", "rails", "crossing"]


def _finish(P, g):
    """hover rotor speed and hover action of the fields, float64 then float32"""
    p = P.astype(np.float64)
    thrust = p[:, 0] * g / 4.0
    hover = (np.sqrt(p[:, 17] ** 2 - 4.0 * p[:, 18] * (p[:, 16] - thrust)) - p[:, 17]) / (2.0 * p[:, 18])
    P[:, 24] = hover
    P[:, 25] = 2.0 * (P[:, 24].astype(np.float64) - p[:, 22]) / (p[:, 23] - p[:, 22]) - 1.0
    return P


def _frames(cfg, scale, r):
    """the specification's scaling laws at ``scale`` [n], the rest drawn from the config's ranges"""
    n = scale.shape[0]
    g = float(np.float32(cfg.gravity))
    P = np.zeros((n, 26), np.float64)
    t2w = r.uniform(cfg.dr_thrust_to_weight_min, cfg.dr_thrust_to_weight_max, n)
    P[:, 0] = 0.027 * scale ** 3
    P[:, 1:4] = np.array([3.85e-6, 3.85e-6, 5.9675e-6])[None] * (scale ** 5)[:, None]
    arm = 0.028 * scale
    P[:, 4:16] = (np.array([[1, -1, 0], [-1, -1, 0], [-1, 1, 0], [1, 1, 0]], np.float64)[None] * arm[:, None, None]).reshape(n, 12)
    P[:, 23] = 20000.0 / np.sqrt(scale)
    P[:, 18] = t2w * P[:, 0] * g / (4.0 * P[:, 23] ** 2)
    P[:, 19] = r.uniform(cfg.dr_torque_const_min, cfg.dr_torque_const_max, n) * scale
    P[:, 20] = P[:, 21] = r.uniform(cfg.dr_motor_tau_min, cfg.dr_motor_tau_max, n)
    return _finish(P.astype(np.float32), g)


def params(name, n, seed, cfg, sampled=None):
    """-> (P float32 [n, 26], vehicle row float32 [n, 4] or None).  ``sampled``: [n, 26] from the sampler at the default domain
    randomisation, which ``sampled``, ``fast_motors`` and ``composed`` start from."""
    assert name in PARAM_FAMILIES, name
    r = np.random.default_rng([seed, PARAM_FAMILIES.index(name)])
    g = float(np.float32(cfg.gravity))
    if name == "nominal":
        P = np.zeros((n, 26), np.float32)
        P[:, 0], P[:, 1:4] = 0.027, [3.85e-6, 3.85e-6, 5.9675e-6]
        P[:, 4:16] = np.array([[1, -1, 0], [-1, -1, 0], [-1, 1, 0], [1, 1, 0]], np.float32).reshape(12) * np.float32(0.028)
        P[:, 18], P[:, 19], P[:, 20:22], P[:, 23] = 3.16e-10, 0.005964552, 0.15, 21702.0
        return _finish(P, g), None
    if name == "smallest":
        return _frames(cfg, np.full(n, 0.5), r), None
    if name == "largest":
        return _frames(cfg, np.full(n, LARGEST_SCALE), r), None
    assert sampled is not None and sampled.shape == (n, 26) and sampled.dtype == np.float32, "this family starts from the sampler's parameters"
    P = sampled.copy()
    if name == "fast_motors":                # the quickest rise of the range against the longest dt, and a fall that differs
        P[:, 20], P[:, 21] = 0.03, r.uniform(0.03, 0.2, n)
        return P, None
    if name == "composed":
        return P, np.exp(r.uniform(np.log(0.5), np.log(2.0), (n, 4))).astype(np.float32)
    return P, None


def _generic(cfg, P, r):
    n = P.shape[0]
    p = P.astype(np.float64)
    S = np.zeros((n, 27))
    S[:, 0:3] = r.uniform(-0.5, 0.5, (n, 3))
    axis = r.standard_normal((n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    half = r.uniform(0.0, np.pi / 4, n)
    S[:, 3], S[:, 4:7] = np.cos(half), axis * np.sin(half)[:, None]
    S[:, 7:10] = r.uniform(-1.0, 1.0, (n, 3))
    S[:, 10:13] = r.uniform(-1.0, 1.0, (n, 3))
    S[:, 13:17] = np.clip(p[:, 24:25] * r.uniform(0.6, 1.4, (n, 4)), p[:, 22:23], p[:, 23:24])
    S[:, 17:21] = r.uniform(-1.0, 1.0, (n, 4))
    mg = p[:, 0] * float(cfg.gravity)
    S[:, 21:24] = 0.05 * mg[:, None] * r.standard_normal((n, 3))
    S[:, 24:27] = 0.02 * (mg * np.hypot(p[:, 4], p[:, 5]))[:, None] * r.standard_normal((n, 3))
    return S


def _directions(r, n, top):
    """[n, 3] of length top * u^3, u uniform: a third of them above 0.3 top, the rest down to nothing; top a number or [n]"""
    d = r.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True) * (top * r.uniform(0.0, 1.0, n) ** 3)[..., None]


def states(name, n, seed, cfg, P, sampled=None):
    """-> S float32 [n, 27].  ``sampled``: the sampler's initial states of P, which ``initial`` is."""
    assert name in STATE_FAMILIES, name
    r = np.random.default_rng([seed, 100 + STATE_FAMILIES.index(name)])
    if name == "initial":
        assert sampled is not None and sampled.shape == (n, 27) and sampled.dtype == np.float32
        return sampled.copy()
    S = _generic(cfg, P, r)
    i = np.arange(n)
    if name == "hover":
        S[:, 0:3], S[:, 3], S[:, 4:7], S[:, 7:13], S[:, 21:27] = 0.0, 1.0, 0.0, 0.0, 0.0
        S[:, 13:17] = P[:, 24:25]
    elif name == "tumbling":
        # RK4 is stable on the imaginary axis up to |lambda| dt = 2 sqrt(2); the free body's largest rate is 0.55 |w| ((Jz - Jx) / Jx
        # of these frames), the quaternion's |w| / 2: beyond |w| dt = 5 the step itself diverges (|w'| reaches 1e5 at dt = 20 ms),
        # the bound is as large as the value and the termination of every eighth such env is undecided.  Seven of eight envs
        # stay inside that limit, every eighth goes up to 0.9 x the threshold whatever dt: the clamp's regime, held to its
        # (large) bound like the rest.
        top = 0.9 * float(cfg.termination_angular_velocity)
        S[:, 10:13] = _directions(r, n, np.where(i % 8 == 0, top, np.minimum(top, 5.0 / float(cfg.dt))))
    elif name == "fast":
        S[:, 7:10] = _directions(r, n, 0.9 * float(cfg.termination_linear_velocity))
    elif name == "near_edge":
        S[:, 7:10] *= 0.01
        side = np.where(i % 2 == 0, 1.0 - 1e-3, 1.0 + 1e-3) * np.where((i // 2) % 2 == 0, 1.0, -1.0)
        S[i, i % 3] = side * float(cfg.termination_position)
    elif name == "off_unit":
        S[:, 3:7] *= r.uniform(0.8, 1.2, n)[:, None]
    elif name == "rotor_rails":
        bits = (i[:, None] >> np.arange(4)[None]) & 1
        S[:, 13:17] = np.where(bits == 1, P[:, 23:24], P[:, 22:23])
    return S.astype(np.float32)


def actions(name, n, seed, cfg, P, S):
    """-> A float32 [n, 4]"""
    assert name in ACTION_FAMILIES, name
    r = np.random.default_rng([seed, 200 + ACTION_FAMILIES.index(name)])
    if name == "inside":
        A = r.uniform(-1.0, 1.0, (n, 4))
    elif name == "clipped":
        A = r.uniform(-3.0, 3.0, (n, 4))
    elif name == "rails":
        pick = r.integers(0, 3, (n, 4))
        A = np.where(pick == 0, -1.0, np.where(pick == 1, 1.0, P[:, 25:26].astype(np.float64)))
    else:                                    # the set-point within 1e-4 relative of the rotor's speed; a quarter as close as float32 gets
        delta = np.where(r.integers(0, 4, (n, 4)) == 0, 0.0, r.uniform(-1e-4, 1e-4, (n, 4)))
        p = P.astype(np.float64)
        A = 2.0 * (S[:, 13:17].astype(np.float64) * (1.0 + delta) - p[:, 22:23]) / (p[:, 23:24] - p[:, 22:23]) - 1.0
    return A.astype(np.float32)


def mixed(n, seed, cfg, P, sampled_states, state_names=STATE_FAMILIES, action_names=ACTION_FAMILIES):
    """One batch that holds every state x action family: env i takes state family i mod 7 and action family (i div 7) mod 4.
    -> S [n, 27], A [n, 4], the state family index [n], the action family index [n]"""
    i = np.arange(n)
    si, ai = i % len(state_names), (i // len(state_names)) % len(action_names)
    S = np.stack([states(s, n, seed, cfg, P, sampled_states) for s in state_names])[si, i]
    A = np.stack([actions(a, n, seed, cfg, P, S) for a in action_names])[ai, i]
    return np.ascontiguousarray(S), np.ascontiguousarray(A), si, ai


def schedule_rows(kind, n, seed, cfg, P):
    """One schedule row per env, float32: ``wrench`` [n, 6] in relative units (force up to 0.5 m g, torque up to 0.1 m g arm),
    ``wrench_absolute`` the same pushes in N and N m, ``vehicle`` [n, 4] factors in [0.5, 2], ``wind`` [n, 4] air up to 8 m/s per
    axis and a drag in [0, 0.7] / s, every fifth (rows 4, 9, ...) exactly 0."""
    r = np.random.default_rng([seed, 300 + ["wrench", "wrench_absolute", "vehicle", "wind"].index(kind)])
    if kind == "vehicle":
        return np.exp(r.uniform(np.log(0.5), np.log(2.0), (n, 4))).astype(np.float32)
    if kind == "wind":
        drag = np.where(np.arange(n) % 5 == 4, 0.0, r.uniform(0.0, 0.7, n))
        return np.concatenate([r.uniform(-8.0, 8.0, (n, 3)), drag[:, None]], axis=1).astype(np.float32)
    row = np.concatenate([r.uniform(-0.5, 0.5, (n, 3)), r.uniform(-0.1, 0.1, (n, 3))], axis=1)
    if kind == "wrench_absolute":
        p = P.astype(np.float64)
        mg = p[:, 0] * float(cfg.gravity)
        row[:, 0:3] *= mg[:, None]
        row[:, 3:6] *= (mg * np.hypot(p[:, 4], p[:, 5]))[:, None]
    return row.astype(np.float32)


# ------------------------------------------------------------------ 4. the series -----
def series_table(products=(0.01, 0.1, 0.5, 1.0, 1.5, 1.8, 2.0, 3.0, 5.0, 10.0, 18.0), scales=(0.8, 0.9, 1.1, 1.2)):
    """What the specified series does.  Rows (|w| dt, e before the pull-back, | |q'| - 1 | after it, in ulps of 1 = 2^-23) for one
    float64 RK4 step of dq = q (x) (0, w) / 2 from a unit quaternion about a fixed axis; then rows (|q| set, | |q'| - 1 | after
    one step at rest, after two) for the off-unit states."""
    def pulled(sq):
        e = np.clip(1.0 - sq, -0.5, 0.5)
        return np.sqrt(sq) * (1.0 + e * (0.5 + 3.0 * e / 8.0)), e
    spinning = []
    for x in products:
        q, w = np.array([[1.0, 0.0, 0.0, 0.0]]), np.array([[0.0, 0.6 * x, 0.0, 0.8 * x]])      # dt = 1
        f = lambda q: 0.5 * qmul(q, w)
        k1 = f(q); k2 = f(q + k1 / 2); k3 = f(q + k2 / 2); k4 = f(q + k3)
        norm, e = pulled(((q + (k1 + 2 * k2 + 2 * k3 + k4) / 6) ** 2).sum())
        spinning.append((x, float(e), abs(float(norm) - 1.0) / 2.0 ** -23))
    off = []
    for s in scales:
        once, _ = pulled(s * s)
        twice, _ = pulled(once * once)
        off.append((s, abs(float(once) - 1.0), abs(float(twice) - 1.0)))
    return spinning, off
