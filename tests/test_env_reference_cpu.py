"""tests/env_reference.py proved on the CPU: the oracle - the kernels' bit-identical stand-in wherever the bit-exact suites reach -
lies inside the float64 bound on every param x state x action family x dt, with schedule rows too; every altered reference puts it
outside; the undecided envs are capped; and the module's own ODE under scipy ties it to physics.  (pytest -s prints the ratios.)"""
import numpy as np
import pytest

import env_reference as R
from raptor_amd import disturbances, vehicles, winds

N = 257
SEED = 3
KINDS = ["wrench", "wrench_absolute", "vehicle", "wind", "all"]


def config(oracle, dt):
    cfg = oracle.default_config()
    cfg.dt = dt
    return cfg


def fleet(oracle, cfg, pf, n=N):
    """-> P, the family's vehicle row or None, the sampler's initial states of P"""
    sampled = oracle.sample_initial_parameters(oracle.default_config(), SEED, 0, 0, n)
    P, vrow = R.params(pf, n, SEED, cfg, sampled)
    return P, vrow, oracle.sample_initial_state(cfg, SEED, np.zeros(n, np.uint32), 0, P)


def rows_of(kind, n, cfg, P):
    """-> dict(wrench_row, vehicle_row, wind_row, units) for step64"""
    kw = {}
    if kind in ("wrench", "wrench_absolute", "all"):
        kw["wrench_row"] = R.schedule_rows("wrench" if kind == "all" else kind, n, SEED, cfg, P)
        kw["units"] = R.ABSOLUTE if kind == "wrench_absolute" else R.RELATIVE
    if kind in ("vehicle", "all"):
        kw["vehicle_row"] = R.schedule_rows("vehicle", n, SEED, cfg, P)
    if kind in ("wind", "all"):
        kw["wind_row"] = R.schedule_rows("wind", n, SEED, cfg, P)
    return kw


def oracle_step(oracle, cfg, P, S, A, wrench_row=None, vehicle_row=None, wind_row=None, units=R.RELATIVE):
    """what a caller gets who writes compose(...) before the step: the next state keeps the state's own wrench columns"""
    Pe = P if vehicle_row is None else vehicles.compose(P, vehicle_row)
    W = S[:, 21:27]
    if wrench_row is not None:
        W = disturbances.compose(W, Pe[:, 0], cfg.gravity, Pe[:, 4:6], wrench_row, units)
    if wind_row is not None:
        W = winds.compose(W, Pe[:, 0], S[:, 7:10], wind_row)
    Se = S.copy()
    Se[:, 21:27] = W
    ns, r, t = oracle.step(cfg, Pe, Se, A)
    ns[:, 21:27] = S[:, 21:27]
    return ns, r, t


def held(got, want, what):
    """got (ns, r, t) against step_bound's answer -> the largest ratio of the state and of the reward; asserts"""
    (ns, r, t), (bn, br), undecided = want
    ratio = R.ratio(got[0], ns, bn)
    bad = np.argwhere(ratio > 1.0)
    assert bad.size == 0, f"{what}: state outside the bound at env {bad[0][0]}, column {bad[0][1]}: ratio {ratio[tuple(bad[0])]:.3g}"
    ok = ~undecided
    assert np.array_equal(np.asarray(got[2])[ok] != 0, t[ok]), f"{what}: terminated differs on decided envs"
    rr = R.ratio(np.asarray(got[1])[ok], r[ok], br[ok])
    assert (rr <= 1.0).all(), f"{what}: reward outside the bound: ratio {rr.max():.3g}"
    return float(ratio.max()), float(rr.max()) if ok.any() else 0.0


def capped(want, sf, what):
    """on the reference alone: at most 1 % undecided; near_edge on both sides of the threshold and outside its own bound"""
    (_, _, t), _, undecided = want
    assert undecided.mean() <= 0.01, f"{what}: {undecided.sum()} of {undecided.size} envs undecided"
    if sf == "near_edge":
        assert undecided.sum() == 0 and 0.2 <= t.mean() <= 0.8, (what, int(undecided.sum()), float(t.mean()))


@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("pf", R.PARAM_FAMILIES)
def test_the_oracle_step_lies_inside_the_bound(oracle, pf, dt):
    cfg = config(oracle, dt)
    P, vrow, sampled = fleet(oracle, cfg, pf)
    worst = {}
    for sf in R.STATE_FAMILIES:
        S = R.states(sf, N, SEED, cfg, P, sampled)
        for af in R.ACTION_FAMILIES:
            A = R.actions(af, N, SEED, cfg, P, S)
            what = f"{pf} {sf} {af} dt={dt}"
            want = R.step_bound(cfg, P, S, A, vehicle_row=vrow)
            capped(want, sf, what)
            worst[sf, af] = held(oracle_step(oracle, cfg, P, S, A, vehicle_row=vrow), want, what)
    for sf in R.STATE_FAMILIES:
        print(f"step {pf:12s} dt={dt:<6} {sf:12s} state {max(worst[sf, a][0] for a in R.ACTION_FAMILIES):.3f} "
              f"reward {max(worst[sf, a][1] for a in R.ACTION_FAMILIES):.3f}")


@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("kind", KINDS)
def test_schedule_rows_as_physics_hold_the_composed_oracle_step(oracle, kind, dt):
    cfg = config(oracle, dt)
    n = 7 * N
    for pf in ("sampled", "smallest", "largest"):
        P, _, sampled = fleet(oracle, cfg, pf, n)
        S, A, si, _ = R.mixed(n, SEED, cfg, P, sampled)
        kw = rows_of(kind, n, cfg, P)
        want = R.step_bound(cfg, P, S, A, **kw)
        assert want[2].mean() <= 0.01
        worst = held(oracle_step(oracle, cfg, P, S, A, **kw), want, f"{kind} {pf} dt={dt}")
        print(f"rows {kind:16s} {pf:9s} dt={dt:<6} state {worst[0]:.3f} reward {worst[1]:.3f}")
        plain = R.step64(cfg, P, S, A)[0]
        assert (np.abs(plain - want[0][0]) > want[1][0]).any(1).mean() > 0.75         # the rows do move the step (a fifth of the winds has no drag)


# every mistake on every param family it applies to: rotors that rise and fall alike cannot show an exchange of the two time
# constants, and fast_motors is the family whose rotors do not
CONTROLS = [(m, pf) for m in R.MISTAKES for pf in R.PARAM_FAMILIES if R.NEEDS.get(m) != "tau_differ" or pf == "fast_motors"]


@pytest.mark.parametrize("mistake, pf", CONTROLS)
def test_every_altered_reference_puts_the_oracle_outside(oracle, mistake, pf):
    """a bound loose enough to hide one of these mistakes would be the failure"""
    cfg = config(oracle, 0.01)
    n = 4 * N
    P, vrow, sampled = fleet(oracle, cfg, pf, n)
    S, A, _, _ = R.mixed(n, SEED, cfg, P, sampled)
    need = R.NEEDS.get(mistake)
    kw = rows_of(need, n, cfg, P) if need in ("wrench", "vehicle", "wind") else {}
    if vrow is not None:
        kw["vehicle_row"] = vrow
    want = R.step_bound(cfg, P, S, A, **kw)
    got = oracle_step(oracle, cfg, P, S, A, **kw)
    held(got, want, f"{mistake} {pf}: the unaltered reference")
    ns, r, _ = R.altered(mistake)(cfg, P, S, A, **kw)
    out_state = (R.ratio(got[0], ns, want[1][0]) > 1.0).any(1)
    out_reward = R.ratio(got[1], r, want[1][1]) > 1.0
    outside = out_state | (out_reward & ~want[2] & ~want[0][2])
    print(f"altered {mistake:30s} {pf:12s} outside on {outside.mean():.3f} of the envs")
    assert outside.any()


@pytest.mark.parametrize("pf", R.PARAM_FAMILIES)
def test_the_oracle_observation_lies_inside_the_bound(oracle, pf):
    cfg = config(oracle, 0.01)
    P, _, sampled = fleet(oracle, cfg, pf)
    for sf in R.STATE_FAMILIES:
        S = R.states(sf, N, SEED, cfg, P, sampled)
        ref, bound = R.observe_bound(P, S)
        got = oracle.observe(cfg, 0, 0, 0, P, S)
        ratio = R.ratio(got, ref, bound)
        print(f"observe {pf:12s} {sf:12s} {ratio.max():.3f}")
        assert (ratio <= 1.0).all(), (pf, sf, float(ratio.max()))
        # columns 3..11 are R(q) row-major: the third column is the body z axis in the world frame
        q = S[:, 3:7].astype(np.float64)
        assert np.allclose(ref[:, 3:12].reshape(-1, 3, 3)[:, :, 2], R.rotation(q) @ np.array([0.0, 0.0, 1.0]))
        if sf == "rotor_rails":
            assert np.isin(ref[:, 22:26], (-1.0, 1.0)).all()


def test_an_altered_observation_is_outside(oracle):
    """the bound of the observation is tight enough to tell a transposed rotation matrix"""
    cfg = config(oracle, 0.01)
    P, _, sampled = fleet(oracle, cfg, "sampled")
    ref, bound = R.observe_bound(P, sampled)
    got = oracle.observe(cfg, 0, 0, 0, P, sampled)
    transposed = ref.copy()
    transposed[:, 3:12] = ref[:, 3:12].reshape(-1, 3, 3).transpose(0, 2, 1).reshape(-1, 9)
    assert (R.ratio(got, transposed, bound) > 1.0).any(1).mean() > 0.8


def test_quarter_steps_of_step64_against_an_adaptive_integrator(oracle):
    """step64 at dt / 4 taken four times against scipy's solve_ivp on the module's own ODE, rtol 1e-10: the 1e-3 of
    tests/test_oracle_env.py::test_step_matches_independent_float64_integration, so the module is tied to physics"""
    from scipy.integrate import solve_ivp
    n = 16
    cfg = config(oracle, 0.01)
    cfg.termination_enabled = 0
    P, _, sampled = fleet(oracle, cfg, "sampled", n)
    S = R.states("tumbling", n, SEED, cfg, P)
    S[:, 10:13] = R.states("initial", n, SEED, cfg, P, sampled)[:, 10:13] * 8.0          # a tumble an integrator can follow
    A = R.actions("inside", n, SEED, cfg, P, S)
    s = S
    for _ in range(4):
        s = R.step64(cfg, P, s, A, dt=float(cfg.dt) / 4)[0].astype(np.float32)          # (a float32 state between the quarters: 6e-8)
    veh = R.Vehicle(R._cfg(cfg), P, S, None, None, None, R.RELATIVE, None)
    p = P.astype(np.float64)
    sp = p[:, 22:23] + (np.clip(A.astype(np.float64), -1, 1) + 1) / 2 * (p[:, 23:24] - p[:, 22:23])
    worst = 0.0
    for i in range(n):
        one = R.Vehicle(R._cfg(cfg), P[i:i + 1], S[i:i + 1], None, None, None, R.RELATIVE, None)
        sol = solve_ivp(lambda t, y: one.ode(y[None], sp[i:i + 1])[0], (0.0, float(cfg.dt)), S[i, :17].astype(np.float64),
                        rtol=1e-10, atol=1e-12)
        ref = sol.y[:, -1]
        ref[3:7] /= np.linalg.norm(ref[3:7])
        err = np.abs(s[i, :17] - ref) / np.maximum(np.abs(ref), 1.0)
        worst = max(worst, float(err.max()))
        assert err.max() < 1e-3, (i, err)
    print(f"quarter steps against solve_ivp: largest relative error {worst:.3g}")
    assert veh.m.shape == (n,)


def test_the_series_against_exact_normalisation():
    """for which |w| dt the specified 1/|q| series stays within one float32 ulp of q / |q|, and what it does beyond"""
    spinning, off = R.series_table()
    print("|w| dt      e          | |q'| - 1 | in ulps of 1")
    for x, e, ulps in spinning:
        print(f"{x:6.2f}  {e:10.3e}  {ulps:12.3g}")
    print("|q| set   | |q'| - 1 | after one step   after two")
    for s, once, twice in off:
        print(f"{s:6.2f}  {once:10.3e}  {twice:10.3e}")
    ulps = {x: u for x, _, u in spinning}
    assert all(u <= 1.0 for x, u in ulps.items() if x <= 1.8), ulps          # the figure DESIGN.md section 2 states
    assert 1.0 < ulps[2.0] < 8.0 and 1e-4 < ulps[3.0] * 2.0 ** -23 < 1e-3     # beyond: ulps, then a fraction of a per cent,
    assert 0.2 < ulps[5.0] * 2.0 ** -23 < 0.5 and all(np.isfinite(u) for u in ulps.values())   # then the clamp: a third, and finite
    assert all(once < 0.024 and twice < 3.2e-5 for _, once, twice in off)
    # the series is what step64 applies; exact_unit is what it approximates
    q = np.array([[0.9, 0.1, -0.2, 0.3]])
    e = 1.0 - (q ** 2).sum()
    assert np.allclose(q * (1 + e * (0.5 + 3 * e / 8)), R.exact_unit(q), atol=5 * abs(e) ** 3 / 16 * 1.3)
