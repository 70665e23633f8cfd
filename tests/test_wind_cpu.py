"""The host side of the wind schedule without a GPU: the four entry points are declared, bound and exported, what needs no device is
refused with its message before the device is looked at, ``winds.compose`` against the rule written out per operation (and against a
fused restatement, which differs), the table builders, the Python surface's refusals before any library call, and the closed
form of the oracle's step fed the composed force."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ("rq_wind_bank_create", "rq_wind_bank_destroy", "rq_env_set_wind_schedule", "rq_env_get_wind_schedule")
S_VEL, S_FORCE, S_WRENCH = slice(7, 10), slice(21, 24), slice(21, 27)        # RQ_S_* linear velocity, force, force | torque
P_MASS = 0


def test_entry_points_are_declared_bound_and_exported():
    from raptor_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "raptor_quad.h")).read()
    dynamic = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        m = re.search(r"RQ_API int %s\(([^;]*)\);" % name, hdr, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib._SIGNATURES[name]), name
        assert re.search(r" T %s$" % name, dynamic, re.M), name
        assert "`%s`" % name in table, name
    assert lib.rq_abi_version() == 5 and _lib.ABI_VERSION == 5
    assert int(re.search(r"#define RQ_ABI_VERSION (\d+)", hdr).group(1)) == 5
    assert re.search(r"still 5: rq_wind_bank_\{create,destroy\}", hdr)
    assert "zero-order hold" in hdr.lower() and "Wind schedule" in hdr


def test_what_needs_no_device_is_refused_first():
    import ctypes as C
    from raptor_amd import _lib
    lib = _lib.load()
    h = C.c_void_p(4096)                     # never followed: everything below is refused before the device is looked at
    rows = (C.c_float * 8)(*([1.0] * 8))
    out = C.c_void_p()
    for args in ((None, rows, 1, 1, C.byref(out)), (h, None, 1, 1, C.byref(out)), (h, rows, 1, 1, None)):
        assert lib.rq_wind_bank_create(*args) == -1
        assert b"null argument" in lib.rq_last_error()
    assert lib.rq_wind_bank_create(h, rows, 0, 1, C.byref(out)) == -1 and b"at least one table" in lib.rq_last_error()
    assert lib.rq_wind_bank_create(h, rows, 1, 0, C.byref(out)) == -1 and b"at least one row" in lib.rq_last_error()
    assert lib.rq_wind_bank_create(h, rows, 1 << 14, 1 << 14, C.byref(out)) == -1 and b"2^28" in lib.rq_last_error()
    # a non-finite entry in any column, a negative drag in column 3: the message names table, row and column
    for value in (float("nan"), float("inf"), -float("inf")):
        for col in (1, 3):
            rows[4 + col] = value
            assert lib.rq_wind_bank_create(h, rows, 1, 2, C.byref(out)) == -1
            msg = lib.rq_last_error()
            assert b"non-finite entry" in msg and b"table 0, row 1, column %d" % col in msg, msg
            assert lib.rq_wind_bank_create(h, rows, 2, 1, C.byref(out)) == -1
            assert b"table 1, row 0, column %d" % col in lib.rq_last_error()
            rows[4 + col] = 1.0
    rows[7] = -0.25
    assert lib.rq_wind_bank_create(h, rows, 1, 2, C.byref(out)) == -1
    msg = lib.rq_last_error()
    assert b"negative drag" in msg and b"table 0, row 1, column 3" in msg, msg
    assert lib.rq_wind_bank_create(h, rows, 2, 1, C.byref(out)) == -1 and b"table 1, row 0, column 3" in lib.rq_last_error()
    assert not out.value
    assert lib.rq_wind_bank_destroy(None) == 0
    ids = (C.c_uint32 * 1)(0)
    assert lib.rq_env_set_wind_schedule(None, h, ids) == -1 and b"null argument" in lib.rq_last_error()
    assert lib.rq_env_set_wind_schedule(None, None, None) == -1 and b"null argument" in lib.rq_last_error()
    assert lib.rq_env_get_wind_schedule(None, C.byref(out), ids) == -1 and b"null argument" in lib.rq_last_error()
    assert lib.rq_env_get_wind_schedule(h, None, ids) == -1 and b"null argument" in lib.rq_last_error()


def _inputs(n, seed=0):
    g = np.random.default_rng(seed)
    base = (g.standard_normal((n, 6)) * g.choice([1e-3, 0.1, 1.0], (n, 6))).astype(np.float32)
    mass = g.uniform(0.02, 2.0, n).astype(np.float32)
    vel = (g.standard_normal((n, 3)) * 3).astype(np.float32)
    row = np.concatenate([g.standard_normal((n, 3)) * 5, g.uniform(0.0, 1.5, (n, 1))], axis=1).astype(np.float32)
    return base, mass, vel, row


def test_compose_is_single_operation_float32_in_the_stated_order():
    from raptor_amd import winds as W
    f32 = np.float32
    n = 513
    base, mass, vel, row = _inputs(n)
    got = W.compose(base, mass, vel, row)
    assert got.dtype == f32 and got.shape == (n, 6)
    fused_differs = 0
    for i in range(n):
        md = f32(mass[i] * row[i, 3])
        for j in range(3):
            u = f32(row[i, j] - vel[i, j])
            want = f32(base[i, j] + f32(md * u))                 # three roundings, in this order
            assert got[i, j].view(np.uint32) == want.view(np.uint32), (i, j)
            fma = f32(np.float64(base[i, j]) + np.float64(md) * np.float64(u))       # the product kept exact: one rounding less
            fused_differs += int(fma.view(np.uint32) != want.view(np.uint32))
        assert np.array_equal(got[i, 3:6].view(np.uint32), base[i, 3:6].view(np.uint32))        # the torque is the base's
    assert fused_differs >= 1, "a fused multiply-add restatement gave the same bits on every input: the order would not matter"
    print(f"\n[winds.compose] a fused restatement differs on {fused_differs} of {3 * n} components")
    # another association differs too: (mass * d) * u is not mass * (d * u)
    other = (base[:, 0:3] + (mass[:, None] * (row[:, 3:4] * (row[:, 0:3] - vel)).astype(f32)).astype(f32)).astype(f32)
    assert (other.view(np.uint32) != got[:, 0:3].view(np.uint32)).any()
    # within three roundings of the exact value
    exact = base[:, 0:3].astype(np.float64) + (mass.astype(np.float64) * row[:, 3])[:, None] * (row[:, 0:3].astype(np.float64) - vel)
    scale = np.abs(base[:, 0:3]) + np.abs((mass * row[:, 3])[:, None] * (row[:, 0:3] - vel))
    assert (np.abs(got[:, 0:3] - exact) <= 3 * 2.0 ** -24 * scale + 1e-45).all()
    # d = 0 keeps the base's bits (no base here is -0); drifting with the wind feels nothing
    still = row.copy(); still[:, 3] = 0
    assert not (base.view(np.uint32) == 0x80000000).any()
    assert np.array_equal(W.compose(base, mass, vel, still).view(np.uint32), base.view(np.uint32))
    assert np.array_equal(W.compose(base, mass, row[:, 0:3], row).view(np.uint32), base.view(np.uint32))
    assert np.array_equal(W.compose(base, mass, vel, W.calm(1)[0]).view(np.uint32), base.view(np.uint32))        # a single row broadcasts
    before = base.copy()
    one = W.compose(base[3], mass[3], vel[3], row[3])
    assert one.shape == (6,) and np.array_equal(one, got[3]) and np.array_equal(base, before)
    for bad in (lambda: W.compose(base[:, :5], mass, vel, row), lambda: W.compose(base, mass, vel[:, :2], row),
                lambda: W.compose(base, mass, vel, row[:, :3])):
        with pytest.raises(ValueError, match="compose takes"):
            bad()


def test_builders_shapes_values_and_refusals():
    from raptor_amd import winds as W
    rows, dt = 60, 0.01
    t = np.arange(rows) * dt

    def same(table, want):
        assert table.dtype == np.float32 and table.shape == (rows, 4) and table.flags.c_contiguous
        assert np.array_equal(table, np.asarray(want, np.float64).astype(np.float32))

    zeros = np.zeros((rows, 4))
    same(W.calm(rows), zeros)
    want = zeros.copy(); want[:, 3] = 0.4
    same(W.still_air(rows, 0.4), want)
    want = zeros.copy(); want[:, 0:3] = (3, -1, 0.5); want[:, 3] = 0.5
    same(W.steady(rows, (3, -1, 0.5), 0.5), want)
    want = zeros.copy(); want[:, 3] = 0.3; want[11:31, 0:3] = (0, 4, 0)            # (edges between two steps: no rounding question)
    same(W.gust(rows, dt, (0, 4, 0), 0.105, 0.2, 0.3), want)
    want = zeros.copy(); want[:, 3] = 0.3; want[:, 0:3] = np.clip((t - 0.1) / 0.2, 0, 1)[:, None] * np.array([5.0, 0, -1])
    same(W.ramp(rows, dt, (5, 0, -1), 0.1, 0.2, 0.3), want)
    want = zeros.copy(); want[:, 3] = 0.3; want[t >= 0.1, 0] = 5
    same(W.ramp(rows, dt, (5, 0, 0), 0.1, 0.0, 0.3), want)            # rise 0: a step
    # turbulence: deterministic per seed, other seeds differ, the mean and the drag are what was asked for
    a, b, c = (W.turbulence(4000, dt, (3, 0, -1), 1.5, 0.5, 0.35, s) for s in (7, 7, 8))
    assert a.dtype == np.float32 and a.shape == (4000, 4) and np.isfinite(a).all()
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert (a[:, 3] == np.float32(0.35)).all()
    assert np.abs(a[:, 0:3].mean(0) - (3, 0, -1)).max() < 1.0 and 0.7 < a[:, 0:3].std(0).mean() < 2.3
    lag = np.corrcoef(a[:-50, 0], a[50:, 0])[0, 1]                    # 50 steps = tau: e^-1 = 0.37
    assert 0.1 < lag < 0.65, lag
    assert (W.turbulence(rows, dt, (1, 2, 3), 0.0, 1.0, 0.2, 0)[:, 0:3] == (1, 2, 3)).all()
    assert W.WIND_NAMES == ("wx", "wy", "wz", "drag")
    for bad in (lambda: W.calm(0), lambda: W.calm(2.5), lambda: W.still_air(5, -0.1), lambda: W.still_air(5, np.nan),
                lambda: W.steady(5, (1, 2), 0.3), lambda: W.steady(5, (1, np.inf, 0), 0.3), lambda: W.steady(5, (1, 0, 0), -1),
                lambda: W.gust(5, 0.0, (1, 0, 0), 0, 1, 0.3), lambda: W.gust(5, dt, (1, 0, 0), -1, 1, 0.3),
                lambda: W.gust(5, dt, (1, 0, 0), 0, -1, 0.3), lambda: W.ramp(5, dt, (1, 0, 0), 0, -1, 0.3),
                lambda: W.ramp(5, dt, (1, 0, 0), 0, 1, -0.3), lambda: W.turbulence(5, dt, (0, 0, 0), -1, 1, 0.3, 0),
                lambda: W.turbulence(5, dt, (0, 0, 0), 1, 0, 0.3, 0), lambda: W.turbulence(5, dt, (0, 0, 0), 1, 1, 0.3, -1),
                lambda: W.turbulence(5, dt, (0, 0, 0), 1, 1, 0.3, 0.5)):
        with pytest.raises(ValueError):
            bad()
    s = W.suite(500, dt)
    assert list(s) == ["calm", "still_air", "steady_2", "steady_5", "steady_8", "gust", "ramp", "turbulence"]
    for name, table in s.items():
        assert table.dtype == np.float32 and table.shape == (500, 4) and np.isfinite(table).all() and (table[:, 3] >= 0).all(), name
    assert (s["calm"] == 0).all() and len({x.tobytes() for x in s.values()}) == len(s)
    assert np.array_equal(s["steady_5"], W.steady(500, (5, 0, 0), W.DEFAULT_DRAG))
    assert W.check_tables(list(s.values())).shape == (len(s), 500, 4)


def test_python_refusals_come_before_any_library_call(monkeypatch):
    import raptor_amd.l2f as l2f
    from raptor_amd import _lib, winds
    from raptor_amd.policy_bank import PolicyBank, block_policy_assignment

    def no_call(name, *a):
        raise AssertionError("library call " + name)
    monkeypatch.setattr(_lib, "call", no_call)
    good = np.ones((3, 9, 4), np.float32)
    for value, col, name in ((np.nan, 2, "wz"), (np.inf, 0, "wx"), (-np.inf, 3, "drag"), (-1.0, 3, "drag")):
        bad = good.copy()
        bad[1, 4, col] = value
        with pytest.raises(ValueError, match=r"table 1, row 4, column %d \(%s\)" % (col, name)):
            l2f.WindBank(None, bad)
        with pytest.raises(ValueError, match=r"table 1, row 4, column %d" % col):
            winds.check_tables([good[0], bad[1]])
    ok = good.copy()
    ok[:, :, 0:3] = -7.0                                   # a negative velocity is a wind from the other side
    ok[:, :, 3] = 0.0
    assert winds.check_tables(ok).shape == (3, 9, 4)
    for tables, words in ((good.astype(np.float64), "float32"), (good[0], "shape"), (good[:, :, :3], "shape"), (good[:0], "shape"),
                          (np.ones((3, 9, 6), np.float32), "shape"), ([], "at least one table"),
                          ([good[0], good[1][:8]], "same number of rows"), ([good[0].astype(np.float64)], "float32"),
                          ([good[0][:, :3]], "shape")):
        with pytest.raises(ValueError, match=words):
            l2f.WindBank(None, tables)
    bank = l2f.WindBank.__new__(l2f.WindBank)              # no device, no handle
    bank.n_tables, bank.rows, bank._h = 3, 9, None
    n = 128
    vector = l2f.vector(n)
    env = vector.VectorEnvironment()
    assert env.wind_schedule is None
    ids = np.arange(n) % 3
    with pytest.raises(ValueError, match="l2f.WindBank"):
        env.set_wind_schedule(good, ids)
    with pytest.raises(ValueError, match="l2f.WindBank"):
        env.set_wind_schedule(None)
    vb = l2f.VehicleBank.__new__(l2f.VehicleBank)
    with pytest.raises(ValueError, match="l2f.WindBank"):
        env.set_wind_schedule(vb, ids)
    with pytest.raises(ValueError, match="one id per env: 64 ids for 128 envs"):
        env.set_wind_schedule(bank, ids[:64])
    with pytest.raises(ValueError, match="integers"):
        env.set_wind_schedule(bank, ids.astype(np.float32))
    with pytest.raises(ValueError, match="integers"):
        env.set_wind_schedule(bank, ids > 0)
    far = ids.copy()
    far[77] = 3
    with pytest.raises(ValueError, match="env 77 names table 3 of a bank of 3"):
        env.set_wind_schedule(bank, far)
    with pytest.raises(ValueError, match="env 77 names table 3 of a bank of 3"):
        winds.check_wind_ids(far, 3, n)
    far[5] = -1
    with pytest.raises(ValueError, match="env 5 names table -1"):
        env.set_wind_schedule(bank, far)
    assert env.wind_schedule is None
    env.clear_wind_schedule()                              # nothing attached, no handle: no call
    pb = PolicyBank.__new__(PolicyBank)
    pb.n_policies = 2
    pids = block_policy_assignment(n, 2)
    with pytest.raises(ValueError, match="attach one first"):
        pb.evaluate(vector, None, env, None, None, None, 1, pids, wind_ids=ids)
    env._wind = (bank, np.zeros(n, np.uint32))             # as set_wind_schedule leaves it
    got = env.wind_schedule
    assert got[0] is bank and np.array_equal(got[1], np.zeros(n, np.uint32))
    with pytest.raises(ValueError, match="env 77 names table 3"):
        far = ids.copy()
        far[77] = 3
        pb.evaluate(vector, None, env, None, None, None, 1, pids, wind_ids=far)
    rb = l2f.ReferenceBank.__new__(l2f.ReferenceBank)
    rb.n_references, rb.rows, rb._h = 3, 9, None
    with pytest.raises(ValueError, match="give one of them"):
        pb.evaluate(vector, None, env, None, None, None, 1, pids, reference=rb, reference_ids=ids, wind_ids=ids)
    # wind_ids beside wrench_ids or vehicle_ids is refused
    wb = l2f.WrenchBank.__new__(l2f.WrenchBank)
    wb.n_tables, wb.rows, wb._h, wb.units = 3, 9, None, "relative"
    env._wrench = (wb, np.zeros(n, np.uint32))
    vb.n_tables, vb.rows, vb._h = 3, 9, None
    env._vehicle = (vb, np.zeros(n, np.uint32))
    for kw in (dict(wrench_ids=ids), dict(vehicle_ids=ids)):
        with pytest.raises(ValueError, match="wind_ids .* give one of them"):
            pb.evaluate(vector, None, env, None, None, None, 1, pids, wind_ids=ids, **kw)


# ------------------------------------------------------------------ the closed form on the oracle ------
WIND, DRAG, STEPS = (3.0, 0.0, 0.0), 0.5, 100
# The float32 trace of the oracle against the float64 recurrence v_{k+1} = v_k + dt d (w - v_k), over 100 steps, measured on the CPU:
# the largest gap is 2.663e-05 m/s, at the last step (v_x = 1.18 m/s).  Nearly all of it is the hover's own float32 drift: in calm air
# the same vehicle reaches |v_x| = 3.0e-05 m/s in those 100 steps (the four rotor thrusts do not cancel to the last bit and the
# vehicle leans by 5e-06); against the still-air run the wind's share of the gap is 6.3e-07.  The tolerance is four times the gap.
MEASURED_GAP = 2.663e-05
TOLERANCE = 4 * MEASURED_GAP


def hover_world(oracle, n=4):
    """n nominal vehicles level at hover, rotors at hover speed, the hover action, termination off"""
    cfg = oracle.default_config()
    cfg.domain_randomization = 0
    cfg.termination_enabled = 0
    cfg.disturbance_force_std = 0.0
    cfg.disturbance_torque_std = 0.0
    P = oracle.sample_initial_parameters(cfg, 5, 0, 0, n)
    S = np.zeros((n, 27), np.float32)
    S[:, 3] = 1.0                            # q = identity
    S[:, 13:17] = P[:, 24:25]                # hover rotor speed
    act = np.repeat(P[:, 25:26], 4, axis=1).astype(np.float32)
    return cfg, P, S, act


def closed_form(dt, steps=STEPS):
    """v_x after k = 1 .. steps steps, float64: w_x (1 - (1 - d dt)^k)"""
    k = np.arange(1, steps + 1, dtype=np.float64)
    return WIND[0] * (1.0 - (1.0 - DRAG * float(dt)) ** k)


def oracle_trace(oracle, step=None, steps=STEPS):
    """The host loop that composes the drag itself: winds.compose into the force columns before every step -> (states [steps, n, 27]
    in the steady wind, in calm air (no drag: the plain step), in still air (w = 0, the same drag), cfg).
    step(cfg, P, S, act) -> next state; default the oracle's."""
    from raptor_amd import winds
    cfg, P, S0, act = hover_world(oracle)
    step = step or (lambda cfg, P, S, act: oracle.step(cfg, P, S, act)[0])
    traces = []
    for row in (winds.steady(1, WIND, DRAG)[0], None, winds.still_air(1, DRAG)[0]):
        S, trace = S0.copy(), []
        for _ in range(steps):
            fed = S.copy()
            if row is not None:
                fed[:, S_WRENCH] = winds.compose(S[:, S_WRENCH], P[:, P_MASS], S[:, S_VEL], row)
            ns = np.array(step(cfg, P, fed, act))
            ns[:, S_WRENCH] = S[:, S_WRENCH]              # the state keeps the per-episode base
            S = ns
            trace.append(S.copy())
        traces.append(np.stack(trace))
    return traces[0], traces[1], traces[2], cfg


def check_closed_form(windy, calm, still, dt, what):
    vx = windy[:, :, 7].astype(np.float64)
    gap = np.abs(vx - closed_form(dt, len(vx))[:, None]).max()
    print(f"\n[{what}] v_x after {len(vx)} steps {vx[-1, 0]:.9f} (closed form {closed_form(dt, len(vx))[-1]:.9f}); "
          f"largest gap to the float64 recurrence {gap:.3e} m/s (tolerance {TOLERANCE:.3e})")
    assert gap <= TOLERANCE, gap
    # the vehicle stays as level as in calm air: attitude, body rates and rotor speeds are those of the plain step, bit for bit
    for cols in (slice(3, 7), slice(10, 13), slice(13, 17)):
        assert np.array_equal(windy[:, :, cols].view(np.uint32), calm[:, :, cols].view(np.uint32)), cols
    # ... and the cross axes are untouched by the wind along x.  The hover itself drifts in float32 (calm air: |v_y| up to 2e-05 m/s),
    # and the drag damps that drift, so the calm air v_y is held to is the air at rest with the same drag: bit for bit
    assert np.array_equal(windy[:, :, 8:10].view(np.uint32), still[:, :, 8:10].view(np.uint32))
    assert (vx[-1] > 1.0).all() and (np.diff(vx, axis=0) > 0).all()          # ... and the wind does carry it along
    return gap


def test_the_oracle_in_a_steady_wind_follows_the_closed_form(oracle):
    """The nominal vehicle level at hover with the hover action in a steady wind (3, 0, 0) m/s, d = 0.5 / s: the drag is a force
    through the centre of mass, so the vehicle stays level, and it is held over the step, so RK4 integrates it exactly:
    v_x(k) = w_x (1 - (1 - d dt)^k)."""
    windy, calm, still, cfg = oracle_trace(oracle)
    check_closed_form(windy, calm, still, cfg.dt, "oracle")
