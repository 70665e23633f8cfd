"""The host side of the vehicle schedule without a GPU: the four entry points are declared, bound and exported, what needs no device
is refused with its message before the device is looked at, ``vehicles.compose`` against the rule written out per field, the table
builders, the Python surface's refusals before any library call, and two closed forms of the oracle's step fed composed parameters."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("rq_vehicle_bank_create", "rq_vehicle_bank_destroy", "rq_env_set_vehicle_schedule", "rq_env_get_vehicle_schedule")
MASS, JXX, JYY, JZZ, C0, C1, C2, TAU_RISE, TAU_FALL = 0, 1, 2, 3, 16, 17, 18, 20, 21        # RQ_P_*


def test_entry_points_are_declared_bound_and_exported():
    import subprocess
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
    assert re.search(r"still 5: rq_vehicle_bank_\{create,destroy\}", hdr)


def test_what_needs_no_device_is_refused_first():
    import ctypes as C
    from raptor_amd import _lib
    lib = _lib.load()
    h = C.c_void_p(4096)                     # never followed: everything below is refused before the device is looked at
    rows = (C.c_float * 8)(*([1.0] * 8))
    out = C.c_void_p()
    for args in ((None, rows, 1, 1, C.byref(out)), (h, None, 1, 1, C.byref(out)), (h, rows, 1, 1, None)):
        assert lib.rq_vehicle_bank_create(*args) == -1
        assert b"null argument" in lib.rq_last_error()
    assert lib.rq_vehicle_bank_create(h, rows, 0, 1, C.byref(out)) == -1 and b"at least one table" in lib.rq_last_error()
    assert lib.rq_vehicle_bank_create(h, rows, 1, 0, C.byref(out)) == -1 and b"at least one row" in lib.rq_last_error()
    assert lib.rq_vehicle_bank_create(h, rows, 1 << 14, 1 << 14, C.byref(out)) == -1 and b"2^28" in lib.rq_last_error()
    # a factor that is not finite or not > 0: the message names table, row and column
    for value, words in ((float("nan"), b"non-finite entry"), (float("inf"), b"non-finite entry"), (0.0, b"not > 0"),
                         (-1.5, b"not > 0"), (-0.0, b"not > 0")):
        rows[6] = value
        assert lib.rq_vehicle_bank_create(h, rows, 1, 2, C.byref(out)) == -1
        msg = lib.rq_last_error()
        assert words in msg and b"table 0, row 1, column 2" in msg, msg
        assert lib.rq_vehicle_bank_create(h, rows, 2, 1, C.byref(out)) == -1
        assert b"table 1, row 0, column 2" in lib.rq_last_error()
    assert not out.value
    assert lib.rq_vehicle_bank_destroy(None) == 0
    ids = (C.c_uint32 * 1)(0)
    assert lib.rq_env_set_vehicle_schedule(None, h, ids) == -1 and b"null argument" in lib.rq_last_error()
    assert lib.rq_env_set_vehicle_schedule(None, None, None) == -1 and b"null argument" in lib.rq_last_error()
    assert lib.rq_env_get_vehicle_schedule(None, C.byref(out), ids) == -1 and b"null argument" in lib.rq_last_error()
    assert lib.rq_env_get_vehicle_schedule(h, None, ids) == -1 and b"null argument" in lib.rq_last_error()


def _params(n, seed=0):
    g = np.random.default_rng(seed)
    return (g.uniform(0.01, 2.0, (n, 26)) * g.choice([1e-5, 1e-2, 1.0, 1e3], (n, 26))).astype(np.float32)


def test_compose_is_the_rule_per_field_in_float32():
    from raptor_amd import vehicles as V
    f32 = np.float32
    n = 257
    P = _params(n)
    R = np.random.default_rng(1).uniform(0.25, 4.0, (n, 4)).astype(f32)
    got = V.compose(P, R)
    assert got.dtype == f32 and got.shape == (n, 26)
    column = {MASS: 0, JXX: 1, JYY: 1, JZZ: 1, C0: 2, C1: 2, C2: 2, TAU_RISE: 3, TAU_FALL: 3}
    for i in range(n):
        for f in range(26):
            want = f32(P[i, f] * R[i, column[f]]) if f in column else P[i, f]         # one float32 product, or the base value
            assert got[i, f].view(np.uint32) == f32(want).view(np.uint32), (i, f)
    # against float64: every scaled field within one rounding of the exact product, every other field exact
    exact = P.astype(np.float64)
    for f, c in column.items():
        exact[:, f] *= R[:, c].astype(np.float64)
    err = np.abs(got.astype(np.float64) - exact)
    assert (err <= np.abs(exact) * 2.0 ** -24).all()
    assert (err[:, [f for f in range(26) if f not in column]] == 0).all()
    # identity: a row of ones is the base, bit for bit
    assert np.array_equal(V.compose(P, np.ones((n, 4), f32)).view(np.uint32), P.view(np.uint32))
    assert np.array_equal(V.compose(P, V.nominal(1)[0]).view(np.uint32), P.view(np.uint32))          # a single row broadcasts
    # one env, and the input is not written
    before = P.copy()
    one = V.compose(P[3], R[3])
    assert one.shape == (26,) and np.array_equal(one, got[3]) and np.array_equal(P, before)
    with pytest.raises(ValueError, match="compose takes"):
        V.compose(P[:, :25], R)
    with pytest.raises(ValueError, match="compose takes"):
        V.compose(P, R[:, :3])


def test_builders_shapes_values_and_refusals():
    from raptor_amd import vehicles as V
    rows = 50
    k = np.arange(rows)

    def same(table, want):
        assert table.dtype == np.float32 and table.shape == (rows, 4) and table.flags.c_contiguous
        assert np.array_equal(table, np.asarray(want, np.float64).astype(np.float32))

    ones = np.ones((rows, 4))
    same(V.nominal(rows), ones)
    want = ones.copy(); want[20:, 0] = 1.5; want[20:, 1] = 1.2
    same(V.payload_pickup(rows, 20, 1.5, 1.2), want)
    want = ones.copy(); want[:20, 0] = 1.5; want[:20, 1] = 1.2
    same(V.payload_drop(rows, 20, 1.5, 1.2), want)
    want = ones.copy(); want[20:, 0] = 2.0
    same(V.payload_pickup(rows, 20, 2.0), want)                      # inertia defaults to 1
    same(V.payload_pickup(rows, rows, 2.0), ones)                    # a change past the table never comes
    want = ones.copy(); want[:, 2] = 1.0 + np.clip((k - 10) / 20.0, 0.0, 1.0) * (0.8 - 1.0)
    sag = V.battery_sag(rows, 10, 30, 0.8)
    same(sag, want)
    assert (sag[:11, 2] == 1.0).all() and (sag[30:, 2] == np.float32(0.8)).all() and (np.diff(sag[:, 2]) <= 0).all()
    want = ones.copy(); want[10:, 2] = 0.8
    same(V.battery_sag(rows, 10, 10, 0.8), want)                     # end == start: a step
    want = ones.copy(); want[5:, 3] = 3.0
    same(V.slow_motors(rows, 5, 3.0), want)
    assert V.VEHICLE_NAMES == ("mass", "inertia", "thrust", "motor_tau")
    for bad in (lambda: V.nominal(0), lambda: V.nominal(2.5), lambda: V.payload_pickup(5, -1, 2.0), lambda: V.payload_pickup(5, 1.5, 2.0),
                lambda: V.payload_pickup(5, 1, 0.0), lambda: V.payload_pickup(5, 1, -2.0), lambda: V.payload_pickup(5, 1, 2.0, 0.0),
                lambda: V.payload_pickup(5, 1, np.nan), lambda: V.payload_drop(5, 1, 0.0), lambda: V.payload_drop(5, 1, 2.0, -1.0),
                lambda: V.battery_sag(5, 1, 3, 0.0), lambda: V.battery_sag(5, 3, 1, 0.9), lambda: V.battery_sag(5, 1, 3, np.inf),
                lambda: V.slow_motors(5, 1, 0.0), lambda: V.slow_motors(5, 1, -1.0), lambda: V.slow_motors(5, -1, 2.0)):
        with pytest.raises(ValueError):
            bad()
    s = V.suite(500)
    assert list(s) == ["nominal", "payload_pickup", "payload_drop", "battery_sag", "slow_motors"]
    for name, table in s.items():
        assert table.dtype == np.float32 and table.shape == (500, 4) and np.isfinite(table).all() and (table > 0).all(), name
    assert (s["nominal"] == 1).all() and len({t.tobytes() for t in s.values()}) == 5
    assert np.array_equal(s["payload_pickup"], V.payload_pickup(500, 100, 1.3, 1.1))
    assert np.array_equal(V.suite(500, step=7)["slow_motors"], V.slow_motors(500, 7, 2.0))
    assert V.check_tables(list(s.values())).shape == (5, 500, 4)


def test_python_refusals_come_before_any_library_call(monkeypatch):
    import raptor_amd.l2f as l2f
    from raptor_amd import _lib
    from raptor_amd.policy_bank import PolicyBank, block_policy_assignment
    from raptor_amd.teachers import TeacherBank

    def no_call(name, *a):
        raise AssertionError("library call " + name)
    monkeypatch.setattr(_lib, "call", no_call)
    good = np.ones((3, 9, 4), np.float32)
    for value in (np.nan, np.inf, 0.0, -1.0):
        bad = good.copy()
        bad[1, 4, 2] = value
        with pytest.raises(ValueError, match=r"table 1, row 4, column 2 \(thrust\)"):
            l2f.VehicleBank(None, bad)
        with pytest.raises(ValueError, match=r"table 1, row 4, column 2"):
            l2f.VehicleBank(None, [good[0], bad[1]])
    for tables, words in ((good.astype(np.float64), "float32"), (good[0], "shape"), (good[:, :, :3], "shape"), (good[:0], "shape"),
                          (np.ones((3, 9, 6), np.float32), "shape"), ([], "at least one table"),
                          ([good[0], good[1][:8]], "same number of rows"), ([good[0].astype(np.float64)], "float32"),
                          ([good[0][:, :3]], "shape")):
        with pytest.raises(ValueError, match=words):
            l2f.VehicleBank(None, tables)
    bank = l2f.VehicleBank.__new__(l2f.VehicleBank)      # no device, no handle
    bank.n_tables, bank.rows, bank._h = 3, 9, None
    n = 128
    vector = l2f.vector(n)
    env = vector.VectorEnvironment()
    assert env.vehicle_schedule is None
    ids = np.arange(n) % 3
    with pytest.raises(ValueError, match="l2f.VehicleBank"):
        env.set_vehicle_schedule(good, ids)
    with pytest.raises(ValueError, match="l2f.VehicleBank"):
        env.set_vehicle_schedule(None)
    wb = l2f.WrenchBank.__new__(l2f.WrenchBank)
    with pytest.raises(ValueError, match="l2f.VehicleBank"):
        env.set_vehicle_schedule(wb, ids)
    with pytest.raises(ValueError, match="one id per env: 64 ids for 128 envs"):
        env.set_vehicle_schedule(bank, ids[:64])
    with pytest.raises(ValueError, match="integers"):
        env.set_vehicle_schedule(bank, ids.astype(np.float32))
    with pytest.raises(ValueError, match="integers"):
        env.set_vehicle_schedule(bank, ids > 0)
    far = ids.copy()
    far[77] = 3
    with pytest.raises(ValueError, match="env 77 names table 3 of a bank of 3"):
        env.set_vehicle_schedule(bank, far)
    far[5] = -1
    with pytest.raises(ValueError, match="env 5 names table -1"):
        env.set_vehicle_schedule(bank, far)
    assert env.vehicle_schedule is None
    env.clear_vehicle_schedule()                       # nothing attached, no handle: no call
    # the banks' evaluations: vehicle_ids name tables of the schedule the env carries
    pb = PolicyBank.__new__(PolicyBank)
    pb.n_policies = 2
    pids = block_policy_assignment(n, 2)
    with pytest.raises(ValueError, match="attach one first"):
        pb.evaluate(vector, None, env, None, None, None, 1, pids, vehicle_ids=ids)
    tb = TeacherBank.__new__(TeacherBank)
    tb.n_teachers = 2
    with pytest.raises(ValueError, match="attach one first"):
        tb.closed_loop(vector, None, env, None, None, None, 1, pids, vehicle_ids=ids)
    env._vehicle = (bank, np.zeros(n, np.uint32))      # as set_vehicle_schedule leaves it
    got = env.vehicle_schedule
    assert got[0] is bank and np.array_equal(got[1], np.zeros(n, np.uint32))
    with pytest.raises(ValueError, match="env 77 names table 3"):
        far = ids.copy()
        far[77] = 3
        pb.evaluate(vector, None, env, None, None, None, 1, pids, vehicle_ids=far)
    with pytest.raises(ValueError, match="one id per env"):
        tb.closed_loop(vector, None, env, None, None, None, 1, pids, vehicle_ids=ids[:5])
    rb = l2f.ReferenceBank.__new__(l2f.ReferenceBank)
    rb.n_references, rb.rows, rb._h = 3, 9, None
    with pytest.raises(ValueError, match="give one of them"):
        pb.evaluate(vector, None, env, None, None, None, 1, pids, reference=rb, reference_ids=ids, vehicle_ids=ids)
    # wrench_ids and vehicle_ids together are refused
    wb.n_tables, wb.rows, wb._h, wb.units = 3, 9, None, "relative"
    env._wrench = (wb, np.zeros(n, np.uint32))
    for fly in (lambda: pb.evaluate(vector, None, env, None, None, None, 1, pids, wrench_ids=ids, vehicle_ids=ids),
                lambda: tb.closed_loop(vector, None, env, None, None, None, 1, pids, wrench_ids=ids, vehicle_ids=ids)):
        with pytest.raises(ValueError, match="vehicle_ids .* wrench_ids .* give one of them"):
            fly()


# ------------------------------------------------------------------ closed forms on the oracle ------
def hover_world(oracle, n=64):
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


def check_closed_form(s, vz, t, what):
    """v_z = vz and z = vz t / 2 within 1e-4 relative; the other axes and the attitude within the wrench suite's hover bounds"""
    s = np.asarray(s, np.float64)
    z = vz * t / 2
    print(f"\n[{what}] v_z {s[0, 9]:.9f} (closed form {vz:.9f}), z {s[0, 2]:.9f} ({z:.9f}), |x|,|y| {np.abs(s[:, 0:2]).max():.2e}, "
          f"|v_xy| {np.abs(s[:, 7:9]).max():.2e}, |w| {np.abs(s[:, 10:13]).max():.2e}, |q_xyz| {np.abs(s[:, 4:7]).max():.2e}")
    assert np.abs(s[:, 9] / vz - 1).max() < 1e-4 and np.abs(s[:, 2] / z - 1).max() < 1e-4
    assert np.abs(s[:, 0:2]).max() < 2e-4 and np.abs(s[:, 7:9]).max() < 5e-4
    assert np.abs(s[:, 10:13]).max() < 1e-4 and np.abs(s[:, 4:7]).max() < 1e-4 and np.abs(s[:, 3] - 1).max() < 1e-6


@pytest.mark.parametrize("column, factor, sign", [(0, 2.0, -1.0), (2, 1.5, +1.0)])
def test_a_mass_or_thrust_factor_gives_the_closed_form(oracle, column, factor, sign):
    """At hover the thrust is m g.  Twice the mass: a_z = m g / 2 m - g = -g / 2; one and a half times the thrust: a_z = 1.5 g - g =
    +g / 2; so v_z = -+ g t / 2 after 50 steps.  RK4 is exact for a constant acceleration and 50 fp32 accumulations bound the error
    near 50 * 2^-24 = 3e-6 relative: 1e-4 leaves about 30 x room (the wrench suite's argument and margin)."""
    from raptor_amd import vehicles
    cfg, P, S, act = hover_world(oracle)
    row = np.ones(4, np.float32)
    row[column] = factor
    Pe = vehicles.compose(P, row)
    steps = 50
    for _ in range(steps):
        S, _, _ = oracle.step(cfg, Pe, S, act)
    t = steps * float(cfg.dt)
    check_closed_form(S, sign * float(cfg.gravity) * t / 2, t, f"column {column} x {factor}")
