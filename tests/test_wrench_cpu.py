"""The host side of the wrench schedule without a GPU: the four entry points are declared, bound and exported, what needs no device is
refused with its message before the device is looked at, the disturbance generators against closed forms in float64, ``compose`` on
hand-made values in both units (with a case an fma would round differently), and the Python surface's refusals before any library
call."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("rq_wrench_bank_create", "rq_wrench_bank_destroy", "rq_env_set_wrench_schedule", "rq_env_get_wrench_schedule")


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
    assert re.search(r"still 5: rq_wrench_bank_\{create,destroy\}", hdr)
    assert re.search(r"RQ_WRENCH_RELATIVE = 0, RQ_WRENCH_ABSOLUTE = 1", hdr)


def test_what_needs_no_device_is_refused_first():
    import ctypes as C
    from raptor_amd import _lib
    lib = _lib.load()
    h = C.c_void_p(4096)                     # never followed: everything below is refused before the device is looked at
    rows = (C.c_float * 12)()
    out = C.c_void_p()
    for args in ((None, rows, 1, 1, 0, C.byref(out)), (h, None, 1, 1, 0, C.byref(out)), (h, rows, 1, 1, 0, None)):
        assert lib.rq_wrench_bank_create(*args) == -1
        assert b"null argument" in lib.rq_last_error()
    assert lib.rq_wrench_bank_create(h, rows, 0, 1, 0, C.byref(out)) == -1 and b"at least one table" in lib.rq_last_error()
    assert lib.rq_wrench_bank_create(h, rows, 1, 0, 0, C.byref(out)) == -1 and b"at least one row" in lib.rq_last_error()
    assert lib.rq_wrench_bank_create(h, rows, 1 << 14, 1 << 14, 0, C.byref(out)) == -1 and b"2^28" in lib.rq_last_error()
    for units in (2, -1, 7):
        assert lib.rq_wrench_bank_create(h, rows, 1, 2, units, C.byref(out)) == -1 and b"unknown units" in lib.rq_last_error()
    rows[10] = float("nan")
    assert lib.rq_wrench_bank_create(h, rows, 1, 2, 1, C.byref(out)) == -1
    assert b"non-finite entry: table 0, row 1" in lib.rq_last_error()
    rows[10] = float("-inf")
    assert lib.rq_wrench_bank_create(h, rows, 2, 1, 0, C.byref(out)) == -1
    assert b"non-finite entry: table 1, row 0" in lib.rq_last_error()
    assert not out.value
    assert lib.rq_wrench_bank_destroy(None) == 0
    ids = (C.c_uint32 * 1)(0)
    assert lib.rq_env_set_wrench_schedule(None, h, ids) == -1 and b"null argument" in lib.rq_last_error()
    assert lib.rq_env_set_wrench_schedule(None, None, None) == -1 and b"null argument" in lib.rq_last_error()
    assert lib.rq_env_get_wrench_schedule(None, C.byref(out), ids) == -1 and b"null argument" in lib.rq_last_error()
    assert lib.rq_env_get_wrench_schedule(h, None, ids) == -1 and b"null argument" in lib.rq_last_error()


def test_generators_against_closed_forms():
    from raptor_amd import disturbances as D
    rows, dt = 500, 0.01
    k = np.arange(rows)
    t = k.astype(np.float64) * dt
    f = np.array([0.3, -0.1, 0.05])

    def expect(force_gain=None, torque_gain=None, vec=f):
        e = np.zeros((rows, 6), np.float64)
        if force_gain is not None:
            e[:, 0:3] = np.asarray(force_gain, np.float64)[:, None] * vec
        if torque_gain is not None:
            e[:, 3:6] = np.asarray(torque_gain, np.float64)[:, None] * vec
        return e.astype(np.float32)

    def same(table, want):
        assert table.dtype == np.float32 and table.shape == (rows, 6) and table.flags.c_contiguous
        assert np.array_equal(table, want)

    same(D.calm(rows), np.zeros((rows, 6), np.float32))
    # the issue's gust: starts at 1.5 s, stops at 2.5 s -> steps 150 .. 249
    g = D.gust(rows, dt, f, 1.5, 1.0)
    same(g, expect((t >= 1.5) & (t < 2.5)))
    on = np.flatnonzero(g[:, 0])
    assert on[0] == 150 and on[-1] == 249 and on.size == 100 and not g[:, 3:].any()
    same(D.gust(rows, dt, f, 0.0, 100.0), expect(np.ones(rows)))
    assert not D.gust(rows, dt, f, 1.0, 0.0).any() and not D.gust(rows, dt, f, 7.0, 1.0).any()
    # a one-step poke and a longer one, cut at the table's end
    same(D.poke(rows, f, 200), expect(k == 200))
    same(D.poke(rows, f, 498, steps=5), expect(k >= 498))
    assert not D.poke(rows, f, 3, steps=0).any() and not D.poke(rows, f, rows).any()
    # ramp: f * clip((t - start) / rise, 0, 1)
    r = D.ramp(rows, dt, f, 1.0, 2.0)
    same(r, expect(np.clip((t - 1.0) / 2.0, 0.0, 1.0)))
    assert not r[:101].any() and np.array_equal(r[300:], np.broadcast_to(expect(np.ones(rows))[0], (200, 6)))
    assert np.allclose(r[200, :3].astype(np.float64), 0.5 * f, rtol=1e-6)
    same(D.ramp(rows, dt, f, 1.0, 0.0), expect(t >= 1.0))
    # the payload that hangs on from step 200: -fraction on z
    p = D.payload(rows, 0.25, 200)
    want = np.zeros((rows, 6), np.float32)
    want[200:, 2] = -0.25
    same(p, want)
    same(D.torque_kick(rows, f, 5), expect(torque_gain=k == 5))
    same(D.torque_kick(rows, f, 5, steps=3), expect(torque_gain=(k >= 5) & (k < 8)))
    for bad in (lambda: D.calm(0), lambda: D.calm(2.5), lambda: D.gust(5, 0.0, f, 0, 1), lambda: D.gust(5, dt, f[:2], 0, 1),
                lambda: D.gust(5, dt, f, -1.0, 1), lambda: D.gust(5, dt, (1, 2, np.nan), 0, 1), lambda: D.poke(5, f, -1),
                lambda: D.poke(5, f, 1.5), lambda: D.poke(5, f, 1, steps=-2), lambda: D.ramp(5, dt, f, 0, -1.0),
                lambda: D.payload(5, np.inf, 1), lambda: D.payload(5, 0.1, -1), lambda: D.torque_kick(5, (1, 2), 1)):
        with pytest.raises(ValueError):
            bad()


def test_suite():
    from raptor_amd import disturbances as D
    s = D.suite(500, 0.01)
    assert list(s) == ["calm", "gust", "poke", "ramp", "payload", "torque_kick"]
    for name, table in s.items():
        assert table.dtype == np.float32 and table.shape == (500, 6) and np.isfinite(table).all(), name
        assert not table[0].any(), name                       # every episode starts undisturbed
        assert np.abs(table).max() <= 1.0, name               # relative units: at most the vehicle's own weight
    assert not s["calm"].any() and len({t.tobytes() for t in s.values()}) == 6
    assert np.array_equal(s["gust"], D.gust(500, 0.01, (0.3, 0.0, 0.0), 1.25, 1.25))
    assert np.array_equal(s["payload"], D.payload(500, 0.2, 250))
    assert D.check_tables(list(s.values())).shape == (6, 500, 6)


def test_compose_is_the_definition_in_float32():
    from raptor_amd import disturbances as D
    f32 = np.float32
    base = np.array([0.01, -0.02, 0.03, 1e-4, -2e-4, 3e-4], f32)
    row = np.array([0.3, -0.5, 0.7, 0.11, 0.13, -0.17], f32)
    mass, gravity, xy = f32(0.027), f32(9.81), np.array([0.028, -0.028], f32)
    # absolute: fs = ts = 1, the products are exact
    a = D.compose(base, mass, gravity, xy, row, "absolute")
    assert a.dtype == f32 and a.shape == (6,) and np.array_equal(a, base + row)
    # relative, operation by operation in the header's order
    mg = f32(mass * gravity)
    arm = f32(np.sqrt(f32(f32(xy[0] * xy[0]) + f32(xy[1] * xy[1]))))
    ts = f32(mg * arm)
    want = np.array([f32(base[j] + f32(mg * row[j])) for j in range(3)] + [f32(base[3 + j] + f32(ts * row[3 + j])) for j in range(3)], f32)
    r = D.compose(base, mass, gravity, xy, row)                  # relative is the default
    assert np.array_equal(r.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(r, D.compose(base, mass, gravity, xy, row, "relative")) and not np.array_equal(r, a)
    assert np.allclose(r[:3].astype(np.float64), base[:3] + 0.027 * 9.81 * row[:3].astype(np.float64), rtol=1e-6)
    assert np.allclose(r[3:].astype(np.float64), base[3:] + 0.027 * 9.81 * 0.028 * np.sqrt(2.0) * row[3:].astype(np.float64), rtol=1e-6)
    # a zero row leaves the base alone, bit for bit (-0.0 + 0.0 aside: the base holds no negative zero here)
    assert np.array_equal(D.compose(base, mass, gravity, xy, np.zeros(6, f32)).view(np.uint32), base.view(np.uint32))
    # the case an fma rounds differently: m g = 1 + 2^-12 exactly, row the same, base -1.  The product 1 + 2^-11 + 2^-24 is a float32
    # tie and rounds to the even 1 + 2^-11, so product-then-sum gives 2^-11; a fused multiply-add keeps the tail: 2^-11 + 2^-24
    e = f32(1.0 + 2.0 ** -12)
    got = D.compose(np.full(6, -1.0, f32), e, f32(1.0), np.array([1.0, 0.0], f32), np.full(6, e, f32))     # arm = 1: ts = m g
    fused = f32(float(e) * float(e) - 1.0)                       # exact in float64, rounded once
    assert fused == f32(2.0 ** -11 + 2.0 ** -24)
    assert (got == f32(2.0 ** -11)).all() and (got != fused).all()
    # batched: [n, 6] rows against [n] masses
    n = 5
    B, R = np.tile(base, (n, 1)), np.tile(row, (n, 1))
    M_ = np.linspace(0.02, 0.05, n).astype(f32)
    XY = np.tile(xy, (n, 1))
    out = D.compose(B, M_, gravity, XY, R)
    assert out.shape == (n, 6) and out.dtype == f32
    for i in range(n):
        assert np.array_equal(out[i].view(np.uint32), D.compose(base, M_[i], gravity, xy, row).view(np.uint32))
    with pytest.raises(ValueError, match="units"):
        D.compose(base, mass, gravity, xy, row, "newton")


def test_python_refusals_come_before_any_library_call(monkeypatch):
    import raptor_amd.l2f as l2f
    from raptor_amd import _lib
    from raptor_amd.policy_bank import PolicyBank, block_policy_assignment
    from raptor_amd.teachers import TeacherBank

    def no_call(name, *a):
        raise AssertionError("library call " + name)
    monkeypatch.setattr(_lib, "call", no_call)
    good = np.zeros((3, 9, 6), np.float32)
    bad = good.copy()
    bad[1, 4, 2] = np.nan
    for tables, words in ((good.astype(np.float64), "float32"), (good[0], "shape"), (good[:, :, :5], "shape"), (good[:0], "shape"),
                          (bad, "finite"), ([], "at least one table"), ([good[0], good[1][:8]], "same number of rows"),
                          ([good[0], bad[1]], "finite"), ([good[0].astype(np.float64)], "float32"), ([good[0][:, :5]], "shape")):
        with pytest.raises(ValueError, match=words):
            l2f.WrenchBank(None, tables)
    with pytest.raises(ValueError, match="units"):
        l2f.WrenchBank(None, good, units="newton")
    bank = l2f.WrenchBank.__new__(l2f.WrenchBank)      # no device, no handle
    bank.n_tables, bank.rows, bank._h, bank.units = 3, 9, None, "relative"
    n = 128
    vector = l2f.vector(n)
    env = vector.VectorEnvironment()
    assert env.wrench_schedule is None
    ids = np.arange(n) % 3
    with pytest.raises(ValueError, match="l2f.WrenchBank"):
        env.set_wrench_schedule(good, ids)
    with pytest.raises(ValueError, match="l2f.WrenchBank"):
        env.set_wrench_schedule(None)
    with pytest.raises(ValueError, match="one id per env: 64 ids for 128 envs"):
        env.set_wrench_schedule(bank, ids[:64])
    with pytest.raises(ValueError, match="one id per env"):
        env.set_wrench_schedule(bank, ids.reshape(2, 64))
    with pytest.raises(ValueError, match="integers"):
        env.set_wrench_schedule(bank, ids.astype(np.float32))
    with pytest.raises(ValueError, match="integers"):
        env.set_wrench_schedule(bank, ids > 0)
    far = ids.copy()
    far[77] = 3
    with pytest.raises(ValueError, match="env 77 names table 3 of a bank of 3"):
        env.set_wrench_schedule(bank, far)
    far[5] = -1
    with pytest.raises(ValueError, match="env 5 names table -1"):
        env.set_wrench_schedule(bank, far)
    assert env.wrench_schedule is None
    env.clear_wrench_schedule()                        # nothing attached, no handle: no call
    # the banks' evaluations: wrench_ids name tables of the schedule the env carries
    pb = PolicyBank.__new__(PolicyBank)
    pb.n_policies = 2
    pids = block_policy_assignment(n, 2)
    with pytest.raises(ValueError, match="attach one first"):
        pb.evaluate(vector, None, env, None, None, None, 1, pids, wrench_ids=ids)
    tb = TeacherBank.__new__(TeacherBank)
    tb.n_teachers = 2
    with pytest.raises(ValueError, match="attach one first"):
        tb.closed_loop(vector, None, env, None, None, None, 1, pids, wrench_ids=ids)
    env._wrench = (bank, np.zeros(n, np.uint32))       # as set_wrench_schedule leaves it
    got = env.wrench_schedule
    assert got[0] is bank and np.array_equal(got[1], np.zeros(n, np.uint32))
    with pytest.raises(ValueError, match="env 77 names table 3"):
        far = ids.copy()
        far[77] = 3
        pb.evaluate(vector, None, env, None, None, None, 1, pids, wrench_ids=far)
    with pytest.raises(ValueError, match="one id per env"):
        tb.closed_loop(vector, None, env, None, None, None, 1, pids, wrench_ids=ids[:5])
    rb = l2f.ReferenceBank.__new__(l2f.ReferenceBank)
    rb.n_references, rb.rows, rb._h = 3, 9, None
    with pytest.raises(ValueError, match="give one of them"):
        pb.evaluate(vector, None, env, None, None, None, 1, pids, reference=rb, reference_ids=ids, wrench_ids=ids)
