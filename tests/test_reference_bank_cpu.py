"""The host side of the reference bank without a GPU: the new entry points are declared, bound and refuse null arguments, the
per-reference tracking table on hand-made arrays, the setpoint generators against closed forms in float64, the id dealing, and the
Python surface's refusals before any library call."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("rq_reference_bank_create", "rq_reference_bank_destroy", "rq_rollout_track_refs", "rq_rollout_policies_track_refs")


def test_entry_points_are_declared_and_bound():
    from raptor_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "raptor_quad.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        m = re.search(r"RQ_API int %s\(([^;]*)\);" % name, hdr, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib._SIGNATURES[name]), name
    assert lib.rq_abi_version() == 5 and _lib.ABI_VERSION == 5
    assert int(re.search(r"#define RQ_ABI_VERSION (\d+)", hdr).group(1)) == 5


def test_null_arguments_are_refused():
    import ctypes as C
    from raptor_amd import _lib
    lib = _lib.load()
    h = C.c_void_p(4096)                     # never followed: a null argument is refused first
    rows = (C.c_float * 6)()
    out = C.c_void_p()
    for args in ((None, rows, 1, 1, C.byref(out)), (h, None, 1, 1, C.byref(out)), (h, rows, 1, 1, None)):
        assert lib.rq_reference_bank_create(*args) == -1
        assert b"null argument" in lib.rq_last_error()
    assert lib.rq_reference_bank_destroy(None) == 0
    # what needs no device is refused before the device is looked at: an empty bank, a non-finite entry, 2^28 rows
    assert lib.rq_reference_bank_create(h, rows, 0, 1, C.byref(out)) == -1 and b"at least one table" in lib.rq_last_error()
    assert lib.rq_reference_bank_create(h, rows, 1, 0, C.byref(out)) == -1 and b"at least one row" in lib.rq_last_error()
    assert lib.rq_reference_bank_create(h, rows, 1 << 14, 1 << 14, C.byref(out)) == -1 and b"2^28" in lib.rq_last_error()
    rows[4] = float("inf")
    assert lib.rq_reference_bank_create(h, rows, 1, 1, C.byref(out)) == -1 and b"non-finite" in lib.rq_last_error()
    assert not out.value
    ids = (C.c_uint32 * 1)(0)
    assert lib.rq_rollout_track_refs(None, None, None, None, None, None, 1, 0, 0, None, None, ids) == -1
    assert b"null reference bank" in lib.rq_last_error()
    assert lib.rq_rollout_track_refs(None, None, None, None, None, None, 1, 0, 0, None, h, None) == -1
    assert b"null reference_id" in lib.rq_last_error()
    assert lib.rq_rollout_track_refs(None, None, None, None, None, None, 1, 0, 0, None, h, ids) != 0
    assert lib.rq_rollout_policies_track_refs(None, None, None, None, None, None, None, 1, 0, 0, None, None, ids) == -1
    assert b"null reference bank" in lib.rq_last_error()
    assert lib.rq_rollout_policies_track_refs(None, None, None, None, None, None, None, 1, 0, 0, None, h, None) == -1
    assert b"null reference_id" in lib.rq_last_error()
    assert lib.rq_rollout_policies_track_refs(None, None, None, None, None, None, None, 1, 0, 0, None, h, ids) != 0


def test_reference_tracking_table():
    from raptor_amd.tracking import reference_tracking_table
    ref = np.array([0, 0, 0, 2, 2, 1], np.uint32)
    sum_sq = np.array([4.0, 12.0, 0.0, 1.0, 2.0, 0.0], np.float32)
    steps = np.array([2, 6, 0, 1, 2, 0], np.uint32)       # env 2 took no counted step; reference 1 none at all; reference 3 flies no env
    t = reference_tracking_table(sum_sq, steps, ref, 4)
    assert t.shape == (4,) and t.dtype == np.float64
    assert np.allclose(t[[0, 2]], [np.sqrt(16.0 / 8.0), 1.0], rtol=1e-15)
    assert np.isnan(t[[1, 3]]).all()
    # the mean is over steps, not over envs: one long flight outweighs a short one
    assert np.isclose(reference_tracking_table([1.0, 99.0], [1, 99], [0, 0], 1)[0], 1.0)
    # [P, M]: cell (p, r) over the envs policy p flew on reference r
    pol = np.array([0, 1, 1, 0, 1, 1], np.uint32)
    t2 = reference_tracking_table(sum_sq, steps, ref, 4, pol, 3)
    assert t2.shape == (3, 4) and t2.dtype == np.float64
    want = np.full((3, 4), np.nan)
    want[0, 0], want[1, 0], want[0, 2], want[1, 2] = np.sqrt(4.0 / 2.0), np.sqrt(12.0 / 6.0), 1.0, 1.0
    assert np.allclose(t2, want, rtol=1e-15, equal_nan=True)
    assert np.isnan(t2[1, 1]) and np.isnan(t2[2]).all()       # no counted step; a policy that flies no env
    for bad in (dict(steps=steps[:-1]), dict(reference_ids=ref[:-1]), dict(policy_ids=pol[:-1], n_policies=3), dict(policy_ids=pol),
                dict(n_policies=3)):
        kw = dict(sum_sq=sum_sq, steps=steps, reference_ids=ref, n_references=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            reference_tracking_table(**kw)


def test_generators_against_closed_forms():
    from raptor_amd import tracking
    rows, dt = 500, 0.01
    t = np.arange(rows, dtype=np.float64) * dt
    # circle: centre (radius, 0, 0), starts at the origin; the analytic velocity is the derivative of the position
    radius, period = 0.15, 5.0
    c64 = tracking.circle64(rows, dt, radius, period)
    w = 2.0 * np.pi / period
    assert c64.dtype == np.float64 and c64.shape == (rows, 6)
    assert np.array_equal(c64[0, :3], np.zeros(3))
    assert np.allclose(np.hypot(c64[:, 0] - radius, c64[:, 1]), radius, rtol=0, atol=1e-15) and not c64[:, 2].any()
    assert np.allclose(c64[:, 0], radius * (1 - np.cos(w * t)), rtol=0, atol=1e-15)
    assert np.allclose(c64[:, 1], radius * np.sin(w * t), rtol=0, atol=1e-15)
    assert np.allclose(np.hypot(c64[:, 3], c64[:, 4]), radius * w, rtol=1e-14) and not c64[:, 5].any()
    # central differences of the position: error <= h^2 / 6 max |p'''| = dt^2 / 6 radius w^3
    central = (c64[2:, :3] - c64[:-2, :3]) / (2 * dt)
    assert np.abs(central - c64[1:-1, 3:]).max() <= dt * dt / 6 * radius * w ** 3 * 1.01
    c = tracking.circle(rows, dt, radius, period)
    assert c.dtype == np.float32 and np.array_equal(c, c64.astype(np.float32)) and not c[0, :3].any()      # rounded once
    # the same derivative check for the figure-eights of the suite
    for per in (5.0, 10.0):
        e = tracking.lissajous64(rows, dt, (0.3, 0.15, 0.0), per)
        central = (e[2:, :3] - e[:-2, :3]) / (2 * dt)
        assert np.abs(central - e[1:-1, 3:]).max() <= dt * dt / 6 * 0.3 * (4 * np.pi / per) ** 3 * 1.01
    # step: the origin, then the offset, at rest
    s = tracking.step_setpoint(rows, dt, (0.2, -0.1, 0.05), 125)
    assert s.dtype == np.float32 and s.shape == (rows, 6)
    assert not s[:125].any() and not s[:, 3:].any()
    assert np.array_equal(s[125:, :3], np.broadcast_to(np.array([0.2, -0.1, 0.05], np.float32), (rows - 125, 3)))
    assert not tracking.step_setpoint(4, dt, (1, 1, 1), 4).any() and tracking.step_setpoint(4, dt, (1, 1, 1), 0)[:, :3].all()
    for bad in (lambda: tracking.circle(0, dt, 1, 1), lambda: tracking.circle(5, 0, 1, 1), lambda: tracking.circle(5, dt, 1, -1),
                lambda: tracking.step_setpoint(5, dt, (1, 2), 1), lambda: tracking.step_setpoint(5, dt, (1, 2, 3), -1),
                lambda: tracking.step_setpoint(5, dt, (1, 2, np.nan), 1), lambda: tracking.step_setpoint(5, dt, (1, 2, 3), 1.5)):
        with pytest.raises(ValueError):
            bad()


def test_suite_stays_inside_the_default_termination_position():
    from raptor_amd import _lib, tracking
    import ctypes
    cfg = _lib.EnvConfig()
    _lib.call("rq_env_default_config", ctypes.byref(cfg))
    s = tracking.suite(500, 0.01)
    assert set(s) == {"hold", "eight_slow", "eight_fast", "circle", "step"}
    for name, table in s.items():
        assert table.dtype == np.float32 and table.shape == (500, 6) and np.isfinite(table).all(), name
        # inside on every axis and in norm, with room for the tracking error
        assert np.linalg.norm(table[:, :3].astype(np.float64), axis=1).max() < 0.5 * cfg.termination_position, name
        assert not table[0, :3].any(), name                  # every episode starts on the path
    assert not s["hold"].any()
    assert np.array_equal(s["eight_fast"], tracking.lissajous(500, 0.01, (0.3, 0.15, 0.0), 5.0))
    assert np.array_equal(s["eight_slow"], tracking.lissajous(500, 0.01, (0.3, 0.15, 0.0), 10.0))
    assert len({t.tobytes() for t in s.values()}) == 5


def test_spread_reference_ids_is_even_and_even_per_policy():
    from raptor_amd.policy_bank import block_policy_assignment
    from raptor_amd.tracking import spread_reference_ids
    ids = spread_reference_ids(1000, 7)
    assert ids.dtype == np.uint32 and ids.shape == (1000,) and ids.flags.c_contiguous
    counts = np.bincount(ids, minlength=7)
    assert counts.max() - counts.min() <= 1 and counts.sum() == 1000
    # per policy: 5 policies on blocks of 64 (the last block ragged), 3 references
    pol = block_policy_assignment(64 * 11 + 17, 5)
    ids = spread_reference_ids(pol.size, 3, pol)
    for p in range(5):
        counts = np.bincount(ids[pol == p], minlength=3)
        assert counts.max() - counts.min() <= 1 and counts.sum() == (pol == p).sum(), p
    # an unsorted assignment is dealt evenly too
    pol = np.array([2, 0, 2, 2, 0, 1, 2, 0, 2, 2])
    ids = spread_reference_ids(10, 2, pol)
    assert list(ids[pol == 2]) == [0, 1, 0, 1, 0, 1] and list(ids[pol == 0]) == [0, 1, 0] and list(ids[pol == 1]) == [0]
    for bad in (lambda: spread_reference_ids(0, 3), lambda: spread_reference_ids(3, 0), lambda: spread_reference_ids(3, 2, [0, 1])):
        with pytest.raises(ValueError):
            bad()


def test_python_refusals_come_before_any_library_call(monkeypatch):
    import raptor_amd.l2f as l2f
    from raptor_amd import _lib
    from raptor_amd.policy_bank import PolicyBank, block_policy_assignment

    def no_call(name, *a):
        raise AssertionError("library call " + name)
    monkeypatch.setattr(_lib, "call", no_call)
    good = np.zeros((3, 9, 6), np.float32)
    bad = good.copy()
    bad[1, 4, 2] = np.nan
    for tables, words in ((good.astype(np.float64), "float32"), (good[0], "shape"), (good[:, :, :5], "shape"), (good[:0], "shape"),
                          (bad, "finite"), ([], "at least one table"), ([good[0], good[1][:8]], "same number of rows"),
                          ([good[0], bad[1]], "finite"), ([good[0].astype(np.float64)], "float32")):
        with pytest.raises(ValueError, match=words):
            l2f.ReferenceBank(None, tables)
    bank = l2f.ReferenceBank.__new__(l2f.ReferenceBank)      # no device, no handle
    bank.n_references, bank.rows, bank._h = 3, 9, None
    ref = l2f.Reference.__new__(l2f.Reference)
    ref._h = None
    n = 128
    vector = l2f.vector(n)
    ids = np.arange(n) % 3

    def roll(**kw):
        vector.rollout(None, None, None, None, None, None, 1, **kw)
    with pytest.raises(ValueError, match="reference_ids belong to a ReferenceBank"):
        roll(reference_ids=ids)
    with pytest.raises(ValueError, match="reference_ids belong to a ReferenceBank"):
        roll(reference=ref, reference_ids=ids)
    with pytest.raises(ValueError, match="one reference id per env is required"):
        roll(reference=bank)
    with pytest.raises(ValueError, match="one id per env: 64 ids for 128 envs"):
        roll(reference=bank, reference_ids=ids[:64])
    with pytest.raises(ValueError, match="integers"):
        roll(reference=bank, reference_ids=ids.astype(np.float32))
    with pytest.raises(ValueError, match="integers"):
        roll(reference=bank, reference_ids=ids > 0)
    far = ids.copy()
    far[77] = 3
    with pytest.raises(ValueError, match="env 77 names reference 3 of a bank of 3"):
        roll(reference=bank, reference_ids=far)
    far[5] = -1
    with pytest.raises(ValueError, match="env 5 names reference -1"):
        roll(reference=bank, reference_ids=far)
    with pytest.raises(ValueError, match="teacher_ids"):
        roll(reference=bank, reference_ids=ids, teacher_ids=ids)
    with pytest.raises(ValueError, match="l2f.Reference"):
        roll(reference=good)
    # the policy bank's own tracked call
    pb = PolicyBank.__new__(PolicyBank)
    pb.n_policies = 2
    pids = block_policy_assignment(n, 2)

    def fly(**kw):
        pb.fly(vector, None, None, None, None, None, 1, pids, **kw)
    with pytest.raises(ValueError, match="reference_ids belong to a ReferenceBank"):
        fly(reference=ref, reference_ids=ids)
    with pytest.raises(ValueError, match="reference_ids belong to a ReferenceBank"):
        fly(reference_ids=ids)
    with pytest.raises(ValueError, match="one reference id per env is required"):
        fly(reference=bank)
    with pytest.raises(ValueError, match="env 77 names reference 3"):
        far = ids.copy()
        far[77] = 3
        fly(reference=bank, reference_ids=far)
    with pytest.raises(ValueError, match="one reference id per env is required"):
        pb.evaluate(vector, None, None, None, None, None, 1, pids, reference=bank)
