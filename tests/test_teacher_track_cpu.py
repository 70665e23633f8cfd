"""The host side of a teacher bank on a moving setpoint, without a GPU: the two entry points are declared, bound and exported, what
``TeacherBank.fly`` refuses before any library call, ``vector.rollout`` still refusing the pair, and the per-teacher (and
per-teacher-per-path) ``tracking_rmse`` on hand-made sums and counts."""
import os
import re

import numpy as np
import pytest

import raptor_amd.l2f as l2f
from conftest import ROOT
from raptor_amd.teachers import TeacherBank

NEW = ("rq_rollout_teachers_track", "rq_rollout_teachers_track_refs")


class _NoDevice:
    """Stands where a Device (or any handle owner) would: touching it is the failure."""

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched ({name}) before the arguments were checked")


def test_entry_points_are_declared_bound_and_exported():
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
    assert "Teacher banks do not track" not in hdr


def _surfaces():
    bank = l2f.ReferenceBank.__new__(l2f.ReferenceBank)
    bank.n_references, bank.rows, bank._h = 3, 9, None
    ref = l2f.Reference.__new__(l2f.Reference)
    ref._h = None
    tb = TeacherBank.__new__(TeacherBank)
    tb.n_teachers = 4
    return bank, ref, tb


def test_fly_refuses_before_any_call():
    bank, ref, tb = _surfaces()
    n = 40
    vector = l2f.vector(n)
    nothing = _NoDevice()
    tids = (np.arange(n) % 4).astype(np.uint32)
    ids = np.arange(n) % 3

    def fly(teacher_ids=tids, **kw):
        tb.fly(vector, nothing, nothing, nothing, nothing, nothing, 1, teacher_ids, **kw)
    with pytest.raises(ValueError, match="reference_ids belong to a ReferenceBank"):
        fly(reference_ids=ids)
    with pytest.raises(ValueError, match="reference_ids belong to a ReferenceBank"):
        fly(reference=ref, reference_ids=ids)
    with pytest.raises(ValueError, match="one reference id per env is required"):
        fly(reference=bank)
    with pytest.raises(ValueError, match="one id per env: 20 ids for 40 envs"):
        fly(reference=bank, reference_ids=ids[:20])
    with pytest.raises(ValueError, match="integers"):
        fly(reference=bank, reference_ids=ids.astype(np.float32))
    with pytest.raises(ValueError, match="integers"):
        fly(reference=bank, reference_ids=ids > 0)
    far = ids.copy()
    far[17] = 3
    with pytest.raises(ValueError, match="env 17 names reference 3 of a bank of 3"):
        fly(reference=bank, reference_ids=far)
    with pytest.raises(ValueError, match="l2f.Reference"):
        fly(reference=np.zeros((9, 6), np.float32))
    for bad in (tids[:39], tids.reshape(2, 20), np.uint32(1)):
        with pytest.raises(ValueError, match="teacher_ids must hold one id per env"):
            fly(bad, reference=ref)
        with pytest.raises(ValueError, match="teacher_ids must hold one id per env"):
            fly(bad, reference=bank, reference_ids=ids)
        with pytest.raises(ValueError, match="teacher_ids must hold one id per env"):
            fly(bad)
    # closed_loop validates first: the statistics of `nothing` are never reset
    with pytest.raises(ValueError, match="one reference id per env is required"):
        tb.closed_loop(vector, nothing, nothing, nothing, nothing, nothing, 1, tids, reference=bank)
    with pytest.raises(ValueError, match="teacher_ids must hold one id per env"):
        tb.closed_loop(vector, nothing, nothing, nothing, nothing, nothing, 1, tids[:3], reference=ref)
    assert not hasattr(TeacherBank, "fly_and_tabulate")


def test_vector_rollout_still_refuses_reference_with_teacher_ids():
    bank, ref, tb = _surfaces()
    v = l2f.vector(8)
    nothing = _NoDevice()
    ids = np.zeros(8, np.uint32)
    with pytest.raises(ValueError, match="reference and teacher_ids"):
        v.rollout(nothing, nothing, nothing, nothing, tb, nothing, 1, reference=ref, teacher_ids=ids)
    with pytest.raises(ValueError, match="teacher_ids"):
        v.rollout(nothing, nothing, nothing, nothing, tb, nothing, 1, reference=bank, reference_ids=ids, teacher_ids=ids)
    with pytest.raises(ValueError, match="TeacherBank.fly"):
        v.rollout(nothing, nothing, nothing, nothing, tb, nothing, 1, reference=ref)


class _Env:
    """the finished-episode records and tracking sums of six hand-made envs"""

    def __init__(self, sq, cnt):
        self.sq, self.cnt, self.resets = np.asarray(sq, np.float32), np.asarray(cnt, np.uint32), 0

    def reset_statistics(self):
        self.resets += 1

    def tracking_error(self):
        return self.sq, self.cnt

    def finished_counts(self):
        return np.array([1, 0, 2, 1, 0, 1], np.uint32)

    def finished_returns(self):
        return np.array([10.0, 0.0, 30.0, 5.0, 0.0, 7.0], np.float32)

    def finished_lengths(self):
        return np.array([4, 0, 6, 2, 0, 8], np.uint32)

    def finished_terminated(self):
        return np.array([1, 0, 0, 1, 0, 0], np.uint32)


def test_closed_loop_groups_by_teacher_and_by_path(monkeypatch):
    """tracking_rmse [K] and [K, M] from hand-made sums and counts; NaN where a teacher, or a cell, has no counted step"""
    from raptor_amd.teachers import teacher_episode_table
    bank, ref, tb = _surfaces()
    tids = np.array([0, 0, 1, 1, 3, 3], np.uint32)            # teacher 2 flies nothing
    rids = np.array([0, 1, 0, 0, 2, 2], np.uint32)
    sq = [4.0, 12.0, 9.0, 27.0, 0.0, 8.0]
    cnt = [4, 4, 1, 3, 0, 2]                                  # env 4 took no counted step
    env = _Env(sq, cnt)
    calls = []
    monkeypatch.setattr(TeacherBank, "fly", lambda self, *a, **kw: calls.append((env.resets, kw)))
    vector = l2f.vector(6)
    t1 = tb.closed_loop(vector, None, env, None, None, None, 5, tids, reference=ref)
    assert calls[-1][0] == 1 and calls[-1][1]["reference"] is ref and calls[-1][1]["autoreset"] is True
    want = np.sqrt(np.array([16.0 / 8, 36.0 / 4, np.nan, 8.0 / 2]))
    assert t1["tracking_rmse"].shape == (4,) and t1["tracking_rmse"].dtype == np.float64
    assert np.array_equal(t1["tracking_rmse"], want, equal_nan=True) and np.isnan(t1["tracking_rmse"][2])
    plain = teacher_episode_table(env, tids, 4)
    for k in plain:
        assert np.array_equal(t1[k], plain[k], equal_nan=True), k
    t2 = tb.closed_loop(vector, None, env, None, None, None, 5, tids, mode="chained", reference=bank, reference_ids=rids)
    assert calls[-1][0] == 2 and calls[-1][1]["mode"] == "chained"
    cells = np.full((4, 3), np.nan)
    cells[0, 0], cells[0, 1], cells[1, 0], cells[3, 2] = np.sqrt(4.0 / 4), np.sqrt(12.0 / 4), np.sqrt(36.0 / 4), np.sqrt(8.0 / 2)
    assert t2["tracking_rmse"].shape == (4, 3)
    assert np.array_equal(t2["tracking_rmse"], cells, equal_nan=True)
    t0 = tb.closed_loop(vector, None, env, None, None, None, 5, tids)
    assert "tracking_rmse" not in t0 and set(t0) == set(plain)
