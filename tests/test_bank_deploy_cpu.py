"""The host side of the policy bank's deployment conditions without a GPU: the new entry points are declared, bound and refuse null
arguments, the per-policy tracking table on hand-made arrays, and the native_interval setter's validation before any library call."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("rq_policy_bank_set_native_interval", "rq_policy_bank_get_native_interval", "rq_rollout_policies_track")


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
    one = (C.c_uint32 * 1)(1)
    h = C.c_void_p(4096)                     # never followed: a null argument is refused first
    assert lib.rq_policy_bank_set_native_interval(None, one, 1) == -1
    assert b"null" in lib.rq_last_error()
    assert lib.rq_policy_bank_set_native_interval(h, None, 1) == -1
    assert lib.rq_policy_bank_get_native_interval(None, one) == -1
    assert lib.rq_policy_bank_get_native_interval(h, None) == -1
    assert lib.rq_rollout_policies_track(None, None, None, None, None, None, None, 1, 0, 0, None, None) == -1
    assert b"null reference" in lib.rq_last_error()
    assert lib.rq_rollout_policies_track(None, None, None, None, None, None, None, 1, 0, 0, None, h) != 0
    assert lib.rq_rollout_policies(None, None, None, None, None, None, None, 1, 0, 0, None) != 0


def test_policy_tracking_table():
    from raptor_amd.policy_bank import policy_tracking_table
    ids = np.array([0, 0, 0, 2, 2, 1], np.uint32)
    sum_sq = np.array([4.0, 12.0, 0.0, 1.0, 2.0, 0.0], np.float32)
    steps = np.array([2, 6, 0, 1, 2, 0], np.uint32)       # env 2 took no counted step; policy 1 none at all; policy 3 flies no env
    t = policy_tracking_table(sum_sq, steps, ids, 4)
    assert t.shape == (4,) and t.dtype == np.float64
    assert np.allclose(t[[0, 2]], [np.sqrt(16.0 / 8.0), 1.0], rtol=1e-15)
    assert np.isnan(t[[1, 3]]).all()
    # the mean is over steps, not over envs: one long flight outweighs a short one
    assert np.isclose(policy_tracking_table([1.0, 99.0], [1, 99], [0, 0], 1)[0], 1.0)
    assert np.isnan(policy_tracking_table([0.0], [0], [0], 1)[0])
    with pytest.raises(ValueError):
        policy_tracking_table(sum_sq, steps[:-1], ids, 4)


def test_native_interval_is_validated_before_any_library_call():
    from raptor_amd.policy_bank import PolicyBank
    bank = PolicyBank.__new__(PolicyBank)                # no device, no handle: a library call would raise AttributeError, not ValueError
    bank.n_policies = 3
    assert list(bank._checked_intervals(4)) == [4, 4, 4]
    out = bank._checked_intervals([4, 1, 64])
    assert out.dtype == np.uint32 and out.flags.c_contiguous and list(out) == [4, 1, 64]
    assert list(bank._checked_intervals(np.array([1, 2, 3], np.int64))) == [1, 2, 3]
    for bad, words in ((0, "1 .. 64: policy 0 is given 0"), (65, "1 .. 64"), ([4, 65, 3], "policy 1 is given 65"), ([1, 0, 1], "policy 1 is given 0"),
                       (-1, "1 .. 64"), ([1, 2], "one interval per policy: 2 for a bank of 3"), ([1, 2, 3, 4], "one interval per policy"),
                       ([], "one interval per policy"), (1.5, "integers"), ([[1, 2, 3]], "scalar or one interval per policy"),
                       (True, "integers")):
        with pytest.raises(ValueError, match=re.escape(words)):
            bank.native_interval = bad
        with pytest.raises(ValueError):
            PolicyBank._checked_intervals(bank, bad)


def test_fly_validates_before_any_library_call():
    """PolicyBank.fly refuses a bad assignment and an unknown mode itself"""
    import raptor_amd.l2f as l2f
    from raptor_amd.policy_bank import PolicyBank, block_policy_assignment
    bank = PolicyBank.__new__(PolicyBank)
    bank.n_policies = 2
    vector = l2f.vector(128)
    ids = block_policy_assignment(128, 2)
    with pytest.raises(ValueError, match="differ inside"):
        bank.fly(vector, None, None, None, None, None, 1, np.arange(128) % 2)
    with pytest.raises(ValueError, match="one id per env"):
        bank.fly(vector, None, None, None, None, None, 1, ids[:64])
    with pytest.raises(KeyError):
        bank.fly(vector, None, None, None, None, None, 1, ids, mode="graph")
