"""Reference tables for tracked rollouts (raptor_amd/tracking.py) and what the Python surface refuses before it touches a device.
No GPU: nothing here creates a Device."""
import numpy as np
import pytest

import raptor_amd.l2f as l2f
from raptor_amd import _lib, tracking


class _NoDevice:
    """Stands where a Device would: touching it is the failure."""

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched ({name}) before the arguments were checked")


@pytest.mark.parametrize("period,ratio,amplitude", [(5.0, (1, 2, 0), (0.3, 0.15, 0.0)), (2.0, (1, 2, 3), 0.4), (7.3, (2, 1, 1), (0.1, 0.2, 0.3))])
def test_lissajous_velocities_match_central_differences_of_its_positions(period, ratio, amplitude):
    """v is the analytic derivative: against (p[k+1] - p[k-1]) / 2 dt of the table's own float64 positions the difference is the
    central difference's truncation term, at most w^3 A dt^2 / 6 per axis (w = 2 pi ratio / period).  Checked on the float64 table;
    the float32 one is that table rounded once."""
    rows, dt = 400, 0.01
    t64 = tracking.lissajous64(rows, dt, amplitude, period, ratio)
    t = tracking.lissajous(rows, dt, amplitude, period, ratio)
    assert t.shape == (rows, 6) and t.dtype == np.float32 and t64.dtype == np.float64
    assert np.array_equal(t, t64.astype(np.float32))
    a = np.broadcast_to(np.asarray(amplitude, np.float64), (3,))
    w = 2 * np.pi * np.asarray(ratio, np.float64) / period
    central = (t64[2:, :3] - t64[:-2, :3]) / (2 * dt)
    bound = w ** 3 * a * dt ** 2 / 6
    err = np.abs(t64[1:-1, 3:] - central).max(axis=0)
    print("max |v - central difference| per axis", err, "bound", bound)
    assert (err <= bound).all(), (err, bound)
    assert (err[bound > 0] > 0.5 * bound[bound > 0]).all()          # and it is that term, not something smaller by accident
    assert not t[0, :3].any()                                         # every axis starts at the origin


def test_hold_is_zeros():
    t = tracking.hold(9)
    assert t.shape == (9, 6) and t.dtype == np.float32 and not t.any()


@pytest.mark.parametrize("call", [lambda: tracking.hold(0), lambda: tracking.hold(2.5), lambda: tracking.lissajous(0, 0.01, 0.1, 5.0),
                                  lambda: tracking.lissajous(10, 0.0, 0.1, 5.0), lambda: tracking.lissajous(10, 0.01, 0.1, -1.0),
                                  lambda: tracking.lissajous(10, 0.01, (0.1, 0.2), 5.0),
                                  lambda: tracking.lissajous(10, 0.01, 0.1, 5.0, ratio=(1, 2))])
def test_table_builders_validate_their_arguments(call):
    with pytest.raises(ValueError):
        call()


@pytest.mark.parametrize("table", [np.zeros((9, 6), np.float64), np.zeros((9, 5), np.float32), np.zeros((0, 6), np.float32),
                                   np.zeros(54, np.float32), [[0.0] * 6] * 9,
                                   np.full((9, 6), np.nan, np.float32), np.full((9, 6), np.inf, np.float32)])
def test_reference_refuses_a_bad_table_before_touching_a_device(table):
    with pytest.raises(ValueError):
        l2f.Reference(_NoDevice(), table)


def test_rollout_refuses_reference_with_teacher_ids_before_touching_a_device():
    v = l2f.VectorModule(4)
    nothing = _NoDevice()
    with pytest.raises(ValueError, match="reference and teacher_ids"):
        v.rollout(nothing, nothing, nothing, nothing, nothing, nothing, 1, reference=object(), teacher_ids=np.zeros(4, np.uint32))


def test_the_tracking_entry_points_are_declared():
    for name in ("rq_reference_create", "rq_reference_destroy", "rq_rollout_track", "rq_env_get_tracking_error"):
        assert name in _lib.EXPORTED_SYMBOLS
