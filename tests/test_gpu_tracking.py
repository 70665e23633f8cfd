"""Tracked rollouts (rq_rollout_track): the policy sees position and velocity relative to a moving setpoint, row = the env's own
episode step count.  The yardstick is the API-granular loop with the subtraction done on the host in NumPy (bit for bit); fused,
chained and one-step launches must agree with it and with one another, accumulators included."""
import ctypes as C

import numpy as np
import pytest

import raptor_amd.l2f as l2f
from raptor_amd import _lib, tracking
from raptor_amd._lib import RaptorQuadError
from gpu_common import World, _lib_set_epoch
from rollout_common import assert_same, assert_same_recording, random_table, roll, world_snapshot

pytestmark = pytest.mark.gpu

LIMIT = 9           # episode_step_limit of tests 1 - 6: episodes end and restart inside every rollout


@pytest.fixture(scope="module")
def table():
    t = random_table(LIMIT)
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def ref(device, table):
    return l2f.Reference(device, table)


# a tracked world against an untracked one: the tracking sums are the one thing that lies between them (asserted beside the call)
UNTRACKED_SKIP = ("track_sq", "track_steps")


# ------------------------------------------------------------------ 1 -----
@pytest.mark.parametrize("mode", ["fused", "chained"])
def test_zero_reference_is_a_no_op(device, oracle, mode):
    n = 65
    a, b = (World(device, oracle, n, seed=5, episode_step_limit=LIMIT) for _ in range(2))
    zero = l2f.Reference(device, tracking.hold(LIMIT))
    for chunk in (7, 12):
        roll(a, chunk, mode, reference=zero)
        roll(b, chunk, mode)
    assert_same(world_snapshot(a), world_snapshot(b), skip=UNTRACKED_SKIP)
    assert a.env.finished_counts().min() >= 1
    assert np.array_equal(a.env.tracking_error()[1], np.full(n, 19, np.uint32)) and not b.env.tracking_error()[1].any()


# ------------------------------------------------------------------ 2 -----
@pytest.mark.parametrize("n,noise", [(65, 0.0), (1100, 0.0), (65, 0.01)])
def test_one_tracked_step_equals_the_api_with_the_host_subtracting(device, oracle, table, ref, n, noise):
    """observe -> NumPy subtraction of ref[k] -> evaluate_step -> step on world b from a's state, against a's tracked one-step
    launch: state, hidden state and reward bit for bit for every env whose episode did not end at that step (an ended env was
    re-sampled by the rollout).  With noise the equality also says that the subtraction comes after it.
    Episodes must end at different times for the envs to be at different rows; in 0.09 s hardly any env drifts past 0.6 m by itself,
    so a third of the envs is put outside (x = 0.7 m) before step 2 and another third before step 5: they terminate there and fly
    their next episodes out of phase with the rest."""
    kw = dict(seed=3, episode_step_limit=LIMIT, termination_position=0.6, noise_position=noise)
    a, b = World(device, oracle, n, **kw), World(device, oracle, n, **kw)
    compared = np.zeros(n, np.int64)
    obs = np.zeros((n, 26), np.float32)
    ragged = False
    for t in range(20):
        if t in (2, 5):
            s = a.state.numpy()
            s[(0 if t == 2 else 1)::3, 0] = 0.7
            a.state.set(s)
        b.state.set(a.state.numpy())
        b.policy.set_hidden_state(a.policy.hidden_state(n))
        _lib_set_epoch(b, a.rng.epoch)
        k = a.env.episode_steps()
        ragged |= len(np.unique(k)) > 2
        roll(a, 1, "fused", reference=ref)
        b.vector.observe(device, b.env, b.params, b.state, obs, b.rng)
        obs[:, :3] -= table[k, :3]
        obs[:, 12:15] -= table[k, 3:]
        act = b.policy.evaluate_step(obs[:, :22])
        b.vector.step(device, b.env, b.params, b.state, act, b.next_state, b.rng)
        live = a.env.done_codes() == 0
        assert np.array_equal(a.state.numpy()[live], b.next_state.numpy()[live])
        assert np.array_equal(a.policy.hidden_state(n)[live], b.policy.hidden_state(n)[live])
        assert np.array_equal(a.env.rewards()[live], b.env.rewards()[live])
        compared += live
    print("one-step comparisons per env: min", compared.min(), "max", compared.max())
    assert ragged, "the envs were never at three different rows at once: the per-env row index was not exercised"
    assert compared.min() >= 10, compared.min()


# ------------------------------------------------------------------ 3 -----
@pytest.mark.parametrize("precision", ["fp32", "bf16", "f16x2"])
@pytest.mark.parametrize("n", [1, 65, 4097, 70001])
def test_tracked_fused_equals_chained_equals_one_step_launches(device, oracle, ref, n, precision):
    kw = dict(seed=5, episode_step_limit=LIMIT)
    a, b, c = (World(device, oracle, n, **kw) for _ in range(3))
    for w in (a, b, c):
        w.policy.set_precision(precision)
    for chunk in (7, 12):
        roll(a, chunk, "fused", reference=ref)
        roll(b, chunk, "chained", reference=ref)
        for _ in range(chunk):
            roll(c, 1, "fused", reference=ref)
    sa, sb, sc = world_snapshot(a), world_snapshot(b), world_snapshot(c)
    assert_same(sa, sb)
    assert_same(sa, sc)
    assert sa["fin_counts"].min() >= 1
    assert np.array_equal(sa["track_steps"], np.full(n, 19, np.uint32)) and (sa["track_sq"] > 0).all()


def test_tracked_without_autoreset_frozen_envs_accumulate_nothing(device, oracle, ref):
    n = 65
    kw = dict(seed=5, episode_step_limit=LIMIT, termination_position=0.6)
    a, b, c = (World(device, oracle, n, **kw) for _ in range(3))
    for w in (a, b, c):                   # a third of the envs starts outside termination_position: their episode is one step long
        s = w.state.numpy()
        s[::3, 0] = 0.7
        w.state.set(s)
    for chunk in (7, 12):
        roll(a, chunk, "fused", False, reference=ref)
        roll(b, chunk, "chained", False, reference=ref)
        for _ in range(chunk):
            roll(c, 1, "fused", False, reference=ref)
    sa, sb, sc = world_snapshot(a), world_snapshot(b), world_snapshot(c)
    assert_same(sa, sb)
    assert_same(sa, sc)
    assert sa["frozen"].all()
    # an env stepped until its episode ended and then sat still: its tracked steps are its one episode's length
    assert np.array_equal(sa["track_steps"], sa["fin_lengths"]) and sa["track_steps"].max() == LIMIT
    assert (sa["track_steps"][::3] == 1).all()


def test_tracked_chained_graph_replay_is_keyed_by_the_reference(device, oracle):
    """From 25 steps on, the chained mode replays a cached hipGraph: with a reference it has one more node per step, and a second
    reference on the same objects must not replay the first one's graph."""
    n, limit = 65, 30
    kw = dict(seed=6, episode_step_limit=limit, termination_position=0.6)
    a, b = World(device, oracle, n, **kw), World(device, oracle, n, **kw)
    r1, r2 = l2f.Reference(device, random_table(limit, 2)), l2f.Reference(device, random_table(limit + 3, 3))
    for r in (r1, r2, r1):
        roll(a, 27, "fused", reference=r)
        roll(b, 27, "chained", reference=r)
        assert_same(world_snapshot(a), world_snapshot(b))
    roll(a, 25, "fused")
    roll(b, 25, "chained")
    assert_same(world_snapshot(a), world_snapshot(b))
    assert a.env.finished_counts().min() >= 1


# ------------------------------------------------------------------ 4 -----
def test_tracked_recording(device, oracle, table, ref):
    n, T = 65, 19
    kw = dict(seed=5, episode_step_limit=LIMIT)
    a, b, u = (World(device, oracle, n, **kw) for _ in range(3))
    ta, tb, tu = (w.vector.Trajectory(w.env, T) for w in (a, b, u))
    for chunk in (7, 12):
        roll(a, chunk, "fused", trajectory=ta, reference=ref)
        roll(b, chunk, "chained", trajectory=tb, reference=ref)
        roll(u, chunk, "fused", trajectory=tu)
    ra, rb, ru = ta.numpy(), tb.numpy(), tu.numpy()
    assert_same_recording(ra, rb, frozen_too=True)
    assert_same(world_snapshot(a), world_snapshot(b))
    a.policy.reset()
    assert np.array_equal(ta.relabel(a.policy), ra["act"])
    # what the policy saw is recorded: the first observation is the untracked one minus row 0, bit for bit, and the rest moved
    assert np.array_equal(ra["obs"][0, :, 0:3], ru["obs"][0, :, 0:3] - table[0, :3])
    assert (ra["obs"][..., 0:3] != ru["obs"][..., 0:3]).any(axis=-1).all()


# ------------------------------------------------------------------ 5 -----
def test_tracking_accumulators_against_float64(device, oracle, table, ref):
    """sum |p - ref[k]|^2 recomputed in float64 from the states read between one-step launches.  At most 20 positive fp32 terms, each
    from three rounded differences, two fmas and a product, and 19 rounded additions: relative error <= ~23 x 2^-24 = 1.4e-6 < 1e-5."""
    n = 65
    a = World(device, oracle, n, seed=5, episode_step_limit=LIMIT, termination_position=0.6)
    want = np.zeros(n, np.float64)
    for _ in range(20):
        k = a.env.episode_steps()
        p = a.state.numpy()[:, :3].astype(np.float64)
        want += ((p - table[k, :3].astype(np.float64)) ** 2).sum(axis=1)
        roll(a, 1, "fused", reference=ref)
    sq, steps = a.env.tracking_error()
    rel = np.abs(sq - want) / want
    print("tracking sum: max relative error vs float64", rel.max())
    assert np.array_equal(steps, np.full(n, 20, np.uint32))
    assert rel.max() <= 1e-5, rel.max()
    assert np.allclose(a.env.tracking_rmse(), np.sqrt(want / 20), rtol=1e-5)
    a.env.reset_statistics()
    sq, steps = a.env.tracking_error()
    assert not sq.any() and not steps.any()


# ------------------------------------------------------------------ 6 -----
def test_refusals_leave_the_env_alone(device, oracle, table, ref):
    n = 65
    a = World(device, oracle, n, seed=5, episode_step_limit=LIMIT)
    roll(a, 3, "fused", reference=ref)
    before, epoch = world_snapshot(a), a.rng.epoch

    def refused(match, **kw):
        for mode in ("fused", "chained"):
            with pytest.raises(RaptorQuadError, match=match):
                roll(a, 5, mode, **kw)
        assert_same(before, world_snapshot(a))
        assert a.rng.epoch == epoch

    refused("fewer rows than episode_step_limit", reference=l2f.Reference(device, random_table(LIMIT - 1)))
    other = l2f.Device(0)
    refused("reference lives on another device", reference=l2f.Reference(other, np.array(table)))
    a.policy.set_sample_and_squash("mean")
    refused("SampleAndSquash", reference=ref)
    a.policy.set_sample_and_squash("off")
    # a NaN never reaches the device: the Python surface refuses it, and so does the C entry point
    bad = np.array(table)
    bad[4, 2] = np.nan
    with pytest.raises(ValueError):
        l2f.Reference(device, bad)
    h = C.c_void_p()
    for rows, arr in ((LIMIT, bad), (0, np.array(table))):
        with pytest.raises(RaptorQuadError, match="non-finite|at least one row"):
            _lib.call("rq_reference_create", device._h, _lib.fptr(arr), rows, C.byref(h))
        assert not h.value
    with pytest.raises(RaptorQuadError, match="null reference"):
        _lib.call("rq_rollout_track", device._h, a.env._h, a.params._h, a.state._h, a.policy._handle(device), a.rng._h, 1, 0, 1, None, None)
    assert_same(before, world_snapshot(a))
    roll(a, 3, "fused", reference=ref)                   # and it still flies
    assert np.array_equal(a.env.tracking_error()[1], np.full(n, 6, np.uint32))


# ------------------------------------------------------------------ 7 -----
def test_the_policy_tracks_a_figure_eight(device, oracle):
    """Nominal Crazyflie from hover at the origin, 500 steps along lissajous(amplitude (0.3, 0.15, 0), period 5 s): nobody
    terminates, and the RMS distance to the setpoint over steps 200..499 is below the RMS of |p_ref| over those rows - what a
    quadrotor hovering at the origin would score, computed here from the table.  (The CPU oracle's observe / actor / step with the
    NumPy subtraction meets this with period 5 s: ratio 0.317, so the period was not lengthened.)"""
    n = 64
    a = World(device, oracle, n, seed=0, domain_randomization=0, init_guidance=1.0)
    t = tracking.lissajous(500, 0.01, amplitude=(0.3, 0.15, 0), period=5.0)
    r = l2f.Reference(device, t)
    roll(a, 200, "fused", False, reference=r)
    a_sq0, a_n0 = a.env.tracking_error()
    roll(a, 300, "fused", False, reference=r)
    sq, steps = a.env.tracking_error()
    assert not a.env.finished_terminated().any() and np.array_equal(steps, np.full(n, 500, np.uint32))
    rmse = np.sqrt((sq.astype(np.float64) - a_sq0) / 300)
    hover = np.sqrt((t[200:, :3].astype(np.float64) ** 2).sum(axis=1).mean())
    print("closed loop: RMSE", rmse.max(), "RMS |p_ref|", hover, "ratio", rmse.max() / hover)
    assert rmse.max() < hover, (rmse.max(), hover)
