"""The sensor schedule (rq_sensor_bank_*, rq_env_set_sensor_schedule): a table of observation latency per env, honoured by everything
that assembles an observation for the env.  The anchor runs no new fused code: rq_observe with a schedule attached against
raptor_amd.sensors.delivered over the observations of a twin without one, kept in a host queue per env (tests/test_sensor_cpu.py
Queue), through several episodes.  Everything else is held to that path, or to the kernels without a schedule, on the bits: no
tolerance anywhere.  No test asserts that latency makes flight worse."""
import ctypes as C

import numpy as np
import pytest

import raptor_amd.l2f as l2f
from raptor_amd import _lib, delays, disturbances, probing, sensors, tracking, vehicles, winds
from raptor_amd._lib import RaptorQuadError
from gpu_common import World
from rollout_common import (NOISE, OFFSET, Batch, assert_same, assert_same_recording, bank_weights, bits, ids_of, random_table,
                            roll, snapshot, world_snapshot)
from schedule_common import LAUNCHES, N, Flights, mixed_ids as _mixed_ids, teachers as _teachers
from test_delay_cpu import History, oracle_delay_step
from test_sensor_cpu import READING, Queue

pytestmark = pytest.mark.gpu

P_MASS, P_ROTOR_XY = 0, slice(4, 6)
S_VEL, S_LAST_ACTION, S_WRENCH = slice(7, 10), slice(17, 21), slice(21, 27)

LIMIT = 12                                   # episodes end inside both launches
T = sum(LAUNCHES)
M = 4
KW = dict(seed=5, domain_randomization=1, episode_step_limit=LIMIT, disturbance_force_std=0.05, disturbance_torque_std=0.02, **NOISE)
RATES = [1, 4, 2]                            # the policy bank's native intervals


def _suite(limit):
    """no delay; 16 steps (longer than an episode: the first reading is held throughout); a delay that changes with the row; 3 steps
    throughout (above k in the first three: the first reading held)"""
    varying = np.array([0, 2, 1, 2, 3, 1, 2, 4, 2, 1, 3, 2], np.uint8)
    return np.stack([sensors.none(limit), sensors.constant(limit, 16), np.resize(varying, limit), sensors.constant(limit, 3)])


def _differ(x, y):
    """per (..., env): do the reading columns differ in bits?"""
    a, b = bits(x[..., :READING]), bits(y[..., :READING])
    return (a.reshape(x.shape[:-1] + (-1,)) != b.reshape(y.shape[:-1] + (-1,))).any(axis=-1)


# ------------------------------------------------------------------ 1. the anchor -----
@pytest.mark.parametrize("noise", [False, True])
def test_observe_with_a_schedule_equals_delivered_over_a_twin(device, oracle, noise):
    n, steps = 70, 3 * LIMIT                 # one full wave plus a ragged 6; three episodes
    tables = _suite(LIMIT)
    ids = _mixed_ids(n, M)
    kw = dict(seed=4, domain_randomization=1, episode_step_limit=LIMIT, disturbance_force_std=0.05, disturbance_torque_std=0.02,
              **(NOISE if noise else {}))
    a, b = World(device, oracle, n, **kw), World(device, oracle, n, **kw)
    bank = l2f.SensorBank(device, tables)
    a.env.set_sensor_schedule(bank, ids)
    got = a.env.sensor_schedule
    assert got[0] is bank and np.array_equal(got[1], ids) and b.env.sensor_schedule is None
    g = np.random.default_rng(7)
    P = b.params.numpy()
    queue, oracle_queue = Queue(n), Queue(n)
    oa, ob = np.zeros((n, 26), np.float32), np.zeros((n, 26), np.float32)
    differ = held = 0
    seen, true, ks = [], [], []
    for t in range(steps):
        k = b.env.episode_steps().astype(np.int64)
        assert np.array_equal(a.env.episode_steps(), k), t
        d = tables[ids, np.minimum(k, tables.shape[1] - 1)].astype(np.int64)
        a.vector.observe(device, a.env, a.params, a.state, oa, a.rng)
        b.vector.observe(device, b.env, b.params, b.state, ob, b.rng)
        want = queue.observe(ob, k, d)
        assert np.array_equal(bits(oa), bits(want)), (noise, t)            # all 26 columns
        if not noise:                        # ... and the oracle's observation through the same queue
            want_o = oracle_queue.observe(oracle.observe(b.cfg, 4, 0, 0, P, b.state.numpy()), k, d)
            assert np.array_equal(bits(oa), bits(want_o)), t
        differ += int(_differ(oa, ob).sum())
        held += int((d > k).sum())
        seen.append(oa.copy()); true.append(ob.copy()); ks.append(k)
        act = g.uniform(-1.5, 1.5, (n, 4)).astype(np.float32)
        for w in (a, b):
            w.vector.step(device, w.env, w.params, w.state, act, w.next_state, w.rng)
            w.state.assign(w.next_state)
        assert np.array_equal(bits(a.state.numpy()), bits(b.state.numpy())), t          # the state and the env step are unchanged
    assert (b.env.finished_counts() >= 3).all()
    # sensors.delivered over the twin's observations, episode by episode (the queue above is the same rule, step by step)
    seen, true, ks = np.stack(seen), np.stack(true), np.stack(ks)
    for i in range(n):
        starts = list(np.flatnonzero(ks[:, i] == 0)) + [steps]
        for s, e in zip(starts[:-1], starts[1:]):
            dd = tables[ids[i], np.minimum(np.arange(e - s), tables.shape[1] - 1)]
            assert np.array_equal(bits(seen[s:e, i]), bits(sensors.delivered(true[s:e, i], dd))), (i, s)
    share = differ / (n * steps)
    print(f"\n[anchor noise={noise}] delivered != true in {share:.2f} of the (env, step) pairs; first reading held in {held}")
    assert share >= 0.5 and held >= n * steps // 8          # not vacuous
    # not vacuous the other way: after clear_sensor_schedule A observes what B observes
    a.env.clear_sensor_schedule()
    assert a.env.sensor_schedule is None
    a.vector.observe(device, a.env, a.params, a.state, oa, a.rng)
    b.vector.observe(device, b.env, b.params, b.state, ob, b.rng)
    assert np.array_equal(bits(oa), bits(ob))


# ------------------------------------------------------------------ the rollouts' shared shape -----
@pytest.fixture(scope="module")
def suite(device):
    t = _suite(LIMIT)
    t.setflags(write=False)
    return t, l2f.SensorBank(device, np.array(t))


@pytest.fixture(scope="module")
def zero_bank(device):
    return l2f.SensorBank(device, np.zeros((2, LIMIT), np.uint8))


@pytest.fixture(scope="module")
def setpoints(device):
    t = np.stack([random_table(LIMIT, 51 + r) for r in range(3)])
    return t, l2f.Reference(device, np.array(t[1])), l2f.ReferenceBank(device, t)


_flights = Flights("sensor", KW, RATES)
_fly_policy, _fly_policy_bank, _fly = _flights.fly_policy, _flights.fly_policy_bank, _flights.fly

CALLS = ["rollout", "track_refs", "policy_bank", "policy_bank_refs"]


def _delays_of(rec, tables, ids):
    """from a recording alone: per (step, env) the episode step count (-1 frozen) and the clamped delay d' = min(d, k)"""
    k = probing.episode_steps(rec["done"])
    d = np.asarray(tables)[ids[None, :], np.clip(k, 0, tables.shape[1] - 1)].astype(np.int64)
    return k, np.where(k >= 0, np.minimum(d, k), 0)


def _not_vacuous(rec, tables, ids, what, second_launch=None):
    """from a recording alone: a reading older than the step is delivered in at least half of the live (env, step) pairs;
    second_launch: at that step at least a quarter of the envs is mid-episode and reads a slot the launch before wrote"""
    k, dp = _delays_of(rec, tables, ids)
    live = rec["done"] != 4
    share = (dp >= 1)[live].mean()
    across = None
    if second_launch is not None:
        t = second_launch
        across = (live[t] & (dp[t] >= 1)).mean()
    print(f"\n[{what}] an older reading delivered in {share:.2f} of the live pairs; envs reading across the launch boundary: {across}")
    assert share >= 0.5, what
    assert across is None or across >= 0.25, what


def _first_reading_held(rec, ids, what, per_env=4):
    """from a recording alone, on the envs of the constant-16 table: columns 0..17 of every live step are those of the episode's
    first step while columns 18..21 change"""
    k = probing.episode_steps(rec["done"])
    envs = np.flatnonzero(ids == 1)
    changed = pairs = 0
    for i in envs:
        for t in np.flatnonzero(k[:, i] > 0):
            first = t - k[t, i]              # every episode of the recording began inside it
            assert first >= 0 and k[first, i] == 0
            assert np.array_equal(bits(rec["obs"][t, i, :READING]), bits(rec["obs"][first, i, :READING])), (what, i, t)
            changed += int(not np.array_equal(bits(rec["obs"][t, i, READING:22]), bits(rec["obs"][first, i, READING:22])))
            pairs += 1
    assert pairs >= len(envs) * per_env and changed >= pairs * 3 // 4, (what, changed, pairs)         # (per_env: steps past the first)


# ------------------------------------------------------------------ 2. a bank of zeros is no schedule -----
@pytest.mark.parametrize("autoreset", [True, False])
@pytest.mark.parametrize("mode", ["fused", "chained"])
@pytest.mark.parametrize("call", CALLS)
def test_a_bank_of_zeros_is_no_schedule(device, oracle, weights, zero_bank, setpoints, call, mode, autoreset):
    """crosses the schedule's kernels with the ones that existed before it: snapshot and recording, bit for bit"""
    ids = _mixed_ids(N, 2)
    out = [_fly(device, oracle, weights, setpoints, call, schedule, mode, autoreset)[1:] for schedule in ((zero_bank, ids), None)]
    what = f"{call} {mode} autoreset={autoreset}"
    assert_same(out[0][0], out[1][0], what=what)
    assert_same_recording(out[0][1], out[1][1], what)
    assert out[0][0]["fin_counts"].min() >= 1 and out[0][0]["epoch"][0] == T


# ------------------------------------------------------------------ 3. fused = chained = the host loop -----
@pytest.mark.parametrize("autoreset", [True, False])
@pytest.mark.parametrize("call", CALLS)
def test_fused_equals_chained_equals_the_loop(device, oracle, weights, suite, setpoints, call, autoreset):
    tables, bank = suite
    ids = _mixed_ids(N, M)
    what = f"{call} autoreset={autoreset}"
    wf, sf, rf = _fly(device, oracle, weights, setpoints, call, (bank, ids), "fused", autoreset)
    wc, sc, rc = _fly(device, oracle, weights, setpoints, call, (bank, ids), "chained", autoreset)
    assert_same(sf, sc, what=what)           # state, hidden state, statistics, finished-episode records, done codes, tracking sums, rng epoch
    assert_same_recording(rf, rc, what)
    assert sf["epoch"][0] == T
    # two launches joined equal one: what a launch reads of the launch before is what one launch reads of itself
    w1, s1, r1 = _fly(device, oracle, weights, setpoints, call, (bank, ids), "fused", autoreset, launches=(T,))
    assert_same(sf, s1, what=what + ", one launch")
    assert_same_recording(rf, r1, what + ", one launch")
    # not vacuous.  Without auto-reset every env is frozen by step LIMIT, before the second launch: the read across the boundary is
    # asked of the auto-reset flights
    _not_vacuous(rf, tables, ids, what, second_launch=LAUNCHES[0] if autoreset else None)
    if not call.endswith("refs"):            # untracked: the recording holds the delivered columns as they were stored
        _first_reading_held(rf, ids, what)
    plain = _fly(device, oracle, weights, setpoints, call, None, "fused", autoreset)[1]
    assert not np.array_equal(plain["state"], sf["state"])
    if call.startswith("policy_bank"):
        return                               # (a bank's flight is held to single policies in test_policy_bank_evaluate_by_sensor)
    loop = _engine_loop(device, oracle, suite, setpoints, ids, "bank" if call == "track_refs" else "none")
    first_end = np.argmax(loop["done"] != 0, axis=0)            # every episode ends within LIMIT < T steps
    assert (loop["done"][first_end, np.arange(N)] != 0).all() and first_end.max() < LIMIT
    in_first = np.arange(T)[:, None] <= first_end[None, :]      # [T, N]: the transitions of each env's first episode
    for k in ("obs", "act", "rew", "done"):
        assert np.array_equal(bits(rf[k][in_first]), bits(loop[k][in_first])), f"{what}: the loop's {k}"
    assert _differ(loop["seen"], loop["true"])[in_first].mean() >= 0.5          # the host loop alone
    at_end = (first_end, np.arange(N))
    if not autoreset:                        # the env froze where its first episode ended: the loop's values of that step
        assert sf["frozen"].all()
        for k, lk in (("state", "state"), ("hidden", "hidden"), ("fin_returns", "fin_returns"), ("fin_lengths", "fin_lengths"),
                      ("fin_terminated", "fin_terminated"), ("rewards", "rew")):
            assert np.array_equal(bits(sf[k]), bits(loop[lk][at_end])), f"{what}: the loop's {k} at the episode end"
    else:
        assert (sf["fin_counts"] >= 2).all()


_engine_loops = {}


def _engine_loop(device, oracle, suite, setpoints, ids, ref):
    """The host loop that applies the rule itself, no schedule attached: observe -> the delivered observation out of a host-held
    queue -> (the setpoint's row off the delivered columns, on the host) -> evaluate_step -> step -> assign, for T steps; per step
    what a recording holds and what a rollout leaves behind.  The API has no per-env reset, so the loop is the yardstick of every
    env's FIRST episode: what it does after an env's episode end is not looked at."""
    if ref not in _engine_loops:
        tables, bank = suite
        w = World(device, oracle, N, **KW)
        obs = np.zeros((N, 26), np.float32)
        rids = {"none": None, "bank": _mixed_ids(N, 3, 2)}[ref]
        queue = Queue(N)
        out = dict(obs=[], act=[], seen=[], true=[], rew=[], done=[], state=[], hidden=[], fin_returns=[], fin_lengths=[], fin_terminated=[])
        for t in range(T):
            w.vector.observe(device, w.env, w.params, w.state, obs, w.rng)
            steps = w.env.episode_steps().astype(np.int64)
            k = np.minimum(steps, LIMIT - 1)
            seen = queue.observe(obs, steps, tables[ids, k].astype(np.int64))
            o = seen[:, :22].copy()
            if rids is not None:
                row = setpoints[0][rids, k]
                o[:, 0:3] -= row[:, 0:3]
                o[:, 12:15] -= row[:, 3:6]
            a = w.policy.evaluate_step(o)
            w.vector.step(device, w.env, w.params, w.state, a, w.next_state, w.rng)
            w.state.assign(w.next_state)
            for key, x in (("obs", o), ("act", a), ("seen", seen), ("true", obs), ("rew", w.env.rewards()), ("done", w.env.done_codes()),
                           ("state", w.state.numpy()), ("hidden", w.policy.hidden_state(N)), ("fin_returns", w.env.finished_returns()),
                           ("fin_lengths", w.env.finished_lengths()), ("fin_terminated", w.env.finished_terminated())):
                out[key].append(np.array(x))
        _engine_loops[ref] = {k: np.stack(v) for k, v in out.items()}
    return _engine_loops[ref]


# ------------------------------------------------------------------ 4. other shapes -----
def test_freeze_then_thaw(device, oracle, suite):
    """a rollout without auto-reset freezes every env at its episode end (no reading is taken of a frozen env), one with auto-reset
    thaws them into a new episode, which never sees a reading of the episode before: fused = chained through both"""
    tables, bank = suite
    n = 70
    ids = _mixed_ids(n, M)
    snaps = []
    for mode in ("fused", "chained"):
        w = World(device, oracle, n, **KW)
        w.env.set_sensor_schedule(bank, ids)
        roll(w, LIMIT + 2, mode, False)
        frozen = world_snapshot(w)
        assert frozen["frozen"].all() and (frozen["steps"] == 0).all()
        roll(w, 5, mode, False)              # later steps do not touch a frozen env
        after = world_snapshot(w)
        assert_same(after, frozen, skip=("epoch", "done"), what=f"frozen, {mode}")
        assert (after["done"] == 4).all()
        roll(w, 10, mode, True)              # thawed: a new episode
        snaps.append(world_snapshot(w))
    assert_same(snaps[0], snaps[1], what="freeze then thaw")
    assert not snaps[0]["frozen"].any()
    # the two modes share the ring: a flight that changes mode between launches equals one that does not
    mixed = World(device, oracle, n, **KW)
    mixed.env.set_sensor_schedule(bank, ids)
    roll(mixed, LIMIT + 2, "chained", False)
    roll(mixed, 5, "fused", False)
    roll(mixed, 10, "fused", True)
    assert_same(world_snapshot(mixed), snaps[0], what="chained then fused")
    # ... mid-episode too: 5 steps chained, then fused, against fused throughout
    flown = []
    for first in ("chained", "fused"):
        w = World(device, oracle, n, **KW)
        w.env.set_sensor_schedule(bank, ids)
        roll(w, 5, first, True)
        roll(w, 9, "fused", True)
        roll(w, 7, "chained", True)
        flown.append(world_snapshot(w))
    assert_same(flown[0], flown[1], what="chained, fused, chained mid-episode")


@pytest.mark.parametrize("n", [8, 65])
def test_small_batches(device, oracle, suite, n):
    tables, bank = suite
    ids = _mixed_ids(n, M)
    out = [_fly_policy(device, oracle, (bank, ids), mode, True, True, {}, n=n)[1:] for mode in ("fused", "chained")]
    assert_same(out[0][0], out[1][0], what=f"{n} envs")
    assert_same_recording(out[0][1], out[1][1], f"{n} envs")
    assert out[0][0]["fin_counts"].min() >= 2
    _not_vacuous(out[0][1], tables, ids, f"{n} envs")
    _first_reading_held(out[0][1], ids, f"{n} envs")


def test_lanes_of_one_wave_at_different_episode_ages(device, oracle, suite):
    """a third of the envs is pushed outside termination_position (0.6 m here), terminates at its first step and flies its following
    episodes one step out of phase with its neighbours: the lanes of a wave read and write different slots of the ring"""
    from rollout_common import push
    tables, bank = suite
    ids = _mixed_ids(N, M)
    out = []
    for mode in ("fused", "chained"):
        w = World(device, oracle, N, **dict(KW, termination_position=0.6))
        push(w, 1)
        w.env.set_sensor_schedule(bank, ids)
        tr = w.vector.Trajectory(w.env, T)
        for c in LAUNCHES:
            roll(w, c, mode, True, trajectory=tr)
        out.append((world_snapshot(w), tr.numpy()))
    assert_same(out[0][0], out[1][0], what="out of phase")
    assert_same_recording(out[0][1], out[1][1], "out of phase")
    assert len(np.unique(out[0][0]["steps"][:64])) >= 2 and (out[0][1]["done"][0] == 1).sum() >= N // 4
    _not_vacuous(out[0][1], tables, ids, "out of phase", second_launch=LAUNCHES[0])


def test_native_interval_four(device, oracle, suite):
    tables, bank = suite
    ids = _mixed_ids(N, M)
    out = [_fly_policy(device, oracle, (bank, ids), mode, True, True, {}, interval=4)[1:] for mode in ("fused", "chained")]
    assert_same(out[0][0], out[1][0], what="interval 4")
    assert_same_recording(out[0][1], out[1][1], "interval 4")
    one = _fly_policy(device, oracle, (bank, ids), "fused", True, True, {}, interval=1)[1]
    assert not np.array_equal(one["state"], out[0][0]["state"])


def test_the_two_wave_build(device):
    """beyond 65 536 envs the fused kernel is the 256-register build: fused = chained, bit for bit"""
    from raptor_amd.foundation_policy import Raptor
    n, limit, steps = 65605, 4, 6            # (the second episode is at row 2 when the launch ends)
    tables = np.array([[0, 1, 2, 1], [16] * 4, [1] * 4, [0, 0, 3, 2]], np.uint8)
    bank = l2f.SensorBank(device, tables)
    ids = _mixed_ids(n, M)
    snaps = []
    for mode in ("fused", "chained"):
        b = Batch(device, n, limit=limit, noise=True)
        b.env.set_sensor_schedule(bank, ids)
        pol = Raptor(device)
        b.fly(pol, steps, mode, True)
        snaps.append(snapshot(b, pol.hidden_state(n)))
    assert_same(snaps[0], snaps[1], what="65 605 envs")
    assert snaps[0]["fin_counts"].min() >= 1
    plain = Batch(device, n, limit=limit, noise=True)
    pol = Raptor(device)
    plain.fly(pol, steps, "fused", True)
    assert not np.array_equal(snapshot(plain, pol.hidden_state(n))["state"], snaps[0]["state"])


# ------------------------------------------------------------------ 5. all five schedules -----
def test_all_five_schedules_chained_equal_the_loop_that_composes_them(device, oracle, suite):
    """a vehicle, a relative wrench, a wind, a delay and a sensor schedule on one env, chained: the host loop delivers the observation
    out of its queue, feeds the oracle the vehicle-composed params, a force composed wrench-then-wind with the step's effective mass
    and the delayed command, and puts the actor's own command into the last-action columns; fused is refused with "chained" in the
    message"""
    tables, bank = suite
    n, steps = 70, LIMIT
    gusts = np.stack([disturbances.calm(LIMIT), disturbances.poke(LIMIT, (0.4, -0.3, 0.1), 3, steps=5),
                      disturbances.torque_kick(LIMIT, (0.02, -0.03, 0.01), 5) + disturbances.payload(LIMIT, 0.25, 2)]).astype(np.float32)
    cars = np.stack([vehicles.nominal(LIMIT), vehicles.payload_pickup(LIMIT, 3, 1.6, 1.2), vehicles.battery_sag(LIMIT, 2, 10, 0.8)])
    air = np.stack([winds.steady(LIMIT, (3.0, -1.0, 0.5), 0.35), winds.steady(LIMIT, (-4.0, 2.0, 1.0), 0.6),
                    winds.still_air(LIMIT, 0.8)]).astype(np.float32)
    lags = np.stack([delays.none(LIMIT), delays.constant(LIMIT, 2), np.resize(np.array([0, 1, 2, 1, 3], np.uint8), LIMIT)])
    wbank, vbank, abank = l2f.WrenchBank(device, gusts, "relative"), l2f.VehicleBank(device, cars), l2f.WindBank(device, air)
    dbank = l2f.DelayBank(device, lags)
    sids, wids, vids, aids, dids = _mixed_ids(n, M), _mixed_ids(n, 3, 1), _mixed_ids(n, 3, 2), _mixed_ids(n, 3, 3), _mixed_ids(n, 3, 4)
    cfg = dict(seed=4, domain_randomization=1, episode_step_limit=LIMIT, disturbance_force_std=0.05, disturbance_torque_std=0.02, **NOISE)
    w = World(device, oracle, n, **cfg)
    w.env.set_vehicle_schedule(vbank, vids)
    w.env.set_wrench_schedule(wbank, wids)
    w.env.set_wind_schedule(abank, aids)
    w.env.set_delay_schedule(dbank, dids)
    w.env.set_sensor_schedule(bank, sids)
    tr = w.vector.Trajectory(w.env, steps)
    before = world_snapshot(w)
    for record in (None, tr):
        with pytest.raises(RaptorQuadError, match="chained"):
            roll(w, steps, "fused", True, trajectory=record)
    assert_same(world_snapshot(w), before, what="five schedules, fused refused")
    assert w.rng.epoch == 0 and len(tr) == 0
    roll(w, steps, "chained", False, trajectory=tr)
    rec = tr.numpy()
    # the loop: the oracle alone steps, the engine observes and evaluates the policy
    u = World(device, oracle, n, **cfg)
    P = u.params.numpy()
    obs = np.zeros((n, 26), np.float32)
    live = np.ones(n, bool)
    hist, queue = History(n), Queue(n)
    differ = pairs = 0
    for t in range(steps):
        u.vector.observe(device, u.env, u.params, u.state, obs, u.rng)
        k = np.full(n, t)                    # every env compared is in its first episode: its step count is the step
        seen = queue.observe(obs, k, tables[sids, k].astype(np.int64))
        o = np.ascontiguousarray(seen[:, :22])
        a = u.policy.evaluate_step(o)
        S = u.state.numpy()
        cmd = hist.command(a, k, lags[dids, k].astype(np.int64))
        differ += int(_differ(seen, obs)[live].sum())
        pairs += int(live.sum())
        Pe = vehicles.compose(P, cars[vids, k])
        fed = S.copy()
        fed[:, S_WRENCH] = disturbances.compose(S[:, S_WRENCH], Pe[:, P_MASS], u.cfg.gravity, P[:, P_ROTOR_XY], gusts[wids, k])
        fed[:, S_WRENCH] = winds.compose(fed[:, S_WRENCH], Pe[:, P_MASS], S[:, S_VEL], air[aids, k])
        ns, r, term = oracle_delay_step(oracle, u.cfg, Pe, fed, a, cmd)
        ns[:, S_WRENCH] = S[:, S_WRENCH]                     # the state keeps the per-episode base
        assert np.array_equal(bits(o[live]), bits(rec["obs"][t][live])) and np.array_equal(bits(a[live]), bits(rec["act"][t][live])), t
        assert np.array_equal(bits(r[live]), bits(rec["rew"][t][live])), t
        assert np.array_equal((term != 0)[live], (rec["done"][t] == 1)[live]), t
        u.state.set(ns)                      # the oracle's state goes on
        live &= rec["done"][t] == 0
    print(f"\n[five schedules] delivered != true in {differ} of {pairs} live pairs")
    assert differ >= pairs // 2 and pairs >= n * steps // 2


# ------------------------------------------------------------------ 6. re-attaching, graph replay, a teacher bank -----
@pytest.mark.parametrize("mode", ["fused", "chained"])
def test_reattaching_mid_episode_zeroes_the_ring(device, oracle, mode):
    """readings from before an attachment read as zeros: after five steps under a constant delay of 2 the schedule is attached
    again, and the next observations carry zeros in columns 0..17 at steps 5 and 6 and the reading of step 5 at step 7 - where a twin
    that was left alone goes on with the readings of steps 3 and 4.  `clean` carries no schedule and shows the true readings."""
    n, limit = 70, 12
    kw = dict(seed=8, domain_randomization=1, episode_step_limit=limit, termination_enabled=0)
    bank = l2f.SensorBank(device, [sensors.constant(limit, 2)])
    w, twin, clean = (World(device, oracle, n, **kw) for _ in range(3))
    for x in (w, twin):
        x.env.set_sensor_schedule(bank)
        roll(x, 5, mode, True)
    assert_same(world_snapshot(w), world_snapshot(twin), what="five steps")
    assert (w.env.episode_steps() == 5).all()
    w.env.set_sensor_schedule(bank)           # again: the ring is zeroed
    acts = np.random.default_rng(3).uniform(-1.5, 1.5, (3, n, 4)).astype(np.float32)
    ow, ot = np.zeros((n, 26), np.float32), np.zeros((n, 26), np.float32)
    z = []
    for t in range(3):
        w.vector.observe(device, w.env, w.params, w.state, ow, w.rng)
        twin.vector.observe(device, twin.env, twin.params, twin.state, ot, twin.rng)
        clean.state.set(w.state.numpy())                                               # the true reading of this step (no noise)
        z.append(np.zeros((n, 26), np.float32))
        clean.vector.observe(device, clean.env, clean.params, clean.state, z[t], clean.rng)
        assert np.array_equal(bits(ow[:, READING:]), bits(z[t][:, READING:])), t          # today's values
        assert np.array_equal(bits(ot[:, READING:]), bits(z[t][:, READING:])), t
        if t < 2:
            assert not bits(ow[:, :READING]).any(), t                                     # +0.0f: what the zeroed ring holds
            assert (ot[:, 0:3] != 0).any(axis=1).all() and _differ(ot, z[t]).all(), t     # the twin: the readings of steps 3 and 4
        else:
            assert np.array_equal(bits(ow[:, :READING]), bits(z[0][:, :READING]))         # the reading of step 5
            assert np.array_equal(bits(ot[:, :READING]), bits(z[0][:, :READING]))
            assert _differ(z[2], z[0]).all()
        for x in (w, twin):
            x.vector.step(device, x.env, x.params, x.state, acts[t], x.state, x.rng)
    assert np.array_equal(bits(w.state.numpy()), bits(twin.state.numpy()))
    assert (w.env.episode_steps() == 8).all()


def test_graph_replay_follows_the_schedule(device, oracle):
    """From 25 steps on the chained mode replays a cached hipGraph whose nodes carry the schedule's pointers - the sensor schedule's
    kernel is a node of its own, absent without it: attaching other ids, detaching and attaching again must not fly a graph built for
    another schedule.  The fused twin shares nothing with the graph but the rule: its ring is zeroed and written at the same steps"""
    n, limit = 70, 30
    kw = dict(seed=6, domain_randomization=1, episode_step_limit=limit)
    tables = np.stack([sensors.constant(limit, 1), sensors.jitter(limit, 0, 5, 2), sensors.dropout(limit, 4, 12)])
    bank = l2f.SensorBank(device, tables)
    a, fresh = World(device, oracle, n, **kw), World(device, oracle, n, **kw)       # `fresh`: the same readings, never through a graph
    states = []
    for shift in (0, 1, None, 0):
        for w in (a, fresh):
            if shift is None:
                w.env.clear_sensor_schedule()
            else:
                w.env.set_sensor_schedule(bank, _mixed_ids(n, 3, shift))
        roll(a, 27, "chained")
        roll(fresh, 27, "fused")
        assert_same(world_snapshot(a), world_snapshot(fresh), what=f"shift {shift}")
        states.append(a.state.numpy())
    stale = World(device, oracle, n, **kw)
    stale.env.set_sensor_schedule(bank, _mixed_ids(n, 3, 0))
    for _ in range(2):
        roll(stale, 27, "fused")
    assert not np.array_equal(stale.state.numpy(), states[1])


def test_a_teacher_bank_chained(device, oracle, suite):
    """rq_rollout_teachers in chained mode on a sensor-carrying env equals observe -> rq_teacher_bank_evaluate -> step -> assign with
    the schedule attached (the anchor's path) over a window without episode ends of the envs compared; fused is refused naming
    "chained\""""
    K = 5
    teachers = _teachers(device, K)
    n, steps = 70, LIMIT - 2                 # (short of the step limit: the envs compared are those that live)
    tables, bank = suite
    ids = _mixed_ids(n, M)
    tids = (np.arange(n) % K).astype(np.uint32)
    cfg = dict(seed=3, domain_randomization=1, episode_step_limit=LIMIT, **NOISE)
    w = World(device, oracle, n, **cfg)
    w.env.set_sensor_schedule(bank, ids)
    tr = w.vector.Trajectory(w.env, steps)
    with pytest.raises(RaptorQuadError, match="chained"):
        teachers.fly(w.vector, device, w.env, w.params, w.state, w.rng, steps, tids, "fused", False, trajectory=tr)
    assert w.rng.epoch == 0 and len(tr) == 0
    teachers.fly(w.vector, device, w.env, w.params, w.state, w.rng, steps, tids, "chained", False, trajectory=tr)
    rec = tr.numpy()
    u = World(device, oracle, n, **cfg)
    u.env.set_sensor_schedule(bank, ids)
    obs = np.zeros((n, 26), np.float32)
    live = np.ones(n, bool)
    for t in range(steps):
        u.vector.observe(device, u.env, u.params, u.state, obs, u.rng)
        o = np.ascontiguousarray(obs[:, :22])
        a = teachers.evaluate(o, tids)
        assert np.array_equal(bits(o[live]), bits(rec["obs"][t][live])) and np.array_equal(bits(a[live]), bits(rec["act"][t][live])), t
        u.vector.step(device, u.env, u.params, u.state, a, u.next_state, u.rng)
        u.state.assign(u.next_state)
        assert np.array_equal(bits(u.env.rewards()[live]), bits(rec["rew"][t][live])), t
        assert np.array_equal(u.env.done_codes()[live], rec["done"][t][live]), t
        live &= rec["done"][t] == 0
    assert live.sum() >= n // 2
    _first_reading_held(rec, ids, "teachers", per_env=1)
    calm = World(device, oracle, n, **cfg)
    teachers.fly(calm.vector, device, calm.env, calm.params, calm.state, calm.rng, steps, tids, "chained", False)
    assert not np.array_equal(snapshot(calm)["state"], snapshot(w)["state"])


# ------------------------------------------------------------------ 9. refusals -----
def test_refusals_leave_everything_untouched(device, oracle, weights, suite):
    from raptor_amd.policy_bank import PolicyBank
    tables, bank = suite
    n = 128
    ids = _mixed_ids(n, M)
    pids = ids_of([1, 0], n)
    teachers = _teachers(device, 2)
    W = bank_weights(weights, 2)

    def world():
        w = World(device, oracle, n, **KW)
        return w, PolicyBank(device, W), w.vector.Trajectory(w.env, 30)

    a, pb, tr = world()
    c, pb_c, tr_c = world()                  # the twin that is refused nothing
    for w, p, t in ((a, pb, tr), (c, pb_c, tr_c)):
        w.env.set_sensor_schedule(bank, ids)
        roll(w, 3, "fused", True, trajectory=t)                    # readings in the ring
        p.fly(w.vector, device, w.env, w.params, w.state, w.rng, 2, pids)

    def look():
        return dict(world_snapshot(a), bank_hidden=pb.hidden(n), recorded=np.full(n, len(tr)), recording=tr.numpy()["obs"].transpose(1, 0, 2))

    before, epoch = look(), a.rng.epoch
    assert epoch == 5 and len(tr) == 3
    calls = {
        "rollout": lambda w, p, t, mode: roll(w, 2, mode, True),
        "record": lambda w, p, t, mode: roll(w, 2, mode, True, trajectory=t),
        "policies": lambda w, p, t, mode: p.fly(w.vector, device, w.env, w.params, w.state, w.rng, 2, pids, mode, True),
        "teachers": lambda w, p, t, mode: teachers.fly(w.vector, device, w.env, w.params, w.state, w.rng, 2, pids, mode, True),
    }

    def refused(what, words, call, mode="fused"):
        with pytest.raises(RaptorQuadError) as e:
            calls[call](a, pb, tr, mode)
        assert words in str(e.value), (what, e.value)
        assert_same(look(), before, what=what)
        assert a.rng.epoch == epoch, what

    # fused mode with what the schedule's fused kernel is not taught: refused naming "chained", nothing runs chained instead
    for precision in ("bf16", "f16x2"):
        a.policy.set_precision(precision)
        refused(f"fused {precision}", "chained", "rollout")
        refused(f"fused {precision} recorded", "sensor schedule, which the fused kernel of a bf16 / f16x2 policy", "record")
    a.policy.set_precision("fp32")
    a.policy.set_sample_and_squash("mean")
    refused("fused SampleAndSquash", "SampleAndSquash", "rollout")
    refused("fused SampleAndSquash", "chained", "record")
    a.policy.set_sample_and_squash("off")
    refused("fused teachers", "sensor schedule, which the fused kernel of a teacher bank", "teachers")
    refused("fused teachers", "chained", "teachers")
    others = (("wrench", lambda: l2f.WrenchBank(device, [disturbances.calm(LIMIT)])),
              ("vehicle", lambda: l2f.VehicleBank(device, [vehicles.nominal(LIMIT)])),
              ("wind", lambda: l2f.WindBank(device, [winds.calm(LIMIT)])),
              ("delay", lambda: l2f.DelayBank(device, [delays.none(LIMIT)])))
    for noun, make in others:
        getattr(a.env, f"set_{noun}_schedule")(make())
        for call in ("rollout", "record", "policies"):
            refused(f"fused {call} with a {noun} schedule too",
                    f"sensor schedule, which the fused kernel of an env that carries a {noun} schedule too", call)
            refused(f"fused {call} with a {noun} schedule too", "chained", call)
        getattr(a.env, f"clear_{noun}_schedule")()
    # creation: an entry above 16 (the Python checks stood aside)
    out = C.c_void_p()
    bad = np.array(tables)
    bad[2, 7] = 17
    with pytest.raises(RaptorQuadError) as e:
        _lib.call("rq_sensor_bank_create", device._h, bad.ctypes.data, M, LIMIT, C.byref(out))
    assert "sensor bank holds a delay above 16 steps: table 2, row 7 (17)" in str(e.value) and not out.value
    for nt, nr in ((0, LIMIT), (1, 0)):
        with pytest.raises(RaptorQuadError, match="a sensor bank needs at least one table of at least one row"):
            _lib.call("rq_sensor_bank_create", device._h, bad.ctypes.data, nt, nr, C.byref(out))
    # a bank of another rq_device; an id outside the bank; destroying an attached bank
    other = l2f.SensorBank(l2f.Device(0), np.array(tables))
    with pytest.raises(RaptorQuadError) as e:
        a.env.set_sensor_schedule(other, ids)
    assert e.value.status == -5 and "sensor bank lives on another device" in str(e.value)
    far = ids.copy()
    far[77] = M
    with pytest.raises(RaptorQuadError) as e:
        _lib.call("rq_env_set_sensor_schedule", a.env._h, bank._h, far.ctypes.data)
    assert "sensor id out of range: env 77 names table 4 of a bank of 4" in str(e.value)
    with pytest.raises(RaptorQuadError) as e:
        _lib.call("rq_sensor_bank_destroy", bank._h)
    assert "the sensor bank is attached to" in str(e.value) and "rq_env_set_sensor_schedule" in str(e.value)
    got, back = C.c_void_p(), np.zeros(n, np.uint32)
    _lib.call("rq_env_get_sensor_schedule", a.env._h, C.byref(got), back.ctypes.data)
    assert got.value == bank._h.value and np.array_equal(back, ids)          # still attached, with the ids it was attached with
    assert_same(look(), before, what="after the refusals")
    # ... and so are the readings: both worlds go on, chained, then fused, and stay the same world
    for w, p, t in ((a, pb, tr), (c, pb_c, tr_c)):
        calls["record"](w, p, t, "chained")
        calls["policies"](w, p, t, "fused")
        calls["teachers"](w, p, t, "chained")
    assert_same(dict(world_snapshot(a), bank_hidden=pb.hidden(n)), dict(world_snapshot(c), bank_hidden=pb_c.hidden(n)),
                what="after the refusals, flying on")
    assert_same_recording(tr.numpy(), tr_c.numpy(), "after the refusals, flying on", frozen_too=True)
    # detached (the C call of its own), every refused call works again
    _lib.call("rq_env_clear_sensor_schedule", a.env._h)
    _lib.call("rq_env_get_sensor_schedule", a.env._h, C.byref(got), None)
    assert not got.value
    a.env.clear_sensor_schedule()
    for precision, sas in (("bf16", "off"), ("fp32", "mean"), ("fp32", "off")):
        a.policy.set_precision(precision)
        a.policy.set_sample_and_squash(sas)
        calls["rollout"](a, pb, tr, "fused")
    calls["teachers"](a, pb, tr, "fused")
    # chained flies what fused refuses: a 16-bit policy and the stage beside the schedule
    a.env.set_sensor_schedule(bank, ids)
    for precision, sas in (("bf16", "off"), ("f16x2", "off"), ("fp32", "mean"), ("fp32", "off")):
        a.policy.set_precision(precision)
        a.policy.set_sample_and_squash(sas)
        calls["rollout"](a, pb, tr, "chained")
    a.env.clear_sensor_schedule()
    # a bank is destroyed once nothing carries it
    solo = l2f.SensorBank(device, [sensors.none(LIMIT)])
    d = World(device, oracle, 8, **KW)
    d.env.set_sensor_schedule(solo)
    with pytest.raises(RaptorQuadError):
        _lib.call("rq_sensor_bank_destroy", solo._h)
    d.env.clear_sensor_schedule()
    solo._fin()                              # destroys the bank: no longer attached


# ------------------------------------------------------------------ 10. PolicyBank.evaluate(sensor_ids=) -----
@pytest.mark.parametrize("mode", ["fused", "chained"])
def test_policy_bank_evaluate_by_sensor(device, weights, suite, mode):
    """tracking_rmse is [P, M]; each cell is what a single Raptor flies on that scenario's envs alone (the same global env ids)"""
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.policy_bank import PolicyBank
    tables, bank = suite
    n, Pn, steps = 128, 2, 40
    W = bank_weights(weights, Pn)
    pids = ids_of([1, 0], n)
    sids = np.tile(np.repeat(np.arange(M, dtype=np.uint32), 64 // M), n // 64)          # runs of 16 envs per scenario inside a block
    hold = l2f.Reference(device, tracking.hold(LIMIT))
    whole = Batch(device, n, limit=LIMIT, noise=True, via="fly")
    whole.env.set_sensor_schedule(bank)
    pb = PolicyBank(device, W)
    table = pb.evaluate(whole.vector, device, whole.env, whole.params, whole.state, whole.rng, steps, pids, mode=mode, reference=hold,
                        sensor_ids=sids)
    assert np.array_equal(whole.env.sensor_schedule[1], sids)
    rmse = np.asarray(table["tracking_rmse"])
    assert rmse.shape == (Pn, M) and np.isfinite(rmse).all() and len(np.unique(rmse)) == Pn * M
    sq, cnt = whole.env.tracking_error()
    for lo in range(0, n, 16):
        p, m = int(pids[lo]), int(sids[lo])
        b = Batch(device, 16, offset=OFFSET + lo, limit=LIMIT, noise=True)
        b.env.set_sensor_schedule(bank, np.full(16, m, np.uint32))
        b.fly(Raptor(device, weights=W[p]), steps, mode, True, ref=hold)
        bsq, bcnt = b.env.tracking_error()
        assert np.array_equal(bits(bsq), bits(sq[lo:lo + 16])) and np.array_equal(bcnt, cnt[lo:lo + 16]), (lo, p, m)
        assert np.isclose(np.sqrt(bsq.astype(np.float64).sum() / bcnt.sum()), rmse[p, m], rtol=1e-12, atol=0), (lo, p, m)
    whole.env.set_delay_schedule(l2f.DelayBank(device, [delays.none(LIMIT)]))
    with pytest.raises(ValueError, match="give one of them"):
        pb.evaluate(whole.vector, device, whole.env, whole.params, whole.state, whole.rng, steps, pids, mode="chained", reference=hold,
                    sensor_ids=sids, delay_ids=np.zeros(n, np.uint32))
