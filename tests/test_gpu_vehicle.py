"""The vehicle schedule (rq_vehicle_bank_*, rq_env_set_vehicle_schedule): a table of factors on mass, inertia, thrust and motor time
constant per env, honoured by everything that steps the env.  The anchor is independent of every new kernel: rq_step with a schedule
attached against the oracle's step fed the parameters composed on the host (raptor_amd.vehicles.compose) - the existing suite shows
the oracle's step and k_step agree bit for bit.  Everything else is held to that path, or to the kernels without a schedule, on the
bits: no tolerance anywhere but in the closed forms."""
import ctypes as C

import numpy as np
import pytest

import raptor_amd.l2f as l2f
from raptor_amd import _lib, disturbances, probing, tracking, vehicles
from raptor_amd._lib import RaptorQuadError
from gpu_common import World
from rollout_common import (NOISE, OFFSET, Batch, assert_same, assert_same_recording, bank_weights, bits, ids_of, random_table,
                            roll, snapshot, world_snapshot)
from schedule_common import LAUNCHES, N, Flights, mixed_ids as _mixed_ids, teachers as _teachers
from test_vehicle_cpu import check_closed_form

pytestmark = pytest.mark.gpu

P_MASS, P_ROTOR_XY = 0, slice(4, 6)         # RQ_P_MASS, RQ_P_ROTOR_POS + 0 / + 1
S_WRENCH = slice(21, 27)                    # RQ_S_FORCE, RQ_S_TORQUE


def test_step_with_a_schedule_equals_the_oracle_fed_the_composed_params(device, oracle):
    n, limit = 70, 12                        # one full wave plus a ragged 6
    # three tables that between them move all four columns: a payload and its inertia from step 2; a thrust ramp; slow motors plus a drop
    tables = np.stack([vehicles.payload_pickup(limit, 2, 1.7, 1.3), vehicles.battery_sag(limit, 1, 9, 0.6),
                       vehicles.slow_motors(limit, 3, 2.5) * vehicles.payload_drop(limit, 6, 0.8, 0.9)]).astype(np.float32)
    assert all((tables[:, :, c] != 1).any() for c in range(4))
    ids = _mixed_ids(n, 3)
    w = World(device, oracle, n, seed=4, domain_randomization=1, episode_step_limit=limit, disturbance_force_std=0.05,
              disturbance_torque_std=0.02)
    bank = l2f.VehicleBank(device, tables)
    w.env.set_vehicle_schedule(bank, ids)
    got = w.env.vehicle_schedule
    assert got[0] is bank and np.array_equal(got[1], ids)
    act = np.random.default_rng(7).uniform(-1, 1, (n, 4)).astype(np.float32)
    P = w.params.numpy()
    assert np.array_equal(P, w.P) and len(np.unique(P[:, P_MASS])) > n // 2          # a domain-randomised population
    composed_differs = 0
    for doubled in (False, True):
        if doubled:                          # rq_params_set after attaching is honoured: the base values come from the call's params
            P = P.copy()
            P[:, P_MASS] *= 2
            w.params.set(P)
        for t in range(limit):
            S = w.state.numpy()
            k = w.env.episode_steps()           # (random actions for 0.12 s: the limit ends the episode at step 12, hardly anything else)
            Pe = vehicles.compose(P, tables[ids, np.minimum(k, limit - 1)])
            composed_differs += int((Pe != P).any())
            ns, r, term = oracle.step(w.cfg, Pe, S, act)
            w.vector.step(device, w.env, w.params, w.state, act, w.next_state, w.rng)
            out = w.next_state.numpy()
            assert np.array_equal(bits(out), bits(ns)), (doubled, t)
            assert np.array_equal(bits(w.env.rewards()), bits(r)) and np.array_equal(w.env.terminated(), term), (doubled, t)
            assert np.array_equal(bits(w.params.numpy()), bits(P)), (doubled, t)       # the params object is never written
            w.state.assign(w.next_state)
        assert (w.env.finished_counts() >= (2 if doubled else 1)).all()
    assert composed_differs >= 2 * (limit - 3)
    # not vacuous the other way: after clear_vehicle_schedule the plain oracle step matches again
    w.env.clear_vehicle_schedule()
    assert w.env.vehicle_schedule is None
    for t in range(4):
        w.vector.step(device, w.env, w.params, w.state, act, w.state, w.rng)
    S = w.state.numpy()
    ns, _, _ = oracle.step(w.cfg, P, S, act)
    w.vector.step(device, w.env, w.params, w.state, act, w.next_state, w.rng)
    assert np.array_equal(bits(w.next_state.numpy()), bits(ns))
    assert not np.array_equal(ns, oracle.step(w.cfg, vehicles.compose(P, tables[ids, 4]), S, act)[0])


# ------------------------------------------------------------------ 2. closed forms -----
@pytest.mark.parametrize("column, factor, sign", [(0, 2.0, -1.0), (2, 1.5, +1.0)])
def test_a_mass_or_thrust_factor_gives_the_closed_form(device, column, factor, sign):
    """tests/test_vehicle_cpu.py's closed forms through rq_step with a schedule attached: the nominal vehicle level at hover, rotors
    at hover speed, hover actions, 50 steps; twice the mass gives v_z = -g t / 2, one and a half times the thrust +g t / 2, within
    1e-4 relative (RK4 is exact for a constant acceleration; 50 fp32 accumulations bound the error near 3e-6)."""
    n, steps = 64, 50
    v = l2f.VectorModule(n, 0)
    rng, env, params, state = v.VectorRng(), v.VectorEnvironment(), v.VectorParameters(), v.VectorState()
    v.initialize_rng(device, rng, 5)
    v.initialize_environment(device, env)
    cfg = env.config
    cfg.domain_randomization = 0
    cfg.termination_enabled = 0
    cfg.disturbance_force_std = 0.0
    cfg.disturbance_torque_std = 0.0
    env.config = cfg
    v.sample_initial_parameters(device, env, params, rng)
    v.sample_initial_state(device, env, params, state, rng)
    P = params.numpy()
    S = np.zeros((n, 27), np.float32)
    S[:, 3] = 1.0                            # q = identity
    S[:, 13:17] = P[:, 24:25]                # hover rotor speed
    state.set(S)
    table = vehicles.nominal(int(cfg.episode_step_limit))
    table[:, column] = factor
    env.set_vehicle_schedule(l2f.VehicleBank(device, [table]))
    act = np.repeat(P[:, 25:26], 4, axis=1).astype(np.float32)          # hover action
    for _ in range(steps):
        v.step(device, env, params, state, act, state, rng)
    t = steps * float(cfg.dt)
    check_closed_form(state.numpy(), sign * float(cfg.gravity) * t / 2, t, f"device, column {column} x {factor}")
    assert np.array_equal(bits(params.numpy()), bits(P))


# ------------------------------------------------------------------ the rollouts' shared shape -----
LIMIT = 16
T = sum(LAUNCHES)
M = 4
# a velocity threshold tight enough that the envs whose mass drops to 15 % shoot up and terminate mid-episode (the CPU oracle flying
# this suite: 39 of table 1's 50 envs terminate, none of the others')
KW = dict(seed=5, domain_randomization=1, episode_step_limit=LIMIT, termination_linear_velocity=2.5, **NOISE)
RATES = [1, 4, 2]                            # the policy bank's native intervals


def _suite(limit):
    return np.stack([vehicles.nominal(limit), vehicles.payload_pickup(limit, 3, 0.15, 0.8), vehicles.battery_sag(limit, 2, 10, 0.6),
                     vehicles.slow_motors(limit, 4, 3.0)]).astype(np.float32)


@pytest.fixture(scope="module")
def suite(device):
    t = _suite(LIMIT)
    t.setflags(write=False)
    return t, l2f.VehicleBank(device, np.array(t))


@pytest.fixture(scope="module")
def ones_bank(device):
    return l2f.VehicleBank(device, [vehicles.nominal(LIMIT), vehicles.nominal(LIMIT)])


@pytest.fixture(scope="module")
def setpoints(device):
    t = np.stack([random_table(LIMIT, 51 + r) for r in range(3)])
    return t, l2f.Reference(device, np.array(t[1])), l2f.ReferenceBank(device, t)


_flights = Flights("vehicle", KW, RATES)
_fly_policy, _fly_policy_bank, _fly = _flights.fly_policy, _flights.fly_policy_bank, _flights.fly

CALLS = ["rollout", "track_refs", "policy_bank", "policy_bank_refs"]


# ------------------------------------------------------------------ 3. the identity bank -----
@pytest.mark.parametrize("autoreset", [True, False])
@pytest.mark.parametrize("mode", ["fused", "chained"])
@pytest.mark.parametrize("call", CALLS)
def test_a_bank_of_ones_is_no_schedule(device, oracle, weights, ones_bank, setpoints, call, mode, autoreset):
    """crosses the schedule's kernels with the ones that existed before it: snapshot and recording, bit for bit (x * 1.0f is x)"""
    ids = _mixed_ids(N, 2)
    out = [_fly(device, oracle, weights, setpoints, call, schedule, mode, autoreset)[1:] for schedule in ((ones_bank, ids), None)]
    what = f"{call} {mode} autoreset={autoreset}"
    assert_same(out[0][0], out[1][0], what=what)
    assert_same_recording(out[0][1], out[1][1], what)
    assert out[0][0]["fin_counts"].min() >= 1 and out[0][0]["epoch"][0] == T


def test_a_teacher_bank_chained(device, oracle, ones_bank, suite):
    """rq_rollout_teachers in chained mode: an all-ones bank is no schedule (across episode ends, recorded); a real suite equals
    observe -> rq_teacher_bank_evaluate -> step -> assign over a window without episode ends; fused is refused naming "chained\""""
    K = 5
    teachers = _teachers(device, K)
    tids = (np.arange(N) % K).astype(np.uint32)
    out = []
    for schedule in ((ones_bank, _mixed_ids(N, 2)), None):
        w = World(device, oracle, N, **KW)
        if schedule:
            w.env.set_vehicle_schedule(*schedule)
        tr = w.vector.Trajectory(w.env, T)
        for c in LAUNCHES:
            teachers.fly(w.vector, device, w.env, w.params, w.state, w.rng, c, tids, "chained", True, trajectory=tr)
        out.append((snapshot(w), tr.numpy()))
    assert_same(out[0][0], out[1][0], what="teachers, ones")
    assert_same_recording(out[0][1], out[1][1], "teachers, ones")
    assert out[0][0]["fin_counts"].min() >= 2
    # the suite, 12 steps from the start of the episode (no env of tables 0, 2, 3 ends; table 1's are compared while they live)
    n, steps = 70, 12
    tables, bank = suite
    ids = _mixed_ids(n, M)
    tids = tids[:n]
    cfg = dict(seed=3, domain_randomization=1, episode_step_limit=LIMIT, **NOISE)
    w = World(device, oracle, n, **cfg)
    w.env.set_vehicle_schedule(bank, ids)
    tr = w.vector.Trajectory(w.env, steps)
    with pytest.raises(RaptorQuadError, match="chained"):
        teachers.fly(w.vector, device, w.env, w.params, w.state, w.rng, steps, tids, "fused", False, trajectory=tr)
    assert w.rng.epoch == 0 and len(tr) == 0
    teachers.fly(w.vector, device, w.env, w.params, w.state, w.rng, steps, tids, "chained", False, trajectory=tr)
    rec = tr.numpy()
    u = World(device, oracle, n, **cfg)
    u.env.set_vehicle_schedule(bank, ids)
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
    calm = World(device, oracle, n, **cfg)
    teachers.fly(calm.vector, device, calm.env, calm.params, calm.state, calm.rng, steps, tids, "chained", False)
    assert not np.array_equal(snapshot(calm)["state"], snapshot(w)["state"])


# ------------------------------------------------------------------ 4. fused = chained = the step-by-step loop -----
_loops = {}


def _host_loop(device, oracle, suite, setpoints, ids, ref):
    """observe -> (the setpoint's row off the observation, on the host) -> evaluate_step -> step -> assign for T steps with the
    schedule attached; per step what a recording holds and what a rollout leaves behind.  The API has no per-env reset, so the
    loop is the yardstick of every env's FIRST episode: what it does after an env's episode end is not looked at."""
    if ref not in _loops:
        tables, bank = suite
        u = World(device, oracle, N, **KW)
        u.env.set_vehicle_schedule(bank, ids)
        obs = np.zeros((N, 26), np.float32)
        rids = {"none": None, "bank": _mixed_ids(N, 3, 2)}[ref]
        out = dict(obs=[], act=[], rew=[], done=[], state=[], hidden=[], fin_returns=[], fin_lengths=[], fin_terminated=[])
        for t in range(T):
            u.vector.observe(device, u.env, u.params, u.state, obs, u.rng)
            o = obs[:, :22].copy()
            if rids is not None:
                row = setpoints[0][rids, np.minimum(u.env.episode_steps(), LIMIT - 1)]
                o[:, 0:3] -= row[:, 0:3]
                o[:, 12:15] -= row[:, 3:6]
            a = u.policy.evaluate_step(o)
            u.vector.step(device, u.env, u.params, u.state, a, u.next_state, u.rng)
            u.state.assign(u.next_state)
            for k, x in (("obs", o), ("act", a), ("rew", u.env.rewards()), ("done", u.env.done_codes()), ("state", u.state.numpy()),
                         ("hidden", u.policy.hidden_state(N)), ("fin_returns", u.env.finished_returns()),
                         ("fin_lengths", u.env.finished_lengths()), ("fin_terminated", u.env.finished_terminated())):
                out[k].append(np.array(x))
        _loops[ref] = {k: np.stack(v) for k, v in out.items()}
    return _loops[ref]


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
    # two launches joined equal one
    w1, s1, r1 = _fly(device, oracle, weights, setpoints, call, (bank, ids), "fused", autoreset, launches=(T,))
    assert_same(sf, s1, what=what + ", one launch")
    assert_same_recording(rf, r1, what + ", one launch")
    # not vacuous: the mass step ends episodes early for some envs and not for others, and lanes of one wave sit at different rows
    terminated = sf["fin_terminated"] > 0
    print(f"\n[{what}] envs with a terminated episode: {int(terminated.sum())} of {N}; per table {[int(terminated[ids == r].sum()) for r in range(M)]}")
    assert terminated.any() and not terminated.all()
    if autoreset:
        assert len(np.unique(sf["steps"][:64])) >= 3, "one wave's lanes were never at different rows"
    plain = _fly(device, oracle, weights, setpoints, call, None, "fused", autoreset)[1]
    assert not np.array_equal(plain["state"], sf["state"])
    if call.startswith("policy_bank"):
        return                               # (a bank's flight is held to single policies in test_policy_bank_evaluate_by_vehicle)
    loop = _host_loop(device, oracle, suite, setpoints, ids, "bank" if call == "track_refs" else "none")
    first_end = np.argmax(loop["done"] != 0, axis=0)            # every episode ends within LIMIT < T steps
    assert (loop["done"][first_end, np.arange(N)] != 0).all() and first_end.max() < LIMIT
    assert len(np.unique(first_end)) >= 3
    in_first = np.arange(T)[:, None] <= first_end[None, :]      # [T, N]: the transitions of each env's first episode
    for k in ("obs", "act", "rew", "done"):
        assert np.array_equal(bits(rf[k][in_first]), bits(loop[k][in_first])), f"{what}: the loop's {k}"
    at_end = (first_end, np.arange(N))
    if not autoreset:                        # the env froze where its first episode ended: the loop's values of that step
        assert sf["frozen"].all()
        for k, lk in (("state", "state"), ("hidden", "hidden"), ("fin_returns", "fin_returns"), ("fin_lengths", "fin_lengths"),
                      ("fin_terminated", "fin_terminated"), ("rewards", "rew")):
            assert np.array_equal(bits(sf[k]), bits(loop[lk][at_end])), f"{what}: the loop's {k} at the episode end"
    else:
        assert (sf["fin_counts"] >= 2).all()


def test_freeze_then_thaw(device, oracle, suite):
    """a rollout without auto-reset freezes every env at its episode end (a frozen env reads nothing), one with auto-reset thaws them:
    fused = chained through both, and rq_env_reset_statistics restarts the table at row 0"""
    tables, bank = suite
    n = 70
    ids = _mixed_ids(n, M)
    snaps = []
    for mode in ("fused", "chained"):
        w = World(device, oracle, n, **KW)
        w.env.set_vehicle_schedule(bank, ids)
        roll(w, LIMIT + 2, mode, False)
        frozen = world_snapshot(w)
        assert frozen["frozen"].all() and (frozen["steps"] == 0).all()
        roll(w, 5, mode, False)              # later steps do not touch a frozen env
        after = world_snapshot(w)
        assert_same(after, frozen, skip=("epoch", "done"), what=f"frozen, {mode}")
        assert (after["done"] == 4).all()
        roll(w, 10, mode, True)              # thawed: a new episode from the base parameters, the table from row 0
        snaps.append(world_snapshot(w))
    assert_same(snaps[0], snaps[1], what="freeze then thaw")
    assert not snaps[0]["frozen"].any()
    # reset_statistics zeroes the step count: the next step reads row 0 again
    u = World(device, oracle, n, seed=6, domain_randomization=1, episode_step_limit=LIMIT)
    restart = np.stack([vehicles.payload_drop(LIMIT, 4, 1.6, 1.2),              # rows 0 .. 3 a payload; from row 4 on nominal
                        vehicles.slow_motors(LIMIT, 0, 2.0) * vehicles.battery_sag(LIMIT, 4, 4, 0.7)]).astype(np.float32)
    rid = _mixed_ids(n, 2)
    u.env.set_vehicle_schedule(l2f.VehicleBank(device, restart), rid)
    act = np.random.default_rng(9).uniform(-1, 1, (n, 4)).astype(np.float32)
    for _ in range(4):
        u.vector.step(device, u.env, u.params, u.state, act, u.state, u.rng)
    assert (u.env.episode_steps() == 4).all()
    u.env.reset_statistics()
    assert (u.env.episode_steps() == 0).all()
    S, P = u.state.numpy(), u.params.numpy()
    ns = {k: oracle.step(u.cfg, vehicles.compose(P, restart[rid, k]), S, act)[0] for k in (0, 4)}
    u.vector.step(device, u.env, u.params, u.state, act, u.next_state, u.rng)
    out = u.next_state.numpy()
    assert np.array_equal(bits(out), bits(ns[0])) and (out[:, :21] != ns[4][:, :21]).any(axis=1).all()


@pytest.mark.parametrize("n", [8, 65])
def test_small_batches(device, oracle, suite, n):
    tables, bank = suite
    ids = _mixed_ids(n, M)
    out = [_fly_policy(device, oracle, (bank, ids), mode, True, True, {}, n=n)[1:] for mode in ("fused", "chained")]
    assert_same(out[0][0], out[1][0], what=f"{n} envs")
    assert_same_recording(out[0][1], out[1][1], f"{n} envs")
    assert out[0][0]["fin_counts"].min() >= 2


def test_the_two_wave_build(device):
    """beyond 65 536 envs the fused kernel is the 256-register build: fused = chained, bit for bit"""
    from raptor_amd.foundation_policy import Raptor
    n, limit, steps = 65605, 4, 6            # (the second episode is at row 2 when the launch ends: the tables change from row 1 on)
    bank = l2f.VehicleBank(device, [vehicles.nominal(limit), vehicles.payload_pickup(limit, 1, 0.5, 0.8),
                                    vehicles.battery_sag(limit, 0, 3, 0.6), vehicles.slow_motors(limit, 1, 3.0)])
    ids = _mixed_ids(n, M)
    snaps = []
    for mode in ("fused", "chained"):
        b = Batch(device, n, limit=limit, noise=True)
        b.env.set_vehicle_schedule(bank, ids)
        pol = Raptor(device)
        b.fly(pol, steps, mode, True)
        snaps.append(snapshot(b, pol.hidden_state(n)))
    assert_same(snaps[0], snaps[1], what="65 605 envs")
    assert snaps[0]["fin_counts"].min() >= 1
    plain = Batch(device, n, limit=limit, noise=True)
    pol = Raptor(device)
    plain.fly(pol, steps, "fused", True)
    assert not np.array_equal(snapshot(plain, pol.hidden_state(n))["state"], snaps[0]["state"])


# ------------------------------------------------------------------ 5. both schedules -----
def test_both_schedules_chained_equal_the_loop_that_composes_both(device, oracle, suite):
    """a vehicle and a relative wrench schedule on one env, chained: the host loop feeds the oracle the composed params and a wrench
    whose relative units are taken from the step's EFFECTIVE mass; fused is refused with "chained" in the message, nothing enqueued"""
    tables, bank = suite
    n, steps = 70, 12
    gusts = np.stack([disturbances.calm(LIMIT), disturbances.poke(LIMIT, (0.4, -0.3, 0.1), 3, steps=5),
                      disturbances.torque_kick(LIMIT, (0.02, -0.03, 0.01), 5) + disturbances.payload(LIMIT, 0.25, 2)]).astype(np.float32)
    wbank = l2f.WrenchBank(device, gusts, "relative")
    vids, wids = _mixed_ids(n, M), _mixed_ids(n, 3, 1)
    cfg = dict(seed=4, domain_randomization=1, episode_step_limit=LIMIT, disturbance_force_std=0.05, disturbance_torque_std=0.02, **NOISE)
    w = World(device, oracle, n, **cfg)
    w.env.set_vehicle_schedule(bank, vids)
    w.env.set_wrench_schedule(wbank, wids)
    tr = w.vector.Trajectory(w.env, steps)
    before = world_snapshot(w)
    for record in (None, tr):
        with pytest.raises(RaptorQuadError, match="chained") as e:
            roll(w, steps, "fused", True, trajectory=record)
        assert "wrench schedule too" in str(e.value)
    assert_same(world_snapshot(w), before, what="both schedules, fused refused")
    assert w.rng.epoch == 0 and len(tr) == 0
    roll(w, steps, "chained", False, trajectory=tr)
    rec = tr.numpy()
    # the loop: the oracle alone steps, the engine observes and evaluates the policy
    u = World(device, oracle, n, **cfg)
    P = u.params.numpy()
    obs = np.zeros((n, 26), np.float32)
    live = np.ones(n, bool)
    differs = 0
    for t in range(steps):
        u.vector.observe(device, u.env, u.params, u.state, obs, u.rng)
        o = np.ascontiguousarray(obs[:, :22])
        a = u.policy.evaluate_step(o)
        S = u.state.numpy()
        k = np.full(n, t)                    # every env compared is in its first episode: its step count is the step
        Pe = vehicles.compose(P, tables[vids, k])
        fed = S.copy()
        fed[:, S_WRENCH] = disturbances.compose(S[:, S_WRENCH], Pe[:, P_MASS], u.cfg.gravity, P[:, P_ROTOR_XY], gusts[wids, k])
        base_mass = S.copy()
        base_mass[:, S_WRENCH] = disturbances.compose(S[:, S_WRENCH], P[:, P_MASS], u.cfg.gravity, P[:, P_ROTOR_XY], gusts[wids, k])
        differs += int((fed != base_mass).any())
        ns, r, term = oracle.step(u.cfg, Pe, fed, a)
        ns[:, S_WRENCH] = S[:, S_WRENCH]                     # the state keeps the per-episode base
        assert np.array_equal(bits(o[live]), bits(rec["obs"][t][live])) and np.array_equal(bits(a[live]), bits(rec["act"][t][live])), t
        assert np.array_equal(bits(r[live]), bits(rec["rew"][t][live])), t
        assert np.array_equal((term != 0)[live], (rec["done"][t] == 1)[live]), t
        u.state.set(ns)                      # the oracle's state goes on
        live &= rec["done"][t] == 0
    assert differs >= 3 and live.sum() >= n // 2
    assert np.array_equal(bits(w.state.numpy()[live]), bits(u.state.numpy()[live]))


# ------------------------------------------------------------------ 6. refusals -----
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
    c, pb_c, tr_c = world()                  # the twin that never carries a schedule
    for w, p, t in ((a, pb, tr), (c, pb_c, tr_c)):
        roll(w, 3, "fused", True, trajectory=t)
        p.fly(w.vector, device, w.env, w.params, w.state, w.rng, 2, pids)
    a.env.set_vehicle_schedule(bank, ids)

    def look():
        return dict(world_snapshot(a), bank_hidden=pb.hidden(n), recorded=np.full(n, len(tr)), recording=tr.numpy()["obs"].transpose(1, 0, 2))

    before, epoch = look(), a.rng.epoch
    assert epoch == 5 and len(tr) == 3
    act = np.zeros((n, 4), np.float32)
    calls = {
        "step": lambda w, p, t, mode: w.vector.step(device, w.env, w.params, w.state, act, w.state, w.rng),
        "rollout": lambda w, p, t, mode: roll(w, 2, mode, True),
        "record": lambda w, p, t, mode: roll(w, 2, mode, True, trajectory=t),
        "policies": lambda w, p, t, mode: p.fly(w.vector, device, w.env, w.params, w.state, w.rng, 2, pids, mode, True),
        "teachers": lambda w, p, t, mode: teachers.fly(w.vector, device, w.env, w.params, w.state, w.rng, 2, pids, mode, True),
    }

    def refused(what, words, call, mode="chained"):
        with pytest.raises(RaptorQuadError) as e:
            calls[call](a, pb, tr, mode)
        assert words in str(e.value), (what, e.value)
        assert_same(look(), before, what=what)
        assert a.rng.epoch == epoch, what

    # the limit raised after attaching: the bank no longer covers an episode, and every call that steps says so
    cfg = a.env.config
    cfg.episode_step_limit = LIMIT + 1
    a.env.config = cfg
    for call in calls:
        for mode in (("chained",) if call == "step" else ("fused", "chained")):
            if (call, mode) != ("teachers", "fused"):
                refused(f"short bank, {call} {mode}", "vehicle schedule has fewer rows (16) than episode_step_limit (17)", call, mode)
    cfg.episode_step_limit = LIMIT
    a.env.config = cfg
    # fused mode with what the schedule's fused kernel is not taught: refused naming "chained", nothing runs chained instead
    for precision in ("bf16", "f16x2"):
        a.policy.set_precision(precision)
        refused(f"fused {precision}", "chained", "rollout", "fused")
        refused(f"fused {precision} recorded", "vehicle schedule, which the fused kernel of a bf16 / f16x2 policy", "record", "fused")
    a.policy.set_precision("fp32")
    a.policy.set_sample_and_squash("mean")
    refused("fused SampleAndSquash", "SampleAndSquash", "rollout", "fused")
    refused("fused SampleAndSquash", "chained", "record", "fused")
    a.policy.set_sample_and_squash("off")
    refused("fused teachers", "a teacher bank", "teachers", "fused")
    refused("fused teachers", "chained", "teachers", "fused")
    wbank = l2f.WrenchBank(device, [disturbances.calm(LIMIT)])
    a.env.set_wrench_schedule(wbank)
    for call in ("rollout", "record", "policies"):
        refused(f"fused {call} with a wrench schedule too", "an env that carries a wrench schedule too", call, "fused")
        refused(f"fused {call} with a wrench schedule too", "chained", call, "fused")
    a.env.clear_wrench_schedule()
    # a bank of another rq_device; an id outside the bank; destroying an attached bank
    other = l2f.VehicleBank(l2f.Device(0), np.array(tables))
    with pytest.raises(RaptorQuadError) as e:
        a.env.set_vehicle_schedule(other, ids)
    assert e.value.status == -5 and "another device" in str(e.value)
    far = ids.copy()
    far[77] = M
    with pytest.raises(RaptorQuadError) as e:
        _lib.call("rq_env_set_vehicle_schedule", a.env._h, bank._h, far.ctypes.data)
    assert "env 77 names table 4 of a bank of 4" in str(e.value)
    with pytest.raises(RaptorQuadError) as e:
        _lib.call("rq_vehicle_bank_destroy", bank._h)
    assert "attached to" in str(e.value)
    got, back = C.c_void_p(), np.zeros(n, np.uint32)
    _lib.call("rq_env_get_vehicle_schedule", a.env._h, C.byref(got), back.ctypes.data)
    assert got.value == bank._h.value and np.array_equal(back, ids)          # still attached, with the ids it was attached with
    assert_same(look(), before, what="after the refusals")
    # detached, every one of those calls works again and gives what an env that never carried a schedule gives
    a.env.clear_vehicle_schedule()
    _lib.call("rq_env_get_vehicle_schedule", a.env._h, C.byref(got), None)
    assert not got.value
    for w, p, t in ((a, pb, tr), (c, pb_c, tr_c)):
        for precision, sas, mode in (("bf16", "off", "fused"), ("f16x2", "off", "fused"), ("fp32", "mean", "fused"), ("fp32", "off", "chained")):
            w.policy.set_precision(precision)
            w.policy.set_sample_and_squash(sas)
            calls["rollout"](w, p, t, mode)
            calls["record"](w, p, t, mode)
        w.policy.set_sample_and_squash("off")
        calls["step"](w, p, t, "chained")
        calls["policies"](w, p, t, "fused")
        calls["teachers"](w, p, t, "fused")
    assert_same(dict(world_snapshot(a), bank_hidden=pb.hidden(n)), dict(world_snapshot(c), bank_hidden=pb_c.hidden(n)),
                what="after clear_vehicle_schedule")
    assert a.rng.epoch == epoch + 20
    assert_same_recording(tr.numpy(), tr_c.numpy(), "after clear_vehicle_schedule", frozen_too=True)
    # a bank is destroyed once nothing carries it
    solo = l2f.VehicleBank(device, [vehicles.nominal(LIMIT)])
    d = World(device, oracle, 8, **KW)
    d.env.set_vehicle_schedule(solo)
    with pytest.raises(RaptorQuadError):
        _lib.call("rq_vehicle_bank_destroy", solo._h)
    d.env.clear_vehicle_schedule()
    solo._fin()                              # destroys the bank: no longer attached


def test_graph_replay_follows_the_schedule(device, oracle):
    """From 25 steps on the chained mode replays a cached hipGraph whose step nodes carry the schedule's pointers: attaching other
    ids, detaching and attaching again must not fly a graph built for another schedule"""
    n, limit = 70, 30
    kw = dict(seed=6, domain_randomization=1, episode_step_limit=limit)
    bank = l2f.VehicleBank(device, _suite(limit)[1:])
    a, fresh = World(device, oracle, n, **kw), World(device, oracle, n, **kw)       # `fresh`: the same history, never through a graph
    states = []
    for shift in (0, 1, None, 0):
        for w in (a, fresh):
            if shift is None:
                w.env.clear_vehicle_schedule()
            else:
                w.env.set_vehicle_schedule(bank, _mixed_ids(n, 3, shift))
        roll(a, 27, "chained")
        roll(fresh, 27, "fused")
        assert_same(world_snapshot(a), world_snapshot(fresh), what=f"shift {shift}")
        states.append(a.state.numpy())
    stale = World(device, oracle, n, **kw)
    stale.env.set_vehicle_schedule(bank, _mixed_ids(n, 3, 0))
    for _ in range(2):
        roll(stale, 27, "fused")
    assert not np.array_equal(stale.state.numpy(), states[1])


# ------------------------------------------------------------------ 7. PolicyBank.evaluate(vehicle_ids=) -----
@pytest.mark.parametrize("mode", ["fused", "chained"])
def test_policy_bank_evaluate_by_vehicle(device, weights, suite, mode):
    """tracking_rmse is [P, M]; each cell is what a single Raptor flies on that scenario's envs alone (the same global env ids)"""
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.policy_bank import PolicyBank
    tables, bank = suite
    n, Pn, steps = 128, 2, 40
    W = bank_weights(weights, Pn)
    pids = ids_of([1, 0], n)
    vids = np.tile(np.repeat(np.arange(M, dtype=np.uint32), 64 // M), n // 64)          # runs of 16 envs per scenario inside a block
    hold = l2f.Reference(device, tracking.hold(LIMIT))
    whole = Batch(device, n, limit=LIMIT, noise=True, via="fly")
    whole.env.set_vehicle_schedule(bank)
    pb = PolicyBank(device, W)
    table = pb.evaluate(whole.vector, device, whole.env, whole.params, whole.state, whole.rng, steps, pids, mode=mode, reference=hold,
                        vehicle_ids=vids)
    assert np.array_equal(whole.env.vehicle_schedule[1], vids)
    rmse = np.asarray(table["tracking_rmse"])
    assert rmse.shape == (Pn, M) and np.isfinite(rmse).all() and len(np.unique(rmse)) == Pn * M
    sq, cnt = whole.env.tracking_error()
    for lo in range(0, n, 16):
        p, m = int(pids[lo]), int(vids[lo])
        b = Batch(device, 16, offset=OFFSET + lo, limit=LIMIT, noise=True)
        b.env.set_vehicle_schedule(bank, np.full(16, m, np.uint32))
        b.fly(Raptor(device, weights=W[p]), steps, mode, True, ref=hold)
        bsq, bcnt = b.env.tracking_error()
        assert np.array_equal(bits(bsq), bits(sq[lo:lo + 16])) and np.array_equal(bcnt, cnt[lo:lo + 16]), (lo, p, m)
        assert np.isclose(np.sqrt(bsq.astype(np.float64).sum() / bcnt.sum()), rmse[p, m], rtol=1e-12, atol=0), (lo, p, m)
    whole.env.set_wrench_schedule(l2f.WrenchBank(device, [disturbances.calm(LIMIT)]))
    with pytest.raises(ValueError, match="give one of them"):
        pb.evaluate(whole.vector, device, whole.env, whole.params, whole.state, whole.rng, steps, pids, mode="chained", reference=hold,
                    vehicle_ids=vids, wrench_ids=np.zeros(n, np.uint32))


# ------------------------------------------------------------------ 8. the point of it -----
def test_a_payload_pickup_makes_the_vehicle_sag(device, oracle):
    """the shipped policy on tracking.hold from near the setpoint, 128 envs, half of them pick up half their mass at step 100: the
    deviation in the 20 steps after the change is above that of the 20 steps before and above the nominal half's.  The ordering
    alone is asserted (the CPU oracle flying this: mean |z| 0.040 -> 0.057 m against 0.028 m nominal); the sizes are the example's."""
    n, limit, at = 128, 160, 100
    hold = l2f.Reference(device, tracking.hold(limit))
    bank = l2f.VehicleBank(device, [vehicles.nominal(limit), vehicles.payload_pickup(limit, at, 1.5, 1.0)])
    ids = (np.arange(n) % 2).astype(np.uint32)
    w = World(device, oracle, n, seed=8, domain_randomization=1, episode_step_limit=limit, init_max_position=0.1,
              init_max_linear_velocity=0.2, init_max_angle=0.3, init_max_angular_velocity=0.2)
    w.env.set_vehicle_schedule(bank, ids)
    tr = w.vector.Trajectory(w.env, limit)
    roll(w, limit, "fused", True, trajectory=tr, reference=hold)
    ft = probing.flight_table(tr, edges=probing.linear_age_edges(at - 20, at + 40, 3), device=False)
    dev = np.asarray(ft.by_group(ids, 2)["rms_position"])          # [2, 3]: nominal | pickup x before, after, later
    rec = tr.numpy()
    age = probing.episode_steps(rec["done"])
    absz = np.abs(rec["obs"][:, :, 2])
    z = np.array([[absz[(age >= lo) & (age < lo + 20) & (ids == g)[None, :] & (rec["done"] != 4)].mean() for lo in (at - 20, at, at + 20)]
                  for g in (0, 1)])
    print(f"\n[payload pickup at {at}] rms deviation nominal {np.round(dev[0], 4)}, pickup {np.round(dev[1], 4)}; "
          f"mean |z| nominal {np.round(z[0], 4)}, pickup {np.round(z[1], 4)}")
    assert z[1, 1] > z[1, 0] and z[1, 1] > z[0, 1]
    assert dev[1, 1] > dev[1, 0] and dev[1, 1] > dev[0, 1]
