"""The wrench schedule (rq_wrench_bank_*, rq_env_set_wrench_schedule): a table of scheduled forces and torques per env, honoured by
everything that steps the env.  The anchor is independent of every new kernel: rq_step with a schedule attached against the
oracle's step fed a state whose wrench fields were composed on the host (raptor_amd.disturbances.compose) - the existing suite
shows the oracle's step and k_step agree bit for bit.  Everything else is held to that path, or to the kernels without a schedule,
on the bits: no tolerance anywhere but in the closed form."""
import ctypes as C

import numpy as np
import pytest

import raptor_amd.l2f as l2f
from raptor_amd import _lib, disturbances, tracking
from raptor_amd._lib import RaptorQuadError
from gpu_common import World
from rollout_common import (NOISE, OFFSET, Batch, assert_same, assert_same_recording, bank_weights, bits, ids_of, join, random_table,
                            roll, snapshot, world_snapshot)
from schedule_common import LAUNCHES, N, Flights, mixed_ids as _mixed_ids, reference_kw as _reference_kw

pytestmark = pytest.mark.gpu

P_MASS, P_ROTOR_XY = 0, slice(4, 6)         # RQ_P_MASS, RQ_P_ROTOR_POS + 0 / + 1
S_WRENCH = slice(21, 27)                    # RQ_S_FORCE, RQ_S_TORQUE


def _anchor_tables(units):
    """calm; a force gust on steps 3..6; a torque kick at step 5 plus a payload - in the bank's units"""
    rows = 12
    f, tq = (1.0, 1.0) if units == "relative" else (0.027 * 9.81, 0.027 * 9.81 * 0.04)      # absolute: about the same physical size
    gust = disturbances.poke(rows, (0.4 * f, -0.3 * f, 0.1 * f), 3, steps=4)
    kick = disturbances.torque_kick(rows, (0.02 * tq, -0.03 * tq, 0.01 * tq), 5) + disturbances.payload(rows, 0.25 * f, 2)
    return np.stack([disturbances.calm(rows), gust, kick]).astype(np.float32)


@pytest.mark.parametrize("units", ["relative", "absolute"])
def test_step_with_a_schedule_equals_the_oracle_fed_the_composed_wrench(device, oracle, units):
    n, limit = 70, 12                        # one full wave plus a ragged 6
    tables = _anchor_tables(units)
    ids = _mixed_ids(n, 3)
    w = World(device, oracle, n, seed=4, domain_randomization=1, episode_step_limit=limit, disturbance_force_std=0.05,
              disturbance_torque_std=0.02)
    bank = l2f.WrenchBank(device, tables, units)
    w.env.set_wrench_schedule(bank, ids)
    got = w.env.wrench_schedule
    assert got[0] is bank and np.array_equal(got[1], ids)
    act = np.random.default_rng(7).uniform(-1, 1, (n, 4)).astype(np.float32)
    P = w.params.numpy()
    assert np.array_equal(P, w.P) and len(np.unique(P[:, P_MASS])) > n // 2          # a domain-randomised population
    composed_differs = 0
    for doubled in (False, True):
        if doubled:                          # rq_params_set after attaching is honoured: the scales come from the call's params
            P = P.copy()
            P[:, P_MASS] *= 2
            w.params.set(P)
        for t in range(limit):
            S = w.state.numpy()
            k = w.env.episode_steps()           # (random actions for 0.12 s: the limit ends the episode at step 12, hardly anything else)
            row = tables[ids, np.minimum(k, limit - 1)]
            fed = S.copy()
            fed[:, S_WRENCH] = disturbances.compose(S[:, S_WRENCH], P[:, P_MASS], w.cfg.gravity, P[:, P_ROTOR_XY], row, units)
            composed_differs += int((fed[:, S_WRENCH] != S[:, S_WRENCH]).any())
            ns, r, term = oracle.step(w.cfg, P, fed, act)
            w.vector.step(device, w.env, w.params, w.state, act, w.next_state, w.rng)
            out = w.next_state.numpy()
            assert np.array_equal(bits(out[:, :21]), bits(ns[:, :21])), (units, doubled, t)
            assert np.array_equal(bits(out[:, S_WRENCH]), bits(S[:, S_WRENCH])), (units, doubled, t)       # the state keeps the base
            assert np.array_equal(bits(w.env.rewards()), bits(r)) and np.array_equal(w.env.terminated(), term), (units, doubled, t)
            w.state.assign(w.next_state)
        assert (w.env.finished_counts() >= (2 if doubled else 1)).all()
    assert composed_differs >= 2 * (limit - 3)          # the tables are not calm: all but the first rows change somebody's wrench
    # not vacuous the other way: without the schedule the same step gives another state
    w.env.clear_wrench_schedule()
    assert w.env.wrench_schedule is None
    for t in range(4):
        w.vector.step(device, w.env, w.params, w.state, act, w.state, w.rng)
    S = w.state.numpy()
    ns, _, _ = oracle.step(w.cfg, P, S, act)
    w.vector.step(device, w.env, w.params, w.state, act, w.next_state, w.rng)
    assert np.array_equal(bits(w.next_state.numpy()), bits(ns))          # rows 4 .. 6 would have pushed the gust's envs


# ------------------------------------------------------------------ 2. closed form -----
def test_a_constant_force_gives_the_closed_form(device):
    """Absolute units, the nominal Crazyflie level at hover with every rotor at hover speed and hover actions, 0.01 N along x for
    50 steps: v_x = F t / m and x = F t^2 / 2 m.  RK4 is exact for a constant acceleration and 50 fp32 accumulations bound the
    error near 50 * 2^-24 = 3e-6 relative: the tolerance of 1e-4 leaves about 30 x room.  |y|, |z|, the other velocities and the
    attitude stay within the bounds of test_hover_equilibrium_and_torque_sign_conventions (2e-4 m, 5e-4 m/s, 1e-4 rad/s)."""
    n, steps, F = 64, 50, 0.01
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
    table = np.zeros((int(cfg.episode_step_limit), 6), np.float32)
    table[:, 0] = F
    env.set_wrench_schedule(l2f.WrenchBank(device, [table], "absolute"))
    act = np.repeat(P[:, 25:26], 4, axis=1).astype(np.float32)          # hover action
    for _ in range(steps):
        v.step(device, env, params, state, act, state, rng)
    s = state.numpy().astype(np.float64)
    t, m = steps * float(cfg.dt), float(P[0, P_MASS])
    vx, x = F * t / m, F * t * t / (2 * m)
    print(f"\n[constant force] v_x {s[0, 7]:.9f} (closed form {vx:.9f}), x {s[0, 0]:.9f} ({x:.9f}), |y|,|z| {np.abs(s[:, 1:3]).max():.2e}, "
          f"|v_yz| {np.abs(s[:, 8:10]).max():.2e}, |w| {np.abs(s[:, 10:13]).max():.2e}, |q_xyz| {np.abs(s[:, 4:7]).max():.2e}")
    assert np.abs(s[:, 7] / vx - 1).max() < 1e-4 and np.abs(s[:, 0] / x - 1).max() < 1e-4
    assert np.abs(s[:, 1:3]).max() < 2e-4 and np.abs(s[:, 8:10]).max() < 5e-4
    assert np.abs(s[:, 10:13]).max() < 1e-4 and np.abs(s[:, 4:7]).max() < 1e-4 and np.abs(s[:, 3] - 1).max() < 1e-6
    assert not s[:, S_WRENCH].any()          # the schedule is never written into the state


# ------------------------------------------------------------------ the rollouts' shared shape -----
LIMIT = 16
T = sum(LAUNCHES)
M = 3
# gusts strong enough, and a velocity threshold tight enough, that the gusted envs terminate mid-episode (table 0 is calm)
KW = dict(seed=5, domain_randomization=1, episode_step_limit=LIMIT, termination_linear_velocity=2.5, **NOISE)


@pytest.fixture(scope="module")
def gusts(device):
    t = np.stack([disturbances.calm(LIMIT),
                  disturbances.poke(LIMIT, (6.0, 0.0, 0.0), 3, steps=6) + disturbances.torque_kick(LIMIT, (0.0, 0.02, 0.0), 2),
                  disturbances.poke(LIMIT, (0.0, -4.0, 1.0), 6, steps=8) + disturbances.payload(LIMIT, 0.3, 1)]).astype(np.float32)
    t.setflags(write=False)
    return t, l2f.WrenchBank(device, np.array(t))


@pytest.fixture(scope="module")
def calm_bank(device):
    return l2f.WrenchBank(device, [disturbances.calm(LIMIT), disturbances.calm(LIMIT)])


@pytest.fixture(scope="module")
def setpoints(device):
    t = np.stack([random_table(LIMIT, 51 + r) for r in range(M)])
    return t, l2f.Reference(device, np.array(t[1])), l2f.ReferenceBank(device, t)


_flights = Flights("wrench", KW)
_fly_policy, _fly_policy_bank = _flights.fly_policy, _flights.fly_policy_bank


# ------------------------------------------------------------------ 3. a zero table is no schedule -----
@pytest.mark.parametrize("autoreset", [True, False])
@pytest.mark.parametrize("mode", ["fused", "chained"])
@pytest.mark.parametrize("call", ["rollout", "track_refs", "interval3", "policy_bank"])
def test_a_calm_schedule_is_no_schedule(device, oracle, weights, calm_bank, setpoints, call, mode, autoreset):
    """crosses the schedule's kernels with the ones that existed before it: snapshot and recording, bit for bit"""
    ids = _mixed_ids(N, 2)
    out = []
    for schedule in ((calm_bank, ids), None):
        if call == "policy_bank":
            _, snap, rec = _fly_policy_bank(device, oracle, weights, schedule, mode, autoreset, True, {})
        else:
            ref_kw = _reference_kw(setpoints, "bank") if call == "track_refs" else {}
            _, snap, rec = _fly_policy(device, oracle, schedule, mode, autoreset, True, ref_kw, 3 if call == "interval3" else 1)
        out.append((snap, rec))
    what = f"{call} {mode} autoreset={autoreset}"
    assert_same(out[0][0], out[1][0], what=what)
    assert_same_recording(out[0][1], out[1][1], what)
    assert out[0][0]["fin_counts"].min() >= 1 and out[0][0]["epoch"][0] == T


# ------------------------------------------------------------------ 4. fused = chained = the step-by-step loop -----
_loops = {}


def _host_loop(device, oracle, gusts, setpoints, ids, ref, interval):
    """observe -> (the setpoint's row off the observation, on the host) -> evaluate_step -> step -> assign for T steps with the
    schedule attached; per step what a recording holds and what a rollout leaves behind.  The API has no per-env reset, so the
    loop is the yardstick of every env's FIRST episode: what it does after an env's episode end is not looked at."""
    key = (ref, interval)
    if key not in _loops:
        tables, bank = gusts
        u = World(device, oracle, N, **KW)
        u.policy.native_interval = interval
        u.env.set_wrench_schedule(bank, ids)
        obs = np.zeros((N, 26), np.float32)
        rids = {"none": None, "single": np.ones(N, np.int64), "bank": _mixed_ids(N, M, 2)}[ref]
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
        _loops[key] = {k: np.stack(v) for k, v in out.items()}
    return _loops[key]


@pytest.mark.parametrize("interval", [1, 3])
@pytest.mark.parametrize("ref", ["none", "single", "bank"])
@pytest.mark.parametrize("record", [True, False])
@pytest.mark.parametrize("autoreset", [True, False])
def test_fused_equals_chained_equals_the_loop(device, oracle, gusts, setpoints, autoreset, record, ref, interval):
    tables, bank = gusts
    ids = _mixed_ids(N, M)
    ref_kw = _reference_kw(setpoints, ref)
    what = f"autoreset={autoreset} record={record} {ref} interval {interval}"
    wf, sf, rf = _fly_policy(device, oracle, (bank, ids), "fused", autoreset, record, ref_kw, interval)
    wc, sc, rc = _fly_policy(device, oracle, (bank, ids), "chained", autoreset, record, ref_kw, interval)
    assert_same(sf, sc, what=what)           # state, hidden state, statistics, finished-episode records, done codes, tracking sums, rng epoch
    if record:
        assert_same_recording(rf, rc, what)
    assert sf["epoch"][0] == T
    # not vacuous: the gusts end episodes early for some envs and not for others, and lanes of one wave sit at different rows
    terminated = sf["fin_terminated"] > 0
    print(f"\n[{what}] envs with a terminated episode: {int(terminated.sum())} of {N}; per table {[int(terminated[ids == r].sum()) for r in range(M)]}")
    assert terminated.any() and not terminated.all()
    if autoreset:
        assert len(np.unique(sf["steps"][:64])) >= 3, "one wave's lanes were never at different rows"
    loop = _host_loop(device, oracle, gusts, setpoints, ids, ref, interval)
    first_end = np.argmax(loop["done"] != 0, axis=0)            # every episode ends within LIMIT < T steps
    assert (loop["done"][first_end, np.arange(N)] != 0).all() and first_end.max() < LIMIT
    assert len(np.unique(first_end)) >= 3
    in_first = np.arange(T)[:, None] <= first_end[None, :]      # [T, N]: the transitions of each env's first episode
    if record:
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


# ------------------------------------------------------------------ 5. bank flight = its slices -----
@pytest.mark.parametrize("mode", ["fused", "chained"])
def test_bank_flight_equals_its_slices(device, weights, gusts, setpoints, mode):
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.policy_bank import PolicyBank
    tables, bank = gusts
    W = bank_weights(weights, 4)
    rates = [1, 3, 1, 2]
    blocks = [2, 0, 3, 1]
    pids, ids = ids_of(blocks, N), _mixed_ids(N, M)
    ref = setpoints[1]
    cfg = dict(termination_linear_velocity=KW["termination_linear_velocity"])

    def batch(n, offset):
        b = Batch(device, n, offset=offset, limit=LIMIT, noise=True, via="fly")
        c = b.env.config
        c.termination_linear_velocity = cfg["termination_linear_velocity"]
        b.env.config = c
        return b

    whole = batch(N, OFFSET)
    whole.env.set_wrench_schedule(bank, ids)
    pb = PolicyBank(device, W, native_interval=rates)
    rec = whole.fly(pb, list(LAUNCHES), mode, True, True, ids=pids, ref=ref)
    snap = snapshot(whole, pb.hidden(N))
    slices = []
    for g, p in enumerate(blocks):
        lo, hi = 64 * g, min(64 * g + 64, N)
        b = batch(hi - lo, OFFSET + lo)
        b.env.set_wrench_schedule(bank, ids[lo:hi])
        pol = Raptor(device, weights=W[p], native_interval=rates[p])
        r = b.fly(pol, list(LAUNCHES), mode, True, True, ref=ref)
        slices.append((snapshot(b, pol.hidden_state(hi - lo)), r))
    want_snap, want_rec = join(slices)
    assert_same(snap, want_snap, what=mode)
    assert_same_recording(rec, want_rec, mode, frozen_too=True)
    assert (snap["fin_terminated"] > 0).any() and snap["fin_counts"].min() >= 2


# ------------------------------------------------------------------ 6. the two-wave build -----
def test_the_two_wave_build(device):
    """beyond 65 536 envs the fused kernel is the 256-register build: fused = chained, bit for bit"""
    from raptor_amd.foundation_policy import Raptor
    n, limit, steps = 65600, 4, 6
    tables = np.stack([disturbances.calm(limit), disturbances.poke(limit, (3.0, 0.0, 0.5), 1, steps=2),
                       disturbances.torque_kick(limit, (0.02, 0.0, -0.01), 0, steps=4)]).astype(np.float32)
    bank = l2f.WrenchBank(device, tables)
    ids = _mixed_ids(n, 3)
    snaps = []
    for mode in ("fused", "chained"):
        b = Batch(device, n, limit=limit, noise=True)
        b.env.set_wrench_schedule(bank, ids)
        pol = Raptor(device)
        b.fly(pol, steps, mode, True)
        snaps.append(snapshot(b, pol.hidden_state(n)))
    assert_same(snaps[0], snaps[1], what="65 600 envs")
    assert snaps[0]["fin_counts"].min() >= 1
    plain = Batch(device, n, limit=limit, noise=True)
    pol = Raptor(device)
    plain.fly(pol, steps, "fused", True)
    assert not np.array_equal(snapshot(plain, pol.hidden_state(n))["state"], snaps[0]["state"])


# ------------------------------------------------------------------ 7. a teacher bank, chained -----
def test_a_teacher_bank_chained_equals_the_evaluate_loop(device, oracle):
    """rq_rollout_teachers in chained mode on an env with a schedule against observe -> rq_teacher_bank_evaluate -> step -> assign,
    12 steps in a window without episode ends; the fused teacher kernel is not taught the rule and says so"""
    from raptor_amd.teachers import TeacherBank, layers_parameter_count
    n, steps, K, rows = 70, 12, 5, 13
    g = np.random.default_rng(2)
    widths, prev, parts = [32, 16], 22, []
    W = np.empty((K, layers_parameter_count(22, widths)), np.float32)
    for k in range(K):
        parts, prev = [], 22
        for h in widths + [4]:
            parts += [g.standard_normal(h * prev) * 0.2 / np.sqrt(prev), g.standard_normal(h) * 0.1]
            prev = h
        W[k] = np.concatenate(parts).astype(np.float32)
    teachers = TeacherBank.from_layers(device, W, 22, widths, "tanh", "identity", "fp32")
    tids = (np.arange(n) % K).astype(np.uint32)
    tables = np.stack([disturbances.calm(rows), disturbances.poke(rows, (0.5, -0.3, 0.2), 3, steps=5),
                       disturbances.torque_kick(rows, (0.01, 0.02, -0.01), 6, steps=2)]).astype(np.float32)
    bank = l2f.WrenchBank(device, tables)
    ids = _mixed_ids(n, 3)
    cfg = dict(seed=3, domain_randomization=1, episode_step_limit=rows, **NOISE)
    w = World(device, oracle, n, **cfg)
    w.env.set_wrench_schedule(bank, ids)
    tr = w.vector.Trajectory(w.env, steps)
    with pytest.raises(RaptorQuadError, match="wrench schedule"):
        teachers.fly(w.vector, device, w.env, w.params, w.state, w.rng, steps, tids, "fused", False, trajectory=tr)
    assert w.rng.epoch == 0 and len(tr) == 0
    teachers.fly(w.vector, device, w.env, w.params, w.state, w.rng, steps, tids, "chained", False, trajectory=tr)
    rec = tr.numpy()
    assert (rec["done"] == 0).all()
    u = World(device, oracle, n, **cfg)
    u.env.set_wrench_schedule(bank, ids)
    obs = np.zeros((n, 26), np.float32)
    for t in range(steps):
        u.vector.observe(device, u.env, u.params, u.state, obs, u.rng)
        o = np.ascontiguousarray(obs[:, :22])
        a = teachers.evaluate(o, tids)
        assert np.array_equal(bits(o), bits(rec["obs"][t])) and np.array_equal(bits(a), bits(rec["act"][t])), t
        u.vector.step(device, u.env, u.params, u.state, a, u.next_state, u.rng)
        u.state.assign(u.next_state)
        assert np.array_equal(bits(u.env.rewards()), bits(rec["rew"][t])) and np.array_equal(u.env.done_codes(), rec["done"][t]), t
    assert_same(snapshot(w), snapshot(u), what="teacher bank")
    calm = World(device, oracle, n, **cfg)
    teachers.fly(calm.vector, device, calm.env, calm.params, calm.state, calm.rng, steps, tids, "chained", False)
    assert not np.array_equal(snapshot(calm)["state"], snapshot(w)["state"])


# ------------------------------------------------------------------ 8. frozen envs and restarts -----
def test_frozen_envs_read_nothing_and_reset_statistics_restarts_the_table(device, oracle, gusts):
    tables, bank = gusts
    n = 70
    ids = _mixed_ids(n, M)
    w = World(device, oracle, n, **KW)
    w.env.set_wrench_schedule(bank, ids)
    roll(w, LIMIT + 2, "fused", False)                   # every env flies its one episode and freezes
    before = world_snapshot(w)
    assert before["frozen"].all() and (before["steps"] == 0).all()
    for mode in ("fused", "chained"):
        roll(w, 5, mode, False)                          # later steps do not touch a frozen env
        after = world_snapshot(w)
        assert_same(after, before, skip=("epoch", "done"), what=f"frozen, {mode}")
        assert (after["done"] == 4).all()
    # rq_env_reset_statistics zeroes the step count: the table restarts at row 0
    restart = np.stack([disturbances.poke(LIMIT, (0.5, 0.0, 0.0), 0) + disturbances.poke(LIMIT, (0.0, 0.5, 0.0), 4),
                        disturbances.torque_kick(LIMIT, (0.02, 0.0, 0.0), 0) + disturbances.payload(LIMIT, 0.3, 4)]).astype(np.float32)
    ids = _mixed_ids(n, 2)
    u = World(device, oracle, n, seed=6, domain_randomization=1, episode_step_limit=LIMIT)
    u.env.set_wrench_schedule(l2f.WrenchBank(device, restart), ids)
    act = np.random.default_rng(9).uniform(-1, 1, (n, 4)).astype(np.float32)
    for _ in range(4):
        u.vector.step(device, u.env, u.params, u.state, act, u.state, u.rng)
    assert (u.env.episode_steps() == 4).all()
    u.env.reset_statistics()
    assert (u.env.episode_steps() == 0).all()
    S, P = u.state.numpy(), u.params.numpy()
    ns = {}
    for k in (0, 4):
        fed = S.copy()
        fed[:, S_WRENCH] = disturbances.compose(S[:, S_WRENCH], P[:, P_MASS], u.cfg.gravity, P[:, P_ROTOR_XY], restart[ids, k])
        ns[k] = oracle.step(u.cfg, P, fed, act)[0]
    unscheduled = oracle.step(u.cfg, P, S, act)[0]
    u.vector.step(device, u.env, u.params, u.state, act, u.next_state, u.rng)
    out = u.next_state.numpy()
    assert np.array_equal(bits(out[:, :21]), bits(ns[0][:, :21]))
    assert (out[:, :21] != ns[4][:, :21]).any(axis=1).all() and (out[:, :21] != unscheduled[:, :21]).any(axis=1).all()


# ------------------------------------------------------------------ 9. refusals -----
def test_refusals_leave_everything_untouched(device, oracle, weights, gusts):
    from raptor_amd.policy_bank import PolicyBank
    from raptor_amd.teachers import TeacherBank, layers_parameter_count
    tables, bank = gusts
    n = 128
    ids = _mixed_ids(n, M)
    pids = ids_of([1, 0], n)
    g = np.random.default_rng(3)
    teachers = TeacherBank.from_layers(device, (0.1 * g.standard_normal((2, layers_parameter_count(22, [16, 16])))).astype(np.float32),
                                       22, [16, 16], "tanh", "tanh", "fp32")
    W = bank_weights(weights, 2)

    def world():
        w = World(device, oracle, n, **KW)
        return w, PolicyBank(device, W), w.vector.Trajectory(w.env, 30)

    a, pb, tr = world()
    c, pb_c, tr_c = world()                  # the twin that never carries a schedule
    for w, p, t in ((a, pb, tr), (c, pb_c, tr_c)):
        roll(w, 3, "fused", True, trajectory=t)
        p.fly(w.vector, device, w.env, w.params, w.state, w.rng, 2, pids)
    a.env.set_wrench_schedule(bank, ids)

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
                refused(f"short bank, {call} {mode}", "fewer rows (16) than episode_step_limit (17)", call, mode)
    cfg.episode_step_limit = LIMIT
    a.env.config = cfg
    # fused mode with what the schedule's fused kernel is not taught: refused naming the schedule, nothing runs chained instead
    for precision in ("bf16", "f16x2"):
        a.policy.set_precision(precision)
        refused(f"fused {precision}", "wrench schedule", "rollout", "fused")
        refused(f"fused {precision} recorded", "bf16 / f16x2 policy", "record", "fused")
    a.policy.set_precision("fp32")
    a.policy.set_sample_and_squash("mean")
    refused("fused SampleAndSquash", "SampleAndSquash", "rollout", "fused")
    a.policy.set_sample_and_squash("off")
    refused("fused teachers", "a teacher bank", "teachers", "fused")
    # a bank of another rq_device; an id outside the bank; destroying an attached bank
    other = l2f.WrenchBank(l2f.Device(0), np.array(tables))
    with pytest.raises(RaptorQuadError) as e:
        a.env.set_wrench_schedule(other, ids)
    assert e.value.status == -5 and "another device" in str(e.value)
    far = ids.copy()
    far[77] = M
    with pytest.raises(RaptorQuadError) as e:
        _lib.call("rq_env_set_wrench_schedule", a.env._h, bank._h, far.ctypes.data)
    assert "env 77 names table 3 of a bank of 3" in str(e.value)
    with pytest.raises(RaptorQuadError) as e:
        _lib.call("rq_wrench_bank_destroy", bank._h)
    assert "attached to" in str(e.value)
    got, back = C.c_void_p(), np.zeros(n, np.uint32)
    _lib.call("rq_env_get_wrench_schedule", a.env._h, C.byref(got), back.ctypes.data)
    assert got.value == bank._h.value and np.array_equal(back, ids)          # still attached, with the ids it was attached with
    assert_same(look(), before, what="after the refusals")
    # detached, every one of those calls works again and gives what an env that never carried a schedule gives
    a.env.clear_wrench_schedule()
    _lib.call("rq_env_get_wrench_schedule", a.env._h, C.byref(got), None)
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
                what="after clear_wrench_schedule")
    assert a.rng.epoch == epoch + 20
    assert_same_recording(tr.numpy(), tr_c.numpy(), "after clear_wrench_schedule", frozen_too=True)


# ------------------------------------------------------------------ the chained mode's graph -----
def test_graph_replay_follows_the_schedule(device, oracle):
    """From 25 steps on the chained mode replays a cached hipGraph whose step nodes carry the schedule's pointers: attaching other
    ids, detaching and attaching again must not fly a graph built for another schedule"""
    n, limit = 70, 30
    kw = dict(seed=6, domain_randomization=1, episode_step_limit=limit)
    tables = np.stack([disturbances.calm(limit), disturbances.poke(limit, (0.5, 0.0, 0.2), 2, steps=20),
                       disturbances.torque_kick(limit, (0.0, 0.01, 0.0), 4, steps=3) + disturbances.payload(limit, 0.3, 1)]).astype(np.float32)
    bank = l2f.WrenchBank(device, tables)
    a, fresh = World(device, oracle, n, **kw), World(device, oracle, n, **kw)       # `fresh`: the same history, never through a graph
    states = []
    for shift in (0, 1, None, 0):
        for w in (a, fresh):
            if shift is None:
                w.env.clear_wrench_schedule()
            else:
                w.env.set_wrench_schedule(bank, _mixed_ids(n, 3, shift))
        roll(a, 27, "chained")
        roll(fresh, 27, "fused")
        assert_same(world_snapshot(a), world_snapshot(fresh), what=f"shift {shift}")
        states.append(a.state.numpy())
    # not vacuous: the first schedule kept for the second launch is another flight (the episode under way at step 54 began at step 30)
    stale = World(device, oracle, n, **kw)
    stale.env.set_wrench_schedule(bank, _mixed_ids(n, 3, 0))
    for _ in range(2):
        roll(stale, 27, "fused")
    assert not np.array_equal(stale.state.numpy(), states[1])


# ------------------------------------------------------------------ 10. it does something -----
def test_a_gust_costs_tracking_error(device, oracle):
    """the shipped policy on tracking.hold, 128 envs, a 100-step episode with and without 0.5 m g along y over steps 20..50"""
    n, limit = 128, 100
    hold = l2f.Reference(device, tracking.hold(limit))
    gust = l2f.WrenchBank(device, [disturbances.poke(limit, (0.0, 0.5, 0.0), 20, steps=31)])
    result = {}
    for name in ("calm", "gust"):
        w = World(device, oracle, n, seed=8, domain_randomization=1, episode_step_limit=limit)
        if name == "gust":
            w.env.set_wrench_schedule(gust)
        roll(w, limit, "fused", True, reference=hold)
        sq, steps = w.env.tracking_error()
        result[name] = (float(np.sqrt(sq.astype(np.float64).sum() / steps.sum())), int((w.env.finished_terminated() > 0).sum()))
        assert steps.sum() == n * limit
    print(f"\n[hold, {n} envs, {limit} steps] tracking RMSE calm {result['calm'][0]:.4f} m, with the gust {result['gust'][0]:.4f} m; "
          f"envs terminated: calm {result['calm'][1]}, gust {result['gust'][1]}")
    assert result["gust"][0] > result["calm"][0]
