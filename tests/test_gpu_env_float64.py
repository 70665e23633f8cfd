"""The env kernels against float64 (tests/env_reference.py): ONE step from a state the test sets - the closed loop is chaotic for a few
per cent of the fleet, so nothing here is a recurrence - through ``vector.step`` (k_step), ``vector.observe``, the three physics
schedules taken as physics, and the fused rollout's hand-packed step flown by policies whose output is a constant.  Every element of
the next state, the reward and the flag is held to the bound ``step_bound`` derives; envs whose termination is undecided (the
reference within its bound of a threshold) are excluded from the flag and the reward only.  The negative controls hold the same
results to references with one mistake each and must find them outside.  ``pytest -s`` prints the largest err / bound per path and
param family.

Largest err / bound on the MI355X, first run (state, reward; 1 is the bound; the batches 1, 63, 64, 65, 1000, 1100 together):
    path                     params       state  reward
    step                     nominal      0.808  0.393
    step                     sampled      0.812  0.366
    step                     smallest     0.877  0.340
    step                     largest      0.788  0.399
    step                     fast_motors  0.827  0.366
    step                     composed     0.840  0.305
    observe                  all five     0.934
    schedule wrench          sampled      0.815  0.383
    schedule wrench_absolute sampled      0.795  0.328
    schedule vehicle         sampled      0.821  0.325
    schedule wind            sampled      0.793  0.377
    schedule all             sampled      0.860  0.385
    fused plain              sampled      0.858  0.352
    fused vehicle            sampled      0.771  0.340
    fused wind               sampled      0.774  0.336
    fused plain              smallest     0.766  0.276
    fused vehicle            smallest     0.878  0.308
    fused wind               smallest     0.883  0.276
    fused plain              largest      0.748  0.334
    fused vehicle            largest      0.797  0.311
    fused wind               largest      0.781  0.325
    fused plain              fast_motors  0.801  0.359
    fused vehicle            fast_motors  0.806  0.361
    fused wind               fast_motors  0.793  0.428
Against the altered references the device is outside on 94 % (k_step) and 99.6 % (fused) of the envs for no_gyroscopic, 98.6 % and
99.9 % for tau_exchanged, and on every env for wind_refreshed_per_stage.  No constant of the model - the reference, the bound, the
families - was changed after the first GPU run; no kernel disagreed, so nothing under csrc changed.
"""
import numpy as np
import pytest

import env_reference as R
import raptor_amd.l2f as l2f
from raptor_amd.policy_bank import PolicyBank
from rollout_common import bits
from schedule_common import mixed_ids
from test_env_reference_cpu import SEED, held, rows_of

pytestmark = pytest.mark.gpu

BATCHES = (1, 63, 64, 65, 1000, 1100)        # the wave tail and both sides of the 1 024-env mailbox
_worst = {}


def _note(path, pf, ratios):
    key = (path, pf)
    _worst[key] = tuple(max(a, b) for a, b in zip(_worst.get(key, (0.0, 0.0)), ratios))
    print(f"largest err / bound  {path:22s} {pf:12s} state {_worst[key][0]:.3f} reward {_worst[key][1]:.3f}")


class Fleet:
    """the l2f objects of one batch with the config's dt and step limit set, the params of a family written in"""

    def __init__(self, device, oracle, n, pf, dt, limit=500):
        self.device, self.n = device, n
        self.vector = v = l2f.VectorModule(n, 0)
        self.rng, self.env = v.VectorRng(), v.VectorEnvironment()
        self.params, self.state, self.next_state = v.VectorParameters(), v.VectorState(), v.VectorState()
        v.initialize_rng(device, self.rng, SEED)
        v.initialize_environment(device, self.env)
        cfg = self.env.config
        cfg.dt, cfg.episode_step_limit = dt, limit
        self.env.config = cfg
        self.cfg = self.env.config
        v.sample_initial_parameters(device, self.env, self.params, self.rng)
        v.sample_initial_state(device, self.env, self.params, self.state, self.rng)
        v.sample_initial_state(device, self.env, self.params, self.next_state, self.rng)
        sampled = oracle.sample_initial_parameters(oracle.default_config(), SEED, 0, 0, n)
        self.P, self.vrow = R.params(pf, n, SEED, self.cfg, sampled)
        self.params.set(self.P)
        self.sampled_states = oracle.sample_initial_state(self.cfg, SEED, np.zeros(n, np.uint32), 0, self.P)
        self.env.reset_statistics()

    def design(self):
        return R.mixed(self.n, SEED, self.cfg, self.P, self.sampled_states)

    def result(self, state):
        return state.numpy(), self.env.rewards(), self.env.terminated()

    def step(self, S, A, device_action, in_place):
        """one vector.step from S -> (next state, rewards, terminated)"""
        self.state.set(S)
        out = self.state if in_place else self.next_state
        if device_action:
            self.env.set_action(A)
        self.vector.step(self.device, self.env, self.params, self.state, None if device_action else A, out, self.rng)
        return self.result(out)


@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("pf", R.PARAM_FAMILIES)
def test_step_lies_inside_the_bound(device, oracle, pf, dt):
    """vector.step with NumPy actions and with the device-resident action buffer, in place and out of place; ``composed`` flies its
    factors as a vehicle bank of one one-row table per env (every step is then an episode's first)"""
    for n in BATCHES:
        f = Fleet(device, oracle, n, pf, dt, limit=500 if pf != "composed" else 1)
        if f.vrow is not None:
            bank = l2f.VehicleBank(device, np.ascontiguousarray(f.vrow[:, None, :]))
            f.env.set_vehicle_schedule(bank, np.arange(n, dtype=np.uint32))
        S, A, _, _ = f.design()
        want = R.step_bound(f.cfg, f.P, S, A, vehicle_row=f.vrow)
        assert want[2].mean() <= 0.01 or n < 100
        for device_action in (False, True):
            for in_place in (False, True):
                what = f"{pf} dt={dt} n={n} device_action={device_action} in_place={in_place}"
                _note("step", pf, held(f.step(S, A, device_action, in_place), want, what))
        assert np.array_equal(bits(f.params.numpy()), bits(f.P))


@pytest.mark.parametrize("pf", [p for p in R.PARAM_FAMILIES if p != "composed"])
def test_observe_lies_inside_the_bound(device, oracle, pf):
    for n in BATCHES:
        f = Fleet(device, oracle, n, pf, 0.01)
        obs = np.zeros((n, 26), np.float32)
        for sf in R.STATE_FAMILIES:
            S = R.states(sf, n, SEED, f.cfg, f.P, f.sampled_states)
            f.state.set(S)
            f.vector.observe(device, f.env, f.params, f.state, obs, f.rng)
            ref, bound = R.observe_bound(f.P, S)
            ratio = R.ratio(obs, ref, bound)
            assert (ratio <= 1.0).all(), (pf, sf, n, float(ratio.max()))
            _note("observe", pf, (float(ratio.max()), 0.0))


# ------------------------------------------------------------------ the schedules as physics -----
def _counts_mixed(f, S):
    """two preliminary steps that leave the envs at episode step counts 0, 1 and 2: env i with i % 3 == 1 terminates in both (it
    starts far outside the position threshold), i % 3 == 2 in the first only -> the counts before the step under test"""
    far = S.copy()
    far[:, 7:13] = 0.0
    far[:, 0:3] = 0.0
    A = np.repeat(f.P[:, 25:26], 4, axis=1)
    i = np.arange(f.n)
    for out in (i % 3 != 0, i % 3 == 1):
        s = far.copy()
        s[out, 0] = 2.0 * float(f.cfg.termination_position)
        f.state.set(s)
        f.vector.step(f.device, f.env, f.params, f.state, A, f.next_state, f.rng)
    k = f.env.episode_steps()
    assert np.array_equal(k, np.array([2, 0, 1])[i % 3]), k[:6]
    return k


def _attach(f, kind, n_rows):
    """banks of ``kind`` with 1 or 3 tables of n_rows rows, ids mixed inside a wave -> (banks kept alive, the tables by step64's keyword)"""
    M = 1 if n_rows == 1 else 3
    ids = mixed_ids(f.n, M)
    tables, banks = {}, []
    kw = rows_of(kind, M * n_rows, f.cfg, np.repeat(f.P[:1], M * n_rows, axis=0))      # (absolute pushes: sized for env 0's frame)
    for key, rows in kw.items():
        if key == "units":
            continue
        t = np.ascontiguousarray(rows.reshape(M, n_rows, -1))
        if key == "wrench_row":
            bank = l2f.WrenchBank(device=f.device, tables=t, units=kw["units"])
            f.env.set_wrench_schedule(bank, ids)
        elif key == "vehicle_row":
            bank = l2f.VehicleBank(f.device, t)
            f.env.set_vehicle_schedule(bank, ids)
        else:
            bank = l2f.WindBank(f.device, t)
            f.env.set_wind_schedule(bank, ids)
        banks.append(bank)
        tables[key] = t
    return banks, tables, ids, kw.get("units", R.RELATIVE)


@pytest.mark.parametrize("n_rows", [1, 3])
@pytest.mark.parametrize("kind", ["wrench", "wrench_absolute", "vehicle", "wind", "all"])
def test_a_schedule_is_the_physics_of_its_row(device, oracle, kind, n_rows):
    """one vector.step with banks attached against step64 given the rows as physics; row 0 and the last row both used"""
    for dt in (0.01, 0.02):
        for n in (65, 1100):
            f = Fleet(device, oracle, n, "sampled", dt, limit=n_rows)
            S, A, _, _ = f.design()
            k = _counts_mixed(f, S) if n_rows == 3 else f.env.episode_steps()
            banks, tables, ids, units = _attach(f, kind, n_rows)
            rows = {key: np.ascontiguousarray(t[ids, np.minimum(k, n_rows - 1)]) for key, t in tables.items()}
            assert (k == 0).any() and (k == n_rows - 1).any()
            want = R.step_bound(f.cfg, f.P, S, A, units=units, **rows)
            _note(f"schedule {kind}", "sampled", held(f.step(S, A, False, False), want, f"{kind} rows={n_rows} dt={dt} n={n}"))
            assert np.array_equal(bits(f.params.numpy()), bits(f.P))
            plain = R.step64(f.cfg, f.P, S, A)[0]
            assert (np.abs(plain - want[0][0]) > want[1][0]).any(1).mean() > 0.75          # the rows do move the step
            del banks


# ------------------------------------------------------------------ the fused kernel's step -----
def _constant_policies(weights, actions):
    """policies whose output layer is W2 = 0, b2 = a_p: whatever they observe, they answer a_p"""
    W = np.repeat(weights[None].astype(np.float32), len(actions), axis=0)
    W[:, 2016:2080] = 0.0
    W[:, 2080:2084] = actions
    return W


def _block_design(f):
    """S, A with A constant on every block of 64 envs, drawn from ACTION_FAMILIES block by block; the ``crossing`` blocks get rotor
    speeds within 1e-4 relative of the block's set-point instead"""
    S, A, _, _ = f.design()
    n = f.n
    blocks = (n + 63) // 64
    r = np.random.default_rng(SEED)
    a = np.empty((blocks, 4), np.float32)
    for b in range(blocks):
        fam = R.ACTION_FAMILIES[b % 4]
        first = A[min(b * 64, n - 1)]
        a[b] = {"inside": r.uniform(-1, 1, 4), "clipped": r.uniform(-3, 3, 4), "rails": np.array([-1.0, 1.0, f.P[min(b * 64, n - 1), 25], 1.0]),
                "crossing": np.clip(first, -0.9, 0.9)}[fam]
    A = np.ascontiguousarray(np.repeat(a, 64, axis=0)[:n])
    p = f.P.astype(np.float64)
    for b in range(3, blocks, 4):
        sl = slice(b * 64, min(n, b * 64 + 64))
        sp = p[sl, 22:23] + (A[sl].astype(np.float64) + 1) / 2 * (p[sl, 23:24] - p[sl, 22:23])
        S[sl, 13:17] = (sp * (1.0 + r.uniform(-1e-4, 1e-4, sp.shape))).astype(np.float32)
    ids = (np.arange(n) // 64).astype(np.uint32)
    return S, A, a, ids


def _fly_one(f, bank, ids, S, mode):
    f.state.set(S)
    f.env.reset_statistics()
    f.vector.rollout(f.device, f.env, f.params, f.state, bank, f.rng, 1, mode, False, policy_ids=ids)
    return f.result(f.state)


@pytest.mark.parametrize("schedule", [None, "vehicle", "wind"])
@pytest.mark.parametrize("pf", ["sampled", "smallest", "largest", "fast_motors"])
def test_the_fused_step_lies_inside_the_bound(device, oracle, weights, pf, schedule):
    for n in BATCHES:
        out = {}
        for mode in ("fused", "chained"):
            f = Fleet(device, oracle, n, pf, 0.01, limit=3)
            S, A, a, ids = _block_design(f)
            bank = PolicyBank(device, _constant_policies(weights, a))
            rows, units, banks = {}, R.RELATIVE, None
            if schedule:
                banks, tables, sids, units = _attach(f, schedule, 3)
                rows = {key: np.ascontiguousarray(t[sids, 0]) for key, t in tables.items()}
            out[mode] = _fly_one(f, bank, ids, S, mode)
        want = R.step_bound(f.cfg, f.P, S, A, units=units, **rows)
        _note(f"fused {schedule or 'plain'}", pf, held(out["fused"], want, f"fused {pf} {schedule} n={n}"))
        for x, y in zip(out["fused"], out["chained"]):
            assert np.array_equal(bits(x), bits(y)), (pf, schedule, n)


# ------------------------------------------------------------------ negative controls on the device -----
@pytest.mark.parametrize("path", ["step", "fused"])
@pytest.mark.parametrize("mistake", ["no_gyroscopic", "tau_exchanged", "wind_refreshed_per_stage"])
def test_the_device_is_outside_an_altered_reference(device, oracle, weights, mistake, path):
    n = 1100
    f = Fleet(device, oracle, n, "fast_motors", 0.01, limit=3)
    rows, banks = {}, None
    if mistake == "wind_refreshed_per_stage":
        banks, tables, sids, _ = _attach(f, "wind", 3)
        rows = {key: np.ascontiguousarray(t[sids, 0]) for key, t in tables.items()}
    if path == "step":
        S, A, _, _ = f.design()
        got = f.step(S, A, False, False)
    else:
        S, A, a, ids = _block_design(f)
        got = _fly_one(f, PolicyBank(device, _constant_policies(weights, a)), ids, S, "fused")
    want = R.step_bound(f.cfg, f.P, S, A, **rows)
    held(got, want, f"{path} {mistake}: the unaltered reference")
    ns, _, _ = R.altered(mistake)(f.cfg, f.P, S, A, **rows)
    outside = (R.ratio(got[0], ns, want[1][0]) > 1.0).any(1)
    print(f"{path} against {mistake}: outside on {outside.mean():.3f} of the envs")
    assert outside.mean() > 0.5
