"""Teacher rollouts: a TeacherBank flying its envs (rq_rollout_teachers, fused and chained) and the bank's one-step evaluation
(rq_teacher_bank_evaluate).  Bars: transitions, statistics and recordings bit for bit against vector.step, the chained mode, the
relabel kernels and the oracle's env; the actions within tests/teacher_reference.py's float64 bound."""
import numpy as np
import pytest

import teacher_reference as R
from gpu_common import World
from rollout_common import assert_same, assert_same_recording, bits, snapshot

pytestmark = pytest.mark.gpu


def _weights(rng, n_teachers, in_dim, widths, scale=1.0):
    from raptor_amd.teachers import layers_parameter_count
    W = np.empty((n_teachers, layers_parameter_count(in_dim, widths)), np.float32)
    for t in range(n_teachers):
        parts, prev = [], in_dim
        for h in list(widths) + [4]:
            parts += [rng.standard_normal(h * prev) * scale / np.sqrt(prev), rng.standard_normal(h) * 0.1]
            prev = h
        W[t] = np.concatenate(parts).astype(np.float32)
    return W


def _bank(device, W, in_dim, widths, act="relu", out_act="tanh", precision="fp32"):
    from raptor_amd.teachers import TeacherBank
    return TeacherBank.from_layers(device, W, in_dim, widths, act, out_act, precision)


def _fly(device, oracle, n, bank, ids, mode, steps, autoreset, seed=7, record=True, chunks=None, **cfg):
    w = World(device, oracle, n, seed=seed, **cfg)
    tr = w.vector.Trajectory(w.env, sum(steps) if isinstance(steps, (list, tuple)) else steps) if record else None
    for s in (steps if isinstance(steps, (list, tuple)) else [steps]):
        w.vector.rollout(device, w.env, w.params, w.state, bank, w.rng, s, mode, autoreset, trajectory=tr, teacher_ids=ids)
    return w, tr


# ------------------------------------------------------------------------------ 1. constant-action teachers -
@pytest.mark.parametrize("mode", ["fused", "chained"])
def test_constant_action_teachers_fly_like_vector_step(device, oracle, mode):
    """Teachers with zero weights and output bias c_k act c_k exactly: the rollout equals observe -> vector.step(c[ids]) -> assign,
    step for step (a window without episode ends), and, with auto-reset and short episodes, the oracle's env sequence."""
    from raptor_amd.teachers import TeacherBank, parameter_count
    n, T, K = 100, 12, 5
    rng = np.random.default_rng(1)
    c = rng.uniform(-0.3, 0.3, (K, 4)).astype(np.float32)
    W = np.zeros((K, parameter_count(22, 16, 16)), np.float32)
    W[:, -4:] = c
    bank = TeacherBank(device, W, 22, 16, 16, "relu", "identity")
    ids = (np.arange(n) % K).astype(np.uint32)
    w, tr = _fly(device, oracle, n, bank, ids, mode, T, False, seed=3)
    rec = tr.numpy()
    u = World(device, oracle, n, seed=3)
    obs = np.zeros((n, u.env.OBSERVATION_DIM), np.float32)
    for t in range(T):
        u.vector.observe(device, u.env, u.params, u.state, obs, u.rng)
        assert np.array_equal(bits(obs[:, :22]), bits(rec["obs"][t])), t
        assert np.array_equal(rec["act"][t], c[ids])
        u.vector.step(device, u.env, u.params, u.state, c[ids], u.next_state, u.rng)
        u.state.assign(u.next_state)
        assert np.array_equal(bits(u.env.rewards()), bits(rec["rew"][t])), t
        assert np.array_equal(u.env.done_codes(), rec["done"][t]), t
    assert (rec["done"] == 0).all()
    assert_same(snapshot(w), snapshot(u), what=mode)
    # the oracle's env: observe / step / stats_update / sample_initial_state with auto-reset and 4-step episodes
    T2 = 11
    w2, tr2 = _fly(device, oracle, n, bank, ids, mode, T2, True, seed=5, episode_step_limit=4)
    rec2 = tr2.numpy()
    v = World(device, oracle, n, seed=5, episode_step_limit=4)
    O, S, st, P = oracle, v.S.copy(), v.st, v.P
    S = v.state.numpy().copy()                     # start from the GPU's initial state (sin / cos ulps)
    reset = np.zeros(n, bool)      # re-sampled envs start from the oracle's sin / cos: within INIT_TOL-grown bars, not bit for bit
    for t in range(T2):
        o = O.observe(v.cfg, v.seed, t, 0, P, S)[:, :22].astype(np.float32)
        assert np.array_equal(bits(o[~reset]), bits(rec2["obs"][t][~reset])), t
        assert np.abs(o[reset] - rec2["obs"][t][reset]).max(initial=0.0) < 1e-4, t
        S, r, term = O.step(v.cfg, P, S, c[ids])
        O.stats_update(v.cfg, r, term, st)
        ended = term.astype(bool) | (st.steps == 0)
        assert np.array_equal(bits(r[~reset]), bits(rec2["rew"][t][~reset])), t
        assert np.abs(r[reset] - rec2["rew"][t][reset]).max(initial=0.0) < 1e-4, t
        codes = np.where(term != 0, 1, np.where(ended, 2, 0)).astype(np.uint8)
        assert np.array_equal(codes, rec2["done"][t]), t
        if ended.any():
            fresh = O.sample_initial_state(v.cfg, v.seed, st.episode, 0, P)      # increments every counter: undo the others
            st.episode[~ended] -= 1
            S[ended] = fresh[ended]
            reset |= ended
    assert (rec2["done"] == 2).any()
    assert np.array_equal(st.episode, w2.env.episode_index())
    assert np.array_equal(st.fin_counts, w2.env.finished_counts())
    assert np.abs(S - w2.state.numpy()).max() < 1e-4


# ------------------------------------------------------------------------------ 2. fused equals chained -
_ARCHS = [((16, 16), "relu", "identity"), ((32, 64), "tanh", "tanh"), ((64, 64), "relu", "tanh")]


def _ids(kind, n, K, rng):
    if kind == "balanced":
        from raptor_amd.teachers import balanced_teacher_assignment
        return balanced_teacher_assignment(n, K)
    if kind == "single":
        return np.full(n, K - 1, np.uint32)
    ids = rng.integers(0, K - 2, n).astype(np.uint32)        # random, non-contiguous; teacher K - 1 flies one env, K - 2 none
    ids[n // 2] = K - 1
    return ids


@pytest.mark.parametrize("arch", _ARCHS)
@pytest.mark.parametrize("n,kind", [(1, "single"), (15, "random"), (16, "balanced"), (17, "random"), (200, "random"),
                                    (4097, "balanced")])
def test_fused_equals_chained(device, oracle, arch, n, kind):
    widths, act, out_act = arch
    rng = np.random.default_rng(n * 7 + widths[0])
    K = 9
    W = _weights(rng, K, 22, widths)
    bank = _bank(device, W, 22, list(widths), act, out_act)
    ids = _ids(kind, n, K, rng)
    for autoreset, noise in ((True, False), (False, True)):
        cfg = dict(episode_step_limit=23)
        if noise:
            cfg.update(noise_position=0.01, noise_linear_velocity=0.02)
        wf, tf = _fly(device, oracle, n, bank, ids, "fused", [50, 30], autoreset, seed=n, **cfg)
        wc, tc = _fly(device, oracle, n, bank, ids, "chained", 80, autoreset, seed=n, **cfg)
        assert_same(snapshot(wf), snapshot(wc), what=f"n={n} {kind} autoreset={autoreset}")
        assert_same_recording(tf.numpy(), tc.numpy())
        assert (tf.numpy()["done"] != 0).any()                 # episode ends were crossed
    # a freezing rollout, then an auto-reset one (thaw)
    wf, tf = _fly(device, oracle, n, bank, ids, "fused", 30, False, seed=n + 1, episode_step_limit=7)
    wc, tc = _fly(device, oracle, n, bank, ids, "chained", 30, False, seed=n + 1, episode_step_limit=7)
    assert_same(snapshot(wf), snapshot(wc), what="freezing")
    assert_same_recording(tf.numpy(), tc.numpy())
    assert wf.env.frozen().all()
    for w, mode in ((wf, "fused"), (wc, "chained")):
        w.vector.rollout(device, w.env, w.params, w.state, bank, w.rng, 5, mode, True, teacher_ids=ids)
    assert_same(snapshot(wf), snapshot(wc), what="thaw")
    assert not wf.env.frozen().any()


# ------------------------------------------------------------------------------ 3. + 4. relabel and the oracle -
@pytest.mark.parametrize("kind", ["fp32", "bf16", "f16x2", "stack"])
def test_recorded_actions_equal_relabelling_and_the_oracle(device, oracle, kind):
    rng = np.random.default_rng(11)
    n, T, K = 300, 40, 13
    widths = [32, 48, 32] if kind == "stack" else [64, 32]
    W = _weights(rng, K, 22 if kind != "fp32" else 19, widths)
    in_dim = 22 if kind != "fp32" else 19
    bank = _bank(device, W, in_dim, widths, "tanh", "identity", "fp32" if kind == "stack" else kind)
    ids = rng.integers(0, K, n).astype(np.uint32)
    mode = "fused" if kind == "fp32" else "chained"
    w, tr = _fly(device, oracle, n, bank, ids, mode, T, False, seed=21, episode_step_limit=1000)
    rec = tr.numpy()
    live = rec["done"] != 4
    lab = tr.relabel_teachers(bank, ids)
    assert np.array_equal(bits(lab[live]), bits(rec["act"][live]))
    ref, e = R.relabel_bound(W, in_dim, widths, "tanh", "identity", rec["obs"], ids, "fp32" if kind == "stack" else kind)
    R.assert_within(np.where(live[..., None], rec["act"], ref), ref, e, kind)
    # the oracle's env replaying the recorded actions from the same start (noise off): observations, rewards, done codes
    v = World(device, oracle, n, seed=21, episode_step_limit=1000)
    S = v.state.numpy().copy()
    alive = np.ones(n, bool)
    for t in range(T):
        o = oracle.observe(v.cfg, v.seed, t, 0, v.P, S)
        assert np.array_equal(bits(o[alive, :22].astype(np.float32)), bits(rec["obs"][t][alive])), t
        S2, r, term = oracle.step(v.cfg, v.P, S, rec["act"][t])
        assert np.array_equal(bits(r[alive].astype(np.float32)), bits(rec["rew"][t][alive])), t
        assert np.array_equal(np.where(term[alive] != 0, 1, 0), rec["done"][t][alive]), t
        S = np.where(alive[:, None], S2, S)
        alive &= term == 0


# ------------------------------------------------------------------------------ 5. row independence -
def test_a_neighbours_teacher_leaves_a_row_alone(device, oracle):
    rng = np.random.default_rng(5)
    n, K = 40, 4
    W = _weights(rng, K, 22, [32, 32])
    W_nan = W.copy()
    W_nan[2, 5] = np.nan
    a = _bank(device, W, 22, [32, 32])
    b = _bank(device, W_nan, 22, [32, 32])
    ids = (np.arange(n) % 3).astype(np.uint32)
    ids2 = ids.copy()
    ids2[ids2 != 0] = 2                       # every other env flown by the NaN teacher
    for mode in ("fused", "chained"):
        wa, ta = _fly(device, oracle, n, a, ids, mode, 25, True, seed=9, episode_step_limit=10)
        wb, tb = _fly(device, oracle, n, b, ids2, mode, 25, True, seed=9, episode_step_limit=10)
        keep = ids == 0
        ra, rb = ta.numpy(), tb.numpy()
        for k in ("obs", "act", "rew", "done"):
            assert np.array_equal(bits(ra[k][:, keep]), bits(rb[k][:, keep])), (mode, k)
        assert np.isnan(rb["act"][:, ~keep]).all()
        assert np.array_equal(bits(wa.state.numpy()[keep]), bits(wb.state.numpy()[keep]))


# ------------------------------------------------------------------------------ 6. evaluate -
@pytest.mark.parametrize("kind", ["fp32", "bf16", "stack"])
def test_evaluate_equals_a_one_step_relabel(device, oracle, kind):
    rng = np.random.default_rng(6)
    n, K = 70, 6
    widths = [64, 64] if kind != "stack" else [80]
    W = _weights(rng, K, 22, widths)
    bank = _bank(device, W, 22, widths, "relu", "tanh", "bf16" if kind == "bf16" else "fp32")
    ids = rng.integers(0, K, n).astype(np.uint32)
    w = World(device, oracle, n, seed=13)
    tr = w.vector.Trajectory(w.env, 1)
    w.vector.rollout(device, w.env, w.params, w.state, w.policy, w.rng, 1, "chained", False, trajectory=tr)
    obs = tr.numpy()["obs"][0]
    lab = tr.relabel_teachers(bank, ids)[0]
    wide = np.concatenate([obs, rng.standard_normal((n, 9)).astype(np.float32)], axis=1)      # obs_stride 31
    assert np.array_equal(bits(bank.evaluate(wide, ids)), bits(lab))
    assert np.array_equal(bits(bank.evaluate(obs[3:4], ids[3:4])), bits(lab[3:4]))      # batch 1
    assert np.array_equal(bits(bank.evaluate(obs[:37], ids[:37])), bits(lab[:37]))     # ragged
    # the env's device buffers: its observation in, host actions out / its action buffer out
    full = np.zeros((n, w.env.OBSERVATION_DIM), np.float32)
    w.vector.observe(device, w.env, w.params, w.state, None, w.rng)
    full = w.env.observation()
    lab2 = bank.evaluate(full[:, :22], ids)
    assert np.array_equal(bits(bank.evaluate(None, ids, env=w.env)), bits(lab2))
    assert bank.evaluate(None, ids, env=w.env, to_device=True) is None
    assert np.array_equal(bits(w.env.action()), bits(lab2))


# ------------------------------------------------------------------------------ 7. refusals -
def test_refusals_leave_everything_untouched(device, oracle):
    rng = np.random.default_rng(8)
    n, K = 20, 3
    W = _weights(rng, K, 22, [16, 16])
    bank = _bank(device, W, 22, [16, 16])
    ids = np.zeros(n, np.uint32)
    w = World(device, oracle, n, seed=4)
    other = World(device, oracle, n, seed=4)
    tr = w.vector.Trajectory(w.env, 10)
    w.vector.rollout(device, w.env, w.params, w.state, bank, w.rng, 3, "fused", False, trajectory=tr, teacher_ids=ids)
    before = snapshot(w)
    rec = tr.numpy()
    bf = _bank(device, W, 22, [16, 16], precision="bf16")
    stack = _bank(device, _weights(rng, K, 22, [16, 16, 16]), 22, [16, 16, 16])
    from raptor_amd import _lib
    cases = [
        dict(policy=bank, ids=np.full(n, K, np.uint32), match="teacher id out of range"),
        dict(policy=bank, ids=ids, traj=other.vector.Trajectory(other.env, 10), match="another env"),
        dict(policy=bank, ids=ids, steps=8, match="too small"),
        dict(policy=bf, ids=ids, match="chained"),
        dict(policy=stack, ids=ids, match="chained"),
    ]
    for cse in cases:
        with pytest.raises(Exception, match=cse["match"]):
            w.vector.rollout(device, w.env, w.params, w.state, cse["policy"], w.rng, cse.get("steps", 2), "fused", False,
                             trajectory=cse.get("traj", tr), teacher_ids=cse["ids"])
    with pytest.raises(Exception, match="unknown mode"):
        _lib.call("rq_rollout_teachers", device._h, w.env._h, w.params._h, w.state._h, bank._h, ids.ctypes.data, w.rng._h, 2, 7, 0, None)
    with pytest.raises(Exception, match="unknown flags"):
        _lib.call("rq_rollout_teachers", device._h, w.env._h, w.params._h, w.state._h, bank._h, ids.ctypes.data, w.rng._h, 2, 0, 8, None)
    import raptor_amd.l2f as l2f
    dev2 = l2f.Device(0)
    bank2 = _bank(dev2, W, 22, [16, 16])
    with pytest.raises(Exception, match="another device"):
        w.vector.rollout(device, w.env, w.params, w.state, bank2, w.rng, 2, "fused", False, teacher_ids=ids)
    with pytest.raises(ValueError):
        w.vector.rollout(device, w.env, w.params, w.state, bank, w.rng, 2, "fused", False)              # ids required
    with pytest.raises(ValueError):
        w.vector.rollout(device, w.env, w.params, w.state, w.policy, w.rng, 2, "fused", False, teacher_ids=ids)
    assert_same(before, snapshot(w), what="after refusals")
    assert len(tr) == 3 and np.array_equal(bits(tr.numpy()["obs"]), bits(rec["obs"]))
    # the rng epoch did not move: the next rollout equals one on a world that never saw the refusals
    w.vector.rollout(device, w.env, w.params, w.state, bank, w.rng, 4, "fused", False, trajectory=tr, teacher_ids=ids)
    u = World(device, oracle, n, seed=4)
    ut = u.vector.Trajectory(u.env, 10)
    u.vector.rollout(device, u.env, u.params, u.state, bank, u.rng, 3, "fused", False, trajectory=ut, teacher_ids=ids)
    u.vector.rollout(device, u.env, u.params, u.state, bank, u.rng, 4, "fused", False, trajectory=ut, teacher_ids=ids)
    assert_same(snapshot(w), snapshot(u), what="epoch")


# ------------------------------------------------------------------------------ 8. resident executor -
def test_a_teacher_rollout_between_resident_loop_iterations(device, oracle):
    rng = np.random.default_rng(12)
    n, K = 8, 2
    bank = _bank(device, _weights(rng, K, 22, [16, 32]), 22, [16, 32])
    ids = (np.arange(n) % K).astype(np.uint32)

    def run(resident):
        device.set_resident(resident)
        w = World(device, oracle, n, seed=17)
        obs = np.zeros((n, w.env.OBSERVATION_DIM), np.float32)
        w.policy.reset()
        O = []
        before = device.resident()

        def loop(iters):
            for _ in range(iters):
                w.vector.observe(device, w.env, w.params, w.state, obs, w.rng)
                a = w.policy.evaluate_step(obs[:, :22])
                w.vector.step(device, w.env, w.params, w.state, a, w.next_state, w.rng)
                w.state.assign(w.next_state)
                O.append(obs.copy())
        loop(30)
        w.vector.rollout(device, w.env, w.params, w.state, bank, w.rng, 20, "fused", True, teacher_ids=ids)
        O.append(w.state.numpy().copy())
        loop(30)
        after = device.resident()
        device.set_resident(True)
        return np.array(O[:-31] + O[-30:]), O[30], w.state.numpy().copy(), {k: after[k] - before[k] for k in ("starts", "commands")}

    on, off = run(True), run(False)
    for x, y in zip(on[:3], off[:3]):
        assert np.array_equal(bits(x), bits(y))
    assert on[3]["commands"] > 0 and on[3]["starts"] >= 2          # the executor served the loop, was retired, and came back
    assert off[3]["commands"] == 0
