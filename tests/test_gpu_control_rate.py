"""The native interval R (rq_policy_set_native_interval): flown at R times the rate it was trained at, the policy's hidden state
moves on only at an env's native steps - episode step count (rollouts) or call index (evaluate_step) a multiple of R - and every
other step acts from the last committed state.  The yardstick is the rule rebuilt from the R = 1 primitives (get / set the hidden
state around single steps), bit for bit; fused, chained and one-step launches must agree with it and with one another.

Throughout: episode_step_limit = 9 and termination_position = 0.6 (episodes end at a phase that is no multiple of R), 23 steps and
then 7 more in a second launch (a launch ends mid-interval), domain randomisation on."""
import ctypes as C

import numpy as np
import pytest

import raptor_amd.l2f as l2f
from raptor_amd import _lib
from raptor_amd._lib import RaptorQuadError
from raptor_amd.foundation_policy import Raptor
from gpu_common import World
from rollout_common import assert_same, assert_same_recording, roll, world_snapshot

pytestmark = pytest.mark.gpu

LIMIT = 9
CHUNKS = (23, 7)
KW = dict(episode_step_limit=LIMIT, termination_position=0.6)


def _world(device, oracle, n, interval=None, precision="fp32", ragged=True, **over):
    """ragged: a third of the envs starts outside termination_position and another third crosses it by hand - their episodes
    are one step long, so the envs of a wave fly out of phase with one another from the second step on."""
    w = World(device, oracle, n, seed=5, **{**KW, **over})
    assert w.env.config.domain_randomization
    w.policy.set_precision(precision)
    if interval is not None:
        w.policy._handle(device)                  # the C object exists: the setter goes through the entry point
        w.policy.native_interval = interval
    if ragged:
        s = w.state.numpy()
        s[::3, 0] = 0.7
        w.state.set(s)
    return w


# ------------------------------------------------------------------ 1 -----
@pytest.mark.parametrize("mode", ["fused", "chained"])
def test_interval_one_is_what_it_was(device, oracle, mode):
    n = 65
    a, b = _world(device, oracle, n, interval=1), _world(device, oracle, n)
    assert a.policy.native_interval == 1 and b.policy.native_interval == 1
    ta, tb = (w.vector.Trajectory(w.env, sum(CHUNKS)) for w in (a, b))
    for chunk in CHUNKS:
        roll(a, chunk, mode, trajectory=ta)
        roll(b, chunk, mode, trajectory=tb)
    assert_same(world_snapshot(a), world_snapshot(b))
    assert_same_recording(ta.numpy(), tb.numpy(), frozen_too=True)
    for chunk in CHUNKS:                          # and without a recording (the chained mode's other step: observe folded in)
        roll(a, chunk, mode)
        roll(b, chunk, mode)
    assert_same(world_snapshot(a), world_snapshot(b))
    assert a.env.finished_counts().min() >= 1


# ------------------------------------------------------------------ 2 -----
@pytest.mark.parametrize("precision", ["fp32", "bf16", "f16x2"])
@pytest.mark.parametrize("batch", [5, 17, 1100])          # 17: above the resident policy's batch; 1100: above the mailbox's
@pytest.mark.parametrize("where", ["host", "device"])
def test_evaluate_step_rule_from_get_and_set_hidden(device, oracle, batch, precision, where):
    """Policy A has R = 4.  Policy B has R = 1 and is driven by hand: get_hidden, evaluate_step, and the hidden state put back when
    the call's index is no multiple of 4.  9 calls, reset, 3 more: actions and hidden states bit for bit."""
    g = np.random.default_rng(batch)
    a, b = Raptor(device, precision=precision, native_interval=4), Raptor(device, precision=precision)
    w = World(device, oracle, batch, seed=7) if where == "device" else None

    def step(policy, obs):
        if w is None:
            return policy.evaluate_step(obs)
        policy.evaluate_step_device(w.env)         # reads the env's observation buffer, writes its action buffer
        return w.env.action()

    for calls in (9, 3):
        a.reset()
        b.reset()
        for k in range(calls):
            if w is None:
                obs = g.uniform(-1.0, 1.0, (batch, 22)).astype(np.float32)
            else:                                   # the env's buffer filled by observe from a state that differs call by call
                s = w.state.numpy()
                s[:, :3] = g.uniform(-0.5, 0.5, (batch, 3)).astype(np.float32)
                w.state.set(s)
                w.vector.observe(device, w.env, w.params, w.state, None, w.rng)
                obs = None
            before = b.hidden_state(batch)
            act_a, act_b = step(a, obs), step(b, obs)
            if k % 4 != 0:
                assert not np.array_equal(b.hidden_state(batch), before)       # the step moved it: putting it back means something
                b.set_hidden_state(before)
            assert np.array_equal(act_a.view(np.uint32), act_b.view(np.uint32)), (calls, k)
            assert np.array_equal(a.hidden_state(batch).view(np.uint32), b.hidden_state(batch).view(np.uint32)), (calls, k)
    assert a.native_interval == 4


@pytest.mark.parametrize("interval", [2, 4])
@pytest.mark.parametrize("n", [1, 65, 4097])
def test_rollout_rule_from_one_step_rollouts(device, oracle, n, interval):
    """World A: R fused.  World B: R = 1, one-step auto-reset rollouts; the test puts back the hidden rows of exactly the envs whose
    step was not native (episode step count before it no multiple of R) and whose episode did not end in it (those were reset)."""
    a, b = _world(device, oracle, n, interval=interval), _world(device, oracle, n)
    tentative_seen = ended_mid_interval = 0
    for chunk in CHUNKS:
        roll(a, chunk, "fused")
        for _ in range(chunk):
            k = b.env.episode_steps()
            before = b.policy.hidden_state(n)
            roll(b, 1, "fused")
            ended = b.env.done_codes() != 0
            keep = (k % interval != 0) & ~ended
            ended_mid_interval += int((ended & ((k + 1) % interval != 0)).sum())
            tentative_seen += int(keep.sum())
            if keep.any():
                h = b.policy.hidden_state(n)
                h[keep] = before[keep]
                b.policy.set_hidden_state(h)
    assert tentative_seen > 0 and ended_mid_interval > 0
    assert_same(world_snapshot(a), world_snapshot(b))
    assert a.env.finished_counts().min() >= 1


# ------------------------------------------------------------------ 3 -----
@pytest.mark.parametrize("precision,n,noise", [(p, n, 0.0) for p in ("fp32", "bf16", "f16x2") for n in (1, 65, 4097, 70001)] +
                         [("fp32", 65, 0.01)])
def test_fused_equals_chained_equals_one_step_launches(device, oracle, precision, n, noise):
    """70 001 envs: the fp32 kernel built for two waves per SIMD."""
    a, b, c = (_world(device, oracle, n, interval=4, precision=precision, noise_position=noise) for _ in range(3))
    ta, tb, tc = (w.vector.Trajectory(w.env, sum(CHUNKS)) for w in (a, b, c))
    for chunk in CHUNKS:
        roll(a, chunk, "fused", trajectory=ta)
        roll(b, chunk, "chained", trajectory=tb)
        for _ in range(chunk):
            roll(c, 1, "fused", trajectory=tc)
    sa = world_snapshot(a)
    assert_same(sa, world_snapshot(b))
    assert_same(sa, world_snapshot(c))
    assert_same_recording(ta.numpy(), tb.numpy(), frozen_too=True)
    assert_same_recording(ta.numpy(), tc.numpy(), frozen_too=True)
    for chunk in CHUNKS:                          # unrecorded: the other fused instantiation, the chained mode's folded observe
        roll(a, chunk, "fused")
        roll(b, chunk, "chained")
    assert_same(world_snapshot(a), world_snapshot(b))
    assert sa["fin_counts"].min() >= 1


# ------------------------------------------------------------------ 4 -----
def test_without_autoreset_envs_freeze_and_thaw_at_phase_zero(device, oracle):
    n = 65
    a, b, c = (_world(device, oracle, n, interval=4) for _ in range(3))
    for chunk in (3, 2):                          # nobody but the displaced third has ended yet: a launch ends mid-interval
        roll(a, chunk, "fused", False)
        roll(b, chunk, "chained", False)
        for _ in range(chunk):
            roll(c, 1, "fused", False)
    sa = world_snapshot(a)
    assert_same(sa, world_snapshot(b))
    assert_same(sa, world_snapshot(c))
    frozen = sa["frozen"] != 0
    assert frozen[::3].all() and not frozen.all() and (sa["steps"][~frozen] == 5).all()
    # frozen envs add nothing and keep their hidden state: two more steps move the others only
    roll(a, 2, "fused", False)
    roll(b, 2, "chained", False)
    s2 = world_snapshot(a)
    assert_same(s2, world_snapshot(b))
    assert np.array_equal(s2["hidden"][frozen], sa["hidden"][frozen]) and np.array_equal(s2["state"][frozen], sa["state"][frozen])
    assert np.array_equal(s2["fin_counts"][frozen], sa["fin_counts"][frozen]) and (s2["done"][frozen] == 4).all()
    # a later auto-reset rollout thaws the frozen ones at k = 0 while the others stand at k = 7: one step commits the thawed
    # envs' state (native) and leaves the others' alone (7 % 4 != 0)
    h_before = a.policy.hidden_state(n)
    roll(a, 1, "fused", True)
    roll(b, 1, "chained", True)
    s3 = world_snapshot(a)
    assert_same(s3, world_snapshot(b))
    assert (s3["steps"][frozen] == 1).all() and (s3["steps"][~frozen] == 8).all()
    assert np.array_equal(s3["hidden"][~frozen], h_before[~frozen])
    assert (s3["hidden"][frozen] != h_before[frozen]).any(axis=1).all()
    for chunk in CHUNKS:
        roll(a, chunk, "fused", True)
        roll(b, chunk, "chained", True)
    assert_same(world_snapshot(a), world_snapshot(b))


# ------------------------------------------------------------------ 5 -----
@pytest.mark.parametrize("precision", ["fp32", "bf16", "f16x2"])
def test_with_tracking(device, oracle, precision):
    n = 65
    g = np.random.default_rng(1)
    ref = l2f.Reference(device, (0.1 * g.uniform(-1.0, 1.0, (LIMIT + 2, 6))).astype(np.float32))
    a, b, c = (_world(device, oracle, n, interval=4, precision=precision) for _ in range(3))
    ta, tb = (w.vector.Trajectory(w.env, sum(CHUNKS)) for w in (a, b))
    for chunk in CHUNKS:
        roll(a, chunk, "fused", reference=ref, trajectory=ta)
        roll(b, chunk, "chained", reference=ref, trajectory=tb)
        roll(c, chunk, "fused")
    sa = world_snapshot(a)
    assert_same(sa, world_snapshot(b))
    assert_same_recording(ta.numpy(), tb.numpy(), frozen_too=True)
    for chunk in CHUNKS:
        roll(a, chunk, "fused", reference=ref)
        roll(b, chunk, "chained", reference=ref)
    s2 = world_snapshot(a)
    assert_same(s2, world_snapshot(b))
    assert np.array_equal(s2["track_steps"], np.full(n, 2 * sum(CHUNKS), np.uint32)) and (s2["track_sq"] > 0).all()
    assert not np.array_equal(sa["state"], c.state.numpy())              # the setpoint moved what the policy did


# ------------------------------------------------------------------ 6 -----
def test_chained_graph_replay_is_keyed_by_the_interval(device, oracle):
    """From 25 steps on the chained mode replays a cached hipGraph whose actor nodes are the interval's kernels with the interval
    in their arguments: R = 4, then 1, then 4 again on the same objects, each segment against a fresh world run the same way."""
    n, steps = 1, 27
    a = _world(device, oracle, n, ragged=False)
    a.policy._handle(device)
    for seg, interval in enumerate((4, 1, 4)):
        a.policy.native_interval = interval
        roll(a, steps, "chained")
        f = _world(device, oracle, n, ragged=False)
        f.policy._handle(device)
        for earlier in (4, 1, 4)[:seg + 1]:
            f.policy.native_interval = earlier
            roll(f, steps, "fused")
        assert_same(world_snapshot(a), world_snapshot(f))
    b = _world(device, oracle, n, ragged=False)          # and the interval matters: R = 1 throughout flies another last episode
    roll(b, 3 * steps, "fused")
    assert not np.array_equal(b.env.finished_returns(), a.env.finished_returns())


# ------------------------------------------------------------------ 7 -----
def _readme_loop(device, n, iters, interval):
    vector = l2f.vector(n)
    rng, env = vector.VectorRng(), vector.VectorEnvironment()
    params, state, next_state = vector.VectorParameters(), vector.VectorState(), vector.VectorState()
    vector.initialize_rng(device, rng, 0)
    vector.initialize_environment(device, env)
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    policy = Raptor(device, native_interval=interval)
    policy.reset()
    obs = np.zeros((n, env.OBSERVATION_DIM), np.float32)
    O, A, H = [], [], []
    for _ in range(iters):
        vector.observe(device, env, params, state, obs, rng)
        action = policy.evaluate_step(obs[:, :22])
        vector.step(device, env, params, state, action, next_state, rng)
        state.assign(next_state)
        O.append(obs.copy())
        A.append(action.copy())
        H.append(policy.hidden_state(n))
    return np.array(O), np.array(A), np.array(H), state.numpy().copy(), env.rewards().copy()


def test_small_batch_loop_stays_plain_launches():
    first, second = l2f.Device(0), l2f.Device(0)
    second.set_resident(False)
    second.set_speculation(False)
    starts = first.resident()["starts"]
    got = _readme_loop(first, 8, 60, 4)
    want = _readme_loop(second, 8, 60, 4)
    for x, y in zip(got, want):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert first.resident()["enabled"] and first.resident()["starts"] == starts == 0 and first.resident()["commands"] == 0
    # the rule held inside the loop: the hidden state after iteration k is that after iteration k - 1 unless k % 4 == 0
    H = got[2]
    for k in range(1, 60):
        assert np.array_equal(H[k], H[k - 1]) == (k % 4 != 0), k


# ------------------------------------------------------------------ 8 -----
def test_refusals_name_the_interval_and_change_nothing(device, oracle):
    from raptor_amd.teachers import TeacherBank, parameter_count
    n, T = 65, 12
    a = _world(device, oracle, n, interval=4)
    tr = a.vector.Trajectory(a.env, T + 5)
    roll(a, T, "fused", trajectory=tr)
    pol = a.policy
    obs = np.random.default_rng(0).uniform(-1, 1, (n, 22)).astype(np.float32)

    def policy_state():
        """weights, hidden state, and the call counter read off what the next evaluate_step does (on a copy of the state)."""
        h = pol.hidden_state(n)
        pol.evaluate_step(obs)
        moved = not np.array_equal(pol.hidden_state(n), h)
        pol.set_hidden_state(h)
        return np.array(pol.weights), h, moved

    a.policy.reset()
    pol.evaluate_step(obs)                        # call 0 of the counter: native; the next call (index 1) is not
    w0, h0, moved0 = policy_state()               # (takes call 1; call 2 is not native either)
    assert not moved0
    before, epoch = world_snapshot(a), a.rng.epoch

    def unchanged():
        w1, h1, moved1 = policy_state()           # calls 2, 3 of the counter at the two checks that see "not native" ...
        assert np.array_equal(w1, w0) and np.array_equal(h1, h0)
        assert_same(before, world_snapshot(a))
        assert a.rng.epoch == epoch and len(tr) == T and pol.native_interval == 4
        return moved1

    def refused(call, *args, **kw):
        with pytest.raises((RaptorQuadError, ValueError), match="interval"):
            call(*args, **kw)

    # the interval itself
    for bad in (0, 65):
        refused(_lib.call, "rq_policy_set_native_interval", pol._handle(device), bad)
        with pytest.raises(ValueError, match="interval"):
            pol.native_interval = bad
        with pytest.raises(ValueError, match="interval"):
            Raptor(device, native_interval=bad)
    # ... a SampleAndSquash stage set second
    refused(pol.set_sample_and_squash, "mean")
    refused(pol.set_sample_and_squash, "sample", seed=3)
    refused(pol.set_squash, True)
    assert not unchanged()                        # call 2: the refusals did not rewind the counter
    # ... what is defined at the native rate only
    seq = np.zeros((3, n, 22), np.float32)
    refused(pol.evaluate_sequence, seq)
    refused(pol.selftest, seq, np.zeros((3, n, 4), np.float32))
    refused(tr.relabel, pol)
    refused(tr.relabel, pol, overwrite=True)
    ld = a.env._ld()
    host_act, host_grad = np.zeros((T, 4, ld), np.float32), np.zeros(2084, np.float32)
    refused(_lib.call, "rq_trajectory_policy_forward", tr._h, pol._handle(device), 1, _lib.fptr(host_act), ld, 0)
    refused(_lib.call, "rq_trajectory_policy_backward", tr._h, pol._handle(device), _lib.fptr(host_act), ld, _lib.fptr(host_grad), None, 0)
    loss = np.zeros(2, np.float32)
    refused(_lib.call, "rq_trajectory_policy_loss_grad", tr._h, pol._handle(device), _lib.fptr(host_act), ld, 1, _lib.fptr(loss),
            _lib.fptr(host_grad), 0)
    opt = C.c_void_p()
    _lib.call("rq_optimizer_create", pol._handle(device), C.byref(_lib.AdamConfig(1e-3, 0.9, 0.999, 1e-8, 0.0)), C.byref(opt))
    refused(_lib.call, "rq_trajectory_distill", tr._h, pol._handle(device), opt, _lib.fptr(host_act), ld, 1, 2, _lib.fptr(loss), 0)
    _lib.call("rq_optimizer_destroy", opt)
    recorded = tr.numpy()
    assert not unchanged()                        # call 3
    assert unchanged()                            # call 4: native - the counter went on counting through every refusal
    # the interval set second beside a stage
    other = Raptor(device)
    other.set_sample_and_squash("mean")
    other._handle(device)
    refused(setattr, other, "native_interval", 4)
    assert other.native_interval == 1
    # teachers carry no state: relabelling an R = 4 recording with them works as ever, and the recording is what it was
    in_dim, h1, h2 = 22, 16, 16
    W = (0.1 * np.random.default_rng(2).standard_normal((3, parameter_count(in_dim, h1, h2)))).astype(np.float32)
    bank = TeacherBank(device, W, in_dim, h1, h2, "relu", "identity")
    labels = tr.relabel_teachers(bank, np.arange(n, dtype=np.uint32) % 3)
    assert labels.shape == (T, n, 4) and np.isfinite(labels).all()
    for k, v in tr.numpy().items():
        assert np.array_equal(v, recorded[k]), k
    # setting the interval keeps weights and hidden state, rewinds the counter - and back at 1 everything is allowed again
    pol.native_interval = 4
    h = pol.hidden_state(n)
    pol.evaluate_step(obs)
    assert not np.array_equal(pol.hidden_state(n), h)             # call 0 again
    pol.native_interval = 1
    assert np.array_equal(np.array(pol.weights), w0)
    pol.reset()
    assert tr.relabel(pol).shape == (T, n, 4)


# ------------------------------------------------------------------ 9 -----
def test_it_does_something(device, oracle):
    """The nominal Crazyflie from hover at 400 Hz for 5 s, with the hidden state at 100 Hz (R = 4) and at 400 Hz (R = 1, the
    misconfiguration): both finite, and different.  No flight-quality threshold: none can be derived here, and what the previous
    action in the observation means at the fast rate is unpinned - the figures are printed and kept in profiles/control_rate.json."""
    n = 64
    out = {}
    for interval in (4, 1):
        w = World(device, oracle, n, seed=0, domain_randomization=0, init_guidance=1.0, dt=0.0025, episode_step_limit=2000)
        w.policy.native_interval = interval
        roll(w, 2000, "fused", False)
        s = w.state.numpy()
        assert np.isfinite(s).all() and np.isfinite(w.policy.hidden_state(n)).all()
        out[interval] = s
        print(f"400 Hz, R = {interval}: terminated {w.env.finished_terminated().mean():.3f}, mean episode length "
              f"{w.env.finished_lengths().mean() * 0.0025:.3f} s, final position error "
              f"{np.linalg.norm(s[:, :3], axis=1).mean():.4f} m")
    assert not np.array_equal(out[4], out[1])
