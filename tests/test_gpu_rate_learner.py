"""The learner at a deployment control rate (``Raptor(native_interval=R)``, R > 1; ``Trajectory.start_steps``): the six *_rate kernels
of csrc/rq_grad.hpp against the recorded actions, the float64 reference of tests/rate_grad_reference.py and the identities the
native-rate learner holds (tests/test_gpu_policy_grad_float64.py, tests/test_gpu_distill.py, tests/test_gpu_error_table.py).

Largest |g - g_ref| / bound on an MI355X over n in {1, 17, 64, 65, 130} and both starts (``pytest -s`` prints every case):
R = 2: 5.4e-4, R = 3: 4.6e-4, R = 4: 3.0e-4 (the first run; no constant of the bound and no kernel was changed after it, and no env was
quieted for a ReLU kink).  The bound is ``rate_grad_reference.bound`` as derived there: it charges every path its magnitude, so the
signed gradient sits far inside it, as the native-rate learner's does on recordings of this length."""
import numpy as np
import pytest

import rate_grad_reference as RR
from distill_common import CURRENT, INITIAL, Opt, _ld, _perturbed, _targets, distill, forward, get_weights, loss_grad, opt_apply, opt_state, same
from gpu_common import World
from test_gpu_policy_grad import _dact, backward

pytestmark = pytest.mark.gpu

SIZES, RATES, T = (1, 17, 64, 65, 130), (2, 3, 4), 24
_made = {}


def _record(device, oracle, n, R):
    """distill_common._record's recipe at interval R, once per (n, R): 3 unrecorded steps, then 12 recorded without auto-reset (frozen
    stretches) and 12 with it; N(0, 1) observations on frozen steps, NaN in the padding -> (world, traj, state before step 0, starts)"""
    if (n, R) not in _made:
        import torch
        w = World(device, oracle, n, seed=300 + n + R, episode_step_limit=9, termination_position=0.6, domain_randomization=1)
        w.policy.native_interval = R
        w.policy.reset()
        roll = lambda steps, auto, traj=None: w.vector.rollout(device, w.env, w.params, w.state, w.policy, w.rng, steps, "fused",
                                                               autoreset=auto, trajectory=traj)
        roll(3, True)
        start, h = w.env.episode_steps(), w.policy.hidden_state(n)
        traj = w.vector.Trajectory(w.env, T)
        roll(T // 2, False, traj)
        roll(T - T // 2, True, traj)
        traj.start_steps = start
        t = traj.tensors()
        ends = (t["done"] == 2).nonzero()
        t["done"][ends[::2, 0], ends[::2, 1]] = 1
        draw = torch.randn(t["obs"].shape, device=t["obs"].device, generator=torch.Generator(t["obs"].device).manual_seed(n))
        t["obs"].copy_(torch.where((t["done"] == 4)[:, None, :], draw, t["obs"]))
        t["obs"][:, :, n:] = float("nan")
        torch.cuda.synchronize()
        assert start.any() and np.array_equal(traj.start_steps, start)
        _made[(n, R)] = (w, traj, h, start)
    return _made[(n, R)]


def _student(device, weights, R, seed=5):
    from raptor_amd.foundation_policy import Raptor
    pol = Raptor(device, weights=_perturbed(weights, seed), native_interval=R)
    pol.reset()
    return pol


@pytest.mark.parametrize("R", RATES)
@pytest.mark.parametrize("n", SIZES)
def test_forward_gives_the_recording_policy_its_own_actions_back(device, oracle, n, R):
    w, traj, h, _ = _record(device, oracle, n, R)
    rec, pol = traj.numpy(), w.policy
    pol.reset()
    pol.evaluate_step(rec["obs"][0])                      # call 0 of the policy's counter: the next call is not native
    pol.set_hidden_state(h)
    act = forward(traj, pol, CURRENT)[:, :, :n].transpose(0, 2, 1)
    live = rec["done"] != 4
    assert live.any() and same(act[live], rec["act"][live])
    assert np.array_equal(pol.hidden_state(n), h)
    pol.evaluate_step(rec["obs"][0])
    assert np.array_equal(pol.hidden_state(n), h)         # call 1: held - the forward moved neither the state nor the counter


@pytest.mark.parametrize("R", RATES)
@pytest.mark.parametrize("n", SIZES)
def test_gradient_within_the_float64_bound(device, oracle, weights, n, R):
    w, traj, _, k0 = _record(device, oracle, n, R)
    rec, ld, pol = traj.numpy(), _ld(traj), _student(device, weights, R)
    for start in (INITIAL, CURRENT):
        if start == CURRENT:
            pol.set_hidden_state(np.random.default_rng(9).uniform(-0.7, 0.7, (n, 16)).astype(np.float32))
        h_start = pol.hidden_state(n)
        act = forward(traj, pol, start)
        dact = _dact(T, n, ld, seed=n + R + start)
        g, gh = backward(traj, pol, dact, want_h=start == CURRENT)
        d = dact[:, :, :n].transpose(0, 2, 1)
        a_ref, cache = RR.forward(pol.weights.astype(np.float64), rec["obs"], rec["done"], R, k0, "initial" if start else "current", h_start)
        assert any((s["hold"] & (s["d"] != 4)).any() for s in cache["steps"]) or n == 1
        assert np.abs(act[:, :, :n].transpose(0, 2, 1) - a_ref).max() < 1e-4
        (g_ref, gh_ref), (b, bh) = RR.backward(cache, d), RR.bound(cache, d, waves=(n + 63) // 64)
        ratio = np.abs(g - g_ref) / b
        print(f"[rate grad] n={n} R={R} start={start}: max err / bound {ratio.max():.3g}, max |g| {np.abs(g_ref).max():.3g}")
        assert np.isfinite(g).all() and (ratio <= 1.0).all(), (int(np.argmax(ratio)), float(ratio.max()))
        if start == CURRENT:
            assert np.isfinite(gh).all() and not gh[:, n:].any()
            assert (np.abs(gh[:, :n].T - gh_ref) <= bh).all()


@pytest.mark.parametrize("n", [17, 130])
def test_loss_seeded_family_is_tied_to_the_unseeded_gradient_bit_for_bit(device, oracle, weights, n):
    from test_gpu_weighted_distill import wloss_grad
    R = 4
    w, traj, _, _ = _record(device, oracle, n, R)
    y, pol = _targets(traj, n, seed=n), _student(device, weights, R)
    act = forward(traj, pol, INITIAL)
    live = np.broadcast_to((traj.numpy()["done"] != 4)[:, None, :], (T, 4, n))
    gact = np.full_like(act, np.nan)
    gact[:, :, :n] = np.where(live, act[:, :, :n] - np.nan_to_num(y[:, :, :n]), np.float32(0))
    g_un, _ = backward(traj, pol, gact)
    loss, g = loss_grad(traj, pol, y)
    assert np.isfinite(loss) and g.any() and same(g, (g_un.astype(np.float64) * (2.0 * (1.0 / int(live.sum())))).astype(np.float32))
    lw, gw = wloss_grad(device, traj, pol, y, np.ones((1, n), np.float32))
    assert same(lw, loss) and same(gw, g)
    a, b = _student(device, weights, R), _student(device, weights, R)
    oa, ob = Opt(a), Opt(b)
    losses = distill(traj, a, oa, 1, y)
    opt_apply(ob, loss_grad(traj, b, y)[1])
    assert same(losses[0], loss) and same(get_weights(a), get_weights(b)) and not same(get_weights(a), pol.weights)
    for x, z in zip(opt_state(oa), opt_state(ob)):
        assert same(x, z)
    oa.close(); ob.close()


@pytest.mark.parametrize("R", RATES)
@pytest.mark.parametrize("n", SIZES)
def test_error_table_is_the_float32_sum_over_the_forwards_actions(device, oracle, n, R):
    from raptor_amd.probing import episode_steps
    from test_gpu_error_table import table
    w, traj, h, _ = _record(device, oracle, n, R)
    y, pol, edges = _targets(traj, n, seed=R), w.policy, np.asarray([0, 3, 2 ** 32 - 1], np.uint32)
    pol.reset()
    pol.set_hidden_state(h)                                         # the first test's forward: the recording policy from its own state
    act = forward(traj, pol, CURRENT)
    sse, count = table(traj, pol, edges, y, start=CURRENT)
    age = episode_steps(traj.numpy()["done"])                       # from 0 at the first recorded step; -1 on frozen steps
    want, cnt = np.zeros((2, n), np.float32), np.zeros((2, n), np.uint32)
    for t in range(T):
        d = np.nan_to_num(act[t, :, :n] - y[t, :, :n])
        e = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]
        for b in range(2):
            hit = (age[t] >= int(edges[b])) & (age[t] < int(edges[b + 1]))
            want[b] = np.where(hit, want[b] + e, want[b])
            cnt[b] += hit
    assert cnt.sum() > 0 and np.array_equal(count, cnt) and same(sse, want)


def test_refusals_and_staleness(device, oracle, weights):
    from raptor_amd._lib import RaptorQuadError
    from raptor_amd.policy_bank import PolicyBank
    from test_gpu_bank_distill import bank_loss_grad
    from test_gpu_error_table import table
    from test_gpu_gain_table import table as gain_table
    from test_gpu_weighted_distill import wdistill, wloss_grad
    n, R = 65, 4
    w, traj, _, k0 = _record(device, oracle, n, R)
    ld, edges, y, pol = _ld(traj), np.asarray([0, 2 ** 32 - 1], np.uint32), _targets(traj, n, seed=1), _student(device, weights, R)
    recorded, d, opt, ones = traj.numpy(), _dact(T, n, ld, 1), Opt(pol), np.ones((1, n), np.float32)

    def refused(words, fn):
        with pytest.raises(RaptorQuadError, match=words):
            fn()
        for k, v in traj.numpy().items():
            assert v.tobytes() == recorded[k].tobytes(), k

    forward(traj, pol, INITIAL)
    traj.start_steps = None                                         # without its phase the recording is refused, by name
    assert traj.start_steps is None
    for call in (lambda: forward(traj, pol, INITIAL), lambda: backward(traj, pol, d), lambda: loss_grad(traj, pol, y),
                 lambda: wloss_grad(device, traj, pol, y, ones), lambda: distill(traj, pol, opt, 1, y),
                 lambda: wdistill(device, traj, pol, opt, 1, y, ones), lambda: table(traj, pol, edges, y)):
        refused("rq_trajectory_set_start_steps", call)
    traj.start_steps = k0
    refused("no matching forward", lambda: backward(traj, pol, d))  # the starts were given anew: a forward from before is not theirs
    forward(traj, pol, INITIAL)
    g, _ = backward(traj, pol, d)
    pol.native_interval = 2
    refused("no matching forward", lambda: backward(traj, pol, d))
    pol.native_interval = R
    traj.start_steps = k0 + 1
    refused("no matching forward", lambda: backward(traj, pol, d))
    traj.start_steps = k0
    forward(traj, pol, INITIAL)
    assert same(backward(traj, pol, d)[0], g) and g.any()
    # what stays at the native rate only
    for call in (lambda: traj.relabel(pol), lambda: traj.hidden(pol), lambda: gain_table(traj, pol, edges, INITIAL),
                 lambda: bank_loss_grad(traj, PolicyBank(device, np.stack([pol.weights] * 2), native_interval=R), np.zeros(n, np.uint32), y)):
        refused("native rate only", call)
    from raptor_amd.probing import HiddenProbe
    refused("native rate only", lambda: HiddenProbe(pol, np.ones((n, 1), np.float32), ["one"], edges).moments(traj))
    # at interval 1 the starts are not read
    pol.native_interval = 1
    with_starts = loss_grad(traj, pol, y)
    traj.start_steps = None
    without = loss_grad(traj, pol, y)
    assert same(with_starts[0], without[0]) and same(with_starts[1], without[1]) and not same(with_starts[1], g)
    traj.start_steps = k0                                           # the recording is shared: as it was
    opt.close()
