"""The policy bank at deployment conditions: every policy at its own native interval (rq_policy_bank_set_native_interval) and / or on a
moving setpoint (rq_rollout_policies_track, PolicyBank.fly).

Reference for everything, as in test_gpu_policy_bank.py: the project's own single-policy path on the slice.  Block g of the batch is
flown, as a batch of its own (`VectorModule(n_g, OFFSET + 64 g)`, same seed, configuration and `reference=`), by
`Raptor(weights=W[p], native_interval=R[p])`, p the block's policy, through the fused single-policy rollout; shard == slice is an
invariant of the engine.  Every comparison is on the bits, no tolerance: the bank's kernels call the single-policy kernels' own
device functions.  Recordings are compared where a transition was taken (done code != 4) and on every done code.
"""
from functools import partial

import numpy as np
import pytest

import rollout_common
from rollout_common import LIMIT, OFFSET, STEPS, assert_same, assert_same_recording, bank_weights, bits, fly_slice, ids_of, join, snapshot

pytestmark = pytest.mark.gpu

# every bank of this file flies through PolicyBank.fly (tests/test_gpu_policy_bank.py keeps to vector.rollout(..., policy_ids=))
Batch, fly_bank = partial(rollout_common.Batch, via="fly"), partial(rollout_common.fly_bank, via="fly")

# N = 200: three full blocks and a ragged one of 8; a non-monotone assignment with a policy reused on non-adjacent blocks
N, P = 200, 3
BLOCK_IDS = [2, 0, 2, 1]
RATES = (4, 1, 3)              # 3 does not divide 16: the phase reset at an episode end counts; interval 1 rides the RATE kernel
ONES = (1, 1, 1)


def differs(a, b):
    return any(not np.array_equal(bits(a[k]), bits(b[k])) for k in ("state", "hidden"))


@pytest.fixture(scope="module")
def W(device, weights):
    from raptor_amd.foundation_policy import Raptor
    W = bank_weights(weights, P)
    obs = np.random.default_rng(0).standard_normal((4, 22)).astype(np.float32)
    a = [Raptor(device, weights=W[k]).evaluate_step(obs) for k in range(P)]
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2]) and not np.array_equal(a[0], a[2])   # the equalities below are not vacuous
    return W


@pytest.fixture(scope="module")
def table():
    from raptor_amd.tracking import lissajous
    t = lissajous(LIMIT, 0.01, (0.3, 0.15, 0.0), 0.16)
    assert t.shape == (LIMIT, 6) and np.isfinite(t).all() and len({r.tobytes() for r in t}) == LIMIT
    return t


@pytest.fixture(scope="module")
def ref(device, table):
    import raptor_amd.l2f as l2f
    return l2f.Reference(device, table)


_slices = {}


@pytest.fixture(scope="module")
def slices(device, W, ref):
    """(rates, tracked, autoreset, noise, record) -> the joined (snapshot, recording) of the four slices' own fused single-policy
    rollouts, each slice's Raptor at the interval of its block's policy; each computed once for the module and left alone"""
    def get(rates, tracked, autoreset, noise, record):
        key = (tuple(rates), tracked, autoreset, noise, record)
        if key not in _slices:
            _slices[key] = join([fly_slice(device, W[p], min(64, N - 64 * g), OFFSET + 64 * g, rate=rates[p], ref=ref if tracked else None,
                                           autoreset=autoreset, noise=noise, record=record) for g, p in enumerate(BLOCK_IDS)])
        return _slices[key]
    return get


# the three deployment cases of the file: (name, intervals, tracked)
CASES = [("rate", RATES, False), ("track", ONES, True), ("both", RATES, True)]


def crossed_episode_ends(snap, autoreset):
    assert (snap["fin_counts"] >= (2 if autoreset else 1)).all()
    assert snap["frozen"].all() != autoreset


# ------------------------------------------------------------------------------ 1. rate: bank == slices -
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("autoreset", [True, False])
def test_rate_bank_equals_slices(device, W, slices, autoreset, noise):
    ids = ids_of(BLOCK_IDS, N)
    _, snap, _ = fly_bank(device, W, N, ids, RATES, autoreset=autoreset, noise=noise)
    want, _ = slices(RATES, False, autoreset, noise, False)
    assert_same(snap, want, what=f"rate autoreset={autoreset} noise={noise}")
    assert snap["epoch"][0] == STEPS
    crossed_episode_ends(snap, autoreset)
    assert not snap["track_steps"].any()
    # not vacuous: the same bank at interval 1 everywhere computes something else - except on the block of policy 1 (interval 1 in both)
    _, plain, _ = fly_bank(device, W, N, ids, ONES, autoreset=autoreset, noise=noise)
    assert differs(snap, plain)
    own = ids == 1
    assert np.array_equal(bits(snap["state"][own]), bits(plain["state"][own]))
    assert np.array_equal(bits(snap["hidden"][own]), bits(plain["hidden"][own]))
    for p in (0, 2):
        assert not np.array_equal(snap["hidden"][ids == p], plain["hidden"][ids == p]), p


# ------------------------------------------------------------------------------ 2. track: bank == slices -
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("autoreset", [True, False])
def test_track_bank_equals_slices(device, W, slices, ref, autoreset, noise):
    ids = ids_of(BLOCK_IDS, N)
    _, snap, _ = fly_bank(device, W, N, ids, ONES, ref=ref, autoreset=autoreset, noise=noise)
    want, _ = slices(ONES, True, autoreset, noise, False)
    assert_same(snap, want, what=f"track autoreset={autoreset} noise={noise}")       # track_sq and track_steps among the keys
    crossed_episode_ends(snap, autoreset)
    # every step an env took counts: all of them under auto-reset, its one episode's without
    assert np.array_equal(snap["track_steps"], np.full(N, STEPS, np.uint32) if autoreset else snap["fin_lengths"]) and (snap["track_sq"] > 0).all()
    _, untracked, _ = fly_bank(device, W, N, ids, ONES, autoreset=autoreset, noise=noise)
    assert differs(snap, untracked)
    assert not untracked["track_steps"].any()


# ------------------------------------------------------------------------------ 3. both together, recorded -
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("autoreset", [True, False])
def test_rate_and_track_recorded(device, W, slices, ref, table, autoreset, noise):
    ids = ids_of(BLOCK_IDS, N)
    _, snap, rec = fly_bank(device, W, N, ids, RATES, ref=ref, autoreset=autoreset, noise=noise, record=True)
    want, want_rec = slices(RATES, True, autoreset, noise, True)
    assert rec["done"].shape == (STEPS, N)
    assert_same(snap, want, what="rate + track, recorded")
    assert_same_recording(rec, want_rec, "rate + track, recorded")
    assert (rec["done"] == 2).any() and ((rec["done"] == 4).any() != autoreset)
    # recording changes nothing, and the recorded observations are setpoint-relative: another flight than rate alone records
    unrecorded, _ = slices(RATES, True, autoreset, noise, False)
    assert_same(snap, unrecorded, what="recorded against unrecorded")
    _, _, rec_rate = fly_bank(device, W, N, ids, RATES, autoreset=autoreset, noise=noise, record=True)
    # step 0: the same states, the same noise; only the setpoint's row 0 (position 0, velocity != 0) lies between the two
    assert np.array_equal(bits(rec["obs"][0][:, :12]), bits(rec_rate["obs"][0][:, :12]))
    assert np.array_equal(rec["obs"][0][:, 12:15], rec_rate["obs"][0][:, 12:15] - table[0, 3:])         # (a float32 subtraction, after the noise)
    assert not np.array_equal(rec["obs"][1], rec_rate["obs"][1])


# ------------------------------------------------------------------------------ 4. fused == chained -
@pytest.mark.parametrize("autoreset", [True, False])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_chained_equals_fused(device, W, slices, ref, case, autoreset):
    _, rates, tracked = case
    ids = ids_of(BLOCK_IDS, N)
    r = ref if tracked else None
    for noise in (False, True):
        want, want_rec = slices(rates, tracked, autoreset, noise, True)
        _, snap_c, _ = fly_bank(device, W, N, ids, rates, ref=r, mode="chained", autoreset=autoreset, noise=noise)
        assert_same(snap_c, want, what=f"chained noise={noise}")
        _, snap_r, rec_c = fly_bank(device, W, N, ids, rates, ref=r, mode="chained", autoreset=autoreset, noise=noise, record=True)
        assert_same(snap_r, want, what=f"chained, recorded noise={noise}")
        assert_same_recording(rec_c, want_rec, f"chained noise={noise}")


# ------------------------------------------------------------------------------ 5. the two-wave build -
def test_two_wave_build(device, W, ref):
    """Above 65 536 envs the fused kernel is the two-waves-per-SIMD build: fused bank == chained bank on the whole batch, and the first
    block, the last full block and the ragged block == their slices (which run the one-wave build)."""
    from raptor_amd.policy_bank import block_policy_assignment
    n, p, steps, limit = 65536 + 64 + 5, 2, 12, 5
    rates = (4, 1)                       # 4 against a limit of 5: the phase restarts at every episode end
    ids = block_policy_assignment(n, p)
    _, snap_f, _ = fly_bank(device, W[:p], n, ids, rates, ref=ref, steps=steps, limit=limit)
    _, snap_c, _ = fly_bank(device, W[:p], n, ids, rates, ref=ref, steps=steps, limit=limit, mode="chained")
    assert_same(snap_f, snap_c, what="two-wave fused against chained")
    assert (snap_f["fin_counts"] == 2).all() and (snap_f["track_steps"] == steps).all()
    for g in (0, 1, 1024, 1025):
        lo, hi = 64 * g, min(64 * g + 64, n)
        want, _ = fly_slice(device, W[ids[lo]], hi - lo, OFFSET + lo, rate=rates[ids[lo]], ref=ref, steps=steps, limit=limit)
        cut = {k: v[lo:hi] for k, v in snap_f.items()}
        assert_same(cut, want, what=f"block {g}")


# ------------------------------------------------------------------------------ 6. two launches join -
@pytest.mark.parametrize("mode", ["fused", "chained"])
def test_two_launches_join(device, W, slices, ref, mode):
    """25 + 15: neither launch ends on a multiple of 4 or 3 or at an episode end - the phase is rebuilt from the episode step count,
    the tracking sums carry on"""
    _, snap, rec = fly_bank(device, W, N, ids_of(BLOCK_IDS, N), RATES, ref=ref, steps=[25, 15], mode=mode, record=True)
    want, want_rec = slices(RATES, True, True, False, True)
    assert_same(snap, want, what="25 + 15")
    assert_same_recording(rec, want_rec, "25 + 15")


# ------------------------------------------------------------------------------ 7. a uniform bank is the policy -
@pytest.mark.parametrize("mode", ["fused", "chained"])
def test_uniform_bank_is_the_policy(device, W, ref, mode):
    from raptor_amd.policy_bank import PolicyBank
    bank = PolicyBank(device, W, native_interval=4)              # a scalar: every policy
    assert list(bank.native_interval) == [4, 4, 4]
    b = Batch(device, N)
    rec = b.fly(bank, STEPS, mode, True, True, ids=np.full(N, 1, np.uint32), ref=ref)
    want, want_rec = fly_slice(device, W[1], N, OFFSET, rate=4, ref=ref, mode=mode, record=True)
    assert_same(snapshot(b, bank.hidden(N)), want, what=mode)
    assert_same_recording(rec, want_rec, mode)


# ------------------------------------------------------------------------------ 8. the per-policy table with the RMSE -
def test_evaluate_with_reference(device, W, slices, ref):
    from raptor_amd.policy_bank import PolicyBank, policy_episode_table
    ids = ids_of(BLOCK_IDS, N)
    want, _ = slices(RATES, True, True, False, False)
    bank = PolicyBank(device, W, native_interval=list(RATES))
    b = Batch(device, N)
    table = bank.evaluate(b.vector, device, b.env, b.params, b.state, b.rng, STEPS, ids, reference=ref)
    assert_same(snapshot(b, bank.hidden(N)), want, what="evaluate")
    assert table["tracking_rmse"].shape == (P,)
    for p in range(P):
        m = ids == p
        rmse = np.sqrt(want["track_sq"][m].astype(np.float64).sum() / want["track_steps"][m].astype(np.float64).sum())
        assert rmse > 0 and np.isclose(table["tracking_rmse"][p], rmse, rtol=1e-12), p
    plain = policy_episode_table(b.env, ids, P)
    assert set(table) == set(plain) | {"tracking_rmse"}
    for k in plain:
        assert np.array_equal(table[k], plain[k], equal_nan=True), k
    # without a reference the table is what it was
    b = Batch(device, N)
    assert "tracking_rmse" not in bank.evaluate(b.vector, device, b.env, b.params, b.state, b.rng, STEPS, ids)


# ------------------------------------------------------------------------------ 9. refusals -
def test_refusals_enqueue_nothing(device, W, ref, table):
    import raptor_amd.l2f as l2f
    from raptor_amd import _lib
    from raptor_amd.policy_bank import PolicyBank
    from raptor_amd.training import BankDistiller
    ids = ids_of(BLOCK_IDS, N)
    bank = PolicyBank(device, W)
    b = Batch(device, N)
    b.fly(bank, 3, ids=ids, ref=ref)                              # some history: statistics, tracking sums, epoch 3, a sized hidden state
    tr = b.vector.Trajectory(b.env, 10)
    bank.fly(b.vector, device, b.env, b.params, b.state, b.rng, 4, ids, "fused", True, trajectory=tr)     # at interval 1: a recording to learn from
    bank.native_interval = list(RATES)
    device2 = l2f.Device(0)
    ref2 = l2f.Reference(device2, table)
    ref15 = l2f.Reference(device, table[:15])

    def intervals():
        out = np.zeros(P, np.uint32)
        _lib.call("rq_policy_bank_get_native_interval", bank._h, out.ctypes.data)
        return out

    def bank_weights_now():
        w = np.empty((P, 2084), np.float32)
        _lib.call("rq_policy_bank_get_weights", bank._h, _lib.fptr(w))
        return w

    def look():
        return dict(snapshot(b, bank.hidden(N)), intervals=intervals(), weights=bank_weights_now(), recorded=np.array([len(tr)]))

    def refused(name, *args):
        with pytest.raises(_lib.RaptorQuadError) as e:
            _lib.call(name, *args)
        return e.value

    def set_interval(values):
        a = np.ascontiguousarray(values, np.uint32)
        return refused("rq_policy_bank_set_native_interval", bank._h, a.ctypes.data, a.size)

    def track(reference, mode):
        return refused("rq_rollout_policies_track", device._h, b.env._h, b.params._h, b.state._h, bank._h, ids.ctypes.data, b.rng._h, 5,
                       mode, _lib.ROLLOUT_AUTORESET, tr._h, reference._h if reference is not None else None)

    distiller = BankDistiller(bank)
    target = np.zeros((len(tr), 4, N), np.float32)

    def learn(how):
        with pytest.raises(_lib.RaptorQuadError) as e:
            how(tr, ids, target=target)
        return e.value

    cases = [("interval 0", lambda: set_interval([0]), -1, "interval[0] is 0"),
             ("interval 65", lambda: set_interval([4, 65, 3]), -1, "interval[1] is 65"),
             ("n neither 1 nor P", lambda: set_interval([2, 2]), -1, "n must be 1"),
             ("reference of another device", lambda: track(ref2, _lib.ROLLOUT_FUSED), -5, "reference lives on another device"),
             ("reference of another device, chained", lambda: track(ref2, _lib.ROLLOUT_CHAINED), -5, "another device"),
             ("reference with 15 rows", lambda: track(ref15, _lib.ROLLOUT_FUSED), -1, "fewer rows than episode_step_limit"),
             ("reference with 15 rows, chained", lambda: track(ref15, _lib.ROLLOUT_CHAINED), -1, "fewer rows"),
             ("no reference", lambda: track(None, _lib.ROLLOUT_FUSED), -1, "null reference"),
             ("BankDistiller.step above interval 1", lambda: learn(distiller.step), -1, "rq_policy_bank_set_native_interval"),
             ("BankDistiller.loss_and_grad above interval 1", lambda: learn(distiller.loss_and_grad), -1,
              "rq_policy_bank_set_native_interval")]
    before = look()
    assert list(before["intervals"]) == list(RATES) and before["epoch"][0] == 7 and before["recorded"][0] == 4
    for what, attempt, status, words in cases:
        err = attempt()
        assert err.status == status, (what, err)
        assert words in str(err), (what, err)
        assert_same(look(), before, what=what)
    assert "policy 0 of the bank has native interval 4" in str(learn(distiller.loss_and_grad))
    # the Python surface refuses a bad interval itself; vector.rollout keeps refusing a bank's reference and names no new call
    for bad in (0, 65, [1, 2], [1, 2, 3, 4], 1.5):
        with pytest.raises(ValueError):
            bank.native_interval = bad
    with pytest.raises(ValueError, match="does not track a reference"):
        b.vector.rollout(device, b.env, b.params, b.state, bank, b.rng, 5, "fused", True, policy_ids=ids, reference=ref)
    assert_same(look(), before, what="ValueError")
    assert list(bank.native_interval) == list(RATES)
    # after the refusals: a valid tracked flight at these intervals, then back at interval 1 the learner takes the bank again
    bank.fly(b.vector, device, b.env, b.params, b.state, b.rng, 5, ids, "fused", True, trajectory=tr, reference=ref)
    after = look()
    assert after["epoch"][0] == 12 and after["recorded"][0] == 9 and differs(after, before)
    bank.native_interval = 1
    assert list(intervals()) == [1, 1, 1]
    loss, grad = distiller.loss_and_grad(tr, ids, target=np.zeros((len(tr), 4, N), np.float32))
    assert np.isfinite(np.asarray(loss)).all() and np.asarray(grad).shape == (P, 2084)
