"""The policy bank (rq_rollout_policies): P student policies in one rollout, one per 64-env block.

Reference for everything: the project's own single-policy path on the slice.  Block g of the batch is flown, as a batch of its own
(`VectorModule(n_g, offset + 64 g)`, same seed, configuration and rng epoch), by `Raptor(weights[ids[64 g]])` through rq_rollout /
rq_rollout_record; shard == slice is an invariant of the engine (test_gpu_fused.py).  Every comparison is on the bits, no tolerance:
the bank's kernels call the single-policy kernels' own device functions.  Recordings are compared where a transition was taken (done
code != 4: the steps an env sat out frozen are never written by the fused kernel) and on every done code.
"""
import numpy as np
import pytest

from rollout_common import (OFFSET, STEPS, Batch, assert_same, assert_same_recording, bank_weights, bits, fly_bank, fly_slice, ids_of,
                            join, snapshot)

pytestmark = pytest.mark.gpu

# N = 200: three full blocks and a ragged one of 8; a non-monotone assignment with a policy reused on non-adjacent blocks
N, P = 200, 3
BLOCK_IDS = [2, 0, 2, 1]


@pytest.fixture(scope="module")
def W(device, weights):
    from raptor_amd.foundation_policy import Raptor
    W = bank_weights(weights, 8)
    obs = np.random.default_rng(0).standard_normal((4, 22)).astype(np.float32)
    a = [Raptor(device, weights=W[k]).evaluate_step(obs) for k in (0, 1, 2)]
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2]) and not np.array_equal(a[0], a[2])   # the equalities below are not vacuous
    assert not np.array_equal(W[0][2000:2016], W[1][2000:2016])            # ... nor is whose initial hidden state an env takes
    return W


_slices = {}


@pytest.fixture(scope="module")
def slices(device, W):
    """(autoreset, noise, record) -> the joined (snapshot, recording) of the four slices' own fused single-policy rollouts; each
    computed once for the module"""
    def get(autoreset, noise, record):
        key = (autoreset, noise, record)
        if key not in _slices:
            _slices[key] = join([fly_slice(device, W[p], min(64, N - 64 * g), OFFSET + 64 * g, autoreset=autoreset, noise=noise,
                                           record=record) for g, p in enumerate(BLOCK_IDS)])
        return _slices[key]
    return get


# ------------------------------------------------------------------------------ 1. bank == slices, fused -
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("autoreset", [True, False])
def test_bank_equals_slices_fused(device, W, slices, autoreset, noise):
    _, snap, _ = fly_bank(device, W[:P], N, ids_of(BLOCK_IDS, N), autoreset=autoreset, noise=noise)
    ref, _ = slices(autoreset, noise, False)
    assert_same(snap, ref, what=f"autoreset={autoreset} noise={noise}")
    assert snap["epoch"][0] == STEPS
    assert (snap["fin_counts"] >= (2 if autoreset else 1)).all()          # episode ends were crossed
    assert snap["frozen"].all() != autoreset


# ------------------------------------------------------------------------------ 2. recorded -
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("autoreset", [True, False])
def test_bank_recording_equals_slices(device, W, slices, autoreset, noise):
    _, snap, rec = fly_bank(device, W[:P], N, ids_of(BLOCK_IDS, N), autoreset=autoreset, noise=noise, record=True)
    ref, ref_rec = slices(autoreset, noise, True)
    assert rec["done"].shape == (STEPS, N)
    assert_same(snap, ref, what="recorded")
    assert_same_recording(rec, ref_rec, "recorded")
    assert (rec["done"] == 2).any() and ((rec["done"] == 4).any() != autoreset)


# ------------------------------------------------------------------------------ 3. fused == chained -
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("autoreset", [True, False])
def test_bank_fused_equals_chained(device, W, slices, autoreset, noise):
    ids = ids_of(BLOCK_IDS, N)
    _, snap_c, _ = fly_bank(device, W[:P], N, ids, mode="chained", autoreset=autoreset, noise=noise)
    ref, ref_rec = slices(autoreset, noise, True)
    assert_same(snap_c, ref, what="chained")
    _, snap_r, rec_c = fly_bank(device, W[:P], N, ids, mode="chained", autoreset=autoreset, noise=noise, record=True)
    assert_same(snap_r, ref, what="chained, recorded")
    assert_same_recording(rec_c, ref_rec, "chained")
    _, snap_f, rec_f = fly_bank(device, W[:P], N, ids, mode="fused", autoreset=autoreset, noise=noise, record=True)
    assert_same(snap_f, snap_r, what="fused against chained")
    assert_same_recording(rec_f, rec_c, "fused against chained")


def test_thaw_takes_each_policys_initial_state(device, W):
    """A freezing rollout, then an auto-reset one: every env starts its next episode from ITS policy's initial hidden state, in both modes."""
    ids = ids_of(BLOCK_IDS, N)
    ref, _ = join([fly_slice(device, W[p], min(64, N - 64 * g), OFFSET + 64 * g, steps=[20], autoreset=False)
                   for g, p in enumerate(BLOCK_IDS)])
    assert ref["frozen"].all()
    from raptor_amd.foundation_policy import Raptor
    thawed = []
    for g, p in enumerate(BLOCK_IDS):
        pol = Raptor(device, weights=W[p])
        b = Batch(device, min(64, N - 64 * g), offset=OFFSET + 64 * g)
        b.fly(pol, 20, autoreset=False)
        b.fly(pol, 5, autoreset=True)
        thawed.append((snapshot(b, pol.hidden_state(b.n)), None))
    ref2, _ = join(thawed)
    for mode in ("fused", "chained"):
        from raptor_amd.policy_bank import PolicyBank
        bank = PolicyBank(device, W[:P])
        b = Batch(device, N)
        b.fly(bank, 20, mode, autoreset=False, ids=ids)
        assert_same(snapshot(b, bank.hidden(N)), ref, what=f"{mode}: frozen")
        b.fly(bank, 5, mode, autoreset=True, ids=ids)
        assert_same(snapshot(b, bank.hidden(N)), ref2, what=f"{mode}: thawed")
        assert not b.env.frozen().any()


# ------------------------------------------------------------------------------ 4. degenerate ids -
@pytest.mark.parametrize("n", [8, 65, N])
@pytest.mark.parametrize("mode", ["fused", "chained"])
def test_one_id_everywhere_is_the_single_policy_rollout(device, W, n, mode):
    _, snap, rec = fly_bank(device, W[:P], n, np.full(n, 1, np.uint32), mode=mode, record=True)
    ref, ref_rec = fly_slice(device, W[1], n, OFFSET, mode=mode, record=True)
    assert_same(snap, ref, what=f"n={n} {mode}")
    assert_same_recording(rec, ref_rec, f"n={n} {mode}")


# ------------------------------------------------------------------------------ 5. the two-wave build -
def test_two_wave_build(device, W):
    """Above 65 536 envs the fused kernel is the two-waves-per-SIMD build: fused bank == chained bank on the whole batch, and the first
    block, the last full block and the ragged block == their slices (which run the one-wave build)."""
    from raptor_amd.policy_bank import block_policy_assignment
    n, p, steps, limit = 65536 + 64 + 5, 5, 12, 5
    ids = block_policy_assignment(n, p)
    _, snap_f, _ = fly_bank(device, W[:p], n, ids, steps=steps, limit=limit)
    _, snap_c, _ = fly_bank(device, W[:p], n, ids, steps=steps, limit=limit, mode="chained")
    assert_same(snap_f, snap_c, what="two-wave fused against chained")
    assert (snap_f["fin_counts"] == 2).all()
    for g in (0, 1024, 1025):
        lo, hi = 64 * g, min(64 * g + 64, n)
        ref, _ = fly_slice(device, W[ids[lo]], hi - lo, OFFSET + lo, steps=steps, limit=limit)
        cut = {k: v[lo:hi] for k, v in snap_f.items()}
        assert_same(cut, ref, what=f"block {g}")


# ------------------------------------------------------------------------------ 6. two launches join -
@pytest.mark.parametrize("mode", ["fused", "chained"])
def test_two_launches_join(device, W, slices, mode):
    _, snap, rec = fly_bank(device, W[:P], N, ids_of(BLOCK_IDS, N), steps=[20, 20], mode=mode, record=True)
    ref, ref_rec = slices(True, False, True)
    assert_same(snap, ref, what="2 x 20")
    assert_same_recording(rec, ref_rec, "2 x 20")


# ------------------------------------------------------------------------------ 7. set_weights, reset -
def test_set_weights_and_reset(device, W):
    from raptor_amd.policy_bank import PolicyBank
    ids = ids_of(BLOCK_IDS, N)
    W2 = W[:P].copy()
    W2[1] = W[7]
    bank = PolicyBank(device, W[:P])
    bank.set_weights(1, W[7])
    assert np.array_equal(bank.weights, W2)
    _, snap_a, _ = fly_bank(device, None, N, ids, bank=bank)
    _, snap_b, _ = fly_bank(device, W2, N, ids)
    _, snap_0, _ = fly_bank(device, W[:P], N, ids)
    assert_same(snap_a, snap_b, what="set_weights")
    blk = slice(192, 200)                                           # the block policy 1 flies
    assert not np.array_equal(snap_a["state"][blk], snap_0["state"][blk])
    assert np.array_equal(bits(snap_a["state"][:192]), bits(snap_0["state"][:192]))
    h0 = W2[ids][:, 2000:2016]
    assert not np.array_equal(bits(bank.hidden(N)), bits(h0))
    bank.reset()
    assert np.array_equal(bits(bank.hidden(N)), bits(h0))
    # ... and a rollout after reset() starts from it: a fresh batch flown by the used bank equals one flown by a new bank
    _, snap_c, _ = fly_bank(device, None, N, ids, bank=bank)
    assert_same(snap_c, snap_b, what="after reset")


# ------------------------------------------------------------------------------ 8. refusals -
def test_refusals_leave_everything_untouched(device, W):
    import raptor_amd.l2f as l2f
    from raptor_amd import _lib
    from raptor_amd.policy_bank import PolicyBank
    bank = PolicyBank(device, W[:P])
    b = Batch(device, N)
    ids = ids_of(BLOCK_IDS, N)
    b.fly(bank, 3, ids=ids)                                       # some history: statistics, epoch 3, a sized hidden state
    tr = b.vector.Trajectory(b.env, 10)
    b.vector.rollout(device, b.env, b.params, b.state, bank, b.rng, 4, "fused", True, trajectory=tr, policy_ids=ids)
    other = Batch(device, N)
    tr_other = other.vector.Trajectory(other.env, 10)
    device2 = l2f.Device(0)
    bank2 = PolicyBank(device2, W[:P])

    def call(bank_=bank, ids_=ids, steps=5, mode=_lib.ROLLOUT_FUSED, flags=_lib.ROLLOUT_AUTORESET, traj=tr):
        ids_ = np.ascontiguousarray(ids_, np.uint32)
        with pytest.raises(_lib.RaptorQuadError) as e:
            _lib.call("rq_rollout_policies", device._h, b.env._h, b.params._h, b.state._h, bank_._h, ids_.ctypes.data, b.rng._h, steps,
                      mode, flags, traj._h if traj is not None else None)
        return e.value

    too_big, split = ids.copy(), ids.copy()
    too_big[64:128] = P
    split[100] = 1
    cases = [("id >= P", dict(ids_=too_big), -1, "out of range"),
             ("ids differ inside a block", dict(ids_=split), -1, "differ inside a 64-env block"),
             ("bank of another device", dict(bank_=bank2), -5, "another device"),
             ("trajectory of another env", dict(traj=tr_other), -5, "another env"),
             ("trajectory without room", dict(steps=7), -1, "too small"),
             ("unknown mode", dict(mode=7), -1, "unknown mode"),
             ("unknown flag", dict(flags=2), -1, "unknown flags")]
    before = snapshot(b, bank.hidden(N))
    for mode in (_lib.ROLLOUT_FUSED, _lib.ROLLOUT_CHAINED):
        for what, kw, status, words in cases:
            err = call(**dict(dict(mode=mode), **kw))
            assert err.status == status, (what, err)
            assert words in str(err), (what, err)
            assert_same(snapshot(b, bank.hidden(N)), before, what=what)
            assert len(tr) == 4 and len(tr_other) == 0, what
    # the Python surface refuses the two id errors itself, before the library is called
    for bad in (too_big, split, ids[:-1]):
        with pytest.raises(ValueError):
            b.vector.rollout(device, b.env, b.params, b.state, bank, b.rng, 5, "fused", True, policy_ids=bad)
    assert_same(snapshot(b, bank.hidden(N)), before, what="ValueError")


# ------------------------------------------------------------------------------ 9. the per-policy table -
def test_policy_episode_table(device, W, slices):
    from raptor_amd.policy_bank import PolicyBank, policy_episode_table
    ids = ids_of(BLOCK_IDS, N)
    ref, _ = slices(True, False, False)
    b, snap, _ = fly_bank(device, W[:P], N, ids)
    table = policy_episode_table(b.env, ids, P)
    for p in range(P):
        m = ids == p
        assert table["envs"][p] == m.sum()
        assert table["episodes"][p] == ref["fin_counts"][m].sum()
        r = ref["fin_returns"][m].astype(np.float64)
        assert np.isclose(table["mean_return"][p], r.mean(), rtol=1e-12)
        assert np.isclose(table["std_return"][p], r.std(), rtol=1e-9)
        assert np.isclose(table["mean_length"][p], ref["fin_lengths"][m].astype(np.float64).mean(), rtol=1e-12)
        assert np.isclose(table["termination_share"][p], ref["fin_terminated"][m].sum() / ref["fin_counts"][m].sum(), rtol=1e-12)
    bank = PolicyBank(device, W[:P])
    fresh = Batch(device, N)
    again = bank.evaluate(fresh.vector, device, fresh.env, fresh.params, fresh.state, fresh.rng, STEPS, ids)
    assert again.keys() == table.keys()
    for k in table:
        assert np.array_equal(table[k], again[k], equal_nan=True), k
    # the default assignment: blocks dealt round-robin
    fresh = Batch(device, N)
    dealt = bank.evaluate(fresh.vector, device, fresh.env, fresh.params, fresh.state, fresh.rng, STEPS)
    assert list(dealt["envs"]) == [72, 64, 64]
