"""The host side of the policy bank (raptor_amd/policy_bank.py) without a GPU: the assignment helper, the validator of an assignment,
the per-policy table on a stand-in env, the dispatch errors of vector.rollout and the declared entry points."""
import numpy as np
import pytest

from raptor_amd.policy_bank import BLOCK, block_policy_assignment, check_policy_ids, policy_episode_table


@pytest.mark.parametrize("p", [1, 3, 7])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_block_policy_assignment(n, p):
    ids = block_policy_assignment(n, p)
    assert ids.dtype == np.uint32 and ids.shape == (n,) and ids.flags.c_contiguous
    assert (ids < p).all()
    for g in range((n + BLOCK - 1) // BLOCK):
        assert (ids[BLOCK * g:BLOCK * (g + 1)] == g % p).all()          # block-constant, dealt round-robin
    assert np.array_equal(check_policy_ids(ids, p, n), ids)


def test_block_policy_assignment_refuses_empty():
    for n, p in ((0, 3), (5, 0), (-1, 2)):
        with pytest.raises(ValueError):
            block_policy_assignment(n, p)


def test_check_policy_ids():
    good = np.repeat(np.array([2, 0, 2, 1]), 64)[:200]
    out = check_policy_ids(good, 3)
    assert out.dtype == np.uint32 and np.array_equal(out, good)
    assert np.array_equal(check_policy_ids(list(good), 3, 200), good)
    mid = good.copy(); mid[100] = 1                      # a change inside block 1
    with pytest.raises(ValueError, match="differ inside a 64-env block: env 100"):
        check_policy_ids(mid, 3)
    edge = good.copy(); edge[63] = 0                     # the block's last env takes the next block's id
    with pytest.raises(ValueError, match="differ inside"):
        check_policy_ids(edge, 3)
    with pytest.raises(ValueError, match="out of range: env 0 names policy 2 of a bank of 1"):
        check_policy_ids(good, 1)
    top = good.copy(); top[128:192] = 3                  # an id = P
    with pytest.raises(ValueError, match="out of range"):
        check_policy_ids(top, 3)
    with pytest.raises(ValueError, match="one id per env: 199 ids for 200 envs"):
        check_policy_ids(good[:-1], 3, 200)
    neg = good.astype(np.int64); neg[0:64] = -1
    with pytest.raises(ValueError, match="out of range"):
        check_policy_ids(neg, 3)
    with pytest.raises(ValueError):
        check_policy_ids(good.reshape(2, 100), 3)
    with pytest.raises(ValueError, match="integers"):
        check_policy_ids(good + 0.5, 3)
    with pytest.raises(ValueError):
        check_policy_ids([], 3)


class _Env:
    """what policy_episode_table reads of a VectorEnvironment"""

    def __init__(self, counts, returns, lengths, terminated):
        self._c, self._r, self._l, self._t = (np.asarray(a) for a in (counts, returns, lengths, terminated))

    def finished_counts(self): return self._c.astype(np.uint32)
    def finished_returns(self): return self._r.astype(np.float32)
    def finished_lengths(self): return self._l.astype(np.uint32)
    def finished_terminated(self): return self._t.astype(np.uint32)


def test_policy_episode_table():
    ids = np.array([0, 0, 0, 2, 2, 1], np.uint32)
    env = _Env(counts=[2, 1, 0, 3, 1, 0], returns=[10.0, 20.0, 99.0, 1.0, 3.0, 99.0], lengths=[16, 8, 0, 4, 6, 0],
               terminated=[1, 1, 0, 0, 1, 0])
    t = policy_episode_table(env, ids, 4)
    assert list(t["envs"]) == [3, 1, 2, 0]
    assert list(t["episodes"]) == [3, 0, 4, 0]
    assert np.allclose(t["mean_return"][[0, 2]], [15.0, 2.0]) and np.isnan(t["mean_return"][[1, 3]]).all()      # an env without an episode does not count
    assert np.allclose(t["std_return"][[0, 2]], [5.0, 1.0]) and np.isnan(t["std_return"][[1, 3]]).all()
    assert np.allclose(t["mean_length"][[0, 2]], [12.0, 5.0])
    assert np.allclose(t["termination_share"][[0, 2]], [2 / 3, 1 / 4]) and np.isnan(t["termination_share"][[1, 3]]).all()


def test_rollout_dispatch_errors():
    """policy_ids with anything but a PolicyBank, a PolicyBank without them or with a reference: ValueError before any library call"""
    import raptor_amd.l2f as l2f
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.policy_bank import PolicyBank
    from raptor_amd.teachers import TeacherBank
    vector = l2f.vector(128)
    ids = block_policy_assignment(128, 2)
    bank = PolicyBank.__new__(PolicyBank)                # no device here: the dispatch looks at the type and n_policies only
    bank.n_policies = 2
    teachers = TeacherBank.__new__(TeacherBank)
    ref = l2f.Reference.__new__(l2f.Reference)
    args = (None, None, None, None)
    with pytest.raises(ValueError, match="policy_ids belong to a PolicyBank"):
        vector.rollout(*args, Raptor(), None, 1, policy_ids=ids)
    with pytest.raises(ValueError, match="policy_ids belong to a PolicyBank"):
        vector.rollout(*args, teachers, None, 1, teacher_ids=ids, policy_ids=ids)
    with pytest.raises(ValueError, match="policy_ids: one policy id per env is required"):
        vector.rollout(*args, bank, None, 1)
    with pytest.raises(ValueError, match="does not track a reference"):
        vector.rollout(*args, bank, None, 1, policy_ids=ids, reference=ref)
    with pytest.raises(ValueError, match="teacher_ids belong to a TeacherBank"):
        vector.rollout(*args, bank, None, 1, policy_ids=ids, teacher_ids=ids)
    with pytest.raises(ValueError, match="differ inside"):
        vector.rollout(*args, bank, None, 1, policy_ids=np.arange(128) % 2)
    with pytest.raises(ValueError, match="one id per env"):
        vector.rollout(*args, bank, None, 1, policy_ids=ids[:64])


def test_entry_points_are_declared_and_bound():
    from raptor_amd import _lib
    lib = _lib.load()
    for name in ("rq_policy_bank_create", "rq_policy_bank_destroy", "rq_policy_bank_set_weights", "rq_policy_bank_reset",
                 "rq_policy_bank_get_hidden", "rq_rollout_policies"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.rq_abi_version() == 5
    assert lib.rq_policy_bank_create(None, None, 1, None) == -1
    assert lib.rq_policy_bank_destroy(None) == 0
    assert lib.rq_policy_bank_reset(None) == -1
    assert lib.rq_rollout_policies(None, None, None, None, None, None, None, 1, 0, 0, None) != 0


class _Stand:
    """a stand-in for anything that carries a handle: an l2f object, a Raptor"""

    def __init__(self, h):
        self._h, self._mirror = h, None

    def _require(self, what):
        return self._h

    def _handle(self, device):
        return self._h


def test_every_rollout_is_one_library_call(monkeypatch):
    """{Raptor, PolicyBank, TeacherBank} x {no reference, Reference, ReferenceBank + ids}, and a Raptor with a trajectory, through
    vector.rollout / PolicyBank.fly / TeacherBank.fly: one library call each, by the expected name, with as many arguments as the
    entry point declares, the ids and the reference where it takes them; what is refused is refused before the library."""
    import ctypes as C
    import raptor_amd.l2f as l2f
    from raptor_amd import _lib
    from raptor_amd.policy_bank import PolicyBank
    from raptor_amd.teachers import TeacherBank
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(_lib, "fast", None)              # the shortcut in front of the plain call would follow the stand-in handles
    n = 128
    vector = l2f.vector(n)
    device, env, params, state, rng, traj, raptor = (_Stand(h) for h in ("dev", "env", "params", "state", "rng", "traj", "policy"))
    world = (device, env, params, state)
    bank = PolicyBank.__new__(PolicyBank)
    bank.n_policies, bank._h = 2, "bank"
    teachers = TeacherBank.__new__(TeacherBank)
    teachers.n_teachers, teachers._h = 3, "teachers"
    ref = l2f.Reference.__new__(l2f.Reference)
    ref._h = "ref"
    refs = l2f.ReferenceBank.__new__(l2f.ReferenceBank)
    refs._h, refs.n_references = "refs", 4
    pids = block_policy_assignment(n, 2)
    tids = (np.arange(n) % 3).astype(np.uint32)
    rids = (np.arange(n) % 4).astype(np.uint32)

    def one(name, fly, ids=None, reference=None, ref_ids=None, trajectory=None):
        del calls[:]
        fly()
        assert [c[0] for c in calls] == [name], (name, calls)
        a = calls[0][1]
        assert len(a) == len(_lib._SIGNATURES[name]), name
        at = 5 if ids is not None else 4                  # the actor's handle, then its ids, then rng ...
        assert a[:4] == ("dev", "env", "params", "state") and a[4] in ("policy", "bank", "teachers"), name
        if ids is not None:
            got = np.ctypeslib.as_array((C.c_uint32 * n).from_address(a[5]))
            assert np.array_equal(got, ids), name
        assert a[at + 1:at + 5] == ("rng", 7, _lib.ROLLOUT_CHAINED, _lib.ROLLOUT_AUTORESET), name
        tail = list(a[at + 5:])
        if name != "rq_rollout":
            assert tail.pop(0) == (trajectory._h if trajectory is not None else None), name
        if reference is not None:
            assert tail.pop(0) == reference._h, name
        if ref_ids is not None:
            got = np.ctypeslib.as_array((C.c_uint32 * n).from_address(tail.pop(0)))
            assert np.array_equal(got, ref_ids), name
        assert tail == [], name

    kw = dict(mode="chained", autoreset=True)
    for reference, ref_ids, suffix in ((None, None, ""), (ref, None, "_track"), (refs, rids, "_track_refs")):
        rkw = dict(kw, reference=reference, reference_ids=ref_ids) if reference is not None else kw
        one("rq_rollout" + suffix, lambda: vector.rollout(*world, raptor, rng, 7, **rkw), None, reference, ref_ids)
        one("rq_rollout_policies" + suffix, lambda: bank.fly(vector, *world, rng, 7, pids, **rkw), pids, reference, ref_ids)
        one("rq_rollout_teachers" + suffix, lambda: teachers.fly(vector, *world, rng, 7, tids, **rkw), tids, reference, ref_ids)
    one("rq_rollout_record", lambda: vector.rollout(*world, raptor, rng, 7, trajectory=traj, **kw), trajectory=traj)
    # a bank through vector.rollout is the same call; a recording rides along in every tracked call
    one("rq_rollout_policies", lambda: vector.rollout(*world, bank, rng, 7, policy_ids=pids, **kw), pids)
    one("rq_rollout_teachers", lambda: vector.rollout(*world, teachers, rng, 7, teacher_ids=tids, trajectory=traj, **kw), tids,
        trajectory=traj)
    one("rq_rollout_track", lambda: vector.rollout(*world, raptor, rng, 7, reference=ref, trajectory=traj, **kw), None, ref,
        trajectory=traj)
    # refused before the library is reached
    del calls[:]
    for words, fly in (("reference and teacher_ids do not combine", lambda: vector.rollout(*world, teachers, rng, 7, teacher_ids=tids, reference=ref)),
                       ("reference_ids belong to a ReferenceBank", lambda: vector.rollout(*world, raptor, rng, 7, reference=ref, reference_ids=rids)),
                       ("reference_ids belong to a ReferenceBank", lambda: bank.fly(vector, *world, rng, 7, pids, reference=ref, reference_ids=rids)),
                       ("a ReferenceBank flies the envs by reference_ids", lambda: vector.rollout(*world, raptor, rng, 7, reference=refs)),
                       ("a ReferenceBank flies the envs by reference_ids", lambda: teachers.fly(vector, *world, rng, 7, tids, reference=refs)),
                       ("policy_ids belong to a PolicyBank", lambda: vector.rollout(*world, raptor, rng, 7, policy_ids=pids)),
                       ("teacher_ids must hold one id per env", lambda: teachers.fly(vector, *world, rng, 7, tids[:64]))):
        with pytest.raises(ValueError, match=words):
            fly()
    assert calls == []
