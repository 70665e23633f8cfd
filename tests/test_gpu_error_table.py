"""The imitation error table on the GPU (rq_trajectory_policy_error_table, rq_trajectory_policies_error_table; csrc/rq_grad_forward.inc
under RQ_GRAD_ERROR_TABLE; raptor_amd.training.imitation_error).

The reference for every bit is the NumPy float32 restatement (tests/error_table_reference.py) applied to the actions the learner's
own forward returns (rq_trajectory_policy_forward): the table is that forward with sums in place of stores.  Beside it: the counts
against ``probing.episode_steps``, the stored actions as the target, output strides and memory modes, recordings whose frozen
observations are unspecified, the loss of rq_trajectory_policy_loss_grad within the project's own bound, a bank against single
policies, the saved state of a pending backward, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import distill_reference as D
import error_table_reference as ER
from distill_common import CURRENT, DEVICE, HOST, INITIAL, _ld, _lib, _perturbed, _record, _targets, forward, loss_grad, same
from rollout_common import ids_of

pytestmark = pytest.mark.gpu

T = 40
SIZES = [1, 64, 65, 130]          # one env; a full wave; a wave and one env; three waves, the last ragged
SENTINEL = np.float32(-777.25)
COUNT_SENTINEL = np.uint32(0xABCD1234)
ALL_AGES = np.asarray([0, 2 ** 32 - 1], np.uint32)


def _edges():
    from raptor_amd import probing
    return {"log": probing.log_age_edges(9, 4),                 # 0, 1, 2, 4, 9: the recordings' episode limit
            "no_age_0": np.asarray([1, 3, 9], np.uint32),       # age 0 is counted nowhere
            "short": np.asarray([0, 2, 5], np.uint32)}          # ages 5 .. 8 are counted nowhere


def table(traj, pol, edges, target=None, start=INITIAL, ld_out=None, memory=HOST, bank_ids=None):
    """-> (sse, count) [B, ld_out], pre-filled with the sentinels; NumPy for HOST, fetched from torch tensors otherwise"""
    L = _lib()
    n = int(traj._env.N_ENVIRONMENTS)
    e = np.ascontiguousarray(edges, np.uint32)
    B, ld_out = e.size - 1, ld_out or n
    sse, count = np.full((B, ld_out), SENTINEL, np.float32), np.full((B, ld_out), COUNT_SENTINEL, np.uint32)
    head = (pol._handle(),) if bank_ids is None else (pol._h, np.ascontiguousarray(bank_ids, np.uint32).ctypes.data)
    name = "rq_trajectory_policy_error_table" if bank_ids is None else "rq_trajectory_policies_error_table"
    t = None if target is None else np.ascontiguousarray(target, np.float32)
    if memory == HOST:
        L.call(name, traj._require("trajectory"), *head, None if t is None else L.fptr(t), 0 if t is None else t.shape[2], e.ctypes.data, B,
               start, L.fptr(sse), count.ctypes.data, ld_out, HOST)
        return sse, count
    import torch
    d_sse, d_count = torch.tensor(sse, device="cuda"), torch.tensor(count.view(np.int32), device="cuda")
    d_t = None if t is None else torch.tensor(t, device="cuda")
    torch.cuda.synchronize()
    L.call(name, traj._require("trajectory"), *head, None if t is None else C.c_void_p(d_t.data_ptr()), 0 if t is None else t.shape[2],
           e.ctypes.data, B, start, C.c_void_p(d_sse.data_ptr()), C.c_void_p(d_count.data_ptr()), ld_out, memory)
    L.call("rq_device_synchronize", traj._env._device._h)
    return d_sse.cpu().numpy(), d_count.cpu().numpy().view(np.uint32)


class Case:
    """One recording of n envs with every done code, a perturbed policy whose current hidden state is not the initial one, labels
    with NaN on frozen steps and padding, and - computed once per start - the learner's own forward."""

    def __init__(self, device, oracle, weights, n):
        from raptor_amd.foundation_policy import Raptor
        self.n = n
        self.world, self.traj = _record(device, oracle, n, T, seed=500 + n, frozen=True)
        self.pol = Raptor(device, weights=_perturbed(weights, 40 + n))
        self.pol.reset()
        self.pol.set_hidden_state(np.random.default_rng(n).uniform(-0.5, 0.5, (n, 16)).astype(np.float32))
        self.y = _targets(self.traj, n, seed=60 + n)
        self.done = self.traj.numpy()["done"]
        self._act = {}

    def act(self, start):
        if start not in self._act:
            self._act[start] = forward(self.traj, self.pol, start)
        return self._act[start]


_cases = {}


@pytest.fixture(scope="module")
def cases(device, oracle, weights):
    def get(n):
        if n not in _cases:
            _cases[n] = Case(device, oracle, weights, n)
        return _cases[n]
    yield get
    _cases.clear()


# ------------------------------------------------------------------------------ 1. bit for bit against the restatement -
@pytest.mark.parametrize("which", ["log", "no_age_0", "short"])
@pytest.mark.parametrize("start", [INITIAL, CURRENT])
@pytest.mark.parametrize("n", SIZES)
def test_the_table_is_the_restatement_bit_for_bit(cases, n, start, which):
    from raptor_amd import probing
    c, edges = cases(n), _edges()[which]
    if n >= 64:          # the recording has what the table must get right: frozen steps, both kinds of end, a bucket met again
        k = ER.ages(c.done)
        assert (c.done == 4).any() and (c.done == 1).any() and (c.done == 2).any() and k.max() == 8
        assert (((c.done == 1) | (c.done == 2)).sum(0) >= 2).any()
    assert np.isnan(c.y[:, :, n:]).all() and (n < 64 or np.isnan(c.y[:, :, :n]).any())
    sse, count = table(c.traj, c.pol, edges, c.y, start)
    ref_sse, ref_count = ER.error_table(c.act(start), c.y, c.done, edges)
    assert same(count, ref_count)
    assert same(sse, ref_sse), np.abs(sse - ref_sse).max()
    assert np.isfinite(sse).all() and sse.any()
    k = probing.episode_steps(c.done)
    for b in range(len(edges) - 1):
        assert np.array_equal(count[b], ((k >= int(edges[b])) & (k < int(edges[b + 1]))).sum(0)), b
    live = int((c.done != 4).sum())
    assert int(count.sum()) == live if which == "log" else int(count.sum()) <= live
    if n >= 64 and which != "log":
        assert int(count.sum()) < live          # these edges leave live steps out: age 0, or ages 5 .. 8


# ------------------------------------------------------------------------------ 2. stored actions, strides, memory modes -
@pytest.mark.parametrize("n", [65, 130])
def test_target_none_is_the_stored_actions_and_strides_and_memory_modes_keep_the_bits(cases, n):
    c, edges = cases(n), _edges()["log"]
    stored = c.traj.tensors()["act"].cpu().numpy()
    sse0, count0 = table(c.traj, c.pol, edges, None)
    sse1, count1 = table(c.traj, c.pol, edges, stored)
    assert same(sse0, sse1) and same(count0, count1) and sse0.any()
    # a target narrower than the trajectory's own stride gives the same bits
    sse2, count2 = table(c.traj, c.pol, edges, np.ascontiguousarray(stored[:, :, :n]))
    assert same(sse0, sse2) and same(count0, count2)
    want_sse, want_count = table(c.traj, c.pol, edges, c.y)
    for memory in (HOST, DEVICE):
        sse, count = table(c.traj, c.pol, edges, c.y, ld_out=n + 3, memory=memory)
        assert same(sse[:, :n], want_sse) and same(count[:, :n], want_count), memory
        assert (sse[:, n:] == SENTINEL).all() and (count[:, n:] == COUNT_SENTINEL).all(), memory
    sse, count = table(c.traj, c.pol, edges, c.y, memory=DEVICE)
    assert same(sse, want_sse) and same(count, want_count)
    sse, count = table(c.traj, c.pol, edges, None, memory=DEVICE)
    assert same(sse, sse0) and same(count, count0)


# ------------------------------------------------------------------------------ 3. frozen steps hold anything -
def test_unspecified_frozen_observations_and_nan_targets_reach_no_sum(device, oracle, weights):
    from raptor_amd.foundation_policy import Raptor
    n = 130
    w, traj = _record(device, oracle, n, T, seed=77, frozen=True, finite=False)
    pol = Raptor(device, weights=_perturbed(weights, 3))
    pol.reset()
    done = traj.numpy()["done"]
    assert (done == 4).any()
    y = _targets(traj, n, seed=4)
    assert np.isnan(y[:, :, :n][np.broadcast_to((done == 4)[:, None, :], (T, 4, n))]).all()
    for edges in (_edges()["log"], _edges()["no_age_0"], ALL_AGES):
        sse, count = table(traj, pol, edges, y)
        assert np.isfinite(sse).all() and sse.any()
        assert int(count.sum()) <= int((done != 4).sum())
    # and the frozen observations themselves may be NaN
    obs = traj.tensors()["obs"]
    import torch
    obs[(traj.tensors()["done"] == 4)[:, None, :].expand_as(obs)] = float("nan")
    torch.cuda.synchronize()
    sse2, count2 = table(traj, pol, ALL_AGES, y)
    assert np.isfinite(sse2).all() and same(count2, count)


# ------------------------------------------------------------------------------ 4. the learner's loss -
@pytest.mark.parametrize("n", SIZES)
def test_the_tables_loss_is_the_learners_within_its_bound(cases, n):
    from raptor_amd.training import ErrorTable
    c = cases(n)
    sse, count = table(c.traj, c.pol, ALL_AGES, c.y)
    loss, _ = loss_grad(c.traj, c.pol, c.y)
    live = np.broadcast_to((c.done != 4)[:, None, :], (T, 4, n))
    ref, _, terms = D.masked_mse(c.act(INITIAL)[:, :, :n], c.y[:, :, :n], live)
    M = int(live.sum())
    assert int(count.sum()) * 4 == M
    bound = D.loss_bound(terms, M)
    got = float(ErrorTable(sse, count, ALL_AGES).loss())
    print(f"n={n}: table {got:.9g}, learner {float(loss):.9g}, float64 {ref:.9g}, bound {bound:.3g}")
    assert abs(got - ref) <= bound and abs(float(loss) - ref) <= bound
    assert abs(got - float(loss)) <= 2 * bound


# ------------------------------------------------------------------------------ 5. a bank -
def test_a_banks_table_is_each_policys_own_block_by_block(cases, device, weights):
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.policy_bank import PolicyBank
    c, edges, n = cases(130), _edges()["log"], 130
    W = np.stack([_perturbed(weights, 90 + p) for p in range(3)])
    singles = []
    for p in range(3):
        pol = Raptor(device, weights=W[p])
        pol.reset()
        singles.append(table(c.traj, pol, edges, c.y))
    assert not same(singles[0][0], singles[1][0]) and not same(singles[1][0], singles[2][0])
    bank = PolicyBank(device, W)
    for blocks in ([0, 1, 2], [2, 0, 2]):
        ids = ids_of(blocks, n)
        sse, count = table(c.traj, bank, edges, c.y, bank_ids=ids)
        for g, p in enumerate(blocks):
            cols = slice(64 * g, min(64 * g + 64, n))
            assert same(sse[:, cols], singles[p][0][:, cols]) and same(count[:, cols], singles[p][1][:, cols]), (blocks, g)
    # policy 1 owns no block of [2, 0, 2]: whatever it is changes nothing
    W2 = W.copy()
    W2[1] = _perturbed(weights, 5, scale=0.5)
    other = table(c.traj, PolicyBank(device, W2), edges, c.y, bank_ids=ids_of([2, 0, 2], n))
    assert same(other[0], sse) and same(other[1], count)
    d_sse, d_count = table(c.traj, bank, edges, c.y, ld_out=n + 5, memory=DEVICE, bank_ids=ids_of([2, 0, 2], n))
    assert same(d_sse[:, :n], sse) and same(d_count[:, :n], count) and (d_sse[:, n:] == SENTINEL).all()


# ------------------------------------------------------------------------------ 6. the saved state of a pending backward -
@pytest.mark.parametrize("start", [INITIAL, CURRENT])
def test_a_call_between_forward_and_backward_leaves_the_backward_as_it_was(cases, start):
    L = _lib()
    c = cases(130)
    ld = _ld(c.traj)
    ga = np.random.default_rng(8).standard_normal((T, 4, ld)).astype(np.float32)

    def backward():
        g = np.empty(2084, np.float32)
        L.call("rq_trajectory_policy_backward", c.traj._require("trajectory"), c.pol._handle(), L.fptr(ga), ld, L.fptr(g), None, HOST)
        return g

    forward(c.traj, c.pol, start)
    want = backward()
    forward(c.traj, c.pol, start)
    for other_start in (INITIAL, CURRENT):
        table(c.traj, c.pol, _edges()["log"], c.y, other_start)
        table(c.traj, c.pol, ALL_AGES, None, other_start, memory=DEVICE)
    got = backward()
    assert same(got, want) and want.any()


# ------------------------------------------------------------------------------ 7. the refusals -
def test_refusals_through_the_c_abi(cases, device, weights):
    import torch
    from raptor_amd._lib import RaptorQuadError
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.policy_bank import PolicyBank
    L = _lib()
    c, n, good = cases(65), 65, _edges()["log"]
    pol = Raptor(device, weights=_perturbed(weights, 1))
    pol.reset()
    bank, ids = PolicyBank(device, np.stack([_perturbed(weights, 1)] * 2)), ids_of([1, 0], n)
    tp = c.traj._require("trajectory")

    def refused(words, edges=good, n_buckets=None, ld_out=n, target=c.y, memory=HOST, who=("policy", "bank")):
        e = np.ascontiguousarray(edges, np.uint32)
        B = e.size - 1 if n_buckets is None else n_buckets
        rows = max(B, 1)
        for name, head in (("rq_trajectory_policy_error_table", (pol._handle(),)), ("rq_trajectory_policies_error_table", (bank._h, ids.ctypes.data))):
            if ("bank" if "policies" in name else "policy") not in who:
                continue
            sse, count = np.full((rows, n), SENTINEL, np.float32), np.full((rows, n), COUNT_SENTINEL, np.uint32)
            t_ptr, ld_t = (L.fptr(target), target.shape[2]) if isinstance(target, np.ndarray) else (C.c_void_p(target.data_ptr()), target.shape[2])
            with pytest.raises(RaptorQuadError) as err:
                L.call(name, tp, *head, t_ptr, ld_t, e.ctypes.data, B, INITIAL, L.fptr(sse), count.ctypes.data, ld_out, memory)
            assert words in str(err.value) and err.value.status < 0, (name, str(err.value))
            assert (sse == SENTINEL).all() and (count == COUNT_SENTINEL).all(), name

    pol.set_precision("bf16")
    refused("fp32 policy only", who=("policy",))
    pol.set_precision("fp32")
    pol.native_interval = 2
    refused("native rate only", who=("policy",))
    pol.native_interval = 1
    one, two = np.asarray([1], np.uint32), np.asarray([2], np.uint32)
    L.call("rq_policy_bank_set_native_interval", bank._h, two.ctypes.data, 1)
    refused("native rate only", who=("bank",))
    L.call("rq_policy_bank_set_native_interval", bank._h, one.ctypes.data, 1)
    refused("ld_out", ld_out=n - 1)
    refused("n_buckets must be 1 .. 32, not 0", n_buckets=0)
    refused("n_buckets must be 1 .. 32, not 33", edges=np.arange(34), n_buckets=33)
    refused("age_edges must ascend strictly (age_edges[2] does not)", edges=[0, 2, 2, 5])
    refused("age_edges must ascend strictly (age_edges[1] does not)", edges=[3, 1])
    refused("ld_target", target=np.ascontiguousarray(c.y[:, :, :n - 1]))
    yd = torch.tensor(c.y, device="cuda")
    torch.cuda.synchronize()
    refused("the target is device memory", target=yd)            # a device target, host memory announced
    refused("memory must be 0, 1 or 2", memory=3)
    split = ids.copy()
    split[10] = 0
    ids, kept = split, ids
    refused("differ inside a 64-env block", who=("bank",))
    ids = kept
    # and the other way round: device memory announced, host arrays given
    sse, count = np.full((4, n), SENTINEL, np.float32), np.full((4, n), COUNT_SENTINEL, np.uint32)
    with pytest.raises(RaptorQuadError) as err:
        L.call("rq_trajectory_policy_error_table", tp, pol._handle(), C.c_void_p(yd.data_ptr()), yd.shape[2], good.ctypes.data, 4, INITIAL,
               L.fptr(sse), count.ctypes.data, n, DEVICE)
    assert "sse lives on another device" in str(err.value) and (sse == SENTINEL).all()
    for null in (7, 8):          # sse, count
        args = [tp, pol._handle(), L.fptr(c.y), c.y.shape[2], good.ctypes.data, 4, INITIAL, L.fptr(sse), count.ctypes.data, n, HOST]
        args[null] = None
        with pytest.raises(RaptorQuadError) as err:
            L.call("rq_trajectory_policy_error_table", *args)
        assert "null argument" in str(err.value)
    # after all that the calls work
    a, b = table(c.traj, pol, good, c.y), table(c.traj, bank, good, c.y, bank_ids=ids)
    assert same(a[0], b[0]) and same(a[1], b[1]) and np.isfinite(a[0]).all()


# ------------------------------------------------------------------------------ 8. through Python -
def test_imitation_error_returns_the_c_abis_bits_as_tensors_or_numpy(cases, device, weights):
    import torch
    from raptor_amd.policy_bank import PolicyBank
    from raptor_amd.training import imitation_error
    c, n, edges = cases(130), 130, _edges()["log"]
    want = table(c.traj, c.pol, edges, c.y)
    tab = imitation_error(c.traj, c.pol, edges=edges, target=c.y)                       # a NumPy target: NumPy out
    assert isinstance(tab.sse, np.ndarray) and same(tab.sse, want[0]) and same(tab.count, want[1])
    yd = torch.tensor(c.y, device="cuda")
    tab = imitation_error(c.traj, c.pol, edges=edges, target=yd)                        # a device target: tensors out
    assert tab.sse.is_cuda and tab.count.is_cuda and tab.sse.shape == (4, n)
    assert same(tab.sse.cpu().numpy(), want[0]) and same(tab.count.cpu().numpy().view(np.uint32), want[1])
    k = ER.ages(c.done)
    by_age = tab.by_age().cpu().numpy()
    assert by_age.shape == (4,) and np.isfinite(by_age).all()
    s64, c64 = want[0].astype(np.float64), want[1].astype(np.float64)
    assert np.allclose(by_age, s64.sum(1) / (4 * c64.sum(1)), rtol=1e-14, atol=0)
    groups = np.arange(n) % 5
    got = tab.by_group(groups, 5).cpu().numpy()
    for g in range(5):
        assert np.allclose(got[g], s64[:, groups == g].sum(1) / (4 * c64[:, groups == g].sum(1)), rtol=1e-14, atol=0)
    assert int(want[1].sum()) == int(((k >= 0) & (k < 9)).sum())
    whole = imitation_error(c.traj, c.pol, target=yd, start="current")                  # edges=None: the per-env error
    ref = table(c.traj, c.pol, ALL_AGES, c.y, CURRENT)
    assert whole.sse.shape == (1, n) and same(whole.sse.cpu().numpy(), ref[0])
    stored = imitation_error(c.traj, c.pol)                                               # the stored actions
    assert same(stored.sse.cpu().numpy(), table(c.traj, c.pol, ALL_AGES, None)[0])
    W = np.stack([_perturbed(weights, 90 + p) for p in range(3)])
    ids = ids_of([2, 0, 1], n)
    banked = imitation_error(c.traj, PolicyBank(device, W), edges=edges, target=yd, policy_ids=ids)
    ref = table(c.traj, PolicyBank(device, W), edges, c.y, bank_ids=ids)
    assert same(banked.sse.cpu().numpy(), ref[0]) and same(banked.count.cpu().numpy().view(np.uint32), ref[1])
    per_policy = banked.by_group(ids, 3).cpu().numpy()
    assert per_policy.shape == (3, 4) and np.isfinite(per_policy).all()
