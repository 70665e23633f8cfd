"""The feedback-gain table on the GPU (rq_trajectory_policy_gain_table, rq_trajectory_policies_gain_table; csrc/rq_gain_table.inc;
raptor_amd.probing.feedback_gains).

The reference is float64: A = da/dp0 from tests/gain_reference.py at the GPU's own entering states (``traj.hidden(pol)``) and the
recorded observations, summed per env and age bucket; every cell must lie within the element-wise bound of that module (proved on the
CPU in tests/test_gain_reference_cpu.py) x (1 + 2^-20).  The cells of an env-bucket that holds a step near a ReLU kink
(``gain_reference.near_kink``) are left out - there the fp32 mask may legitimately differ - and only those, at most 2 % of the cells
that count anything.  Beside it: the counts against ``probing.episode_steps``, both starts, determinism, output strides and memory
modes, recordings whose frozen observations are NaN, a bank against single policies, the saved state of a pending backward, the
refusals, and the Python call.

Largest |got - ref| / bound on an MI355X (``pytest -s`` prints it per case), no constant of the bound changed after the first GPU
run; no env-bucket was left out for a kink in any case:

              log     no_age_0  short
    n = 1     0.007   0.006     0.005
    n = 64    0.015   0.012     0.014
    n = 65    0.022   0.015     0.013
    n = 130   0.017   0.013     0.013
    T = 1, start = current, n = 130:  0.020

The bound charges every rounding at its worst and adds the absolute-value products; the kernel's errors largely cancel in the
48-term contraction, hence ratios of a few percent.  The bound is not vacuous for that: a wrong operand image leaves it by three
orders of magnitude (tests/test_gain_reference_cpu.py).
"""
import ctypes as C

import numpy as np
import pytest

import gain_reference as GR
from distill_common import ASYNC, CURRENT, DEVICE, HOST, INITIAL, _lib, _perturbed, _record, same
from rollout_common import ids_of

pytestmark = pytest.mark.gpu

T = 40
SIZES = [1, 64, 65, 130]          # one env; a full wave; a wave and one env; three waves, the last ragged
SENTINEL = np.float32(-777.25)
COUNT_SENTINEL = np.uint32(0xABCD1234)
BAR = 1.0 + 2.0 ** -20
MAX_LEFT_OUT = 0.02


def _edges():
    from raptor_amd import probing
    return {"log": probing.log_age_edges(9, 4),                 # 0, 1, 2, 4, 9: the recordings' episode limit
            "no_age_0": np.asarray([1, 3, 9], np.uint32),       # age 0 is counted nowhere
            "short": np.asarray([0, 2, 5], np.uint32)}          # ages 5 .. 8 are counted nowhere


def table(traj, pol, edges, start=INITIAL, ld_out=None, memory=HOST, bank_ids=None):
    """-> (sum [B, 4, 16, ld_out], count [B, ld_out]), pre-filled with the sentinels; NumPy for HOST, fetched from torch tensors otherwise"""
    L = _lib()
    n = int(traj._env.N_ENVIRONMENTS)
    e = np.ascontiguousarray(edges, np.uint32)
    B, ld_out = e.size - 1, ld_out or n
    total, count = np.full((B, 4, 16, ld_out), SENTINEL, np.float32), np.full((B, ld_out), COUNT_SENTINEL, np.uint32)
    head = (pol._handle(),) if bank_ids is None else (pol._h, np.ascontiguousarray(bank_ids, np.uint32).ctypes.data)
    name = "rq_trajectory_policy_gain_table" if bank_ids is None else "rq_trajectory_policies_gain_table"
    if memory == HOST:
        L.call(name, traj._require("trajectory"), *head, e.ctypes.data, B, start, L.fptr(total), count.ctypes.data, ld_out, HOST)
        return total, count
    import torch
    d_total, d_count = torch.tensor(total, device="cuda"), torch.tensor(count.view(np.int32), device="cuda")
    torch.cuda.synchronize()
    L.call(name, traj._require("trajectory"), *head, e.ctypes.data, B, start, C.c_void_p(d_total.data_ptr()), C.c_void_p(d_count.data_ptr()),
           ld_out, memory)
    L.call("rq_device_synchronize", traj._env._device._h)
    return d_total.cpu().numpy(), d_count.cpu().numpy().view(np.uint32)


def reference(w, obs, hid, done, edges):
    """float64: (sum [B, 4, 16, N], count, bound [B, 4, 16, N], left_out [B, N]) from obs [T, N, 22], hid [T, N, 16], done [T, N]"""
    steps, n = done.shape
    A, EA, _ = GR.gain_bound(w, obs.reshape(steps * n, 22), hid.reshape(steps * n, 16))
    A, EA = A.reshape(steps, n, 4, 16), EA.reshape(steps, n, 4, 16)
    live = done != 4
    A[~live], EA[~live] = 0.0, 0.0                      # what a frozen step holds reaches no sum
    total, count = GR.gain_table(A, done, edges)
    bound = GR.table_bound(A, EA, done, edges)
    kink = GR.near_kink(w, obs.reshape(steps * n, 22)).reshape(steps, n) & live
    b = GR.buckets(GR.ages(done), edges)
    left_out = np.zeros(count.shape, bool)
    for t, e in zip(*np.nonzero(kink & (b >= 0))):
        left_out[b[t, e], e] = True
    return total, count, bound, left_out


def held_to_float64(got, got_count, w, obs, hid, done, edges, what):
    """the assertions of test 1 on one table -> the largest error / bound"""
    total, count, bound, left_out = reference(w, obs, hid, done, edges)
    assert same(got_count, count), what
    counted = count > 0
    frac = float((left_out & counted).sum()) / max(int(counted.sum()), 1)
    assert frac <= MAX_LEFT_OUT, (what, frac)
    assert np.isfinite(got).all(), what
    assert not got[np.broadcast_to(~counted[:, None, None, :], got.shape)].any(), what          # nothing counted: exact zeros
    keep = np.broadcast_to((counted & ~left_out)[:, None, None, :], got.shape)
    err = np.abs(got.astype(np.float64) - total)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    worst = float(ratio[keep].max()) if keep.any() else 0.0
    print(f"{what}: largest error / bound {worst:.3f}, {int((left_out & counted).sum())} of {int(counted.sum())} env-buckets left out "
          f"({100 * frac:.2f} %), largest |sum| {np.abs(total).max():.3g}")
    assert worst <= BAR, (what, worst)
    return worst


class Case:
    """One recording of n envs with every done code, a perturbed policy, and the float64 side's inputs: the recorded observations and
    the state entering every step as the GPU's own forward from the learned initial state leaves it."""

    def __init__(self, device, oracle, weights, n):
        from raptor_amd.foundation_policy import Raptor
        self.n = n
        self.world, self.traj = _record(device, oracle, n, T, seed=700 + n, frozen=True)
        self.w = _perturbed(weights, 20 + n)
        self.pol = Raptor(device, weights=self.w)
        self.pol.reset()
        rec = self.traj.numpy()
        self.obs, self.done = rec["obs"], rec["done"]
        self.hid = self.traj.hidden(self.pol)
        self._tables = {}

    def table(self, which):
        if which not in self._tables:
            self._tables[which] = table(self.traj, self.pol, _edges()[which])
        return self._tables[which]


_cases = {}


@pytest.fixture(scope="module")
def cases(device, oracle, weights):
    def get(n):
        if n not in _cases:
            _cases[n] = Case(device, oracle, weights, n)
        return _cases[n]
    yield get
    _cases.clear()


# ------------------------------------------------------------------------------ 1. counts and the float64 bound -
@pytest.mark.parametrize("which", ["log", "no_age_0", "short"])
@pytest.mark.parametrize("n", SIZES)
def test_counts_are_exact_and_sums_lie_inside_the_float64_bound(cases, n, which):
    from raptor_amd import probing
    c, edges = cases(n), _edges()[which]
    if n >= 64:          # the recording has what the table must get right: frozen steps, both kinds of end, a bucket met again
        k = GR.ages(c.done)
        assert (c.done == 4).any() and (c.done == 1).any() and (c.done == 2).any() and k.max() == 8
        assert (((c.done == 1) | (c.done == 2)).sum(0) >= 2).any()
    total, count = c.table(which)
    k = probing.episode_steps(c.done)
    for b in range(len(edges) - 1):
        assert np.array_equal(count[b], ((k >= int(edges[b])) & (k < int(edges[b + 1]))).sum(0)), b
    live = int((c.done != 4).sum())
    assert int(count.sum()) == live if which == "log" else int(count.sum()) <= live
    assert total.any()
    held_to_float64(total, count, c.w, c.obs, c.hid, c.done, edges, f"n={n} {which}")


# ------------------------------------------------------------------------------ 2. start = current -
@pytest.mark.parametrize("n", [65, 130])
def test_current_start_from_the_initial_state_is_the_initial_table(cases, n):
    c, edges = cases(n), _edges()["log"]
    c.pol.reset()                                        # the hidden state <- the learned initial state
    a = table(c.traj, c.pol, edges, CURRENT)
    assert same(a[0], c.table("log")[0]) and same(a[1], c.table("log")[1])
    c.pol.set_hidden_state(np.random.default_rng(n).uniform(-0.5, 0.5, (n, 16)).astype(np.float32))
    b = table(c.traj, c.pol, edges, CURRENT)
    assert not same(b[0], a[0]) and same(b[1], a[1])
    assert same(table(c.traj, c.pol, edges, INITIAL)[0], a[0])      # and the initial start does not read it
    c.pol.reset()


def test_one_step_from_a_random_current_state_lies_inside_the_bound(device, oracle, weights):
    from raptor_amd.foundation_policy import Raptor
    n = 130
    _, traj = _record(device, oracle, n, 1, seed=31, frozen=True)
    w = _perturbed(weights, 32)
    pol = Raptor(device, weights=w)
    pol.reset()
    h = np.random.default_rng(33).uniform(-0.9, 0.9, (n, 16)).astype(np.float32)
    pol.set_hidden_state(h)
    rec = traj.numpy()
    edges = np.asarray([0, 2 ** 32 - 1], np.uint32)
    total, count = table(traj, pol, edges, CURRENT)
    assert int(count.sum()) == int((rec["done"] != 4).sum()) > 0
    held_to_float64(total, count, w, rec["obs"], h[None], rec["done"], edges, "T=1 current")
    assert np.array_equal(pol.hidden_state(n), h)        # the policy's hidden state is not changed


# ------------------------------------------------------------------------------ 3. determinism, strides, memory -
@pytest.mark.parametrize("n", [65, 130])
def test_two_runs_strides_and_memory_modes_give_the_same_bits(cases, n):
    c, edges = cases(n), _edges()["log"]
    want = c.table("log")
    again = table(c.traj, c.pol, edges)
    assert same(again[0], want[0]) and same(again[1], want[1])
    assert (want[0] != SENTINEL).all() and (want[1] != COUNT_SENTINEL).all()       # every cell < n is written
    for memory in (HOST, DEVICE, ASYNC):
        total, count = table(c.traj, c.pol, edges, ld_out=n + 3, memory=memory)
        assert same(total[..., :n], want[0]) and same(count[:, :n], want[1]), memory
        assert (total[..., n:] == SENTINEL).all() and (count[:, n:] == COUNT_SENTINEL).all(), memory
        if memory != HOST:
            total, count = table(c.traj, c.pol, edges, memory=memory)
            assert same(total, want[0]) and same(count, want[1]), memory


# ------------------------------------------------------------------------------ 4. frozen steps hold anything -
def test_nan_on_frozen_observations_reaches_no_sum(device, oracle, weights):
    import torch
    from raptor_amd.foundation_policy import Raptor
    n = 130
    _, traj = _record(device, oracle, n, T, seed=77, frozen=True, finite=False)
    pol = Raptor(device, weights=_perturbed(weights, 3))
    pol.reset()
    obs, done = traj.tensors()["obs"], traj.tensors()["done"]
    frozen = (done == 4)[:, None, :].expand_as(obs)
    assert frozen[:, :, :n].any()
    all_edges = (_edges()["log"], _edges()["no_age_0"], np.asarray([0, 2 ** 32 - 1], np.uint32))
    # the same recording twice: its frozen observations finite (the draws _record(finite=True) puts there), then NaN
    draw = torch.randn(obs.shape, device=obs.device, generator=torch.Generator(obs.device).manual_seed(5))
    obs.copy_(torch.where(frozen, draw, obs))
    torch.cuda.synchronize()
    finite = [table(traj, pol, edges) for edges in all_edges]
    obs[frozen] = float("nan")
    torch.cuda.synchronize()
    assert torch.isnan(traj.tensors()["obs"][:, :, :n]).any()
    for edges, a in zip(all_edges, finite):
        b = table(traj, pol, edges)
        assert np.isfinite(b[0]).all() and b[0].any()
        assert same(a[0], b[0]) and same(a[1], b[1])


# ------------------------------------------------------------------------------ 5. a bank -
def test_a_banks_table_is_each_policys_own_block_by_block(cases, device, weights):
    from raptor_amd import probing
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.policy_bank import PolicyBank
    c, edges, n = cases(130), _edges()["log"], 130
    W = np.stack([_perturbed(weights, 90 + p) for p in range(3)])
    singles = []
    for p in range(3):
        pol = Raptor(device, weights=W[p])
        pol.reset()
        singles.append(table(c.traj, pol, edges))
    assert not same(singles[0][0], singles[1][0]) and not same(singles[1][0], singles[2][0])
    bank = PolicyBank(device, W)
    for blocks in ([0, 1, 2], [2, 0, 2]):
        ids = ids_of(blocks, n)
        total, count = table(c.traj, bank, edges, bank_ids=ids)
        for g, p in enumerate(blocks):
            cols = slice(64 * g, min(64 * g + 64, n))
            assert same(total[..., cols], singles[p][0][..., cols]) and same(count[:, cols], singles[p][1][:, cols]), (blocks, g)
    d_total, d_count = table(c.traj, bank, edges, ld_out=n + 5, memory=DEVICE, bank_ids=ids_of([2, 0, 2], n))
    assert same(d_total[..., :n], total) and same(d_count[:, :n], count) and (d_total[..., n:] == SENTINEL).all()
    # by_group under the bank: a group that mixes policies, against the float64 recomputation from the raw arrays
    ids = ids_of([2, 0, 1], n)
    tab = probing.feedback_gains(c.traj, bank, edges=edges, policy_ids=ids)
    raw = table(c.traj, bank, edges, bank_ids=ids)
    s = tab.sum.cpu().numpy() if hasattr(tab.sum, "data_ptr") else tab.sum
    assert same(s, raw[0])
    groups = np.arange(n) % 4
    got = tab.by_group(groups, 4)
    got = got.cpu().numpy() if hasattr(got, "data_ptr") else got
    W0 = W[:, 0:352].reshape(3, 16, 22).astype(np.float64)
    for g in range(4):
        for b in range(len(edges) - 1):
            acc, cnt = np.zeros((4, 22)), 0
            for e in np.flatnonzero(groups == g):
                acc += raw[0][b, :, :, e].astype(np.float64) @ W0[ids[e]]
                cnt += int(raw[1][b, e])
            assert cnt > 0 and np.allclose(got[g, b], acc / cnt, rtol=1e-12, atol=1e-14), (g, b)


# ------------------------------------------------------------------------------ 6. the saved state of a pending backward -
def test_a_table_between_forward_and_backward_leaves_the_gradient_as_it_was(cases):
    import torch
    from raptor_amd import probing
    from raptor_amd.training import trajectory_actions
    c = cases(130)

    def grad(with_table):
        w = torch.tensor(c.w, device="cuda", requires_grad=True)
        act = trajectory_actions(c.traj, c.pol, w)
        if with_table:
            probing.feedback_gains(c.traj, c.pol, edges=_edges()["log"])
            probing.feedback_gains(c.traj, c.pol, start="current")
        live = (c.traj.tensors()["done"] != 4)[:, None, :].expand_as(act)
        torch.where(live, act, torch.zeros_like(act))[:, :, :130].square().sum().backward()
        return w.grad.cpu().numpy()

    want = grad(False)
    got = grad(True)
    assert same(got, want) and want.any() and np.isfinite(want).all()


# ------------------------------------------------------------------------------ 7. the refusals -
def test_refusals_through_the_c_abi(cases, device, weights):
    from raptor_amd._lib import RaptorQuadError
    from raptor_amd.foundation_policy import Raptor
    from raptor_amd.policy_bank import PolicyBank
    L = _lib()
    c, n, good = cases(65), 65, _edges()["log"]
    pol = Raptor(device, weights=_perturbed(weights, 1))
    pol.reset()
    bank, ids = PolicyBank(device, np.stack([_perturbed(weights, 1)] * 2)), ids_of([1, 0], n)
    tp = c.traj._require("trajectory")

    def refused(words, edges=good, n_buckets=None, ld_out=n, memory=HOST, who=("policy", "bank")):
        e = np.ascontiguousarray(edges, np.uint32)
        B = e.size - 1 if n_buckets is None else n_buckets
        rows = max(B, 1)
        for name, head in (("rq_trajectory_policy_gain_table", (pol._handle(),)), ("rq_trajectory_policies_gain_table", (bank._h, ids.ctypes.data))):
            if ("bank" if "policies" in name else "policy") not in who:
                continue
            total, count = np.full((rows, 4, 16, n), SENTINEL, np.float32), np.full((rows, n), COUNT_SENTINEL, np.uint32)
            with pytest.raises(RaptorQuadError) as err:
                L.call(name, tp, *head, e.ctypes.data, B, INITIAL, L.fptr(total), count.ctypes.data, ld_out, memory)
            assert words in str(err.value) and err.value.status < 0, (name, str(err.value))
            assert (total == SENTINEL).all() and (count == COUNT_SENTINEL).all(), name

    pol.set_precision("bf16")
    refused("fp32 policy only", who=("policy",))
    pol.set_precision("fp32")
    pol.set_standardize(np.zeros(22, np.float32), np.ones(22, np.float32))
    refused("the Standardize stage has no gradient here", who=("policy",))
    pol.set_standardize(None)
    pol.native_interval = 2
    refused("native rate only", who=("policy",))
    pol.native_interval = 1
    one, two = np.asarray([1], np.uint32), np.asarray([2], np.uint32)
    L.call("rq_policy_bank_set_native_interval", bank._h, two.ctypes.data, 1)
    refused("native rate only", who=("bank",))
    L.call("rq_policy_bank_set_native_interval", bank._h, one.ctypes.data, 1)
    refused("ld_out must be at least the number of envs", ld_out=n - 1)
    refused("n_buckets must be 1 .. 32, not 0", n_buckets=0)
    refused("n_buckets must be 1 .. 32, not 33", edges=np.arange(34), n_buckets=33)
    refused("age_edges must ascend strictly (age_edges[2] does not)", edges=[0, 2, 2, 5])
    refused("age_edges must ascend strictly (age_edges[1] does not)", edges=[3, 1])
    refused("memory must be 0, 1 or 2", memory=3)
    split = ids.copy()
    split[10] = 0
    ids, kept = split, ids
    refused("differ inside a 64-env block", who=("bank",))
    ids = kept
    # device memory announced, host arrays given; null outputs
    total, count = np.full((4, 4, 16, n), SENTINEL, np.float32), np.full((4, n), COUNT_SENTINEL, np.uint32)
    with pytest.raises(RaptorQuadError) as err:
        L.call("rq_trajectory_policy_gain_table", tp, pol._handle(), good.ctypes.data, 4, INITIAL, L.fptr(total), count.ctypes.data, n, DEVICE)
    assert "sum lives on another device" in str(err.value) and (total == SENTINEL).all()
    for null, noun in ((2, "age_edges"), (5, "sum"), (6, "count")):
        args = [tp, pol._handle(), good.ctypes.data, 4, INITIAL, L.fptr(total), count.ctypes.data, n, HOST]
        args[null] = None
        with pytest.raises(RaptorQuadError) as err:
            L.call("rq_trajectory_policy_gain_table", *args)
        assert "null argument: " + noun in str(err.value)
    # after all that the calls work
    a, b = table(c.traj, pol, good), table(c.traj, bank, good, bank_ids=ids)
    assert same(a[0], b[0]) and same(a[1], b[1]) and np.isfinite(a[0]).all()


# ------------------------------------------------------------------------------ 8. through Python -
def test_feedback_gains_returns_the_c_abis_bits_and_by_age_is_a_w0_over_count(cases):
    from raptor_amd import probing
    c, n, edges = cases(130), 130, _edges()["log"]
    want = c.table("log")
    tab = probing.feedback_gains(c.traj, c.pol, edges=edges)
    assert tab.sum.is_cuda and tab.count.is_cuda and tuple(tab.sum.shape) == (4, 4, 16, n)
    assert same(tab.sum.cpu().numpy(), want[0]) and same(tab.count.cpu().numpy().view(np.uint32), want[1])
    W0 = c.w[0:352].reshape(16, 22).astype(np.float64)
    assert np.array_equal(tab.W0[0], W0)
    s64, c64 = want[0].astype(np.float64), want[1].astype(np.float64)
    by_age = tab.by_age().cpu().numpy()
    assert by_age.shape == (4, 4, 22) and np.isfinite(by_age).all()
    assert np.allclose(by_age, np.einsum("bik,kf->bif", s64.sum(3), W0) / c64.sum(1)[:, None, None], rtol=1e-12, atol=1e-14)
    per_env = tab.per_env().cpu().numpy()
    assert per_env.shape == (4, 22, n)
    e = int(np.argmax(c64.sum(0)))
    assert np.allclose(per_env[:, :, e], s64[:, :, :, e].sum(0) @ W0 / c64[:, e].sum(), rtol=1e-12, atol=1e-14)
    assert tuple(probing.GainTable.block(by_age, "linear_velocity").shape) == (4, 4, 3)
    whole = probing.feedback_gains(c.traj, c.pol, start="current")                        # edges=None: one bucket for every age
    ref = table(c.traj, c.pol, np.asarray([0, 2 ** 32 - 1], np.uint32), CURRENT)
    assert tuple(whole.sum.shape) == (1, 4, 16, n) and same(whole.sum.cpu().numpy(), ref[0])
