"""The lagged-gain table on the GPU (rq_trajectory_policy_lag_table; csrc/rq_lag_table.inc; raptor_amd.probing.lag_gains).

The reference is float64 (tests/lag_reference.py: explicit products of the step Jacobians) at the GPU's own entering states
(``traj.hidden(pol)``) and the recorded observations; every cell must lie within that module's element-wise bound x (1 + 2^-20), the
counts are exact, and a lag beyond the recordings' episode limit of 9 has count 0 and sum exactly 0.  The cells of an env-lag whose
counted chains meet a step near a ReLU kink are left out, and only those, at most 2 % of the cells that count anything.

Largest |got - ref| / bound on an MI355X (``pytest -s`` prints it per case; the same for n_lags = 1, 4, 5 and 16), no constant of
the bound changed after the first GPU run:

    n = 1     0.009
    n = 16    0.012
    n = 17    0.014
    n = 50    0.015      (one env meets a near-kink step: 1 of 50 env-lags left out at lag 0, 2 of 450 over 16 lags)
    select, n = 50:  age < 3  0.010,  age >= 3  0.010

The bound charges every rounding at its worst and carries absolute-value products through every lag; the kernel's errors largely
cancel in the 48-term contractions, hence ratios of a percent or two.  The bound is not vacuous for that: an untransposed operand
leaves it by three orders of magnitude (tests/test_lag_reference_cpu.py).
"""
import ctypes as C

import numpy as np
import pytest

import gain_reference as GR
import lag_reference as LR
from distill_common import ASYNC, CURRENT, DEVICE, HOST, INITIAL, _lib, _perturbed, _record, same

pytestmark = pytest.mark.gpu

T = 40
SIZES = [1, 16, 17, 50]           # one env; a full wave of 16; a wave and one env; four waves, the last ragged
LAGS = [1, 4, 5, 16]              # every instantiation (4, 8, 16), a rounded-up one, one longer than the episode limit of 9
NAME = "rq_trajectory_policy_lag_table"
SENTINEL = np.float32(-777.25)
COUNT_SENTINEL = np.uint32(0xABCD1234)
BAR = 1.0 + 2.0 ** -20
MAX_LEFT_OUT = 0.02


def table(traj, pol, n_lags, select=None, start=INITIAL, ld_out=None, memory=HOST):
    """-> (sum [K, 4, 16, ld_out], count [K, ld_out]), pre-filled with the sentinels; select [T, n] bool or None"""
    L = _lib()
    n = int(traj._env.N_ENVIRONMENTS)
    ld_out = ld_out or n
    total, count = np.full((n_lags, 4, 16, ld_out), SENTINEL, np.float32), np.full((n_lags, ld_out), COUNT_SENTINEL, np.uint32)
    sel = None if select is None else np.ascontiguousarray(select, np.uint8)
    head = (traj._require("trajectory"), pol._handle(), n_lags, start)
    if memory == HOST:
        L.call(NAME, *head, None if sel is None else sel.ctypes.data, n, L.fptr(total), count.ctypes.data, ld_out, HOST)
        return total, count
    import torch
    d_total, d_count = torch.tensor(total, device="cuda"), torch.tensor(count.view(np.int32), device="cuda")
    d_sel = None if sel is None else torch.tensor(sel, device="cuda")
    torch.cuda.synchronize()
    L.call(NAME, *head, None if sel is None else C.c_void_p(d_sel.data_ptr()), n, C.c_void_p(d_total.data_ptr()), C.c_void_p(d_count.data_ptr()),
           ld_out, memory)
    L.call("rq_device_synchronize", traj._env._device._h)
    return d_total.cpu().numpy(), d_count.cpu().numpy().view(np.uint32)


def held_to_float64(got, got_count, ref, what):
    """the assertions of test 1 on one table against ``lag_reference.lag_table``'s (sum, count, bound, left_out), cut to the table's lags
    -> the largest error / bound"""
    k = got.shape[0]
    total, count, bound, left_out = (a[:k] for a in ref)
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
    print(f"{what}: largest error / bound {worst:.3f}, {int((left_out & counted).sum())} of {int(counted.sum())} env-lags left out "
          f"({100 * frac:.2f} %), largest |sum| {np.abs(total).max():.3g}")
    assert worst <= BAR, (what, worst)
    return worst


class Case:
    """One recording of n envs with every done code, a perturbed policy, and the float64 side: the recorded observations, the state
    entering every step as the GPU's own forward from the learned initial state leaves it, and the reference at 16 lags."""

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
        self.ref = LR.lag_table(self.w, self.obs, self.hid, self.done, 16)
        self.full = table(self.traj, self.pol, 16)


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
@pytest.mark.parametrize("n_lags", LAGS)
@pytest.mark.parametrize("n", SIZES)
def test_counts_are_exact_and_sums_lie_inside_the_float64_bound(cases, n, n_lags):
    from raptor_amd import probing
    c = cases(n)
    total, count = c.full if n_lags == 16 else table(c.traj, c.pol, n_lags)
    age = probing.episode_steps(c.done)
    for k in range(n_lags):          # a live step of age a reaches back a steps
        assert np.array_equal(count[k], ((c.done != 4) & (age >= k)).sum(0)), k
    assert total[0].any() and not count[9:].any() and not total[9:].any()
    held_to_float64(total, count, c.ref, f"n={n} n_lags={n_lags}")
    assert same(total, c.full[0][:n_lags]) and same(count, c.full[1][:n_lags])      # a lag does not depend on the instantiation


@pytest.mark.parametrize("n", [17, 50])
def test_lag_0_lies_inside_the_gain_tables_own_bound(cases, n):
    c = cases(n)
    edges = np.asarray([0, 2 ** 32 - 1], np.uint32)
    A, EA, _ = GR.gain_bound(c.w, c.obs.reshape(T * n, 22), c.hid.reshape(T * n, 16))
    A, EA = A.reshape(T, n, 4, 16), EA.reshape(T, n, 4, 16)
    A[c.done == 4], EA[c.done == 4] = 0.0, 0.0
    total, count = GR.gain_table(A, c.done, edges)
    bound = GR.table_bound(A, EA, c.done, edges)
    kink = (GR.near_kink(c.w, c.obs.reshape(T * n, 22)).reshape(T, n) & (c.done != 4)).any(0)
    assert same(c.full[1][0], count[0]) and kink.mean() <= MAX_LEFT_OUT
    err = np.abs(c.full[0][0].astype(np.float64) - total[0])
    assert (err[..., ~kink] <= bound[0][..., ~kink] * BAR).all()


# ------------------------------------------------------------------------------ 2. select -
def test_select_as_an_age_window_and_of_all_ones(cases):
    from raptor_amd import probing
    c, n = cases(50), 50
    young = (probing.episode_steps(c.done) < 3) & (c.done != 4)
    got = table(c.traj, c.pol, 8, select=young)
    ref = LR.lag_table(c.w, c.obs, c.hid, c.done, 8, young)
    assert 0 < int(got[1].sum()) < int(c.full[1][:8].sum()) and not got[1][3:].any()
    held_to_float64(got[0], got[1], ref, "age < 3")
    old = table(c.traj, c.pol, 8, select=~young)           # the unselected steps still carry the chains of the later ones
    held_to_float64(old[0], old[1], LR.lag_table(c.w, c.obs, c.hid, c.done, 8, ~young), "age >= 3")
    assert old[1][3:].any() and same(got[1] + old[1], c.full[1][:8])
    ones = table(c.traj, c.pol, 16, select=np.ones((T, n), bool))
    assert same(ones[0], c.full[0]) and same(ones[1], c.full[1])


# ------------------------------------------------------------------------------ 3. starts, determinism, strides, memory -
def test_both_starts_two_runs_strides_and_memory_modes(cases):
    c, n = cases(50), 50
    want = c.full
    again = table(c.traj, c.pol, 16)
    assert same(again[0], want[0]) and same(again[1], want[1])
    assert (want[0] != SENTINEL).all() and (want[1] != COUNT_SENTINEL).all()       # every cell < n is written
    young = np.random.default_rng(2).random((T, n)) < 0.5
    host = table(c.traj, c.pol, 5, select=young)
    for memory in (HOST, DEVICE, ASYNC):
        total, count = table(c.traj, c.pol, 5, select=young, ld_out=n + 3, memory=memory)
        assert same(total[..., :n], host[0]) and same(count[:, :n], host[1]), memory
        assert (total[..., n:] == SENTINEL).all() and (count[:, n:] == COUNT_SENTINEL).all(), memory
    c.pol.reset()                                        # the hidden state <- the learned initial state
    a = table(c.traj, c.pol, 16, start=CURRENT)
    assert same(a[0], want[0]) and same(a[1], want[1])
    h = np.random.default_rng(n).uniform(-0.5, 0.5, (n, 16)).astype(np.float32)
    c.pol.set_hidden_state(h)
    b = table(c.traj, c.pol, 16, start=CURRENT)
    assert not same(b[0], a[0]) and same(b[1], a[1])
    assert np.array_equal(c.pol.hidden_state(n), h)      # the policy's hidden state is not changed
    assert same(table(c.traj, c.pol, 16)[0], want[0])    # and the initial start does not read it
    c.pol.reset()


# ------------------------------------------------------------------------------ 4. frozen steps hold anything -
def test_nan_on_frozen_observations_reaches_no_cell(device, oracle, weights):
    import torch
    from raptor_amd.foundation_policy import Raptor
    n = 50
    _, traj = _record(device, oracle, n, T, seed=77, frozen=True, finite=False)
    pol = Raptor(device, weights=_perturbed(weights, 3))
    pol.reset()
    obs, done = traj.tensors()["obs"], traj.tensors()["done"]
    frozen = (done == 4)[:, None, :].expand_as(obs)
    assert frozen[:, :, :n].any()
    draw = torch.randn(obs.shape, device=obs.device, generator=torch.Generator(obs.device).manual_seed(5))
    obs.copy_(torch.where(frozen, draw, obs))
    torch.cuda.synchronize()
    finite = table(traj, pol, 16)
    obs[frozen] = float("nan")
    torch.cuda.synchronize()
    assert torch.isnan(traj.tensors()["obs"][:, :, :n]).any()
    b = table(traj, pol, 16)
    assert np.isfinite(b[0]).all() and b[0].any()
    assert same(finite[0], b[0]) and same(finite[1], b[1])


# ------------------------------------------------------------------------------ 5. the saved state -
def test_a_backward_after_the_call_finds_no_matching_forward(cases):
    from raptor_amd._lib import RaptorQuadError
    L = _lib()
    c, n = cases(17), 17
    ld = int(c.traj.tensors()["act"].shape[2])
    act, g = np.empty((T, 4, n), np.float32), np.ones((T, 4, n), np.float32)
    gw = np.empty(2084, np.float32)
    tp = c.traj._require("trajectory")
    L.call("rq_trajectory_policy_forward", tp, c.pol._handle(), INITIAL, L.fptr(act), n, HOST)
    L.call("rq_trajectory_policy_backward", tp, c.pol._handle(), L.fptr(g), n, L.fptr(gw), None, HOST)      # the pair works
    L.call("rq_trajectory_policy_forward", tp, c.pol._handle(), INITIAL, L.fptr(act), n, HOST)
    table(c.traj, c.pol, 4)
    with pytest.raises(RaptorQuadError) as err:
        L.call("rq_trajectory_policy_backward", tp, c.pol._handle(), L.fptr(g), n, L.fptr(gw), None, HOST)
    assert "no matching forward" in str(err.value) and ld >= n


# ------------------------------------------------------------------------------ 6. the refusals -
def test_refusals_through_the_c_abi(cases, device, weights):
    from raptor_amd._lib import RaptorQuadError
    from raptor_amd.foundation_policy import Raptor
    L = _lib()
    c, n = cases(17), 17
    pol = Raptor(device, weights=_perturbed(weights, 1))
    pol.reset()
    tp = c.traj._require("trajectory")
    sel = np.ones((T, n), np.uint8)

    def refused(words, n_lags=4, ld_out=n, ld_select=n, memory=HOST, select=True, null=None):
        total, count = np.full((16, 4, 16, n), SENTINEL, np.float32), np.full((16, n), COUNT_SENTINEL, np.uint32)
        args = [tp, pol._handle(), n_lags, INITIAL, sel.ctypes.data if select else None, ld_select, L.fptr(total), count.ctypes.data, ld_out, memory]
        if null is not None:
            args[null] = None
        with pytest.raises(RaptorQuadError) as err:
            L.call(NAME, *args)
        assert words in str(err.value) and err.value.status < 0, str(err.value)
        assert (total == SENTINEL).all() and (count == COUNT_SENTINEL).all(), words

    pol.set_precision("bf16")
    refused("fp32 policy only")
    pol.set_precision("fp32")
    pol.set_standardize(np.zeros(22, np.float32), np.ones(22, np.float32))
    refused("the Standardize stage has no gradient here")
    pol.set_standardize(None)
    pol.native_interval = 2
    refused("native rate only")
    pol.native_interval = 1
    refused("ld_out must be at least the number of envs", ld_out=n - 1)
    refused("n_lags must be 1 .. 16, not 0", n_lags=0)
    refused("n_lags must be 1 .. 16, not 17", n_lags=17)
    refused("ld_select must be at least the number of envs", ld_select=n - 1)
    refused("memory must be 0, 1 or 2", memory=3)
    refused("sum lives on another device", memory=DEVICE, select=False)
    refused("null argument: sum", null=6)
    refused("null argument: count", null=7)
    refused("null argument", null=0)
    refused("null argument", null=1)
    empty = c.world.vector.Trajectory(c.world.env, 4)
    tp = empty._require("trajectory")
    refused("the trajectory is empty")
    tp = c.traj._require("trajectory")
    a = table(c.traj, pol, 4, select=sel)                # after all that the call works
    assert np.isfinite(a[0]).all() and a[1].any()


# ------------------------------------------------------------------------------ 7. through Python -
def test_lag_gains_returns_the_c_abis_bits_and_by_lag_is_a_w0_over_count(cases):
    import torch
    from raptor_amd import probing
    c, n = cases(50), 50
    tab = probing.lag_gains(c.traj, c.pol)
    assert tab.sum.is_cuda and tab.count.is_cuda and tuple(tab.sum.shape) == (16, 4, 16, n)
    assert same(tab.sum.cpu().numpy(), c.full[0]) and same(tab.count.cpu().numpy().view(np.uint32), c.full[1])
    W0 = c.w[0:352].reshape(16, 22).astype(np.float64)
    s64, c64 = c.full[0].astype(np.float64), c.full[1].astype(np.float64)
    by_lag = tab.by_lag().cpu().numpy()
    assert by_lag.shape == (16, 4, 22) and np.isfinite(by_lag[:9]).all() and np.isnan(by_lag[9:]).all()
    assert np.allclose(by_lag[:9], np.einsum("kij,jf->kif", s64.sum(3), W0)[:9] / c64.sum(1)[:9, None, None], rtol=1e-12, atol=1e-14)
    norms = tab.norm_by_lag()
    assert norms["position"].shape == (16,) and (norms["position"][:9] > 0).all()
    young = (probing.episode_steps(c.done) < 3) & (c.done != 4)
    want = table(c.traj, c.pol, 8, select=young)
    for select in (young, torch.tensor(young, device="cuda")):
        got = probing.lag_gains(c.traj, c.pol, n_lags=8, select=select)
        assert same(got.sum.cpu().numpy(), want[0]) and same(got.count.cpu().numpy().view(np.uint32), want[1])
    host = probing.lag_gains(c.traj, c.pol, n_lags=8, select=young, device=False)
    assert isinstance(host.sum, np.ndarray) and same(host.sum, want[0])
