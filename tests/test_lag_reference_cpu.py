"""tests/lag_reference.py on the CPU: the float64 lagged gains against the gain table's formula, the bound against a float32
restatement of the kernel's chain in two contraction orders, a wrong operand far outside it; the entry point's declaration and its
refusals that need no device; ``probing.LagTable`` against loops."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import actor_reference as AR
import gain_reference as GR
import lag_reference as LR
from conftest import ROOT

NAME = "rq_trajectory_policy_lag_table"
T, N, K = 24, 12, 16


def _recording(family, seed=0):
    """random weights, observations and entering states, and done codes with every rule of the walk: frozen steps, both kinds of end,
    episodes longer and shorter than K, a select that drops a third of the steps"""
    rng = np.random.default_rng([seed, 5])
    w = AR.weights(family, seed)
    x, h = AR.inputs("normal", T * N, seed)
    done = rng.choice(np.asarray([0, 0, 0, 0, 0, 0, 1, 2, 4, 4], np.uint8), (T, N))
    done[:, 0] = 0                                       # one env whose single episode outlasts the window
    select = rng.random((T, N)) > 1.0 / 3.0
    return w, x.reshape(T, N, 22), h.reshape(T, N, 16), done, select


@pytest.fixture(scope="module", params=["perturbed", "fresh"])
def case(request):
    w, obs, hid, done, select = _recording(request.param)
    return dict(w=w, obs=obs, hid=hid, done=done, select=select, ref=LR.lag_table(w, obs, hid, done, K, select))


def test_lag_0_is_the_gain_tables_a_and_the_counts_follow_the_episode_rules(case):
    c = case
    total, count, bound, _ = LR.lag_table(c["w"], c["obs"], c["hid"], c["done"], K)
    A = GR.gain_A(c["w"], c["obs"].reshape(T * N, 22), c["hid"].reshape(T * N, 16)).reshape(T, N, 4, 16)
    _, EA, _ = GR.gain_bound(c["w"], c["obs"].reshape(T * N, 22), c["hid"].reshape(T * N, 16))
    live = c["done"] != 4
    A[~live] = 0.0
    assert np.allclose(total[0], A.sum(0).transpose(1, 2, 0), rtol=1e-12, atol=1e-15)
    # one step alone at lag 0: the bound is gain_bound's
    one = LR.lag_table(c["w"], c["obs"][:1], c["hid"][:1], np.zeros((1, N), np.uint8), 1)
    assert np.allclose(one[2][0], EA.reshape(T, N, 4, 16)[0].transpose(1, 2, 0), rtol=1e-6, atol=0)
    # brute force: step t counts at lag k when k live steps of its own episode lie before it
    want = np.zeros((K, N), np.uint32)
    for e in range(N):
        age = 0
        for t in range(T):
            if c["done"][t, e] == 4:
                continue
            want[:min(age, K - 1) + 1, e] += 1
            age = 0 if c["done"][t, e] in (1, 2) else age + 1
    assert np.array_equal(count, want) and want[K - 1, 0] > 0 and (want[K - 1] == 0).any()
    assert not total[np.broadcast_to((count == 0)[:, None, None, :], total.shape)].any()


@pytest.mark.parametrize("order", [0, 1])
def test_the_float32_chain_lies_inside_the_bound_in_either_contraction_order(case, order):
    c = case
    total, count, bound, left_out = c["ref"]
    got = LR.emulate_table(c["w"], c["obs"], c["hid"], c["done"], K, c["select"], order)
    keep = np.broadcast_to(((count > 0) & ~left_out)[:, None, None, :], got.shape)
    err = np.abs(got.astype(np.float64) - total)
    assert keep.any() and left_out.sum() <= 0.05 * (count > 0).sum()
    assert (err[keep] <= bound[keep]).all(), float((err[keep] / bound[keep]).max())
    assert not got[~np.broadcast_to((count > 0)[:, None, None, :], got.shape)].any()
    if order:
        assert not np.array_equal(got, LR.emulate_table(c["w"], c["obs"], c["hid"], c["done"], K, c["select"], 0))


@pytest.mark.parametrize("block", ["Whr", "Whn", "Wiz"])
def test_an_untransposed_operand_leaves_the_bound_by_orders_of_magnitude(case, block):
    c = case
    total, count, bound, left_out = c["ref"]
    got = LR.emulate_table(c["w"], c["obs"], c["hid"], c["done"], K, c["select"], 0, untransposed=block)
    keep = np.broadcast_to(((count > 0) & ~left_out)[:, None, None, :], got.shape)
    err = np.abs(got.astype(np.float64) - total)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(keep & (err > 0), err / bound, 0.0)
    assert ratio.max() > 1e3
    if block[1] == "h":          # the recurrent operands do not touch lag 0
        assert ratio[0].max() <= 1.0 and ratio[1:].max() > 1e3


# ------------------------------------------------------------------------------ the C layer -
def test_the_entry_point_is_declared_bound_and_exported_and_refuses_null_arguments():
    from raptor_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "raptor_quad.h")).read()
    dynamic = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    m = re.search(r"RQ_API int %s\(([^;]*)\);" % NAME, hdr, re.S)
    assert m and len(m.group(1).split(",")) == len(_lib._SIGNATURES[NAME]) == 10
    assert NAME in _lib.EXPORTED_SYMBOLS and hasattr(lib, NAME) and re.search(r" T %s$" % NAME, dynamic, re.M)
    assert "`%s`" % NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert _lib.ABI_VERSION == 5 and "#define RQ_ABI_VERSION 5" in hdr
    h = C.c_void_p(4096)                     # never followed: a null argument is refused before anything is looked at
    assert lib.rq_trajectory_policy_lag_table(None, h, 4, 1, None, 0, None, None, 1, 0) == -1 and b"null argument" in lib.rq_last_error()
    assert lib.rq_trajectory_policy_lag_table(h, None, 4, 1, None, 0, None, None, 1, 0) == -1 and b"null argument" in lib.rq_last_error()


# ------------------------------------------------------------------------------ LagTable -
@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_lag_table_methods_against_loops(kind):
    from raptor_amd import probing
    rng = np.random.default_rng(3)
    k, n = 5, 7
    total = rng.standard_normal((k, 4, 16, n)).astype(np.float32)
    count = rng.integers(0, 4, (k, n)).astype(np.uint32)
    count[4] = 0                                          # a lag nothing reaches
    count[2, 3] = 0
    W0 = rng.standard_normal((16, 22))
    if kind == "torch":
        torch = pytest.importorskip("torch")
        tab = probing.LagTable(torch.tensor(total), torch.tensor(count.astype(np.int32)), W0)
    else:
        tab = probing.LagTable(total, count, W0)
    host = lambda a: a.numpy() if hasattr(a, "data_ptr") else a
    s64 = total.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        by_lag, per_env = host(tab.by_lag()), host(tab.per_env())
    assert by_lag.shape == (k, 4, 22) and per_env.shape == (k, 4, 22, n)
    groups = np.arange(n) % 3
    by_group = host(tab.by_group(groups, 3))
    for lag in range(k):
        acc, cnt = np.zeros((4, 22)), 0
        for e in range(n):
            g = s64[lag, :, :, e] @ W0
            acc, cnt = acc + g, cnt + int(count[lag, e])
            if count[lag, e]:
                assert np.allclose(per_env[lag, :, :, e], g / count[lag, e], rtol=1e-12, atol=1e-14)
            else:
                assert np.isnan(per_env[lag, :, :, e]).all()
        if cnt:
            assert np.allclose(by_lag[lag], acc / cnt, rtol=1e-12, atol=1e-14)
        else:
            assert np.isnan(by_lag[lag]).all()
        for g in range(3):
            members = np.flatnonzero(groups == g)
            cnt = int(count[lag, members].sum())
            want = sum(s64[lag, :, :, e] @ W0 for e in members) / cnt if cnt else np.full((4, 22), np.nan)
            assert np.allclose(by_group[g, lag], want, rtol=1e-12, atol=1e-14, equal_nan=True)
    norms = tab.norm_by_lag()
    assert set(norms) == set(probing.OBSERVATION_BLOCKS)
    a, z = probing.OBSERVATION_BLOCKS["orientation"]
    assert np.allclose(norms["orientation"][:4], [np.linalg.norm(by_lag[lag][:, a:z]) for lag in range(4)]) and np.isnan(norms["orientation"][4])
    with pytest.raises(ValueError):
        probing.LagTable(total[0], count, W0)
    with pytest.raises(ValueError):
        tab.by_group(np.zeros(n + 1, int), 1)
