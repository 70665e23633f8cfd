"""The feedback-gain table without a GPU: the float64 reference (tests/gain_reference.py) against central differences and autograd,
its bound proved on a NumPy float32 evaluation of the kernel's chain with sequential float32 sums, the kink test, the bucket sums,
``probing.GainTable``'s methods against brute-force loops, and the two entry points declared, bound and exported."""
import os
import re
import subprocess

import numpy as np
import pytest

import actor_reference as AR
import gain_reference as GR
from conftest import ROOT

NEW = ("rq_trajectory_policy_gain_table", "rq_trajectory_policies_gain_table")


def _case(family, n=32, seed=0, inputs="normal"):
    w = AR.weights(family, seed)
    x, h = AR.inputs(inputs, n, seed)
    return w, x[:, :22], h


# ------------------------------------------------------------------------------ the formula -
@pytest.mark.parametrize("family", AR.WEIGHT_FAMILIES)
def test_jacobian_is_autograds(family):
    import torch
    w, x, h = _case(family, 32, seed=3)
    B = {k: torch.tensor(v.astype(np.float64)) for k, v in AR.blocks(w).items()}

    def step(xv, hv):
        y0 = torch.relu(B["W0"] @ xv + B["b0"])
        gi, gh = B["Wi"] @ y0 + B["bi"], B["Wh"] @ hv + B["bh"]
        r, z = torch.sigmoid(gi[:16] + gh[:16]), torch.sigmoid(gi[16:32] + gh[16:32])
        n = torch.tanh(gi[32:] + r * gh[32:])
        return B["W2"] @ ((1 - z) * n + z * hv) + B["b2"]

    G = GR.jacobian(w, x, h)
    assert G.shape == (32, 4, 22) and G.dtype == np.float64
    worst = 0.0
    for i in range(32):
        xv, hv = torch.tensor(x[i].astype(np.float64)), torch.tensor(h[i].astype(np.float64))
        J = torch.autograd.functional.jacobian(lambda v: step(v, hv), xv).numpy()
        scale = max(np.abs(J).max(), 1e-300)
        worst = max(worst, np.abs(G[i] - J).max() / scale)
    assert worst < 1e-12, worst
    # and the float64 step itself is the one autograd differentiated
    a, _ = GR.step64(w, x, h)
    assert np.allclose(a[0], step(torch.tensor(x[0].astype(np.float64)), torch.tensor(h[0].astype(np.float64))).numpy(), rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("family", ["shipped", "perturbed", "fresh", "sat8", "signed_pos", "signed_neg"])
def test_jacobian_is_the_central_difference_away_from_kinks(family):
    w, x, h = _case(family, 32, seed=5)
    x, h = x.astype(np.float64), h.astype(np.float64)
    B = AR.blocks(w)
    p0 = x @ B["W0"].astype(np.float64).T + B["b0"].astype(np.float64)
    G = GR.jacobian(w, x, h)
    eps = 1e-6
    # a kink within the difference's reach: some p0_k changes sign for a move of eps along some coordinate
    reach = eps * np.abs(B["W0"].astype(np.float64)).max(axis=1)
    away = (np.abs(p0) > 4 * reach).all(axis=1)
    assert away.sum() >= 24
    D = np.empty_like(G)
    for f in range(22):
        d = np.zeros(22)
        d[f] = eps
        D[:, :, f] = (GR.step64(w, x + d, h)[0] - GR.step64(w, x - d, h)[0]) / (2 * eps)
    scale = np.abs(G[away]).max()
    assert scale > 0
    assert np.abs(G[away] - D[away]).max() <= 1e-6 * scale, np.abs(G[away] - D[away]).max() / scale


def test_the_mask_is_relu_prime_with_zero_at_zero():
    w = AR.weights("fresh", 1).copy()
    w[352:368] = 0.0                                   # b0 = 0: x = 0 puts every p0_k on the kink
    A = GR.gain_A(w, np.zeros((1, 22), np.float32), np.zeros((1, 16), np.float32))
    assert not A.any()
    assert not GR.near_kink(w, np.zeros((1, 22), np.float32)).any()        # 0 < 0 is false: fp32 gives that exact 0 too
    x = np.zeros((2, 22), np.float32)
    x[1, 0] = 1.0
    w[0:352] = 0.0
    w[0] = 1.0                                          # p0_0 = x_0
    w[352] = np.float32(-1.0)                           # ... - 1: exactly 0 at x_0 = 1
    assert list(GR.near_kink(w, x)) == [False, True]


# ------------------------------------------------------------------------------ the bound, proved on the CPU -
@pytest.mark.parametrize("inputs", AR.INPUT_FAMILIES)
@pytest.mark.parametrize("family", AR.WEIGHT_FAMILIES)
def test_the_float32_chain_lies_inside_the_bound_step_by_step_and_summed(family, inputs):
    T = 500
    w, x, h = _case(family, T, seed=11, inputs=inputs)
    got = GR.emulate_A(w, x, h)
    A, EA, share = GR.gain_bound(w, x, h, count=T)
    assert np.allclose(A, GR.gain_A(w, x, h), rtol=1e-10, atol=1e-12 * np.abs(A).max())        # two float64 orders of one sum
    keep = ~GR.near_kink(w, x)
    assert keep.mean() > 0.9, keep.mean()
    # where the masks differ the step is near a kink - and nowhere else
    B = AR.blocks(w)
    m64 = x.astype(np.float64) @ B["W0"].astype(np.float64).T + B["b0"].astype(np.float64) > 0
    assert np.isfinite(got).all() and np.isfinite(EA).all()
    r = AR.ratio(got[keep], A[keep], EA[keep])
    assert r.max() <= 1.0, (family, inputs, r.max())
    # a running float32 sum in step order, as the lane keeps it
    total = np.zeros((4, 16), np.float32)
    for t in np.flatnonzero(keep):
        total = (total + got[t]).astype(np.float32)
    n = int(keep.sum())
    _, _, share = GR.gain_bound(w, x[keep], h[keep], count=n)
    rs = AR.ratio(total, A[keep].sum(0), share.sum(0))
    assert rs.max() <= 1.0, (family, inputs, rs.max())
    assert m64.any() and (family == "tiny" or np.abs(A).max() > 0)


def test_the_bound_is_not_vacuous():
    """an error the size of a wrong operand image leaves the bound by orders of magnitude"""
    w, x, h = _case("shipped", 64, seed=2)
    A, EA, _ = GR.gain_bound(w, x, h)
    wrong = GR.gain_A(AR.altered(w, "swap_Wi"), x, h)
    live = EA > 0
    assert (np.abs(wrong - A)[live] / EA[live]).max() > 1e3
    rel = EA[live] / np.maximum(np.abs(A[live]), 1e-30)
    assert np.median(rel) < 1e-4, np.median(rel)


# ------------------------------------------------------------------------------ the table -
def test_gain_table_is_the_brute_force_sum():
    rng = np.random.default_rng(0)
    T, N = 30, 5
    done = rng.choice([0, 0, 0, 1, 2, 4], size=(T, N)).astype(np.uint8)
    A = rng.standard_normal((T, N, 4, 16))
    A[done == 4] = np.nan                              # frozen steps hold anything
    edges = np.asarray([1, 3, 6], np.uint32)
    total, count = GR.gain_table(A, done, edges)
    assert total.shape == (2, 4, 16, N) and count.shape == (2, N) and np.isfinite(total).all()
    for e in range(N):
        age = 0
        want, cnt = np.zeros((2, 4, 16)), np.zeros(2, int)
        for t in range(T):
            if done[t, e] == 4:
                continue
            for b in range(2):
                if edges[b] <= age < edges[b + 1]:
                    want[b] += A[t, e]
                    cnt[b] += 1
            age = 0 if done[t, e] in (1, 2) else age + 1
        assert np.allclose(total[:, :, :, e], want, rtol=1e-13) and list(count[:, e]) == list(cnt)
    tb = GR.table_bound(np.nan_to_num(A), np.full(A.shape, 1e-7), done, edges)
    assert tb.shape == total.shape and (tb[:, :, :, :][np.broadcast_to(count[:, None, None, :] > 0, tb.shape)] > 0).all()


def _brute(total, count, W0, pids, groups, G):
    """[G, B, 4, 22] by loops: every env's A sums times its own policy's W0, added, over the count"""
    B, N = count.shape
    out = np.full((G, B, 4, 22), np.nan)
    for g in range(G):
        for b in range(B):
            acc, c = np.zeros((4, 22)), 0
            for e in range(N):
                if groups[e] == g:
                    acc += total[b, :, :, e].astype(np.float64) @ W0[pids[e]]
                    c += int(count[b, e])
            if c:
                out[g, b] = acc / c
    return out


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_gain_table_methods_against_loops(kind):
    from raptor_amd import probing
    rng = np.random.default_rng(1)
    B, N, P = 3, 13, 2
    total = rng.standard_normal((B, 4, 16, N)).astype(np.float32)
    count = rng.integers(0, 5, (B, N)).astype(np.uint32)
    count[1, :] = 0                                    # a bucket nobody met
    count[:, 4] = 0                                    # an env that was never live
    total[np.broadcast_to(count[:, None, None, :] == 0, total.shape)] = 0
    edges = np.asarray([0, 1, 4, 9], np.uint32)
    W0 = rng.standard_normal((P, 16, 22))
    pids = np.asarray([0] * 7 + [1] * 6)
    groups = np.arange(N) % 3                          # every group mixes the two policies
    if kind == "torch":
        import torch
        make = lambda a, dt: torch.tensor(a.astype(dt))
        back = lambda t: t.numpy()
    else:
        make = lambda a, dt: a.astype(dt)
        back = lambda a: a
    single = probing.GainTable(make(total, np.float32), make(count, np.int32 if kind == "torch" else np.uint32), edges, W0[0])
    bank = probing.GainTable(make(total, np.float32), make(count, np.int32 if kind == "torch" else np.uint32), edges, W0, pids)
    for tab, ids in ((single, np.zeros(N, int)), (bank, pids)):
        want = _brute(total, count, W0, ids, np.zeros(N, int), 1)[0]
        got = back(tab.by_age())
        assert got.shape == (B, 4, 22) and got.dtype == np.float64
        assert np.isnan(got[1]).all() and np.allclose(got[[0, 2]], want[[0, 2]], rtol=1e-12, atol=1e-13)
        got = back(tab.by_group(groups, 3))
        assert got.shape == (3, B, 4, 22)
        assert np.allclose(got, _brute(total, count, W0, ids, groups, 3), rtol=1e-12, atol=1e-13, equal_nan=True)
        for bucket in (None, 0, 2):
            got = back(tab.per_env(bucket))
            assert got.shape == (4, 22, N)
            for e in range(N):
                s = total[:, :, :, e].astype(np.float64).sum(0) if bucket is None else total[bucket, :, :, e].astype(np.float64)
                c = int(count[:, e].sum()) if bucket is None else int(count[bucket, e])
                if c == 0:
                    assert np.isnan(got[:, :, e]).all()
                else:
                    assert np.allclose(got[:, :, e], s @ W0[ids[e]] / c, rtol=1e-12, atol=1e-13)
        g = tab.by_age()
        assert tuple(probing.GainTable.block(g, "position").shape) == (B, 4, 3)
        assert tuple(probing.GainTable.block(tab.per_env(), "orientation").shape) == (4, 9, N)
        assert np.array_equal(back(probing.GainTable.block(g, "last_action")), back(g)[..., 18:22], equal_nan=True)
    # the bank differs from the single policy exactly where policy 1 flies
    assert not np.allclose(back(single.per_env())[:, :, 8], back(bank.per_env())[:, :, 8])
    assert np.allclose(back(single.per_env())[:, :, 0], back(bank.per_env())[:, :, 0])
    assert probing.OBSERVATION_BLOCKS == {"position": (0, 3), "orientation": (3, 12), "linear_velocity": (12, 15),
                                          "angular_velocity": (15, 18), "last_action": (18, 22)}
    with pytest.raises(ValueError):
        probing.GainTable.block(g, "thrust")
    with pytest.raises(ValueError):
        single.by_group(np.arange(N), 3)
    with pytest.raises(ValueError):
        probing.GainTable(total, count, edges, W0)                     # a bank's W0 without ids
    with pytest.raises(ValueError):
        probing.GainTable(total[:, :, :8], count, edges, W0[0])


def test_python_refusals_come_before_any_library_call(monkeypatch):
    from raptor_amd import _lib, probing

    def no_call(name, *a):
        raise AssertionError("library call " + name)
    monkeypatch.setattr(_lib, "call", no_call)

    class Env:
        N_ENVIRONMENTS = 64
        _device = None

    class Traj:
        _env = Env()

    class Bank:
        n_policies = 2

    with pytest.raises(ValueError, match="start"):
        probing.feedback_gains(Traj(), object(), start="later")
    with pytest.raises(ValueError, match="edges"):
        probing.feedback_gains(Traj(), object(), edges=[0, 2, 2])
    with pytest.raises(ValueError, match="edges"):
        probing.feedback_gains(Traj(), object(), edges=np.arange(35))
    with pytest.raises(ValueError, match="needs policy_ids"):
        probing.feedback_gains(Traj(), Bank())
    with pytest.raises(ValueError, match="belong to a PolicyBank"):
        probing.feedback_gains(Traj(), object(), policy_ids=np.zeros(64, int))


# ------------------------------------------------------------------------------ the C layer -
def test_entry_points_are_declared_bound_and_exported():
    from raptor_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "raptor_quad.h")).read()
    dynamic = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        m = re.search(r"RQ_API int %s\(([^;]*)\);" % name, hdr, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib._SIGNATURES[name]), name
        assert re.search(r" T %s$" % name, dynamic, re.M), name
        assert "`%s`" % name in table, name


def test_what_needs_no_device_is_refused_first():
    import ctypes as C
    from raptor_amd import _lib
    lib = _lib.load()
    h = C.c_void_p(4096)                     # never followed: a null argument is refused before anything is looked at
    assert lib.rq_trajectory_policy_gain_table(None, h, None, 1, 1, None, None, 1, 0) == -1 and b"null argument" in lib.rq_last_error()
    assert lib.rq_trajectory_policy_gain_table(h, None, None, 1, 1, None, None, 1, 0) == -1 and b"null argument" in lib.rq_last_error()
    assert lib.rq_trajectory_policies_gain_table(h, h, None, None, 1, 1, None, None, 1, 0) == -1 and b"null argument" in lib.rq_last_error()
    assert lib.rq_trajectory_policies_gain_table(None, h, h, None, 1, 1, None, None, 1, 0) == -1 and b"null argument" in lib.rq_last_error()


def test_gain_table_launch_defaults_under_a_plain_compiler(tmp_path):
    exe = str(tmp_path / "gain_launch_driver")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "raptor_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "gain_launch_driver.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["0", "33"], r.stdout + r.stderr


def test_the_kernel_text_is_one_file_included_once_per_kernel():
    csrc = os.path.join(ROOT, "raptor_amd", "csrc")
    grad, bank = open(os.path.join(csrc, "rq_grad.hpp")).read(), open(os.path.join(csrc, "rq_grad_bank.hpp")).read()
    assert len(re.findall(r'#define RQ_GAIN_TABLE_KERNEL k_policy_gain_table\n#define RQ_GRAD_BANK 0\n#include "rq_gain_table.inc"', grad)) == 1
    assert len(re.findall(r'#define RQ_GAIN_TABLE_KERNEL k_policy_gain_table_bank\n#define RQ_GRAD_BANK 1\n#include "rq_gain_table.inc"', bank)) == 1
    text = open(os.path.join(csrc, "rq_gain_table.inc")).read()
    assert "__launch_bounds__(64, 1)" in text and "atomic" not in text.replace("no atomics", "")
