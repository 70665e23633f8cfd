"""The flight table without a GPU: the NumPy restatement (tests/flight_reference.py) against a straightforward float64 computation
and against ``probing.episode_steps``, NaN where nothing is counted, the header's declaration against raptor_amd/_lib.py and the
built library, ``probing.FlightTable``'s algebra on hand-made arrays, ``linear_age_edges``, the refusals Python makes itself, and
``FlightTableLaunch`` under a plain host compiler with the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import flight_reference as FR
from conftest import ROOT
from raptor_amd import probing
from raptor_amd.probing import FLIGHT_PEAKS, FLIGHT_SUMS, FlightTable, flight_table, linear_age_edges      # noqa: F401

T, N = 40, 24
EPS = 64 * 2.0 ** -24          # at most 43 rounded additions for T = 40: three or four per value, 39 in a cell


def _synthetic(seed=0):
    """[T, N] data with every done code: episodes of 5 .. 9 steps ending in 1 or 2, frozen stretches (4), truncations (3), actions
    beyond the clip, a start count per env"""
    rng = np.random.default_rng(seed)
    done = np.zeros((T, N), np.uint8)
    for i in range(N):
        t = int(rng.integers(0, 9))
        while t < T:
            done[t, i] = rng.choice([1, 2])
            if rng.random() < 0.4:
                done[t + 1:t + 1 + int(rng.integers(1, 5)), i] = 4
            t += int(rng.integers(5, 10))
    done[rng.random((T, N)) < 0.03] = 3
    obs = rng.standard_normal((T, N, 22)).astype(np.float32)
    obs[:, :, :3] *= 0.1
    act = rng.uniform(-1.3, 1.3, (T, N, 4)).astype(np.float32)
    act[rng.random((T, N, 4)) < 0.05] = 1.0          # exactly at the clip: saturated
    rew = rng.standard_normal((T, N)).astype(np.float32)
    start = rng.integers(0, 9, N).astype(np.uint32)
    return obs, act, rew, done, start


EDGES = {"doubling": np.asarray([0, 1, 2, 4, 9], np.uint32), "no_age_0": np.asarray([1, 3, 9], np.uint32),
         "short": np.asarray([0, 2, 5], np.uint32), "all": np.asarray([0, 2 ** 32 - 1], np.uint32), "units": np.arange(33, dtype=np.uint32)}


def _float64_table(obs, act, rew, k, edges, tol):
    """the same table, straightforwardly, in float64 -> (sum, sum of absolute terms [B, 9, N], peak [B, 3, N], count [B, N])"""
    x, a = obs.astype(np.float64), act.astype(np.float64)
    d = a - x[..., 18:22]
    pos2 = (x[..., :3] ** 2).sum(-1)
    v = np.stack([pos2, (x[..., 12:15] ** 2).sum(-1), (x[..., 15:18] ** 2).sum(-1), 1.0 - x[..., 11], (a ** 2).sum(-1), (d ** 2).sum(-1),
                  (np.abs(a) >= 1.0).sum(-1).astype(np.float64), (pos2 > tol * tol).astype(np.float64), rew.astype(np.float64)], -1)
    B = len(edges) - 1
    s, sa, p, c = np.zeros((B, 9, N)), np.zeros((B, 9, N)), np.zeros((B, 3, N)), np.zeros((B, N), np.int64)
    for b in range(B):
        m = (k >= int(edges[b])) & (k < int(edges[b + 1]))
        s[b] = np.where(m[..., None], v, 0.0).sum(0).T
        sa[b] = np.where(m[..., None], np.abs(v), 0.0).sum(0).T
        p[b] = np.where(m[..., None], v[..., [0, 3, 2]], 0.0).max(0).T
        c[b] = m.sum(0)
    return s, sa, p, c, v


@pytest.mark.parametrize("which", sorted(EDGES))
@pytest.mark.parametrize("started", [False, True])
def test_the_restatement_against_float64_and_against_episode_steps(which, started):
    obs, act, rew, done, start = _synthetic()
    assert all((done == code).any() for code in range(5))
    edges, start, tol = EDGES[which], (start if started else None), 0.05
    k = probing.episode_steps(done, start)
    assert np.array_equal(FR.ages(done, start), k)
    total, peak, count = FR.flight_table(obs, act, rew, done, edges, start, tol)
    s, sa, p, c, v = _float64_table(obs, act, rew, k, edges, float(np.float32(tol)))
    assert np.array_equal(count, c) and count.dtype == np.uint32
    if which == "all":          # every age has a bucket: every live step is counted
        assert int(count.sum()) == int((done != 4).sum())
    # outside: the float32 decision pos2 > tol2 is the restatement's; away from the threshold float64 decides the same
    pos2 = v[..., 0]
    tol2 = float(np.float32(tol) * np.float32(tol))
    assert (np.abs(pos2 - tol2) > 1e-6 * tol2).all()
    assert np.array_equal(total[:, 6], s[:, 6]) and np.array_equal(total[:, 7], s[:, 7])          # saturated and outside: exact
    assert total[:, 6].any() and total[:, 7].any()
    assert (np.abs(peak - p) <= 4 * 2.0 ** -24 * np.abs(p)).all()          # three or four roundings from the float64 value
    # the peaks are exactly float32 values of the restated per-step values
    v32 = FR.step_values(obs, act, rew, np.float32(np.float32(tol) * np.float32(tol)))
    for b in range(len(edges) - 1):
        m = (k >= int(edges[b])) & (k < int(edges[b + 1]))
        assert np.array_equal(peak[b], np.where(m[..., None], v32[..., [0, 3, 2]], np.float32(0)).max(0).T.clip(min=0))
    assert (np.abs(total.astype(np.float64) - s) <= EPS * sa).all(), (np.abs(total - s) / np.maximum(sa, 1e-300)).max()


def test_nan_on_frozen_steps_and_in_dropped_ages_changes_no_bit():
    obs, act, rew, done, start = _synthetic(1)
    edges = EDGES["short"]
    want = FR.flight_table(obs, act, rew, done, edges, start)
    k = probing.episode_steps(done, start)
    away = (k < 0) | (k >= 5)
    assert (k < 0).any() and (k >= 5).any()
    obs2, act2, rew2 = obs.copy(), act.copy(), rew.copy()
    obs2[away], act2[away], rew2[away] = np.nan, np.nan, np.nan
    got = FR.flight_table(obs2, act2, rew2, done, edges, start)
    for a, b in zip(want, got):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # a live, counted NaN goes into its own env's cells and nowhere else; it never replaces a peak
    t, i = np.argwhere((k >= 0) & (k < 2))[3]
    obs2[t, i, 0] = np.nan
    got = FR.flight_table(obs2, act2, rew2, done, edges, start)
    others = np.arange(N) != i
    assert np.isnan(got[0][0, 0, i]) and np.isfinite(got[0][:, :, others]).all() and np.isfinite(got[1]).all()
    assert np.array_equal(got[0][:, :, others].view(np.uint32), want[0][:, :, others].view(np.uint32))


def test_the_header_declares_the_call_and_the_enums_as_bound_and_exported():
    from raptor_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "raptor_quad.h")).read()
    name = "rq_trajectory_flight_table"
    assert name in _lib._SIGNATURES and name in _lib.EXPORTED_SYMBOLS
    m = re.search(r"RQ_API int %s\(([^;]*)\);" % name, hdr, re.S)
    assert m, f"{name} is not declared in include/raptor_quad.h"
    args = [re.sub(r"/\*.*?\*/", "", a, flags=re.S).split() for a in m.group(1).split(",")]
    assert [a[-1].lstrip("*") for a in args] == ["t", "start_steps", "tolerance", "age_edges", "n_buckets", "sum", "peak", "count", "ld_out", "memory"]
    assert [" ".join(a[:-1]) + ("*" if a[-1].startswith("*") else "") for a in args] == \
        ["rq_trajectory*", "const uint32_t*", "float", "const uint32_t*", "uint32_t", "float*", "float*", "uint32_t*", "uint32_t", "int"]
    sig = _lib._SIGNATURES[name]
    assert len(sig) == 10 and sig[2] is C.c_float and sig[4] is C.c_uint32 and sig[8] is C.c_uint32 and sig[9] is C.c_int
    sums = re.search(r"enum \{ (RQ_FLIGHT_POS2[^}]*?), RQ_FLIGHT_SUMS \}", hdr, re.S).group(1)
    assert [w.strip()[len("RQ_FLIGHT_"):].lower() for w in sums.split(",")] == FLIGHT_SUMS
    peaks = re.search(r"enum \{ (RQ_FLIGHT_PEAK_POS2[^}]*?), RQ_FLIGHT_PEAKS \}", hdr, re.S).group(1)
    assert [w.strip()[len("RQ_FLIGHT_PEAK_"):].lower() for w in peaks.split(",")] == FLIGHT_PEAKS
    assert FR.SUMS == FLIGHT_SUMS and FR.PEAKS == FLIGHT_PEAKS
    dynamic = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T %s$" % name, dynamic, re.M)
    assert "`%s`" % name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"#define RQ_ABI_VERSION (\d+)", hdr).group(1)) == 5 == _lib.load().rq_abi_version()
    h = C.c_void_p(4096)                     # never followed: a null argument is refused before anything is looked at
    lib = _lib.load()
    assert lib.rq_trajectory_flight_table(None, None, 0.05, h, 1, h, h, h, 1, 0) == -1 and b"null argument: trajectory" in lib.rq_last_error()
    build = open(os.path.join(ROOT, "raptor_amd", "build.py")).read()
    assert '"rq_flight_launch.hpp"' in build and '"rq_flight_table.inc"' in build


def _table(kind):
    """B = 3, N = 4 by hand; env 3 counts nothing anywhere, bucket 2 is empty for everyone"""
    s = np.zeros((3, 9, 4), np.float32)
    c = np.asarray([[2, 1, 4, 0], [1, 1, 0, 0], [0, 0, 0, 0]], np.uint32)
    for k in range(9):
        s[0, k] = [2 * (k + 1), k + 1, 8 * (k + 1), 0]
        s[1, k] = [k + 1, 3 * (k + 1), 0, 0]
    p = np.zeros((3, 3, 4), np.float32)
    p[0] = [[4, 1, 9, 0], [0.5, 0.25, 0.125, 0], [1, 2, 3, 0]]
    p[1] = [[16, 2, 0, 0], [0.1, 0.2, 0, 0], [7, 5, 0, 0]]
    e = [0, 2, 5, 9]
    if kind == "torch":
        torch = pytest.importorskip("torch")
        return FlightTable(torch.tensor(s), torch.tensor(p), torch.tensor(c.astype(np.int32)), e)
    return FlightTable(s, p, c, e)


def _np(a):
    return a.numpy() if hasattr(a, "numpy") and not isinstance(a, np.ndarray) else np.asarray(a)


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_flight_table_algebra_in_float64_with_nan_where_nothing_counts(kind):
    tab = _table(kind)
    m = _np(tab.mean("pos2"))
    assert m.dtype == np.float64 and m.shape == (3, 4)
    assert np.array_equal(m[0, :3], [1.0, 1.0, 2.0]) and np.isnan(m[0, 3]) and np.isnan(m[2]).all() and np.isnan(m[1, 2])
    assert np.allclose(_np(tab.rms_position())[0, :3], np.sqrt([1.0, 1.0, 2.0]), rtol=1e-15)
    with pytest.raises(ValueError, match="unknown column"):
        tab.mean("height")
    age = {k: _np(v) for k, v in tab.by_age().items()}
    assert sorted(age) == sorted(FlightTable.CURVES) and all(v.shape == (3,) and v.dtype == np.float64 for v in age.values())
    # bucket 0: sums (2 + 1 + 8) (k + 1) over 7 steps; bucket 1: 4 (k + 1) over 2
    assert np.allclose(age["rms_position"][:2], np.sqrt([11 / 7, 4 / 2]), rtol=1e-15) and np.isnan(age["rms_position"][2])
    assert np.allclose(age["mean_tilt"][:2], [4 * 11 / 7, 4 * 4 / 2]) and np.allclose(age["rms_rate"][:2], np.sqrt([3 * 11 / 7, 3 * 4 / 2]))
    assert np.allclose(age["effort"][:2], [5 * 11 / 7, 5 * 4 / 2]) and np.allclose(age["command_change"][:2], [6 * 11 / 7, 6 * 4 / 2])
    assert np.allclose(age["share_saturated"][:2], [7 * 11 / 7 / 4, 7 * 4 / 2 / 4]) and np.allclose(age["share_outside"][:2], [8 * 11 / 7, 8 * 4 / 2])
    assert np.allclose(age["mean_reward"][:2], [9 * 11 / 7, 9 * 4 / 2])
    ids = np.asarray([0, 2, 0, 2])          # group 1 is empty
    grp = {k: _np(v) for k, v in tab.by_group(ids, 3).items()}
    assert all(v.shape == (3, 3) for v in grp.values())
    assert np.allclose(grp["mean_reward"][0, :2], [9 * 10 / 6, 9 * 1 / 1]) and np.allclose(grp["mean_reward"][2, :2], [9 * 1 / 1, 9 * 3 / 1])
    assert np.isnan(grp["mean_reward"][1]).all() and np.isnan(grp["mean_reward"][:, 2]).all()
    pk = _np(tab.peak_by_group(ids, 3))
    assert pk.shape == (3, 3, 3) and np.array_equal(pk[0, 0], [9, 0.5, 3]) and np.array_equal(pk[2, 0], [1, 0.25, 2])
    assert np.allclose(pk[0, 1], [16, 0.1, 7]) and np.allclose(pk[2, 1], [2, 0.2, 5])
    assert np.isnan(pk[1]).all() and np.isnan(pk[:, 2]).all()
    env = {k: _np(v) for k, v in tab.per_env().items()}
    assert all(v.shape == (4,) for v in env.values()) and np.isnan(env["mean_reward"][3])
    assert np.allclose(env["mean_reward"][:3], [9 * 3 / 3, 9 * 4 / 2, 9 * 8 / 4])
    for bad in ([0, 1, 2], [0, 1, 2, 3], [0.0, 1.0, 2.0, 0.0], [0, -1, 0, 0]):
        with pytest.raises(ValueError, match="ids must be"):
            tab.by_group(np.asarray(bad), 3)
    with pytest.raises(ValueError, match=r"sum must be \[B, 9, N\]"):
        FlightTable(np.zeros((3, 8, 4), np.float32), np.zeros((3, 3, 4), np.float32), np.zeros((3, 4), np.uint32), [0, 1, 2, 3])


def test_recovery_is_the_first_bucket_from_which_the_curve_stays_below():
    y = [0.01, 0.40, 0.20, 0.04, 0.06, 0.03, 0.02]
    assert FlightTable.recovery(y, 1, 0.05) == 5 and FlightTable.recovery(y, 1, 0.06) == 3 and FlightTable.recovery(y, 0, 1.0) == 0
    assert FlightTable.recovery(y, 1, 0.01) == -1 and FlightTable.recovery(y, 6, 0.02) == 6
    assert FlightTable.recovery([0.01, np.nan, 0.01], 0, 0.05) == 2 and FlightTable.recovery([0.01, np.nan], 0, 0.05) == -1
    with pytest.raises(ValueError):
        FlightTable.recovery(y, 7, 0.05)


def test_linear_age_edges_and_pythons_own_refusals():
    e = linear_age_edges(90, 250, 32)
    assert e.dtype == np.uint32 and e.shape == (33,) and e[0] == 90 and e[-1] == 250 and (np.diff(e) == 5).all()
    assert np.array_equal(linear_age_edges(0, 10, 3), [0, 3, 6, 9])
    for lo, hi, n in ((0, 100, 33), (0, 100, 0), (0, 31, 32), (5, 5, 1), (7, 3, 2), (-1, 10, 2), (0, 1 << 32, 2)):
        with pytest.raises(ValueError):
            linear_age_edges(lo, hi, n)

    class Env:
        N_ENVIRONMENTS = 64
        _device = None

    class Traj:
        _env = Env()

    with pytest.raises(ValueError, match="edges"):
        flight_table(Traj(), edges=[0, 2, 2])
    with pytest.raises(ValueError, match="edges"):
        flight_table(Traj(), edges=np.arange(35))
    for tol in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tolerance"):
            flight_table(Traj(), tolerance=tol)
    for start in (np.zeros(63, int), np.zeros(64), -np.ones(64, int), np.zeros(64, bool)):
        with pytest.raises(ValueError, match="start_steps"):
            flight_table(Traj(), start_steps=start)


def test_flight_launch_defaults_refusals_and_layout_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "flight_launch_driver")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "raptor_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "flight_launch_driver.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["0", str(5 * 9 * 137), str(5 * 3 * 137), str(5 * 137)], r.stdout + r.stderr


def test_the_kernel_text_is_one_file_without_atomics_and_strides_a_recording_by_22():
    csrc = os.path.join(ROOT, "raptor_amd", "csrc")
    probe, text = open(os.path.join(csrc, "rq_probe.hip")).read(), open(os.path.join(csrc, "rq_flight_table.inc")).read()
    assert len(re.findall(r'#define RQ_FLIGHT_KERNEL k_trajectory_flight_table\n#define RQ_FLIGHT_DEPTH \d\n#define RQ_FLIGHT_BLOCK \d+\n'
                          r'#include "rq_flight_table.inc"', probe)) == 1
    code = re.sub(r"//[^\n]*", "", text)
    assert "atomic" not in code and "memset" not in code
    assert "RQ_POLICY_INPUT_DIM" in code and "RQ_OBSERVATION_DIM" not in code          # a recording's rows are the policy's 22
    assert "fmaf" not in code and "__fmul_rn" in code and "__fadd_rn" in code and "__fsub_rn" in code
