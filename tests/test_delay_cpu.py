"""The delay schedule without a GPU: the entry points and what they refuse before the device is looked at, raptor_amd.delays (the rule
against a literal per-env deque, the table builders, the checks), the oracle loop that is the specification the GPU suite reuses
(tests/test_gpu_delay.py imports it from here) and the owner of the env's command history (tests/delay_history_driver.cpp on tests/fake_hip_memory,
a stand-alone program under the address and undefined-behaviour sanitizers)."""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ("rq_delay_bank_create", "rq_delay_bank_destroy", "rq_env_set_delay_schedule", "rq_env_clear_delay_schedule",
       "rq_env_get_delay_schedule")
S_LAST_ACTION = slice(17, 21)                # RQ_S_LAST_ACTION
MAX = 16


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def test_entry_points_are_declared_bound_and_exported():
    from raptor_amd import _lib, delays
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
    assert lib.rq_abi_version() == 5 and _lib.ABI_VERSION == 5
    assert int(re.search(r"#define RQ_DELAY_MAX_STEPS (\d+)", hdr).group(1)) == MAX == delays.MAX_STEPS
    assert re.search(r"still 5: rq_delay_bank_\{create,destroy\}", hdr) and "Delay schedule" in hdr


def test_what_needs_no_device_is_refused_first():
    import ctypes as C
    from raptor_amd import _lib
    lib = _lib.load()
    h = C.c_void_p(4096)                     # never followed: everything below is refused before the device is looked at
    rows = (C.c_uint8 * 8)(*([1] * 8))
    out = C.c_void_p()
    for args in ((None, rows, 1, 1, C.byref(out)), (h, None, 1, 1, C.byref(out)), (h, rows, 1, 1, None)):
        assert lib.rq_delay_bank_create(*args) == -1
        assert b"null argument" in lib.rq_last_error()
    assert lib.rq_delay_bank_create(h, rows, 0, 1, C.byref(out)) == -1 and b"at least one table" in lib.rq_last_error()
    assert lib.rq_delay_bank_create(h, rows, 1, 0, C.byref(out)) == -1 and b"at least one row" in lib.rq_last_error()
    assert lib.rq_delay_bank_create(h, rows, 1 << 14, 1 << 14, C.byref(out)) == -1 and b"2^28" in lib.rq_last_error()
    for value in (MAX + 1, 255):             # an entry above the maximum: the message names table and row
        rows[5] = value
        assert lib.rq_delay_bank_create(h, rows, 1, 8, C.byref(out)) == -1
        msg = lib.rq_last_error()
        assert b"above 16 steps" in msg and b"table 0, row 5 (%d)" % value in msg, msg
        assert lib.rq_delay_bank_create(h, rows, 4, 2, C.byref(out)) == -1 and b"table 2, row 1" in lib.rq_last_error()
    assert not out.value
    assert lib.rq_delay_bank_destroy(None) == 0
    ids = (C.c_uint32 * 1)(0)
    assert lib.rq_env_set_delay_schedule(None, h, ids) == -1 and b"null argument" in lib.rq_last_error()
    assert lib.rq_env_clear_delay_schedule(None) == -1 and b"null argument" in lib.rq_last_error()
    assert lib.rq_env_get_delay_schedule(None, C.byref(out), ids) == -1 and b"null argument" in lib.rq_last_error()
    assert lib.rq_env_get_delay_schedule(h, None, ids) == -1 and b"null argument" in lib.rq_last_error()


# ------------------------------------------------------------------ the rule ------
def deque_loop(actions, table, steps_before=0):
    """The rule, literally: per env a deque of the commands given so far in the episode; actions [K, N, 4] of one episode, table
    [rows] -> u [K, N, 4]"""
    K, N = actions.shape[:2]
    u = np.zeros_like(actions)
    for i in range(N):
        sent = collections.deque(maxlen=MAX + 1)
        for k in range(K):
            sent.append(actions[k, i])
            d = int(table[min(k, len(table) - 1)])
            if d <= k:
                u[k, i] = sent[len(sent) - 1 - d]
            # else: four +0.0f
    return u


def test_applied_is_the_deque_loop():
    from raptor_amd import delays
    g = np.random.default_rng(0)
    K, N = 40, 5
    a = g.uniform(-1.5, 1.5, (K, N, 4)).astype(np.float32)
    a[3, 1] = -0.0                            # bits, not values
    tables = {
        "d above k": np.array([5] * K, np.uint8),
        "sixteen": delays.constant(K, 16),
        "every row another": g.integers(0, 17, K).astype(np.uint8),
        "shorter than the episode": np.array([0, 3, 1, 2, 7], np.uint8),
        "none": delays.none(K),
        "dropout": delays.dropout(K, 4, 9),
    }
    for what, table in tables.items():
        d = table[np.minimum(np.arange(K), len(table) - 1)]
        want = deque_loop(a, table)
        got = delays.applied(a, np.broadcast_to(d[:, None], (K, N)))
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), what
        assert np.array_equal(bits(delays.applied(a[:, 0], d)), bits(want[:, 0])), what        # [K, 4] and [K]
    assert not delays.applied(a, np.full((K, N), 16))[:16].any() and np.array_equal(delays.applied(a, np.full((K, N), 16))[16:], a[:-16])
    assert np.array_equal(bits(delays.applied(a, np.zeros((K, N), np.int64))), bits(a))
    assert not np.signbit(delays.applied(-np.abs(a), np.full((K, N), 16))[:16]).any()          # a command older than the episode: +0.0
    for bad in (np.zeros((K, N)), -np.ones((K, N), np.int64), np.zeros((K,), np.int64)):
        with pytest.raises(ValueError):
            delays.applied(a, bad)


def test_applied_actions_follows_the_episodes_of_a_recording():
    from raptor_amd import delays
    g = np.random.default_rng(1)
    T, N = 30, 4
    act = g.uniform(-1, 1, (T, N, 4)).astype(np.float32)
    done = np.zeros((T, N), np.uint8)
    done[6, 0] = 1; done[11, 1] = 2; done[23, 1] = 2; done[9, 2] = 2; done[10:, 2] = 4          # env 2 freezes at its end; env 3 runs on
    tables = np.stack([delays.constant(12, 2), np.array([0, 1, 1, 3, 2, 2, 0, 4, 1, 1, 2, 5], np.uint8)])
    ids = np.array([0, 1, 1, 0])
    u = delays.applied_actions(dict(act=act, done=done), tables, ids)
    for i in range(N):
        start = 0
        while start < T and done[start, i] != 4:
            end = start
            while end < T - 1 and done[end, i] == 0:
                end += 1
            want = deque_loop(act[start:end + 1, i:i + 1], tables[ids[i]])[:, 0]
            assert np.array_equal(bits(u[start:end + 1, i]), bits(want)), (i, start)
            start = end + 1
        assert not u[start:, i].any()
    # a recording that begins mid-episode: the commands from before it are not in it
    late = delays.applied_actions(dict(act=act, done=np.zeros((T, N), np.uint8)), tables[:1], None, start_steps=np.full(N, 5))
    assert np.isnan(late[:2]).all() and np.array_equal(late[2:], act[:-2])


def test_table_builders_bounds_and_dtypes():
    from raptor_amd import delays
    assert delays.steps_for(0.010, 0.0025) == 4 and delays.steps_for(0.0, 0.01) == 0 and delays.steps_for(0.16, 0.01) == 16
    assert delays.steps_for(0.004, 0.01) == 0 and delays.steps_for(0.005, 0.01) == 1
    for bad in ((0.17, 0.01), (-0.01, 0.01), (0.01, 0.0), (np.nan, 0.01)):
        with pytest.raises(ValueError):
            delays.steps_for(*bad)
    rows = 40
    made = dict(delays.suite(rows), jitter=delays.jitter(rows, 2, 16, 3), dropout=delays.dropout(rows, 5, 16), onset=delays.onset(rows, 7, 16))
    assert list(delays.suite(rows)) == ["none", "constant_1", "constant_2", "constant_4", "constant_8", "jitter_0_3", "dropout_8", "onset_4"]
    for name, t in made.items():
        assert t.dtype == np.uint8 and t.shape == (rows,) and t.max() <= MAX, name
    assert not delays.none(rows).any() and (delays.constant(rows, 16) == 16).all()
    j = delays.jitter(1000, 2, 5, 3)
    assert set(j) == {2, 3, 4, 5} and np.array_equal(j, delays.jitter(1000, 2, 5, 3)) and not np.array_equal(j, delays.jitter(1000, 2, 5, 4))
    # a dropout holds the last command it got: d = 0, 1, .., length, then back to 0
    d = delays.dropout(rows, 5, 9)
    assert not d[:5].any() and np.array_equal(d[5:15], np.arange(10)) and not d[15:].any()
    a = np.arange(rows * 4, dtype=np.float32).reshape(rows, 4)
    held = delays.applied(a, d)
    assert (held[5:15] == a[5]).all() and np.array_equal(held[15:], a[15:]) and np.array_equal(held[:5], a[:5])
    assert np.array_equal(delays.dropout(8, 6, 5), [0, 0, 0, 0, 0, 0, 0, 1]) and not delays.dropout(8, 8, 5).any()        # cut at the table's end
    o = delays.onset(rows, 7, 3)
    assert not o[:7].any() and (o[7:] == 3).all()
    for call in (lambda: delays.constant(rows, 17), lambda: delays.constant(0, 1), lambda: delays.constant(rows, 1.5),
                 lambda: delays.jitter(rows, 3, 2, 0), lambda: delays.jitter(rows, 0, 17, 0), lambda: delays.jitter(rows, 0, 3, -1),
                 lambda: delays.dropout(rows, 3, 17), lambda: delays.dropout(rows, -1, 3), lambda: delays.onset(rows, 3, -1)):
        with pytest.raises(ValueError):
            call()


def test_python_checks_of_tables_and_ids():
    from raptor_amd import delays
    good = np.stack([delays.none(6), delays.constant(6, 16)])
    assert np.array_equal(delays.check_tables(good), good) and delays.check_tables(list(good)).shape == (2, 6)
    bad = good.copy()
    bad[1, 4] = 17
    with pytest.raises(ValueError, match=r"above 16 steps: table 1, row 4 \(17\)"):
        delays.check_tables(bad)
    for tables in (good.astype(np.float32), good[0], [], [good[0], good[0][:3]], good[:, :0], [good[0].astype(np.int64)]):
        with pytest.raises(ValueError):
            delays.check_tables(tables)
    assert delays.check_delay_ids([1, 0, 1], 2, 3).dtype == np.uint32
    with pytest.raises(ValueError, match="delay id out of range: env 2 names table 2 of a bank of 2"):
        delays.check_delay_ids([1, 0, 2], 2, 3)
    with pytest.raises(ValueError, match="one id per env"):
        delays.check_delay_ids([1, 0], 2, 3)


def test_python_refusals_come_before_any_library_call(monkeypatch):
    import raptor_amd.l2f as l2f
    from raptor_amd import _lib
    from raptor_amd.policy_bank import PolicyBank
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("a library call was made"))
    with pytest.raises(ValueError, match="above 16 steps"):
        l2f.DelayBank(None, np.full((1, 4), 17, np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        l2f.DelayBank(None, np.zeros((1, 4), np.float32))
    vector = l2f.VectorModule(4)
    env = vector.VectorEnvironment()
    with pytest.raises(ValueError, match="l2f.DelayBank"):
        env.set_delay_schedule(object())
    assert env.delay_schedule is None
    pb = PolicyBank.__new__(PolicyBank)
    pb.n_policies = 1
    with pytest.raises(ValueError, match="attach one first"):
        pb.evaluate(vector, None, env, None, None, None, 1, np.zeros(4, np.uint32), delay_ids=np.zeros(4, np.uint32))


# ------------------------------------------------------------------ the oracle loop: the specification ------
def oracle_delay_step(oracle, cfg, P, S, a, u):
    """One transition under the rule: the oracle's step computed from u, then the last-action columns overwritten with the actor's
    own command, clamp(a, -1, 1), or a under action_history_raw -> next state, reward, terminated"""
    ns, r, term = oracle.step(cfg, P, S, np.ascontiguousarray(u, np.float32))
    ns = np.array(ns)
    ns[:, S_LAST_ACTION] = a if cfg.action_history_raw else np.clip(a, np.float32(-1), np.float32(1))
    return ns, r, term


class History:
    """The host-held command history of n envs: what an env's ring holds, without its slots"""

    def __init__(self, n):
        self.sent = [[] for _ in range(n)]

    def command(self, a, k, d):
        """a [n, 4] the commands of this step, k [n] the episode step counts entering it, d [n] the delays -> u [n, 4]; the command
        is remembered under its step count (a count of 0 begins an episode: older commands are never reached again)"""
        u = np.zeros_like(a)
        for i in range(len(a)):
            if k[i] == 0:
                self.sent[i] = []
            assert len(self.sent[i]) == k[i]
            self.sent[i].append(a[i].copy())
            if d[i] <= k[i]:
                u[i] = self.sent[i][k[i] - d[i]]
        return u


def hover_world(oracle, n=6, raw=0):
    cfg = oracle.default_config()
    cfg.domain_randomization = 1
    cfg.termination_enabled = 0
    cfg.action_history_raw = raw
    P = oracle.sample_initial_parameters(cfg, 5, 0, 0, n)
    st = oracle.Stats(n)
    S = oracle.sample_initial_state(cfg, 5, st.episode, 0, P)
    return cfg, P, np.array(S)


@pytest.mark.parametrize("raw", [0, 1])
@pytest.mark.parametrize("d", [1, 3, 16])
def test_a_constant_delay_is_the_plain_trace_fed_zeros_first(oracle, d, raw):
    """constant(d) fed a_0, a_1, ... equals the plain step fed 0 x d, a_0, ... in columns 0..16, bit for bit; the last-action
    columns differ: they hold the actor's own command of the step, clamped unless raw"""
    cfg, P, S0 = hover_world(oracle, raw=raw)
    n, K = len(S0), 24
    a = np.random.default_rng(d).uniform(-1.5, 1.5, (K, n, 4)).astype(np.float32)
    fed = np.concatenate([np.zeros((d, n, 4), np.float32), a])[:K]
    hist = History(n)
    S, plain = S0.copy(), S0.copy()
    differ = 0
    for k in range(K):
        u = hist.command(a[k], np.full(n, k), np.full(n, d))
        assert np.array_equal(bits(u), bits(fed[k]))
        differ += int((bits(u).reshape(n, -1) != bits(a[k]).reshape(n, -1)).any(axis=1).sum())
        S, r, term = oracle_delay_step(oracle, cfg, P, S, a[k], u)
        plain, rp, tp = oracle.step(cfg, P, plain, fed[k])
        plain = np.array(plain)
        assert np.array_equal(bits(S[:, :17]), bits(plain[:, :17])) and np.array_equal(bits(r), bits(rp)) and np.array_equal(term, tp), k
        want = a[k] if raw else np.clip(a[k], -1, 1)
        assert np.array_equal(bits(S[:, S_LAST_ACTION]), bits(want)), k
        assert raw or (np.abs(S[:, S_LAST_ACTION]) <= 1).all()
        plain[:, S_LAST_ACTION] = S[:, S_LAST_ACTION]            # (what the next plain step reads of them: nothing the dynamics use)
    assert differ >= K * n // 2 and (np.abs(a) > 1).any()


def test_a_table_of_zeros_is_the_plain_step(oracle):
    from raptor_amd import delays
    cfg, P, S = hover_world(oracle)
    n = len(S)
    a = np.random.default_rng(2).uniform(-1.5, 1.5, (8, n, 4)).astype(np.float32)
    hist, plain = History(n), S.copy()
    for k in range(8):
        u = hist.command(a[k], np.full(n, k), delays.none(8)[np.full(n, k)])
        S, r, term = oracle_delay_step(oracle, cfg, P, S, a[k], u)
        plain = np.array(oracle.step(cfg, P, plain, a[k])[0])
        assert np.array_equal(bits(S), bits(plain)), k


# ------------------------------------------------------------------ the ring's owner ------
def test_the_command_history_against_a_counting_hip_stand_in(tmp_path):
    """rq::DelayHistory (raptor_amd/csrc/rq_env_schedule.hpp) with tests/delay_history_driver.cpp: the ring is allocated once, at the
    first attachment, and zeroed at every one - also after a detach, also for the bank already attached -; a failing allocation,
    zeroing or copy is returned and leaves bank, ids, generation and both banks' counts as they were; every block is freed exactly
    once - a stand-alone program under AddressSanitizer + UBSan (host code, no GPU)."""
    here = os.path.join(ROOT, "tests")
    exe = str(tmp_path / "delay_history_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", exe,
                    os.path.join(here, "delay_history_driver.cpp"), os.path.join(here, "fake_hip_memory.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
