"""The sensor schedule without a GPU: the entry points and what they refuse before the device is looked at, raptor_amd.sensors (the
rule against a brute-force loop over (k, env), the table builders, the checks, every message as a literal), the host queue that is the
specification the GPU suite reuses (tests/test_gpu_sensor.py imports it from here) and the owner of the env's two rings (tests/sensor_history_driver.cpp on
tests/fake_hip_memory, a stand-alone program under the address and undefined-behaviour sanitizers)."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ("rq_sensor_bank_create", "rq_sensor_bank_destroy", "rq_env_set_sensor_schedule", "rq_env_clear_sensor_schedule",
       "rq_env_get_sensor_schedule")
MAX = 16
READING = 18                                 # columns 0..17: position, rotation matrix, linear and angular velocity


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def test_entry_points_are_declared_bound_and_exported():
    from raptor_amd import _lib, sensors
    import raptor_amd.l2f as l2f
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
    assert int(re.search(r"#define RQ_SENSOR_MAX_STEPS (\d+)", hdr).group(1)) == MAX == sensors.MAX_STEPS
    assert re.search(r"still 5: rq_sensor_bank_\{create,destroy\}", hdr) and "Sensor schedule" in hdr
    assert "SensorBank" in l2f.__all__ and sensors.READING_COLUMNS == READING
    # the declarations were appended: behind the delay schedule's
    assert hdr.index("rq_env_get_delay_schedule(") < hdr.index("rq_sensor_bank_create(")


def test_what_needs_no_device_is_refused_first():
    import ctypes as C
    from raptor_amd import _lib
    lib = _lib.load()
    h = C.c_void_p(4096)                     # never followed: everything below is refused before the device is looked at
    rows = (C.c_uint8 * 8)(*([1] * 8))
    out = C.c_void_p()
    for args in ((None, rows, 1, 1, C.byref(out)), (h, None, 1, 1, C.byref(out)), (h, rows, 1, 1, None)):
        assert lib.rq_sensor_bank_create(*args) == -1
        assert lib.rq_last_error() == b"rq_sensor_bank_create: null argument"
    assert lib.rq_sensor_bank_create(h, rows, 0, 1, C.byref(out)) == -1
    assert lib.rq_last_error() == b"rq_sensor_bank_create: a sensor bank needs at least one table of at least one row"
    assert lib.rq_sensor_bank_create(h, rows, 1, 0, C.byref(out)) == -1
    assert lib.rq_last_error() == b"rq_sensor_bank_create: a sensor bank needs at least one table of at least one row"
    assert lib.rq_sensor_bank_create(h, rows, 1 << 14, 1 << 14, C.byref(out)) == -1
    assert lib.rq_last_error() == b"rq_sensor_bank_create: a sensor bank holds fewer than 2^28 rows in all"
    for value in (MAX + 1, 255):             # an entry above the maximum: the message names table and row
        rows[5] = value
        assert lib.rq_sensor_bank_create(h, rows, 1, 8, C.byref(out)) == -1
        assert lib.rq_last_error() == b"rq_sensor_bank_create: sensor bank holds a delay above 16 steps: table 0, row 5 (%d)" % value
        assert lib.rq_sensor_bank_create(h, rows, 4, 2, C.byref(out)) == -1
        assert lib.rq_last_error() == b"rq_sensor_bank_create: sensor bank holds a delay above 16 steps: table 2, row 1 (%d)" % value
    # the delay bank's words, with "delay" for "sensor"
    assert lib.rq_delay_bank_create(h, rows, 1, 8, C.byref(out)) == -1
    assert lib.rq_last_error() == b"rq_delay_bank_create: delay bank holds a delay above 16 steps: table 0, row 5 (255)"
    assert not out.value
    assert lib.rq_sensor_bank_destroy(None) == 0
    ids = (C.c_uint32 * 1)(0)
    assert lib.rq_env_set_sensor_schedule(None, h, ids) == -1 and lib.rq_last_error() == b"rq_env_set_sensor_schedule: null argument"
    assert lib.rq_env_clear_sensor_schedule(None) == -1 and lib.rq_last_error() == b"rq_env_clear_sensor_schedule: null argument"
    assert lib.rq_env_get_sensor_schedule(None, C.byref(out), ids) == -1 and lib.rq_last_error() == b"rq_env_get_sensor_schedule: null argument"
    assert lib.rq_env_get_sensor_schedule(h, None, ids) == -1 and lib.rq_last_error() == b"rq_env_get_sensor_schedule: null argument"


# ------------------------------------------------------------------ the rule ------
def brute_force(readings, d):
    """The rule, literally, one (k, env) at a time: readings [K, N, C] of one episode, d [K, N] -> delivered [K, N, C]"""
    K, N, Cn = readings.shape
    out = np.empty_like(readings)
    for k in range(K):
        for i in range(N):
            dp = min(int(d[k, i]), k)
            for c in range(Cn):
                out[k, i, c] = readings[k - dp, i, c] if c < READING else readings[k, i, c]
    return out


class Queue:
    """The host-held readings of n envs: what an env's ring holds, without its slots.  observe(z, k, d): z [n, C >= 18] the
    observations assembled at this step without a schedule, k [n] the episode step counts, d [n] the table's delays -> what the policy
    sees; a count of 0 begins an episode (older readings are never reached again); observing twice at one count rewrites the reading;
    ``skip`` [n] bool: envs whose observation is passed through and not remembered (frozen)."""

    def __init__(self, n):
        self.seen = [[] for _ in range(n)]

    def observe(self, z, k, d, skip=None):
        out = np.array(z)
        for i in range(len(z)):
            if skip is not None and skip[i]:
                continue
            if k[i] == 0:
                self.seen[i] = []
            assert len(self.seen[i]) in (k[i], k[i] + 1), (i, len(self.seen[i]), k[i])
            del self.seen[i][k[i]:]
            self.seen[i].append(z[i, :READING].copy())
            out[i, :READING] = self.seen[i][k[i] - min(int(d[i]), int(k[i]))]
        return out


def test_delivered_is_the_brute_force_loop():
    from raptor_amd import sensors
    g = np.random.default_rng(0)
    K, N = 40, 5
    for Cn in (18, 22, 26):
        z = g.uniform(-1.5, 1.5, (K, N, Cn)).astype(np.float32)
        z[3, 1] = -0.0                            # bits, not values
        z[7, 2, 4] = np.nan
        tables = {
            "d = 0": sensors.none(K),
            "d above k: the first reading held": np.array([5] * K, np.uint8),
            "sixteen": sensors.constant(K, 16),
            "every row another": g.integers(0, 17, K).astype(np.uint8),
            "shorter than the episode": np.array([0, 3, 1, 2, 7], np.uint8),
            "low rate": sensors.low_rate(K, 4),
        }
        for what, table in tables.items():
            d = np.broadcast_to(table[np.minimum(np.arange(K), len(table) - 1)][:, None], (K, N))
            want = brute_force(z, d)
            got = sensors.delivered(z, d)
            assert got.dtype == np.float32 and got.shape == z.shape and np.array_equal(bits(got), bits(want)), (what, Cn)
            assert np.array_equal(bits(sensors.delivered(z[:, 0], d[:, 0])), bits(want[:, 0])), what        # [K, C] and [K]
            q = Queue(N)
            for k in range(K):                    # ... and the queue the GPU suite holds the kernels to
                assert np.array_equal(bits(q.observe(z[k], np.full(N, k), d[k])), bits(want[k])), (what, k)
        per_env = g.integers(0, 17, (K, N))       # another delay per env and step
        assert np.array_equal(bits(sensors.delivered(z, per_env)), bits(brute_force(z, per_env)))
        held = sensors.delivered(z, np.full((K, N), 16))
        assert np.array_equal(bits(held[:17, :, :READING]), bits(np.broadcast_to(z[0, :, :READING], (17, N, READING))))
        assert np.array_equal(bits(held[16:, :, :READING]), bits(z[:-16, :, :READING]))
        assert np.array_equal(bits(held[..., READING:]), bits(z[..., READING:]))           # columns from 18 on pass through
        assert np.array_equal(bits(sensors.delivered(z, np.zeros((K, N), np.int64))), bits(z))
    for bad, message in ((np.zeros((K, N)), "a delay is a non-negative whole number of steps"),
                         (-np.ones((K, N), np.int64), "a delay is a non-negative whole number of steps"),
                         (np.zeros((K, N), bool), "a delay is a non-negative whole number of steps"),
                         (np.zeros((K,), np.int64), "delivered takes readings [K, ..., C >= 18] and a delay per step [K, ...]; got (40, 5, 26) and (40,)")):
        with pytest.raises(ValueError) as e:
            sensors.delivered(z, bad)
        assert str(e.value) == message
    with pytest.raises(ValueError) as e:
        sensors.delivered(z[..., :17], np.zeros((K, N), np.int64))
    assert str(e.value) == "delivered takes readings [K, ..., C >= 18] and a delay per step [K, ...]; got (40, 5, 17) and (40, 5)"


def test_table_builders_bounds_and_dtypes():
    from raptor_amd import sensors
    assert sensors.steps_for(0.010, 0.0025) == 4 and sensors.steps_for(0.0, 0.01) == 0 and sensors.steps_for(0.16, 0.01) == 16
    assert sensors.steps_for(0.004, 0.01) == 0 and sensors.steps_for(0.005, 0.01) == 1
    with pytest.raises(ValueError) as e:
        sensors.steps_for(0.17, 0.01)
    assert str(e.value) == "0.17 s at dt = 0.01 s are 17 steps: a sensor schedule holds at most 16"
    for bad in ((-0.01, 0.01), (0.01, 0.0), (np.nan, 0.01)):
        with pytest.raises(ValueError) as e:
            sensors.steps_for(*bad)
        assert str(e.value) == "seconds must be non-negative and dt positive"
    rows = 40
    made = dict(sensors.suite(rows), jitter=sensors.jitter(rows, 2, 16, 3), dropout=sensors.dropout(rows, 5, 16),
                onset=sensors.onset(rows, 7, 16), low_rate=sensors.low_rate(rows, 17))
    assert list(sensors.suite(rows)) == ["none", "constant_1", "constant_2", "constant_4", "constant_8", "jitter_0_3", "low_rate_4",
                                         "dropout_8", "onset_4"]
    for name, t in made.items():
        assert t.dtype == np.uint8 and t.shape == (rows,) and t.max() <= MAX, name
    assert np.array_equal(sensors.check_tables(list(sensors.suite(rows).values())), np.stack(list(sensors.suite(rows).values())))
    assert not sensors.none(rows).any() and (sensors.constant(rows, 16) == 16).all()
    j = sensors.jitter(1000, 2, 5, 3)
    assert set(j) == {2, 3, 4, 5} and np.array_equal(j, sensors.jitter(1000, 2, 5, 3)) and not np.array_equal(j, sensors.jitter(1000, 2, 5, 4))
    # a sensor at a quarter of the control rate: refreshed at every fourth step, held between
    lr = sensors.low_rate(rows, 4)
    assert np.array_equal(lr, np.arange(rows) % 4) and not sensors.low_rate(rows, 1).any() and sensors.low_rate(rows, 17).max() == 16
    z = np.arange(rows * READING, dtype=np.float32).reshape(rows, READING)
    assert np.array_equal(sensors.delivered(z, lr), z[(np.arange(rows) // 4) * 4])
    # a dropout holds the last reading it got: d = 0, 1, .., length, then back to 0
    d = sensors.dropout(rows, 5, 9)
    assert not d[:5].any() and np.array_equal(d[5:15], np.arange(10)) and not d[15:].any()
    held = sensors.delivered(z, d)
    assert (held[5:15] == z[5]).all() and np.array_equal(held[15:], z[15:]) and np.array_equal(held[:5], z[:5])
    assert np.array_equal(sensors.dropout(8, 6, 5), [0, 0, 0, 0, 0, 0, 0, 1]) and not sensors.dropout(8, 8, 5).any()        # cut at the table's end
    o = sensors.onset(rows, 7, 3)
    assert not o[:7].any() and (o[7:] == 3).all()
    refused = (
        (lambda: sensors.constant(rows, 17), "d is a whole number of steps in [0, 16]; got 17"),
        (lambda: sensors.constant(0, 1), "rows must be a positive integer"),
        (lambda: sensors.constant(rows, 1.5), "d is a whole number of steps in [0, 16]; got 1.5"),
        (lambda: sensors.jitter(rows, 3, 2, 0), "lo must not exceed hi"),
        (lambda: sensors.jitter(rows, 0, 17, 0), "hi is a whole number of steps in [0, 16]; got 17"),
        (lambda: sensors.jitter(rows, 0, 3, -1), "seed must be a non-negative integer"),
        (lambda: sensors.low_rate(rows, 0), "period is a whole number of steps in [1, 17]; got 0"),
        (lambda: sensors.low_rate(rows, 18), "period is a whole number of steps in [1, 17]; got 18"),
        (lambda: sensors.low_rate(rows, 2.5), "period is a whole number of steps in [1, 17]; got 2.5"),
        (lambda: sensors.dropout(rows, 3, 17), "length is a whole number of steps in [0, 16]; got 17"),
        (lambda: sensors.dropout(rows, -1, 3), "start is a non-negative step count"),
        (lambda: sensors.onset(rows, 3, -1), "d is a whole number of steps in [0, 16]; got -1"),
    )
    for call, message in refused:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == message


def test_python_checks_of_tables_and_ids():
    from raptor_amd import schedules, sensors
    good = np.stack([sensors.none(6), sensors.constant(6, 16)])
    assert np.array_equal(sensors.check_tables(good), good) and sensors.check_tables(list(good)).shape == (2, 6)
    assert np.array_equal(sensors.check_table(good[1]), good[1])
    bad = good.copy()
    bad[1, 4] = 17
    refused = (
        (bad, "a sensor table holds a delay above 16 steps: table 1, row 4 (17)"),
        (good.astype(np.float32), "a sensor bank is a uint8 NumPy array [M, rows] or a list of M [rows] tables"),
        (good[0], "a sensor bank has shape [M >= 1, rows >= 1]; got (6,)"),
        ([], "a sensor bank holds at least one table"),
        ([good[0], good[0][:3]], "the tables of a sensor bank have the same number of rows; got 6, 3"),
        (good[:, :0], "a sensor bank has shape [M >= 1, rows >= 1]; got (2, 0)"),
        ([good[0].astype(np.int64)], "a sensor table is a uint8 NumPy array [rows] (raptor_amd.sensors builds them)"),
        ([good], "a sensor table has shape [rows >= 1]: the delay in steps; got (2, 6)"),
    )
    for tables, message in refused:
        with pytest.raises(ValueError) as e:
            sensors.check_tables(tables)
        assert str(e.value) == message
    assert sensors.check_sensor_ids([1, 0, 1], 2, 3).dtype == np.uint32
    for ids, message in (([1, 0, 2], "sensor id out of range: env 2 names table 2 of a bank of 2"),
                         ([1, 0], "sensor ids must hold one id per env: 2 ids for 3 envs"),
                         ([1.0, 0.0, 0.0], "sensor ids must be integers")):
        with pytest.raises(ValueError) as e:
            sensors.check_sensor_ids(ids, 2, 3)
        assert str(e.value) == message
    # the kind: appended to the schedules, behind the delay schedule as in the C layer's walk
    assert schedules.KINDS[-1] is schedules.SENSOR and schedules.KINDS[-2] is schedules.DELAY and len(schedules.KINDS) == 5
    assert schedules.SENSOR.noun == "sensor" and schedules.SENSOR.scenario == "sensor" and schedules.SENSOR.builder == "raptor_amd.sensors"
    assert schedules.SENSOR.beside == ("sensor_ids group the tracking error by sensor scenario, wrench_ids by disturbance, vehicle_ids by "
                                       "vehicle scenario, wind_ids by wind scenario and delay_ids by latency scenario: give one of them")


def test_python_refusals_come_before_any_library_call(monkeypatch):
    import raptor_amd.l2f as l2f
    from raptor_amd import _lib
    from raptor_amd.policy_bank import PolicyBank
    from raptor_amd.teachers import TeacherBank
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("a library call was made"))
    with pytest.raises(ValueError) as e:
        l2f.SensorBank(None, np.full((1, 4), 17, np.uint8))
    assert str(e.value) == "a sensor table holds a delay above 16 steps: table 0, row 0 (17)"
    with pytest.raises(ValueError) as e:
        l2f.SensorBank(None, np.zeros((1, 4), np.float32))
    assert str(e.value) == "a sensor bank is a uint8 NumPy array [M, rows] or a list of M [rows] tables"
    vector = l2f.VectorModule(4)
    env = vector.VectorEnvironment()
    with pytest.raises(ValueError) as e:
        env.set_sensor_schedule(object())
    assert str(e.value) == "bank must be an l2f.SensorBank (clear_sensor_schedule() detaches)"
    assert env.sensor_schedule is None
    pb = PolicyBank.__new__(PolicyBank)
    pb.n_policies = 1
    with pytest.raises(ValueError) as e:
        pb.evaluate(vector, None, env, None, None, None, 1, np.zeros(4, np.uint32), sensor_ids=np.zeros(4, np.uint32))
    assert str(e.value) == "sensor_ids name tables of the env's sensor schedule: attach one first (env.set_sensor_schedule(bank))"
    tb = TeacherBank.__new__(TeacherBank)
    tb.n_teachers = 1
    with pytest.raises(ValueError) as e:
        tb.closed_loop(vector, None, env, None, None, None, 1, np.zeros(4, np.uint32), sensor_ids=np.zeros(4, np.uint32))
    assert str(e.value) == "sensor_ids name tables of the env's sensor schedule: attach one first (env.set_sensor_schedule(bank))"


# ------------------------------------------------------------------ the rings' owner ------
def test_the_two_histories_against_a_counting_hip_stand_in(tmp_path):
    """The env's command history and its readings are two rq::DelayHistory (raptor_amd/csrc/rq_env_schedule.hpp) beside two schedule
    slots; tests/sensor_history_driver.cpp: each ring is allocated once, at its kind's first attachment, with its own size, and
    zeroed at every attachment of its kind and at no attachment of the other; a failing allocation, zeroing or copy is returned and
    leaves both slots, both rings and every bank's count as they were; every block is freed exactly once - a stand-alone program
    under AddressSanitizer + UBSan (host code, no GPU)."""
    here = os.path.join(ROOT, "tests")
    exe = str(tmp_path / "sensor_history_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", exe,
                    os.path.join(here, "sensor_history_driver.cpp"), os.path.join(here, "fake_hip_memory.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
