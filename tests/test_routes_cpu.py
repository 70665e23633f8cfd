"""The two routes of the schedule kernels, without a GPU: which kernel flies a fused rollout (rq::route_fused,
raptor_amd/csrc/rq_fused_route.hpp) and which serves an env step (rq::route_env_step, raptor_amd/csrc/rq_step_launch.hpp), over the
whole grid of launch descriptions.  tests/route_driver.cpp includes the two headers alone under a plain host compiler and prints one
row per description; every row's expected answer is restated here by hand, not derived from the headers."""
import itertools
import os
import subprocess

import pytest

from conftest import ROOT

SCHEDULES = ("WRENCH", "VEHICLE", "WIND", "DELAY", "SENSOR")      # kind order


def _expected_fused(n, precision, sas, tracked, interval, actor, wrench, vehicle, wind, delay, sensor):
    """(family, build, vehicle kernel, wind kernel, delay kernel, sensor kernel) by hand, from the issues that added the schedules: a
    schedule's kernel flies fp32 policies and policy banks, tracked or not, at every interval, in the 512-register build up to 65 536
    envs and the 256-register one beyond; beside a bf16 / f16x2 policy, a SampleAndSquash stage or another schedule nothing is built.
    `family` is what the launch would be without a vehicle, wind, delay or sensor schedule (the vocabulary the route spoke when
    these rows were written; _new_vocabulary translates).  precision: 0 fp32, 1 bf16, 2 f16x2; actor: 0 a policy (native interval
    `interval`), 1 a bank at intervals all 1, 2 a bank with one interval above 1 (a bank's intervals are its own table: `interval`
    says nothing about it)."""
    fp32, bank = precision == 0, actor != 0
    unsupported = ("UNSUPPORTED", "-", 0, 0, 0, 0)
    if wrench and (not fp32 or sas):
        return unsupported
    if sas and (tracked or bank or interval > 1):
        return unsupported
    if bank and not fp32:
        return unsupported
    if vehicle and (not fp32 or sas or wrench):
        return unsupported
    if wind and (not fp32 or sas or wrench or vehicle):
        return unsupported
    if delay and (not fp32 or sas or wrench or vehicle or wind):
        return unsupported
    if sensor and (not fp32 or sas or wrench or vehicle or wind or delay):
        return unsupported
    if wrench:
        family = "WRENCH"
    elif bank:
        family = "BANK_RATE" if tracked or actor == 2 else "BANK"
    else:
        family = "RATE" if interval > 1 else "TRACK" if tracked else "PLAIN"
    if precision:
        return family, ("ActorBF16", "ActorF16X2")[precision - 1], 0, 0, 0, 0
    lean = (family == "PLAIN" and sas) or n > 65536
    return family, "ActorF32Lean" if lean else "ActorF32", vehicle, wind, delay, sensor


def _new_vocabulary(family, build, vk, wk, dk, sk):
    """(family, build) as the route says it now: the schedule's family where its flag was 1, the old family otherwise."""
    for flag, name in zip((vk, wk, dk, sk), SCHEDULES[1:]):
        if flag:
            return name, build
    return family, build


def _expected_step(rollout, bank, wrench, vehicle, mailbox, wind, delay, sensor):
    """The kernel of an env step and its template arguments, by hand: the outermost schedule attached names the kernel (delay > wind >
    vehicle > wrench), the ones inside it are its template bools; a policy's kernels take ROLLOUT first, a bank's are a rollout's in
    place, without host rows; a sensor schedule changes nothing."""
    if bank and (not rollout or mailbox):
        return "UNSUPPORTED"
    inner = [wrench, vehicle, wind, delay]
    if delay:
        kind, bools = "_delay", inner[:3]
    elif wind:
        kind, bools = "_wind", inner[:2]
    elif vehicle:
        kind, bools = "_vehicle", inner[:1]
    elif wrench:
        kind, bools = "_wrench", []
    else:
        kind, bools = "", []
    if bank:
        return "k_step_bank" + kind + ("<" + ", ".join(map(str, bools)) + ">" if bools else "")
    return "k_step" + kind + "<" + ", ".join(map(str, [rollout] + bools)) + ">"


def _kernel_of(supported, bank, rollout, wrench, vehicle, wind, delay, family):
    """The route's answer as launch_step (raptor_amd/csrc/rq_kernels.hip) reads it: the family's kernel - the bank's if `bank` - with
    `rollout` (a policy's kernels only) and the bools of the kinds nested inside the family as template arguments."""
    if not supported:
        return "UNSUPPORTED"
    nest = ("NONE", "WRENCH", "VEHICLE", "WIND", "DELAY")
    bools = [wrench, vehicle, wind, delay][:max(nest.index(family) - 1, 0)]
    kind = "" if family == "NONE" else "_" + family.lower()
    if bank:
        return "k_step_bank" + kind + ("<" + ", ".join(map(str, bools)) + ">" if bools else "")
    return "k_step" + kind + "<" + ", ".join(map(str, [rollout] + bools)) + ">"


def _compile(tmp_path, source, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "raptor_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", source)], check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    """(the driver's text, fused rows, step rows) of tests/route_driver.cpp, built and run once."""
    tmp_path = tmp_path_factory.mktemp("routes")
    r = subprocess.run([_compile(tmp_path, "route_driver.cpp", "route_driver")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    fused, step = {}, {}
    for line in r.stdout.splitlines():
        kind, *rest = line.split()
        if kind == "fused":
            *key, family, build = rest
            assert tuple(map(int, key)) not in fused, line
            fused[tuple(map(int, key))] = (family, build)
        else:
            assert kind == "step", line
            key, answer, family = rest[:8], rest[8:15], rest[15]
            assert tuple(map(int, key)) not in step, line
            step[tuple(map(int, key))] = tuple(map(int, answer)) + (family,)
    return r.stdout, fused, step


def test_the_fused_route_names_the_family_and_the_register_build_of_every_launch(routes):
    """The bit-exact GPU suites cannot see a wrong pick between the 512- and the 256-register fp32 build - the arithmetic is the
    same, only speed is lost - so the whole grid is held here: 5 batch sizes (both sides of 65 536) x 3 precisions x SampleAndSquash x
    tracked x interval 1 / 2 x (policy, bank, rated bank) x wrench x vehicle x wind x delay x sensor = 11 520 rows; every row, the
    unsupported ones included, must be _expected_fused's in the route's vocabulary."""
    _, fused, _ = routes
    grid = list(itertools.product((1, 64, 65536, 65537, 70001), (0, 1, 2), (0, 1), (0, 1), (1, 2), (0, 1, 2),
                                  (0, 1), (0, 1), (0, 1), (0, 1), (0, 1)))
    assert len(grid) == 11520 and sorted(fused) == sorted(grid)
    wrong = [(k, fused[k], _new_vocabulary(*_expected_fused(*k))) for k in grid if fused[k] != _new_vocabulary(*_expected_fused(*k))]
    assert not wrong, wrong[:10]
    # the grid reaches every family and every build, and both fp32 builds on either side of the threshold
    assert {f for f, _ in fused.values()} == {"UNSUPPORTED", "PLAIN", "TRACK", "RATE", "BANK", "BANK_RATE", *SCHEDULES}
    assert {b for _, b in fused.values()} == {"-", "ActorF32", "ActorF32Lean", "ActorBF16", "ActorF16X2"}
    none = (0, 0, 0, 0, 0)
    assert fused[(65536, 0, 0, 0, 1, 0) + none] == ("PLAIN", "ActorF32") and fused[(65537, 0, 0, 0, 1, 0) + none] == ("PLAIN", "ActorF32Lean")
    assert fused[(64, 1, 0, 0, 1, 0) + none] == ("PLAIN", "ActorBF16")                                # without a schedule: as before
    # a few rows by hand, per schedule (the one-hot tuple is wrench, vehicle, wind, delay, sensor)
    for kind, family in enumerate(SCHEDULES[1:], start=1):
        only = tuple(int(j == kind) for j in range(5))
        assert fused[(64, 0, 0, 0, 1, 0) + only] == (family, "ActorF32")                              # rq_rollout, fp32, the schedule
        assert fused[(65536, 0, 0, 1, 1, 0) + only] == (family, "ActorF32")                           # the 512-register build up to 65 536
        assert fused[(65537, 0, 0, 1, 2, 2) + only] == (family, "ActorF32Lean")                       # a rated bank, tracked, beyond
        assert fused[(64, 0, 0, 0, 1, 1) + only] == (family, "ActorF32")                              # an fp32 bank
        assert fused[(64, 0, 0, 0, 2, 0) + only] == (family, "ActorF32")                              # a native interval above 1
        assert fused[(64, 1, 0, 0, 1, 0) + only] == ("UNSUPPORTED", "-")                              # bf16
        assert fused[(64, 2, 0, 0, 1, 0) + only] == ("UNSUPPORTED", "-")                              # f16x2
        assert fused[(64, 0, 1, 0, 1, 0) + only] == ("UNSUPPORTED", "-")                              # SampleAndSquash
        for other in range(5):                                                                        # the schedule + another schedule
            if other != kind:
                both = tuple(int(j in (kind, other)) for j in range(5))
                assert fused[(64, 0, 0, 0, 1, 0) + both] == ("UNSUPPORTED", "-")
    assert fused[(64, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)] == ("DELAY", "ActorF32")                         # without sensor: as before
    assert fused[(64, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0)] == ("WIND", "ActorF32")                          # without delay: as before
    assert fused[(64, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0)] == ("VEHICLE", "ActorF32")                       # without wind: as before
    assert fused[(64, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0)] == ("WRENCH", "ActorF32")


def test_the_step_route_names_the_kernel_of_every_env_step(routes):
    """The env step's kernel for rollout x bank x wrench x vehicle x host rows x wind x delay x sensor, 256 rows (a teacher bank's
    chained step is the row rollout, no bank): the kernel the route's answer names and its template arguments are _expected_step's,
    what the route says is attached is what is attached, and a sensor schedule changes no row."""
    _, _, step = routes
    sgrid = list(itertools.product((0, 1), repeat=8))
    assert sorted(step) == sorted(sgrid)
    wrong = [(k, step[k], _expected_step(*k)) for k in sgrid if _kernel_of(*step[k]) != _expected_step(*k)]
    assert not wrong, wrong[:10]
    for k in sgrid:
        rollout, bank, wrench, vehicle, mailbox, wind, delay, sensor = k
        assert step[k] == step[k[:7] + (0,)], k               # unchanged by a sensor schedule: the row with it is the row without it
        if step[k][0]:
            assert step[k][1:7] == (bank, rollout, wrench, vehicle, wind, delay), k
    kernel = {k: _kernel_of(*v) for k, v in step.items()}
    # a few rows by hand
    assert kernel[(0, 0, 0, 0, 0, 0, 0, 0)] == "k_step<0>"
    assert kernel[(0, 0, 0, 0, 1, 0, 0, 1)] == "k_step<0>"                          # rq_step with host rows: k_step
    assert kernel[(0, 0, 0, 1, 1, 0, 0, 0)] == "k_step_vehicle<0, 0>"               # rq_step with host rows
    assert kernel[(1, 0, 1, 1, 0, 0, 0, 0)] == "k_step_vehicle<1, 1>"               # a chained rollout, both schedules
    assert kernel[(1, 1, 0, 1, 0, 0, 0, 0)] == "k_step_bank_vehicle<0>"
    assert kernel[(1, 1, 1, 0, 0, 0, 0, 0)] == "k_step_bank_wrench"
    assert kernel[(0, 0, 0, 0, 1, 1, 0, 0)] == "k_step_wind<0, 0, 0>"               # rq_step with host rows: k_step_wind<0, 0, 0>
    assert kernel[(1, 0, 1, 1, 0, 1, 0, 0)] == "k_step_wind<1, 1, 1>"               # all three: k_step_wind<1, 1, 1>
    assert kernel[(1, 1, 1, 0, 0, 1, 0, 0)] == "k_step_bank_wind<1, 0>"             # k_step_bank_wind<1, 0>
    assert kernel[(0, 1, 0, 0, 0, 1, 0, 0)] == "UNSUPPORTED"
    assert kernel[(0, 0, 0, 0, 1, 0, 1, 0)] == "k_step_delay<0, 0, 0, 0>"           # rq_step with host rows: k_step_delay<0, 0, 0, 0>
    assert kernel[(1, 0, 1, 1, 0, 1, 1, 0)] == "k_step_delay<1, 1, 1, 1>"           # all four: k_step_delay<1, 1, 1, 1>
    assert kernel[(1, 1, 1, 0, 0, 0, 1, 0)] == "k_step_bank_delay<1, 0, 0>"         # k_step_bank_delay<1, 0, 0>
    assert kernel[(0, 1, 0, 0, 0, 0, 1, 0)] == "UNSUPPORTED"
    assert kernel[(1, 0, 1, 1, 0, 1, 1, 1)] == "k_step_delay<1, 1, 1, 1>"           # all five: k_step_delay<1, 1, 1, 1>
    assert step[(1, 0, 1, 1, 0, 1, 1, 1)] == (1, 0, 1, 1, 1, 1, 1, "DELAY")


def test_the_route_headers_stand_alone_and_the_driver_is_clean_under_the_sanitizers(routes, tmp_path):
    """The drivers that switch over the routes' enums without a default compile under -Wall -Werror; tests/route_driver.cpp built a
    second time as a stand-alone program with -fsanitize=address,undefined (the sanitizers' runtimes linked into the program itself:
    it needs nothing from the environment it is started in) prints the same text and reports nothing."""
    text, _, _ = routes
    _compile(tmp_path, "actor_step_route_driver.cpp", "actor_step_route_driver")
    san = _compile(tmp_path, "route_driver.cpp", "route_driver_san",
                   ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan",
                    "-static-libubsan"))
    s = subprocess.run([san], capture_output=True, text=True)
    assert s.returncode == 0 and s.stderr == "", s.stderr[-2000:]
    assert s.stdout == text
