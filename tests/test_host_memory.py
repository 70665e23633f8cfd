"""rq::DeviceBuffer / rq::PinnedBuffer (raptor_amd/csrc/rq_memory.hpp), the one owner of device and pinned memory in the C layer, on
the CPU: the header is compiled with a short driver (tests/host_memory_driver.cpp) against a stand-in for the five HIP entry
points it calls (tests/fake_hip_memory.cpp) that counts calls, logs their order and fails an allocation on request.  rq::CallMemory
(raptor_amd/csrc/rq_call_memory.hpp) the same way, with the four entry points more that it calls, and rq::EnvSchedule
(raptor_amd/csrc/rq_env_schedule.hpp), an env's slot per kind of schedule, with entry points both of them call."""
import os
import subprocess


def test_owning_buffers_against_a_counting_hip_stand_in(tmp_path):
    """Every allocation is freed exactly once when its owner goes; reserve() with room makes no call; growing a buffer that holds
    memory synchronises the stream before it frees, growing an empty one does not; the floor is honoured; a failed alloc / reserve
    leaves get() == nullptr and count() == 0 and nothing for the destructor to free; a moved-from buffer is empty; swap exchanges
    pointer and count - under AddressSanitizer + UBSan (host code, no GPU)."""
    _run_driver(tmp_path, "host_memory_driver.cpp")


def test_call_memory_against_a_counting_hip_stand_in(tmp_path):
    """rq::CallMemory (raptor_amd/csrc/rq_call_memory.hpp), the `memory` argument of the calls that read a recorded trajectory, with
    tests/call_memory_driver.cpp.  Per mode the exact calls: host memory - one upload per input, one download per output in the
    order they were named, then one synchronise; device memory - one synchronise; device memory, enqueued only - not one HIP call.
    The bytes arrive: an input is staged, an output comes back, the 2-D output writes the first n of ld columns of every row and
    leaves the caller's other columns (a sentinel) alone.  on_device is true for device memory of the call's ordinal only - false for
    host memory, for another ordinal and for a failing query, whose sticky error is taken - and asks nothing in a host-memory call.
    A copy that fails in finish() is returned with no copy and no synchronise after it.  valid: 0, 1, 2, not -1 or 3."""
    _run_driver(tmp_path, "call_memory_driver.cpp")


def test_env_schedule_slot_against_a_counting_hip_stand_in(tmp_path):
    """rq::EnvSchedule (raptor_amd/csrc/rq_env_schedule.hpp), the slot an env keeps per kind of schedule, with
    tests/env_schedule_driver.cpp.  A first attach makes exactly one device allocation, one upload and one synchronise, a later one
    no allocation; the uploaded first rows are id * rows below n and 0 up to ld, all 0 with null ids; the banks' `attached` counts
    follow attach, re-attach and detach, and detach leaves generation 0 and no ids; two attachments carry different non-zero
    generations; a failing allocation or copy is returned and leaves bank, ids, generation and both counts as they were; an env
    object that goes with three attached slots lets all three banks go; every block is freed exactly once."""
    _run_driver(tmp_path, "env_schedule_driver.cpp")


def _run_driver(tmp_path, driver):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / os.path.splitext(driver)[0])
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", exe,
                    os.path.join(here, driver), os.path.join(here, "fake_hip_memory.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
