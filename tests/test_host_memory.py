"""rq::DeviceBuffer / rq::PinnedBuffer (raptor_amd/csrc/rq_memory.hpp), the one owner of device and pinned memory in the C layer, on
the CPU: the header is compiled with a short driver (tests/host_memory_driver.cpp) against a stand-in for the five HIP entry
points it calls (tests/fake_hip_memory.cpp) that counts calls, logs their order and fails an allocation on request."""
import os
import subprocess


def test_owning_buffers_against_a_counting_hip_stand_in(tmp_path):
    """Every allocation is freed exactly once when its owner goes; reserve() with room makes no call; growing a buffer that holds
    memory synchronises the stream before it frees, growing an empty one does not; the floor is honoured; a failed alloc / reserve
    leaves get() == nullptr and count() == 0 and nothing for the destructor to free; a moved-from buffer is empty; swap exchanges
    pointer and count - under AddressSanitizer + UBSan (host code, no GPU)."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "host_memory")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", exe,
                    os.path.join(here, "host_memory_driver.cpp"), os.path.join(here, "fake_hip_memory.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
