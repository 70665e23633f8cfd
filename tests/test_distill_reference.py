"""The float64 helpers of the distillation tests against torch (tests/distill_reference.py), and the gather tables of the device-side
repack (csrc/rq_pack.cpp pack_gather_table) against the host packers - no GPU needed."""
import os
import subprocess

import numpy as np
import pytest

import distill_reference as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_helper_equals_torch_over_fifty_steps(wd):
    import torch
    rng = np.random.default_rng(3)
    w0 = rng.standard_normal(2084)
    wt = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
    cls = torch.optim.AdamW if wd else torch.optim.Adam
    kw = dict(weight_decay=wd) if wd else {}
    opt = cls([wt], lr=2e-3, betas=(0.9, 0.999), eps=1e-8, **kw)
    ref = D.Adam(w0, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    for k in range(50):
        g = rng.standard_normal(2084) * 10.0 ** rng.integers(-6, 2)
        wt.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        w = ref.step(g)
        assert np.abs(w - wt.detach().numpy()).max() <= 1e-12 * np.abs(w).max(), k


def test_masked_mse_helper_equals_training_masked_mse_through_autograd():
    import torch
    from raptor_amd.training import masked_mse
    rng = np.random.default_rng(4)
    T, n = 7, 9
    act = rng.standard_normal((T, 4, n))
    target = rng.standard_normal((T, 4, n))
    live = np.broadcast_to((rng.random((T, 1, n)) > 0.3), (T, 4, n)).copy()
    act[~live] = np.nan
    target[~live] = np.nan
    at = torch.tensor(act, dtype=torch.float64, requires_grad=True)
    loss = masked_mse(at, torch.tensor(target, dtype=torch.float64), torch.tensor(live))
    loss.backward()
    ref_loss, ref_seed, _ = D.masked_mse(act, target, live)
    assert abs(float(loss.detach()) - ref_loss) <= 1e-14 * abs(ref_loss)
    assert np.isfinite(ref_seed).all() and not ref_seed[~live].any()
    assert np.abs(at.grad.numpy() - ref_seed).max() <= 1e-15
    none = np.zeros_like(live)
    assert D.masked_mse(act, target, none)[0] == 0.0 and not D.masked_mse(act, target, none)[1].any()


PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "rq_kernels.hpp"
int main(int argc, char** argv) {
    const size_t nf = rq::RQ_PACKED_FLOATS, ng = rq::RQ_PACKED_GRAD_FLOATS;
    std::vector<rq::PackGather> table(nf + ng);
    rq::pack_gather_table(table.data());
    std::mt19937 gen(7);
    std::normal_distribution<float> draw(0.0f, 1.0f);
    std::vector<float> w(RQ_POLICY_NUM_WEIGHTS), image(nf + ng), mine(nf + ng);
    for (int round = 0; round < 4; ++round) {
        for (auto& x : w) x = draw(gen) * (round == 3 ? 1e-30f : 1.0f);
        rq::pack_policy(w.data(), image.data());
        rq::pack_policy_grad(w.data(), image.data() + nf);
        for (size_t e = 0; e < nf + ng; ++e) {
            const rq::PackGather t = table[e];
            float x = 0.0f;
            if (t.a != rq::PACK_GATHER_NONE) {
                x = w[t.a];
                if (t.b != rq::PACK_GATHER_NONE) x = x + w[t.b];
                x = t.k * x;
            }
            mine[e] = x;
        }
        if (std::memcmp(mine.data(), image.data(), (nf + ng) * sizeof(float)) != 0) { std::printf("MISMATCH round %d\n", round); return 1; }
    }
    FILE* f = std::fopen(argv[1], "wb");
    std::fwrite(table.data(), sizeof(rq::PackGather), nf + ng, f);
    std::fclose(f);
    std::printf("OK %zu %zu %zu\n", nf, ng, sizeof(rq::PackGather));
    return 0;
}
"""


def test_gather_tables_reproduce_both_host_images_bit_for_bit(tmp_path):
    """pack_gather_table against pack_policy and pack_policy_grad in a host program built from csrc/rq_pack.cpp (the transposed
    image has no entry point of its own), then the forward table, applied in NumPy, against rq_policy_pack_image."""
    import ctypes as C
    from raptor_amd import _lib
    from raptor_amd.build import _hipcc
    csrc = os.path.join(ROOT, "raptor_amd", "csrc")
    src, exe, out = tmp_path / "gather.cpp", tmp_path / "gather", tmp_path / "table.bin"
    src.write_text(PROGRAM)
    rocm_include = os.path.join(os.path.dirname(os.path.realpath(_hipcc())), "..", "include")      # hip_runtime_api.h: types only
    r = subprocess.run([_hipcc(), "-x", "c++", "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", csrc, "-I", rocm_include, str(src),
                        os.path.join(csrc, "rq_pack.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    nf, ng, size = (int(x) for x in r.stdout.split()[1:4])
    assert size == 8
    table = np.fromfile(out, dtype=np.dtype([("a", "<u2"), ("b", "<u2"), ("k", "<f4")]))
    assert table.size == nf + ng
    used = set(table["a"][table["a"] != 0xFFFF].tolist()) | set(table["b"][table["b"] != 0xFFFF].tolist())
    assert used == set(range(2084))                              # every weight reaches the forward image
    assert (table["b"][nf:] == 0xFFFF).all() and (table["k"][nf:] == 1.0).all()      # the transposed image: plain weights
    w = np.random.default_rng(5).standard_normal(2084).astype(np.float32)
    image = np.empty(nf, np.float32)
    floats = C.c_size_t()
    _lib.call("rq_policy_pack_image", _lib.fptr(w), w.size, _lib.POLICY_FP32, _lib.fptr(image), image.size, C.byref(floats))
    assert floats.value == nf
    assert np.array_equal(D.apply_gather(table[:nf], w).view(np.uint32), image.view(np.uint32))
