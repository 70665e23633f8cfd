// flight_table_sweep.hip - how the flight table's prefetch depth and workgroup size were chosen: the kernel text of the library
// (raptor_amd/csrc/rq_flight_table.inc) compiled once per (depth, workgroup) pair into one stand-alone program, every variant run
// on the same synthetic recording, timed with device events, alternating, medians over --rounds rounds, and held to the first
// variant's output bit for bit (depth and workgroup size must not change a bit).
//
//   hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 tools/flight_table_sweep.hip -o flight_table_sweep
//   ./flight_table_sweep [envs 65536] [steps 500] [buckets 10] [rounds 5]
//
// The recording is generated on the device from a hash: observations, actions and rewards uniform in [-1.25, 1.25], an episode end
// (code 2) every 500 steps at a phase of the env's own, a few terminations (1) and frozen steps (4).  Bytes per env-step: 77.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../raptor_amd/csrc/rq_probe.hpp"

#define CHECK(expr)                                                                                   \
    do {                                                                                              \
        const hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                       \
            std::fprintf(stderr, "%s: %s (line %d)\n", #expr, hipGetErrorString(e_), __LINE__);       \
            std::exit(2);                                                                             \
        }                                                                                             \
    } while (0)

namespace rq {
namespace {

#define RQ_FLIGHT_KERNEL k_d0_b64
#define RQ_FLIGHT_DEPTH 0
#define RQ_FLIGHT_BLOCK 64
#include "../raptor_amd/csrc/rq_flight_table.inc"
#define RQ_FLIGHT_KERNEL k_d1_b64
#define RQ_FLIGHT_DEPTH 1
#define RQ_FLIGHT_BLOCK 64
#include "../raptor_amd/csrc/rq_flight_table.inc"
#define RQ_FLIGHT_KERNEL k_d2_b64
#define RQ_FLIGHT_DEPTH 2
#define RQ_FLIGHT_BLOCK 64
#include "../raptor_amd/csrc/rq_flight_table.inc"
#define RQ_FLIGHT_KERNEL k_d3_b64
#define RQ_FLIGHT_DEPTH 3
#define RQ_FLIGHT_BLOCK 64
#include "../raptor_amd/csrc/rq_flight_table.inc"
#define RQ_FLIGHT_KERNEL k_d4_b64
#define RQ_FLIGHT_DEPTH 4
#define RQ_FLIGHT_BLOCK 64
#include "../raptor_amd/csrc/rq_flight_table.inc"
#define RQ_FLIGHT_KERNEL k_d0_b256
#define RQ_FLIGHT_DEPTH 0
#define RQ_FLIGHT_BLOCK 256
#include "../raptor_amd/csrc/rq_flight_table.inc"
#define RQ_FLIGHT_KERNEL k_d1_b256
#define RQ_FLIGHT_DEPTH 1
#define RQ_FLIGHT_BLOCK 256
#include "../raptor_amd/csrc/rq_flight_table.inc"
#define RQ_FLIGHT_KERNEL k_d2_b128
#define RQ_FLIGHT_DEPTH 2
#define RQ_FLIGHT_BLOCK 128
#include "../raptor_amd/csrc/rq_flight_table.inc"
#define RQ_FLIGHT_KERNEL k_d2_b256
#define RQ_FLIGHT_DEPTH 2
#define RQ_FLIGHT_BLOCK 256
#include "../raptor_amd/csrc/rq_flight_table.inc"
#define RQ_FLIGHT_KERNEL k_d3_b256
#define RQ_FLIGHT_DEPTH 3
#define RQ_FLIGHT_BLOCK 256
#include "../raptor_amd/csrc/rq_flight_table.inc"

typedef void (*Kernel)(uint32_t, uint32_t, uint32_t, const float*, const float*, const float*, const uint8_t*, const uint32_t*, float,
                       const ProbeEdges, uint32_t, float*, float*, uint32_t*, uint32_t);
struct Variant { const char* name; int depth; uint32_t block; Kernel k; };
const Variant kVariants[] = {{"depth 0, block 64", 0, 64, k_d0_b64},   {"depth 1, block 64", 1, 64, k_d1_b64},
                             {"depth 2, block 64", 2, 64, k_d2_b64},   {"depth 3, block 64", 3, 64, k_d3_b64},
                             {"depth 4, block 64", 4, 64, k_d4_b64},   {"depth 0, block 256", 0, 256, k_d0_b256},
                             {"depth 1, block 256", 1, 256, k_d1_b256},
                             {"depth 2, block 128", 2, 128, k_d2_b128}, {"depth 2, block 256", 2, 256, k_d2_b256},
                             {"depth 3, block 256", 3, 256, k_d3_b256}};

__device__ __forceinline__ uint32_t mix(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return (uint32_t)x;
}

__global__ void k_fill(float* p, size_t count, uint64_t seed) {
    for (size_t o = blockIdx.x * (size_t)blockDim.x + threadIdx.x; o < count; o += (size_t)gridDim.x * blockDim.x)
        p[o] = ((float)(mix(o + seed) >> 8) * (1.0f / 16777216.0f) - 0.5f) * 2.5f;
}

__global__ void k_done(uint8_t* done, uint32_t steps, uint32_t ld) {
    for (size_t o = blockIdx.x * (size_t)blockDim.x + threadIdx.x; o < (size_t)steps * ld; o += (size_t)gridDim.x * blockDim.x) {
        const uint32_t t = (uint32_t)(o / ld), i = (uint32_t)(o % ld), h = mix(o + 77);
        done[o] = (t + mix(i) % 500u) % 500u == 499u ? 2 : h % 997u == 0 ? 1 : h % 211u == 0 ? 4 : 0;
    }
}

}  // namespace
}  // namespace rq

int main(int argc, char** argv) {
    using namespace rq;
    const uint32_t n = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 65536u, steps = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 500u;
    const uint32_t B = argc > 3 ? (uint32_t)std::atoi(argv[3]) : 10u, rounds = argc > 4 ? (uint32_t)std::atoi(argv[4]) : 5u;
    if (n == 0 || steps == 0 || B == 0 || B > kProbeMaxBuckets || rounds == 0) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    const uint32_t ld = (n + 255u) / 256u * 256u;
    ProbeEdges edges{};
    const bool doubling = B <= 10;                    // 0, 1, 2, 4, ..., 500 as log_age_edges while that fits below 500; else equal widths
    for (uint32_t b = 0; b <= B; ++b) edges.v[b] = !doubling ? b * (500u / B) : b == 0 ? 0 : b == B ? 500u : 1u << (b - 1);
    for (uint32_t b = 1; b <= B; ++b)
        if (edges.v[b] <= edges.v[b - 1]) { std::fprintf(stderr, "the edges of %u buckets do not ascend\n", B); return 2; }

    float *obs, *act, *rew, *sum, *peak;
    uint8_t* done;
    uint32_t* count;
    const size_t cells = (size_t)B * ld;
    CHECK(hipMalloc(&obs, (size_t)steps * 22 * ld * sizeof(float)));
    CHECK(hipMalloc(&act, (size_t)steps * 4 * ld * sizeof(float)));
    CHECK(hipMalloc(&rew, (size_t)steps * ld * sizeof(float)));
    CHECK(hipMalloc(&done, (size_t)steps * ld));
    CHECK(hipMalloc(&sum, cells * RQ_FLIGHT_SUMS * sizeof(float)));
    CHECK(hipMalloc(&peak, cells * RQ_FLIGHT_PEAKS * sizeof(float)));
    CHECK(hipMalloc(&count, cells * sizeof(uint32_t)));
    k_fill<<<2048, 256>>>(obs, (size_t)steps * 22 * ld, 1);
    k_fill<<<2048, 256>>>(act, (size_t)steps * 4 * ld, 2);
    k_fill<<<2048, 256>>>(rew, (size_t)steps * ld, 3);
    k_done<<<2048, 256>>>(done, steps, ld);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());

    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const size_t nv = sizeof(kVariants) / sizeof(kVariants[0]);
    auto run = [&](const Variant& v) {
        CHECK(hipEventRecord(e0));
        v.k<<<(n + v.block - 1) / v.block, v.block>>>(n, ld, steps, obs, act, rew, done, nullptr, 0.25f, edges, B, sum, peak, count, ld);
        CHECK(hipEventRecord(e1));
        CHECK(hipGetLastError());
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        return ms;
    };
    // warm-up and the bits: every variant against the first
    std::vector<float> want(cells * (RQ_FLIGHT_SUMS + RQ_FLIGHT_PEAKS + 1)), got(want.size());
    auto fetch = [&](std::vector<float>& to) {
        CHECK(hipMemcpy(to.data(), sum, cells * RQ_FLIGHT_SUMS * sizeof(float), hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(to.data() + cells * RQ_FLIGHT_SUMS, peak, cells * RQ_FLIGHT_PEAKS * sizeof(float), hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(to.data() + cells * (RQ_FLIGHT_SUMS + RQ_FLIGHT_PEAKS), count, cells * sizeof(uint32_t), hipMemcpyDeviceToHost));
    };
    bool same = true;
    for (size_t v = 0; v < nv; ++v) {
        CHECK(hipMemset(sum, 0xff, cells * RQ_FLIGHT_SUMS * sizeof(float)));
        CHECK(hipMemset(count, 0xff, cells * sizeof(uint32_t)));
        run(kVariants[v]);
        fetch(v == 0 ? want : got);
        if (v && std::memcmp(want.data(), got.data(), want.size() * sizeof(float)) != 0) {
            same = false;
            std::printf("%s: output differs from %s\n", kVariants[v].name, kVariants[0].name);
        }
    }
    unsigned long long counted = 0;
    for (size_t o = 0; o < cells; ++o) {
        uint32_t c;
        std::memcpy(&c, &want[cells * (RQ_FLIGHT_SUMS + RQ_FLIGHT_PEAKS) + o], 4);
        counted += o % ld < n ? c : 0;
    }
    std::vector<std::vector<float>> ms(nv);
    for (uint32_t r = 0; r < rounds; ++r)
        for (size_t v = 0; v < nv; ++v) ms[v].push_back(run(kVariants[v]));
    const double bytes = 77.0 * n * steps;
    std::printf("envs %u, steps %u (ld %u), buckets %u, rounds %u; counted steps %llu; all variants the same bits: %s\n", n, steps, ld, B,
                rounds, counted, same ? "yes" : "NO");
    std::printf("%-22s %10s %10s %10s %10s\n", "variant", "median ms", "min ms", "max ms", "GB/s");
    for (size_t v = 0; v < nv; ++v) {
        std::sort(ms[v].begin(), ms[v].end());
        const float med = ms[v][ms[v].size() / 2];
        std::printf("%-22s %10.3f %10.3f %10.3f %10.0f\n", kVariants[v].name, med, ms[v].front(), ms[v].back(), bytes / (med * 1e-3) / 1e9);
    }
    return same ? 0 : 1;
}
