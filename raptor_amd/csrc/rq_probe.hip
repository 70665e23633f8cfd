// rq_probe.hip - linear probes of the GRU state: the second moments of z = [1, h_t (16), y (M)], zero-padded to D = 32, over the
// state entering every recorded step (rq_trajectory::Grad::saved, what the learner's forward leaves), split by the age of the episode.
//
//   kernel            what                                                                       bound
//   k_probe_moments   a wave per 64 envs, t = 0 .. T-1: S_b += z z^T for the bucket b of the age  HBM (64 B/env-step read) / f32 MFMA rate
//   k_probe_reduce    the waves' partials in ascending wave order, in float64                     HBM (4 KB per wave and bucket)
//   k_probe_hidden_rows   saved [T][16][ld] -> [T][n][16], the learner layout (rq_trajectory_get_hidden)
//   k_probe_moments_timed   k_probe_moments with targets per step, y [T][M][ld_y]              HBM ((64 + 4 M) B/env-step read)
//   k_probe_wrench_targets  a lane per env, t = 0 .. T-1: the scheduled wrench row the env flew  HBM (24 B/env-step written)
//   k_trajectory_flight_table   a lane per env, t = 0 .. T-1: deviation, tilt, rates, effort, reward per age bucket - nine sums,
//                               three peaks, a count (rq_flight_table.inc; reads no saved state)  HBM (77 B/env-step read)
// k_probe_moments and k_probe_moments_timed are one text (rq_probe_moments.inc under RQ_PROBE_TIMED), compiled once per kernel.
//
// Layout.  Lane l of a wave IS env 64 w + l: it loads its 16 state rows (16 coalesced 256-byte reads per step), keeps its age and
// its targets in registers and owns row l of the wave's LDS tile, [64][PZ_ROW]: columns 0 .. 31 = z, column 32 = the bucket of the
// sample (-1: none).  The contraction runs over envs on v_mfma_f32_16x16x4_f32: both operands need feature j on lane j and the env
// on the k-slot q (lane = 16 q + j), so K-step u reads rows 4u + q column-wise: A = B = z[16 a + j] of env 4u + q.  Of the 2 x 2
// output tiles S[a][b] three are computed; S[1][0] is S[0][1] transposed - the same products in the same order, hence the same
// bits - and the reduction mirrors it.  PZ_ROW = 49: odd, so the row-wise writes of a step touch 32 distinct banks per half wave,
// and = 17 mod 32, so the two rows a half wave reads column-wise share one bank only.
//
// The age rule is the forward's episode rule (rq_grad_forward.inc): age 0 at t = 0; a step is live when its done code is not 4
// and its column is below n; a live step contributes (h entering step t, age); after a live step with code 1 or 2 the age is 0
// again, after any other live step it grows by 1; a frozen step changes nothing and contributes nothing.  Sample of age a goes to
// bucket b when edges[b] <= a < edges[b + 1]; others are dropped.  The lane keeps idx = the number of edges <= age, which moves by
// at most one per step (the edges ascend strictly).
//
// Lanes of a wave sit in different buckets at the same step (episodes end at different times): every bucket present is handled in a
// wave-uniform loop, the one whose accumulators are in registers first.  A lane that is not live or not in the bucket contributes
// through SELECTS, never products: an exact zero whatever its registers or its LDS row hold (NaN in a padding column or in the
// state of a frozen step reaches no sum).  The accumulators of the bucket in flight are added to the wave's own partial slot
// [wave][bucket][D][D] when another bucket takes over and at the end: plain loads and stores to memory no other wave touches.
//
// Not a translation unit of its own: rq_teacher.hip includes this file at its end, so the kernels live in that unit's code object
// and its listing (the library ships three code objects and the gate that decodes them counts them).  Nothing here uses anything
// of that unit, and adding kernels to a unit leaves its other kernels' text as it was (tools/kernel_listing_diff.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rq_device_math.hpp"
#include "rq_probe.hpp"

namespace rq {

namespace {

typedef float pf32x4 __attribute__((ext_vector_type(4)));

enum { PZ_BUCKET = 32, PZ_ROW = 49, PZ_TILE = 32 * 32 };

__device__ __forceinline__ pf32x4 probe_mfma(float a, float b, pf32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// the accumulators of bucket `b` into the wave's slot; `first`: the slot has not been written yet
__device__ __forceinline__ void probe_flush(float* __restrict__ slot, uint32_t* __restrict__ count, bool first, uint32_t lane,
                                            const pf32x4& s00, const pf32x4& s01, const pf32x4& s11, uint32_t cnt) {
    const uint32_t q = lane >> 4, j = lane & 15;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float* p00 = slot + (4 * q + r) * 32 + j;
        float* p11 = slot + (16 + 4 * q + r) * 32 + 16 + j;
        if (first) {
            p00[0] = s00[r]; p00[16] = s01[r]; p11[0] = s11[r];
        } else {
            p00[0] = p00[0] + s00[r]; p00[16] = p00[16] + s01[r]; p11[0] = p11[0] + s11[r];
        }
    }
    if (lane == 0) count[0] = first ? cnt : count[0] + cnt;
}

// the moment kernel is one text (rq_probe_moments.inc), compiled once per kernel
#define RQ_PROBE_KERNEL k_probe_moments
#define RQ_PROBE_TIMED 0
#include "rq_probe_moments.inc"

// moments[b][i][k] = sum over waves w = 0, 1, ... of the partial, in that order, in float64; the lower left tile is the upper
// right one mirrored (k_probe_moments computes S[0][1] only).  counts[b] = the waves' counts.
__global__ __launch_bounds__(256) void k_probe_reduce(uint32_t waves, uint32_t n_buckets, const float* __restrict__ partial,
                                                      const uint32_t* __restrict__ wave_counts, double* __restrict__ moments,
                                                      unsigned long long* __restrict__ counts) {
    const uint32_t o = blockIdx.x * 256 + threadIdx.x;
    if (o >= n_buckets * PZ_TILE) return;
    const uint32_t b = o / PZ_TILE, i = (o % PZ_TILE) / 32, k = o % 32;
    const uint32_t src = i >= 16 && k < 16 ? k * 32 + i : i * 32 + k;
    double acc = 0.0;
    for (uint32_t w = 0; w < waves; ++w) acc += (double)partial[((size_t)w * n_buckets + b) * PZ_TILE + src];
    moments[o] = acc;
    if (o % PZ_TILE == 0) {
        unsigned long long c = 0;
        for (uint32_t w = 0; w < waves; ++w) c += wave_counts[(size_t)w * n_buckets + b];
        counts[b] = c;
    }
}

__global__ __launch_bounds__(256) void k_probe_hidden_rows(uint32_t n, uint32_t ld, uint32_t steps, const float* __restrict__ saved,
                                                           float* __restrict__ out) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    for (uint32_t t = blockIdx.y; t < steps; t += gridDim.y) {
        float v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = saved[((size_t)t * 16 + r) * ld + e];      // coalesced over envs
        float* dst = out + ((size_t)t * n + e) * 16;
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[r] = v[r];
    }
}

// k_probe_moments with targets that change over time: y [steps][n_targets][ld_y]
#define RQ_PROBE_KERNEL k_probe_moments_timed
#define RQ_PROBE_TIMED 1
#include "rq_probe_moments.inc"

// The scheduled wrench env i was flown with at every recorded step, rebuilt from what decides it: the table, the env's first row
// (id * rows), its episode step count when the recording began and the recording's done codes.  k in a register: a frozen step
// (code 4) writes six 0.0f and leaves k; any other step writes row min(k, rows - 1) - as it is, or scaled to N / N m with the
// scales of the params (fs = ts = 1.0f unless `scale`) - then k = 0 after code 1 or 2, else k + 1.  out [steps][6][ld_out]: six
// coalesced stores per step; columns >= n are not written.
__global__ __launch_bounds__(256) void k_probe_wrench_targets(uint32_t n, uint32_t ld, uint32_t steps, const uint8_t* __restrict__ done,
                                                              const float* __restrict__ tab, uint32_t rows,
                                                              const uint32_t* __restrict__ row0, const uint32_t* __restrict__ start,
                                                              uint32_t scale, const float* __restrict__ params, float gravity,
                                                              float* __restrict__ out, uint32_t ld_out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float fs, ts;
    wrench_scales(scale, params[(size_t)RQ_P_MASS * ld + i], gravity, params[(size_t)RQ_P_ROTOR_POS * ld + i],
                  params[(size_t)(RQ_P_ROTOR_POS + 1) * ld + i], fs, ts);
    const uint32_t r0 = row0[i];
    uint32_t k = start[i];
    for (uint32_t t = 0; t < steps; ++t) {
        const uint32_t d = done[(size_t)t * ld + i];
        float w[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (d != 4u) {
            float r[6];
            wrench_row(tab, rows, r0, k, r);
#pragma unroll
            for (int c = 0; c < 3; ++c) { w[c] = __fmul_rn(fs, r[c]); w[3 + c] = __fmul_rn(ts, r[3 + c]); }
            k = d == 1u || d == 2u ? 0u : k + 1u;
        }
        float* dst = out + (size_t)t * 6 * ld_out + i;
#pragma unroll
        for (int c = 0; c < 6; ++c) dst[(size_t)c * ld_out] = w[c];
    }
}

// The flight table (rq_flight_table.inc): the loads of the next step ahead of the arithmetic, workgroups of four waves - what
// tools/flight_table_sweep.hip measured (profiles/flight_table_sweep.txt: one step ahead is worth 18 % at 10 buckets, a second or a
// third nothing; four waves a workgroup 4 - 7 % over one).
#define RQ_FLIGHT_KERNEL k_trajectory_flight_table
#define RQ_FLIGHT_DEPTH 1
#define RQ_FLIGHT_BLOCK 256
#include "rq_flight_table.inc"
constexpr uint32_t kFlightBlock = 256;

}  // namespace

hipError_t launch_probe_moments(hipStream_t s, uint32_t n, uint32_t ld, uint32_t steps, const float* saved, const uint8_t* done,
                                const float* y, uint32_t ld_y, uint32_t n_targets, const ProbeEdges& edges, uint32_t n_buckets,
                                float* partial, double* moments, unsigned long long* counts, bool timed) {
    if (n == 0 || steps == 0 || n_targets == 0 || n_targets > kProbeMaxTargets || n_buckets == 0 || n_buckets > kProbeMaxBuckets ||
        ld_y < n)
        return hipErrorInvalidValue;
    const uint32_t waves = (n + 63) / 64;
    if (ld < 64 * waves) return hipErrorInvalidValue;          // every lane of every wave reads its own column of saved / done
    uint32_t* wave_counts = reinterpret_cast<uint32_t*>(partial + (size_t)waves * n_buckets * PZ_TILE);
    if (timed)
        k_probe_moments_timed<<<waves, 64, 0, s>>>(n, ld, steps, saved, done, y, ld_y, n_targets, edges, n_buckets, partial, wave_counts);
    else
        k_probe_moments<<<waves, 64, 0, s>>>(n, ld, steps, saved, done, y, ld_y, n_targets, edges, n_buckets, partial, wave_counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_probe_reduce<<<(n_buckets * PZ_TILE + 255) / 256, 256, 0, s>>>(waves, n_buckets, partial, wave_counts, moments, counts);
    return hipGetLastError();
}

hipError_t launch_probe_wrench_targets(hipStream_t s, uint32_t n, uint32_t ld, uint32_t steps, const uint8_t* done, const float* tab,
                                       uint32_t rows, const uint32_t* row0, const uint32_t* start, bool scale, const float* params,
                                       float gravity, float* out, uint32_t ld_out) {
    if (n == 0 || steps == 0 || rows == 0 || ld < n || ld_out < n) return hipErrorInvalidValue;
    k_probe_wrench_targets<<<(n + 255) / 256, 256, 0, s>>>(n, ld, steps, done, tab, rows, row0, start, scale ? 1u : 0u, params, gravity,
                                                           out, ld_out);
    return hipGetLastError();
}

hipError_t launch_trajectory_flight_table(hipStream_t s, const FlightTableLaunch& a) {
    if (flight_launch_refusal(a)) return hipErrorInvalidValue;      // a lane would touch memory beside its column
    ProbeEdges edges{};
    for (uint32_t b = 0; b <= a.n_buckets; ++b) edges.v[b] = a.edges[b];
    k_trajectory_flight_table<<<(a.n + kFlightBlock - 1) / kFlightBlock, kFlightBlock, 0, s>>>(
        a.n, a.ld, a.steps, a.obs, a.act, a.rew, a.done, a.start, a.tol2, edges, a.n_buckets, a.sum, a.peak, a.count, a.ld_out);
    return hipGetLastError();
}

hipError_t launch_probe_hidden_rows(hipStream_t s, uint32_t n, uint32_t ld, uint32_t steps, const float* saved, float* out) {
    if (n == 0 || steps == 0) return hipSuccess;
    k_probe_hidden_rows<<<dim3((n + 255) / 256, steps < 65535u ? steps : 65535u), 256, 0, s>>>(n, ld, steps, saved, out);
    return hipGetLastError();
}

}  // namespace rq
