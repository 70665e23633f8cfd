// rq_flight_table.inc - the body of the flight-table kernel, included by rq_probe.hip (and, once per variant, by
// tools/flight_table_sweep.hip, which is how depth and workgroup size were chosen):
//   RQ_FLIGHT_KERNEL   the kernel's name
//   RQ_FLIGHT_DEPTH    how many steps' loads are in flight ahead of the arithmetic: 0 = none (load, then use), d >= 1 = the loads of
//                      step t + d are issued before the arithmetic of step t, from a ring of d steps held in registers
//   RQ_FLIGHT_BLOCK    the workgroup size, a multiple of 64
//
// One lane is one env, walked from t = 0 to steps - 1.  Per step the lane reads 14 observation fields (0-2 position relative to the
// setpoint, 11 = R22, 12-14 linear velocity, 15-17 angular velocity, 18-21 the previous action), the four actions, the reward and the
// done code: 19 coalesced dword rows and one byte row, 77 B per env-step.  Age and bucket index move as in rq_grad_forward.inc under
// RQ_GRAD_ERROR_TABLE (idx = the number of edges <= age, ed[] in LDS), except that the age at t = 0 is start[i].  The lane keeps
// the thirteen running values of its current bucket - nine sums, three peaks, the count - in registers; when its bucket changes
// it stores them to its own column and loads the new bucket's, so an env that returns to a bucket in a later episode continues from
// the stored total.  The kernel zeroes its column's cells first: no atomics, no memset, no exchange between lanes, the same bits
// every run.  What is frozen, outside every bucket or a padding lane is SELECTED away: its values may be anything, NaN included.
// Every operation is rounded to fp32 on its own (__fmul_rn / __fadd_rn / __fsub_rn: no contraction).
//
// Why a ring: a lane-per-env walk has ceil(n / 64) waves - one per SIMD at 65 536 envs - and the bucket change's stores and loads
// sit in the loop, so the compiler keeps one step's loads in flight at most.  The ring's index is static after unrolling (the
// outer loop advances by RQ_FLIGHT_DEPTH steps), the loads past the end re-read the last step (in bounds, never used).  The depth
// that pays is bounded by the wave's load counter: 6 bits, 63 loads in flight, three steps of 20.
#ifndef RQ_FLIGHT_TABLE_SHARED
#define RQ_FLIGHT_TABLE_SHARED

struct FlightStep {
    float x[14];          // obs 0, 1, 2 | 11 | 12 .. 17 | 18 .. 21
    float a[4];
    float r;
    uint32_t d;
};

__device__ __forceinline__ void flight_load(FlightStep& s, const float* __restrict__ obs, const float* __restrict__ act,
                                            const float* __restrict__ rew, const uint8_t* __restrict__ done, uint32_t t, uint32_t ld,
                                            uint32_t i) {
    const float* o = obs + (size_t)t * RQ_POLICY_INPUT_DIM * ld + i;          // a recording holds the policy's 22, not the env's 26
#pragma unroll
    for (int k = 0; k < 3; ++k) s.x[k] = o[(size_t)k * ld];
    s.x[3] = o[(size_t)11 * ld];
#pragma unroll
    for (int k = 0; k < 10; ++k) s.x[4 + k] = o[(size_t)(12 + k) * ld];
    const float* a = act + (size_t)t * RQ_ACTION_DIM * ld + i;
#pragma unroll
    for (int k = 0; k < 4; ++k) s.a[k] = a[(size_t)k * ld];
    s.r = rew[(size_t)t * ld + i];
    s.d = done[(size_t)t * ld + i];
}

// the running values of one bucket of one env
struct FlightCell {
    float s[RQ_FLIGHT_SUMS];
    float p[RQ_FLIGHT_PEAKS];
    uint32_t c;
};

__device__ __forceinline__ float flight_sq3(float a, float b, float c) {
    return __fadd_rn(__fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)), __fmul_rn(c, c));
}

// one counted step into the cell; `on` false: nothing changes, whatever the step holds
__device__ __forceinline__ void flight_add(FlightCell& c, const FlightStep& s, float tol2, bool on) {
    const float* x = s.x;
    float v[RQ_FLIGHT_SUMS];
    v[RQ_FLIGHT_POS2] = flight_sq3(x[0], x[1], x[2]);
    v[RQ_FLIGHT_VEL2] = flight_sq3(x[4], x[5], x[6]);
    v[RQ_FLIGHT_OMEGA2] = flight_sq3(x[7], x[8], x[9]);
    v[RQ_FLIGHT_TILT] = __fsub_rn(1.0f, x[3]);
    v[RQ_FLIGHT_ACT2] = __fadd_rn(flight_sq3(s.a[0], s.a[1], s.a[2]), __fmul_rn(s.a[3], s.a[3]));
    const float d0 = __fsub_rn(s.a[0], x[10]), d1 = __fsub_rn(s.a[1], x[11]), d2 = __fsub_rn(s.a[2], x[12]), d3 = __fsub_rn(s.a[3], x[13]);
    v[RQ_FLIGHT_DACT2] = __fadd_rn(flight_sq3(d0, d1, d2), __fmul_rn(d3, d3));
    uint32_t sat = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) sat += fabsf(s.a[k]) >= 1.0f ? 1u : 0u;
    v[RQ_FLIGHT_SATURATED] = (float)sat;
    v[RQ_FLIGHT_OUTSIDE] = v[RQ_FLIGHT_POS2] > tol2 ? 1.0f : 0.0f;
    v[RQ_FLIGHT_REWARD] = s.r;
#pragma unroll
    for (int k = 0; k < RQ_FLIGHT_SUMS; ++k) c.s[k] = on ? __fadd_rn(c.s[k], v[k]) : c.s[k];      // selected, never multiplied
    const float pv[RQ_FLIGHT_PEAKS] = {v[RQ_FLIGHT_POS2], v[RQ_FLIGHT_TILT], v[RQ_FLIGHT_OMEGA2]};
#pragma unroll
    for (int k = 0; k < RQ_FLIGHT_PEAKS; ++k) c.p[k] = on && pv[k] > c.p[k] ? pv[k] : c.p[k];     // a NaN never replaces a peak
    c.c += on ? 1u : 0u;
}

__device__ __forceinline__ void flight_store(const FlightCell& c, float* sum, float* peak, uint32_t* count, uint32_t b, uint32_t i,
                                             uint32_t ld_out) {
#pragma unroll
    for (int k = 0; k < RQ_FLIGHT_SUMS; ++k) sum[flight_sum_cell(b, k, i, ld_out)] = c.s[k];
#pragma unroll
    for (int k = 0; k < RQ_FLIGHT_PEAKS; ++k) peak[flight_peak_cell(b, k, i, ld_out)] = c.p[k];
    count[flight_count_cell(b, i, ld_out)] = c.c;
}

__device__ __forceinline__ void flight_fetch(FlightCell& c, const float* sum, const float* peak, const uint32_t* count, uint32_t b,
                                             uint32_t i, uint32_t ld_out) {
#pragma unroll
    for (int k = 0; k < RQ_FLIGHT_SUMS; ++k) c.s[k] = sum[flight_sum_cell(b, k, i, ld_out)];
#pragma unroll
    for (int k = 0; k < RQ_FLIGHT_PEAKS; ++k) c.p[k] = peak[flight_peak_cell(b, k, i, ld_out)];
    c.c = count[flight_count_cell(b, i, ld_out)];
    // The values are pinned as arrived HERE, inside the rare branch: an empty statement that reads each register makes the compiler
    // place its wait for these loads in front of it.  Without it the wait lands behind the branch's join, where it is executed by
    // every step whether or not the bucket changed - and since loads return in order it drains the ring's loads with it.
#pragma unroll
    for (int k = 0; k < RQ_FLIGHT_SUMS; ++k) asm volatile("" : "+v"(c.s[k]));
#pragma unroll
    for (int k = 0; k < RQ_FLIGHT_PEAKS; ++k) asm volatile("" : "+v"(c.p[k]));
    asm volatile("" : "+v"(c.c));
}
#endif  // RQ_FLIGHT_TABLE_SHARED

__global__ __launch_bounds__(RQ_FLIGHT_BLOCK) void RQ_FLIGHT_KERNEL(uint32_t n, uint32_t ld, uint32_t steps, const float* __restrict__ obs,
                                                                    const float* __restrict__ act, const float* __restrict__ rew,
                                                                    const uint8_t* __restrict__ done, const uint32_t* __restrict__ start,
                                                                    float tol2, const ProbeEdges edges, uint32_t n_buckets, float* sum,
                                                                    float* peak, uint32_t* count, uint32_t ld_out) {
    __shared__ uint32_t ed[kProbeMaxBuckets + 1];
    const uint32_t i0 = blockIdx.x * RQ_FLIGHT_BLOCK + threadIdx.x;
    const bool valid = i0 < n;
    const uint32_t i = valid ? i0 : n - 1;          // a padding lane reads the last env's column and writes nothing
    if (threadIdx.x <= n_buckets) ed[threadIdx.x] = edges.v[threadIdx.x];
    FlightCell cell;
#pragma unroll
    for (int k = 0; k < RQ_FLIGHT_SUMS; ++k) cell.s[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < RQ_FLIGHT_PEAKS; ++k) cell.p[k] = 0.0f;
    cell.c = 0u;
    if (valid)
        for (uint32_t b = 0; b < n_buckets; ++b) flight_store(cell, sum, peak, count, b, i0, ld_out);
    __syncthreads();
    const uint32_t idx0 = ed[0] == 0u ? 1u : 0u;     // edges <= age 0
    uint32_t age = start ? start[i] : 0u, idx = 0;
    for (uint32_t b = 0; b <= n_buckets; ++b) idx += ed[b] <= age ? 1u : 0u;
    int cur = -1;                                     // the bucket whose values the lane holds

    // one step: the move of (age, idx) is rq_grad_forward.inc's, word for word
    auto step = [&](const FlightStep& s) {
        const uint32_t d = s.d;
        const bool live = valid && d != 4u;
        const int bk = live && idx >= 1u && idx <= n_buckets ? (int)idx - 1 : -1;
        if (live) {
            if (d == 1u || d == 2u) { age = 0; idx = idx0; }
            else {
                ++age;
                if (idx <= n_buckets && ed[idx] == age) ++idx;
            }
        }
        if (bk >= 0 && bk != cur) {                   // the lane's bucket changes: its values go to its column, the new bucket's come
            if (cur >= 0) flight_store(cell, sum, peak, count, (uint32_t)cur, i0, ld_out);
            flight_fetch(cell, sum, peak, count, (uint32_t)bk, i0, ld_out);
            cur = bk;
        }
        flight_add(cell, s, tol2, bk >= 0);
    };

#if RQ_FLIGHT_DEPTH == 0
    for (uint32_t t = 0; t < steps; ++t) {
        FlightStep s;
        flight_load(s, obs, act, rew, done, t, ld, i);
        step(s);
    }
#else
    // The ring fills inside the loop (its first RQ_FLIGHT_DEPTH turns issue loads and run no step), not in a prologue of its own: the
    // waits the compiler places are then counted for one order of issue - with a prologue it is free to issue the ring's steps in
    // another order, and the loop's waits, which must hold on both ways in, cover one step less than the ring holds.
    const uint32_t last = steps - 1u;
    FlightStep ring[RQ_FLIGHT_DEPTH] = {};
    for (uint32_t t0 = 0; t0 < steps + RQ_FLIGHT_DEPTH; t0 += RQ_FLIGHT_DEPTH) {
#pragma unroll
        for (int k = 0; k < RQ_FLIGHT_DEPTH; ++k) {
            const uint32_t ahead = t0 + k;            // the step whose loads are issued now; the step that runs is RQ_FLIGHT_DEPTH back
            const FlightStep s = ring[k];
            flight_load(ring[k], obs, act, rew, done, ahead < last ? ahead : last, ld, i);
            if (ahead >= RQ_FLIGHT_DEPTH && ahead - RQ_FLIGHT_DEPTH < steps) step(s);          // wave-uniform
        }
    }
#endif
    if (cur >= 0) flight_store(cell, sum, peak, count, (uint32_t)cur, i0, ld_out);
}
#undef RQ_FLIGHT_KERNEL
#undef RQ_FLIGHT_DEPTH
#undef RQ_FLIGHT_BLOCK
