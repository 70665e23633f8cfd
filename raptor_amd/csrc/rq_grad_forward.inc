// rq_grad_forward.inc - the body of the learner's forward kernel, included by rq_grad.hpp once per kernel:
//   RQ_GRAD_FORWARD_KERNEL   the kernel's name
//   RQ_GRAD_STORE_ACT        1: the actions are written to act [t][4][ld_act] (k_policy_grad_forward); 0: they are not, and the
//                            kernel has no such parameters (k_policy_grad_forward_state: the distillation update's pass)
//   RQ_GRAD_BANK             1: the wave's image is that of its block's policy, images + block_policy[blockIdx.x] * image_floats
//                            (k_policy_grad_forward_state_bank: one workgroup = one wave = one 64-env block); 0: `packed` is it
//   RQ_GRAD_ERROR_TABLE      (optional, default 0) 1: nothing of the pass is stored - neither `saved` nor act, the kernel has no such
//                            parameters.  The lane loads its step's four targets y [t][0..3][ld_y] beside the observation and sums its
//                            env's squared imitation error e = ((d0 d0 + d1 d1) + d2 d2) + d3 d3, d = a - y, each operation rounded to
//                            fp32 on its own, per bucket of episode age: sse [b][ld_out] and count [b][ld_out], columns < n
//                            (k_policy_error_table, k_policy_error_table_bank).  Age and bucket index move as in rq_probe_moments.inc;
//                            the edges lie in LDS.  The lane keeps the running pair of its current bucket in registers; when its
//                            bucket changes it stores the pair to its own column and loads the new bucket's, so an env that comes
//                            back to a bucket in a later episode goes on from the stored total.  The kernel zeroes its column's
//                            n_buckets cells first: no atomics, no exchange between lanes, no memset, the same bits every run.  What
//                            is frozen, outside every bucket or a padding lane is selected away before any arithmetic.
// One text for all, and each a kernel of its own rather than a call into a shared function: the existing kernel's listing stays
// the parent build's to the instruction.
#ifndef RQ_GRAD_ERROR_TABLE
#define RQ_GRAD_ERROR_TABLE 0
#endif
template <typename ACTOR>
__global__ __launch_bounds__(kFusedBlock, WavesPerSimd<ACTOR>::value) void RQ_GRAD_FORWARD_KERNEL(
        uint32_t n, uint32_t ld, uint32_t steps,
#if RQ_GRAD_BANK
        const float* __restrict__ images, const uint32_t* __restrict__ block_policy, uint32_t image_floats,
#else
        const float* __restrict__ packed,
#endif
        const float* __restrict__ obs, const uint8_t* __restrict__ done, const float* __restrict__ hidden, uint32_t ld_h, uint32_t start_initial,
#if RQ_GRAD_STORE_ACT
        float* __restrict__ act, uint32_t ld_act,
#endif
#if RQ_GRAD_ERROR_TABLE
        const float* __restrict__ y, uint32_t ld_y, const ProbeEdges edges, uint32_t n_buckets, float* __restrict__ sse,
        uint32_t* __restrict__ count, uint32_t ld_out) {
    __shared__ uint32_t ed[kProbeMaxBuckets + 1];
#else
        float* __restrict__ saved) {
#endif
#if RQ_GRAD_BANK
    const float* __restrict__ packed = images + (size_t)block_policy[blockIdx.x] * image_floats;
#endif
    ACTOR actor;
    actor.template load<kFusedBlock / 64>(packed);
    const uint32_t lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15;
    const uint32_t wave_base = blockIdx.x * kFusedBlock;
    const uint32_t i0 = wave_base + lane;
    const uint32_t i = i0 < n ? i0 : n - 1;
    const bool valid = i0 < n;
    float hQ[4][4], h0Q[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) h0Q[t][r] = actor.h0(r);
    if (start_initial) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) hQ[t][r] = h0Q[t][r];
    } else {
        load_hidden_q(hidden, ld_h, wave_base, n, hQ);
    }
    typename ACTOR::Carry carry;
    actor.prime(hQ, carry);
#if RQ_GRAD_ERROR_TABLE
    if (lane <= n_buckets) ed[lane] = edges.v[lane];
    float* const sse_col = sse + i0;                 // the lane's own column; written where `valid` only (i0 < n <= ld_out)
    uint32_t* const count_col = count + i0;
    if (valid)
        for (uint32_t b = 0; b < n_buckets; ++b) {
            sse_col[(size_t)b * ld_out] = 0.0f;
            count_col[(size_t)b * ld_out] = 0u;
        }
    __syncthreads();
    const uint32_t idx0 = ed[0] == 0u ? 1u : 0u;     // edges <= age 0
    uint32_t age = 0, idx = idx0, run_count = 0;
    float run_sse = 0.0f;
    int cur = -1;                                     // the bucket whose pair the lane holds
#endif
    for (uint32_t t = 0; t < steps; ++t) {
        float x[22], a[4], hn[4][4];
#if !RQ_GRAD_ERROR_TABLE
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) saved[((size_t)t * 16 + 4 * q + r) * ld + wave_base + 16 * tt + j] = hQ[tt][r];
#endif
#pragma unroll
        for (int k = 0; k < 22; ++k) x[k] = field(obs, t * 22 + k, ld)[i];
        const uint8_t d = done[(size_t)t * ld + i];
#if RQ_GRAD_ERROR_TABLE
        float yt[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) yt[k] = field(y, t * 4 + k, ld_y)[i];
        const bool live = valid && d != 4;
        const int bk = live && idx >= 1u && idx <= n_buckets ? (int)idx - 1 : -1;
        if (live) {                                   // rq_probe_moments.inc's move of (age, idx), word for word
            if (d == 1 || d == 2) { age = 0; idx = idx0; }
            else {
                ++age;
                if (idx <= n_buckets && ed[idx] == age) ++idx;
            }
        }
#endif
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) hn[tt][r] = hQ[tt][r];
        const typename ACTOR::Saved before = actor.carry_of(carry);
        actor.template step_fused<0>(x, hn, a, carry, [] {});
        select_hidden_q(__builtin_amdgcn_ballot_w64(d != 4), hn, hQ);          // frozen: state not advanced
        const uint64_t held = __builtin_amdgcn_ballot_w64(d == 4);
        if (held != 0) actor.hold_carry(held, before, carry);
        const uint64_t ended = __builtin_amdgcn_ballot_w64(d == 1 || d == 2);
        if (ended != 0) {                                                       // episode end: the learned initial state
            select_hidden_q(ended, h0Q, hQ);
            actor.reset_carry(ended, hQ, carry);
        }
#if RQ_GRAD_STORE_ACT
        if (valid) {
#pragma unroll
            for (int k = 0; k < 4; ++k) field(act, t * 4 + k, ld_act)[i] = a[k];
        }
#endif
#if RQ_GRAD_ERROR_TABLE
        if (bk >= 0 && bk != cur) {                   // the lane's bucket changes: its pair goes to its column, the new bucket's comes
            if (cur >= 0) {
                sse_col[(size_t)cur * ld_out] = run_sse;
                count_col[(size_t)cur * ld_out] = run_count;
            }
            run_sse = sse_col[(size_t)bk * ld_out];
            run_count = count_col[(size_t)bk * ld_out];
            cur = bk;
        }
        {
            const float d0 = __fsub_rn(a[0], yt[0]), d1 = __fsub_rn(a[1], yt[1]), d2 = __fsub_rn(a[2], yt[2]), d3 = __fsub_rn(a[3], yt[3]);
            const float e = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2)), __fmul_rn(d3, d3));
            run_sse = bk >= 0 ? __fadd_rn(run_sse, e) : run_sse;          // selected, never multiplied: NaN elsewhere reaches no sum
            run_count += bk >= 0 ? 1u : 0u;
        }
#endif
    }
#if RQ_GRAD_ERROR_TABLE
    if (cur >= 0) {
        sse_col[(size_t)cur * ld_out] = run_sse;
        count_col[(size_t)cur * ld_out] = run_count;
    }
#endif
}
#undef RQ_GRAD_FORWARD_KERNEL
#undef RQ_GRAD_STORE_ACT
#undef RQ_GRAD_BANK
#undef RQ_GRAD_ERROR_TABLE
