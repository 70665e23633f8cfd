// rq_grad_bank.hpp - the distillation update of rq_grad.hpp for a bank of P policies, one per 64-env block (rq_rollout_policies'
// granularity): a sweep of learning rates or seeds costs one student's launch count.
//
//   kernel                             what                                                              grid
//   k_policy_grad_forward_state_bank   k_policy_grad_forward_state, the wave's image picked per block      waves
//   k_policy_loss_backward_bank        k_policy_loss_backward, both images picked per block                waves
//   k_policy_loss_reduce_bank          policy p: its waves' partials in ascending wave order, x 2 / M_p    (ceil(2084 / 256), P)
//   k_policy_loss_backward_weighted_bank   k_policy_loss_backward_weighted, both images picked per block   waves
//   k_policy_loss_reduce_weighted_bank     policy p: as above with W4_p, its waves' float64 weight sums    (ceil(2084 / 256), P)
//   k_adam_repack_bank                 k_adam_repack on slot p; a policy that owns no wave is skipped       P
//   k_adam_set_lr_bank                 up to 256 learning rates, carried as kernel arguments                1
// The weights are wave-uniform MFMA operands read once from an image pointer, so the seeded pair is the single policy's text
// (rq_grad_forward.inc, rq_grad_backward.inc under RQ_GRAD_BANK) with that pointer chosen by block_policy[blockIdx.x], as
// k_rollout_fused_bank chooses it: a wave computes what it computes for a policy of its own, bit for bit.  The reduction is the single
// policy's, segmented: a policy's waves come from a CSR list (wave_offsets [P + 1] into wave_list [waves], ascending within a
// policy), so its gradient and loss are those of a recording that holds its blocks only, in order.
// Device code, compiled as part of rq_kernels.hip.
#pragma once
#include "rq_grad.hpp"

namespace rq {

#define RQ_GRAD_FORWARD_KERNEL k_policy_grad_forward_state_bank
#define RQ_GRAD_STORE_ACT 0
#define RQ_GRAD_BANK 1
#include "rq_grad_forward.inc"

#define RQ_GRAD_BACKWARD_KERNEL k_policy_loss_backward_bank
#define RQ_GRAD_SEEDED 1
#define RQ_GRAD_BANK 1
#include "rq_grad_backward.inc"

#define RQ_GRAD_BACKWARD_KERNEL k_policy_loss_backward_weighted_bank
#define RQ_GRAD_SEEDED 1
#define RQ_GRAD_BANK 1
#define RQ_GRAD_WEIGHTED 1
#include "rq_grad_backward.inc"

// k_policy_loss_reduce per policy (blockIdx.y): M_p = the live entries of p's waves (an integer sum), grad [p][:] = the partials of
// p's waves summed in ascending wave order x 2 / M_p - the product in float64, one rounding to fp32 - and loss [p] = SSE_p / M_p.
// M_p = 0: loss and gradient 0.  A policy that owns no wave: loss NaN, its gradient row is not written.
__global__ __launch_bounds__(256) void k_policy_loss_reduce_bank(const uint32_t* __restrict__ wave_offsets,
                                                                const uint32_t* __restrict__ wave_list,
                                                                const float* __restrict__ partial, const float* __restrict__ wave_sse,
                                                                const uint32_t* __restrict__ wave_live, float* __restrict__ grad,
                                                                float* __restrict__ loss) {
    __shared__ unsigned long long cnt[256];
    const uint32_t pol = blockIdx.y;
    const uint32_t w0 = wave_offsets[pol], w1 = wave_offsets[pol + 1];
    if (w0 == w1) {                     // uniform for the workgroup
        if (blockIdx.x == 0 && threadIdx.x == 0) loss[pol] = __builtin_nanf("");
        return;
    }
    unsigned long long mine = 0;
    for (uint32_t k = w0 + threadIdx.x; k < w1; k += 256) mine += wave_live[wave_list[k]];
    cnt[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) cnt[threadIdx.x] += cnt[threadIdx.x + h];
        __syncthreads();
    }
    const unsigned long long M = cnt[0];
    const double inv = M ? 1.0 / (double)M : 0.0;
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p < RQ_POLICY_NUM_WEIGHTS) {
        float acc = 0.0f;
        for (uint32_t k = w0; k < w1; ++k) acc += partial[(size_t)wave_list[k] * RQ_POLICY_NUM_WEIGHTS + p];
        grad[(size_t)pol * RQ_POLICY_NUM_WEIGHTS + p] = M ? (float)((double)acc * (2.0 * inv)) : 0.0f;
    }
    if (p == 0) {
        float acc = 0.0f;
        for (uint32_t k = w0; k < w1; ++k) acc += wave_sse[wave_list[k]];
        loss[pol] = M ? (float)((double)acc * inv) : 0.0f;
    }
}

// k_policy_loss_reduce_weighted per policy (blockIdx.y), as k_policy_loss_reduce_bank is k_policy_loss_reduce per policy: W4_p = the
// wave_wsum of p's waves added in ascending wave order in float64, grad [p][:] = its waves' partials in that order x 2 / W4_p, loss
// [p] = SSE_p / W4_p.  W4_p = 0 (none of p's entries counts): loss and gradient 0, and Adam sees a zero gradient.  A policy that owns
// no wave: loss NaN, its gradient row is not written.
__global__ __launch_bounds__(256) void k_policy_loss_reduce_weighted_bank(const uint32_t* __restrict__ wave_offsets,
                                                                         const uint32_t* __restrict__ wave_list,
                                                                         const float* __restrict__ partial,
                                                                         const float* __restrict__ wave_sse,
                                                                         const double* __restrict__ wave_wsum, float* __restrict__ grad,
                                                                         float* __restrict__ loss) {
    const uint32_t pol = blockIdx.y;
    const uint32_t w0 = wave_offsets[pol], w1 = wave_offsets[pol + 1];
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (w0 == w1) {
        if (p == 0) loss[pol] = __builtin_nanf("");
        return;
    }
    if (p >= RQ_POLICY_NUM_WEIGHTS) return;
    float acc = 0.0f;
    double W4 = 0.0;
    for (uint32_t k = w0; k < w1; ++k) {
        const uint32_t w = wave_list[k];
        acc += partial[(size_t)w * RQ_POLICY_NUM_WEIGHTS + p];
        W4 += wave_wsum[w];
    }
    const bool any = W4 > 0.0;
    const double inv = any ? 1.0 / W4 : 0.0;
    grad[(size_t)pol * RQ_POLICY_NUM_WEIGHTS + p] = any ? (float)((double)acc * (2.0 * inv)) : 0.0f;
    if (p == 0) {
        float sse = 0.0f;
        for (uint32_t k = w0; k < w1; ++k) sse += wave_sse[wave_list[k]];
        loss[pol] = any ? (float)((double)sse * inv) : 0.0f;
    }
}

// k_adam_repack, workgroup p on slot p: grad / w / m / v [p][2084], st [p] (every hyper-parameter per policy), packed [p][n_forward]
// and gpacked [p][n_grad] through the one gather table.  A policy that owns no wave in this assignment has no gradient: its weights,
// moments, step count and images stay as they were.
__global__ __launch_bounds__(1024) void k_adam_repack_bank(const uint32_t* __restrict__ wave_offsets, const float* __restrict__ grad_all,
                                                           float* __restrict__ w_all, float* __restrict__ m_all, float* __restrict__ v_all,
                                                           AdamState* __restrict__ st_all, const PackGather* __restrict__ table,
                                                           uint32_t n_forward, uint32_t n_grad, float* __restrict__ packed_all,
                                                           float* __restrict__ gpacked_all) {
    __shared__ float ws[RQ_POLICY_NUM_WEIGHTS];
    const uint32_t pol = blockIdx.x;
    if (wave_offsets[pol] == wave_offsets[pol + 1]) return;            // uniform for the workgroup
    const float* __restrict__ grad = grad_all + (size_t)pol * RQ_POLICY_NUM_WEIGHTS;
    float* __restrict__ w = w_all + (size_t)pol * RQ_POLICY_NUM_WEIGHTS;
    float* __restrict__ m = m_all + (size_t)pol * RQ_POLICY_NUM_WEIGHTS;
    float* __restrict__ v = v_all + (size_t)pol * RQ_POLICY_NUM_WEIGHTS;
    AdamState* __restrict__ st = st_all + pol;
    float* __restrict__ packed = packed_all + (size_t)pol * n_forward;
    float* __restrict__ gpacked = gpacked_all + (size_t)pol * n_grad;
    const double lr = st->lr, beta1 = st->beta1, beta2 = st->beta2, eps = st->eps, wd = st->weight_decay;
    const double b1t = st->beta1_t * beta1, b2t = st->beta2_t * beta2;
    const uint32_t step = st->step;
    for (uint32_t p = threadIdx.x; p < RQ_POLICY_NUM_WEIGHTS; p += 1024) {
        const double g = grad[p];
        const double mm = beta1 * (double)m[p] + (1.0 - beta1) * g;
        const double vv = beta2 * (double)v[p] + (1.0 - beta2) * g * g;
        const double mhat = mm / (1.0 - b1t), vhat = vv / (1.0 - b2t);
        double x = w[p];
        x = x * (1.0 - lr * wd) - lr * mhat / (sqrt(vhat) + eps);
        const float xf = (float)x;
        m[p] = (float)mm;
        v[p] = (float)vv;
        w[p] = xf;
        ws[p] = xf;
    }
    __syncthreads();                    // every thread has read the state; the weights are in LDS
    if (threadIdx.x == 0) { st->beta1_t = b1t; st->beta2_t = b2t; st->step = step + 1; }
    for (uint32_t e = threadIdx.x; e < n_forward + n_grad; e += 1024) {
        const PackGather t = table[e];
        float x = 0.0f;
        if (t.a != PACK_GATHER_NONE) {
            x = ws[t.a];
            if (t.b != PACK_GATHER_NONE) x = x + ws[t.b];
            x = t.k * x;
        }
        if (e < n_forward) packed[e] = x;
        else gpacked[e - n_forward] = x;
    }
}

// st [first + i].lr = rates.lr [i * stride] for i < count <= 256 (stride 0: one rate for all).  The rates travel as kernel arguments:
// a call takes effect in stream order, and the caller's array is its own again when the launch returns.
struct AdamLrChunk { double lr[256]; };
__global__ __launch_bounds__(256) void k_adam_set_lr_bank(AdamState* __restrict__ st, uint32_t first, uint32_t count, uint32_t stride,
                                                          AdamLrChunk rates) {
    const uint32_t i = threadIdx.x;
    if (i < count) st[first + i].lr = rates.lr[i * stride];
}

hipError_t launch_policy_loss_grad_bank(hipStream_t s, uint32_t n, uint32_t ld, uint32_t steps, uint32_t n_policies, const float* images,
                                        const float* gimages, const uint32_t* block_policy, const uint32_t* wave_offsets,
                                        const uint32_t* wave_list, const float* obs, const uint8_t* done, const float* hidden,
                                        uint32_t ld_h, int start_initial, float* saved, const float* target, uint32_t ld_y,
                                        float* partial, float* grad, float* loss) {
    if (n == 0 || steps == 0 || n_policies == 0) return hipErrorInvalidValue;
    const unsigned g = (n + kFusedBlock - 1) / kFusedBlock;
    const uint32_t si = start_initial ? 1u : 0u, waves = (n + 63) / 64;
    if (n > kOneWavePerSimdEnvs)        // launch_policy_loss_grad's choice of build
        k_policy_grad_forward_state_bank<ActorF32Lean><<<g, kFusedBlock, 0, s>>>(n, ld, steps, images, block_policy,
                                                                                 (uint32_t)RQ_PACKED_FLOATS, obs, done, hidden, ld_h, si, saved);
    else
        k_policy_grad_forward_state_bank<ActorF32><<<g, kFusedBlock, 0, s>>>(n, ld, steps, images, block_policy,
                                                                             (uint32_t)RQ_PACKED_FLOATS, obs, done, hidden, ld_h, si, saved);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    float* wave_sse = partial + (size_t)waves * RQ_POLICY_NUM_WEIGHTS;         // partial: [waves][2084] | sse [waves] | live [waves]
    uint32_t* wave_live = reinterpret_cast<uint32_t*>(wave_sse + waves);
    k_policy_loss_backward_bank<<<waves, 64, 0, s>>>(n, ld, steps, images, gimages, block_policy, (uint32_t)RQ_PACKED_FLOATS,
                                                     (uint32_t)RQ_PACKED_GRAD_FLOATS, obs, done, saved, target, ld_y, si, partial,
                                                     wave_sse, wave_live);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_policy_loss_reduce_bank<<<dim3((RQ_POLICY_NUM_WEIGHTS + 255) / 256, n_policies), 256, 0, s>>>(wave_offsets, wave_list, partial,
                                                                                                   wave_sse, wave_live, grad, loss);
    return hipGetLastError();
}

hipError_t launch_policy_loss_grad_weighted_bank(hipStream_t s, uint32_t n, uint32_t ld, uint32_t steps, uint32_t n_policies,
                                                 const float* images, const float* gimages, const uint32_t* block_policy,
                                                 const uint32_t* wave_offsets, const uint32_t* wave_list, const float* obs,
                                                 const uint8_t* done, const float* hidden, uint32_t ld_h, int start_initial, float* saved,
                                                 const float* target, uint32_t ld_y, const float* weight, uint32_t ld_w,
                                                 uint32_t weight_steps, float* partial, float* grad, float* loss) {
    if (n == 0 || steps == 0 || n_policies == 0) return hipErrorInvalidValue;
    if (weight == nullptr || ld_w < n || (weight_steps != 1 && weight_steps != steps)) return hipErrorInvalidValue;
    const unsigned g = (n + kFusedBlock - 1) / kFusedBlock;
    const uint32_t si = start_initial ? 1u : 0u, waves = (n + 63) / 64;
    if (n > kOneWavePerSimdEnvs)        // launch_policy_loss_grad_bank's choice of build
        k_policy_grad_forward_state_bank<ActorF32Lean><<<g, kFusedBlock, 0, s>>>(n, ld, steps, images, block_policy,
                                                                                 (uint32_t)RQ_PACKED_FLOATS, obs, done, hidden, ld_h, si, saved);
    else
        k_policy_grad_forward_state_bank<ActorF32><<<g, kFusedBlock, 0, s>>>(n, ld, steps, images, block_policy,
                                                                             (uint32_t)RQ_PACKED_FLOATS, obs, done, hidden, ld_h, si, saved);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    double* wave_wsum = reinterpret_cast<double*>(partial + (size_t)waves * RQ_POLICY_NUM_WEIGHTS);   // launch_policy_loss_grad_weighted's layout
    float* wave_sse = reinterpret_cast<float*>(wave_wsum + waves);
    k_policy_loss_backward_weighted_bank<<<waves, 64, 0, s>>>(n, ld, steps, images, gimages, block_policy, (uint32_t)RQ_PACKED_FLOATS,
                                                              (uint32_t)RQ_PACKED_GRAD_FLOATS, obs, done, saved, target, ld_y, weight, ld_w,
                                                              weight_steps == 1 ? 0u : ld_w, si, partial, wave_sse, wave_wsum);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_policy_loss_reduce_weighted_bank<<<dim3((RQ_POLICY_NUM_WEIGHTS + 255) / 256, n_policies), 256, 0, s>>>(
        wave_offsets, wave_list, partial, wave_sse, wave_wsum, grad, loss);
    return hipGetLastError();
}

hipError_t launch_adam_repack_bank(hipStream_t s, uint32_t n_policies, const uint32_t* wave_offsets, const float* grad, float* w, float* m,
                                   float* v, AdamState* st, const PackGather* table, float* images, float* gimages) {
    if (n_policies == 0) return hipErrorInvalidValue;
    k_adam_repack_bank<<<n_policies, 1024, 0, s>>>(wave_offsets, grad, w, m, v, st, table, (uint32_t)RQ_PACKED_FLOATS,
                                                   (uint32_t)RQ_PACKED_GRAD_FLOATS, images, gimages);
    return hipGetLastError();
}

hipError_t launch_adam_set_lr_bank(hipStream_t s, AdamState* st, uint32_t n_policies, const double* lr, uint32_t n_lr) {
    if (n_lr != 1 && n_lr != n_policies) return hipErrorInvalidValue;
    AdamLrChunk c{};
    for (uint32_t first = 0; first < n_policies; first += 256) {
        const uint32_t count = n_policies - first < 256u ? n_policies - first : 256u;
        if (n_lr == 1) c.lr[0] = lr[0];
        else for (uint32_t i = 0; i < count; ++i) c.lr[i] = lr[first + i];
        k_adam_set_lr_bank<<<1, 256, 0, s>>>(st, first, count, n_lr == 1 ? 0u : 1u, c);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace rq
