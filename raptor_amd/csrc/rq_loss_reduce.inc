// rq_loss_reduce.inc - the body of the seeded backward's reduction, included once per kernel:
//   RQ_LOSS_REDUCE_KERNEL  the kernel's name
//   RQ_GRAD_BANK           0: one policy, the waves 0 .. waves-1 in that order -> grad [2084], loss [1] (rq_grad.hpp)
//                          1: policy blockIdx.y, its waves from a CSR list in ascending order (wave_offsets [P + 1] into wave_list) ->
//                             grad [p][2084], loss [p] (rq_grad_bank.hpp).  A policy that owns no wave: loss NaN, its gradient row is
//                             not written
//   RQ_GRAD_WEIGHTED       0 or not defined: the normaliser is M = the waves' wave_live added up, an integer sum (4 x the live
//                             env-steps); the single policy's kernel also stores it, live_out[0] = M
//                          1: it is W4 = the waves' wave_wsum added in the walk's order in float64 - every thread adds them itself,
//                             beside the partials it is walking anyway: one order, no exchange
// One text for the four, and each a kernel of its own rather than a call into a shared function: a kernel's listing stays what it was.
//
// grad = the partials summed in the walk's order x 2 / normaliser, with the scale applied once - the product in float64, one rounding
// to fp32 - and loss = SSE / normaliser with the waves' SSE summed in the same order.  Normaliser 0 (every step frozen, or nothing
// counts): loss and gradient 0, and Adam sees a zero gradient.  With every weight 1.0f W4 is the integer M exactly and the weighted
// results are the unweighted bits; a bank's policy gets what a recording that holds its blocks only, in order, would give.
#ifndef RQ_GRAD_WEIGHTED
#define RQ_GRAD_WEIGHTED 0
#endif
#if RQ_GRAD_BANK
#define RQ_WAVE(k) wave_list[k]
#define RQ_UNROLL_WAVES
#else
#define RQ_WAVE(k) (k)
#define RQ_UNROLL_WAVES _Pragma("unroll 8")
#endif
__global__ __launch_bounds__(256) void RQ_LOSS_REDUCE_KERNEL(
#if RQ_GRAD_BANK
        const uint32_t* __restrict__ wave_offsets, const uint32_t* __restrict__ wave_list,
#else
        uint32_t waves,
#endif
        const float* __restrict__ partial, const float* __restrict__ wave_sse,
#if RQ_GRAD_WEIGHTED
        const double* __restrict__ wave_wsum, float* __restrict__ grad, float* __restrict__ loss) {
#elif RQ_GRAD_BANK
        const uint32_t* __restrict__ wave_live, float* __restrict__ grad, float* __restrict__ loss) {
#else
        const uint32_t* __restrict__ wave_live, float* __restrict__ grad, float* __restrict__ loss,
        unsigned long long* __restrict__ live_out) {
#endif
#if RQ_GRAD_BANK
    const uint32_t pol = blockIdx.y, w0 = wave_offsets[pol], w1 = wave_offsets[pol + 1];
#else
    const uint32_t pol = 0, w0 = 0, w1 = waves;
#endif
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
#if RQ_GRAD_BANK
    if (w0 == w1) {                     // uniform for the workgroup
#if RQ_GRAD_WEIGHTED
        if (p == 0) loss[pol] = __builtin_nanf("");
#else
        if (blockIdx.x == 0 && threadIdx.x == 0) loss[pol] = __builtin_nanf("");
#endif
        return;
    }
#endif
#if RQ_GRAD_WEIGHTED
    if (p >= RQ_POLICY_NUM_WEIGHTS) return;
    float acc = 0.0f;
    double W4 = 0.0;
    RQ_UNROLL_WAVES
    for (uint32_t k = w0; k < w1; ++k) {
        const uint32_t w = RQ_WAVE(k);
        acc += partial[(size_t)w * RQ_POLICY_NUM_WEIGHTS + p];
        W4 += wave_wsum[w];
    }
    const bool any = W4 > 0.0;
    const double inv = any ? 1.0 / W4 : 0.0;
    grad[(size_t)pol * RQ_POLICY_NUM_WEIGHTS + p] = any ? (float)((double)acc * (2.0 * inv)) : 0.0f;
    if (p == 0) {
        float sse = 0.0f;
        RQ_UNROLL_WAVES
        for (uint32_t k = w0; k < w1; ++k) sse += wave_sse[RQ_WAVE(k)];
        loss[pol] = any ? (float)((double)sse * inv) : 0.0f;
    }
#else
    __shared__ unsigned long long cnt[256];
    unsigned long long mine = 0;
    for (uint32_t k = w0 + threadIdx.x; k < w1; k += 256) mine += wave_live[RQ_WAVE(k)];
    cnt[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) cnt[threadIdx.x] += cnt[threadIdx.x + h];
        __syncthreads();
    }
    const unsigned long long M = cnt[0];
    const double inv = M ? 1.0 / (double)M : 0.0;
    if (p < RQ_POLICY_NUM_WEIGHTS) {
        float acc = 0.0f;
        RQ_UNROLL_WAVES
        for (uint32_t k = w0; k < w1; ++k) acc += partial[(size_t)RQ_WAVE(k) * RQ_POLICY_NUM_WEIGHTS + p];
        grad[(size_t)pol * RQ_POLICY_NUM_WEIGHTS + p] = M ? (float)((double)acc * (2.0 * inv)) : 0.0f;
    }
    if (p == 0) {
        float acc = 0.0f;
        RQ_UNROLL_WAVES
        for (uint32_t k = w0; k < w1; ++k) acc += wave_sse[RQ_WAVE(k)];
        loss[pol] = M ? (float)((double)acc * inv) : 0.0f;
#if !RQ_GRAD_BANK
        live_out[0] = M;
#endif
    }
#endif
}
#undef RQ_WAVE
#undef RQ_UNROLL_WAVES
#undef RQ_LOSS_REDUCE_KERNEL
#undef RQ_GRAD_BANK
#undef RQ_GRAD_WEIGHTED
