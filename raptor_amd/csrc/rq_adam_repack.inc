// rq_adam_repack.inc - the body of the Adam-and-repack kernel, included once per kernel:
//   RQ_ADAM_KERNEL  the kernel's name
//   RQ_GRAD_BANK    0: one workgroup on one policy's grad / w / m / v [2084], st, packed, gpacked (k_adam_repack, rq_grad.hpp)
//                   1: workgroup p on slot p of grad / w / m / v [P][2084], st [P] (every hyper-parameter per policy), packed
//                      [P][n_forward] and gpacked [P][n_grad], through the one gather table (k_adam_repack_bank, rq_grad_bank.hpp).  A
//                      policy that owns no wave in this assignment (wave_offsets, the CSR list of the reduction) has no gradient: its
//                      weights, moments, step count and images stay as they were.
// One text for both, and each a kernel of its own rather than a call into a shared function (that changed both listings).
//
// Adam (torch.optim.Adam's update; weight_decay decoupled as in AdamW) on the device's master weights, then both fp32 operand
// images rebuilt from them.  Hyper-parameters, the step count and the running powers beta^t live in device memory (AdamState), so
// that updates queue back to back.  Per element, in float64 from the fp32 inputs and rounded to fp32 once each:
//     m' = beta1 m + (1 - beta1) g,  v' = beta2 v + (1 - beta2) g g,
//     w' = w (1 - lr wd) - lr (m' / (1 - beta1^t)) / (sqrt(v' / (1 - beta2^t)) + eps)
// The images come from a gather table (rq_pack.cpp pack_gather_table: pack_policy / pack_policy_grad run on symbols): element e is
// 0, k w[a] or k (w[a] + w[b]) in fp32 - the host packers' expressions, no contraction - so the images equal theirs bit for bit.
#if RQ_GRAD_BANK
__global__ __launch_bounds__(1024) void RQ_ADAM_KERNEL(const uint32_t* __restrict__ wave_offsets, const float* __restrict__ grad_all,
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
#else
__global__ __launch_bounds__(1024) void RQ_ADAM_KERNEL(const float* __restrict__ grad, float* __restrict__ w, float* __restrict__ m,
                                                       float* __restrict__ v, AdamState* __restrict__ st,
                                                       const PackGather* __restrict__ table, uint32_t n_forward, uint32_t n_grad,
                                                       float* __restrict__ packed, float* __restrict__ gpacked) {
    __shared__ float ws[RQ_POLICY_NUM_WEIGHTS];
#endif
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
#undef RQ_ADAM_KERNEL
#undef RQ_GRAD_BANK
