// rq_grad_forward.inc - the body of the learner's forward kernel, included by rq_grad.hpp once per kernel:
//   RQ_GRAD_FORWARD_KERNEL   the kernel's name
//   RQ_GRAD_STORE_ACT        1: the actions are written to act [t][4][ld_act] (k_policy_grad_forward); 0: they are not, and the
//                            kernel has no such parameters (k_policy_grad_forward_state: the distillation update's pass)
//   RQ_GRAD_BANK             1: the wave's image is that of its block's policy, images + block_policy[blockIdx.x] * image_floats
//                            (k_policy_grad_forward_state_bank: one workgroup = one wave = one 64-env block); 0: `packed` is it
// One text for both, and each a kernel of its own rather than a call into a shared function: the existing kernel's listing stays
// the parent build's to the instruction.
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
        float* __restrict__ saved) {
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
    for (uint32_t t = 0; t < steps; ++t) {
        float x[22], a[4], hn[4][4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) saved[((size_t)t * 16 + 4 * q + r) * ld + wave_base + 16 * tt + j] = hQ[tt][r];
#pragma unroll
        for (int k = 0; k < 22; ++k) x[k] = field(obs, t * 22 + k, ld)[i];
        const uint8_t d = done[(size_t)t * ld + i];
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
    }
}
#undef RQ_GRAD_FORWARD_KERNEL
#undef RQ_GRAD_STORE_ACT
#undef RQ_GRAD_BANK
