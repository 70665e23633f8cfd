// rq_thaw_frozen.inc - the thaw of a chained rollout under auto-reset, included once per kernel (rq_kernels.hip):
//   RQ_THAW_KERNEL  the kernel's name
//   RQ_THAW_BANK    0: one policy - the policy state returns to the initial state in `weights` (checkpoint order)
//                   1: a policy bank - to the initial state of the env's OWN policy: block block_policy[i >> 6] of weights
//                      [P][RQ_POLICY_NUM_WEIGHTS]
// Envs left frozen by an earlier rollout start their next episode (sample_initial_state with the env's episode counter, policy
// state reset), as the fused kernel's prologue does.  One text for both, and each a kernel of its own rather than a call into a
// shared function (that changed both listings).
__global__ __launch_bounds__(kBlock) void RQ_THAW_KERNEL(Batch b, SampleCfg c, uint64_t seed,
                                                         const float* __restrict__ params, float* __restrict__ state,
                                                         StatsPtrs st, float* __restrict__ hidden,
#if RQ_THAW_BANK
                                                         const float* __restrict__ weights,
                                                         const uint32_t* __restrict__ block_policy) {
#else
                                                         const float* __restrict__ w) {
#endif
    const uint32_t i = env_index();
    if (i >= b.n || !st.frozen[i]) return;
    const size_t ld = b.ld;
    const uint32_t ep = st.episode[i];
#if RQ_THAW_BANK
    const float* w = weights + (size_t)block_policy[i >> 6] * RQ_POLICY_NUM_WEIGHTS;
#endif
    float s[17], la[4], f[6];
    sample_state(c, seed, ep, b.env_offset + i, field(params, RQ_P_MASS, ld)[i], field(params, RQ_P_HOVER_RPM, ld)[i],
                 field(params, RQ_P_ROTOR_POS, ld)[i], field(params, (RQ_P_ROTOR_POS + 1), ld)[i], s, la, f);
#pragma unroll
    for (int k = 0; k < 17; ++k) field(state, k, ld)[i] = s[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) field(state, (RQ_S_LAST_ACTION + k), ld)[i] = la[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) field(state, (RQ_S_FORCE + k), ld)[i] = f[k];
#pragma unroll
    for (int j = 0; j < 16; ++j) field(hidden, j, ld)[i] = w[OFF_H0 + j];
    st.episode[i] = ep + 1;
    st.frozen[i] = 0;
}
#undef RQ_THAW_KERNEL
#undef RQ_THAW_BANK
