// rq_actor_step.inc - the actor step of the chained rollout, rq_policy_evaluate_step and the small-batch loop, one 64-env group per
// wave; included once per kernel (rq_kernels.hip):
//   RQ_ACTOR_KERNEL  the kernel's name
//   RQ_ACTOR_BANK    0: one policy, its operand image `packed`; host rows in and out and the host flag (Mailbox).
//                    1: a policy bank - the image of the wave's 64-env block (block = wave_base / 64), images + block_policy[block] *
//                       image_floats; no host rows.  The wave index is made a scalar first: the table reads are then scalar loads too.
//   RQ_ACTOR_RATE    0: the hidden state is written back for every row that commits; one policy has its SampleAndSquash stage and may
//                       read the state from a buffer of its own (hidden_in: speculation).
//                    1: a native interval above 1 (rq_policy_set_native_interval; a bank: policy_interval[policy], every entry 1 ..
//                       RQ_POLICY_MAX_NATIVE_INTERVAL) - the same loads, the same ACTOR::step, the same action stores, and the hidden
//                       state written back only for the rows at a native step: steps[i] % interval == 0 (the env's episode step count
//                       at this step's observation; the env step moves it on), or, one policy without `steps`, every row iff native.
// One text for the four, and each a kernel of its own with its own argument block: graph_add copies a node's arguments by the kernel's
// signature, and the profiles name the kernels.
//
// MFMA ignores the EXEC mask and mixes the lanes of a wave, so every MFMA must execute in wave-uniform control flow with all 64 lanes
// holding valid data: lanes past the end of the batch (and frozen envs) compute on a clamped index and only their STORES are
// predicated - no lane leaves early.
template <typename ACTOR>
#if RQ_ACTOR_BANK && RQ_ACTOR_RATE
__global__ __launch_bounds__(kBlock, 2) void RQ_ACTOR_KERNEL(uint32_t n, const float* __restrict__ images,
                                                            const uint32_t* __restrict__ block_policy,
                                                            const uint32_t* __restrict__ policy_interval, uint32_t image_floats,
                                                            const float* __restrict__ obs, uint32_t ld_obs,
                                                            float* hidden, uint32_t ld_h, float* __restrict__ act, uint32_t ld_act,
                                                            const uint8_t* __restrict__ frozen, const uint32_t* __restrict__ steps) {
#elif RQ_ACTOR_BANK
__global__ __launch_bounds__(kBlock, 2) void RQ_ACTOR_KERNEL(uint32_t n, const float* __restrict__ images,
                                                            const uint32_t* __restrict__ block_policy, uint32_t image_floats,
                                                            const float* __restrict__ obs, uint32_t ld_obs,
                                                            float* hidden, uint32_t ld_h, float* __restrict__ act, uint32_t ld_act,
                                                            const uint8_t* __restrict__ frozen) {
#elif RQ_ACTOR_RATE
__global__ __launch_bounds__(kBlock, 2) void RQ_ACTOR_KERNEL(uint32_t n, const float* __restrict__ packed,
                                                            const float* __restrict__ obs, uint32_t ld_obs,
                                                            float* hidden, uint32_t ld_h, float* __restrict__ act, uint32_t ld_act,
                                                            const uint8_t* __restrict__ frozen,
                                                            const uint32_t* __restrict__ steps, uint32_t interval, uint32_t native,
                                                            Mailbox mb) {
#else
__global__ __launch_bounds__(kBlock, 2) void RQ_ACTOR_KERNEL(uint32_t n, const float* __restrict__ packed,
                                                            const float* __restrict__ obs, uint32_t ld_obs,
                                                            const float* hidden_in, float* hidden,   // the same buffer unless speculative
                                                            uint32_t ld_h, float* __restrict__ act, uint32_t ld_act,
                                                            const uint8_t* __restrict__ frozen, SasArgs sas,
                                                            Mailbox mb) {
#endif
#if RQ_ACTOR_BANK
    constexpr Mailbox mb{};
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t wave_base = wave * 64u;
    if (wave_base >= n) return;                                  // wave-uniform; the table has ceil(n / 64) entries
    const uint32_t policy = block_policy[wave];
#if RQ_ACTOR_RATE
    const uint32_t interval = policy_interval[policy];
#endif
    ACTOR actor;
    actor.template load<kBlock / 64>(images + (size_t)policy * image_floats);
    const uint32_t lane = threadIdx.x & 63;
#else
    ACTOR actor;
    actor.template load<kBlock / 64>(packed);     // 18 KB of operand image per wave
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave_base = ((blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 64;
    if (wave_base >= n) { mailbox_signal(mb); return; }          // wave-uniform
#endif
#if RQ_ACTOR_BANK || RQ_ACTOR_RATE
    constexpr SasArgs sas{};
    const float* const hidden_in = hidden;
#endif
    const uint32_t i0 = wave_base + lane;
    const uint32_t i = i0 < n ? i0 : n - 1;
    float x[22], hQ[4][4], a[4];
    if (mb.rows_in != nullptr) {         // wave-uniform (kernel argument)
#pragma unroll
        for (int k = 0; k < 22; ++k) x[k] = mb.rows_in[(size_t)i * mb.in_stride + k];
    } else {
#pragma unroll
        for (int k = 0; k < 22; ++k) x[k] = field(obs, k, ld_obs)[i];
    }
    load_hidden_q(hidden_in, ld_h, wave_base, n, hQ);      // == hidden unless the new state goes elsewhere (speculation)
    const uint32_t fz = frozen != nullptr ? (uint32_t)frozen[i] : 0u;
    const bool commit = (i0 < n) && fz == 0;
#if RQ_ACTOR_BANK && RQ_ACTOR_RATE
    const bool at_native = steps[i] % interval == 0;
    const uint64_t hidden_mask = __builtin_amdgcn_ballot_w64(commit && at_native);
#elif RQ_ACTOR_RATE
    const bool at_native = steps != nullptr ? steps[i] % interval == 0 : native != 0;
    const uint64_t hidden_mask = __builtin_amdgcn_ballot_w64(commit && at_native);
#else
    const uint64_t hidden_mask = __builtin_amdgcn_ballot_w64(commit);
#endif
    actor.step(x, hQ, a);
    if (sas.mode)                        // wave-uniform (kernel argument)
        sample_and_squash(sas, sas.epoch + (sas.epoch_base != nullptr ? *sas.epoch_base : 0u), sas.env_offset + i, hQ, a);
    store_hidden_q(hidden, ld_h, wave_base, hidden_mask, hQ);
    if (commit) {
#pragma unroll
        for (int k = 0; k < 4; ++k) field(act, k, ld_act)[i] = a[k];
        if (mb.rows_out != nullptr) {
#pragma unroll
            for (int k = 0; k < 4; ++k) mb.rows_out[(size_t)i * 4 + k] = a[k];
        }
    }
    mailbox_signal(mb);
}
#undef RQ_ACTOR_KERNEL
#undef RQ_ACTOR_BANK
#undef RQ_ACTOR_RATE
