// rq_probe_moments.inc - the body of the probe's moment kernel, included by rq_probe.hip once per kernel:
//   RQ_PROBE_KERNEL  the kernel's name
//   RQ_PROBE_TIMED   0: targets constant over time, y [n_targets][ld_y] (k_probe_moments): written into the lane's row once, selected
//                       to 0.0f on padding lanes and beyond n_targets
//                    1: targets per step, y [steps][n_targets][ld_y] (k_probe_moments_timed): the lane's n_targets values of step s + 1
//                       are loaded beside its 16 state rows while step s is contracted, and written into its row beside h every step -
//                       raw, like h: what is not live, not in a bucket or a padding lane is selected away where the tile is read
//                       (`in`), so NaN there reaches no sum.  Columns 17 + n_targets .. 31 are zeroed once.
// One text for both, and each a kernel of its own rather than a call into a shared function: a kernel's listing stays what it was.
// Every bucket decision, flush and MFMA is the same text in the same order: targets constant over time give the untimed bits.
__global__ __launch_bounds__(64) void RQ_PROBE_KERNEL(uint32_t n, uint32_t ld, uint32_t steps, const float* __restrict__ saved,
                                                      const uint8_t* __restrict__ done, const float* __restrict__ y, uint32_t ld_y,
                                                      uint32_t n_targets, const ProbeEdges edges, uint32_t n_buckets,
                                                      float* __restrict__ partial, uint32_t* __restrict__ wave_counts) {
    __shared__ float zt[64 * PZ_ROW];
    __shared__ uint32_t ed[kProbeMaxBuckets + 1];
    const uint32_t lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15;
    const uint32_t wave = blockIdx.x, e = wave * 64 + lane;
    const bool ev = e < n;                           // e < ld (the launcher checks): the forward saved the state of every column
    const uint32_t ey = ev ? e : 0u;                 // padding lanes read env 0's targets and select them away (their bucket is -1)
    if (lane <= n_buckets) ed[lane] = edges.v[lane];
    float* row = zt + lane * PZ_ROW;
    row[0] = 1.0f;
#if RQ_PROBE_TIMED
#pragma unroll
    for (uint32_t m = 0; m < kProbeMaxTargets; ++m) row[17 + m] = 0.0f;
#else
#pragma unroll
    for (uint32_t m = 0; m < kProbeMaxTargets; ++m) {
        const float v = y[(size_t)(m < n_targets ? m : 0u) * ld_y + ey];
        row[17 + m] = ev && m < n_targets ? v : 0.0f;
    }
#endif
    __syncthreads();
    const uint32_t idx0 = ed[0] == 0u ? 1u : 0u;     // edges <= age 0
    uint32_t age = 0, idx = idx0;

    float* const wave_slot = partial + (size_t)wave * n_buckets * PZ_TILE;
    uint32_t* const wave_count = wave_counts + (size_t)wave * n_buckets;
    const pf32x4 zero = {0.f, 0.f, 0.f, 0.f};
    pf32x4 s00 = zero, s01 = zero, s11 = zero;
    uint32_t cnt = 0, touched = 0;
    int cur = -1;                                     // the bucket in flight (wave-uniform)

#if RQ_PROBE_TIMED
    float hn[16], yn[kProbeMaxTargets];
#else
    float hn[16];
#endif
    uint32_t dn = 4;
#pragma unroll
    for (int r = 0; r < 16; ++r) hn[r] = saved[(size_t)r * ld + e];
#if RQ_PROBE_TIMED
#pragma unroll
    for (uint32_t m = 0; m < kProbeMaxTargets; ++m) yn[m] = m < n_targets ? y[(size_t)m * ld_y + ey] : 0.0f;
#endif
    dn = done[e];

    for (uint32_t s = 0; s < steps; ++s) {
#if RQ_PROBE_TIMED
        float h[16], yv[kProbeMaxTargets];
#else
        float h[16];
#endif
#pragma unroll
        for (int r = 0; r < 16; ++r) h[r] = hn[r];
#if RQ_PROBE_TIMED
#pragma unroll
        for (uint32_t m = 0; m < kProbeMaxTargets; ++m) yv[m] = yn[m];
#endif
        const uint32_t d = dn;
        if (s + 1 < steps) {                          // the next step's rows are on their way while this one is contracted
#pragma unroll
            for (int r = 0; r < 16; ++r) hn[r] = saved[((size_t)(s + 1) * 16 + r) * ld + e];
#if RQ_PROBE_TIMED
#pragma unroll
            for (uint32_t m = 0; m < kProbeMaxTargets; ++m)
                if (m < n_targets) yn[m] = y[((size_t)(s + 1) * n_targets + m) * ld_y + ey];
#endif
            dn = done[(size_t)(s + 1) * ld + e];
        }
        const bool live = ev && d != 4u;
        const int bk = live && idx >= 1u && idx <= n_buckets ? (int)idx - 1 : -1;
#pragma unroll
        for (int r = 0; r < 16; ++r) row[1 + r] = h[r];
#if RQ_PROBE_TIMED
#pragma unroll
        for (uint32_t m = 0; m < kProbeMaxTargets; ++m)
            if (m < n_targets) row[17 + m] = yv[m];
#endif
        row[PZ_BUCKET] = __int_as_float(bk);
        if (live) {
            if (d == 1u || d == 2u) { age = 0; idx = idx0; }
            else {
                ++age;
                if (idx <= n_buckets && ed[idx] == age) ++idx;
            }
        }
        __syncthreads();

        uint64_t todo = __builtin_amdgcn_ballot_w64(bk >= 0);
        bool head = true;
        while (todo) {
            int b;
            const uint64_t in_cur = head && cur >= 0 ? __builtin_amdgcn_ballot_w64(bk == cur) : 0ull;
            if (in_cur) b = cur;
            else b = __builtin_amdgcn_readlane(bk, (int)__builtin_ctzll(todo));
            head = false;
            const uint64_t members = __builtin_amdgcn_ballot_w64(bk == b);
            todo &= ~members;
            if (b != cur) {
                if (cur >= 0) {
                    probe_flush(wave_slot + (size_t)cur * PZ_TILE, wave_count + cur, !((touched >> cur) & 1u), lane, s00, s01, s11, cnt);
                    touched |= 1u << cur;
                }
                s00 = s01 = s11 = zero;
                cnt = 0;
                cur = b;
            }
            cnt += (uint32_t)__builtin_popcountll(members);
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                if (((members >> (4 * u)) & 0xfull) == 0) continue;          // none of envs 4u .. 4u+3 is in the bucket: exact zeros
                const float* src = zt + (4 * u + q) * PZ_ROW;                // k-slot q = env 4u + q of the wave
                const bool in = __float_as_int(src[PZ_BUCKET]) == b;
                const float lo = in ? src[j] : 0.0f, hi = in ? src[16 + j] : 0.0f;
                s00 = probe_mfma(lo, lo, s00);
                s01 = probe_mfma(lo, hi, s01);
                s11 = probe_mfma(hi, hi, s11);
            }
        }
        __syncthreads();
    }
    if (cur >= 0) {
        probe_flush(wave_slot + (size_t)cur * PZ_TILE, wave_count + cur, !((touched >> cur) & 1u), lane, s00, s01, s11, cnt);
        touched |= 1u << cur;
    }
    for (uint32_t b = 0; b < n_buckets; ++b)          // a bucket this wave never met: zeros, so that the reduction reads no stale word
        if (!((touched >> b) & 1u)) probe_flush(wave_slot + (size_t)b * PZ_TILE, wave_count + b, true, lane, zero, zero, zero, 0u);
}
#undef RQ_PROBE_KERNEL
#undef RQ_PROBE_TIMED
