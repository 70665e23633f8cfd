// rq_lag_table.inc - the lagged-gain table's kernel, k_policy_lag_table<K>, included by rq_grad.hpp once (after sigm2).
//
// What it sums: A^(k)_t = da_t/dp0_(s_k) [4][16], the Jacobian of the action at live step t with respect to layer_0's pre-activation
// k live steps earlier in the same episode, everything else held fixed - the linearised impulse response of the control law along the
// flown trajectory (the gain at lag k is G^(k) = A^(k) W0; W0 is constant over the recording, so the host multiplies the sums once).
// A^(0) is the gain table's A (rq_gain_table.inc); A^(k) = W2 D_t D_(s_1) .. D_(s_(k-1)) E_(s_k) with D_s = dh'/dh and E_s = dh'/dp0 of
// step s - the learner's reverse sweep (rq_grad_backward.inc) with four action seeds and a sliding window of K lags.
//
// The split is this kernel's own.  ONE WAVE OWNS 16 ENVS for the whole recording, walked backwards: a 16x16 tile of
// v_mfma_f32_16x16x4_f32 is 16 hidden units by the wave's 16 envs FOR ONE ACTION ROW, lane (q, j) holding units 4q .. 4q+3 of env j.
// Four tiles, one per action row i, are one lag's adjoint set dh^(k) = da_t/dh'_s [4 seeds][16 units] per env: 16 VGPRs per lag.
//   * per step s the gates are recomputed ONCE, from the recorded observation and saved[s] - the state entering the step, as the
//     learner's state-saving forward left it - with rq_grad_backward.inc's own block; the elementwise factors of the gate adjoints
//     (1 - z, h - n, 1 - n n, c, r (1 - r), z (1 - z)) are formed once and serve every seed and lag;
//   * the window: slot k >= 1 holds the set that reaches step s from the seed k live steps later; slot 0 is the seed of t = s itself,
//     rows of W2 as they lie in the forward image (W[QW_L2 + 4r + i]).  For k = K-1 .. 0 and every seed: dPr, dPz, dGni, dGnh as the
//     backward forms them; dp0 = m (Wir^T dPr + Wiz^T dPz + Win^T dGni), 12 MFMAs over the transposed image's GW_WIT block, added into
//     sum[k]; and - but for the last slot - dh <- dh' z + Whr^T dPr + Whz^T dPz + Whn^T dGnh, 12 MFMAs over GW_WHT, written to slot
//     k + 1.  Walking k downwards makes that write the window's shift: every register index is static, no tile is moved.
//     The six transposed 16x16 matrices are the register-stationary A operands the backward already packs (pack_policy_grad): 24 VGPRs;
//   * one mask register per lane, bit k = slot k holds the set of a SELECTED seed of this episode.  A live step shifts it, an episode
//     end (done code 1 or 2: the steps behind it in the walk belong to the next episode) clears it before the seed enters, a frozen
//     step (code 4) leaves mask and window as they are.  What a slot without its bit holds is never zeroed and never summed: the bit
//     SELECTS, nothing is multiplied by it - NaN in a frozen observation, an unselected step and a padding column reach no cell (an
//     MFMA keeps an env's values in its own column of N);
//   * the sums live in LDS, [K][4 seeds][64 lanes] float4 - K x 4 KB, 64 KB at K = 16 - each lane adding into its own cells with
//     __fadd_rn in the walk's order: no atomics, no exchange between lanes, no barrier (one wave, lane-private cells), the same bits
//     every run.  The window of K = 16 alone is 240 VGPRs; sums beside it would not fit 512 registers.  The counts are four (K / 4)
//     registers: lane group q counts the lags k = 4m + q;
//   * sum [n_lags][4][16][ld_out] and count [n_lags][ld_out] are stored once at the end, the asked lags only, columns e < n only.
// Instantiated for K = 4, 8, 16; a lag k >= n_lags of a rounded-up instantiation is skipped by a wave-uniform branch.
template <int K>
__global__ __launch_bounds__(64, 1) void k_policy_lag_table(
        uint32_t n, uint32_t ld, uint32_t steps, const float* __restrict__ packed, const float* __restrict__ gpacked,
        const float* __restrict__ obs, const uint8_t* __restrict__ done, const float* __restrict__ saved,
        const uint8_t* __restrict__ select, uint32_t ld_select, uint32_t n_lags, float* __restrict__ sum, uint32_t* __restrict__ count,
        uint32_t ld_out) {
    static_assert(K == 4 || K == 8 || K == 16, "the instantiations: 4, 8 and 16 lags");
    __shared__ f32x4 acc[K * 4 * 64];                          // [lag][seed][lane]: the lane's four rows
    const uint32_t lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15;
    const uint32_t e = blockIdx.x * 16 + j;
    const bool ev = e < n;
    const uint32_t ec = ev ? e : n - 1;                        // padding columns run on the last env's data and are never live
    float W[QW_REGS], G[24];
#pragma unroll
    for (int v = 0; v < QW_H0; ++v) W[v] = packed[qw_slot(v, lane)];          // the learned initial state and b2 are not read
#pragma unroll
    for (int v = 0; v < 24; ++v) G[v] = gpacked[v * 64 + lane];               // GW_WIT, GW_WHT
    static_assert(GW_WIT == 0 && GW_WHT == 12 && QW_H0 > QW_BNH && QW_H0 > QW_L2, "the images' blocks this kernel loads");
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 cbr = {W[QW_BR], W[QW_BR + 1], W[QW_BR + 2], W[QW_BR + 3]};
    const f32x4 cbz = {W[QW_BZ], W[QW_BZ + 1], W[QW_BZ + 2], W[QW_BZ + 3]};
    const f32x4 cbni = {W[QW_BNI], W[QW_BNI + 1], W[QW_BNI + 2], W[QW_BNI + 3]};
    const f32x4 cbnh = {W[QW_BNH], W[QW_BNH + 1], W[QW_BNH + 2], W[QW_BNH + 3]};
    constexpr float kInvT = 1.0f / -2.8853900817779268f;     // the n rows' pre-scale undone: gnh / (-2 log2 e) = W_hn h + b_hn
    // observation features of the B layout: K-step s, k-slot q = feature 4s + q (22 = the constant 1, 23 = 0)
    const uint32_t f5 = 20 + (q < 2 ? q : 1);
    const float x5c = q == 2 ? 1.0f : 0.0f;

#pragma unroll
    for (int c = 0; c < K * 4; ++c) acc[c * 64 + lane] = zero;
    f32x4 win[K][4];                                           // slot 0 is not carried: the seed enters it every step
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) win[k][i] = zero;
    uint32_t mask = 0, cnt[K / 4] = {};
    constexpr uint32_t kAll = (1u << K) - 1u;

    for (uint32_t s = steps; s-- > 0;) {
        float X[6], hp[4];
#pragma unroll
        for (int k = 0; k < 5; ++k) X[k] = obs[((size_t)s * 22 + 4 * k + q) * ld + ec];
        {
            const float v = obs[((size_t)s * 22 + f5) * ld + ec];
            X[5] = q < 2 ? v : x5c;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) hp[r] = saved[((size_t)s * 16 + 4 * q + r) * ld + ec];
        const uint8_t d = done[(size_t)s * ld + ec];
        const bool chosen = select == nullptr || select[(size_t)s * ld_select + ec] != 0;
        const bool live = ev && d != 4;
        if (__builtin_amdgcn_ballot_w64(live) == 0) continue;  // a step the whole wave sat out

        // ---- recompute: layer_0, the gates' chains (bias, W_h h, W_i y0: the forward's order), the gates ----
        f32x4 y0 = mfma16(W[QW_L0], X[0], zero);
#pragma unroll
        for (int k = 1; k < 6; ++k) y0 = mfma16(W[QW_L0 + k], X[k], y0);
#pragma unroll
        for (int r = 0; r < 4; ++r) y0[r] = relu(y0[r]);
        f32x4 gr = mfma16(W[QW_GH + 0], hp[0], cbr);
        f32x4 gz = mfma16(W[QW_GH + 4], hp[0], cbz);
        f32x4 gnh = mfma16(W[QW_GH + 8], hp[0], cbnh);
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            gr = mfma16(W[QW_GH + 0 + k], hp[k], gr);
            gz = mfma16(W[QW_GH + 4 + k], hp[k], gz);
            gnh = mfma16(W[QW_GH + 8 + k], hp[k], gnh);
        }
        f32x4 gni = mfma16(W[QW_GI + 8], y0[0], cbni);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            gr = mfma16(W[QW_GI + 0 + k], y0[k], gr);
            gz = mfma16(W[QW_GI + 4 + k], y0[k], gz);
            if (k > 0) gni = mfma16(W[QW_GI + 8 + k], y0[k], gni);
        }
        // the factors of the gate adjoints, the backward's own sub-expressions: shared by the four seeds and every lag
        float rr[4], zz[4], omz[4], hmn[4], omn[4], cc[4], rr1[4], zz1[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            rr[r] = sigm2(gr[r]);
            zz[r] = sigm2(gz[r]);
            const float nn = fmaf(2.0f, sigm2(fmaf(rr[r], gnh[r], gni[r])), -1.0f);
            omz[r] = 1.0f - zz[r];
            hmn[r] = hp[r] - nn;
            omn[r] = 1.0f - nn * nn;
            cc[r] = gnh[r] * kInvT;
            rr1[r] = rr[r] * (1.0f - rr[r]);
            zz1[r] = zz[r] * (1.0f - zz[r]);
        }

        // ---- the episode structure, backwards: an end cuts every chain from later steps; then the seed of t = s enters ----
        const bool ended = d == 1 || d == 2;
        const uint32_t cur = live ? ((ended ? 0u : mask) | (chosen ? 1u : 0u)) : 0u;      // bit k: slot k counts at this step
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) win[0][i][r] = W[QW_L2 + 4 * r + i];
#pragma unroll
        for (int m = 0; m < K / 4; ++m) cnt[m] += (cur >> (4 * m + q)) & 1u;

#pragma unroll
        for (int k = K - 1; k >= 0; --k) {
            if ((uint32_t)k >= n_lags) continue;               // wave-uniform: a rounded-up instantiation
            const bool on = ((cur >> k) & 1u) != 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float dPr[4], dPz[4], dGni[4], dGnh[4];
                f32x4 dhd;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float dh = win[k][i][r];
                    const float dn = dh * omz[r];
                    const float dz = dh * hmn[r];
                    dhd[r] = dh * zz[r];
                    const float du = dn * omn[r];
                    dPr[r] = du * cc[r] * rr1[r];
                    dPz[r] = dz * zz1[r];
                    dGni[r] = du;
                    dGnh[r] = du * rr[r];
                }
                f32x4 dy0 = mfma16(G[GW_WIT + 0], dPr[0], zero);
#pragma unroll
                for (int r = 1; r < 4; ++r) dy0 = mfma16(G[GW_WIT + r], dPr[r], dy0);
#pragma unroll
                for (int r = 0; r < 4; ++r) dy0 = mfma16(G[GW_WIT + 4 + r], dPz[r], dy0);
#pragma unroll
                for (int r = 0; r < 4; ++r) dy0 = mfma16(G[GW_WIT + 8 + r], dGni[r], dy0);
                f32x4 a = acc[(k * 4 + i) * 64 + lane];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float dp0 = y0[r] > 0.0f ? dy0[r] : 0.0f;          // ReLU'(0) = 0
                    a[r] = on ? __fadd_rn(a[r], dp0) : a[r];                 // selected, never multiplied
                }
                acc[(k * 4 + i) * 64 + lane] = a;
                if (k + 1 < K && (uint32_t)(k + 1) < n_lags) {               // one step back, into the next slot: the window's shift
                    f32x4 dhp = mfma16(G[GW_WHT + 0], dPr[0], dhd);
#pragma unroll
                    for (int r = 1; r < 4; ++r) dhp = mfma16(G[GW_WHT + r], dPr[r], dhp);
#pragma unroll
                    for (int r = 0; r < 4; ++r) dhp = mfma16(G[GW_WHT + 4 + r], dPz[r], dhp);
#pragma unroll
                    for (int r = 0; r < 4; ++r) dhp = mfma16(G[GW_WHT + 8 + r], dGnh[r], dhp);
#pragma unroll
                    for (int r = 0; r < 4; ++r) win[(k + 1) % K][i][r] = live ? dhp[r] : win[(k + 1) % K][i][r];
                }
            }
        }
        mask = live ? (cur << 1) & kAll : mask;
    }

    if (ev) {
        const size_t plane = (size_t)16 * ld_out;             // one seed of one lag
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if ((uint32_t)k >= n_lags) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 a = acc[(k * 4 + i) * 64 + lane];
#pragma unroll
                for (int r = 0; r < 4; ++r) sum[((size_t)k * 4 + i) * plane + (size_t)(4 * q + r) * ld_out + e] = a[r];
            }
            if ((uint32_t)(k & 3) == q) count[(size_t)k * ld_out + e] = cnt[k >> 2];
        }
    }
}
