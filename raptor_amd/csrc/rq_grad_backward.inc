// rq_grad_backward.inc - the body of the learner's backward kernel, included by rq_grad.hpp once per kernel:
//   RQ_GRAD_BACKWARD_KERNEL  the kernel's name
//   RQ_GRAD_SEEDED           0: dL/da is read from gact (k_policy_grad_backward)
//                            1: it is formed here from the masked squared error against a target (k_policy_loss_backward)
//   RQ_GRAD_BANK             1: both images are those of the wave's policy, images + block_policy[blockIdx.x] * image_floats and
//                            gimages + block_policy[blockIdx.x] * gimage_floats (k_policy_loss_backward_bank); 0: `packed`, `gpacked`
//   RQ_GRAD_WEIGHTED         with RQ_GRAD_SEEDED 1 only; 1: every entry carries a weight w (k_policy_loss_backward_weighted, ..._bank),
//                            below; 0 or not defined: none
// One text for all, and each a kernel of its own rather than a call into a shared function: the existing kernel's listing stays
// the parent build's to the instruction.
//
// RQ_GRAD_SEEDED: `target` y [steps][4][ld_y].  From the recomputed h' the action is the forward's own layer_2 (ActorF32T::run): the
// lane's slice p_i = the fma chain over r of W2[i][4q+r] h'[4q+r] starting from b2[i] (lane group 0) or 0, through LDS to the four
// lanes of the env, a_i = (p_i@0 + p_i@1) + (p_i@2 + p_i@3): the bits rq_trajectory_policy_forward stores.  Lane (q, j) then holds
// dL/da_q = a_q - y_q of env (t, j) where the entry is live (done code != 4, column < n) and 0 elsewhere - selected, never
// multiplied, so NaN in the targets or in the observations of frozen steps goes nowhere.  The 2 / M of the mean is applied once, by
// the reduction.  Beside its partials the wave leaves its squared error (lane-local sums, folded lane 0 .. 63) and its count of
// live entries in wave_sse / wave_live [gridDim.x].
//
// RQ_GRAD_WEIGHTED: `weight` w [1 or steps][ld_w], env i of step s at weight[s * w_step + i] (w_step = 0: one weight per env for
// every step; ld_w: one per env and step).  An entry COUNTS where it is live and w > 0 - a weight that is 0, negative or NaN drops it,
// selected like the frozen steps, so NaN in its target goes nowhere either.  On a counting entry e = a - y, dL/da = fl(w e) before the
// 2 / W4 of the reduction, and its squared error is fl(fl(w e) e): with w = 1.0f both are the unweighted kernel's bits.  In place of
// the live count the wave leaves W4's share, the sum of w over its counting entries (so each env-step's weight four times): per lane
// in float64 in the order the lane walks its entries, the lanes folded 0 .. 63 in float64, in wave_wsum [gridDim.x].
#ifndef RQ_GRAD_WEIGHTED
#define RQ_GRAD_WEIGHTED 0
#endif
#if RQ_GRAD_WEIGHTED && !RQ_GRAD_SEEDED
#error "RQ_GRAD_WEIGHTED weights the loss seed: it needs RQ_GRAD_SEEDED 1"
#endif
__global__ __launch_bounds__(64, 1) void RQ_GRAD_BACKWARD_KERNEL(
        uint32_t n, uint32_t ld, uint32_t steps,
#if RQ_GRAD_BANK
        const float* __restrict__ images, const float* __restrict__ gimages, const uint32_t* __restrict__ block_policy,
        uint32_t image_floats, uint32_t gimage_floats,
#else
        const float* __restrict__ packed, const float* __restrict__ gpacked,
#endif
        const float* __restrict__ obs, const uint8_t* __restrict__ done, const float* __restrict__ saved,
#if RQ_GRAD_SEEDED
        const float* __restrict__ target, uint32_t ld_y,
#if RQ_GRAD_WEIGHTED
        const float* __restrict__ weight, uint32_t ld_w, uint32_t w_step,
#endif
        uint32_t start_initial, float* __restrict__ partial,
#if RQ_GRAD_WEIGHTED
        float* __restrict__ wave_sse, double* __restrict__ wave_wsum) {
    __shared__ double wfold[64];
    double wsum = 0.0;                  // this lane's weights of counting entries
#else
        float* __restrict__ wave_sse, uint32_t* __restrict__ wave_live) {
    uint32_t live_entries = 0;          // the wave's live entries
#endif
    float* const gh_start = nullptr;
    __shared__ float red[16 * 17];      // row = env of the tile, column 4 q + i = p_i of lane group q
    float sse = 0.0f;                   // this lane's squared errors
#else
        const float* __restrict__ gact, uint32_t ld_g, uint32_t start_initial, float* __restrict__ gh_start,
        float* __restrict__ partial) {
#endif
#if RQ_GRAD_BANK
    const float* __restrict__ packed = images + (size_t)block_policy[blockIdx.x] * image_floats;
    const float* __restrict__ gpacked = gimages + (size_t)block_policy[blockIdx.x] * gimage_floats;
#endif
    __shared__ float tile[16 * GL_ROW];
    __shared__ float sums[64 * GRAD_LANE_SUMS];
    const uint32_t lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15;
    const uint32_t wave_base = blockIdx.x * 64;
    float W[QW_REGS], G[GW_REGS];
#pragma unroll
    for (int v = 0; v < QW_REGS; ++v) W[v] = packed[qw_slot(v, lane)];
#pragma unroll
    for (int v = 0; v < GW_REGS; ++v) G[v] = gpacked[v * 64 + lane];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 cbr = {W[QW_BR], W[QW_BR + 1], W[QW_BR + 2], W[QW_BR + 3]};
    const f32x4 cbz = {W[QW_BZ], W[QW_BZ + 1], W[QW_BZ + 2], W[QW_BZ + 3]};
    const f32x4 cbni = {W[QW_BNI], W[QW_BNI + 1], W[QW_BNI + 2], W[QW_BNI + 3]};
    const f32x4 cbnh = {W[QW_BNH], W[QW_BNH + 1], W[QW_BNH + 2], W[QW_BNH + 3]};
    constexpr float kInvT = 1.0f / -2.8853900817779268f;     // the n rows' pre-scale undone: gnh / (-2 log2 e) = W_hn h + b_hn

    f32x4 aWi[3] = {zero, zero, zero}, aWh[3] = {zero, zero, zero}, aW0[2] = {zero, zero}, aW2 = zero;
    float bR[4] = {}, bZ[4] = {}, bNI[4] = {}, bNH[4] = {}, bH0[4] = {}, bB2 = 0.0f;
    float dc[4][4] = {};
    // observation features of the B layout: K-step s, k-slot q = feature 4s + q (22 = the constant 1, 23 = 0)
    const uint32_t f5 = 20 + (q < 2 ? q : 1);
    const float x5c = q == 2 ? 1.0f : 0.0f;

    for (uint32_t s = steps; s-- > 0;) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint32_t e = wave_base + 16 * t + j;           // < ld: the state of every column was saved
            const bool ev = e < n;
            const uint32_t ec = ev ? e : n - 1;                  // padding columns run on the last env's data, as the forward
            float X[6], hp[4];
#pragma unroll
            for (int k = 0; k < 5; ++k) X[k] = obs[((size_t)s * 22 + 4 * k + q) * ld + ec];
            {
                const float v = obs[((size_t)s * 22 + f5) * ld + ec];
                X[5] = q < 2 ? v : x5c;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) hp[r] = saved[((size_t)s * 16 + 4 * q + r) * ld + e];
#if !RQ_GRAD_SEEDED
            const float daB = ev ? gact[((size_t)s * 4 + q) * ld_g + e] : 0.0f;   // lane (q, j): dL/da_q of env (t, j)
#endif
            const uint8_t d = done[(size_t)s * ld + ec];
#if RQ_GRAD_WEIGHTED
            // the entry's label and weight, asked for here so that the recompute hides the wait; both arrays hold every env's column
            // of every step (e < n <= ld_y, ld_w), what they hold where the entry does not count is selected away below
            const float y_in = ev ? target[((size_t)s * 4 + q) * ld_y + e] : 0.0f;
            const float w_in = ev ? weight[(size_t)s * w_step + e] : 0.0f;
#endif

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
            float rr[4], zz[4], nn[4], hn[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                rr[r] = sigm2(gr[r]);
                zz[r] = sigm2(gz[r]);
                nn[r] = fmaf(2.0f, sigm2(fmaf(rr[r], gnh[r], gni[r])), -1.0f);
                hn[r] = fmaf(zz[r], hp[r] - nn[r], nn[r]);
            }

#if RQ_GRAD_SEEDED
            // ---- the seed: the forward's layer_2 on h' (ActorF32T::run: the lane's slice, then the four lane groups), a - y ----
            float p[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                p[i] = W[QW_B2 + i];
#pragma unroll
                for (int r = 0; r < 4; ++r) p[i] = fmaf(W[QW_L2 + 4 * r + i], hn[r], p[i]);
                red[j * 17 + 4 * q + i] = p[i];
            }
            __syncthreads();
            const float a = (red[j * 17 + q] + red[j * 17 + 4 + q]) + (red[j * 17 + 8 + q] + red[j * 17 + 12 + q]);
            const bool live = ev && d != 4;
#if RQ_GRAD_WEIGHTED
            const float wt = live ? w_in : 0.0f;
            const bool counts = wt > 0.0f;                       // false for 0, a negative weight and NaN
            const float err = counts ? a - y_in : 0.0f;
            const float daB = counts ? wt * err : 0.0f;          // lane (q, j): dL/da_q of env (t, j), before the 2 / W4
            sse += daB * err;
            wsum += counts ? (double)wt : 0.0;
#else
            const float y = live ? target[((size_t)s * 4 + q) * ld_y + e] : 0.0f;
            const float daB = live ? a - y : 0.0f;               // lane (q, j): dL/da_q of env (t, j), before the 2 / M
            sse += daB * daB;
            live_entries += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(live));
#endif
#endif
            // ---- the episode structure, backwards: an end feeds h0 and cuts the recurrence; a frozen step passes it on ----
            const bool ended = d == 1 || d == 2, frozen = d == 4;
            f32x4 din, pass;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (ended) { bH0[r] += dc[t][r]; dc[t][r] = 0.0f; }
                din[r] = frozen ? 0.0f : dc[t][r];
                pass[r] = frozen ? dc[t][r] : 0.0f;
            }
            // An env that receives nothing at this step (dL/da = 0 and nothing from later steps: padding columns, masked-out
            // frozen steps) contributes exactly nothing, whatever its recorded observation holds - a recording leaves the
            // observations of steps a whole frozen wave skipped unwritten.  Its deltas and operands are zeroed below rather
            // than multiplied by zero (0 x NaN).  Lanes (0..3, j) hold the env's 16 rows: one ballot decides.
            bool nz = daB != 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) nz = nz || din[r] != 0.0f;
            const uint64_t nzm = __builtin_amdgcn_ballot_w64(nz);
            const bool quiet = (((nzm >> j) | (nzm >> (16 + j)) | (nzm >> (32 + j)) | (nzm >> (48 + j))) & 1ull) == 0;
            // dL/dh' = W2^T da + what the later steps send back
            const f32x4 dh = mfma16(G[GW_W2T], daB, din);
            float dPr[4], dPz[4], dGni[4], dGnh[4];
            f32x4 dhd;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float dn = dh[r] * (1.0f - zz[r]);
                const float dz = dh[r] * (hp[r] - nn[r]);
                dhd[r] = dh[r] * zz[r];
                const float du = dn * (1.0f - nn[r] * nn[r]);
                dPr[r] = du * (gnh[r] * kInvT) * (rr[r] * (1.0f - rr[r]));
                dPz[r] = dz * (zz[r] * (1.0f - zz[r]));
                dGni[r] = du;
                dGnh[r] = du * rr[r];
                if (quiet) { dPr[r] = dPz[r] = dGni[r] = dGnh[r] = dhd[r] = 0.0f; y0[r] = hp[r] = hn[r] = 0.0f; }
            }
            if (quiet) {
#pragma unroll
                for (int k = 0; k < 6; ++k) X[k] = 0.0f;
            }
            // W_i^T and W_h^T of the gate deltas (K = 48 gate rows, 12 K-steps each)
            f32x4 dy0 = mfma16(G[GW_WIT + 0], dPr[0], zero);
            f32x4 dhp = mfma16(G[GW_WHT + 0], dPr[0], dhd);
#pragma unroll
            for (int r = 1; r < 4; ++r) {
                dy0 = mfma16(G[GW_WIT + r], dPr[r], dy0);
                dhp = mfma16(G[GW_WHT + r], dPr[r], dhp);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                dy0 = mfma16(G[GW_WIT + 4 + r], dPz[r], dy0);
                dhp = mfma16(G[GW_WHT + 4 + r], dPz[r], dhp);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                dy0 = mfma16(G[GW_WIT + 8 + r], dGni[r], dy0);
                dhp = mfma16(G[GW_WHT + 8 + r], dGnh[r], dhp);
            }
            float dp0[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                dp0[r] = y0[r] > 0.0f ? dy0[r] : 0.0f;           // ReLU'(0) = 0
                dc[t][r] = dhp[r] + pass[r];
                bR[r] += dPr[r];
                bZ[r] += dPz[r];
                bNI[r] += dGni[r];
                bNH[r] += dGnh[r];
            }
            bB2 += daB;

            // ---- outer products: the tile's 16 envs on K through LDS ----
            float* row = tile + j * GL_ROW;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                row[GL_DR + 4 * q + r] = dPr[r];
                row[GL_DZ + 4 * q + r] = dPz[r];
                row[GL_DNI + 4 * q + r] = dGni[r];
                row[GL_DNH + 4 * q + r] = dGnh[r];
                row[GL_D0 + 4 * q + r] = dp0[r];
                row[GL_Y0 + 4 * q + r] = y0[r];
                row[GL_HP + 4 * q + r] = hp[r];
                row[GL_HN + 4 * q + r] = hn[r];
            }
            row[GL_DA + q] = daB;
#pragma unroll
            for (int k = 0; k < 6; ++k) row[GL_X + 4 * k + q] = X[k];
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float* src = tile + (4 * u + q) * GL_ROW;   // k-slot q = env 4u + q of the tile
                const float ar = src[GL_DR + j], az = src[GL_DZ + j], ani = src[GL_DNI + j], anh = src[GL_DNH + j];
                const float a0 = src[GL_D0 + j];
                const float ada = src[GL_DA + (j & 3)];
                const float by0 = src[GL_Y0 + j], bhp = src[GL_HP + j], bhn = src[GL_HN + j];
                const float bx0 = src[GL_X + j], bx1 = src[GL_X + 16 + (j & 7)];
                aWi[0] = mfma16(ar, by0, aWi[0]);
                aWi[1] = mfma16(az, by0, aWi[1]);
                aWi[2] = mfma16(ani, by0, aWi[2]);
                aWh[0] = mfma16(ar, bhp, aWh[0]);
                aWh[1] = mfma16(az, bhp, aWh[1]);
                aWh[2] = mfma16(anh, bhp, aWh[2]);
                aW0[0] = mfma16(a0, bx0, aW0[0]);
                aW0[1] = mfma16(a0, j < 8 ? bx1 : 0.0f, aW0[1]);
                aW2 = mfma16(j < 4 ? ada : 0.0f, bhn, aW2);
            }
            __syncthreads();
        }
    }

    // ---- the start: the learned initial state takes what reaches it, or dL/dh_start is handed out ----
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (start_initial) bH0[r] += dc[t][r];
            else if (gh_start != nullptr) gh_start[(size_t)(4 * q + r) * ld + wave_base + 16 * t + j] = dc[t][r];
        }

    // ---- this wave's partial gradient, every one of the 2 084 entries written once ----
    float* out = partial + (size_t)blockIdx.x * RQ_POLICY_NUM_WEIGHTS;
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            out[OFF_WI + (16 * g + 4 * q + r) * 16 + j] = aWi[g][r];
            out[OFF_WH + (16 * g + 4 * q + r) * 16 + j] = aWh[g][r];
        }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t o = 4 * q + r;
        out[OFF_W0 + o * 22 + j] = aW0[0][r];
        if (j < 6) out[OFF_W0 + o * 22 + 16 + j] = aW0[1][r];
        else if (j == 6) out[OFF_B0 + o] = aW0[1][r];
        if (q == 0) out[OFF_W2 + r * 16 + j] = aW2[r];
    }
    // the lane sums: lane (q, j) holds rows 4q .. 4q+3 summed over its envs; fold the 16 lanes of each group, j ascending
    float* mine = sums + lane * GRAD_LANE_SUMS;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        mine[r] = bR[r]; mine[4 + r] = bZ[r]; mine[8 + r] = bNI[r]; mine[12 + r] = bNH[r]; mine[16 + r] = bH0[r];
    }
    mine[20] = bB2;
    __syncthreads();
    for (uint32_t o = lane; o < 4 * GRAD_LANE_SUMS; o += 64) {
        const uint32_t qq = o / GRAD_LANE_SUMS, k = o % GRAD_LANE_SUMS;
        float acc = 0.0f;
        for (int jj = 0; jj < 16; ++jj) acc += sums[(qq * 16 + jj) * GRAD_LANE_SUMS + k];
        const uint32_t rowi = 4 * qq + (k & 3);
        if (k < 4) { out[OFF_BI + rowi] = acc; out[OFF_BH + rowi] = acc; }
        else if (k < 8) { out[OFF_BI + 16 + rowi] = acc; out[OFF_BH + 16 + rowi] = acc; }
        else if (k < 12) out[OFF_BI + 32 + rowi] = acc;
        else if (k < 16) out[OFF_BH + 32 + rowi] = acc;
        else if (k < 20) out[OFF_H0 + rowi] = acc;
        else out[OFF_B2 + qq] = acc;
    }
#if RQ_GRAD_SEEDED
    __syncthreads();
    sums[lane] = sse;
#if RQ_GRAD_WEIGHTED
    wfold[lane] = wsum;
#endif
    __syncthreads();
    if (lane == 0) {
        float acc = 0.0f;
        for (int l = 0; l < 64; ++l) acc += sums[l];
        wave_sse[blockIdx.x] = acc;
#if RQ_GRAD_WEIGHTED
        double wacc = 0.0;
        for (int l = 0; l < 64; ++l) wacc += wfold[l];
        wave_wsum[blockIdx.x] = wacc;
#else
        wave_live[blockIdx.x] = live_entries;
#endif
    }
#endif
}
#undef RQ_GRAD_BACKWARD_KERNEL
#undef RQ_GRAD_SEEDED
#undef RQ_GRAD_BANK
#undef RQ_GRAD_WEIGHTED
