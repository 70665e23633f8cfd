// rq_gain_table.inc - the body of the feedback-gain table's kernel, included by rq_grad.hpp / rq_grad_bank.hpp once per kernel:
//   RQ_GAIN_TABLE_KERNEL     the kernel's name
//   RQ_GRAD_BANK             1: both images are those of the wave's policy, images + block_policy[blockIdx.x] * image_floats and
//                            gimages + block_policy[blockIdx.x] * gimage_floats (k_policy_gain_table_bank); 0: `packed`, `gpacked`
// One text for both, and each a kernel of its own: no other kernel's listing moves.
//
// What it sums: A = da/dp0 [4][16], the local Jacobian of the action with respect to layer_0's pre-activation at the recorded
// observation and the state entering the step (the instantaneous gain at fixed h is G = A W0; W0 is constant over the recording, so
// the host multiplies the sums once).  One wave = one 64-env block for the whole recording, walked forwards, in the backward's layout:
// lane (q, j) holds rows 4q .. 4q+3 of env (tile t, j).  Per step and tile
//   * the step is recomputed with rq_grad_backward.inc's own block (layer_0, the gate chains, sigm2, the n rows' pre-scale undone),
//     and its h' is the next state as rq_grad_forward.inc moves it: held on done code 4, the learned initial state after codes 1
//     and 2; padding columns run on the last env's data;
//   * four local backward seeds e_i: dL/dh' = W2[i][4q+r] is the lane's W[QW_L2 + 4r + i] as it lies; dPr, dPz, dGni as the backward
//     forms them; dy0 = Wi^T [dPr; dPz; dGni] over G[GW_WIT ..], 12 MFMAs; the ReLU mask (ReLU'(0) = 0).  No Wh^T product, no outer
//     product, no LDS tile;
//   * the lane adds its four rows of each seed to the running sums of the env's current age bucket with __fadd_rn, in step order:
//     16 floats per tile, 64 per lane.  Age, bucket index and the edges in LDS move as in rq_probe_moments.inc and the error table
//     (rq_grad_forward.inc, RQ_GRAD_ERROR_TABLE); when the env's bucket changes the lane stores its sums to its own cells and loads
//     the new bucket's, so an env that comes back to a bucket in a later episode goes on from the stored total.
// sum [n_buckets][4][16][ld_out], cell (b, i, k, e), and count [n_buckets][ld_out] (written by lane group 0); the kernel zeroes its
// columns' cells first: no atomics, no exchange between lanes, no memset, the same bits every run.  What is frozen, outside every
// bucket or a padding column is selected away before any arithmetic on the sums: NaN in a frozen observation reaches no sum - an
// MFMA keeps an env's values in its own column of N.
__global__ __launch_bounds__(64, 1) void RQ_GAIN_TABLE_KERNEL(
        uint32_t n, uint32_t ld, uint32_t steps,
#if RQ_GRAD_BANK
        const float* __restrict__ images, const float* __restrict__ gimages, const uint32_t* __restrict__ block_policy,
        uint32_t image_floats, uint32_t gimage_floats,
#else
        const float* __restrict__ packed, const float* __restrict__ gpacked,
#endif
        const float* __restrict__ obs, const uint8_t* __restrict__ done, const float* __restrict__ hidden, uint32_t ld_h,
        uint32_t start_initial, const ProbeEdges edges, uint32_t n_buckets, float* sum, uint32_t* count, uint32_t ld_out) {
    __shared__ uint32_t ed[kProbeMaxBuckets + 1];
#if RQ_GRAD_BANK
    const float* __restrict__ packed = images + (size_t)block_policy[blockIdx.x] * image_floats;
    const float* __restrict__ gpacked = gimages + (size_t)block_policy[blockIdx.x] * gimage_floats;
#endif
    const uint32_t lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15;
    const uint32_t wave_base = blockIdx.x * 64;
    float W[QW_REGS], G[12];
#pragma unroll
    for (int v = 0; v < QW_REGS; ++v) W[v] = packed[qw_slot(v, lane)];
#pragma unroll
    for (int v = 0; v < 12; ++v) G[v] = gpacked[(GW_WIT + v) * 64 + lane];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 cbr = {W[QW_BR], W[QW_BR + 1], W[QW_BR + 2], W[QW_BR + 3]};
    const f32x4 cbz = {W[QW_BZ], W[QW_BZ + 1], W[QW_BZ + 2], W[QW_BZ + 3]};
    const f32x4 cbni = {W[QW_BNI], W[QW_BNI + 1], W[QW_BNI + 2], W[QW_BNI + 3]};
    const f32x4 cbnh = {W[QW_BNH], W[QW_BNH + 1], W[QW_BNH + 2], W[QW_BNH + 3]};
    constexpr float kInvT = 1.0f / -2.8853900817779268f;     // the n rows' pre-scale undone: gnh / (-2 log2 e) = W_hn h + b_hn
    // observation features of the B layout: K-step s, k-slot q = feature 4s + q (22 = the constant 1, 23 = 0)
    const uint32_t f5 = 20 + (q < 2 ? q : 1);
    const float x5c = q == 2 ? 1.0f : 0.0f;

    float hQ[4][4];
    if (start_initial) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) hQ[t][r] = W[QW_H0 + r];
    } else {
        load_hidden_q(hidden, ld_h, wave_base, n, hQ);
    }

    if (lane <= n_buckets) ed[lane] = edges.v[lane];
    // the lane's cells: column e of tile t, rows 4q .. 4q+3 of every seed; written where e < n <= ld_out only
    const size_t plane = (size_t)16 * ld_out;                 // one seed of one bucket
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const uint32_t e = wave_base + 16 * t + j;
        if (e < n)
            for (uint32_t b = 0; b < n_buckets; ++b) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sum[((size_t)b * 4 + i) * plane + (size_t)(4 * q + r) * ld_out + e] = 0.0f;
                if (q == 0) count[(size_t)b * ld_out + e] = 0u;
            }
    }
    __syncthreads();
    const uint32_t idx0 = ed[0] == 0u ? 1u : 0u;             // edges <= age 0
    uint32_t age[4], idx[4], run_count[4];
    int cur[4];                                               // the bucket whose sums the lane holds for tile t
    float acc[4][4][4];                                       // [tile][seed i][row r]
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        age[t] = 0; idx[t] = idx0; run_count[t] = 0; cur[t] = -1;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t][i][r] = 0.0f;
    }

    for (uint32_t s = 0; s < steps; ++s) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint32_t e = wave_base + 16 * t + j;
            const bool ev = e < n;
            const uint32_t ec = ev ? e : n - 1;                  // padding columns run on the last env's data, as the forward
            float X[6], hp[4];
#pragma unroll
            for (int k = 0; k < 5; ++k) X[k] = obs[((size_t)s * 22 + 4 * k + q) * ld + ec];
            {
                const float v = obs[((size_t)s * 22 + f5) * ld + ec];
                X[5] = q < 2 ? v : x5c;
            }
            const uint8_t d = done[(size_t)s * ld + ec];
#pragma unroll
            for (int r = 0; r < 4; ++r) hp[r] = hQ[t][r];
            const bool live = ev && d != 4;
            const int bk = live && idx[t] >= 1u && idx[t] <= n_buckets ? (int)idx[t] - 1 : -1;
            if (live) {                                          // rq_probe_moments.inc's move of (age, idx), word for word
                if (d == 1 || d == 2) { age[t] = 0; idx[t] = idx0; }
                else {
                    ++age[t];
                    if (idx[t] <= n_buckets && ed[idx[t]] == age[t]) ++idx[t];
                }
            }

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
            float rr[4], zz[4], nn[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                rr[r] = sigm2(gr[r]);
                zz[r] = sigm2(gz[r]);
                nn[r] = fmaf(2.0f, sigm2(fmaf(rr[r], gnh[r], gni[r])), -1.0f);
                const float hn = fmaf(zz[r], hp[r] - nn[r], nn[r]);
                // the next state: frozen - not advanced; an episode end - the learned initial state
                hQ[t][r] = d == 4 ? hp[r] : (d == 1 || d == 2 ? W[QW_H0 + r] : hn);
            }

            // ---- the env's bucket changes: the lane's sums go to its cells, the new bucket's come ----
            if (bk >= 0 && bk != cur[t]) {
                if (cur[t] >= 0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            sum[((size_t)cur[t] * 4 + i) * plane + (size_t)(4 * q + r) * ld_out + e] = acc[t][i][r];
                    if (q == 0) count[(size_t)cur[t] * ld_out + e] = run_count[t];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[t][i][r] = sum[((size_t)bk * 4 + i) * plane + (size_t)(4 * q + r) * ld_out + e];
                if (q == 0) run_count[t] = count[(size_t)bk * ld_out + e];
                cur[t] = bk;
            }
            run_count[t] += bk >= 0 ? 1u : 0u;

            // ---- four seeds e_i: dL/dh' = W2[i][.], the gate deltas, Wi^T of them, the ReLU mask ----
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float dPr[4], dPz[4], dGni[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float dh = W[QW_L2 + 4 * r + i];
                    const float dn = dh * (1.0f - zz[r]);
                    const float dz = dh * (hp[r] - nn[r]);
                    const float du = dn * (1.0f - nn[r] * nn[r]);
                    dPr[r] = du * (gnh[r] * kInvT) * (rr[r] * (1.0f - rr[r]));
                    dPz[r] = dz * (zz[r] * (1.0f - zz[r]));
                    dGni[r] = du;
                }
                f32x4 dy0 = mfma16(G[0], dPr[0], zero);
#pragma unroll
                for (int r = 1; r < 4; ++r) dy0 = mfma16(G[r], dPr[r], dy0);
#pragma unroll
                for (int r = 0; r < 4; ++r) dy0 = mfma16(G[4 + r], dPz[r], dy0);
#pragma unroll
                for (int r = 0; r < 4; ++r) dy0 = mfma16(G[8 + r], dGni[r], dy0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float dp0 = y0[r] > 0.0f ? dy0[r] : 0.0f;          // ReLU'(0) = 0
                    acc[t][i][r] = bk >= 0 ? __fadd_rn(acc[t][i][r], dp0) : acc[t][i][r];   // selected, never multiplied
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const uint32_t e = wave_base + 16 * t + j;
        if (cur[t] >= 0) {                                       // implies e < n
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) sum[((size_t)cur[t] * 4 + i) * plane + (size_t)(4 * q + r) * ld_out + e] = acc[t][i][r];
            if (q == 0) count[(size_t)cur[t] * ld_out + e] = run_count[t];
        }
    }
}
#undef RQ_GAIN_TABLE_KERNEL
#undef RQ_GRAD_BANK
