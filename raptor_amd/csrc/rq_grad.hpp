// rq_grad.hpp — the learner half of distillation (README.md:208-216): the fp32 student's actions over a recorded trajectory and
// their exact gradient with respect to the 2 084 parameters, back through time along the recorded episode structure.
//
//   kernel                    what                                                           bound
//   k_policy_grad_forward     k_actor_relabel's pass + the state entering every step saved   f32 MFMA rate (+ 64 B/env-step stored)
//   k_policy_grad_backward    t = T-1 .. 0: recompute, W2^T / Wi^T / Wh^T da, outer products  f32 MFMA rate (+ 168 B/env-step read)
//   k_policy_grad_reduce      per-wave partials [waves][2084] -> [2084] in wave order         HBM (8 KB per wave)
//
// Layouts (rq_device_math.hpp "actor"): a wave owns 64 envs as 4 tiles of 16; lane (q, j) = (l >> 4, l & 15) holds, in the Q
// layout, rows 4q .. 4q+3 of a 16-vector of env (tile t, j).  What the reverse pass needs where:
//   * transposed products (feature on M, env on N, K = the vector being contracted): the delta in the Q layout is directly the B
//     operand (K-step r carries row 4q + r in k-slot q) and the transposed image (rq_pack.cpp pack_policy_grad) is the A operand;
//     the result is again in the Q layout - the reverse recurrence never changes layout;
//   * weight-gradient outer products (K = envs): both operands need feature j on lane j and env on k-slot q.  Every vector a
//     tile contributes goes through one 16-env x 156-float LDS tile per wave (row = env, one ds_write per value, read back
//     column-wise: k-step u takes envs 4u .. 4u+3), the way the observation already changes layout in the forward;
//   * the observation is read straight from the trajectory's field-major block in the B layout (feature 4s+q of env (t, j)),
//     the same floats k_actor_relabel's LDS trip gives its MFMAs; layer_0's bias rides on the constant-1 feature 22.
// Gate biases and the initial state's gradient are sums of deltas over envs: lane-local sums in the Q layout, folded over the 16
// lanes of a lane group in a fixed order at the end.  Nothing is accumulated with atomics: the result is the same bits every run.
// Device code, compiled as part of rq_kernels.hip (the library keeps one code object per kernel source).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rq_rollout.hpp"      // the actors, field(), kFusedBlock, WavesPerSimd

namespace rq {

// ------------------------------------------------------------------ forward ------------
// k_actor_relabel (rq_kernels.hip) with one addition, the state entering step t in the Q layout to saved [t][16][ld] (every lane
// of the wave, padding included: the backward reads whole tiles), and two differences: the first state is the policy's (loaded)
// or the learned initial one, and nothing is written back to the policy.  The step is the actor's own: the actions are
// rq_trajectory_relabel's bit for bit.
template <typename ACTOR>
__global__ __launch_bounds__(kFusedBlock, WavesPerSimd<ACTOR>::value) void k_policy_grad_forward(
        uint32_t n, uint32_t ld, uint32_t steps, const float* __restrict__ packed, const float* __restrict__ obs,
        const uint8_t* __restrict__ done, const float* __restrict__ hidden, uint32_t ld_h, uint32_t start_initial,
        float* __restrict__ act, uint32_t ld_act, float* __restrict__ saved) {
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
        if (valid) {
#pragma unroll
            for (int k = 0; k < 4; ++k) field(act, t * 4 + k, ld_act)[i] = a[k];
        }
    }
}

// ------------------------------------------------------------------ backward -----------
// The LDS tile of the outer products: row = env of the tile, columns = the deltas (A operands) and inputs (B operands).
enum {
    GL_DR = 0, GL_DZ = 16, GL_DNI = 32, GL_DNH = 48, GL_D0 = 64,     // dL/d pre-activation: r, z, n (input half), n (hidden half), layer_0
    GL_DA = 80,                                                       // dL/da (4)
    GL_Y0 = 84, GL_HP = 100, GL_HN = 116, GL_X = 132,                 // layer_0 output, state before and after, observation (24)
    GL_ROW = 157                                                      // 156 used; odd: a column read touches 16 distinct banks
};
enum { GRAD_LANE_SUMS = 21 };      // per lane: r, z, n-input, n-hidden bias rows (4 each), h0 rows (4), b2 (1)

__device__ __forceinline__ float sigm2(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x)); }

// One wave = 64 envs for the whole trajectory, walked backwards.  Per step and tile the forward step is recomputed from the saved
// state and the recorded observation with the forward's own MFMA chains and gate arithmetic (gru_gates_prescaled, element by
// element), so r, z, n and h' are the values the actions were computed from.  dc[t] = dL/d(state after the step) of tile t.
__global__ __launch_bounds__(64, 1) void k_policy_grad_backward(
        uint32_t n, uint32_t ld, uint32_t steps, const float* __restrict__ packed, const float* __restrict__ gpacked,
        const float* __restrict__ obs, const uint8_t* __restrict__ done, const float* __restrict__ saved,
        const float* __restrict__ gact, uint32_t ld_g, uint32_t start_initial, float* __restrict__ gh_start,
        float* __restrict__ partial) {
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
            const float daB = ev ? gact[((size_t)s * 4 + q) * ld_g + e] : 0.0f;   // lane (q, j): dL/da_q of env (t, j)
            const uint8_t d = done[(size_t)s * ld + ec];

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
}

// grad[p] = sum over waves w = 0, 1, ... of partial[w][p], in that order
__global__ __launch_bounds__(256) void k_policy_grad_reduce(uint32_t waves, const float* __restrict__ partial,
                                                            float* __restrict__ grad) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= RQ_POLICY_NUM_WEIGHTS) return;
    float acc = 0.0f;
#pragma unroll 8
    for (uint32_t w = 0; w < waves; ++w) acc += partial[(size_t)w * RQ_POLICY_NUM_WEIGHTS + p];
    grad[p] = acc;
}

hipError_t launch_policy_grad_forward(hipStream_t s, uint32_t n, uint32_t ld, uint32_t steps, const float* packed,
                                      const float* obs, const uint8_t* done, const float* hidden, uint32_t ld_h,
                                      int start_initial, float* act, uint32_t ld_act, float* saved) {
    if (n == 0 || steps == 0) return hipSuccess;
    const unsigned g = (n + kFusedBlock - 1) / kFusedBlock;
    const uint32_t si = start_initial ? 1u : 0u;
    if (n > 65536u)        // launch_actor_relabel's choice of build (the two give the same bits)
        k_policy_grad_forward<ActorF32Lean><<<g, kFusedBlock, 0, s>>>(n, ld, steps, packed, obs, done, hidden, ld_h, si, act, ld_act, saved);
    else
        k_policy_grad_forward<ActorF32><<<g, kFusedBlock, 0, s>>>(n, ld, steps, packed, obs, done, hidden, ld_h, si, act, ld_act, saved);
    return hipGetLastError();
}

hipError_t launch_policy_grad_backward(hipStream_t s, uint32_t n, uint32_t ld, uint32_t steps, const float* packed,
                                       const float* gpacked, const float* obs, const uint8_t* done, const float* saved,
                                       const float* grad_act, uint32_t ld_g, int start_initial, float* grad_h_start,
                                       float* partial, float* grad) {
    if (n == 0 || steps == 0) return hipSuccess;
    const uint32_t waves = (n + 63) / 64;
    k_policy_grad_backward<<<waves, 64, 0, s>>>(n, ld, steps, packed, gpacked, obs, done, saved, grad_act, ld_g,
                                                start_initial ? 1u : 0u, grad_h_start, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_policy_grad_reduce<<<(RQ_POLICY_NUM_WEIGHTS + 255) / 256, 256, 0, s>>>(waves, partial, grad);
    return hipGetLastError();
}

}  // namespace rq
