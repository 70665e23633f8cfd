// rq_teacher.hpp - the register-stationary teacher's layers as device code shared by the two kernels of rq_teacher.hip that run them:
//   k_teacher_relabel_f32: a teacher over a recorded trajectory (the relabel pass, T steps per wave)
//   k_rollout_teachers:    a teacher flying its env (the closed loop of README.md:95-99)
// The input plan (bias constant at K slot in_dim) and the activations are shared as they are.  TeacherF32 below is the MFMA chain of
// k_teacher_relabel_f32 - same K order, same accumulator seeds - as functions; the relabel kernel keeps its own text of it because
// routed through these functions its scheduling moves (24 - 36 of the unit's 116 listings change: rq_teacher.hip is unchanged code).
// The operations are the same, so a rollout's action for an observation equals the relabel kernel's label for it bit for bit
// (tests/test_gpu_teacher_rollout.py).  Layouts and the image format: rq_teacher.hip's header comment and pack_teacher_f32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rq_kernels.hpp"

namespace rq {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t dwordx4 __attribute__((ext_vector_type(4)));

template <int ACT>
__device__ __forceinline__ float teacher_act(float x) {
    if (ACT == RQ_ACT_RELU) {          // one v_max_i32 on the bit pattern (see relu() in rq_device_math.hpp)
        const int b = __builtin_bit_cast(int, x);
        return __builtin_bit_cast(float, b > 0 ? b : 0);
    }
    if (ACT == RQ_ACT_TANH)            // rows pre-scaled by -2 log2 e: x = -2 log2e * pre-activation
        return fmaf(2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x)), -1.0f);
    return x;
}

// B operand of layer 1 for this lane: feature f = 4s + q of env `e` at step t; feature in_dim is the constant 1
// that carries the bias, anything beyond is padding.  obs is the trajectory's [T][22][ld] block.  The lane's six
// element offsets inside a step's block are fixed; the step's block base is wave-uniform (scalar registers), so a
// load is one instruction with no per-step 64-bit address arithmetic on the VALU.
struct InputPlan {
    uint32_t off[6];       // (feature row) * ld + env, in elements (< 2^30: ld <= 2^24 rows of 22)
    uint32_t f[6];
    uint32_t in_dim, ld;
    __device__ __forceinline__ InputPlan(uint32_t ld_, uint32_t e, uint32_t q, uint32_t in_dim_) : in_dim(in_dim_), ld(ld_) {
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            f[s] = 4 * s + q;
            off[s] = (f[s] < in_dim ? f[s] : 0u) * ld + e;
        }
    }
    // the bias constant and the padding replace what was loaded for features >= in_dim.  Kept apart from load(): the
    // loads run one or two steps ahead and their values cross the loop's back edge raw - written as one expression
    // the compiler sinks each load into its select and a step pays six exec-masked branches
    __device__ __forceinline__ void finish(float (&x)[6]) const {
#pragma unroll
        for (int s = 0; s < 6; ++s) x[s] = f[s] < in_dim ? x[s] : (f[s] == in_dim ? 1.0f : 0.0f);
    }
    __device__ __forceinline__ void load(const float* __restrict__ obs, uint32_t t, float (&x)[6]) const {
        const float* __restrict__ block = obs + (size_t)t * RQ_POLICY_INPUT_DIM * ld;      // wave-uniform
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            x[s] = block[off[s]];
        }
    }
};

// The exact-fp32 teacher of the register-stationary family: operands A1 [M1][6], A2 [M2][K2], A3 [K3] and biases B2 [M2], B3 in
// registers (124 VGPRs for 22-64-64-4), declared by the kernel (TeacherF32<H1, H2> gives the shapes).
template <int H1, int H2>
struct TeacherF32 {
    static constexpr int M1 = H1 / 16, M2 = H2 / 16, K2 = H1 / 4, K3 = H2 / 4;
    static constexpr int REGS = teacher_image_regs_f32(H1, H2);
    // img = this teacher's image + lane
    __device__ static __forceinline__ void load(const float* img, float (&A1)[M1][6], float (&A2)[M2][K2], float (&A3)[K3],
                                                f32x4 (&B2)[M2], f32x4& B3) {
        int v = 0;
#pragma unroll
        for (int m = 0; m < M1; ++m)
#pragma unroll
            for (int s = 0; s < 6; ++s) A1[m][s] = img[(v++) * 64];
#pragma unroll
        for (int m = 0; m < M2; ++m)
#pragma unroll
            for (int k = 0; k < K2; ++k) A2[m][k] = img[(v++) * 64];
#pragma unroll
        for (int k = 0; k < K3; ++k) A3[k] = img[(v++) * 64];
#pragma unroll
        for (int m = 0; m < M2; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) B2[m][r] = img[(v++) * 64];
#pragma unroll
        for (int r = 0; r < 4; ++r) B3[r] = img[(v++) * 64];
    }
    // Xc: the finished B operand of layer 1 (InputPlan::finish) -> the output layer's accumulators: rows 0..3 of the 16-row
    // output tile (register r at lane group 0) are the 4 actions before the output activation
    template <int ACT>
    __device__ static __forceinline__ f32x4 forward(const float (&A1)[M1][6], const float (&A2)[M2][K2], const float (&A3)[K3],
                                                    const f32x4 (&B2)[M2], const f32x4& B3, const f32x4& zero, const float (&Xc)[6]) {
        f32x4 y1[M1], y2[M2];
#pragma unroll
        for (int m = 0; m < M1; ++m) y1[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(A1[m][0], Xc[0], zero, 0, 0, 0);
#pragma unroll
        for (int s = 1; s < 6; ++s)
#pragma unroll
            for (int m = 0; m < M1; ++m) y1[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(A1[m][s], Xc[s], y1[m], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < M1; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) y1[m][r] = teacher_act<ACT>(y1[m][r]);
#pragma unroll
        for (int m = 0; m < M2; ++m) y2[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(A2[m][0], y1[0][0], B2[m], 0, 0, 0);
#pragma unroll
        for (int k = 1; k < K2; ++k)
#pragma unroll
            for (int m = 0; m < M2; ++m)
                y2[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(A2[m][k], y1[k / 4][k % 4], y2[m], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < M2; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) y2[m][r] = teacher_act<ACT>(y2[m][r]);
        f32x4 o = __builtin_amdgcn_mfma_f32_16x16x4f32(A3[0], y2[0][0], B3, 0, 0, 0);
#pragma unroll
        for (int k = 1; k < K3; ++k) o = __builtin_amdgcn_mfma_f32_16x16x4f32(A3[k], y2[k / 4][k % 4], o, 0, 0, 0);
        return o;
    }
};

}  // namespace rq
