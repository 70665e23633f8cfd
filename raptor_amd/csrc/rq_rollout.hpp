// rq_rollout.hpp - the fused rollout kernel (the loop body of README.md:95-99 x K in one launch) as a template over the
// actor build, shared by the two translation units that instantiate it:
//   rq_kernels.hip        the exact-fp32 actors (ActorF32 / ActorF32Lean): their instruction order is pinned by hand
//                         (sched_barrier / sched_group_barrier around the MFMA batches);
//   rq_kernels_16bit.hip  the bf16 and split-f16 actors, whose MFMAs co-execute with the vector unit and whose loop is therefore
//                         a scheduling problem of its own.  Round 4 compiled this unit with -mllvm
//                         -amdgpu-sched-strategy=max-ilp (a lone wave issues one vector instruction per 5.06 cycles but stalls to
//                         8.25 when it consumes the result of the one right in front of it, tools/lonewave.hip: 24 -> 5 such pairs
//                         per step) - and took it back: the two-waves-per-SIMD bf16 build then differed from run to run
//                         (raptor_amd/build.py SOURCE_FLAGS, test_fused_rollout_is_deterministic).  The unit stays the place
//                         for such per-build flags.
#pragma once
#include <hip/hip_ext.h>

#include <cstdlib>
#include <type_traits>

#include "rq_device_math.hpp"
#include "rq_dispatch.hpp"

namespace rq {

static constexpr int kBlock = 256;      // 4 waves; streaming kernels
static constexpr int kFusedBlock = 64;  // 1 wave per workgroup: spreads 65 536 envs as 1024 WGs over 256 CUs

// Stores of write-once streams leave as NON-TEMPORAL stores (round 5, same-box A/B, profiles/r05_ab_nt_stores.txt): the observation
// k_observe / k_step write (k_observe at 2 097 152 envs 84 -> 63 us = 0.61 -> 0.82 of 8 TB/s, at 262 144 envs 8.2 -> 6.2 us, at
// 65 536 envs inside the noise) and the trajectory recorder's (2.5 - 4 % on the recorded rollout).  NOT the next state, the policy
// state or the actions (k_step, k_actor_step / k_actor_stream, the fused kernel's epilogue: measured, nothing), and not loads
// (round 5's first experiment: non-temporal LOADS cost k_actor_stream 10 - 25 %).
template <bool NT, class T>
__device__ __forceinline__ void put(T* p, T v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}
static constexpr bool kNtObs = true, kNtTraj = true;
static constexpr int kNtTrajAux = 2;           // the `nt` cache-policy bit of a raw buffer store

__device__ __forceinline__ uint32_t env_index() { return blockIdx.x * blockDim.x + threadIdx.x; }

// Field f of a field-major SoA buffer: env i of the batch is element i of this row.
template <typename T>
__device__ __forceinline__ T* field(T* base, uint32_t f, uint32_t ld) { return base + (size_t)f * ld; }

// register budget of a kernel built around an actor type: waves per SIMD it is compiled for
template <typename A> struct WavesPerSimd { static constexpr int value = 1; static constexpr bool bf16 = false; };
template <> struct WavesPerSimd<ActorF32Lean> { static constexpr int value = 2; static constexpr bool bf16 = false; };
template <> struct WavesPerSimd<ActorBF16> { static constexpr int value = 1; static constexpr bool bf16 = true; };
// the split-f16 actor: its MFMAs co-execute with the VALU like the bf16 ones; one build, the 512-register budget
template <> struct WavesPerSimd<ActorF16X2> { static constexpr int value = 1; static constexpr bool bf16 = true; };

// ------------------------------------------------------------------ fused rollout ------
// K iterations of observe -> evaluate_step -> step -> assign with the env state, the GRU
// hidden state, the per-env constants, the policy weights and the episode statistics resident
// in VGPRs; HBM is touched once before and once after the K steps.
// Control flow is wave-uniform around the MFMAs (see k_actor_step): lanes past the end of the
// batch shadow env n-1, frozen envs keep stepping a scratch copy that is never committed; only
// the rare auto-reset branch (no MFMA inside) diverges.

template <bool NOISE, bool AUTORESET, bool RECORD, bool SAS, typename ACTOR>
__global__ __launch_bounds__(kFusedBlock, WavesPerSimd<ACTOR>::value) void k_rollout_fused(Batch b, StepCfg c, NoiseCfg nc, SampleCfg sc,
                                                               uint64_t seed, uint32_t epoch0, uint32_t n_steps,
                                                               const float* __restrict__ params,
                                                               float* __restrict__ state,
                                                               float* __restrict__ hidden,
                                                               const float* __restrict__ w,
                                                               const float* __restrict__ packed, StatsPtrs st,
                                                               TrajPtrs traj, SasArgs sas,
                                                               unsigned long long* __restrict__ span) {
#define RQ_FUSED_TAKES_SAS
#include "rq_rollout_body.inc"
}

// The TRACK variant (rq_rollout_track): the same loop flying a moving setpoint - after observe_head the row of the env's own episode
// step count comes off what the policy sees, and the tracking error is kept (rq_device_math.hpp track_*).  No SampleAndSquash stage
// (the host refuses it).
template <bool NOISE, bool AUTORESET, bool RECORD, typename ACTOR>
__global__ __launch_bounds__(kFusedBlock, WavesPerSimd<ACTOR>::value) void k_rollout_fused_track(Batch b, StepCfg c, NoiseCfg nc, SampleCfg sc,
                                                               uint64_t seed, uint32_t epoch0, uint32_t n_steps,
                                                               const float* __restrict__ params,
                                                               float* __restrict__ state,
                                                               float* __restrict__ hidden,
                                                               const float* __restrict__ w,
                                                               const float* __restrict__ packed, StatsPtrs st,
                                                               TrajPtrs traj, TrackPtrs trk,
                                                               unsigned long long* __restrict__ span) {
    constexpr bool TRACK = true;
#define RQ_FUSED_TAKES_TRACK
#include "rq_rollout_body.inc"
}

// The RATE variant (rq_policy_set_native_interval above 1): the same loop with the policy's hidden state moving on only at an env's
// native steps - those whose episode step count is a multiple of `interval` - and the action of every other step computed from the
// last committed state.  Tracked or not (trk.ref), no SampleAndSquash stage (the host refuses the pair).
template <bool NOISE, bool AUTORESET, bool RECORD, bool TRACK, typename ACTOR>
__global__ __launch_bounds__(kFusedBlock, WavesPerSimd<ACTOR>::value) void k_rollout_fused_rate(Batch b, StepCfg c, NoiseCfg nc, SampleCfg sc,
                                                               uint64_t seed, uint32_t epoch0, uint32_t n_steps,
                                                               const float* __restrict__ params,
                                                               float* __restrict__ state,
                                                               float* __restrict__ hidden,
                                                               const float* __restrict__ w,
                                                               const float* __restrict__ packed, StatsPtrs st,
                                                               TrajPtrs traj, TrackPtrs trk, uint32_t interval,
                                                               unsigned long long* __restrict__ span) {
#define RQ_FUSED_TAKES_TRACK
#define RQ_FUSED_TAKES_RATE
#include "rq_rollout_body.inc"
}

// ------------------------------------------------------------------ launch -------------
// the 16-bit actors' instantiations of `family`: PLAIN, TRACK or RATE (rq_kernels_16bit.hip); the actor is a.precision's
hipError_t launch_rollout_fused_16bit(hipStream_t s, const FusedArgs& a, FusedFamily family);

inline unsigned fused_grid(const FusedArgs& a) { return (a.b.n + kFusedBlock - 1) / kFusedBlock; }

// One launcher per family: the instantiation for (noise, auto-reset, recording[, tracking]) of one actor build, the run-time bools
// made template arguments by dispatch_bools, the launch description (rq_kernels.hpp FusedArgs) unpacked into the kernel's positional
// parameters.  SAS = with the SampleAndSquash output stage.
template <bool SAS, typename ACTOR>
inline void launch_fused_actor(hipStream_t s, const FusedArgs& a) {
    dispatch_bools([&](auto NZ, auto AR, auto RC) {
        hipLaunchKernelGGL((k_rollout_fused<NZ(), AR(), RC(), SAS, ACTOR>), dim3(fused_grid(a)), dim3(kFusedBlock), 0, s,
                           a.b, a.c, a.nc, a.sc, a.seed, a.epoch0, a.n_steps, a.params, a.state, a.hidden, a.weights, a.images,
                           a.st, a.traj, a.sas, a.span);
    }, a.noise, a.autoreset, a.traj.obs != nullptr);
}

template <typename ACTOR>
inline void launch_fused_track_actor(hipStream_t s, const FusedArgs& a) {
    dispatch_bools([&](auto NZ, auto AR, auto RC) {
        hipLaunchKernelGGL((k_rollout_fused_track<NZ(), AR(), RC(), ACTOR>), dim3(fused_grid(a)), dim3(kFusedBlock), 0, s,
                           a.b, a.c, a.nc, a.sc, a.seed, a.epoch0, a.n_steps, a.params, a.state, a.hidden, a.weights, a.images,
                           a.st, a.traj, a.trk, a.span);
    }, a.noise, a.autoreset, a.traj.obs != nullptr);
}

template <typename ACTOR>
inline void launch_fused_rate_actor(hipStream_t s, const FusedArgs& a) {
    dispatch_bools([&](auto NZ, auto AR, auto RC, auto TK) {
        hipLaunchKernelGGL((k_rollout_fused_rate<NZ(), AR(), RC(), TK(), ACTOR>), dim3(fused_grid(a)), dim3(kFusedBlock), 0, s,
                           a.b, a.c, a.nc, a.sc, a.seed, a.epoch0, a.n_steps, a.params, a.state, a.hidden, a.weights, a.images,
                           a.st, a.traj, a.trk, a.interval, a.span);
    }, a.noise, a.autoreset, a.traj.obs != nullptr, a.trk.ref != nullptr);
}

}  // namespace rq
