// rq_rollout_schedule.inc - the fused kernel of an env that carries a schedule, and its launcher; included once per kind of schedule
// (rq_kernels.hip):
//   RQ_SCHEDULE_KERNEL        the kernel's name, k_rollout_fused_<kind>
//   RQ_FUSED_TAKES_<KIND>     the kind that is on (rq_rollout_body.inc: its `if constexpr (<KIND>)` blocks)
//   RQ_SCHEDULE_PTRS, _NAME   the type of the schedule's argument (rq_step_launch.hpp) and the name the body knows it by
// One text for the five, and each a kernel of its own with its own argument block: the listings of the kernels without a schedule,
// and of every older schedule's, stay what they were when a kind is added, and the profiles name the kernels.
//
// The text of k_rollout_fused_bank_rate - the RATE loop, image and interval chosen per workgroup - with one schedule on.  The block
// tables are optional: block_policy == nullptr is ONE policy, whose image is `images` and whose native interval is `single_interval`.
// At interval 1 the RATE text computes the plain kernel's bits (see k_rollout_fused_bank_rate), so this one entry point serves
// rq_rollout, rq_rollout_record, rq_rollout_track[_refs] and rq_rollout_policies[_track[_refs]] at every native interval.  fp32 actors
// only: the host refuses the 16-bit policies, the SampleAndSquash stage and a second schedule while a schedule is attached in fused
// mode.
template <bool NOISE, bool AUTORESET, bool RECORD, bool TRACK, typename ACTOR>
__global__ __launch_bounds__(kFusedBlock, WavesPerSimd<ACTOR>::value) void RQ_SCHEDULE_KERNEL(Batch b, StepCfg c, NoiseCfg nc, SampleCfg sc,
                                                               uint64_t seed, uint32_t epoch0, uint32_t n_steps,
                                                               const float* __restrict__ params,
                                                               float* __restrict__ state,
                                                               float* __restrict__ hidden,
                                                               const float* __restrict__ w,
                                                               const float* __restrict__ images,
                                                               const uint32_t* __restrict__ block_policy,
                                                               const uint32_t* __restrict__ policy_interval, uint32_t image_floats,
                                                               uint32_t single_interval,
                                                               StatsPtrs st, TrajPtrs traj, TrackPtrs trk,
                                                               RQ_SCHEDULE_PTRS RQ_SCHEDULE_NAME,
                                                               unsigned long long* __restrict__ span) {
    uint32_t policy = 0, interval = single_interval;
    if (block_policy != nullptr) {                   // wave-uniform (kernel argument): scalar loads, as in k_rollout_fused_bank_rate
        policy = block_policy[blockIdx.x];
        interval = policy_interval[policy];
    }
    const float* __restrict__ packed = images + (size_t)policy * image_floats;
#define RQ_FUSED_TAKES_TRACK
#define RQ_FUSED_TAKES_RATE
#include "rq_rollout_body.inc"
}

// one policy: the tables null, its image and its interval; a bank: the tables (a.interval, left at 1, is not read).  `schedule`: the
// member of `a` that is this kind's - the overload is chosen by its type
template <typename ACTOR>
static inline void launch_fused_schedule_actor(hipStream_t s, const FusedArgs& a, const RQ_SCHEDULE_PTRS& schedule) {
    dispatch_bools([&](auto NZ, auto AR, auto RC, auto TK) {
        hipLaunchKernelGGL((RQ_SCHEDULE_KERNEL<NZ(), AR(), RC(), TK(), ACTOR>), dim3(fused_grid(a)), dim3(kFusedBlock), 0, s,
                           a.b, a.c, a.nc, a.sc, a.seed, a.epoch0, a.n_steps, a.params, a.state, a.hidden, a.weights, a.images,
                           a.block_policy, a.policy_interval, (uint32_t)RQ_PACKED_FLOATS, a.interval, a.st, a.traj, a.trk, schedule, a.span);
    }, a.noise, a.autoreset, a.traj.obs != nullptr, a.trk.ref != nullptr);
}
#undef RQ_SCHEDULE_KERNEL
#undef RQ_SCHEDULE_PTRS
#undef RQ_SCHEDULE_NAME
