// rq_objects.hpp - the objects behind the opaque handles of include/raptor_quad.h and the host-side helpers the translation units of the
// C-ABI layer share.  Round 6 split rq_capi.cpp (2 300 lines: handle management, host caches, speculation, graphs, teacher packing in
// one file) by what the entry points serve:
//   rq_capi.cpp          library, Device, Rng, Environment, Parameters / State containers, statistics, timing diagnostics
//   rq_capi_vector.cpp   the five l2f vector:: functions
//   rq_small_batch.cpp   the small-batch loop behind them and behind evaluate_step: mailbox, observation cache, speculative policy step
//   rq_resident.cpp      the resident executor's host side (both kinds: the loop's rq_step and the policy alone)
//   rq_capi_policy.cpp   Raptor: create / configure / reset / evaluate_step / evaluate_sequence / selftest
//   rq_capi_rollout.cpp  the loop body x K on the device (fused, or chained under a hipGraph), trajectories, relabelling with a policy
//   rq_capi_teacher.cpp  the teacher bank
//   rq_capi_policy_bank.cpp  the policy bank: many student checkpoints in one rollout, one per 64-env block
//   rq_capi_grad.cpp     the student's forward / backward over a recorded trajectory; the distillation update (loss, Adam, repack),
//                        for one policy and for a policy bank
//   rq_memory.hpp        rq::DeviceBuffer / rq::PinnedBuffer: every object below owns its device and pinned memory through them
//   rq_env_schedule.hpp  rq::EnvSchedule: a schedule slot of an env - bank, ids, first rows on the device, attachment number
//   rq_call_memory.hpp   rq::CallMemory: the `memory` argument of the learner's and the probes' calls - staging in and out, the final wait
// The ten rq_rollout* entry points (a policy's, a policy bank's, the teacher bank's; plain, _track, _track_refs) each describe their call
// (RolloutCall) and go through rollout_run below with the actor type of their file; their row tables are one type (RowTables).
// Helpers live in namespace rqh (each .cpp says `using namespace rqh;`); nothing here is visible outside libraptor_quad.so.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <emmintrin.h>
#include <mutex>
#include <new>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../../include/raptor_quad.h"
#include "rq_kernels.hpp"

#include "rq_host.hpp"
#include "rq_memory.hpp"
#include "rq_call_memory.hpp"
#include "rq_env_schedule.hpp"

using rq::fail;
using rq::DeviceScope;
using rq::DeviceBuffer;
using rq::PinnedBuffer;
using rq::CallMemory;

inline uint32_t round_up64(uint32_t n) { return (n + 63u) & ~63u; }

// ---------------------------------------------------------------------------- objects ---
// Versions of params / state / policy objects and the ids of envs come from ONE counter: the caches below are keyed by
// (address, version), and an address that is freed and handed out again must never meet a version it has carried before.
inline uint64_t fresh_version() {
    static std::atomic<uint64_t> counter{1};
    return counter.fetch_add(1, std::memory_order_relaxed) + 1;
}

// the two launches of a small-batch step: k_step (+ the next observation) and the speculative policy step on it
// (`spec`: there is one; it reads the observation the step leaves in step.obs_of_next)
struct StepPair { rq::EnvStepLaunch step; bool spec; rq::ActorStepLaunch actor; };

// the launch of a small-batch policy step on host rows (mailbox in -> out): what a policy command replays as
using PolicyCmd = rq::ActorStepLaunch;

// ---- resident executor (rq_resident.cpp; kernels: rq_kernels.hip k_resident_small / k_resident_loop / k_resident_policy) -------------
constexpr uint32_t kResidentMaxEnvs = 256;            // one workgroup, a wave per SIMD of one CU (at 512 envs the launches, spread over the chip, are faster)

// What a resident kernel is started for, and what a call must still be for if its command is to go to that kernel: the same objects at
// the same versions, and the buffers it names among the kernel's ping-pong pairs.  The loop's pairs are {obs, obs_alt} and {hidden,
// hidden_alt} (a command's bits pick the current one); the policy's are {nullptr, nullptr} and {hidden, hidden} (updated in place).
// Of a call's own pairs, obs[1] is where its step writes the observation and hidden[0] the hidden state it reads.
struct ResidentBinding {
    bool policy_kind;                            // k_resident_policy (else the loop's kernels)
    const rq_env* env; uint64_t env_uid;
    const rq_params* params; uint64_t params_version;
    const rq_policy* pol; const float* packed; uint32_t batch;
    rq_env_config cfg; uint64_t seed;
    float* obs[2]; float* hidden[2];
};

// eligible calls in a row, each within kResidentMaxGapNs of the one before and for the same (who, key)
struct ResidentStreak {
    uint32_t n = 0;
    uint64_t last_ns = 0; const void* who = nullptr; uint64_t key = 0;      // the last eligible call (`who` is never dereferenced)
    uint32_t follow(bool eligible, uint64_t now_ns, const void* call_who, uint64_t call_key);     // this call's length (0: not eligible)
};

struct ResidentExecutor {
    // settings, read from the environment at rq_device_create (resident_setup)
    bool enabled = true;                 // RQ_NO_RESIDENT: off; rq_device_set_resident
    bool timing = false;                 // RQ_RESIDENT_TIMING: the kernel records its timestamps (rq_device_get_resident_timing)
    uint64_t idle_ticks = 0, life_ticks = 0, host_idle_ns = 0, host_life_ns = 0;
    // memory (rq_resident.cpp ResidentWord)
    hipStream_t stream = nullptr;
    PinnedBuffer<uint32_t> mem;          // the command line, what the kernel says as it leaves, its timing, the rows
    DeviceBuffer<uint32_t> cmd_dev;      // on a large-BAR platform: fine-grained device memory for the commands
    uint32_t* cmd = nullptr;             // where commands are written: mem or cmd_dev
    bool cmd_on_device = false;
    // the kernel
    bool running = false;
    ResidentBinding bound{};             // what the running kernel was started for
    uint32_t launch_id = 0, packet = 0;  // id of the kernel that is running; commands posted to it
    uint64_t born_ns = 0;                // host clock at its launch
    uint64_t last_post_ns = 0;           // host clock of the last command: a kernel idle for too long may be leaving, it is not posted to
    uint64_t posts_at_start = 0;         // posts when it was started: what it has served = posts - this
    uint32_t backoff = 0, backoff_left = 0;     // eligible calls still to let pass before another kernel is started
    ResidentStreak loop_streak, policy_streak;  // the two kinds count apart: rq_step zeroes the policy's, any other call both
    // the command posted last: what a replay as launches needs (of the running kernel's kind)
    bool pending = false;                // posted and not known to have been consumed
    uint32_t pending_first = 0, pending_last = 0;   // its sequence numbers: the first one published = consumed
    union { StepPair step; PolicyCmd policy; } last{};
    uint64_t starts = 0, posts = 0, replays = 0;    // diagnostics
};

// ---- the small-batch loop (rq_small_batch.cpp).  Mailbox (rq::Mailbox): below kGpuLayoutMinEnvs envs rows cross the boundary in pinned
// host memory the kernels read and write themselves, and the host waits on a flag instead of the stream.
struct HostMailbox {
    PinnedBuffer<uint32_t> flag;     // sequence number of the last finished mailbox launch
    DeviceBuffer<uint32_t> counter;  // workgroup counter of the launch in flight
    PinnedBuffer<float> in, out;     // rows read by kernels (observations / actions), rows written by kernels
    PinnedBuffer<float> obs, act;    // rows of the observation cache [n][RQ_OBSERVATION_DIM], of the speculated action [n][4]
    uint32_t seq = 0, in_busy = 0;     // the last sequence number handed to a launch; that of the last launch that reads `in`
};
enum class MbOut { none, out, obs, act };     // which pinned rows a mailbox launch writes
// Observation cache (round 3): k_step also assembles the observation of the state it produced - into the env's device buffer and, row-major,
// into the mailbox's `obs` rows - so that the observe() that follows step() + assign() (README.md:96-99) is a host memcpy, no launch.  Valid
// for the (env, params, state) objects and versions recorded here; any write to one of them, a real observe launch or another step ends it.
struct ObservationCache {
    const rq_env* env = nullptr; uint64_t env_uid = 0;                     // env == nullptr: nothing cached
    const rq_params* params = nullptr; uint64_t params_version = 0;
    const rq_state* state[2] = {nullptr, nullptr};     // the state k_step wrote, and the one it was assigned to
    uint64_t version[2] = {0, 0};
    uint32_t seq = 0, n = 0;       // mailbox sequence number of the launch that fills the cache; its rows (the env may be gone by then)
    bool in_alt = false;           // the field-major copy still sits in the env's obs_alt (not yet swapped in)
};
// Speculative policy step (round 3): the reference's loop hands the observation it was just given straight to Raptor.evaluate_step
// (README.md:96-97), so rq_step also launches the policy last evaluated here on the observation it caches (hidden state into the policy's
// spare buffer, actions into the mailbox's `act`).  evaluate_step takes that result - a memcmp, a memcpy and a pointer swap, no launch - iff
// called with bit-identical rows and the same policy at the same version, and only while the cache entry it was made from still exists
// (speculation_current: obs_cache.env set and oc_seq == obs_cache.seq).  After kSpeculationMissLimit untaken steps in a row (each a wasted
// launch) the device stops speculating; it resumes when evaluate_step is again called with exactly the cached rows.
struct Speculation {
    bool enabled = true;                 // rq_device_set_speculation; RQ_NO_SPECULATION in the environment: off at creation
    rq_policy* last_policy = nullptr;    // the policy of the most recent small-batch host evaluate_step
    rq_policy* policy = nullptr; uint64_t policy_version = 0;    // speculation in flight / available for this policy at this version
    uint32_t batch = 0, seq = 0, oc_seq = 0;
    bool outstanding = false;            // a speculated step was launched and not taken (yet)
    bool suspended = false; uint32_t misses = 0;
};
constexpr uint32_t kSpeculationMissLimit = 4;

struct rq_device {
    int ordinal = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    DeviceBuffer<unsigned long long> k_span;     // [waves][4]: per wave, in / out / loop begin / loop end ticks of the last timed fused rollout;
                                                 // behind the [k_span_used][4] in use: [k_span_used] core-clock cycles of the waves' steps
    uint32_t k_span_used = 0;
    std::vector<unsigned long long> k_host;      // the records of the last timed rollout on the host (fetched once per launch)
    bool k_fetched = false;
    double k_ticks_per_ms = 1e5;                 // wall clock rate (100 MHz on gfx950)
    bool graphs_enabled = true;    // RQ_NO_GRAPHS in the environment: chained rollouts never capture
    uint32_t graph_fallbacks = 0;  // chained rollouts whose hipGraph capture was invalidated from outside and that went out as plain launches
    bool k_timing = false;         // rq_device_set_rollout_timing
    bool k_timed = false;          // a launch carried the two events
    PinnedBuffer<float> staging;   // for transposing device -> host copies
    DeviceBuffer<float> rows;      // scratch, row-major side of the GPU layout changes (large batches)
    DeviceBuffer<float> rows2;     // second scratch (sequence evaluation, relabelling: actions)
    PinnedBuffer<float> staging_in;    // for host -> device copies (asynchronous)
    hipEvent_t ev_h2d = nullptr;   // recorded after the last copy out of staging_in
    bool h2d_pending = false;
    HostMailbox mailbox;
    ObservationCache obs_cache;
    Speculation spec;
    // Resident executor (round 6; rq_resident.cpp): while the host keeps calling rq_step on the same small env / params / policy, or
    // rq_policy_evaluate_step on the same policy, the work is not launched but posted, as a 64-byte command, to one workgroup that stays
    // on the device - on a stream of its own - and publishes the same sequence numbers in mailbox.flag.  Anything else the device is asked
    // to do retires it first (resident_scope_hook).
    ResidentExecutor resident;
};
struct rq_rng {
    rq_device* dev = nullptr;
    uint64_t seed = 0;
    uint32_t epoch = 0;        // observation-noise counter: +1 per observe / per rollout step
    uint32_t param_epoch = 0;  // +1 per sample_initial_parameters
    bool initialized = false;
};

// Row tables on the device, [rows][cols] row-major each, one after another: a moving setpoint (rq_reference_create: one table), M of
// them (rq_reference_bank_create) or the tables of a schedule (rq_wrench_bank_create and its kin).  Env i of a rollout or of an env the
// tables are attached to reads the table that begins at row id[i] * rows; a single reference is every env's table 0.
namespace rqh {
struct RowTables {
    const rq_device* dev = nullptr;     // compared, never followed: the device may be gone before its tables
    int ordinal = 0;
    uint32_t n_tables = 0, rows = 0;
    DeviceBuffer<float> d;              // [n_tables * rows][cols] row-major
    uint64_t uid = fresh_version();     // what an env knows the tables by, beside their address (rq_env::row0_key)
};
// the tables of a schedule, of any kind: what an env's slot (rq::EnvSchedule) attaches
struct ScheduleBank : RowTables {
    uint32_t attached = 0;              // live envs it is attached to: the bank's destruction is refused while any
};

// What a kind of row tables is to the host: its words, its shape and what an entry may be.  The two references and the three kinds
// of schedule are rows of one table (kTableKinds); everything else about a schedule is the kernels'.
struct TableKind {
    const char* tables;                 // what a message calls the tables: "reference", "wrench bank"
    const char* noun;                   // a schedule's kind, as in "wrench schedule", "wrench id" (a reference: none)
    uint32_t cols;
    enum Rule { kFinite, kPositive, kNonNegativeColumn, kSteps } rule;      // every entry finite; and > 0; and those of `rule_col` >= 0;
                                        // kSteps: bytes, not floats, each at most RQ_DELAY_MAX_STEPS / RQ_SENSOR_MAX_STEPS (the bank's create makes its own check)
    int rule_col;                       // (a rule about columns names the column in every message)
    const char* detach;                 // the entry point that detaches: what a refused destruction names
};
// the schedules first, in the order every walk over them takes: it is the order in which refusals are heard
enum TableKindId { kWrench, kVehicle, kWind, kDelay, kSensor, kScheduleKinds, kReference = kScheduleKinds, kReferenceBank, kTableKindCount };
inline constexpr TableKind kTableKinds[kTableKindCount] = {
    {"wrench bank", "wrench", 6, TableKind::kFinite, -1, "rq_env_set_wrench_schedule"},
    {"vehicle bank", "vehicle", 4, TableKind::kPositive, -1, "rq_env_set_vehicle_schedule"},      // factors on mass, inertia, thrust, motor lag
    {"wind bank", "wind", 4, TableKind::kNonNegativeColumn, 3, "rq_env_set_wind_schedule"},       // air velocity, specific drag
    {"delay bank", "delay", 1, TableKind::kSteps, -1, "rq_env_set_delay_schedule"},               // control latency in steps
    {"sensor bank", "sensor", 1, TableKind::kSteps, -1, "rq_env_set_sensor_schedule"},            // observation latency in steps
    {"reference", nullptr, 6, TableKind::kFinite, -1, nullptr},
    {"reference bank", nullptr, 6, TableKind::kFinite, -1, nullptr},
};
}  // namespace rqh
struct rq_reference : rqh::RowTables {};
struct rq_reference_bank : rqh::RowTables {};
struct rq_wrench_bank : rqh::ScheduleBank { int units = RQ_WRENCH_RELATIVE; };
struct rq_vehicle_bank : rqh::ScheduleBank {};
struct rq_wind_bank : rqh::ScheduleBank {};
struct rq_delay_bank : rqh::ScheduleBank { rq::DeviceBuffer<uint8_t> steps; };      // [n_tables * rows] bytes; `d` stays empty
struct rq_sensor_bank : rqh::ScheduleBank { rq::DeviceBuffer<uint8_t> steps; };     // likewise

struct rq_env {
    rq_device* dev = nullptr;
    uint64_t uid = fresh_version();   // what the device's caches know this env by, beside its address
    int ordinal = 0;            // copy: destruction must not dereference the parent (GC order is arbitrary)
    uint32_t n = 0, ld = 0;
    uint64_t offset = 0;
    rq_env_config cfg{};
    bool initialized = false;
    DeviceBuffer<float> obs;    // [RQ_OBSERVATION_DIM][ld]
    DeviceBuffer<float> act;    // [RQ_ACTION_DIM][ld]
    DeviceBuffer<char> stats_block;
    rq::StatsPtrs st{};         // views into stats_block
    // tracked rollouts' statistics, [ld] float sums then [ld] uint32 counts, and behind them the [ld] uint32 first rows of a reference
    // bank's rollout (env_track_stats: first use)
    DeviceBuffer<char> track_block;
    // what the first rows were built from, cached as the policy bank caches its id table: (row0_key = the reference bank's uid,
    // row0_ids = one id per env) - a loop of rollouts with one assignment uploads them once; other ids wait for the stream, then
    // rewrite the rows.  row0_gen names the upload: a chained rollout's hipGraph is keyed by it.
    bool row0_valid = false;
    uint64_t row0_key = 0, row0_gen = 0;
    std::vector<uint32_t> row0_ids;
    // The schedules (rq_env_set_wrench_schedule and its kin), one slot per kind, indexed by rqh::TableKindId: the bank, the ids it was
    // attached with, the [ld] first rows every stepping kernel reads and the number that names the attachment.
    rq::EnvSchedule<rqh::ScheduleBank> schedule[rqh::kScheduleKinds];
    rq::DelayHistory delay_history;     // the delay schedule's command history: [rq::kDelaySlots][RQ_ACTION_DIM][ld]
    rq::DelayHistory sensor_history;    // the sensor schedule's readings: [rq::kSensorSlots][rq::kSensorFields][ld], a ring of its own
    bool has_sensor_schedule() const { return schedule[rqh::kSensor].bank != nullptr; }
    bool has_schedule() const { for (const auto& s : schedule) if (s.bank) return true; return false; }
    // chained rollouts replay a captured hipGraph of kGraphSteps steps (3 kernel nodes per step + the
    // epoch-counter bump); one executable graph per distinct argument set: what the nodes carry by value, named once
    struct GraphKey {
        const float* params = nullptr; float* state = nullptr; float* hidden = nullptr; const float* packed = nullptr;
        const float* weights = nullptr; const float* obs = nullptr;
        uint32_t flags = 0; int precision = 0; rq_env_config cfg{}; uint64_t seed = 0;
        int sas_mode = 0; uint64_t sas_seed = 0; const float* ls_image = nullptr;
        const float* ref = nullptr; uint32_t ref_rows = 0;     // tracked rollouts: the reference table (nullptr: untracked)
        uint32_t row0_at = 0; uint64_t row0_gen = 0;           // a reference bank's per-env first rows and which upload they are (0, 0: none)
        uint32_t interval = 1;                                 // the policy's native interval: the actor nodes of another one are other kernels
        uint64_t schedule_gen[rqh::kScheduleKinds] = {};      // the env's schedules at construction (0: none): the step nodes carry their pointers
        bool operator==(const GraphKey& o) const {             // field by field (padding is not compared); cfg is plain floats and words
            return params == o.params && state == o.state && hidden == o.hidden && packed == o.packed && weights == o.weights &&
                   obs == o.obs && flags == o.flags && precision == o.precision && seed == o.seed && sas_mode == o.sas_mode &&
                   sas_seed == o.sas_seed && ls_image == o.ls_image && ref == o.ref && ref_rows == o.ref_rows && row0_at == o.row0_at &&
                   row0_gen == o.row0_gen && interval == o.interval && std::equal(schedule_gen, schedule_gen + rqh::kScheduleKinds, o.schedule_gen) &&
                   std::memcmp(&cfg, &o.cfg, sizeof(rq_env_config)) == 0;
        }
    };
    struct GraphEntry { GraphKey key; hipGraphExec_t exec; };
    std::vector<GraphEntry> graphs;
    DeviceBuffer<uint32_t> epoch_dev;    // device-side noise epoch read by the graph's observe nodes
    bool obs_exposed = false;        // rq_env_observation_device_ptr was called: the caller may write the buffer (no observation cache)
    std::vector<float*> state_pool;  // state buffers [RQ_STATE_DIM][ld] no rq_state holds at the moment (copy-on-write assign)
    DeviceBuffer<float> obs_alt;     // [RQ_OBSERVATION_DIM][ld]: where k_step leaves the observation of the state it wrote; a cached
                                     // observe() swaps it with `obs` (the env's observation buffer changes on observe only)
};

// version: bumped by every library call that writes the buffer; exposed: the raw device pointer was handed out, the
// library no longer knows when it is written (the observation cache then never applies)
struct rq_params { rq_env* env = nullptr; int ordinal = 0; DeviceBuffer<float> d; uint64_t version = fresh_version(); bool exposed = false; };
// rq_state buffers are copy-on-write (round 3): state.assign(next_state) makes the two objects SHARE one buffer, and the
// next call that overwrites one of them (the following step writes next_state in full) gives it a fresh buffer from the
// env's pool instead - the README loop's assign costs no copy command.  `refs` counts the objects on a buffer.
struct rq_state { rq_env* env = nullptr; int ordinal = 0; float* d = nullptr; uint64_t version = fresh_version(); bool exposed = false;
                  int* refs = nullptr; };

struct rq_trajectory {
    rq_env* env = nullptr;
    int ordinal = 0;
    uint32_t capacity = 0, length = 0;
    DeviceBuffer<float> obs;     // [capacity][22][ld]
    DeviceBuffer<float> act;     // [capacity][4][ld]
    DeviceBuffer<float> rew;     // [capacity][ld]
    DeviceBuffer<uint8_t> done;  // [capacity][ld]
    // the learner's workspace (rq_capi_grad.cpp): what the last rq_trajectory_policy_forward saved for the backward, and by whom
    struct Grad {
        DeviceBuffer<float> saved;     // [length][16][ld]: the state entering each step
        DeviceBuffer<float> partial;   // [waves][2084]: per-wave partial gradients
        DeviceBuffer<float> rows;      // host-memory calls: the device side of the caller's arrays
        bool valid = false;            // a forward ran and nothing it read has changed since (rq_trajectory_reset clears it)
        const rq_policy* policy = nullptr;
        uint64_t weight_version = 0;   // rq_policy::weight_version at the forward
        uint32_t length = 0;
        int start = 0;                 // enum rq_grad_start
        void stamp(const rq_policy* pol, uint32_t steps, int from);      // `saved` is now pol's forward over `steps` steps from `from`
        bool matches(const rq_policy* pol, uint32_t steps) const { return valid && policy == pol && length == steps; }
        DeviceBuffer<float> out;       // the loss-seeded calls: grad [2084] | losses [n_updates] before they go to the caller
        DeviceBuffer<unsigned long long> live;    // [1]: M, the live entries of the last loss
        // the probes (rq_capi_probe.cpp): the waves' partial moments and counts (rq::probe_partial_floats), and the call's small
        // device-side block: moments | counts | age edges (| the targets of a host-memory call)
        DeviceBuffer<float> probe;
        DeviceBuffer<double> probe_io;
        // targets per step (rq_trajectory_probe_moments_timed): the device side of a host-memory call's targets [length][M][ld_targets]
        DeviceBuffer<float> probe_targets;
        // rq_trajectory_wrench_targets: first rows [n] | start steps [n] on the device, and the pinned rows they were copied from -
        // a call with the rows of the call before uploads nothing; other rows wait for the stream, then rewrite the pinned block
        DeviceBuffer<uint32_t> probe_rows;
        PinnedBuffer<uint32_t> probe_rows_host;
        bool probe_rows_valid = false;
        // rq_trajectory_flight_table: the start steps [n] on the device and the pinned block they were copied from, kept as the
        // wrench targets keep theirs - the starts of the call before upload nothing
        DeviceBuffer<uint32_t> flight_start;
        PinnedBuffer<uint32_t> flight_start_host;
        bool flight_start_valid = false;
    } grad;
};

struct rq_policy {
    rq_device* dev = nullptr;
    int ordinal = 0;
    DeviceBuffer<float> w_dev;           // raw parameters (checkpoint order)
    DeviceBuffer<float> w_packed;        // f32 MFMA operand image, rq::RQ_PACKED_FLOATS floats
    DeviceBuffer<float> w_packed_bf16;   // bf16 MFMA operand image, rq::RQ_PACKED_BF16_FLOATS floats
    DeviceBuffer<float> w_packed_f16x2;  // split-f16 MFMA operand image, rq::RQ_PACKED_F16X2_FLOATS floats
    float w_host[RQ_POLICY_NUM_WEIGHTS];      // as loaded (checkpoint order)
    float w_eff[RQ_POLICY_NUM_WEIGHTS];       // with the optional Standardize stage folded into layer_0
    bool standardize = false;
    float std_mean[RQ_POLICY_INPUT_DIM], std_inv[RQ_POLICY_INPUT_DIM];
    int sas_mode = RQ_SAS_OFF;        // SampleAndSquash output stage
    uint64_t sas_seed = 0;
    uint32_t sas_counter = 0;         // sampling step of the next rq_policy_evaluate_step call
    uint32_t native_interval = 1;     // rq_policy_set_native_interval: the hidden state moves on every native_interval-th step
    uint32_t rate_counter = 0;        // index k of the next rq_policy_evaluate_step call (native iff k % native_interval == 0)
    DeviceBuffer<float> ls_image;     // rq::RQ_LOGSTD_FLOATS (log-std head operands), allocated on first use
    int precision = RQ_POLICY_FP32;
    uint32_t batch = 0, ld = 0;   // 0 = not sized yet
    bool needs_reset = true;      // hidden must be (re)filled with initial_hidden_state before use
    DeviceBuffer<float> hidden;      // [16][ld]
    DeviceBuffer<float> hidden_alt;  // [16][ld]: where a speculative step leaves the next hidden state (swapped in on a hit)
    uint64_t version = fresh_version();   // renewed by every call that reads-and-writes or reconfigures the policy's state
    uint64_t weight_version = fresh_version();   // renewed whenever the parameters are (re)uploaded: create, set_standardize, set_weights
    DeviceBuffer<float> w_packed_grad;    // the learner's transposed image, rq::RQ_PACKED_GRAD_FLOATS floats (allocated on first use)
    uint64_t grad_image_version = 0;  // the weight_version w_packed_grad was packed from
    DeviceBuffer<float> obs;      // [22][ld] staging for host observations
    DeviceBuffer<float> act;      // [4][ld]
    // A device-side update (rq_trajectory_distill) writes w_dev, w_packed and w_packed_grad only.  Until policy_mirror() has fetched
    // w_dev, w_host / w_eff are not read (policy_size fills the state from w_dev), and the 16-bit images are repacked before a
    // 16-bit precision is next selected.
    bool mirror_stale = false;    // w_host, w_eff are older than w_dev
    bool images16_stale = false;  // w_packed_bf16, w_packed_f16x2 are older than w_dev
};

inline void rq_trajectory::Grad::stamp(const rq_policy* pol, uint32_t steps, int from) {
    valid = true; policy = pol; weight_version = pol->weight_version; length = steps; start = from;
}

// Adam's state (rq_capi_grad.cpp adam_alloc) for one policy (kernel: rq_grad.hpp k_adam_repack) or a bank's (rq_grad_bank.hpp)
namespace rqh {
struct AdamBuffers {
    rq_device* dev = nullptr;
    int ordinal = 0;
    DeviceBuffer<float> m, v, grad;          // [slots][2084] each
    DeviceBuffer<rq::AdamState> state;       // [slots]: every hyper-parameter per policy
    DeviceBuffer<rq::PackGather> table;      // pack_gather_table, shared
};
}  // namespace rqh
struct rq_optimizer : rqh::AdamBuffers { rq_policy* policy = nullptr; };
struct rq_policy_bank;
struct rq_bank_optimizer : rqh::AdamBuffers {
    const rq_policy_bank* bank = nullptr;    // compared, with bank_uid, never followed
    uint64_t bank_uid = 0;
    uint32_t n_policies = 0;
};

struct rq_teacher_bank {
    rq_device* dev = nullptr;
    int ordinal = 0;
    uint32_t n_teachers = 0, in_dim = 0, h1 = 0, h2 = 0;
    int act = RQ_ACT_RELU, out_act = RQ_ACT_IDENTITY;
    int precision = RQ_POLICY_FP32;
    DeviceBuffer<float> images_f32;      // [n_teachers][teacher_image_regs_f32 * 64]
    DeviceBuffer<float> images_bf16;     // [n_teachers][teacher_image_regs_bf16 * 64]
    DeviceBuffer<float> images_f16x2;    // [n_teachers][teacher_image_regs_f16x2 * 64]
    uint32_t f16x2_misfit = UINT32_MAX;  // the first teacher with a weight the f16x2 image cannot hold (set_precision refuses it)
    DeviceBuffer<uint32_t> tiles;    // tile_teacher [tiles] followed by tile_env [tiles][16]; dense stacks: teacher_start | sorted_env
    // the generic dense stack (rq_teacher_bank_create_layers outside the register-stationary family): fp32, operands streamed
    bool layers = false;
    uint32_t n_hidden = 2, widths[3] = {0, 0, 0}, hp = 0;
    DeviceBuffer<float> images_layers;   // [n_teachers][teacher_layers_image_floats(hp, n_hidden)]
    // what `tiles` holds (rq_capi_teacher.cpp bank_tiles): the list built from tiles_ids for tiles_key (the env's uid, 0 = host rows)
    // - a loop of rollout chunks or relabels with one assignment uploads it once
    bool tiles_valid = false;
    uint64_t tiles_key = 0;
    uint32_t tiles_count = 0;
    std::vector<uint32_t> tiles_ids;
    // teacher rollouts, chained mode: k_step's policy-state reset needs a [16][ld] target and a weight block (a teacher has no state)
    DeviceBuffer<float> sink;
    // rq_teacher_bank_evaluate from host rows: [batch][stride] rows | [22][ld] observation | [4][ld] actions
    DeviceBuffer<float> eval_buf;
};

// a bank of fp32 student policies flown one per 64-env block (rq_capi_policy_bank.cpp)
struct rq_policy_bank {
    rq_device* dev = nullptr;
    int ordinal = 0;
    uint32_t n_policies = 0;
    DeviceBuffer<float> images;      // [n_policies][rq::RQ_PACKED_FLOATS]: the images rq::pack_policy makes, slot after slot
    DeviceBuffer<float> weights;     // [n_policies][RQ_POLICY_NUM_WEIGHTS], checkpoint order: the initial hidden states are read here
    // the per-block id table and what it was built from: (table_key = the env's uid, table_ids = one id per block) - a loop of
    // rollouts with one assignment uploads it once (as rq_teacher_bank::tiles)
    DeviceBuffer<uint32_t> table;    // [blocks]
    bool table_valid = false;
    uint64_t table_key = 0;
    std::vector<uint32_t> table_ids;
    uint32_t batch = 0, ld = 0;      // 0 = not sized yet
    bool needs_reset = true;         // hidden must be (re)filled with every env's own policy's initial state before use
    DeviceBuffer<float> hidden;      // [16][ld]
    // rq_policy_bank_set_native_interval: policy p's hidden state moves on every intervals[p]-th step.  The device table is what the
    // RATE kernels read; `rated` = any entry above 1 (all 1: the rollout launches the kernels it launched before the table existed)
    std::vector<uint32_t> intervals;         // [n_policies], the host's copy
    DeviceBuffer<uint32_t> intervals_dev;    // [n_policies]
    bool rated = false;
    // the learner (rq_trajectory_policies_loss_grad / _distill): the transposed images, packed from `weights` at the first learner
    // use and kept current from then on (rq_policy_bank_set_weights; a device-side update writes them itself), and the policies'
    // waves as a CSR list built from table_ids - valid while `table` is what it was built from
    uint64_t uid = fresh_version();  // what an optimizer knows its bank by, beside the address
    DeviceBuffer<float> gimages;     // [n_policies][rq::RQ_PACKED_GRAD_FLOATS]
    DeviceBuffer<uint32_t> waves;    // wave_offsets [n_policies + 1] | wave_list [blocks]
    bool waves_valid = false;
};

// From kGpuLayoutMinEnvs envs up the row-major <-> field-major change runs on the GPU (k_soa_to_rows /
// k_rows_to_soa) and the PCIe copy goes straight between the caller's array and a device row buffer; below
// it the few KB are transposed by the host through a pinned staging buffer (one launch less).
constexpr uint32_t kGpuLayoutMinEnvs = 1024;

namespace rqh {

// ---- rq_capi.cpp ----
// live rq_device / rq_policy / rq_policy_bank objects (op: +1 register, -1 unregister, 0 query): objects die in any order, a parent or a remembered
// policy is followed only while it is in here
bool device_registry(const void* dev, int op);
bool policy_registry(const void* pol, int op);
bool policy_bank_registry(const void* bank, int op);
int soa_to_host(rq_device* dev, const float* d_soa, uint32_t n, uint32_t ld, uint32_t dim, float* host);
int host_to_soa(rq_device* dev, const float* host, uint32_t n, uint32_t stride, uint32_t ld, uint32_t dim, float* d_soa);
int check_env_objects(const rq_device* dev, const rq_env* env, const rq_params* params, const rq_state* state);
int state_fresh_buffer(rq_env* env, float** out);
void state_release_buffer(rq_state* s);
int state_make_private(rq_state* s, bool keep);
inline rq::Batch batch_of(const rq_env* env) { return {env->n, env->ld, env->offset}; }
// the env's tracking statistics, allocated and zeroed (on the device's stream) at their first use; call inside a DeviceScope
int env_track_stats(rq_env* env, float** sum_sq, uint32_t** steps);
// ---- rq_capi_rollout.cpp: the env's schedules ----
// One schedule as the kernels take it, before it is typed (all-null: none attached).  `flag`: the wrench bank's units, 1 = relative.
// `ring`: the delay schedule's command history, the sensor schedule's readings.
struct SchedulePtrs { const void* rows = nullptr; const uint32_t* row0 = nullptr; uint32_t n_rows = 0, flag = 0; float* ring = nullptr; };
int schedule_too_short(const char* who, const rq_env* env, int kind);      // the refusal below, worded
// The env's schedules, p[kScheduleKinds] in kind order.  Every call that steps asks here before anything is enqueued: a bank with
// fewer rows than episode_step_limit is refused, but a delay or a sensor bank (`who`: the caller's name; the config may have changed since the schedule was
// attached).  Nothing is allocated and no string made unless it refuses: rq_step asks on every call.
inline int env_schedules(const char* who, const rq_env* env, SchedulePtrs* p) {
    for (int k = 0; k < kScheduleKinds; ++k) {
        p[k] = SchedulePtrs{};
        const auto& s = env->schedule[k];
        if (!s.bank) continue;
        // (a delay table shorter than an episode holds its last row: a latency is a property of the link, not a course of events)
        if (k != kDelay && k != kSensor && s.bank->rows < env->cfg.episode_step_limit) return schedule_too_short(who, env, k);
        p[k] = {s.bank->d.get(), s.row0, s.bank->rows,
                k == kWrench && static_cast<const rq_wrench_bank*>(s.bank)->units == RQ_WRENCH_RELATIVE ? 1u : 0u, nullptr};
        if (k == kDelay) { p[k].rows = static_cast<const rq_delay_bank*>(s.bank)->steps.get(); p[k].ring = env->delay_history.ring; }
        if (k == kSensor) { p[k].rows = static_cast<const rq_sensor_bank*>(s.bank)->steps.get(); p[k].ring = env->sensor_history.ring; }
    }
    return RQ_OK;
}
// the sensor schedule as k_sensor_apply and k_rollout_fused_sensor take it
inline rq::SensorPtrs sensor_ptrs(const SchedulePtrs* p) {
    return {static_cast<const uint8_t*>(p[kSensor].rows), p[kSensor].row0, p[kSensor].ring, p[kSensor].n_rows, 0u};
}
// ... typed, for the launch descriptions (rq::EnvStepLaunch, rq::FusedArgs): the kernels' argument types are one per kind
template <typename Launch>
void set_schedules(Launch& l, const SchedulePtrs* p) {
    l.wr = {static_cast<const float*>(p[kWrench].rows), p[kWrench].row0, p[kWrench].n_rows, p[kWrench].flag};
    l.vh = {static_cast<const float*>(p[kVehicle].rows), p[kVehicle].row0, p[kVehicle].n_rows, 0u};
    l.wd = {static_cast<const float*>(p[kWind].rows), p[kWind].row0, p[kWind].n_rows, 0u};
    l.dl = {static_cast<const uint8_t*>(p[kDelay].rows), p[kDelay].row0, p[kDelay].ring, p[kDelay].n_rows, 0u};
    l.sn = sensor_ptrs(p);
}
// What fused mode cannot fly while a schedule of `kind` is attached, refused naming the schedule (`what`: a bf16 / f16x2 policy, a
// SampleAndSquash stage, a teacher bank, another schedule beside it); nothing runs chained in its place.
int refuses_fused(const char* who, int kind, const char* what);

// ---- rq_small_batch.cpp: the small-batch loop (rq_device::mailbox, obs_cache, spec) ----
void small_batch_setup(rq_device* dev);      // rq_device_create: settings
int ensure_mailbox(rq_device* dev);
int mailbox_wait(rq_device* dev, uint32_t seq);
int mailbox_copy_out(rq_device* dev, uint32_t seq, const float* rows, float* dst, size_t floats);
int mailbox_put_in(rq_device* dev, const float* rows, uint32_t n, uint32_t dim, size_t stride);
rq::Mailbox mailbox_for(rq_device* dev, bool reads_in, uint32_t in_stride, MbOut out);
int mailbox_for_step(rq_device* dev, const float* action, uint32_t n, bool cache_obs, rq::Mailbox* mb);
void mailbox_abort(rq_device* dev, const rq::Mailbox& mb);
void mailbox_resident_args(const rq_device* dev, rq::ResidentArgs& ra, bool policy_kind);
bool obs_cache_holds(const rq_device* dev, const rq_env* env, const rq_params* params, const rq_state* state);
int obs_cache_read(rq_device* dev, rq_env* env, float* observation);
void obs_cache_drop(rq_device* dev);
void obs_cache_drop_if(rq_device* dev, const rq_env* env);     // only if the cache holds env's observation
void obs_cache_fill(rq_device* dev, const rq_env* env, const rq_params* params, const rq_state* state, uint32_t seq, rq_policy* pol, uint32_t spec_seq);
void obs_cache_follow_assign(rq_device* dev, const rq_state* dst, const rq_state* src);
rq_policy* speculation_candidate(rq_device* dev, const rq_env* env, bool cache_obs, bool action);
int speculation_take(rq_device* dev, rq_policy* pol, const float* observation, uint32_t batch, uint32_t obs_stride, float* action, bool* hit);
hipError_t launch_step_pair(rq_device* dev, const StepPair& p);

// ---- rq_resident.cpp: the resident executor ----
uint64_t host_now_ns();
void resident_setup(rq_device* dev);         // rq_device_create: settings, stream and command memory (a failure is tolerated)
void resident_teardown(rq_device* dev);      // rq_device_destroy: retire, free
int resident_retire(rq_device* dev);         // tell a running kernel to leave and wait until it has
int resident_gone(rq_device* dev);           // the kernel has left: replay its command if it never consumed it
bool resident_left(const rq_device* dev);    // has the running kernel published that it left?
int resident_admit(rq_device* dev, bool ready, const ResidentBinding& want, uint64_t now_ns, uint32_t streak, bool* use);
int resident_start(rq_device* dev, rq::ResidentArgs& ra, const ResidentBinding& want);
void resident_post(rq_device* dev, const StepPair& p);      // the command's rows and checksum, then its line
void resident_post(rq_device* dev, const PolicyCmd& p);
int resident_drain(rq_device* dev);

// ---- rq_capi_policy.cpp ----
int mode_of(const rq_policy* pol);       // precision in bits 0-7, bit 8 = tanh on the output (what the sequence / relabel launchers take)
rq::SasArgs sas_of(const rq_policy* pol, uint32_t epoch, const uint32_t* epoch_base, uint64_t env_offset);
const float* packed_of(const rq_policy* pol);
int policy_size(rq_policy* pol, uint32_t batch);
int policy_mirror(rq_policy* pol);       // w_host / w_eff <- w_dev after a device-side update (one 8 KB copy; nothing to do otherwise)
int policy_images16(rq_policy* pol);     // the bf16 / f16x2 images repacked from the weights if an update left them behind
// what is defined at the native rate only (sequence evaluation, relabelling, the learner, the self test) refuses a policy whose
// native interval is above 1: a recording does not carry the phase it started at
int require_native_rate(const rq_policy* pol, const char* what);

// ---- rq_capi_grad.cpp: what the learner and the probes (rq_capi_probe.cpp) share ----
// what every call over a (recording, policy) pair refuses: only the fp32 student without input or output stages, at the native rate
int grad_check_pair(rq_trajectory* t, rq_policy* pol, const char* what);
// inside the caller's DeviceScope: t->grad.saved holds the state of a forward by `pol` from the learned initial state at its current
// weights - the one a forward or a loss call left if its tags say so, else the state-only forward is enqueued and tagged
int grad_saved_initial(rq_trajectory* t, rq_policy* pol);
// what every `memory` argument refuses: its range; an array (`noun`: as the message names it) that is not the call's device's memory
int check_memory(int memory);
int check_device_array(const CallMemory& mem, const void* p, const char* what, const char* noun);

// ---- rq_capi_policy_bank.cpp: what the bank's rollout and its learner (rq_capi_grad.cpp) share; all but bank_check_ids need the
// caller's DeviceScope ----
int bank_check_ids(const rq_policy_bank* bank, const uint32_t* policy_id, uint32_t n);      // before anything is enqueued
int bank_table(rq_policy_bank* bank, rq_device* dev, uint64_t key, const uint32_t* policy_id, uint32_t n);
int bank_size(rq_policy_bank* bank, uint32_t batch);
int bank_apply_reset(rq_policy_bank* bank);
int bank_grad_images(rq_policy_bank* bank);       // gimages packed from the device's weights, once
int bank_wave_lists(rq_policy_bank* bank);        // `waves` for the current table
// what is defined at the native rate only (the bank's learner) refuses a bank with a native interval above 1, as
// require_native_rate refuses a policy
int require_bank_native_rate(const rq_policy_bank* bank, const char* what);

// ---- rq_capi_rollout.cpp: the frame of every rollout ----
// One call of any of the ten rq_rollout* entry points, as its body describes it.
struct RolloutCall {
    const char* who;                  // the public entry point's name: what a refusal's message begins with
    rq_device* dev; rq_env* env; const rq_params* params; rq_state* state; rq_rng* rng;
    uint32_t n_steps; int mode; uint32_t flags; rq_trajectory* traj;
    const RowTables* tables;          // a tracked rollout's reference or reference bank (null: untracked)
    const uint32_t* reference_id;     // a reference bank's table per env (null: `tables` is one reference, every env's table)
};
// What rollout_run gathers on its way and the launches take: where a recording goes, the tracked rollout's pointers, the env's
// schedules and the env's configuration as the kernels take it.
struct RolloutFrame {
    rq::TrajPtrs tp{nullptr, nullptr, nullptr, nullptr, 0};
    rq::TrackPtrs trk{};                                          // ref != nullptr: a tracked rollout
    uint64_t row0_gen = 0;                                         // a reference bank's rollout: rq_env::row0_gen
    SchedulePtrs sched[kScheduleKinds];                            // rows != nullptr: the env carries a schedule of that kind (rollout_check)
    rq::Batch b; rq::StepCfg sc; rq::NoiseCfg nc; rq::SampleCfg smp; bool noise;
};
// a refusal inside the frame, worded as RQ_REQUIRE words it but begun with the call's own name
#define RQ_REFUSE(who, cond, status, msg)                                          \
    do {                                                                           \
        if (!(cond)) return rq::fail((status), std::string(who) + ": " + (msg));   \
    } while (0)
// The pieces of rollout_run, in its order.  rollout_check, before the call's DeviceScope: what every rollout refuses (`actor`: the
// caller was given what acts), where a recording goes, the env's schedules and which of them fused mode does not fly side by side.
// rollout_check_tables: a tracked rollout's tables and, with ids, every id (one outside the bank is refused naming the env).  rollout_track, inside the scope: the tracked
// rollout's pointers; with ids the per-env first rows go to the device unless the env holds them for (tables, ids) already.
// rollout_begin, after the actor's preparation: the observation cache dropped, the state private, the env's configuration as the
// kernels take it, the `done` rows preset.  rollout_end: the noise epoch, the recording's length and the state's version move on.
int rollout_check(RolloutFrame& f, const RolloutCall& c, bool actor);
int rollout_check_tables(const RolloutCall& c);
int rollout_track(RolloutFrame& f, const RolloutCall& c);
int rollout_begin(RolloutFrame& f, const RolloutCall& c);
void rollout_end(const RolloutCall& c);
// A failed rq::upload_first_rows or rq::EnvSchedule::attach, worded: `what` ("reference bank", "wrench schedule") begins the message
// of a failed allocation.
int first_rows_failed(const char* what, const rq::FirstRowsStatus& s);
// a failed HIP call of a shared piece, reported as the caller's own RQ_HIP would: `who` is the caller's name, `what` the call
inline int hip_failed(const char* who, const char* what, hipError_t e) {
    return fail(e == hipErrorOutOfMemory ? RQ_ERR_OUT_OF_MEMORY : RQ_ERR_HIP, std::string(who) + ": " + what + " -> " + hipGetErrorString(e));
}
// RQ_HIP inside a body several entry points share: the message begins with the entry point's name
#define RQ_HIP_AS(who, expr)                                                \
    do {                                                                    \
        const hipError_t e_ = (expr);                                       \
        if (e_ != hipSuccess) return rqh::hip_failed((who), #expr, e_);     \
    } while (0)
// The fused mode of a policy or a policy bank.  fused_args: the launch description, all but the actor; the actor adds its fields and
// calls fused_launch: under rq_device_set_rollout_timing the span buffer sized for the env's waves, the one
// rq::launch_rollout_fused (rq_fused_route.hpp picks the kernel), and behind it what rq_device_last_rollout_ms goes by.
rq::FusedArgs fused_args(const RolloutCall& c, const RolloutFrame& f);
int fused_launch(const RolloutCall& c, rq::FusedArgs& a);
// The chained mode's env step, and its thaw: the description, all but the actor's share of it - where a policy state is reset
// (hidden, weights, block_policy) and, folding, the next observation.  A rollout's step, in place.
rq::EnvStepLaunch env_step_launch(const RolloutCall& c, const RolloutFrame& f);

constexpr uint32_t kGraphSteps = 25;   // steps per replayed graph (divides the 500-step episode)
constexpr size_t kMaxGraphs = 8;       // executable graphs kept per env (one per distinct argument set)

// The chained rollout: thaw under auto-reset, then per step observe -> the setpoint taken off the observation if tracked (one small
// kernel in front of the actor, wherever the observation came from; it keeps the tracking error) -> actor -> step -> record if
// recording, on the device's stream.  The actor's launches: thaw(c, f), act(c, f, epoch, epoch_base), step(c, f, epoch, epoch_base,
// fold), each -> hipError_t; the env's episode step count is that of this step's observation until `step` moves it on.
// An actor with kFoldAndReplay (one policy) turns two options on when nothing is recorded.  fold: its step kernel also assembles the
// NEXT step's observation (two launches per step instead of three; the rollout's first observation is a launch of its own, the one
// the last step assembles is not used and never shifted).  Replay: kGraphSteps steps go out as one hipGraph keyed by what the
// actor's graph_key(c, f) says its nodes carry by value; kernel boundaries stay (~1.5 us each) but the host no longer pays ~3.5 us
// per launch, which is what bounds small batches.  The banks go out as plain launches.
template <typename Actor>
int rollout_chained(const RolloutCall& c, const RolloutFrame& f, const Actor& actor) {
    rq_device* dev = c.dev; rq_env* env = c.env; const rq_rng* rng = c.rng;
    const uint32_t n_steps = c.n_steps;
    const bool fold = Actor::kFoldAndReplay && !c.traj;
    const char* what = "";            // the launch a failure is reported for
    // A sensor schedule: k_sensor_apply delivers in env->obs, right behind whatever assembled the observation there - the observe
    // launch, or the step that folds the next one - and in front of the setpoint's shift; one more kernel node per step of a graph.
    const rq::SensorPtrs sn = sensor_ptrs(f.sched);
    auto deliver = [&](hipError_t e) -> hipError_t {
        if (e != hipSuccess || !sn.rows) return e;
        what = "rq::launch_sensor_apply";
        return rq::launch_sensor_apply(dev->stream, f.b, env->st, env->obs, sn);
    };
    auto one_step = [&](uint32_t epoch, const uint32_t* epoch_base, uint32_t t_record) -> hipError_t {
        hipError_t e = hipSuccess;
        if (!fold) {
            what = "rq::launch_observe";
            e = deliver(rq::launch_observe(dev->stream, f.b, f.nc, f.noise, rng->seed, epoch, epoch_base, c.params->d, c.state->d, env->obs));
        }
        if (e == hipSuccess && f.trk.ref) { what = "rq::launch_track_shift"; e = rq::launch_track_shift(dev->stream, f.b, c.state->d, env->st, env->obs, f.trk); }
        if (e == hipSuccess) { what = "the actor launch"; e = actor.act(c, f, epoch, epoch_base); }
        if (e == hipSuccess) { what = "the step launch"; e = actor.step(c, f, epoch, epoch_base, fold); if (fold) e = deliver(e); }
        if (e == hipSuccess && c.traj) {
            rq::TrajPtrs tt = f.tp; tt.t0 = f.tp.t0 + t_record;
            what = "rq::launch_record"; e = rq::launch_record(dev->stream, f.b, env->obs, env->act, env->st, tt);
        }
        return e;
    };
    hipError_t e = hipSuccess;
    if (n_steps && (c.flags & RQ_ROLLOUT_AUTORESET))      // envs frozen by an earlier rollout start their next episode
        if ((e = actor.thaw(c, f)) != hipSuccess) return hip_failed(c.who, "the thaw launch", e);
    if (fold && n_steps) {           // the rollout's first observation (after the thaw: of the re-sampled states)
        what = "rq::launch_observe";
        e = deliver(rq::launch_observe(dev->stream, f.b, f.nc, f.noise, rng->seed, rng->epoch, nullptr, c.params->d, c.state->d, env->obs));
        if (e != hipSuccess) return hip_failed(c.who, what, e);
    }
    uint32_t done_steps = 0;
    if constexpr (Actor::kFoldAndReplay) {
        if (fold && n_steps >= kGraphSteps) {
            const rq_env::GraphKey key = actor.graph_key(c, f);     // another value of any of its fields is another graph
            const uint32_t step_nodes = (f.trk.ref ? 3u : 2u) + (sn.rows ? 1u : 0u);
            hipGraphExec_t exec = nullptr;
            for (auto& g : env->graphs)
                if (g.key == key) { exec = g.exec; break; }
            if (!exec) {
                // Built node by node (rq_kernels.hpp GraphSink), NOT by stream capture: while any stream of a process captures, HIP
                // fails hipDeviceSynchronize on every other thread (hipErrorStreamCaptureUnsupported) and invalidates the capture -
                // a learner's PyTorch thread on the same GPU broke the rollout and was broken by it (tools/foreign_soak.py, round 6).
                // Should the construction fail all the same, the steps go out as plain launches: same kernels, same order.
                hipGraph_t graph = nullptr;
                hipError_t ce = dev->graphs_enabled ? hipGraphCreate(&graph, 0) : hipErrorNotSupported;
                if (ce == hipSuccess) {
                    rq::GraphSink sink;
                    sink.graph = graph;
                    rq::set_graph_sink(&sink);
                    for (uint32_t t = 0; t < kGraphSteps && ce == hipSuccess; ++t) ce = one_step(t, env->epoch_dev, 0);
                    if (ce == hipSuccess) ce = rq::launch_add_u32(dev->stream, env->epoch_dev, kGraphSteps);
                    rq::set_graph_sink(nullptr);
                    if (ce == hipSuccess && sink.nodes != step_nodes * kGraphSteps + 1) ce = hipErrorUnknown;     // a launcher that bypassed the sink
                }
                if (ce == hipSuccess) ce = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
                if (graph) (void)hipGraphDestroy(graph);
                if (ce != hipSuccess) {
                    (void)hipGetLastError();         // the failed construction's; the direct launches below report their own
                    exec = nullptr;
                    ++dev->graph_fallbacks;
                } else {
                    if (env->graphs.size() >= kMaxGraphs) {        // least recently created goes (a replay is cheap to rebuild)
                        RQ_HIP(hipStreamSynchronize(dev->stream));
                        (void)hipGraphExecDestroy(env->graphs.front().exec);
                        env->graphs.erase(env->graphs.begin());
                    }
                    try {                       // nothing throws across the boundary
                        env->graphs.push_back({key, exec});
                    } catch (const std::bad_alloc&) {
                        (void)hipGraphExecDestroy(exec);
                        return fail(RQ_ERR_OUT_OF_MEMORY, "rollout: host allocation failed");
                    }
                }
            }
            if (exec) {
                RQ_HIP(rq::launch_set_u32(dev->stream, env->epoch_dev, rng->epoch));
                for (; done_steps + kGraphSteps <= n_steps; done_steps += kGraphSteps)
                    RQ_HIP(hipGraphLaunch(exec, dev->stream));
            }
        }
    }
    for (uint32_t t = done_steps; t < n_steps; ++t)
        if ((e = one_step(rng->epoch + t, nullptr, t)) != hipSuccess) return hip_failed(c.who, what, e);
    return RQ_OK;
}

// A rollout of any kind, start to end: every refusal comes before the DeviceScope, hence before anything is enqueued or any object
// modified.  The actor (one policy: rq_capi_rollout.cpp; a policy bank: rq_capi_policy_bank.cpp; the teacher bank:
// rq_capi_teacher.cpp) supplies given() (it was handed what acts), check(c, f) (its refusals, its own device first), prepare(c)
// (inside the scope: sizing, tables, a pending reset, the sink), fused(c, f) and the chained launches rollout_chained takes.
template <typename Actor>
int rollout_run(const RolloutCall& c, Actor actor) {
    RolloutFrame f;
    int rc = rollout_check(f, c, actor.given()); if (rc) return rc;
    rc = actor.check(c, f); if (rc) return rc;
    rc = rollout_check_tables(c); if (rc) return rc;
    DeviceScope on_device(c.dev); rc = on_device.rc; if (rc) return rc;
    rc = actor.prepare(c); if (rc) return rc;
    rc = rollout_track(f, c); if (rc) return rc;
    rc = rollout_begin(f, c); if (rc) return rc;
    rc = c.mode == RQ_ROLLOUT_FUSED ? actor.fused(c, f) : rollout_chained(c, f, actor); if (rc) return rc;
    rollout_end(c);
    return RQ_OK;
}
int traj_block_to_host(rq_device* dev, const float* d_soa, uint32_t steps, uint32_t n, uint32_t ld, uint32_t dim, float* host);

template <typename T>
int copy_out(const rq_env* env, const T* src, T* dst, int dst_is_device) {
    RQ_REQUIRE(env && dst, RQ_ERR_INVALID_ARGUMENT, "null argument");
    DeviceScope on_device(env->dev); int rc = on_device.rc; if (rc) return rc;
    RQ_REQUIRE(CallMemory::valid(dst_is_device), RQ_ERR_INVALID_ARGUMENT, "dst_is_device must be 0, 1 or 2");
    CallMemory mem(dst_is_device, env->dev->stream, env->dev->ordinal);
    RQ_HIP(hipMemcpyAsync(dst, src, (size_t)env->n * sizeof(T),
                          dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, env->dev->stream));
    RQ_HIP(mem.finish());
    return RQ_OK;
}


}  // namespace rqh

#define RQ_HIP_MB(expr, dev, mb)                                                                  \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            mailbox_abort((dev), (mb));                                                           \
            return fail(RQ_ERR_HIP, std::string(__func__) + ": " #expr " -> " + hipGetErrorString(e_)); \
        }                                                                                         \
    } while (0)

