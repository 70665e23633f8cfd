// rq_resident.cpp - the resident executor's host side (round 6): one workgroup that stays on the device, on a stream of its own, and takes
// commands in memory instead of launches - the README loop's rq_step (rq_kernels.hip k_resident_small / k_resident_loop) or the policy
// alone, rq_policy_evaluate_step on host rows (k_resident_policy); one kernel per device at a time.  What a kind computes stays with its
// caller; the command format - line, rows, checksum - is this file's.
#include "rq_objects.hpp"

namespace rqh {

constexpr uint32_t kResidentStreak = 3;               // eligible steps in a row before a kernel is started
// The loop must really be running: an eligible step counts towards the streak only when it follows the previous one within 200 us (the
// README loop as the reference writes it sleeps 10 ms per step: it keeps its launches, nothing spins for it).
constexpr uint64_t kResidentMaxGapNs = 200000;
constexpr uint64_t kResidentIdleTicks = 30000;        // the kernel leaves after 300 us without a command (100 MHz ticks) ...
constexpr uint64_t kResidentHostIdleNs = 150000;      // ... and the host stops posting to one it has not fed for 150 us
// A kernel that never ends would make hipDeviceSynchronize - a learner's torch.cuda.synchronize() on another thread, any hipFree - wait
// for as long as the loop runs: the kernel leaves between two commands once it is 1 ms old, and the host, which knows its age, retires it
// at 0.75 ms and starts the next one (one launch per ~100 iterations at 8 envs).
constexpr uint64_t kResidentLifeTicks = 100000;
constexpr uint64_t kResidentHostLifeNs = 750000;
// A kernel that left by itself (idle) after fewer than 8 commands was not worth its launch - something stalls the loop that the host
// cannot see (a device-wide synchronize of the caller's own, a slow consumer): the next kernel is started only after 8, 16, ... 1 024
// further eligible steps; a kernel that served 64 commands resets that.
constexpr uint32_t kResidentMinCommands = 8, kResidentGoodCommands = 64, kResidentMaxBackoff = 1024;

// The executor's memory in 32-bit words: `mem` (pinned host memory) holds all of it; `cmd`, where commands are written, is `mem` or
// fine-grained device memory with the line and the rows at the same places.
enum ResidentWord : uint32_t {
    kRwLine = 0,                  // [0..15] the command line (rq::ResidentPacket)
    kRwExited = 16, kRwWhy = 17,  // written by the kernel as it leaves: its launch id, and why (rq::kRbLeftIdle / kRbLeftOld; 0: told to)
    kRwTiming = 32,               // [32..43] six 64-bit timestamps of the last command (RQ_RESIDENT_TIMING)
    kRwRows = 64,                 // the rows beside a command (12 x 4 action dwords; 16 x 24 observation dwords; 256 x 4 in device memory)
};
constexpr size_t kResMemBytes = 4096, kResCmdBytes = 8192;

uint64_t host_now_ns() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

// ---- memory -----------------------------------------------------------------------------------------------------------------------
static int ensure_memory(rq_device* dev) {
    ResidentExecutor& rx = dev->resident;
    if (rx.mem) return RQ_OK;
    PinnedBuffer<uint32_t> mem;
    RQ_HIP(mem.alloc(kResMemBytes / sizeof(uint32_t)));
    std::memset(mem.get(), 0, kResMemBytes);
    RQ_HIP(hipStreamCreateWithFlags(&rx.stream, hipStreamNonBlocking));
    rx.mem = std::move(mem);
    rx.cmd = rx.mem;
    // Where the wave looks for its commands.  Pinned host memory works everywhere: every poll is a read across PCIe, and a command is
    // seen ~1.7 us after it was written.  Where the platform maps VRAM for the CPU (large BAR) the command line lives in fine-grained
    // device memory instead: the host's stores cross PCIe once, as posted writes, the wave polls its own memory - a host -> wave ->
    // host round trip of 1.8 us instead of 2.5 (tools/bar_probe.hip).  The host never reads that memory.
    int large_bar = 0;
    if (std::getenv("RQ_RESIDENT_HOST_COMMANDS") == nullptr &&
        hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, dev->ordinal) == hipSuccess && large_bar) {
        void* fine = nullptr;
        if (hipExtMallocWithFlags(&fine, kResCmdBytes, hipDeviceMallocFinegrained) == hipSuccess) {
            // zeroed by the host through the BAR it will write its commands through (a hipMemset of this memory costs 8 ms the first time)
            __m128i* z = static_cast<__m128i*>(fine);
            for (size_t k = 0; k < kResCmdBytes / sizeof(__m128i); ++k) _mm_store_si128(z + k, _mm_setzero_si128());
            _mm_sfence();
            rx.cmd_dev.adopt(static_cast<uint32_t*>(fine), kResCmdBytes / sizeof(uint32_t));
            rx.cmd = rx.cmd_dev;
            rx.cmd_on_device = true;
        }
        (void)hipGetLastError();
    }
    return RQ_OK;
}

void resident_setup(rq_device* dev) {
    ResidentExecutor& rx = dev->resident;
    rx.enabled = std::getenv("RQ_NO_RESIDENT") == nullptr;
    rx.timing = std::getenv("RQ_RESIDENT_TIMING") != nullptr;
    rx.idle_ticks = kResidentIdleTicks; rx.life_ticks = kResidentLifeTicks; rx.host_idle_ns = kResidentHostIdleNs; rx.host_life_ns = kResidentHostLifeNs;
    if (const char* v = std::getenv("RQ_RESIDENT_IDLE_TICKS")) rx.idle_ticks = std::strtoull(v, nullptr, 10);      // (tests)
    if (const char* v = std::getenv("RQ_RESIDENT_LIFE_TICKS")) rx.life_ticks = std::strtoull(v, nullptr, 10);
    if (const char* v = std::getenv("RQ_RESIDENT_HOST_IDLE_NS")) rx.host_idle_ns = std::strtoull(v, nullptr, 10);
    if (const char* v = std::getenv("RQ_RESIDENT_HOST_LIFE_NS")) rx.host_life_ns = std::strtoull(v, nullptr, 10);
    // the stream and command memory now, not inside somebody's loop: creating a second stream costs ~8 ms (a hardware queue of its
    // own); a failure here is not the device's - the executor tries again when it first wants them
    if (rx.enabled && ensure_memory(dev) != RQ_OK) (void)hipGetLastError();
}

void resident_teardown(rq_device* dev) {
    (void)resident_retire(dev);
    if (dev->resident.stream) (void)hipStreamDestroy(dev->resident.stream);
}

bool resident_left(const rq_device* dev) { return __atomic_load_n(&dev->resident.mem[kRwExited], __ATOMIC_ACQUIRE) == dev->resident.launch_id; }

// ---- lifecycle --------------------------------------------------------------------------------------------------------------------
// the resident kernel has left (told to, idle for too long, or never started properly): take note, and if the command posted last
// was not consumed, run it as launches - nothing will ever publish its sequence numbers otherwise
int resident_gone(rq_device* dev) {
    ResidentExecutor& rx = dev->resident;
    if (!rx.running) return RQ_OK;
    rx.running = false;
    // A kernel that has published `exited` has nothing left to do but end (its stores were fenced before that word): whatever follows
    // may go ahead - the next resident kernel queues behind it on the executor's stream by itself - and a restart does not pay for a
    // stream synchronize (~10 us of completion signalling, once per ~100 iterations of the loop).  Otherwise (the stream was found
    // drained, or failed) the synchronize returns at once or reports the error.
    if (!resident_left(dev)) RQ_HIP(hipStreamSynchronize(rx.stream));
    // was it worth its launch?  A kernel that idled out after a handful of commands was not (see kResidentMinCommands): back off.
    const uint64_t served = rx.posts - rx.posts_at_start;
    const uint32_t why = __atomic_load_n(&rx.mem[kRwWhy], __ATOMIC_ACQUIRE);
    if (served >= kResidentGoodCommands) {
        rx.backoff = 0;
    } else if ((why & rq::kRbLeftIdle) && served < kResidentMinCommands) {
        rx.backoff = rx.backoff ? std::min(2 * rx.backoff, kResidentMaxBackoff) : kResidentMinCommands;
        rx.backoff_left = rx.backoff;
    }
    if (rx.pending) {
        rx.pending = false;
        const uint32_t f = __atomic_load_n(dev->mailbox.flag.get(), __ATOMIC_ACQUIRE);
        if ((int32_t)(f - rx.pending_last) < 0) {
            RQ_REQUIRE((int32_t)(f - rx.pending_first) < 0, RQ_ERR_HIP, "the resident executor left in the middle of a command");
            ++rx.replays;
            if (rx.bound.policy_kind) RQ_HIP(rq::launch_actor_step(dev->stream, rx.last.policy));
            else                      RQ_HIP(launch_step_pair(dev, rx.last.step));
        }
    }
    return RQ_OK;
}

// wait until the command posted last has been consumed (its first sequence number published) or the kernel has left
int resident_drain(rq_device* dev) {
    ResidentExecutor& rx = dev->resident;
    if (!rx.running || !rx.pending) return RQ_OK;
    const int rc = mailbox_wait(dev, rx.pending_first);
    if (rc == RQ_OK && rx.running) rx.pending = false;
    return rc;
}

// The command line is written as four 16-byte stores, the quarter that holds `head` last: device memory behind the BAR is mapped
// uncached or write-combining, where every store is a transaction of its own (forty 4-byte stores cost rq_step 0.5 us) and, write-
// combining, may leave in any order until a store fence.  A reader that finds head == tail == id has the whole line - and the rows,
// which were written (one 16-byte store per env) before it.
static void write_line(ResidentExecutor& rx, uint32_t bits, const float* state_in, float* state_out, uint32_t seq_step, uint32_t seq_spec,
                       uint32_t checksum) {
    const uint32_t id = ++rx.packet;
    const uint64_t a = reinterpret_cast<uint64_t>(state_in), b = reinterpret_cast<uint64_t>(state_out);
    alignas(16) uint32_t line[16] = {};
    line[rq::kRpHead] = id; line[rq::kRpBits] = bits;
    line[rq::kRpStateInLo] = (uint32_t)a; line[rq::kRpStateInHi] = (uint32_t)(a >> 32);
    line[rq::kRpStateOutLo] = (uint32_t)b; line[rq::kRpStateOutHi] = (uint32_t)(b >> 32);
    line[rq::kRpSeqStep] = seq_step; line[rq::kRpSeqSpec] = seq_spec; line[rq::kRpChecksum] = checksum;
    line[rq::kRpTail] = id;
    __m128i* dst = reinterpret_cast<__m128i*>(rx.cmd + kRwLine);
    const __m128i* src = reinterpret_cast<const __m128i*>(line);
    _mm_store_si128(dst + 1, _mm_load_si128(src + 1));
    _mm_store_si128(dst + 2, _mm_load_si128(src + 2));
    _mm_store_si128(dst + 3, _mm_load_si128(src + 3));
    _mm_sfence();
    _mm_store_si128(dst + 0, _mm_load_si128(src + 0));
    _mm_sfence();
}

// tell the kernel to leave and wait until it has
int resident_retire(rq_device* dev) {
    ResidentExecutor& rx = dev->resident;
    if (!rx.running) return RQ_OK;
    int rc = resident_drain(dev); if (rc) return rc;
    if (!rx.running) return RQ_OK;                         // it left by itself meanwhile (resident_gone has dealt with it)
    write_line(rx, rq::kRbQuit, nullptr, nullptr, 0, 0, 0);
    for (uint64_t spins = 1;; ++spins) {
        if (resident_left(dev)) break;
        if ((spins & 0xFFFFu) == 0 && hipStreamQuery(rx.stream) != hipErrorNotReady) break;
        __builtin_ia32_pause();
    }
    return resident_gone(dev);
}

// ---- admission, start, post -------------------------------------------------------------------------------------------------------
static bool in_pair(float* const pair[2], const float* p) { return p == pair[0] || p == pair[1]; }

// may a call with binding `c` post to the kernel started for `k`?
static bool binds(const ResidentBinding& k, const ResidentBinding& c) {
    return k.policy_kind == c.policy_kind && k.env == c.env && k.env_uid == c.env_uid && k.params == c.params &&
           k.params_version == c.params_version && k.pol == c.pol && k.packed == c.packed && k.batch == c.batch && k.seed == c.seed &&
           std::memcmp(&k.cfg, &c.cfg, sizeof(rq_env_config)) == 0 && in_pair(k.obs, c.obs[1]) && in_pair(k.hidden, c.hidden[0]);
}

// Admission of a call of either kind (ready: a resident kernel could serve it, bound to `want`): a running kernel it cannot use - bound to
// something else, not fed for host_idle_ns, host_life_ns old - is retired.  -> *use: the call goes to the executor.
int resident_admit(rq_device* dev, bool ready, const ResidentBinding& want, uint64_t now_ns, uint32_t streak, bool* use) {
    ResidentExecutor& rx = dev->resident;
    const bool bound = ready && rx.running && binds(rx.bound, want) && now_ns - rx.last_post_ns < rx.host_idle_ns &&
                       now_ns - rx.born_ns < rx.host_life_ns;
    if (rx.running && !bound) { const int rc = resident_retire(dev); if (rc) return rc; }
    *use = ready && (bound || streak >= kResidentStreak);
    if (*use && !rx.running && rx.backoff_left) { --rx.backoff_left; *use = false; }     // see kResidentMinCommands
    return RQ_OK;
}

// Start a kernel of want's kind (none is running) on ra: the caller's objects as its kernel reads them; the pairs and the operand image
// are the binding's, the rows and flag the mailbox's, the rest the executor's.  A failed launch is no error: the caller launches.
int resident_start(rq_device* dev, rq::ResidentArgs& ra, const ResidentBinding& want) {
    ResidentExecutor& rx = dev->resident;
    int rc = ensure_memory(dev); if (rc) return rc;
    // nothing of the stream's may still be in flight when a kernel outside it starts reading the same buffers
    RQ_HIP(hipStreamSynchronize(dev->stream));
    mailbox_resident_args(dev, ra, want.policy_kind);
    ra.obs_buf[0] = want.obs[0]; ra.obs_buf[1] = want.obs[1]; ra.hidden[0] = want.hidden[0]; ra.hidden[1] = want.hidden[1]; ra.packed = want.packed;
    ra.packet = rx.cmd + kRwLine; ra.exited = rx.mem + kRwExited; ra.small_rows = rx.cmd + kRwRows;
    if (rx.cmd_on_device) ra.rows_action = reinterpret_cast<const float*>(rx.cmd + kRwRows);     // the rows beside the line
    ra.timing = rx.timing ? reinterpret_cast<unsigned long long*>(rx.mem + kRwTiming) : nullptr;
    ra.launch_id = ++rx.launch_id; if (ra.launch_id == 0) ra.launch_id = ++rx.launch_id;
    ra.first_packet = rx.packet + 1;
    ra.idle_ticks = rx.idle_ticks; ra.life_ticks = rx.life_ticks;
    const hipError_t e = want.policy_kind ? rq::launch_resident_policy(rx.stream, ra) : rq::launch_resident(rx.stream, ra);
    if (e != hipSuccess) { (void)hipGetLastError(); return RQ_OK; }
    rx.running = true; ++rx.starts; rx.born_ns = host_now_ns(); rx.posts_at_start = rx.posts; rx.bound = want;
    return RQ_OK;
}

// one command slot: the caller has drained the previous command; this one's rows are in command memory
static void post(ResidentExecutor& rx, uint32_t bits, const float* state_in, float* state_out, uint32_t seq_step, uint32_t seq_spec,
                 uint32_t checksum, uint32_t seq_first) {
    rx.pending = true; rx.pending_first = seq_first; rx.pending_last = seq_spec;
    write_line(rx, bits, state_in, state_out, seq_step, seq_spec, checksum);
    rx.last_post_ns = host_now_ns(); ++rx.posts;
}

// what the kernel verifies a command's rows (n x dim floats at `stride`; the ones its mailbox reads) against: the uint32 sum of their dwords
static uint32_t checksum(const float* rows, uint32_t n, uint32_t dim, uint32_t stride) {
    uint32_t sum = 0, u;
    for (uint32_t i = 0; i < n; ++i) for (uint32_t k = 0; k < dim; ++k) { std::memcpy(&u, rows + (size_t)i * stride + k, 4); sum += u; }
    return sum;
}

// the loop's actions, n x 4 dwords, beside the line where the small kernel reads them in the same load; in device memory all kernels do
void resident_post(rq_device* dev, const StepPair& p) {
    ResidentExecutor& rx = dev->resident;
    const rq::EnvStepLaunch& e = p.step;
    const float* a = e.mb.rows_in;
    if (e.b.n <= rq::kResidentSmallEnvs || rx.cmd_on_device) {
        __m128i* rows = reinterpret_cast<__m128i*>(rx.cmd + kRwRows);
        for (uint32_t k = 0; k < e.b.n; ++k) _mm_store_si128(rows + k, _mm_loadu_si128(reinterpret_cast<const __m128i*>(a) + k));
    }
    rx.last.step = p;
    const uint32_t bits = (e.obs_of_next == rx.bound.obs[1] ? rq::kRbObsSel : 0u) | (p.actor.hidden_in == rx.bound.hidden[1] ? rq::kRbHiddenSel : 0u);
    post(rx, bits, e.state, e.next_state, e.mb.seq, p.actor.mb.seq, checksum(a, e.b.n, RQ_ACTION_DIM, RQ_ACTION_DIM), e.mb.seq);
}

// the policy's observation rows, each padded to kResidentPolicyRow floats: whole 16-byte stores
void resident_post(rq_device* dev, const PolicyCmd& p) {
    ResidentExecutor& rx = dev->resident;
    __m128i* rows = reinterpret_cast<__m128i*>(rx.cmd + kRwRows);
    for (uint32_t i = 0; i < p.n; ++i) {
        alignas(16) float row[rq::kResidentPolicyRow] = {};
        std::memcpy(row, p.mb.rows_in + (size_t)i * p.mb.in_stride, RQ_POLICY_INPUT_DIM * sizeof(float));
        for (uint32_t k = 0; k < rq::kResidentPolicyRow / 4; ++k)
            _mm_store_si128(rows + (size_t)i * (rq::kResidentPolicyRow / 4) + k, _mm_load_si128(reinterpret_cast<const __m128i*>(row) + k));
    }
    rx.last.policy = p;
    post(rx, 0u, nullptr, nullptr, 0u, p.mb.seq, checksum(p.mb.rows_in, p.n, RQ_POLICY_INPUT_DIM, p.mb.in_stride), p.mb.seq);
}

}  // namespace rqh

using namespace rqh;

uint32_t ResidentStreak::follow(bool eligible, uint64_t now_ns, const void* call_who, uint64_t call_key) {
    if (!eligible) return 0;
    const uint32_t len = now_ns - last_ns < kResidentMaxGapNs && who == call_who && key == call_key ? n + 1 : 1;
    last_ns = now_ns; who = call_who; key = call_key;
    return len;
}

int rq::resident_scope_hook(const rq_device* dev_) {
    rq_device* dev = const_cast<rq_device*>(dev_);
    dev->resident.loop_streak.n = 0; dev->resident.policy_streak.n = 0;
    return dev->resident.running ? resident_retire(dev) : RQ_OK;
}

extern "C" {

RQ_API int rq_device_set_resident(rq_device* dev, int enable) {
    RQ_REQUIRE(dev, RQ_ERR_INVALID_ARGUMENT, "null argument");
    DeviceScope on_device(dev); int rc = on_device.rc; if (rc) return rc;      // retires a running one
    dev->resident.enabled = enable != 0;
    dev->resident.backoff = dev->resident.backoff_left = 0;
    return RQ_OK;
}

RQ_API int rq_device_get_resident(const rq_device* dev, int* enabled, int* running, uint64_t* starts, uint64_t* commands, uint64_t* replays) {
    RQ_REQUIRE(dev, RQ_ERR_INVALID_ARGUMENT, "null argument");
    const ResidentExecutor& rx = dev->resident;
    if (enabled) *enabled = rx.enabled ? 1 : 0;
    if (running) *running = rx.running && !resident_left(dev) ? 1 : 0;
    if (starts) *starts = rx.starts;
    if (commands) *commands = rx.posts;
    if (replays) *replays = rx.replays;
    return RQ_OK;
}

RQ_API int rq_device_get_resident_timing(const rq_device* dev, uint64_t* ticks6) {
    RQ_REQUIRE(dev && ticks6, RQ_ERR_INVALID_ARGUMENT, "null argument");
    RQ_REQUIRE(!dev->resident.mem.empty(), RQ_ERR_NOT_INITIALIZED, "no resident executor has run on this device");
    std::memcpy(ticks6, dev->resident.mem + kRwTiming, 6 * sizeof(uint64_t));
    return RQ_OK;
}

}  // extern "C"
