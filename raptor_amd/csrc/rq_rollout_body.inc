// rq_rollout_body.inc - the body of the fused rollout kernel, included once per entry point: k_rollout_fused, k_rollout_fused_track
// and k_rollout_fused_rate (rq_rollout.hpp), the bank's two (rq_kernels.hip) and the schedules' five (rq_rollout_schedule.inc).  Text,
// not a function: the untracked kernel is compiled from
// exactly what it was compiled from when the body stood between its braces - its listing does not move when the tracked variant
// changes - and a __device__ function in between does cost that (the work-group-size folds of a kernel are made before inlining).
// In scope at the point of inclusion: the template parameters NOISE, AUTORESET, RECORD, ACTOR, the names b, c, nc, sc, seed, epoch0,
// n_steps, params, state, hidden, w, packed, st, traj, span - and what the entry point says it takes, by a #define in front of the
// #include (all of them are #undef'd at the end of this file):
//   RQ_FUSED_TAKES_SAS      SAS and sas: the SampleAndSquash output stage
//   RQ_FUSED_TAKES_TRACK    TRACK and trk: a moving setpoint
//   RQ_FUSED_TAKES_RATE     interval: the policy's native interval - RATE is then true
//   RQ_FUSED_TAKES_WRENCH   wr: the env carries a wrench schedule - WRENCH is then true; likewise _VEHICLE and vh, _WIND and wd, _DELAY
//                           and dl, _SENSOR and sn (the entry points of rq_rollout_schedule.inc, one each)
// What an entry point does not take is declared here, once: the switch false, the argument empty, the interval 1 - all constexpr.
#ifndef RQ_FUSED_TAKES_SAS
    constexpr bool SAS = false;
    constexpr SasArgs sas{};
#endif
#ifndef RQ_FUSED_TAKES_TRACK
    constexpr bool TRACK = false;
    constexpr TrackPtrs trk{};
#endif
#ifdef RQ_FUSED_TAKES_RATE
    constexpr bool RATE = true;
#else
    constexpr bool RATE = false;
    constexpr uint32_t interval = 1;
#endif
#ifdef RQ_FUSED_TAKES_WRENCH
    constexpr bool WRENCH = true;
#else
    constexpr bool WRENCH = false;
    constexpr WrenchPtrs wr{};
#endif
#ifdef RQ_FUSED_TAKES_VEHICLE
    constexpr bool VEHICLE = true;
#else
    constexpr bool VEHICLE = false;
    constexpr VehiclePtrs vh{};
#endif
#ifdef RQ_FUSED_TAKES_WIND
    constexpr bool WIND = true;
#else
    constexpr bool WIND = false;
    constexpr WindPtrs wd{};
#endif
#ifdef RQ_FUSED_TAKES_DELAY
    constexpr bool DELAY = true;
#else
    constexpr bool DELAY = false;
    constexpr DelayPtrs dl{};
#endif
#ifdef RQ_FUSED_TAKES_SENSOR
    constexpr bool SENSOR = true;
#else
    constexpr bool SENSOR = false;
    constexpr SensorPtrs sn{};
#endif
    // kernel-level timing (rq_device_set_rollout_timing): every wave leaves the wall-clock ticks (constant rate) at which it
    // came in and went out, and its XCD: the eight dies' counters are offset against one another by microseconds, one die's
    // are consistent - the host takes first-in / last-out per die
    // (one record per wave, no atomics: 128 waves of a die updating one word cost the launch 8 us)
    unsigned long long t_in = 0;
    if (span != nullptr) t_in = (unsigned long long)wall_clock64();
    const uint32_t i0 = env_index();
    const uint32_t wave_base = i0 & ~63u;
    const uint32_t i = i0 < b.n ? i0 : b.n - 1;
    const bool valid = i0 < b.n;
    const size_t ld = b.ld;
    const uint64_t genv = b.env_offset + i;
    // what the ahead-of-time sampler needs is asked for first: it runs while the rest of the prologue's loads are in flight
    uint32_t ep = AUTORESET ? st.episode[i] : 0u;
    float hover_rpm = 0.0f;
    if (AUTORESET) hover_rpm = field(params, RQ_P_HOVER_RPM, ld)[i];
    const EnvConsts k = make_consts([&](int f) { return field(params, f, ld)[i]; });
    QuadState y;
    f32x2 LA01, LA23;
    float f6[6], hQ[4][4];
    y.load([&](int j) { return field(state, j, ld)[i]; });
    LA01 = f32x2{field(state, (RQ_S_LAST_ACTION + 0), ld)[i], field(state, (RQ_S_LAST_ACTION + 1), ld)[i]};
    LA23 = f32x2{field(state, (RQ_S_LAST_ACTION + 2), ld)[i], field(state, (RQ_S_LAST_ACTION + 3), ld)[i]};
#pragma unroll
    for (int j = 0; j < 6; ++j) f6[j] = field(state, (RQ_S_FORCE + j), ld)[i];
    load_hidden_q(hidden, ld, wave_base, b.n, hQ);
    // the running episode's return and length ride in registers; a FINISHED episode's record goes straight to memory when
    // it ends (below): four values less to carry through the loop, five instructions less per step
    float ep_ret = st.returns[i];
    uint32_t ep_steps = st.steps[i];
    float last_r = st.last_reward[i];
    // tracked rollouts: the env's running sum of |p - p_ref|^2 and the steps it covers (rq_env_get_tracking_error)
    float trk_sq = 0.0f;
    uint32_t trk_n = 0;
    // (a reference bank: the first row of the env's own table, loaded once per launch and carried in one register)
    [[maybe_unused]] uint32_t trk_row0 = 0;
    if constexpr (TRACK) {
        trk_sq = trk.sq[i]; trk_n = trk.steps[i];
        if (trk.row0_at != 0) trk_row0 = trk.steps[(size_t)trk.row0_at + i];       // wave-uniform test (kernel argument)
    }
    // RATE (rq_policy_set_native_interval): the env's episode step count modulo the native interval - the launch's only division.
    // The hidden state moves on at the steps where it is 0; at the others the policy acts from the last committed state.
    [[maybe_unused]] uint32_t phase = 0;
    if constexpr (RATE) phase = ep_steps % interval;
    // WRENCH: the two scales (from the params of this call) and the first row of the env's own table, once per launch
    [[maybe_unused]] float wr_fs = 1.0f, wr_ts = 1.0f;
    [[maybe_unused]] uint32_t wr_row0 = 0;
    if constexpr (WRENCH) {
        wrench_scales(wr.relative, field(params, RQ_P_MASS, ld)[i], c.gravity, field(params, RQ_P_ROTOR_POS, ld)[i],
                      field(params, (RQ_P_ROTOR_POS + 1), ld)[i], wr_fs, wr_ts);
        wr_row0 = wr.row0[i];
    }
    // VEHICLE: the nine base fields the schedule scales stay live through the loop (the other builds let them die after make_consts),
    // and the first row of the env's own table, once per launch
    [[maybe_unused]] VehicleBase vh_base{};
    [[maybe_unused]] uint32_t vh_row0 = 0;
    if constexpr (VEHICLE) {
        vh_base = vehicle_base([&](int f) { return field(params, f, ld)[i]; });
        vh_row0 = vh.row0[i];
    }
    // WIND: the mass (from the params of this call) and the first row of the env's own table, once per launch
    [[maybe_unused]] float wd_mass = 0.0f;
    [[maybe_unused]] uint32_t wd_row0 = 0;
    if constexpr (WIND) {
        wd_mass = field(params, RQ_P_MASS, ld)[i];
        wd_row0 = wd.row0[i];
    }
    // DELAY: the first row of the env's own table, once per launch
    [[maybe_unused]] uint32_t dl_row0 = 0;
    if constexpr (DELAY) dl_row0 = dl.row0[i];
    // SENSOR: likewise
    [[maybe_unused]] uint32_t sn_row0 = 0;
    if constexpr (SENSOR) sn_row0 = sn.row0[i];
    const uint8_t last_t_raw = st.last_terminated[i];
    uint8_t last_d = AUTORESET ? (uint8_t)0 : st.last_done[i];       // auto-reset: rebuilt in the epilogue
    const uint8_t frozen_raw = st.frozen[i];
    // the operand image (L2-resident after a die's first wave) is asked for AFTER the env's own fields: those come from
    // HBM / the memory-side cache and their latency is the long one
    ACTOR actor;
    actor.template load_issue<kFusedBlock / 64>(packed);
    // (kAhead, pre, pre_mask: see "sampled AHEAD" below)
    constexpr bool kAhead = AUTORESET && (WavesPerSimd<ACTOR>::value == 1 || WavesPerSimd<ACTOR>::bf16);
    constexpr int kPre = 19;
    float pre[kPre];
    uint64_t pre_mask = 0;                       // wave-uniform
    if (kAhead) {
        // Every launch STARTS with valid parked values (round 4, second half): the sampler runs here, inline, for all 64
        // lanes, while the prologue's ~90 load instructions are in flight - its inputs were asked for first, and it sits
        // between the request for the operand image and the image's move into its registers (a CALL would wait for every
        // outstanding load; so would anything placed behind actor.park()).  Before, a launch began with nothing parked and
        // the wave that met the launch's first episode end sampled there and then: 1.9 us that the other 1 023 waves of a
        // 65 536-env launch waited for at its end (tools/wave_timeline.py: the slowest wave's steps 2.4 us longer than the
        // median wave's in a 20-step launch; now 0.9, for 1.2 us more prologue in every wave: 20-step regions 77.24 ->
        // 76.66 us on one box, three alternations).
        float s0[17], la0[4], f0[6];
        sample_state(sc, seed, ep, genv, field(params, RQ_P_MASS, ld)[i], hover_rpm, field(params, RQ_P_ROTOR_POS, ld)[i],
                     field(params, (RQ_P_ROTOR_POS + 1), ld)[i], s0, la0, f0);
#pragma unroll
        for (int j = 0; j < 13; ++j) asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(pre[j]) : "v"(s0[j]));
#pragma unroll
        for (int j = 0; j < 6; ++j) asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(pre[13 + j]) : "v"(f0[j]));
        pre_mask = ~0ull;
    }
    actor.park();
    float h0Q[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) h0Q[t][r] = actor.h0(r);
    // looked at only now (the empty asm keeps the compares from drifting up between the image's loads, where they
    // made those wait for every load before them)
    uint32_t last_t_bits = last_t_raw, frozen_bits = frozen_raw;
    asm volatile("" : "+v"(last_t_bits), "+v"(frozen_bits));
    bool last_t = last_t_bits != 0;
    const bool was_frozen = frozen_bits != 0;
    // The next episode's initial state, sampled AHEAD of the episode end (round 3).  sample_initial_state of an env depends
    // on (seed, episode counter, global env id, a few parameters) and on nothing the running episode computes, so it need
    // not wait for the end: the 19 values that are not constants (position .. angular velocity, the disturbance) are kept
    // in ACCUMULATION registers for every lane, and an env whose episode ends takes them with 19 register reads.  The
    // sampler itself (six Philox blocks, sin / cos, Box-Muller: ~1 000 instructions, and at an episode end it used to run
    // for the one or two lanes concerned while the other 62 waited - the slowest wave of a 20-step launch paid it three
    // times, tools/wave_timeline.py) runs for ALL 64 lanes at once: in the prologue of every launch (above, under the
    // prologue's loads) and again only when an ending env finds its values used up - its second end since the last
    // sampling: `pre_mask` has a bit per lane whose parked values are for its current episode counter.  Lanes that still
    // hold valid ones get the same values again (same counter, same function), so the refill is unconditional.
    // Only the builds with one wave per SIMD do this: the two-waves-per-SIMD builds have 256 registers per wave in all,
    // every one of them an architected register; asking for accumulation registers splits that budget 128 + 128 and the
    // hot loop spills (262 144 envs: 0.70 -> 0.55 of the peak).  There the second wave fills the time one spends sampling.
    // (The two-wave bf16 build has the room: 6.45 -> 5.7 us per step of 262 144 envs with it.)
    // the env index as the rare paths see it: opaque, so that the addresses they form are computed there and then instead of
    // being kept through the loop (see the epilogue)
    auto rare_index = [&]() { uint32_t r = i; asm volatile("" : "+v"(r)); return r; };
    auto refill = [&]() {                        // every lane: sample_initial_state for its episode counter ep
        const uint32_t ir = rare_index();
        const PreSample fresh = sample_state_ahead(sc, seed, ep, genv, field(params, RQ_P_MASS, ld)[ir], hover_rpm,
                                                   field(params, RQ_P_ROTOR_POS, ld)[ir], field(params, (RQ_P_ROTOR_POS + 1), ld)[ir]);
#pragma unroll
        for (int j = 0; j < kPre; ++j) asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(pre[j]) : "v"(fresh[j]));
        pre_mask = ~0ull;
    };
    auto take_presampled = [&]() {               // this lane's env starts its next episode (its parked values are valid)
        float fr[kPre];
        if constexpr (kAhead) {
#pragma unroll
            for (int j = 0; j < kPre; ++j) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(fr[j]) : "a"(pre[j]));
        } else {                                 // sampled here and now, for the lanes whose episode ended
            const PreSample fresh = sample_state_ahead(sc, seed, ep, genv, field(params, RQ_P_MASS, ld)[i], hover_rpm,
                                                       field(params, RQ_P_ROTOR_POS, ld)[i],
                                                       field(params, (RQ_P_ROTOR_POS + 1), ld)[i]);
#pragma unroll
            for (int j = 0; j < kPre; ++j) fr[j] = fresh[j];
        }
        y.load([&](int j) { return j < 13 ? fr[j] : hover_rpm; });
        LA01 = f32x2{0.0f, 0.0f}; LA23 = f32x2{0.0f, 0.0f};       // sample_state: last action 0, rotors at hover
#pragma unroll
        for (int j = 0; j < 6; ++j) f6[j] = fr[13 + j];
        if (valid) {                                 // the new episode's disturbance: written now, not carried to the end
            const uint32_t ir = rare_index();
#pragma unroll
            for (int j = 0; j < 6; ++j) field(state, (RQ_S_FORCE + j), ld)[ir] = fr[13 + j];
        }
        ep += 1;
    };
    if (AUTORESET) {
        // An env left frozen by an earlier rollout WITHOUT auto-reset (its episode is over) starts its next
        // episode here, as every episode end under auto-reset does: re-sampled, policy state reset.  The
        // chained mode does the same before its first step (k_thaw_frozen).
        const uint64_t thaw = __builtin_amdgcn_ballot_w64(was_frozen);
        if (thaw != 0) {                             // (kAhead: the prologue parked the values they take)
            if (was_frozen) take_presampled();
            pre_mask &= ~thaw;
            select_hidden_q(thaw, h0Q, hQ);
        }
    }
    typename ACTOR::Carry carry;          // what the actor carries from one step into the next (ActorF32T::Carry)
    actor.prime(hQ, carry);
    Disturbance ds = make_disturbance(k, c.gravity, f6);
    bool frozen = AUTORESET ? false : was_frozen;
    uint32_t last_step = n_steps;                      // without auto-reset: the last step of this launch the env took
    // wave-uniform: no env of this wave distinguishes rotor spin-up from spin-down (see dynamics<SYM_TAU>)
    // (VEHICLE: decided from the base time constants, so that it holds for every row - equal inputs times one factor are equal, and
    // so are their reciprocals; a comparison of reciprocals could be broken by one row)
    const bool sym_tau = VEHICLE ? __builtin_amdgcn_ballot_w64(vh_base.tau_rise != vh_base.tau_fall) == 0
                                 : __builtin_amdgcn_ballot_w64(k.itr != k.itf) == 0;

    // The loop exists twice, once per dynamics variant (round 3): with the wave-uniform choice inside the loop the two
    // variants met in a join that cost the state's registers a copy per step (~8 moves) plus the branch itself.
    auto rollout_loop = [&](auto sym_choice) {
    constexpr bool SYM = decltype(sym_choice)::value;
    for (uint32_t t = 0; t < n_steps; ++t) {
        const uint64_t live = AUTORESET ? ~0ull : __builtin_amdgcn_ballot_w64(!frozen);
        if (!AUTORESET && live == 0) break;   // wave-uniform exit: every env of the wave is frozen
        float o[22], a[4];
        // WRENCH: this step's row of the env's own table (lanes are at different rows: per-lane loads of a table that stays in the
        // cache), asked for here so that the actor's MFMA batches cover the latency; it is consumed just before the env step
        [[maybe_unused]] float wr_row[6];
        if constexpr (WRENCH) wrench_row(wr.rows, wr.n_rows, wr_row0, ep_steps, wr_row);
        // VEHICLE: likewise this step's 16-byte row of factors, one load; it is consumed just before the env step
        [[maybe_unused]] float vh_row[4];
        if constexpr (VEHICLE) vehicle_row(vh.rows, vh.n_rows, vh_row0, ep_steps, vh_row);
        // WIND: likewise this step's 16-byte row of air velocity and drag, one load; it is consumed just before the env step
        [[maybe_unused]] float wd_row[4];
        if constexpr (WIND) wind_row(wd.rows, wd.n_rows, wd_row0, ep_steps, wd_row);
        // DELAY: likewise this step's byte of delay and, out of the env's command history, the command given that many steps ago
        // (four loads behind the byte; lanes at one episode age read one slot: coalesced); consumed just before the env step
        [[maybe_unused]] uint32_t dl_d = 0;
        [[maybe_unused]] float dl_u[4];
        if constexpr (DELAY) {
            dl_d = delay_row(dl.rows, dl.n_rows, dl_row0, ep_steps);
            delay_read(dl.ring, ld, i, ep_steps, dl_d, dl_u);
        }
        // SENSOR: this step's byte of delay, clamped to the episode's age, and out of the env's readings the 18 floats of the
        // reading taken that many steps ago (lanes at one episode age read one slot: coalesced); skipped when no lane of the wave
        // is behind (wave-uniform); consumed behind observe_head
        [[maybe_unused]] uint32_t sn_d = 0;
        [[maybe_unused]] bool sn_behind = false;
        [[maybe_unused]] float sn_z[kSensorFields];
        if constexpr (SENSOR) {
            sn_d = sensor_row(sn.rows, sn.n_rows, sn_row0, ep_steps);
            sn_behind = __builtin_amdgcn_ballot_w64(sn_d != 0) != 0;
            if (sn_behind) {
#pragma unroll
                for (uint32_t j = 0; j < kSensorFields; ++j) sn_z[j] = 0.0f;
                sensor_read(sn.ring, ld, i, ep_steps, sn_d, sn_z);
            }
        }
        observe_head<NOISE>(y, LA01, LA23, nc, seed, epoch0 + t, genv, o);
        if constexpr (SENSOR) {      // the reading of this step goes into the ring where the env is inside the batch - not a lane past it
            // shadowing env n - 1 - and not frozen; the policy, the setpoint's shift and a recording see the old one
            if (valid && (AUTORESET || !frozen)) sensor_write(sn.ring, ld, i, ep_steps, o);
            if (sn_behind) {
#pragma unroll
                for (uint32_t j = 0; j < kSensorFields; ++j) o[j] = sn_d != 0 ? sn_z[j] : o[j];
            }
        }
        if constexpr (TRACK) {
            // the setpoint of this step: the row of the env's own episode step count (lanes are at different rows: per-lane
            // loads of a table that stays in the cache), taken off what the policy sees; the error on the true position
            float tr[6];
            track_row(trk.ref, trk.rows, trk_row0, ep_steps, tr);
            track_shift(tr, o);
            if (AUTORESET || !frozen) { trk_sq = track_accumulate(trk_sq, y.P01[0], y.P01[1], y.p2, tr); trk_n += 1; }
        }
        float hn[4][4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) hn[tt][r] = hQ[tt][r];
        // RATE: the envs at a native step, and what the actor carries for the others (it is theirs again after the step)
        [[maybe_unused]] uint64_t native = ~0ull;
        [[maybe_unused]] typename ACTOR::Saved held{};
        if constexpr (RATE) {
            native = __builtin_amdgcn_ballot_w64(phase == 0);
            held = actor.carry_of(carry);
        }
        // Trajectory stores (RECORD): one coalesced 256-byte store per field per wave; buffer stores: resource = this
        // step's block of the trajectory (base moved on the SALU), scalar offset = field row, vector offset = the
        // lane's env - no per-lane 64-bit address arithmetic, no per-lane pointers kept alive across the loop; lanes
        // past the batch are sent out of range (the hardware drops out-of-range buffer stores).  The 22 observation
        // stores are handed to the actor, which places them between the MFMAs of its first GRU pass; the action
        // follows the actor, reward and done code the env step.
        const uint32_t row = (uint32_t)ld * 4u;                     // bytes per field row (ld < 2^30)
        const uint32_t lane_off = valid ? i * 4u : 0xFFFFFFFFu;
        if (RECORD) {
            const size_t tt = traj.t0 + t;
            const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(traj.obs + tt * 22 * ld, 0, 22u * row, 0x00020000);
            actor.template step_fused<22>(o, hn, a, carry, [&] {
#pragma unroll
                for (int j = 0; j < 22; ++j)
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, o[j]), ro, lane_off, (uint32_t)j * row, kNtTrajAux);
            });
        } else {
            actor.template step_fused<0>(o, hn, a, carry, [] {});
        }
        if (SAS) sample_and_squash(sas, epoch0 + t, genv, hn, a);        // SampleAndSquash output stage (rare)
        if (RECORD) {
            const size_t tt = traj.t0 + t;
            const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(traj.act + tt * 4 * ld, 0, 4u * row, 0x00020000);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, a[j]), ra, lane_off, (uint32_t)j * row, kNtTrajAux);
        }
        if constexpr (RATE) {
            select_hidden_q(AUTORESET ? native : live & native, hn, hQ);      // a tentative step leaves the hidden state alone
            actor.hold_carry(~native, held, carry);
        } else if (AUTORESET) {
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) hQ[tt][r] = hn[tt][r];
        } else {
            select_hidden_q(live, hn, hQ);    // frozen envs keep their hidden state
        }
        // everything above belongs to the actor (MFMA results consumed, transposes done); the env step below
        // contains hand-placed packed instructions the compiler's hazard tracking does not see through
        // (round 4 measured the 16-bit builds without this barrier - the env step free to mix with their co-executing MFMAs:
        // no gain)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (WRENCH) {      // the wrench of this transition: the per-episode base (f6, which the state keeps) + the scaled row
            float w6[6];
            wrench_compose(f6, wr_fs, wr_ts, wr_row, w6);
            ds = make_disturbance(k, c.gravity, w6);
        }
        if constexpr (WIND) {        // the force of this transition: the per-episode base (f6, which the state keeps) + the drag against
            float w6[6];             // the air at y, the state before the step, held across the RK4 stages
#pragma unroll
            for (int j = 0; j < 6; ++j) w6[j] = f6[j];
            wind_compose(w6, wd_mass, y.V01[0], y.V01[1], y.VW[0], wd_row);
            ds = make_disturbance(k, c.gravity, w6);
        }
        if constexpr (DELAY) {       // a (the actor's command of this step, which the recording took above) goes into the history where
            // the step commits - not frozen, not a lane past the batch shadowing env n - 1 -; a delay of 0 acts on it as it stands
            if (valid && (AUTORESET || !frozen)) delay_write(dl.ring, ld, i, ep_steps, a);
            if (dl_d == 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) dl_u[j] = a[j];
            }
        }
        QuadState yn = y;
        f32x2 A01, A23;
        bool term;
        float r;
        if constexpr (DELAY) {       // the transition of the delayed command; the last-action columns keep the actor's own
            r = step_inplace<SYM>(c, k, ds, yn, dl_u, A01, A23, term);
            A01 = delay_history(a[0], a[1]); A23 = delay_history(a[2], a[3]);
        } else if constexpr (VEHICLE) {     // this transition's vehicle: the scheduled members of the constants rebuilt from the base fields
            EnvConsts kv = k;
            vehicle_consts(vh_base, vh_row, kv);
            ds = make_disturbance(kv, c.gravity, f6);
            r = step_inplace<SYM>(c, kv, ds, yn, a, A01, A23, term);
        } else {
            r = step_inplace<SYM>(c, k, ds, yn, a, A01, A23, term);
        }
        // the reward is wanted HERE: left to itself its arithmetic sinks below the episode-end block, which overwrites the
        // state it reads - and the state then lives twice, nine copies per step
        asm volatile("" :: "v"(r));
        bool ended = false;
        uint8_t done_code = 4;          // frozen: computed on a scratch copy, not committed
        if constexpr (AUTORESET) {
            // every env steps (auto-reset never freezes).  What an episode END needs - the finished episode's record, the
            // counters' reset, the next initial state - sits behind ONE wave-uniform test of the ballot further down
            // (round 4: as lane-wise selects and an exec-masked block it cost every step ~6 vector and ~8 scalar
            // instructions, the ballot itself was rebuilt from a 0 / 1 select); last_terminated / last_done are not
            // carried either: the epilogue reads them off the last step's termination mask and the step counter.
            y = yn;
            LA01 = A01; LA23 = A23;
            if (__builtin_expect(c.action_history_raw != 0, 0)) {      // wave-uniform (kernel argument)
                LA01 = f32x2{a[0], a[1]}; LA23 = f32x2{a[2], a[3]};
            }
            last_r = r; last_t = term;
            ep_ret += r;
            ep_steps += 1;
            if constexpr (RATE) { phase += 1; phase = phase >= interval ? 0u : phase; }
            // ONE compare whose result is the ballot (a termination counts as the limit reached): the ballot of an OR of
            // two lane masks is rebuilt by the compiler from a 0 / 1 select and a compare
            // (opaque, or the compiler turns the select + compare back into the OR)
            uint32_t reached = term ? 0xFFFFFFFFu : ep_steps;
            asm volatile("" : "+v"(reached));
            ended = reached >= c.episode_step_limit;
            if (RECORD) done_code = term ? 1 : (ended ? 2 : 0);
        } else if (!frozen) {           // commit
            y = yn;
            LA01 = A01; LA23 = A23;
            if (__builtin_expect(c.action_history_raw != 0, 0)) {      // wave-uniform (kernel argument)
                LA01 = f32x2{a[0], a[1]}; LA23 = f32x2{a[2], a[3]};
            }
            last_r = r; last_t = term;
            ep_ret += r;
            ep_steps += 1;
            if constexpr (RATE) { phase += 1; phase = phase >= interval ? 0u : phase; }
            ended = term || ep_steps >= c.episode_step_limit;
            done_code = term ? 1 : (ended ? 2 : 0);
            last_d = done_code;
            last_step = t;                             // (an env that froze earlier in the launch reports 4: see below)
            if (ended) {
                if (valid) {                           // lanes past the batch shadow env n - 1: they must not count twice
                    const uint32_t ir = rare_index();
                    st.fin_returns[ir] = ep_ret;
                    st.fin_lengths[ir] = ep_steps;
                    (void)__hip_atomic_fetch_add(&st.fin_counts[ir], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (term) (void)__hip_atomic_fetch_add(&st.fin_terminated[ir], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                ep_ret = 0.0f;
                ep_steps = 0;
                if constexpr (RATE) phase = 0;
                frozen = true;
            }
        }
        if (RECORD) {   // reward and done code of this transition (the observation and action went out above)
            const size_t tt = traj.t0 + t;
            const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(traj.rew + tt * ld, 0, row, 0x00020000);
            const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(traj.done + tt * ld, 0, (uint32_t)ld, 0x00020000);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, r), rr, valid ? i * 4u : 0xFFFFFFFFu, 0, kNtTrajAux);
            __builtin_amdgcn_raw_buffer_store_b8(done_code, rd, valid ? i : 0xFFFFFFFFu, 0, kNtTrajAux);
        }
        if (AUTORESET) {   // the envs whose episode ended: record, next initial state, h <- initial_hidden_state
            const uint64_t ended_mask = __builtin_amdgcn_ballot_w64(ended);
            if (ended_mask != 0) {
                if (ended) {
                    if (valid) {                           // lanes past the batch shadow env n - 1: they must not count twice
                        const uint32_t ir = rare_index();
                        st.fin_returns[ir] = ep_ret;
                        st.fin_lengths[ir] = ep_steps;
                        (void)__hip_atomic_fetch_add(&st.fin_counts[ir], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (term) (void)__hip_atomic_fetch_add(&st.fin_terminated[ir], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    ep_ret = 0.0f;
                    ep_steps = 0;
                    if constexpr (RATE) phase = 0;      // the first step of every episode is native
                }
                if constexpr (kAhead) {
                    if ((ended_mask & ~pre_mask) != 0) refill();      // wave-uniform; rare (see above)
                }
                if (ended) {
                    take_presampled();
                    ds = make_disturbance(k, c.gravity, f6);
                }
                pre_mask &= ~ended_mask;
                select_hidden_q(ended_mask, h0Q, hQ);
                actor.reset_carry(ended_mask, hQ, carry);
            }
        }
    }
    };
    // (the core-clock counter beside the constant-rate one: cycles over ticks is the clock the wave's steps really ran at)
    unsigned long long t_loop = 0, t_done = 0, c_loop = 0, c_done = 0;
    if (span != nullptr) { t_loop = (unsigned long long)wall_clock64(); c_loop = (unsigned long long)__builtin_readcyclecounter(); }
    if (sym_tau) rollout_loop(std::true_type{});
    else         rollout_loop(std::false_type{});
    if (span != nullptr) { c_done = (unsigned long long)__builtin_readcyclecounter(); t_done = (unsigned long long)wall_clock64(); }

    const bool commit = AUTORESET || !was_frozen;     // under auto-reset a frozen env was thawed above
    // an env whose episode ended BEFORE the launch's last step sat out the rest of it: its last transition of this rollout is
    // "not stepped" (4), as the chain of k_step launches reports it (found by the random-settings test, round 3)
    if (!AUTORESET && n_steps > 0 && last_step + 1 != n_steps) last_d = 4;
    // auto-reset: the last transition's done code from what the loop left behind - terminated, or ended by the step limit
    // (an episode end zeroes the step counter; n_steps > 0 in every launch), or neither
    if (AUTORESET) last_d = last_t ? 1 : (ep_steps == 0 ? 2 : 0);
    // The stores go to the addresses the prologue loaded from, and left alone the compiler keeps those ~55 64-bit
    // addresses alive through the whole loop - parked in accumulation registers: ~110 moves in, ~110 out, per launch.
    // An env index it cannot see through makes it compute them again here (55 adds).
    uint32_t ie = i;
    asm volatile("" : "+v"(ie));
    size_t lde = ld;                                  // likewise the field rows' scalar bases (they were kept in VGPR lanes)
    asm volatile("" : "+s"(lde));
    if (valid && commit) {
        y.store([&](int j, float v) { field(state, j, lde)[ie] = v; });
        field(state, (RQ_S_LAST_ACTION + 0), lde)[ie] = LA01[0]; field(state, (RQ_S_LAST_ACTION + 1), lde)[ie] = LA01[1];
        field(state, (RQ_S_LAST_ACTION + 2), lde)[ie] = LA23[0]; field(state, (RQ_S_LAST_ACTION + 3), lde)[ie] = LA23[1];
        st.returns[ie] = ep_ret;
        st.steps[ie] = ep_steps;
        st.last_reward[ie] = last_r;
        st.last_terminated[ie] = last_t ? 1 : 0;
        st.last_done[ie] = last_d;
        if constexpr (TRACK) { trk.sq[ie] = trk_sq; trk.steps[ie] = trk_n; }
        if (AUTORESET) {
            st.episode[ie] = ep;
            if (was_frozen) st.frozen[ie] = 0;
        }
        if (frozen) st.frozen[ie] = 1;
    }
    if (valid && !commit && n_steps > 0) st.last_done[ie] = 4;   // not stepped by this rollout (as k_step reports it)
    store_hidden_q(hidden, lde, wave_base, __builtin_amdgcn_ballot_w64(valid && commit), hQ);
    if (span != nullptr) {
        __builtin_amdgcn_s_waitcnt(0);                // the wave's stores have left
        if (threadIdx.x == 0) {
            const unsigned long long xcd = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u;        // HW_REG_XCC_ID[3:0]
            unsigned long long* rec = span + 4 * (size_t)blockIdx.x;
            rec[0] = t_in;
            rec[1] = ((unsigned long long)wall_clock64() & 0x0FFFFFFFFFFFFFFFull) | (xcd << 60);
            rec[2] = t_loop;          // prologue issued (its loads may still be in flight), first step about to start
            rec[3] = t_done;          // last step done, the epilogue's stores not yet issued
            span[4 * (size_t)gridDim.x + blockIdx.x] = c_done - c_loop;      // core-clock cycles between rec[2] and rec[3]
        }
    }
#undef RQ_FUSED_TAKES_SAS
#undef RQ_FUSED_TAKES_TRACK
#undef RQ_FUSED_TAKES_RATE
#undef RQ_FUSED_TAKES_WRENCH
#undef RQ_FUSED_TAKES_VEHICLE
#undef RQ_FUSED_TAKES_WIND
#undef RQ_FUSED_TAKES_DELAY
#undef RQ_FUSED_TAKES_SENSOR
