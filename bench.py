#!/usr/bin/env python3
"""Headline benchmark: env-steps/sec of the quadrotor rollout path on MI355X.

    python bench.py --gpus 1 --steps 10000 --warmup 5000
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A "step" is one pass of the hot path over the whole batch: observe -> Raptor.evaluate_step ->
step -> assign for every environment (README.md:96-99).  Workload = BASELINE.json configs[1]:
65 536 parallel quadrotors per GPU, fp32 RK4 dynamics + fp32 GRU actor, per-env domain-
randomised parameters, synthetic (seeded Philox) initial states, the shipped RAPTOR checkpoint
as the policy.  Auto-reset keeps every env stepping, so every counted env-step is a real one.
Multi-GPU is weak scaling: each rank owns 65 536 envs (global ids rank*65536 ...), no data-path
collective, one all-gather of episode returns per 500-step episode (RCCL over xGMI, issued by the C++ host:
rq_allgather_returns), enqueued behind the rollout that completed the episode and overlapped with the next one.

Timing: after 0.25 s of rollouts on a scratch shard (the chip's clocks) and, on the benchmarked shard, one untimed step and
exactly --warmup more, ONE timed region of exactly --steps steps (one fused launch per <= 500
of them), bracketed by barrier + synchronize on both sides (max over ranks), gives `value` and `ms_per_step`.  That is all a
plain run does before it prints its line; `--dump-outputs DIR` first writes what the last timed step left (GpuEngine.outputs,
write_outputs).  Everything below is `--full`, which runs after the headline region:

With --full, timed regions of exactly --steps steps are REPEATED (at least 5 times and until 0.25 s of timed
regions have accumulated, at most 2000); every region is timed (max over ranks) and `timing.repeated_regions`
reports first / min / median / mean / max.  The exchange belongs to the episode: one all-gather per 500 steps,
posted by the region in which the 500th step falls and waited for inside that region.  The repeated regions'
`ms_per_step` and `value` charge every region its share of it: the median region WITHOUT an exchange plus
steps/500 of the difference to the median region WITH one (round 3; the plain median of round 2 never saw the
1-in-25 region that carries the collective when --steps is 20).  A short region (--steps 20 is one 70 us launch)
is bound by launch overhead and by the clock ramp of the first ~20 ms; `steady_state` therefore adds 10
back-to-back 500-step launches measured in the same run, so that the record carries the steady-state figure
too, and `config4` the same workload at BASELINE config 3/4's 262 144 envs per GPU.

The orchestration (rendezvous, native-communicator consensus with its torch fallback, timed regions, max over
ranks, the one JSON line) is `run_benchmark(args, engine, ...)`: `engine` is the product on this rank
(`GpuEngine`) or, in the CPU tests, a stand-in with the same interface (`--engine tests.bench_stub_engine
--backend gloo`: tests/test_bench_orchestration.py runs two gloo ranks through it, including a rank that
fails phase 1 or phase 2 of the consensus).

Rank 0 prints ONE JSON line: metric, value, unit, higher_is_better, dtype, ms_per_step, config and `timing` (the
headline region), and with --full these extra objects:
  timing.repeated_regions  repetitions and the spread of the repeated timed regions
  steady_state  10 x 500-step launches back to back: env-steps/s, us/step, fraction of the fp32 peak
  roofline      dominant kernel of the timed region (the fused rollout kernel)
  cpu_baseline  the oracle's C restatement timed on this box's host cores (a reported
                baseline, not the target)
and, as additional evidence, `kernels`: HBM-roofline figures of the API-granular kernels
(k_observe / k_actor_step / k_step) at the same batch and at 2 097 152 envs (true HBM traffic:
the 65 536-env working set fits the 256 MiB Infinity Cache).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ENVS_PER_GPU = 65536
EPISODE = 500
MIN_REPETITIONS, MAX_REPETITIONS, MIN_TIMED_SECONDS = 5, 2000, 0.25
CLOCK_WARMUP_SECONDS = 0.25

# ---- algorithmic work per env-step (DESIGN.md "Work per env-step") ---------------------------
# actor: 2*(16*22 + 48*16 + 48*16 + 4*16) = 3904 FLOP + gates: per hidden element
#        2 sigmoids (exp, add, rcp) + tanh (fma, exp, add, rcp, fma) + blend (sub, fma) = 16 -> 256
# env:   4 dynamics evaluations x 108 + RK4 accumulation 7 x 17 fma = 238 + set-points 16 +
#        normalise 18 + rotor clamp 8 + reward/termination 70 + observation 26 = 808
FLOP_ACTOR, FLOP_GATES, FLOP_ENV = 3904, 256, 808
FLOP_PER_ENV_STEP = FLOP_ACTOR + FLOP_GATES + FLOP_ENV
# bytes per env per launch of the API-granular kernels (float32 fields actually touched)
BYTES_OBSERVE = 4 * (17 + 4 + 2) + 4 * 26                      # read state+action history+2 params, write obs
BYTES_ACTOR = 4 * (22 + 16) + 4 * (16 + 4)                     # 232 B
BYTES_STEP = 4 * (21 + 17 + 6 + 4 + 2) + 4 * (17 + 4) + 4 + 1 + 8   # params, state, dist, action, stats -> state, stats
# fused kernel, per env per launch (K steps): params 21 + state 27 + hidden 16 + stats in; state 21 + hidden 16 + stats out
BYTES_FUSED_LAUNCH = 4 * (21 + 27 + 16 + 8) + 4 * (21 + 16 + 8)
PEAK_FP32_TFLOPS = 157.3     # MI355X_MICROARCH.md: fp32 vector peak = f32 MFMA peak (dense)
PEAK_BF16_TFLOPS = 2500.0    # MI355X_MICROARCH.md: bf16 MFMA dense peak
PEAK_HBM_GBPS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=5000)
    ap.add_argument("--envs-per-gpu", type=int, default=ENVS_PER_GPU)
    ap.add_argument("--mode", default="fused", choices=["fused", "chained"])
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16", "f16x2"],
                    help="actor operand precision: fp32 = BASELINE config 2 (headline), bf16 = config 5, "
                         "f16x2 = split-f16 operands (fp32-grade results on the co-executing matrix pipe)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-probe", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--force-native-exchange", action="store_true",
                    help="use the C++ host's RCCL all-gather even with one rank (it is always used with more)")
    ap.add_argument("--backend", default=None, choices=["nccl", "gloo"],
                    help="torch.distributed backend of the rendezvous (default: the engine's: nccl = RCCL)")
    ap.add_argument("--engine", default="hip",
                    help="'hip' = libraptor_quad.so on this rank's GPU (the product); a module path = a stand-in with "
                         "the same interface (module.create_engine(local_rank, args)): CPU tests of the orchestration")
    ap.add_argument("--no-config4", action="store_true", help="skip the 262 144-envs-per-GPU block")
    ap.add_argument("--allow-oversubscribe", action="store_true",
                    help="TESTS ONLY: more ranks than GPUs - rank r drives GPU r %% (GPUs of the node), the rendezvous backend defaults to "
                         "gloo (RCCL cannot put two ranks on one device; RQ_RCCL_LIBRARY names the tests' stand-in for the native exchange). "
                         "What the driver's 8-GPU command meets, on the one GPU of a test box; the record says `oversubscribed`")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, everything else the record can hold: repeated timed regions, kernel-level timing, "
                         "steady state, the gathered returns' layout check, config 4, roofline, API-granular kernels, extensions, "
                         "parity and the CPU baseline (a plain run sets up, warms up, times --steps steps and prints the headline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step left (rank 0's shard) as DIR/<name>.npy, float32, at most 64 MB in all "
                         "(a fixed, seeded sample of envs beyond that)")
    return ap.parse_args(argv)


class Shard:
    """The l2f-shaped objects of one rank's shard."""

    def __init__(self, device, n, offset, seed=0, precision="fp32"):
        import raptor_amd.l2f as l2f
        from raptor_amd.foundation_policy import Raptor
        self.device, self.n = device, n
        self.vector = v = l2f.VectorModule(n, offset)
        self.rng, self.env = v.VectorRng(), v.VectorEnvironment()
        self.params, self.state = v.VectorParameters(), v.VectorState()
        v.initialize_rng(device, self.rng, seed)
        v.initialize_environment(device, self.env)
        cfg = self.env.config
        # the one fitted MDP constant of the specification, pinned here as well: a change of the library's default
        #  must not move the benchmarked workload unnoticed
        cfg.termination_position = 1.0
        self.env.config = cfg
        v.sample_initial_parameters(device, self.env, self.params, self.rng)
        v.sample_initial_state(device, self.env, self.params, self.state, self.rng)
        self.policy = Raptor(device, precision=precision)
        self.policy.reset()

    def rollout(self, steps, mode):
        self.vector.rollout(self.device, self.env, self.params, self.state, self.policy, self.rng, steps, mode,
                            autoreset=True)


OUTPUT_LIMIT_BYTES = 64 << 20


def write_outputs(directory, arrays, limit=OUTPUT_LIMIT_BYTES):
    """`--dump-outputs`: one DIR/<name>.npy per array (float32, env-major: row i = env i).  Beyond `limit` bytes in all, the same
    rows of every array are kept - a sorted sample drawn with a fixed seed - and `sample_envs.npy` (float64) says which envs."""
    arrays = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in arrays.items()}
    rows = {v.shape[0] for v in arrays.values()}
    assert len(rows) == 1, f"outputs of different lengths: { {k: v.shape for k, v in arrays.items()} }"
    n = rows.pop()
    total = sum(v.nbytes for v in arrays.values())
    limit -= 256 * (len(arrays) + 1)                 # the .npy headers (128 bytes each as numpy writes them)
    if total > limit:
        keep = limit * n // (total + 8 * n)          # 8 more bytes per kept row: its index
        pick = np.sort(np.random.default_rng(0).choice(n, size=keep, replace=False))
        arrays = {k: v[pick] for k, v in arrays.items()}
        arrays["sample_envs"] = pick.astype(np.float64)
    os.makedirs(directory, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(directory, k + ".npy"), v)


def actor_groups_per_wave(n):
    """raptor_amd/csrc/rq_kernels.hpp actor_groups_per_wave: 64-env groups per wave of k_actor_step at n envs"""
    groups = (n + 63) // 64
    return 1 if groups < 4096 else min(64, groups // 1024)


def actor_step_kernel_name(n, actor="rq::ActorF32T<true>"):
    """The kernel launch_actor_step picks at n envs, as rocprofv3 prints it: one 64-env group per wave (k_actor_step) up to
    262 144 envs, the streaming kernel (k_actor_stream: groups / 1 024 groups per wave) beyond - two kernels, two names: a profile
    tells a 2 097 152-env launch from a 65 536-env one even where the grids coincide."""
    return f"rq::k_actor_stream<{actor} >" if actor_groups_per_wave(n) > 1 else f"rq::k_actor_step<{actor} >"


def launch_grid(kernel, n):
    """Threads in the grid the launcher picks for `kernel` at n envs (raptor_amd/csrc/rq_kernels.hip)."""
    if kernel.startswith("rq::k_actor_stream"):
        groups = (n + 63) // 64
        gpw = actor_groups_per_wave(n)
        return ((groups + gpw - 1) // gpw * 64 + 255) // 256 * 256
    if kernel.startswith(("rq::k_rollout_fused", "rq::k_actor_sequence", "rq::k_actor_relabel")):
        return (n + 63) // 64 * 64
    return (n + 255) // 256 * 256


def pmc_key(kernel, n):
    """Key of a kernel's entry in profiles/*_pmc.json: (instantiation, env count) - round 4; rounds 1-3 keyed by grid size,
    which is not the env count for k_actor_step and made the launch shape part of the bookkeeping."""
    return f"{kernel.replace(' ', '')}#n{n}"          # no blanks: demanglers differ in "> >" against ">>"


def pmc_traffic(kernel, n, library=None):
    """HBM bytes per launch of EXACTLY the kernel instantiation `kernel` (profiled name without its argument
    list, e.g. "rq::k_rollout_fused<false, true, false, rq::ActorF32T<false> >") at `n` envs, from the
    newest committed rocprofv3 PMC summary that has it (profiles/*_pmc.json: separate FETCH_SIZE / WRITE_SIZE
    passes of this same command, FETCH_SIZE doubled per the gfx950 correction of MI355X_MICROARCH.md; the
    median over that kernel's launches, so the handful of warm-up launches of another length do not count).
    None when no profile covers it.  `same_library`: whether that summary was collected from the build loaded now (round 6: the
    file carries `_library_sha256`); counters are not re-collected live, so a figure from another build is reported as such
    and does not become the record's `traffic`."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc.json")), reverse=True):
        try:
            table = json.load(open(path))
        except Exception:
            continue
        d = table.get(pmc_key(kernel, n))
        if d is None:                                     # rounds 1-3: "<name as printed>@<grid>"
            legacy = f"{kernel}@{launch_grid(kernel, n)}".replace(" ", "")
            d = next((v for k, v in table.items() if k.replace(" ", "") == legacy and v.get("envs", n) == n), None)
        if d and d.get("hbm_bytes_per_launch_corrected"):
            return {"same_library": (table.get("_library_sha256") == library) if library else None,
                    "bytes_per_launch": d["hbm_bytes_per_launch_corrected"],
                    "bytes_per_env": round(d["hbm_bytes_per_launch_corrected"] / n, 2), "source": os.path.basename(path),
                    "kernel": kernel, "profiled_launch_us": d.get("median_dur_us", d.get("avg_dur_us_fetch")),
                    "profiled_launches": d.get("calls_fetch")}
    return None


_library_hash = None


def library_sha256():
    """sha256 of the libraptor_quad.so this process loads (RAPTOR_QUAD_LIB honoured): what ties a committed profile to a build."""
    global _library_hash
    if _library_hash is None:
        import hashlib
        from raptor_amd import _lib
        h = hashlib.sha256()
        with open(_lib.LIB_PATH, "rb") as f:
            for chunk in iter(lambda: f.read(1 << 20), b""):
                h.update(chunk)
        _library_hash = h.hexdigest()
    return _library_hash


def traffic_of(tr):
    """`traffic` of a record from pmc_traffic()'s answer: the counters' bytes per launch when the summary was collected from the
    build loaded now; None (with the reason left in `traffic_source`) when it covers another build or nothing."""
    if tr is None or tr.get("same_library") is False:
        return None
    return tr["bytes_per_launch"]


def rocprof_launch_stats(kernel, n, steps, library=None, profiles_dir=None):
    """What rocprofv3 printed for the launches of `kernel` in the timed regions of this same command (newest committed
    profiles/rNN_fused_launch_stats.json, written by tools/summarize_profiles.py from the kernel trace: End - Start per
    dispatch).  The profiler's duration begins when the command processor takes the dispatch and ends when the kernel's
    writes are released; the waves' own clocks (`avg_launch_ms`) begin with their first instruction and end with their
    last - ~2.6 us less for a 20-step launch.
    Round 6: a trace counts only for the BUILD it was taken from - the file carries the sha256 of the library that ran under
    the profiler (`library_sha256`), and it is used iff that equals `library`, the hash of the library loaded now.  Rounds 1-5
    matched on kernel NAME, env count and step count only, so a changed kernel with the same name inherited an old fraction.
    -> (stats or None, reason why not)"""
    import glob
    import re
    paths = [p for p in glob.glob(os.path.join(profiles_dir or os.path.join(ROOT, "profiles"), "*_fused_launch_stats.json"))
             if re.fullmatch(r"r\d+_fused_launch_stats\.json", os.path.basename(p))]
    reason = "no committed rocprofv3 trace of this command (kernel, env count and steps per region must all match)"
    for path in sorted(paths, reverse=True):
        try:
            d = json.load(open(path))
            if int(d.get("steps", -1)) != int(steps) or int(d.get("envs_per_gpu") or -1) != int(n):
                continue
            row = d[kernel.replace(" ", "")]["timed_region_launches"]
            if library is not None and d.get("library_sha256") != library:
                if "another build" not in reason:          # the newest such trace is the one worth naming
                    theirs = d.get("library_sha256")
                    reason = (f"profiles/{os.path.basename(path)} was taken from another build of the library "
                              f"({'it records no sha256' if not theirs else 'its sha256 ' + theirs[:12] + '...'}; loaded {library[:12]}...)")
                continue
            return {"launches": row["launches"], "mean_us": row["mean_us"], "median_us": row["median_us"],
                    "source": os.path.basename(path), "command": d.get("command"), "library_sha256": d.get("library_sha256")}, None
        except Exception:
            continue
    return None, reason


def fused_kernel_name(precision, n, steps_per_launch):
    """The instantiation launch_rollout_fused picks (raptor_amd/csrc/rq_kernels.hip), as rocprofv3 prints it."""
    if precision == "f16x2":
        actor = "rq::ActorF16X2"
    elif precision == "bf16":
        actor = "rq::ActorBF16"                     # (round 4: the one-wave build at every size)
    else:
        actor = "rq::ActorF32T<true> " if n > 65536 else "rq::ActorF32T<false> "
    return f"rq::k_rollout_fused<false, true, false, false, {actor}>"     # <NOISE, AUTORESET, RECORD, SAS, ACTOR>


# what ONE wave per SIMD pays per instruction (tools/lonewave.hip on the MI355X, profiles/r04_lonewave.txt; core-clock cycles):
# any instruction 4.6; an independent vector instruction 5.06 (8.25 when it reads the result of the one right before it);
# a transcendental 8.75; v_permlane*_swap 9.4; a bf16 MFMA hidden behind >= 4 vector instructions ~6
LONE_WAVE_CYCLES = {"valu": 5.06, "trans": 8.75, "mfma_16bit_overlapped": 6.0, "salu": 4.63}


def sq_profile(precision):
    """MFMA utilisation of the FUSED ROLLOUT kernel from its committed SQ-counter pass (tools/sq_profile.sh ->
    profiles/rNN_sq_counters.json; exactly that file name: round 3 globbed *_sq_counters.json and read the teacher
    kernel's counters for the bf16 rollout): matrix-pipe busy cycles / wave cycles (SQ_WAVE_CYCLES counts quad-cycles),
    the co-execution share, the clock of the PROFILED launch (GRBM_GUI_ACTIVE over the eight dies / duration: counter
    collection itself holds the chip ~10 % below the clock of an un-profiled run, so this is not the clock of the record's
    own launches - those carry `clock_ghz_under_load` from rq_device_last_rollout_clock) and the instruction counts per
    wave-step with the lone-wave issue model built from them."""
    import glob
    import re
    paths = [p for p in glob.glob(os.path.join(ROOT, "profiles", "*_sq_counters.json"))
             if re.fullmatch(r"r\d+_sq_counters\.json", os.path.basename(p))]
    for path in sorted(paths, reverse=True):
        try:
            d = json.load(open(path))[precision]
            busy, wave = d["SQ_VALU_MFMA_BUSY_CYCLES"], 4.0 * d["SQ_WAVE_CYCLES"]
            out = {"mfma_busy_frac": round(busy / wave, 4),
                   "mfma_valu_coexec_frac_of_busy": round(d["SQ_VALU_MFMA_COEXEC_CYCLES"] / busy, 4),
                   "issue_stall_frac": round(d["SQ_WAIT_INST_ANY"] / d["SQ_WAVE_CYCLES"], 4),
                   "source": os.path.basename(path)}
            if d.get("GRBM_GUI_ACTIVE") and d.get("dur_us_pass_b"):
                out["clock_ghz_under_profiler"] = round(d["GRBM_GUI_ACTIVE"] / 8.0 / (d["dur_us_pass_b"] * 1e3), 3)
            steps = d.get("wave_steps")          # waves x steps of the profiled launch (tools/sq_profile.sh, round 4)
            if steps:
                mfma = d["SQ_INSTS_MFMA"] / steps
                trans = d["SQ_INSTS_VALU_TRANS_F32"] / steps
                valu = d["SQ_INSTS_VALU"] / steps - mfma - trans
                out["per_wave_step"] = {"mfma": round(mfma, 1), "transcendental": round(trans, 1), "other_vector": round(valu, 1),
                                        "scalar": round(d["SQ_INSTS_SALU"] / steps, 1),
                                        "cycles": round(wave / steps, 1)}
                if precision != "fp32":      # the 16-bit MFMAs hide behind the vector work: the loop is vector-issue-bound
                    floor = (valu * LONE_WAVE_CYCLES["valu"] + trans * LONE_WAVE_CYCLES["trans"]
                             + mfma * LONE_WAVE_CYCLES["mfma_16bit_overlapped"] + d["SQ_INSTS_SALU"] / steps * LONE_WAVE_CYCLES["salu"])
                    out["lone_wave_issue_model_cycles"] = round(floor, 1)
                    out["measured_over_issue_model"] = round(wave / steps / floor, 4)
            return out
        except Exception:
            continue
    return None


def sixteen_bit_roofline(precision, n, steps_per_launch, avg_launch_s):
    """`roofline` of the fused kernel with a 16-bit actor (BASELINE config 5: bf16 operands; the split-f16 build): the
    contractions run on the 16-bit matrix pipe (24 MFMAs per wave-step, a few % of its peak) BESIDE the vector unit, so
    what bounds the kernel is the fp32 vector work that remains - gates + env, priced against the fp32 vector peak - and,
    at one wave per SIMD, the rate at which a lone wave issues instructions at all (sq_counters.lone_wave_issue_model)."""
    valu = (FLOP_GATES + FLOP_ENV) * n * steps_per_launch / avg_launch_s / 1e12
    mfma = FLOP_ACTOR * n * steps_per_launch / avg_launch_s / 1e12
    kname = fused_kernel_name(precision, n, steps_per_launch)
    tr = pmc_traffic(kname, n, library_sha256())
    return {"kernel": kname, "bound": "valu_issue", "achieved": round(valu, 3),
            "peak": PEAK_FP32_TFLOPS, "unit": "TFLOP/s", "frac": round(valu / PEAK_FP32_TFLOPS, 4),
            "traffic": traffic_of(tr), "traffic_source": tr,
            "note": f"fp32 VALU work only ({FLOP_GATES + FLOP_ENV} FLOP/env-step: gates + env) against the fp32 "
                    f"vector peak; the actor's {FLOP_ACTOR} FLOP/env-step run on the 16-bit MFMA pipe at "
                    f"{mfma:.1f} TFLOP/s = {mfma / PEAK_BF16_TFLOPS:.3f} of its 2.5 PFLOP/s dense peak"
                    + (" (x3 issued: hi.hi, hi.lo, lo.hi products)" if precision == "f16x2" else "")
                    + "; one wave per SIMD: the binding limit is the lone wave's instruction issue (5.06 cycles per vector "
                      "instruction, 8.75 per transcendental: tools/lonewave.hip), see sq_counters.measured_over_issue_model",
            "mfma_TFLOPs": round(mfma, 2), "mfma_peak_TFLOPs": PEAK_BF16_TFLOPS, "mfma_frac_of_peak": round(mfma / PEAK_BF16_TFLOPS, 5),
            "avg_launch_ms": round(avg_launch_s * 1e3, 4), "steps_per_launch": steps_per_launch,
            "hbm_bytes_per_env_step": round(BYTES_FUSED_LAUNCH / steps_per_launch, 3),
            "sq_counters": sq_profile("bf16") if precision == "bf16" else None}


def chunks(total, size):
    out = []
    while total > 0:
        out.append(min(size, total))
        total -= out[-1]
    return out


def kernel_probe(device, n, reps):
    """Median launch duration (HIP events on the kernels' own stream) of the three API-granular
    kernels at batch n, device-resident chain, and their algorithmic HBM bandwidth."""
    sh = Shard(device, n, 0)
    v = sh.vector
    out = {}

    def fresh_episode():
        # k_step is timed stepping the SAME action over and over: left alone the quadrotors fly off, and a terminated env
        # writes its episode statistics on every further step (16 B per env more than the 297 the figure is priced at)
        v.sample_initial_state(device, sh.env, sh.params, sh.state, sh.rng)

    def timed(fn):
        """(median, min, max) microseconds per launch: >= 50 warm-up launches, then >= 20 timed batches of `reps`
        launches each (HIP events on the engine's stream around a batch), every batch from a freshly sampled state.
        The median of batches, not a mean of launches: one preempted batch (the driver's round-2 record carried a
        175 us k_observe) cannot print."""
        for _ in range(max(50, reps)):
            fn()
        device.synchronize()
        per = []
        for _ in range(20):
            fresh_episode()
            device.synchronize()
            device.timer_start()
            for _ in range(reps):
                fn()
            per.append(device.timer_stop() / reps * 1e3)
        return float(np.median(per)), float(min(per)), float(max(per))

    v.observe(device, sh.env, sh.params, sh.state, None, sh.rng)
    sh.policy.evaluate_step_device(sh.env)
    for name, nbytes, fn in (
        ("k_observe", BYTES_OBSERVE, lambda: v.observe(device, sh.env, sh.params, sh.state, None, sh.rng)),
        ("k_actor_step", BYTES_ACTOR, lambda: sh.policy.evaluate_step_device(sh.env)),
        ("k_step", BYTES_STEP, lambda: v.step_device(device, sh.env, sh.params, sh.state, sh.state, sh.rng)),
    ):
        us, us_min, us_max = timed(fn)
        gbps = nbytes * n / (us * 1e-6) / 1e9
        tr = pmc_traffic({"k_observe": "rq::k_observe<false>", "k_actor_step": actor_step_kernel_name(n),
                          "k_step": "rq::k_step<false>"}[name], n, library_sha256())
        out[name] = {"bound": "hbm", "us_per_launch": round(us, 3),
                     "us_per_launch_min_max": [round(us_min, 3), round(us_max, 3)], "statistic": "median of 20 batches",
                     "bytes_per_env": nbytes,
                     "achieved_GBps": round(gbps, 1), "peak_GBps": PEAK_HBM_GBPS,
                     "frac": round(gbps / PEAK_HBM_GBPS, 4),
                     "traffic": traffic_of(tr),
                     "traffic_bytes_per_env": None if traffic_of(tr) is None else tr["bytes_per_env"],
                     "traffic_same_library": None if tr is None else tr["same_library"]}
    # A standalone launch at 65 536 envs is launch-latency-bound and its 20-30 MB working set sits in the 256 MiB
    # Infinity Cache, so its fraction of the HBM peak is not a bandwidth statement.  Split it instead: back-to-back
    # launches of a kernel that only stores one float per thread on the same grid take `near_empty_launch_us` each
    # (rq_device_launch_floor, HIP events); the rest of the launch is the phase that moves this kernel's bytes.
    floor_us = device.launch_floor(n, 200)
    for name in ("k_observe", "k_actor_step", "k_step"):
        nb = out[name]["bytes_per_env"] * n
        data_us = max(out[name]["us_per_launch"] - floor_us, 1e-3)
        out[name]["launch_split"] = {"near_empty_launch_us": round(floor_us, 3), "data_phase_us": round(data_us, 3),
                                     "data_phase_GBps": round(nb / (data_us * 1e-6) / 1e9, 1),
                                     "working_set_MB": round(nb / 1e6, 1),
                                     "resident_in_infinity_cache": bool(nb < 256 * 2 ** 20)}
        if name == "k_actor_step" and n >= 262144:
            # what bounds the large batches' actor step (k_actor_stream): the matrix + gate work of n / 64 groups over the
            # 1 024 SIMDs (120 f32 MFMAs x 32 cycles + 96 transcendentals x 8.75 + ~130 vector instructions x 5.06 per group,
            # at the 2.37 GHz the chip runs at in a busy loop) and the traffic at the rate a pure copy of its access shape
            # reaches (38 + 20 field-major streams: 5.3 TB/s, tools/streams.hip); perfect overlap would be their maximum
            groups_per_simd = (n + 63) // 64 / 1024.0
            matrix_us = groups_per_simd * (120 * 32 + 96 * 8.75 + 130 * 5.06) / 2.37e3
            traffic_us = nb / 5.3e6
            out[name]["bounds"] = {"kernel": actor_step_kernel_name(n), "matrix_and_gates_us": round(matrix_us, 1),
                                   "traffic_at_copy_rate_of_its_shape_us": round(traffic_us, 1),
                                   "measured_over_max_of_bounds": round(out[name]["us_per_launch"] / max(matrix_us, traffic_us), 3)}
        if nb < 256 * 2 ** 20:
            out[name]["note"] = ("launch-latency-bound at this size: the working set sits in the 256 MiB memory-side cache and "
                                 f"{floor_us:.1f} of the {out[name]['us_per_launch']:.1f} us are what any launch on this grid costs; "
                                 "`frac` is not a bandwidth statement here - the HBM-bound figure is kernels.n2097152."
                                 + name + " (north_star's >= 0.6 of HBM on the step kernel holds there)")
    return out


def extension_probe(device, n):
    """The two rows beside the loop body: the rollout WITH trajectory recording, and the
    policy over a whole [T, n, 22] device tensor in one launch (Raptor.evaluate_sequence)."""
    import torch
    from raptor_amd.foundation_policy import Raptor
    out = {}
    sh = Shard(device, n, 0)
    steps = 200
    traj = sh.vector.Trajectory(sh.env, steps)
    for _ in range(4):
        sh.rollout(500, "fused")
    best = 1e9
    for _ in range(3):
        traj.reset()
        device.timer_start()
        sh.vector.rollout(device, sh.env, sh.params, sh.state, sh.policy, sh.rng, steps, "fused", autoreset=True,
                          trajectory=traj)
        best = min(best, device.timer_stop())
    rate = n * steps / (best * 1e-3)
    out["rollout_recorded"] = {"env_steps_per_s": round(rate, 1), "us_per_step": round(best * 1e3 / steps, 3),
                               "trajectory_bytes_per_env_step": 109, "trajectory_GBps": round(rate * 109 / 1e9, 1)}
    del traj
    # the other actor precisions on the same workload (the headline above stays the exact-fp32 build).  Sustained figure,
    # like `steady_state` for the fp32 build: regions of 10 x 500-step launches back to back (the chip's clock follows its
    # load of the last ~millisecond, tools/idle_clock.py: a single launch behind an idle gap runs ~12 % slower, also
    # reported); kernel = the last launch's own first-wave-in / last-wave-out span of further such regions (back-to-back
    # launches overlap their ends - the next one's waves start on SIMDs the finished ones freed - so a launch's own span
    # can read slightly above the region's time per launch)
    for prec, key in (("bf16", "rollout_bf16_actor"), ("f16x2", "rollout_split_f16_actor")):
        sh.policy.set_precision(prec)
        for _ in range(6):
            sh.rollout(500, "fused")
        regions, single = [], []
        for _ in range(5):
            device.synchronize()
            device.timer_start()
            for _ in range(10):
                sh.rollout(500, "fused")
            regions.append(device.timer_stop() / 10)
        for _ in range(5):
            device.synchronize()
            time.sleep(0.002)                       # an idle gap, as between two synchronised calls of a host loop
            device.timer_start()
            sh.rollout(500, "fused")
            single.append(device.timer_stop())
        device.set_rollout_timing(True)
        spans, clocks = [], []
        for _ in range(5):                          # the LAST of ten launches back to back, as in the regions above: a
            for _ in range(10):                     # read-back after every launch idles the chip and lowers its clock
                sh.rollout(500, "fused")
            spans.append(device.last_rollout_ms())
            clocks.append(device.last_rollout_clock_ghz())
        device.set_rollout_timing(False)
        ms, kernel_ms = float(np.median(regions)), float(np.median(spans))
        out[key] = {"env_steps_per_s": round(n * 500 / (ms * 1e-3), 1), "us_per_step": round(ms * 1e3 / 500, 3),
                    "us_per_step_kernel": round(kernel_ms * 1e3 / 500, 3),
                    "us_per_step_single_launch_after_idle": round(float(np.median(single)) * 1e3 / 500, 3),
                    "clock_ghz_under_load": round(float(np.median(clocks)), 3),
                    "statistic": "median of 5 regions of 10 x 500-step launches back to back (kernel span and core clock: the last launch of 5 more such regions)"}
        if prec == "bf16":      # BASELINE config 5 with its roofline (round 4), as `roofline` is built for --precision bf16
            out[key]["roofline"] = sixteen_bit_roofline("bf16", n, 500, kernel_ms * 1e-3)
            out[key]["roofline"]["clock_ghz_under_load"] = out[key]["clock_ghz_under_load"]
    out["rollout_split_f16_actor"]["note"] = ("operands as two f16 pieces each on v_mfma_f32_16x16x32_f16 (22 significand "
                                             "bits, known-answer error 1.2e-6): not fp32 arithmetic, not the headline")
    del sh
    pol = Raptor(device)
    pol.reset()
    x = torch.randn(steps, n, 22, device="cuda:%d" % torch.cuda.current_device())
    for _ in range(3):
        pol.evaluate_sequence(x)
    single = 1e9
    for _ in range(3):
        device.timer_start()
        pol.evaluate_sequence(x)
        single = min(single, device.timer_stop())
    # sustained, like the rollout figures: the chip's clock follows its load of the last milliseconds (tools/idle_clock.py) -
    # the twentieth of twenty launches back to back runs 17 % faster than one launch between two synchronisations
    regions = []
    for _ in range(3):
        device.synchronize()
        device.timer_start()
        for _ in range(16):
            pol.evaluate_sequence(x)
        regions.append(device.timer_stop() / 16)
    best = float(np.median(regions))
    rate = n * steps / (best * 1e-3)
    tf = rate * FLOP_ACTOR / 1e12
    out["evaluate_sequence"] = {"bound": "mfma", "policy_steps_per_s": round(rate, 1),
                                "us_per_step": round(best * 1e3 / steps, 3),
                                "us_per_step_single_launch": round(single * 1e3 / steps, 3), "achieved_TFLOPs": round(tf, 2),
                                "peak_TFLOPs": PEAK_FP32_TFLOPS, "frac": round(tf / PEAK_FP32_TFLOPS, 4),
                                "bytes_per_step": 104, "achieved_GBps": round(rate * 104 / 1e9, 1),
                                "statistic": "median of 3 regions of 16 launches back to back (single: best of 3 launches, each between two synchronisations)"}
    return out


def teacher_probe(device, n, steps=500, hidden=64):
    """SURVEY.md section 8(f) row 2 in the record: n envs x `steps` recorded steps labelled by the reference's
    1 000 teachers (README.md:207-216) and by 1 024, exact-f32 MFMA path; envs assigned to teachers by
    raptor_amd.teachers.balanced_teacher_assignment (whole 16-env tiles per teacher)."""
    from raptor_amd.teachers import TeacherBank, parameter_count, balanced_teacher_assignment
    sh = Shard(device, n, 0)
    tr = sh.vector.Trajectory(sh.env, steps)
    sh.vector.rollout(device, sh.env, sh.params, sh.state, sh.policy, sh.rng, steps, "fused", autoreset=True, trajectory=tr)
    rng = np.random.default_rng(0)
    flop_label = 2 * (22 * hidden + hidden * hidden + hidden * 4)
    out = {"topology": f"22-{hidden}-{hidden}-4 [UPSTREAM-UNVERIFIED]", "envs": n, "steps": steps, "flop_per_label": flop_label}
    for teachers in (1000, 1024):
        W = (rng.standard_normal((teachers, parameter_count(22, hidden, hidden))) * 0.1).astype(np.float32)
        bank = TeacherBank(device, W, 22, hidden, hidden, "relu", "identity", precision="fp32")
        for name, ids in (("balanced", balanced_teacher_assignment(n, teachers)),
                          ("contiguous", (np.arange(n, dtype=np.int64) * teachers // n).astype(np.uint32))):
            for _ in range(4):                     # untimed: the first launches of a bank run on cold caches and clocks
                tr.relabel_teachers(bank, ids, fetch=False)
            per = []
            for _ in range(3):                     # regions of 4 launches back to back (the clock follows the load: see evaluate_sequence)
                device.synchronize()
                device.timer_start()
                for _ in range(4):
                    tr.relabel_teachers(bank, ids, fetch=False)
                per.append(device.timer_stop() / 4)
            ms = float(np.median(per))
            tf = flop_label * n * steps / (ms * 1e-3) / 1e12
            out[f"teachers_{teachers}_{name}"] = {"ms": round(ms, 3), "labels_per_s": round(n * steps / (ms * 1e-3), 1),
                                                 "achieved_TFLOPs": round(tf, 2), "peak_TFLOPs": PEAK_FP32_TFLOPS,
                                                 "frac": round(tf / PEAK_FP32_TFLOPS, 4)}
        del bank
    # a teacher topology outside the register-stationary family (round 5: what TeacherBank.from_checkpoints may meet): three hidden
    # layers of 128 units through the streaming kernel (operands shared through LDS by the four step-slices of a tile), fp32
    from raptor_amd.teachers import layers_parameter_count
    widths = [128, 128, 128]
    W = (rng.standard_normal((1000, layers_parameter_count(22, widths))) * 0.05).astype(np.float32)
    bank = TeacherBank.from_layers(device, W, 22, widths, "relu", "identity")
    ids = balanced_teacher_assignment(n, 1000)
    for _ in range(2):
        tr.relabel_teachers(bank, ids, fetch=False)
    per = []
    for _ in range(3):
        device.synchronize()
        device.timer_start()
        tr.relabel_teachers(bank, ids, fetch=False)
        per.append(device.timer_stop())
    ms = float(np.median(per))
    fl = 2 * (22 * 128 + 128 * 128 * 2 + 128 * 4)
    tf = fl * n * steps / (ms * 1e-3) / 1e12
    out["dense_stack_22-128-128-128-4_teachers_1000"] = {"ms": round(ms, 3), "labels_per_s": round(n * steps / (ms * 1e-3), 1), "flop_per_label": fl,
                                                         "achieved_TFLOPs": round(tf, 2), "peak_TFLOPs": PEAK_FP32_TFLOPS, "frac": round(tf / PEAK_FP32_TFLOPS, 4)}
    del bank
    return out


def dagger_epoch_probe(device, teachers=1000, hidden=64):
    """SURVEY.md section 8(f) rows 1 + 2 timed as the pipeline the reference's post-training would call them in (round 4):
    one DAgger epoch of the reference collects ~77.7 k student-visited transitions (README.md:208; the step axis of its
    training log: 75.3 M steps over 1 000 epochs) and labels them with the teacher of each quadrotor (1 000 teachers,
    README.md:207-216) - here `rq_rollout_record` (fused rollout writing the trajectory) followed by
    `rq_trajectory_relabel_teachers`, everything device-resident.  Two shapes of the same ~78 k transitions: one env per
    teacher flown for 78 steps (what a per-teacher collection looks like; a 16-env tile then carries one env), and 16 envs
    per teacher for 5 steps (whole tiles).  The reference's log spends 7.13 s per epoch on ITS whole epoch (collection in the
    CPU l2f, teacher inference and 146 gradient steps): quoted for scale, not the same work."""
    from raptor_amd.teachers import TeacherBank, parameter_count, balanced_teacher_assignment
    rng = np.random.default_rng(0)
    W = (rng.standard_normal((teachers, parameter_count(22, hidden, hidden))) * 0.1).astype(np.float32)
    bank = TeacherBank(device, W, 22, hidden, hidden, "relu", "identity", precision="fp32")
    out = {"teachers": teachers, "topology": f"22-{hidden}-{hidden}-4 [UPSTREAM-UNVERIFIED]",
           "reference_log_seconds_per_epoch": 7.127, "reference_transitions_per_epoch": 77700}
    for name, n, steps in (("one_env_per_teacher", teachers, 78), ("sixteen_envs_per_teacher", 16 * teachers, 5)):
        sh = Shard(device, n, 0)
        ids = (np.arange(n, dtype=np.int64) * teachers // n).astype(np.uint32)
        tr = sh.vector.Trajectory(sh.env, steps)

        def epoch():
            tr.reset()
            sh.vector.rollout(device, sh.env, sh.params, sh.state, sh.policy, sh.rng, steps, "fused", autoreset=True, trajectory=tr)
            tr.relabel_teachers(bank, ids, fetch=False)

        for _ in range(5):
            epoch()
        device.synchronize()
        per, per_roll = [], []
        for _ in range(9):
            device.timer_start()
            epoch()
            per.append(device.timer_stop())
        for _ in range(9):
            tr.reset()
            device.timer_start()
            sh.vector.rollout(device, sh.env, sh.params, sh.state, sh.policy, sh.rng, steps, "fused", autoreset=True, trajectory=tr)
            per_roll.append(device.timer_stop())
        ms, ms_roll = float(np.median(per)), float(np.median(per_roll))
        out[name] = {"envs": n, "steps": steps, "transitions": n * steps, "ms_per_epoch": round(ms, 4),
                     "ms_rollout_record": round(ms_roll, 4), "ms_relabel": round(ms - ms_roll, 4),
                     "transitions_per_s": round(n * steps / (ms * 1e-3), 1),
                     "epochs_per_reference_epoch_time": round(7127.0 / ms, 1)}
        del tr, sh
    return out


def api_loop_probe(device, n=8, iters=500):
    """BASELINE config 1 shape: the README loop (README.md:94-99), NumPy arrays crossing the boundary
    every call (PCIe-inclusive, host-bound by construction), and the same loop kept on the device.
    Reported as microseconds per loop iteration."""
    import raptor_amd.l2f as l2f
    from raptor_amd.foundation_policy import Raptor
    vector = l2f.vector(n)
    rng, env = vector.VectorRng(), vector.VectorEnvironment()
    params, state, next_state = vector.VectorParameters(), vector.VectorState(), vector.VectorState()
    vector.initialize_rng(device, rng, 0)
    vector.initialize_environment(device, env)
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    policy = Raptor(device)
    observation = np.zeros((env.N_ENVIRONMENTS, env.OBSERVATION_DIM), dtype=np.float32)
    out = {}
    import gc
    gc.collect()      # free the previous probes' device buffers now, not inside the timed loop
    # numpy_arrays: the loop as the README writes it; below 257 envs its step + speculated policy step are commands to the resident
    # executor (round 6: one workgroup stays on the device, include/raptor_quad.h rq_device_set_resident) - `numpy_arrays_launches`
    # is the same loop with the executor switched off (two launches per iteration, what rounds 3-5 measured)
    for name in ("numpy_arrays", "numpy_arrays_launches", "device_resident"):
        policy.reset()
        device.set_resident(name != "numpy_arrays_launches")
        t0 = None
        warm = max(5, iters // 10)
        before = None
        for it in range(iters + warm):
            if it == warm:
                before = device.resident()
                t0 = time.perf_counter()
            if name != "device_resident":
                vector.observe(device, env, params, state, observation, rng)
                action = policy.evaluate_step(observation[:, :22])
                vector.step(device, env, params, state, action, next_state, rng)
                state.assign(next_state)
            else:
                vector.observe(device, env, params, state, None, rng)
                policy.evaluate_step_device(env)
                vector.step_device(device, env, params, state, state, rng)
        if name == "device_resident":
            device.synchronize()
        elapsed = time.perf_counter() - t0
        out[name + "_us_per_iteration"] = round(elapsed / iters * 1e6, 2)
        if name == "numpy_arrays":
            after = device.resident()
            out["resident_executor"] = {k: after[k] - before[k] for k in ("starts", "commands", "replays")}
            out["resident_executor"]["iterations"] = iters
        device.synchronize()
    device.set_resident(True)
    out["env_steps_per_s_numpy_arrays"] = round(n / (out["numpy_arrays_us_per_iteration"] * 1e-6), 1)
    return out


def policy_alone_probe(device, batch=1, calls=2000):
    """README.md:17-25: `policy.evaluate_step(observation)[0]` inside a caller's own simulator - the policy alone, batch 1, NumPy
    arrays at every call.  Microseconds per call with the resident policy executor (round 6: k_resident_policy) and as the launch
    it replaces."""
    from raptor_amd.foundation_policy import Raptor
    policy = Raptor(device)
    X = np.random.default_rng(0).standard_normal((calls + 200, batch, 22)).astype(np.float32)
    out = {"batch": batch, "calls": calls}
    for name in ("resident_executor", "launches"):
        policy.reset()
        device.set_resident(name == "resident_executor")
        before = None
        for t in range(calls + 200):
            if t == 200:
                before = device.resident()
                t0 = time.perf_counter()
            policy.evaluate_step(X[t])
        out[name + "_us_per_call"] = round((time.perf_counter() - t0) / calls * 1e6, 2)
        if name == "resident_executor":
            after = device.resident()
            out["commands"] = {k: after[k] - before[k] for k in ("starts", "commands", "replays")}
        device.synchronize()
    device.set_resident(True)
    return out


def cpu_baseline(seconds):
    """Oracle (C restatement of the reference semantics; the reference binary is unavailable) on
    this box's host cores: same workload, bounded sample, all OpenMP threads."""
    from oracle import oracle as O
    from raptor_amd.foundation_policy import load_weights
    w = load_weights()
    cfg = O.default_config()
    threads = O.max_threads()

    def run(n, steps):
        P = O.sample_initial_parameters(cfg, 0, 0, 0, n)
        st = O.Stats(n)
        S = O.sample_initial_state(cfg, 0, st.episode, 0, P)
        H = np.zeros((n, 16), np.float32)
        t0 = time.perf_counter()
        O.rollout(cfg, w, 0, 0, 0, P, S, H, steps, 1, st, threads)
        return n * steps / (time.perf_counter() - t0)

    rate = run(max(64 * threads, 1024), 100)                 # calibration
    n = ENVS_PER_GPU                                          # the bench's own batch
    steps = int(max(20, min(2000, rate * seconds / n)))       # ~`seconds` of wall time on all host cores
    # BASELINE.md section 2 side lines (all with the same C restatement): B2 = N 8, one thread, native loop;
    # B4 = one thread on a larger batch; B1 = the README loop at N 8 driven call by call from Python
    extras = {}
    threads_all, threads = threads, 1
    extras["B2_n8_1thread_env_steps_per_s"] = round(max(run(8, 500) for _ in range(3)), 1)
    extras["B4_n1024_1thread_env_steps_per_s"] = round(run(1024, 300), 1)
    threads = threads_all
    P8 = O.sample_initial_parameters(cfg, 0, 0, 0, 8)
    st8 = O.Stats(8)
    S8 = O.sample_initial_state(cfg, 0, st8.episode, 0, P8)
    H8 = np.zeros((8, 16), np.float32)
    t1 = time.perf_counter()
    for k in range(500):
        obs = O.observe(cfg, 0, k, 0, P8, S8)
        act = O.actor_batch_step(w, obs, H8)
        S8, _, _ = O.step(cfg, P8, S8, act)
    extras["B1_n8_python_loop_us_per_iteration"] = round((time.perf_counter() - t1) / 500 * 1e6, 2)
    c0, t0 = time.process_time(), time.perf_counter()
    value = run(n, steps)
    busy = (time.process_time() - c0) / (time.perf_counter() - t0)   # CPU-seconds per wall-second
    # the same sample with as many threads as the container really gets (its CPU quota can sit far below the cores the
    # OpenMP runtime sees: 128 threads on ~16 effective cores in the driver's box): the figure without oversubscription
    eff = max(1, int(round(busy)))
    value_eff = None
    if eff < threads_all:
        threads = eff
        value_eff = run(n, max(20, steps // 2))
        threads = threads_all
    # `value` is the BEST the host did (round 5): with more OpenMP threads than the container's CPU quota serves, the
    # all-threads run is the slower one (128 threads on ~16 effective cores: 1.44e7 against 1.92e7 with 16 threads)
    runs = [{"threads": threads_all, "env_steps_per_s": round(value, 1)}]
    if value_eff is not None:
        runs.append({"threads": eff, "env_steps_per_s": round(value_eff, 1)})
    best = max(runs, key=lambda r: r["env_steps_per_s"])
    return {"value": best["env_steps_per_s"], "unit": "env-steps/s", "cores": best["threads"], "kind": "port",
            "runs": runs, "host_threads_available": threads_all,
            "effective_cores": round(busy, 1),      # CPU-seconds per wall-second of the all-threads run: the container's quota
            "extras": extras,
            "sample": f"{n} envs x {steps} steps of the same workload (domain-randomised, auto-reset), "
                      f"oracle/raptor_oracle.c, gcc -O2 -march=x86-64-v3 -fopenmp, {threads_all} threads "
                      "(deviation from BASELINE.md section 2, which planned -O3 -march=native: the oracle's .so is built once and "
                      "travels to the GPU box, whose host CPU is another one - x86-64-v3 is the portable AVX2/FMA level - and -O2 "
                      "because the env arithmetic is contract-ordered scalar fp32 (-ffp-contract=off) that -O3 does not vectorise further)"
                      + ("" if value_eff is None else f"; again with {eff} threads ({max(20, steps // 2)} steps); `value` is the faster run")}


def parity_block(device):
    """What the record may claim about agreement with the reference, next to the headline (round 5): the actor against the
    reference's two known-answer vectors, measured NOW on the HIP path; the environment's status (nothing in the reference tree can
    pin it); and the one reference-produced statistic with no free parameter on the dynamics side - the training log's crazyflie/*
    tags - against what this specification gives, which it does NOT reproduce (numbers from the newest committed
    profiles/*_env_constraints.json, oracle runs of tools/env_constraint_study.py; the joint scan of
    tools/joint_constraint_scan.py beside it)."""
    import glob
    from raptor_amd.foundation_policy import Raptor
    out = {"actor": {"pinned_by": "checkpoint.h example (checkpoint.h:197-215) and h5:/example/{input,output}: 2 x [500, 2, 22] -> [500, 2, 4]",
                     "tolerance": 1e-5},
           "env": {"status": "unpinned vs l2f: the reference tree holds no source, test or trajectory of vector::step / observe / sample_* "
                             "(.gitmodules:1-3: empty rl-tools submodule; README.md:33: pip packages not in the container)",
                   "checked_instead": "bit-exact against oracle/raptor_oracle.c (the repository's own restatement) in `pytest -m gpu`; "
                                      "closed-loop stabilisation by the shipped checkpoint"}}
    gold = os.path.join(ROOT, "tests", "golden")
    try:
        pol = Raptor(device)
        x = np.fromfile(os.path.join(gold, "kat_h_input.bin"), "<f4").reshape(500, 2, 22)
        y = np.fromfile(os.path.join(gold, "kat_h_output.bin"), "<f4").reshape(500, 2, 4)
        out["actor"]["kat_h_max_abs_err"] = float(pol.selftest(x, y, tolerance=1e-5))
        from raptor_amd.checkpoint import load_checkpoint_h5
        _, example, _ = load_checkpoint_h5(os.path.join(gold, "checkpoint.h5"))
        if example is not None:
            out["actor"]["kat_h5_max_abs_err"] = float(pol.selftest(example[0], example[1], tolerance=1e-5))
    except Exception as exc:      # noqa: BLE001
        out["actor"]["error"] = str(exc)
    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_env_constraints.json")), reverse=True)
    if paths:
        d = json.load(open(paths[0]))
        row = next((r for r in d["rows"] if not r["change"]), None)
        keys = ("share_terminated", "episode_length", "terminated_episode_length")
        if row:
            out["reference_log"] = {
                "source": "logs.tfevents of the reference's checkpoint (tests/golden/reference_log.json), pool of the last 100 epochs; "
                          "this specification: " + os.path.basename(paths[0]) + " (oracle, " + str(d["envs"]) + " envs)",
                "evaluation": {"log": {k: round(d["log_sampled_quadrotors"][k], 4) for k in keys},
                               "this_specification": {k: row["sampled_quadrotors"][k] for k in keys},
                               "note": "termination_position = 1 m was FITTED to this tag's share: agreement there is not evidence"},
                "crazyflie": {"log": {k: round(d["log_nominal_crazyflie"][k], 4) for k in keys},
                              "this_specification": {k: row["nominal_crazyflie"][k] for k in keys},
                              "note": "NOT reproduced (share three times too low); no fitted constant enters here"},
                "reward_per_step": {"log": d.get("log_reward_per_step"), "this_specification": row["sampled_quadrotors"].get("reward_per_step")}}
    joint = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_joint_constraints.json")), reverse=True)
    if joint and "reference_log" in out:
        j = json.load(open(joint[0]))
        out["reference_log"]["joint_scan"] = {"source": os.path.basename(joint[0]), "verdict": j["verdict"],
                                              "settings_reproducing_both_tags": len(j["joint_matches"])}
    # round 6: the one non-fitting experiment that closed the topic (tools/policy_competence.py, oracle): the shipped policy's competence
    # boundary brackets this specification's randomisation ranges; the log is not reproduced with them either
    comp = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_policy_competence.json")), reverse=True)
    if comp and "reference_log" in out:
        c = json.load(open(comp[0]))
        out["reference_log"]["policy_competence"] = {
            "source": os.path.basename(comp[0]), "verdict": c["verdict"],
            "competence_ranges": {k: (v or {}).get("range") for k, v in c["competence_ranges"].items()}}
    out["summary"] = "actor pinned; env unpinned (under-determined by the reference tree): parity is partial"
    return out


def native_exchange_probe(engine, n, launches=6, repeats=5):
    """What the path's one exchange costs where it matters (round 4): the C++ host's all-gather (rq_allgather_returns /
    rq_comm_gathered on the REAL librccl, one rank - the communicator, the copy on the engine's stream, the event
    hand-over to the side stream, ncclAllGather and the completion event are what N ranks execute too; only the xGMI
    transfer itself is absent) posted after every 500-step launch with the NEXT 500-step launch enqueued right behind it,
    at n envs per GPU.  -> us added per episode against the same launches without an exchange, the slowdown of the
    rollout kernel itself (its own first-wave-in / last-wave-out span) with an exchange in flight beside it, the
    exchange's latency on an otherwise idle device and the host time of the posting call."""
    sh = engine.make_shard(n, 0)
    ex = engine.native_exchange(1, 0, engine.native_unique_id())
    dev = engine.device

    def region(with_exchange):
        engine.synchronize()
        t0 = time.perf_counter()
        for _ in range(launches):
            sh.rollout(EPISODE, "fused")
            if with_exchange:
                ex.post(sh)
        if with_exchange:
            ex.finish()
        engine.synchronize()
        return (time.perf_counter() - t0) / launches * 1e6

    region(True)
    region(False)                                   # clocks, lazy allocations, the communicator's first collective
    plain = [region(False) for _ in range(repeats)]
    with_ex = [region(True) for _ in range(repeats)]
    engine.set_rollout_timing(True)
    span_plain, span_beside = [], []
    for _ in range(repeats):
        sh.rollout(EPISODE, "fused")
        span_plain.append(engine.last_rollout_ms() * 1e3)
    for _ in range(repeats):
        sh.rollout(EPISODE, "fused")                # the episode whose returns are gathered ...
        ex.post(sh)
        sh.rollout(EPISODE, "fused")                # ... beside this launch
        span_beside.append(engine.last_rollout_ms() * 1e3)
        ex.finish()
    engine.set_rollout_timing(False)
    alone, post_call = [], []
    for _ in range(4 * repeats):
        engine.synchronize()
        t0 = time.perf_counter()
        ex.post(sh)
        t1 = time.perf_counter()
        ex.finish()
        alone.append((time.perf_counter() - t0) * 1e6)
        post_call.append((t1 - t0) * 1e6)
    gathered = ex.result()
    local = np.asarray(engine.local_returns(sh), dtype=np.float32)
    d = ex.describe()
    base, withx = float(np.median(plain)), float(np.median(with_ex))
    return {"envs": n, "launches_per_region": launches, "exchange": ex.kind + ", 1 rank, real librccl",
            "rccl": {"ranks": d["ranks"], "version": d["version"], "version_code": d["version_code"], "library_path": d["library_path"],
                     "per_rank": [{k: d[k] for k in ("rank", "ranks", "device", "pci_bus_id")}]},
            "exchange_verified": bool(np.array_equal(np.asarray(gathered, dtype=np.float32).reshape(-1), local)),
            "us_per_episode_without_exchange": round(base, 2), "us_per_episode_with_exchange": round(withx, 2),
            "added_us_per_episode": round(withx - base, 2), "added_fraction": round((withx - base) / base, 5),
            "rollout_kernel_us": round(float(np.median(span_plain)), 2),
            "rollout_kernel_us_with_exchange_in_flight": round(float(np.median(span_beside)), 2),
            "rollout_slowdown_fraction": round(float(np.median(span_beside) / np.median(span_plain) - 1.0), 5),
            "exchange_alone_us_post_to_gathered": round(float(np.median(alone)), 2),
            "post_call_host_us": round(float(np.median(post_call)), 2),
            "gathered_returns": int(np.prod(np.shape(gathered))),
            "bytes_per_rank": 4 * n}


class _NativeExchange:
    """rq_comm_* / rq_allgather_returns: the all-gather issued by the C++ host (raptor_amd/csrc/rq_comm.cpp)."""
    kind = "native RCCL (rq_allgather_returns)"

    def __init__(self, ex):
        self.ex = ex

    def post(self, shard):
        self.ex.post(shard.env)

    def finish(self):
        return self.ex.finish(to_host=False)

    def result(self):
        return self.ex.finish()

    def describe(self):
        """ranks / rank / RCCL version / library file / device / PCI bus id as RCCL and the HIP runtime report them
        (rq_comm_describe: ncclCommCount, ncclCommUserRank, ncclGetVersion, ncclCommCuDevice, dladdr, hipDeviceGetPCIBusId)"""
        return self.ex.describe()


class _TorchExchange:
    """raptor_amd.distributed.ReturnsExchange: the same double-buffered exchange through torch.distributed."""

    def __init__(self, ex, why):
        self.ex = ex
        self.kind = f"torch.distributed all_gather_into_tensor (native communicator unavailable: {why})"

    def post(self, shard):
        self.ex.post(lambda buf: shard.env.finished_returns(out=buf, wait=False))

    def finish(self):
        return self.ex.finish()

    def result(self):
        t = self.ex.finish()
        return None if t is None else t.detach().cpu().numpy()

    def describe(self):
        import torch
        import torch.distributed as dist
        version = None
        try:
            version = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:      # noqa: BLE001
            pass
        return {"ranks": dist.get_world_size(), "rank": dist.get_rank(), "version": version, "version_code": None,
                "device": None, "pci_bus_id": None, "library_path": "torch.distributed process group (" + dist.get_backend() + ")",
                "collectives_posted": None}


class GpuEngine:
    """What the orchestration needs from the product on one rank: libraptor_quad.so on this rank's MI355X.
    tests/bench_stub_engine.py implements the same interface without a GPU (CPU tests of run_benchmark)."""
    name = "hip"
    default_backend = "nccl"

    def __init__(self, local_rank, args):
        import torch
        import raptor_amd.l2f as l2f
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
        # RQ_BENCH_DEVICE: every rank on ONE device (tests: two ranks share the single GPU of the test box, with the
        # tests-only RCCL of tests/fake_rccl.cpp and the gloo rendezvous); normally rank r of the node drives GPU r
        local_rank = int(os.environ.get("RQ_BENCH_DEVICE", local_rank))
        if getattr(args, "allow_oversubscribe", False):              # tests only: rank r of more ranks than GPUs drives GPU r % GPUs
            local_rank = local_rank % torch.cuda.device_count()
        torch.cuda.set_device(local_rank)
        self.torch, self.local_rank, self.precision = torch, local_rank, args.precision
        self.device = l2f.Device(local_rank)
        self.tensor_device = f"cuda:{local_rank}"

    def init_process_group(self, dist, backend):
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=self.torch.device("cuda", self.local_rank))
        else:
            dist.init_process_group(backend)
            self.tensor_device = "cpu"        # the few control scalars (consensus flags, max over ranks) travel through gloo

    def make_shard(self, n, offset):
        return Shard(self.device, n, offset, precision=self.precision)

    def synchronize(self):
        # hipDeviceSynchronize: every stream of the device, the library's own included - one wait, not two (a stream
        # synchronize in front of it made the timed region 2.6 us longer: tools/region_split.py, "torch only" against
        # "lib+torch")
        self.torch.cuda.synchronize()

    def native_unique_id(self):
        from raptor_amd.distributed import NativeReturnsExchange
        return NativeReturnsExchange.unique_id()

    def native_exchange(self, world, rank, ident):
        from raptor_amd.distributed import NativeReturnsExchange
        return _NativeExchange(NativeReturnsExchange(self.device, world, rank, ident))

    def torch_exchange(self, n, n_total, why):
        from raptor_amd.distributed import ReturnsExchange
        return _TorchExchange(ReturnsExchange(n, n_total, self.tensor_device, engine_stream=self.device.stream), why)

    def local_returns(self, shard):
        return shard.env.finished_returns()

    @staticmethod
    def outputs(shard):
        """What a caller of the rollout has after its last step, one row per env: the state, the policy's hidden state and the
        env's episode statistics (counts and flags as float32, exact below 2**24)."""
        env = shard.env
        return {"state": shard.state.numpy(), "hidden_state": shard.policy.hidden_state(shard.n), "rewards": env.rewards(),
                "terminated": env.terminated().astype(np.float32), "returns": env.returns(),
                "episode_steps": env.episode_steps().astype(np.float32), "finished_returns": env.finished_returns(),
                "finished_counts": env.finished_counts().astype(np.float32)}

    def set_rollout_timing(self, enable):
        self.device.set_rollout_timing(enable)

    def last_rollout_ms(self):
        return self.device.last_rollout_ms()

    def last_rollout_clock_ghz(self):
        return self.device.last_rollout_clock_ghz()

    def timer_start(self):
        self.device.timer_start()

    def timer_stop(self):
        return self.device.timer_stop()

    def describe(self):
        return {"device": self.torch.cuda.get_device_name(self.local_rank), "hip_runtime": self.torch.version.hip}


def make_engine(spec, local_rank, args):
    if spec == "hip":
        return GpuEngine(local_rank, args)
    import importlib
    return importlib.import_module(spec).create_engine(local_rank, args)


def effective_region(walls, posts, steps, has_exchange):
    """Seconds of one timed region of `steps` steps with its share of the per-episode exchange: the median region
    that posted floor(steps/500) exchanges plus the fractional part of steps/500 times the difference to the median
    region that posted one more.  -> (seconds, detail dict)"""
    walls = np.asarray(walls, dtype=np.float64)
    posts = np.asarray(posts, dtype=np.int64)
    per = steps / EPISODE if has_exchange else 0.0
    lo = int(np.floor(per))
    frac = per - lo
    detail = {"exchanges_per_region": round(per, 4)}
    if not has_exchange or frac == 0.0 or not (posts == lo + 1).any() or not (posts == lo).any():
        sel = walls if not has_exchange or frac == 0.0 else walls[posts == (lo if (posts == lo).any() else lo + 1)]
        if has_exchange and frac != 0.0:
            detail["note"] = "only one kind of region was sampled: no exchange share could be charged"
        return float(np.median(sel)), detail
    t_lo, t_hi = float(np.median(walls[posts == lo])), float(np.median(walls[posts == lo + 1]))
    detail.update({"median_region_ms_without_extra_exchange": round(t_lo * 1e3, 4),
                   "median_region_ms_with_extra_exchange": round(t_hi * 1e3, 4),
                   "regions_with_extra_exchange": int((posts == lo + 1).sum()),
                   "exchange_share_ms_per_region": round(frac * (t_hi - t_lo) * 1e3, 5)})
    return t_lo + frac * (t_hi - t_lo), detail


def run_benchmark(args, engine, rank, local_rank, world, dist):
    """The benchmark on one rank; rank 0 returns the result dict (and main() prints it), the others None."""
    import torch
    n = args.envs_per_gpu
    n_total = n * world
    shard = engine.make_shard(n, rank * n)
    tdev = engine.tensor_device

    def all_ranks_ok(ok):
        if dist is None:
            return ok
        flag = torch.tensor([1.0 if ok else 0.0], device=tdev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        return bool(flag.item() > 0.5)

    def max_over_ranks(values):
        if dist is None:
            return list(values)
        t = torch.tensor(list(values), dtype=torch.float64, device=tdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t.tolist()

    # ---- the one exchange step of the path: after every episode (500 steps) the last
    # finished return of every env is all-gathered - copy enqueued on the engine's stream, collective on a side
    # stream.  Issued by the C++ host (rq_comm_* / rq_allgather_returns: RCCL bound by libraptor_quad.so itself);
    # torch.distributed only ships the communicator id, provides the barriers and the max over ranks.  Two-phase
    # consensus: should the native communicator not come up on EVERY rank, every rank takes the torch-side
    # exchange (same structure) and the JSON says so - no rank is left waiting in a collective the others skipped.
    want_native = world > 1 or args.force_native_exchange
    exchange, why = None, "single rank"
    if want_native:
        why = ""
        try:      # phase 1 (no collective inside): can every rank bind RCCL?  rank 0's id is the one that is used
            ident = [engine.native_unique_id()]
        except Exception as exc:      # noqa: BLE001
            ident, why = [None], f"rank {rank}: {exc}"
        native = all_ranks_ok(ident[0] is not None)
        if native:
            if dist is not None:
                dist.broadcast_object_list(ident, src=0)
            try:  # phase 2: the collective communicator creation
                exchange = engine.native_exchange(world, rank, ident[0])
            except Exception as exc:  # noqa: BLE001
                exchange, why = None, f"rank {rank}: {exc}"
            native = all_ranks_ok(exchange is not None)
        if not native:
            if dist is not None:      # every rank reports the same reason: the first failing rank's
                reasons = [None] * world
                dist.all_gather_object(reasons, why)
                why = next((r for r in reasons if r), "another rank failed")
            exchange = engine.torch_exchange(n, n_total, why or "another rank failed")
    exchange_kind = exchange.kind if exchange is not None else "none (one rank: nothing to gather)"

    def gather_objects(obj):
        if dist is None:
            return [obj]
        out = [None] * world
        dist.all_gather_object(out, obj)
        return out

    # What the communicator says about itself, rank by rank (round 5): a record of an N-rank run must show that the
    # library that moved the data saw N ranks on N different GPUs - asked of RCCL, not echoed from this script's arguments.
    rccl = None
    if exchange is not None:
        mine = exchange.describe()
        everyone = gather_objects(mine)
        rccl = {"ranks": mine["ranks"], "version": mine["version"], "version_code": mine["version_code"],
                "library_path": mine["library_path"],
                "per_rank": [{k: d[k] for k in ("rank", "ranks", "device", "pci_bus_id")} for d in everyone]}
        bad = [d for r, d in enumerate(everyone) if d["ranks"] != world or d["rank"] != r]
        if bad:
            raise RuntimeError(f"the communicator does not span this job: {world} ranks launched, it reports {everyone}")
        buses = [d["pci_bus_id"] for d in everyone if d["pci_bus_id"]]
        rccl["distinct_gpus"] = len(set(buses)) if buses else None

    def verify_layout(sh, ex, n_envs):
        """The all-gather's result against every rank's OWN finished returns (round 5): block r of what this rank received
        must be what rank r sent - checked through a CRC every rank computes of its local returns and ships beside the data
        (all_gather_object) - and this rank's block must equal its local returns element for element.  Called right after an
        episode whose exchange was the last thing enqueued.  -> (ok on every rank, detail)"""
        import zlib
        got = ex.result()
        local = np.ascontiguousarray(engine.local_returns(sh), dtype=np.float32)
        sums = gather_objects((rank, zlib.crc32(local.tobytes()), int(local.size)))
        ok = got is not None and int(np.prod(np.shape(got))) == world * n_envs
        blocks_ok = 0
        if ok:
            got = np.ascontiguousarray(got, dtype=np.float32).reshape(-1)
            for r, crc, size in sums:
                blocks_ok += int(size == n_envs and zlib.crc32(got[r * n_envs:(r + 1) * n_envs].tobytes()) == crc)
            ok = blocks_ok == world and bool(np.array_equal(got[rank * n_envs:(rank + 1) * n_envs], local))
        everywhere = all_ranks_ok(ok)
        return everywhere, {"envs_per_rank": n_envs, "blocks_checked": world, "blocks_matching_their_rank_on_rank0": blocks_ok,
                            "nonzero_returns_on_rank0": int(np.count_nonzero(local)),
                            "method": "crc32 of every rank's local finished returns (all_gather_object) against the block the "
                                      "all-gather put at that rank's offset, on every rank; own block compared element-wise"}

    # The exchange belongs to the EPISODE (500 steps of simulated time), not to a rollout call: a region shorter
    # than an episode posts one all-gather every 500 steps across regions (a 20-step region: one in 25).
    since_exchange = [0]

    def run(plan, sh=None, ex=None):
        sh = shard if sh is None else sh
        ex = exchange if ex is None else ex
        posted = 0
        for c in plan:
            sh.rollout(c, args.mode)
            since_exchange[0] += c
            if since_exchange[0] >= EPISODE:
                since_exchange[0] -= EPISODE
                if ex is not None:
                    ex.post(sh)
                    posted += 1
        return posted

    def finish(ex=None):
        ex = exchange if ex is None else ex
        if ex is not None:
            ex.finish()

    def sync_all():
        engine.synchronize()
        if dist is not None:
            dist.barrier()

    def timed_region(plan, sh=None, ex=None):
        """exactly sum(plan) steps, barrier + synchronize before, synchronize + barrier after -> (wall seconds, posts)"""
        sync_all()
        t0 = time.perf_counter()
        posted = run(plan, sh, ex)
        finish(ex)
        engine.synchronize()
        wall = time.perf_counter() - t0              # this rank's clock stops when ITS work is done: the max over
        if dist is not None:                         # ranks is taken afterwards, so the closing barrier is not timed
            dist.barrier()
        return wall, posted

    probe_clock = [None]

    def kernel_probe_ms(plan, repetitions, sh=None, ex=None, stride=1):
        """Average duration (ms) of one rollout launch of the kind `plan` ends with.  Fused mode: regions exactly like the
        timed ones (barrier + synchronize on both sides) are run again with kernel-level timing on
        (rq_device_set_rollout_timing: every wave records the wall-clock tick at which it came in and went out and the
        core-clock cycles of its steps; the duration is first-wave-in to last-wave-out on one die), and the records of every
        `stride`-th region's launch are read back.  Against rocprofv3's per-dispatch duration of the same launches the span
        reads ~2.6 us short (63.3 against 65.9 us in the profiled run of the driver's command: the profiler's clock runs from
        the command processor taking the dispatch to the release of the kernel's writes; `roofline.rocprofv3` carries its
        figure).  Why only every stride-th: the chip's core clock follows its load averaged over about a millisecond
        (tools/idle_clock.py: 2.37 GHz with the ~15 us between two timed regions, 2.07 GHz behind 5 ms of idling, and many
        launches to come back), and a read-back after EVERY launch - a copy, a synchronize, host arithmetic: ~50-100 us of
        idle chip - lowered the clock of the launches it was timing (2.25 GHz, 65.4 us for the 20-step launch that takes
        62.3 us inside a timed region).  Regions between two read-backs keep the timed regions' own cadence.  The stride is
        one more than the regions of an episode, so the samples walk through the episode's phases: every env's episode
        started together, so every 500 steps the whole batch resets at once and the launches right after it run ~10 %
        longer than those late in the episode.  Chained mode: HIP events around a region, per step."""
        out, clocks = [], []
        sync_all()
        if args.mode == "fused":
            engine.set_rollout_timing(True)
            for k in range(repetitions * stride):
                timed_region(plan, sh, ex)
                if (k + 1) % stride == 0:
                    out.append(engine.last_rollout_ms())
                    clocks.append(engine.last_rollout_clock_ghz())
            engine.set_rollout_timing(False)
        else:
            for _ in range(repetitions):
                sync_all()
                engine.timer_start()
                run(plan, sh, ex)
                out.append(engine.timer_stop() / sum(plan))
                finish(ex)
        sync_all()
        if os.environ.get("RQ_BENCH_DEBUG"):
            print("kernel_probe_ms", sum(plan), [round(x * 1e3, 1) for x in out], file=sys.stderr)
        probe_clock[0] = float(np.mean(clocks)) if clocks else None       # core clock of the launches just timed
        return float(np.mean(out)) if args.mode == "fused" else float(np.median(out))

    # ---- the chip's clocks first: a region that follows an idle chip runs its first milliseconds at a lower clock (the first of
    # 2000-step regions read 6.3 ms against a 5.7 ms median), so 500-step rollouts of a scratch shard of the same size run for
    # CLOCK_WARMUP_SECONDS.  It has state of its own: the benchmarked shard still sees exactly 1 + --warmup steps before its
    # timed ones ----
    scratch, t_end = engine.make_shard(n, rank * n), time.perf_counter() + CLOCK_WARMUP_SECONDS
    while time.perf_counter() < t_end:
        scratch.rollout(EPISODE, args.mode)
        engine.synchronize()
    del scratch

    # ---- warm-up: one-off costs first (RCCL communicator, first barrier, lazy allocations), then EXACTLY
    # --warmup untimed steps of the same rollout ----
    run([1])
    finish()
    sync_all()
    if args.warmup > 0:
        run(chunks(args.warmup, EPISODE))
        finish()

    # ---- the headline: ONE timed region of exactly --steps steps (barrier + synchronize on both sides, max over ranks) ----
    plan = chunks(args.steps, EPISODE)
    wall, posted = timed_region(plan)
    elapsed = max_over_ranks([wall])[0]
    if args.dump_outputs and rank == 0:            # what the last timed step left, before anything else touches the shard
        write_outputs(args.dump_outputs, engine.outputs(shard))
    value = n_total * args.steps / elapsed
    result = {
        "metric": f"env-steps/sec (whole node) at {n} quadrotors per GPU",
        "value": round(value, 1), "unit": "env-steps/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 6),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": {"fp32": "f32", "bf16": "bf16 actor operands (fp32 accumulate) + f32 dynamics",
                  "f16x2": "actor operands as two f16 pieces each (22 significand bits, fp32 accumulate) + f32 dynamics"
                  }[args.precision],
        "data": "synthetic",
        "config": {"workload": f"{n} parallel quadrotors per GPU, fp32 RK4 dynamics + {args.precision} GRU actor "
                               f"(RAPTOR checkpoint), domain-randomised params, auto-reset, {args.mode} rollout",
                   "envs_per_gpu": n, "total_envs": n_total, "episode_length": EPISODE,
                   "parallelism": f"env-sharded x{world}, all-gather of returns per episode" if world > 1
                                  else "single GPU", "mode": args.mode, "engine": engine.name, **engine.describe(),
                   "exchange": exchange_kind},
        "timing": {"repetitions": 1, "steps_per_region": args.steps,
                   "statistic": "one region of exactly --steps steps, barrier + synchronize on both sides, max over ranks",
                   "region_ms": {"charged": round(elapsed * 1e3, 4)}, "exchanges_in_region": posted,
                   "untimed_steps_before_first_region": args.warmup + 1},
    }
    if rccl is not None:
        result["config"]["rccl"] = rccl
    if not args.full:
        return result if rank == 0 else None

    # ---- --full: timed regions of exactly --steps steps each, repeated (module docstring) ----
    per_region = args.steps / EPISODE if exchange is not None else 0.0
    fractional = per_region != int(per_region)
    walls, posts = [], []
    while True:
        w, p = timed_region(plan)
        walls.append(w)
        posts.append(p)
        total = max_over_ranks([sum(walls)])[0]      # every rank must take the same decision: the slowest rank's clock decides
        enough = len(walls) >= MIN_REPETITIONS and total >= MIN_TIMED_SECONDS
        if enough and fractional:                    # the regions that carry the exchange must have been sampled
            enough = sum(1 for q in posts if q > int(per_region)) >= 3
        if len(walls) >= MAX_REPETITIONS or enough:
            break
    walls = max_over_ranks(walls)                    # max over ranks, region by region
    rep_elapsed, share = effective_region(walls, posts, args.steps, exchange is not None)
    # one rollout launch of the region's kind; fused: whole episode periods of regions (at least 2, ~0.2 s at most)
    periods = max(1, int(np.ceil(EPISODE / max(args.steps, 1)))) if args.steps < EPISODE else 1
    # fused: samples spread over the phases of an episode (two per phase, at most 60), `stride` regions apart
    samples = min(2 * periods, 60)
    stride = periods + max(1, periods // samples)
    launch_ms = kernel_probe_ms(plan, samples if args.mode == "fused" else min(len(walls), 50), stride=stride)
    launch_clock_ghz = probe_clock[0]
    # the same launch between two HIP events on the engine's stream (torch's events would see torch's stream only): regions like the
    # timed ones, every one bracketed; the events add their own ~2 us of stream work to what they measure
    event_launch_ms = None
    if args.mode == "fused" and hasattr(engine, "timer_start"):
        ev = []
        for _ in range(min(max(samples, 20), 60)):
            sync_all()
            engine.timer_start()
            run(plan)
            ev.append(engine.timer_stop() / len(plan))
            finish()
        sync_all()
        event_launch_ms = float(np.mean(ev))

    flop_step = FLOP_PER_ENV_STEP if args.precision == "fp32" else FLOP_GATES + FLOP_ENV

    def long_launches(sh, ex, n_envs, launches, label):
        """`launches` x 500-step launches back to back per region (clocks warm): three regions, each timed on the wall
        clock (barrier + synchronize on both sides, max over ranks) WITH kernel-level timing on, the kernel span read off
        each region's last launch after the clock stopped - wall and kernel figures describe the same regions (round 3
        took them from different ones, and the record showed a kernel time above the wall time) -> dict"""
        ss_plan = [EPISODE] * launches
        run(ss_plan, sh, ex)                         # untimed: the clocks reach their steady state
        finish(ex)
        walls3, spans3, clocks3 = [], [], []
        if args.mode == "fused":
            engine.set_rollout_timing(True)
        for _ in range(3):
            w, _ = timed_region(ss_plan, sh, ex)
            walls3.append(w)
            spans3.append(engine.last_rollout_ms() if args.mode == "fused" else w * 1e3 / launches)
            if args.mode == "fused":
                clocks3.append(engine.last_rollout_clock_ghz())
        engine.set_rollout_timing(False)
        ss_wall = float(np.median(max_over_ranks(walls3)))
        ss_kernel_ms = float(np.mean(spans3)) * len(ss_plan)
        ss_steps = sum(ss_plan)
        ss_flops = flop_step * n_envs * ss_steps / (ss_kernel_ms * 1e-3) / 1e12
        ss_clock = float(np.mean(clocks3)) if clocks3 else None
        at_clock = {} if not ss_clock else {
            "clock_ghz_under_load": round(ss_clock, 3),
            "frac_of_peak_at_that_clock": round(ss_flops / (PEAK_FP32_TFLOPS * ss_clock / 2.4), 4)}
        return {**at_clock, "launches": len(ss_plan), "steps_per_launch": EPISODE, "envs_per_gpu": n_envs, "regions": 3,
                "env_steps_per_s": round(n_envs * world * ss_steps / ss_wall, 1),
                "us_per_step_wall": round(ss_wall / ss_steps * 1e6, 4),
                "us_per_step_kernel": round(ss_kernel_ms / ss_steps * 1e3, 4),
                "avg_launch_ms": round(ss_kernel_ms / len(ss_plan), 4),
                "kernel": fused_kernel_name(args.precision, n_envs, EPISODE),
                "achieved_TFLOPs": round(ss_flops, 3), "peak_TFLOPs": PEAK_FP32_TFLOPS,
                "frac": round(ss_flops / PEAK_FP32_TFLOPS, 4), "exchanges": launches if ex is not None else 0,
                "note": label}

    # ---- steady state: 10 x 500-step launches back to back (clocks are warm now), one region ----
    steady = None
    if args.mode == "fused":
        steady = long_launches(shard, exchange, n, 10,
                               "same process, after the timed regions and 10 untimed launches of the same kind; three regions: wall = "
                               "median region (barrier + synchronize on both sides, max over ranks, one all-gather per launch when "
                               "there is more than one rank); kernel = first-wave-in / last-wave-out span of the last launch of each "
                               "of the SAME three regions (mean), on rank 0")

    # ---- the gather's layout, checked once per run BEFORE a value may be printed: one whole episode, its exchange the last
    # thing enqueued, then block r of the result against rank r's own returns on every rank ----
    exchange_verified, exchange_check = None, None
    if exchange is not None:
        since_exchange[0] = 0
        run([EPISODE])
        finish()
        sync_all()
        exchange_verified, exchange_check = verify_layout(shard, exchange, n)
        if not exchange_verified:
            raise RuntimeError(f"the all-gathered returns are not the ranks' returns in global env order: {exchange_check}")

    # the last all-gathered returns (numpy [world * n]); one rank: the env's own
    gathered = exchange.result() if exchange is not None else None
    if gathered is None:
        gathered = engine.local_returns(shard)
    gathered_count = int(np.prod(np.shape(gathered)))

    # ---- BASELINE config 3 / 4: 262 144 envs per GPU (2 097 152 on 8 GPUs), one all-gather per 500-step launch ----
    config4 = None
    if args.mode == "fused" and not args.no_config4:
        n4 = 262144
        shard4 = engine.make_shard(n4, rank * n4)
        ex4 = exchange
        if isinstance(exchange, _TorchExchange) or (exchange is not None and not hasattr(exchange, "ex")):
            ex4 = engine.torch_exchange(n4, n4 * world, why)     # torch-side buffers are sized per shard
        since_exchange[0] = 0
        config4 = long_launches(shard4, ex4, n4, 4,
                                "BASELINE config 3 (one GPU) / config 4 (262 144 envs on each of N GPUs, all-gather of returns per "
                                "episode): 4 x 500-step launches per region, three regions after 4 untimed launches, same process; "
                                "wall and kernel from the same regions")
        config4["total_envs"] = n4 * world
        if ex4 is not None:            # the same check at this shard size (the communicator's buffers were re-sized for it)
            since_exchange[0] = 0
            run([EPISODE], shard4, ex4)
            finish(ex4)
            sync_all()
            ok4, check4 = verify_layout(shard4, ex4, n4)
            if not ok4:
                raise RuntimeError(f"config 4: the all-gathered returns are not the ranks' returns in global env order: {check4}")
            config4["exchange_verified"] = ok4
        del shard4

    result["timing"]["repeated_regions"] = {
        "repetitions": len(walls), "steps_per_region": args.steps,
        "statistic": "median region without an exchange + steps/500 of the difference to the median region with one"
                     if exchange is not None else "median",
        "region_ms": {"first": round(walls[0] * 1e3, 4), "min": round(min(walls) * 1e3, 4),
                      "median": round(float(np.median(walls)) * 1e3, 4),
                      "mean": round(float(np.mean(walls)) * 1e3, 4),
                      "max": round(max(walls) * 1e3, 4), "charged": round(rep_elapsed * 1e3, 4)},
        "exchange_share": share,
        "value": round(n_total * args.steps / rep_elapsed, 1), "ms_per_step": round(rep_elapsed / args.steps * 1e3, 6)}
    if steady is not None:
        result["steady_state"] = steady
    if config4 is not None:
        result["config4"] = config4
    if rank != 0:
        return None

    launches = len(plan) if args.mode == "fused" else 3 * args.steps
    avg_launch_s = launch_ms * 1e-3                  # one rollout launch (median over the timed regions)
    if args.mode == "fused" and args.precision in ("bf16", "f16x2"):
        steps_per_launch = args.steps / len(plan)
        result["roofline"] = sixteen_bit_roofline(args.precision, n, steps_per_launch, avg_launch_s)
        result["roofline"]["launches"] = launches
    elif args.mode == "fused":
        steps_per_launch = args.steps / len(plan)
        flop_per_launch = FLOP_PER_ENV_STEP * n * steps_per_launch
        achieved = flop_per_launch / avg_launch_s / 1e12
        kname = fused_kernel_name("fp32", n, steps_per_launch)
        tr = pmc_traffic(kname, n, library_sha256())
        result["roofline"] = {
            "kernel": kname, "bound": "mfma", "achieved": round(achieved, 3),
            "peak": PEAK_FP32_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / PEAK_FP32_TFLOPS, 4),
            "traffic": traffic_of(tr),
            "traffic_source": tr,
            "note": "compute-bound: state, hidden and constants stay in VGPRs for the whole launch; "
                    f"algorithmic {FLOP_PER_ENV_STEP} FLOP/env-step (actor {FLOP_ACTOR} + gates {FLOP_GATES} + "
                    f"env {FLOP_ENV}) against the fp32 vector = f32-MFMA dense peak; algorithmic HBM bytes are "
                    f"{BYTES_FUSED_LAUNCH} B/env per launch of {int(steps_per_launch)} steps; the measured `traffic` adds "
                    "the operand image every wave loads and the loop-invariant registers parked in scratch before "
                    "the loop - a few bytes per env-step, HBM idle; `frac_basis` says which clock avg_launch_ms is on: the committed "
                    "rocprofv3 trace of this command when there is one (then `wave_span` holds this run's own first-wave-in / "
                    "last-wave-out span, ~2.6 us shorter per launch), else that span; short launches carry the "
                    "kernel's prologue and epilogue (see steady_state for 500-step launches); the north-star's "
                    "'>= 60 % of the HBM roofline on the step kernel' is kernels.n2097152.k_step (HBM-bound there; at "
                    "65 536 envs the API-granular kernels are launch-latency-bound on Infinity-Cache-resident data)",
            "avg_launch_ms": round(avg_launch_s * 1e3, 4), "launches": launches,
            "steps_per_launch": steps_per_launch,
            "hbm_bytes_per_env_step": round(BYTES_FUSED_LAUNCH / steps_per_launch, 3),
            "sq_counters": sq_profile("fp32")}
        # ---- which clock the headline fraction is on (round 6: a record that cannot go stale) ----
        # Three measurements of THIS run, flat so that the driver's `parsed` keeps them:
        #   frac_in_run / avg_launch_ms_in_run       the kernel's own first-wave-in -> last-wave-out span (per-wave records)
        #   frac_hip_events / avg_launch_ms_hip_events  HIP events on the engine's stream around the region's launch
        #   frac_by_region                            the same flops over the timed region itself (= over ms_per_step x steps)
        # and one from profiles/: rocprofv3's per-dispatch duration of this kernel in the timed regions of this same command.  The
        # committed trace is the headline ONLY when it was taken from the very build loaded now (sha256 of the library recorded at
        # profile time) - then a reader can recompute `frac` from profiles/ - otherwise the headline is this run's own span and
        # `frac_basis` says why.  Rounds 1-5 matched the trace by kernel name, so a changed kernel kept an old fraction.
        rl = result["roofline"]
        rl["avg_launch_ms_in_run"] = round(avg_launch_s * 1e3, 4)
        rl["frac_in_run"] = round(achieved / PEAK_FP32_TFLOPS, 4)
        region_s = rep_elapsed / len(plan)
        rl["frac_by_region"] = round(flop_per_launch / region_s / 1e12 / PEAK_FP32_TFLOPS, 4)
        if event_launch_ms:
            rl["avg_launch_ms_hip_events"] = round(event_launch_ms, 4)
            rl["frac_hip_events"] = round(flop_per_launch / (event_launch_ms * 1e-3) / 1e12 / PEAK_FP32_TFLOPS, 4)
        lib_hash = library_sha256() if engine.name == "hip" else None
        rl["library_sha256"] = lib_hash
        rp, why_not = (rocprof_launch_stats(kname, n, args.steps, lib_hash) if launches == 1 and lib_hash
                       else (None, "not the one-launch-per-region command the committed traces are of"))
        rl["frac_basis"] = f"wave span measured in this run ({why_not})"
        if rp:
            rp_flops = flop_step * n * steps_per_launch / (rp["mean_us"] * 1e-6) / 1e12
            gap_us = rp["mean_us"] - avg_launch_s * 1e6
            rl["wave_span"] = {"avg_launch_ms": round(avg_launch_s * 1e3, 4), "achieved": round(achieved, 3),
                               "frac": round(achieved / PEAK_FP32_TFLOPS, 4),
                               "method": "rq_device_set_rollout_timing: first wave in -> last wave out on one die, "
                                         "mean over launches of this run's own regions",
                               "rocprofv3_mean_minus_wave_span_us": round(gap_us, 2)}
            rl["rocprofv3"] = rp
            # the profiler's clock also counts the dispatch and the end-of-kernel release: 2 - 5 us more than the waves' own span
            # (measured 2.6 - 3.3).  Outside that window the trace and this run disagree about the kernel and the trace is not used.
            if 0.0 <= gap_us <= 8.0:
                rl.update({"achieved": round(rp_flops, 3), "frac": round(rp_flops / PEAK_FP32_TFLOPS, 4),
                           "avg_launch_ms": round(rp["mean_us"] * 1e-3, 4),
                           "frac_basis": f"rocprofv3 --kernel-trace of this command on this build (library sha256 {lib_hash[:12]}...), "
                                         f"profiles/{rp['source']}: mean End - Start of {rp['launches']} timed-region launches of this kernel; "
                                         f"this run's own span reads {gap_us:.1f} us less (frac_in_run)"})
            else:
                rl["frac_basis"] = (f"wave span measured in this run (profiles/{rp['source']} is of this build but reads {gap_us:.1f} us "
                                    "away from this run's span: outside the 0 - 8 us the profiler's dispatch-to-release clock explains)")
        if launch_clock_ghz:
            # the peak assumes 2.4 GHz.  The clock these launches really ran their steps at (rq_device_last_rollout_clock:
            # shader-clock cycles over constant-rate ticks, median wave, mean over the probed launches): a launch that
            # follows an idle gap - every timed region does - runs its first ~30 us at ~2.0 GHz and reaches ~2.38 GHz
            # after ~60 us, so a 20-step launch averages ~2.2 GHz where back-to-back 500-step launches hold ~2.36
            # (tools/wave_timeline.py).  That share of the shortfall is the power management's, not the kernel's.
            # (Round 3 / early round 4 printed the clock of the PROFILED launch here, GRBM_GUI_ACTIVE / duration = 2.12-2.16:
            # counter collection itself slows the chip; it is kept as sq_counters.clock_ghz_under_profiler.)
            result["roofline"]["clock_ghz_under_load"] = round(launch_clock_ghz, 3)
            result["roofline"]["frac_of_peak_at_that_clock"] = round(result["roofline"]["achieved"] / (PEAK_FP32_TFLOPS * launch_clock_ghz / 2.4), 4)
    else:
        # round 3: two launches per step - k_step also writes the next step's observation (104 B/env) from the state it
        # holds in registers, so the chain no longer re-reads the state for a k_observe launch
        bytes_obs_write = 4 * 26
        bytes_per_step = (BYTES_ACTOR + BYTES_STEP + bytes_obs_write) * n
        achieved = bytes_per_step / (launch_ms * 1e-3) / 1e9
        result["roofline"] = {
            "kernel": "k_actor_step+k_step (chain, observation assembled by the step)", "bound": "hbm",
            "achieved": round(achieved, 1), "peak": PEAK_HBM_GBPS, "unit": "GB/s", "frac": round(achieved / PEAK_HBM_GBPS, 4),
            "traffic": None, "launches": 2 * args.steps,
            "note": f"algorithmic {BYTES_ACTOR}+{BYTES_STEP}+{bytes_obs_write} B/env-step; launch-latency-bound at 65 536 envs "
                    "(Infinity-Cache-resident working set), see `kernels`"}
    if world == 1 and not args.no_kernel_probe and engine.name == "hip":
        device = engine.device
        result["kernels"] = {"n65536": kernel_probe(device, ENVS_PER_GPU, 50),
                             "n2097152": kernel_probe(device, 2097152, 5)}
        result["extensions_n65536"] = extension_probe(device, ENVS_PER_GPU)
        result["extensions_n65536"]["teacher_bank"] = teacher_probe(device, ENVS_PER_GPU)
        result["dagger_epoch"] = dagger_epoch_probe(device)
        try:       # needs an RCCL to bind (librccl of the process or of ROCm): absent -> the reason, not a failed benchmark
            result["native_exchange_1rank"] = {f"n{m}": native_exchange_probe(engine, m) for m in (ENVS_PER_GPU, 262144)}
            result["native_exchange_1rank"]["rccl"] = result["native_exchange_1rank"][f"n{ENVS_PER_GPU}"]["rccl"]
            result["native_exchange_1rank"]["note"] = (
                "rq_allgather_returns + rq_comm_gathered on the real librccl with ONE rank, posted after every 500-step "
                "launch with the next launch enqueued behind it: the host-side and stream-ordering cost every rank of an N-GPU "
                "run pays per episode (copy, events, ncclAllGather call, completion); the xGMI transfer of N x 4 B x envs is "
                "what a multi-GPU node adds on top (256 KiB per rank at 65 536 envs: ~2 us per hop at 153 GB/s per link)")
        except Exception as exc:      # noqa: BLE001
            result["native_exchange_1rank"] = {"unavailable": str(exc)}
        result["readme_loop_n8"] = api_loop_probe(device)
        result["policy_alone_n1"] = policy_alone_probe(device)
        result["readme_loop_n65536_pcie_inclusive"] = api_loop_probe(device, ENVS_PER_GPU, 20)
    if world == 1 and engine.name == "hip":
        result["parity"] = parity_block(engine.device)
    if world == 1 and not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline(args.cpu_seconds)
    result["config"]["exchanges_per_timed_region"] = round(args.steps / EPISODE, 4) if exchange is not None else 0
    result["config"]["gathered_returns"] = gathered_count
    result["config"]["exchange_verified"] = exchange_verified
    if exchange_check is not None:
        result["config"]["exchange_check"] = exchange_check
    if rccl is None and isinstance(result.get("native_exchange_1rank"), dict) and "rccl" in result["native_exchange_1rank"]:
        # one rank and nothing to gather in the timed regions: the 1-rank communicator of the `native_exchange_1rank` block
        # is the one RCCL this process met - its own account of itself (ranks == 1 from ncclCommCount)
        result["config"]["rccl"] = result["native_exchange_1rank"]["rccl"]
    return result


def engine_device_count(spec):
    """GPUs this node offers the engine `spec` ('hip': rq_device_count of libraptor_quad.so - the HIP runtime's own
    count, no torch involved; a stand-in module: its device_count())."""
    if spec == "hip":
        from raptor_amd import _lib
        import ctypes
        count = ctypes.c_int(0)
        _lib.check(_lib.load().rq_device_count(ctypes.byref(count)))
        return int(count.value)
    import importlib
    return int(importlib.import_module(spec).device_count())


def spawn_local_ranks(args, argv):
    """`python bench.py --gpus N` with N > 1 and no launcher around it (no RANK in the environment): this process
    becomes the launcher - N copies of the same command line, one rank per GPU of this node (RANK = LOCAL_RANK = 0 ..
    N-1, WORLD_SIZE = N, rendezvous on 127.0.0.1 at a free port), what `python -m torch.distributed.run --nnodes=1
    --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N ...` does.  Rank 0 inherits this process's stdout,
    so its ONE JSON line stays the last line of stdout; the other ranks' stdout (RCCL / gloo banners) is sent to
    stderr.  Any rank dying takes the job down (the others are killed by PID) and the exit status is non-zero.
    More ranks than GPUs is an error, not a fallback - except under RQ_BENCH_DEVICE (tests: every rank on one
    device).  -> exit status"""
    import socket
    import subprocess
    n = args.gpus
    have = engine_device_count(args.engine)
    if "RQ_BENCH_DEVICE" not in os.environ and not args.allow_oversubscribe and n > have:
        raise SystemExit(f"bench.py --gpus {n}: this node has {have} GPU(s) (engine '{args.engine}'); there is no "
                         "fallback to fewer ranks")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, os.path.abspath(__file__)] + list(sys.argv[1:] if argv is None else argv)
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen(cmd, env=env, stdout=None if r == 0 else sys.stderr))
    status, alive = 0, set(range(n))
    import signal

    def stop(signum, _frame):          # the launcher being told to stop (a driver's timeout) takes its ranks along
        raise SystemExit(128 + signum)
    signal.signal(signal.SIGTERM, stop)
    try:
        while alive:
            for r in sorted(alive):
                rc = procs[r].poll()
                if rc is None:
                    continue
                alive.discard(r)
                if rc != 0 and status == 0:
                    status = rc if rc > 0 else 1
                    print(f"bench.py: rank {r} exited with status {rc}; stopping the other ranks", file=sys.stderr)
                    for q in alive:
                        procs[q].terminate()
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return status


def main(argv=None):
    args = parse_args(argv)
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if "RANK" not in os.environ and args.gpus > 1:
        sys.exit(spawn_local_ranks(args, argv))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: one rank per GPU (launch with "
                         f"`python bench.py --gpus {args.gpus}` or torch.distributed.run --nproc-per-node {args.gpus})")
    engine = make_engine(args.engine, local_rank, args)
    dist = None
    if world > 1 or "RANK" in os.environ:      # launched by torch.distributed.run (also with one rank)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        oversubscribed = args.allow_oversubscribe and engine.name == "hip" and world > engine_device_count(args.engine)
        engine.init_process_group(dist, args.backend or ("gloo" if oversubscribed else engine.default_backend))
    try:
        result = run_benchmark(args, engine, rank, local_rank, world, dist)
        if rank == 0 and args.allow_oversubscribe:
            result["config"]["oversubscribed"] = (f"{world} ranks on {engine_device_count(args.engine)} GPU(s): a test of the orchestration, "
                                                  "not a measurement")
        if rank == 0:
            # RCCL / the HIP runtime print banners through C stdio, which a redirected stdout only flushes at exit:
            # push them out now so that the JSON line is the LAST line of stdout
            import ctypes
            sys.stdout.flush()
            ctypes.CDLL(None).fflush(None)
            print(json.dumps(result), flush=True)
    finally:
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
