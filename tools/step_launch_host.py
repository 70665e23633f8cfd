#!/usr/bin/env python3
"""What the host side of the chained step's launches costs, one build against another -> profiles/step_launch_host.json.
    python tools/step_launch_host.py --parent PATH/libraptor_quad.so [--rounds 5] [--json profiles/step_launch_host.json]
    python tools/step_launch_host.py --one          # the figures of the library in use (RAPTOR_QUAD_LIB), one JSON line
The kernels of the two builds are the same machine code (tools/kernel_listing_diff.py), so only the host can differ, and it shows
where launches are the bound.  Per round and build, in a process of its own, the two builds alternating:
    readme_loop_8_us, readme_loop_8_launches_us   one iteration of the README loop (README.md:96-99) at 8 envs, NumPy arrays across
                                                  the boundary, as shipped (resident executor) and as plain launches (rq_step's two
                                                  launches with the speculated policy step, evaluate_step's hit)
    k_observe_us, k_actor_step_us, k_step_us      bench.py's per-launch figures at 65 536 envs (kernel_probe: HIP events)
    chained_64_us_per_step, chained_65536_us_per_step   a chained auto-reset rollout, wall time through a device synchronise
Medians per build; the check: each median of the new build is no slower than the parent's own slowest round of that figure.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def readme_loop_us(device, resident, iters=3000, warm=500):
    import numpy as np
    import raptor_amd.l2f as l2f
    from raptor_amd.foundation_policy import Raptor
    device.set_resident(resident)
    vector = l2f.vector(8)
    rng, env = vector.VectorRng(), vector.VectorEnvironment()
    params, state, next_state = vector.VectorParameters(), vector.VectorState(), vector.VectorState()
    vector.initialize_rng(device, rng, 0)
    vector.initialize_environment(device, env)
    vector.sample_initial_parameters(device, env, params, rng)
    vector.sample_initial_state(device, env, params, state, rng)
    policy = Raptor(device)
    policy.reset()
    obs = np.zeros((8, env.OBSERVATION_DIM), np.float32)
    t0 = 0.0
    for it in range(iters + warm):
        if it == warm:
            t0 = time.perf_counter()
        vector.observe(device, env, params, state, obs, rng)
        action = policy.evaluate_step(obs[:, :22])
        vector.step(device, env, params, state, action, next_state, rng)
        state.assign(next_state)
    us = (time.perf_counter() - t0) / iters * 1e6
    device.set_resident(True)
    return us


def chained_us_per_step(device, n, steps, reps):
    import bench
    sh = bench.Shard(device, n, 0)
    sh.rollout(steps, "chained")
    device.synchronize()
    per = []
    for _ in range(reps):
        t0 = time.perf_counter()
        sh.rollout(steps, "chained")
        device.synchronize()
        per.append((time.perf_counter() - t0) / steps * 1e6)
    return statistics.median(per)


def one():
    import bench
    import raptor_amd.l2f as l2f
    from raptor_amd import build as rq_build
    from raptor_amd import _lib
    device = l2f.Device()
    out = {"library_sha256": rq_build.library_sha256(_lib.LIB_PATH)}
    out["readme_loop_8_us"] = readme_loop_us(device, True)
    out["readme_loop_8_launches_us"] = readme_loop_us(device, False)
    for name, rec in bench.kernel_probe(device, 65536, 50).items():
        out[name + "_us"] = rec["us_per_launch"]
    out["chained_64_us_per_step"] = chained_us_per_step(device, 64, 500, 7)
    out["chained_65536_us_per_step"] = chained_us_per_step(device, 65536, 100, 7)
    print("STEP_LAUNCH_HOST " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "step_launch_host.json"))
    a = ap.parse_args()
    if a.one:
        return one()
    if not a.parent:
        ap.error("--parent: the library to compare with")
    builds = {"parent": os.path.abspath(a.parent), "new": os.path.join(ROOT, "raptor_amd", "libraptor_quad.so")}
    rounds = {k: [] for k in builds}
    for r in range(a.rounds):
        for name in (("parent", "new") if r % 2 == 0 else ("new", "parent")):      # alternating, and who goes first too
            env = dict(os.environ, RAPTOR_QUAD_LIB=builds[name])
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one"], env=env, capture_output=True, text=True, timeout=300)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("STEP_LAUNCH_HOST ")]
            if p.returncode != 0 or not line:
                sys.exit(f"round {r}, {name}: exit status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            rounds[name].append(json.loads(line[0].split(" ", 1)[1]))
            print(r, name, rounds[name][-1], flush=True)
    figures = [k for k in rounds["new"][0] if k != "library_sha256"]
    result = {"what": "host cost of the chained step's launches: the parent build against this one, same kernels (see tools/step_launch_host.py)",
              "rounds": rounds, "medians": {}, "parent_slowest_round": {}, "new_median_within_parent_spread": {}}
    for k in figures:
        med = {name: statistics.median(x[k] for x in rounds[name]) for name in builds}
        worst = max(x[k] for x in rounds["parent"])
        result["medians"][k] = med
        result["parent_slowest_round"][k] = worst
        result["new_median_within_parent_spread"][k] = med["new"] <= worst
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: result[k] for k in ("medians", "parent_slowest_round", "new_median_within_parent_spread")}, indent=1))
    return 0 if all(result["new_median_within_parent_spread"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
