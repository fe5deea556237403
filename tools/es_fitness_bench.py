#!/usr/bin/env python3
"""Evolution-strategy fitness evaluation (ref daisy/evo/sges.py:144-181, :314-349) as one batched ensemble:
P random MLP policies x `wpm` worlds each, device-resident in chunks (dw_run_episode_mlp), with the reference's bookkeeping
on the host (`bookkeeping="host"`: NumPy on the downloaded rewards) or on the device (`"device"`: dw_run_episode_mlp_fitness).

usage: es_fitness_bench.py [P] [wpm] [dim] [max_steps] [chunk[,chunk...]] [--bookkeeping host|device|both]
           one line per chunk size and arm: the first generation and the best of three later ones
       es_fitness_bench.py --measure [--out profiles/es_fitness_device_bench.json] [--rounds 9] [--quick]
           the two arms INTERLEAVED in one process at shape 1 (64 members x 32 worlds of 16x16, 4 agents, chunk 64) and
           shape 2 (1000 worlds of 8x8 as ONE pair, `get_fitness`), medians of the rounds after one warm-up round:
             chunk       one 64-step chunk from the same restored snapshot: HIP events around the chunk call (host arm:
                         dw_run_episode_mlp into page-locked buffers; device arm: dw_run_episode_mlp_fitness), and the wall
                         time of the call plus, for the host arm, `_population_chunk` on what it downloaded
             generation  wall time of one `get_fitness_population` / `get_fitness` from the same seed, reset included
           and whether both arms returned the same bits.
       es_fitness_bench.py [P] [wpm] [dim] --profiled-run
           three generations of the device arm (default: shape 1) and nothing else: the program of a separate
           `rocprofv3 --kernel-trace --stats` run
       es_fitness_bench.py --kernel-stats SHAPE=STATS.csv [SHAPE=STATS.csv ...] [--out ...]
           fold the rows of those runs' kernel statistics (the fitness kernels, the episode kernel) into the result file"""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ARMS = ("host", "device")


def _arms(which):
    return ARMS if which == "both" else (which,)


def _generation(amd, shape, arm, pop, max_steps, chunk, env=None):
    """One generation from the seed every arm starts from: (result, wall seconds, steps, env)."""
    from therldaisyworld_amd.harness import get_fitness, get_fitness_population
    P, wpm, dim = shape
    np.random.seed(11)
    if env is None:
        env = amd.RLDaisyWorld(grid_dimension=dim, n_agents=4)
    t0 = time.perf_counter()
    if P == 1:                                                  # one pair: the reference's get_fitness on wpm worlds
        env.batch_size = wpm
        res = [get_fitness(env, pop[0], pop[1], max_steps=max_steps, chunk=chunk, bookkeeping=arm)]
    else:
        res = get_fitness_population(env, pop, worlds_per_member=wpm, max_steps=max_steps, chunk=chunk, bookkeeping=arm)
    return res, time.perf_counter() - t0, env.step_count, env


def _same(a, b):
    return all(np.float64(x[0]).tobytes() == np.float64(y[0]).tobytes() and np.array_equal(x[1], y[1]) and
               np.array_equal(np.asarray(x[2]), np.asarray(y[2])) for x, y in zip(a, b))


def lines(amd, P, wpm, dim, max_steps, chunks, which):
    np.random.seed(7)
    pop = [amd.MLP() for _ in range(max(P, 2))]
    for chunk in chunks + chunks[:1]:
        for arm in _arms(which):
            res, dt, steps, env = _generation(amd, (P, wpm, dim), arm, pop, max_steps, chunk)
            # later generations on the same environment, as in an ES loop: no device handle to (re)create, kernels loaded
            later = []
            for _ in range(3):
                _, dt2, steps2, _ = _generation(amd, (P, wpm, dim), arm, pop, max_steps, chunk, env)
                later.append((dt2, steps2))
            dt2, steps2 = min(later)
            print(f"P={P} x {wpm} worlds of {dim}x{dim}, 4 agents, chunk={chunk}, bookkeeping={arm}: first generation (creates "
                  f"the device handle) {steps} steps in {dt:.3f} s = {dt / steps * 1e6:.0f} us/step; later generations (best of "
                  f"3) {steps2} steps in {dt2:.3f} s = {dt2 / steps2 * 1e6:.0f} us/step, "
                  f"{P * wpm * 4 * steps2 / dt2 / 1e6:.2f} M agent-steps/s (all three: "
                  f"{', '.join(f'{t * 1e3:.1f} ms' for t, _ in later)}); best fitness {max(r[0] for r in res):.4f}", flush=True)
            env.close()


def _spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def measure_chunk(amd, _ffi, shape, rounds, K=64):
    """One K-step chunk per arm from the same restored snapshot."""
    from therldaisyworld_amd import harness
    P, wpm, dim = shape
    B, N, half = P * wpm, 4, 2
    p = amd.default_params(B, dim, dim, N)
    eng = amd.Engine(p)
    eng.init_random(42, quantised=True)
    eng.step(0.9, np.zeros((B, N, 1), dtype=np.int64))        # current and previous state quantised: the chunk is ONE launch
    eng.snapshot_save()
    Ls = np.linspace(0.9, 1.0, K)
    n_sets = max(P, 2)
    params = np.random.RandomState(7).randn(n_sets, 1808) * 0.5
    if P == 1:
        ma, mb = np.zeros(B, dtype=np.int32), np.ones(B, dtype=np.int32)
    else:
        ma = mb = np.repeat(np.arange(P), wpm).astype(np.int32)
    eng.run_episode_mlp(Ls[:1], params, ma, mb, half)         # the parameter sets stay on the device, as in the harness
    stream, wall = {a: [] for a in ARMS}, {a: [] for a in ARMS}
    outcome = {}
    for r in range(rounds + 1):                                # round 0 warms up (allocations, first launches)
        for arm in ARMS:
            eng.snapshot_restore()
            acc = {"done_at": np.zeros((B, N, 1), dtype=int), "total_steps": np.zeros((B, N, 1), dtype=int),
                   "sum_reward": np.zeros(P), "running": np.ones(P, dtype=bool)}
            if arm == "device":
                eng.fitness_begin(wpm, half)
            eng.sync()
            t0 = time.perf_counter()
            eng.timer_start()
            if arm == "host":
                rewards, dones = eng.run_episode_mlp(Ls, None, ma, mb, half, reuse_buffers=True, n_members=n_sets)
                ms = eng.timer_stop()
                got = harness._population_chunk(acc, rewards, dones, half, wpm)
            else:
                got = eng.run_episode_mlp_fitness(Ls, None, ma, mb, half, n_members=n_sets)
                ms = eng.timer_stop()
            w = (time.perf_counter() - t0) * 1e3
            if arm == "device":
                s, d, run = eng.fitness_download()
                acc = {"sum_reward": s, "done_at": d, "running": run}
            outcome[arm] = (got, acc["sum_reward"].tobytes(), np.asarray(acc["done_at"]).astype(int).tobytes(),
                            np.asarray(acc["running"]).tobytes())
            if r:
                stream[arm].append(ms)
                wall[arm].append(w)
    info = eng.kernel_info()
    eng.close()
    return {"chunk_steps": K, "stream_ms_per_chunk": {a: _spread(stream[a]) for a in ARMS},
            "wall_ms_per_chunk_with_bookkeeping": {a: _spread(wall[a]) for a in ARMS},
            "same_bits": outcome["host"] == outcome["device"],
            "form": info.split("; mlp episode: ", 1)[-1].split(";")[0]}


def measure_generation(amd, shape, rounds, max_steps, chunk=64):
    P, wpm, dim = shape
    np.random.seed(7)
    pop = [amd.MLP() for _ in range(max(P, 2))]
    env = None
    wall, steps, res = {a: [] for a in ARMS}, {}, {}
    for r in range(rounds + 1):
        for arm in ARMS:
            res[arm], dt, steps[arm], env = _generation(amd, shape, arm, pop, max_steps, chunk, env)
            if r:
                wall[arm].append(dt * 1e3)
    env.close()
    out = {"max_steps": max_steps, "chunk": chunk, "steps": steps, "wall_ms_per_generation": {a: _spread(wall[a]) for a in ARMS},
           "wall_us_per_step": {a: {k: v * 1e3 / steps[a] for k, v in _spread(wall[a]).items()} for a in ARMS},
           "same_bits": _same(res["host"], res["device"])}
    return out


def _verdict(spreads):
    """device beats host by more than the host arm's min-max spread over the rounds?"""
    h, d = spreads["host"], spreads["device"]
    gain, spread = h["median"] - d["median"], h["max"] - h["min"]
    return {"host_median_minus_device_median": gain, "host_min_max_spread": spread, "device_beats_host_by_more_than_spread": gain > spread}


def measure(a):
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi
    shapes = [(4, 4, 16), (1, 40, 8)] if a.quick else [(64, 32, 16), (1, 1000, 8)]
    result = {"tool": "tools/es_fitness_bench.py --measure", "build_id": _ffi.load().dw_build_id().decode(), "rounds": a.rounds,
              "method": "host and device arms interleaved in one process, one warm-up round, then `rounds` timed rounds: median, "
                        "min, max.  chunk: one 64-step chunk per arm from the same restored snapshot; stream = HIP events on the "
                        "handle's stream around the chunk call (upload, kernels, download), wall = perf_counter around the call "
                        "and, host arm, harness._population_chunk on its rewards.  generation: perf_counter around one "
                        "get_fitness_population / get_fitness from the same seed (environment reset included).",
              "cases": []}
    for shape in shapes:
        P, wpm, dim = shape
        case = {"members": P, "worlds_per_member": wpm, "grid": dim, "n_agents": 4,
                "chunk": measure_chunk(amd, _ffi, shape, a.rounds),
                "generation": measure_generation(amd, shape, a.rounds, a.max_steps)}
        case["chunk"]["verdict_wall"] = _verdict(case["chunk"]["wall_ms_per_chunk_with_bookkeeping"])
        case["generation"]["verdict_wall"] = _verdict(case["generation"]["wall_ms_per_generation"])
        result["cases"].append(case)
        c, g = case["chunk"], case["generation"]
        print(f"{P} x {wpm} worlds of {dim}x{dim} ({c['form']}): chunk stream ms host {c['stream_ms_per_chunk']['host']['median']:.3f} "
              f"device {c['stream_ms_per_chunk']['device']['median']:.3f}; chunk wall ms with bookkeeping host "
              f"{c['wall_ms_per_chunk_with_bookkeeping']['host']['median']:.3f} device "
              f"{c['wall_ms_per_chunk_with_bookkeeping']['device']['median']:.3f}; generation of {g['steps']['host']} steps: wall "
              f"us/step host {g['wall_us_per_step']['host']['median']:.1f} [{g['wall_us_per_step']['host']['min']:.1f}, "
              f"{g['wall_us_per_step']['host']['max']:.1f}] device {g['wall_us_per_step']['device']['median']:.1f} "
              f"[{g['wall_us_per_step']['device']['min']:.1f}, {g['wall_us_per_step']['device']['max']:.1f}]; same bits: chunk "
              f"{c['same_bits']}, generation {g['same_bits']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


def profiled_run(a):
    import therldaisyworld_amd as amd
    np.random.seed(7)
    pop = [amd.MLP() for _ in range(max(a.P, 2))]
    env = None
    for _ in range(3):
        _, dt, steps, env = _generation(amd, (a.P, a.wpm, a.dim), "device", pop, a.max_steps, 64, env)
        print(f"device arm: {steps} steps in {dt * 1e3:.1f} ms", flush=True)
    env.close()


def kernel_stats(a):
    with open(a.out) as f:
        result = json.load(f)
    result["kernel_stats"] = {"source": "separate rocprofv3 --kernel-trace --stats runs of `tools/es_fitness_bench.py P wpm dim "
                                        "--profiled-run` (three generations of the device arm, chunk 64), one run per shape",
                              "runs": []}
    for item in a.kernel_stats:                                 # "P x wpm x dim=STATS.csv"
        label, path = item.split("=", 1)
        with open(path, newline="") as f:
            rows = [r for r in csv.DictReader(f) if "fitness_" in r["Name"] or "episode_mlp" in r["Name"]]
        kernels = [{"name": r["Name"], "calls": int(r["Calls"]), "average_ns": float(r["AverageNs"]), "min_ns": int(r["MinNs"]),
                    "max_ns": int(r["MaxNs"]), "total_ns": int(r["TotalDurationNs"])} for r in rows]
        result["kernel_stats"]["runs"].append({"shape": label, "kernels": kernels})
        for k in kernels:
            print(f"{label}: {k['average_ns'] / 1e3:9.2f} us x {k['calls']:5d}  {k['name'][:100]}")
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("P", nargs="?", type=int, default=64)
    ap.add_argument("wpm", nargs="?", type=int, default=32)
    ap.add_argument("dim", nargs="?", type=int, default=16)
    ap.add_argument("max_steps", nargs="?", type=int, default=768)
    ap.add_argument("chunk", nargs="?", default="64,1")
    ap.add_argument("--bookkeeping", choices=("host", "device", "both"), default="host")
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--profiled-run", action="store_true")
    ap.add_argument("--kernel-stats", nargs="+", metavar="SHAPE=STATS.csv")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "es_fitness_device_bench.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="small ensembles (a check of the tool itself)")
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a)
    if a.profiled_run:
        return profiled_run(a)
    if a.measure:
        return measure(a)
    import therldaisyworld_amd as amd
    lines(amd, a.P, a.wpm, a.dim, a.max_steps, [int(c) for c in a.chunk.split(",")], a.bookkeeping)


if __name__ == "__main__":
    main()
