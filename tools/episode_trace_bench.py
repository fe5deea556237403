#!/usr/bin/env python3
"""episode_trace_bench.py — what the per-step records cost in the episode loop and what they buy (dw_run_episode_trace).

    python tools/episode_trace_bench.py [--out profiles/episode_trace_bench.json] [--rounds 9] [--quick]

At 1000 worlds of 8x8 with 4 greedy agents and at 64 worlds of 16x16 with 16, both precisions, 64-step chunks; the arms
INTERLEAVED in one process (tools/kbench.py's way), each from the same restored snapshot of a quantised state:
    TRACE   one dw_run_episode_trace call (episode_wave_stats_pw): flags and the records of every step
    FLAGS   the same chunk by dw_run_episode (episode_wave, unchanged by the records:
            tests/test_per_world_cpu.py::test_no_existing_kernel_changed): flags only
    STEPS   64 x (dw_run_episode of one step + dw_reduce): the only way to the records before this call
Per arm: time on the handle's stream from HIP events around the arm (uploads, kernels, downloads) and wall clock, per
chunk and per step, medians after one warm-up round; TRACE's records are compared with STEPS's, its flags with FLAGS's.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def chunk_abc(amd, _ffi, shape, precision, rounds, K=64):
    B, H, W, N = shape
    p = amd.default_params(B, H, W, N)
    p.precision = _ffi.PRECISION[precision]
    eng = amd.Engine(p)
    eng.init_random(42)
    eng.step(0.9, np.zeros((B, N, 1), dtype=np.int64))
    eng.snapshot_save()
    Ls = np.linspace(0.9, 1.0, K)

    def single_steps():
        rows = np.zeros((K, B), dtype=_ffi.STATS_DTYPE)
        for t in range(K):
            eng.run_episode(Ls[t:t + 1], _ffi.POLICY_ARGMAX, reuse_buffers=True)
            rows[t] = eng.reduce()
        return rows

    arms = (("TRACE", lambda: eng.run_episode_trace(Ls, _ffi.POLICY_ARGMAX)),
            ("FLAGS", lambda: eng.run_episode(Ls, _ffi.POLICY_ARGMAX)),
            ("STEPS", single_steps))
    stream = {name: [] for name, _ in arms}
    wall = {name: [] for name, _ in arms}
    out = {}
    for r in range(rounds + 1):                                # round 0 warms up (allocations, first launches)
        for name, fn in arms:
            eng.snapshot_restore()
            eng.sync()
            t0 = time.perf_counter()
            eng.timer_start()
            out[name] = fn()
            ms = eng.timer_stop()
            w = (time.perf_counter() - t0) * 1e3
            if r:
                stream[name].append(ms)
                wall[name].append(w)
    stats, alive, ok = out["TRACE"]
    flags_equal = bool(np.array_equal(alive, out["FLAGS"][0]) and np.array_equal(ok, out["FLAGS"][1]))
    records_equal = all(bool(np.array_equal(stats[f], out["STEPS"][f])) for f in ("max_k", "sum_light_k", "sum_dark_k"))
    info = eng.kernel_info()
    eng.close()
    sm = {k: statistics.median(v) for k, v in stream.items()}
    wm = {k: statistics.median(v) for k, v in wall.items()}
    return {"precision": precision, "B_H_W_N": [B, H, W, N], "chunk_steps": K, "rounds": rounds,
            "stream_ms_per_chunk_median": sm, "stream_ms_per_chunk_min": {k: min(v) for k, v in stream.items()},
            "wall_ms_per_chunk_median": wm, "stream_us_per_step_median": {k: v * 1e3 / K for k, v in sm.items()},
            "wall_us_per_step_median": {k: v * 1e3 / K for k, v in wm.items()},
            "TRACE_over_FLAGS_stream": sm["TRACE"] / sm["FLAGS"], "TRACE_over_FLAGS_wall": wm["TRACE"] / wm["FLAGS"],
            "STEPS_over_TRACE_stream": sm["STEPS"] / sm["TRACE"], "STEPS_over_TRACE_wall": wm["STEPS"] / wm["TRACE"],
            "flags_equal": flags_equal, "records_equal": records_equal,
            "form": info.split("; episode trace: ", 1)[-1].split(";")[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "episode_trace_bench.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="small ensembles (a check of the tool itself)")
    a = ap.parse_args()
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi
    result = {"tool": "tools/episode_trace_bench.py", "build_id": _ffi.load().dw_build_id().decode(),
              "method": "TRACE / FLAGS / STEPS interleaved in one process, each from one restored snapshot, one warm-up round, "
                        "median of the timed rounds; stream = HIP events around the arm (copies + kernels), wall = perf_counter.",
              "cases": []}
    shapes = [(40, 8, 8, 4), (8, 16, 16, 16)] if a.quick else [(1000, 8, 8, 4), (64, 16, 16, 16)]
    for shape in shapes:
        for precision in ("exact", "fast"):
            r = chunk_abc(amd, _ffi, shape, precision, a.rounds)
            result["cases"].append(r)
            print(f"{shape} {precision} ({r['form']}): stream us/step " +
                  ", ".join(f"{k} {v:.3f}" for k, v in r["stream_us_per_step_median"].items()) + "; wall us/step " +
                  ", ".join(f"{k} {v:.3f}" for k, v in r["wall_us_per_step_median"].items()) +
                  f"; TRACE/FLAGS stream {r['TRACE_over_FLAGS_stream']:.3f} wall {r['TRACE_over_FLAGS_wall']:.3f}; STEPS/TRACE stream "
                  f"{r['STEPS_over_TRACE_stream']:.2f} wall {r['STEPS_over_TRACE_wall']:.2f}; flags equal {r['flags_equal']}, "
                  f"records equal {r['records_equal']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
