#!/usr/bin/env python3
"""episode_temp_trace_bench.py — what the per-step temperature records cost in the episode loop and what they buy
(dw_run_episode_trace_temperature).

    python tools/episode_temp_trace_bench.py [--out profiles/episode_temp_trace_bench.json] [--rounds 9] [--quick]

At 1000 worlds of 8x8 with 4 greedy agents and at 64 worlds of 16x16 with 16, both precisions, 64-step chunks; the arms
INTERLEAVED in one process (tools/episode_trace_bench.py's way), each from the same restored snapshot of a quantised state:
    TEMPS   one dw_run_episode_trace_temperature call (episode_wave_temp_pw): flags, cover and temperature records
    TRACE   the same chunk by dw_run_episode_trace (episode_wave_stats_pw, unchanged): flags and cover records
    STEPS   64 x (dw_run_episode of one step + dw_reduce + dw_reduce_temperature): the only way to both records before
    NOWAVE  the TEMPS call on a second handle created under DW_NO_EPISODE_WAVE, from the same state: launches per step
Per arm: time on the handle's stream from HIP events around the arm (uploads, kernels, downloads) and wall clock, per
chunk and per step, medians after one warm-up round.  TEMPS's temperature rows are compared with STEPS's and NOWAVE's byte
for byte, its cover records and flags with TRACE's.
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


def chunk_arms(amd, _ffi, shape, precision, rounds, K=64):
    B, H, W, N = shape

    def engine(switch=None):
        for name in ("DW_NO_EPISODE_WAVE", "DW_NO_EPISODE_KERNEL"):
            os.environ.pop(name, None)
        if switch:
            os.environ[switch] = "1"                            # (read when the handle is created)
        p = amd.default_params(B, H, W, N)
        p.precision = _ffi.PRECISION[precision]
        e = amd.Engine(p)
        os.environ.pop(switch or "", None)
        e.init_random(42)
        e.step(0.9, np.zeros((B, N, 1), dtype=np.int64))
        e.snapshot_save()
        return e

    eng, slow = engine(), engine("DW_NO_EPISODE_WAVE")
    Ls = np.linspace(0.9, 1.0, K)

    def single_steps():
        rows = np.zeros((K, B), dtype=_ffi.STATS_DTYPE)
        temps = np.zeros((K, B), dtype=_ffi.TEMP_STATS_DTYPE)
        for t in range(K):
            eng.run_episode(Ls[t:t + 1], _ffi.POLICY_ARGMAX, reuse_buffers=True)
            rows[t] = eng.reduce()
            temps[t] = eng.reduce_temperature(Ls[t])
        return rows, temps

    arms = (("TEMPS", eng, lambda: eng.run_episode_trace(Ls, _ffi.POLICY_ARGMAX, temperature=True)),
            ("TRACE", eng, lambda: eng.run_episode_trace(Ls, _ffi.POLICY_ARGMAX)),
            ("STEPS", eng, single_steps),
            ("NOWAVE", slow, lambda: slow.run_episode_trace(Ls, _ffi.POLICY_ARGMAX, temperature=True)))
    stream = {name: [] for name, _, _ in arms}
    wall = {name: [] for name, _, _ in arms}
    out = {}
    for r in range(rounds + 1):                                # round 0 warms up (allocations, first launches)
        for name, e, fn in arms:
            e.snapshot_restore()
            e.sync()
            t0 = time.perf_counter()
            e.timer_start()
            out[name] = fn()
            ms = e.timer_stop()
            w = (time.perf_counter() - t0) * 1e3
            if r:
                stream[name].append(ms)
                wall[name].append(w)
    stats, alive, ok, temps = out["TEMPS"]
    records_equal = bool(stats.tobytes() == out["TRACE"][0].tobytes() and np.array_equal(alive, out["TRACE"][1])
                         and np.array_equal(ok, out["TRACE"][2]))
    temps_equal_steps = bool(temps.tobytes() == out["STEPS"][1].tobytes())
    temps_equal_nowave = bool(temps.tobytes() == out["NOWAVE"][3].tobytes())
    forms = [e.kernel_info().split("; episode temperature: ", 1)[-1].split(";")[0] for e in (eng, slow)]
    eng.close()
    slow.close()
    sm = {k: statistics.median(v) for k, v in stream.items()}
    wm = {k: statistics.median(v) for k, v in wall.items()}
    return {"precision": precision, "B_H_W_N": [B, H, W, N], "chunk_steps": K, "rounds": rounds,
            "stream_ms_per_chunk_median": sm, "stream_ms_per_chunk_min": {k: min(v) for k, v in stream.items()},
            "wall_ms_per_chunk_median": wm, "stream_us_per_step_median": {k: v * 1e3 / K for k, v in sm.items()},
            "wall_us_per_step_median": {k: v * 1e3 / K for k, v in wm.items()},
            "TEMPS_over_TRACE_stream": sm["TEMPS"] / sm["TRACE"], "TEMPS_over_TRACE_wall": wm["TEMPS"] / wm["TRACE"],
            "STEPS_over_TEMPS_stream": sm["STEPS"] / sm["TEMPS"], "STEPS_over_TEMPS_wall": wm["STEPS"] / wm["TEMPS"],
            "NOWAVE_over_TEMPS_stream": sm["NOWAVE"] / sm["TEMPS"], "NOWAVE_over_TEMPS_wall": wm["NOWAVE"] / wm["TEMPS"],
            "records_equal_TRACE": records_equal, "temps_equal_STEPS": temps_equal_steps, "temps_equal_NOWAVE": temps_equal_nowave,
            "form": forms[0], "form_NOWAVE": forms[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "episode_temp_trace_bench.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="small ensembles (a check of the tool itself)")
    a = ap.parse_args()
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi
    result = {"tool": "tools/episode_temp_trace_bench.py", "build_id": _ffi.load().dw_build_id().decode(),
              "method": "TEMPS / TRACE / STEPS / NOWAVE interleaved in one process, each from one restored snapshot, one warm-up "
                        "round, median of the timed rounds; stream = HIP events around the arm (copies + kernels), wall = perf_counter.",
              "cases": []}
    shapes = [(40, 8, 8, 4), (8, 16, 16, 16)] if a.quick else [(1000, 8, 8, 4), (64, 16, 16, 16)]
    for shape in shapes:
        for precision in ("exact", "fast"):
            r = chunk_arms(amd, _ffi, shape, precision, a.rounds)
            result["cases"].append(r)
            print(f"{shape} {precision} ({r['form']} | {r['form_NOWAVE']}): stream us/step " +
                  ", ".join(f"{k} {v:.3f}" for k, v in r["stream_us_per_step_median"].items()) + "; wall us/step " +
                  ", ".join(f"{k} {v:.3f}" for k, v in r["wall_us_per_step_median"].items()) +
                  f"; TEMPS/TRACE stream {r['TEMPS_over_TRACE_stream']:.3f} wall {r['TEMPS_over_TRACE_wall']:.3f}; STEPS/TEMPS stream "
                  f"{r['STEPS_over_TEMPS_stream']:.2f} wall {r['STEPS_over_TEMPS_wall']:.2f}; NOWAVE/TEMPS stream "
                  f"{r['NOWAVE_over_TEMPS_stream']:.2f} wall {r['NOWAVE_over_TEMPS_wall']:.2f}; records equal {r['records_equal_TRACE']}, "
                  f"temps equal {r['temps_equal_STEPS']} {r['temps_equal_NOWAVE']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
