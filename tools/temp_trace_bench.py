#!/usr/bin/env python3
"""temp_trace_bench.py — what the per-world temperature statistics cost (dw_reduce_temperature,
dw_step_n_trace_temperature), on one GPU.

    python tools/temp_trace_bench.py [--out profiles/temp_trace_bench.json] [--repeats 5] [--quick]

Three measurements, exact mode:

  1  the reduction alone at C2's shape (1024 worlds of 256^2, quantised planes): HIP events on the handle's stream around
     dw_reduce_temperature - temp_moments_pw, the finishing kernel and the 32 KB download of the records - beside the
     floor of the 4 bytes per cell it reads (two binary16 planes) at `--hbm-gbs`;
  2  512 steps of the ramp at the same shape, from one restored device snapshot, interleaved in one process:
       B  dw_step_n_trace              the cover series (step pairs where the shape takes them)
       T  dw_step_n_trace_temperature  covers and temperatures: single steps plus one reduction each
     T / B is the price of the temperature series;
  3  at 64 worlds of 256^2, the only way the library offered before: dw_step + dw_download_caches(temps only) + NumPy
     mean / std per step (24 bytes per cell over the host link per step), beside T on the same handle.

One warm-up round, median of `--repeats` rounds, wall clock around each synchronised run divided by its steps.
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

MIN_L, MAX_L, DL = 0.75, 1.5, 0.75 / 512


def ramp(n):
    return np.minimum(MIN_L + DL * np.arange(n), MAX_L)


def engine(amd, _ffi, B, H, W):
    p = amd.default_params(B, H, W, 0)
    p.precision = _ffi.PRECISION["exact"]
    eng = amd.Engine(p)
    eng.init_random(42, quantised=True)
    eng.step(MIN_L)                                             # a retained previous state in binary16
    eng.snapshot_save()
    return eng


def interleaved(eng, ways, steps, repeats):
    times = {k: [] for k, _ in ways}
    for rep in range(repeats + 1):                              # round 0 warms up
        for name, fn in ways:
            eng.snapshot_restore()
            eng.sync()
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if rep:
                times[name].append(dt / steps * 1e3)
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temp_trace_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM bandwidth the 4 B/cell floor is stated at (GB/s)")
    ap.add_argument("--quick", action="store_true", help="small shapes (a check of the tool itself)")
    a = ap.parse_args()
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi
    big, small, steps = ((16, 256, 256), (4, 256, 256), 16) if a.quick else ((1024, 256, 256), (64, 256, 256), 512)
    Ls = ramp(steps)
    result = {"tool": "tools/temp_trace_bench.py", "build_id": _ffi.load().dw_build_id().decode(), "precision": "exact",
              "repeats": a.repeats, "steps": steps}

    # 1: the reduction alone
    eng = engine(amd, _ffi, *big)
    cells = big[0] * big[1] * big[2]
    ms = []
    for rep in range(a.repeats + 1):
        eng.timer_start()
        eng.reduce_temperature(1.0)
        dt = eng.timer_stop()
        if rep:
            ms.append(dt)
    floor_ms = 4.0 * cells / (a.hbm_gbs * 1e9) * 1e3
    k_ms = statistics.median(ms)
    result["kernel_alone"] = {"B_H_W": list(big), "ms_median": k_ms, "ms_min": min(ms), "ms_max": max(ms),
                              "ns_per_cell": k_ms * 1e6 / cells, "bytes_read_per_cell": 4,
                              "floor_ms_at_hbm_gbs": floor_ms, "hbm_gbs": a.hbm_gbs, "times_floor": k_ms / floor_ms,
                              "achieved_gbs": 4.0 * cells / (k_ms * 1e-3) / 1e9,
                              "includes": "temp_moments_pw, temp_moments_finish_pw, 32 B per world downloaded"}
    print(f"1  reduction alone {big}: {k_ms:.3f} ms ({k_ms * 1e6 / cells:.4f} ns/cell), floor {floor_ms:.3f} ms "
          f"at {a.hbm_gbs:.0f} GB/s: {k_ms / floor_ms:.1f} x the floor", flush=True)

    # 2: the temperature trace beside the cover trace
    r = interleaved(eng, (("B_step_n_trace", lambda: eng.step_n_trace(Ls)),
                          ("T_step_n_trace_temperature", lambda: eng.step_n_trace_temperature(Ls))), steps, a.repeats)
    info = eng.kernel_info()
    eng.close()
    result["trace"] = {"B_H_W": list(big), "ms_per_step": r,
                       "T_over_B": r["T_step_n_trace_temperature"]["median"] / r["B_step_n_trace"]["median"],
                       "cover_trace_form": "step pairs" if "trace: step pairs" in info else "single steps"}
    print(f"2  {big} per step: cover trace {r['B_step_n_trace']['median']:.4f} ms, with temperatures "
          f"{r['T_step_n_trace_temperature']['median']:.4f} ms: T/B {result['trace']['T_over_B']:.2f}", flush=True)

    # 3: the way through the caches
    eng = engine(amd, _ffi, *small)

    def through_caches():
        out = []
        for L in Ls:
            eng.step(float(L))
            t = eng.download_caches(float(L), betas=False, growth=False, temp_effective=False)[0][:, 0]
            out.append((t.mean(axis=(1, 2)), t.std(axis=(1, 2))))
        return out

    r = interleaved(eng, (("A_step_download_caches_numpy", through_caches),
                          ("T_step_n_trace_temperature", lambda: eng.step_n_trace_temperature(Ls))), steps, a.repeats)
    eng.close()
    result["through_caches"] = {"B_H_W": list(small), "ms_per_step": r,
                                "A_over_T": r["A_step_download_caches_numpy"]["median"] / r["T_step_n_trace_temperature"]["median"]}
    print(f"3  {small} per step: step + download_caches + NumPy {r['A_step_download_caches_numpy']['median']:.4f} ms, "
          f"temperature trace {r['T_step_n_trace_temperature']['median']:.4f} ms: A/T {result['through_caches']['A_over_T']:.1f}",
          flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
