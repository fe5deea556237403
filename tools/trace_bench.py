#!/usr/bin/env python3
"""trace_bench.py — what the per-step world statistics cost (dw_step_n_trace), on one GPU.

    python tools/trace_bench.py [--out profiles/trace_bench.json] [--repeats 5] [--quick]

For C2 (1024 worlds of 256^2, the 512-step ramp), 64 x 4096^2 and 256 x 1024^2 (64 steps each), in both arithmetic
modes, the time per step of three ways through the SAME steps from the SAME state (a device snapshot restored before
every timed run):

  A  dw_step + dw_reduce per step   the only way to the series without dw_step_n_trace: single-step kernels, a stream
                                    synchronisation and a download per step
  B  dw_step_n                      step pairs, no series
  C  dw_step_n_trace                the series recorded on the device, one download at the end

interleaved in one process (A, B, C, A, B, C, ...), after a warm-up round, median of `--repeats` rounds.  The rule of
DESIGN.md 3.2f: a trace pair kernel is kept only where C < A; C / B is the price of the series.
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

# name, (B, H, W), timed steps, warm-up steps before the snapshot
SHAPES = [("c2_1024x256^2", (1024, 256, 256), 512, 0),
          ("64x4096^2", (64, 4096, 4096), 64, 128),
          ("256x1024^2", (256, 1024, 1024), 64, 128)]


def ramp(L0, n):
    out, L = [], L0
    for _ in range(n):
        out.append(L)
        L = min(max(L + DL, MIN_L), MAX_L)
    return np.array(out), L


def measure(amd, _ffi, shape, steps, warm, precision, repeats):
    B, H, W = shape
    p = amd.default_params(B, H, W, 0)
    p.precision = _ffi.PRECISION[precision]
    eng = amd.Engine(p)
    eng.init_random(42, quantised=True)
    L0 = MIN_L
    if warm:
        L0 = eng.step_n(warm, L0, DL, MIN_L, MAX_L)
    eng.snapshot_save()
    Ls, _ = ramp(L0, steps)

    def run_a():
        rows = []
        for L in Ls:
            eng.step(float(L))
            rows.append(eng.reduce())
        return np.stack(rows)

    def run_b():
        eng.step_n(steps, L0, DL, MIN_L, MAX_L)
        eng.sync()
        return None

    def run_c():
        return eng.step_n_trace(Ls)

    ways = (("A_step_reduce", run_a), ("B_step_n", run_b), ("C_step_n_trace", run_c))
    times = {k: [] for k, _ in ways}
    series = {}
    for rep in range(repeats + 1):                              # round 0 warms up
        for name, fn in ways:
            eng.snapshot_restore()
            eng.sync()
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            if rep:
                times[name].append(dt / steps * 1e3)
            elif out is not None:
                series[name] = out
    same = all(np.array_equal(series["A_step_reduce"][f], series["C_step_n_trace"][f])
               for f in ("max_k", "sum_light_k", "sum_dark_k"))
    info = eng.kernel_info()
    eng.close()
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"precision": precision, "steps": steps, "warmup_steps": warm, "repeats": repeats,
            "ms_per_step_median": med, "ms_per_step_min": {k: min(v) for k, v in times.items()},
            "ms_per_step_max": {k: max(v) for k, v in times.items()},
            "C_over_A": med["C_step_n_trace"] / med["A_step_reduce"], "C_over_B": med["C_step_n_trace"] / med["B_step_n"],
            "series_A_equals_C": bool(same),
            "trace_form": "step pairs" if "trace: step pairs" in info else "single steps"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="small shapes (a check of the tool itself)")
    a = ap.parse_args()
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi
    shapes = [("quick_8x256^2", (8, 256, 256), 32, 8), ("quick_2x512x4096", (2, 512, 4096), 16, 8)] if a.quick else SHAPES
    result = {"tool": "tools/trace_bench.py", "build_id": _ffi.load().dw_build_id().decode(),
              "method": "A, B, C interleaved in one process from one restored device snapshot; one warm-up round; "
                        "median of the timed rounds; wall clock around each whole run (synchronised), divided by its steps",
              "shapes": {}}
    for name, shape, steps, warm in shapes:
        result["shapes"][name] = {"B_H_W": list(shape)}
        for precision in ("fast", "exact"):
            r = measure(amd, _ffi, shape, steps, warm, precision, a.repeats)
            result["shapes"][name][precision] = r
            print(f"{name} {precision}: " + ", ".join(f"{k} {v:.4f} ms" for k, v in r["ms_per_step_median"].items()) +
                  f"; C/A {r['C_over_A']:.3f}, C/B {r['C_over_B']:.3f}; {r['trace_form']}; series equal: {r['series_A_equals_C']}",
                  flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
