#!/usr/bin/env python3
"""lum_sweep_bench.py — what per-world luminosities cost and what they buy (dw_step_n_trace_per_world), on one GPU.

    python tools/lum_sweep_bench.py [--out profiles/lum_sweep_bench.json] [--rounds 7] [--quick] [--skip-diagram]

(a) The per-world single-step kernel against the shared-L single-step kernel (unchanged code) at the same shape, from
    the same developed quantised state, 1024 x 256^2 and 64 x 4096^2, `fast` and `exact`.  Three arms INTERLEAVED in one
    process (tools/kbench.py's way), device time from HIP events on the handle's stream:
        S1, S2   n calls of dw_step at one luminosity - twice: S2 / S1 is the null A/B, the noise floor
        PW       dw_step_n_trace_per_world, all columns equal to that luminosity, no series
    Every arm is timed for n and for 2n steps and reports (t(2n) - t(n)) / n: what a step costs once the call's fixed
    part - for PW the derivation and upload of the one table row that equal steps share - is paid.  That fixed part is
    reported on its own (host wall time of deriving and uploading B sets, and of a schedule that changes every step:
    B * n sets).
(b) A 256-luminosity, 512-step diagram of 256^2 worlds through harness.simulate_luminosity_sweep against the same
    diagram as 256 sequential one-world Engine.step_n_trace runs (what the API offered before): wall time, ratio only.
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

SHAPES = [("1024x256^2", (1024, 256, 256), 48), ("64x4096^2", (64, 4096, 4096), 8)]
QUICK = [("quick_16x256^2", (16, 256, 256), 16), ("quick_2x512x4096", (2, 512, 4096), 8)]


def kernel_ab(amd, _ffi, shape, n, precision, rounds):
    B, H, W = shape
    p = amd.default_params(B, H, W, 0)
    p.precision = _ffi.PRECISION[precision]
    eng = amd.Engine(p)
    eng.init_random(42, quantised=True)
    L = eng.step_n(220, 0.75, 0.75 / 512, 0.75, 1.5)           # developed state, L ~ 1.07 (kbench.py's)
    eng.snapshot_save()
    cols = {k: np.full((k, B), L) for k in (n, 2 * n)}

    def shared(k):
        for _ in range(k):
            eng.step(L)

    def per_world(k):
        eng.step_n_trace_per_world(cols[k], trace=False)

    arms = (("S1", shared), ("S2", shared), ("PW", per_world))
    ms = {name: [] for name, _ in arms}
    for r in range(rounds + 1):                                # round 0 warms up (allocations, first launches)
        for name, fn in arms:
            t = {}
            for k in (n, 2 * n):
                eng.snapshot_restore()
                eng.sync()
                eng.timer_start()
                fn(k)
                t[k] = eng.timer_stop()
            if r:
                ms[name].append((t[2 * n] - t[n]) / n)
    # the call's fixed part and the cost of a schedule that changes every step, host wall clock around whole calls
    ramp = np.ascontiguousarray(L + 1e-4 * np.arange(n)[:, None] + np.zeros((1, B)))
    wall = {}
    for name, sched in (("equal_columns", cols[n]), ("every_step_differs", ramp)):
        best = []
        for _ in range(3):
            eng.snapshot_restore()
            eng.sync()
            t0 = time.perf_counter()
            eng.step_n_trace_per_world(sched, trace=False)
            best.append((time.perf_counter() - t0) * 1e3)
        wall[name] = min(best)
    info = eng.kernel_info()
    eng.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    floor = abs(med["S2"] / med["S1"] - 1.0)
    spread = max(max(v) / min(v) - 1.0 for v in (ms["S1"], ms["S2"]))
    ratio = med["PW"] / (0.5 * (med["S1"] + med["S2"]))
    return {"precision": precision, "steps": n, "rounds": rounds, "luminosity": L,
            "ms_per_step_median": med, "ms_per_step_min": {k: min(v) for k, v in ms.items()},
            "ms_per_step_max": {k: max(v) for k, v in ms.items()},
            "null_ab_S2_over_S1": med["S2"] / med["S1"], "noise_floor": max(floor, spread),
            "PW_over_shared": ratio, "within_floor": bool(abs(ratio - 1.0) <= max(floor, spread)),
            "wall_ms_whole_call": wall,
            "table_host_ms_per_step_when_every_step_differs": (wall["every_step_differs"] - wall["equal_columns"]) / n,
            "derivations": {"equal_columns": B, "every_step_differs": B * n},
            "per_world_form": "wave strips" if "per-world L: wave strips" in info else "generic"}


def diagram(amd, _ffi, nl, nsteps, dim):
    Lv = np.linspace(0.6, 1.7, nl)
    np.random.seed(1)
    env = amd.RLDaisyWorld(grid_dimension=dim, n_agents=0)
    env.batch_size = nl
    env.reset_synthetic(3)
    env._ensure_engine().sync()
    t0 = time.perf_counter()
    out = amd.simulate_luminosity_sweep(env, Lv, nsteps, obs=True)
    t_sweep = time.perf_counter() - t0
    env.close()
    p = amd.default_params(1, dim, dim, 0)
    t0 = time.perf_counter()
    alive = []
    for b in range(nl):
        p.world_offset = b
        one = amd.Engine(p)
        one.init_random(3)
        tr = one.step_n_trace(np.full(nsteps, Lv[b]))
        alive.append(tr["max_k"][-1, 0] > 5)
        one.close()
    t_seq = time.perf_counter() - t0
    return {"luminosities": nl, "steps": nsteps, "world": [dim, dim], "sweep_wall_s": t_sweep, "sequential_wall_s": t_seq,
            "sequential_over_sweep": t_seq / t_sweep, "alive_at_the_end": int(out["alive"][-1].sum()),
            "same_alive_set": bool(np.array_equal(out["alive"][-1], np.array(alive)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lum_sweep_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="small shapes (a check of the tool itself)")
    ap.add_argument("--skip-diagram", action="store_true")
    a = ap.parse_args()
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi
    result = {"tool": "tools/lum_sweep_bench.py", "build_id": _ffi.load().dw_build_id().decode(),
              "method": "(a) S1, S2 (dw_step, shared L) and PW (dw_step_n_trace_per_world, equal columns) interleaved in one "
                        "process from one restored snapshot; HIP-event time of n and of 2n steps, (t(2n) - t(n)) / n; one "
                        "warm-up round, median of the timed rounds; noise floor = the larger of |S2/S1 - 1| and the "
                        "max/min spread of S1 and S2.  (b) wall clock.",
              "kernel_ab": {}}
    for name, shape, n in (QUICK if a.quick else SHAPES):
        result["kernel_ab"][name] = {"B_H_W": list(shape)}
        for precision in ("fast", "exact"):
            r = kernel_ab(amd, _ffi, shape, n, precision, a.rounds)
            result["kernel_ab"][name][precision] = r
            print(f"{name} {precision}: " + ", ".join(f"{k} {v:.4f} ms" for k, v in r["ms_per_step_median"].items()) +
                  f"; PW/shared {r['PW_over_shared']:.4f}, floor {r['noise_floor']:.4f}, within: {r['within_floor']}; "
                  f"table host cost {r['table_host_ms_per_step_when_every_step_differs']:.4f} ms/step when every step differs",
                  flush=True)
    if not a.skip_diagram:
        result["diagram"] = diagram(amd, _ffi, 16 if a.quick else 256, 32 if a.quick else 512, 256)
        d = result["diagram"]
        print(f"diagram: sweep {d['sweep_wall_s']:.3f} s, sequential {d['sequential_wall_s']:.3f} s, ratio "
              f"{d['sequential_over_sweep']:.1f}; same alive set: {d['same_alive_set']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
