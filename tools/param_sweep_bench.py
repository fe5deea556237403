#!/usr/bin/env python3
"""param_sweep_bench.py — what per-world physics constants cost and what they buy (dw_step_n_trace_ensemble), on one GPU.

    python tools/param_sweep_bench.py [--out profiles/param_sweep_bench.json] [--parent-lib PATH] [--rounds 7] [--quick]

Arms INTERLEAVED in one process (tools/kbench.py's way) from one restored snapshot of a developed quantised state, device
time from HIP events on the handle's stream, (t(2n) - t(n)) / n per arm: 1024 x 256^2 and 64 x 2048^2, `fast` and `exact`.
(a) OWN  dw_step_n_trace_ensemble, every world at the handle's own constants (step pairs in the float32-only mode)
    PW   dw_step_n_trace_per_world with the same schedule: single steps.  With --parent-lib (a library built from the
         parent commit, same ABI) PW runs on THAT library; without it on this one, whose single-step kernels are unchanged
         (tests/test_per_world_cpu.py::test_no_existing_kernel_changed).
(b) MIX  the same run with a mixed, asymmetric parameter table: the cost of SYM = false in the exact mode.
(c) the three-value q2 figure (q2 = 0, q/64, q/8 x 20 worlds of 256^2, 512 steps, temperature=True) as ONE
    simulate_parameter_sweep call against three sequential simulate_ramp(temperature=True) runs: wall clock.
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

SHAPES = [("1024x256^2", (1024, 256, 256), 48), ("64x2048^2", (64, 2048, 2048), 16)]
QUICK = [("quick_16x256^2", (16, 256, 256), 16), ("quick_2x512x2048", (2, 512, 2048), 8)]


def mixed_table(own, B):
    tab = np.repeat(own[None], B)
    q = float(own["q"])
    for b in range(B):
        kind = b % 5
        if kind == 1:
            tab["q2"][b] = 0.0
        elif kind == 2:
            tab["q2"][b] = q / 64.0
        elif kind == 3:
            tab["albedo_light"][b], tab["albedo_dark"][b], tab["gamma"][b] = 0.8, 0.3, 0.3
        elif kind == 4:
            tab["temp_optimal"][b], tab["dt"][b] = 290.0, 0.5
    return tab


def kernel_ab(amd, _ffi, shape, n, precision, rounds, parent_lib):
    B, H, W = shape
    p = amd.default_params(B, H, W, 0)
    p.precision = _ffi.PRECISION[precision]
    eng = amd.Engine(p)
    old = amd.Engine(p, lib_path=parent_lib) if parent_lib else eng
    for e in {id(eng): eng, id(old): old}.values():
        e.init_random(42, quantised=True)
        L = e.step_n(220, 0.75, 0.75 / 512, 0.75, 1.5)          # developed state, L ~ 1.07 (kbench.py's)
        e.snapshot_save()
    cols = {k: np.full((k, B), L) for k in (n, 2 * n)}
    own = np.repeat(eng.world_params()[None], B)
    mix = mixed_table(eng.world_params(), B)
    arms = (("OWN", eng, lambda k: eng.step_n_trace_ensemble(own, cols[k], trace=False)),
            ("PW", old, lambda k: old.step_n_trace_per_world(cols[k], trace=False)),
            ("MIX", eng, lambda k: eng.step_n_trace_ensemble(mix, cols[k], trace=False)))
    ms = {name: [] for name, _, _ in arms}
    for r in range(rounds + 1):                                # round 0 warms up (allocations, first launches)
        for name, e, fn in arms:
            t = {}
            for k in (n, 2 * n):
                e.snapshot_restore()
                e.sync()
                e.timer_start()
                fn(k)
                t[k] = e.timer_stop()
            if r:
                ms[name].append((t[2 * n] - t[n]) / n)
    info = eng.kernel_info()
    if old is not eng:
        old.close()
    eng.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"precision": precision, "steps": n, "rounds": rounds, "luminosity": L, "ms_per_step_median": med,
            "ms_per_step_min": {k: min(v) for k, v in ms.items()}, "ms_per_step_max": {k: max(v) for k, v in ms.items()},
            "OWN_over_PW": med["OWN"] / med["PW"], "MIX_over_OWN": med["MIX"] / med["OWN"],
            "PW_library": "parent" if parent_lib else "this build", "form": info.rsplit("; per-world constants: ", 1)[-1]}


def q2_figure(amd, worlds_each, nsteps, dim):
    def fresh(B):
        np.random.seed(1)
        env = amd.RLDaisyWorld(grid_dimension=dim, n_agents=0)
        env.batch_size = B
        env.reset_synthetic(3)
        env._ensure_engine().sync()
        return env

    env = fresh(3 * worlds_each)
    q2 = np.repeat([0.0, env.q / 64.0, env.q / 8.0], worlds_each)
    t0 = time.perf_counter()
    out = amd.simulate_parameter_sweep(env, {"q2": q2}, nsteps, obs=True, temperature=True)
    t_one = time.perf_counter() - t0
    env.close()
    t_seq, means = 0.0, []
    for value in (0.0, None, None):
        ref = fresh(worlds_each)
        ref.q2 = {0: 0.0, 1: ref.q / 64.0, 2: ref.q / 8.0}[len(means)]
        t0 = time.perf_counter()
        r = amd.simulate_ramp(ref, nsteps, obs=True, temperature=True)
        t_seq += time.perf_counter() - t0
        means.append(float(r["mean_temp"][-1].mean()))
        ref.close()
    return {"worlds_per_value": worlds_each, "steps": nsteps, "world": [dim, dim], "one_call_wall_s": t_one,
            "three_runs_wall_s": t_seq, "three_runs_over_one_call": t_seq / t_one,
            "final_mean_temp_one_call": [float(out["mean_temp"][-1, i * worlds_each:(i + 1) * worlds_each].mean()) for i in range(3)],
            "final_mean_temp_three_runs": means}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "param_sweep_bench.json"))
    ap.add_argument("--parent-lib", default=None, help="a library built from the parent commit (arm PW runs on it)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="small shapes (a check of the tool itself)")
    ap.add_argument("--skip-figure", action="store_true")
    a = ap.parse_args()
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi, build
    result = {"tool": "tools/param_sweep_bench.py", "build_id": _ffi.load().dw_build_id().decode(),
              "parent_build_id": build.library_id(a.parent_lib) if a.parent_lib else None,
              "method": "OWN / PW / MIX interleaved in one process from one restored snapshot; HIP-event time of n and of 2n "
                        "steps, (t(2n) - t(n)) / n; one warm-up round, median of the timed rounds.  q2 figure: wall clock.",
              "kernel_ab": {}}
    for name, shape, n in (QUICK if a.quick else SHAPES):
        result["kernel_ab"][name] = {"B_H_W": list(shape)}
        for precision in ("fast", "exact"):
            r = kernel_ab(amd, _ffi, shape, n, precision, a.rounds, a.parent_lib)
            result["kernel_ab"][name][precision] = r
            print(f"{name} {precision} ({r['form']}): " + ", ".join(f"{k} {v:.4f} ms" for k, v in r["ms_per_step_median"].items()) +
                  f"; OWN/PW {r['OWN_over_PW']:.4f}, MIX/OWN {r['MIX_over_OWN']:.4f}", flush=True)
    if not a.skip_figure:
        result["q2_figure"] = q2_figure(amd, 4 if a.quick else 20, 32 if a.quick else 512, 256)
        d = result["q2_figure"]
        print(f"q2 figure: one call {d['one_call_wall_s']:.3f} s, three runs {d['three_runs_wall_s']:.3f} s, ratio "
              f"{d['three_runs_over_one_call']:.2f}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
