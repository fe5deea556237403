#!/usr/bin/env python3
"""episode_ensemble_trace_bench.py — what the per-step records cost in the ensemble episode loop, what the one-wave-per-world
kernel buys, and what the call replaces (dw_run_episode_ensemble_trace).

    python tools/episode_ensemble_trace_bench.py [--out profiles/episode_ensemble_trace_bench.json] [--rounds 9] [--quick]

Two shapes, both precisions, 64-step chunks: the README table - 8 scenarios ({default, neutral albedo} x {greedy,
anti-greedy, no agent} and greedy at q2 = 0 under both albedos: tools/lifespan_sweep_bench.py's table) x 125 worlds of 8x8
with 4 agents - and 4 scenarios x 16 worlds of 16x16 with 16 agents.  Scenario s owns a contiguous block of worlds; its
policy is its block of the action table (DW_POLICY_TABLE: -1 greedy, -2 anti-greedy, 0 no agent).  The arms INTERLEAVED in
one process, each from the same restored snapshot of a quantised state:
    A       dw_run_episode_ensemble_trace with trace and temps (episode_wave_ens_trace_pw<., true>)
    A1      the same call with trace only (episode_wave_ens_trace_pw<., false>)
    B       dw_run_episode_ensemble: flags only (episode_wave_pw, unchanged) - A / B is the price of the records
    C       A on a second handle created under DW_NO_EPISODE_WAVE: launches per step - C / A is what the kernel buys
    D       what the call replaces: one handle per scenario (world_offset = its block's first world: the same worlds) with
            dw_set_params, each running dw_run_episode_trace_temperature on its block; times summed over the scenarios
Per arm: time on the handle's stream from HIP events around the call (uploads, kernels, downloads) and wall clock, per
chunk; medians of the timed rounds after one warm-up round, minimum and maximum kept.  BEFORE anything is timed the tool
asserts that A's records, temperature rows and flags equal C's byte for byte; D's are compared with A's as well.
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

NEUTRAL = {"albedo_light": 0.5, "albedo_dark": 0.5}
README_TABLE = [(dict(alb), code) for alb in ({}, NEUTRAL) for code in (-1, -2, 0)] + [(dict(alb, q2=0.0), -1) for alb in ({}, NEUTRAL)]
SMALL_TABLE = [({}, -1), (dict(NEUTRAL), -2), ({"q2": 0.0}, -1), (dict(NEUTRAL, q2=0.0), 0)]


def chunk_arms(amd, _ffi, scenarios, Bs, H, W, N, precision, rounds, K=64):
    S = len(scenarios)
    B = S * Bs

    def engine(batch, offset=0, switch=None):
        for name in ("DW_NO_EPISODE_WAVE", "DW_NO_EPISODE_KERNEL"):
            os.environ.pop(name, None)
        if switch:
            os.environ[switch] = "1"                            # (read when the handle is created)
        p = amd.default_params(batch, H, W, N)
        p.precision = _ffi.PRECISION[precision]
        p.world_offset = offset
        e = amd.Engine(p)
        os.environ.pop(switch or "", None)
        e.init_random(42)
        e.step(0.9, np.zeros((batch, N, 1), dtype=np.int64))
        return e, p

    eng, _ = engine(B)
    slow, _ = engine(B, switch="DW_NO_EPISODE_WAVE")
    table = np.repeat(eng.world_params()[None], B)
    codes = np.zeros((K, B, N), dtype=np.int8)
    for s, (params, code) in enumerate(scenarios):
        for name, value in params.items():
            table[name][s * Bs:(s + 1) * Bs] = value
        codes[:, s * Bs:(s + 1) * Bs] = code
    blocks = []                                                 # arm D: one handle per scenario, its constants set
    for s, (params, code) in enumerate(scenarios):
        e, p = engine(Bs, offset=s * Bs)
        for name, value in params.items():
            setattr(p, name, value)
        e.set_params(p)
        blocks.append(e)
    for e in [eng, slow] + blocks:
        e.snapshot_save()
    Ls = np.linspace(0.9, 1.0, K)
    cols = np.ascontiguousarray(np.repeat(Ls[:, None], B, axis=1))
    T = _ffi.POLICY_TABLE

    def one_handle_per_scenario():
        """(stream ms, results): the blocks one after the other, each between its own events"""
        ms, res = 0.0, []
        for s, e in enumerate(blocks):
            e.timer_start()
            res.append(e.run_episode_trace(Ls, T, None, np.ascontiguousarray(codes[:, s * Bs:(s + 1) * Bs]), temperature=True))
            ms += e.timer_stop()
        return ms, res

    def timed(e, fn):
        e.timer_start()
        out = fn()
        return e.timer_stop(), out

    arms = (("A", [eng], lambda: timed(eng, lambda: eng.run_episode_ensemble(table, cols, T, None, codes, trace=True, temperature=True))),
            ("A1", [eng], lambda: timed(eng, lambda: eng.run_episode_ensemble(table, cols, T, None, codes, trace=True))),
            ("B", [eng], lambda: timed(eng, lambda: eng.run_episode_ensemble(table, cols, T, None, codes))),
            ("C", [slow], lambda: timed(slow, lambda: slow.run_episode_ensemble(table, cols, T, None, codes, trace=True, temperature=True))),
            ("D", blocks, one_handle_per_scenario))

    def run(name, handles, fn):
        for e in handles:
            e.snapshot_restore()
            e.sync()
        t0 = time.perf_counter()
        ms, out = fn()
        return ms, (time.perf_counter() - t0) * 1e3, out

    # ---- the records of both forms are the same bytes: asserted before anything is timed ----
    out = {name: run(name, handles, fn)[2] for name, handles, fn in arms}
    alive, ok, stats, temps = out["A"]
    calive, cok, cstats, ctemps = out["C"]
    assert stats.tobytes() == cstats.tobytes(), "cover records differ between the wave form and the launches per step"
    assert temps.tobytes() == ctemps.tobytes(), "temperature rows differ between the wave form and the launches per step"
    assert np.array_equal(alive, calive) and np.array_equal(ok, cok), "flags differ between the two forms"
    assert out["A1"][2].tobytes() == stats.tobytes() and out["A1"][3] is None
    assert np.array_equal(out["B"][0], alive) and np.array_equal(out["B"][1], ok)
    d_stats = np.concatenate([r[0] for r in out["D"]], axis=1)
    d_temps = np.concatenate([r[3] for r in out["D"]], axis=1)
    equal_D = bool(d_stats.tobytes() == stats.tobytes() and d_temps.tobytes() == temps.tobytes())
    assert stats["max_k"].max() > 5 and (temps["std"] > 0).any(), "nothing is alive"

    stream = {name: [] for name, _, _ in arms}
    wall = {name: [] for name, _, _ in arms}
    for r in range(rounds):
        for name, handles, fn in arms:
            ms, w, _ = run(name, handles, fn)
            stream[name].append(ms)
            wall[name].append(w)
    forms = [e.kernel_info().split("; ensemble trace: ", 1)[-1].split(";")[0] for e in (eng, slow)]
    for e in [eng, slow] + blocks:
        e.close()

    def summary(v):
        return {k: {"median": statistics.median(x), "min": min(x), "max": max(x)} for k, x in v.items()}

    sm = {k: statistics.median(v) for k, v in stream.items()}
    wm = {k: statistics.median(v) for k, v in wall.items()}
    return {"precision": precision, "scenarios": S, "worlds_per_scenario": Bs, "B_H_W_N": [B, H, W, N], "chunk_steps": K,
            "rounds": rounds, "stream_ms_per_chunk": summary(stream), "wall_ms_per_chunk": summary(wall),
            "A_over_B_stream": sm["A"] / sm["B"], "A_over_B_wall": wm["A"] / wm["B"],
            "A1_over_B_stream": sm["A1"] / sm["B"], "A1_over_B_wall": wm["A1"] / wm["B"],
            "C_over_A_stream": sm["C"] / sm["A"], "C_over_A_wall": wm["C"] / wm["A"],
            "D_over_A_stream": sm["D"] / sm["A"], "D_over_A_wall": wm["D"] / wm["A"],
            "A_faster_than_C_ranges_apart": bool(max(stream["A"]) < min(stream["C"]) and max(wall["A"]) < min(wall["C"])),
            "records_equal_C": True, "records_equal_D": equal_D, "form": forms[0], "form_C": forms[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "episode_ensemble_trace_bench.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="small ensembles (a check of the tool itself)")
    a = ap.parse_args()
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi
    result = {"tool": "tools/episode_ensemble_trace_bench.py", "build_id": _ffi.load().dw_build_id().decode(),
              "method": "A / A1 / B / C / D interleaved in one process, each from one restored snapshot, one untimed round in which "
                        "the records of A and C are asserted equal, then the timed rounds: median, min, max; stream = HIP events "
                        "around the call (copies + kernels; D: summed over its handles), wall = perf_counter.",
              "cases": []}
    shapes = [(README_TABLE, 5, 8, 8, 4), (SMALL_TABLE, 2, 16, 16, 16)] if a.quick else \
             [(README_TABLE, 125, 8, 8, 4), (SMALL_TABLE, 16, 16, 16, 16)]
    for scenarios, Bs, H, W, N in shapes:
        for precision in ("exact", "fast"):
            r = chunk_arms(amd, _ffi, scenarios, Bs, H, W, N, precision, a.rounds)
            result["cases"].append(r)
            print(f"{r['B_H_W_N']} {precision} ({r['form']} | {r['form_C']}): stream ms/chunk " +
                  ", ".join(f"{k} {v['median']:.3f} [{v['min']:.3f}, {v['max']:.3f}]" for k, v in r["stream_ms_per_chunk"].items()) +
                  "; wall ms/chunk " +
                  ", ".join(f"{k} {v['median']:.3f} [{v['min']:.3f}, {v['max']:.3f}]" for k, v in r["wall_ms_per_chunk"].items()) +
                  f"; A/B stream {r['A_over_B_stream']:.3f} wall {r['A_over_B_wall']:.3f}; A1/B stream {r['A1_over_B_stream']:.3f} "
                  f"wall {r['A1_over_B_wall']:.3f}; C/A stream {r['C_over_A_stream']:.2f} wall {r['C_over_A_wall']:.2f}; D/A stream "
                  f"{r['D_over_A_stream']:.2f} wall {r['D_over_A_wall']:.2f}; A < C with ranges apart {r['A_faster_than_C_ranges_apart']}; "
                  f"records equal D {r['records_equal_D']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
