#!/usr/bin/env python3
"""lifespan_sweep_bench.py — what per-world constants cost in the episode loop and what they buy (dw_run_episode_ensemble).

    python tools/lifespan_sweep_bench.py [--out profiles/lifespan_sweep_bench.json] [--parent-lib PATH] [--rounds 9] [--quick]

(a) 1000 worlds of 8x8 with 4 greedy agents, 64-step chunks, both precisions; arms INTERLEAVED in one process
    (tools/kbench.py's way) from one restored snapshot of a quantised state:
      OWN  dw_run_episode_ensemble, every world on the handle's own constants (episode_wave_pw)
      ONE  dw_run_episode (episode_wave).  With --parent-lib (a library built from the parent commit, same ABI) ONE runs
           on THAT library; without it on this one, whose episode_wave is unchanged
           (tests/test_per_world_cpu.py::test_no_existing_kernel_changed).
    Per arm: time on the handle's stream from HIP events around the call (uploads, the kernel, the flags' download) and
    wall clock (adds the host's derivation of the rows), per chunk and per step; the bytes of OWN's table of rows.
    Neither arm's kernel is timed apart from its copies: `stream` is the closest the C ABI gives.
(b) the 8-scenario lifespan table ({default, neutral albedo} x {greedy, anti-greedy, no agent, greedy at q2 = 0}) x 125
    worlds of 8x8 with 4 agents: ONE simulate_lifespan_sweep call against eight sequential
    simulate_lifespan(final_state=False) runs on the same worlds; wall clock, and the counts are compared.
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


def chunk_ab(amd, _ffi, B, precision, rounds, parent_lib, K=64, H=8, W=8, N=4):
    p = amd.default_params(B, H, W, N)
    p.precision = _ffi.PRECISION[precision]
    eng = amd.Engine(p)
    old = amd.Engine(p, lib_path=parent_lib) if parent_lib else eng
    for e in {id(eng): eng, id(old): old}.values():
        e.init_random(42)
        e.step(0.9, np.zeros((B, N, 1), dtype=np.int64))
        e.snapshot_save()
    Ls = np.linspace(0.9, 1.0, K)
    cols = np.ascontiguousarray(np.repeat(Ls[:, None], B, axis=1))
    own = np.repeat(eng.world_params()[None], B)
    arms = (("OWN", eng, lambda: eng.run_episode_ensemble(own, cols, _ffi.POLICY_ARGMAX)),
            ("ONE", old, lambda: old.run_episode(Ls, _ffi.POLICY_ARGMAX)))
    stream = {name: [] for name, _, _ in arms}
    wall = {name: [] for name, _, _ in arms}
    flags = {}
    for r in range(rounds + 1):                                # round 0 warms up (allocations, first launches)
        for name, e, fn in arms:
            e.snapshot_restore()
            e.sync()
            t0 = time.perf_counter()
            e.timer_start()
            out = fn()
            ms = e.timer_stop()
            w = (time.perf_counter() - t0) * 1e3
            flags[name] = out
            if r:
                stream[name].append(ms)
                wall[name].append(w)
    same = bool(np.array_equal(flags["OWN"][0], flags["ONE"][0]) and np.array_equal(flags["OWN"][1], flags["ONE"][1]))
    info = eng.kernel_info()
    if old is not eng:
        old.close()
    eng.close()
    sm = {k: statistics.median(v) for k, v in stream.items()}
    wm = {k: statistics.median(v) for k, v in wall.items()}
    return {"precision": precision, "B_H_W_N": [B, H, W, N], "chunk_steps": K, "rounds": rounds,
            "stream_ms_per_chunk_median": sm, "stream_ms_per_chunk_min": {k: min(v) for k, v in stream.items()},
            "wall_ms_per_chunk_median": wm, "wall_us_per_step_median": {k: v * 1e3 / K for k, v in wm.items()},
            "OWN_over_ONE_stream": sm["OWN"] / sm["ONE"], "OWN_over_ONE_wall": wm["OWN"] / wm["ONE"],
            "table_bytes_per_chunk": int(K * B * (128 + 8) + B * 128), "flags_equal": same,
            "ONE_library": "parent" if parent_lib else "this build", "form": info.split("; ensemble episode: ", 1)[-1].split(";")[0]}


def lifespan_table(amd, worlds_each, dim=8, N=4, seed=11):
    neutral = {"albedo_light": 0.5, "albedo_dark": 0.5}
    policies = [lambda: amd.Greedy(epsilon=0.0, greedy=True), lambda: amd.Greedy(epsilon=0.0, greedy=False), lambda: None]
    scenarios = [{"params": dict(alb), "agent": pol()} for alb in ({}, neutral) for pol in policies]
    scenarios += [{"params": dict(alb, q2=0.0), "agent": amd.Greedy(epsilon=0.0, greedy=True)} for alb in ({}, neutral)]
    S = len(scenarios)

    def fresh(B, offset):
        env = amd.RLDaisyWorld(grid_dimension=dim, n_agents=N)
        env.batch_size = B
        env.world_offset = offset
        return env

    env = fresh(S * worlds_each, 0)
    env.reset_synthetic(seed)
    obs = env.get_obs()
    t0 = time.perf_counter()
    done_at, agents_done_at, _ = amd.simulate_lifespan_sweep(env, scenarios, worlds_each, obs=obs)
    t_one = time.perf_counter() - t0
    env.close()
    t_seq, equal = 0.0, True
    for s, sc in enumerate(scenarios):
        one = fresh(worlds_each, s * worlds_each)
        for name, value in sc["params"].items():
            setattr(one, name, value)
        one.reset_synthetic(seed)
        obs = one.get_obs()
        t0 = time.perf_counter()
        d, a = amd.simulate_lifespan(one, sc["agent"], obs=obs, final_state=False)
        t_seq += time.perf_counter() - t0
        one.close()
        equal = equal and bool(np.array_equal(d, done_at[s]) and np.array_equal(a, agents_done_at[s]))
    return {"scenarios": S, "worlds_per_scenario": worlds_each, "world": [dim, dim], "agents": N,
            "one_call_wall_s": t_one, "sequential_runs_wall_s": t_seq, "sequential_over_one_call": t_seq / t_one,
            "counts_equal": equal, "mean_lifespan_per_scenario": [float(x) for x in done_at.mean(axis=1)],
            "longest_lifespan": int(done_at.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lifespan_sweep_bench.json"))
    ap.add_argument("--parent-lib", default=None, help="a library built from the parent commit (arm ONE runs on it)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="small ensembles (a check of the tool itself)")
    a = ap.parse_args()
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi, build
    result = {"tool": "tools/lifespan_sweep_bench.py", "build_id": _ffi.load().dw_build_id().decode(),
              "parent_build_id": build.library_id(a.parent_lib) if a.parent_lib else None,
              "method": "(a) OWN / ONE interleaved in one process from one restored snapshot, one warm-up round, median of the "
                        "timed rounds; stream = HIP events around the call (copies + kernel), wall = perf_counter.  (b) wall clock "
                        "of the harness calls, resets excluded, the one-call run first.",
              "chunk_ab": {}}
    B = 40 if a.quick else 1000
    for precision in ("exact", "fast"):
        r = chunk_ab(amd, _ffi, B, precision, a.rounds, a.parent_lib)
        result["chunk_ab"][precision] = r
        print(f"(a) {precision} ({r['form']}): stream " + ", ".join(f"{k} {v:.4f} ms" for k, v in r["stream_ms_per_chunk_median"].items()) +
              "; wall " + ", ".join(f"{k} {v:.4f} ms" for k, v in r["wall_ms_per_chunk_median"].items()) +
              f"; OWN/ONE stream {r['OWN_over_ONE_stream']:.3f} wall {r['OWN_over_ONE_wall']:.3f}; table {r['table_bytes_per_chunk']} B; "
              f"flags equal {r['flags_equal']}", flush=True)
    d = result["lifespan_table"] = lifespan_table(amd, 5 if a.quick else 125)
    print(f"(b) one call {d['one_call_wall_s']:.3f} s, {d['scenarios']} runs {d['sequential_runs_wall_s']:.3f} s, ratio "
          f"{d['sequential_over_one_call']:.2f}, counts equal {d['counts_equal']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
