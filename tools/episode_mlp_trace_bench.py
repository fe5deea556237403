#!/usr/bin/env python3
"""episode_mlp_trace_bench.py — what the per-step cover and temperature records cost in the MLP episode loop and what they
buy (dw_run_episode_mlp_trace).

    python tools/episode_mlp_trace_bench.py [--out profiles/episode_mlp_trace_bench.json] [--rounds 9] [--quick]

At the ES shape (64 members x 32 worlds of 16x16, 4 agents, every world's agents driven by its member) and at 1000 worlds of
8x8 with 4 agents (one parameter set), both precisions, 64-step chunks; the arms INTERLEAVED in one process
(tools/episode_temp_trace_bench.py's way), each from the same restored snapshot of a quantised state:
    MLP     one dw_run_episode_mlp call (episode_mlp_wave, unchanged): rewards and done flags
    TRACE   one dw_run_episode_mlp_trace call with cover records only (episode_mlp_wave_trace_pw<., false>)
    BOTH    ... with cover and temperature records (episode_mlp_wave_trace_pw<., true>)
    NOWAVE  the BOTH call on a second handle created under DW_NO_EPISODE_WAVE, from the same state: launches per step
    STEPS   64 x (dw_policy_mlp_population + dw_step_device_actions + dw_reduce + dw_reduce_temperature): the only way to
            both records before (dw_policy_mlp's kernel with the member map)
Per arm: time on the handle's stream from HIP events around the arm (uploads, kernels, downloads) and wall clock, per
chunk and per step, medians after one warm-up round.  BOTH's rows are compared with NOWAVE's and STEPS's byte for byte, its
rewards with MLP's.
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


def chunk_arms(amd, _ffi, shape, members, precision, rounds, K=64):
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
        e.init_random(42, quantised=True)
        e.step(0.9, np.zeros((B, N, 1), dtype=np.int64))        # current and previous state quantised: the whole chunk in one form
        e.snapshot_save()
        return e

    eng, slow = engine(), engine("DW_NO_EPISODE_WAVE")
    Ls = np.linspace(0.9, 1.0, K)
    params = np.random.RandomState(7).randn(members, 1808) * 0.5
    member = (np.arange(B) * members // B).astype(np.int32)

    def single_steps():
        rows = np.zeros((K, B), dtype=_ffi.STATS_DTYPE)
        temps = np.zeros((K, B), dtype=_ffi.TEMP_STATS_DTYPE)
        for t in range(K):
            eng.policy_mlp_population(params, member, 0, N)
            eng.step_device_actions(Ls[t])
            rows[t] = eng.reduce()
            temps[t] = eng.reduce_temperature(Ls[t])
        return rows, temps

    def episode(e, **kw):
        return lambda: e.run_episode_mlp(Ls, params, member, member, N, reuse_buffers=True, **kw)

    arms = (("MLP", eng, episode(eng)),
            ("TRACE", eng, episode(eng, trace=True)),
            ("BOTH", eng, episode(eng, trace=True, temperature=True)),
            ("NOWAVE", slow, episode(slow, trace=True, temperature=True)),
            ("STEPS", eng, single_steps))
    stream = {name: [] for name, _, _ in arms}
    wall = {name: [] for name, _, _ in arms}
    out = {}
    for r in range(rounds + 1):                                # round 0 warms up (allocations, first launches)
        for name, e, fn in arms:
            e.snapshot_restore()
            e.sync()
            t0 = time.perf_counter()
            e.timer_start()
            res = fn()
            ms = e.timer_stop()
            w = (time.perf_counter() - t0) * 1e3
            out[name] = tuple(None if a is None else np.array(a) for a in res)     # (the reward buffers are reused)
            if r:
                stream[name].append(ms)
                wall[name].append(w)
    reward, done, stats, temps = out["BOTH"]
    rewards_equal = bool(all(reward.tobytes() == out[k][0].tobytes() and np.array_equal(done, out[k][1])
                             for k in ("MLP", "TRACE", "NOWAVE")))
    records_equal = bool(stats.tobytes() == out["TRACE"][2].tobytes() and stats.tobytes() == out["NOWAVE"][2].tobytes()
                         and temps.tobytes() == out["NOWAVE"][3].tobytes())
    stats_s, temps_s = out["STEPS"]
    equal_steps = bool(temps.tobytes() == temps_s.tobytes() and
                       all(np.array_equal(stats[f], stats_s[f]) for f in ("max_k", "sum_light_k", "sum_dark_k")))
    forms = [e.kernel_info().split("; mlp trace: ", 1)[-1].split(";")[0] for e in (eng, slow)]
    eng.close()
    slow.close()
    sm = {k: statistics.median(v) for k, v in stream.items()}
    wm = {k: statistics.median(v) for k, v in wall.items()}
    ratios = {}
    for a, b in (("TRACE", "MLP"), ("BOTH", "MLP"), ("BOTH", "TRACE"), ("NOWAVE", "BOTH"), ("STEPS", "BOTH")):
        ratios[f"{a}_over_{b}_stream"] = sm[a] / sm[b]
        ratios[f"{a}_over_{b}_wall"] = wm[a] / wm[b]
    return {"precision": precision, "B_H_W_N": [B, H, W, N], "members": members, "chunk_steps": K, "rounds": rounds,
            "stream_ms_per_chunk_median": sm, "stream_ms_per_chunk_min": {k: min(v) for k, v in stream.items()},
            "wall_ms_per_chunk_median": wm, "stream_us_per_step_median": {k: v * 1e3 / K for k, v in sm.items()},
            "wall_us_per_step_median": {k: v * 1e3 / K for k, v in wm.items()}, **ratios,
            "rewards_equal_MLP_TRACE_NOWAVE": rewards_equal, "records_equal_TRACE_NOWAVE": records_equal,
            "records_equal_STEPS": equal_steps, "form": forms[0], "form_NOWAVE": forms[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "episode_mlp_trace_bench.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="small ensembles (a check of the tool itself)")
    a = ap.parse_args()
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi
    result = {"tool": "tools/episode_mlp_trace_bench.py", "build_id": _ffi.load().dw_build_id().decode(),
              "method": "MLP / TRACE / BOTH / NOWAVE / STEPS interleaved in one process, each from one restored snapshot, one "
                        "warm-up round, median of the timed rounds; stream = HIP events around the arm (copies + kernels), "
                        "wall = perf_counter.",
              "cases": []}
    shapes = [((16, 16, 16, 4), 4), ((40, 8, 8, 4), 1)] if a.quick else [((64 * 32, 16, 16, 4), 64), ((1000, 8, 8, 4), 1)]
    for shape, members in shapes:
        for precision in ("exact", "fast"):
            r = chunk_arms(amd, _ffi, shape, members, precision, a.rounds)
            result["cases"].append(r)
            print(f"{shape} {precision} ({r['form']} | {r['form_NOWAVE']}): stream us/step " +
                  ", ".join(f"{k} {v:.3f}" for k, v in r["stream_us_per_step_median"].items()) + "; wall us/step " +
                  ", ".join(f"{k} {v:.3f}" for k, v in r["wall_us_per_step_median"].items()) +
                  f"; TRACE/MLP stream {r['TRACE_over_MLP_stream']:.3f}; BOTH/MLP stream {r['BOTH_over_MLP_stream']:.3f}; "
                  f"NOWAVE/BOTH stream {r['NOWAVE_over_BOTH_stream']:.2f} wall {r['NOWAVE_over_BOTH_wall']:.2f}; STEPS/BOTH stream "
                  f"{r['STEPS_over_BOTH_stream']:.2f} wall {r['STEPS_over_BOTH_wall']:.2f}; equal: rewards "
                  f"{r['rewards_equal_MLP_TRACE_NOWAVE']}, records {r['records_equal_TRACE_NOWAVE']} {r['records_equal_STEPS']}",
                  flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
