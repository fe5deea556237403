#!/usr/bin/env python3
"""What dw_run_episode_mlp_counts costs against the existing calls on unchanged code (notebook
daisy_world_existential_risk_and_agency.ipynb, cells fd8ad489 .. 227e4895: the agent-count scans).

usage: agent_count_sweep_bench.py [--out profiles/agent_count_sweep_bench.json] [--rounds 9] [--quick]
           the arms of each shape INTERLEAVED in one process, one 64-step chunk per arm and round from the same restored
           snapshot, one warm-up round, then medians / min / max of `rounds` rounds; stream = dw_timer_start / dw_timer_stop
           around the call(s) (uploads, kernels, downloads), wall = perf_counter around the same.
             (a) scan   10 counts (1, 31, .. 271) x 10 worlds of 16x16, N = 271: the count call; the same call on a handle
                        created under DW_NO_EPISODE_KERNEL; ten handles with their own n_agents, each dw_run_episode_mlp_trace
                        (their times added up)
             (b) demo   64 worlds of 16x16, 16 agents, all counts = N: the count call; dw_run_episode_mlp_trace (launches per
                        step there); dw_run_episode_mlp (workgroup kernel, no records)
             (c) es     64 x 32 worlds of 16x16, 4 agents, all counts = N: the count call; dw_run_episode_mlp_trace (one wave
                        per world)
       agent_count_sweep_bench.py --resources [--out ...]
           registers, LDS and scratch of the new kernels from one gfx950 compilation (tools/isa_report.py; no GPU needed),
           folded into the result file"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

K = 64
L0 = 0.9


def _spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def _engine(amd, B, dim, N, switch=None):
    """A handle after init_random(quantised) and one zero-action step - current and previous state quantised, the whole
    chunk takes the form the handle names - with that state in snapshot slot 0."""
    if switch:
        os.environ[switch] = "1"
    try:
        eng = amd.Engine(amd.default_params(B, dim, dim, N))
    finally:
        if switch:
            del os.environ[switch]
    eng.init_random(42, quantised=True)
    eng.step(L0, np.zeros((B, N, 1), dtype=np.int64) if N else None)
    eng.snapshot_save()
    return eng


def _timed(engines, call):
    """stream ms (added up over the engines) and wall ms of `call(eng)` on each engine, each from its restored snapshot"""
    for eng in engines:
        eng.snapshot_restore()
        eng.sync()
    t0 = time.perf_counter()
    ms, out = 0.0, []
    for eng in engines:
        eng.timer_start()
        out.append(call(eng))
        ms += eng.timer_stop()
    return ms, (time.perf_counter() - t0) * 1e3, out


def _run(arms, rounds):
    """arms: {name: (engines, call)} -> ({name: {stream_ms, wall_ms}}, {name: last outputs})"""
    stream, wall, last = {a: [] for a in arms}, {a: [] for a in arms}, {}
    for r in range(rounds + 1):                                # round 0 warms up (allocations, first launches)
        for name, (engines, call) in arms.items():
            ms, w, last[name] = _timed(engines, call)
            if r:
                stream[name].append(ms)
                wall[name].append(w)
    return {a: {"stream_ms_per_chunk": _spread(stream[a]), "wall_ms_per_chunk": _spread(wall[a])} for a in arms}, last


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def scan(amd, rounds, quick):
    counts = [1, 4, 7] if quick else list(range(1, 272, 30))
    Bs, dim, N = (2, 16, 7) if quick else (10, 16, 271)
    B = len(counts) * Bs
    n_active = np.repeat(np.asarray(counts, dtype=np.int32), Bs)
    Ls = np.linspace(0.9, 1.0, K)
    params = np.random.RandomState(7).randn(1, 1808) * 0.5
    big, step = _engine(amd, B, dim, N), _engine(amd, B, dim, N, "DW_NO_EPISODE_KERNEL")
    ten = [_engine(amd, Bs, dim, c) for c in counts]
    arms = {"counts": ([big], lambda e: e.run_episode_mlp_counts(Ls, params, n_active, split=N)),
            "counts_launches_per_step": ([step], lambda e: e.run_episode_mlp_counts(Ls, params, n_active, split=N)),
            "one_handle_per_count_mlp_trace": (ten, lambda e: e.run_episode_mlp(Ls, params, split=e.N, trace=True))}
    res, last = _run(arms, rounds)
    a, b = last["counts"][0], last["counts_launches_per_step"][0]
    out = {"shape": {"counts": counts, "worlds_per_count": Bs, "grid": dim, "n_agents": N, "chunk_steps": K}, "arms": res,
           "forms": {"counts": big.kernel_info().split("; mlp counts: ", 1)[-1].split(";")[0],
                     "counts_launches_per_step": step.kernel_info().split("; mlp counts: ", 1)[-1].split(";")[0],
                     "one_handle_per_count_mlp_trace": sorted({e.kernel_info().split("; mlp trace: ", 1)[-1].split(";")[0] for e in ten})},
           "same_bits_both_forms": _bits(a[0]) == _bits(b[0]) and _bits(a[2]) == _bits(b[2]),
           "live_cover_at_the_end": int(a[2]["max_k"][-1].max()), "rewards_positive": bool((a[0] > 0).any())}
    for e in [big, step, *ten]:
        e.close()
    return out


def all_present(amd, rounds, B, dim, N, with_plain):
    n_active = np.full(B, N, dtype=np.int32)
    Ls = np.linspace(0.9, 1.0, K)
    params = np.random.RandomState(7).randn(1, 1808) * 0.5
    eng = _engine(amd, B, dim, N)
    arms = {"counts": ([eng], lambda e: e.run_episode_mlp_counts(Ls, params, n_active, split=N)),
            "mlp_trace": ([eng], lambda e: e.run_episode_mlp(Ls, params, split=N, trace=True))}
    if with_plain:
        arms["mlp_no_records"] = ([eng], lambda e: e.run_episode_mlp(Ls, params, split=N))
    res, last = _run(arms, rounds)
    info = eng.kernel_info()
    a, b = last["counts"][0], last["mlp_trace"][0]
    out = {"shape": {"worlds": B, "grid": dim, "n_agents": N, "chunk_steps": K}, "arms": res,
           "forms": {"counts": info.split("; mlp counts: ", 1)[-1].split(";")[0],
                     "mlp_trace": info.split("; mlp trace: ", 1)[-1].split(";")[0],
                     "mlp_no_records": info.split("; mlp episode: ", 1)[-1].split(";")[0]},
           "same_bits_as_mlp_trace": _bits(a[0]) == _bits(b[0]) and _bits(a[2]) == _bits(b[2])}
    eng.close()
    return out


def measure(a):
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi
    result = {"tool": "tools/agent_count_sweep_bench.py", "build_id": _ffi.load().dw_build_id().decode(), "rounds": a.rounds,
              "method": "the arms of a shape interleaved in one process; every arm and round runs one 64-step chunk from the same "
                        "restored snapshot (current and previous state quantised); one warm-up round, then `rounds` timed rounds: "
                        "median, min, max.  stream = dw_timer_start / dw_timer_stop around the call (for the ten handles: added "
                        "up), wall = perf_counter around the same."}
    result["scan"] = scan(amd, a.rounds, a.quick)
    result["demo"] = all_present(amd, a.rounds, 8 if a.quick else 64, 16, 16, True)
    result["es"] = all_present(amd, a.rounds, 16 if a.quick else 64 * 32, 16, 4, False)
    for name in ("scan", "demo", "es"):
        case = result[name]
        print(name, json.dumps(case["shape"]), {k: v for k, v in case.items() if k.startswith("same") or k.startswith("live")})
        for arm, r in case["arms"].items():
            s, w = r["stream_ms_per_chunk"], r["wall_ms_per_chunk"]
            print(f"  {arm:34s} {case['forms'].get(arm)!s:28s} stream {s['median']:9.3f} ms [{s['min']:.3f}, {s['max']:.3f}]  "
                  f"wall {w['median']:9.3f} ms [{w['min']:.3f}, {w['max']:.3f}]", flush=True)
    _merge(a.out, result)


def _merge(path, update):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    result = {}
    if os.path.exists(path):
        with open(path) as f:
            result = json.load(f)
    result.update(update)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", path)


def resources(a):
    import isa_report
    text = open(isa_report.build([])).read()
    out = {}
    for name in re.findall(r"\.amdhsa_kernel (\S+)\n", text):
        if not any(stem in name for stem in ("episode_mlp_counts_pw", "observe_counts_pw", "zero_absent_states_pw")):
            continue
        info = re.search(re.escape(name) + r":.*?; Kernel info:(.*?)(?=\n\t\.(?:text|section)|\Z)", text, re.S)
        vals = {k: int(v) for k, v in re.findall(r"; (\w+)\s*[:=] (\d+)", info.group(1))}
        out[name] = {k: vals[k] for k in ("NumVgprs", "NumAgprs", "TotalNumSgprs", "Occupancy", "LDSByteSize", "ScratchSize") if k in vals}
        print(name, out[name])
    _merge(a.out, {"kernel_resources": {"source": "tools/isa_report.py: one hipcc --offload-arch=gfx950 --save-temps compilation; "
                                                  "LDSByteSize is the static part (the workgroup kernel adds its dynamic LDS)",
                                        "kernels": out}})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agent_count_sweep_bench.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="small shapes (a check of the tool itself)")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    return resources(a) if a.resources else measure(a)


if __name__ == "__main__":
    main()
