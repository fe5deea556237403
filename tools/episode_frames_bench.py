#!/usr/bin/env python3
"""episode_frames_bench.py — what the frames cost in the episode loop and what they buy (dw_run_episode_frames).

    python tools/episode_frames_bench.py [--out profiles/episode_frames_bench.json] [--rounds 9] [--quick]

Cases: 1000 worlds of 8x8 with 4 greedy agents, 64 steps, 1 x 1 tiles, stride 1 - once with worlds = [0, 1, 2, 3] and once
with all worlds - and 64 worlds of 16x16 with 16 agents, 4 x 4 tiles, stride 8; both precisions.  The arms are INTERLEAVED
in one process (tools/episode_temp_trace_bench.py's way), each from the same restored snapshot of a quantised state:
    TEMPS   one dw_run_episode_trace_temperature call (episode_wave_temp_pw, unchanged): flags, cover and temperature records
    FRAMES  one dw_run_episode_frames call with the same records and cover, temperature and agent frames
    STEPS   64 x (dw_run_episode of one step + dw_reduce_tiles + dw_download_agents): the only way to the frames before
    NOWAVE  the FRAMES call on a second handle created under DW_NO_EPISODE_WAVE, from the same state: launches per step
Per arm: time on the handle's stream from HIP events around the arm (uploads, kernels, downloads) and wall clock, per
chunk and per step, medians after one warm-up round.  FRAMES's records are compared with TEMPS's byte for byte, its frames
with STEPS's and NOWAVE's; `frame_bytes` is what the frames of a chunk move to the host.
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


def chunk_arms(amd, _ffi, shape, precision, rounds, tile, stride, worlds, K=64):
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
    pick = slice(None) if worlds is None else np.asarray(worlds)

    def frames_of(e):
        return e.run_episode_frames(Ls, _ffi.POLICY_ARGMAX, stride=stride, tile=tile, worlds=worlds, temps=True)

    def single_steps():
        cov, tmp, ag = [], [], []
        for t in range(K):
            eng.run_episode(Ls[t:t + 1], _ffi.POLICY_ARGMAX, reuse_buffers=True)
            if (t + 1) % stride:
                continue
            c, m = eng.reduce_tiles(Ls[t], tile=tile, worlds=worlds)
            idx, st = eng.download_agents()
            a = np.zeros(st[pick].shape, dtype=_ffi.AGENT_FRAME_DTYPE)
            a["row"], a["col"], a["state"] = idx[pick][..., 0], idx[pick][..., 1], st[pick]
            cov.append(c), tmp.append(m), ag.append(a)
        return np.array(cov), np.array(tmp), np.array(ag)

    arms = (("TEMPS", eng, lambda: eng.run_episode_trace(Ls, _ffi.POLICY_ARGMAX, temperature=True)),
            ("FRAMES", eng, lambda: frames_of(eng)),
            ("STEPS", eng, single_steps),
            ("NOWAVE", slow, lambda: frames_of(slow)))
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
    cov, tmp, ag, stats, alive, ok, temps = out["FRAMES"]
    records_equal = bool(all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip((stats, alive, ok, temps), out["TEMPS"])))
    frames_equal_steps = bool(all(a.tobytes() == b.tobytes() for a, b in zip((cov, tmp, ag), out["STEPS"])))
    frames_equal_nowave = bool(all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(out["FRAMES"], out["NOWAVE"])))
    forms = [e.kernel_info().split("; episode frames: ", 1)[-1].split(";")[0] for e in (eng, slow)]
    eng.close()
    slow.close()
    sm = {k: statistics.median(v) for k, v in stream.items()}
    wm = {k: statistics.median(v) for k, v in wall.items()}
    return {"precision": precision, "B_H_W_N": [B, H, W, N], "chunk_steps": K, "tile": list(tile), "stride": stride,
            "worlds": "all" if worlds is None else list(worlds), "frames": K // stride,
            "frame_bytes": int(cov.nbytes + tmp.nbytes + ag.nbytes), "record_bytes": int(stats.nbytes + alive.nbytes + ok.nbytes + temps.nbytes),
            "rounds": rounds,
            "stream_ms_per_chunk_median": sm, "stream_ms_per_chunk_min": {k: min(v) for k, v in stream.items()},
            "wall_ms_per_chunk_median": wm, "stream_us_per_step_median": {k: v * 1e3 / K for k, v in sm.items()},
            "wall_us_per_step_median": {k: v * 1e3 / K for k, v in wm.items()},
            "FRAMES_over_TEMPS_stream": sm["FRAMES"] / sm["TEMPS"], "FRAMES_over_TEMPS_wall": wm["FRAMES"] / wm["TEMPS"],
            "STEPS_over_FRAMES_stream": sm["STEPS"] / sm["FRAMES"], "STEPS_over_FRAMES_wall": wm["STEPS"] / wm["FRAMES"],
            "NOWAVE_over_FRAMES_stream": sm["NOWAVE"] / sm["FRAMES"], "NOWAVE_over_FRAMES_wall": wm["NOWAVE"] / wm["FRAMES"],
            "records_equal_TEMPS": records_equal, "frames_equal_STEPS": frames_equal_steps, "frames_equal_NOWAVE": frames_equal_nowave,
            "form": forms[0], "form_NOWAVE": forms[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "episode_frames_bench.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="small ensembles (a check of the tool itself)")
    a = ap.parse_args()
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi
    result = {"tool": "tools/episode_frames_bench.py", "build_id": _ffi.load().dw_build_id().decode(),
              "method": "TEMPS / FRAMES / STEPS / NOWAVE interleaved in one process, each from one restored snapshot, one warm-up "
                        "round, median of the timed rounds; stream = HIP events around the arm (copies + kernels), wall = perf_counter.",
              "cases": []}
    small, large = ((40, 8, 8, 4), (8, 16, 16, 16)) if a.quick else ((1000, 8, 8, 4), (64, 16, 16, 16))
    cases = [(small, (1, 1), 1, [0, 1, 2, 3]), (small, (1, 1), 1, None), (large, (4, 4), 8, None)]
    for shape, tile, stride, worlds in cases:
        for precision in ("exact", "fast"):
            r = chunk_arms(amd, _ffi, shape, precision, a.rounds, tile, stride, worlds)
            result["cases"].append(r)
            print(f"{shape} tile {tile} stride {stride} worlds {r['worlds']} {precision} ({r['form']} | {r['form_NOWAVE']}): "
                  f"frames {r['frame_bytes']} B, records {r['record_bytes']} B; stream us/step " +
                  ", ".join(f"{k} {v:.3f}" for k, v in r["stream_us_per_step_median"].items()) + "; wall us/step " +
                  ", ".join(f"{k} {v:.3f}" for k, v in r["wall_us_per_step_median"].items()) +
                  f"; FRAMES/TEMPS stream {r['FRAMES_over_TEMPS_stream']:.3f} wall {r['FRAMES_over_TEMPS_wall']:.3f}; STEPS/FRAMES stream "
                  f"{r['STEPS_over_FRAMES_stream']:.2f} wall {r['STEPS_over_FRAMES_wall']:.2f}; NOWAVE/FRAMES stream "
                  f"{r['NOWAVE_over_FRAMES_stream']:.2f} wall {r['NOWAVE_over_FRAMES_wall']:.2f}; records equal {r['records_equal_TEMPS']}, "
                  f"frames equal {r['frames_equal_STEPS']} {r['frames_equal_NOWAVE']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
