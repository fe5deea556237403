#!/usr/bin/env python3
"""frames_bench.py — what spatial frames cost (dw_step_n_frames, dw_reduce_tiles), on one GPU.

    python tools/frames_bench.py [--out profiles/frames_bench.json] [--rounds 9] [--quick]

Every figure is the time between dw_timer_start and dw_timer_stop (HIP events on the handle's stream) around one call -
or, for the host loop, around the whole loop; the arms of a comparison are interleaved in one process from one restored
device snapshot; one warm-up round, then the median of `--rounds` rounds.

  1  64 worlds of 256^2, 512 steps, stride 8, 4 x 4 tiles, cover alone and cover + temperature:
       T  dw_step_n_trace                the run without frames: F / T is the price of frames
       F  dw_step_n_frames
       P  the only way before: dw_step_n_trace per 8 steps + dw_download_planes (+ dw_download_caches, temps only) + NumPy
          block means: P / F
  2  1024 worlds of 256^2, 1024 steps, stride 16, 16 x 16 tiles, cover alone
  3  1000 worlds of 8 x 8, 1000 steps, stride 1, 1 x 1 tiles, both outputs (the notebooks' animation data)
  4  dw_reduce_tiles at 64 and 1024 worlds of 256^2, 16 x 16 tiles: cover alone and temperature alone, as bytes read (4 per
     cell: two binary16 planes) over time
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIN_L, MAX_L, DL = 0.75, 1.5, 0.75 / 512


def ramp(n):
    return np.minimum(MIN_L + DL * np.arange(n), MAX_L)


def engine(amd, _ffi, B, H, W, precision):
    p = amd.default_params(B, H, W, 0)
    p.precision = _ffi.PRECISION[precision]
    eng = amd.Engine(p)
    eng.init_random(42, quantised=True)
    eng.step(MIN_L)                                             # a retained previous state in binary16
    eng.snapshot_save()
    return eng


def interleaved(eng, arms, rounds, restore=True):
    """arms: (name, fn) -> {name: {median, min, max}} in ms per call"""
    times = {k: [] for k, _ in arms}
    for rep in range(rounds + 1):                               # round 0 warms up
        for name, fn in arms:
            if restore:
                eng.snapshot_restore()
            eng.sync()
            eng.timer_start()
            fn()
            dt = eng.timer_stop()
            if rep:
                times[name].append(dt)
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}


def block_means(a, th, tw):
    B, H, W = a.shape
    return a.reshape(B, H // th, th, W // tw, tw).mean(axis=(2, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_bench.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--precision", default="fast")
    ap.add_argument("--quick", action="store_true", help="small shapes (a check of the tool itself)")
    a = ap.parse_args()
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi
    q = a.quick
    result = {"tool": "tools/frames_bench.py", "build_id": _ffi.load().dw_build_id().decode(), "precision": a.precision,
              "rounds": a.rounds, "timing": "dw_timer_start / dw_timer_stop around each call, ms"}

    # 1: the price of frames, and the way through the downloads
    B, H, W = (4, 256, 256) if q else (64, 256, 256)
    steps, stride, tile = (32 if q else 512), 8, (4, 4)
    Ls = ramp(steps)
    eng = engine(amd, _ffi, B, H, W, a.precision)

    def parent_way(temperature):
        def run():
            out = []
            for f in range(steps // stride):
                seg = Ls[f * stride:(f + 1) * stride]
                eng.step_n_trace(seg)
                light, dark = eng.download_planes()
                frame = [block_means(light, *tile), block_means(dark, *tile)]
                if temperature:
                    t = eng.download_caches(float(seg[-1]), betas=False, growth=False, temp_effective=False)[0][:, 0]
                    frame.append(block_means(t, *tile))
                out.append(frame)
            return out
        return run

    r = interleaved(eng, (("T_step_n_trace", lambda: eng.step_n_trace(Ls)),
                          ("F_cover", lambda: eng.step_n_frames(Ls, stride=stride, tile=tile, temperature=False)),
                          ("F_cover_temp", lambda: eng.step_n_frames(Ls, stride=stride, tile=tile)),
                          ("P_cover", parent_way(False)), ("P_cover_temp", parent_way(True))), a.rounds)
    info = eng.kernel_info()
    eng.close()
    m = {k: v["median"] for k, v in r.items()}
    result["price_of_frames"] = {
        "B_H_W": [B, H, W], "steps": steps, "stride": stride, "tile": list(tile), "ms_per_run": r,
        "trace_form": "step pairs" if "trace: step pairs" in info else "single steps",
        "F_over_T_cover": m["F_cover"] / m["T_step_n_trace"], "F_over_T_cover_temp": m["F_cover_temp"] / m["T_step_n_trace"],
        "P_over_F_cover": m["P_cover"] / m["F_cover"], "P_over_F_cover_temp": m["P_cover_temp"] / m["F_cover_temp"]}
    print("1", json.dumps(result["price_of_frames"]), flush=True)

    # 2: a large ensemble, coarse pictures
    B, H, W = (16, 256, 256) if q else (1024, 256, 256)
    steps = 64 if q else 1024
    Ls = ramp(steps)
    eng = engine(amd, _ffi, B, H, W, a.precision)
    r = interleaved(eng, (("T_step_n_trace", lambda: eng.step_n_trace(Ls)),
                          ("F_cover", lambda: eng.step_n_frames(Ls, stride=16, tile=(16, 16), temperature=False))), a.rounds)
    result["ensemble_cover"] = {"B_H_W": [B, H, W], "steps": steps, "stride": 16, "tile": [16, 16], "ms_per_run": r,
                                "F_over_T": r["F_cover"]["median"] / r["T_step_n_trace"]["median"]}
    print("2", json.dumps(result["ensemble_cover"]), flush=True)

    # 4 (on the same handle): one frame on demand, as bytes read over time
    on_demand = {}
    for Bn in ((4, 16) if q else (64, 1024)):
        e2 = eng if Bn == B else engine(amd, _ffi, Bn, H, W, a.precision)
        r = interleaved(e2, (("cover", lambda: e2.reduce_tiles(1.0, tile=(16, 16), temperature=False)),
                             ("temperature", lambda: e2.reduce_tiles(1.0, tile=(16, 16), cover=False))), a.rounds, restore=False)
        cells = Bn * H * W
        on_demand[f"{Bn}x{H}x{W}"] = {"tile": [16, 16], "ms": r, "bytes_read": 4 * cells,
                                      "cover_gbs": 4.0 * cells / (r["cover"]["median"] * 1e-3) / 1e9,
                                      "temperature_gbs": 4.0 * cells / (r["temperature"]["median"] * 1e-3) / 1e9,
                                      "temperature_ns_per_cell": r["temperature"]["median"] * 1e6 / cells,
                                      "includes": "the memset, the kernels, the download of the records"}
        if e2 is not eng:
            e2.close()
    eng.close()
    result["reduce_tiles"] = on_demand
    print("4", json.dumps(on_demand), flush=True)

    # 3: the notebooks' animation data
    B, H, W = (50, 8, 8) if q else (1000, 8, 8)
    steps = 50 if q else 1000
    Ls = ramp(steps)
    eng = engine(amd, _ffi, B, H, W, a.precision)
    r = interleaved(eng, (("T_step_n_trace", lambda: eng.step_n_trace(Ls)),
                          ("F_cover_temp", lambda: eng.step_n_frames(Ls, stride=1, tile=(1, 1)))), a.rounds)
    eng.close()
    result["animation"] = {"B_H_W": [B, H, W], "steps": steps, "stride": 1, "tile": [1, 1], "ms_per_run": r,
                           "F_over_T": r["F_cover_temp"]["median"] / r["T_step_n_trace"]["median"],
                           "frame_bytes": 16 * B * H * W}
    print("3", json.dumps(result["animation"]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
