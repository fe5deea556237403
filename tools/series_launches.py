#!/usr/bin/env python3
"""series_launches.py — one call of each step-series and episode entry point, for a count of kernel launches.

    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/series_launches.py

On a wide-grid plan that takes step pairs (3 worlds of 70 x 320, float32-only) and on an 8 x 8 plan that takes the
one-wave-per-world episode kernels (6 worlds, 2 agents each): dw_step_n_trace, dw_step_n_trace_temperature (shared L and
per-world), dw_step_n_trace_per_world, dw_step_n_trace_ensemble (with and without temperature records), dw_run_episode,
dw_run_episode_ensemble and dw_run_episode_trace, 11 steps each, from an un-quantised and from a quantised state.  Two builds of the library that
launch the same kernels the same number of times give the same per-kernel call counts (profiles/series_launches_*).
DW_LIB selects the library.  Prints what was called; the numbers are the profiler's.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi
    n = 11
    for (B, H, W, N), precision in (((3, 70, 320, 2), "fast"), ((6, 8, 8, 2), "exact")):
        p = amd.default_params(B, H, W, N)
        p.precision = _ffi.PRECISION[precision]
        eng = amd.Engine(p)
        L = 0.8 + 0.002 * np.arange(n)[:, None] + 0.01 * np.arange(B)[None, :]
        L[:5] = L[0]                                        # steps that share a row of the per-world table
        tab = np.repeat(eng.world_params()[None], B)
        tab["q2"][1] = 0.0
        for quantised in (False, True):
            eng.init_random(3, quantised=quantised)
            eng.step_n_trace(L[:, 0])
            eng.step_n_trace_temperature(L[:, 0])
            eng.step_n_trace_temperature(L)
            eng.step_n_trace_per_world(L)
            eng.step_n_trace_ensemble(tab, L)
            eng.step_n_trace_ensemble(tab, L, temperature=True)
            eng.step(0.9)                                   # (the episode calls want a shared-L predecessor)
            table = np.random.RandomState(1).randint(-2, 9, size=(n, B, N)).astype(np.int8)
            use = (np.arange(n) % 2).astype(np.uint8)
            eng.run_episode(L[:, 0], 0, use_table=use, table=table)
            eng.run_episode_ensemble(tab, L, 0, use_table=use, table=table)
            eng.run_episode_trace(L[:, 0], 0, use_table=use, table=table)
            eng.step(0.9)
        print(f"{(B, H, W, N)} {precision}: {eng.kernel_info()}")
        eng.close()


if __name__ == "__main__":
    main()
