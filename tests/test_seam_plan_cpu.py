"""The plan rule of the seam-strip layout (csrc/dw_plan.hpp: seam_layout, StepPlan::seam_strips / seam_geom / left_geom),
without a GPU: tests/seam_plan_driver.cpp includes only dw_plan.hpp and is compiled as plain C++17 by the clang++ of ROCm,
as tests/test_plan_cpu.py compiles its driver.

The rule, for un-packed float32 plans that take format-access step pairs on overlapped strips: n_full = W // 252 whole seam
strips per row band, L = W - 252 n_full columns left over, which take L/4 + 2 lanes per row band, so G = 64 // (L/4 + 2) row
bands of a world share a leftover wave; a world takes nrs * n_full + ceil(nrs / G) waves, and the layout is planned only
where that is below the nrs * ceil(W / 248) waves of the overlapped strips.  The expected numbers below are written out by
hand from that rule, and checked against it once more in Python.
"""
import json
import os
import subprocess

import pytest

from test_plan_cpu import CSRC, ROOT, _rocm_clang

EXACT, FAST = 0, 1


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    clang = _rocm_clang()
    if clang is None:
        pytest.skip("the clang++ of ROCm is not installed")
    exe = tmp_path_factory.mktemp("seam_plan") / "seam_plan_driver"
    subprocess.check_call([clang, "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CSRC,
                           os.path.join(ROOT, "tests", "seam_plan_driver.cpp"), "-o", str(exe)])

    def run(B, H, W, precision=FAST, strip_rows=64, no_seam=0, no_fmt=0):
        out = subprocess.run([str(exe), *map(str, (B, H, W, precision, strip_rows, no_seam, no_fmt))], capture_output=True,
                             text=True, check=True)
        return json.loads(out.stdout)[0]
    return run


def _rule(W, nrs):
    n_full = W // 252
    L = W - 252 * n_full
    G = 64 // (L // 4 + 2) if L else 0
    return n_full, L, G, nrs * n_full + (-(-nrs // G) if L else 0), nrs * -(-W // 248)


# W: (n_full, L, lanes per band, G, waves per world, waves per world of the overlapped strips) at 8 row bands (H = 512)
CASES = {
    316: (1, 64, 18, 3, 8 + 3, 16),
    504: (2, 0, 0, 0, 16, 24),
    520: (2, 16, 6, 10, 16 + 1, 24),
    760: (3, 4, 3, 21, 24 + 1, 32),
    1280: (5, 20, 7, 9, 40 + 1, 48),
    4096: (16, 64, 18, 3, 128 + 3, 136),
    8192: (32, 128, 34, 1, 256 + 8, 272),
}


@pytest.mark.parametrize("W", sorted(CASES))
def test_wave_counts(plan, W):
    n_full, L, lanes, G, waves, old = CASES[W]
    assert _rule(W, 8) == (n_full, L, G, waves, old)
    B = 3
    s = plan(B, 512, W)
    assert s["fmt_planes"] == 1 and s["seam_strips"] == 1 and s["fused_mode"] == 0, s
    assert (s["nrs"], s["old_ncs"], s["old_nstrips"]) == (8, old // 8, B * old), s
    assert (s["n_full"], s["seam_cols"], s["seam_nstrips"]) == (n_full, 252, B * 8 * n_full), s
    assert s["waves_per_world"] == waves and waves < old
    if L:
        assert (s["left_cols"], s["left_lanes"], s["left_bands"]) == (L, lanes, G), s
        assert s["left_nstrips"] == B * -(-8 // G) and lanes * G <= 64
    else:
        assert s["left_nstrips"] == 0 and s["left_nwg"] == 0 and s["left_chunk"] == 0, s
    assert s["seam_nstrips"] + s["left_nstrips"] == B * waves
    for k in ("seam", "left"):                                  # four waves to a workgroup, eight chunks of workgroups
        assert s[k + "_nwg"] == -(-s[k + "_nstrips"] // 4) and s[k + "_chunk"] == -(-s[k + "_nwg"] // 8), s


def test_the_headline_shape_takes_1046_waves_per_world_for_1088(plan):
    s = plan(1024, 4096, 4096, strip_rows=0)                    # the plan's own strip height: 64 rows
    assert s["seam_strips"] == 1 and s["nrs"] == 64
    assert s["old_nstrips"] == 1024 * 1088 and s["old_ncs"] == 17
    assert s["waves_per_world"] == 1046 == 64 * 16 + 22
    assert (s["seam_nstrips"], s["left_nstrips"]) == (1024 * 64 * 16, 1024 * 22)
    assert (s["left_cols"], s["left_lanes"], s["left_bands"]) == (64, 18, 3)


@pytest.mark.parametrize("case", [
    dict(W=256),                                                # rotating strips: no overlap to begin with
    dict(W=1024),                                               # the ring of four waves
    dict(W=496),                                                # 2 x 248: 1 seam strip + 244 columns (63 lanes) are two waves too
    dict(W=4096, precision=EXACT),
    dict(W=4096, no_seam=1),
    dict(W=4096, no_fmt=1),                                     # the seam kernels are format-access kernels
], ids=lambda c: " ".join(f"{k}={v}" for k, v in c.items()))
def test_layout_is_off(plan, case):
    case = dict(case)
    s = plan(2, 512, case.pop("W"), **case)
    assert s["seam_strips"] == 0, s
    assert s["seam_nstrips"] == 0 and s["left_nstrips"] == 0 and s["n_full"] == 0, s


def test_switch_leaves_the_format_kernel_on(plan):
    s = plan(2, 512, 4096, no_seam=1)
    assert s["fmt_planes"] == 1 and s["seam_strips"] == 0
