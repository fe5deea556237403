"""The staging layout of the episode calls (csrc/dw_episode_staging.hpp), without a GPU.

tests/episode_staging_driver.cpp includes only dw_episode_staging.hpp and is compiled here as plain C++17 by the clang++
that ships with ROCm (the recipe of test_plan_cpu.py; once more with -fsanitize=address,undefined where that clang++ links
its sanitizer runtime).  It prints the layout of every kind of episode call over a grid of (K, B, N).

The totals below were computed once, by hand-written arithmetic, from the formulas each call carried in dw_api.hip before
they were folded into the one layout (the chains of `o_x = up(o_y + bytes)` of run_episode_impl, the wave path of
dw_run_episode_ensemble, the three launches-per-step loops and dw_run_episode_mlp), with sizeof(PhysF32) = sizeof(PhysF64)
= 128 and sizeof(StatsDev) = 24: buffer sizes are observable (allocation failures, the 64 MiB threshold of the page-locked
image), so they must not move.
"""
import json
import os
import subprocess

import pytest

from test_plan_cpu import CSRC, ROOT, _rocm_clang

GRID = [(1, 1, 0), (11, 3, 2), (64, 6, 2), (130, 5, 64), (4096, 3000, 8)]
FORMS = ("episode", "episode_trace", "ensemble_wave", "stepwise", "stepwise_trace", "stepwise_ensemble", "mlp")
TOTALS = {
    (1, 1, 0): {'episode': 1024, 'episode_trace': 1280, 'ensemble_wave': 1280, 'stepwise': 768, 'stepwise_trace': 768,
                'stepwise_ensemble': 512, 'mlp': 1024},
    (11, 3, 2): {'episode': 2816, 'episode_trace': 3840, 'ensemble_wave': 6400, 'stepwise': 1536, 'stepwise_trace': 2048,
                 'stepwise_ensemble': 1024, 'mlp': 3328},
    (64, 6, 2): {'episode': 11008, 'episode_trace': 20224, 'ensemble_wave': 55296, 'stepwise': 2816, 'stepwise_trace': 11520,
                 'stepwise_ensemble': 2304, 'mlp': 16128},
    (130, 5, 64): {'episode': 102400, 'episode_trace': 118016, 'ensemble_wave': 173824, 'stepwise': 85248,
                   'stepwise_trace': 100096, 'stepwise_ensemble': 84480, 'mlp': 392960},
    (4096, 3000, 8): {'episode': 209457152, 'episode_trace': 504369152, 'ensemble_wave': 235396096, 'stepwise': 208944384,
                      'stepwise_trace': 503808256, 'stepwise_ensemble': 208896256, 'mlp': 885317120},
}
ORDER = ["member_a", "member_b", "reward", "done", "p32", "ls", "p64", "use_table", "table", "world_alive", "agent_ok", "trace",
         "code", "pair_stats"]
F32, F64, STATS = 128, 128, 24


def _build(tmp, extra=()):
    exe = tmp / ("episode_staging_driver" + ("_san" if extra else ""))
    subprocess.check_call([_rocm_clang(), "-std=c++17", "-O2", "-Wall", "-Wextra", *extra, "-I", CSRC,
                           os.path.join(ROOT, "tests", "episode_staging_driver.cpp"), "-o", str(exe)])
    return exe


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    if _rocm_clang() is None:
        pytest.skip("the clang++ of ROCm is not installed")
    return tmp_path_factory.mktemp("episode_staging")


@pytest.fixture(scope="module")
def driver_output(build_dir):
    out = subprocess.run([str(_build(build_dir))], capture_output=True, text=True, check=True)
    return json.loads(out.stdout)


def _present(c):
    """The bytes of every region the form has, by the contract of each call (not by the header's code)."""
    K, B, N, rows, form = c["K"], c["B"], c["N"], c["rows"], c["form"]
    bn = B * N
    if form == "mlp":
        return {"member_a": 4 * B, "member_b": 4 * B, "reward": 8 * K * bn, "done": K * bn, "p32": F32 * K, "ls": 8 * K}
    want = {"table": K * bn, "world_alive": K * B, "agent_ok": K * bn}
    if form in ("episode", "episode_trace"):
        want.update(p32=F32 * K, ls=8 * K, use_table=K)
    if form == "ensemble_wave":
        want.update(p32=F32 * rows * B, ls=8 * rows * B, p64=F64 * B, use_table=K)
    if form in ("episode_trace", "stepwise_trace"):
        want.update(trace=STATS * K * B)
    if form == "stepwise":
        want.update(code=bn, pair_stats=8 * B)
    return want


def test_the_grid_is_the_one_asked_for(driver_output):
    assert driver_output["sizes"] == {"PhysF32": F32, "PhysF64": F64, "StatsDev": STATS}
    cases = driver_output["cases"]
    assert [(c["K"], c["B"], c["N"], c["form"]) for c in cases] == [(*g, f) for g in GRID for f in FORMS]
    assert any(not c["fits_image"] for c in cases) and any(c["fits_image"] for c in cases)
    # the wave path of the ensemble call: one launch where the rows fit, 64-step launches in the large case
    assert [c["rows"] for c in cases if c["form"] == "ensemble_wave"] == [1, 11, 64, 130, 64]


def test_regions_are_aligned_disjoint_and_in_order(driver_output):
    for c in driver_output["cases"]:
        names = [r[0] for r in c["regions"]]
        assert names == ORDER, c
        end = 0
        for name, off, size in c["regions"]:
            assert off % 256 == 0, (c["form"], name)
            assert off >= end, (c["form"], name)                 # behind everything before it: disjoint, in order
            assert off - end < 256, (c["form"], name)            # ... and no further than alignment asks
            end = off + size
        assert c["regions"][0][1] == 0
        slack = 256 if c["form"].startswith("stepwise") else 0
        assert c["total"] == (end + 255) // 256 * 256 + slack, c


def test_each_form_has_its_regions_and_no_others(driver_output):
    for c in driver_output["cases"]:
        want = _present(c)
        for name, _, size in c["regions"]:
            assert size == want.get(name, 0), (c["form"], c["K"], c["B"], c["N"], name)
        by = {r[0]: r for r in c["regions"]}
        # the one upload of a staged call ends behind the table, or behind use_table when the caller gave no table
        assert c["input_end_table"] == by["table"][1] + by["table"][2]
        assert c["input_end_no_table"] == by["use_table"][1] + by["use_table"][2]
        assert c["input_end_no_table"] <= by["table"][1] <= by["world_alive"][1]


def test_totals_equal_the_former_layouts(driver_output):
    for c in driver_output["cases"]:
        assert c["total"] == TOTALS[(c["K"], c["B"], c["N"])][c["form"]], (c["form"], c["K"], c["B"], c["N"])
        assert c["fits_image"] == (c["total"] <= 64 << 20)


def test_driver_is_clean_under_the_sanitizers(build_dir, driver_output):
    """The same stand-alone host program with -fsanitize=address,undefined: same answers, nothing reported."""
    probe = build_dir / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    can = subprocess.run([_rocm_clang(), "-fsanitize=address,undefined", str(probe), "-o", str(build_dir / "probe")],
                         capture_output=True).returncode == 0
    if not can:
        pytest.skip("this clang++ does not link its sanitizer runtime")
    exe = _build(build_dir, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    assert json.loads(out.stdout) == driver_output
