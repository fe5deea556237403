"""The staging layout of dw_run_episode_trace_temperature (csrc/dw_episode_staging.hpp, EpisodeRegions::temps), without a GPU.

tests/episode_temp_staging_driver.cpp includes only dw_episode_staging.hpp and is compiled here as plain C++17 by the clang++
that ships with ROCm (the recipe of test_episode_staging_cpu.py; once more with -fsanitize=address,undefined, run as the
stand-alone program it is).  For the (K, B, N) grid and the forms of tests/episode_staging_driver.cpp it prints every layout
without and with the temperature block:

  * without, every form has the offsets and totals it has always had (the totals of test_episode_staging_cpu.py, and the
    existing driver's own output region for region);
  * with, the forms that keep records ("episode_trace", "stepwise_trace") grow TRACE by exactly 32 K B: [K][B] StatsDev,
    then [K][B] temperature rows at off[TRACE] + sizeof(StatsDev) K B, 8-byte aligned; the regions behind stay 256-aligned;
    a form without records has no temperature block either.
"""
import json
import os
import subprocess

import pytest

from test_episode_staging_cpu import FORMS, GRID, ORDER, STATS, TOTALS
from test_plan_cpu import CSRC, ROOT, _rocm_clang

ROW = 32
RECORD_FORMS = ("episode_trace", "stepwise_trace")


def _build(tmp, source, extra=()):
    exe = tmp / (os.path.splitext(source)[0] + ("_san" if extra else ""))
    subprocess.check_call([_rocm_clang(), "-std=c++17", "-O2", "-Wall", "-Wextra", *extra, "-I", CSRC,
                           os.path.join(ROOT, "tests", source), "-o", str(exe)])
    return exe


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    if _rocm_clang() is None:
        pytest.skip("the clang++ of ROCm is not installed")
    return tmp_path_factory.mktemp("episode_temp_staging")


@pytest.fixture(scope="module")
def driver_output(build_dir):
    out = subprocess.run([str(_build(build_dir, "episode_temp_staging_driver.cpp"))], capture_output=True, text=True, check=True)
    return json.loads(out.stdout)


@pytest.fixture(scope="module")
def former_output(build_dir):
    """What the existing driver prints: the layouts of the calls without temperature records."""
    out = subprocess.run([str(_build(build_dir, "episode_staging_driver.cpp"))], capture_output=True, text=True, check=True)
    return json.loads(out.stdout)


def _cases(doc, temps):
    return [c for c in doc["cases"] if c["temps"] == temps]


def test_the_grid_is_the_existing_drivers(driver_output):
    assert driver_output["sizes"] == {"StatsDev": STATS, "temp_row": ROW}
    for temps in (0, 1):
        assert [(c["K"], c["B"], c["N"], c["form"]) for c in _cases(driver_output, temps)] == [(*g, f) for g in GRID for f in FORMS]


def test_without_temps_every_layout_is_todays(driver_output, former_output):
    for c, old in zip(_cases(driver_output, 0), former_output["cases"]):
        assert (c["form"], c["K"], c["B"], c["N"]) == (old["form"], old["K"], old["B"], old["N"])
        assert c["regions"] == old["regions"], (c["form"], c["K"], c["B"], c["N"])
        for name in ("total", "fits_image", "input_end_table", "input_end_no_table"):
            assert c[name] == old[name], (c["form"], name)
        assert c["total"] == TOTALS[(c["K"], c["B"], c["N"])][c["form"]]
        assert c["temps_bytes"] == 0
        assert c["stats_bytes"] == dict(map(lambda r: (r[0], r[2]), c["regions"]))["trace"]


def test_with_temps_the_record_forms_grow_trace_by_32_K_B(driver_output):
    for c, plain in zip(_cases(driver_output, 1), _cases(driver_output, 0)):
        K, B = c["K"], c["B"]
        what = (c["form"], K, B, c["N"])
        by, was = {r[0]: r for r in c["regions"]}, {r[0]: r for r in plain["regions"]}
        assert [r[0] for r in c["regions"]] == ORDER
        if c["form"] not in RECORD_FORMS:                        # no records: no temperature block, nothing moves
            assert c["regions"] == plain["regions"] and c["total"] == plain["total"] and c["temps_bytes"] == 0, what
            continue
        assert by["trace"][2] == was["trace"][2] + ROW * K * B == (STATS + ROW) * K * B, what
        assert c["stats_bytes"] == STATS * K * B and c["temps_bytes"] == ROW * K * B, what
        assert c["temps_off"] == by["trace"][1] + STATS * K * B, what
        assert c["temps_off"] % 8 == 0, what
        assert c["temps_off"] + c["temps_bytes"] == by["trace"][1] + by["trace"][2], what
        # everything up to TRACE is where it was; what follows is behind the block and 256-aligned, in order
        end = 0
        for name, off, size in c["regions"]:
            if ORDER.index(name) <= ORDER.index("trace"):
                assert off == was[name][1], (what, name)
            assert off % 256 == 0 and off >= end and off - end < 256, (what, name)
            end = off + size
        slack = 256 if c["form"].startswith("stepwise") else 0
        assert c["total"] == (end + 255) // 256 * 256 + slack, what
        assert c["fits_image"] == (c["total"] <= 64 << 20)
        assert c["input_end_table"] == plain["input_end_table"] and c["input_end_no_table"] == plain["input_end_no_table"]


def test_driver_is_clean_under_the_sanitizers(build_dir, driver_output):
    """The same stand-alone host program with -fsanitize=address,undefined: same answers, nothing reported."""
    probe = build_dir / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    can = subprocess.run([_rocm_clang(), "-fsanitize=address,undefined", str(probe), "-o", str(build_dir / "probe")],
                         capture_output=True).returncode == 0
    if not can:
        pytest.skip("this clang++ does not link its sanitizer runtime")
    exe = _build(build_dir, "episode_temp_staging_driver.cpp", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    assert json.loads(out.stdout) == driver_output
