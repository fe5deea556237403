"""Properties of episode_wave_frames_pw (csrc/dw_episode_wave_frames_pw.hpp) on the gfx950 assembly hipcc emits (no GPU needed;
one compilation of csrc/dw_api.hip with --save-temps, as tests/test_isa_episode_temperature.py):

  * the six instantiations (float32-only / exact x FIELD 0 / 1 / 2) and frame_agents_pw exist and carry `_pw` in their names
    (tests/test_per_world_cpu.py accepts added kernels only so);
  * no scratch and no AGPRs: the float64 temperatures of up to four cells per lane, the butterflies and the tile loops stay
    in registers;
  * the static LDS is zero - the launch asks for its LDS dynamically, and the header's static_assert holds that request
    (256 cells, 64 agents) to the 64 KB a launch may ask for without a function attribute;
  * waves per SIMD as DESIGN.md 3.2p states them.  A workgroup is four waves, one per SIMD, so any of them leaves room for
    the workgroups of more worlds.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LDS_LIMIT = 64 * 1024
# (exact, FIELD) -> waves per SIMD, as DESIGN.md 3.2p quotes them from this compiler's output
OCCUPANCY = {(False, 0): 4, (False, 1): 2, (False, 2): 2, (True, 0): 3, (True, 1): 2, (True, 2): 2}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    import isa_report
    isa_report.OUT = str(tmp_path_factory.mktemp("dw_isa_frames"))   # a private build directory, not the tool's shared default
    text = open(isa_report.build([])).read()
    out = {}
    for name in re.findall(r"\.amdhsa_kernel (\S+)\n", text):
        if "episode_wave_frames" not in name and "frame_agents" not in name:
            continue
        body = re.search(r"\n" + re.escape(name) + r":[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S)
        info = re.search(re.escape(name) + r":.*?; Kernel info:(.*?)(?=\n\t\.(?:text|section)|\Z)", text, re.S)
        assert body and info, name
        out[name] = ({k: int(v) for k, v in re.findall(r"; (\w+)\s*[:=] (\d+)", info.group(1))}, body.group(1))
    return out


def _wave_kernels(kernels):
    """(exact, FIELD) -> name: the template arguments are mangled as Lb0 / Lb1 and Li0 / Li1 / Li2"""
    by = {}
    for name in kernels:
        m = re.search(r"episode_wave_frames_pwILb([01])ELi([012])E", name)
        if m:
            by[(m.group(1) == "1", int(m.group(2)))] = name
    return by


def test_the_instantiations_exist_with_pw_names(kernels):
    by = _wave_kernels(kernels)
    assert sorted(by) == sorted(OCCUPANCY), sorted(kernels)
    others = [n for n in kernels if n not in by.values()]
    assert len(others) == 1 and "frame_agents_pw" in others[0], others
    for name in kernels:
        assert "_pw" in name, name


def test_no_scratch(kernels):
    for name, (info, body) in kernels.items():
        assert info["ScratchSize"] == 0, (name, info)
        assert not re.search(r"\tscratch_", body), name
        assert info.get("NumAgprs", 0) == 0, (name, info)          # nothing parked in accumulation registers either


def test_lds_within_the_asserted_limit(kernels):
    """Static LDS is zero (the launch's request is dynamic); the request's bound is the header's static_assert, restated
    here from its formula: shared P32 | Ls | use_table of a segment + 4 x (planes, table slice, ok masks, records, the
    temperature of every cell)."""
    for name, (info, _) in kernels.items():
        assert info["LDSByteSize"] == 0, (name, info)
    seg, C, N = 64, 256, 64
    shared = seg * 128 + seg * 8 + seg
    world = 16 * C + (seg * N + 15) // 16 * 16 + (8 * N + 15) // 16 * 16 + seg * 12 + (8 * C + 15) // 16 * 16
    assert shared + 4 * (world - 8 * C) == 46656                # episode_wave_temp_pw's launch, plus 4 x 2048 B of staging
    assert shared + 4 * world == 54848 <= LDS_LIMIT
    src = open(os.path.join(ROOT, "therldaisyworld_amd", "csrc", "dw_episode_wave_frames_pw.hpp")).read()
    assert re.search(r"static_assert\(episode_wave_frames_lds_bytes\(kEwMaxCells, 64\) <= 64 \* 1024", src)


def test_waves_per_simd_as_stated(kernels):
    by = _wave_kernels(kernels)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 3.2p"):]
    for key, name in by.items():
        assert kernels[name][0]["Occupancy"] == OCCUPANCY[key], (key, kernels[name][0])
        prec = "exact" if key[0] else "float32-only"
        assert re.search(rf"\| {prec} \| {key[1]} \|[^\n]*\| {OCCUPANCY[key]} \|", section), (key, "DESIGN.md 3.2p")
