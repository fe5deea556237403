"""Properties of episode_wave_temp_pw (csrc/dw_episode_wave_temp_pw.hpp) on the gfx950 assembly hipcc emits (no GPU needed;
one compilation of csrc/dw_api.hip with --save-temps, as tests/test_isa_properties.py):

  * both instantiations exist and carry `_pw` in their names (tests/test_per_world_cpu.py accepts added kernels only so);
  * no scratch: the float64 temperature of up to four cells per lane and the 64-bit butterflies stay in registers;
  * the static LDS is zero - the launch asks for its LDS dynamically, and the header's static_assert holds that request
    (256 cells, 64 agents) to the 64 KB a launch may ask for without a function attribute;
  * waves per SIMD as DESIGN.md 3.2l states them: 3 (float32-only) and 2 (exact) - a workgroup is four waves, one per
    SIMD, so either leaves room for the workgroups of more worlds.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LDS_LIMIT = 64 * 1024


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    import isa_report
    isa_report.OUT = str(tmp_path_factory.mktemp("dw_isa_temp"))   # a private build directory, not the tool's shared default
    text = open(isa_report.build([])).read()
    out = {}
    for name in re.findall(r"\.amdhsa_kernel (\S+)\n", text):
        if "episode_wave_temp" not in name:
            continue
        body = re.search(r"\n" + re.escape(name) + r":[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S)
        info = re.search(re.escape(name) + r":.*?; Kernel info:(.*?)(?=\n\t\.(?:text|section)|\Z)", text, re.S)
        assert body and info, name
        out[name] = ({k: int(v) for k, v in re.findall(r"; (\w+)\s*[:=] (\d+)", info.group(1))}, body.group(1))
    return out


def _by_mode(kernels):
    """(float32-only, exact): the template argument is mangled as Lb0 / Lb1"""
    fast = [n for n in kernels if "Lb0" in n]
    exact = [n for n in kernels if "Lb1" in n]
    assert len(fast) == 1 and len(exact) == 1 and len(kernels) == 2, sorted(kernels)
    return fast[0], exact[0]


def test_both_instantiations_exist_with_pw_names(kernels):
    for name in _by_mode(kernels):
        assert "episode_wave_temp_pw" in name and "_pw" in name, name


def test_no_scratch(kernels):
    for name, (info, body) in kernels.items():
        assert info["ScratchSize"] == 0, (name, info)
        assert not re.search(r"\tscratch_", body), name
        assert info.get("NumAgprs", 0) == 0, (name, info)          # nothing parked in accumulation registers either


def test_lds_within_the_asserted_limit(kernels):
    """Static LDS is zero (the launch's request is dynamic); the request's bound is the header's static_assert, restated
    here from its formula: shared P32 | Ls | use_table of a segment + 4 x (planes, table slice, ok masks, records)."""
    for name, (info, _) in kernels.items():
        assert 0 <= info["LDSByteSize"] <= LDS_LIMIT, (name, info)
        assert info["LDSByteSize"] == 0, (name, info)
    seg, C, N = 64, 256, 64
    shared = seg * 128 + seg * 8 + seg
    world = 16 * C + (seg * N + 15) // 16 * 16 + (8 * N + 15) // 16 * 16 + seg * 12
    assert shared + 4 * world <= LDS_LIMIT
    src = open(os.path.join(ROOT, "therldaisyworld_amd", "csrc", "dw_episode_wave_temp_pw.hpp")).read()
    assert re.search(r"static_assert\(episode_wave_temp_lds_bytes\(kEwMaxCells, 64\) <= 64 \* 1024", src)


def test_waves_per_simd_as_stated(kernels):
    fast, exact = _by_mode(kernels)
    assert kernels[fast][0]["Occupancy"] == 3, kernels[fast][0]
    assert kernels[exact][0]["Occupancy"] == 2, kernels[exact][0]
