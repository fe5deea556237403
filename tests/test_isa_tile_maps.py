"""Properties of the frame kernels (csrc/dw_tile_maps.hpp) on the gfx950 assembly hipcc emits (no GPU needed; one
compilation of csrc/dw_api.hip with --save-temps, as tests/test_isa_episode_temperature.py), read from the kernel-info
fields only:

  * the instantiations exist and carry `_pw` in their names (tests/test_per_world_cpu.py accepts added kernels only so):
    tile_cover_pw<8> and <1>, tile_temp_pw<InT, MAP> for the three plane formats x the three mappings, tile_temp_finish_pw;
  * no scratch and no accumulation registers: a thread's eight column sums and its 3x3 neighbourhoods stay in registers;
  * LDS: none, but the four doubles through which the waves of tile_temp_pw<., 2> combine;
  * waves per SIMD as DESIGN.md 3.2o states them: 8 for the cover kernels, for the finishing kernel and for the binary16
    temperature kernels (every frame step after the first), 7 / 8 / 8 from a float64 upload and 4 from a float32 one.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LDS_LIMIT = 64 * 1024
FORMATS = {"DF16_": "binary16", "f": "float32", "d": "float64"}     # the mangled element type of the planes
OCCUPANCY = {"binary16": (8, 8, 8), "float64": (7, 8, 8), "float32": (4, 4, 4)}     # per mapping 0, 1, 2


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    import isa_report
    isa_report.OUT = str(tmp_path_factory.mktemp("dw_isa_tiles"))   # a private build directory, not the tool's shared default
    text = open(isa_report.build([])).read()
    out = {}
    for name in re.findall(r"\.amdhsa_kernel (\S+)\n", text):
        if not re.search(r"tile_(cover|temp|temp_finish)_pw", name):
            continue
        info = re.search(re.escape(name) + r":.*?; Kernel info:(.*?)(?=\n\t\.(?:text|section)|\Z)", text, re.S)
        assert info, name
        out[name] = {k: int(v) for k, v in re.findall(r"; (\w+)\s*[:=] (\d+)", info.group(1))}
    return out


def _temp(kernels):
    """(format, mapping) -> name of tile_temp_pw<InT, MAP>"""
    out = {}
    for name in kernels:
        m = re.search(r"tile_temp_pwI(DF16_|f|d)Li([012])EE", name)
        if m:
            out[(FORMATS[m.group(1)], int(m.group(2)))] = name
    return out


def test_the_instantiations_exist_with_pw_names(kernels):
    assert all("_pw" in n for n in kernels)
    cover = sorted(n for n in kernels if "tile_cover_pw" in n)
    assert len(cover) == 2 and any("ILi8EE" in n for n in cover) and any("ILi1EE" in n for n in cover), cover
    assert len([n for n in kernels if "tile_temp_finish_pw" in n]) == 1
    assert set(_temp(kernels)) == {(f, m) for f in FORMATS.values() for m in range(3)}
    assert len(kernels) == 2 + 1 + 9, sorted(kernels)


def test_no_scratch(kernels):
    for name, info in kernels.items():
        assert info["ScratchSize"] == 0, (name, info)
        assert info.get("NumAgprs", 0) == 0, (name, info)


def test_lds(kernels):
    temp = _temp(kernels)
    for name, info in kernels.items():
        assert 0 <= info["LDSByteSize"] <= LDS_LIMIT, (name, info)
        large = name in {temp[(f, 2)] for f in FORMATS.values()}
        assert info["LDSByteSize"] == (32 if large else 0), (name, info)


def test_waves_per_simd_as_stated(kernels):
    for (fmt, mapping), name in _temp(kernels).items():
        assert kernels[name]["Occupancy"] == OCCUPANCY[fmt][mapping], (name, kernels[name])
    for name, info in kernels.items():
        if "tile_cover_pw" in name or "tile_temp_finish_pw" in name:
            assert info["Occupancy"] == 8, (name, info)
