"""Properties of episode_mlp_wave_trace_pw (csrc/dw_episode_mlp_wave_trace_pw.hpp) on the gfx950 assembly hipcc emits (no GPU
needed; one compilation of csrc/dw_api.hip with --save-temps, as tests/test_isa_episode_temperature.py):

  * the four instantiations <EXACT, TEMPS> exist and carry `_pw` in their names (tests/test_per_world_cpu.py accepts added
    kernels only so);
  * no scratch and no accumulation registers: the float64 observation, the temperatures of up to four cells per lane and the
    64-bit butterflies stay in vector registers;
  * the static LDS is zero - the launch asks for its LDS dynamically, and the header's static_assert holds that request
    (256 cells, 4 agents: 44 864 bytes) to the 64 KB a launch may ask for without a function attribute;
  * at least one wave per SIMD (a workgroup is four waves, one per SIMD); the measured values are recorded in DESIGN.md
    3.2n, not asserted.
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
    isa_report.OUT = str(tmp_path_factory.mktemp("dw_isa_mlp_trace"))   # a private build directory, not the tool's shared default
    text = open(isa_report.build([])).read()
    out = {}
    for name in re.findall(r"\.amdhsa_kernel (\S+)\n", text):
        if "episode_mlp_wave_trace" not in name:
            continue
        body = re.search(r"\n" + re.escape(name) + r":[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S)
        info = re.search(re.escape(name) + r":.*?; Kernel info:(.*?)(?=\n\t\.(?:text|section)|\Z)", text, re.S)
        assert body and info, name
        out[name] = ({k: int(v) for k, v in re.findall(r"; (\w+)\s*[:=] (\d+)", info.group(1))}, body.group(1))
    return out


def test_four_instantiations_exist_with_pw_names(kernels):
    assert len(kernels) == 4, sorted(kernels)
    for exact in (0, 1):
        for temps in (0, 1):                                    # the template arguments are mangled as Lb0 / Lb1
            hit = [n for n in kernels if f"episode_mlp_wave_trace_pwILb{exact}ELb{temps}EE" in n]
            assert len(hit) == 1, (exact, temps, sorted(kernels))
    assert all("_pw" in n for n in kernels)


def test_no_scratch(kernels):
    for name, (info, body) in kernels.items():
        assert info["ScratchSize"] == 0, (name, info)
        assert not re.search(r"\tscratch_", body), name
        assert info.get("NumAgprs", 0) == 0, (name, info)


def test_lds_within_the_asserted_limit(kernels):
    """Static LDS is zero (the launch's request is dynamic); the request's bound is the header's static_assert, restated
    here from its formula: shared P32 | Ls | use_table of a segment + 4 x (planes, 128 doubles per agent, agent states,
    positions, records)."""
    for name, (info, _) in kernels.items():
        assert info["LDSByteSize"] == 0, (name, info)
    seg, C, N = 64, 256, 4
    shared = seg * 128 + seg * 8 + seg
    world = 16 * C + N * 128 * 8 + 2 * ((8 * N + 15) // 16 * 16) + seg * 12
    assert shared + 4 * world == 44864 <= LDS_LIMIT
    src = open(os.path.join(ROOT, "therldaisyworld_amd", "csrc", "dw_episode_mlp_wave_trace_pw.hpp")).read()
    assert re.search(r"static_assert\(episode_mlp_wave_trace_lds_bytes\(kEwMaxCells, 4\) <= 64 \* 1024", src)
    assert "return episode_wave_shared_bytes() + 4 * episode_mlp_wave_trace_world_bytes(C, N);" in src
    assert "return episode_mlp_wave_world_bytes(C, N) + kEwRecBytes;" in src


def test_at_least_one_wave_per_simd(kernels):
    for name, (info, _) in kernels.items():
        print(name, {k: info[k] for k in ("NumVgprs", "TotalNumSgprs", "Occupancy") if k in info})
        assert info["Occupancy"] >= 1, (name, info)
