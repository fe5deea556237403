"""Properties of episode_wave_ens_trace_pw (csrc/dw_episode_wave_ens_trace_pw.hpp) on the gfx950 assembly hipcc emits (no GPU
needed; one compilation of csrc/dw_api.hip with --save-temps, as tests/test_isa_properties.py):

  * the four instantiations <EXACT, TEMPS> exist and carry `_pw` in their names (tests/test_per_world_cpu.py accepts added
    kernels only so);
  * registers: each form keeps the waves per SIMD of the parent it takes its forward pass from - episode_wave_pw<EXACT>
    without TEMPS, episode_wave_temp_pw<EXACT> with - and the scratch bytes of that parent (the forms with TEMPS: none);
  * a call without temps pays for no float64 field: the form without TEMPS holds no more float64 instructions than
    episode_wave_pw (the agents' state and, exact, the cold near-tie repair), far fewer than the form with, and in the
    float32-only mode no float64 square root at all;
  * the static LDS is zero - the launch asks for its LDS dynamically, above the 64 KB default at the largest shape, and the
    header's static_assert holds that request to a CU's 160 KB; the formula is restated here.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FAMILIES = ("episode_wave_ens_trace_pw", "episode_wave_pw", "episode_wave_temp_pw")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    import isa_report
    isa_report.OUT = str(tmp_path_factory.mktemp("dw_isa_ens_trace"))   # a private build directory, not the tool's shared default
    text = open(isa_report.build([])).read()
    out = {}
    for name in re.findall(r"\.amdhsa_kernel (\S+)\n", text):
        if not any(f"{len(f)}{f}I" in name for f in FAMILIES):
            continue
        body = re.search(r"\n" + re.escape(name) + r":[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S)
        info = re.search(re.escape(name) + r":.*?; Kernel info:(.*?)(?=\n\t\.(?:text|section)|\Z)", text, re.S)
        assert body and info, name
        out[name] = ({k: int(v) for k, v in re.findall(r"; (\w+)\s*[:=] (\d+)", info.group(1))}, body.group(1))
    return out


def _one(kernels, family, args):
    """The instantiation of `family` whose bool template arguments are `args` (mangled Lb0 / Lb1)."""
    tag = f"{len(family)}{family}I" + "".join(f"Lb{int(a)}E" for a in args) + "E"
    hits = [n for n in kernels if tag in n]
    assert len(hits) == 1, (tag, sorted(kernels))
    return hits[0]


def _new(kernels, exact, temps):
    return _one(kernels, "episode_wave_ens_trace_pw", (exact, temps))


def test_four_instantiations_exist_with_pw_names(kernels):
    names = {_new(kernels, e, t) for e in (False, True) for t in (False, True)}
    assert len(names) == 4
    assert all("_pw" in n for n in names)
    assert len([n for n in kernels if "episode_wave_ens_trace_pw" in n]) == 4


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("temps", [False, True])
def test_registers_of_the_parent_kernel(kernels, exact, temps):
    name = _new(kernels, exact, temps)
    parent = _one(kernels, "episode_wave_temp_pw" if temps else "episode_wave_pw", (exact,))
    info, body = kernels[name]
    pinfo, _ = kernels[parent]
    print(f"{name}: {info['NumVgprs']} VGPRs, {info['ScratchSize']} B scratch, {info['Occupancy']} waves per SIMD "
          f"(parent {pinfo['NumVgprs']}, {pinfo['ScratchSize']}, {pinfo['Occupancy']})")
    assert info["Occupancy"] == pinfo["Occupancy"], (name, info, pinfo)
    assert info["ScratchSize"] == pinfo["ScratchSize"], (name, info, pinfo)
    assert info.get("NumAgprs", 0) == 0, (name, info)
    if temps:
        assert info["ScratchSize"] == 0 and not re.search(r"\tscratch_", body), name


@pytest.mark.parametrize("exact", [False, True])
def test_without_temps_no_float64_field_is_evaluated(kernels, exact):
    f64 = lambda body: len(re.findall(r"\tv_\w+_f64", body))
    plain, with_temps = kernels[_new(kernels, exact, False)][1], kernels[_new(kernels, exact, True)][1]
    parent = kernels[_one(kernels, "episode_wave_pw", (exact,))][1]
    print(f"exact={exact}: float64 VALU instructions {f64(plain)} without temps, {f64(with_temps)} with, "
          f"{f64(parent)} in episode_wave_pw")
    if not exact:                                               # (the exact mode's cold repair takes float64 roots of its own)
        assert not re.search(r"\tv_sqrt_f64|\tv_rsq_f64", plain)
    assert re.search(r"\tv_sqrt_f64|\tv_rsq_f64", with_temps)
    # what is left without temps is the agents' float64 state and (exact) the cold near-tie repair, as in episode_wave_pw
    assert f64(plain) <= f64(parent) + 8, (f64(plain), f64(parent))
    assert f64(with_temps) > f64(plain) + 100, (f64(with_temps), f64(plain))


def test_lds_is_dynamic_and_within_a_cu(kernels):
    for name, (info, _) in kernels.items():
        if "episode_wave_ens_trace_pw" in name:
            assert info["LDSByteSize"] == 0, (name, info)
    seg, C, N = 64, 256, 64
    shared = seg                                                             # use_table of a segment
    consts = seg * 128 + seg * 8                                             # a world's P32 | Ls rows
    world = 16 * C + (seg * N + 15) // 16 * 16 + (8 * N + 15) // 16 * 16 + seg * 12   # planes, table slice, ok masks, records
    lds = shared + 4 * (consts + world)
    assert 64 * 1024 < lds <= 160 * 1024 and lds // 1024 == 71, lds
    src = open(os.path.join(ROOT, "therldaisyworld_amd", "csrc", "dw_episode_wave_ens_trace_pw.hpp")).read()
    assert re.search(r"static_assert\(episode_wave_ens_trace_lds_bytes\(kEwMaxCells, 64\) <= 160 \* 1024", src)
    api = open(os.path.join(ROOT, "therldaisyworld_amd", "csrc", "dw_api.hip")).read()
    assert re.search(r"set_lds_limit\(h, rec_kern, lds\)", api)
