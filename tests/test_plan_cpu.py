"""Kernel selection, launch geometry and the per-step constants (csrc/dw_plan.hpp) held bit for bit, without a GPU.

tests/plan_driver.cpp includes only dw_plan.hpp and is compiled here as plain C++17 by the clang++ that ships with ROCm
(PhysF32 is built on clang's ext_vector_type; no ``-x hip``, no HIP header on the include path).  It prints every scalar
of StepPlan and of its four geometry structs for each shape, precision and switch setting, and the words of PhysF64,
PhysF32, FirstStepBound (from a float64 and from a float32 state) and derive_f32_pair for each parameter set; the output
must equal tests/golden/plan_constants.json.

How the fixture was recorded - once, from commit ec43b27a746b81b3f0b5adcf1e0411ab30185d49, the last one in which these
functions lived inside csrc/dw_api.hip, before any of them moved.  A scratch generator (not committed) of two lines,

    #include "<checkout of ec43b27>/therldaisyworld_amd/csrc/dw_api.hip"
    #include "<this tree>/tests/plan_driver.cpp"

was compiled with ``hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -I <dir holding an EMPTY dw_plan.hpp>
-I <checkout>/therldaisyworld_amd/csrc`` (the empty header stands in for the one that commit does not have; the driver's
calls then reach the functions of dw_api.hip itself) and run on a machine without a GPU - none of these functions makes
a HIP call.  Its standard output is the fixture.  (-O1 does not compile that file, --cuda-host-only does not link.)
"""
import json
import os
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "therldaisyworld_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_constants.json")


def _rocm_clang():
    roots = [os.environ.get("ROCM_PATH"), "/opt/rocm"]
    hipcc = shutil.which("hipcc")
    if hipcc:
        roots.append(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    for root in filter(None, roots):
        for sub in ("llvm/bin/clang++", "lib/llvm/bin/clang++"):
            path = os.path.join(root, sub)
            if os.path.exists(path):
                return path
    return None


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    clang = _rocm_clang()
    if clang is None:
        pytest.skip("the clang++ of ROCm is not installed")
    exe = tmp_path_factory.mktemp("plan") / "plan_driver"
    subprocess.check_call([clang, "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CSRC,
                           os.path.join(ROOT, "tests", "plan_driver.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True)
    return json.loads(out.stdout)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_plans_equal_the_recorded_ones(driver_output, recorded):
    fields = recorded["plan_fields"]
    assert driver_output["plan_fields"] == fields
    assert list(driver_output["plan"]) == list(recorded["plan"])
    wrong = {}
    for name, want in recorded["plan"].items():
        got = driver_output["plan"][name]
        diff = {f: (g, w) for f, g, w in zip(fields, got, want) if g != w}
        if diff or len(got) != len(want):
            wrong[name] = diff
    assert not wrong, f"{len(wrong)} plans differ (field: (now, recorded)), e.g. {dict(list(wrong.items())[:3])}"


def test_constants_equal_the_recorded_ones_bit_for_bit(driver_output, recorded):
    assert list(driver_output["constants"]) == list(recorded["constants"])
    wrong = {}
    for name, want in recorded["constants"].items():
        got = driver_output["constants"][name]
        assert list(got) == list(want)
        for key in want:
            g, w = got[key].split(), want[key].split()
            words = [i for i in range(max(len(g), len(w))) if g[i:i + 1] != w[i:i + 1]]
            if words:
                wrong[f"{name}: {key}"] = words
    assert not wrong, f"words that differ: {wrong}"


def _f32(word):
    return struct.unpack("<f", struct.pack("<I", int(word, 16)))[0]


def test_the_recorded_cases_reach_every_branch(recorded):
    """The fixture is only worth something if its cases take every path of plan_steps and both admissibility branches
    of the two bounds: checked on the recorded values themselves."""
    fields = recorded["plan_fields"]
    plans = {name: dict(zip(fields, row)) for name, row in recorded["plan"].items()}

    def seen(field):
        return {p[field] for p in plans.values()}

    assert seen("kind") == {0, 1, 2}                                    # generic, tiled, wave-strip
    assert seen("halo") == {0, 1, 2, 3}
    assert {(p["tcq"], p["rpt"]) for p in plans.values() if p["kind"] == 1} == {(16, 2), (32, 4), (64, 4), (64, 8)}
    assert seen("fused_mode") == {0, 1, 2} and seen("fgeom.cols_per_strip") == {0, 248, 256, 1024}
    for field in ("packed", "allow_fuse", "fmt_planes", "trace_pairs", "sym_albedo", "first_stream", "need_fixq",
                  "pw_stream", "sgeom.force_rescan"):
        assert seen(field) == {0, 1}, field
    assert seen("first_prec") == {1, 2, 3}
    assert plans["2x96x1280 fast default"]["fmt_planes"] == 1
    assert plans["2x96x1280 fast no_fmt_planes"]["fmt_planes"] == 0
    assert plans["1x40000x32768 fast default"]["fmt_planes"] == 0      # a world's plane of 2^31 bytes or more
    assert plans["4096x16x64 exact default"]["packed"] == 1 and plans["8x16x64 exact default"]["kind"] == 1
    assert plans["4096x16x96 exact default"]["sgeom.wpr"] == 2
    # DW_STRIP_ROWS: the grid's height caps both, 64 rows the first step's
    assert plans["2x96x512 exact strip_rows=128"]["sgeom.SR"] == 96
    assert plans["2x96x512 exact strip_rows=128"]["first_geom.SR"] == 64
    assert plans["1x40000x32768 exact strip_rows=128"]["sgeom.SR"] == 128
    assert plans["2x96x512 exact strip_rows=8"]["first_geom.SR"] == 8
    assert {plans["2x96x512 exact queue_cap=4"]["sgeom.qcap"], plans["2x40x64 exact queue_cap=4"]["geom.qcap"]} == {4}
    # constants: PhysF32 word 27 is tie_lo, word 31 hi_bits; FirstStepBound word 11 is slack
    consts = recorded["constants"]
    tie_lo = {name: _f32(c["f32"].split()[27]) for name, c in consts.items()}
    slack = {name: _f32(c["first_from_f64"].split()[11]) for name, c in consts.items()}
    assert tie_lo["default L=0.1"] == -0.5 and slack["default L=0.1"] == 1.0          # inadmissible: A0 = 1, slack = 1
    four_millionths = struct.unpack("<f", struct.pack("<f", 4e-6))[0]
    assert all(0.49 < t < 0.5 and slack[name] == four_millionths for name, t in tie_lo.items() if name != "default L=0.1")
    assert _f32(consts["g=0 L=1"]["f32"].split()[21]) == 2.0 ** 60                      # kbeta
    a, b = consts["albedo=0.45/0.8/0.2 L=0.9"]["f32"].split(), consts["albedo=0.45/0.8/0.2 L=0.9"]["pair"].split()
    assert int(a[31], 16) == 22 and int(b[31], 16) == int(b[63], 16) == 21              # the pair: the coarser split
    assert consts["p=0.7 L=1"]["f32"] != consts["default L=1"]["f32"]
