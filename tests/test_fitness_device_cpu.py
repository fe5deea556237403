"""CPU-side tests (no GPU) of the fitness bookkeeping on the device (dw_fitness_begin / dw_fitness_account /
dw_run_episode_mlp_fitness / dw_fitness_download, csrc/dw_fitness.hpp):

  * the four symbols are declared in the header with the reference lines they restate, bound in `_ffi` and reachable from
    `Engine`; the harnesses take `bookkeeping=`; the ABI version is still 6;
  * the order of the kernel's sums (csrc/dw_fitness_order.hpp, a header without HIP): tests/fitness_order_driver.cpp does
    what a group of eight lanes does and must give `numpy.sum` / `.mean()` bit for bit - built with the clang++ of ROCm by
    the recipe of tests/test_plan_cpu.py, and once more with -fsanitize=address,undefined where that links;
  * the gfx950 code of the three kernels (one compilation of csrc/dw_api.hip with --save-temps, as the test_isa_* files):
    they exist, carry `_pw` in their names, use no scratch memory and make no calls.
"""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "therldaisyworld_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ("dw_fitness_begin", "dw_fitness_account", "dw_run_episode_mlp_fitness", "dw_fitness_download")
SIZES = (1, 3, 7, 8, 14, 64, 100, 128, 129, 130, 136, 300, 2000)


def test_symbols_are_declared_bound_and_reachable():
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi, harness
    header = open(os.path.join(ROOT, "include", "daisyworld_hip.h")).read()
    assert re.search(r"#define DW_ABI_VERSION 6\b", header) and _ffi.DW_ABI_VERSION == 6
    assert "sges.py:160-176" in header                       # the reference's bookkeeping statements
    assert re.search(r"\bint dw_fitness_begin\(dw_handle\* h, int32_t worlds_per_member, int32_t half\);", header)
    assert re.search(r"\bint dw_fitness_account\(dw_handle\* h, int32_t nsteps, const double\* reward[^;]*const uint8_t\* done"
                     r"[^;]*int32_t\* executed, int32_t\* finished\);", header)
    assert re.search(r"\bint dw_run_episode_mlp_fitness\(dw_handle\* h, int32_t nsteps, const double\* L_schedule, const double\* "
                     r"params[^;]*int32_t split, double L_init, int32_t\* executed, int32_t\* finished\);", header)
    assert re.search(r"\bint dw_fitness_download\(dw_handle\* h, double\* sum_reward[^;]*int32_t\* done_at[^;]*uint8_t\* running"
                     r"[^;]*\);", header)
    lib = _ffi.load()
    assert lib.dw_abi_version() == 6
    for name in SYMBOLS:
        assert name in _ffi.SIGNATURES, name
        assert getattr(lib, name).argtypes == _ffi.SIGNATURES[name][1]
    # a null handle is refused before anything else
    assert lib.dw_fitness_begin(None, 1, 1) == _ffi.DW_EINVAL and b"null" in lib.dw_last_error()
    assert lib.dw_fitness_download(None, None, None, None) == _ffi.DW_EINVAL
    e, f = C.c_int32(0), C.c_int32(0)
    assert lib.dw_fitness_account(None, 1, None, None, C.byref(e), C.byref(f)) == _ffi.DW_EINVAL
    assert lib.dw_run_episode_mlp_fitness(None, 1, None, None, 1, None, None, 0, 0.75, C.byref(e), C.byref(f)) == _ffi.DW_EINVAL
    for method in ("fitness_begin", "fitness_account", "run_episode_mlp_fitness", "fitness_download"):
        assert callable(getattr(amd.Engine, method)), method
    for fn in (harness.get_fitness, harness.get_fitness_population):
        assert inspect.signature(fn).parameters["bookkeeping"].default == "host"


def test_harness_refuses_unknown_and_empty_half_bookkeeping():
    from therldaisyworld_amd import harness
    with pytest.raises(ValueError, match="host"):
        harness._check_bookkeeping("device", 0)              # N = 1: the message names the host route
    with pytest.raises(ValueError, match="bookkeeping"):
        harness._check_bookkeeping("gpu", 2)
    assert harness._check_bookkeeping("device", 2) is True and harness._check_bookkeeping("host", 0) is False


# ---- the order of the sums ----------------------------------------------------------------------------------------------
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
def values(tmp_path_factory):
    """Random per-mille values (what rewards are: agent states rounded to three decimals), and the file the driver reads."""
    rng = np.random.RandomState(20261021)
    a = np.round(rng.rand(max(SIZES)), 3)
    path = tmp_path_factory.mktemp("fitness_order") / "values.f64"
    a.tofile(str(path))
    return a, str(path)


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def _check_driver(exe, values):
    a, path = values
    _assert_inputs_tell_the_orders_apart(a)
    out = subprocess.run([exe, path, *[str(n) for n in SIZES]], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rows = [ln.split() for ln in out.stdout.strip().split("\n")]
    assert [int(r[0]) for r in rows] == list(SIZES)
    wrong = [(n, r[1], f"{_bits(np.sum(a[:n])):016x}", r[2], f"{_bits(a[:n].mean()):016x}") for n, r in zip(SIZES, rows)
             if int(r[1], 16) != _bits(np.sum(a[:n])) or int(r[2], 16) != _bits(a[:n].mean())]
    assert not wrong, wrong


def _assert_inputs_tell_the_orders_apart(a):
    """Otherwise the comparison with the driver could not fail: for at least one n >= 16 the left-to-right sum of these
    values is not NumPy's."""
    def plain(n):
        s = 0.0
        for v in a[:n]:
            s += float(v)
        return s
    assert any(_bits(plain(n)) != _bits(np.sum(a[:n])) for n in SIZES if n >= 16)


def test_lane_emulation_equals_numpy_bit_for_bit(values, tmp_path):
    clang = _rocm_clang()
    if clang is None:
        pytest.skip("the clang++ of ROCm is not installed")
    exe = str(tmp_path / "fitness_order_driver")
    subprocess.check_call([clang, "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CSRC,
                           os.path.join(ROOT, "tests", "fitness_order_driver.cpp"), "-o", exe])
    _check_driver(exe, values)


def test_lane_emulation_under_address_and_undefined_behaviour_sanitizers(values, tmp_path):
    """The same program stand-alone with -fsanitize=address,undefined: the leaf walk reads no value outside [0, n) and the
    stack of waiting sums neither overflows nor underflows."""
    clang = _rocm_clang()
    if clang is None:
        pytest.skip("the clang++ of ROCm is not installed")
    exe = str(tmp_path / "fitness_order_driver_san")
    built = subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", CSRC, os.path.join(ROOT, "tests", "fitness_order_driver.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if built.returncode != 0:
        # only a missing sanitizer runtime excuses the build: anything else is an error in the driver or the header
        assert re.search(r"libclang_rt\.(asan|ubsan)|clang_rt\.(asan|ubsan)", built.stderr), built.stderr
        pytest.skip("the sanitizer runtimes of this clang++ do not link here: " + built.stderr.strip().split("\n")[-1])
    _check_driver(exe, values)


# ---- the gfx950 assembly -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    import isa_report
    isa_report.OUT = str(tmp_path_factory.mktemp("dw_isa_fitness"))   # a private build directory, not the tool's shared default
    text = open(isa_report.build([])).read()
    out = {}
    for name in re.findall(r"\.amdhsa_kernel (\S+)\n", text):
        if "fitness_" not in name:
            continue
        body = re.search(r"\n" + re.escape(name) + r":[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S)
        info = re.search(re.escape(name) + r":.*?; Kernel info:(.*?)(?=\n\t\.(?:text|section)|\Z)", text, re.S)
        assert body and info, name
        out[name] = ({k: int(v) for k, v in re.findall(r"; (\w+)\s*[:=] (\d+)", info.group(1))}, body.group(1))
    return out


def test_the_three_kernels_exist_with_pw_names(kernels):
    for stem in ("fitness_means_pw", "fitness_scan_pw", "fitness_counts_pw"):
        assert len([n for n in kernels if stem in n]) == 1, (stem, sorted(kernels))
    assert len(kernels) == 3 and all("_pw" in n for n in kernels), sorted(kernels)


def test_no_scratch_and_no_calls(kernels):
    for name, (info, body) in kernels.items():
        print(name, {k: info[k] for k in ("NumVgprs", "TotalNumSgprs", "Occupancy", "LDSByteSize") if k in info})
        assert info["ScratchSize"] == 0, (name, info)
        assert not re.search(r"\tscratch_", body), name
        assert not re.search(r"\ts_(swappc|call|setpc)", body), name
        assert info.get("NumAgprs", 0) == 0, (name, info)
    # the waiting sums of fitness_means_pw: 32 groups x kFitStackDepth doubles of static LDS, nothing in the other two
    src = open(os.path.join(CSRC, "dw_fitness_order.hpp")).read()
    depth = int(re.search(r"constexpr int kFitStackDepth = (\d+);", src).group(1))
    lds = {stem: info["LDSByteSize"] for stem in ("means", "scan", "counts") for n, (info, _) in kernels.items() if f"fitness_{stem}_pw" in n}
    assert lds == {"means": 32 * depth * 8, "scan": 0, "counts": 0}, lds
