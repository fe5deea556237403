"""CPU-side tests (no GPU) of the per-world physics constants (dw_step_n_trace_ensemble, dw_world_params_of):

  * the struct and both functions are declared, exported and bound; sizeof(dw_world_params) == 96; null arguments are
    refused; the ABI version is still 6;
  * the Python surface exists and refuses wrong shapes and names before any device call;
  * csrc/dw_plan.hpp alone (tests/ensemble_driver.cpp, the host clang++ of ROCm): a world's constants are those of a
    dw_params that carries its twelve members - one derivation - and the call-wide SYM decision falls with the first
    asymmetric world;
  * the gfx950 code of the per-world step pairs (one compilation of csrc/dw_api.hip with --save-temps, the recipe of
    test_isa_properties.py): registers, occupancy, scratch and LDS of the shared-L trace_pair_* kernel of the same
    MODE / SYM, a row loop whose main path has no scratch traffic and no scalar load, and no more VALU instructions in it
    than the shared-L kernel's.
"""
import ctypes as C
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "therldaisyworld_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

MEMBERS = ("p", "g", "S", "sigma", "gamma", "q", "q2", "dt", "albedo_bare", "albedo_light", "albedo_dark", "temp_optimal")


def test_struct_and_symbols_are_declared_exported_and_bound():
    from therldaisyworld_amd import _ffi
    header = open(os.path.join(ROOT, "include", "daisyworld_hip.h")).read()
    m = re.search(r"typedef struct dw_world_params \{\s*double ([^;]*);\s*\} dw_world_params;", header)
    assert m and tuple(x.strip() for x in m.group(1).split(",")) == MEMBERS
    assert re.search(r"\bint dw_world_params_of\(const dw_handle\* h, dw_world_params\* out\);", header)
    assert re.search(r"\bint dw_step_n_trace_ensemble\(dw_handle\* h, int32_t nsteps,\s*const dw_world_params\* worlds[^;]*"
                     r"const double\* L_schedule[^;]*dw_world_stats\* trace[^;]*dw_temp_stats\* temps[^;]*\);", header)
    assert re.search(r"#define DW_ABI_VERSION 6\b", header)
    assert _ffi.DW_ABI_VERSION == 6
    assert C.sizeof(_ffi.DwWorldParams) == 96 and _ffi.WORLD_PARAMS_DTYPE.itemsize == 96
    assert tuple(n for n, _ in _ffi.DwWorldParams._fields_) == MEMBERS == _ffi.WORLD_PARAM_NAMES == _ffi.WORLD_PARAMS_DTYPE.names
    # the twelve members are a run of dw_params in the same order
    names = [n for n, _ in _ffi.DwParams._fields_]
    assert tuple(names[names.index("p"):names.index("p") + 12]) == MEMBERS
    lib = _ffi.load()
    assert lib.dw_abi_version() == 6
    assert lib.dw_world_params_of.argtypes == [C.c_void_p, C.POINTER(_ffi.DwWorldParams)]
    assert lib.dw_step_n_trace_ensemble.argtypes == [C.c_void_p, C.c_int32, C.POINTER(_ffi.DwWorldParams), C.POINTER(C.c_double),
                                                     C.POINTER(_ffi.DwWorldStats), C.POINTER(_ffi.DwTempStats)]
    w = _ffi.DwWorldParams()
    assert lib.dw_world_params_of(None, C.byref(w)) == _ffi.DW_EINVAL and b"null" in lib.dw_last_error()
    Ls = np.ones((4, 1))
    assert lib.dw_step_n_trace_ensemble(None, 4, C.byref(w), _ffi.ptr_d(Ls), None, None) == _ffi.DW_EINVAL
    assert b"null" in lib.dw_last_error()


def test_python_surface_and_shape_checks_without_a_device():
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi, harness
    assert callable(amd.Engine.step_n_trace_ensemble) and callable(amd.Engine.world_params)
    assert amd.simulate_parameter_sweep is harness.simulate_parameter_sweep
    assert "simulate_parameter_sweep" in amd.__all__

    class _NoDevice:                                           # any touch of the library is an AttributeError
        B = 3
        _world_table = amd.Engine._world_table
    good = np.zeros(3, dtype=_ffi.WORLD_PARAMS_DTYPE)
    for bad in (np.zeros((3, 11)), np.zeros((2, 12)), np.zeros(12), np.zeros(2, dtype=_ffi.WORLD_PARAMS_DTYPE),
                np.zeros(3, dtype=[("p", "<f8"), ("g", "<f8")])):
        with pytest.raises(ValueError, match="per-world constants"):
            amd.Engine.step_n_trace_ensemble(_NoDevice(), bad, np.ones((4, 3)))
    for bad_L in (np.ones((4, 2)), np.ones(3)):
        with pytest.raises(ValueError, match="shape"):
            amd.Engine.step_n_trace_ensemble(_NoDevice(), good, bad_L)
    # a (B, 12) float64 array is read in the struct's order
    tab = amd.Engine._world_table(_NoDevice(), np.arange(36, dtype=np.float64).reshape(3, 12))
    assert tab.dtype == _ffi.WORLD_PARAMS_DTYPE and tab["p"].tolist() == [0, 12, 24] and tab["temp_optimal"].tolist() == [11, 23, 35]

    env = types.SimpleNamespace(n_agents=0, batch_size=3, dim=8, **{n: 1.0 for n in MEMBERS})
    with pytest.raises(ValueError, match="not a per-world constant"):
        harness.simulate_parameter_sweep(env, {"agent_gamma": 0.1}, 5, obs=True)
    with pytest.raises(ValueError, match="scalar or shape"):
        harness.simulate_parameter_sweep(env, {"q2": np.ones(4)}, 5, obs=True)
    with pytest.raises(ValueError, match="shape"):
        harness.simulate_parameter_sweep(env, {"q2": np.ones(3)}, 5, L_values=np.ones(4), obs=True)
    with pytest.raises(ValueError, match="agent-free"):
        harness.simulate_parameter_sweep(types.SimpleNamespace(n_agents=2, batch_size=3, dim=8), {}, 5, obs=True)


# ---- csrc/dw_plan.hpp alone ---------------------------------------------------------------------------------------------
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
    exe = tmp_path_factory.mktemp("ensemble") / "ensemble_driver"
    subprocess.check_call([clang, "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CSRC,
                           os.path.join(ROOT, "tests", "ensemble_driver.cpp"), "-o", str(exe)])
    return json.loads(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout)


def test_a_worlds_constants_are_those_of_params_that_carry_its_members(driver_output):
    cases = driver_output["cases"]
    assert len(cases) == 6
    for i, c in enumerate(cases):
        assert c["via_world"] == c["direct"], i
        assert c["round_trip"]["in"] == c["round_trip"]["out"], i
        assert c["shape_kept"] == 1, i
    # the cases are different worlds: every set of derived words occurs once
    assert len({json.dumps(c["direct"], sort_keys=True) for c in cases}) == len(cases)
    # ... and there is one derivation in the sources: each function is defined once, and the ensemble call goes through
    # the handle's params with the world's members replaced
    sources = "".join(open(f).read() for f in sorted(glob.glob(os.path.join(CSRC, "*.h*"))))
    for fn in ("PhysF32 derive_f32(", "void derive_f32_pair(", "PhysF64 make_f64(", "FirstStepBound derive_first_bound("):
        assert sources.count("inline " + fn) == 1, fn
    api = open(os.path.join(CSRC, "dw_api.hip")).read()
    assert "with_world_params(p, worlds[b])" in sources and "worlds_symmetric(worlds, B)" in api


def test_the_sym_decision_is_call_wide(driver_output):
    sym = driver_output["sym"]
    assert sym == {"all_symmetric": 1, "last_asymmetric": 0, "first_asymmetric": 0, "single_asymmetric": 0, "plan_own": 1}


# ---- the gfx950 assembly ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def asm_path(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    import isa_report
    isa_report.OUT = str(tmp_path_factory.mktemp("dw_isa_ensemble"))
    return isa_report.build([])


def _kernels(text):
    out = {}
    for name in re.findall(r"\.amdhsa_kernel (\S+)\n", text):
        m = re.search(r"\n" + re.escape(name) + r":[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S)
        info = re.search(re.escape(name) + r":.*?; Kernel info:(.*?)(?=\n\t\.(?:text|section)|\Z)", text, re.S)
        if not (m and info):
            continue
        vals = {k: int(v) for k, v in re.findall(r"; (\w+)\s*[:=] (\d+)", info.group(1))}
        out[name] = (vals, m.group(1))
    return out


def _hot_loop_span(body):
    lines = body.split("\n")
    labels = {m.group(1): i for i, ln in enumerate(lines) for m in [re.match(r"(\.LBB\S+):", ln)] if m}
    best, best_pk = None, -1
    for i, ln in enumerate(lines):
        m = re.match(r"\ts_c?branch\S* (\.LBB\S+)", ln)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            npk = sum(1 for x in lines[labels[m.group(1)]:i + 1] if x.startswith("\tv_pk_"))
            if npk > best_pk:
                best, best_pk = (labels[m.group(1)], i), npk
    return lines, best


def _main_path(loop):
    """The loop without its queue-push segments (they hold v_mbcnt / ds_write_b128 and run for well under 1 % of the rows)."""
    segs, cur = [], []
    for ln in loop:
        if re.match(r"(\.LBB\S+):", ln):
            segs.append(cur)
            cur = []
        cur.append(ln)
        if re.match(r"\ts_c?branch", ln):
            segs.append(cur)
            cur = []
    segs.append(cur)
    return [ln for sg in segs if not any("v_mbcnt" in x or "ds_write_b128" in x for x in sg) for ln in sg]


# (per-world kernel, its shared-L twin) by the substrings of their mangled names: MODE 0 overlapped, 1 rotating.  There is
# no exact form: it did not keep the shared-L kernel's row loop (csrc/dw_step_fused_pw.hpp) and was left out.
TWINS = [(f"trace_pair_fast_pwILi{m}EE", f"trace_pair_fastILi{m}EE") for m in (0, 1)]


@pytest.mark.parametrize("pw,shared", TWINS)
def test_per_world_step_pairs_cost_what_the_shared_ones_cost(asm_path, pw, shared):
    ks = _kernels(open(asm_path).read())
    a = next((n for n in ks if pw in n), None)
    b = next((n for n in ks if shared in n), None)
    assert a and b, (pw, shared)
    (ia, ba), (ib, bb) = ks[a], ks[b]
    for key in ("NumVgprs", "NumAgprs", "Occupancy", "ScratchSize", "LDSByteSize"):
        assert ia[key] == ib[key], (a, key, ia[key], ib[key])
    (la, sa), (lb, sb) = _hot_loop_span(ba), _hot_loop_span(bb)
    assert sa and sb, a
    loop_a, loop_b = la[sa[0]:sa[1] + 1], lb[sb[0]:sb[1] + 1]
    main_a = _main_path(loop_a)
    assert not any(ln.startswith("\tscratch_") for ln in main_a), f"{a}: scratch traffic on the row loop's main path"
    # the constants are loaded once, in front of the row loop: by scalar loads, more of them than the shared kernel has
    assert not any(re.match(r"\ts_(buffer_)?load", ln) for ln in main_a), f"{a}: a scalar load on the row loop's main path"
    sload = lambda lines, end: sum(1 for ln in lines[:end] if re.match(r"\ts_load_dword", ln))
    assert sload(la, sa[0]) > sload(lb, sb[0]), (a, sload(la, sa[0]), sload(lb, sb[0]))
    vload = lambda loop: sum(1 for ln in loop if re.match(r"\t(global|flat|buffer)_load", ln))
    assert vload(_main_path(loop_a)) == vload(_main_path(loop_b)), (a, vload(main_a), vload(_main_path(loop_b)))
    valu = lambda lines: sum(1 for ln in lines if ln.startswith("\tv_"))
    print(f"{a}: row loop {valu(loop_a)} VALU (shared-L: {valu(loop_b)}), {ia['NumVgprs']} VGPRs, {ia['TotalNumSgprs']} SGPRs "
          f"(shared-L: {ib['TotalNumSgprs']})")
    assert valu(loop_a) <= valu(loop_b), (a, valu(loop_a), valu(loop_b))
