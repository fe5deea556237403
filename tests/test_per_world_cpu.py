"""CPU-side tests (no GPU) of the per-world luminosity schedules (dw_step_n_trace_per_world):

  * the symbol is declared, exported and bound; a null handle is refused; the ABI version is still 6;
  * the Python surface exists and refuses a wrong shape before any device call;
  * the gfx950 code of the per-world wave-strip kernels (one extra compilation of csrc/dw_api.hip with --save-temps, the
    recipe of test_isa_properties.py): registers and occupancy of the shared-L kernel of the same mode, a row loop
    without scratch traffic, without a load of the table, and with no more VALU instructions than the shared-L kernel's;
  * no kernel that existed before this feature changed: its instructions and descriptor hash to what
    tests/golden/kernel_fingerprint.json holds.
"""
import ctypes as C
import json
import os
import re
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_symbol_is_declared_exported_and_bound():
    from therldaisyworld_amd import _ffi
    header = open(os.path.join(ROOT, "include", "daisyworld_hip.h")).read()
    assert re.search(r"\bint dw_step_n_trace_per_world\(dw_handle\* h, int32_t nsteps,\s*const double\* L_schedule", header)
    assert "daisy_world_rl.py:405,408" in header             # where L enters the reference's map
    assert re.search(r"#define DW_ABI_VERSION 6\b", header)
    assert _ffi.DW_ABI_VERSION == 6
    assert "dw_step_n_trace_per_world" in _ffi.SIGNATURES
    lib = _ffi.load()
    assert lib.dw_abi_version() == 6
    assert lib.dw_step_n_trace_per_world.argtypes == [C.c_void_p, C.c_int32, C.POINTER(C.c_double),
                                                      C.POINTER(_ffi.DwWorldStats)]
    Ls = np.ones((4, 1))
    out = np.zeros((4, 1), dtype=_ffi.STATS_DTYPE)
    rc = lib.dw_step_n_trace_per_world(None, 4, _ffi.ptr_d(Ls), out.ctypes.data_as(C.POINTER(_ffi.DwWorldStats)))
    assert rc == _ffi.DW_EINVAL and b"null" in lib.dw_last_error()


def test_python_surface_and_shape_checks_without_a_device():
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import harness
    assert callable(amd.Engine.step_n_trace_per_world)
    assert amd.simulate_luminosity_sweep is harness.simulate_luminosity_sweep
    assert "simulate_luminosity_sweep" in amd.__all__

    class _NoDevice:                                           # any touch of the library is an AttributeError
        B = 3
    for bad in (np.ones((4, 2)), np.ones(3), np.ones((4, 3, 1))):
        with pytest.raises(ValueError, match="shape"):
            amd.Engine.step_n_trace_per_world(_NoDevice(), bad)
    env = types.SimpleNamespace(n_agents=0, batch_size=3, dim=8)
    with pytest.raises(ValueError, match="shape"):
        harness.simulate_luminosity_sweep(env, np.ones(4), 5, obs=True)
    with pytest.raises(ValueError, match="shape"):
        harness.simulate_luminosity_sweep(env, np.ones((4, 3)), 5, obs=True)
    with pytest.raises(ValueError, match="agent-free"):
        harness.simulate_luminosity_sweep(types.SimpleNamespace(n_agents=2, batch_size=3, dim=8), np.ones(3), 5, obs=True)


def test_series_post_processing_is_shared_with_simulate_ramp():
    from therldaisyworld_amd import _ffi, harness
    stats = np.zeros((2, 3), dtype=_ffi.STATS_DTYPE)
    stats["max_k"] = [[0, 5, 6], [1000, 4, 0]]
    stats["sum_light_k"] = 6400
    env = types.SimpleNamespace(dim=8)
    L = np.ones((2, 3))
    out = harness._series_dict(env, L, stats)
    assert out["L"] is L and out["stats"] is stats
    assert np.array_equal(out["alive"], [[False, False, True], [True, False, False]])
    assert np.array_equal(out["mean_light"], np.full((2, 3), 0.1))


# ---- the gfx950 assembly ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def asm_path(tmp_path_factory):
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    import isa_report
    isa_report.OUT = str(tmp_path_factory.mktemp("dw_isa_per_world"))
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


# (per-world kernel, shared-L kernel of the same mode) by the substrings of their mangled names: HALO 0, 1, 2; SYM both ways
PAIRS = [(f"step_stream_fast_pwILi{h}EE", f"step_stream_fastILi{h}EE") for h in (0, 1, 2)] + \
        [(f"step_stream_exact_pwILi{h}ELb{s}EE", f"step_stream_exactILi{h}ELb{s}EE") for h in (0, 1, 2) for s in (0, 1)]
# VALU instructions the world-index derivation may add IN FRONT of the row loop: the strip numbering's 32-bit division by
# a run-time value (about 20 VALU instructions where the compiler does not share it with stream_body's own), the clamp
# and the readfirstlane.  The code BEHIND the loop (the exact kernels' float64 repair) is cold and not counted: it reads
# the world's float64 set through a pointer where the shared-L kernel reads kernel arguments.
INDEX_VALU_ALLOWANCE = 24


@pytest.mark.parametrize("pw,shared", PAIRS)
def test_per_world_wave_strip_kernels_cost_what_the_shared_ones_cost(asm_path, pw, shared):
    text = open(asm_path).read()
    assert not re.search(r"\tv_mfma", text)
    ks = _kernels(text)
    a = next((n for n in ks if pw in n), None)
    b = next((n for n in ks if shared in n), None)
    assert a and b, (pw, shared)
    (ia, ba), (ib, bb) = ks[a], ks[b]
    for key in ("NumVgprs", "NumAgprs", "Occupancy", "ScratchSize", "LDSByteSize"):
        assert ia[key] == ib[key], (a, key, ia[key], ib[key])
    assert ia["TotalNumSgprs"] <= ib["TotalNumSgprs"], (a, ia["TotalNumSgprs"], ib["TotalNumSgprs"])
    (la, sa), (lb, sb) = _hot_loop_span(ba), _hot_loop_span(bb)
    assert sa and sb, a
    loop_a, loop_b = la[sa[0]:sa[1] + 1], lb[sb[0]:sb[1] + 1]
    assert not any(ln.startswith("\tscratch_") for ln in _main_path(loop_a)), f"{a}: scratch traffic inside the row loop"
    # the constants are loaded once: scalar loads (the table and the kernel arguments) all sit in front of the row loop,
    # and the loop's vector loads are the shared kernel's (the rows of the two planes and their halo columns)
    assert not any(re.match(r"\ts_(buffer_)?load", ln) for ln in loop_a), f"{a}: a scalar load inside the row loop"
    vload = lambda loop: sum(1 for ln in loop if re.match(r"\t(global|flat|buffer)_load", ln))
    assert vload(loop_a) == vload(loop_b), (a, vload(loop_a), vload(loop_b))
    # ... and the table IS read by scalar loads: more of them in front of the loop than the shared kernel has
    sload = lambda lines, end: sum(1 for ln in lines[:end] if re.match(r"\ts_load_dword", ln))
    assert sload(la, sa[0]) > sload(lb, sb[0]), (a, sload(la, sa[0]), sload(lb, sb[0]))
    valu = lambda lines: sum(1 for ln in lines if ln.startswith("\tv_"))
    print(f"{a}: row loop {valu(loop_a)} VALU (shared-L: {valu(loop_b)}); in front of it {valu(la[:sa[0]])} "
          f"(shared-L: {valu(lb[:sb[0]])})")
    assert valu(loop_a) <= valu(loop_b), (a, valu(loop_a), valu(loop_b))
    assert valu(la[:sa[0]]) <= valu(lb[:sb[0]]) + INDEX_VALU_ALLOWANCE, (a, valu(la[:sa[0]]), valu(lb[:sb[0]]))


def test_generic_per_world_kernels_exist(asm_path):
    ks = _kernels(open(asm_path).read())
    for inp, precs in (("DF16_", (0, 1, 2)), ("f", (1, 2, 3)), ("d", (1, 2, 3))):
        for prec in precs:
            assert any(f"step_generic_pwI{inp}Li{prec}E" in n for n in ks), (inp, prec)


def test_no_existing_kernel_changed(asm_path):
    """The kernels as they were BEFORE the per-world variants were added are kept by the tool, not rebuilt here:
    `tools/isa_report.py --fingerprint` wrote tests/golden/kernel_fingerprint.json from the parent commit's assembly (a
    hash per kernel of its instructions and descriptor, as `--compare` normalises them).  Every kernel named there must
    still exist and hash the same; kernels that are not named there are the additions.  The hashes depend on the
    compiler: under another hipcc than the one recorded in the file the comparison says nothing and is not made."""
    import isa_report
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_fingerprint.json")))
    have = isa_report.fingerprint(asm_path)
    if have["compiler"] != want["compiler"]:
        pytest.skip(f"fingerprint recorded under another compiler: {want['compiler']!r}, here {have['compiler']!r}")
    assert len(want["kernels"]) >= 130
    gone = sorted(set(want["kernels"]) - set(have["kernels"]))
    assert not gone, gone
    differ = [n for n, h in want["kernels"].items() if have["kernels"][n] != h]
    assert not differ, isa_report.demangle(differ)
    added = sorted(set(have["kernels"]) - set(want["kernels"]))
    assert all("_pw" in n for n in added), added
