"""CPU-side tests (no GPU) of the per-world temperature statistics (dw_reduce_temperature, dw_step_n_trace_temperature):

  * the symbols are declared, exported and bound, the record is 32 bytes, null handles are refused;
  * the host `dead_temp` formula against the oracle's calculate_temperature over the luminosity ramp;
  * the dict `simulate_ramp` / `simulate_luminosity_sweep` assemble from temperature records;
  * the Python surface refuses a wrong shape before any device call;
  * the gfx950 code (one compilation of csrc/dw_api.hip with --save-temps, the recipe of test_per_world_cpu.py):
    temp_moments_pw exists for the three input formats and both sources of the constants, uses no scratch memory and no
    atomic, and reads the table of constants by scalar loads.
"""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import daisy_oracle as O  # noqa: E402


def test_symbols_are_declared_exported_and_bound():
    from therldaisyworld_amd import _ffi
    header = open(os.path.join(ROOT, "include", "daisyworld_hip.h")).read()
    assert re.search(r"typedef struct dw_temp_stats \{ double mean, std, min, max; \} dw_temp_stats;", header)
    assert re.search(r"\bint dw_reduce_temperature\(dw_handle\* h, double L, dw_temp_stats\* per_world", header)
    assert re.search(r"\bint dw_step_n_trace_temperature\(dw_handle\* h, int32_t nsteps, const double\* L_schedule, int per_world,",
                     header)
    assert "daisy_world_rl.py:410,415" in header and "notebook_helpers.py:50-52" in header
    assert C.sizeof(_ffi.DwTempStats) == 32 == _ffi.TEMP_STATS_DTYPE.itemsize
    assert _ffi.TEMP_STATS_DTYPE.names == ("mean", "std", "min", "max")
    assert [n for n, _ in _ffi.DwTempStats._fields_] == ["mean", "std", "min", "max"]
    lib = _ffi.load()
    assert lib.dw_abi_version() == _ffi.DW_ABI_VERSION
    pt, ps = C.POINTER(_ffi.DwTempStats), C.POINTER(_ffi.DwWorldStats)
    assert lib.dw_reduce_temperature.argtypes == [C.c_void_p, C.c_double, pt]
    assert lib.dw_step_n_trace_temperature.argtypes == [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.c_int, ps, pt]
    out = np.zeros((4, 1), dtype=_ffi.TEMP_STATS_DTYPE)
    assert lib.dw_reduce_temperature(None, 1.0, out.ctypes.data_as(pt)) == _ffi.DW_EINVAL
    assert b"null" in lib.dw_last_error()
    Ls = np.ones((4, 1))
    for per_world in (0, 1):
        assert lib.dw_step_n_trace_temperature(None, 4, _ffi.ptr_d(Ls), per_world, None, out.ctypes.data_as(pt)) == _ffi.DW_EINVAL
    assert not out["mean"].any()


def test_python_surface_and_shape_checks_without_a_device():
    import inspect
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import harness
    assert callable(amd.Engine.reduce_temperature) and callable(amd.Engine.step_n_trace_temperature)
    for fn in (harness.simulate_ramp, harness.simulate_luminosity_sweep):
        assert inspect.signature(fn).parameters["temperature"].default is False

    class _NoDevice:                                           # any touch of the library is an AttributeError
        B = 3
    for bad in (np.ones((4, 2)), np.ones((4, 3, 1))):
        with pytest.raises(ValueError, match="shape"):
            amd.Engine.step_n_trace_temperature(_NoDevice(), bad)
    with pytest.raises(ValueError, match="agent-free"):
        harness.simulate_ramp(types.SimpleNamespace(n_agents=2), 5, obs=True, temperature=True)
    with pytest.raises(ValueError, match="shape"):
        harness.simulate_luminosity_sweep(types.SimpleNamespace(n_agents=0, batch_size=3, dim=8), np.ones(4), 5, obs=True,
                                          temperature=True)


def test_dead_temperature_is_the_oracles_over_the_ramp():
    """ref :407-408.  The same float64 expression, once through NumPy's array power and once through Python's scalar
    one: they may differ in the last bit."""
    from therldaisyworld_amd import harness
    P = O.Params()
    L = P.min_L + (P.max_L - P.min_L) * np.arange(513) / 512.0
    ours = harness.dead_temperature(P, L)
    assert ours.shape == L.shape and ours.dtype == np.float64
    one = np.ones((1, 1, 2, 2))
    want = np.array([O.calculate_temperature(P, float(x), 0.5 * one, 0.5 * one)[4][0] for x in L])
    np.testing.assert_allclose(ours, want, rtol=4e-16, atol=0)
    assert 255.0 < ours[0] < ours[-1] < 345.0 and np.all(np.diff(ours) > 0)
    assert harness.dead_temperature(P, np.ones((4, 3))).shape == (4, 3)
    assert np.ndim(harness.dead_temperature(P, 1.0)) == 0


def test_series_dict_with_temperature_records():
    from therldaisyworld_amd import _ffi, harness
    stats = np.zeros((2, 3), dtype=_ffi.STATS_DTYPE)
    stats["max_k"] = [[0, 5, 6], [1000, 4, 0]]
    stats["sum_light_k"] = 6400
    temps = np.zeros((2, 3), dtype=_ffi.TEMP_STATS_DTYPE)
    temps["mean"] = [[290.0, 291.0, 292.0], [293.0, 294.0, 295.0]]
    temps["std"] = 0.5
    temps["min"] = temps["mean"] - 1.0
    temps["max"] = temps["mean"] + 2.0
    env = types.SimpleNamespace(dim=8, S=1000.0, sigma=5.67e-8, albedo_bare=0.5)
    for L in (np.array([0.8, 1.1]), np.array([[0.8, 0.9, 1.0], [1.1, 1.2, 1.3]])):
        plain = harness._series_dict(env, L, stats)
        out = harness._series_dict(env, L, stats, temps)
        assert set(out) - set(plain) == {"mean_temp", "std_temp", "min_temp", "max_temp", "dead_temp"}
        for k in plain:
            assert np.array_equal(out[k], plain[k]), k
        assert out["L"] is L and out["stats"] is stats
        assert np.array_equal(out["mean_temp"], temps["mean"]) and np.array_equal(out["std_temp"], np.full((2, 3), 0.5))
        assert np.array_equal(out["min_temp"], temps["mean"] - 1.0) and np.array_equal(out["max_temp"], temps["mean"] + 2.0)
        assert out["dead_temp"].shape == L.shape
        assert np.array_equal(out["dead_temp"], ((1000.0 * L * 0.5) / 5.67e-8) ** 0.25)
    assert np.array_equal(harness._series_dict(env, L, stats)["mean_light"], np.full((2, 3), 0.1))


# ---- the gfx950 assembly ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    import isa_report
    isa_report.OUT = str(tmp_path_factory.mktemp("dw_isa_temperature"))
    text = open(isa_report.build([])).read()
    out = {}
    for name in re.findall(r"\.amdhsa_kernel (\S+)\n", text):
        m = re.search(r"\n" + re.escape(name) + r":[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S)
        info = re.search(re.escape(name) + r":.*?; Kernel info:(.*?)(?=\n\t\.(?:text|section)|\Z)", text, re.S)
        if m and info:
            out[name] = ({k: int(v) for k, v in re.findall(r"; (\w+)\s*[:=] (\d+)", info.group(1))}, m.group(1))
    return out


@pytest.mark.parametrize("table", [0, 1], ids=["by-value", "table"])
@pytest.mark.parametrize("inp", ["DF16_", "f", "d"], ids=["binary16", "float32", "float64"])
def test_temp_moments_kernels(kernels, inp, table):
    name = next((n for n in kernels if f"temp_moments_pwI{inp}Lb{table}EE" in n), None)
    assert name, (inp, table, [n for n in kernels if "temp_moments" in n])
    info, body = kernels[name]
    assert info["ScratchSize"] == 0, (name, info["ScratchSize"])
    lines = body.split("\n")
    assert not any(re.match(r"\tscratch_", ln) for ln in lines), name
    assert not any("atomic" in ln for ln in lines), name       # deterministic: partials, no atomics
    assert any(re.match(r"\tv_(rsq|sqrt)_f64", ln) for ln in lines), name   # the float64 fourth roots of cell_f64
    assert info["LDSByteSize"] == 128                           # the four waves' four partial values
    sloads = sum(1 for ln in lines if re.match(r"\ts_load_dword", ln))
    by_value = next(n for n in kernels if f"temp_moments_pwI{inp}Lb0EE" in n)
    if table:                                                   # the world's constants come from the table, by scalar loads
        assert sloads > sum(1 for ln in kernels[by_value][1].split("\n") if re.match(r"\ts_load_dword", ln)), name


def test_finishing_kernel_exists_and_every_new_kernel_is_named_per_world(kernels):
    fin = [n for n in kernels if "temp_moments_finish_pw" in n]
    assert len(fin) == 1 and kernels[fin[0]][0]["ScratchSize"] == 0
    assert not any("atomic" in ln for ln in kernels[fin[0]][1].split("\n"))
    assert all("_pw" in n for n in kernels if "temp_moments" in n)
