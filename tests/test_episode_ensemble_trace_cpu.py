"""CPU-side tests (no GPU) of dw_run_episode_ensemble_trace and harness.simulate_grazing_sweep:

  * the symbol is declared in the header, exported by the library and bound by _ffi with the declared argument list; the
    ABI number is still 6; a null handle is refused, and so is a call without a record array;
  * Engine.run_episode_ensemble takes `trace` and `temperature`: with both false it makes the call it has always made and
    returns its pair, otherwise the new call with the arrays asked for (a stub library object, no device);
  * the harness refuses what it cannot run before any device call, and its post-processing reshapes every per-world
    entry to (n, S, Bs, ...);
  * the staging layout of the call (tests/episode_ens_trace_staging_driver.cpp, host C++17 compiled by the clang++ of ROCm;
    once more with -fsanitize=address,undefined as the stand-alone program it is): the inputs of
    dw_run_episode_ensemble where they were, the records behind the flags, and which calls pass the page-locked image's
    64 MiB - the README sweep's 64-step chunk does not, 4096 steps of 1000 worlds do.
"""
import ctypes as C
import json
import os
import re
import subprocess
import types

import numpy as np
import pytest

from test_plan_cpu import CSRC, ROOT, _rocm_clang


def _new_argtypes(_ffi):
    return [C.c_void_p, C.c_int32, C.POINTER(_ffi.DwWorldParams), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_uint8),
            C.POINTER(C.c_int8), C.c_uint32, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(_ffi.DwWorldStats),
            C.POINTER(_ffi.DwTempStats)]


def test_symbol_is_declared_exported_and_bound():
    from therldaisyworld_amd import _ffi
    header = open(os.path.join(ROOT, "include", "daisyworld_hip.h")).read()
    m = re.search(r"\bint dw_run_episode_ensemble_trace\(([^;]*)\);", header)
    assert m, "dw_run_episode_ensemble_trace is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    assert len(args) == 12 == len(_ffi.SIGNATURES["dw_run_episode_ensemble_trace"][1])
    assert "dw_world_stats* trace" in args[10] and "dw_temp_stats* temps" in args[11]
    assert re.search(r"#define DW_ABI_VERSION 6\b", header) and _ffi.DW_ABI_VERSION == 6
    assert '"; ensemble trace: ..."' in header
    lib = _ffi.load()
    assert lib.dw_abi_version() == 6
    assert lib.dw_run_episode_ensemble_trace.argtypes == _new_argtypes(_ffi)
    Ls = np.ones((4, 1))
    tab = np.zeros(1, dtype=_ffi.WORLD_PARAMS_DTYPE)
    stats = np.zeros((4, 1), dtype=_ffi.STATS_DTYPE)
    rc = lib.dw_run_episode_ensemble_trace(None, 4, tab.ctypes.data_as(C.POINTER(_ffi.DwWorldParams)), _ffi.ptr_d(Ls), 0, None, None,
                                           5, None, None, stats.ctypes.data_as(C.POINTER(_ffi.DwWorldStats)), None)
    assert rc == _ffi.DW_EINVAL and b"null" in lib.dw_last_error()
    assert not stats.view(np.uint8).any()


class _StubLib:
    """Records the calls Engine.run_episode_ensemble makes; fills what a call would write with recognisable values."""

    def __init__(self):
        self.calls = []

    def dw_run_episode_ensemble(self, *args):
        self.calls.append(("dw_run_episode_ensemble", args))
        return 0

    def dw_run_episode_ensemble_trace(self, *args):
        self.calls.append(("dw_run_episode_ensemble_trace", args))
        K = args[1]
        if args[10]:
            for i in range(K * 3):
                args[10][i].max_k = 7
        if args[11]:
            for i in range(K * 3):
                args[11][i].mean = 295.0
        return 0


def _stub_engine():
    import therldaisyworld_amd as amd

    class _Stub:
        B, N = 3, 2
        _h = C.c_void_p(1)
        _world_table = amd.Engine._world_table
        run_episode_ensemble = amd.Engine.run_episode_ensemble

        def _check(self, rc):
            assert rc == 0
    eng = _Stub()
    eng._lib = _StubLib()
    return eng


def test_engine_makes_todays_call_unless_records_are_asked_for():
    from therldaisyworld_amd import _ffi
    K = 4
    tab = np.zeros(3, dtype=_ffi.WORLD_PARAMS_DTYPE)
    L = np.ones((K, 3))
    codes = np.zeros((K, 3, 2), dtype=np.int8)
    eng = _stub_engine()
    out = eng.run_episode_ensemble(tab, L, _ffi.POLICY_TABLE, None, codes, 5)
    (name, args), = eng._lib.calls
    assert name == "dw_run_episode_ensemble" and len(args) == 10 and args[1] == K and args[4] == _ffi.POLICY_TABLE and args[7] == 5
    assert len(out) == 2 and out[0].shape == (K, 3) and out[0].dtype == np.bool_ and out[1].shape == (K, 3, 2)
    assert eng.run_episode_ensemble(tab, L, _ffi.POLICY_TABLE, None, codes, 5, trace=False, temperature=False)[0].shape == (K, 3)
    assert [c[0] for c in eng._lib.calls] == ["dw_run_episode_ensemble"] * 2

    for trace, temperature in ((True, True), (True, False), (False, True)):
        eng = _stub_engine()
        alive, ok, stats, temps = eng.run_episode_ensemble(tab, L, _ffi.POLICY_ARGMAX, None, codes, 5, trace=trace,
                                                           temperature=temperature)
        (name, args), = eng._lib.calls
        assert name == "dw_run_episode_ensemble_trace" and len(args) == 12 and args[:2] == (eng._h, K)
        assert alive.shape == (K, 3) and alive.dtype == np.bool_ and ok.shape == (K, 3, 2) and ok.dtype == np.bool_
        if trace:
            assert stats.dtype == _ffi.STATS_DTYPE and stats.shape == (K, 3) and (stats["max_k"] == 7).all()
        else:
            assert stats is None and args[10] is None
        if temperature:
            assert temps.dtype == _ffi.TEMP_STATS_DTYPE and temps.shape == (K, 3) and (temps["mean"] == 295.0).all()
        else:
            assert temps is None and args[11] is None
    eng = _stub_engine()
    with pytest.raises(ValueError, match="shape"):
        eng.run_episode_ensemble(tab, np.ones((K, 2)), _ffi.POLICY_ARGMAX, trace=True)
    assert not eng._lib.calls


def test_harness_surface_and_refusals_without_a_device():
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import harness
    assert amd.simulate_grazing_sweep is harness.simulate_grazing_sweep and "simulate_grazing_sweep" in amd.__all__
    env = types.SimpleNamespace(batch_size=6, n_agents=2, precision="exact", collision_mode=0)
    greedy = amd.Greedy()
    two = [{"params": {}, "agent": greedy}] * 2
    with pytest.raises(ValueError, match="batch_size"):
        harness.simulate_grazing_sweep(env, two, 4, 10, obs=True)
    with pytest.raises(ValueError, match="Greedy or None"):
        harness.simulate_grazing_sweep(env, [{"params": {}, "agent": lambda obs: obs}] * 2, 3, 10, obs=True)
    with pytest.raises(ValueError, match="nsteps"):
        harness.simulate_grazing_sweep(env, two, 3, 0, obs=True)
    with pytest.raises(ValueError, match="chunk"):
        harness.simulate_grazing_sweep(env, two, 3, 10, chunk=0, obs=True)
    for over in ({"precision": "f64"}, {"collision_mode": 1}):
        bad = types.SimpleNamespace(**{**vars(env), **over})
        with pytest.raises(ValueError, match="device-resident"):
            harness.simulate_grazing_sweep(bad, two, 3, 10, obs=True)


# ---- the staging layout -----------------------------------------------------------------------------------------------
STATS, ROW, P32, P64 = 24, 32, 128, 128
ORDER = ["member_a", "member_b", "reward", "done", "p32", "ls", "p64", "use_table", "table", "world_alive", "agent_ok", "trace",
         "code", "pair_stats"]


def _build(tmp, extra=()):
    exe = tmp / ("episode_ens_trace_staging_driver" + ("_san" if extra else ""))
    subprocess.check_call([_rocm_clang(), "-std=c++17", "-O2", "-Wall", "-Wextra", *extra, "-I", CSRC,
                           os.path.join(ROOT, "tests", "episode_ens_trace_staging_driver.cpp"), "-o", str(exe)])
    return exe


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    if _rocm_clang() is None:
        pytest.skip("the clang++ of ROCm is not installed")
    return tmp_path_factory.mktemp("episode_ens_trace_staging")


@pytest.fixture(scope="module")
def driver_output(build_dir):
    out = subprocess.run([str(_build(build_dir))], capture_output=True, text=True, check=True)
    return json.loads(out.stdout)


def test_records_sit_behind_the_flags_and_the_inputs_stay(driver_output):
    assert driver_output["sizes"] == {"StatsDev": STATS, "temp_row": ROW, "PhysF32": P32, "PhysF64": P64}
    cases = driver_output["cases"]
    assert len(cases) % 3 == 0
    for flags, trace, temps in zip(cases[0::3], cases[1::3], cases[2::3]):
        assert (flags["form"], trace["form"], temps["form"]) == ("flags", "trace", "temps")
        K, B, N, rows = flags["K"], flags["B"], flags["N"], flags["rows"]
        what = (K, B, N)
        assert rows == min(K, max(64, (32 << 20) // (136 * B) // 64 * 64)), what
        base = {r[0]: r for r in flags["regions"]}
        assert base["p32"][2] == P32 * rows * B and base["ls"][2] == 8 * rows * B and base["p64"][2] == P64 * B, what
        assert base["trace"][2] == 0 and flags["stats_bytes"] == 0 and flags["temps_bytes"] == 0
        for c in (trace, temps):
            by = {r[0]: r for r in c["regions"]}
            assert [r[0] for r in c["regions"]] == ORDER
            for name in ORDER[:ORDER.index("trace")]:                 # inputs and flags: where dw_run_episode_ensemble has them
                assert by[name] == base[name], (what, c["form"], name)
            assert c["input_end_table"] == flags["input_end_table"] and c["image_inputs_only"] == by["world_alive"][1], what
            assert c["image_inputs_only"] >= c["input_end_table"], what
            assert c["stats_bytes"] == STATS * K * B, what
            assert c["temps_bytes"] == (ROW * K * B if c["form"] == "temps" else 0), what
            assert by["trace"][2] == c["stats_bytes"] + c["temps_bytes"], what
            assert c["temps_off"] == by["trace"][1] + c["stats_bytes"] and c["temps_off"] % 8 == 0, what
            assert by["trace"][1] % 256 == 0 and by["trace"][1] >= by["agent_ok"][1] + by["agent_ok"][2], what
            assert c["total"] == (by["trace"][1] + by["trace"][2] + 255) // 256 * 256, what
            assert c["fits_image"] == (c["total"] <= 64 << 20), what


def test_which_calls_pass_the_image(driver_output):
    by = {(c["form"], c["K"], c["B"], c["N"]): c for c in driver_output["cases"]}
    assert by[("temps", 64, 1000, 4)]["fits_image"] == 1          # the README sweep's chunk: staged, one copy back
    assert by[("temps", 70, 2000, 2)]["fits_image"] == 1
    big = by[("temps", 4096, 1000, 4)]
    assert big["fits_image"] == 0 and big["stats_bytes"] + big["temps_bytes"] == 56 * 4096 * 1000    # 229 MB of records
    assert big["image_inputs_only"] <= 64 << 20                   # ... whose inputs alone are a modest image


def test_driver_is_clean_under_the_sanitizers(build_dir, driver_output):
    """The same stand-alone host program with -fsanitize=address,undefined: same answers, nothing reported."""
    probe = build_dir / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    can = subprocess.run([_rocm_clang(), "-fsanitize=address,undefined", str(probe), "-o", str(build_dir / "probe")],
                         capture_output=True).returncode == 0
    if not can:
        pytest.skip("this clang++ does not link its sanitizer runtime")
    exe = _build(build_dir, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    assert json.loads(out.stdout) == driver_output
