"""CPU-side tests (no GPU) of the per-step world statistics (dw_step_n_trace, ABI 6):

  * the symbol is declared, exported and bound; a null handle is refused; the ABI version is 6 everywhere;
  * the gfx950 code of the trace pair kernels (one extra compilation of csrc/dw_api.hip with --save-temps, the recipe of
    test_isa_properties.py): they exist for overlapped and rotating strips in both arithmetic modes, keep scratch traffic
    off the main path of their row loops, evaluate nothing twice, and reach the occupancy DESIGN.md 3.2f states;
  * harness.simulate_ramp's host bookkeeping on the reference's recorded triangle ramp (fixture G12).
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# waves per SIMD the trace pair kernels are planned for
TRACE_FAST_OCCUPANCY = 3
TRACE_EXACT_OCCUPANCY = 2


def test_symbol_is_declared_exported_and_bound():
    from therldaisyworld_amd import _ffi
    header = open(os.path.join(ROOT, "include", "daisyworld_hip.h")).read()
    assert re.search(r"\bint dw_step_n_trace\(dw_handle\* h, int32_t nsteps, const double\* L_schedule, dw_world_stats\* trace", header)
    assert re.search(r"#define DW_ABI_VERSION 6\b", header)
    assert _ffi.DW_ABI_VERSION == 6
    assert "dw_step_n_trace" in _ffi.SIGNATURES
    lib = _ffi.load()
    assert lib.dw_abi_version() == 6
    assert lib.dw_step_n_trace.argtypes == [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(_ffi.DwWorldStats)]
    Ls = np.zeros(4)
    out = np.zeros((4, 1), dtype=_ffi.STATS_DTYPE)
    rc = lib.dw_step_n_trace(None, 4, _ffi.ptr_d(Ls), out.ctypes.data_as(C.POINTER(_ffi.DwWorldStats)))
    assert rc == _ffi.DW_EINVAL and b"null" in lib.dw_last_error()


def test_python_surface():
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import harness
    assert callable(amd.Engine.step_n_trace)
    assert amd.simulate_ramp is harness.simulate_ramp


# ---- the gfx950 assembly ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    import isa_report
    isa_report.OUT = str(tmp_path_factory.mktemp("dw_isa_trace"))
    return open(isa_report.build([])).read()


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


def _hot_loop(body):
    lines = body.split("\n")
    labels = {m.group(1): i for i, ln in enumerate(lines) for m in [re.match(r"(\.LBB\S+):", ln)] if m}
    best, best_pk = None, -1
    for i, ln in enumerate(lines):
        m = re.match(r"\ts_c?branch\S* (\.LBB\S+)", ln)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            npk = sum(1 for x in lines[labels[m.group(1)]:i + 1] if x.startswith("\tv_pk_"))
            if npk > best_pk:
                best, best_pk = (labels[m.group(1)], i), npk
    return lines[best[0]:best[1] + 1] if best else []


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


def test_trace_pair_kernels_exist_and_keep_their_row_loops_clean(asm):
    assert not re.search(r"\tv_mfma", asm)
    ks = _kernels(asm)
    trace = {n: v for n, v in ks.items() if "trace_pair" in n}
    assert not any("step_stream" in n for n in trace)        # the budgets of test_isa_properties.py are not theirs
    wanted = [f"trace_pair_fastILi{m}E" for m in (0, 1)] + [f"trace_pair_exactILi{m}ELb{s}E" for m in (0, 1) for s in (0, 1)]
    for w in wanted:                                          # overlapped strips (0), in-wave rotation (1); SYM both ways
        name = next((n for n in trace if w in n), None)
        assert name, w
        info, body = trace[name]
        loop = _hot_loop(body)
        assert loop, name
        assert not any(ln.startswith("\tscratch_") for ln in _main_path(loop)), f"{name}: scratch traffic inside the row loop"
        ntr = sum(1 for ln in loop if re.match(r"\tv_(sqrt|rcp)_f32", ln))
        npk = sum(1 for ln in loop if ln.startswith("\tv_pk_"))
        assert npk >= 150, (name, npk)
        if "fast" in w:
            assert ntr == 144, (name, ntr)                    # 3 rows x 4 columns x 2 steps x 6: nothing evaluated twice
            assert info["Occupancy"] >= TRACE_FAST_OCCUPANCY, (name, info["NumVgprs"])
        else:
            assert ntr >= 144, (name, ntr)
            assert info["Occupancy"] >= TRACE_EXACT_OCCUPANCY, (name, info["NumVgprs"])


# ---- simulate_ramp's host bookkeeping ---------------------------------------------------------------------------------
class _HostEnv:
    """The drop-in's host scalars without a device: just what the ramp bookkeeping touches."""

    def __init__(self, g, n_agents=0):
        from therldaisyworld_amd.daisy_world_rl import RLDaisyWorld
        self._update_L = RLDaisyWorld.update_L
        self.n_agents, self.dim, self.batch_size = n_agents, 8, 3
        self.ramp_up_down, self.ramp_period, self.ddL = True, 12, 0.01
        self.min_L, self.max_L = 0.9, 1.2
        self.L, self.dL, self.step_count = float(g["L0"]), float(g["dL0"]), 0
        self._L_pass = self.L
        self.invalidated = 0

    def update_L(self, L):
        return self._update_L(self, L)

    def _invalidate(self):
        self.invalidated += 1


@pytest.mark.parametrize("k", [1, 11, 12, 13, 36, 60])
def test_simulate_ramp_bookkeeping_on_the_triangle_ramp_g12(golden, k):
    """G12 (ramp_period = 12, min_L, max_L, ddL = 0.9, 1.2, 0.01) recorded L, dL, min_L, max_L, step_count AFTER each of 60
    reference steps (it ran with agents; only its luminosity bookkeeping is used): after k steps through the ramp
    harness the scalars equal entry k - 1, and the schedule's entry j is the luminosity step j used, i.e. the recorded L
    after step j - 1."""
    from therldaisyworld_amd import _ffi, harness
    g = golden("G12_ramp_up_down")
    env = _HostEnv(g)
    calls = []

    def stub(Ls):
        calls.append(np.array(Ls))
        return np.zeros((len(Ls), env.batch_size), dtype=_ffi.STATS_DTYPE)

    out = harness._ramp_series(env, k, stub)
    assert len(calls) == 1 and calls[0].shape == (k,)        # ONE engine call
    assert env.L == g["L"][k - 1] and env.dL == g["dL"][k - 1]
    assert env.min_L == g["min_L"][k - 1] and env.max_L == g["max_L"][k - 1]
    assert env.step_count == g["step_count"][k - 1] == k
    assert env.invalidated >= 1
    assert out["L"][0] == float(g["L0"])
    for j in range(1, k):
        assert out["L"][j] == g["L"][j - 1], j
    assert np.array_equal(out["L"], calls[0])
    assert env._L_pass == out["L"][-1]
    assert out["mean_light"].shape == out["mean_dark"].shape == out["max_cover"].shape == (k, 3)
    assert out["alive"].dtype == bool and not out["alive"].any()
    # the next schedule continues where the recorded series does
    if k < 60:
        assert harness._luminosity_schedule(env, 1)[0] == g["L"][k - 1]


def test_simulate_ramp_series_arithmetic_and_agents():
    from therldaisyworld_amd import _ffi, harness

    class G(dict):
        pass
    env = _HostEnv({"L0": 0.9, "dL0": 0.025})

    def stub(Ls):
        s = np.zeros((len(Ls), 3), dtype=_ffi.STATS_DTYPE)
        s["max_k"][1] = (5, 6, 1000)
        s["sum_light_k"][1] = (64 * 300, 0, 64 * 1000)
        s["sum_dark_k"][1] = (0, 1, 0)
        return s

    out = harness._ramp_series(env, 2, stub)
    assert np.array_equal(out["alive"][1], [False, True, True])          # the notebook's test: max > 0.005
    assert np.array_equal(out["mean_light"][1], [0.3, 0.0, 1.0])
    assert out["mean_dark"][1][1] == 1 / 1000.0 / 64.0
    assert np.array_equal(out["max_cover"][1], [0.005, 0.006, 1.0])
    with pytest.raises(ValueError):
        harness._ramp_series(_HostEnv({"L0": 0.9, "dL0": 0.025}, n_agents=2), 3, stub)
    with pytest.raises(ValueError):
        harness.simulate_ramp(_HostEnv({"L0": 0.9, "dL0": 0.025}, n_agents=2), 3)
