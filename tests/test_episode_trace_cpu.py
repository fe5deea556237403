"""CPU-side tests (no GPU) of dw_run_episode_trace and harness.simulate_grazing:

  * the symbol is declared in the header, exported by the library and bound by _ffi with the ten-argument signature; the ABI
    number is still 6; a null handle and a null trace are refused;
  * the compiled module holds exactly two episode_wave_stats_pw instantiations and one episode_stats_row_pw, neither wave
    instantiation touches scratch memory, and the float32 one keeps four waves per SIMD;
  * the Python surface exists, refuses wrong shapes before any device call, and simulate_ramp still refuses agents.
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


def test_symbol_is_declared_exported_and_bound():
    from therldaisyworld_amd import _ffi
    header = open(os.path.join(ROOT, "include", "daisyworld_hip.h")).read()
    assert re.search(r"\bint dw_run_episode_trace\(dw_handle\* h, int32_t nsteps, const double\* L_schedule, int policy_mode,\s*"
                     r"const uint8_t\* use_table, const int8_t\* table, uint32_t threshold_k,\s*uint8_t\* world_alive[^;]*?,"
                     r"\s*uint8_t\* agent_ok[^;]*?,\s*dw_world_stats\* trace[^;]*?\);", header)
    declared = int(re.search(r"#define DW_ABI_VERSION (\d+)\b", header).group(1))
    lib = _ffi.load()
    assert declared == _ffi.DW_ABI_VERSION == lib.dw_abi_version() == 6
    assert "dw_run_episode_trace" in _ffi.SIGNATURES
    assert lib.dw_run_episode_trace.argtypes == [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_uint8),
                                                 C.POINTER(C.c_int8), C.c_uint32, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8),
                                                 C.POINTER(_ffi.DwWorldStats)]
    assert len(lib.dw_run_episode_trace.argtypes) == 10
    Ls = np.ones(4)
    out = np.zeros((4, 1), dtype=_ffi.STATS_DTYPE)
    rc = lib.dw_run_episode_trace(None, 4, _ffi.ptr_d(Ls), 0, None, None, 5, None, None,
                                  out.ctypes.data_as(C.POINTER(_ffi.DwWorldStats)))
    assert rc == _ffi.DW_EINVAL and b"null" in lib.dw_last_error()


@pytest.fixture(scope="module")
def asm_path(tmp_path_factory):
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    import isa_report
    isa_report.OUT = str(tmp_path_factory.mktemp("dw_isa_episode_trace"))
    return isa_report.build([])


@pytest.fixture(scope="module")
def asm(asm_path):
    return open(asm_path).read()


def _kernels(text):
    """name -> (info dict, body text) for every kernel of the module."""
    out = {}
    for name in re.findall(r"\.amdhsa_kernel (\S+)\n", text):
        m = re.search(r"\n" + re.escape(name) + r":[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S)
        info = re.search(re.escape(name) + r":.*?; Kernel info:(.*?)(?=\n\t\.(?:text|section)|\Z)", text, re.S)
        if not (m and info):
            continue
        vals = {k: int(v) for k, v in re.findall(r"; (\w+)\s*[:=] (\d+)", info.group(1))}
        out[name] = (vals, m.group(1))
    return out


def test_the_new_kernels_exist_without_scratch(asm):
    ks = _kernels(asm)
    wave = sorted(n for n in ks if re.search(r"episode_wave_stats_pwILb[01]EE", n))
    assert len(wave) == 2, wave
    assert len([n for n in ks if "episode_wave_stats_pw" in n]) == 2
    assert len([n for n in ks if "episode_stats_row_pw" in n]) == 1
    # the existing one-wave-per-world kernels are still two (the new ones are separately named)
    assert len([n for n in ks if re.search(r"episode_waveILb[01]EE", n)]) == 2
    for name in wave:
        info, body = ks[name]
        assert info["ScratchSize"] == 0, (name, info["ScratchSize"])
        assert not any(ln.startswith("\tscratch_") for ln in body.split("\n")), f"{name}: a scratch access"
        assert not re.search(r"\tv_mfma", body)
        assert re.search(r"\tv_(add|max)\w*_dpp|\tv_mov_b32_dpp", body), f"{name}: no DPP operation in the reduction"
        assert info["LDSByteSize"] == 0                         # dynamic LDS only: sized per launch
    fast = next(n for n in wave if "ILb0EE" in n)
    assert ks[fast][0]["Occupancy"] >= 4, ks[fast][0]


def test_lds_of_the_largest_launch_is_under_the_default_limit():
    """The header's own static_assert restated from its formulas: constants of a 64-step segment, and per world the planes,
    the action-table slice, the agents' masks and 64 records of 12 bytes."""
    src = open(os.path.join(ROOT, "therldaisyworld_amd", "csrc", "dw_episode_wave_stats_pw.hpp")).read()
    assert re.search(r"static_assert\(episode_wave_stats_lds_bytes\(kEwMaxCells, 64\) <= 64 \* 1024", src)
    C_, N = 256, 64
    world = 16 * C_ + (64 * N + 15) // 16 * 16 + (8 * N + 15) // 16 * 16 + 64 * 12
    shared = 64 * 128 + 64 * 8 + 64                             # PhysF32 is 128 bytes (136 per step and world with its double)
    assert shared + 4 * world <= 64 * 1024


def test_python_surface_and_shape_checks_without_a_device():
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi, harness
    assert callable(amd.Engine.run_episode_trace)
    assert amd.simulate_grazing is harness.simulate_grazing
    assert "simulate_grazing" in amd.__all__

    class _NoDevice:                                           # any touch of the library is an AttributeError
        B, N = 3, 2
    with pytest.raises(ValueError, match="use_table must have shape"):
        amd.Engine.run_episode_trace(_NoDevice(), np.ones(4), _ffi.POLICY_ARGMAX, np.zeros(3, dtype=np.uint8))
    with pytest.raises(ValueError, match="table must have shape"):
        amd.Engine.run_episode_trace(_NoDevice(), np.ones(4), _ffi.POLICY_TABLE, None, np.zeros((4, 3, 1), dtype=np.int8))
    env = types.SimpleNamespace(batch_size=3, n_agents=2)
    with pytest.raises(ValueError, match="nsteps"):
        harness.simulate_grazing(env, None, 0, obs=True)
    with pytest.raises(ValueError, match="chunk"):
        harness.simulate_grazing(env, None, 3, chunk=0, obs=True)


def test_simulate_ramp_still_refuses_agents():
    from therldaisyworld_amd import harness
    env = types.SimpleNamespace(n_agents=2)
    with pytest.raises(ValueError, match="agent-free"):
        harness.simulate_ramp(env, 3)


def test_simulate_grazing_host_loop_and_draw_order():
    """The host loop (any callable agent) on a stand-in environment: one `env.step` and one `reduce()` per step, rows and
    flags in step order, the luminosity each step USED; and the device loop's draws - one coin per step, the batch's codes
    on the random branch - for exactly nsteps steps, in chunks, against the reference's loop on the same seed."""
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi, harness
    B, N, n = 3, 2, 11

    class Eng:
        def __init__(self):
            self.calls, self.t = [], 0

        def reduce(self):
            s = np.zeros(B, dtype=_ffi.STATS_DTYPE)
            s["max_k"], s["sum_light_k"], s["sum_dark_k"], s["reserved"] = self.t, 64 * self.t, self.t, 7
            return s

        def run_episode_trace(self, Ls, mode, use_table, table, thr):
            k = len(Ls)
            self.calls.append((np.array(Ls), mode, use_table.copy(), table.copy(), thr))
            s = np.zeros((k, B), dtype=_ffi.STATS_DTYPE)
            s["max_k"] = (self.t + 1 + np.arange(k))[:, None]
            self.t += k
            return s, s["max_k"] > thr, np.ones((k, B, N), dtype=bool)

    class Env:
        def __init__(self):
            self.batch_size, self.n_agents, self.dim = B, N, 8
            self.precision, self.collision_mode = "exact", 0
            self.L, self.dL, self.step_count = 0.9, 0.01, 0
            self.ramp_up_down, self.ramp_period, self.ddL, self.min_L, self.max_L = False, 12, 0.0, 0.5, 1.5
            self._engine, self.actions, self.invalidated = Eng(), [], 0

        def update_L(self, L):
            self.step_count += 1
            return max(min(L + self.dL, self.max_L), self.min_L)

        def _invalidate(self):
            self.invalidated += 1

        def step(self, action):
            self.actions.append(action)
            self._engine.t += 1
            self.L = self.update_L(self.L)
            done = np.zeros((B, N, 1), dtype=bool)
            done[0, 1] = True
            return "obs%d" % self._engine.t, None, done, {}

    # host loop: a callable that is no Greedy
    env = Env()
    out = harness.simulate_grazing(env, lambda obs: ("act", obs), n, obs="obs0")
    assert env.actions == [("act", "obs%d" % t) for t in range(n)] and not env._engine.calls
    assert np.array_equal(out["stats"]["max_k"], np.arange(1, n + 1)[:, None] * np.ones((1, B), dtype=np.uint32))
    assert not out["stats"]["reserved"].any()
    assert out["L"][0] == 0.9 and np.allclose(out["L"], 0.9 + 0.01 * np.arange(n), rtol=0, atol=1e-12)
    assert out["agent_ok"].shape == (n, B, N) and np.array_equal(out["agents_alive"], np.tile([1, 2, 2], (n, 1)))
    assert np.array_equal(out["alive"], out["stats"]["max_k"] > 5) and env.step_count == n

    # device loop: chunks of 4 after the first step, epsilon-greedy draws in the reference's order
    env = Env()
    agent = amd.Greedy(epsilon=0.5)
    np.random.seed(11)
    real_call = amd.Greedy.__call__
    obs0 = np.zeros((B, N, 7, 3, 3))
    out = harness.simulate_grazing(env, agent, n, chunk=4, obs=obs0)
    after = np.random.get_state()
    assert len(env.actions) == 1 and [len(c[0]) for c in env._engine.calls] == [4, 4, 2]
    assert all(c[1] == _ffi.POLICY_ARGMAX and c[4] == harness.LIFESPAN_THRESHOLD_K for c in env._engine.calls)
    assert env.step_count == n and env.invalidated >= 3
    assert np.array_equal(out["stats"]["max_k"][:, 0], np.arange(1, n + 1))
    L_used = np.concatenate([[0.9], *[c[0] for c in env._engine.calls]])
    assert np.array_equal(out["L"], L_used) and np.allclose(np.diff(L_used), 0.01, rtol=0, atol=1e-12)
    use_table = np.concatenate([c[2] for c in env._engine.calls])
    table = np.concatenate([c[3] for c in env._engine.calls])
    np.random.seed(11)
    real_call(agent, obs0)                                      # step 0's draws (the stand-in ignores the action)
    for t in range(n - 1):
        if np.random.rand() > 0.5:
            assert use_table[t] == 0
        else:
            assert use_table[t] == 1
            assert np.array_equal(table[t], np.random.randint(9, size=(B, N, 1, 1)).reshape(B, N))
    assert 0 < use_table.sum() < n - 1
    want = np.random.get_state()
    assert after[2] == want[2] and np.array_equal(after[1], want[1])
