"""CPU-side tests (no GPU) of the episode loop with frames: dw_run_episode_frames, Engine.run_episode_frames and
harness.simulate_grazing_frames.

  * the symbol is declared, exported and bound with the declared argument list; dw_agent_frame is 16 bytes with its members
    at 0 / 4 / 8; null arguments are refused; the ABI version is 6 everywhere;
  * the launch split of the one-wave-per-world form (plan_frame_launches, csrc/dw_episode_staging.hpp), printed by
    tests/episode_frames_driver.cpp over K x stride x ring capacity: the launches tile [0, K) without gap or overlap, every
    launch but the last is a whole number of strides, no launch holds more frames than the ring, the frames across
    launches number K / stride at the steps (f + 1) * stride - 1, and an unlimited ring gives one launch;
  * simulate_grazing_frames against a fake engine: the lengths and strides of the device calls, the schedule passed, keys,
    shapes, frame_steps / frame_L, cover scaled to fractions, an agent-free environment served without agent_pos.
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from test_plan_cpu import CSRC, ROOT, _rocm_clang

KS = (1, 2, 63, 64, 65, 130, 4096)
STRIDES = (1, 3, 7, 64, 100)
RINGS = (1, 2, 5, 0)                                            # 0: unlimited


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound():
    from therldaisyworld_amd import _ffi
    header = open(os.path.join(ROOT, "include", "daisyworld_hip.h")).read()
    assert re.search(r"\bint dw_run_episode_frames\(dw_handle\* h, int32_t nsteps, const double\* L_schedule, int policy_mode,"
                     r"\s*const uint8_t\* use_table, const int8_t\* table, uint32_t threshold_k,\s*uint8_t\* world_alive[^;]*?,"
                     r"\s*uint8_t\* agent_ok[^;]*?,\s*dw_world_stats\* trace[^;]*?,\s*dw_temp_stats\* temps[^;]*?,"
                     r"\s*const dw_frame_spec\* spec, int32_t stride,\s*dw_tile_cover\* cover[^;]*?,\s*double\* temp_mean[^;]*?,"
                     r"\s*dw_agent_frame\* agents[^;]*?\);", header)
    assert re.search(r"typedef struct dw_agent_frame \{ int32_t row, col; double state; \} dw_agent_frame;", header)
    declared = int(re.search(r"#define DW_ABI_VERSION (\d+)\b", header).group(1))
    lib = _ffi.load()
    assert declared == _ffi.DW_ABI_VERSION == lib.dw_abi_version() == 6
    assert lib.dw_run_episode_frames.restype == C.c_int
    assert lib.dw_run_episode_frames.argtypes == [
        C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_int8), C.c_uint32,
        C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(_ffi.DwWorldStats), C.POINTER(_ffi.DwTempStats),
        C.POINTER(_ffi.DwFrameSpec), C.c_int32, C.POINTER(_ffi.DwTileCover), C.POINTER(C.c_double), C.POINTER(_ffi.DwAgentFrame)]
    assert C.sizeof(_ffi.DwAgentFrame) == 16 == _ffi.AGENT_FRAME_DTYPE.itemsize
    assert [(n, getattr(_ffi.DwAgentFrame, n).offset) for n, _ in _ffi.DwAgentFrame._fields_] == [("row", 0), ("col", 4), ("state", 8)]
    assert [(n, _ffi.AGENT_FRAME_DTYPE.fields[n][1]) for n in _ffi.AGENT_FRAME_DTYPE.names] == [("row", 0), ("col", 4), ("state", 8)]
    # a null handle, schedule or spec is refused before anything else
    spec = _ffi.DwFrameSpec(1, 1, 0, None)
    Ls, tm = np.ones(4), np.zeros(4)
    fake = C.c_void_p(8)                                        # never dereferenced: the null checks come first

    def call(h, ls, sp):
        return lib.dw_run_episode_frames(h, 4, ls, 0, None, None, 5, None, None, None, None, sp, 1, None, _ffi.ptr_d(tm), None)
    assert call(None, _ffi.ptr_d(Ls), C.byref(spec)) == _ffi.DW_EINVAL and b"null" in lib.dw_last_error()
    assert call(fake, None, C.byref(spec)) == _ffi.DW_EINVAL and b"null" in lib.dw_last_error()
    assert call(fake, _ffi.ptr_d(Ls), None) == _ffi.DW_EINVAL and b"null" in lib.dw_last_error()


def test_the_library_checks_the_record_layout():
    src = open(os.path.join(CSRC, "dw_api.hip")).read()
    assert "static_assert(sizeof(dw_agent_frame) == 16 && sizeof(dw_agent_frame) == sizeof(AgentFrameDev)" in src
    hdr = open(os.path.join(CSRC, "dw_episode_wave_frames_pw.hpp")).read()
    assert re.search(r"static_assert\(episode_wave_frames_lds_bytes\(kEwMaxCells, 64\) <= 64 \* 1024", hdr)
    staging = open(os.path.join(CSRC, "dw_episode_staging.hpp")).read()
    assert "hip/" not in staging                                 # the split is host-only: no HIP header


# ---- the launch split ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if _rocm_clang() is None:
        pytest.skip("the clang++ of ROCm is not installed")
    tmp = tmp_path_factory.mktemp("episode_frames")
    exe = tmp / "episode_frames_driver"
    subprocess.check_call([_rocm_clang(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CSRC,
                           os.path.join(ROOT, "tests", "episode_frames_driver.cpp"), "-o", str(exe)])
    return json.loads(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout)


def test_agent_frame_record_layout(driver):
    assert driver["record"] == {"size": 16, "row": 0, "col": 4, "state": 8}


def test_the_grid_is_the_one_asked_for(driver):
    combos = [(c["K"], c["stride"], c["ring"]) for c in driver["launches"]]
    assert set(combos) == {(k, s, r) for k in KS for s in STRIDES for r in RINGS} and len(combos) == len(set(combos))


def test_launches_tile_the_call_at_whole_strides_within_the_ring(driver):
    several = 0
    for c in driver["launches"]:
        K, stride, ring, launches = c["K"], c["stride"], c["ring"], c["launches"]
        assert launches, c
        t, f, steps_of_frames = 0, 0, []
        for i, (t0, steps, f0, frames) in enumerate(launches):
            assert t0 == t and f0 == f, c                       # no gap, no overlap: steps and frames continue
            assert steps >= 1 or K == 0, c
            assert t0 % stride == 0, c                          # a launch begins at a whole stride of the call
            if i + 1 < len(launches):
                assert steps % stride == 0, c
            assert frames == steps // stride, c                 # the frames the kernel leaves in that many steps
            if ring:
                assert frames <= ring, c
            steps_of_frames += [t0 + (j + 1) * stride - 1 for j in range(frames)]
            t, f = t + steps, f + frames
        assert t == K and f == K // stride, c
        assert steps_of_frames == [(j + 1) * stride - 1 for j in range(K // stride)], c
        if not ring:
            assert len(launches) == 1, c                        # unlimited capacity, K <= 4096: one launch
        several += len(launches) > 1
    assert several >= 20                                        # the grid does hold calls of several launches


def test_episode_staging_layout_is_unchanged(driver, tmp_path):
    """The split lives beside EpisodeStaging: the existing driver still compiles against the header (its output is held by
    tests/test_episode_staging_cpu.py)."""
    exe = tmp_path / "episode_staging_driver"
    subprocess.check_call([_rocm_clang(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CSRC,
                           os.path.join(ROOT, "tests", "episode_staging_driver.cpp"), "-o", str(exe)])
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip()


# ---- Engine / harness ------------------------------------------------------------------------------------------------------
def test_python_surface_and_shape_checks_without_a_device():
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi, harness
    assert callable(amd.Engine.run_episode_frames)
    assert amd.simulate_grazing_frames is harness.simulate_grazing_frames and "simulate_grazing_frames" in amd.__all__

    class _NoDevice:                                           # any touch of the library is an AttributeError
        B, N = 3, 2
    with pytest.raises(ValueError, match="use_table must have shape"):
        amd.Engine.run_episode_frames(_NoDevice(), np.ones(4), _ffi.POLICY_ARGMAX, np.zeros(3, dtype=np.uint8))
    with pytest.raises(ValueError, match="table must have shape"):
        amd.Engine.run_episode_frames(_NoDevice(), np.ones(4), _ffi.POLICY_TABLE, None, np.zeros((4, 3, 1), dtype=np.int8))


B_, N_, DIM = 3, 2, 8


class _Eng:
    def __init__(self, n_agents):
        self.N, self.calls, self.t, self.on_demand = n_agents, [], 0, []

    def reduce(self):
        from therldaisyworld_amd import _ffi
        s = np.zeros(B_, dtype=_ffi.STATS_DTYPE)
        s["max_k"] = self.t
        return s

    def _frame(self, F, t_of, tile, worlds, temperature, agents):
        from therldaisyworld_amd import _ffi
        th, tw = (tile, tile) if np.isscalar(tile) else tile
        S = B_ if worlds is None else len(worlds)
        shape = (F, S, DIM // th, DIM // tw)
        cov = np.zeros(shape, dtype=_ffi.TILE_COVER_DTYPE)
        cov["sum_light_k"] = np.asarray(t_of).reshape(F, 1, 1, 1)     # a frame is marked with the step it belongs to
        cov["sum_dark_k"] = 7
        tmp = 290.0 + np.zeros(shape) + np.asarray(t_of).reshape(F, 1, 1, 1) if temperature else None
        ag = None
        if agents:
            ag = np.zeros((F, S, self.N), dtype=_ffi.AGENT_FRAME_DTYPE)
            ag["row"], ag["col"] = np.asarray(t_of).reshape(F, 1, 1), np.arange(self.N)
            ag["state"] = 0.5
        return cov, tmp, ag

    def reduce_tiles(self, L, tile=(1, 1), worlds=None, cover=True, temperature=True):
        self.on_demand.append(self.t)
        cov, tmp, _ = self._frame(1, [self.t], tile, worlds, temperature, False)
        return cov[0], None if tmp is None else tmp[0]

    def download_agents(self):
        idx = np.zeros((B_, self.N, 2), dtype=np.int32)
        idx[..., 0], idx[..., 1] = self.t, np.arange(self.N)
        return idx, np.full((B_, self.N), 0.5)

    def run_episode_frames(self, Ls, mode, use_table, table, thr, stride=1, tile=(1, 1), worlds=None, cover=True, temperature=True,
                           agents=True, trace=True, temps=False):
        from therldaisyworld_amd import _ffi
        k = len(Ls)
        self.calls.append(dict(Ls=np.array(Ls), mode=mode, stride=stride, tile=tile, worlds=worlds, cover=cover,
                               temperature=temperature, agents=agents, trace=trace, temps=temps, t0=self.t))
        F = k // stride
        t_of = self.t + (1 + np.arange(F)) * stride               # steps taken once the frame's step is done
        s = np.zeros((k, B_), dtype=_ffi.STATS_DTYPE)
        s["max_k"] = (self.t + 1 + np.arange(k))[:, None]
        self.t += k
        return self._frame(F, t_of, tile, worlds, temperature, agents) + (s, s["max_k"] > thr, np.ones((k, B_, self.N), dtype=bool))


class _Env:
    def __init__(self, n_agents=N_):
        self.batch_size, self.n_agents, self.dim = B_, n_agents, DIM
        self.precision, self.collision_mode = "exact", 0
        self.L, self.dL, self.step_count = 0.9, 0.01, 0
        self.ramp_up_down, self.ramp_period, self.ddL, self.min_L, self.max_L = False, 12, 0.0, 0.5, 1.5
        self.S, self.albedo_bare, self.sigma = 1000.0, 0.5, 5.67e-8
        self._engine, self.actions, self.invalidated = _Eng(n_agents), [], 0

    def update_L(self, L):
        self.step_count += 1
        return max(min(L + self.dL, self.max_L), self.min_L)

    def _invalidate(self):
        self.invalidated += 1

    def step(self, action):
        self.actions.append(action)
        self._engine.t += 1
        self.L = self.update_L(self.L)
        return "obs%d" % self._engine.t, None, np.zeros((B_, self.n_agents, 1), dtype=bool), {}


@pytest.mark.parametrize("n,stride,chunk", [(40, 3, 16), (11, 1, 4), (23, 7, 5), (5, 7, 64), (30, 4, 4)])
def test_simulate_grazing_frames_on_a_fake_engine(n, stride, chunk):
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi, harness
    env = _Env()
    out = harness.simulate_grazing_frames(env, amd.Greedy(epsilon=0.0), n, stride=stride, tile=(2, 4), worlds=[2, 0], chunk=chunk,
                                          obs=np.zeros((B_, N_, 7, 3, 3)))
    calls = env._engine.calls
    F = n // stride
    assert len(env.actions) == 1                                # the first step is the host's
    assert sum(len(c["Ls"]) for c in calls) == n - 1
    # every call starts where the one before it ended; from a whole stride of the run on, a call is a whole number of
    # strides (at most `chunk` steps, at least one stride) unless it ends the run, and takes the run's stride
    rounded = max(chunk // stride * stride, stride)
    for c in calls:
        k, t0 = len(c["Ls"]), c["t0"]
        if t0 % stride:
            assert c is calls[0] and c["stride"] == stride - t0 % stride and k == min(c["stride"], n - t0), c
        else:
            assert c["stride"] == stride and k == min(rounded, n - t0), c
            assert k % stride == 0 or t0 + k == n, c
        assert c["tile"] == (2, 4) and c["worlds"] == [2, 0] and c["cover"] and c["temperature"] and c["agents"] and c["trace"]
        assert not c["temps"] and c["mode"] == _ffi.POLICY_ARGMAX
    L_used = np.concatenate([[0.9], *[c["Ls"] for c in calls]])
    assert np.array_equal(out["L"], L_used) and np.allclose(np.diff(L_used), 0.01, rtol=0, atol=1e-12)
    assert set(out) == {"L", "mean_light", "mean_dark", "max_cover", "alive", "stats", "agent_ok", "agents_alive", "frame_steps",
                        "frame_L", "light", "dark", "cover", "worlds", "temp", "frame_dead_temp", "agent_pos", "agent_state"}
    assert np.array_equal(out["stats"]["max_k"][:, 0], np.arange(1, n + 1)) and out["agent_ok"].shape == (n, B_, N_)
    # frame f belongs to step (f + 1) * stride - 1 of the run: the fake marks every frame with the steps taken by then
    want = stride * (1 + np.arange(F))
    assert np.array_equal(out["frame_steps"], want)
    assert np.array_equal(out["frame_L"], L_used[stride - 1::stride][:F])
    assert np.array_equal(out["worlds"], [2, 0])
    assert env._engine.on_demand == ([1] if stride == 1 else [])
    if F:
        for key in ("light", "dark", "cover", "temp"):
            assert out[key].shape == (F, 2, 4, 2), key
        assert np.array_equal(out["cover"]["sum_light_k"][:, 0, 0, 0], want)
        assert np.array_equal(out["light"], out["cover"]["sum_light_k"] / 1000.0 / 8)   # fractions of the tile's cells
        assert np.array_equal(out["dark"], out["cover"]["sum_dark_k"] / 1000.0 / 8)
        assert np.array_equal(out["temp"][:, 0, 0, 0], 290.0 + want)
        assert out["agent_pos"].shape == (F, 2, N_, 2) and out["agent_state"].shape == (F, 2, N_)
        assert np.array_equal(out["agent_pos"][:, 0, :, 0], np.tile(want[:, None], (1, N_)))
        assert np.array_equal(out["agent_pos"][0, 0, :, 1], np.arange(N_)) and np.all(out["agent_state"] == 0.5)
        assert np.array_equal(out["frame_dead_temp"], harness.dead_temperature(env, out["frame_L"]))
    assert env.step_count == n


def test_an_agent_free_environment_is_served_without_agent_frames():
    from therldaisyworld_amd import harness
    env = _Env(n_agents=0)
    out = harness.simulate_grazing_frames(env, None, 9, stride=2, tile=1, temperature=False, chunk=4, obs="obs0")
    assert "agent_pos" not in out and "agent_state" not in out and "temp" not in out
    assert all(not c["agents"] and not c["temperature"] for c in env._engine.calls)
    assert out["light"].shape == (4, B_, DIM, DIM) and np.array_equal(out["frame_steps"], [2, 4, 6, 8])


def test_simulate_grazing_is_unchanged_by_the_shared_loop():
    """simulate_grazing goes through the same loop with no frames: it never touches run_episode_frames or reduce_tiles."""
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi, harness

    class Eng(_Eng):
        def run_episode_trace(self, Ls, mode, use_table, table, thr):
            k = len(Ls)
            self.calls.append(k)
            s = np.zeros((k, B_), dtype=_ffi.STATS_DTYPE)
            self.t += k
            return s, s["max_k"] > thr, np.ones((k, B_, N_), dtype=bool)

        def run_episode_frames(self, *a, **k):
            raise AssertionError("simulate_grazing took the frames call")

    env = _Env()
    env._engine = Eng(N_)
    out = harness.simulate_grazing(env, amd.Greedy(epsilon=0.0), 11, chunk=4, obs=np.zeros((B_, N_, 7, 3, 3)))
    assert env._engine.calls == [4, 4, 2] and not env._engine.on_demand
    assert "frame_steps" not in out and "cover" not in out
