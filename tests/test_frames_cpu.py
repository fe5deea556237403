"""CPU-side tests (no GPU) of the spatial frames: dw_reduce_tiles, dw_step_n_frames, Engine.reduce_tiles /
step_n_frames and harness.simulate_frames.

  * the frame rule of plan_series (csrc/dw_series.hpp), printed by tests/frames_driver.cpp over nsteps x stride x pairs
    allowed x quantised start x temperature frames: no frame step is inside a pair; every stretch of steps between frames
    pairs exactly as the same spec without frames pairs a run of that length (a stretch that begins the run: with the
    spec's own "quantised"; a later one: from a quantised state, which any step leaves); the plan does not depend on whether
    temperature frames are wanted; with the new members at their defaults the existing grid plans as before;
  * both symbols are declared, exported and bound; the two structs have the stated layout; null arguments are refused;
  * simulate_frames against a fake engine: the schedule passed, the shapes and keys, the host scalars, the refusal of agents.
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from test_plan_cpu import CSRC, ROOT, _rocm_clang
from test_series_cpu import _expected

NSTEPS = (1, 2, 3, 4, 5, 7, 8, 11, 13)
STRIDES = (1, 2, 3, 4, 5)


def _run(tmp, name):
    exe = tmp / name
    subprocess.check_call([_rocm_clang(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CSRC,
                           os.path.join(ROOT, "tests", name + ".cpp"), "-o", str(exe)])
    return json.loads(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout)


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    if _rocm_clang() is None:
        pytest.skip("the clang++ of ROCm is not installed")
    return tmp_path_factory.mktemp("frames")


@pytest.fixture(scope="module")
def plans(build_dir):
    return _run(build_dir, "frames_driver")


# ---- plan_series ---------------------------------------------------------------------------------------------------------
def test_the_grid_is_the_one_asked_for(plans):
    combos = {(c["nsteps"], c["stride"], c["may_pair"], c["quantised"], c["frame_temps"]) for c in plans["frames"]}
    assert combos == {(n, s, p, q, t) for n in NSTEPS for s in STRIDES for p in (0, 1) for q in (0, 1) for t in (0, 1)}
    assert len(plans["frames"]) == len(combos)


def test_frame_steps_are_marked_and_never_inside_a_pair(plans):
    for c in plans["frames"]:
        n, stride, is_pair, is_frame = c["nsteps"], c["stride"], c["is_pair"], c["is_frame"]
        assert is_frame == [int((t + 1) % stride == 0) for t in range(n)], c
        assert c["nframes"] == n // stride == sum(is_frame), c
        assert c["plan_frame_temps"] == c["frame_temps"], c
        taken, t = [0] * n, 0
        while t < n:                                            # every step is taken exactly once
            for i in range(is_pair[t] + 1):
                taken[t + i] += 1
            t += is_pair[t] + 1
        assert taken == [1] * n and t == n, c
        for t in range(n):
            if is_frame[t]:                                     # neither half of a pair
                assert not is_pair[t] and not (t and is_pair[t - 1]), (t, c)
        if not c["may_pair"]:
            assert not any(is_pair), c
        assert c["quantised"] or not is_pair[0], c


def test_stretches_between_frames_pair_as_a_run_of_their_length(plans):
    plain = {(c["nsteps"], c["may_pair"], c["quantised"]): c["is_pair"] for c in plans["plain"]}
    assert all(c["nframes"] == 0 and not any(c["is_frame"]) for c in plans["plain"])
    stretches = paired = 0
    for c in plans["frames"]:
        n, is_pair, is_frame = c["nsteps"], c["is_pair"], c["is_frame"]
        t = 0
        while t < n:
            if is_frame[t]:
                t += 1
                continue
            end = t
            while end < n and not is_frame[end]:
                end += 1
            want = plain[(end - t, c["may_pair"], c["quantised"] if t == 0 else 1)]
            assert is_pair[t:end] == want, (t, end, c)
            stretches += 1
            paired += sum(want)
            t = end
    assert stretches > 500 and paired >= 50                     # the grid does hold stretches that pair


def test_the_plan_does_not_depend_on_temperature_frames(plans):
    by = {}
    for c in plans["frames"]:
        key = (c["nsteps"], c["stride"], c["may_pair"], c["quantised"])
        by.setdefault(key, []).append((c["is_pair"], c["is_frame"], c["rows"], c["npairs"]))
    assert all(len(v) == 2 and v[0] == v[1] for v in by.values())


def test_defaults_reproduce_the_existing_plans(plans, build_dir):
    """The shared-luminosity cases of tests/series_driver.cpp's grid: the rules of test_series_cpu restated (its _expected),
    and the existing driver itself - which fills the struct member by member - compiled against this header."""
    assert len(plans["defaults"]) == 8 * 5 * 2 * 2 * 2
    for c in plans["defaults"]:
        assert c["nframes"] == 0
        for key, value in _expected(c).items():
            assert c[key] == value, (key, c)
    existing = [c for c in _run(build_dir, "series_driver")["schedules"] if c["form"] != "table"]
    mine = {(c["form"], c["nsteps"], c["trace_rows"], c["may_pair"], c["quantised"], c["temps"]): c for c in plans["defaults"]}
    assert len(existing) == len(plans["defaults"])
    for c in existing:
        d = mine[(c["form"], c["nsteps"], c["trace_rows"], c["may_pair"], c["quantised"], c["temps"])]
        assert all(c[k] == d[k] for k in c), (c, d)


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    from therldaisyworld_amd import _ffi
    header = open(os.path.join(ROOT, "include", "daisyworld_hip.h")).read()
    assert re.search(r"\bint dw_reduce_tiles\(dw_handle\* h, double L, const dw_frame_spec\* spec,\s*dw_tile_cover\* cover[^;]*?,"
                     r"\s*double\* temp_mean[^;]*?\);", header)
    assert re.search(r"\bint dw_step_n_frames\(dw_handle\* h, int32_t nsteps, const double\* L_schedule[^;]*?, const dw_frame_spec\* spec,"
                     r"\s*int32_t stride, dw_tile_cover\* cover[^;]*?,\s*double\* temp_mean[^;]*?, dw_world_stats\* trace[^;]*?\);", header)
    assert re.search(r"typedef struct dw_tile_cover \{ uint32_t sum_light_k, sum_dark_k; \} dw_tile_cover;", header)
    assert re.search(r"typedef struct dw_frame_spec \{\s*int32_t tile_h, tile_w;[^}]*int32_t n_worlds;[^}]*const int32_t\* worlds;[^}]*\} "
                     r"dw_frame_spec;", header)
    declared = int(re.search(r"#define DW_ABI_VERSION (\d+)\b", header).group(1))
    lib = _ffi.load()
    assert declared == _ffi.DW_ABI_VERSION == lib.dw_abi_version() == 6
    assert lib.dw_reduce_tiles.argtypes == [C.c_void_p, C.c_double, C.POINTER(_ffi.DwFrameSpec), C.POINTER(_ffi.DwTileCover),
                                            C.POINTER(C.c_double)]
    assert lib.dw_step_n_frames.argtypes == [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(_ffi.DwFrameSpec), C.c_int32,
                                             C.POINTER(_ffi.DwTileCover), C.POINTER(C.c_double), C.POINTER(_ffi.DwWorldStats)]
    # layouts: 8-byte records; the spec is three int32 and, after four bytes of padding, a pointer
    assert C.sizeof(_ffi.DwTileCover) == 8 == _ffi.TILE_COVER_DTYPE.itemsize
    assert _ffi.TILE_COVER_DTYPE.names == ("sum_light_k", "sum_dark_k")
    assert [(n, getattr(_ffi.DwFrameSpec, n).offset) for n, _ in _ffi.DwFrameSpec._fields_] == \
        [("tile_h", 0), ("tile_w", 4), ("n_worlds", 8), ("worlds", 16)]
    assert C.sizeof(_ffi.DwFrameSpec) == 24
    # null arguments are refused before anything else
    spec = _ffi.DwFrameSpec(1, 1, 0, None)
    Ls, tm = np.ones(4), np.zeros(4)
    assert lib.dw_reduce_tiles(None, 1.0, C.byref(spec), None, _ffi.ptr_d(tm)) == _ffi.DW_EINVAL and b"null" in lib.dw_last_error()
    assert lib.dw_step_n_frames(None, 4, _ffi.ptr_d(Ls), C.byref(spec), 1, None, _ffi.ptr_d(tm), None) == _ffi.DW_EINVAL
    assert b"null" in lib.dw_last_error()


def test_the_library_checks_the_record_layout():
    src = open(os.path.join(CSRC, "dw_api.hip")).read()
    assert "static_assert(sizeof(dw_tile_cover) == 8 && sizeof(dw_tile_cover) == sizeof(TileCoverDev)" in src


# ---- simulate_frames ---------------------------------------------------------------------------------------------------------
B_, DIM = 3, 8


class _Eng:
    def __init__(self):
        self.calls = []

    def step_n_frames(self, L_schedule, stride=1, tile=(1, 1), worlds=None, cover=True, temperature=True, trace=True):
        from therldaisyworld_amd import _ffi
        Ls = np.array(L_schedule)
        self.calls.append(dict(Ls=Ls, stride=stride, tile=tile, worlds=worlds, cover=cover, temperature=temperature, trace=trace))
        th, tw = (tile, tile) if np.isscalar(tile) else tile
        n, F, S = len(Ls), len(Ls) // stride, B_ if worlds is None else len(worlds)
        shape = (F, S, DIM // th, DIM // tw)
        cov = np.zeros(shape, dtype=_ffi.TILE_COVER_DTYPE)
        cov["sum_light_k"] = np.arange(np.prod(shape)).reshape(shape) % (1000 * th * tw)
        cov["sum_dark_k"] = 7
        tmp = 290.0 + np.arange(np.prod(shape), dtype=np.float64).reshape(shape)
        s = np.zeros((n, B_), dtype=_ffi.STATS_DTYPE)
        s["max_k"], s["sum_light_k"] = 1 + np.arange(n)[:, None], 64 * np.arange(n)[:, None]
        return (cov if cover else None), (tmp if temperature else None), (s if trace else None)


class _Env:
    def __init__(self, **over):
        self.batch_size, self.n_agents, self.dim = B_, 0, DIM
        self.L, self.dL, self.step_count, self._L_pass = 0.9, 0.01, 0, 0.9
        self.ramp_up_down, self.ramp_period, self.ddL, self.min_L, self.max_L = False, 12, 0.0, 0.5, 1.5
        self.S, self.albedo_bare, self.sigma = 1000.0, 0.5, 5.67e-8
        self._engine, self.invalidated, self.synced, self.resets = _Eng(), 0, 0, 0
        vars(self).update(over)

    def update_L(self, L):
        self.step_count += 1
        return max(min(L + self.dL, self.max_L), self.min_L)

    def _invalidate(self):
        self.invalidated += 1

    def _ensure_engine(self):
        return self._engine

    def _sync_to_device(self):
        self.synced += 1

    def reset(self):
        self.resets += 1
        return "obs"


def test_simulate_frames_on_a_fake_engine():
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi, harness
    assert amd.simulate_frames is harness.simulate_frames and "simulate_frames" in amd.__all__
    assert callable(amd.Engine.reduce_tiles) and callable(amd.Engine.step_n_frames)
    n, stride = 11, 3
    env = _Env(step_count=5)
    out = harness.simulate_frames(env, n, stride=stride, tile=(2, 4), worlds=[2, 0])
    (call,) = env._engine.calls                                 # ONE device call
    assert env.resets == 1 and env.synced == 1
    assert call["stride"] == stride and call["tile"] == (2, 4) and call["worlds"] == [2, 0]
    assert call["cover"] and call["temperature"] and call["trace"]
    assert call["Ls"][0] == 0.9 and np.allclose(np.diff(call["Ls"]), 0.01, rtol=0, atol=1e-12) and len(call["Ls"]) == n
    assert np.array_equal(out["L"], call["Ls"])
    assert set(out) == {"L", "mean_light", "mean_dark", "max_cover", "alive", "stats", "frame_steps", "frame_L", "light", "dark",
                        "cover", "worlds", "temp", "frame_dead_temp"}
    F = n // stride
    assert out["stats"].shape == (n, B_) and out["mean_light"].shape == (n, B_)
    assert np.array_equal(out["mean_light"], out["stats"]["sum_light_k"] / 1000.0 / (DIM * DIM))
    for key in ("light", "dark", "cover", "temp"):
        assert out[key].shape == (F, 2, 4, 2), key
    assert out["cover"].dtype == _ffi.TILE_COVER_DTYPE
    assert np.array_equal(out["light"], out["cover"]["sum_light_k"] / 1000.0 / 8)
    assert np.array_equal(out["dark"], out["cover"]["sum_dark_k"] / 1000.0 / 8)
    assert np.array_equal(out["worlds"], [2, 0])
    # frame f belongs to step (f + 1) * stride - 1 of the run; the environment had taken five steps before it
    assert np.array_equal(out["frame_steps"], 5 + stride * (1 + np.arange(F)))
    assert np.array_equal(out["frame_L"], call["Ls"][stride - 1::stride][:F])
    assert np.array_equal(out["frame_dead_temp"], harness.dead_temperature(env, out["frame_L"]))
    # the host scalars advanced by all n steps, the trailing ones without a frame included
    assert env.step_count == 5 + n and env.invalidated >= 1 and env._L_pass == call["Ls"][-1]
    assert env.L == pytest.approx(0.9 + 0.01 * n, rel=0, abs=1e-12)

    # an int tile, all worlds, no temperature, the caller's own reset
    env = _Env()
    out = harness.simulate_frames(env, 4, stride=1, tile=1, temperature=False, obs="obs0")
    (call,) = env._engine.calls
    assert env.resets == 0 and not call["temperature"] and call["worlds"] is None
    assert "temp" not in out and "frame_dead_temp" not in out
    assert out["light"].shape == (4, B_, DIM, DIM) and np.array_equal(out["worlds"], np.arange(B_))
    assert np.array_equal(out["light"], out["cover"]["sum_light_k"] / 1000.0)
    assert np.array_equal(out["frame_steps"], 1 + np.arange(4))


def test_simulate_frames_refuses_agents():
    from therldaisyworld_amd import harness
    env = _Env(n_agents=2)
    with pytest.raises(ValueError, match="agent-free.*reduce_tiles"):
        harness.simulate_frames(env, 5, obs=True)
    assert not env._engine.calls and env.resets == 0
