"""CPU-side tests (no GPU) of dw_run_episode_mlp_trace, Engine.run_episode_mlp(trace=, temperature=) and
harness.simulate_grazing_mlp:

  * the symbol is declared in the header, exported by the library and bound by _ffi with the declared argument list; the
    ABI number is still 6; a null handle is refused;
  * Engine.run_episode_mlp with its defaults makes the call it has always made and returns its pair; with `trace` /
    `temperature` the new call with the arrays asked for (a stub library object, no device);
  * simulate_grazing_mlp on a stand-in environment: the chunking, `params=None` after the first chunk, the split values,
    the dict's keys and shapes, and what it refuses before any device call;
  * the staging layout of the call (tests/episode_mlp_trace_staging_driver.cpp, host C++17): TRACE behind DONE, the
    temperature rows 8-byte aligned, the layout of dw_run_episode_mlp itself unchanged.
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
    return [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_int32),
            C.POINTER(C.c_int32), C.c_int32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_uint8),
            C.POINTER(_ffi.DwWorldStats), C.POINTER(_ffi.DwTempStats)]


def test_symbol_is_declared_exported_and_bound():
    from therldaisyworld_amd import _ffi
    header = open(os.path.join(ROOT, "include", "daisyworld_hip.h")).read()
    m = re.search(r"\bint dw_run_episode_mlp_trace\(([^;]*)\);", header)
    assert m, "dw_run_episode_mlp_trace is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    assert len(args) == 13 == len(_ffi.SIGNATURES["dw_run_episode_mlp_trace"][1])
    assert "double* reward" in args[9] and "uint8_t* done" in args[10]
    assert "dw_world_stats* trace" in args[11] and "dw_temp_stats* temps" in args[12]
    # ... the arguments of dw_run_episode_mlp, then the two record arrays
    old = re.search(r"\bint dw_run_episode_mlp\(([^;]*)\);", header)
    old_args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", old.group(1), flags=re.S).split(",")]
    assert [a.strip() for a in args[:11]] == old_args
    assert _ffi.SIGNATURES["dw_run_episode_mlp_trace"][1][:11] == _ffi.SIGNATURES["dw_run_episode_mlp"][1]
    assert re.search(r"#define DW_ABI_VERSION 6\b", header) and _ffi.DW_ABI_VERSION == 6
    assert '"; mlp trace: ..."' in header and "notebook_helpers.py:210-223" in header
    lib = _ffi.load()
    assert lib.dw_abi_version() == 6
    assert lib.dw_run_episode_mlp_trace.argtypes == _new_argtypes(_ffi)
    Ls = np.ones(4)
    stats = np.zeros((4, 1), dtype=_ffi.STATS_DTYPE)
    rc = lib.dw_run_episode_mlp_trace(None, 4, _ffi.ptr_d(Ls), None, 1, None, None, 0, 0.75, None, None,
                                      stats.ctypes.data_as(C.POINTER(_ffi.DwWorldStats)), None)
    assert rc == _ffi.DW_EINVAL and b"null" in lib.dw_last_error()
    assert not stats.view(np.uint8).any()


def test_kernel_info_names_the_form_from_the_mlp_predicate():
    src = open(os.path.join(CSRC, "dw_api.hip")).read()
    assert re.search(r'"; mlp trace: %s", episode_mlp_form\(h\) == EPISODE_WAVE \? "one wave per world" : "launches per step"', src)
    # the existing fragments, byte for byte
    for frag in ('"; episode: %s; mlp episode: %s"', '"; ensemble episode: %s"', '"; episode trace: %s"',
                 '"; episode temperature: %s"', '"; ensemble trace: %s"', '"; per-world constants: %s"'):
        assert frag in src, frag
    assert src.index('"; ensemble trace: %s"') < src.index('"; mlp trace: %s"') < src.index('"; per-world constants: %s"')


class _StubLib:
    """Records the calls Engine.run_episode_mlp makes; fills what a call would write with recognisable values."""

    def __init__(self):
        self.calls = []

    def dw_run_episode_mlp(self, *args):
        self.calls.append(("dw_run_episode_mlp", args))
        return 0

    def dw_run_episode_mlp_trace(self, *args):
        self.calls.append(("dw_run_episode_mlp_trace", args))
        K = args[1]
        if args[11]:
            for i in range(K * 3):
                args[11][i].max_k = 7
        if args[12]:
            for i in range(K * 3):
                args[12][i].mean = 295.0
        return 0


def _stub_engine():
    import therldaisyworld_amd as amd

    class _Stub:
        B, N = 3, 2
        _h = C.c_void_p(1)
        run_episode_mlp = amd.Engine.run_episode_mlp

        def _check(self, rc):
            assert rc == 0
    eng = _Stub()
    eng._lib = _StubLib()
    return eng


def test_engine_makes_todays_call_unless_records_are_asked_for():
    from therldaisyworld_amd import _ffi
    K = 4
    Ls = np.ones(K)
    w = np.zeros((2, 1808))
    ma, mb = np.zeros(3, dtype=np.int32), np.ones(3, dtype=np.int32)
    eng = _stub_engine()
    out = eng.run_episode_mlp(Ls, w, ma, mb)
    (name, args), = eng._lib.calls
    assert name == "dw_run_episode_mlp" and len(args) == 11 and args[1] == K and args[4] == 2 and args[7] == 1 and args[8] == 0.75
    assert len(out) == 2 and out[0].shape == (K, 3, 2, 1) and out[1].shape == (K, 3, 2, 1) and out[1].dtype == np.bool_
    assert len(eng.run_episode_mlp(Ls, w, ma, mb, trace=False, temperature=False)) == 2
    assert [c[0] for c in eng._lib.calls] == ["dw_run_episode_mlp"] * 2

    for trace, temperature in ((True, True), (True, False), (False, True)):
        eng = _stub_engine()
        reward, done, stats, temps = eng.run_episode_mlp(Ls, w, ma, mb, 2, 0.8, trace=trace, temperature=temperature)
        (name, args), = eng._lib.calls
        assert name == "dw_run_episode_mlp_trace" and len(args) == 13 and args[:2] == (eng._h, K)
        assert args[4] == 2 and args[7] == 2 and args[8] == 0.8
        assert reward.shape == (K, 3, 2, 1) and done.shape == (K, 3, 2, 1) and done.dtype == np.bool_
        if trace:
            assert stats.dtype == _ffi.STATS_DTYPE and stats.shape == (K, 3) and (stats["max_k"] == 7).all()
        else:
            assert stats is None and args[11] is None
        if temperature:
            assert temps.dtype == _ffi.TEMP_STATS_DTYPE and temps.shape == (K, 3) and (temps["mean"] == 295.0).all()
        else:
            assert temps is None and args[12] is None
    eng = _stub_engine()                                        # params=None: the sets of an earlier call
    eng.run_episode_mlp(Ls, None, ma, mb, n_members=2, trace=True)
    (name, args), = eng._lib.calls
    assert name == "dw_run_episode_mlp_trace" and args[3] is None and args[4] == 2
    with pytest.raises(ValueError, match="n_members"):
        eng.run_episode_mlp(Ls, None, ma, mb, trace=True)
    with pytest.raises(ValueError, match="member maps"):
        eng.run_episode_mlp(Ls, w, ma[:2], mb, trace=True)
    assert len(eng._lib.calls) == 1


# ---- simulate_grazing_mlp on a stand-in environment -----------------------------------------------------------------------
B_, N_, DIM = 3, 4, 8


class _Eng:
    def __init__(self):
        self.calls, self.t = [], 0

    def run_episode_mlp(self, Ls, params, member_a, member_b, split, L_init, n_members=None, trace=False, temperature=False):
        from therldaisyworld_amd import _ffi
        k = len(Ls)
        self.calls.append(dict(Ls=np.array(Ls), params=None if params is None else np.array(params), member_a=member_a,
                               member_b=member_b, split=split, L_init=L_init, n_members=n_members, trace=trace,
                               temperature=temperature))
        steps = (self.t + 1 + np.arange(k))
        s = np.zeros((k, B_), dtype=_ffi.STATS_DTYPE)
        s["max_k"], s["sum_light_k"], s["sum_dark_k"] = steps[:, None], 64 * steps[:, None], steps[:, None]
        tp = np.zeros((k, B_), dtype=_ffi.TEMP_STATS_DTYPE)
        tp["mean"] = 290.0 + steps[:, None]
        reward = np.broadcast_to(steps[:, None, None, None] / 1000.0, (k, B_, N_, 1)).copy()
        done = np.zeros((k, B_, N_, 1), dtype=bool)
        done[:, 0, 1] = True
        self.t += k
        return reward, done, (s if trace else None), (tp if temperature else None)


class _Env:
    def __init__(self, **over):
        self.batch_size, self.n_agents, self.dim = B_, N_, DIM
        self.precision, self.collision_mode = "exact", 0
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


class _Mlp:
    def __init__(self, v):
        self.v = v

    def get_parameters(self):
        return np.full(1808, self.v)


def test_simulate_grazing_mlp_chunks_params_and_split():
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi, harness
    assert amd.simulate_grazing_mlp is harness.simulate_grazing_mlp and "simulate_grazing_mlp" in amd.__all__
    n = 11
    env = _Env()
    out = harness.simulate_grazing_mlp(env, _Mlp(1.0), n, adversary=_Mlp(2.0), chunk=4, obs="obs0", temperature=True)
    calls = env._engine.calls
    assert [len(c["Ls"]) for c in calls] == [4, 4, 3] and env.resets == 0 and env.synced >= 1
    assert calls[0]["params"].shape == (2, 1808) and (calls[0]["params"][0] == 1.0).all() and (calls[0]["params"][1] == 2.0).all()
    assert all(c["params"] is None for c in calls[1:]) and all(c["n_members"] == 2 for c in calls)
    assert all(c["split"] == N_ // 2 and c["trace"] and c["temperature"] for c in calls)
    assert all(np.array_equal(c["member_a"], np.zeros(B_)) and np.array_equal(c["member_b"], np.ones(B_)) for c in calls)
    L_used = np.concatenate([c["Ls"] for c in calls])
    assert np.array_equal(out["L"], L_used) and L_used[0] == 0.9 and np.allclose(np.diff(L_used), 0.01, rtol=0, atol=1e-12)
    # the observations' luminosity: that of the last pass - the reset's, then the last step of the chunk before
    assert [c["L_init"] for c in calls] == [0.9, L_used[3], L_used[7]]
    assert env.step_count == n and env.invalidated >= 3 and env._L_pass == L_used[-1]
    assert set(out) == {"L", "mean_light", "mean_dark", "max_cover", "alive", "stats", "agent_ok", "agents_alive", "reward",
                        "mean_temp", "std_temp", "min_temp", "max_temp", "dead_temp"}
    assert out["stats"].shape == (n, B_) and out["stats"].dtype == _ffi.STATS_DTYPE
    assert np.array_equal(out["stats"]["max_k"][:, 0], np.arange(1, n + 1))
    assert np.array_equal(out["mean_light"], out["stats"]["sum_light_k"] / 1000.0 / (DIM * DIM))
    assert out["reward"].shape == (n, B_, N_) and np.array_equal(out["reward"][:, 0, 0], np.arange(1, n + 1) / 1000.0)
    assert out["agent_ok"].shape == (n, B_, N_) and out["agent_ok"].dtype == np.bool_
    assert not out["agent_ok"][:, 0, 1].any() and out["agent_ok"][:, 1:].all()
    assert np.array_equal(out["agents_alive"], np.tile([N_ - 1, N_, N_], (n, 1)))
    assert out["mean_temp"].shape == (n, B_) and np.array_equal(out["mean_temp"][:, 1], 290.0 + np.arange(1, n + 1))
    assert out["dead_temp"].shape == (n,)
    assert np.array_equal(out["alive"], out["stats"]["max_k"] > 5)

    # no adversary: `agent` drives every agent, one parameter set, no member maps; cover records only; obs=None resets
    env = _Env()
    out = harness.simulate_grazing_mlp(env, _Mlp(3.0), 5, chunk=64)
    (c,) = env._engine.calls
    assert env.resets == 1 and len(c["Ls"]) == 5 and c["split"] == N_ and c["n_members"] == 1
    assert c["params"].shape == (1, 1808) and c["member_a"] is None and c["member_b"] is None
    assert c["trace"] and not c["temperature"]
    assert set(out) == {"L", "mean_light", "mean_dark", "max_cover", "alive", "stats", "agent_ok", "agents_alive", "reward"}


def test_simulate_grazing_mlp_refuses_before_any_device_call():
    from therldaisyworld_amd import harness
    env = _Env()
    with pytest.raises(ValueError, match="nsteps"):
        harness.simulate_grazing_mlp(env, _Mlp(1.0), 0, obs=True)
    with pytest.raises(ValueError, match="chunk"):
        harness.simulate_grazing_mlp(env, _Mlp(1.0), 3, chunk=0, obs=True)
    for over in ({"precision": "f64"}, {"collision_mode": 1}):
        bad = _Env(**over)
        with pytest.raises(ValueError, match=r"simulate_grazing with a callable"):
            harness.simulate_grazing_mlp(bad, _Mlp(1.0), 3, obs=True)
        assert not bad._engine.calls and not bad.synced and not bad.resets
    assert not env._engine.calls and not env.synced


def test_simulate_grazing_is_untouched_by_the_sibling():
    """simulate_grazing still sends a callable that is no Greedy to the host loop."""
    from therldaisyworld_amd import harness
    assert harness._policy_mode(_Mlp(1.0)) is None


# ---- the staging layout -----------------------------------------------------------------------------------------------
STATS, ROW, P32 = 24, 32, 128
ORDER = ["member_a", "member_b", "reward", "done", "p32", "ls", "p64", "use_table", "table", "world_alive", "agent_ok", "trace",
         "code", "pair_stats"]


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    if _rocm_clang() is None:
        pytest.skip("the clang++ of ROCm is not installed")
    exe = tmp_path_factory.mktemp("episode_mlp_trace_staging") / "episode_mlp_trace_staging_driver"
    subprocess.check_call([_rocm_clang(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CSRC,
                           os.path.join(ROOT, "tests", "episode_mlp_trace_staging_driver.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True)
    return json.loads(out.stdout)


def _up(v):
    return (v + 255) // 256 * 256


def test_records_sit_behind_done_and_the_mlp_layout_stays(driver_output):
    assert driver_output["sizes"] == {"StatsDev": STATS, "temp_row": ROW, "PhysF32": P32}
    cases = driver_output["cases"]
    assert len(cases) == 15
    for mlp, trace, temps in zip(cases[0::3], cases[1::3], cases[2::3]):
        assert (mlp["form"], trace["form"], temps["form"]) == ("mlp", "trace", "temps")
        K, B, N = mlp["K"], mlp["B"], mlp["N"]
        what = (K, B, N)
        # the layout of dw_run_episode_mlp, restated: member maps, reward, done, the rows of the steps; nothing else
        want, o = [], 0
        sizes = {"member_a": 4 * B, "member_b": 4 * B, "reward": 8 * K * B * N, "done": K * B * N, "p32": P32 * K, "ls": 8 * K}
        for name in ORDER:
            want.append([name, o, sizes.get(name, 0)])
            o = _up(o + sizes.get(name, 0))
        assert mlp["regions"] == want and mlp["total"] == o, what
        assert mlp["stats_bytes"] == 0 and mlp["temps_bytes"] == 0
        base = {r[0]: r for r in mlp["regions"]}
        for c in (trace, temps):
            by = {r[0]: r for r in c["regions"]}
            assert [r[0] for r in c["regions"]] == ORDER
            for name in ORDER[:ORDER.index("trace")]:                 # everything in front of the records: where it was
                assert by[name] == base[name], (what, c["form"], name)
            assert by["table"][2] == by["world_alive"][2] == by["agent_ok"][2] == by["use_table"][2] == 0, what
            assert by["trace"][1] % 256 == 0 and by["trace"][1] >= by["done"][1] + by["done"][2], what
            assert by["trace"][1] >= by["ls"][1] + by["ls"][2], what
            assert c["stats_bytes"] == STATS * K * B, what
            assert c["temps_bytes"] == (ROW * K * B if c["form"] == "temps" else 0), what
            assert by["trace"][2] == c["stats_bytes"] + c["temps_bytes"], what
            assert c["temps_off"] == by["trace"][1] + c["stats_bytes"] and c["temps_off"] % 8 == 0, what
            assert c["total"] == _up(by["trace"][1] + by["trace"][2]), what
