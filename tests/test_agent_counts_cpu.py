"""CPU-side tests (no GPU) of dw_run_episode_mlp_counts, harness.simulate_agent_count_sweep and the `"n_agents"` scenarios of
simulate_lifespan_sweep:

  * the symbol is declared in the header, exported, bound with the declared argument list and reachable from `Engine`; the
    ABI version is still 6; a null handle and a null `n_active` are refused; the harnesses refuse what they document;
  * the three rules of the call - an absent agent has state 0, leaves no stamp in channel 4 and observes all-zero rows - make
    an N-agent world equal to a world of k agents: on the NumPy oracle, step by step, under an MLP and both greedy policies;
    and the weaker claim the `"n_agents"` scenarios rest on (plainly zeroed states, ordinary stamps, policies that read
    channels 1 and 2 only);
  * the form decision (csrc/dw_counts_plan.hpp, a header without HIP): tests/counts_plan_driver.cpp against a Python
    restatement, built with the clang++ of ROCm and once more with -fsanitize=address,undefined as a stand-alone program;
  * the gfx950 code of the new kernels (one compilation of csrc/dw_api.hip with --save-temps, as the test_isa_* files): they
    exist in every instantiation, carry `_pw`, use no scratch memory, make no calls, and the workgroup kernel's static LDS is
    what the header states.
"""
import ctypes as C
import inspect
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

from oracle import daisy_oracle as O  # noqa: E402


# ---- symbol and refusals ---------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_bound_and_reachable():
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi, harness
    header = open(os.path.join(ROOT, "include", "daisyworld_hip.h")).read()
    assert re.search(r"#define DW_ABI_VERSION 6\b", header) and _ffi.DW_ABI_VERSION == 6
    assert re.search(r"\bint dw_run_episode_mlp_counts\(dw_handle\* h, int32_t nsteps, const double\* L_schedule, const double\* "
                     r"params[^;,]*,\s*int32_t n_members, const int32_t\* member_a[^;,]*, const int32_t\* member_b[^;,]*,\s*"
                     r"int32_t split, const int32_t\* n_active[^;]*, double L_init,\s*double\* reward[^;]*, uint8_t\* done[^;]*,\s*"
                     r"dw_world_stats\* trace[^;]*\);", header)
    assert "fd8ad489" in header and "227e4895" in header     # the notebook cells the call serves
    assert "dw_get_obs sees them as dead agents" in header   # the counts are not a property of the handle
    lib = _ffi.load()
    assert lib.dw_abi_version() == 6
    assert lib.dw_run_episode_mlp_counts.argtypes == _ffi.SIGNATURES["dw_run_episode_mlp_counts"][1] == [
        C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
        C.c_int32, C.POINTER(C.c_int32), C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(_ffi.DwWorldStats)]
    Ls, na = np.ones(4), np.zeros(1, dtype=np.int32)
    rc = lib.dw_run_episode_mlp_counts(None, 4, _ffi.ptr_d(Ls), None, 1, None, None, 0, _ffi.ptr_i(na), 0.75, None, None, None)
    assert rc == _ffi.DW_EINVAL and b"null" in lib.dw_last_error()
    rc = lib.dw_run_episode_mlp_counts(None, 4, _ffi.ptr_d(Ls), None, 1, None, None, 0, None, 0.75, None, None, None)
    assert rc == _ffi.DW_EINVAL and b"n_active" in lib.dw_last_error()
    sig = inspect.signature(amd.Engine.run_episode_mlp_counts)
    assert list(sig.parameters)[1:] == ["L_schedule", "params", "n_active", "member_a", "member_b", "split", "L_init", "n_members",
                                        "trace"]
    assert sig.parameters["trace"].default is True and sig.parameters["L_init"].default == 0.75
    assert amd.simulate_agent_count_sweep is harness.simulate_agent_count_sweep and "simulate_agent_count_sweep" in amd.__all__
    sig = inspect.signature(harness.simulate_agent_count_sweep)
    assert list(sig.parameters) == ["env", "agent", "counts", "worlds_per_count", "chunk", "max_steps", "obs"]
    assert sig.parameters["chunk"].default == 64 and sig.parameters["max_steps"].default is None


def test_engine_refuses_a_wrong_count_shape_without_a_device():
    import therldaisyworld_amd as amd

    class _NoDevice:                                           # any touch of the library is an AttributeError
        B, N = 3, 2
    with pytest.raises(ValueError, match="n_active"):
        amd.Engine.run_episode_mlp_counts(_NoDevice(), np.ones(4), np.zeros((1, 1808)), np.zeros(2, dtype=np.int32))


def test_harnesses_refuse_before_anything_is_reset():
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import harness
    env = types.SimpleNamespace(batch_size=6, n_agents=4, precision="exact", collision_mode=0)   # reset() would be an AttributeError
    mlp = amd.MLP()
    with pytest.raises(ValueError, match="batch_size"):
        harness.simulate_agent_count_sweep(env, mlp, [1, 2], 4)
    with pytest.raises(ValueError, match="counts"):
        harness.simulate_agent_count_sweep(env, mlp, [1, 5], 3)
    with pytest.raises(ValueError, match="counts"):
        harness.simulate_agent_count_sweep(env, mlp, [-1, 2], 3)
    with pytest.raises(ValueError, match="MLP"):
        harness.simulate_agent_count_sweep(env, lambda obs: obs, [1, 2], 3)
    with pytest.raises(ValueError, match="MLP"):
        harness.simulate_agent_count_sweep(env, amd.Greedy(epsilon=0.1), [1, 2], 3)
    env.precision = "f64"
    with pytest.raises(ValueError, match="device-resident"):
        harness.simulate_agent_count_sweep(env, mlp, [1, 2], 3)
    env.precision = "exact"
    greedy = amd.Greedy(epsilon=0.0)
    for bad in (-1, 5):
        with pytest.raises(ValueError, match="n_agents"):
            harness.simulate_lifespan_sweep(env, [{"agent": greedy}, {"agent": greedy, "n_agents": bad}], 3)


# ---- the three rules on the oracle -----------------------------------------------------------------------------------
class CountedWorld(O.OracleDaisyWorld):
    """An N-agent oracle world with the rules of dw_run_episode_mlp_counts: in world b only agents [0, n_active[b]) are
    stamped into channel 4 (ref forward :454-459) and the observation rows of the others are zero; the caller zeroes the
    absent agents' states."""
    n_active = None

    def forward(self, grid):
        kept = self.P.n_agents
        self.P.n_agents = 0                                    # the parent's stamp loop is skipped ...
        try:
            new_grid = super().forward(grid)
        finally:
            self.P.n_agents = kept
        for bb in range(self.P.batch_size):                    # ... and taken over the world's own agents
            for nn in range(self.n_active[bb]):
                r, c = self.agent_indices[bb, nn, 0], self.agent_indices[bb, nn, 1]
                new_grid[bb, O.CH_TEMP_LIGHT, r, c] = self.agent_states[bb, nn, 0]
        return new_grid

    def get_obs(self, agent_indices):
        obs = super().get_obs(agent_indices)
        for bb, k in enumerate(self.n_active or ()):          # (reset() observes before the counts are set)
            obs[bb, k:] = 0.0
        return obs


class PerRowMLP(O.OracleMLP):
    """The oracle's MLP evaluated one observation at a time: the same matrix shapes whatever the batch, so the worlds of
    different sizes compared below see the same floating-point sums."""

    def get_action(self, obs):
        flat = obs.reshape(-1, 1, self.IN)
        act = np.array([int(np.argmax(self.forward(x))) for x in flat], dtype=np.int64)
        return act.reshape(*obs.shape[:-3], 1)

    __call__ = get_action


def _policies():
    return {"mlp": PerRowMLP(np.random.RandomState(7).randn(1808) * 0.5), "greedy": O.OracleGreedy(0.0, True),
            "antigreedy": O.OracleGreedy(0.0, False)}


def _start(cls, dim, N, counts, seed, L):
    """The big world (class `cls`, absent states zeroed) and one plain world of counts[b] agents per world b, all at
    luminosity L with the same covers and first agents."""
    B = len(counts)
    np.random.seed(seed)
    big = cls(grid_dimension=dim, n_agents=N, batch_size=B)
    big.reset()
    big.L = L
    light, dark = big.grid[:, O.CH_LIGHT].copy(), big.grid[:, O.CH_DARK].copy()
    big.set_initial_cover(light, dark)
    big.n_active = list(counts)
    for b, k in enumerate(counts):
        big.agent_states[b, k:] = 0.0
    small = []
    for b, k in enumerate(counts):
        one = O.OracleDaisyWorld(grid_dimension=dim, n_agents=k, batch_size=1)
        one.L = L
        one.set_initial_cover(light[b:b + 1], dark[b:b + 1])
        one.agent_indices = big.agent_indices[b:b + 1, :k].copy()
        one.agent_states = np.ones((1, k, 1))
        small.append(one)
    return big, small


#        dim, N, counts,        steps
MODEL_CASES = [(8, 6, (0, 1, 3, 6), 60),
               (4, 40, (40, 17, 2), 25)]       # more agents than cells: stamps collide


@pytest.mark.parametrize("policy", ("mlp", "greedy", "antigreedy"))
@pytest.mark.parametrize("dim,N,counts,steps", MODEL_CASES, ids=("8x8", "4x4"))
def test_the_three_rules_equal_a_smaller_environment(dim, N, counts, steps, policy):
    agent = _policies()[policy]
    big, small = _start(CountedWorld, dim, N, counts, 100 + dim, 0.9)
    obs = big.get_obs(big.agent_indices)
    sobs = [one.get_obs(one.agent_indices) for one in small]
    grazed = False
    for t in range(steps):
        action = agent(obs)
        for b, k in enumerate(counts):
            assert np.array_equal(obs[b, :k], sobs[b][0]) and not obs[b, k:].any(), (t, b, "observations")
        obs, reward, done, _ = big.step(action)
        for b, (k, one) in enumerate(zip(counts, small)):
            if k:
                saction = agent(sobs[b])
                assert np.array_equal(saction, action[b:b + 1, :k]), (t, b, "actions")
                sobs[b], sreward, sdone, _ = one.step(saction)
                assert np.array_equal(reward[b, :k], sreward[0]) and np.array_equal(done[b, :k], sdone[0]), (t, b, "reward / done")
                assert np.array_equal(big.agent_indices[b, :k], one.agent_indices[0]), (t, b, "positions")
                assert np.array_equal(big.agent_states[b, :k], one.agent_states[0]), (t, b, "states")
            else:
                one.step(None)
            assert np.array_equal(big.grid[b], one.grid[0]), (t, b, "the 7-channel grid")
            assert not reward[b, k:].any() and done[b, k:].all() and not big.agent_states[b, k:].any(), (t, b, "absent agents")
        grazed = grazed or bool((reward > 0).any())
    assert grazed and big.grid[:, 1:3].max() > 0.005            # (not a comparison of dead worlds)


def test_the_model_can_tell_a_stamp_from_no_stamp():
    """Otherwise the comparison above could not fail: with the stamps of the absent (state-0) agents left in channel 4,
    the MLP's observations differ from the smaller world's."""
    dim, N, counts, steps = MODEL_CASES[1][:4]
    big, small = _start(O.OracleDaisyWorld, dim, N, counts, 100 + dim, 0.9)
    big.step(np.full((len(counts), N, 1), 8))                    # one resting step: forward stamps every agent
    for one in small:
        one.step(np.full((1, one.P.n_agents, 1), 8))
    obs = big.get_obs(big.agent_indices)
    assert any(not np.array_equal(obs[b, :k], one.get_obs(one.agent_indices)[0]) for b, (k, one) in enumerate(zip(counts, small)))


@pytest.mark.parametrize("greedy", (True, False))
@pytest.mark.parametrize("dim,N,counts,steps", MODEL_CASES, ids=("8x8", "4x4"))
def test_zeroed_states_suffice_for_policies_that_read_the_covers(dim, N, counts, steps, greedy):
    """The `"n_agents"` scenarios of simulate_lifespan_sweep: an N-agent world with plainly zeroed states and ORDINARY
    stamps, under a greedy policy, has the planes and the lifespan counts of the k-agent world."""
    agent = O.OracleGreedy(0.0, greedy)
    big, small = _start(O.OracleDaisyWorld, dim, N, counts, 200 + dim, 0.9)
    B = len(counts)
    done_at, agents_done_at = np.zeros(B, dtype=int), np.zeros((B, N), dtype=int)
    s_done_at, s_agents = np.zeros(B, dtype=int), [np.zeros(k, dtype=int) for k in counts]
    obs = big.get_obs(big.agent_indices)
    sobs = [one.get_obs(one.agent_indices) for one in small]
    for t in range(steps):
        obs, reward, done, _ = big.step(agent(obs))
        done_at += big.grid[:, 1:3].max(axis=(1, 2, 3)) > 0.005
        agents_done_at += ~done[..., 0]
        for b, (k, one) in enumerate(zip(counts, small)):
            if k:
                sobs[b], _, sdone, _ = one.step(agent(sobs[b]))
                s_agents[b] += ~sdone[0, :, 0]
            else:
                one.step(None)
            s_done_at[b] += one.grid[0, 1:3].max() > 0.005
            assert np.array_equal(big.grid[b, :3], one.grid[0, :3]), (t, b, "planes")
    assert np.array_equal(done_at, s_done_at) and done_at.max() > 0
    for b, k in enumerate(counts):
        assert np.array_equal(agents_done_at[b, :k], s_agents[b]) and not agents_done_at[b, k:].any(), b


# ---- the form decision -----------------------------------------------------------------------------------------------
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


def _plan(C_, N, f64=False, collision_mode=0, no_episode_kernel=False):
    """The header's decision restated: (worlds per block, bytes of a world, dynamic LDS, all LDS, workgroup kernel?)."""
    wpb = 4 if C_ <= 256 else (2 if C_ <= 1024 else 1)
    world = (16 * C_ + 20 * N + 4 * C_ + 32 + 2 * 240 + 15) // 16 * 16
    static = 16 * 128 * 8
    total = static + wpb * world
    ok = C_ <= 4096 and total <= 160 * 1024 and not f64 and collision_mode == 0 and not no_episode_kernel
    return wpb, world, wpb * world, total, int(ok)


#             C,    N,    f64, collision, no kernel
PLAN_SHAPES = [(256, 271, 0, 0, 0),       # the notebook's largest scan point: the LDS kernel
               (256, 4, 0, 0, 0),         # the ES shape
               (256, 1700, 0, 0, 0),      # 4 x 39 632 + 16 384 bytes > 160 KiB: launches per step
               (256, 1600, 0, 0, 0),
               (64, 70, 0, 0, 0), (400, 9, 0, 0, 0), (1155, 5, 0, 0, 0), (1024, 0, 0, 0, 0), (1025, 100, 0, 0, 0),
               (4096, 3000, 0, 0, 0), (4096, 3300, 0, 0, 0), (4097, 1, 0, 0, 0),
               (256, 16, 1, 0, 0), (256, 16, 0, 1, 0), (256, 16, 0, 0, 1)]


def _check_plan_driver(exe):
    args = [str(v) for shape in PLAN_SHAPES for v in shape]
    out = subprocess.run([exe, *args], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert lines[0] == "static 16384 groups 16"
    rows = [tuple(int(v) for v in ln.split()) for ln in lines[1:]]
    assert rows == [(s[0], s[1], *_plan(s[0], s[1], bool(s[2]), s[3], bool(s[4]))) for s in PLAN_SHAPES]
    by_shape = {r[:2]: r for r in rows if r[:2] not in ((256, 16),)}
    assert by_shape[(256, 271)][6] == 1 and by_shape[(256, 4)][6] == 1
    assert by_shape[(256, 1700)][5] > 160 * 1024 and by_shape[(256, 1700)][6] == 0
    assert by_shape[(4097, 1)][6] == 0 and [r[6] for r in rows[-3:]] == [0, 0, 0]
    assert by_shape[(256, 271)][3] < 16 * 1024                  # ~11 KB of a world where episode_mlp asks for ~281 KB


def test_form_decision_equals_its_restatement(tmp_path):
    clang = _rocm_clang()
    if clang is None:
        pytest.skip("the clang++ of ROCm is not installed")
    exe = str(tmp_path / "counts_plan_driver")
    subprocess.check_call([clang, "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CSRC,
                           os.path.join(ROOT, "tests", "counts_plan_driver.cpp"), "-o", exe])
    _check_plan_driver(exe)


def test_form_decision_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    clang = _rocm_clang()
    if clang is None:
        pytest.skip("the clang++ of ROCm is not installed")
    exe = str(tmp_path / "counts_plan_driver_san")
    built = subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", CSRC, os.path.join(ROOT, "tests", "counts_plan_driver.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if built.returncode != 0:
        # only a missing sanitizer runtime excuses the build: anything else is an error in the driver or the header
        assert re.search(r"libclang_rt\.(asan|ubsan)|clang_rt\.(asan|ubsan)", built.stderr), built.stderr
        pytest.skip("the sanitizer runtimes of this clang++ do not link here: " + built.stderr.strip().split("\n")[-1])
    _check_plan_driver(exe)


def test_kernel_info_names_the_form_before_the_first_step_fragment():
    src = open(os.path.join(CSRC, "dw_api.hip")).read()
    body = src[src.index("int dw_kernel_info("):src.index("int dw_audit_tie_bound(")]
    assert body.index('"; mlp counts: %s"') < body.index('"; first step: wave-strip=%dx256"') < body.index('"; per-world constants: %s"')
    assert '"workgroup (LDS)" : "launches per step"' in body[body.index('"; mlp counts: %s"'):]


# ---- the gfx950 assembly ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    import isa_report
    isa_report.OUT = str(tmp_path_factory.mktemp("dw_isa_counts"))   # a private build directory, not the tool's shared default
    text = open(isa_report.build([])).read()
    out = {}
    for name in re.findall(r"\.amdhsa_kernel (\S+)\n", text):
        if not any(stem in name for stem in ("episode_mlp_counts_pw", "observe_counts_pw", "zero_absent_states_pw")):
            continue
        body = re.search(r"\n" + re.escape(name) + r":[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S)
        info = re.search(re.escape(name) + r":.*?; Kernel info:(.*?)(?=\n\t\.(?:text|section)|\Z)", text, re.S)
        assert body and info, name
        out[name] = ({k: int(v) for k, v in re.findall(r"; (\w+)\s*[:=] (\d+)", info.group(1))}, body.group(1))
    return out


def test_the_kernels_exist_in_every_instantiation_with_pw_names(kernels):
    assert all("_pw" in n for n in kernels), sorted(kernels)
    for exact in (0, 1):                                         # both precisions of the workgroup kernel
        assert len([n for n in kernels if f"episode_mlp_counts_pwILb{exact}EE" in n]) == 1, sorted(kernels)
    for prev in ("DF16_", "f", "d"):                             # the formats of the state the channels derive from ...
        for post in (0, 1):                                      # ... before and after the first step
            assert len([n for n in kernels if f"observe_counts_pwI{prev}Lb{post}EE" in n]) == 1, (prev, post, sorted(kernels))
    assert len([n for n in kernels if "zero_absent_states_pw" in n]) == 1
    assert len(kernels) == 9, sorted(kernels)


def test_no_scratch_no_calls_and_the_static_lds_the_header_states(kernels):
    src = open(os.path.join(CSRC, "dw_counts_plan.hpp")).read()
    groups = re.search(r"constexpr int kCountsGroups = kCountsThreads / 16;", src)
    doubles = int(re.search(r"constexpr int kCountsBlockDoubles = (\d+);", src).group(1))
    threads = int(re.search(r"constexpr int kCountsThreads = (\d+);", src).group(1))
    assert groups and "16 384 bytes" in src
    static = threads // 16 * doubles * 8
    assert static == 16384
    for name, (info, body) in kernels.items():
        print(name, {k: info[k] for k in ("NumVgprs", "NumAgprs", "TotalNumSgprs", "Occupancy", "LDSByteSize") if k in info})
        assert info["ScratchSize"] == 0, (name, info)
        assert not re.search(r"\tscratch_", body), name
        assert not re.search(r"\ts_(swappc|call|setpc)", body), name
        assert info["LDSByteSize"] == (static if "episode_mlp_counts_pw" in name else 0), (name, info["LDSByteSize"])
