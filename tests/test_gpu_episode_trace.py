"""dw_run_episode_trace / Engine.run_episode_trace / harness.simulate_grazing (run with ``-m gpu``): dw_run_episode that also
records, for every step and world, what dw_reduce would report after that step.

  wave form    episode_wave_stats_pw (csrc/dw_episode_wave_stats_pw.hpp), exact mode, against the float64 oracle: the records
               of every step, the flags and the whole final state, at shapes on and off the wave's 64-cell slots, run
               lengths around the 64-step segment (1, 64, 65, 130), N = 64 (every lane an agent) and N = 0;
  twins        both precisions against engines with the same seed: `run_episode` with the same arguments (flags, final
               state, last_fixup_count) and K x (`run_episode` of one step + `reduce()`) (the records) - for the fast mode
               this is the bit-for-bit check: float32 results are identical across kernel families in this project;
  other forms  N = 65, C = 4096, the wave-strip step kernel, DW_NO_EPISODE_WAVE and DW_NO_EPISODE_KERNEL: launches per step;
  also         a dying biosphere, the error codes, and simulate_grazing against the notebook's loop on the oracle.

Protocol of every engine case (that of tests/test_gpu_episode_wave.py, whose helpers are repeated here):
``init_random(seed)``, one ``dw_step`` with zero actions (quantises the state; mirrored on the oracle through
``set_initial_cover``), then the call with the rising schedule 0.9 + 0.002 t.  Every comparison is exact equality, and
every case asserts from ``kernel_info()`` which form it ran.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import daisy_oracle as O  # noqa: E402

WAVE, STEPWISE = "one wave per world", "launches per step"
THRESHOLD_K = 5
L0 = 0.9


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _k(x):
    return np.rint(np.asarray(x) * 1000.0).astype(np.int64)


def _engine(amd, B, H, W, N, precision, monkeypatch, switch=None):
    """A handle created under exactly one (or none) of the DW_NO_EPISODE_* switches: they are read at creation."""
    from therldaisyworld_amd import _ffi
    for name in ("DW_NO_EPISODE_WAVE", "DW_NO_EPISODE_KERNEL"):
        monkeypatch.delenv(name, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")
    p = amd.default_params(B, H, W, N)
    p.precision = _ffi.PRECISION[precision]
    return amd.Engine(p)


def _oracle_like(eng, L):
    """Oracle environment (H x W through set_initial_cover) holding the engine's current (downloaded) state."""
    light, dark = eng.download_planes()
    env = O.OracleDaisyWorldC(grid_dimension=max(eng.H, eng.W), n_agents=eng.N, batch_size=eng.B)
    env.P.agent_gamma = eng.params.agent_gamma
    env.L = L
    env.set_initial_cover(light, dark)
    assert env.shape == (eng.H, eng.W)
    if eng.N:
        idx, st = eng.download_agents()
        env.agent_indices = idx.astype(np.int64)
        env.agent_states = st.reshape(eng.B, eng.N, 1).copy()
    else:
        env.agent_indices = np.zeros((eng.B, 0, 2), dtype=np.int64)
        env.agent_states = np.ones((eng.B, 0, 1))
    return env


def _oracle_step(env, L, action):
    """One reference step at luminosity L (ref :475-497).  Returns (reward, done, light, dark) - the covers as forward
    read them: after the agents grazed, which is the engine's retained previous state."""
    env.L = L
    kept = {}
    inner = env.forward

    def forward(grid):
        kept["light"], kept["dark"] = grid[:, O.CH_LIGHT].copy(), grid[:, O.CH_DARK].copy()
        return inner(grid)

    env.forward = forward
    try:
        if env.P.n_agents:
            a = np.asarray(action).reshape(env.P.batch_size, env.P.n_agents, 1).astype(np.int64)
        else:
            a = None
        _, reward, done, _ = env.step(a)
    finally:
        del env.forward
    return reward, done, kept["light"], kept["dark"]


def _resolve_codes(env, codes):
    """Table codes -> actions on the oracle: -1 / -2 are the greedy / anti-greedy choice of that agent
    (ref Greedy.__call__, agents/greedy.py:25-30, epsilon = 0)."""
    if not env.P.n_agents:
        return None
    obs = env.get_obs(env.agent_indices)
    g1 = O.OracleGreedy(epsilon=0.0, greedy=True)(obs)
    g2 = O.OracleGreedy(epsilon=0.0, greedy=False)(obs)
    c = codes.astype(np.int64)[..., None]
    return np.where(c == -1, g1, np.where(c == -2, g2, c))


def _record(env):
    kl, kd = _k(env.grid[:, 1]), _k(env.grid[:, 2])
    return (np.maximum(kl.max(axis=(1, 2)), kd.max(axis=(1, 2))).astype(np.uint32), kl.sum(axis=(1, 2)).astype(np.uint64),
            kd.sum(axis=(1, 2)).astype(np.uint64))


def _quantise(eng, L):
    """The protocol's first step: zero actions from the un-quantised init_random state, mirrored on the oracle."""
    env = _oracle_like(eng, L)
    zeros = np.zeros((eng.B, eng.N, 1), dtype=np.int64)
    eng.step(L, zeros if eng.N else None)
    _oracle_step(env, L, zeros)
    return env


def _schedule(K):
    return 0.9 + 0.002 * np.arange(K, dtype=np.float64)


# ---------------------------------------------------------------------------------------------
# inputs: a function of the case alone
# ---------------------------------------------------------------------------------------------
POLICIES = ("argmax", "argmin", "zeros", "mixed")


def _inputs(shape, K, policy):
    """(policy_mode, use_table (K,) uint8 or None, codes (K, B, N) int8 or None).  "mixed": POLICY_ARGMAX with the table
    taken on some steps only (around the segment boundary among them), codes 0..8 mixed with -1 / -2; "table": every step
    from such a table."""
    from therldaisyworld_amd import _ffi
    B, H, W, N = shape
    if policy in ("argmax", "argmin", "zeros"):
        return {"argmax": _ffi.POLICY_ARGMAX, "argmin": _ffi.POLICY_ARGMIN, "zeros": _ffi.POLICY_ZEROS}[policy], None, None
    rng = np.random.RandomState(97 * B + 13 * H + W + 1000 * N + K)
    codes = rng.randint(-2, 9, size=(K, B, N)).astype(np.int8)
    if policy == "table":
        return _ffi.POLICY_TABLE, None, codes
    ut = (rng.rand(K) < 0.4).astype(np.uint8)
    ut[[t for t in (0, 63, 64, 65) if t < K]] = 1
    ut[[t for t in (1, 62) if t < K]] = 0
    return _ffi.POLICY_ARGMAX, ut, codes


def _codes_of_step(shape, mode, ut, codes, t):
    """The table codes the oracle resolves at step t for these inputs."""
    from therldaisyworld_amd import _ffi
    B, H, W, N = shape
    if mode == _ffi.POLICY_TABLE or (ut is not None and ut[t]):
        return codes[t]
    fill = {_ffi.POLICY_ARGMAX: -1, _ffi.POLICY_ARGMIN: -2, _ffi.POLICY_ZEROS: 0}[mode]
    return np.full((B, N), fill, dtype=np.int8)


_REF = {}


def _reference(env, shape, K, policy, Ls=None, key_extra=None):
    """The oracle's K steps from the quantised state `env` holds: the record, the flags of every step and the final
    state - computed once per case and shared by the runs that start from the same state (asserted)."""
    key = (shape, K, policy, key_extra)
    start = (_k(env.grid[:, 1]), _k(env.grid[:, 2]), env.agent_indices.copy())
    if key in _REF:
        ref = _REF[key]
        assert all(np.array_equal(a, b) for a, b in zip(start, ref["start"])), "the shared reference starts elsewhere"
        return ref
    B, H, W, N = shape
    mode, ut, codes = _inputs(shape, K, policy)
    Ls = _schedule(K) if Ls is None else Ls
    from therldaisyworld_amd import _ffi
    stats = np.zeros((K, B), dtype=_ffi.STATS_DTYPE)
    alive = np.zeros((K, B), dtype=bool)
    ok = np.zeros((K, B, N), dtype=bool)
    for t in range(K):
        action = _resolve_codes(env, _codes_of_step(shape, mode, ut, codes, t))
        reward, done, pl, pd = _oracle_step(env, Ls[t], action)
        stats["max_k"][t], stats["sum_light_k"][t], stats["sum_dark_k"][t] = _record(env)
        alive[t] = stats["max_k"][t] > THRESHOLD_K
        if N:
            ok[t] = ~done[..., 0]
    ref = {"start": start, "stats": stats, "alive": alive, "ok": ok, "light": _k(env.grid[:, 1]), "dark": _k(env.grid[:, 2]),
           "prev_light": _k(pl), "prev_dark": _k(pd)}
    if N:
        ref.update(idx=env.agent_indices.copy(), st=env.agent_states.copy(), reward=reward.copy(), done=done.copy(),
                   obs=env.get_obs(env.agent_indices), action=np.asarray(action)[..., 0].astype(np.int64))
    _REF[key] = ref
    return ref


def _state_of(eng, L_last):
    """Everything the engine can be asked for after a call."""
    from therldaisyworld_amd import _ffi
    out = {}
    out["light"], out["dark"] = (_k(x) for x in eng.download_planes())
    out["prev_light"], out["prev_dark"] = (_k(x) for x in eng.download_planes(_ffi.STATE_PREVIOUS))
    s = eng.reduce()
    for f in ("max_k", "sum_light_k", "sum_dark_k"):
        out["reduce_" + f] = s[f].copy()
    if eng.N:
        idx, st = eng.download_agents()
        out["idx"], out["st"] = idx.astype(np.int64), st[..., None].copy()
        out["reward"], out["done"] = eng.reward_done()
        out["obs"] = eng.get_obs(L_last)
        out["action"] = eng.download_actions().astype(np.int64)
    return out


def _check_invariants(eng, stats, alive, what):
    assert np.array_equal(alive, stats["max_k"] > THRESHOLD_K), f"{what}: world_alive != (max_k > threshold)"
    assert not stats["reserved"].any(), f"{what}: reserved"
    s = eng.reduce()
    for f in ("max_k", "sum_light_k", "sum_dark_k"):
        assert np.array_equal(stats[f][-1], s[f]), f"{what}: the last row is not reduce() ({f})"


def _run_vs_oracle(amd, monkeypatch, shape, K, policy, switch, form, Ls=None, key_extra=None, before_compare=None):
    B, H, W, N = shape
    what = f"{shape} K={K} {policy} {switch or 'default'}"
    eng = _engine(amd, B, H, W, N, "exact", monkeypatch, switch)
    info = eng.kernel_info()
    assert f"; episode trace: {form}" in info, info
    assert info.rsplit("; ", 1)[-1].startswith("per-world constants: "), info
    eng.init_random(300 + 7 * B + H + W + N)
    env = _quantise(eng, L0)
    ref = _reference(env, shape, K, policy, Ls, key_extra)
    if before_compare:
        before_compare(ref)
    mode, ut, codes = _inputs(shape, K, policy)
    Ls = _schedule(K) if Ls is None else Ls
    stats, alive, ok = eng.run_episode_trace(Ls, mode, ut, codes, threshold_k=THRESHOLD_K)
    assert stats.shape == (K, B) and alive.shape == (K, B) and ok.shape == (K, B, N)
    for t in range(K):
        for f in ("max_k", "sum_light_k", "sum_dark_k"):
            assert np.array_equal(stats[f][t], ref["stats"][f][t]), f"{what}: {f}[{t}]"
        assert np.array_equal(alive[t], ref["alive"][t]), f"{what}: world_alive[{t}]"
        assert np.array_equal(ok[t], ref["ok"][t]), f"{what}: agent_ok[{t}]"
    _check_invariants(eng, stats, alive, what)
    got = _state_of(eng, Ls[-1])
    for name in got:
        if not name.startswith("reduce_"):
            assert np.array_equal(got[name], ref[name]), f"{what}: {name}"
    eng.close()
    return ref


# ---------------------------------------------------------------------------------------------
# A. the wave form, exact mode, against the oracle
# ---------------------------------------------------------------------------------------------
#              B, H,  W,  N     Ks
WAVE_SHAPES = [((5, 8, 8, 4), (1, 64, 65, 130)),    # segment boundaries; three segments
               ((3, 16, 16, 16), (65,)),
               ((3, 16, 16, 64), (65,)),            # every lane an agent
               ((2, 5, 13, 3), (65,)),              # C = 65: one cell in the second slot
               ((6, 3, 3, 2), (65,)),               # C < 64, B % 4 != 0
               ((2, 8, 8, 0), (65,))]               # no agents
CASES_A = [(s, K, pol) for s, ks in WAVE_SHAPES for K in ks for pol in POLICIES if s[3] or pol in ("argmax", "zeros")]
CASES_A.append(((5, 8, 8, 4), 130, "table"))


@pytest.mark.parametrize("shape,K,policy", CASES_A, ids=lambda v: str(v).replace(" ", ""))
def test_wave_form_exact_vs_oracle(amd, monkeypatch, shape, K, policy):
    _run_vs_oracle(amd, monkeypatch, shape, K, policy, None, WAVE)


# ---------------------------------------------------------------------------------------------
# B. launches per step, exact mode, against the oracle
# ---------------------------------------------------------------------------------------------
STEPWISE_CASES = [((2, 16, 16, 65), 65, None),      # the first agent count the wave kernel refuses
                  ((2, 64, 64, 4), 65, None),       # C = 4096
                  ((1, 20, 256, 3), 7, None),       # wave-strip step kernel; a K at which dw_run_episode would pair
                  ((5, 8, 8, 4), 130, "DW_NO_EPISODE_WAVE"),
                  ((5, 8, 8, 4), 130, "DW_NO_EPISODE_KERNEL")]


@pytest.mark.parametrize("shape,K,switch", STEPWISE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_launches_per_step_exact_vs_oracle(amd, monkeypatch, shape, K, switch):
    """(5, 8, 8, 4) under either switch shares the wave form's reference: the same records."""
    _run_vs_oracle(amd, monkeypatch, shape, K, "mixed", switch, STEPWISE)


# ---------------------------------------------------------------------------------------------
# C. both precisions against twin engines with the same seed
# ---------------------------------------------------------------------------------------------
TWIN_CASES = [(s, max(ks), None, WAVE) for s, ks in WAVE_SHAPES] + [(s, K, sw, STEPWISE) for s, K, sw in STEPWISE_CASES]


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("shape,K,switch,form", TWIN_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_trace_equals_run_episode_and_single_steps(amd, monkeypatch, shape, K, switch, form, precision):
    """Twin A runs `run_episode` with the same arguments: flags, final state and last_fixup_count identical.  Twin B takes
    K calls of `run_episode` of one step, each followed by `reduce()`: the records identical."""
    B, H, W, N = shape
    what = f"{shape} K={K} {precision} {switch or 'default'}"
    mode, ut, codes = _inputs(shape, K, "mixed")
    Ls = _schedule(K)

    def fresh():
        eng = _engine(amd, B, H, W, N, precision, monkeypatch, switch)
        eng.init_random(41 + H)
        eng.step(L0, np.zeros((B, N, 1), dtype=np.int64) if N else None)
        return eng

    eng = fresh()
    assert f"; episode trace: {form}" in eng.kernel_info(), eng.kernel_info()
    stats, alive, ok = eng.run_episode_trace(Ls, mode, ut, codes, threshold_k=THRESHOLD_K)
    _check_invariants(eng, stats, alive, what)
    got, got_fix = _state_of(eng, Ls[-1]), eng.last_fixup_count()
    eng.close()

    twin = fresh()
    alive_a, ok_a = twin.run_episode(Ls, mode, ut, codes, threshold_k=THRESHOLD_K)
    want, want_fix = _state_of(twin, Ls[-1]), twin.last_fixup_count()
    twin.close()
    assert np.array_equal(alive, alive_a), f"{what}: world_alive"
    assert np.array_equal(ok, ok_a), f"{what}: agent_ok"
    for name in want:
        assert np.array_equal(got[name], want[name]), f"{what}: {name}"
    assert got_fix == want_fix, f"{what}: last_fixup_count {got_fix} != {want_fix}"
    assert stats["max_k"].max() > THRESHOLD_K                   # (not a comparison of dead worlds)

    twin = fresh()
    for t in range(K):
        a1, o1 = twin.run_episode(Ls[t:t + 1], mode, None if ut is None else ut[t:t + 1], codes[t:t + 1], threshold_k=THRESHOLD_K)
        s = twin.reduce()
        for f in ("max_k", "sum_light_k", "sum_dark_k"):
            assert np.array_equal(stats[f][t], s[f]), f"{what}: {f}[{t}] against single steps"
        assert np.array_equal(alive[t], a1[0]) and np.array_equal(ok[t], o1[0]), f"{what}: flags[{t}] against single steps"
    twin.close()


# ---------------------------------------------------------------------------------------------
# D. a dying biosphere
# ---------------------------------------------------------------------------------------------
def test_records_of_a_dying_biosphere(amd, monkeypatch):
    """0.03 per step from 0.9 (L = 2.8 at the end: far beyond what daisies regulate): alive after the first step, dead at
    the end - asserted on the oracle's own series before anything is compared."""
    K = 65
    Ls = 0.9 + 0.03 * np.arange(K, dtype=np.float64)

    def input_condition(ref):
        m = ref["stats"]["max_k"]
        assert (m[0] > THRESHOLD_K).all(), "a world is dead after step 0"
        assert (m[-1] <= THRESHOLD_K).any(), "no world has died"
        assert 0 < (m > THRESHOLD_K).sum() < m.size

    ref = _run_vs_oracle(amd, monkeypatch, (5, 8, 8, 4), K, "argmax", None, WAVE, Ls=Ls, key_extra="dying",
                         before_compare=input_condition)
    assert not ref["alive"][-1].all()


# ---------------------------------------------------------------------------------------------
# E. errors: checked before anything runs, the state is untouched
# ---------------------------------------------------------------------------------------------
def _snapshot(eng):
    light, dark = eng.download_planes()
    s = eng.reduce()
    return light, dark, s


def _assert_untouched(eng, before, what):
    after = _snapshot(eng)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), f"{what}: planes changed"
    assert np.array_equal(before[2], after[2]), f"{what}: reduce() changed"


def test_errors_leave_the_state_untouched(amd, monkeypatch):
    from therldaisyworld_amd import _ffi
    B, H, W, N, K = 3, 8, 8, 2, 4
    Ls = _schedule(K)
    eng = _engine(amd, B, H, W, N, "exact", monkeypatch)
    eng.init_random(5)
    before = _snapshot(eng)
    with pytest.raises(amd.DaisyHipError) as e:                 # the current state is an un-quantised upload
        eng.run_episode_trace(Ls, _ffi.POLICY_ARGMAX)
    assert e.value.code == _ffi.DW_ESTATE
    _assert_untouched(eng, before, "un-quantised")
    eng.step(L0, np.zeros((B, N, 1), dtype=np.int64))
    before = _snapshot(eng)
    rc = eng._lib.dw_run_episode_trace(eng._h, K, _ffi.ptr_d(Ls), _ffi.POLICY_ARGMAX, None, None, THRESHOLD_K, None, None, None)
    assert rc == _ffi.DW_EINVAL and b"trace" in eng._lib.dw_last_error()
    _assert_untouched(eng, before, "null trace")
    with pytest.raises(amd.DaisyHipError) as e:                 # use_table without a table
        eng.run_episode_trace(Ls, _ffi.POLICY_ARGMAX, np.array([0, 1, 0, 0], dtype=np.uint8), None)
    assert e.value.code == _ffi.DW_EINVAL
    _assert_untouched(eng, before, "use_table without a table")
    with pytest.raises(amd.DaisyHipError) as e:
        eng.run_episode_trace(Ls, _ffi.POLICY_TABLE)
    assert e.value.code == _ffi.DW_EINVAL
    _assert_untouched(eng, before, "POLICY_TABLE without a table")
    stats, alive, ok = eng.run_episode_trace(Ls, _ffi.POLICY_ARGMAX)      # ... and the handle still works
    _check_invariants(eng, stats, alive, "after the errors")
    eng.close()

    f64 = _engine(amd, B, H, W, N, "f64", monkeypatch)
    f64.init_random(5)
    f64.step(L0, np.zeros((B, N, 1), dtype=np.int64))
    before = _snapshot(f64)
    with pytest.raises(amd.DaisyHipError) as e:
        f64.run_episode_trace(Ls, _ffi.POLICY_ARGMAX)
    assert e.value.code == _ffi.DW_EINVAL
    _assert_untouched(f64, before, "f64")
    f64.close()


# ---------------------------------------------------------------------------------------------
# F. simulate_grazing against the notebook's loop on the oracle environment
# ---------------------------------------------------------------------------------------------
GRAZING_AGENTS = {"none": None, "greedy": dict(epsilon=0.0), "antigreedy": dict(greedy=False, epsilon=0.0),
                  "half_random": dict(epsilon=0.5)}
_NOTEBOOK = {}


def _notebook_run(agent_key, nsteps, B):
    """The reference's loop (update_fig_agent / the notebooks' cells): step, then append the population means - on the
    oracle environment, from seed 17, once per agent; then what the environment holds, and one further step."""
    key = agent_key
    if key in _NOTEBOOK:
        return _NOTEBOOK[key]
    kw = GRAZING_AGENTS[agent_key]
    np.random.seed(17)
    ref = O.OracleDaisyWorld.like_reference_ctor(grid_dimension=8, n_agents=4)
    ref.P.batch_size = B
    obs = ref.reset()
    agent = None if kw is None else O.OracleGreedy(**kw)
    out = {k: [] for k in ("L", "light", "dark", "max", "agents_alive", "ok")}
    for _ in range(nsteps):
        action = agent(obs) if agent is not None else None
        out["L"].append(ref.L)
        obs, reward, done, _ = ref.step(action)
        out["light"].append(ref.grid[:, 1].mean(axis=(1, 2)))
        out["dark"].append(ref.grid[:, 2].mean(axis=(1, 2)))
        out["max"].append(ref.grid[:, 1:3].max(axis=(1, 2, 3)))
        out["ok"].append(~done[..., 0])
        out["agents_alive"].append((~done[..., 0]).sum(axis=1))
    out = {k: np.array(v) for k, v in out.items()}
    out.update(grid=ref.grid.copy(), env_L=ref.L, step_count=ref.step_count, rng=np.random.get_state())
    a = agent(obs) if agent is not None else None
    out["next_obs"], out["next_reward"], _, _ = ref.step(a)
    out["next_action"] = a
    _NOTEBOOK[key] = out
    return out


@pytest.mark.parametrize("precision", ["exact", "f64"])
@pytest.mark.parametrize("agent_key", list(GRAZING_AGENTS))
def test_simulate_grazing_vs_notebook_loop(amd, agent_key, precision):
    """8x8, N = 4, B = 6, 70 steps in chunks of 32 (a partial last chunk): curves, agents_alive, env.grid, env.L,
    env.step_count and the legacy generator's state equal the oracle loop's, and one further env.step agrees.  An "f64"
    environment gives the same dict through the host loop."""
    from therldaisyworld_amd import harness
    B, nsteps = 6, 70
    ref = _notebook_run(agent_key, nsteps, B)
    kw = GRAZING_AGENTS[agent_key]
    np.random.seed(17)
    env = amd.RLDaisyWorld(grid_dimension=8, n_agents=4, precision=precision)
    env.batch_size = B
    agent = None if kw is None else amd.Greedy(**kw)
    out = harness.simulate_grazing(env, agent, nsteps, chunk=32)
    assert np.array_equal(out["L"], ref["L"])
    # per-mille integers: sum_k / 1000 / 64 against the oracle's mean of 64 three-decimal covers
    assert np.array_equal(out["stats"]["sum_light_k"], np.rint(ref["light"] * 64000).astype(np.uint64))
    assert np.array_equal(out["stats"]["sum_dark_k"], np.rint(ref["dark"] * 64000).astype(np.uint64))
    assert np.array_equal(out["stats"]["max_k"], np.rint(ref["max"] * 1000).astype(np.uint32))
    assert np.allclose(out["mean_light"], ref["light"], rtol=0, atol=1e-12)
    assert np.allclose(out["mean_dark"], ref["dark"], rtol=0, atol=1e-12)
    assert np.array_equal(out["alive"], ref["max"] > 0.005)
    assert np.array_equal(out["agent_ok"], ref["ok"]) and np.array_equal(out["agents_alive"], ref["agents_alive"])
    assert out["stats"]["max_k"].max() > THRESHOLD_K            # (not the curves of dead worlds)
    assert np.array_equal(env.grid, ref["grid"])
    assert env.L == ref["env_L"] and env.step_count == ref["step_count"] == nsteps
    have, want = np.random.get_state(), ref["rng"]
    assert have[2] == want[2] and np.array_equal(have[1], want[1])
    obs, reward, _, _ = env.step(ref["next_action"])
    assert np.array_equal(obs, ref["next_obs"]) and np.array_equal(reward, ref["next_reward"])
    env.close()
