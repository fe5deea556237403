"""dw_run_episode_mlp_counts / Engine.run_episode_mlp_counts / harness.simulate_agent_count_sweep and the `"n_agents"`
scenarios of simulate_lifespan_sweep (run with ``-m gpu``): MLP episodes in which every world has its own number of agents.

The contract is independence: for world b with k = n_active[b] the call leaves what a ONE-world engine with n_agents = k
holds that was given world b's planes and first k agents and took the same steps with the existing calls
(`policy_mlp_population` for [0, min(split, k)) and [min(split, k), k), `step_device_actions`, `reward_done`, `reduce`; k = 0:
an agent-free engine, `step` / `reduce`).  Every comparison is byte-exact, in both precisions.

Protocol: quantised random planes and agents go up (`upload_state_f32(quantised=True)`); in every world with 0 < k < N the
absent agent k sits on agent 0's cell, so the stamp of an absent agent lies inside an observed patch; one zero-action
`dw_step` (the retained previous state is quantised too: the whole call runs in the form the handle names); then the call
with three parameter sets and member maps that differ per world, schedule 0.9 + 0.002 t.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L0 = 0.9
WORKGROUP, STEPWISE = "workgroup (LDS)", "launches per step"
N_MEMBERS = 3
PRECISIONS = ("exact", "fast")
KS = (1, 9)
#            B, H,  W,  N, split, counts
CASES = {"A": (6, 16, 16, 21, 2, (0, 1, 4, 5, 21, 20)),    # four worlds per workgroup, a second one with two invalid worlds;
                                                            # count 0, below split, = N, a partial last pass
         "B": (3, 8, 8, 70, 35, (70, 33, 2)),               # more agents than cells
         "C": (3, 20, 20, 9, 9, (9, 3, 0)),                 # two worlds per workgroup, one invalid; no adversary
         "D": (2, 33, 35, 5, 0, (5, 2))}                    # one world per workgroup, H != W, everyone on member_b


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _schedule(K):
    return 0.9 + 0.002 * np.arange(K, dtype=np.float64)


def _engine(amd, B, H, W, N, precision, monkeypatch, switch=None):
    """A handle created under DW_NO_EPISODE_KERNEL or not: the switches are read at creation."""
    from therldaisyworld_amd import _ffi
    for name in ("DW_NO_EPISODE_WAVE", "DW_NO_EPISODE_KERNEL"):
        monkeypatch.delenv(name, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")
    p = amd.default_params(B, H, W, N)
    p.precision = _ffi.PRECISION[precision]
    return amd.Engine(p)


_INPUTS = {}


def _inputs(case, raw=False):
    """Planes (float32 natural units; `raw`: not multiples of 1/1000), agents, parameter sets, member maps of a case."""
    key = (case, raw)
    if key not in _INPUTS:
        B, H, W, N, split, counts = CASES[case]
        rng = np.random.RandomState(sum(map(ord, case)) * 100 + B + H + W + N + raw)
        if raw:
            light = (rng.rand(B, H, W) * 0.45).astype(np.float32)
            dark = (rng.rand(B, H, W) * 0.45).astype(np.float32)
        else:
            light = (rng.randint(0, 450, size=(B, H, W)) / 1000.0).astype(np.float32)
            dark = (rng.randint(0, 450, size=(B, H, W)) / 1000.0).astype(np.float32)
        idx = np.stack([rng.randint(0, H, size=(B, N)), rng.randint(0, W, size=(B, N))], axis=-1).astype(np.int32)
        st = rng.uniform(0.3, 1.0, size=(B, N))
        for b, k in enumerate(counts):
            if 0 < k < N:
                idx[b, k] = idx[b, 0]                            # an absent agent's stamp inside an observed patch
        params = rng.randn(N_MEMBERS, 1808) * 0.5
        ma = (np.arange(B) % N_MEMBERS).astype(np.int32)
        mb = ((np.arange(B) + 1 + np.arange(B) // N_MEMBERS) % N_MEMBERS).astype(np.int32)
        out = dict(light=light, dark=dark, idx=idx, st=st, params=params, ma=ma, mb=mb)
        for a in out.values():
            a.flags.writeable = False
        _INPUTS[key] = out
    return _INPUTS[key]


def _fresh(amd, case, precision, monkeypatch, switch=None, raw=False):
    """The engine of a case after the protocol's uploads (and, unless `raw`, its zero-action step)."""
    B, H, W, N, split, counts = CASES[case]
    inp = _inputs(case, raw)
    eng = _engine(amd, B, H, W, N, precision, monkeypatch, switch)
    eng.upload_state_f32(inp["light"], inp["dark"], quantised=not raw)
    eng.upload_agents(inp["idx"], inp["st"])
    if not raw:
        eng.step(L0, np.zeros((B, N, 1), dtype=np.int64))
    return eng


def _world_state(eng):
    from therldaisyworld_amd import _ffi
    out = {}
    out["light"], out["dark"] = eng.download_planes()
    out["prev_light"], out["prev_dark"] = eng.download_planes(_ffi.STATE_PREVIOUS)
    out["reduce"] = eng.reduce()
    if eng.N:
        out["idx"], out["st"] = eng.download_agents()
        out["action"] = eng.download_actions()
    out["fixups"] = eng.last_fixup_count()
    return out


_REF = {}


def _reference(amd, case, precision, monkeypatch, K_max=max(KS), keep=KS, raw=False):
    """One engine per world, as in the contract, K_max steps; the state each holds after the step counts in `keep`.
    Computed once per (case, precision, start) and shared."""
    from therldaisyworld_amd import _ffi
    key = (case, precision, raw, K_max)
    if key in _REF:
        return _REF[key]
    B, H, W, N, split, counts = CASES[case]
    inp = _inputs(case, raw)
    Ls = _schedule(K_max)
    reward = np.zeros((K_max, B, N, 1))
    done = np.ones((K_max, B, N, 1), dtype=bool)
    stats = np.zeros((K_max, B), dtype=_ffi.STATS_DTYPE)
    states = {K: [None] * B for K in keep}
    for b, k in enumerate(counts):
        eng = _engine(amd, 1, H, W, k, precision, monkeypatch)
        eng.upload_state_f32(inp["light"][b:b + 1], inp["dark"][b:b + 1], quantised=not raw)
        if k:
            eng.upload_agents(inp["idx"][b:b + 1, :k], inp["st"][b:b + 1, :k])
        if not raw:
            eng.step(L0, np.zeros((1, k, 1), dtype=np.int64) if k else None)
        s = min(split, k)
        for t in range(K_max):
            if k:
                eng.policy_mlp_population(inp["params"], inp["ma"][b:b + 1], 0, s)
                eng.policy_mlp_population(inp["params"], inp["mb"][b:b + 1], s, k)
                eng.step_device_actions(Ls[t])
                r, d = eng.reward_done()
                reward[t, b, :k], done[t, b, :k] = r[0], d[0].astype(bool)
            else:
                eng.step(Ls[t], None)
            row = eng.reduce()
            for f in ("max_k", "sum_light_k", "sum_dark_k"):
                stats[f][t, b] = row[f][0]
            if t + 1 in keep:
                states[t + 1][b] = _world_state(eng)
        eng.close()
    for a in (reward, done, stats):
        a.flags.writeable = False
    _REF[key] = (reward, done, stats, states)
    return _REF[key]


def _call(eng, case, K, Ls=None, raw=False, params=True, t0=0):
    B, H, W, N, split, counts = CASES[case]
    inp = _inputs(case, raw)
    Ls = _schedule(t0 + K)[t0:] if Ls is None else Ls
    return eng.run_episode_mlp_counts(Ls, inp["params"] if params else None, np.asarray(counts, dtype=np.int32), inp["ma"],
                                      inp["mb"], split, n_members=N_MEMBERS)


def _assert_rows(got, ref, case, t0, K, what):
    B, H, W, N, split, counts = CASES[case]
    reward, done, stats = got
    r_reward, r_done, r_stats, _ = ref
    assert reward.shape == (K, B, N, 1) and done.shape == (K, B, N, 1) and stats.shape == (K, B)
    assert _bits(reward) == _bits(r_reward[t0:t0 + K]), f"{what}: reward"
    assert np.array_equal(done, r_done[t0:t0 + K]), f"{what}: done"
    for b, k in enumerate(counts):                               # the absent agents' bytes
        assert not np.ascontiguousarray(reward[:, b, k:]).view(np.uint8).any(), f"{what}: world {b}: reward of absent agents"
        assert done[:, b, k:].all(), f"{what}: world {b}: done of absent agents"
    assert not stats["reserved"].any(), f"{what}: reserved"
    assert _bits(stats) == _bits(r_stats[t0:t0 + K]), f"{what}: records"


def _assert_state(eng, ref_states, case, positions_before, what):
    """Everything the contract names, world by world; the absent agents' state 0, action 0, position as it was."""
    B, H, W, N, split, counts = CASES[case]
    got = _world_state(eng)
    for b, k in enumerate(counts):
        want = ref_states[b]
        for name in ("light", "dark", "prev_light", "prev_dark"):
            assert np.array_equal(got[name][b], want[name][0]), f"{what}: world {b}: {name}"
        for f in ("max_k", "sum_light_k", "sum_dark_k"):
            assert got["reduce"][f][b] == want["reduce"][f][0], f"{what}: world {b}: reduce() {f}"
        if k:
            assert np.array_equal(got["idx"][b, :k], want["idx"][0]), f"{what}: world {b}: positions"
            assert _bits(got["st"][b, :k]) == _bits(want["st"][0]), f"{what}: world {b}: states"
            assert np.array_equal(got["action"][b, :k], want["action"][0]), f"{what}: world {b}: actions"
        assert not np.ascontiguousarray(got["st"][b, k:]).view(np.uint8).any(), f"{what}: world {b}: absent states are not 0.0"
        assert not got["action"][b, k:].any(), f"{what}: world {b}: absent actions"
        assert np.array_equal(got["idx"][b, k:], positions_before[b, k:]), f"{what}: world {b}: absent positions moved"
    assert got["fixups"] == sum(w["fixups"] for w in ref_states), f"{what}: last_fixup_count"


def _assert_last_row(eng, stats, what):
    s = eng.reduce()
    for f in ("max_k", "sum_light_k", "sum_dark_k"):
        assert np.array_equal(stats[f][-1], s[f]), f"{what}: the last row is not reduce() ({f})"


def _assert_form(eng, form):
    info = eng.kernel_info()
    assert f"; mlp counts: {form}" in info, info
    assert info.rsplit("; ", 1)[-1].startswith("per-world constants: "), info
    if "; first step:" in info:
        assert info.index("; mlp counts:") < info.index("; first step:"), info


def _run_and_check(amd, monkeypatch, case, K, precision, switch, form):
    what = f"{case} K={K} {precision} {form}"
    ref = _reference(amd, case, precision, monkeypatch)
    assert (ref[0] > 0).any() and ref[2]["max_k"].max() > 5     # (not a comparison of dead worlds)
    eng = _fresh(amd, case, precision, monkeypatch, switch)
    _assert_form(eng, form)
    before = eng.download_agents()[0]
    got = _call(eng, case, K)
    _assert_rows(got, ref, case, 0, K, what)
    _assert_state(eng, ref[3][K], case, before, what)
    _assert_last_row(eng, got[2], what)
    eng.close()


# ---------------------------------------------------------------------------------------------
# 1. the workgroup kernel against one engine per world
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_each_world_is_an_engine_of_its_own(amd, monkeypatch, case, K, precision):
    _run_and_check(amd, monkeypatch, case, K, precision, None, WORKGROUP)


# ---------------------------------------------------------------------------------------------
# 2. the launches per step return the same bytes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_launches_per_step_under_the_switch(amd, monkeypatch, case, precision):
    _run_and_check(amd, monkeypatch, case, 9, precision, "DW_NO_EPISODE_KERNEL", STEPWISE)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", ("A", "B"))
def test_a_call_straight_after_an_unquantised_upload(amd, monkeypatch, case, precision):
    """The first steps run per step (the state, then the retained previous state, is the un-quantised upload), the rest
    in the workgroup kernel: one continuous set of rows."""
    K = 6
    what = f"{case} raw {precision}"
    ref = _reference(amd, case, precision, monkeypatch, K_max=K, keep=(K,), raw=True)
    eng = _fresh(amd, case, precision, monkeypatch, raw=True)
    _assert_form(eng, WORKGROUP)
    before = eng.download_agents()[0]
    got = _call(eng, case, K, raw=True)
    _assert_rows(got, ref, case, 0, K, what)
    _assert_state(eng, ref[3][K], case, before, what)
    _assert_last_row(eng, got[2], what)
    eng.close()


# ---------------------------------------------------------------------------------------------
# 3. the control: without the counts the stamps of the absent agents are there, and the results differ
# ---------------------------------------------------------------------------------------------
def test_zeroed_states_alone_do_not_imitate_absent_agents(amd, monkeypatch):
    differs = {}
    for case in ("A", "B"):
        B, H, W, N, split, counts = CASES[case]
        inp = _inputs(case)
        eng = _fresh(amd, case, "exact", monkeypatch)
        reward, done, _ = _call(eng, case, 9)
        action = eng.download_actions()
        eng.close()
        twin = _fresh(amd, case, "exact", monkeypatch)
        idx, st = twin.download_agents()
        for b, k in enumerate(counts):
            st[b, k:] = 0.0
        twin.upload_agents(idx, st)
        t_reward, t_done = twin.run_episode_mlp(_schedule(9), inp["params"], inp["ma"], inp["mb"], split)
        t_action = twin.download_actions()
        twin.close()
        differs[case] = _bits(reward) != _bits(t_reward) or not np.array_equal(action, t_action)
    assert any(differs.values()), differs


# ---------------------------------------------------------------------------------------------
# 4. the ends of the range: every agent present, no agent present
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_all_counts_n_is_run_episode_mlp(amd, monkeypatch, precision):
    from test_gpu_episode_trace import _state_of
    B, H, W, N, split, counts = CASES["A"]
    inp, Ls = _inputs("A"), _schedule(9)
    twin = _fresh(amd, "A", precision, monkeypatch)
    want = twin.run_episode_mlp(Ls, inp["params"], inp["ma"], inp["mb"], split, trace=True)
    want_state, want_fix = _state_of(twin, Ls[-1]), twin.last_fixup_count()
    twin.close()
    eng = _fresh(amd, "A", precision, monkeypatch)
    got = eng.run_episode_mlp_counts(Ls, inp["params"], np.full(B, N, dtype=np.int32), inp["ma"], inp["mb"], split)
    assert _bits(got[0]) == _bits(want[0]) and np.array_equal(got[1], want[1]) and _bits(got[2]) == _bits(want[2])
    got_state = _state_of(eng, Ls[-1])
    for name in want_state:
        assert np.array_equal(got_state[name], want_state[name]), name
    assert eng.last_fixup_count() == want_fix
    eng.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_all_counts_zero_is_an_agent_free_run(amd, monkeypatch, precision):
    B, H, W, N, split, counts = CASES["C"]
    inp, Ls = _inputs("C"), _schedule(9)
    twin = _fresh(amd, "C", precision, monkeypatch)
    want = twin.step_n_trace(Ls)
    want_planes, want_reduce = twin.download_planes(), twin.reduce()
    twin.close()
    eng = _fresh(amd, "C", precision, monkeypatch)
    reward, done, stats = eng.run_episode_mlp_counts(Ls, inp["params"], np.zeros(B, dtype=np.int32), inp["ma"], inp["mb"], split)
    assert not reward.any() and done.all()
    for f in ("max_k", "sum_light_k", "sum_dark_k"):
        assert np.array_equal(stats[f], want[f]), f
    for a, b in zip(eng.download_planes(), want_planes):
        assert np.array_equal(a, b)
    assert _bits(eng.reduce()) == _bits(want_reduce)
    assert not eng.download_agents()[1].any() and not eng.download_actions().any()
    eng.close()


# ---------------------------------------------------------------------------------------------
# 5. refusals leave everything as it was
# ---------------------------------------------------------------------------------------------
def test_refusals_leave_state_agents_and_parameter_sets_untouched(amd, monkeypatch):
    from therldaisyworld_amd import _ffi
    case = "A"
    B, H, W, N, split, counts = CASES[case]
    inp = _inputs(case)
    ref = _reference(amd, case, "exact", monkeypatch)
    eng = _fresh(amd, case, "exact", monkeypatch)
    _assert_rows(_call(eng, case, 1), ref, case, 0, 1, "first step")      # the parameter sets are on the device now
    before = _world_state(eng)
    Ls = _schedule(9)[1:]
    other = np.zeros((N_MEMBERS, 1808))                          # sets that must NOT replace the resident ones

    def refused(n_active, pattern):
        with pytest.raises(amd.DaisyHipError, match=pattern) as e:
            eng.run_episode_mlp_counts(Ls, other, n_active, inp["ma"], inp["mb"], split)
        assert e.value.code == _ffi.DW_EINVAL
        after = _world_state(eng)
        for name in before:
            assert _bits(after[name]) == _bits(before[name]) if name != "fixups" else after[name] == before[name], name

    bad = np.asarray(counts, dtype=np.int32)
    bad[3] = -1
    refused(bad, "world 3")
    bad[3], bad[5] = counts[3], N + 1
    refused(bad, "world 5")
    refused(None, "n_active")
    # ... and the handle still works, with the sets it had: the rows continue the reference's
    got = _call(eng, case, 8, params=False, t0=1)
    _assert_rows(got, ref, case, 1, 8, "after the refusals")
    eng.close()


# ---------------------------------------------------------------------------------------------
# 6. the harnesses
# ---------------------------------------------------------------------------------------------
def _notebook_rule(alive, ok):
    """done_at (Bs,), agents_done_at (Bs, N) of ONE block from its flags (n, Bs), (n, Bs, N): every step up to and including
    the first at which all of its worlds are dead is counted."""
    dead = ~alive.any(axis=1)
    n = int(np.argmax(dead)) + 1 if dead.any() else alive.shape[0]
    return alive[:n].sum(axis=0), ok[:n].sum(axis=0)


def test_agent_count_sweep_with_an_mlp_equals_one_environment_per_count(amd):
    dim, N, Bs, counts = 8, 9, 3, [0, 1, 3, 9]
    mlp = amd.MLP()
    mlp.set_parameters(np.random.RandomState(3).randn(1808) * 0.5)
    env = amd.RLDaisyWorld(grid_dimension=dim, n_agents=N)
    env.batch_size = len(counts) * Bs
    env.ramp_period = 64
    np.random.seed(11)
    obs = env.reset()
    grid0, idx0, st0 = env.grid.copy(), env.agent_indices.copy(), env.agent_states.copy()
    done_at, agents_done_at, n_active = amd.simulate_agent_count_sweep(env, mlp, counts, Bs, chunk=32, obs=obs)
    steps = int(env.step_count)
    env.close()
    assert done_at.shape == (len(counts), Bs) and agents_done_at.shape == (len(counts), Bs, N, 1)
    assert np.array_equal(n_active, np.repeat(counts, Bs)) and 0 < steps <= 512 and done_at.max() > 1
    for s, c in enumerate(counts):
        blk = slice(s * Bs, (s + 1) * Bs)
        one = amd.RLDaisyWorld(grid_dimension=dim, n_agents=c)
        one.batch_size = Bs
        one.ramp_period = 64
        np.random.seed(0)
        first = one.reset()
        one.grid = grid0[blk].copy()
        if c:
            one.agent_indices = idx0[blk, :c].copy()
            one.agent_states = st0[blk, :c].copy()
            out = amd.simulate_grazing_mlp(one, mlp, steps, obs=first)
            ok = out["agent_ok"]
        else:
            out = amd.simulate_ramp(one, steps, obs=first)
            ok = np.zeros((steps, Bs, 0), dtype=bool)
        one.close()
        want_done_at, want_agents = _notebook_rule(out["stats"]["max_k"] > 5, ok)
        assert np.array_equal(done_at[s], want_done_at), (c, done_at[s], want_done_at)
        assert np.array_equal(agents_done_at[s, :, :c, 0], want_agents), c
        assert not agents_done_at[s, :, c:].any(), c


@pytest.mark.parametrize("greedy", (True, False))
def test_lifespan_sweep_with_n_agents_equals_smaller_environments(amd, greedy):
    dim, N, Bs, counts = 8, 4, 3, [1, 3]
    env = amd.RLDaisyWorld(grid_dimension=dim, n_agents=N)
    env.batch_size = len(counts) * Bs
    np.random.seed(5)
    obs = env.reset()
    grid0, idx0, st0 = env.grid.copy(), env.agent_indices.copy(), env.agent_states.copy()
    scenarios = [{"agent": amd.Greedy(epsilon=0.0, greedy=greedy), "n_agents": c} for c in counts]
    done_at, agents_done_at, _ = amd.simulate_lifespan_sweep(env, scenarios, Bs, obs=obs)
    env.close()
    assert done_at.max() > 1
    for s, c in enumerate(counts):
        blk = slice(s * Bs, (s + 1) * Bs)
        one = amd.RLDaisyWorld(grid_dimension=dim, n_agents=c)
        one.batch_size = Bs
        np.random.seed(0)
        one.reset()
        one.grid = grid0[blk].copy()
        one.agent_indices = idx0[blk, :c].copy()
        one.agent_states = st0[blk, :c].copy()
        want_done_at, want_agents = amd.simulate_lifespan(one, amd.Greedy(epsilon=0.0, greedy=greedy), obs=one.get_obs(),
                                                          final_state=False)
        one.close()
        assert np.array_equal(done_at[s], want_done_at), (c, done_at[s], want_done_at)
        assert np.array_equal(agents_done_at[s, :, :c], want_agents), c
        assert not agents_done_at[s, :, c:].any(), c
