"""GPU tests (``-m gpu``) of dw_run_episode_ensemble / Engine.run_episode_ensemble / harness.simulate_lifespan_sweep:
the device-resident episode loop with physics constants AND a luminosity column of its own for every world.

The contract is independence: world b ends, and reports the per-step flags, exactly as a ONE-world handle that holds
world b and its agents (world_offset = b: Philox draws the same world), carries the world's constants (dw_set_params)
and runs dw_run_episode with column b of the schedule and slice [:, b] of the table.  Everything compared is
integer-valued or float64-exact in that contract - planes, retained previous planes, agent positions and states,
reduce(), the device action buffer, world_alive / agent_ok, the fix-up count - so every comparison is exact equality, in
the exact and the float32-only mode, in the one-wave-per-world form (episode_wave_pw) and in the launches-per-step form.

Protocol of every case: ``init_random(seed)``, one ``dw_step`` with zero actions at the handle's own constants (quantises
the state), then the call under test.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import daisy_oracle as O  # noqa: E402

WAVE, STEPWISE = "one wave per world", "launches per step"
THRESHOLD_K = 5
L0 = 0.94
FIELDS = ("max_k", "sum_light_k", "sum_dark_k")


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _k(x):
    return np.rint(np.asarray(x) * 1000.0).astype(np.int64)


def _params(amd, B, H, W, N, precision, **over):
    from therldaisyworld_amd import _ffi
    p = amd.default_params(B, H, W, N)
    p.precision = _ffi.PRECISION[precision]
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _engine(amd, B, H, W, N, precision, monkeypatch, switch=None, **over):
    """A handle created under exactly one (or none) of the DW_NO_EPISODE_* switches: they are read at creation."""
    for name in ("DW_NO_EPISODE_WAVE", "DW_NO_EPISODE_KERNEL"):
        monkeypatch.delenv(name, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")
    return amd.Engine(_params(amd, B, H, W, N, precision, **over))


def _table(eng, B):
    """The mixed five-kind table: the defaults | q2 = 0 | q2 = q/8 | asymmetric albedos with another gamma | another
    temp_optimal and dt."""
    own = eng.world_params()
    tab = np.repeat(own[None], B)
    for b in range(B):
        kind = b % 5
        if kind == 1:
            tab["q2"][b] = 0.0
        elif kind == 2:
            tab["q2"][b] = float(own["q"]) / 8.0
        elif kind == 3:
            tab["albedo_light"][b], tab["albedo_dark"][b], tab["gamma"][b] = 0.8, 0.3, 0.3
        elif kind == 4:
            tab["temp_optimal"][b], tab["dt"][b] = 290.0, 0.5
    return tab


def _schedule(n, B):
    """(n, B): distinct luminosities per world within 0.6 ... 1.7, not monotone in b, drifting over the run (odd worlds
    up, even worlds down); world 0 is held fixed (its row is derived once)."""
    base = np.linspace(0.65, 1.6, B)[np.random.RandomState(B).permutation(B)]
    drift = 0.036 * (np.arange(n) / max(n - 1, 1))[:, None] * np.where(np.arange(B) % 2, 1.0, -1.0)[None, :]
    drift[:, 0] = 0.0
    L = np.ascontiguousarray(base[None, :] + drift)
    assert L.min() >= 0.6 and L.max() <= 1.7
    return L


def _inputs(K, B, N, seed):
    """codes (K, B, N) int8 from -2 ... 8; use_table (K,) uint8 set on ~40 % of the steps and around the 64-step segment."""
    rng = np.random.RandomState(seed)
    codes = rng.randint(-2, 9, size=(K, B, N)).astype(np.int8)
    ut = (rng.rand(K) < 0.4).astype(np.uint8)
    ut[[t for t in (0, 63, 64, 65) if t < K]] = 1
    return codes, ut


def _quantise(eng):
    eng.step(L0, np.zeros((eng.B, eng.N, 1), dtype=np.int64))


def _collide(eng, idx=None, st=None, world=None):
    """Agent 1 of every world onto agent 0's cell (the first to graze a cell eats it all)."""
    if idx is None:
        idx, st = eng.download_agents()
        idx[:, 1] = idx[:, 0]
        eng.upload_agents(idx, st)
        return idx, st
    eng.upload_agents(idx[world:world + 1], st[world:world + 1])
    return idx, st


def _everything(eng):
    from therldaisyworld_amd import _ffi
    cur = eng.download_planes()
    prev = eng.download_planes(_ffi.STATE_PREVIOUS)
    idx, st = eng.download_agents()
    return {"light": _k(cur[0]), "dark": _k(cur[1]), "prev_light": _k(prev[0]), "prev_dark": _k(prev[1]), "idx": idx, "st": st,
            "reduce": eng.reduce(), "action": eng.download_actions(), "fix": eng.last_fixup_count()}


def _world_by_world(amd, monkeypatch, switch, shape, precision, seed, tab, L, mode, ut, codes, collide=None):
    """The reference of the contract: world b alone on a one-world handle with its constants, column and table slice."""
    from therldaisyworld_amd import _ffi
    B, H, W, N = shape
    parts, alive, ok = [], [], []
    for b in range(B):
        one = _engine(amd, 1, H, W, N, precision, monkeypatch, switch, world_offset=b)
        one.init_random(seed)
        _quantise(one)
        if collide is not None:
            _collide(one, collide[0], collide[1], b)
        p = _params(amd, 1, H, W, N, precision, world_offset=b)
        for name in _ffi.WORLD_PARAM_NAMES:
            setattr(p, name, float(tab[b][name]))
        one.set_params(p)
        a, o = one.run_episode(np.ascontiguousarray(L[:, b]), mode, ut, np.ascontiguousarray(codes[:, b:b + 1]),
                               threshold_k=THRESHOLD_K)
        alive.append(a)
        ok.append(o)
        parts.append(_everything(one))
        one.close()
    ref = {k: np.concatenate([p[k] for p in parts]) for k in parts[0] if k != "fix"}
    ref["fix"] = sum(p["fix"] for p in parts)
    ref["alive"] = np.concatenate(alive, axis=1)
    ref["ok"] = np.concatenate(ok, axis=1)
    return ref


def _assert_same(got, alive, ok, ref, what):
    for t in range(alive.shape[0]):
        assert np.array_equal(alive[t], ref["alive"][t]), f"{what}: world_alive[{t}]"
        assert np.array_equal(ok[t], ref["ok"][t]), f"{what}: agent_ok[{t}]"
    for k in ("light", "dark", "prev_light", "prev_dark", "idx", "st", "action"):
        assert np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:5].tolist())
    for f in FIELDS:
        assert np.array_equal(got["reduce"][f], ref["reduce"][f]), f"{what}: reduce() {f}"
    assert got["fix"] == ref["fix"], f"{what}: fix-up count {got['fix']} != {ref['fix']}"


def _independence(amd, monkeypatch, shape, precision, K, switch, form, collide=False):
    from therldaisyworld_amd import _ffi
    B, H, W, N = shape
    what = f"{shape} {precision} K={K} {switch or 'default'}{' collide' if collide else ''}"
    eng = _engine(amd, B, H, W, N, precision, monkeypatch, switch)
    assert f"; ensemble episode: {form}" in eng.kernel_info(), eng.kernel_info()
    tab = _table(eng, B)
    L = _schedule(K, B)
    codes, ut = _inputs(K, B, N, 7 * B + K)
    eng.init_random(31)
    _quantise(eng)
    placed = _collide(eng) if collide else None
    alive, ok = eng.run_episode_ensemble(tab, L, _ffi.POLICY_ARGMAX, ut, codes, threshold_k=THRESHOLD_K)
    got = _everything(eng)
    eng.close()
    ref = _world_by_world(amd, monkeypatch, switch, shape, precision, 31, tab, L, _ffi.POLICY_ARGMAX, ut, codes, placed)
    assert ref["alive"].any() and ref["ok"].any(), f"{what}: nothing is alive in the reference run"
    _assert_same(got, alive, ok, ref, what)


# ---------------------------------------------------------------------------------------------
# 1. independence, one wave per world: a full and a half-filled block | four cells per lane | 65 cells: one in the second slot
# ---------------------------------------------------------------------------------------------
WAVE_SHAPES = [(6, 8, 8, 4), (6, 16, 16, 4), (5, 5, 13, 3)]


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("shape", WAVE_SHAPES)
def test_wave_kernel_runs_every_world_as_if_alone(amd, monkeypatch, shape, precision):
    _independence(amd, monkeypatch, shape, precision, 70, None, WAVE)          # K = 70 crosses the 64-step segment


def test_wave_kernel_two_agents_on_one_cell(amd, monkeypatch):
    _independence(amd, monkeypatch, (6, 8, 8, 4), "exact", 70, None, WAVE, collide=True)


# ---------------------------------------------------------------------------------------------
# 2. against the float64 oracle, world by world with the world's attributes
# ---------------------------------------------------------------------------------------------
def _resolve_codes(env, codes):
    obs = env.get_obs(env.agent_indices)
    g1 = O.OracleGreedy(epsilon=0.0, greedy=True)(obs)
    g2 = O.OracleGreedy(epsilon=0.0, greedy=False)(obs)
    c = codes.astype(np.int64)[..., None]
    return np.where(c == -1, g1, np.where(c == -2, g2, c))


def test_exact_mode_matches_the_oracle_with_each_worlds_attributes(amd, monkeypatch):
    from therldaisyworld_amd import _ffi
    B, H, W, N, K = 4, 8, 8, 4, 70
    eng = _engine(amd, B, H, W, N, "exact", monkeypatch)
    tab = _table(eng, B)
    L = _schedule(K, B)
    codes, ut = _inputs(K, B, N, 99)
    eng.init_random(17)
    _quantise(eng)
    light, dark = eng.download_planes()
    idx, st = eng.download_agents()
    alive, ok = eng.run_episode_ensemble(tab, L, _ffi.POLICY_ARGMIN, ut, codes, threshold_k=THRESHOLD_K)
    gl, gd = eng.download_planes()
    gidx, gst = eng.download_agents()
    for b in range(B):
        env = O.OracleDaisyWorldC(grid_dimension=H, n_agents=N, batch_size=1)
        env.P.agent_gamma = eng.params.agent_gamma
        for name in _ffi.WORLD_PARAM_NAMES:
            setattr(env.P, name, float(tab[b][name]))
        env.L = L0
        env.set_initial_cover(light[b:b + 1], dark[b:b + 1])
        env.agent_indices = idx[b:b + 1].astype(np.int64)
        env.agent_states = st[b:b + 1].reshape(1, N, 1).copy()
        for t in range(K):
            c = codes[t, b:b + 1] if ut[t] else np.full((1, N), -2, dtype=np.int8)
            env.L = float(L[t, b])
            _, reward, done, _ = env.step(_resolve_codes(env, c).reshape(1, N, 1).astype(np.int64))
            mk = max(_k(env.grid[:, 1]).max(), _k(env.grid[:, 2]).max())
            assert alive[t, b] == (mk > THRESHOLD_K), f"world {b}: world_alive[{t}]"
            assert np.array_equal(ok[t, b], ~done[0, :, 0]), f"world {b}: agent_ok[{t}]"
        assert np.array_equal(_k(gl[b]), _k(env.grid[0, 1])), f"world {b}: light plane"
        assert np.array_equal(_k(gd[b]), _k(env.grid[0, 2])), f"world {b}: dark plane"
        assert np.array_equal(gidx[b], env.agent_indices[0]), f"world {b}: agent positions"
        assert np.array_equal(gst[b], env.agent_states[0, :, 0]), f"world {b}: agent states"
    eng.close()


# ---------------------------------------------------------------------------------------------
# 3. launches per step: the generic per-world step | the per-world wave strips | the wave shape under DW_NO_EPISODE_WAVE
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("shape,switch", [((3, 20, 20, 2), None), ((2, 40, 256, 2), None), ((6, 8, 8, 4), "DW_NO_EPISODE_WAVE")])
def test_launches_per_step_run_every_world_as_if_alone(amd, monkeypatch, shape, switch, precision):
    _independence(amd, monkeypatch, shape, precision, 5, switch, STEPWISE)


def test_wave_kernel_continues_in_a_second_launch(amd, monkeypatch):
    """The wave path keeps at most 32 MiB of rows (136 B per step and world) on the device, in whole 64-step segments: 2000
    worlds leave 123 -> 64 steps per launch, so K = 70 takes a second launch of 6 steps that continues from the planes and
    agents the first wrote back, with its own slices of use_table, the table and the flags.  Reference: the same call as
    launches per step (DW_NO_EPISODE_WAVE), the form held world by world to one-world handles above; everything but the
    count of float64 re-evaluations (a property of the kernel family) is equal bit for bit."""
    from therldaisyworld_amd import _ffi
    shape, K = (2000, 8, 8, 2), 70
    B, H, W, N = shape
    assert (32 << 20) // (136 * B) // 64 * 64 < K
    outs = []
    for switch, form in ((None, WAVE), ("DW_NO_EPISODE_WAVE", STEPWISE)):
        eng = _engine(amd, B, H, W, N, "exact", monkeypatch, switch)
        assert f"; ensemble episode: {form}" in eng.kernel_info(), eng.kernel_info()
        tab = _table(eng, B)
        L = _schedule(K, B)
        codes, ut = _inputs(K, B, N, 11)
        eng.init_random(31)
        _quantise(eng)
        alive, ok = eng.run_episode_ensemble(tab, L, _ffi.POLICY_ARGMIN, ut, codes, threshold_k=THRESHOLD_K)
        outs.append((alive, ok, _everything(eng)))
        eng.close()
    (alive, ok, got), (ralive, rok, ref) = outs
    assert ralive[64:].any() and rok[64:].any() and not rok[64:].all(), "nothing happens in the second launch's steps"
    assert np.array_equal(alive, ralive) and np.array_equal(ok, rok)
    for k in ("light", "dark", "prev_light", "prev_dark", "idx", "st", "action"):
        assert np.array_equal(got[k], ref[k]), k
    for f in FIELDS:
        assert np.array_equal(got["reduce"][f], ref["reduce"][f]), f


# ---------------------------------------------------------------------------------------------
# 4. the degenerate table: the handle's own constants for every world, one luminosity per step
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["exact", "fast"])
def test_degenerate_table_equals_run_episode(amd, monkeypatch, precision):
    from therldaisyworld_amd import _ffi
    B, H, W, N, K = 6, 8, 8, 4, 70
    Ls = np.linspace(0.9, 1.3, K)
    codes, ut = _inputs(K, B, N, 5)
    out = []
    for ensemble in (True, False):
        eng = _engine(amd, B, H, W, N, precision, monkeypatch)
        eng.init_random(3)
        _quantise(eng)
        if ensemble:
            tab = np.repeat(eng.world_params()[None], B)
            flags = eng.run_episode_ensemble(tab, np.repeat(Ls[:, None], B, axis=1), _ffi.POLICY_ARGMAX, ut, codes, THRESHOLD_K)
        else:
            flags = eng.run_episode(Ls, _ffi.POLICY_ARGMAX, ut, codes, threshold_k=THRESHOLD_K)
        out.append((flags, _everything(eng)))
        eng.close()
    (flags, got), ((alive, ok), ref) = out
    ref.update(alive=alive, ok=ok)
    _assert_same(got, flags[0], flags[1], ref, f"degenerate {precision}")
    assert np.array_equal(got["reduce"]["reserved"], ref["reduce"]["reserved"])


# ---------------------------------------------------------------------------------------------
# 5. errors and marks
# ---------------------------------------------------------------------------------------------
def _raises(code, match, fn):
    from therldaisyworld_amd import _ffi
    with pytest.raises(_ffi.DaisyHipError, match=match) as e:
        fn()
    assert e.value.code == code, e.value


def test_errors_leave_the_state_untouched_and_marks_are_kept(amd, monkeypatch):
    from therldaisyworld_amd import _ffi
    B, H, W, N, K = 6, 8, 8, 4, 4
    eng = _engine(amd, B, H, W, N, "exact", monkeypatch)
    tab = _table(eng, B)
    L = _schedule(K, B)
    eng.init_random(9)
    call = lambda t=tab, l=L: eng.run_episode_ensemble(t, l, _ffi.POLICY_ARGMAX)
    _raises(_ffi.DW_ESTATE, "not quantised", call)              # the un-quantised initial state
    _quantise(eng)
    before = _everything(eng)
    bad = tab.copy()
    bad["g"][3] = -1.0
    _raises(_ffi.DW_EINVAL, r"worlds\[3\]\.g", lambda: call(t=bad))
    nan = L.copy()
    nan[2, 1] = np.nan
    _raises(_ffi.DW_EINVAL, "luminosity", lambda: call(l=nan))
    after = _everything(eng)
    for k in ("light", "dark", "idx", "st"):
        assert np.array_equal(before[k], after[k]), k
    eng.get_obs(L0)                                             # still a shared-L handle
    call()
    for fn in (lambda: eng.get_obs(L0), lambda: eng.download_caches(L0), lambda: eng.download_grid(L0),
               lambda: eng.reduce_temperature(L0)):
        _raises(_ffi.DW_ESTATE, "per-world", fn)
    eng.snapshot_save()
    eng.step(1.0, np.zeros((B, N, 1), dtype=np.int64))          # a shared-L step clears the mark ...
    eng.get_obs(1.0)
    eng.download_caches(1.0)
    eng.snapshot_restore()                                      # ... and the snapshot brings it back
    _raises(_ffi.DW_ESTATE, "per-world", lambda: eng.get_obs(L0))
    _raises(_ffi.DW_ESTATE, "per-world", lambda: eng.download_caches(L0))
    eng.close()
    for over in ({"precision": "f64"}, {"collision_mode": 1}):
        e2 = amd.Engine(_params(amd, B, H, W, N, over.get("precision", "exact"), collision_mode=over.get("collision_mode", 0)))
        e2.init_random(9, quantised=True)
        _raises(_ffi.DW_EINVAL, "precision|collision_mode",
                lambda: e2.run_episode_ensemble(np.repeat(e2.world_params()[None], B), L, _ffi.POLICY_ARGMAX))
        e2.close()


# ---------------------------------------------------------------------------------------------
# 6. the harness: the policy x albedo table in one call against one simulate_lifespan per scenario
# ---------------------------------------------------------------------------------------------
def test_lifespan_sweep_equals_one_simulate_lifespan_per_scenario(amd):
    Bs, N, dim, seed = 12, 4, 8, 21
    neutral = {"albedo_light": 0.5, "albedo_dark": 0.5}
    hot = dict(neutral, S=2000.0)                                # a scenario that dies early: the others run on
    scenarios = [{"params": {}, "agent": amd.Greedy(epsilon=0.0, greedy=True)},
                 {"params": hot, "agent": amd.Greedy(epsilon=0.0, greedy=True)},
                 {"params": {}, "agent": amd.Greedy(epsilon=0.0, greedy=False)},
                 {"params": neutral, "agent": amd.Greedy(epsilon=0.0, greedy=False)}]
    S = len(scenarios)
    env = amd.RLDaisyWorld(grid_dimension=dim, n_agents=N)
    env.batch_size = S * Bs
    env.reset_synthetic(seed)
    done_at, agents_done_at, table = amd.simulate_lifespan_sweep(env, scenarios, Bs, obs=env.get_obs())
    with pytest.raises(RuntimeError, match="reset"):
        env.step()
    env.close()
    assert done_at.shape == (S, Bs) and agents_done_at.shape == (S, Bs, N, 1) and table.shape == (S * Bs,)
    for s, sc in enumerate(scenarios):
        one = amd.RLDaisyWorld(grid_dimension=dim, n_agents=N)
        one.batch_size = Bs
        one.world_offset = s * Bs                               # the same global world ids: the same Philox worlds
        for name, value in sc["params"].items():
            setattr(one, name, value)
            assert np.all(table[name][s * Bs:(s + 1) * Bs] == value)
        one.reset_synthetic(seed)
        d, a = amd.simulate_lifespan(one, sc["agent"], obs=one.get_obs(), final_state=False)
        one.close()
        assert np.array_equal(done_at[s], d), (s, done_at[s], d)
        assert np.array_equal(agents_done_at[s], a), s
    ends = done_at.max(axis=1)
    assert ends.min() < ends.max(), ends                        # one scenario ended earlier than the others
