"""dw_run_episode_mlp_trace / Engine.run_episode_mlp(trace=, temperature=) / harness.simulate_grazing_mlp (run with
``-m gpu``): dw_run_episode_mlp that also records, for every step and world, what dw_reduce would report after that step
and the statistics of the temperature field that step computes.

  twins        two engines from the same state: `run_episode_mlp` and the traced call leave the same reward, done, planes
               (current and previous), agents, actions, `reduce()` and fixup count - with `trace` only, `temps` only, both;
  records      a third engine takes K x (`policy_mlp_population` for both halves, `step_device_actions`, `reduce()`,
               `reduce_temperature(L_t)`): the rows are equal, `reserved` is 0, the last rows are `reduce()` and
               `reduce_temperature` after the call;
  forms        the same bytes under DW_NO_EPISODE_WAVE, on a workgroup shape and with N = 5 (`kernel_info()` names the form);
  also         a call straight after an un-quantised upload (stepwise first steps, then the wave kernel: continuous rows), a
               world without cover, the error codes, and simulate_grazing_mlp against the reference's trained-agent fixture.

Every comparison of the engine cases is byte-exact and runs in both precisions.  Protocol: ``init_random(seed,
quantised=True)`` and one zero-action ``dw_step`` - the current and the retained previous state are quantised, so the whole
call runs in the form the handle names - then the schedule 0.9 + 0.002 t.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_episode_trace import L0, STEPWISE, WAVE, _assert_untouched, _engine, _schedule, _snapshot, _state_of  # noqa: E402


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


#          B, H,  W,  N, split
SHAPES = [(5, 16, 16, 4, 2),       # four slots per lane; a last workgroup with three invalid waves
          (3, 8, 8, 2, 1),         # one slot
          (2, 10, 13, 3, 3),       # 130 cells: a partly owned third slot, H != W, no adversary
          (1, 16, 16, 1, 0)]       # a single agent
KS = (1, 64, 65, 70)               # records across the 64-step segment seam
K_MAX = max(KS)
N_MEMBERS = 3
PRECISIONS = ("exact", "fast")
_ids = lambda v: str(v).replace(" ", "")  # noqa: E731


def _members(B):
    """member_a / member_b, differing per world"""
    return (np.array([0, 1, 2, 0, 1], dtype=np.int32)[:B].copy(), np.array([2, 0, 1, 1, 2], dtype=np.int32)[:B].copy())


def _params(shape):
    B, H, W, N, split = shape
    return np.random.RandomState(1000 * B + 10 * H + W + N).randn(N_MEMBERS, 1808) * 0.5


def _fresh(amd, shape, precision, monkeypatch, switch=None):
    B, H, W, N, split = shape
    eng = _engine(amd, B, H, W, N, precision, monkeypatch, switch)
    eng.init_random(500 + 7 * B + H + W + N, quantised=True)
    eng.step(L0, np.zeros((B, N, 1), dtype=np.int64))
    return eng


def _assert_form(eng, form):
    info = eng.kernel_info()
    assert f"; mlp trace: {form}" in info, info
    assert info.rsplit("; ", 1)[-1].startswith("per-world constants: "), info


def _loop(eng, shape, K, Ls, L_init=0.75):
    """K x (policy for both halves, step, reduce(), reduce_temperature(L_t)) -> (reward, done, stats, temps)"""
    from therldaisyworld_amd import _ffi
    B, H, W, N, split = shape
    ma, mb = _members(B)
    params = _params(shape)
    reward, done = np.zeros((K, B, N, 1)), np.zeros((K, B, N, 1), dtype=bool)
    stats, temps = np.zeros((K, B), dtype=_ffi.STATS_DTYPE), np.zeros((K, B), dtype=_ffi.TEMP_STATS_DTYPE)
    for t in range(K):
        eng.policy_mlp_population(params, ma, 0, split, L_init)
        eng.policy_mlp_population(params, mb, split, N, L_init)
        eng.step_device_actions(Ls[t])
        reward[t], done[t] = eng.reward_done()
        row = eng.reduce()
        for f in ("max_k", "sum_light_k", "sum_dark_k"):
            stats[f][t] = row[f]
        temps[t] = eng.reduce_temperature(Ls[t])
    return reward * (reward > 0), done, stats, temps


_REF = {}


def _reference(amd, shape, precision, monkeypatch):
    """The per-step loop's K_MAX steps, once per (shape, precision): the rows of a shorter run are its first rows."""
    key = (shape, precision)
    if key not in _REF:
        eng = _fresh(amd, shape, precision, monkeypatch)
        ref = _loop(eng, shape, K_MAX, _schedule(K_MAX))
        eng.close()
        for a in ref:
            a.flags.writeable = False
        _REF[key] = ref
    return _REF[key]


def _traced(eng, shape, K, trace=True, temperature=True, Ls=None):
    B, H, W, N, split = shape
    ma, mb = _members(B)
    return eng.run_episode_mlp(_schedule(K) if Ls is None else Ls, _params(shape), ma, mb, split, trace=trace,
                               temperature=temperature)


def _assert_rows(got, ref, K, what):
    reward, done, stats, temps = got
    r_reward, r_done, r_stats, r_temps = ref
    assert _bits(reward) == _bits(r_reward[:K]) and np.array_equal(done, r_done[:K]), f"{what}: reward / done"
    if stats is not None:
        assert not stats["reserved"].any(), f"{what}: reserved"
        assert _bits(stats) == _bits(r_stats[:K]), f"{what}: cover records"
    if temps is not None:
        assert _bits(temps) == _bits(r_temps[:K]), f"{what}: temperature rows"


def _assert_last_rows(eng, stats, temps, L_last, what):
    s = eng.reduce()
    if stats is not None:
        for f in ("max_k", "sum_light_k", "sum_dark_k"):
            assert np.array_equal(stats[f][-1], s[f]), f"{what}: the last row is not reduce() ({f})"
    if temps is not None:
        assert _bits(temps[-1]) == _bits(eng.reduce_temperature(L_last)), f"{what}: the last row is not reduce_temperature()"


# ---------------------------------------------------------------------------------------------
# 1. twin handles: everything run_episode_mlp leaves
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_twin_handles_leave_the_same(amd, monkeypatch, shape, K, precision):
    B, H, W, N, split = shape
    Ls = _schedule(K)
    ma, mb = _members(B)
    plain = _fresh(amd, shape, precision, monkeypatch)
    _assert_form(plain, WAVE)
    assert "; mlp episode: one wave per world" in plain.kernel_info()
    reward, done = plain.run_episode_mlp(Ls, _params(shape), ma, mb, split)
    want, want_fix = _state_of(plain, Ls[-1]), plain.last_fixup_count()
    plain.close()
    assert (reward > 0).any()
    for trace, temperature in ((True, False), (False, True), (True, True)):
        what = f"{shape} K={K} {precision} trace={trace} temperature={temperature}"
        eng = _fresh(amd, shape, precision, monkeypatch)
        r, d, stats, temps = _traced(eng, shape, K, trace, temperature)
        assert (stats is None) == (not trace) and (temps is None) == (not temperature)
        assert r.shape == (K, B, N, 1) and d.shape == (K, B, N, 1)
        assert _bits(r) == _bits(reward) and np.array_equal(d, done), f"{what}: reward / done"
        got, got_fix = _state_of(eng, Ls[-1]), eng.last_fixup_count()
        for name in want:
            assert np.array_equal(got[name], want[name]), f"{what}: {name}"
        assert got_fix == want_fix, f"{what}: last_fixup_count {got_fix} != {want_fix}"
        _assert_last_rows(eng, stats, temps, Ls[-1], what)
        # ... and the parameter sets stay on the device for a later params=None, as after run_episode_mlp
        eng.run_episode_mlp(Ls[:1], None, ma, mb, split, n_members=N_MEMBERS, trace=trace, temperature=temperature)
        eng.close()


# ---------------------------------------------------------------------------------------------
# 2. the records against the per-step loop
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_records_equal_the_per_step_loop(amd, monkeypatch, shape, K, precision):
    from therldaisyworld_amd import _ffi
    B = shape[0]
    what = f"{shape} K={K} {precision}"
    ref = _reference(amd, shape, precision, monkeypatch)
    assert ref[2]["max_k"].max() > 5 and (ref[3]["std"] > 0).any()          # (not a comparison of dead worlds)
    eng = _fresh(amd, shape, precision, monkeypatch)
    _assert_form(eng, WAVE)
    got = _traced(eng, shape, K)
    assert got[2].shape == (K, B) and got[2].dtype == _ffi.STATS_DTYPE
    assert got[3].shape == (K, B) and got[3].dtype == _ffi.TEMP_STATS_DTYPE
    _assert_rows(got, ref, K, what)
    _assert_last_rows(eng, got[2], got[3], _schedule(K)[-1], what)
    eng.close()


# ---------------------------------------------------------------------------------------------
# 3. both forms return the same bytes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_launches_per_step_under_the_switch(amd, monkeypatch, shape, precision):
    K = 65
    ref = _reference(amd, shape, precision, monkeypatch)
    for switch in ("DW_NO_EPISODE_WAVE", "DW_NO_EPISODE_KERNEL"):
        eng = _fresh(amd, shape, precision, monkeypatch, switch)
        _assert_form(eng, STEPWISE)
        got = _traced(eng, shape, K)
        _assert_rows(got, ref, K, f"{shape} {precision} {switch}")
        _assert_last_rows(eng, got[2], got[3], _schedule(K)[-1], f"{shape} {precision} {switch}")
        eng.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", [(2, 20, 20, 4, 2), (2, 16, 16, 5, 2)], ids=_ids)
def test_shapes_outside_the_wave_form(amd, monkeypatch, shape, precision):
    """A workgroup shape (400 cells) and N = 5 (16 N > 64): launches per step, no LDS workgroup kernel with records."""
    B, H, W, N, split = shape
    K = 9
    Ls = _schedule(K)
    what = f"{shape} {precision}"
    third = _fresh(amd, shape, precision, monkeypatch)
    ref = _loop(third, shape, K, Ls)
    third.close()
    plain = _fresh(amd, shape, precision, monkeypatch)
    assert "; mlp episode: workgroup (LDS)" in plain.kernel_info()
    ma, mb = _members(B)
    reward, done = plain.run_episode_mlp(Ls, _params(shape), ma, mb, split)
    want, want_fix = _state_of(plain, Ls[-1]), plain.last_fixup_count()
    plain.close()
    eng = _fresh(amd, shape, precision, monkeypatch)
    _assert_form(eng, STEPWISE)
    got = _traced(eng, shape, K)
    _assert_rows(got, ref, K, what)
    assert _bits(got[0]) == _bits(reward) and np.array_equal(got[1], done), f"{what}: reward / done against run_episode_mlp"
    have = _state_of(eng, Ls[-1])
    for name in want:
        assert np.array_equal(have[name], want[name]), f"{what}: {name}"
    assert eng.last_fixup_count() == want_fix
    _assert_last_rows(eng, got[2], got[3], Ls[-1], what)
    eng.close()


# ---------------------------------------------------------------------------------------------
# 4. from an un-quantised upload: stepwise first steps, the wave kernel's remainder, one continuous set of rows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES[:2], ids=_ids)
def test_from_an_unquantised_upload(amd, monkeypatch, shape, precision):
    B, H, W, N, split = shape
    K = 6
    Ls = _schedule(K)
    rng = np.random.RandomState(31 + H)
    light, dark = rng.rand(B, H, W) * 0.45, rng.rand(B, H, W) * 0.45
    idx = np.stack([rng.randint(0, H, size=(B, N)), rng.randint(0, W, size=(B, N))], axis=-1)
    st = np.ones((B, N))

    def fresh():
        eng = _engine(amd, B, H, W, N, precision, monkeypatch)
        eng.upload_state(light, dark)
        eng.upload_agents(idx, st)
        return eng

    third = fresh()
    ref = _loop(third, shape, K, Ls, L_init=L0)
    third.close()
    eng = fresh()
    _assert_form(eng, WAVE)
    ma, mb = _members(B)
    got = eng.run_episode_mlp(Ls, _params(shape), ma, mb, split, L_init=L0, trace=True, temperature=True)
    _assert_rows(got, ref, K, f"{shape} {precision} un-quantised")
    _assert_last_rows(eng, got[2], got[3], Ls[-1], f"{shape} {precision} un-quantised")
    eng.close()
    # row 0 is taken from the grazed UN-QUANTISED state: the covers' sub-per-mille digits are in it
    q = fresh()
    q.upload_state_f32(np.round(light, 3).astype(np.float32), np.round(dark, 3).astype(np.float32), quantised=True)
    q.upload_agents(idx, st)
    rounded = q.run_episode_mlp(Ls[:1], _params(shape), ma, mb, split, L_init=L0, temperature=True)[3]
    q.close()
    assert _bits(rounded[0]) != _bits(got[3][0])


# ---------------------------------------------------------------------------------------------
# 5. a world without cover
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("switch,form", [(None, WAVE), ("DW_NO_EPISODE_WAVE", STEPWISE)])
def test_a_world_without_cover_is_uniform(amd, monkeypatch, switch, form, precision):
    shape = B, H, W, N, split = SHAPES[1]
    K = 4
    eng = _engine(amd, B, H, W, N, precision, monkeypatch, switch)
    _assert_form(eng, form)
    eng.init_random(9, quantised=True)
    idx, st = eng.download_agents()
    zeros = np.zeros((B, H, W), dtype=np.float32)
    eng.upload_state_f32(zeros, zeros, quantised=True)
    eng.upload_agents(idx, st)
    eng.step(L0, np.zeros((B, N, 1), dtype=np.int64))
    _, _, stats, temps = _traced(eng, shape, K)
    eng.close()
    assert not stats["max_k"].any()
    assert (temps["std"] == 0.0).all()
    assert np.array_equal(temps["min"], temps["mean"]) and np.array_equal(temps["max"], temps["mean"])
    assert np.isfinite(temps["mean"]).all() and (temps["mean"] > 0).all()


# ---------------------------------------------------------------------------------------------
# 6. errors: checked before anything runs, the state is untouched
# ---------------------------------------------------------------------------------------------
def _raw_call(eng, K, Ls, params, n_members, stats, temps, split=1):
    from therldaisyworld_amd import _ffi
    return eng._lib.dw_run_episode_mlp_trace(
        eng._h, K, _ffi.ptr_d(Ls), _ffi.ptr_d(params), n_members, None, None, split, 0.75, None, None,
        None if stats is None else stats.ctypes.data_as(C.POINTER(_ffi.DwWorldStats)),
        None if temps is None else temps.ctypes.data_as(C.POINTER(_ffi.DwTempStats)))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_errors_leave_the_state_untouched(amd, monkeypatch, precision):
    from therldaisyworld_amd import _ffi
    shape = B, H, W, N, split = SHAPES[1]
    K = 4
    Ls = _schedule(K)
    one = np.ascontiguousarray(_params(shape)[:1])
    eng = _fresh(amd, shape, precision, monkeypatch)
    before, agents = _snapshot(eng), eng.download_agents()

    def untouched(what):
        _assert_untouched(eng, before, what)
        idx, st = eng.download_agents()
        assert np.array_equal(idx, agents[0]) and np.array_equal(st, agents[1]), f"{what}: agents changed"

    assert _raw_call(eng, K, Ls, one, 1, None, None) == _ffi.DW_EINVAL             # both outputs null
    assert b"dw_run_episode_mlp" in eng._lib.dw_last_error()
    untouched("both outputs null")
    stats = np.zeros((K, B), dtype=_ffi.STATS_DTYPE)
    temps = np.zeros((K, B), dtype=_ffi.TEMP_STATS_DTYPE)
    assert _raw_call(eng, K, Ls, None, 1, stats, temps) == _ffi.DW_ESTATE           # params=None, nothing on the device
    untouched("params=None")
    for bad in (0, 4097):
        assert _raw_call(eng, bad, _schedule(max(bad, 1)), one, 1, stats, temps) == _ffi.DW_EINVAL, bad
        untouched(f"nsteps = {bad}")
    assert _raw_call(eng, K, Ls, one, 1, stats, temps, split=N + 1) == _ffi.DW_EINVAL
    untouched("split")
    assert _raw_call(eng, K, Ls, one, 2, stats, temps) == _ffi.DW_EINVAL            # several sets need both member maps
    untouched("member maps")
    assert not stats.view(np.uint8).any() and not temps.view(np.float64).any()
    assert _raw_call(eng, K, Ls, one, 1, stats, temps) == _ffi.DW_OK                # ... and the handle still works
    assert _bits(temps[-1]) == _bits(eng.reduce_temperature(Ls[-1]))
    assert np.array_equal(stats["max_k"][-1], eng.reduce()["max_k"])
    eng.close()


# ---------------------------------------------------------------------------------------------
# 7. simulate_grazing_mlp against the reference's trained-agent rollout (fixture G11)
# ---------------------------------------------------------------------------------------------
def _g11_env(amd, g):
    """tests/test_gpu_parity.py::test_trained_mlp_rollout_on_device_matches_reference_fixture_g11's setup"""
    agent = amd.MLP()
    agent.set_parameters(g["parameters"])
    np.random.seed(11)
    amd.MLP()                                                # the fixture drew one Glorot init before the env
    env = amd.RLDaisyWorld(grid_dimension=16, n_agents=4)
    env.batch_size = 8
    obs = env.reset()
    return agent, env, obs


def test_simulate_grazing_mlp_vs_reference_fixture_g11(amd, golden):
    from therldaisyworld_amd import harness
    g = golden("G11_trained_mlp")
    n, B, N = 160, 8, 4
    agent, env, obs = _g11_env(amd, g)
    out = amd.simulate_grazing_mlp(env, agent, n, chunk=48, obs=obs, temperature=True)
    assert harness.simulate_grazing_mlp is amd.simulate_grazing_mlp
    assert out["reward"].shape == (n, B, N) and out["agent_ok"].shape == (n, B, N) and out["stats"].shape == (n, B)
    for t in range(n):
        assert np.array_equal(out["reward"][t][..., None], g["rewards"][t]), t
        assert np.array_equal(out["agent_ok"][t][..., None], ~g["dones"][t]), t
        if t % 16 == 15:
            assert np.array_equal(out["stats"]["sum_light_k"][t], np.rint(g["mean_light"][t] * 256000).astype(np.uint64)), t
            assert np.array_equal(out["stats"]["sum_dark_k"][t], np.rint(g["mean_dark"][t] * 256000).astype(np.uint64)), t
    assert np.array_equal(out["agents_alive"], out["agent_ok"].sum(axis=2))
    assert np.array_equal(env.grid, g["grid_final"])
    assert np.array_equal(env.agent_indices, g["agent_indices_final"])
    assert env.L == float(g["L_final"])
    assert env.step_count == n
    env.close()

    # the temperature curve against a plain env.step loop on a second environment (the fixture's actions), at the
    # tolerance tests/test_gpu_episode_temperature.py asserts for the mean of a row against the float64 field
    _, env2, _ = _g11_env(amd, g)
    for t in range(n):
        assert out["L"][t] == env2.L, t
        env2.step(g["actions"][t])
        mean = np.asarray(env2.temp).mean(axis=(-2, -1)).reshape(B)
        np.testing.assert_allclose(out["mean_temp"][t], mean, rtol=2e-12, atol=0, err_msg=f"step {t}")
    np.testing.assert_allclose(out["dead_temp"], harness.dead_temperature(env2, out["L"]), rtol=0, atol=0)
    assert np.array_equal(env2.grid, g["grid_final"])
    env2.close()
