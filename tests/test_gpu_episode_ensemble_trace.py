"""GPU tests (``-m gpu``) of dw_run_episode_ensemble_trace / Engine.run_episode_ensemble(trace=, temperature=) /
harness.simulate_grazing_sweep: the device-resident episode loop with physics constants and a luminosity column of its own
for every world that also records, for every step and world, what dw_reduce would report and the statistics of the
temperature field the step computes.

The contract is independence, in bytes: column b of the records and of the temperature rows is what a ONE-world handle
that holds world b and its agents (world_offset = b), carries the world's constants (dw_set_params) and is given column b
of the schedule and slice [:, b] of the table gets from dw_run_episode_trace_temperature; and everything
dw_run_episode_ensemble leaves for the same arguments - planes, retained previous planes, agents, reduce(), the device
action buffer, the fix-up count, the flags - this call leaves too.  Both forms of the call (one wave per world, launches
per step) return the same bytes.

Protocol, inputs and helpers are those of tests/test_gpu_episode_ensemble.py: ``init_random(seed)``, one zero-action
``dw_step`` at the handle's own constants, then the call under test; every case asserts its form from ``kernel_info()``.
"""
import ctypes as C
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import daisy_oracle as O  # noqa: E402
from test_gpu_episode_ensemble import (FIELDS, L0, STEPWISE, THRESHOLD_K, WAVE, _engine, _everything, _inputs, _k, _params,  # noqa: E402
                                       _raises, _resolve_codes, _schedule, _table)
from test_gpu_episode_temperature import _assert_rows_close  # noqa: E402

STATE = ("light", "dark", "prev_light", "prev_dark", "idx", "st", "action")


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _quantise(eng):
    eng.step(L0, np.zeros((eng.B, eng.N, 1), dtype=np.int64) if eng.N else None)


def _assert_form(eng, form):
    info = eng.kernel_info()
    assert f"; ensemble trace: {form}" in info, info
    assert f"; episode temperature: {form}; ensemble trace: {form}" in info, info
    assert info.rsplit("; ", 1)[-1].startswith("per-world constants: "), info
    assert len(info) < 1023, len(info)                          # (Engine.kernel_info passes 1024 bytes)


def _fresh(amd, monkeypatch, shape, precision, switch, seed):
    B, H, W, N = shape
    eng = _engine(amd, B, H, W, N, precision, monkeypatch, switch)
    eng.init_random(seed)
    _quantise(eng)
    return eng


def _one_world_traces(amd, monkeypatch, switch, shape, precision, seed, tab, L, mode, ut, codes):
    """The reference of the contract: world b alone on a one-world handle with its constants, its column and its table
    slice, through run_episode_trace(temperature=True).  Returns (stats (K, B), temps (K, B))."""
    from therldaisyworld_amd import _ffi
    B, H, W, N = shape
    stats, temps = [], []
    for b in range(B):
        one = _engine(amd, 1, H, W, N, precision, monkeypatch, switch, world_offset=b)
        one.init_random(seed)
        _quantise(one)
        p = _params(amd, 1, H, W, N, precision, world_offset=b)
        for name in _ffi.WORLD_PARAM_NAMES:
            setattr(p, name, float(tab[b][name]))
        one.set_params(p)
        s, _, _, t = one.run_episode_trace(np.ascontiguousarray(L[:, b]), mode, ut, np.ascontiguousarray(codes[:, b:b + 1]),
                                           threshold_k=THRESHOLD_K, temperature=True)
        one.close()
        stats.append(s)
        temps.append(t)
    return np.concatenate(stats, axis=1), np.concatenate(temps, axis=1)


def _independence(amd, monkeypatch, shape, precision, K, switch, form):
    from therldaisyworld_amd import _ffi
    B, H, W, N = shape
    what = f"{shape} {precision} K={K} {switch or 'default'}"
    seed, mode = 31, _ffi.POLICY_ARGMAX
    eng = _fresh(amd, monkeypatch, shape, precision, switch, seed)
    _assert_form(eng, form)
    tab = _table(eng, B)
    L = _schedule(K, B)
    codes, ut = _inputs(K, B, N, 7 * B + K)
    alive, ok, stats, temps = eng.run_episode_ensemble(tab, L, mode, ut, codes, threshold_k=THRESHOLD_K, trace=True,
                                                       temperature=True)
    got = _everything(eng)
    eng.close()
    assert stats.shape == (K, B) and temps.shape == (K, B) and alive.shape == (K, B) and ok.shape == (K, B, N)
    assert (temps["std"] > 0).any() and np.isfinite(temps.view(np.float64)).all(), f"{what}: nothing is alive"
    assert not stats["reserved"].any()
    assert np.array_equal(alive, stats["max_k"] > THRESHOLD_K), f"{what}: world_alive against the records"
    for f in FIELDS:
        assert np.array_equal(stats[f][-1], got["reduce"][f]), f"{what}: the last row is not reduce() {f}"

    rstats, rtemps = _one_world_traces(amd, monkeypatch, switch, shape, precision, seed, tab, L, mode, ut, codes)
    for b in range(B):
        assert _bits(stats[:, b]) == _bits(rstats[:, b]), f"{what}: cover records of world {b}"
        assert _bits(temps[:, b]) == _bits(rtemps[:, b]), (what, b, np.argwhere(temps[:, b] != rtemps[:, b])[:3].tolist())

    twin = _fresh(amd, monkeypatch, shape, precision, switch, seed)            # the call without records
    ralive, rok = twin.run_episode_ensemble(tab, L, mode, ut, codes, threshold_k=THRESHOLD_K)
    want = _everything(twin)
    twin.close()
    assert np.array_equal(alive, ralive) and np.array_equal(ok, rok), f"{what}: flags"
    for k in STATE:
        assert np.array_equal(got[k], want[k]), (what, k)
    assert _bits(got["reduce"]) == _bits(want["reduce"]), f"{what}: reduce()"
    assert got["fix"] == want["fix"], f"{what}: fix-up count {got['fix']} != {want['fix']}"


# ---------------------------------------------------------------------------------------------
# 1. independence, one wave per world, bytes: cells on every pattern of the four slots, agents on every lane
# ---------------------------------------------------------------------------------------------
WAVE_SHAPES = [(6, 8, 8, 4),        # one full slot; a full and a half-filled block
               (5, 5, 13, 3),       # 65 cells: one in slot 1
               (3, 10, 10, 3),      # a partial slot 1
               (6, 16, 16, 4),      # four slots
               (2, 16, 16, 64),     # every lane an agent
               (3, 8, 8, 0)]        # no agents
CASES_1 = [(s, 70) for s in WAVE_SHAPES] + [(WAVE_SHAPES[0], K) for K in (1, 64, 65, 130)]


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("shape,K", CASES_1, ids=lambda v: str(v).replace(" ", ""))
def test_wave_form_records_every_world_as_if_alone(amd, monkeypatch, shape, K, precision):
    _independence(amd, monkeypatch, shape, precision, K, None, WAVE)


# ---------------------------------------------------------------------------------------------
# 2. twins: the other forms of the same call, and the call with one kind of record only
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("shape", [(6, 8, 8, 4), (3, 10, 10, 3), (3, 8, 8, 0)], ids=lambda v: str(v).replace(" ", ""))
def test_twins_return_identical_bytes(amd, monkeypatch, shape, precision):
    from therldaisyworld_amd import _ffi
    B, H, W, N = shape
    K, seed, mode = 70, 31, _ffi.POLICY_ARGMAX
    what = f"{shape} {precision}"
    L = _schedule(K, B)
    codes, ut = _inputs(K, B, N, 7 * B + K)

    def run(switch, form, **kw):
        eng = _fresh(amd, monkeypatch, shape, precision, switch, seed)
        _assert_form(eng, form)
        out = eng.run_episode_ensemble(_table(eng, B), L, mode, ut, codes, threshold_k=THRESHOLD_K, **kw)
        state = _everything(eng)
        eng.close()
        return out, state

    (alive, ok, stats, temps), got = run(None, WAVE, trace=True, temperature=True)
    assert stats["max_k"].max() > THRESHOLD_K and (temps["std"] > 0).any()
    for switch in ("DW_NO_EPISODE_WAVE", "DW_NO_EPISODE_KERNEL"):
        (a2, o2, s2, t2), twin = run(switch, STEPWISE, trace=True, temperature=True)
        assert _bits(t2) == _bits(temps), f"{what}: temps under {switch}"
        assert _bits(s2) == _bits(stats), f"{what}: trace under {switch}"
        assert np.array_equal(a2, alive) and np.array_equal(o2, ok), f"{what}: flags under {switch}"
        for k in STATE:
            assert np.array_equal(got[k], twin[k]), (what, switch, k)
        for f in FIELDS:                                            # (reserved: the kernel family's count, not compared)
            assert np.array_equal(got["reduce"][f], twin["reduce"][f]), (what, switch, f)
    for switch, form in ((None, WAVE), ("DW_NO_EPISODE_WAVE", STEPWISE)):
        (a3, o3, s3, t3), only = run(switch, form, trace=True)
        assert t3 is None and _bits(s3) == _bits(stats), f"{what}: trace alone, {form}"
        assert np.array_equal(a3, alive) and np.array_equal(o3, ok)
        (a4, o4, s4, t4), only2 = run(switch, form, temperature=True)
        assert s4 is None and _bits(t4) == _bits(temps), f"{what}: temps alone, {form}"
        assert np.array_equal(a4, alive) and np.array_equal(o4, ok)
        for k in STATE:
            assert np.array_equal(got[k], only[k]) and np.array_equal(got[k], only2[k]), (what, form, k)


# ---------------------------------------------------------------------------------------------
# 3. exact mode against the float64 oracle, world by world with the world's attributes
# ---------------------------------------------------------------------------------------------
def test_exact_mode_matches_the_oracle_with_each_worlds_attributes(amd, monkeypatch):
    from therldaisyworld_amd import _ffi
    B, H, W, N, K = 5, 8, 8, 4, 70                              # B = 5: every kind of _table
    eng = _engine(amd, B, H, W, N, "exact", monkeypatch)
    _assert_form(eng, WAVE)
    tab = _table(eng, B)
    L = _schedule(K, B)
    codes, ut = _inputs(K, B, N, 99)
    eng.init_random(17)
    _quantise(eng)
    light, dark = eng.download_planes()
    idx, st = eng.download_agents()
    alive, ok, stats, temps = eng.run_episode_ensemble(tab, L, _ffi.POLICY_ARGMIN, ut, codes, threshold_k=THRESHOLD_K,
                                                       trace=True, temperature=True)
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
            kl, kd = _k(env.grid[:, 1]), _k(env.grid[:, 2])
            assert stats["max_k"][t, b] == max(kl.max(), kd.max()), f"world {b}: max_k[{t}]"
            assert stats["sum_light_k"][t, b] == kl.sum() and stats["sum_dark_k"][t, b] == kd.sum(), f"world {b}: sums[{t}]"
            assert alive[t, b] == (max(kl.max(), kd.max()) > THRESHOLD_K), f"world {b}: world_alive[{t}]"
            assert np.array_equal(ok[t, b], ~done[0, :, 0]), f"world {b}: agent_ok[{t}]"
            _assert_rows_close(temps[t, b:b + 1], np.asarray(env.temp).reshape(1, H, W), f"world {b}: temps[{t}]")
        assert np.array_equal(_k(gl[b]), _k(env.grid[0, 1])), f"world {b}: light plane"
        assert np.array_equal(_k(gd[b]), _k(env.grid[0, 2])), f"world {b}: dark plane"
        assert np.array_equal(gidx[b], env.agent_indices[0]), f"world {b}: agent positions"
        assert np.array_equal(gst[b], env.agent_states[0, :, 0]), f"world {b}: agent states"
    eng.close()


# ---------------------------------------------------------------------------------------------
# 4. launches per step on shapes outside the wave form: the generic per-world step | the per-world wave strips
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("shape", [(3, 20, 20, 2), (2, 40, 256, 2)], ids=lambda v: str(v).replace(" ", ""))
def test_launches_per_step_record_every_world_as_if_alone(amd, monkeypatch, shape, precision):
    _independence(amd, monkeypatch, shape, precision, 5, None, STEPWISE)


# ---------------------------------------------------------------------------------------------
# 5. a second launch writes its flags and records behind the first one's
# ---------------------------------------------------------------------------------------------
def test_wave_form_continues_in_a_second_launch(amd, monkeypatch):
    """2000 worlds leave 64 steps of rows per launch: K = 70 takes a second launch of 6 steps, whose flags, records and
    temperature rows start at row 64 of their blocks.  Reference: the same call as launches per step."""
    from therldaisyworld_amd import _ffi
    shape, K = (2000, 8, 8, 2), 70
    B, H, W, N = shape
    assert (32 << 20) // (136 * B) // 64 * 64 < K
    L = _schedule(K, B)
    codes, ut = _inputs(K, B, N, 11)
    outs = []
    for switch, form in ((None, WAVE), ("DW_NO_EPISODE_WAVE", STEPWISE)):
        eng = _fresh(amd, monkeypatch, shape, "exact", switch, 31)
        _assert_form(eng, form)
        out = eng.run_episode_ensemble(_table(eng, B), L, _ffi.POLICY_ARGMIN, ut, codes, threshold_k=THRESHOLD_K, trace=True,
                                       temperature=True)
        outs.append((out, _everything(eng)))
        eng.close()
    ((alive, ok, stats, temps), got), ((ralive, rok, rstats, rtemps), ref) = outs
    assert ralive[64:].any() and rok[64:].any() and (rtemps["std"][64:] > 0).any(), "rows 64... are all dead"
    assert _bits(stats) == _bits(rstats), "trace"
    assert _bits(temps) == _bits(rtemps), "temps"
    assert np.array_equal(alive, ralive) and np.array_equal(ok, rok)
    for k in STATE:
        assert np.array_equal(got[k], ref[k]), k
    for f in FIELDS:
        assert np.array_equal(got["reduce"][f], ref["reduce"][f]), f


# ---------------------------------------------------------------------------------------------
# 6. the degenerate table: the handle's own constants for every world, one luminosity per step
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["exact", "fast"])
def test_degenerate_table_equals_run_episode_trace(amd, monkeypatch, precision):
    from therldaisyworld_amd import _ffi
    shape = B, H, W, N = 6, 8, 8, 4
    K = 70
    Ls = np.linspace(0.9, 1.3, K)
    codes, ut = _inputs(K, B, N, 5)
    eng = _fresh(amd, monkeypatch, shape, precision, None, 3)
    _assert_form(eng, WAVE)
    tab = np.repeat(eng.world_params()[None], B)
    alive, ok, stats, temps = eng.run_episode_ensemble(tab, np.repeat(Ls[:, None], B, axis=1), _ffi.POLICY_ARGMAX, ut, codes,
                                                       THRESHOLD_K, trace=True, temperature=True)
    got = _everything(eng)
    eng.close()
    twin = _fresh(amd, monkeypatch, shape, precision, None, 3)
    rstats, ralive, rok, rtemps = twin.run_episode_trace(Ls, _ffi.POLICY_ARGMAX, ut, codes, threshold_k=THRESHOLD_K,
                                                         temperature=True)
    ref = _everything(twin)
    twin.close()
    assert _bits(stats) == _bits(rstats) and _bits(temps) == _bits(rtemps)
    assert np.array_equal(alive, ralive) and np.array_equal(ok, rok)
    for k in STATE:
        assert np.array_equal(got[k], ref[k]), k
    assert _bits(got["reduce"]) == _bits(ref["reduce"]) and got["fix"] == ref["fix"]


# ---------------------------------------------------------------------------------------------
# 7. a dead world
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch,form", [(None, WAVE), ("DW_NO_EPISODE_WAVE", STEPWISE)])
def test_a_dead_world_is_uniform_at_its_own_lifeless_temperature(amd, monkeypatch, switch, form):
    from therldaisyworld_amd import _ffi, harness
    shape = B, H, W, N = 5, 8, 8, 2
    K = 3
    eng = _engine(amd, B, H, W, N, "exact", monkeypatch, switch)
    _assert_form(eng, form)
    eng.init_random(9)
    idx, st = eng.download_agents()
    zeros = np.zeros((B, H, W), dtype=np.float32)
    eng.upload_state_f32(zeros, zeros, quantised=True)
    eng.upload_agents(idx, st)
    tab = _table(eng, B)
    tab["S"][1], tab["albedo_bare"][2], tab["sigma"][3] = 1200.0, 0.4, 6.0e-8    # each world's own lifeless temperature
    L = _schedule(K, B)
    alive, ok, stats, temps = eng.run_episode_ensemble(tab, L, _ffi.POLICY_ARGMAX, threshold_k=THRESHOLD_K, trace=True,
                                                       temperature=True)
    eng.close()
    assert not stats["max_k"].any() and not alive.any()
    assert (temps["std"] == 0.0).all()
    assert np.array_equal(temps["min"], temps["mean"]) and np.array_equal(temps["max"], temps["mean"])
    for b in range(B):
        w = types.SimpleNamespace(S=float(tab["S"][b]), albedo_bare=float(tab["albedo_bare"][b]), sigma=float(tab["sigma"][b]))
        np.testing.assert_allclose(temps["mean"][:, b], harness.dead_temperature(w, L[:, b]), rtol=1e-12, atol=0)
    assert len(set(temps["mean"][0].tolist())) == B            # (the worlds do differ)


# ---------------------------------------------------------------------------------------------
# 8. errors: checked before anything runs, the state is untouched; the per-world marks
# ---------------------------------------------------------------------------------------------
def _raw_call(eng, K, tab, L, stats, temps):
    from therldaisyworld_amd import _ffi
    return eng._lib.dw_run_episode_ensemble_trace(
        eng._h, K, tab.ctypes.data_as(C.POINTER(_ffi.DwWorldParams)), _ffi.ptr_d(L), _ffi.POLICY_ARGMAX, None, None, THRESHOLD_K,
        None, None, None if stats is None else stats.ctypes.data_as(C.POINTER(_ffi.DwWorldStats)),
        None if temps is None else temps.ctypes.data_as(C.POINTER(_ffi.DwTempStats)))


def test_errors_leave_the_state_untouched_and_marks_are_kept(amd, monkeypatch):
    from therldaisyworld_amd import _ffi
    B, H, W, N, K = 6, 8, 8, 4, 4
    eng = _engine(amd, B, H, W, N, "exact", monkeypatch)
    tab = _table(eng, B)
    L = _schedule(K, B)
    eng.init_random(9)
    stats = np.zeros((4097, B), dtype=_ffi.STATS_DTYPE)
    temps = np.zeros((4097, B), dtype=_ffi.TEMP_STATS_DTYPE)

    def unwritten():
        return not stats.view(np.uint8).any() and not temps.view(np.uint8).any()

    call = lambda t=tab, l=L: eng.run_episode_ensemble(t, l, _ffi.POLICY_ARGMAX, trace=True, temperature=True)
    _raises(_ffi.DW_ESTATE, "not quantised", call)              # the un-quantised initial state
    assert _raw_call(eng, K, tab, L, stats, temps) == _ffi.DW_ESTATE and unwritten()
    _quantise(eng)
    before = _everything(eng)

    def untouched(what):
        after = _everything(eng)
        for k in ("light", "dark", "prev_light", "prev_dark", "idx", "st"):
            assert np.array_equal(before[k], after[k]), (what, k)
        assert unwritten(), what

    assert _raw_call(eng, K, tab, L, None, None) == _ffi.DW_EINVAL
    assert b"dw_run_episode_ensemble" in eng._lib.dw_last_error()
    untouched("no record array")
    bad = tab.copy()
    bad["g"][3] = -1.0
    _raises(_ffi.DW_EINVAL, r"worlds\[3\]\.g", lambda: call(t=bad))
    assert _raw_call(eng, K, bad, L, stats, temps) == _ffi.DW_EINVAL
    untouched("g < 0")
    nan = L.copy()
    nan[2, 1] = np.nan
    _raises(_ffi.DW_EINVAL, "luminosity", lambda: call(l=nan))
    assert _raw_call(eng, K, tab, nan, stats, temps) == _ffi.DW_EINVAL
    untouched("NaN luminosity")
    long_L = _schedule(4097, B)
    for n in (0, 4097):
        assert _raw_call(eng, n, tab, long_L, stats, temps) == _ffi.DW_EINVAL, n
        untouched(f"nsteps = {n}")
    eng.get_obs(L0)                                             # still a shared-L handle
    alive, ok, s, t = call()                                    # ... and a valid call works
    assert np.array_equal(alive, s["max_k"] > THRESHOLD_K) and np.isfinite(t.view(np.float64)).all()
    for fn in (lambda: eng.get_obs(L0), lambda: eng.reduce_temperature(L0)):
        _raises(_ffi.DW_ESTATE, "per-world", fn)
    eng.snapshot_save()
    eng.step(1.0, np.zeros((B, N, 1), dtype=np.int64))          # a shared-L step clears the mark ...
    eng.get_obs(1.0)
    eng.reduce_temperature(1.0)
    eng.snapshot_restore()                                      # ... and the snapshot brings it back
    _raises(_ffi.DW_ESTATE, "per-world", lambda: eng.get_obs(L0))
    eng.close()
    for over in ({"precision": "f64"}, {"collision_mode": 1}):
        e2 = amd.Engine(_params(amd, B, H, W, N, over.get("precision", "exact"), collision_mode=over.get("collision_mode", 0)))
        e2.init_random(9, quantised=True)
        planes = e2.download_planes()
        _raises(_ffi.DW_EINVAL, "precision|collision_mode",
                lambda: e2.run_episode_ensemble(np.repeat(e2.world_params()[None], B), L, _ffi.POLICY_ARGMAX, trace=True,
                                                temperature=True))
        assert all(np.array_equal(a, b) for a, b in zip(planes, e2.download_planes()))
        e2.close()


def test_kernel_info_keeps_its_last_fragment_on_the_longest_shape(amd, monkeypatch):
    """A seam-strip shape with a switch set has the longest description: the new fragment must not push the last one
    ("; per-world constants: ...", which other tests split on) out of the 1024 bytes Engine.kernel_info passes."""
    for precision in ("fast", "exact"):
        eng = _engine(amd, 1, 8, 4096, 0, precision, monkeypatch, "DW_NO_EPISODE_WAVE")
        info = eng.kernel_info()
        eng.close()
        assert "switches[" in info and "; episode temperature: launches per step; ensemble trace: launches per step" in info, info
        assert info.rsplit("; ", 1)[-1] in ("per-world constants: step pairs", "per-world constants: wave strips",
                                            "per-world constants: generic"), info
        assert len(info.encode()) < 1023, len(info.encode())


# ---------------------------------------------------------------------------------------------
# 9. the harness: the scenarios' curves in one call against one simulate_grazing per scenario
# ---------------------------------------------------------------------------------------------
def test_grazing_sweep_equals_one_simulate_grazing_per_scenario(amd):
    Bs, N, dim, seed, n, chunk = 12, 4, 8, 21, 40, 16
    neutral = {"albedo_light": 0.5, "albedo_dark": 0.5}
    hot = dict(neutral, S=2000.0)
    scenarios = [{"params": {}, "agent": amd.Greedy(epsilon=0.0, greedy=True)},
                 {"params": hot, "agent": amd.Greedy(epsilon=0.0, greedy=True)},
                 {"params": {}, "agent": amd.Greedy(epsilon=0.0, greedy=False)},
                 {"params": neutral, "agent": amd.Greedy(epsilon=0.0, greedy=False)}]
    S = len(scenarios)

    def sweep(temperature):
        env = amd.RLDaisyWorld(grid_dimension=dim, n_agents=N)
        env.batch_size = S * Bs
        env.reset_synthetic(seed)
        out = amd.simulate_grazing_sweep(env, scenarios, Bs, n, chunk=chunk, obs=env.get_obs(), temperature=temperature)
        with pytest.raises(RuntimeError, match="reset"):
            env.step()
        env.close()
        return out

    out = sweep(True)
    temp_keys = {"mean_temp", "std_temp", "min_temp", "max_temp", "dead_temp"}
    assert out["L"].shape == (n,) and out["params"].shape == (S * Bs,)
    for key in ("mean_light", "mean_dark", "max_cover", "alive", "stats", "agents_alive") + tuple(temp_keys):
        assert out[key].shape == (n, S, Bs), key
    assert out["agent_ok"].shape == (n, S, Bs, N)
    assert out["alive"].any() and (out["std_temp"] > 0).any()
    for s, sc in enumerate(scenarios):
        one = amd.RLDaisyWorld(grid_dimension=dim, n_agents=N)
        one.batch_size = Bs
        one.world_offset = s * Bs                               # the same global world ids: the same Philox worlds
        for name, value in sc["params"].items():
            setattr(one, name, value)
        one.reset_synthetic(seed)
        ref = amd.simulate_grazing(one, sc["agent"], n, chunk=chunk, obs=one.get_obs(), temperature=True)
        one.close()
        assert set(ref) | {"params"} == set(out)
        assert _bits(ref["L"]) == _bits(out["L"])
        for key in ref:
            if key == "L":
                continue
            want = np.repeat(ref[key][:, None], Bs, axis=1) if key == "dead_temp" else ref[key]
            assert _bits(out[key][:, s]) == _bits(want), (s, key)

    plain = sweep(False)                                        # the same dict minus the temperature keys
    assert set(plain) == set(out) - temp_keys
    for key in plain:
        assert _bits(plain[key]) == _bits(out[key]), key
