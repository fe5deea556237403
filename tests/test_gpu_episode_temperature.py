"""dw_run_episode_trace_temperature / Engine.run_episode_trace(temperature=True) / harness.simulate_grazing(temperature=True)
(run with ``-m gpu``): dw_run_episode_trace that also records, for every step and world, the statistics of the temperature
field that step computes - from the state after the step's grazing and before its growth (the reference's ``env.temp``
after the t-th ``env.step(action)``).

  oracle       every row against the float64 oracle's field, at the tolerances tests/test_gpu_temperature.py asserts for
               the on-demand reduction (mean rtol 2e-12, min / max rtol 1e-12, |d std| <= 2e-12 max); exact mode: also the
               planes, agents, flags and cover records by equality;
  twins        both precisions, bytes: the wave form against engines under DW_NO_EPISODE_WAVE and DW_NO_EPISODE_KERNEL,
               against `run_episode_trace` (everything that call leaves), against `reduce_temperature` after the call
               and against K x (`run_episode` of one step, `reduce_temperature`);
  also         shapes outside the wave form, a dead world, batch independence, the error codes and simulate_grazing
               against the notebook's loop on the oracle.

The shapes put the world's cells on every pattern of the wave's four 64-cell slots.  Protocol, inputs and helpers are those
of tests/test_gpu_episode_trace.py: ``init_random``, one zero-action ``dw_step``, the schedule 0.9 + 0.002 t; every case
asserts its form from ``kernel_info()``.
"""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import daisy_oracle as O  # noqa: E402
from test_gpu_episode_trace import (L0, STEPWISE, THRESHOLD_K, WAVE, _assert_untouched, _check_invariants, _codes_of_step,  # noqa: E402
                                    _engine, _inputs, _k, _oracle_step, _quantise, _record, _resolve_codes, _schedule,
                                    _snapshot, _state_of)


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _assert_rows_close(rec, temp, what):
    """rec: (B,) temperature records; temp: the oracle's field (B, H, W) - the bounds of
    tests/test_gpu_temperature.py::_assert_close_to_oracle."""
    mean, std = temp.mean(axis=(1, 2)), temp.std(axis=(1, 2))
    mn, mx = temp.min(axis=(1, 2)), temp.max(axis=(1, 2))
    np.testing.assert_allclose(rec["mean"], mean, rtol=2e-12, atol=0, err_msg=what)
    np.testing.assert_allclose(rec["min"], mn, rtol=1e-12, atol=0, err_msg=what)
    np.testing.assert_allclose(rec["max"], mx, rtol=1e-12, atol=0, err_msg=what)
    err = np.abs(rec["std"] - std)
    assert (err <= 2e-12 * mx).all(), (what, err, mx)


def _assert_form(eng, form):
    info = eng.kernel_info()
    assert f"; episode temperature: {form}" in info, info
    assert f"; episode trace: {form}" in info, info
    assert info.rsplit("; ", 1)[-1].startswith("per-world constants: "), info


#          B, H,  W,  N
SHAPES = [(5, 8, 8, 4),        # one full slot
          (3, 5, 7, 2),        # a partial slot 0, rectangular
          (3, 10, 10, 3),      # a partial slot 1
          (2, 16, 16, 16),     # four full slots
          (2, 16, 16, 64),     # every lane an agent
          (3, 8, 8, 0)]        # N = 0
KS = {SHAPES[0]: (1, 64, 65, 130)}      # run lengths around the 64-step segment; K = 65 elsewhere
POLICIES = ("argmax", "zeros", "mixed")

_REF = {}


def _reference(env, shape, K, policy):
    """The oracle's K steps from the quantised state `env` holds: the cover record, the flags and the temperature field
    of every step (env.temp after the step: computed from the grazed state), and the final state - once per case, shared
    by the runs that start from the same state (asserted), never modified."""
    from therldaisyworld_amd import _ffi
    key = (shape, K, policy)
    start = (_k(env.grid[:, 1]), _k(env.grid[:, 2]), env.agent_indices.copy())
    if key in _REF:
        ref = _REF[key]
        assert all(np.array_equal(a, b) for a, b in zip(start, ref["start"])), "the shared reference starts elsewhere"
        return ref
    B, H, W, N = shape
    mode, ut, codes = _inputs(shape, K, policy)
    Ls = _schedule(K)
    stats = np.zeros((K, B), dtype=_ffi.STATS_DTYPE)
    alive = np.zeros((K, B), dtype=bool)
    ok = np.zeros((K, B, N), dtype=bool)
    temp = np.zeros((K, B, H, W))
    for t in range(K):
        action = _resolve_codes(env, _codes_of_step(shape, mode, ut, codes, t))
        reward, done, pl, pd = _oracle_step(env, Ls[t], action)
        temp[t] = np.asarray(env.temp).reshape(B, H, W)
        stats["max_k"][t], stats["sum_light_k"][t], stats["sum_dark_k"][t] = _record(env)
        alive[t] = stats["max_k"][t] > THRESHOLD_K
        if N:
            ok[t] = ~done[..., 0]
    ref = {"start": start, "stats": stats, "alive": alive, "ok": ok, "temp": temp, "light": _k(env.grid[:, 1]),
           "dark": _k(env.grid[:, 2]), "prev_light": _k(pl), "prev_dark": _k(pd)}
    if N:
        ref.update(idx=env.agent_indices.copy(), st=env.agent_states.copy(), reward=reward.copy(), done=done.copy(),
                   obs=env.get_obs(env.agent_indices), action=np.asarray(action)[..., 0].astype(np.int64))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    _REF[key] = ref
    return ref


def _run_vs_oracle(amd, monkeypatch, shape, K, policy, switch, form):
    B, H, W, N = shape
    what = f"{shape} K={K} {policy} {switch or 'default'}"
    eng = _engine(amd, B, H, W, N, "exact", monkeypatch, switch)
    _assert_form(eng, form)
    eng.init_random(300 + 7 * B + H + W + N)
    env = _quantise(eng, L0)
    ref = _reference(env, shape, K, policy)
    mode, ut, codes = _inputs(shape, K, policy)
    Ls = _schedule(K)
    stats, alive, ok, temps = eng.run_episode_trace(Ls, mode, ut, codes, threshold_k=THRESHOLD_K, temperature=True)
    assert stats.shape == (K, B) and alive.shape == (K, B) and ok.shape == (K, B, N) and temps.shape == (K, B)
    for t in range(K):
        _assert_rows_close(temps[t], ref["temp"][t], f"{what}: temps[{t}]")
        for f in ("max_k", "sum_light_k", "sum_dark_k"):
            assert np.array_equal(stats[f][t], ref["stats"][f][t]), f"{what}: {f}[{t}]"
        assert np.array_equal(alive[t], ref["alive"][t]), f"{what}: world_alive[{t}]"
        assert np.array_equal(ok[t], ref["ok"][t]), f"{what}: agent_ok[{t}]"
    _check_invariants(eng, stats, alive, what)
    assert _bits(temps[-1]) == _bits(eng.reduce_temperature(Ls[-1])), f"{what}: the last row is not reduce_temperature()"
    got = _state_of(eng, Ls[-1])
    for name in got:
        if not name.startswith("reduce_"):
            assert np.array_equal(got[name], ref[name]), f"{what}: {name}"
    eng.close()


# ---------------------------------------------------------------------------------------------
# 1. the wave form, exact mode, against the oracle
# ---------------------------------------------------------------------------------------------
CASES_1 = [(s, K, pol) for s in SHAPES for K in KS.get(s, (65,)) for pol in POLICIES if s[3] or pol != "mixed"]


@pytest.mark.parametrize("shape,K,policy", CASES_1, ids=lambda v: str(v).replace(" ", ""))
def test_wave_form_vs_oracle(amd, monkeypatch, shape, K, policy):
    _run_vs_oracle(amd, monkeypatch, shape, K, policy, None, WAVE)


# ---------------------------------------------------------------------------------------------
# 2. twins, both precisions, bytes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_twins_return_identical_bytes(amd, monkeypatch, shape, precision):
    B, H, W, N = shape
    K = max(KS.get(shape, (65,)))
    what = f"{shape} K={K} {precision}"
    mode, ut, codes = _inputs(shape, K, "mixed" if N else "argmax")
    Ls = _schedule(K)

    def fresh(switch=None):
        eng = _engine(amd, B, H, W, N, precision, monkeypatch, switch)
        eng.init_random(41 + H)
        eng.step(L0, np.zeros((B, N, 1), dtype=np.int64) if N else None)
        return eng

    eng = fresh()
    _assert_form(eng, WAVE)
    stats, alive, ok, temps = eng.run_episode_trace(Ls, mode, ut, codes, threshold_k=THRESHOLD_K, temperature=True)
    _check_invariants(eng, stats, alive, what)
    got, got_fix = _state_of(eng, Ls[-1]), eng.last_fixup_count()
    assert _bits(temps[-1]) == _bits(eng.reduce_temperature(Ls[-1])), f"{what}: the last row is not reduce_temperature()"
    eng.close()
    assert stats["max_k"].max() > THRESHOLD_K                   # (not a comparison of dead worlds)
    assert (temps["std"] > 0).any() and np.isfinite(temps.view(np.float64)).all()

    for switch in ("DW_NO_EPISODE_WAVE", "DW_NO_EPISODE_KERNEL"):   # the other form of the same call
        twin = fresh(switch)
        _assert_form(twin, STEPWISE)
        s2, a2, o2, t2 = twin.run_episode_trace(Ls, mode, ut, codes, threshold_k=THRESHOLD_K, temperature=True)
        twin.close()
        assert _bits(t2) == _bits(temps), f"{what}: temps under {switch}"
        assert _bits(s2) == _bits(stats) and np.array_equal(a2, alive) and np.array_equal(o2, ok), f"{what}: records under {switch}"

    twin = fresh()                                                  # the call without temperature records
    s3, a3, o3 = twin.run_episode_trace(Ls, mode, ut, codes, threshold_k=THRESHOLD_K)
    want, want_fix = _state_of(twin, Ls[-1]), twin.last_fixup_count()
    twin.close()
    assert _bits(s3) == _bits(stats) and np.array_equal(a3, alive) and np.array_equal(o3, ok), f"{what}: records, flags"
    for name in want:
        assert np.array_equal(got[name], want[name]), f"{what}: {name}"
    assert got_fix == want_fix, f"{what}: last_fixup_count {got_fix} != {want_fix}"

    twin = fresh()                                                  # single steps, the on-demand reduction after each
    for t in range(K):
        twin.run_episode(Ls[t:t + 1], mode, None if ut is None else ut[t:t + 1], None if codes is None else codes[t:t + 1],
                         threshold_k=THRESHOLD_K)
        assert _bits(twin.reduce_temperature(Ls[t])) == _bits(temps[t]), f"{what}: temps[{t}] against single steps"
    twin.close()


# ---------------------------------------------------------------------------------------------
# 3. shapes outside the wave form
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 64, 64, 2), (2, 8, 8, 65)], ids=lambda v: str(v).replace(" ", ""))
def test_launches_per_step_vs_oracle(amd, monkeypatch, shape):
    _run_vs_oracle(amd, monkeypatch, shape, 65, "mixed", None, STEPWISE)


# ---------------------------------------------------------------------------------------------
# 4. a dead world
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch,form", [(None, WAVE), ("DW_NO_EPISODE_WAVE", STEPWISE)])
def test_a_dead_world_is_uniform(amd, monkeypatch, switch, form):
    from therldaisyworld_amd import _ffi, harness
    B, H, W, N, K = 3, 8, 8, 2, 3
    eng = _engine(amd, B, H, W, N, "exact", monkeypatch, switch)
    _assert_form(eng, form)
    eng.init_random(9)
    idx, st = eng.download_agents()
    zeros = np.zeros((B, H, W), dtype=np.float32)
    eng.upload_state_f32(zeros, zeros, quantised=True)
    eng.upload_agents(idx, st)
    Ls = _schedule(K)
    stats, alive, ok, temps = eng.run_episode_trace(Ls, _ffi.POLICY_ARGMAX, threshold_k=THRESHOLD_K, temperature=True)
    assert not stats["max_k"].any() and not alive.any()
    assert (temps["std"] == 0.0).all()
    assert np.array_equal(temps["min"], temps["mean"]) and np.array_equal(temps["max"], temps["mean"])
    p = eng.params
    dead = harness.dead_temperature(types.SimpleNamespace(S=p.S, albedo_bare=p.albedo_bare, sigma=p.sigma), Ls)
    np.testing.assert_allclose(temps["mean"], np.broadcast_to(dead[:, None], (K, B)), rtol=1e-12, atol=0)
    eng.close()


# ---------------------------------------------------------------------------------------------
# 5. batch independence
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["exact", "fast"])
def test_rows_do_not_depend_on_the_batch(amd, monkeypatch, precision):
    """World b of a five-world engine and a one-world engine holding world b: identical rows."""
    shape = B, H, W, N = SHAPES[0]
    K = 65
    mode, ut, codes = _inputs(shape, K, "mixed")
    Ls = _schedule(K)
    eng = _engine(amd, B, H, W, N, precision, monkeypatch)
    _assert_form(eng, WAVE)
    eng.init_random(77)
    eng.step(L0, np.zeros((B, N, 1), dtype=np.int64))
    light, dark = eng.download_planes()
    idx, st = eng.download_agents()
    stats, _, _, temps = eng.run_episode_trace(Ls, mode, ut, codes, threshold_k=THRESHOLD_K, temperature=True)
    eng.close()
    for b in range(B):
        one = _engine(amd, 1, H, W, N, precision, monkeypatch)
        _assert_form(one, WAVE)
        one.upload_state_f32(light[b:b + 1].astype(np.float32), dark[b:b + 1].astype(np.float32), quantised=True)
        one.upload_agents(idx[b:b + 1], st[b:b + 1])
        s1, _, _, t1 = one.run_episode_trace(Ls, mode, ut, codes[:, b:b + 1], threshold_k=THRESHOLD_K, temperature=True)
        one.close()
        assert _bits(s1[:, 0]) == _bits(stats[:, b]), f"world {b}: cover records"
        assert _bits(t1[:, 0]) == _bits(temps[:, b]), f"world {b}: temperature rows"


# ---------------------------------------------------------------------------------------------
# 6. errors: checked before anything runs, the state is untouched
# ---------------------------------------------------------------------------------------------
def _raw_call(eng, K, Ls, temps, stats=None):
    import ctypes as C
    from therldaisyworld_amd import _ffi
    return eng._lib.dw_run_episode_trace_temperature(
        eng._h, K, _ffi.ptr_d(Ls), _ffi.POLICY_ARGMAX, None, None, THRESHOLD_K, None, None,
        None if stats is None else stats.ctypes.data_as(C.POINTER(_ffi.DwWorldStats)),
        None if temps is None else temps.ctypes.data_as(C.POINTER(_ffi.DwTempStats)))


def _agents_snapshot(eng):
    idx, st = eng.download_agents()
    return idx.copy(), st.copy()


def _assert_all_untouched(eng, before, agents, what):
    _assert_untouched(eng, before, what)
    idx, st = eng.download_agents()
    assert np.array_equal(idx, agents[0]) and np.array_equal(st, agents[1]), f"{what}: agents changed"


def test_errors_leave_the_state_untouched(amd, monkeypatch):
    from therldaisyworld_amd import _ffi
    B, H, W, N, K = 3, 8, 8, 2, 4
    Ls = _schedule(K)
    eng = _engine(amd, B, H, W, N, "exact", monkeypatch)
    eng.init_random(5)
    before, agents = _snapshot(eng), _agents_snapshot(eng)
    with pytest.raises(amd.DaisyHipError) as e:                 # the current state is an un-quantised upload
        eng.run_episode_trace(Ls, _ffi.POLICY_ARGMAX, temperature=True)
    assert e.value.code == _ffi.DW_ESTATE
    _assert_all_untouched(eng, before, agents, "un-quantised")
    eng.step(L0, np.zeros((B, N, 1), dtype=np.int64))
    before, agents = _snapshot(eng), _agents_snapshot(eng)
    stats = np.zeros((K, B), dtype=_ffi.STATS_DTYPE)
    assert _raw_call(eng, K, Ls, None, stats) == _ffi.DW_EINVAL and b"temps" in eng._lib.dw_last_error()
    _assert_all_untouched(eng, before, agents, "null temps")
    for bad in (0, 4097):
        long_Ls = _schedule(max(bad, 1))
        temps = np.zeros((max(bad, 1), B), dtype=_ffi.TEMP_STATS_DTYPE)
        assert _raw_call(eng, bad, long_Ls, temps) == _ffi.DW_EINVAL, bad
        assert not temps.view(np.float64).any()
        _assert_all_untouched(eng, before, agents, f"nsteps = {bad}")
    temps = np.zeros((K, B), dtype=_ffi.TEMP_STATS_DTYPE)
    assert _raw_call(eng, K, Ls, temps) == _ffi.DW_OK                # ... the handle still works, and `trace` may be null
    assert _bits(temps[-1]) == _bits(eng.reduce_temperature(Ls[-1]))
    eng.close()

    f64 = _engine(amd, B, H, W, N, "f64", monkeypatch)
    f64.init_random(5)
    f64.step(L0, np.zeros((B, N, 1), dtype=np.int64))
    before, agents = _snapshot(f64), _agents_snapshot(f64)
    with pytest.raises(amd.DaisyHipError) as e:
        f64.run_episode_trace(Ls, _ffi.POLICY_ARGMAX, temperature=True)
    assert e.value.code == _ffi.DW_EINVAL
    _assert_all_untouched(f64, before, agents, "f64")
    f64.close()


# ---------------------------------------------------------------------------------------------
# 7. simulate_grazing(temperature=True) against the notebook's loop on the oracle environment
# ---------------------------------------------------------------------------------------------
GRAZING_AGENTS = {"none": None, "greedy": dict(epsilon=0.0), "half_random": dict(epsilon=0.5)}
GRAZING_B, GRAZING_STEPS, GRAZING_CHUNK = 6, 40, 16
_NOTEBOOK = {}


def _notebook_run(agent_key):
    """update_fig_agent's loop on the oracle from seed 17, once per agent: step, then append temp.mean(), temp.std(),
    dead_temp and the population means."""
    if agent_key in _NOTEBOOK:
        return _NOTEBOOK[agent_key]
    kw = GRAZING_AGENTS[agent_key]
    np.random.seed(17)
    ref = O.OracleDaisyWorld.like_reference_ctor(grid_dimension=8, n_agents=4)
    ref.P.batch_size = GRAZING_B
    obs = ref.reset()
    agent = None if kw is None else O.OracleGreedy(**kw)
    out = {k: [] for k in ("L", "temp", "dead")}
    for _ in range(GRAZING_STEPS):
        action = agent(obs) if agent is not None else None
        out["L"].append(ref.L)
        obs, _, _, _ = ref.step(action)
        out["temp"].append(np.asarray(ref.temp).reshape(GRAZING_B, 8, 8).copy())
        out["dead"].append(float(np.asarray(ref.dead_temp).reshape(-1)[0]))
    out = {k: np.array(v) for k, v in out.items()}
    out.update(grid=ref.grid.copy(), rng=np.random.get_state())
    _NOTEBOOK[agent_key] = out
    return out


@pytest.mark.parametrize("agent_key", list(GRAZING_AGENTS))
def test_simulate_grazing_temperature_vs_notebook_loop(amd, agent_key):
    from therldaisyworld_amd import harness
    ref = _notebook_run(agent_key)
    kw = GRAZING_AGENTS[agent_key]

    def run(precision, temperature):
        np.random.seed(17)
        env = amd.RLDaisyWorld(grid_dimension=8, n_agents=4, precision=precision)
        env.batch_size = GRAZING_B
        agent = None if kw is None else amd.Greedy(**kw)
        out = harness.simulate_grazing(env, agent, GRAZING_STEPS, chunk=GRAZING_CHUNK, temperature=temperature)
        grid, rng = env.grid.copy(), np.random.get_state()
        env.close()
        return out, grid, rng

    out, grid, rng = run("exact", True)
    assert np.array_equal(out["L"], ref["L"])
    for t in range(GRAZING_STEPS):
        row = np.zeros(GRAZING_B, dtype=[("mean", "<f8"), ("std", "<f8"), ("min", "<f8"), ("max", "<f8")])
        for f in ("mean", "std", "min", "max"):
            row[f] = out[f + "_temp"][t]
        _assert_rows_close(row, ref["temp"][t], f"{agent_key}: step {t}")
    assert out["dead_temp"].shape == (GRAZING_STEPS,)
    np.testing.assert_allclose(out["dead_temp"], ref["dead"], rtol=2e-12, atol=0)
    assert np.array_equal(grid, ref["grid"])
    assert rng[2] == ref["rng"][2] and np.array_equal(rng[1], ref["rng"][1])

    plain, grid0, rng0 = run("exact", False)                        # everything returned today, unchanged
    assert set(out) == set(plain) | {"mean_temp", "std_temp", "min_temp", "max_temp", "dead_temp"}
    for name in plain:
        assert _bits(plain[name]) == _bits(out[name]), name
    assert np.array_equal(grid, grid0) and rng[2] == rng0[2] and np.array_equal(rng[1], rng0[1])

    host, grid64, rng64 = run("f64", True)                          # the host loop: the same dict
    assert set(host) == set(out)
    for name in out:
        assert _bits(host[name]) == _bits(out[name]), f"f64 host loop: {name}"
    assert np.array_equal(grid64, grid) and rng64[2] == rng[2] and np.array_equal(rng64[1], rng[1])
