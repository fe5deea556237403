"""CPU-side tests (no GPU) of dw_run_episode_ensemble and harness.simulate_lifespan_sweep:

  * the symbol is declared in the header, exported by the library and bound by _ffi with the declared argument list; the
    ABI number of header, _ffi and library agree; a null handle is refused;
  * the Python surface exists and refuses wrong shapes before any device call;
  * the harness's per-block parameter and action tables and its per-scenario counting / stopping rule, on synthetic flag
    arrays against the notebook's loop written out per scenario.
"""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_exported_and_bound():
    from therldaisyworld_amd import _ffi
    header = open(os.path.join(ROOT, "include", "daisyworld_hip.h")).read()
    assert re.search(r"\bint dw_run_episode_ensemble\(dw_handle\* h, int32_t nsteps,\s*const dw_world_params\* worlds[^;]*"
                     r"const double\* L_schedule[^;]*int policy_mode, const uint8_t\* use_table, const int8_t\* table,\s*"
                     r"uint32_t threshold_k, uint8_t\* world_alive, uint8_t\* agent_ok\);", header)
    declared = int(re.search(r"#define DW_ABI_VERSION (\d+)\b", header).group(1))
    lib = _ffi.load()
    assert declared == _ffi.DW_ABI_VERSION == lib.dw_abi_version()
    assert "dw_run_episode_ensemble" in _ffi.SIGNATURES
    assert lib.dw_run_episode_ensemble.argtypes == [C.c_void_p, C.c_int32, C.POINTER(_ffi.DwWorldParams), C.POINTER(C.c_double),
                                                    C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_int8), C.c_uint32,
                                                    C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]
    Ls = np.ones((4, 1))
    tab = np.zeros(1, dtype=_ffi.WORLD_PARAMS_DTYPE)
    rc = lib.dw_run_episode_ensemble(None, 4, tab.ctypes.data_as(C.POINTER(_ffi.DwWorldParams)), _ffi.ptr_d(Ls), 0, None, None,
                                     5, None, None)
    assert rc == _ffi.DW_EINVAL and b"null" in lib.dw_last_error()


def test_python_surface_and_shape_checks_without_a_device():
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import _ffi, harness
    assert callable(amd.Engine.run_episode_ensemble)
    assert amd.simulate_lifespan_sweep is harness.simulate_lifespan_sweep
    assert "simulate_lifespan_sweep" in amd.__all__

    class _NoDevice:                                           # any touch of the library is an AttributeError
        B, N = 3, 2
        _world_table = amd.Engine._world_table
    tab = np.zeros(3, dtype=_ffi.WORLD_PARAMS_DTYPE)
    for bad in (np.ones((4, 2)), np.ones(3), np.ones((4, 3, 1))):
        with pytest.raises(ValueError, match="shape"):
            amd.Engine.run_episode_ensemble(_NoDevice(), tab, bad, _ffi.POLICY_ARGMAX)
    with pytest.raises(ValueError, match="per-world constants"):
        amd.Engine.run_episode_ensemble(_NoDevice(), tab[:2], np.ones((4, 3)), _ffi.POLICY_ARGMAX)
    with pytest.raises(ValueError, match="table must have shape"):
        amd.Engine.run_episode_ensemble(_NoDevice(), tab, np.ones((4, 3)), _ffi.POLICY_TABLE, None, np.zeros((4, 3, 1), dtype=np.int8))
    env = types.SimpleNamespace(batch_size=6, n_agents=2, precision="exact", collision_mode=0)
    greedy = amd.Greedy()
    with pytest.raises(ValueError, match="batch_size"):
        harness.simulate_lifespan_sweep(env, [{"params": {}, "agent": greedy}] * 2, 4, obs=True)
    with pytest.raises(ValueError, match="Greedy or None"):
        harness.simulate_lifespan_sweep(env, [{"params": {}, "agent": lambda obs: obs}] * 2, 3, obs=True)
    env.precision = "f64"
    with pytest.raises(ValueError, match="device-resident"):
        harness.simulate_lifespan_sweep(env, [{"params": {}, "agent": greedy}] * 2, 3, obs=True)


def _env_constants():
    from therldaisyworld_amd import _ffi
    return types.SimpleNamespace(**{name: float(i + 1) for i, name in enumerate(_ffi.WORLD_PARAM_NAMES)})


def test_parameter_table_is_filled_per_block():
    from therldaisyworld_amd import _ffi, harness
    env = _env_constants()
    scenarios = [{"params": {}, "agent": None}, {"params": {"q2": 0.0, "gamma": np.array([0.1, 0.2, 0.3])}, "agent": None}]
    tab = harness._sweep_param_table(env, scenarios, 3)
    assert tab.dtype == _ffi.WORLD_PARAMS_DTYPE and tab.shape == (6,)
    for name in _ffi.WORLD_PARAM_NAMES:
        assert np.all(tab[name][:3] == getattr(env, name))
        if name not in ("q2", "gamma"):
            assert np.all(tab[name][3:] == getattr(env, name))
    assert np.all(tab["q2"][3:] == 0.0) and np.array_equal(tab["gamma"][3:], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="not a per-world constant"):
        harness._sweep_param_table(env, [{"params": {"agent_gamma": 0.1}}], 3)
    with pytest.raises(ValueError, match="scalar or shape"):
        harness._sweep_param_table(env, [{"params": {"q2": np.zeros(2)}}], 3)


def test_action_table_codes_and_draw_order():
    import therldaisyworld_amd as amd
    from therldaisyworld_amd import harness
    K, Bs, N = 6, 3, 2
    scenarios = [{"agent": amd.Greedy(greedy=True)}, {"agent": None}, {"agent": amd.Greedy(greedy=False)},
                 {"agent": amd.Greedy(epsilon=0.5, greedy=True)}, {"agent": amd.Greedy(epsilon=0.5, greedy=False)},
                 {"agent": amd.Greedy(epsilon=0.5, greedy=True)}]
    running = np.array([True, True, True, True, True, False])
    np.random.seed(5)
    tab = harness._sweep_action_table(scenarios, running, K, Bs, N)
    after = np.random.get_state()[2]
    assert tab.shape == (K, 6 * Bs, N) and tab.dtype == np.int8
    assert np.all(tab[:, 0:3] == -1) and np.all(tab[:, 3:6] == 0) and np.all(tab[:, 6:9] == -2)
    assert np.all(tab[:, 15:18] == -1)                          # ended: draws nothing, keeps the greedy code
    # the documented order: step-major, scenario-major, one coin and (on the random branch) one block of codes
    np.random.seed(5)
    want = np.zeros((K, 2 * Bs, N), dtype=np.int8)
    want[:, :Bs], want[:, Bs:] = -1, -2
    random_steps = 0
    for t in range(K):
        for j in range(2):
            if not np.random.rand() > 0.5:
                want[t, j * Bs:(j + 1) * Bs] = np.random.randint(9, size=(Bs, N, 1, 1)).reshape(Bs, N)
                random_steps += 1
    assert 0 < random_steps < 2 * K
    assert np.array_equal(tab[:, 9:15], want) and np.random.get_state()[2] == after
    # deterministic scenarios alone draw nothing
    before = np.random.get_state()[2]
    harness._sweep_action_table(scenarios[:3], running[:3], K, Bs, N)
    assert np.random.get_state()[2] == before


def _notebook_counts(alive, ok):
    """The notebook's loop (cell 2:46-57) on one scenario's flags: count until the step at which all its worlds are dead."""
    done_at = np.zeros(alive.shape[1], dtype=int)
    agents = np.zeros(ok.shape[1:] + (1,), dtype=int)
    for t in range(alive.shape[0]):
        done_at += alive[t]
        agents += ok[t][..., None]
        if not alive[t].any():
            return done_at, agents, True
    return done_at, agents, False


def test_counting_and_stopping_rule_per_scenario():
    from therldaisyworld_amd import harness
    S, Bs, N, K = 4, 3, 2, 8
    rng = np.random.RandomState(2)
    # scenario 0 dies at step 9 (second chunk), 1 at step 2 and "revives" afterwards (must stay frozen), 2 never dies,
    # 3 is dead from the first step
    T = 2 * K
    alive = rng.rand(T, S, Bs) < 0.7
    alive[:, :, 0] = True
    alive[9, 0] = False
    alive[2, 1] = False
    alive[0, 3] = False
    ok = rng.rand(T, S, Bs, N) < 0.6
    done_at = np.zeros((S, Bs), dtype=int)
    agents = np.zeros((S, Bs, N, 1), dtype=int)
    running = np.ones(S, dtype=bool)
    for c in range(2):
        sl = slice(c * K, (c + 1) * K)
        harness._sweep_account(done_at, agents, running, alive[sl].reshape(K, S * Bs), ok[sl].reshape(K, S * Bs, N))
        if c == 0:
            assert running.tolist() == [True, False, True, False]
    assert running.tolist() == [False, False, True, False]
    for s in range(S):
        d, a, ended = _notebook_counts(alive[:, s], ok[:, s])
        assert np.array_equal(done_at[s], d) and np.array_equal(agents[s], a), s
        assert ended == (not running[s])
    # agent-free ensembles: nothing to count per agent
    harness._sweep_account(np.zeros((S, Bs), dtype=int), np.zeros((S, Bs, 0, 1), dtype=int), np.ones(S, dtype=bool),
                           alive[:K].reshape(K, S * Bs), np.zeros((K, S * Bs, 0), dtype=bool))
