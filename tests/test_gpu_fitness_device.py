"""The fitness bookkeeping of ES populations on the device (run with ``-m gpu``): dw_fitness_begin / dw_fitness_account /
dw_run_episode_mlp_fitness / dw_fitness_download and `get_fitness[_population](bookkeeping="device")`.

  account     `Engine.fitness_account` on random episodes against `harness._population_chunk`, the host's bookkeeping: every
              call's (executed, finished), and afterwards the bytes of `sum_reward`, `done_at` and `running`; member blocks of
              fewer than 8 values, of one leaf and of several leaves of the pairwise order (n = wpm * half up to 2000);
  harness     `get_fitness_population(bookkeeping="device")` against `"host"` from the same seed: fitness bits, counters and
              the environment afterwards - one wave per world, the workgroup form (20 x 20), launches per step
              (DW_NO_EPISODE_WAVE), episodes that end inside a chunk;
  reference   `get_fitness(bookkeeping="device")` reproduces the reference rollout of tests/golden/G10_mlp.npz;
  twins       `run_episode_mlp_fitness` leaves what `run_episode_mlp` leaves, and accounts the rewards it left on the device;
  errors      the codes of the header, each with the handle untouched.

Every comparison is byte-exact."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_abi_and_host import _random_episode  # noqa: E402
from test_gpu_episode_trace import L0, _assert_untouched, _engine, _schedule, _snapshot, _state_of  # noqa: E402


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _host_acc(B, N, P):
    return {"done_at": np.zeros((B, N, 1), dtype=int), "total_steps": np.zeros((B, N, 1), dtype=int),
            "sum_reward": np.zeros(P), "running": np.ones(P, dtype=bool)}


def _assert_accumulators(eng, acc, what):
    sum_reward, done_at, running = eng.fitness_download()
    assert _bits(sum_reward) == _bits(acc["sum_reward"]), (what, sum_reward, acc["sum_reward"])
    assert np.array_equal(done_at, acc["done_at"]) and np.array_equal(done_at, acc["total_steps"]), what
    assert np.array_equal(running, acc["running"]), (what, running, acc["running"])


# ---------------------------------------------------------------------------------------------
# fitness_account against harness._population_chunk
# ---------------------------------------------------------------------------------------------
#          P, wpm,  N, half
BLOCKS = [(3, 4, 4, 2), (2, 32, 4, 2), (1, 50, 4, 2), (2, 3, 2, 1), (5, 1, 3, 1), (2, 7, 5, 2), (1, 64, 4, 2), (1, 65, 4, 2),
          (1, 150, 4, 2), (1, 1000, 4, 2)]
K_EPISODE = 40


@pytest.mark.parametrize("block", BLOCKS, ids=lambda v: str(v).replace(" ", ""))
def test_fitness_account_equals_the_host_bookkeeping(amd, monkeypatch, block):
    from therldaisyworld_amd import harness
    P, wpm, N, half = block
    B = P * wpm
    eng = _engine(amd, B, 8, 8, N, "exact", monkeypatch)
    ended = 0
    for p_done in (0.0, 0.02, 0.2):
        for chunk in (1, 5, 64):
            what = (block, p_done, chunk)
            rng = np.random.RandomState(int(chunk * 100 + p_done * 1000) + 7 * B + N)
            rewards, dones = _random_episode(rng, K_EPISODE, B, N, p_done)
            acc = _host_acc(B, N, P)
            eng.fitness_begin(wpm, half)
            finished = False
            for t0 in range(0, K_EPISODE, chunk):              # every chunk, also those behind the end of the episode
                want = harness._population_chunk(acc, rewards[t0:t0 + chunk], dones[t0:t0 + chunk], half, wpm)
                got = eng.fitness_account(rewards[t0:t0 + chunk], dones[t0:t0 + chunk])
                assert got == want, (what, t0, got, want)
                finished = finished or want[1]
            _assert_accumulators(eng, acc, what)
            if finished:                                        # no member runs: a further chunk changes nothing
                ended += 1
                assert eng.fitness_account(rewards[:chunk], dones[:chunk]) == (1, True), what
                _assert_accumulators(eng, acc, what)
    assert ended >= 1, "no episode of this block ended: the frozen accumulators were not exercised"
    eng.close()


# ---------------------------------------------------------------------------------------------
# the harnesses
# ---------------------------------------------------------------------------------------------
def _population(amd, kind, P):
    pop = [amd.MLP() for _ in range(P)]
    if kind == "lazy":                                          # all-zero networks: action 0, the agents starve after ~19 steps
        for m in pop:
            m.set_parameters(np.zeros(1808))
    elif kind == "mixed":                                       # member 0's own agents never graze, the others' do
        pop[0].set_parameters(np.zeros(1808))
    return pop


def _run_population(amd, bookkeeping, dim, chunk, precision, kind, max_steps=70, P=3, wpm=4):
    from therldaisyworld_amd.harness import get_fitness_population
    np.random.seed(1234 + dim)
    pop = _population(amd, kind, P)
    env = amd.RLDaisyWorld(grid_dimension=dim, n_agents=4, precision=precision)
    res = get_fitness_population(env, pop, adversary_of=[1, 2, 0], worlds_per_member=wpm, max_steps=max_steps, chunk=chunk,
                                 bookkeeping=bookkeeping)
    out = {"fitness": np.array([r[0] for r in res]), "total_steps": np.stack([np.asarray(r[1]) for r in res]),
           "done_at": np.stack([np.asarray(r[2]) for r in res]), "grid": env.grid.copy(), "L": env.L,
           "step_count": env.step_count, "agent_indices": env.agent_indices.copy(), "agent_states": env.agent_states.copy(),
           "info": env._engine.kernel_info()}
    env.close()
    return out


def _assert_same_run(dev, host, what):
    assert _bits(dev["fitness"]) == _bits(host["fitness"]), (what, dev["fitness"], host["fitness"])
    for key in ("total_steps", "done_at", "grid", "L", "step_count", "agent_indices", "agent_states"):
        assert np.array_equal(dev[key], host[key]), (what, key)


HARNESS_CASES = [(dim, chunk, precision, "random") for dim in (8, 16) for chunk in (16, 64) for precision in ("exact", "fast")]
HARNESS_CASES += [(16, 16, "exact", "lazy"), (16, 64, "exact", "lazy"), (8, 16, "exact", "mixed"), (16, 64, "fast", "mixed")]


@pytest.mark.parametrize("dim,chunk,precision,kind", HARNESS_CASES, ids=lambda v: str(v))
def test_population_fitness_on_the_device_equals_the_host_route(amd, monkeypatch, dim, chunk, precision, kind):
    for name in ("DW_NO_EPISODE_WAVE", "DW_NO_EPISODE_KERNEL"):
        monkeypatch.delenv(name, raising=False)
    host = _run_population(amd, "host", dim, chunk, precision, kind)
    dev = _run_population(amd, "device", dim, chunk, precision, kind)
    assert "; mlp episode: one wave per world" in dev["info"], dev["info"]
    _assert_same_run(dev, host, (dim, chunk, precision, kind))
    if kind == "lazy":                                          # the episode ended inside a chunk (step 1 is a chunk of its own)
        assert 10 < dev["step_count"] < 40 and (dev["step_count"] - 1) % chunk != 0, dev["step_count"]


def test_population_fitness_workgroup_form(amd, monkeypatch):
    for name in ("DW_NO_EPISODE_WAVE", "DW_NO_EPISODE_KERNEL"):
        monkeypatch.delenv(name, raising=False)
    host = _run_population(amd, "host", 20, 16, "exact", "mixed")
    dev = _run_population(amd, "device", 20, 16, "exact", "mixed")
    assert "; mlp episode: workgroup (LDS)" in dev["info"], dev["info"]
    _assert_same_run(dev, host, "20 x 20")


def test_population_fitness_without_the_wave_kernel(amd, monkeypatch):
    monkeypatch.delenv("DW_NO_EPISODE_KERNEL", raising=False)
    monkeypatch.setenv("DW_NO_EPISODE_WAVE", "1")
    host = _run_population(amd, "host", 8, 16, "exact", "mixed")
    dev = _run_population(amd, "device", 8, 16, "exact", "mixed")
    assert "; mlp episode: workgroup (LDS)" in dev["info"], dev["info"]
    _assert_same_run(dev, host, "DW_NO_EPISODE_WAVE")


def test_get_fitness_on_the_device_matches_reference_rollout_g10(amd, golden):
    from therldaisyworld_amd.harness import get_fitness
    g = golden("G10_mlp")
    np.random.seed(4242)
    agent, adversary = amd.MLP(), amd.MLP()
    env = amd.RLDaisyWorld(grid_dimension=8, n_agents=4)     # consumes the constructor's draws, as the fixture did
    env.batch_size = 6
    fitness, total_steps, done_at = get_fitness(env, agent, adversary, max_steps=40, bookkeeping="device")
    assert fitness == float(g["sum_reward"]) / (6 * 4)
    assert np.array_equal(np.array(done_at), (1 - 1 * g["dones"]).sum(axis=0))
    assert np.array_equal(total_steps, (1 - 1 * g["dones"]).sum(axis=0))
    assert np.array_equal(env.grid, g["grid_final"])
    env.close()


def test_get_fitness_with_one_agent_names_the_host_route(amd):
    from therldaisyworld_amd.harness import get_fitness
    np.random.seed(3)
    agent, adversary = amd.MLP(), amd.MLP()
    env = amd.RLDaisyWorld(grid_dimension=8, n_agents=1)
    env.batch_size = 2
    with pytest.raises(ValueError, match='bookkeeping="host"'):
        get_fitness(env, agent, adversary, max_steps=4, bookkeeping="device")
    env.close()


# ---------------------------------------------------------------------------------------------
# twins: run_episode_mlp_fitness leaves what run_episode_mlp leaves
# ---------------------------------------------------------------------------------------------
#              B,  H,  W, N, wpm, precision, switch,                 form
TWIN_CASES = [(6, 16, 16, 4, 3, "exact", None, "one wave per world"),
              (6, 8, 8, 4, 2, "fast", None, "one wave per world"),
              (4, 20, 20, 4, 2, "exact", None, "workgroup (LDS)"),
              (6, 8, 8, 4, 3, "exact", "DW_NO_EPISODE_WAVE", "workgroup (LDS)"),
              (6, 8, 8, 4, 6, "exact", "DW_NO_EPISODE_KERNEL", "launches per step")]


@pytest.mark.parametrize("B,H,W,N,wpm,precision,switch,form", TWIN_CASES, ids=lambda v: str(v))
def test_run_episode_mlp_fitness_leaves_what_run_episode_mlp_leaves(amd, monkeypatch, B, H, W, N, wpm, precision, switch, form):
    from therldaisyworld_amd import harness
    K, half, P = 21, N // 2, B // wpm
    params = np.random.RandomState(B + H + N).randn(3, 1808) * 0.5
    ma = (np.arange(B) % 3).astype(np.int32)
    mb = ((np.arange(B) + 1) % 3).astype(np.int32)
    twins = []
    for _ in range(2):
        eng = _engine(amd, B, H, W, N, precision, monkeypatch, switch)
        eng.init_random(77 + B + H, quantised=True)
        eng.step(L0, np.zeros((B, N, 1), dtype=np.int64))
        twins.append(eng)
    plain, fit = twins
    assert f"; mlp episode: {form}" in fit.kernel_info(), fit.kernel_info()
    acc = _host_acc(B, N, P)
    fit.fitness_begin(wpm, half)
    for call, Ls in enumerate((_schedule(K), _schedule(K + 5)[K:])):   # the second call: the resident parameter sets
        w = params if call == 0 else None
        rewards, dones = plain.run_episode_mlp(Ls, w, ma, mb, half, n_members=3)
        want = harness._population_chunk(acc, rewards, dones, half, wpm)
        got = fit.run_episode_mlp_fitness(Ls, w, ma, mb, half, n_members=3)
        assert got == want, (call, got, want)
        a, b = _state_of(plain, Ls[-1]), _state_of(fit, Ls[-1])
        for key in a:
            assert np.array_equal(a[key], b[key]), (call, key)
        assert plain.last_fixup_count() == fit.last_fixup_count()
    _assert_accumulators(fit, acc, form)
    plain.close(); fit.close()


# ---------------------------------------------------------------------------------------------
# error codes
# ---------------------------------------------------------------------------------------------
def test_errors_leave_the_handle_untouched(amd, monkeypatch):
    from therldaisyworld_amd import _ffi
    B, N, K = 6, 4, 3
    eng = _engine(amd, B, 8, 8, N, "exact", monkeypatch)
    eng.init_random(5, quantised=True)
    eng.step(L0, np.zeros((B, N, 1), dtype=np.int64))
    lib, h = eng._lib, eng._h
    rewards, dones = _random_episode(np.random.RandomState(1), K, B, N, 0.02)
    r, d = np.ascontiguousarray(rewards), np.ascontiguousarray(dones).view(np.uint8)
    Ls, w = _schedule(K), np.random.RandomState(2).randn(1, 1808)
    e, f = C.c_int32(-7), C.c_int32(-7)
    before = _snapshot(eng)

    def account(n):
        return lib.dw_fitness_account(h, n, _ffi.ptr_d(r), _ffi.ptr_u8(d), C.byref(e), C.byref(f))

    def run(n):
        return lib.dw_run_episode_mlp_fitness(h, n, _ffi.ptr_d(Ls), _ffi.ptr_d(w), 1, None, None, 2, 0.75, C.byref(e), C.byref(f))

    # before dw_fitness_begin
    assert account(K) == _ffi.DW_ESTATE and b"dw_fitness_begin" in lib.dw_last_error()
    assert run(K) == _ffi.DW_ESTATE
    assert lib.dw_fitness_download(h, None, None, None) == _ffi.DW_ESTATE
    with pytest.raises(amd.DaisyHipError) as err:
        eng.fitness_download()
    assert err.value.code == _ffi.DW_ESTATE
    # dw_fitness_begin's arguments
    for wpm, half in ((4, 2), (0, 2), (-1, 2), (3, 0), (3, N + 1)):
        assert lib.dw_fitness_begin(h, wpm, half) == _ffi.DW_EINVAL, (wpm, half)
    assert account(K) == _ffi.DW_ESTATE                         # a refused begin began nothing
    _assert_untouched(eng, before, "before begin")
    eng.fitness_begin(3, 2)
    assert eng.fitness_account(rewards, dones)[0] == K
    kept = eng.fitness_download()
    for n in (0, -1, 4097):
        assert account(n) == _ffi.DW_EINVAL and run(n) == _ffi.DW_EINVAL, n
    assert lib.dw_fitness_begin(h, 4, 2) == _ffi.DW_EINVAL      # refused: the accumulators of the running episode stay
    assert (e.value, f.value) == (-7, -7)                       # a refused call writes no outcome
    after = eng.fitness_download()
    for x, y in zip(kept, after):
        assert _bits(x) == _bits(y)
    _assert_untouched(eng, before, "refused calls")
    assert eng.fitness_account(rewards, dones)[0] >= 1          # and the episode goes on
    eng.close()
