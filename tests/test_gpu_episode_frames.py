"""dw_run_episode_frames / Engine.run_episode_frames / harness.simulate_grazing_frames (run with ``-m gpu``): the episode loop
with frames - per tile of selected worlds the cover sums after every stride-th step, the mean of the temperature field
that step computes, and the agents on it.

  per-step twin  K x (`run_episode` of one step, `reduce_tiles`, `download_agents`) on an engine with the same seed: cover,
                 temperature and agents byte for byte, both precisions, shapes on and off the wave's 64-cell slots, every
                 tile mapping a 256-cell world reaches, K / stride pairs around the 64-step segment, selections, policies;
  records twin   `run_episode_trace(temperature=True)` (or `run_episode`) with the same arguments: flags, records,
                 temperature rows, the whole state and last_fixup_count;
  oracle         exact mode against the float64 oracle at 1 x 1 tiles (cover and agents exactly, the field within
                 rtol 2e-12, the bound tests/test_gpu_frames.py derives), block tiles within (n + 3) 2^-53 of the exact mean
                 of the same call's 1 x 1 frame (derived there too);
  other forms    DW_NO_EPISODE_WAVE, DW_NO_EPISODE_KERNEL, N = 65, C = 4096 and the wave-strip step kernel;
  also           output subsets, a tiny ring (several launches in the wave form), the error codes, and
                 simulate_grazing_frames against the notebook's loop on the oracle.

Protocol (tests/test_gpu_episode_trace.py's): ``init_random(seed)``, one zero-action step to quantise, the schedule
0.9 + 0.002 t.  Every comparison is exact equality unless stated, and every case asserts from ``kernel_info()`` which form
it ran.
"""
import math

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


def _schedule(K):
    return 0.9 + 0.002 * np.arange(K, dtype=np.float64)


def _engine(amd, shape, precision, monkeypatch, switch=None, ring=None):
    """A handle created under exactly one (or none) of the DW_NO_EPISODE_* switches and, `ring`, the frame ring hook: they
    are read at creation."""
    from therldaisyworld_amd import _ffi
    for name in ("DW_NO_EPISODE_WAVE", "DW_NO_EPISODE_KERNEL", "DW_TEST_HOOKS", "DW_TEST_FRAME_RING"):
        monkeypatch.delenv(name, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")
    if ring:
        monkeypatch.setenv("DW_TEST_HOOKS", "1")
        monkeypatch.setenv("DW_TEST_FRAME_RING", str(ring))
    p = amd.default_params(*shape)
    p.precision = _ffi.PRECISION[precision]
    eng = amd.Engine(p)
    if ring:
        assert f"DW_TEST_FRAME_RING={ring}" in eng.kernel_info()
    return eng


def _fresh(amd, shape, precision, monkeypatch, switch=None, ring=None, form=None):
    B, H, W, N = shape
    eng = _engine(amd, shape, precision, monkeypatch, switch, ring)
    if form:
        assert f"; episode frames: {form}" in eng.kernel_info(), eng.kernel_info()
    eng.init_random(41 + H + 3 * W + N)
    eng.step(L0, np.zeros((B, N, 1), dtype=np.int64) if N else None)
    return eng


def _inputs(shape, K, policy):
    """(policy_mode, use_table (K,) uint8 or None, codes (K, B, N) int8 or None): "argmax", or POLICY_ARGMAX with the table
    taken on some steps (around the segment boundary among them), codes 0..8 mixed with -1 / -2."""
    from therldaisyworld_amd import _ffi
    B, H, W, N = shape
    if policy == "argmax":
        return _ffi.POLICY_ARGMAX, None, None
    rng = np.random.RandomState(97 * B + 13 * H + W + 1000 * N + K)
    codes = rng.randint(-2, 9, size=(K, B, N)).astype(np.int8)
    ut = (rng.rand(K) < 0.4).astype(np.uint8)
    ut[[t for t in (0, 63, 64, 65) if t < K]] = 1
    ut[[t for t in (1, 62) if t < K]] = 0
    return _ffi.POLICY_ARGMAX, ut, codes


def _state_of(eng, L_last):
    """Everything the engine can be asked for after a call."""
    from therldaisyworld_amd import _ffi
    out = {}
    out["light"], out["dark"] = (_k(x) for x in eng.download_planes())
    out["prev_light"], out["prev_dark"] = (_k(x) for x in eng.download_planes(_ffi.STATE_PREVIOUS))
    s = eng.reduce()
    for f in ("max_k", "sum_light_k", "sum_dark_k"):
        out["reduce_" + f] = s[f].copy()
    out["fixups"] = np.array(eng.last_fixup_count())
    if eng.N:
        idx, st = eng.download_agents()
        out["idx"], out["st"] = idx.copy(), st.copy()
        out["action"] = eng.download_actions().copy()
        out["obs"] = eng.get_obs(L_last)
    return out


def _agent_records(idx, st, worlds):
    from therldaisyworld_amd import _ffi
    pick = slice(None) if worlds is None else np.asarray(worlds)
    rec = np.zeros(st[pick].shape, dtype=_ffi.AGENT_FRAME_DTYPE)
    rec["row"], rec["col"], rec["state"] = idx[pick][..., 0], idx[pick][..., 1], st[pick]
    return rec


_TWIN = {}


def _per_step_twin(amd, monkeypatch, shape, precision, K, policy, tiles, worlds):
    """K x (run_episode of one step, reduce_tiles per tile size, download_agents): the frames of EVERY step, for all the
    tile sizes of a case at once; computed once per case and left unchanged."""
    key = (shape, precision, K, policy, tuple(tiles), None if worlds is None else tuple(worlds))
    if key in _TWIN:
        return _TWIN[key]
    mode, ut, codes = _inputs(shape, K, policy)
    Ls = _schedule(K)
    twin = _fresh(amd, shape, precision, monkeypatch)
    out = {"cover": {t: [] for t in tiles}, "temp": {t: [] for t in tiles}, "agents": []}
    for t in range(K):
        twin.run_episode(Ls[t:t + 1], mode, None if ut is None else ut[t:t + 1], None if codes is None else codes[t:t + 1],
                         threshold_k=THRESHOLD_K)
        for tile in tiles:
            cov, tmp = twin.reduce_tiles(Ls[t], tile=tile, worlds=worlds)
            out["cover"][tile].append(cov)
            out["temp"][tile].append(tmp)
        if shape[3]:
            out["agents"].append(_agent_records(*twin.download_agents(), worlds))
    twin.close()
    _TWIN[key] = out
    return out


def _bytes_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_frames(res, twin, tile, K, stride, what, with_agents):
    cov, tmp, ag = res[:3]
    F = K // stride
    assert cov.shape[0] == F and tmp.shape[0] == F, what
    for f in range(F):
        t = (f + 1) * stride - 1
        assert _bytes_equal(cov[f], twin["cover"][tile][t]), f"{what}: cover of frame {f} (step {t})"
        assert _bytes_equal(tmp[f], twin["temp"][tile][t]), f"{what}: temperature of frame {f} (step {t})"
        if with_agents:
            assert _bytes_equal(ag[f], twin["agents"][t]), f"{what}: agents of frame {f} (step {t})"
    if F:
        assert cov["sum_light_k"].max() > THRESHOLD_K           # (not the pictures of dead worlds)


# ---------------------------------------------------------------------------------------------
# 1. + 2. the wave form against the per-step twin and against the records twin
# ---------------------------------------------------------------------------------------------
#            shape (B, H, W, N)   K   stride  policy    worlds       tiles
WAVE_CASES = [((5, 8, 8, 4), 64, 1, "argmax", None, ((1, 1), (2, 4), (4, 4), (4, 8), (8, 8))),
              ((5, 8, 8, 4), 65, 3, "mixed", [4, 0, 2], ((1, 1), (2, 4), (8, 8))),
              ((5, 8, 8, 4), 130, 7, "mixed", [3], ((1, 1), (4, 8))),
              ((5, 8, 8, 4), 130, 64, "argmax", None, ((4, 4),)),
              ((5, 8, 8, 4), 1, 1, "mixed", None, ((1, 1),)),
              ((5, 8, 8, 4), 5, 7, "argmax", None, ((1, 1),)),                       # F = 0: no frame, the state advanced
              ((3, 5, 12, 3), 65, 3, "mixed", [2, 0], ((1, 1), (5, 12), (1, 4), (5, 1))),   # 60 cells: off the 64-cell slot
              ((2, 16, 16, 16), 65, 3, "mixed", None, ((1, 1), (2, 4), (4, 4), (4, 8), (8, 8), (16, 16))),   # four slots
              ((2, 16, 16, 64), 10, 1, "argmax", [1], ((1, 1), (16, 16))),           # every lane an agent
              ((3, 13, 17, 0), 65, 3, "argmax", [2, 0], ((1, 1), (13, 1), (1, 17), (13, 17)))]  # no agents, 221 cells


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("shape,K,stride,policy,worlds,tiles", WAVE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_wave_form_vs_per_step_twin_and_records_twin(amd, monkeypatch, shape, K, stride, policy, worlds, tiles, precision):
    B, H, W, N = shape
    mode, ut, codes = _inputs(shape, K, policy)
    Ls = _schedule(K)
    twin = _per_step_twin(amd, monkeypatch, shape, precision, K, policy, tiles, worlds)
    S = B if worlds is None else len(worlds)
    first = None
    for tile in tiles:
        what = f"{shape} {precision} K={K} stride={stride} {policy} worlds={worlds} tile={tile}"
        eng = _fresh(amd, shape, precision, monkeypatch, form=WAVE)
        res = eng.run_episode_frames(Ls, mode, ut, codes, THRESHOLD_K, stride=stride, tile=tile, worlds=worlds, agents=N > 0,
                                     trace=True, temps=True)
        cov, tmp, ag, stats, alive, ok, temps = res
        F = K // stride
        assert cov.shape == tmp.shape == (F, S, H // tile[0], W // tile[1]), what
        assert (ag is None) == (N == 0) and (ag is None or ag.shape == (F, S, N)), what
        _check_frames(res, twin, tile, K, stride, what, N > 0)
        got = (stats, alive, ok, temps, _state_of(eng, Ls[-1]))
        eng.close()
        if first is None:
            first = got
            rec = _fresh(amd, shape, precision, monkeypatch)     # the records twin
            want = rec.run_episode_trace(Ls, mode, ut, codes, threshold_k=THRESHOLD_K, temperature=True)
            want_state = _state_of(rec, Ls[-1])
            rec.close()
            for name, a, b in zip(("stats", "world_alive", "agent_ok", "temps"), got[:4], want):
                assert _bytes_equal(np.asarray(a), np.asarray(b)), f"{what}: {name}"
            for name in want_state:
                assert np.array_equal(got[4][name], want_state[name]), f"{what}: {name}"
        else:                                                   # the records and the state do not depend on the tile
            for a, b in zip(got[:4], first[:4]):
                assert _bytes_equal(np.asarray(a), np.asarray(b)), what
            assert all(np.array_equal(got[4][n], first[4][n]) for n in first[4]), what


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("shape", [(5, 8, 8, 4), (3, 13, 17, 0)], ids=str)
def test_without_records_the_state_is_run_episodes(amd, monkeypatch, shape, precision):
    K, stride = 65, 3
    mode, ut, codes = _inputs(shape, K, "mixed")
    Ls = _schedule(K)
    eng = _fresh(amd, shape, precision, monkeypatch, form=WAVE)
    cov, tmp, ag, stats, alive, ok = eng.run_episode_frames(Ls, mode, ut, codes, THRESHOLD_K, stride=stride, tile=(1, 1),
                                                            agents=shape[3] > 0, trace=False, temps=False)
    assert stats is None
    got = _state_of(eng, Ls[-1])
    eng.close()
    twin = _fresh(amd, shape, precision, monkeypatch)
    alive_a, ok_a = twin.run_episode(Ls, mode, ut, codes, threshold_k=THRESHOLD_K)
    want = _state_of(twin, Ls[-1])
    twin.close()
    assert np.array_equal(alive, alive_a) and np.array_equal(ok, ok_a)
    for name in want:
        assert np.array_equal(got[name], want[name]), f"{shape} {precision}: {name}"


# ---------------------------------------------------------------------------------------------
# 3. exact mode against the float64 oracle
# ---------------------------------------------------------------------------------------------
def _oracle_like(eng, L):
    light, dark = eng.download_planes()
    env = O.OracleDaisyWorldC(grid_dimension=max(eng.H, eng.W), n_agents=eng.N, batch_size=eng.B)
    env.P.agent_gamma = eng.params.agent_gamma
    env.L = L
    env.set_initial_cover(light, dark)
    idx, st = eng.download_agents()
    env.agent_indices = idx.astype(np.int64)
    env.agent_states = st.reshape(eng.B, eng.N, 1).copy()
    return env


@pytest.mark.parametrize("shape,block", [((5, 8, 8, 4), (4, 8)), ((2, 16, 16, 16), (4, 4))], ids=str)
def test_exact_mode_vs_float64_oracle(amd, monkeypatch, shape, block):
    from therldaisyworld_amd import _ffi
    B, H, W, N = shape
    K = 20
    Ls = _schedule(K)
    eng = _engine(amd, shape, "exact", monkeypatch)
    assert f"; episode frames: {WAVE}" in eng.kernel_info()
    eng.init_random(300 + 7 * B + H + W + N)
    env = _oracle_like(eng, L0)
    zeros = np.zeros((B, N, 1), dtype=np.int64)
    eng.step(L0, zeros)
    env.L = L0
    env.step(zeros)
    cov, tmp, ag = eng.run_episode_frames(Ls, _ffi.POLICY_ARGMAX, threshold_k=THRESHOLD_K, stride=1, tile=(1, 1))[:3]
    eng.close()
    greedy = O.OracleGreedy(epsilon=0.0, greedy=True)
    fields = []
    for t in range(K):
        env.L = Ls[t]
        action = greedy(env.get_obs(env.agent_indices))
        env.step(action)
        what = f"{shape} step {t}"
        assert np.array_equal(cov["sum_light_k"][t], _k(env.grid[:, 1])), what
        assert np.array_equal(cov["sum_dark_k"][t], _k(env.grid[:, 2])), what
        assert np.array_equal(np.stack([ag["row"][t], ag["col"][t]], axis=-1), env.agent_indices), what
        assert np.array_equal(ag["state"][t], env.agent_states[..., 0]), what
        field = np.asarray(env.temp).reshape(B, H, W)
        np.testing.assert_allclose(tmp[t], field, rtol=2e-12, atol=0, err_msg=what)
        fields.append(field)
    assert cov["sum_light_k"].max() > THRESHOLD_K
    # a block tile against the exact mean of the same run's 1 x 1 frames (the same seed and arguments: the same doubles)
    eng = _engine(amd, shape, "exact", monkeypatch)
    eng.init_random(300 + 7 * B + H + W + N)
    eng.step(L0, zeros)
    th, tw = block
    n = th * tw
    bt = eng.run_episode_frames(Ls, _ffi.POLICY_ARGMAX, threshold_k=THRESHOLD_K, stride=1, tile=block, cover=False, agents=False)[1]
    eng.close()
    cells = tmp.reshape(K, B, H // th, th, W // tw, tw).transpose(0, 1, 2, 4, 3, 5).reshape(K, B, H // th, W // tw, n)
    for i in np.ndindex(bt.shape):
        exact = math.fsum(cells[i]) / n
        assert abs(bt[i] - exact) <= (n + 3) * 2.0 ** -53 * abs(exact), (shape, block, i, bt[i], exact)


# ---------------------------------------------------------------------------------------------
# 4. the other forms return the wave form's bytes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("switch", ["DW_NO_EPISODE_WAVE", "DW_NO_EPISODE_KERNEL"])
def test_switched_forms_return_the_wave_forms_bytes(amd, monkeypatch, switch, precision):
    shape, K, stride, worlds = (5, 8, 8, 4), 65, 3, [4, 0, 2]
    mode, ut, codes = _inputs(shape, K, "mixed")
    Ls = _schedule(K)
    for tile in ((1, 1), (2, 4), (4, 8)):
        runs = []
        for sw, form in ((None, WAVE), (switch, STEPWISE)):
            eng = _fresh(amd, shape, precision, monkeypatch, sw, form=form)
            res = eng.run_episode_frames(Ls, mode, ut, codes, THRESHOLD_K, stride=stride, tile=tile, worlds=worlds, temps=True)
            runs.append(res + tuple(_state_of(eng, Ls[-1]).items()))
            eng.close()
        for i, (a, b) in enumerate(zip(*runs)):
            if isinstance(a, tuple):
                assert a[0] == b[0] and np.array_equal(a[1], b[1]), f"{switch} {precision} {tile}: {a[0]}"
            else:
                assert _bytes_equal(np.asarray(a), np.asarray(b)), f"{switch} {precision} {tile}: output {i}"


STEPWISE_CASES = [((2, 8, 8, 65), 9, 2, (2, 4), [1]),            # the first agent count the wave kernel refuses
                  ((2, 64, 64, 4), 9, 2, (8, 16), None),         # C = 4096: the workgroup shape
                  ((2, 16, 256, 4), 7, 3, (16, 256), [1, 0])]    # the wave-strip step kernel; a tile of 4096 cells


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("shape,K,stride,tile,worlds", STEPWISE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_launches_per_step_vs_per_step_twin(amd, monkeypatch, shape, K, stride, tile, worlds, precision):
    mode, ut, codes = _inputs(shape, K, "mixed")
    Ls = _schedule(K)
    what = f"{shape} {precision}"
    twin = _per_step_twin(amd, monkeypatch, shape, precision, K, "mixed", ((1, 1), tile), worlds)
    for tl in ((1, 1), tile):
        eng = _fresh(amd, shape, precision, monkeypatch, form=STEPWISE)
        res = eng.run_episode_frames(Ls, mode, ut, codes, THRESHOLD_K, stride=stride, tile=tl, worlds=worlds, temps=True)
        _check_frames(res, twin, tl, K, stride, what, True)
        got, got_state = res[3:], _state_of(eng, Ls[-1])
        eng.close()
    rec = _fresh(amd, shape, precision, monkeypatch)
    want = rec.run_episode_trace(Ls, mode, ut, codes, threshold_k=THRESHOLD_K, temperature=True)
    want_state = _state_of(rec, Ls[-1])
    rec.close()
    for name, a, b in zip(("stats", "world_alive", "agent_ok", "temps"), got, want):
        assert _bytes_equal(np.asarray(a), np.asarray(b)), f"{what}: {name}"
    for name in want_state:
        assert np.array_equal(got_state[name], want_state[name]), f"{what}: {name}"


# ---------------------------------------------------------------------------------------------
# 5. output subsets   6. a tiny ring
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch,form", [(None, WAVE), ("DW_NO_EPISODE_WAVE", STEPWISE)])
def test_output_subsets_equal_their_part_of_the_full_call(amd, monkeypatch, switch, form):
    shape, K, stride, tile, worlds = (5, 8, 8, 4), 65, 3, (2, 4), [4, 0, 2]
    mode, ut, codes = _inputs(shape, K, "mixed")
    Ls = _schedule(K)

    def run(**kw):
        eng = _fresh(amd, shape, "exact", monkeypatch, switch, form=form)
        res = eng.run_episode_frames(Ls, mode, ut, codes, THRESHOLD_K, stride=stride, tile=tile, worlds=worlds, **kw)
        eng.close()
        return res

    full = run(temps=True)
    for i, only in enumerate(("cover", "temperature", "agents")):
        kw = {k: k == only for k in ("cover", "temperature", "agents")}
        part = run(**kw)
        assert [x is None for x in part[:3]] == [j != i for j in range(3)], only
        assert _bytes_equal(part[i], full[i]), only
        assert _bytes_equal(part[3], full[3]), only              # the records are the same call's
    # temp_mean without temps (the field only in frame steps of selected worlds) equals temp_mean with it
    assert _bytes_equal(run(temps=False)[1], full[1])


@pytest.mark.parametrize("ring", [1, 2])
@pytest.mark.parametrize("switch,form", [(None, WAVE), ("DW_NO_EPISODE_WAVE", STEPWISE)])
def test_a_tiny_frame_ring_changes_nothing(amd, monkeypatch, switch, form, ring):
    shape, K, stride, tile, worlds = (5, 8, 8, 4), 130, 7, (2, 4), [4, 0, 2]      # 18 frames: up to 18 launches of the wave form
    mode, ut, codes = _inputs(shape, K, "mixed")
    Ls = _schedule(K)
    runs = []
    for r in (None, ring):
        eng = _fresh(amd, shape, "exact", monkeypatch, switch, ring=r, form=form)
        res = eng.run_episode_frames(Ls, mode, ut, codes, THRESHOLD_K, stride=stride, tile=tile, worlds=worlds, temps=True)
        runs.append(res + tuple(_state_of(eng, Ls[-1]).items()))
        eng.close()
    for i, (a, b) in enumerate(zip(*runs)):
        if isinstance(a, tuple):
            assert a[0] == b[0] and np.array_equal(a[1], b[1]), f"ring {ring} {form}: {a[0]}"
        else:
            assert _bytes_equal(np.asarray(a), np.asarray(b)), f"ring {ring} {form}: output {i}"


# ---------------------------------------------------------------------------------------------
# 7. errors: checked before anything runs, the state is untouched
# ---------------------------------------------------------------------------------------------
def _snapshot(eng):
    return eng.download_planes() + (eng.download_agents() if eng.N else ()) + (eng.reduce(),)


def _assert_untouched(eng, before, what):
    assert all(np.array_equal(a, b) for a, b in zip(before, _snapshot(eng))), f"{what}: the state changed"


def test_errors_leave_the_state_untouched(amd, monkeypatch):
    from therldaisyworld_amd import _ffi
    shape, K = (3, 8, 8, 2), 4
    B, H, W, N = shape
    Ls = _schedule(K)
    eng = _engine(amd, shape, "exact", monkeypatch)
    eng.init_random(5)
    before = _snapshot(eng)
    with pytest.raises(amd.DaisyHipError) as e:                 # the current state is an un-quantised upload
        eng.run_episode_frames(Ls, _ffi.POLICY_ARGMAX)
    assert e.value.code == _ffi.DW_ESTATE
    _assert_untouched(eng, before, "un-quantised")
    eng.step(L0, np.zeros((B, N, 1), dtype=np.int64))
    before = _snapshot(eng)
    for what, kw in (("stride 0", dict(stride=0)),
                     ("all outputs null", dict(cover=False, temperature=False, agents=False)),
                     ("a tile that does not divide", dict(tile=(3, 8))),
                     ("a world listed twice", dict(worlds=[1, 0, 1])),
                     ("a world out of range", dict(worlds=[3]))):
        with pytest.raises(amd.DaisyHipError) as e:
            eng.run_episode_frames(Ls, _ffi.POLICY_ARGMAX, **kw)
        assert e.value.code == _ffi.DW_EINVAL, what
        _assert_untouched(eng, before, what)
    res = eng.run_episode_frames(Ls, _ffi.POLICY_ARGMAX)          # ... and the handle still works
    assert res[0].shape == (K, B, H, W) and res[2].shape == (K, B, N)
    eng.close()

    free = _engine(amd, (3, 8, 8, 0), "exact", monkeypatch)
    free.init_random(5)
    free.step(L0, None)
    before = _snapshot(free)
    with pytest.raises(amd.DaisyHipError) as e:                 # agents of a handle without agents
        free.run_episode_frames(Ls, _ffi.POLICY_ARGMAX, agents=True)
    assert e.value.code == _ffi.DW_EINVAL
    _assert_untouched(free, before, "agents with N = 0")
    free.close()

    f64 = _engine(amd, shape, "f64", monkeypatch)
    f64.init_random(5)
    f64.step(L0, np.zeros((B, N, 1), dtype=np.int64))
    before = _snapshot(f64)
    with pytest.raises(amd.DaisyHipError) as e:
        f64.run_episode_frames(Ls, _ffi.POLICY_ARGMAX)
    assert e.value.code == _ffi.DW_EINVAL
    _assert_untouched(f64, before, "f64")
    f64.close()


# ---------------------------------------------------------------------------------------------
# 8. simulate_grazing_frames against the notebook's loop on the oracle environment
# ---------------------------------------------------------------------------------------------
def test_simulate_grazing_frames_vs_notebook_loop(amd):
    from therldaisyworld_amd import harness
    B, N, nsteps, stride = 3, 4, 40, 3
    np.random.seed(17)
    ref = O.OracleDaisyWorld.like_reference_ctor(grid_dimension=8, n_agents=N)
    ref.P.batch_size = B
    obs = ref.reset()
    agent = O.OracleGreedy(epsilon=0.0)
    want = {k: [] for k in ("L", "light", "dark", "grid", "temp", "idx", "st", "steps", "frame_L")}
    for t in range(nsteps):
        action = agent(obs)
        L_t = ref.L
        want["L"].append(L_t)
        obs, _, done, _ = ref.step(action)
        want["light"].append(ref.grid[:, 1].mean(axis=(1, 2)))
        want["dark"].append(ref.grid[:, 2].mean(axis=(1, 2)))
        if (t + 1) % stride == 0:
            want["grid"].append(ref.grid.copy())
            want["temp"].append(np.asarray(ref.temp).reshape(B, 8, 8).copy())
            want["idx"].append(ref.agent_indices.copy())
            want["st"].append(ref.agent_states[..., 0].copy())
            want["steps"].append(ref.step_count)
            want["frame_L"].append(L_t)
    want = {k: np.array(v) for k, v in want.items()}

    np.random.seed(17)
    env = amd.RLDaisyWorld(grid_dimension=8, n_agents=N, precision="exact")
    env.batch_size = B
    out = harness.simulate_grazing_frames(env, amd.Greedy(epsilon=0.0), nsteps, stride=stride, tile=1, chunk=16)
    F = nsteps // stride
    assert np.array_equal(out["L"], want["L"])
    assert np.array_equal(out["stats"]["sum_light_k"], np.rint(want["light"] * 64000).astype(np.uint64))
    assert np.array_equal(out["stats"]["sum_dark_k"], np.rint(want["dark"] * 64000).astype(np.uint64))
    assert np.array_equal(out["frame_steps"], want["steps"]) and np.array_equal(out["frame_L"], want["frame_L"])
    assert out["light"].shape == (F, B, 8, 8) and out["agent_pos"].shape == (F, B, N, 2)
    assert np.array_equal(out["cover"]["sum_light_k"], _k(want["grid"][:, :, 1]))
    assert np.array_equal(out["cover"]["sum_dark_k"], _k(want["grid"][:, :, 2]))
    np.testing.assert_allclose(out["temp"], want["temp"], rtol=2e-12, atol=0)
    assert np.array_equal(out["agent_pos"], want["idx"]) and np.array_equal(out["agent_state"], want["st"])
    # the agent channel: the reference writes each agent's store into channel 4 at its position, agent by agent (where
    # several stand on one cell the last one's stays)
    for f in range(F):
        for b in range(B):
            last = {tuple(out["agent_pos"][f, b, n]): out["agent_state"][f, b, n] for n in range(N)}
            for (r, c), state in last.items():
                assert want["grid"][f][b, 4, r, c] == state, (f, b, r, c)
    assert out["stats"]["max_k"].max() > THRESHOLD_K
    assert np.array_equal(env.grid, ref.grid) and env.L == ref.L and env.step_count == ref.step_count == nsteps
    env.close()
