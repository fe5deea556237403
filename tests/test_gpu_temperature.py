"""GPU tests (``-m gpu``) of the per-world temperature statistics: dw_reduce_temperature / Engine.reduce_temperature,
dw_step_n_trace_temperature / Engine.step_n_trace_temperature and the `temperature=True` runs of harness.simulate_ramp.

The statistics are of the local temperature field `temp` (ref daisy_world_rl.py:410,415), float64, un-quantised.  Bounds
against the NumPy oracle (none of them free):
  * 1e-12 relative is what tests/test_gpu_parity.py already asserts per cell for this cache; a mean, a minimum or a maximum
    of values each within r is within r;
  * two population standard deviations differ by at most the largest per-cell difference: absolute, against the world's
    maximum temperature;
  * the factor 2 (mean, std) covers the fixed-order summation (<= log2(n) 2^-53 relative).
Everything else is EXACT equality: min / max against the downloaded cache, determinism, world independence, the state a
temperature trace leaves against the cover-only traces, its records against step + reduce_temperature one call at a time,
chunked against unchunked.

Shapes: one partial workgroup (3x3, 7x5, 3x85, 33x67), several chunks of 4096 cells with a ragged tail (40x320: 12800
cells) and without (64x256), row wrap on tiny grids, and the generic, W == 256 and W >= 256 non-multiple step paths.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import daisy_oracle as O  # noqa: E402

SHAPES = [(1, 3, 3), (3, 7, 5), (2, 3, 85), (2, 33, 67), (1, 64, 256), (2, 40, 320)]
TRACE_SHAPES = [(3, 7, 5), (2, 33, 67), (1, 64, 256), (2, 40, 320)]
PRECISIONS = ("exact", "fast", "f64")
RAMP = (0.8, 1.0, 1.3)
NTRACE = 7                                                   # odd: the un-quantised first step and steady steps both occur
STAT_FIELDS = ("max_k", "sum_light_k", "sum_dark_k")


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _engine(amd, B, H, W, precision="exact", N=0, **over):
    from therldaisyworld_amd import _ffi
    p = amd.default_params(B, H, W, N)
    p.precision = _ffi.PRECISION[precision]
    for k, v in over.items():
        setattr(p, k, v)
    return amd.Engine(p)


@functools.lru_cache(maxsize=None)
def _state(B, H, W):
    """Covers in the reference's init distribution (ref initialize_grid :287-302: dark drawn first), fixed seed; read-only."""
    P = O.Params()
    rng = np.random.RandomState(7000 + 131 * H + W)
    dp, lp = rng.rand(B, 2, H, W), rng.rand(B, 2, H, W)
    dark = 1.0 * (dp[:, 0] < P.dark_proportion) * P.initial_ad * dp[:, 1]
    light = 1.0 * (lp[:, 0] < P.light_proportion) * P.initial_al * lp[:, 1]
    light.flags.writeable = dark.flags.writeable = False
    return light, dark


def _as_f32_upload(x):
    """What the library holds of a float32 natural-unit upload: float32 per-mille, read back as k / 1000 in float64."""
    return (x.astype(np.float32) * np.float32(1000.0)).astype(np.float64) / 1000.0


def _schedule(n, B, per_world):
    """Luminosities from the ramp: (n,) rising, or (n, B) - distinct per world, changing per step, not monotone in b."""
    t = np.arange(n)
    if not per_world:
        return 0.8 + 0.5 * t / max(n - 1, 1)
    base = np.linspace(0.8, 1.3, B + 2)[1:-1][::-1] if B > 1 else np.array([1.0])
    drift = 0.01 * t[:, None] * np.where(np.arange(B) % 2, 1.0, -1.0)[None, :]
    return np.ascontiguousarray(base[None, :] + drift)


@functools.lru_cache(maxsize=None)
def _oracle_temps(B, H, W, fmt, L_key):
    """env.temp after every step of the NumPy oracle: (n, B, H, W).  L_key: the schedule as nested tuples, (n,) or (n, B);
    every world runs on a one-world oracle at its own column (the oracle's L is one number)."""
    L = np.asarray(L_key, dtype=np.float64)
    if L.ndim == 1:
        L = np.repeat(L[:, None], B, axis=1)
    light, dark = _state(B, H, W)
    if fmt == "f32":
        light, dark = _as_f32_upload(light), _as_f32_upload(dark)
    out = np.zeros((L.shape[0], B, H, W))
    for b in range(B):
        o = O.OracleDaisyWorld(grid_dimension=W, n_agents=0, batch_size=1)
        o.L = float(L[0, b])
        o.set_initial_cover(light[b:b + 1].copy(), dark[b:b + 1].copy())
        for t in range(L.shape[0]):
            o.L = float(L[t, b])
            o.grid = o.forward(o.grid)
            out[t, b] = o.temp[0, 0]
    out.flags.writeable = False
    return out


def _key(L):
    return tuple(map(tuple, L)) if np.ndim(L) == 2 else tuple(float(x) for x in L)


def _upload(eng, light, dark, fmt="f64"):
    if fmt == "f32":
        eng.upload_state_f32(light.astype(np.float32), dark.astype(np.float32), quantised=False)
    else:
        eng.upload_state(light, dark)


def _assert_close_to_oracle(rec, temp, what):
    """rec: (B,) temperature records; temp: the oracle's field (B, H, W)."""
    mean, std = temp.mean(axis=(1, 2)), temp.std(axis=(1, 2))
    mn, mx = temp.min(axis=(1, 2)), temp.max(axis=(1, 2))
    err = np.abs(rec["std"] - std)
    print(what, "mean rel", np.max(np.abs(rec["mean"] / mean - 1)), "min rel", np.max(np.abs(rec["min"] / mn - 1)),
          "max rel", np.max(np.abs(rec["max"] / mx - 1)), "std abs / Tmax", np.max(err / mx))
    np.testing.assert_allclose(rec["mean"], mean, rtol=2e-12, atol=0, err_msg=what)
    np.testing.assert_allclose(rec["min"], mn, rtol=1e-12, atol=0, err_msg=what)
    np.testing.assert_allclose(rec["max"], mx, rtol=1e-12, atol=0, err_msg=what)
    assert (err <= 2e-12 * mx).all(), (what, err, mx)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---- 1. on demand against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,fmt", [(*s, "f64") for s in SHAPES] + [(2, 33, 67, "f32")])
def test_on_demand_against_the_oracle(amd, B, H, W, fmt):
    """After the first step (the retained previous state is the un-quantised upload) and after the second (binary16)."""
    temps = _oracle_temps(B, H, W, fmt, RAMP[:2])
    eng = _engine(amd, B, H, W, "exact")
    _upload(eng, *_state(B, H, W), fmt)
    for t in range(2):
        eng.step(RAMP[t])
        rec = eng.reduce_temperature(RAMP[t])
        assert rec.shape == (B,)
        _assert_close_to_oracle(rec, temps[t], f"{(B, H, W)} {fmt} after step {t + 1}")
    eng.close()


# ---- 2. the same cell values as the caches ------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f64", "f32"])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_min_and_max_are_cells_of_the_temps_cache(amd, B, H, W, fmt):
    """Before any step (the upload in its own format, the caller's L), after one step (the upload as the previous state,
    the step's L) and after two (binary16): min and max are bit-equal to the minimum and maximum of download_caches'
    temps[:, 0], and the mean lies between them."""
    eng = _engine(amd, B, H, W, "exact")
    _upload(eng, *_state(B, H, W), fmt)
    for t in range(3):
        L = RAMP[t]
        rec = eng.reduce_temperature(L)
        field = eng.download_caches(L, betas=False, growth=False, temp_effective=False)[0][:, 0]
        assert np.array_equal(rec["min"], field.min(axis=(1, 2))), (t, rec["min"], field.min(axis=(1, 2)))
        assert np.array_equal(rec["max"], field.max(axis=(1, 2))), (t, rec["max"], field.max(axis=(1, 2)))
        assert ((rec["min"] <= rec["mean"]) & (rec["mean"] <= rec["max"])).all()
        np.testing.assert_allclose(rec["mean"], field.mean(axis=(1, 2)), rtol=2e-12, atol=0)
        assert (np.abs(rec["std"] - field.std(axis=(1, 2))) <= 2e-12 * field.max(axis=(1, 2))).all()
        if t < 2:
            eng.step(RAMP[t + 1])                            # (L_last = RAMP[t + 1]: the L the next round passes)
    eng.close()


# ---- 3. uniform and dead worlds -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(3, 7, 5), (2, 33, 67), (2, 40, 320)])
@pytest.mark.parametrize("light,dark", [(0.3, 0.2), (0.0, 0.0)], ids=["uniform", "dead"])
def test_uniform_worlds_have_no_spread(amd, B, H, W, light, dark):
    from therldaisyworld_amd import harness
    eng = _engine(amd, B, H, W, "exact")
    eng.upload_state_f32(np.full((B, H, W), light, np.float32), np.full((B, H, W), dark, np.float32), quantised=True)
    L = 1.0
    eng.step(L)                                              # the retained previous state is the uniform field
    rec = eng.reduce_temperature(L)
    assert (rec["std"] == 0.0).all(), rec["std"]
    assert _bits(rec["min"]) == _bits(rec["max"]) == _bits(rec["mean"]), rec
    if light == 0.0:
        p = eng.params
        env = type("P", (), dict(S=p.S, albedo_bare=p.albedo_bare, sigma=p.sigma))
        np.testing.assert_allclose(rec["mean"], harness.dead_temperature(env, L), rtol=1e-12, atol=0)
    eng.close()


# ---- 4. determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(7, 5), (40, 320)])
def test_deterministic_and_independent_of_the_batch(amd, H, W):
    B = 3
    light, dark = _state(B, H, W)
    eng = _engine(amd, B, H, W, "exact")
    eng.upload_state(light, dark)
    ones = []
    for b in range(B):
        one = _engine(amd, 1, H, W, "exact")
        one.upload_state(light[b:b + 1], dark[b:b + 1])
        ones.append(one)
    for t in range(3):                                       # float64 input, then float64 previous, then binary16
        rec = eng.reduce_temperature(RAMP[t])
        assert _bits(rec) == _bits(eng.reduce_temperature(RAMP[t]))
        for b, one in enumerate(ones):
            assert _bits(one.reduce_temperature(RAMP[t])) == _bits(rec[b:b + 1]), (t, b)
        if t < 2:
            for e in [eng] + ones:
                e.step(RAMP[t + 1])
    for e in [eng] + ones:
        e.close()


# ---- 5. trace -----------------------------------------------------------------------------------------------------------
def _assert_same_state(a, b, what):
    from therldaisyworld_amd import _ffi
    for which in (_ffi.STATE_CURRENT, _ffi.STATE_PREVIOUS):
        for x, y in zip(a.download_planes(which), b.download_planes(which)):
            assert np.array_equal(x, y), (what, "planes", which)
    ra, rb = a.reduce(), b.reduce()
    for f in STAT_FIELDS:
        assert np.array_equal(ra[f], rb[f]), (what, "reduce", f)
    assert a.last_fixup_count() == b.last_fixup_count(), (what, "fix-up count")


def _run_trace_case(amd, B, H, W, precision, per_world):
    """(temps, stats) of the 7-step temperature trace from the float64 upload, after checks (a), (b) and (d)."""
    light, dark = _state(B, H, W)
    L = _schedule(NTRACE, B, per_world)
    what = f"{(B, H, W)} {precision} {'per-world' if per_world else 'shared'}"
    eng, twin, quiet = (_engine(amd, B, H, W, precision) for _ in range(3))
    for e in (eng, twin, quiet):
        e.upload_state(light, dark)
    stats, temps = eng.step_n_trace_temperature(L)
    assert temps.shape == (NTRACE, B) and stats.shape == (NTRACE, B)
    # (a) the state and the cover records of the cover-only trace
    want = twin.step_n_trace_per_world(L) if per_world else twin.step_n_trace(L)
    for f in STAT_FIELDS:
        assert np.array_equal(stats[f], want[f]), (what, f)
    _assert_same_state(eng, twin, what)
    # (d) without the cover records: the same temperatures, the same state
    none, temps_quiet = quiet.step_n_trace_temperature(L, trace=False)
    assert none is None and _bits(temps_quiet) == _bits(temps), what
    _assert_same_state(quiet, twin, what + " trace=None")
    # (b) one call at a time: step, then the statistics of the field that step computed
    if per_world:
        for b in range(B):
            one = _engine(amd, 1, H, W, precision)
            one.upload_state(light[b:b + 1], dark[b:b + 1])
            for t in range(NTRACE):
                one.step(float(L[t, b]))
                assert _bits(one.reduce_temperature(float(L[t, b]))) == _bits(temps[t, b:b + 1]), (what, t, b)
            one.close()
    else:
        one = _engine(amd, B, H, W, precision)
        one.upload_state(light, dark)
        for t in range(NTRACE):
            one.step(float(L[t]))
            assert _bits(one.reduce_temperature(float(L[t]))) == _bits(temps[t]), (what, t)
        one.close()
    for e in (eng, twin, quiet):
        e.close()
    return stats, temps, L


@pytest.mark.parametrize("per_world", [False, True], ids=["shared", "per-world"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("B,H,W", TRACE_SHAPES)
def test_trace(amd, B, H, W, precision, per_world):
    stats, temps, L = _run_trace_case(amd, B, H, W, precision, per_world)
    if precision == "exact":                                 # (c) against the oracle stepped with the same schedule
        want = _oracle_temps(B, H, W, "f64", _key(L))
        for t in range(NTRACE):
            _assert_close_to_oracle(temps[t], want[t], f"{(B, H, W)} step {t}")


def test_per_world_trace_leaves_the_per_world_state(amd):
    from therldaisyworld_amd import _ffi
    B, H, W = 3, 16, 16
    eng = _engine(amd, B, H, W, "exact", N=2)
    eng.init_random(5)
    eng.get_obs(0.9)                                         # not stepped yet: fine
    eng.step_n_trace_temperature(_schedule(4, B, True))
    with pytest.raises(amd.DaisyHipError) as err:
        eng.get_obs(0.9)
    assert err.value.code == _ffi.DW_ESTATE and "per-world" in str(err.value)
    rec = eng.reduce_temperature(1.1)                        # takes the caller's L, as download_caches does
    field = eng.download_caches(1.1, betas=False, growth=False, temp_effective=False)[0][:, 0]
    assert np.array_equal(rec["max"], field.max(axis=(1, 2)))
    eng.step_n_trace_temperature(_schedule(3, B, False))     # a shared-L run: the rule is lifted
    eng.get_obs(0.9)
    eng.close()


# ---- 6. chunking --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_world", [False, True], ids=["shared", "per-world"])
@pytest.mark.parametrize("B,H,W", [(3, 7, 5), (2, 40, 320)])
def test_chunked_download_equals_the_unchunked_run(amd, monkeypatch, B, H, W, per_world):
    light, dark = _state(B, H, W)
    L = _schedule(NTRACE, B, per_world)
    whole = _engine(amd, B, H, W, "exact")
    monkeypatch.setenv("DW_TEST_HOOKS", "1")
    monkeypatch.setenv("DW_TEST_TRACE_ROWS", "2")
    chunked = _engine(amd, B, H, W, "exact")
    assert "DW_TEST_TRACE_ROWS=2" in chunked.kernel_info()
    assert "DW_TEST_TRACE_ROWS" not in whole.kernel_info()
    for e in (whole, chunked):
        e.upload_state(light, dark)
    s0, t0 = whole.step_n_trace_temperature(L)
    s1, t1 = chunked.step_n_trace_temperature(L)
    assert _bits(t0) == _bits(t1)
    for f in STAT_FIELDS:
        assert np.array_equal(s0[f], s1[f]), f
    _assert_same_state(whole, chunked, "chunked")
    whole.close()
    chunked.close()


# ---- 7. errors ----------------------------------------------------------------------------------------------------------
def test_errors(amd):
    from therldaisyworld_amd import _ffi
    lib = _ffi.load()
    B, H, W = 2, 33, 67
    pt = lambda a: a.ctypes.data_as(C.POINTER(_ffi.DwTempStats))
    ps = lambda a: a.ctypes.data_as(C.POINTER(_ffi.DwWorldStats))
    eng = _engine(amd, B, H, W)
    Ls, Lw = _schedule(4, B, False), _schedule(4, B, True)
    temps = np.zeros((4, B), dtype=_ffi.TEMP_STATS_DTYPE)
    stats = np.zeros((4, B), dtype=_ffi.STATS_DTYPE)
    one = np.zeros(B, dtype=_ffi.TEMP_STATS_DTYPE)
    # no state
    assert lib.dw_reduce_temperature(eng._h, 1.0, pt(one)) == _ffi.DW_ESTATE
    for pw, L in ((0, Ls), (1, Lw)):
        assert lib.dw_step_n_trace_temperature(eng._h, 4, _ffi.ptr_d(L), pw, ps(stats), pt(temps)) == _ffi.DW_ESTATE
    eng.upload_state(*_state(B, H, W))
    # null arguments
    assert lib.dw_reduce_temperature(None, 1.0, pt(one)) == _ffi.DW_EINVAL
    assert lib.dw_reduce_temperature(eng._h, 1.0, None) == _ffi.DW_EINVAL
    for pw, L in ((0, Ls), (1, Lw)):
        assert lib.dw_step_n_trace_temperature(None, 4, _ffi.ptr_d(L), pw, ps(stats), pt(temps)) == _ffi.DW_EINVAL
        assert lib.dw_step_n_trace_temperature(eng._h, 4, None, pw, ps(stats), pt(temps)) == _ffi.DW_EINVAL
        assert lib.dw_step_n_trace_temperature(eng._h, 4, _ffi.ptr_d(L), pw, ps(stats), None) == _ffi.DW_EINVAL
        assert lib.dw_step_n_trace_temperature(eng._h, -1, _ffi.ptr_d(L), pw, ps(stats), pt(temps)) == _ffi.DW_EINVAL
    # a per-world luminosity that is none: refused before anything runs
    before = eng.download_planes()
    for bad in (np.nan, -0.5, np.inf):
        Lb = Lw.copy()
        Lb[2, 1] = bad
        assert lib.dw_step_n_trace_temperature(eng._h, 4, _ffi.ptr_d(Lb), 1, ps(stats), pt(temps)) == _ffi.DW_EINVAL
        assert b"luminosity" in lib.dw_last_error()
    # nsteps == 0: nothing happens, nothing is written
    temps["mean"] = -7.0
    for pw, L in ((0, Ls), (1, Lw)):
        assert lib.dw_step_n_trace_temperature(eng._h, 0, _ffi.ptr_d(L), pw, ps(stats), pt(temps)) == _ffi.DW_OK
    assert (temps["mean"] == -7.0).all() and not temps["max"].any()
    for x, y in zip(before, eng.download_planes()):
        assert np.array_equal(x, y)
    with pytest.raises(ValueError, match="shape"):
        eng.step_n_trace_temperature(np.ones((4, B + 1)))
    eng.close()


# ---- 8. harness ---------------------------------------------------------------------------------------------------------
def test_simulate_ramp_with_temperature(amd):
    from therldaisyworld_amd.harness import simulate_ramp
    n, B = 9, 3

    def dropin():
        np.random.seed(77)
        env = amd.RLDaisyWorld(grid_dimension=16, n_agents=0)
        env.batch_size = B
        return env

    env = dropin()
    out = simulate_ramp(env, n, temperature=True)
    np.random.seed(77)
    ref = O.OracleDaisyWorld.like_reference_ctor(grid_dimension=16, n_agents=0)
    ref.P.batch_size = B
    ref.reset()
    for t in range(n):
        assert out["L"][t] == ref.L
        ref.step()
        rec = np.zeros(B, dtype=[("mean", "f8"), ("std", "f8"), ("min", "f8"), ("max", "f8")])
        for f, key in (("mean", "mean_temp"), ("std", "std_temp"), ("min", "min_temp"), ("max", "max_temp")):
            assert out[key].shape == (n, B)
            rec[f] = out[key][t]
        _assert_close_to_oracle(rec, ref.temp[:, 0], f"ramp step {t}")
        np.testing.assert_allclose(out["dead_temp"][t], ref.dead_temp[0], rtol=4e-15, atol=0)
    assert out["dead_temp"].shape == out["L"].shape == (n,)
    # the cover entries: those of a temperature=False run from the same seed
    env2 = dropin()
    plain = simulate_ramp(env2, n)
    assert set(out) - set(plain) == {"mean_temp", "std_temp", "min_temp", "max_temp", "dead_temp"}
    for key in ("L", "mean_light", "mean_dark", "max_cover", "alive"):
        assert np.array_equal(out[key], plain[key]), key
    for f in STAT_FIELDS:
        assert np.array_equal(out["stats"][f], plain["stats"][f]), f
    # ... and the environment goes on as after simulate_ramp today
    assert env.step_count == n == env2.step_count and env.L == ref.L == env2.L
    assert np.array_equal(env.grid, ref.grid) and np.array_equal(env.grid, env2.grid)
    for e in (env, env2, ref):
        e.step()
    assert np.array_equal(env.grid, ref.grid) and np.array_equal(env2.grid, ref.grid)
    env.close()
    env2.close()


def test_luminosity_sweep_with_temperature(amd):
    """Every world at its own luminosity: the curves are (n, B), dead_temp too, and the covers are the plain sweep's."""
    from therldaisyworld_amd.harness import dead_temperature, simulate_luminosity_sweep
    n, B = 5, 3
    Lv = np.array([1.2, 0.8, 1.0])
    outs = []
    for temperature in (True, False):
        np.random.seed(3)
        env = amd.RLDaisyWorld(grid_dimension=16, n_agents=0)
        env.batch_size = B
        outs.append(simulate_luminosity_sweep(env, Lv, n, temperature=temperature))
        env.close()
    out, plain = outs
    for key in ("mean_temp", "std_temp", "min_temp", "max_temp", "dead_temp"):
        assert out[key].shape == (n, B) and key not in plain
    assert np.array_equal(out["dead_temp"], dead_temperature(env, out["L"]))
    assert ((out["min_temp"] <= out["mean_temp"]) & (out["mean_temp"] <= out["max_temp"])).all()
    for f in STAT_FIELDS:
        assert np.array_equal(out["stats"][f], plain["stats"][f]), f
