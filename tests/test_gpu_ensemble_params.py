"""GPU tests (``-m gpu``) of dw_step_n_trace_ensemble / Engine.step_n_trace_ensemble / harness.simulate_parameter_sweep:
every world of a handle stepped with physics constants AND a luminosity of its own.  The contract is independence -
world b ends exactly where a ONE-world handle that carries its constants (dw_set_params) and steps with its column
ends - so every comparison with such handles is EXACT equality: trace rows, current and retained previous planes,
reduce() and the fix-up count, in all three precisions, from quantised and un-quantised states, on shapes that take the
per-world step pairs (float32-only mode on overlapped and rotating strips), the per-world wave-strip single steps (the
exact mode there, and the ring shape) and the generic kernel.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import daisy_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("max_k", "sum_light_k", "sum_dark_k")
# two overlapped strips (a partial one) | rotating strips, three row strips | the ring: single wave-strip steps | generic
SHAPES = [(3, 70, 320), (3, 130, 256), (2, 40, 1024), (4, 64, 64), (3, 37, 52)]
FORMS = ["step pairs", "step pairs", "wave strips", "generic", "generic"]
PRECISIONS = ("exact", "fast", "f64")
NSTEPS = 9                                                   # the first step, pairs, and a closing single step


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _params(amd, B, H, W, precision="exact", **over):
    from therldaisyworld_amd import _ffi
    p = amd.default_params(B, H, W, 0)
    p.precision = _ffi.PRECISION[precision]
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _engine(amd, B, H, W, precision="exact", **over):
    return amd.Engine(_params(amd, B, H, W, precision, **over))


def _table(eng, B, offset=0):
    """The mixed parameter table, per world and cycled from `offset`: the defaults | q2 = 0 | q2 = q/8 | asymmetric albedos
    with another gamma | another temp_optimal and dt."""
    own = eng.world_params()
    tab = np.repeat(own[None], B)
    for b in range(B):
        kind = (b + offset) % 5
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
    """(n, B): distinct luminosities per world within 0.6 ... 1.7, not monotone in b, drifting by 0.036 over the run (odd worlds up,
    even worlds down)."""
    base = np.linspace(0.65, 1.6, B)[np.random.RandomState(B).permutation(B)]
    drift = 0.036 * (np.arange(n) / max(n - 1, 1))[:, None] * np.where(np.arange(B) % 2, 1.0, -1.0)[None, :]
    L = np.ascontiguousarray(base[None, :] + drift)
    assert L.min() >= 0.6 and L.max() <= 1.7
    return L


def _blocky_state(B, H, W, seed):
    """An un-quantised float64 state made of uniform blocks - whole regions of EQUAL covers, one of them exactly 1.000 -
    beside a noisy region."""
    rng = np.random.RandomState(seed)
    light = np.zeros((B, H, W))
    dark = np.zeros((B, H, W))
    h2, w2 = H // 2, W // 2
    light[:, :h2, :w2] = 0.4
    dark[:, :h2, w2:] = 0.3
    light[:, h2:, :w2] = 0.2 * rng.rand(B, H - h2, w2)
    dark[:, h2:, :w2] = 0.2 * rng.rand(B, H - h2, w2)
    light[:, h2:, w2:] = 1.0
    return light, dark


def _init(eng, how, seed, state=None, world=None):
    if how == "philox":
        eng.init_random(seed)                               # un-quantised: the first step reads the float32 state
    elif how == "philox_q":
        eng.init_random(seed, quantised=True)
    else:
        light, dark = state
        eng.upload_state(*(state if world is None else (light[world:world + 1], dark[world:world + 1])))


def _assert_rows_equal(a, b, what=""):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), (what, f, np.argwhere(a[f] != b[f])[:5].tolist())


def _world_by_world(amd, B, H, W, precision, how, seed, tab, L, state=None):
    """The reference: world b alone on a fresh one-world handle (world_offset = b: Philox draws the same world) that is
    given the world's constants by dw_set_params, dw_step + dw_reduce per step with column b."""
    from therldaisyworld_amd import _ffi
    rows = np.zeros(L.shape, dtype=_ffi.STATS_DTYPE)
    cur, prev, red, fix = [], [], [], 0
    for b in range(B):
        one = _engine(amd, 1, H, W, precision, world_offset=b)
        p = _params(amd, 1, H, W, precision, world_offset=b)
        for name in _ffi.WORLD_PARAM_NAMES:
            setattr(p, name, float(tab[b][name]))
        one.set_params(p)
        _init(one, how, seed, state, b)
        for t in range(L.shape[0]):
            one.step(float(L[t, b]))
            rows[t, b] = one.reduce()[0]
        cur.append(one.download_planes())
        prev.append(one.download_planes(_ffi.STATE_PREVIOUS))
        red.append(one.reduce()[0])
        fix += one.last_fixup_count()
        one.close()
    cat = lambda pairs: tuple(np.concatenate([p[i] for p in pairs]) for i in (0, 1))
    return rows, cat(cur), cat(prev), np.array(red, dtype=_ffi.STATS_DTYPE), fix


# the table's starting row per kind of state: between them every shape sees an all-symmetric table (the SYM kernels) and
# tables with the asymmetric world (SYM = false for the whole call)
OFFSET = {"philox": 0, "philox_q": 2, "upload": 3}


@pytest.mark.parametrize("how", ["philox", "philox_q", "upload"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_every_world_is_stepped_as_if_alone(amd, B, H, W, precision, how):
    from therldaisyworld_amd import _ffi
    state = _blocky_state(B, H, W, 5) if how == "upload" else None
    L = _schedule(NSTEPS, B)
    what = f"{(B, H, W)} {precision} {how}"
    eng = _engine(amd, B, H, W, precision)
    own = eng.world_params().copy()
    tab = _table(eng, B, OFFSET[how])
    _init(eng, how, 11, state)
    tr = eng.step_n_trace_ensemble(tab, L)
    rows, cur, prev, red, fix = _world_by_world(amd, B, H, W, precision, how, 11, tab, L, state)
    _assert_rows_equal(tr, rows, what)
    for a, b in zip(eng.download_planes(), cur):
        assert np.array_equal(a, b), (what, "current planes", np.argwhere(a != b)[:5].tolist())
    for a, b in zip(eng.download_planes(_ffi.STATE_PREVIOUS), prev):
        assert np.array_equal(a, b), (what, "previous planes")
    _assert_rows_equal(eng.reduce()[None], red[None], what + " reduce")
    assert eng.last_fixup_count() == fix, (what, "fix-up count")
    assert eng.world_params() == own                        # the handle's own set is unchanged
    eng.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _hold_rows(monkeypatch, trace_rows):
    """Handles created from now on hold `trace_rows` rows of the series (and of the tables) on the device at a time."""
    monkeypatch.setenv("DW_TEST_HOOKS", "1")
    monkeypatch.setenv("DW_TEST_TRACE_ROWS", trace_rows)


@pytest.mark.parametrize("trace_rows", [None, "4"], ids=["one-chunk", "rows=4"])
@pytest.mark.parametrize("precision", ("exact", "fast"))
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_own_constants_are_the_per_world_luminosity_run(amd, monkeypatch, B, H, W, precision, trace_rows):
    """Every row the handle's own set: planes, trace and temps of dw_step_n_trace_per_world /
    dw_step_n_trace_temperature(per_world = 1) on a twin handle, bit for bit - also when the handles hold only four rows
    of the series (and of the tables) on the device at a time."""
    from therldaisyworld_amd import _ffi
    if trace_rows:
        _hold_rows(monkeypatch, trace_rows)
    L = _schedule(13, B)
    what = f"{(B, H, W)} {precision}"
    for temperature in (False, True):
        a, b = _engine(amd, B, H, W, precision), _engine(amd, B, H, W, precision)
        if trace_rows:
            assert "DW_TEST_TRACE_ROWS=4" in a.kernel_info()
        for e in (a, b):
            e.init_random(11)
        tab = np.repeat(a.world_params()[None], B)
        if temperature:
            tr, temps = a.step_n_trace_ensemble(tab, L, temperature=True)
            ref, ref_temps = b.step_n_trace_temperature(L)
            for f in ("mean", "std", "min", "max"):
                assert np.array_equal(_bits(temps[f]), _bits(ref_temps[f])), (what, f)
        else:
            tr = a.step_n_trace_ensemble(tab, L)
            ref = b.step_n_trace_per_world(L)
        _assert_rows_equal(tr, ref, what)
        for which in (_ffi.STATE_CURRENT, _ffi.STATE_PREVIOUS):
            for x, y in zip(a.download_planes(which), b.download_planes(which)):
                assert np.array_equal(x, y), (what, which, temperature)
        _assert_rows_equal(a.reduce()[None], b.reduce()[None], what + " reduce")
        assert a.last_fixup_count() == b.last_fixup_count()
        assert a.step_n_trace_ensemble(tab, L[:3], trace=False) is None
        a.close()
        b.close()


@pytest.mark.parametrize("how", ["philox_q", "philox"])
def test_chunks_of_the_table_and_of_the_series_drift_apart(amd, monkeypatch, how):
    """The rows=4 run of the test above on the smallest shape that takes step pairs, 11 steps, constant luminosities for
    steps 0-4 and distinct ones afterwards: steps at equal luminosities share a table row, so the chunks of the table
    (4 single-step rows, 2 pair rows) end elsewhere than those of the series (4 rows).  Trace and planes equal the one-chunk
    run's bit for bit, with the mixed table and with the handle's own set in every row; the latter with equal columns is
    dw_step_n_trace."""
    from therldaisyworld_amd import _ffi
    shapes = []
    for shape in sorted(SHAPES, key=lambda s: s[0] * s[1] * s[2]):
        probe = _engine(amd, *shape, "fast")
        if probe.kernel_info().endswith("; per-world constants: step pairs"):
            shapes.append(shape)
        probe.close()
    B, H, W = shapes[0]
    L = _schedule(11, B)
    L[:5] = L[0]
    assert len({row.tobytes() for row in L}) == 7
    shared = np.repeat(L[:, :1], B, axis=1)
    whole = [_engine(amd, B, H, W, "fast") for _ in range(3)]          # mixed table | own set | dw_step_n_trace
    _hold_rows(monkeypatch, "4")
    chunked = [_engine(amd, B, H, W, "fast") for _ in range(3)]
    assert all("DW_TEST_TRACE_ROWS=4" in e.kernel_info() for e in chunked)
    assert not any("DW_TEST_TRACE_ROWS" in e.kernel_info() for e in whole)
    for e in whole + chunked:
        _init(e, how, 11)
    own = np.repeat(whole[0].world_params()[None], B)
    traces = [[e[0].step_n_trace_ensemble(_table(e[0], B, 1), L), e[1].step_n_trace_ensemble(own, shared),
               e[2].step_n_trace(shared[:, 0])] for e in (whole, chunked)]
    for i, what in enumerate(("mixed table", "own set", "dw_step_n_trace")):
        _assert_rows_equal(traces[1][i], traces[0][i], f"{what}: rows=4 against one chunk")
        for which in (_ffi.STATE_CURRENT, _ffi.STATE_PREVIOUS):
            for x, y in zip(chunked[i].download_planes(which), whole[i].download_planes(which)):
                assert np.array_equal(x, y), (what, which)
    for run, engines in zip(traces, (whole, chunked)):
        _assert_rows_equal(run[1], run[2], "own set, equal columns: dw_step_n_trace")
        for x, y in zip(engines[1].download_planes(), engines[2].download_planes()):
            assert np.array_equal(x, y)
    for e in whole + chunked:
        e.close()


def _k(x):
    return np.rint(np.asarray(x) * 1000.0).astype(np.int64)


@pytest.mark.parametrize("B,H,W", [(4, 64, 64), (3, 70, 320)])
def test_ensemble_run_equals_the_oracle(amd, B, H, W):
    """Exact mode against the float64 NumPy oracle, 41 steps with the mixed table (offset 1: q2 = 0, q2 = q/8, the
    asymmetric world, ...): one oracle environment per world with its attributes set.  Planes equal at every 10th step
    and at the end - of the cover-only run and of the run with temperature records - and
    the temperature records within the tolerances tests/test_gpu_temperature.py holds the same quantities to."""
    from therldaisyworld_amd import _ffi
    n = 41
    rng = np.random.RandomState(1000 + W)
    light, dark = 0.3 * rng.rand(B, H, W), 0.3 * rng.rand(B, H, W)
    L = _schedule(n, B)
    plain, withT = _engine(amd, B, H, W, "exact"), _engine(amd, B, H, W, "exact")
    tab = _table(plain, B, 1)
    oracles = []
    for b in range(B):
        o = O.OracleDaisyWorld(grid_dimension=W, n_agents=0, batch_size=1)
        for name in _ffi.WORLD_PARAM_NAMES:
            setattr(o.P, name, float(tab[b][name]))
        o.L = float(L[0, b])
        o.set_initial_cover(light[b:b + 1].copy(), dark[b:b + 1].copy())
        oracles.append(o)
    for e in (plain, withT):
        e.upload_state(light, dark)
    t = 0
    while t < n:
        seg = min(10, n - t)                                # planes are compared after steps 10, 20, 30, 40 and 41
        stats = plain.step_n_trace_ensemble(tab, L[t:t + seg])
        stats_T, temps = withT.step_n_trace_ensemble(tab, L[t:t + seg], temperature=True)
        _assert_rows_equal(stats, stats_T, f"step {t}")
        for s in range(seg):
            field = np.zeros((B, H, W))
            for b, o in enumerate(oracles):
                o.L = float(L[t + s, b])
                o.grid = o.forward(o.grid)
                field[b] = o.temp[0, 0]
            rec = temps[s]
            mean, std = field.mean(axis=(1, 2)), field.std(axis=(1, 2))
            mn, mx = field.min(axis=(1, 2)), field.max(axis=(1, 2))
            what = f"{(B, H, W)} step {t + s}"
            np.testing.assert_allclose(rec["mean"], mean, rtol=2e-12, atol=0, err_msg=what)
            np.testing.assert_allclose(rec["min"], mn, rtol=1e-12, atol=0, err_msg=what)
            np.testing.assert_allclose(rec["max"], mx, rtol=1e-12, atol=0, err_msg=what)
            assert (np.abs(rec["std"] - std) <= 2e-12 * mx).all(), what
        t += seg
        want_l = np.concatenate([o.grid[:, 1] for o in oracles])
        want_d = np.concatenate([o.grid[:, 2] for o in oracles])
        for e in (plain, withT):
            gl, gd = e.download_planes()
            assert np.array_equal(_k(gl), _k(want_l)) and np.array_equal(_k(gd), _k(want_d)), (t, e is withT)
    assert t == n
    plain.close()
    withT.close()


def test_rules(amd):
    import ctypes as C
    from therldaisyworld_amd import _ffi
    lib = _ffi.load()
    B, H, W = 3, 64, 64
    p = _params(amd, B, H, W, "exact", n_agents=2)
    eng = amd.Engine(p)
    eng.init_random(5)
    L = _schedule(4, B)
    tab = _table(eng, B)
    wp = lambda t: t.ctypes.data_as(C.POINTER(_ffi.DwWorldParams))
    no_trace, no_temps = C.POINTER(_ffi.DwWorldStats)(), C.POINTER(_ffi.DwTempStats)()
    call = lambda h, n, t, l: lib.dw_step_n_trace_ensemble(h, n, wp(t) if t is not None else None, l, no_trace, no_temps)
    assert call(eng._h, 0, tab, _ffi.ptr_d(L)) == _ffi.DW_OK            # nsteps == 0: a no-op
    fresh = amd.Engine(p)
    assert call(fresh._h, 4, tab, _ffi.ptr_d(L)) == _ffi.DW_ESTATE
    fresh.close()
    params_before = _ffi.DwParams()
    _ffi.check(lib.dw_get_params(eng._h, C.byref(params_before)))
    before, red_before = eng.download_planes(), eng.reduce()

    def untouched():
        for x, y in zip(before, eng.download_planes()):
            assert np.array_equal(x, y)
        assert np.array_equal(red_before, eng.reduce())

    assert call(eng._h, 4, None, _ffi.ptr_d(L)) == _ffi.DW_EINVAL and b"null" in lib.dw_last_error()
    assert call(eng._h, 4, tab, None) == _ffi.DW_EINVAL and b"null" in lib.dw_last_error()
    for bad in (np.nan, -0.5, np.inf):
        Lb = L.copy()
        Lb[2, 1] = bad
        assert call(eng._h, 4, tab, _ffi.ptr_d(Lb)) == _ffi.DW_EINVAL
        assert b"luminosity" in lib.dw_last_error() and b"world 1" in lib.dw_last_error()
    bad_tab = tab.copy()
    bad_tab["g"][2] = -0.001                                # a growth curve opening upwards: float64 arithmetic only
    assert call(eng._h, 4, bad_tab, _ffi.ptr_d(L)) == _ffi.DW_EINVAL
    assert b"worlds[2].g" in lib.dw_last_error(), lib.dw_last_error()
    untouched()
    f64 = _engine(amd, B, H, W, "f64")
    f64.init_random(5)
    f64.step_n_trace_ensemble(bad_tab, L)                   # ... and accepted there
    f64.close()

    own = eng.world_params().copy()
    eng.get_obs(0.9)                                        # not stepped yet: fine
    eng.step_n_trace_ensemble(tab, L)
    for fn in (lambda: eng.get_obs(0.9), lambda: eng.download_grid(0.9), lambda: eng.download_caches(0.9),
               lambda: eng.reduce_temperature(0.9)):
        with pytest.raises(amd.DaisyHipError) as err:
            fn()
        assert err.value.code == _ffi.DW_ESTATE and "per-world" in str(err.value)
    eng.download_planes(), eng.reduce()                     # keep working
    assert eng.world_params() == own
    q = _ffi.DwParams()
    _ffi.check(lib.dw_get_params(eng._h, C.byref(q)))
    assert bytes(q) == bytes(params_before)                 # dw_get_params is unchanged
    eng.snapshot_save()
    eng.step(1.0)                                           # ONE shared-L step, and everything works again
    eng.get_obs(0.9), eng.download_grid(0.9), eng.download_caches(0.9), eng.reduce_temperature(0.9)
    eng.snapshot_restore()                                  # back to the per-world state: the mark is restored
    for fn in (lambda: eng.download_grid(0.9), lambda: eng.download_caches(0.9), lambda: eng.reduce_temperature(0.9)):
        with pytest.raises(amd.DaisyHipError) as err:
            fn()
        assert err.value.code == _ffi.DW_ESTATE
    # after the per-world LUMINOSITY run the caches keep working, as ever: one constant set, the caller's luminosity
    eng.step(1.0)
    eng.step_n_trace_per_world(L)
    eng.download_caches(0.9), eng.reduce_temperature(0.9)
    eng.close()


@pytest.mark.parametrize("shape,form", list(zip(SHAPES, FORMS)))
def test_kernel_info_names_the_form(amd, shape, form):
    """Step pairs in the float32-only mode; the exact pair kernel was left out (it did not keep the shared-L kernel's row
    loop, csrc/dw_step_fused_pw.hpp), so the exact mode takes wave-strip single steps on those shapes."""
    eng = _engine(amd, *shape, "fast")
    info = eng.kernel_info()
    assert info.endswith(f"; per-world constants: {form}"), info
    eng.close()
    eng = _engine(amd, *shape, "exact")
    assert eng.kernel_info().endswith("; per-world constants: " + ("wave strips" if form == "step pairs" else form))
    eng.close()
    eng = _engine(amd, *shape, "f64")                       # float64 arithmetic: always the generic kernel
    assert eng.kernel_info().endswith("; per-world constants: generic")
    eng.close()


def test_parameter_sweep_harness(amd):
    """The q2 figure on 6 worlds of 64 x 64, 24 steps with temperature records, in one call: array for array the three
    simulate_ramp(temperature=True) runs of environments with q2 assigned."""
    from therldaisyworld_amd import harness
    B, n = 6, 24

    def fresh_env():
        np.random.seed(42)
        env = amd.RLDaisyWorld(grid_dimension=64, n_agents=0)
        env.batch_size = B
        env.reset()
        return env

    env = fresh_env()
    q = env.q
    q2 = np.repeat([0.0, q / 64.0, q / 8.0], 2)
    L_before = env.L
    out = amd.simulate_parameter_sweep(env, {"q2": q2}, n, obs=True, temperature=True)
    assert out["L"].shape == (n, B) and out["dead_temp"].shape == (n, B) and np.array_equal(out["params"]["q2"], q2)
    assert out["params"]["gamma"].tolist() == [env.gamma] * B and env.q2 == q / 8.0
    for value in (0.0, q / 64.0, q / 8.0):
        ref = fresh_env()
        ref.q2 = value
        assert ref.L == L_before
        want = amd.simulate_ramp(ref, n, obs=True, temperature=True)
        cols = np.flatnonzero(q2 == value)
        assert len(cols) == 2
        for key in ("mean_light", "mean_dark", "max_cover", "alive", "mean_temp", "std_temp", "min_temp", "max_temp"):
            assert np.array_equal(out[key][:, cols], want[key][:, cols]), (value, key)
        for f in FIELDS:
            assert np.array_equal(out["stats"][f][:, cols], want["stats"][f][:, cols]), (value, f)
        for b in cols:
            assert np.array_equal(out["L"][:, b], want["L"])
            assert np.array_equal(out["dead_temp"][:, b], harness.dead_temperature(ref, want["L"])), b
        assert env.L == ref.L                               # the environment's ramp advanced with the run
        ref.close()
    assert not np.array_equal(out["mean_temp"][:, 0], out["mean_temp"][:, 4])      # the three settings differ
    with pytest.raises(RuntimeError, match=r"reset\(\)"):
        env.step()
    env.reset()
    env.step()
    # luminosities per world, as simulate_luminosity_sweep reads them; scalars apply to every world
    out2 = amd.simulate_parameter_sweep(env, {"q2": q2, "gamma": 0.3}, 5, L_values=np.linspace(0.7, 1.5, B))
    assert out2["L"].shape == (5, B) and out2["params"]["gamma"].tolist() == [0.3] * B and "dead_temp" not in out2
    env.close()


_ALLOC_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import therldaisyworld_amd as amd
from therldaisyworld_amd import _ffi
p = amd.default_params(3, 40, 512, 0)
L = np.array([[0.7, 1.0, 1.4]] * 5)
eng, ref = amd.Engine(p), amd.Engine(p)
tab = np.repeat(eng.world_params()[None], 3)
tab["q2"] = [0.0, tab["q"][0] / 64, tab["q"][0] / 8]
for e in (eng, ref):
    e.init_random(9, quantised=True)                     # straight into the binary16 planes: no group allocated
before = eng.download_planes()
try:
    eng.step_n_trace_ensemble(tab, L)                    # the tables' group cannot be allocated
except amd.DaisyHipError as err:
    assert err.code == _ffi.DW_ENOMEM, err
else:
    raise SystemExit("the injected allocation failure was not reported")
assert all(np.array_equal(x, y) for x, y in zip(before, eng.download_planes()))
tr = eng.step_n_trace_ensemble(tab, L)                   # the hook is spent
want = ref.step_n_trace_ensemble(tab, L)
assert all(np.array_equal(tr[f], want[f]) for f in ("max_k", "sum_light_k", "sum_dark_k"))
assert all(np.array_equal(x, y) for x, y in zip(eng.download_planes(), ref.download_planes()))
print("ok")
"""


def test_failed_table_allocation_is_reported_and_retryable():
    env = dict(os.environ, DW_TEST_HOOKS="1", DW_TEST_FAIL_GROUP_ALLOC="1")
    p = subprocess.run([sys.executable, "-c", _ALLOC_SCRIPT, ROOT], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.returncode, p.stdout[-500:], p.stderr[-2000:])
