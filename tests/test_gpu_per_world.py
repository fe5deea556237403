"""GPU tests (``-m gpu``) of dw_step_n_trace_per_world / Engine.step_n_trace_per_world / harness.simulate_luminosity_sweep:
every world of a handle stepped at a luminosity of its own.  The contract is independence - world b ends exactly where a
ONE-world handle stepped with column b of the schedule ends - so every comparison is EXACT equality: trace rows, current
and retained previous planes, reduce() and the fix-up count, in all three precisions, from quantised and un-quantised
states, on shapes that take the per-world wave-strip kernels (W >= 256) and on shapes that take the generic one.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import c_oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("max_k", "sum_light_k", "sum_dark_k")
SHAPES = [(6, 70, 320), (4, 96, 512), (3, 130, 4096), (5, 80, 1024), (3, 130, 256), (16, 16, 16), (4, 64, 64), (3, 37, 52)]
NSTEPS = (1, 2, 3, 9)
PRECISIONS = ("exact", "fast", "f64")


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _engine(amd, B, H, W, precision="exact", **over):
    from therldaisyworld_amd import _ffi
    p = amd.default_params(B, H, W, 0)
    p.precision = _ffi.PRECISION[precision]
    for k, v in over.items():
        setattr(p, k, v)
    return amd.Engine(p)


def _k(x):
    return np.rint(np.asarray(x) * 1000.0).astype(np.int64)


def _columns(B, lo=0.6, hi=1.7):
    """One luminosity per world, spread over lo ... hi and NOT monotone in b."""
    base = np.linspace(lo, hi, B)
    order = np.random.RandomState(B).permutation(B)
    if B >= 3 and (np.all(np.diff(order) > 0) or np.all(np.diff(order) < 0)):
        order[[0, 1]] = order[[1, 0]]
    return base[order]


def _schedule(n, B):
    """(n, B): the columns of _columns, each drifting a little from step to step (odd worlds up, even worlds down)."""
    drift = 0.004 * np.arange(n)[:, None] * np.where(np.arange(B) % 2, 1.0, -1.0)[None, :]
    return np.ascontiguousarray(_columns(B)[None, :] + drift)


def _blocky_state(B, H, W, seed):
    """An un-quantised float64 state made of uniform blocks - whole regions of EQUAL covers, one of them exactly 1.000 -
    beside a noisy region; the last world all equal."""
    rng = np.random.RandomState(seed)
    light = np.zeros((B, H, W))
    dark = np.zeros((B, H, W))
    h2, w2 = H // 2, W // 2
    light[:, :h2, :w2] = 0.4
    dark[:, :h2, w2:] = 0.3
    light[:, h2:, :w2] = 0.2 * rng.rand(B, H - h2, w2)
    dark[:, h2:, :w2] = 0.2 * rng.rand(B, H - h2, w2)
    light[:, h2:, w2:] = 1.0
    if B > 1:
        light[-1] = 0.25
        dark[-1] = 0.25
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


def _world_by_world(amd, B, H, W, precision, how, seed, L, state=None):
    """The reference: world b alone on a fresh one-world handle (world_offset = b: Philox draws the same world), dw_step +
    dw_reduce per step with column b.  Returns rows (n, B), current planes, previous planes, final reduce, fix-up sum."""
    from therldaisyworld_amd import _ffi
    rows = np.zeros(L.shape, dtype=_ffi.STATS_DTYPE)
    cur, prev, red, fix = [], [], [], 0
    for b in range(B):
        one = _engine(amd, 1, H, W, precision, world_offset=b)
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


@pytest.mark.parametrize("how", ["philox", "philox_q", "upload"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_every_world_is_stepped_as_if_alone(amd, B, H, W, precision, how):
    from therldaisyworld_amd import _ffi
    state = _blocky_state(B, H, W, 5) if how == "upload" else None
    for n in NSTEPS:
        L = _schedule(n, B)
        what = f"{(B, H, W)} {precision} {how} n={n}"
        eng = _engine(amd, B, H, W, precision)
        _init(eng, how, 11, state)
        tr = eng.step_n_trace_per_world(L)
        rows, cur, prev, red, fix = _world_by_world(amd, B, H, W, precision, how, 11, L, state)
        _assert_rows_equal(tr, rows, what)
        for a, b in zip(eng.download_planes(), cur):
            assert np.array_equal(a, b), (what, "current planes")
        for a, b in zip(eng.download_planes(_ffi.STATE_PREVIOUS), prev):
            assert np.array_equal(a, b), (what, "previous planes")
        _assert_rows_equal(eng.reduce()[None], red[None], what + " reduce")
        assert eng.last_fixup_count() == fix, (what, "fix-up count")
        eng.close()


@pytest.mark.parametrize("trace_rows", [None, "4"], ids=["one-chunk", "rows=4"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("B,H,W", [(2, 70, 320), (3, 130, 256), (4, 64, 64), (3, 37, 52)])
def test_equal_columns_are_the_shared_luminosity_run(amd, monkeypatch, B, H, W, precision, trace_rows):
    """All columns equal: the same series and the same state as dw_step_n_trace on a twin handle (which records step pairs
    on the wide shapes), also when both hold only four rows of the series (and of the table) on the device at a time."""
    from therldaisyworld_amd import _ffi
    if trace_rows:
        monkeypatch.setenv("DW_TEST_HOOKS", "1")
        monkeypatch.setenv("DW_TEST_TRACE_ROWS", trace_rows)
    Ls = 0.8 + (1.55 - 0.8) * np.arange(41) / 40.0
    a, b = _engine(amd, B, H, W, precision), _engine(amd, B, H, W, precision)
    if trace_rows:
        assert "DW_TEST_TRACE_ROWS=4" in a.kernel_info()
    for e in (a, b):
        e.init_random(11)
    tr = a.step_n_trace_per_world(np.repeat(Ls[:, None], B, axis=1))
    ref = b.step_n_trace(Ls)
    what = f"{(B, H, W)} {precision}"
    _assert_rows_equal(tr, ref, what)
    for which in (_ffi.STATE_CURRENT, _ffi.STATE_PREVIOUS):
        for x, y in zip(a.download_planes(which), b.download_planes(which)):
            assert np.array_equal(x, y), (what, which)
    _assert_rows_equal(a.reduce()[None], b.reduce()[None], what + " reduce")
    assert a.last_fixup_count() == b.last_fixup_count()
    assert a.step_n_trace_per_world(np.repeat(Ls[:3, None], B, axis=1), trace=False) is None
    a.close()
    b.close()


def _oracle_run(light, dark, L):
    """Every world through c_oracle.forward with its own luminosity, step by step; returns the int64 series."""
    n, B = L.shape
    out = {f: np.zeros((n, B), dtype=np.int64) for f in FIELDS}
    for t in range(n):
        for b in range(B):
            g = c_oracle.forward(light[b:b + 1], dark[b:b + 1], float(L[t, b]))
            light[b], dark[b] = g[0, 1], g[0, 2]
        kl, kd = _k(light), _k(dark)
        out["max_k"][t] = np.maximum(kl.max(axis=(1, 2)), kd.max(axis=(1, 2)))
        out["sum_light_k"][t] = kl.sum(axis=(1, 2))
        out["sum_dark_k"][t] = kd.sum(axis=(1, 2))
    return out


def _oracle_state(B, H, W):
    rng = np.random.RandomState(1000 + W)
    return 0.3 * rng.rand(B, H, W), 0.3 * rng.rand(B, H, W)


@pytest.mark.parametrize("B,H,W,n", [(6, 70, 320, 41), (4, 64, 64, 41), (2, 130, 4096, 9)])
def test_per_world_run_equals_the_oracle(amd, B, H, W, n):
    """Exact mode against the float64 C oracle, each world with its own L: planes and integer statistics bit-identical.
    The 41-step runs must span the diagram - judged on the ORACLE's series: a dead world and a populated one."""
    light, dark = _oracle_state(B, H, W)
    L = np.ascontiguousarray(np.repeat(_columns(B)[None, :], n, axis=0))
    eng = _engine(amd, B, H, W, "exact")
    eng.upload_state(light, dark)
    tr = eng.step_n_trace_per_world(L)
    want = _oracle_run(light, dark, L)
    if n == 41:
        assert (want["max_k"][-1] == 0).any() and (want["max_k"][-1] >= 500).any(), want["max_k"][-1]
    for f in FIELDS:
        assert np.array_equal(tr[f].astype(np.int64), want[f]), f
    gl, gd = eng.download_planes()
    assert np.array_equal(_k(gl), _k(light)) and np.array_equal(_k(gd), _k(dark))
    eng.close()


def test_state_rules(amd):
    import ctypes as C
    from therldaisyworld_amd import _ffi
    lib = _ffi.load()
    B, H, W = 3, 64, 64
    from therldaisyworld_amd import default_params
    p = default_params(B, H, W, 2)
    eng, twin = amd.Engine(p), amd.Engine(p)
    for e in (eng, twin):
        e.init_random(5)
    L = _schedule(4, B)
    null = C.POINTER(_ffi.DwWorldStats)()
    assert lib.dw_step_n_trace_per_world(eng._h, 0, _ffi.ptr_d(L), null) == _ffi.DW_OK
    fresh = amd.Engine(p)
    assert lib.dw_step_n_trace_per_world(fresh._h, 4, _ffi.ptr_d(L), null) == _ffi.DW_ESTATE
    fresh.close()
    assert lib.dw_step_n_trace_per_world(eng._h, 4, None, null) == _ffi.DW_EINVAL
    # a luminosity that is no luminosity: refused before anything runs, the state untouched
    before = eng.download_planes()
    for bad in (np.nan, -0.5, np.inf):
        Lb = L.copy()
        Lb[2, 1] = bad
        assert lib.dw_step_n_trace_per_world(eng._h, 4, _ffi.ptr_d(Lb), null) == _ffi.DW_EINVAL
        assert b"luminosity" in lib.dw_last_error()
    for x, y in zip(before, eng.download_planes()):
        assert np.array_equal(x, y)
    eng.get_obs(0.9)                                        # not stepped yet: fine
    eng.step_n_trace_per_world(L)
    for call in (lambda: eng.get_obs(0.9), lambda: eng.download_grid(0.9)):
        with pytest.raises(amd.DaisyHipError) as err:
            call()
        assert err.value.code == _ffi.DW_ESTATE and "per-world" in str(err.value)
    eng.download_planes(), eng.reduce(), eng.download_caches(0.9)      # keep working
    eng.snapshot_save()
    # ONE shared-L step, and everything works again - and agrees with a twin that took the same calls ...
    twin.step_n_trace_per_world(L, trace=False)
    eng.step(1.0)
    twin.step(1.0)
    assert np.array_equal(eng.get_obs(0.9), twin.get_obs(0.9))
    assert np.array_equal(eng.download_grid(0.9), twin.download_grid(0.9))
    # ... and with one-world handles that took column b, then the shared step
    grid = eng.download_grid(0.9)
    for b in range(B):
        q = default_params(1, H, W, 2)
        q.world_offset = b
        one = amd.Engine(q)
        one.init_random(5)
        for t in range(4):
            one.step(float(L[t, b]))
        one.step(1.0)
        g1 = one.download_grid(0.9)
        assert np.array_equal(np.delete(grid[b], 4, axis=0), np.delete(g1[0], 4, axis=0)), b   # channel 4: agent states
        one.close()
    eng.snapshot_restore()                                  # back to the per-world state: the rule holds again
    with pytest.raises(amd.DaisyHipError):
        eng.download_grid(0.9)
    eng.close()
    twin.close()


@pytest.mark.parametrize("shape,form", [((2, 40, 512), "wave strips"), ((2, 130, 256), "wave strips"), ((2, 70, 320), "wave strips"),
                                        ((2, 37, 52), "generic"), ((2, 64, 64), "generic"), ((600, 64, 64), "generic")])
def test_kernel_info_names_the_per_world_form(amd, shape, form):
    eng = _engine(amd, *shape, "exact")
    assert f"; per-world L: {form}" in eng.kernel_info(), eng.kernel_info()
    eng.close()
    if form == "wave strips":                               # float64 arithmetic: always the generic kernel
        eng = _engine(amd, *shape, "f64")
        assert "; per-world L: generic" in eng.kernel_info()
        eng.close()


def test_luminosity_sweep_harness(amd):
    """64 worlds of 64 x 64 held at 64 luminosities for 200 steps: the end of every curve equals a one-world engine's
    own loop; the environment refuses to go on without a reset."""
    B, n = 64, 200
    Lv = np.linspace(0.6, 1.7, B)
    np.random.seed(42)
    env = amd.RLDaisyWorld(grid_dimension=64, n_agents=0)
    env.batch_size = B
    env.reset()
    grid0 = env.grid.copy()
    out = amd.simulate_luminosity_sweep(env, Lv, n, obs=True)
    assert out["L"].shape == (n, B) and out["stats"].shape == (n, B) and np.array_equal(out["L"][7], Lv)
    cells = 64.0 * 64.0
    for b in range(B):
        one = _engine(amd, 1, 64, 64, "exact")
        one.upload_state(grid0[b:b + 1, 1], grid0[b:b + 1, 2])
        for _ in range(n):
            one.step(float(Lv[b]))
        r = one.reduce()[0]
        assert out["mean_light"][-1, b] == r["sum_light_k"] / 1000.0 / cells, b
        assert out["mean_dark"][-1, b] == r["sum_dark_k"] / 1000.0 / cells, b
        assert out["alive"][-1, b] == (r["max_k"] / 1000.0 > 0.005), b
        one.close()
    assert out["alive"][-1].any() and not out["alive"][-1].all()       # the diagram has both branches
    with pytest.raises(RuntimeError, match=r"reset\(\)"):
        env.step()
    with pytest.raises(RuntimeError, match=r"reset\(\)"):
        env.grid
    env.reset()
    env.step()
    assert env.grid.shape == (B, 7, 64, 64)
    # a schedule per world: half the worlds ramp up, half ramp down
    up = np.linspace(0.7, 1.6, 30)
    sched = np.stack([up if b % 2 == 0 else up[::-1] for b in range(B)], axis=1)
    out2 = amd.simulate_luminosity_sweep(env, sched, 30)
    assert out2["L"].shape == (30, B) and np.array_equal(out2["L"], sched)
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
for e in (eng, ref):
    e.init_random(9, quantised=True)                     # straight into the binary16 planes: no group allocated
before = eng.download_planes()
try:
    eng.step_n_trace_per_world(L)                        # the table's group cannot be allocated
except amd.DaisyHipError as err:
    assert err.code == _ffi.DW_ENOMEM, err
else:
    raise SystemExit("the injected allocation failure was not reported")
assert all(np.array_equal(x, y) for x, y in zip(before, eng.download_planes()))
tr = eng.step_n_trace_per_world(L)                       # the hook is spent
want = ref.step_n_trace_per_world(L)
assert all(np.array_equal(tr[f], want[f]) for f in ("max_k", "sum_light_k", "sum_dark_k"))
assert all(np.array_equal(x, y) for x, y in zip(eng.download_planes(), ref.download_planes()))
one = amd.default_params(1, 40, 512, 0)
one.world_offset = 1
w1 = amd.Engine(one)
w1.init_random(9, quantised=True)
for t in range(5):
    w1.step(1.0)
assert np.array_equal(w1.download_planes()[0][0], eng.download_planes()[0][1])
print("ok")
"""


def test_failed_table_allocation_is_reported_and_retryable():
    env = dict(os.environ, DW_TEST_HOOKS="1", DW_TEST_FAIL_GROUP_ALLOC="1")
    p = subprocess.run([sys.executable, "-c", _ALLOC_SCRIPT, ROOT], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.returncode, p.stdout[-500:], p.stderr[-2000:])
