"""GPU tests (``-m gpu``) of the spatial frames: dw_reduce_tiles / Engine.reduce_tiles, dw_step_n_frames /
Engine.step_n_frames and harness.simulate_frames.

References are existing calls on a twin handle with the same `init_random` seed, stepped with `step(L)` one step at a time:
the per-mille planes `_k(download_planes())`, the temperatures `download_caches(L)[0][:, 0]`; the float64 NumPy oracle
supplies the field where stated.  Bounds, none of them measured:
  * cover: exact integers everywhere;
  * 1 x 1 tiles: the cache's doubles bit for bit;
  * a tile of n cells: |temp_mean - fsum(cells) / n| <= (n + 3) 2^-53 |mean| - any summation order of n positive doubles
    is within (n - 1) 2^-53 relative of the exact sum, the division and fsum's own rounding add one each, one to spare;
  * against the oracle's field rtol = 2e-12, the bound tests/test_gpu_temperature.py holds the world mean to (1e-12 per
    cell from tests/test_gpu_parity.py; the cells of a tile are all positive, so their exact mean is within that too, and the
    kernels' fixed order puts at most 16 + 6 + 3 + 4 roundings on any path of a sum here, 3e-15).
Shapes: tile widths no vector load divides (12, 4, 1, 36 on W = 36), the three mappings of the temperature kernel (one
thread, one wave, workgroups with and without partials per tile), a tile that is the whole world, more than 65 535 worlds.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import daisy_oracle as O  # noqa: E402

STAT_FIELDS = ("max_k", "sum_light_k", "sum_dark_k")
NRUN = 13
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _engine(amd, B, H, W, precision="exact", N=0):
    from therldaisyworld_amd import _ffi
    p = amd.default_params(B, H, W, N)
    p.precision = _ffi.PRECISION[precision]
    return amd.Engine(p)


def _k(x):
    return np.rint(np.asarray(x) * 1000.0).astype(np.int64)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _L(t):
    return 0.85 + 0.02 * t


def _tiles(a, th, tw):
    """(B, H, W) -> (B, TH, TW, th * tw): the cells of every tile, row-major within the tile"""
    B, H, W = a.shape
    return a.reshape(B, H // th, th, W // tw, tw).transpose(0, 1, 3, 2, 4).reshape(B, H // th, W // tw, th * tw)


def _assert_cover(cover, kl, kd, th, tw, what):
    assert cover.shape == (kl.shape[0], kl.shape[1] // th, kl.shape[2] // tw), what
    assert np.array_equal(cover["sum_light_k"], _tiles(kl, th, tw).sum(axis=3)), what
    assert np.array_equal(cover["sum_dark_k"], _tiles(kd, th, tw).sum(axis=3)), what


def _assert_temp_within_bound(temp, field, th, tw, what):
    """|temp_mean - fsum(cells) / n| <= (n + 3) 2^-53 |mean| for every tile"""
    cells = _tiles(field, th, tw)
    n = th * tw
    want = np.array([math.fsum(c) / n for c in cells.reshape(-1, n)]).reshape(cells.shape[:3])
    assert temp.shape == want.shape, what
    err = np.abs(temp - want)
    print(what, f"{th}x{tw}: max |err| / (eps |mean|) = {np.max(err / (EPS * np.abs(want))):.2f} (bound {n + 3})")
    assert (err <= (n + 3) * EPS * np.abs(want)).all(), (what, th, tw, np.max(err / (EPS * np.abs(want))))


def _oracle_field(light, dark, L):
    """env.temp of the NumPy oracle after ONE forward pass at L from the covers (B, H, W): (B, H, W)"""
    B, H, W = light.shape
    out = np.zeros((B, H, W))
    for b in range(B):
        o = O.OracleDaisyWorld(grid_dimension=W, n_agents=0, batch_size=1)
        o.L = float(L)
        o.set_initial_cover(light[b:b + 1].copy(), dark[b:b + 1].copy())
        o.grid = o.forward(o.grid)
        out[b] = o.temp[0, 0]
    return out


def _raises(code, fn, *args, **kw):
    from therldaisyworld_amd import _ffi
    with pytest.raises(_ffi.DaisyHipError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


# ---- 1. 1 x 1 tiles: the planes and the cache themselves ---------------------------------------------------------------
@pytest.mark.parametrize("precision", ["exact", "fast", "f64"])
@pytest.mark.parametrize("H,W", [(5, 12), (8, 8)])
@pytest.mark.parametrize("start", ["init_random", "upload_f64"])
def test_unit_tiles_are_the_planes_and_the_cache(amd, precision, H, W, start):
    from therldaisyworld_amd import _ffi
    B = 3
    eng = _engine(amd, B, H, W, precision)
    eng.init_random(11)
    if start == "upload_f64":                                   # the same covers as an un-quantised float64 upload
        eng.upload_state(*eng.download_planes())
    # un-quantised: no cover, but the temperatures of the upload in its own format (float32 per-mille / float64)
    before = eng.download_planes()
    msg = _raises(_ffi.DW_ESTATE, eng.reduce_tiles, _L(0))
    assert "not quantised yet; take the first step with dw_step" in msg
    _raises(_ffi.DW_ESTATE, eng.reduce_tiles, _L(0), temperature=False)
    cov, temp = eng.reduce_tiles(_L(0), cover=False)
    assert cov is None and _bits(temp) == _bits(eng.download_caches(_L(0))[0][:, 0])
    assert all(np.array_equal(a, b) for a, b in zip(before, eng.download_planes()))
    for t in range(3):                                          # previous state: the upload, then binary16 planes
        eng.step(_L(t))
        cov, temp = eng.reduce_tiles(1.234)                     # (after a step the luminosity is the step's own)
        kl, kd = map(_k, eng.download_planes())
        assert cov.shape == temp.shape == (B, H, W)
        assert np.array_equal(cov["sum_light_k"], kl) and np.array_equal(cov["sum_dark_k"], kd)
        assert _bits(temp) == _bits(eng.download_caches(_L(t))[0][:, 0]), (precision, t)
    eng.close()


# ---- 2. block tiles ----------------------------------------------------------------------------------------------------------
BLOCKS = [((3, 24, 36), [(8, 12), (3, 4), (24, 1), (1, 36)]),
          ((2, 16, 48), [(16, 16)]),
          ((3, 8, 8), [(8, 8)]),
          ((2, 64, 256), [(64, 256), (16, 16)])]


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("shape,tiles", BLOCKS, ids=[f"{s[1]}x{s[2]}" for s, _ in BLOCKS])
def test_block_tiles(amd, precision, shape, tiles):
    B, H, W = shape
    eng = _engine(amd, B, H, W, precision)
    eng.init_random(23)
    for t in range(2):                                          # the field of the un-quantised upload, then of binary16 planes
        eng.step(_L(t))
        kl, kd = map(_k, eng.download_planes())
        field = eng.download_caches(_L(t))[0][:, 0]
        oracle = _oracle_field(*eng.download_planes(1), _L(t))  # (1: DW_STATE_PREVIOUS, the state that step read)
        red = eng.reduce()
        for th, tw in tiles:
            what = f"{shape} {precision} step {t}"
            cov, temp = eng.reduce_tiles(_L(t), tile=(th, tw))
            _assert_cover(cov, kl, kd, th, tw, what)
            _assert_temp_within_bound(temp, field, th, tw, what)
            np.testing.assert_allclose(temp, _tiles(oracle, th, tw).mean(axis=3), rtol=2e-12, atol=0, err_msg=what)
            if (th, tw) == (H, W):                              # the tile is the world: dw_reduce's sums
                assert np.array_equal(cov["sum_light_k"][:, 0, 0], red["sum_light_k"])
                assert np.array_equal(cov["sum_dark_k"][:, 0, 0], red["sum_dark_k"])
    eng.close()


# ---- 3. independence of the batch, the selection and the call ---------------------------------------------------------
@pytest.mark.parametrize("H,W,tiles", [(24, 36, [(1, 1), (3, 4), (8, 12)]), (64, 256, [(64, 256), (32, 64), (16, 16)])])
def test_a_world_reduces_the_same_alone_and_in_any_selection(amd, H, W, tiles):
    big = _engine(amd, 5, H, W, "exact")
    big.init_random(31, quantised=True)
    light, dark = big.download_planes()
    one = _engine(amd, 1, H, W, "exact")
    one.upload_state_f32(light[3:4].astype(np.float32), dark[3:4].astype(np.float32), quantised=True)
    assert np.array_equal(_k(one.download_planes()[0]), _k(light[3:4]))
    for th, tw in tiles:
        alone = one.reduce_tiles(0.93, tile=(th, tw))
        sel3 = big.reduce_tiles(0.93, tile=(th, tw), worlds=[3])
        mixed = big.reduce_tiles(0.93, tile=(th, tw), worlds=[4, 0, 3])
        everyone = big.reduce_tiles(0.93, tile=(th, tw))
        again = big.reduce_tiles(0.93, tile=(th, tw), worlds=[4, 0, 3])
        for i in range(2):                                      # cover, temperature
            assert _bits(alone[i][0]) == _bits(sel3[i][0]) == _bits(mixed[i][2]) == _bits(everyone[i][3]), (th, tw, i)
            assert _bits(mixed[i][0]) == _bits(everyone[i][4]) and _bits(mixed[i][1]) == _bits(everyone[i][0])
            assert _bits(mixed[i]) == _bits(again[i])
        assert len({_bits(everyone[1][b]) for b in range(5)}) == 5      # (the worlds do differ)
    big.close()
    one.close()


# ---- 4. runs ------------------------------------------------------------------------------------------------------------------
RUNS = {(70, 320): (10, 16), (8, 8): (2, 4)}                    # shape -> tile (one wave per tile; one thread per tile)


def _start(eng, quantised):
    eng.init_random(47, quantised=quantised)


@functools.lru_cache(maxsize=None)
def _reference(H, W, precision, quantised):
    """The twin handles of a run of NRUN steps from init_random(47): one stepped with step(L) one step at a time - after
    step t its planes, the field that step computed (the cache) and reduce_tiles of it - and one through step_n_trace."""
    import therldaisyworld_amd as amd
    th, tw = RUNS[(H, W)]
    Ls = np.array([_L(t) for t in range(NRUN)])
    eng = _engine(amd, 3, H, W, precision)
    _start(eng, quantised)
    ref = dict(kl=[], kd=[], field=[], cover=[], temp=[])
    for t in range(NRUN):
        eng.step(Ls[t])
        kl, kd = map(_k, eng.download_planes())
        cov, temp = eng.reduce_tiles(Ls[t], tile=(th, tw))
        field = eng.download_caches(Ls[t])[0][:, 0]
        _assert_cover(cov, kl, kd, th, tw, f"twin step {t}")
        _assert_temp_within_bound(temp, field, th, tw, f"twin {(H, W)} {precision} step {t}")
        for key, v in zip(("kl", "kd", "field", "cover", "temp"), (kl, kd, field, cov, temp)):
            ref[key].append(v)
    eng.close()
    eng = _engine(amd, 3, H, W, precision)
    _start(eng, quantised)
    ref["trace"] = eng.step_n_trace(Ls)
    ref["final"] = _final(eng)
    ref["pairs"] = "trace: step pairs" in eng.kernel_info()
    eng.close()
    return ref


def _final(eng):
    red = eng.reduce()
    return (_bits(np.stack(eng.download_planes())), _bits(np.stack(eng.download_planes(1))),
            tuple(_bits(red[f]) for f in STAT_FIELDS), eng.last_fixup_count())


def _check_run(eng, ref, stride, H, W):
    th, tw = RUNS[(H, W)]
    Ls = np.array([_L(t) for t in range(NRUN)])
    cover, temp, trace = eng.step_n_frames(Ls, stride=stride, tile=(th, tw))
    F = NRUN // stride
    assert cover.shape == temp.shape == (F, 3, H // th, W // tw) and trace.shape == (NRUN, 3)
    for f in STAT_FIELDS:
        assert np.array_equal(trace[f], ref["trace"][f]), f
    assert _final(eng) == ref["final"]
    for f in range(F):
        t = (f + 1) * stride - 1
        _assert_cover(cover[f], ref["kl"][t], ref["kd"][t], th, tw, f"frame {f}")
        assert np.array_equal(cover[f]["sum_light_k"].sum(axis=(1, 2)), trace["sum_light_k"][t])
        assert np.array_equal(cover[f]["sum_dark_k"].sum(axis=(1, 2)), trace["sum_dark_k"][t])
        assert _bits(cover[f]) == _bits(ref["cover"][t])
        assert _bits(temp[f]) == _bits(ref["temp"][t]), (stride, f)     # (held to the cache's field in _reference)
    return cover


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("quantised", [True, False], ids=["quantised", "unquantised"])
@pytest.mark.parametrize("stride", [1, 3, 4, 5])
@pytest.mark.parametrize("H,W", list(RUNS))
def test_runs_with_frames(amd, H, W, stride, quantised, precision):
    ref = _reference(H, W, precision, quantised)
    assert ref["pairs"] == ((H, W) == (70, 320))                # the wide shape is one whose traces take step pairs
    eng = _engine(amd, 3, H, W, precision)
    _start(eng, quantised)
    cover = _check_run(eng, ref, stride, H, W)
    # cover alone: the same records, the same state
    _start(eng, quantised)
    Ls = np.array([_L(t) for t in range(NRUN)])
    cov2, none, trace = eng.step_n_frames(Ls, stride=stride, tile=RUNS[(H, W)], temperature=False, trace=False)
    assert none is None and trace is None and _bits(cov2) == _bits(cover) and _final(eng) == ref["final"]
    eng.close()


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("H,W,stride,ring", [(70, 320, 1, 2), (70, 320, 3, 3), (8, 8, 1, 5), (8, 8, 4, 1)])
def test_a_tiny_frame_ring_changes_nothing(amd, monkeypatch, H, W, stride, ring, precision):
    ref = _reference(H, W, precision, False)
    monkeypatch.setenv("DW_TEST_HOOKS", "1")
    monkeypatch.setenv("DW_TEST_FRAME_RING", str(ring))
    eng = _engine(amd, 3, H, W, precision)                      # (the library reads the switches here)
    assert f"DW_TEST_FRAME_RING={ring}" in eng.kernel_info()
    _start(eng, False)
    _check_run(eng, ref, stride, H, W)
    eng.close()


# ---- 5. more worlds than a grid holds in y -------------------------------------------------------------------------------
def test_more_than_65535_worlds(amd):
    from therldaisyworld_amd import _ffi
    B, sel = 70000, [0, 65534, 65535, 65536, 69999]
    try:
        eng = _engine(amd, B, 4, 4, "exact")
        eng.init_random(5)
        eng.step(0.9)
        cov, none = eng.reduce_tiles(0.9, temperature=False)
        c5, t5 = eng.reduce_tiles(0.9, worlds=sel)
        kl, kd = map(_k, eng.download_planes())
        field = eng.download_caches(0.9)[0][:, 0]
    except _ffi.DaisyHipError as e:
        if e.code == _ffi.DW_ENOMEM:
            pytest.skip("the device cannot hold 70 000 worlds of 4x4")
        raise
    assert none is None and cov.shape == (B, 4, 4)
    assert np.array_equal(cov["sum_light_k"], kl) and np.array_equal(cov["sum_dark_k"], kd)
    assert np.array_equal(c5["sum_light_k"], kl[sel]) and np.array_equal(c5["sum_dark_k"], kd[sel])
    assert _bits(t5) == _bits(field[sel])
    assert len({_bits(kl[b]) for b in sel}) == len(sel)         # (the probes differ)
    eng.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def _spec(th=1, tw=1, worlds=None, n=None):
    from therldaisyworld_amd import _ffi
    arr = None if worlds is None else np.asarray(worlds, dtype=np.int32)
    spec = _ffi.DwFrameSpec(th, tw, (0 if arr is None else arr.size) if n is None else n,
                            None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_int32)))
    return spec, arr


def test_refusals_leave_the_state_untouched(amd):
    from therldaisyworld_amd import _ffi
    B, H, W = 3, 8, 8
    eng = _engine(amd, B, H, W, "exact")
    lib, h = eng._lib, eng._h
    cov = np.zeros((4, B, H, W), dtype=_ffi.TILE_COVER_DTYPE)
    tmp = np.zeros((4, B, H, W))
    pc, pt = cov.ctypes.data_as(C.POINTER(_ffi.DwTileCover)), _ffi.ptr_d(tmp)
    Ls = np.full(4, 0.9)
    ok = _spec()

    def tiles(spec, L=0.9, c=pc, t=pt):
        return lib.dw_reduce_tiles(h, L, None if spec is None else C.byref(spec[0]), c, t)

    def frames(spec, n=4, L=Ls, stride=1, c=pc, t=pt):
        return lib.dw_step_n_frames(h, n, _ffi.ptr_d(L) if L is not None else None, None if spec is None else C.byref(spec[0]),
                                    stride, c, t, None)

    # no state
    assert tiles(ok) == _ffi.DW_ESTATE and frames(ok) == _ffi.DW_ESTATE
    eng.init_random(3)
    eng.step(0.9)
    state = (_bits(np.stack(eng.download_planes())), _bits(eng.reduce()))
    bad_L = [np.array([0.9, np.nan, 0.9, 0.9]), np.array([0.9, 0.9, -0.1, 0.9]), np.array([0.9, 0.9, 0.9, np.inf])]
    invalid = [lambda: tiles(None), lambda: tiles(ok, c=None, t=None), lambda: tiles(_spec(3, 3)), lambda: tiles(_spec(8, 5)),
               lambda: tiles(_spec(0, 1)), lambda: tiles(_spec(n=-1)), lambda: tiles(_spec(n=2)), lambda: tiles(_spec(worlds=[0, 3])),
               lambda: tiles(_spec(worlds=[-1])), lambda: tiles(_spec(worlds=[1, 2, 1])), lambda: tiles(ok, L=float("nan")),
               lambda: tiles(ok, L=-1.0), lambda: tiles(ok, L=float("inf")),
               lambda: frames(None), lambda: frames(ok, L=None), lambda: frames(ok, c=None, t=None), lambda: frames(ok, stride=0),
               lambda: frames(ok, stride=-2), lambda: frames(ok, n=-1), lambda: frames(_spec(3, 3)), lambda: frames(_spec(n=-1)),
               lambda: frames(_spec(n=2)), lambda: frames(_spec(worlds=[3])), lambda: frames(_spec(worlds=[2, 2])),
               *[(lambda L=L: frames(ok, L=L)) for L in bad_L]]
    for i, call in enumerate(invalid):
        assert call() == _ffi.DW_EINVAL, (i, lib.dw_last_error())
        assert (_bits(np.stack(eng.download_planes())), _bits(eng.reduce())) == state, i
    # nsteps == 0 is a no-op (a stride beyond the run: no frame either)
    assert frames(ok, n=0) == _ffi.DW_OK and frames(ok, n=0, stride=7) == _ffi.DW_OK
    assert (_bits(np.stack(eng.download_planes())), _bits(eng.reduce())) == state
    # per-world constants: no single set to evaluate the retained state with - the cover is still there
    worlds = np.repeat(eng.world_params(), B)
    eng.step_n_trace_ensemble(worlds, np.full((2, B), 0.9))
    state = (_bits(np.stack(eng.download_planes())), _bits(eng.reduce()))
    assert "dw_step_n_trace_ensemble" in _raises(_ffi.DW_ESTATE, eng.reduce_tiles, 0.9)
    cov1, none = eng.reduce_tiles(0.9, temperature=False)
    assert np.array_equal(cov1["sum_light_k"], _k(eng.download_planes()[0]))
    assert (_bits(np.stack(eng.download_planes())), _bits(eng.reduce())) == state
    eng.close()


def test_a_tile_of_more_than_2_pow_20_cells_is_refused(amd):
    from therldaisyworld_amd import _ffi
    eng = _engine(amd, 1, 2048, 1024, "fast")
    eng.init_random(1, quantised=True)
    assert "1 048 576" in _raises(_ffi.DW_EINVAL, eng.reduce_tiles, 0.9, tile=(2048, 1024), temperature=False)
    cov, _ = eng.reduce_tiles(0.9, tile=(1024, 1024), temperature=False)     # 2^20 cells: the largest tile
    assert np.array_equal(cov["sum_light_k"][0, :, 0], _k(eng.download_planes()[0])[0].reshape(2, -1).sum(axis=1))
    eng.close()


# ---- 7. the drop-in class -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["exact", "fast"])
def test_simulate_frames_against_env_step(amd, precision):
    n, stride = 20, 2

    def make():
        np.random.seed(77)
        env = amd.RLDaisyWorld(grid_dimension=8, n_agents=0, precision=precision)
        env.batch_size = 3
        env.reset()
        return env

    env, twin = make(), make()
    out = amd.simulate_frames(env, n, stride=stride, tile=1, obs=True)
    assert out["light"].shape == out["dark"].shape == out["temp"].shape == (n // stride, 3, 8, 8)
    f = 0
    for t in range(n):
        twin.step()
        if (t + 1) % stride:
            continue
        assert out["frame_steps"][f] == twin.step_count
        assert np.array_equal(out["light"][f], twin.grid[:, 1]) and np.array_equal(out["dark"][f], twin.grid[:, 2]), f
        assert _bits(out["temp"][f]) == _bits(twin.temp[:, 0]), f
        f += 1
    assert f == n // stride
    assert np.array_equal(env.grid, twin.grid) and env.L == twin.L and env.step_count == twin.step_count
    env.close()
    twin.close()
