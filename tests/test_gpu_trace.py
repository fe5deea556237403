"""GPU tests (``-m gpu``) of dw_step_n_trace / Engine.step_n_trace / harness.simulate_ramp: the per-step, per-world
reductions of a whole run of steps, recorded on the device.  Every comparison is on max_k, sum_light_k, sum_dark_k and
every one is EXACT equality - the quantities are integers.  The tests are black-box: they hold whether a shape records
step pairs (trace_pair_fast / trace_pair_exact) or single steps, except the last one, which pins the two layouts that
must take the pair kernels.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import c_oracle  # noqa: E402

FIELDS = ("max_k", "sum_light_k", "sum_dark_k")
SHAPES = [(3, 130, 256), (2, 70, 320), (2, 96, 512), (1, 130, 4096), (2, 80, 1024), (64, 16, 16), (1, 64, 64), (3, 37, 52)]
NSTEPS = (0, 1, 2, 3, 4, 41)


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


def _ramp(n=41, L0=0.8, L1=1.55):
    """Growth (L ~ 0.8 - 0.95), the populated plateau (~1.0 - 1.2), decline and death of every world (L > ~1.45: the last
    rows of the series are all zero)."""
    return L0 + (L1 - L0) * np.arange(n) / 40.0


def _blocky_state(B, H, W, seed):
    """An un-quantised float64 state made of uniform blocks - whole regions of EQUAL covers, one of them exactly 1.000
    (the equal-maxima case of the maximum's re-scan rule) - beside a noisy region."""
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
        light[-1] = 0.25                                     # a whole world of equal covers
        dark[-1] = 0.25
    return light, dark


def _init(eng, how, seed):
    if how == "philox":
        eng.init_random(seed)                               # un-quantised: the first step is the first-step kernel
    elif how == "philox_q":
        eng.init_random(seed, quantised=True)
    else:
        eng.upload_state(*_blocky_state(eng.B, eng.H, eng.W, seed))


def _stepwise(eng, Ls):
    """The only way to the series without dw_step_n_trace: dw_step + dw_reduce per step."""
    rows = []
    for L in Ls:
        eng.step(float(L))
        rows.append(eng.reduce())
    return np.stack(rows) if rows else np.zeros((0, eng.B), dtype=eng.reduce().dtype)


def _assert_rows_equal(a, b, what=""):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), (what, f, np.argwhere(a[f] != b[f])[:5].tolist())


def _assert_same_state(x, y, stepped, what=""):
    from therldaisyworld_amd import _ffi
    for a, b in zip(x.download_planes(), y.download_planes()):
        assert np.array_equal(a, b), (what, "current planes")
    if stepped:
        for a, b in zip(x.download_planes(_ffi.STATE_PREVIOUS), y.download_planes(_ffi.STATE_PREVIOUS)):
            assert np.array_equal(a, b), (what, "previous planes")
    _assert_rows_equal(x.reduce()[None], y.reduce()[None], what + " final reduce")


def _compare_with_stepwise(amd, B, H, W, precision, how, nsteps_list=NSTEPS, seed=11, Ls=None, warm=0):
    Ls = _ramp() if Ls is None else Ls
    for n in nsteps_list:
        a, b = _engine(amd, B, H, W, precision), _engine(amd, B, H, W, precision)
        for e in (a, b):
            _init(e, how, seed)
            if warm:
                e.step_n(warm, 0.8, 0.002, 0.75, 1.5)
        tr = a.step_n_trace(Ls[:n])
        ref = _stepwise(b, Ls[:n])
        what = f"{(B, H, W)} {precision} {how} n={n}"
        assert tr.shape == (n, B)
        _assert_rows_equal(tr, ref, what)
        _assert_same_state(a, b, n > 0 or warm > 0, what)
        if n == 41 and not warm and how != "upload":
            assert (tr["max_k"][-1] == 0).all() and (tr["max_k"] > 500).any(), "the ramp is meant to end in death"
        a.close()
        b.close()


@pytest.mark.parametrize("how", ["philox", "philox_q", "upload"])
@pytest.mark.parametrize("precision", ["fast", "exact"])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_trace_equals_the_step_by_step_loop(amd, B, H, W, precision, how):
    """Two engines from the same state; one calls step_n_trace, the other step + reduce per step: series rows, final
    planes, retained previous planes and the final reduce() are equal, for 0, 1, 2, 3, 4 and 41 steps of a ramp through
    growth, plateau and death."""
    _compare_with_stepwise(amd, B, H, W, precision, how)


@pytest.mark.parametrize("B,H,W", [(64, 16, 16), (3, 37, 52)])
def test_trace_equals_the_step_by_step_loop_f64(amd, B, H, W):
    _compare_with_stepwise(amd, B, H, W, "f64", "upload")


_ASYM = dict(albedo_light=0.8)                             # a_dark - a_bare != -(a_light - a_bare): the non-SYM kernels


@pytest.mark.parametrize("consts", [{}, _ASYM], ids=["default", "asymmetric"])
@pytest.mark.parametrize("B,H,W", [(2, 130, 256), (1, 70, 320), (1, 130, 4096)])
def test_trace_equals_the_oracle(amd, B, H, W, consts):
    """Exact mode against the float64 C oracle stepped one step at a time: sums and maximum of rint(1000 x) in int64."""
    eng = _engine(amd, B, H, W, "exact", **consts)
    eng.init_random(23)
    light, dark = eng.download_planes()
    P = c_oracle.OracleParams.defaults(**consts)
    Ls = _ramp()
    tr = eng.step_n_trace(Ls)
    for t, L in enumerate(Ls):
        c_oracle.step_n(light, dark, float(L), 0.0, 1, min_L=0.0, max_L=10.0, params=P)
        kl, kd = _k(light), _k(dark)
        assert np.array_equal(tr["max_k"][t], np.maximum(kl.max(axis=(1, 2)), kd.max(axis=(1, 2)))), t
        assert np.array_equal(tr["sum_light_k"][t], kl.sum(axis=(1, 2))), t
        assert np.array_equal(tr["sum_dark_k"][t], kd.sum(axis=(1, 2))), t
    gl, gd = eng.download_planes()
    assert np.array_equal(_k(gl), _k(light)) and np.array_equal(_k(gd), _k(dark))
    eng.close()


_DEV_LS = 1.2 + 0.00625 * np.arange(41)                     # continues the warm-up's ramp (0.8 + 200 x 0.002) to death


def _developed_run(amd, B, H, W):
    """step_n_trace against the step-by-step loop from a developed state (200 warm-up steps of the ramp: near-ties
    exist); returns the fix-up count of the run's last step."""
    a, b = _engine(amd, B, H, W, "exact"), _engine(amd, B, H, W, "exact")
    for e in (a, b):
        e.init_random(7)
        e.step_n(200, 0.8, 0.002, 0.75, 1.5)
    tr = a.step_n_trace(_DEV_LS[:16])                       # stops while the worlds are populated: the last step has near-ties
    ref = _stepwise(b, _DEV_LS[:16])
    _assert_rows_equal(tr, ref, "developed, first part")
    count = a.last_fixup_count()
    assert count == b.last_fixup_count()
    tr2 = a.step_n_trace(_DEV_LS[16:])
    ref2 = _stepwise(b, _DEV_LS[16:])
    _assert_rows_equal(tr2, ref2, "developed, to death")
    _assert_same_state(a, b, True, "developed")
    info = a.kernel_info()
    a.close()
    b.close()
    return tr, count, info


@pytest.mark.parametrize("B,H,W", [(2, 130, 256), (1, 70, 320)])
def test_every_repair_path_reaches_the_series(amd, monkeypatch, B, H, W):
    """From a developed state, with the repair machinery squeezed (switches are read when a handle is created):
      (a) DW_TEST_QUEUE_CAP=40: the pair kernels sweep their queue INSIDE the row loop when it is half full, so those
          sweeps feed the sums and maxima too; the fix-up count of the run's last step (a single step, whose kernel
          sweeps the same way) equal to the run without the hook shows that no strip fell back;
      (b) DW_TEST_MISMATCH_CAP=0: every strip with a float32 step-1 mismatch is recomputed whole in float64 and sums both
          steps from scratch (the pair kernels keep no fix-up count, so this run shows no more than the equal series);
          then with DW_TEST_QUEUE_CAP=0 as well EVERY strip that queues a near-tie cell falls back, in the pair kernels
          and in the single steps - a strip that fell back does not count its cells, so the fix-up count of the run's
          last step below run (a)'s shows it happened;
      (c) DW_TEST_FORCE_RESCAN: every strip re-reads its step-2 maximum from the finished planes.
    The series must be the same in all of them (each run is also compared with its own step-by-step loop)."""
    base, count0, _ = _developed_run(amd, B, H, W)
    assert count0 > 0, "the developed state is meant to have near-ties"
    monkeypatch.setenv("DW_TEST_QUEUE_CAP", "40")
    tr_a, count_a, info = _developed_run(amd, B, H, W)
    assert "DW_TEST_QUEUE_CAP=40" in info
    _assert_rows_equal(tr_a, base, "(a)")
    assert count_a == count0
    monkeypatch.delenv("DW_TEST_QUEUE_CAP")
    monkeypatch.setenv("DW_TEST_MISMATCH_CAP", "0")
    tr_b0, _, _ = _developed_run(amd, B, H, W)
    _assert_rows_equal(tr_b0, base, "(b) mismatch list only")
    monkeypatch.setenv("DW_TEST_QUEUE_CAP", "0")
    tr_b, count_b, _ = _developed_run(amd, B, H, W)
    _assert_rows_equal(tr_b, base, "(b)")
    assert count_b < count_a
    monkeypatch.delenv("DW_TEST_QUEUE_CAP")
    monkeypatch.delenv("DW_TEST_MISMATCH_CAP")
    monkeypatch.setenv("DW_TEST_FORCE_RESCAN", "1")
    tr_c, _, info = _developed_run(amd, B, H, W)
    assert "DW_TEST_FORCE_RESCAN" in info
    _assert_rows_equal(tr_c, base, "(c)")


def test_the_references_own_curve_g2(amd, golden):
    """G2's initial state, 500 steps on G2's L_used, exact mode: sum_k / 1000 / 4096 against the reference's recorded
    mean_light / mean_dark with rtol = 1e-13, atol = 0.  The fixture is NumPy's pairwise float64 mean of 4096 values
    k / 1000: its rounding error is below 13 x 2^-53 ~ 1.5e-15 relative; 1e-13 leaves two orders of margin and is six
    orders below what one per-mille quantum in one cell does to a mean of 0.3 (8e-7).  alive[t] is false wherever both
    of G2's means are 0 and true wherever either exceeds 0.005 (a mean above the threshold implies a cell above it)."""
    g = golden("G2_c1_trajectory")
    eng = _engine(amd, 1, 64, 64, "exact")
    eng.upload_state(g["light0"], g["dark0"])
    tr = eng.step_n_trace(g["L_used"])
    assert tr.shape == (500, 1)
    ml, md = tr["sum_light_k"][:, 0] / 1000.0 / 4096.0, tr["sum_dark_k"][:, 0] / 1000.0 / 4096.0
    np.testing.assert_allclose(ml, g["mean_light"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(md, g["mean_dark"], rtol=1e-13, atol=0)
    alive = tr["max_k"][:, 0] / 1000.0 > 0.005
    dead = (g["mean_light"] == 0) & (g["mean_dark"] == 0)
    sure = (g["mean_light"] > 0.005) | (g["mean_dark"] > 0.005)
    assert not alive[dead].any() and alive[sure].all()
    gl, gd = eng.download_planes()
    assert np.array_equal(_k(gl).astype(np.uint16), g["light_k_500"]) and np.array_equal(_k(gd).astype(np.uint16), g["dark_k_500"])
    eng.close()


def test_simulate_ramp_on_the_dropin_g2(amd, golden):
    """The same through harness.simulate_ramp on the drop-in (seed 42, G2's protocol): the first 100 steps' curves,
    env.grid equal to G2's snapshot at the stopping step, and 300 further steps reach snapshot 400."""
    from therldaisyworld_amd.harness import simulate_ramp
    g = golden("G2_c1_trajectory")
    np.random.seed(42)
    env = amd.RLDaisyWorld(grid_dimension=64, n_agents=0)
    env.batch_size = 1
    out = simulate_ramp(env, 100)
    assert out["stats"].shape == (100, 1) and out["L"].shape == (100,)
    assert np.array_equal(out["L"], g["L_used"][:100])
    np.testing.assert_allclose(out["mean_light"][:, 0], g["mean_light"][:100], rtol=1e-13, atol=0)
    np.testing.assert_allclose(out["mean_dark"][:, 0], g["mean_dark"][:100], rtol=1e-13, atol=0)
    assert out["alive"].dtype == bool and out["alive"].shape == (100, 1)
    assert np.array_equal(out["alive"], out["max_cover"] > 0.005)
    assert env.step_count == 100 and env.L == g["L_used"][100]
    assert np.array_equal(_k(env.grid[:, 1]).astype(np.uint16), g["light_k_100"])
    assert np.array_equal(_k(env.grid[:, 2]).astype(np.uint16), g["dark_k_100"])
    assert np.array_equal(env.grid[:, 3:6], g["temp3_100"])
    out2 = simulate_ramp(env, 200, obs=env.get_obs())        # continues (no reset)
    np.testing.assert_allclose(out2["mean_light"][:, 0], g["mean_light"][100:300], rtol=1e-13, atol=0)
    for t in range(300, 400):                                # ... and so does env.step()
        assert env.L == g["L_used"][t]
        env.step()
    assert np.array_equal(_k(env.grid[:, 1]).astype(np.uint16), g["light_k_400"])
    assert np.array_equal(_k(env.grid[:, 2]).astype(np.uint16), g["dark_k_400"])
    env.close()


@pytest.mark.parametrize("precision", ["fast", "exact"])
@pytest.mark.parametrize("B,H,W", [(3, 130, 256), (1, 130, 4096)])
def test_required_layouts_record_step_pairs(amd, B, H, W, precision):
    """Rotating strips (W = 256) and overlapped strips (W = 4096) really take the trace pair kernels."""
    eng = _engine(amd, B, H, W, precision)
    assert "trace: step pairs" in eng.kernel_info()
    eng.close()


def test_trace_argument_checks_and_long_runs(amd):
    """nsteps * B of 512 x 1024 in one call (one download), and the usual errors."""
    import ctypes as C
    from therldaisyworld_amd import _ffi
    lib = _ffi.load()
    eng = _engine(amd, 1024, 8, 8, "fast")
    Ls = np.full(512, 1.0)
    out = np.zeros((512, 1024), dtype=_ffi.STATS_DTYPE)
    ptr = out.ctypes.data_as(C.POINTER(_ffi.DwWorldStats))
    assert lib.dw_step_n_trace(eng._h, 0, _ffi.ptr_d(Ls), ptr) == _ffi.DW_OK           # a no-op, even without a state
    assert lib.dw_step_n_trace(eng._h, 4, _ffi.ptr_d(Ls), ptr) == _ffi.DW_ESTATE
    eng.init_random(3, quantised=True)
    assert lib.dw_step_n_trace(eng._h, -1, _ffi.ptr_d(Ls), ptr) == _ffi.DW_EINVAL
    assert lib.dw_step_n_trace(eng._h, 4, None, ptr) == _ffi.DW_EINVAL
    assert lib.dw_step_n_trace(eng._h, 4, _ffi.ptr_d(Ls), None) == _ffi.DW_EINVAL
    assert b"null" in lib.dw_last_error()
    other = _engine(amd, 1024, 8, 8, "fast")
    other.init_random(3, quantised=True)
    tr = eng.step_n_trace(Ls)
    assert tr.shape == (512, 1024)
    for t in range(512):
        other.step(1.0)
        if t in (0, 1, 255, 510, 511):
            _assert_rows_equal(tr[t][None], other.reduce()[None], f"row {t}")
    eng.close()
    other.close()
