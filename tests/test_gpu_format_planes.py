"""GPU tests (``-m gpu``) of the format-buffer-access step pairs (step_stream_fused2_fmt_pw, StepPlan::fmt_planes).

The format form moves the binary16 <-> float32 conversion of a row and its address arithmetic from the vector unit into
the memory path; every value it loads or stores is the value the plain kernel loads or stores.  So the check is bit
identity of ``dw_step_n`` between a default handle and a ``DW_NO_FMT_PLANES=1`` handle started from the same state:
planes, per-world reductions and (exact mode) the fix-up count.  There is no tolerance in this file.

Only the float32 (``fast``) kernel has a format form (the exact kernels do not fit it: DESIGN.md section 7), so in exact
mode both handles run the same kernels; those cases stay as the guard that the switch changes nothing there, and tie the
shapes to the float64 oracle.

Shapes: the smallest at which each thing can go wrong -
  3 x 3 x 260     two strips, the second with 12 output columns; column wrap on both sides; every halo row wraps (H < 3);
                  a nonzero world base
  2 x 70 x 320    a second, partial row block
  1 x 130 x 4096  the headline's 17-strip geometry
  2 x 66 x 8192
  34 x 8192^2     above toy size: a world base beyond 2^32 bytes (skipped when the device cannot hold 18 GiB)
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import c_oracle  # noqa: E402

FIELDS = ("max_k", "sum_light_k", "sum_dark_k")
SHAPES = ((3, 3, 260), (2, 70, 320), (1, 130, 4096), (2, 66, 8192))
L0, DL = 0.9, 0.75 / 512
_SWITCHES = ("DW_NO_FMT_PLANES", "DW_STRIP_ROWS", "DW_NO_FUSE", "DW_NO_RING", "DW_KERNEL")
_states = {}


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _engine(amd, monkeypatch, B, H, W, precision, fmt):
    from therldaisyworld_amd import _ffi
    for name in _SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if not fmt:
        monkeypatch.setenv("DW_NO_FMT_PLANES", "1")
    p = amd.default_params(B, H, W, 0)
    p.precision = _ffi.PRECISION[precision]
    eng = amd.Engine(p)                                      # (the library reads the switches here)
    info = eng.kernel_info()
    assert "fuses step pairs" in info, info
    # which kernel takes the pairs: the format form only in a default handle, and only in fast mode
    assert ("format buffer accesses" in info) == (fmt and precision == "fast"), info
    assert ("DW_NO_FMT_PLANES" in info) == (not fmt), info
    return eng


def _state(B, H, W):
    """a quantised state in natural units (k / 1000 with integer k; light + dark <= 1), computed once per shape and never
    changed"""
    if (B, H, W) not in _states:
        rng = np.random.RandomState(B * 1000003 + H * 1009 + W)
        kl = rng.randint(0, 600, size=(B, H, W))
        kd = np.minimum(rng.randint(0, 600, size=(B, H, W)), 1000 - kl)
        light, dark = (kl / 1000.0).astype(np.float32), (kd / 1000.0).astype(np.float32)
        light.setflags(write=False)
        dark.setflags(write=False)
        _states[(B, H, W)] = (light, dark)
    return _states[(B, H, W)]


def _run(amd, monkeypatch, shape, precision, fmt, steps):
    eng = _engine(amd, monkeypatch, *shape, precision, fmt)
    try:
        eng.upload_state_f32(*_state(*shape), quantised=True)
        L = eng.step_n(steps, L0, DL, 0.75, 1.5)
        light, dark = eng.download_planes()
        return L, light, dark, eng.reduce(), eng.last_fixup_count()
    finally:
        eng.close()


@pytest.mark.parametrize("steps", (5, 6))
@pytest.mark.parametrize("precision", ("fast", "exact"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_step_n_bit_identical_with_and_without_format_planes(amd, monkeypatch, shape, precision, steps):
    a = _run(amd, monkeypatch, shape, precision, True, steps)
    b = _run(amd, monkeypatch, shape, precision, False, steps)
    assert a[0] == b[0]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    for f in FIELDS:
        assert np.array_equal(a[3][f], b[3][f]), f
    if precision == "exact":
        assert a[4] == b[4]
    # not a dead state: the comparison means something
    assert a[3]["max_k"].max() > 0


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_exact_mode_against_the_oracle(amd, monkeypatch, shape):
    L, light, dark, red, _ = _run(amd, monkeypatch, shape, "exact", True, 6)
    l0, d0 = _state(*shape)
    ol = np.rint(l0.astype(np.float64) * 1000.0) / 1000.0    # the per-mille integers the upload rounds to
    od = np.rint(d0.astype(np.float64) * 1000.0) / 1000.0
    Lo = c_oracle.step_n(ol, od, L0, DL, 6)
    k = lambda x: np.rint(np.asarray(x) * 1000.0).astype(np.int64)
    assert L == Lo
    assert np.array_equal(k(light), k(ol)) and np.array_equal(k(dark), k(od))
    assert np.array_equal(red["sum_light_k"], k(ol).sum(axis=(1, 2)))
    assert np.array_equal(red["sum_dark_k"], k(od).sum(axis=(1, 2)))
    assert np.array_equal(red["max_k"], np.maximum(k(ol), k(od)).max(axis=(1, 2)))


def test_world_base_beyond_32_bits(amd, monkeypatch):
    """34 worlds of 8192^2: a plane is 4.25 GiB, so the bases of worlds 32 and 33 do not fit 32 bits.  Per-world reductions
    of all worlds and 8 sampled rows of worlds 0, 16 and 33, fast mode, 4 steps, one handle after the other.

    This compares two builds of the step pairs with each other, at thresholds that fall on world boundaries.  The test of
    the addressing itself - every kernel family past 2^32 cells with the thresholds inside a world, against small handles
    holding the same global worlds and against the C oracle - is tests/test_gpu_large_offsets.py."""
    from therldaisyworld_amd import _ffi
    B, H, W = 34, 8192, 8192
    hip = ctypes.CDLL("libamdhip64.so")
    rows = (0, 1, 63, 64, 4095, 4096, 8190, 8191)

    def run(fmt):
        try:
            eng = _engine(amd, monkeypatch, B, H, W, "fast", fmt)
        except _ffi.DaisyHipError as e:
            if e.code == _ffi.DW_ENOMEM:
                pytest.skip("the device cannot hold 34 worlds of 8192^2")
            raise
        try:
            try:
                eng.init_random(11, quantised=True)
            except _ffi.DaisyHipError as e:
                if e.code == _ffi.DW_ENOMEM:
                    pytest.skip("the device cannot hold 34 worlds of 8192^2")
                raise
            eng.step_n(4, L0, DL, 0.75, 1.5)
            red = eng.reduce()
            eng.sync()
            out = np.empty((2, 3, len(rows), W), dtype=np.float16)
            for pi, ptr in enumerate(eng.device_planes()):
                for wi, w in enumerate((0, 16, 33)):
                    for ri, r in enumerate(rows):
                        src = ptr + 2 * ((w * H + r) * W)
                        rc = hip.hipMemcpy(ctypes.c_void_p(out[pi, wi, ri].ctypes.data), ctypes.c_void_p(src),
                                           ctypes.c_size_t(2 * W), 2)    # hipMemcpyDeviceToHost
                        assert rc == 0, rc
            return red, out
        finally:
            eng.close()

    ra, pa = run(True)
    rb, pb = run(False)
    for f in FIELDS:
        assert np.array_equal(ra[f], rb[f]), f
    assert np.array_equal(pa.view(np.uint16), pb.view(np.uint16))
    assert ra["max_k"].min() > 0                              # every world alive: none compared as zeros
