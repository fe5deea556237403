"""GPU tests (``-m gpu``) of the seam-strip layout of the float32 step pairs (step_stream_fused2_seam_pw and
step_stream_fused2_left_pw, StepPlan::seam_strips).

The layout changes which wave and lane evaluates a cell, never the cell's arithmetic, so the check is bit identity of
float32 (``fast``) ``dw_step_n`` over 5 and 6 steps - two pairs and one or two closing single steps - from a quantised,
developed state, against two references: the same number of ``dw_step`` calls (the single-step kernels), and the same
``dw_step_n`` under ``DW_NO_SEAM_STRIPS=1`` (the overlapped 248-column strips).  Planes and per-world reductions; there is
no tolerance in this file.  Every case first asserts from ``kernel_info()`` that the seam form was really planned.

Shapes (strip height by DW_STRIP_ROWS, so that small heights make several row bands):
  2 x 40 x 316   rows 8   1 seam strip + 64 leftover columns (18 lanes, 3 bands per wave): 5 bands make one full and one
                          partly filled leftover wave; a nonzero world base
  3 x 44 x 520   rows 8   2 seam strips + 16 leftover columns, 10 bands per wave; last band of 4 rows; asymmetric albedos too
  2 x 24 x 504   rows 8   no leftover columns: the last seam lane's right half wraps to column 0
  1 x 24 x 4096  rows 8   the headline's column geometry; the leftover's right halo lane wraps to column 0
  2 x 16 x 760   rows 8   3 seam strips + 4 leftover columns (3 lanes per band)
  2 x 136 x 316  rows 64  the production strip height: bands of 64, 64 and 8 rows in ONE leftover wave - the top wrap and
                          the bottom wrap in different groups of it, and a group shorter than the wave's march
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("max_k", "sum_light_k", "sum_dark_k")
ASYM = dict(albedo_light=0.8)                                # a_dark - a_bare != -(a_light - a_bare), as tests/test_gpu_trace.py
CASES = (((2, 40, 316), 8, {}), ((3, 44, 520), 8, {}), ((3, 44, 520), 8, ASYM), ((2, 24, 504), 8, {}),
         ((1, 24, 4096), 8, {}), ((2, 16, 760), 8, {}), ((2, 136, 316), 64, {}))
L0, DL, MIN_L, MAX_L = 0.95, 0.75 / 512, 0.75, 1.5
_SWITCHES = ("DW_NO_SEAM_STRIPS", "DW_NO_FMT_PLANES", "DW_STRIP_ROWS", "DW_NO_FUSE", "DW_NO_RING", "DW_KERNEL")
_states = {}


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _engine(amd, monkeypatch, shape, rows, consts, seam):
    from therldaisyworld_amd import _ffi
    for name in _SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("DW_STRIP_ROWS", str(rows))
    if not seam:
        monkeypatch.setenv("DW_NO_SEAM_STRIPS", "1")
    p = amd.default_params(*shape, 0)
    p.precision = _ffi.PRECISION["fast"]
    for k, v in consts.items():
        setattr(p, k, v)
    eng = amd.Engine(p)                                      # (the library reads the switches here)
    info = eng.kernel_info()
    assert f"wave-strip={min(rows, shape[1])}x256" in info, info
    assert "format buffer accesses" in info, info
    assert ("step_stream_fused2_seam_pw" in info) == seam and ("step_stream_fused2_fmt_pw" in info) == (not seam), info
    assert ("DW_NO_SEAM_STRIPS" in info) == (not seam), info
    return eng


def _state(amd, monkeypatch, shape, rows, consts):
    """A developed quantised state in natural units (k / 1000, integer k): 40 steps up the ramp from a random one, taken by
    the overlapped-strip kernels; computed once per case and never changed."""
    key = (shape, tuple(sorted(consts.items())))
    if key not in _states:
        eng = _engine(amd, monkeypatch, shape, rows, consts, False)
        try:
            eng.init_random(shape[0] * 1000003 + shape[1] * 1009 + shape[2], quantised=True)
            eng.step_n(40, 0.8, 0.00375, MIN_L, MAX_L)
            light, dark = (x.astype(np.float32) for x in eng.download_planes())
        finally:
            eng.close()
        k = np.rint(light.astype(np.float64) * 1000.0)
        assert 0 < k.max() <= 1000 and len(np.unique(k)) > 50   # alive and structured: the comparison means something
        light.setflags(write=False)
        dark.setflags(write=False)
        _states[key] = (light, dark)
    return _states[key]


def _run(amd, monkeypatch, case, steps, how):
    shape, rows, consts = case
    state = _state(amd, monkeypatch, *case)
    eng = _engine(amd, monkeypatch, shape, rows, consts, how != "overlapped")
    try:
        eng.upload_state_f32(*state, quantised=True)
        if how == "single":
            L = L0
            for _ in range(steps):
                eng.step(L)
                L = min(max(L + DL, MIN_L), MAX_L)
        else:
            L = eng.step_n(steps, L0, DL, MIN_L, MAX_L)
        light, dark = eng.download_planes()
        return L, light, dark, eng.reduce()
    finally:
        eng.close()


def _id(case):
    shape, rows, consts = case
    return "x".join(map(str, shape)) + f"-rows{rows}" + ("-asym" if consts else "")


@pytest.mark.parametrize("steps", (5, 6))
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_step_n_bit_identical_to_single_steps_and_to_overlapped_strips(amd, monkeypatch, case, steps):
    a = _run(amd, monkeypatch, case, steps, "seam")
    assert a[3]["max_k"].min() > 0                            # no dead world: none compared as zeros
    for how in ("single", "overlapped"):
        b = _run(amd, monkeypatch, case, steps, how)
        assert a[0] == b[0], how
        for pa, pb, name in ((a[1], b[1], "light"), (a[2], b[2], "dark")):
            assert np.array_equal(pa, pb), (how, name, np.argwhere(pa != pb)[:8].tolist(), int((pa != pb).sum()))
        for f in FIELDS:
            assert np.array_equal(a[3][f], b[3][f]), (how, f)
