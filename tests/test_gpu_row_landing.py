"""GPU tests (``-m gpu``) of the step-pair kernels whose input rows land in their window slots
(step_stream_fused2_land_seam_pw and step_stream_fused2_land_left_pw, StepPlan::row_landing).

The kernels load a row into the registers it stays in, from inline assembly, and read it behind a counted wait; the map and
the strip geometry are those of the seam-strip kernels.  So the check is bit identity of float32 (``fast``) ``dw_step_n``
over 5 and 6 steps - two pairs and one or two closing single steps - from a quantised, developed state (the ``_state``
recipe of tests/test_gpu_seam_strips.py), against two references: the same call under ``DW_NO_ROW_LANDING=1`` (the seam-strip
kernels, which move each row once), and the same number of ``dw_step`` calls.  Planes, the returned luminosity and the three
per-world reductions; there is no tolerance in this file.  Every case first asserts from ``kernel_info()`` which form was
planned.  A wrong wait or offset is wrong first where a strip starts and ends, hence the two short-strip shapes; the buffer
descriptors are the range-checked ones of the seam-strip kernels.

Shapes (strip height by DW_STRIP_ROWS):
  2 x 40 x 316   rows 8   leftover waves with a part-filled band
  2 x 24 x 504   rows 8   no leftover columns; the seam lane wraps to column 0
  1 x 24 x 4096  rows 8   the headline's columns
  2 x 136 x 316  rows 64  the production strip height; top and bottom wrap inside one leftover wave
  2 x 9 x 316    rows 8   a last strip of ONE row: the row loop is never entered, only the prologue and the tail land rows
  2 x 12 x 316   rows 2   strips of two rows
  3 x 44 x 520   rows 8   albedo_light = 0.8: constants that are not the defaults
"""
import numpy as np
import pytest

from test_gpu_seam_strips import ASYM, DL, FIELDS, L0, MAX_L, MIN_L, _SWITCHES, _state

pytestmark = pytest.mark.gpu

CASES = (((2, 40, 316), 8, {}), ((2, 24, 504), 8, {}), ((1, 24, 4096), 8, {}), ((2, 136, 316), 64, {}),
         ((2, 9, 316), 8, {}), ((2, 12, 316), 2, {}), ((3, 44, 520), 8, ASYM))


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _engine(amd, monkeypatch, shape, rows, consts, landing):
    from therldaisyworld_amd import _ffi
    for name in _SWITCHES + ("DW_NO_ROW_LANDING",):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("DW_STRIP_ROWS", str(rows))
    if not landing:
        monkeypatch.setenv("DW_NO_ROW_LANDING", "1")
    p = amd.default_params(*shape, 0)
    p.precision = _ffi.PRECISION["fast"]
    for k, v in consts.items():
        setattr(p, k, v)
    eng = amd.Engine(p)                                      # (the library reads the switches here)
    info = eng.kernel_info()
    assert f"wave-strip={min(rows, shape[1])}x256" in info, info
    assert "step_stream_fused2_seam_pw" in info, info        # the seam-strip layout, in either form
    assert ("step_stream_fused2_land_seam_pw" in info) == landing, info
    assert ("DW_NO_ROW_LANDING" in info) == (not landing), info
    return eng


def _run(amd, monkeypatch, case, steps, how):
    shape, rows, consts = case
    monkeypatch.delenv("DW_NO_ROW_LANDING", raising=False)
    state = _state(amd, monkeypatch, *case)
    eng = _engine(amd, monkeypatch, shape, rows, consts, how != "moves")
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
def test_step_n_bit_identical_to_the_moving_kernels_and_to_single_steps(amd, monkeypatch, case, steps):
    a = _run(amd, monkeypatch, case, steps, "landing")
    assert a[3]["max_k"].min() > 0                            # no dead world: none compared as zeros
    for how in ("moves", "single"):
        b = _run(amd, monkeypatch, case, steps, how)
        assert a[0] == b[0], how
        for pa, pb, name in ((a[1], b[1], "light"), (a[2], b[2], "dark")):
            assert np.array_equal(pa, pb), (how, name, np.argwhere(pa != pb)[:8].tolist(), int((pa != pb).sum()))
        for f in FIELDS:
            assert np.array_equal(a[3][f], b[3][f]), (how, f)
