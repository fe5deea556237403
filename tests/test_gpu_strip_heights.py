"""GPU tests (``-m gpu``) of the wave-strip kernels at the strip heights production shapes run: 16, 32 and 64 rows.

The oracle-compared tests elsewhere use a handful of worlds, for which ``strip_rows`` (dw_plan.hpp) falls through to 8-row
strips.  Here the height is forced with ``DW_STRIP_ROWS`` on small worlds (it governs the steady-state, the step-pair and
the first-step kernels) or chosen by the batch size alone, and every case first asserts from ``kernel_info()`` that the
height it asked for is the one in use.  What changes with the height: the trip count of the row loop and its prologue /
epilogue, the ragged last strip (grid heights SR + 1 and 2 SR + 2 leave strips of 1 and 2 rows), how full a strip's
near-tie queue gets, the size of a lane's float32 partial sums, the early-out of the STATS pair kernels, and the
strip -> workgroup map (nstrips, nwg, chunk).

Exact mode: every comparison is integer equality with the float64 oracle (``oracle.c_oracle`` / ``OracleDaisyWorldC``).
Fast mode: float32 results do not depend on the launch geometry, so every output equals the same run at 8 rows bit for bit
(the 8-row results are tied to the oracle's tolerance by the rest of the suite).  There is no tolerance in this file.

  A  single steps from a quantised state: planes, dw_reduce, the retained previous planes
  B  the first step from an un-quantised state (float64 / float32 uploads, Philox)
  C  dw_step_n (step pairs + closing single steps): 9 and 41 steps of the growth - plateau - death ramp
  D  dw_step_n_trace: every row of the series
  E  dw_run_episode with agents on the strip seams, with and without world flags, through the death of the worlds
  F  dw_step_n_trace in several chunks (DW_TEST_TRACE_ROWS, and one run that really crosses 32 MiB of rows)
"""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import c_oracle  # noqa: E402

FIELDS = ("max_k", "sum_light_k", "sum_dark_k")
HEIGHTS = (16, 32, 64)
_SWITCHES = ("DW_STRIP_ROWS", "DW_PACK_MIN_STRIPS", "DW_NO_EPISODE_KERNEL", "DW_NO_EPISODE_WAVE", "DW_TEST_TRACE_ROWS",
             "DW_TEST_QUEUE_CAP", "DW_TEST_MISMATCH_CAP", "DW_NO_FUSE", "DW_NO_RING", "DW_NO_PACK", "DW_KERNEL")


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _k(x):
    return np.rint(np.asarray(x) * 1000.0).astype(np.int64)


def _family(W):
    return "packed" if W < 256 else ("rot" if W == 256 else ("ring" if W == 1024 else "ovl"))


def _set_env(monkeypatch, W, rows=None, **extra):
    """The switches of one case (the library reads them when a handle is created).  Packed worlds: the packing threshold
    down to one strip, and no LDS-resident episode kernels - small worlds would otherwise never reach the strips."""
    for name in _SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if rows:
        monkeypatch.setenv("DW_STRIP_ROWS", str(rows))
    if W < 256:
        monkeypatch.setenv("DW_PACK_MIN_STRIPS", "1")
        monkeypatch.setenv("DW_NO_EPISODE_KERNEL", "1")
        monkeypatch.setenv("DW_NO_EPISODE_WAVE", "1")
    for name, v in extra.items():
        monkeypatch.setenv(name, str(v))


def _engine(amd, B, H, W, precision, N=0):
    from therldaisyworld_amd import _ffi
    p = amd.default_params(B, H, W, N)
    p.precision = _ffi.PRECISION[precision]
    return amd.Engine(p)


def _heights_in_use(eng):
    """(rows per strip of the steady-state / pair kernels, of the first-step kernel) as the handle reports them."""
    info = eng.kernel_info()
    m = re.match(r"step_stream_\w+<halo=[\w-]+> wave-strip=(\d+)x256 ", info)
    assert m, info
    f = re.search(r"; first step: wave-strip=(\d+)x256", info)
    assert f, info
    return int(m.group(1)), int(f.group(1))


def _assert_heights(eng, steady, first):
    assert _heights_in_use(eng) == (steady, first), (eng.kernel_info(), steady, first)


RAMP_DL = 0.75 / 40.0


def _schedule(n, L0=0.8, dL=RAMP_DL):
    """test_gpu_trace._ramp (growth, plateau, decline, death of every world by step 41) accumulated the way dw_step_n
    and the oracle advance L, so that dw_step_n, dw_step_n_trace and the oracle see the same doubles."""
    Ls, L = [], L0
    for _ in range(n):
        Ls.append(L)
        L += dL
    return np.array(Ls), L


def _dense_state(B, H, W, seed):
    """A dense random QUANTISED state (per-mille integers): light + dark in 990 .. 1000 with odd values almost everywhere, a
    tenth of the cells sparse, one block with light exactly 1000 and the last world entirely 1000 / 0 - strip sums at
    their maximum.  Random on purpose: a regular pattern produces exact rounding ties."""
    rng = np.random.RandomState(seed)
    total = 990 + rng.randint(0, 11, size=(B, H, W))
    light = rng.randint(0, 495, size=(B, H, W)) * 2 + 1          # odd, below every total
    dark = total - light
    sparse = rng.rand(B, H, W) < 0.1
    light[sparse] = rng.randint(0, 300, size=int(sparse.sum()))
    dark[sparse] = rng.randint(0, 300, size=int(sparse.sum()))
    light[0, : max(1, H // 3), : max(4, W // 4)] = 1000
    dark[0, : max(1, H // 3), : max(4, W // 4)] = 0
    if B > 1:
        light[-1] = 1000
        dark[-1] = 0
    return light.astype(np.int64), dark.astype(np.int64)


def _start_state(amd, B, H, W, state, seed):
    """(kind, light, dark): kind "philox" - an un-quantised device draw, light / dark its float64 download; kind "q" -
    per-mille integer planes (developed: 200 warm-up steps of the ramp on the device; dense: _dense_state)."""
    if state == "philox":
        eng = _engine(amd, B, H, W, "exact")
        eng.init_random(seed)
        light, dark = eng.download_planes()
        eng.close()
        return "philox", light, dark
    if state == "developed":
        eng = _engine(amd, B, H, W, "exact")
        eng.init_random(seed)
        eng.step_n(200, 0.8, 0.002, 0.75, 1.5)
        assert eng.last_fixup_count() > 0, "a developed state is meant to have near-ties"
        light, dark = eng.download_planes()
        eng.close()
        return "q", _k(light), _k(dark)
    return ("q", *_dense_state(B, H, W, seed))


def _upload(eng, kind, light, dark, fmt, seed):
    if kind == "philox":
        eng.init_random(seed)
    elif fmt == "q":
        eng.upload_state_f32((light / 1000.0).astype(np.float32), (dark / 1000.0).astype(np.float32), quantised=True)
    elif fmt == "f64":                                          # the same values as an UN-QUANTISED state: first-step kernel
        eng.upload_state(light / 1000.0, dark / 1000.0)
    else:
        eng.upload_state_f32((light / 1000.0).astype(np.float32), (dark / 1000.0).astype(np.float32), quantised=False)


def _stats_of(kl, kd):
    return {"max_k": np.maximum(kl.max(axis=(1, 2)), kd.max(axis=(1, 2))), "sum_light_k": kl.sum(axis=(1, 2)),
            "sum_dark_k": kd.sum(axis=(1, 2))}


def _oracle_run(kind, light, dark, Ls, keep):
    """The float64 oracle one step at a time from the start state: per-step stats and the planes after the steps in
    `keep` (per-mille integers)."""
    l = np.ascontiguousarray(light if kind == "philox" else light / 1000.0, dtype=np.float64).copy()
    d = np.ascontiguousarray(dark if kind == "philox" else dark / 1000.0, dtype=np.float64).copy()
    rows, planes = [], {}
    for t, L in enumerate(Ls):
        c_oracle.step_n(l, d, float(L), 0.0, 1, min_L=0.0, max_L=10.0)
        kl, kd = _k(l), _k(d)
        rows.append(_stats_of(kl, kd))
        if t + 1 in keep:
            planes[t + 1] = (kl, kd)
    return rows, planes


def _snapshot(eng, previous=False):
    """Everything a run leaves behind, as integer arrays: planes, reductions, optionally the retained previous planes."""
    from therldaisyworld_amd import _ffi
    gl, gd = eng.download_planes()
    s = eng.reduce()
    out = {"light": _k(gl), "dark": _k(gd), **{f: s[f].astype(np.int64) for f in FIELDS}}
    if previous:
        pl, pd = eng.download_planes(_ffi.STATE_PREVIOUS)
        out["prev_light"], out["prev_dark"] = _k(pl), _k(pd)
    return out


def _stages(amd, B, H, W, precision, start, Ls, seed, steady, first, runs):
    """The checks A - D of one case as a dictionary of outputs.  Every engine asserts its strip heights."""
    kind, light, dark = start
    n = len(Ls)
    dL = RAMP_DL
    out = {}

    def fresh(fmt):
        eng = _engine(amd, B, H, W, precision)
        _assert_heights(eng, steady, first)
        _upload(eng, kind, light, dark, fmt, seed)
        return eng

    fmts = ["philox"] if kind == "philox" else ["q", "f64", "f32"]
    for fmt in fmts:                                            # A (fmt q) and B (the un-quantised formats): one step
        eng = fresh(fmt)
        if fmt == "f32":                                        # float32 holds k / 1000 inexactly: the state as the library holds it
            out["start", fmt] = dict(zip(("light", "dark"), eng.download_planes()))
        eng.step(float(Ls[0]))
        out["step1", fmt] = _snapshot(eng, previous=fmt == "q")
        eng.close()
    for fmt in fmts[:2]:                                        # C and D: pairs from row 0 (q) and after a first step
        for k in runs:
            eng = fresh(fmt)
            Lend = eng.step_n(k, float(Ls[0]), dL, 0.0, 10.0)
            assert Lend == _schedule(k, float(Ls[0]), dL)[1]
            out["step_n", fmt, k] = _snapshot(eng, previous=True)
            eng.close()
        eng = fresh(fmt)
        tr = eng.step_n_trace(Ls)
        out["trace", fmt] = {f: tr[f].astype(np.int64) for f in FIELDS}
        out["trace_end", fmt] = _snapshot(eng, previous=True)
        out["trace_fixups", fmt] = eng.last_fixup_count()
        eng.close()
    assert n >= max(runs)
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys(), what
    for key in a:
        if isinstance(a[key], dict):
            for f in a[key]:
                assert np.array_equal(a[key][f], b[key][f]), (what, key, f, np.argwhere(a[key][f] != b[key][f])[:4].tolist())
        else:
            assert a[key] == b[key], (what, key, a[key], b[key])


def _assert_against_oracle(out, start, Ls, runs):
    kind, light, dark = start
    n = len(Ls)
    rows, planes = _oracle_run(kind, light, dark, Ls, {1, n, *runs, *(k - 1 for k in runs), n - 1})

    def state(snap, t, what):
        kl, kd = planes[t]
        assert np.array_equal(snap["light"], kl) and np.array_equal(snap["dark"], kd), (what, "planes")
        for f in FIELDS:
            assert np.array_equal(snap[f], rows[t - 1][f]), (what, f, snap[f], rows[t - 1][f])
        if "prev_light" in snap:
            pl, pd = planes[t - 1] if t > 1 else (light, dark)
            if t > 1 or kind == "q":
                assert np.array_equal(snap["prev_light"], pl) and np.array_equal(snap["prev_dark"], pd), (what, "previous planes")

    for key, val in out.items():
        if key == ("step1", "f32"):                             # the oracle on the float32 upload as downloaded
            l, d = out["start", "f32"]["light"].copy(), out["start", "f32"]["dark"].copy()
            c_oracle.step_n(l, d, float(Ls[0]), 0.0, 1, min_L=0.0, max_L=10.0)
            kl, kd = _k(l), _k(d)
            assert np.array_equal(val["light"], kl) and np.array_equal(val["dark"], kd), (key, "planes")
            ref = _stats_of(kl, kd)
            for f in FIELDS:
                assert np.array_equal(val[f], ref[f]), (key, f)
        elif key[0] == "step1":
            state(val, 1, key)
        elif key[0] == "step_n":
            state(val, key[2], key)
        elif key[0] == "trace_end":
            state(val, n, key)
        elif key[0] == "trace":
            for f in FIELDS:
                ref = np.stack([r[f] for r in rows])
                assert np.array_equal(val[f], ref), (key, f, np.argwhere(val[f] != ref)[:4].tolist())


# ---------------------------------------------------------------------------------------------------------------------
# the case matrix of the forced heights
# ---------------------------------------------------------------------------------------------------------------------
WIDTHS = {"rot": [256], "ovl": [320, 512, 516, 4096], "ring": [1024], "packed": [64, 128, 96, 16]}
STATES = ("philox", "developed", "dense")
NWG_TARGETS = (1, 7, 8, 9, 13)


def _geometry(B, H, W, SR):
    """plan_steps' strip counts for the shape at strip height SR (dw_plan.hpp): steady-state strips, the workgroups of the
    single-step launch and of the step-pair launch."""
    sr = min(SR, H)
    nrs = (H + sr - 1) // sr
    if W < 256:
        groups, ncs, fcs = (B + 64 // (W // 4) - 1) // (64 // (W // 4)), 1, 1
    else:
        groups, ncs = B, (W + 255) // 256
        fcs = 1 if W == 256 else (1 if W == 1024 else (W + 247) // 248)
    nwg = (groups * nrs * ncs + 3) // 4
    fwg = groups * nrs * fcs if W == 1024 else (groups * nrs * fcs + 3) // 4
    return groups * nrs * ncs, nwg, fwg


def _pick_batch(H, W, SR, target):
    """The batch whose step-pair launch has `target` workgroups, or as near as the shape allows from below."""
    B = 1
    while _geometry(B + 1, H, W, SR)[2] <= target and (B + 1) * H * W <= 600000:
        B += 1
    return B


def _matrix():
    cases = []
    for si, SR in enumerate(HEIGHTS):
        for hi, H in enumerate((SR, SR + 1, SR - 1, 2 * SR + 2, 3 * SR - 1)):
            for fi, (fam, widths) in enumerate(WIDTHS.items()):
                W = widths[(si + hi) % len(widths)]
                target = NWG_TARGETS[(si + hi + fi) % len(NWG_TARGETS)]
                B = _pick_batch(H, W, SR, target)
                state = STATES[(si + hi + fi) % len(STATES)]
                cases.append(pytest.param(fam, SR, H, W, B, state, id=f"{fam}-sr{SR}-{B}x{H}x{W}-{state}"))
    return cases


MATRIX = _matrix()
# the strip -> workgroup map: launches of 1, 7, 8, 9 workgroups and of a larger count that is no multiple of 8 all occur
_NWG = {_geometry(c.values[4], c.values[2], c.values[3], c.values[1])[2] for c in MATRIX}
assert {1, 7, 8, 9} <= _NWG and any(v > 9 and v % 8 for v in _NWG), sorted(_NWG)
# every family at every height, every width of the issue's table at least once
assert {(c.values[0], c.values[1]) for c in MATRIX} == {(f, s) for f in WIDTHS for s in HEIGHTS}
assert {c.values[3] for c in MATRIX} == {w for ws in WIDTHS.values() for w in ws}


@pytest.mark.parametrize("fam,SR,H,W,B,state", MATRIX)
def test_forced_strip_heights_vs_oracle_and_vs_8_rows(amd, monkeypatch, fam, SR, H, W, B, state):
    """A, B, C, D at a forced strip height: exact mode against the oracle, fast mode against the same run at 8 rows.  The
    grid heights SR, SR + 1, SR - 1, 2 SR + 2 and 3 SR - 1 give a full strip, last strips of 1 and 2 rows and a single
    (shorter) strip; the 2 SR + 2 cases also run the whole 41-step ramp to the death of every world."""
    assert _family(W) == fam
    seed = 100 * SR + H + W
    long_run = H == 2 * SR + 2
    n = 41 if long_run else 9
    runs = (9, 41) if long_run else (9,)
    Ls, _ = _schedule(n)
    rows = min(SR, H)
    _set_env(monkeypatch, W, rows=SR)
    start = _start_state(amd, B, H, W, state, seed)
    exact = _stages(amd, B, H, W, "exact", start, Ls, seed, rows, rows, runs)
    _assert_against_oracle(exact, start, Ls, runs)
    if long_run and state != "developed":
        assert (exact["trace", "q" if start[0] == "q" else "philox"]["max_k"][-1] == 0).all(), "the ramp is meant to end in death"
    fast = _stages(amd, B, H, W, "fast", start, Ls, seed, rows, rows, runs)
    _set_env(monkeypatch, W, rows=8)
    base = _stages(amd, B, H, W, "fast", start, Ls, seed, min(8, H), min(8, H), runs)
    _assert_same(fast, base, f"fast mode, {rows} rows against 8 rows")


_DEV_LS = 1.2 + 0.00625 * np.arange(16)                       # continues the warm-up's ramp; the worlds stay populated


@pytest.mark.parametrize("SR", HEIGHTS)
@pytest.mark.parametrize("B,H,W", [(3, 130, 256), (2, 130, 320), (1, 66, 4096)])
def test_trace_from_a_developed_state_repairs_the_same_cells(amd, monkeypatch, SR, B, H, W):
    """D from a developed state (near-ties in every strip): the series equals the oracle's, and the fix-up count of the
    run's last step equals that of the same run at 8 rows - the same cells went through float64 one by one, so no strip
    overflowed its queue and fell back to a whole-strip recomputation at the taller height."""
    _set_env(monkeypatch, W, rows=SR)
    start = _start_state(amd, B, H, W, "developed", 7)
    rows, _ = _oracle_run(*start, _DEV_LS, set())
    counts = []
    for r in (SR, 8):
        _set_env(monkeypatch, W, rows=r)
        eng = _engine(amd, B, H, W, "exact")
        _assert_heights(eng, r, r)
        _upload(eng, *start, "q", 7)
        tr = eng.step_n_trace(_DEV_LS)
        for f in FIELDS:
            assert np.array_equal(tr[f].astype(np.int64), np.stack([x[f] for x in rows])), (r, f)
        counts.append(eng.last_fixup_count())
        eng.close()
    assert counts[0] == counts[1] > 0, counts


# ---------------------------------------------------------------------------------------------------------------------
# heights chosen by the batch size alone
# ---------------------------------------------------------------------------------------------------------------------
def _strip_rows(groups, H, target):
    """strip_rows of dw_plan.hpp: 64 rows, halved down to 8 until the launch has at least `target` strips."""
    sr = 64
    while sr > 8 and groups * ((H + sr - 1) // sr) < target:
        sr >>= 1
    return min(H, sr)


def _natural(B, H, W):
    groups = (B + 64 // (W // 4) - 1) // (64 // (W // 4)) if W < 256 else B * ((W + 255) // 256)
    return _strip_rows(groups, H, 2048), _strip_rows(groups, H, 4096)


# 64-row grids: 2048 / 1024 / 512 strip columns make 64 / 32 / 16 rows by the 2048-strip rule (and 32 / 16 / 8 rows of the
# first-step kernel by its 4096-strip rule); (rotating, overlapped with two strip columns per world, packed four per wave)
NATURAL = [pytest.param(B * m // d, 64, W, SR, id=f"{_family(W)}-sr{SR}-{B * m // d}x64x{W}")
           for W, m, d in ((256, 1, 1), (320, 1, 2), (64, 4, 1)) for B, SR in ((2048, 64), (1024, 32), (512, 16))]


@pytest.mark.parametrize("B,H,W,SR", NATURAL)
def test_heights_chosen_by_the_batch_vs_oracle(amd, monkeypatch, B, H, W, SR):
    """No switch set: the batch alone makes strip_rows choose the height.  From the un-quantised Philox state: the first
    step (its kernel at half the height: the 4096-strip rule), then one step pair and a closing single step, planes and
    reductions against the oracle after the first step and at the end."""
    assert _natural(B, H, W) == (SR, SR // 2)
    _set_env(monkeypatch, 256)                                  # (no switch at all: packed worlds by their own threshold)
    eng = _engine(amd, B, H, W, "exact")
    _assert_heights(eng, SR, SR // 2)
    eng.init_random(SR)
    light, dark = eng.download_planes()
    Ls, Lend = _schedule(4, 0.9, 0.05)
    eng.step(float(Ls[0]))
    c_oracle.step_n(light, dark, float(Ls[0]), 0.0, 1, min_L=0.0, max_L=10.0)
    snap = _snapshot(eng)
    assert np.array_equal(snap["light"], _k(light)) and np.array_equal(snap["dark"], _k(dark)), "first step"
    assert eng.step_n(3, float(Ls[1]), 0.05, 0.0, 10.0) == Lend
    c_oracle.step_n(light, dark, float(Ls[1]), 0.05, 3, min_L=0.0, max_L=10.0)
    snap = _snapshot(eng)
    kl, kd = _k(light), _k(dark)
    assert np.array_equal(snap["light"], kl) and np.array_equal(snap["dark"], kd), "pair + single"
    ref = _stats_of(kl, kd)
    for f in FIELDS:
        assert np.array_equal(snap[f], ref[f]), f
    eng.close()


@pytest.mark.parametrize("B,H,W", [(4096, 64, 256), (2048, 64, 320), (16384, 64, 64)],
                         ids=["rot", "ovl", "packed"])
def test_first_step_at_64_rows_chosen_by_the_batch_vs_oracle(amd, monkeypatch, B, H, W):
    """4096 strip columns: the first-step kernel's own rule gives it 64-row strips - its lanes' float32 partial sums at
    the height FirstGeom::SR allows at most.  One step, planes and reductions against the oracle."""
    assert _natural(B, H, W) == (64, 64)
    _set_env(monkeypatch, 256)
    eng = _engine(amd, B, H, W, "exact")
    _assert_heights(eng, 64, 64)
    eng.init_random(5)
    light, dark = eng.download_planes()
    eng.step(1.0)
    c_oracle.step_n(light, dark, 1.0, 0.0, 1, min_L=0.0, max_L=10.0)
    snap = _snapshot(eng)
    kl, kd = _k(light), _k(dark)
    assert np.array_equal(snap["light"], kl) and np.array_equal(snap["dark"], kd)
    ref = _stats_of(kl, kd)
    for f in FIELDS:
        assert np.array_equal(snap[f], ref[f]), f
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# E: agents on the seams
# ---------------------------------------------------------------------------------------------------------------------
def _seam_agents(B, G, SR):
    """Eight agents per world on the strip seams: rows SR - 1, SR, 0 and G - 1; columns 247 / 248 (overlapped strips),
    255 / 256 (single-step strips) where the grid has them, 0 and G - 1 (the first and last lanes of a world); the last
    agent shares the first one's cell."""
    c1, c2 = (247, 248) if G > 256 else (G // 2 - 1, G // 2)
    c3, c4 = (255, 256) if G > 256 else (3, G - 4)
    cells = [(SR - 1, c1), (SR, c2), (0, 0), (G - 1, G - 1), (SR - 1, c3), (SR, c4), (0, G - 1), (SR - 1, c1)]
    idx = np.array([[(r % G, c % G) for r, c in cells]] * B, dtype=np.int32)
    idx[1::2, :, 0] = (idx[1::2, :, 0] + SR) % G              # every other world: one strip further down
    return idx


def _episode(amd, monkeypatch, G, B, SR, precision, world_flags, oracle, seams=None):
    import test_gpu_configs as cfg
    from therldaisyworld_amd import _ffi
    N = 8
    _set_env(monkeypatch, G, rows=SR)
    eng = _engine(amd, B, G, G, precision, N)
    _assert_heights(eng, min(SR, G), min(SR, G))
    eng.init_random(31)
    L = eng.step_n(30, 1.0, 0.004, 0.75, 1.5)                   # something to graze
    eng.upload_agents(_seam_agents(B, G, seams or SR), np.ones((B, N)))
    env = cfg._oracle_like(eng, G, L) if oracle else None
    rng = np.random.RandomState(G + (seams or SR))
    dL, outs = 0.06, []
    for ci, K in enumerate((5, 8)):                             # L = 1.12 .. 1.84: every world dies inside the second chunk
        Ls = [L + i * dL for i in range(K)]
        L += K * dL
        table = rng.randint(-2, 9, size=(K, B, N)).astype(np.int8)
        alive, ok = eng.run_episode(Ls, _ffi.POLICY_TABLE, None, table, world_flags=world_flags)
        if oracle:
            for t in range(K):
                reward, done = cfg._oracle_step(env, Ls[t], cfg._resolve_codes(env, table[t]))
                assert np.array_equal(ok[t][..., None], ~done), f"chunk {ci} step {t}: agent flags"
                if world_flags:
                    mx = np.maximum(_k(env.grid[:, 1]).max(axis=(1, 2)), _k(env.grid[:, 2]).max(axis=(1, 2)))
                    assert np.array_equal(alive[t], mx > 5), f"chunk {ci} step {t}: world flags"
            r_dev, d_dev = eng.reward_done()
            assert np.array_equal(r_dev, reward) and np.array_equal(d_dev, done), f"chunk {ci}: reward / done"
            cfg._compare_exact(eng, env, Ls[-1], f"chunk {ci} (K={K}, flags={world_flags})")
        outs += [ok.copy(), None if alive is None else alive.copy(), *(_snapshot(eng).values()), *eng.download_agents()]
    if world_flags:
        assert not alive[-1].any(), "the schedule is meant to kill every world"
    eng.close()
    return outs


E_SHAPES = [(256, 3), (260, 2), (1024, 1), (64, 6)]           # rotating, overlapped (last strip: 4 rows), ring, packed


@pytest.mark.parametrize("world_flags", [False, True])
@pytest.mark.parametrize("SR", HEIGHTS)
@pytest.mark.parametrize("G,B", E_SHAPES, ids=[_family(g) for g, _ in E_SHAPES])
def test_agents_on_the_seams_exact_vs_oracle(amd, monkeypatch, G, B, SR, world_flags):
    """dw_run_episode (step pairs with the agents' step patched in, STATS pairs with world flags, closing single steps)
    with mixed table codes (-2 .. 8) for agents on the row and column seams, two of them on one cell, from a grazed
    populated state through the death of every world: agent flags, world flags, reward / done, planes, agents,
    observations and reductions against OracleDaisyWorldC after every chunk."""
    _episode(amd, monkeypatch, G, B, SR, "exact", world_flags, True)


@pytest.mark.parametrize("world_flags", [False, True])
@pytest.mark.parametrize("SR", HEIGHTS)
@pytest.mark.parametrize("G,B", E_SHAPES, ids=[_family(g) for g, _ in E_SHAPES])
def test_agents_on_the_seams_fast_equals_8_rows(amd, monkeypatch, G, B, SR, world_flags):
    a = _episode(amd, monkeypatch, G, B, SR, "fast", world_flags, False)
    b = _episode(amd, monkeypatch, G, B, 8, "fast", world_flags, False, seams=SR)   # the same agents and codes
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None and y is None) or np.array_equal(x, y), i


# ---------------------------------------------------------------------------------------------------------------------
# F: the series in several chunks
# ---------------------------------------------------------------------------------------------------------------------
def _trace_run(amd, B, H, W, precision, how, Ls, seed=19):
    eng = _engine(amd, B, H, W, precision)
    eng.init_random(seed, quantised=how == "q")
    tr = eng.step_n_trace(Ls)
    out = {"trace": {f: tr[f].astype(np.int64) for f in FIELDS}}
    if len(Ls):
        out["end"] = _snapshot(eng, previous=len(Ls) > 1 or how == "q")
    info = eng.kernel_info()
    eng.close()
    return out, info


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("B,H,W", [(3, 70, 256), (2, 40, 320), (5, 24, 64), (2, 24, 1024)])
def test_trace_in_small_chunks_equals_one_chunk(amd, monkeypatch, B, H, W, precision):
    """DW_TEST_TRACE_ROWS = 2, 4, 6 rows of the series on the device at a time, 1 .. 41 steps from un-quantised starts (a
    first step, then pairs from row 1: odd) and quantised ones (pairs from row 0): series, planes, previous planes and
    reduce() equal the run with the whole series in one chunk.  The hook is reported by the handle."""
    for how in ("unq", "q"):
        for n in (1, 2, 3, 7, 8, 41):
            Ls, _ = _schedule(n)
            _set_env(monkeypatch, W)
            ref, info = _trace_run(amd, B, H, W, precision, how, Ls)
            assert "DW_TEST_TRACE_ROWS" not in info
            for rows in (2, 4, 6):
                _set_env(monkeypatch, W, DW_TEST_TRACE_ROWS=rows)
                got, info = _trace_run(amd, B, H, W, precision, how, Ls)
                assert f"DW_TEST_TRACE_ROWS={rows}" in info
                _assert_same(got, ref, f"{how} n={n} rows={rows}")


@pytest.mark.parametrize("rows", [2, 3, 6])
def test_trace_in_small_chunks_vs_oracle(amd, monkeypatch, rows):
    """The chunked series against the oracle itself (3 is rounded down to 2 rows)."""
    B, H, W = 2, 70, 320
    _set_env(monkeypatch, W, DW_TEST_TRACE_ROWS=rows)
    for how in ("unq", "q"):
        eng = _engine(amd, B, H, W, "exact")
        eng.init_random(23, quantised=how == "q")
        light, dark = eng.download_planes()
        eng.close()
        Ls, _ = _schedule(41)
        got, _ = _trace_run(amd, B, H, W, "exact", how, Ls, seed=23)
        ref_rows, planes = _oracle_run("philox", light, dark, Ls, {41})
        for f in FIELDS:
            assert np.array_equal(got["trace"][f], np.stack([r[f] for r in ref_rows])), (how, f)
        assert np.array_equal(got["end"]["light"], planes[41][0]) and np.array_equal(got["end"]["dark"], planes[41][1])


def test_trace_across_the_32_mib_row_budget(amd, monkeypatch):
    """No hook: 65536 worlds of 8 x 8 make rows of 1.5 MiB, so 32 MiB hold 20 of them and 45 steps take three chunks;
    every row against the step-by-step loop (dw_step + dw_reduce)."""
    B, n = 65536, 45
    _set_env(monkeypatch, 256)
    Ls = np.linspace(0.9, 1.3, n)
    a, b = _engine(amd, B, 8, 8, "exact"), _engine(amd, B, 8, 8, "exact")
    for e in (a, b):
        e.init_random(3)
    tr = a.step_n_trace(Ls)
    assert tr.shape == (n, B) and tr.nbytes > 2 * (32 << 20)
    for t in range(n):
        b.step(float(Ls[t]))
        s = b.reduce()
        for f in FIELDS:
            assert np.array_equal(tr[f][t], s[f]), (t, f)
    _assert_same({"end": _snapshot(a, previous=True)}, {"end": _snapshot(b, previous=True)}, "final state")
    a.close()
    b.close()


@pytest.mark.parametrize("B,H,W", [(3, 70, 256), (2, 40, 320), (4, 16, 16)])
def test_trace_on_a_handle_with_agents_leaves_what_dw_step_leaves(amd, monkeypatch, B, H, W):
    """include/daisyworld_hip.h: after dw_step_n_trace the state, the retained previous state and the observations are
    those of the same number of dw_step(h, NULL, ...) calls - on a handle with agents: get_obs and download_grid."""
    _set_env(monkeypatch, W)
    N = 3
    for n in (1, 2, 7):
        Ls, _ = _schedule(n, 0.9, 0.02)
        a, b = _engine(amd, B, H, W, "exact", N), _engine(amd, B, H, W, "exact", N)
        for e in (a, b):
            e.init_random(41)
        tr = a.step_n_trace(Ls)
        for t in range(n):
            b.step(float(Ls[t]))
        for f in FIELDS:
            assert np.array_equal(tr[f][-1], b.reduce()[f]), (n, f)
        assert np.array_equal(a.get_obs(0.9), b.get_obs(0.9)), n
        assert np.array_equal(a.download_grid(0.9), b.download_grid(0.9)), n
        for x, y in zip(a.download_agents(), b.download_agents()):
            assert np.array_equal(x, y)
        a.close()
        b.close()
