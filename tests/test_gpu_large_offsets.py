"""GPU tests (``-m gpu``) of the addressing contract: a cell index inside one world is int32, everything above it - the
world's base, the per-world tables and records, the grids that spread the batch - is 64-bit (``check_params``).

A. Ensembles of more than 65 535 worlds (70 000 worlds of 7x5: the one-thread-per-cell kernels; of 8x8: the packed
   wave-strips).  A grid dimension holds 65 535 workgroups, and the kernels that take their world from ``blockIdx.y`` are
   launched in slices of that many worlds (``for_world_slices``, csrc/dw_api.hip): every call of the ensemble is held to
   the float64 oracle run on one world at a time, for the first and last 64 worlds and the worlds 65 500 .. 65 600 around
   the seam between two slices, and ``reduce`` to the checksums of the downloaded planes for all 70 000.

B. One handle of just over 2^32 cells per step-kernel family, with an H*W that does not divide 2^30: the cell offsets
   2^30, 2^31 and 2^32 all fall INSIDE a world, so the row and column terms are added to a world base on either side of
   each threshold.  Probe worlds (``_probes``) are read straight from the device planes, one ``hipMemcpy`` per plane, and
   compared with two references, neither of which is the code under test at this size: a small handle ("shard") that
   holds the same global worlds through ``world_offset``, and in exact mode the C oracle started from the shard's state.
   Worlds 0, 1, 2 are probes because an offset truncated to 32 bits lands in them.

No tolerance is new.  Everything is bit identity except the temperature records (the bounds of
tests/test_gpu_temperature.py: 2e-12 relative on the mean, 1e-12 on min and max, the std within 2e-12 * max) and the
un-rounded caches (the per-cell bounds of tests/test_gpu_parity.py).  The only skip is DW_ENOMEM from ``dw_create`` or
``dw_init_random*`` (a part-B case holds 8 bytes per cell, 35 GB; 70 GB with an un-quantised start).
"""
import ctypes
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import c_oracle, daisy_oracle as O  # noqa: E402

FIELDS = ("max_k", "sum_light_k", "sum_dark_k")
L0, DL, MIN_L, MAX_L = 0.95, 0.75 / 512, 0.75, 1.5
SEED = 20260
_SWITCHES = ("DW_KERNEL", "DW_PACK_MIN_STRIPS", "DW_NO_PACK", "DW_STRIP_ROWS", "DW_NO_FUSE", "DW_NO_RING", "DW_NO_FMT_PLANES",
             "DW_NO_SEAM_STRIPS", "DW_NO_SYM", "DW_FIRST_GENERIC", "DW_FIRST_STEP_F64", "DW_NO_EPISODE_KERNEL",
             "DW_NO_EPISODE_WAVE")


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


@pytest.fixture(scope="module")
def hip():
    return ctypes.CDLL("libamdhip64.so")


def _k(x):
    return np.rint(np.asarray(x) * 1000.0).astype(np.int64)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _ramp(L, n):
    """The luminosities dw_step_n takes from L on (ref update_L: clamp(L + dL))."""
    out = []
    for _ in range(n):
        out.append(L)
        L = min(max(L + DL, MIN_L), MAX_L)
    return out, L


def _engine(amd, monkeypatch, B, H, W, precision, switches=(), N=0, world_offset=0):
    """A handle created under exactly `switches`; DW_ENOMEM (the device cannot hold it) is the one permitted skip."""
    from therldaisyworld_amd import _ffi
    for name in _SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in switches:
        monkeypatch.setenv(name, value)
    p = amd.default_params(B, H, W, N)
    p.precision = _ffi.PRECISION[precision]
    p.world_offset = world_offset
    try:
        return amd.Engine(p)                                 # (the library reads the switches here)
    except _ffi.DaisyHipError as e:
        if e.code == _ffi.DW_ENOMEM:
            pytest.skip(f"the device cannot hold {B} worlds of {H}x{W}")
        raise


def _init(eng, seed, quantised=True):
    from therldaisyworld_amd import _ffi
    try:
        eng.init_random(seed, quantised=quantised)
        eng.sync()
    except _ffi.DaisyHipError as e:
        if e.code == _ffi.DW_ENOMEM:
            pytest.skip(f"the device cannot hold the initial state of {eng.B} worlds of {eng.H}x{eng.W}")
        raise


def _assert_reduce_is_checksum(red, kl, kd, what):
    """reduce() of every world against the sums and the maximum of its per-mille planes."""
    assert np.array_equal(red["sum_light_k"], kl.sum(axis=(1, 2)).astype(np.uint64)), what
    assert np.array_equal(red["sum_dark_k"], kd.sum(axis=(1, 2)).astype(np.uint64)), what
    assert np.array_equal(red["max_k"], np.maximum(kl.max(axis=(1, 2)), kd.max(axis=(1, 2))).astype(np.uint32)), what


def _assert_temps_close(rec, temp, what):
    """rec: (n,) temperature records; temp: the oracle's field (n, H, W) - the bounds of tests/test_gpu_temperature.py."""
    mean, std = temp.mean(axis=(1, 2)), temp.std(axis=(1, 2))
    mn, mx = temp.min(axis=(1, 2)), temp.max(axis=(1, 2))
    err = np.abs(rec["std"] - std)
    np.testing.assert_allclose(rec["mean"], mean, rtol=2e-12, atol=0, err_msg=what)
    np.testing.assert_allclose(rec["min"], mn, rtol=1e-12, atol=0, err_msg=what)
    np.testing.assert_allclose(rec["max"], mx, rtol=1e-12, atol=0, err_msg=what)
    assert (err <= 2e-12 * mx).all(), (what, err, mx)


# =========================================================================================================================
# A. more than 65 535 worlds
# =========================================================================================================================
BIG_B = 70000
SEL = tuple(range(64)) + tuple(range(65500, 65601)) + tuple(range(BIG_B - 64, BIG_B))
ENSEMBLES = {"generic-7x5": ((7, 5), (), "step_generic<exact>"),
             "packed-8x8": ((8, 8), (("DW_PACK_MIN_STRIPS", "1"),), "step_stream_exact<halo=packed>")}


def _numpy_world(light, dark, L, idx=None, st=None):
    """The NumPy oracle holding ONE world: covers (H, W) in natural units, luminosity L, optionally its agents."""
    n = 0 if idx is None else idx.shape[0]
    env = O.OracleDaisyWorld(grid_dimension=light.shape[-1], n_agents=n, batch_size=1)
    env.L = L
    env.set_initial_cover(light[None].copy(), dark[None].copy())
    env.agent_indices = np.zeros((1, 0, 2), dtype=np.int64) if idx is None else idx[None].astype(np.int64)
    env.agent_states = np.ones((1, 0, 1)) if st is None else st.reshape(1, n, 1).copy()
    return env


def _c_step(light, dark, L):
    """One float64 step of ONE world by the C oracle: (H, W) natural units in, per-mille integers out."""
    out = c_oracle.forward(light[None], dark[None], L)
    return _k(out[0, 1]), _k(out[0, 2])


def _records_of(kl, kd):
    return int(max(kl.max(), kd.max())), int(kl.sum()), int(kd.sum())


@pytest.mark.parametrize("name", sorted(ENSEMBLES))
def test_more_worlds_than_a_grid_dimension_holds(amd, monkeypatch, name):
    """init_random, download_planes, reduce, step, reduce_temperature, download_caches, step_n, step_n_trace_temperature
    and step_n_trace_per_world on 70 000 worlds: each either matches the oracle or the handle is refused at dw_create."""
    (H, W), switches, kernel = ENSEMBLES[name]
    B = BIG_B
    t0 = time.perf_counter()
    eng = _engine(amd, monkeypatch, B, H, W, "exact", switches)
    try:
        assert kernel in eng.kernel_info(), eng.kernel_info()
        _init(eng, SEED)
        p0 = eng.download_planes()
        k0 = _k(p0[0]), _k(p0[1])
        red = eng.reduce()
        _assert_reduce_is_checksum(red, *k0, "after init_random")
        assert red["max_k"].min() > 0                        # no dead world: none compared as zeros

        # the draw is keyed by the global world id: a shard across the seam between two launch slices draws the same worlds
        shard = _engine(amd, monkeypatch, 101, H, W, "exact", switches, world_offset=65500)
        try:
            _init(shard, SEED)
            sl, sd = shard.download_planes()
            assert _bits(sl) == _bits(p0[0][65500:65601]) and _bits(sd) == _bits(p0[1][65500:65601])
            sred = shard.reduce()
            for f in FIELDS:
                assert np.array_equal(sred[f], red[f][65500:65601]), f
        finally:
            shard.close()

        # step: the single-step kernel
        eng.step(L0)
        p1 = eng.download_planes()
        k1 = _k(p1[0]), _k(p1[1])
        red = eng.reduce()
        _assert_reduce_is_checksum(red, *k1, "after step")
        for b in SEL:
            ol, od = _c_step(p0[0][b], p0[1][b], L0)
            assert np.array_equal(k1[0][b], ol) and np.array_equal(k1[1][b], od), ("step", b)

        # reduce_temperature and download_caches: the field that step computed (the previous state at L0)
        rt = eng.reduce_temperature(L0)
        t, bt, gr, te = eng.download_caches(L0)
        assert np.array_equal(rt["min"], t[:, 0].min(axis=(1, 2))) and np.array_equal(rt["max"], t[:, 0].max(axis=(1, 2)))
        for b in SEL:
            env = _numpy_world(p0[0][b], p0[1][b], L0)
            _assert_temps_close(rt[b:b + 1], env.temp[0], f"reduce_temperature, world {b}")
            for ours, ref in ((t[b, 0], env.temp), (t[b, 1], env.temp_light), (t[b, 2], env.temp_dark), (te[b, 0], env.temp_effective)):
                np.testing.assert_allclose(ours, ref[0, 0], rtol=1e-12, atol=0, err_msg=f"caches, world {b}")
            for ours, ref in ((bt[b, 0], env.beta), (bt[b, 1], env.beta_l), (bt[b, 2], env.beta_d)):
                np.testing.assert_allclose(ours, ref[0, 0], rtol=1e-9, atol=1e-12, err_msg=f"caches, world {b}")
            np.testing.assert_allclose(gr[b], env.growth[0], rtol=1e-9, atol=1e-14, err_msg=f"caches, world {b}")
        del t, bt, gr, te

        # step_n over 5 steps
        Ls, L_end = _ramp(L0 + DL, 5)
        assert eng.step_n(5, Ls[0], DL, MIN_L, MAX_L) == L_end
        p2 = eng.download_planes()
        k2 = _k(p2[0]), _k(p2[1])
        red = eng.reduce()
        _assert_reduce_is_checksum(red, *k2, "after step_n")
        for b in SEL:
            ol, od = p1[0][b:b + 1].copy(), p1[1][b:b + 1].copy()
            assert c_oracle.step_n(ol, od, Ls[0], DL, 5, MIN_L, MAX_L) == L_end
            assert np.array_equal(k2[0][b], _k(ol[0])) and np.array_equal(k2[1][b], _k(od[0])), ("step_n", b)

        # step_n_trace_temperature over 3 steps
        Lt, _ = _ramp(L_end, 3)
        stats, temps = eng.step_n_trace_temperature(Lt)
        assert stats.shape == temps.shape == (3, B)
        p3 = eng.download_planes()
        k3 = _k(p3[0]), _k(p3[1])
        red = eng.reduce()
        _assert_reduce_is_checksum(red, *k3, "after step_n_trace_temperature")
        for f in FIELDS:
            assert np.array_equal(stats[-1][f], red[f]), f
        for b in SEL:
            env = _numpy_world(p2[0][b], p2[1][b], Lt[0])
            for s in range(3):
                env.L = Lt[s]
                env.grid = env.forward(env.grid)
                _assert_temps_close(temps[s, b:b + 1], env.temp[0], f"step_n_trace_temperature, step {s}, world {b}")
                rec = _records_of(_k(env.grid[0, 1]), _k(env.grid[0, 2]))
                assert tuple(int(stats[s, b][f]) for f in FIELDS) == rec, ("step_n_trace_temperature", s, b)
            assert np.array_equal(k3[0][b], _k(env.grid[0, 1])) and np.array_equal(k3[1][b], _k(env.grid[0, 2])), b

        # step_n_trace_per_world over 3 steps: a luminosity column per world, not monotone in b
        Lpw = np.ascontiguousarray(0.8 + 0.5 * ((np.arange(B) * 7919) % 1000)[None, :] / 1000.0 + 0.01 * np.arange(3)[:, None])
        stats = eng.step_n_trace_per_world(Lpw)
        p4 = eng.download_planes()
        k4 = _k(p4[0]), _k(p4[1])
        red = eng.reduce()
        _assert_reduce_is_checksum(red, *k4, "after step_n_trace_per_world")
        for f in FIELDS:
            assert np.array_equal(stats[-1][f], red[f]), f
        for b in SEL:
            ol, od = p3[0][b], p3[1][b]
            for s in range(3):
                kl, kd = _c_step(ol, od, float(Lpw[s, b]))
                assert tuple(int(stats[s, b][f]) for f in FIELDS) == _records_of(kl, kd), ("step_n_trace_per_world", s, b)
                ol, od = kl / 1000.0, kd / 1000.0
            assert np.array_equal(k4[0][b], kl) and np.array_equal(k4[1][b], kd), ("step_n_trace_per_world", b)
    finally:
        eng.close()
    print(f"{name}: {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("name", sorted(ENSEMBLES))
def test_agents_of_more_worlds_than_a_grid_dimension_holds(amd, monkeypatch, name):
    """70 000 worlds with 2 agents each: init_random's agents, policy_greedy, step_device_actions, get_obs and
    download_agents against the NumPy oracle and its Greedy(epsilon=0), one world at a time."""
    (H, W), switches, kernel = ENSEMBLES[name]
    B, N = BIG_B, 2
    t0 = time.perf_counter()
    eng = _engine(amd, monkeypatch, B, H, W, "exact", switches, N=N)
    try:
        assert kernel in eng.kernel_info(), eng.kernel_info()
        _init(eng, SEED)
        p0 = eng.download_planes()
        idx0, st0 = eng.download_agents()
        assert (idx0 >= 0).all() and (idx0[..., 0] < H).all() and (idx0[..., 1] < W).all() and (st0 == 1.0).all()
        shard = _engine(amd, monkeypatch, 101, H, W, "exact", switches, N=N, world_offset=65500)
        try:
            _init(shard, SEED)
            assert _bits(shard.download_agents()[0]) == _bits(idx0[65500:65601])
        finally:
            shard.close()
        eng.policy_greedy()
        actions = eng.download_actions()
        eng.step_device_actions(L0)
        obs = eng.get_obs(L0)
        idx1, st1 = eng.download_agents()
        p1 = eng.download_planes()
        for b in SEL:
            env = _numpy_world(p0[0][b], p0[1][b], L0, idx0[b], st0[b])
            a = O.OracleGreedy(epsilon=0.0, greedy=True)(env.get_obs(env.agent_indices))
            assert np.array_equal(actions[b], a[0, :, 0]), ("policy_greedy", b)
            env.step(a.astype(np.int64))
            assert np.array_equal(idx1[b], env.agent_indices[0]), ("agent positions", b)
            assert np.array_equal(st1[b], env.agent_states[0, :, 0]), ("agent states", b)
            assert np.array_equal(_k(p1[0][b]), _k(env.grid[0, 1])) and np.array_equal(_k(p1[1][b]), _k(env.grid[0, 2])), b
            assert np.array_equal(obs[b], env.get_obs(env.agent_indices)[0]), ("observations", b)
        _assert_reduce_is_checksum(eng.reduce(), _k(p1[0]), _k(p1[1]), "after step_device_actions")
    finally:
        eng.close()
    print(f"{name} with agents: {time.perf_counter() - t0:.1f} s")


# =========================================================================================================================
# B. cell offsets past 2^30, 2^31 and 2^32 in every step-kernel family
# =========================================================================================================================
_PACK = (("DW_PACK_MIN_STRIPS", "1"),)                       # a shard of 3 worlds stays in the packed family
_TILED = (("DW_KERNEL", "tiled"),)
# family -> (B, H, W), switches of the big handle, extra switches of its shards, what kernel_info() must say by precision
FAMILIES = {
    "seam": ((8100, 130, 4096), (), (), {"fast": ("step_stream_fast<halo=dpp-old>", "step_stream_fused2_seam_pw", "trace: step pairs"),
                                         "exact": ("step_stream_exact<halo=dpp-old>", "(step_stream_fused2_exact)", "trace: step pairs")}),
    "rotating": ((168000, 100, 256), (), (), {"fast": ("step_stream_fast<halo=rotate>", "fuses step pairs", "trace: step pairs"),
                                              "exact": ("step_stream_exact<halo=rotate>", "fuses step pairs", "trace: step pairs")}),
    # (W == 1024 without DW_NO_RING: one workgroup per row strip; its pairs are not traced)
    "ring": ((60000, 70, 1024), (), (), {"fast": ("step_stream_fast<halo=dpp-old>", "fuses step pairs", "trace: single steps"),
                                         "exact": ("step_stream_exact<halo=dpp-old>", "fuses step pairs", "trace: single steps")}),
    "packed16": ((1343000, 50, 64), (), _PACK, {"fast": ("step_stream_fast<halo=packed>", "fuses step pairs"),
                                                "exact": ("step_stream_exact<halo=packed>", "fuses step pairs")}),
    "packed24": ((1119000, 40, 96), (), _PACK, {"fast": ("step_stream_fast<halo=packed>", "fuses step pairs"),
                                                "exact": ("step_stream_exact<halo=packed>", "fuses step pairs")}),
    "tiled": ((168000, 100, 256), _TILED, (), {"fast": ("step_tiled<TCQ=64,RPT=4,fast>",), "exact": ("step_tiled<TCQ=64,RPT=4,exact>",)}),
    # (the one family whose launches are sliced by worlds: 30 slices of 65 535)
    "generic": ((1943000, 33, 67), (), (), {"fast": ("step_generic<fast>",), "exact": ("step_generic<exact>",)}),
}
TRACED = ("seam", "rotating")                                # the families whose dw_step_n_trace runs the trace_pair_* kernels
THRESHOLDS = (1 << 30, 1 << 31, 1 << 32)


def _probes(B, H, W):
    """The probe worlds as runs of adjacent worlds [(first, count)]: 0, 1, 2; the world that holds each threshold and its
    two neighbours; B-2, B-1."""
    n = H * W
    assert B * n > THRESHOLDS[-1] and all(t % n for t in THRESHOLDS)      # every threshold falls inside a world
    worlds = {0, 1, 2, B - 2, B - 1}
    for t in THRESHOLDS:
        worlds |= {t // n - 1, t // n, t // n + 1}
    worlds = sorted(worlds)
    assert 0 <= worlds[0] and worlds[-1] < B
    runs = []
    for w in worlds:
        if runs and runs[-1][0] + runs[-1][1] == w:
            runs[-1][1] += 1
        else:
            runs.append([w, 1])
    return [tuple(r) for r in runs]


def _read_worlds(hip, eng, first, count):
    """The two binary16 planes of worlds [first, first + count) straight from the device: (2, count, H, W) float16, one
    hipMemcpy per plane, the address computed in Python integers."""
    n = eng.H * eng.W
    out = np.empty((2, count, eng.H, eng.W), dtype=np.float16)
    eng.sync()
    for pi, ptr in enumerate(eng.device_planes()):
        rc = hip.hipMemcpy(ctypes.c_void_p(out[pi].ctypes.data), ctypes.c_void_p(ptr + 2 * first * n),
                           ctypes.c_size_t(2 * count * n), 2)    # hipMemcpyDeviceToHost
        assert rc == 0, rc
    return out


class _Case:
    """One big handle and a small handle per run of probe worlds, driven in lock step."""

    def __init__(self, amd, monkeypatch, hip, family, precision, N=0):
        (B, H, W), switches, shard_switches, says = FAMILIES[family]
        self.hip, self.family, self.precision = hip, family, precision
        self.runs = _probes(B, H, W)
        self.big = None
        self.shards = []
        try:
            self.big = _engine(amd, monkeypatch, B, H, W, precision, switches, N=N)
            info = self.big.kernel_info()
            for text in says[precision]:
                assert text in info, (text, info)
            for first, count in self.runs:
                self.shards.append(_engine(amd, monkeypatch, count, H, W, precision, switches + shard_switches, N=N,
                                           world_offset=first))
                assert says[precision][0] in self.shards[-1].kernel_info(), self.shards[-1].kernel_info()
        except BaseException:
            self.close()
            raise

    def close(self):
        for e in self.shards + ([self.big] if self.big is not None else []):
            e.close()
        self.shards, self.big = [], None

    def each(self, f):
        """f(engine) on the big handle, then on every shard."""
        f(self.big)
        for s in self.shards:
            f(s)

    def assert_planes_equal(self, what):
        """The big handle's probe worlds against the shards', bit for bit; returns the per-mille planes [(2, count, H, W)]."""
        out, differ = [], []
        for (first, count), s in zip(self.runs, self.shards):
            big = _read_worlds(self.hip, self.big, first, count)
            ref = _read_worlds(self.hip, s, 0, count)
            same = (big.view(np.uint16) == ref.view(np.uint16)).all(axis=(0, 2, 3))
            differ += [first + int(i) for i in np.flatnonzero(~same)]
            out.append(big.astype(np.int64))
        assert not differ, (self.family, self.precision, what, "probe worlds that differ from their shard", differ)
        return out

    def assert_rows_equal(self, rows, shard_rows, what):
        """(..., B) records of the big handle against the shards' (..., count), field by field."""
        for (first, count), ref in zip(self.runs, shard_rows):
            for f in ref.dtype.names:
                if f != "reserved":
                    assert _bits(rows[..., first:first + count][f]) == _bits(ref[f]), (self.family, self.precision, what, f, first)

    def assert_reduce(self, what, oracle=None):
        """reduce(): probe rows against the shards' (and the oracle's planes); every world alive and within range."""
        n = self.big.H * self.big.W
        red = self.big.reduce()
        self.assert_rows_equal(red, [s.reduce() for s in self.shards], what)
        assert red["max_k"].min() > 0 and red["max_k"].max() <= 1000, what      # no world is compared as zeros
        assert (red["sum_light_k"] + red["sum_dark_k"] <= 1000 * n).all(), what
        if oracle is not None:
            for (first, count), (kl, kd) in zip(self.runs, oracle):
                _assert_reduce_is_checksum(red[first:first + count], kl, kd, (what, first))
        return red


def _oracle_states(shards):
    """The shards' current states as the C oracle takes them: [(light, dark)] float64 natural units, (count, H, W)."""
    return [tuple(np.ascontiguousarray(x) for x in s.download_planes()) for s in shards]


def _assert_oracle_planes(case, planes, states, what):
    for (first, _), got, (ol, od) in zip(case.runs, planes, states):
        assert np.array_equal(got[0], _k(ol)) and np.array_equal(got[1], _k(od)), (case.family, what, first)


@pytest.mark.parametrize("precision", ("exact", "fast"))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_offsets_beyond_32_bits(amd, monkeypatch, hip, family, precision):
    """init_random, one step, step_n over 5 steps (two pairs and the closing single step), reduce - and on the traced
    families step_n_trace over 4 steps, on the rotating strips reduce_temperature - on just over 2^32 cells."""
    t0 = time.perf_counter()
    case = _Case(amd, monkeypatch, hip, family, precision)
    exact = precision == "exact"
    try:
        case.each(lambda e: _init(e, SEED))
        case.assert_planes_equal("init_random")
        states = _oracle_states(case.shards) if exact else None

        case.each(lambda e: e.step(L0))
        planes = case.assert_planes_equal("step")
        if exact:
            states = [tuple(np.ascontiguousarray(c_oracle.forward(ol, od, L0)[:, ch]) for ch in (1, 2)) for ol, od in states]
            _assert_oracle_planes(case, planes, states, "step")

        Ls, L_end = _ramp(L0 + DL, 5)
        case.each(lambda e: e.step_n(5, Ls[0], DL, MIN_L, MAX_L))
        planes = case.assert_planes_equal("step_n")
        if exact:
            for ol, od in states:
                assert c_oracle.step_n(ol, od, Ls[0], DL, 5, MIN_L, MAX_L) == L_end
            _assert_oracle_planes(case, planes, states, "step_n")
        red = case.assert_reduce("reduce after step_n", [(_k(ol), _k(od)) for ol, od in states] if exact else None)

        if family in TRACED:
            Lt, _ = _ramp(L_end, 4)
            rec = case.big.step_n_trace(Lt)
            assert rec.shape == (4, case.big.B)
            case.assert_rows_equal(rec, [s.step_n_trace(Lt) for s in case.shards], "step_n_trace")
            planes = case.assert_planes_equal("step_n_trace")
            if exact:
                for i, L in enumerate(Lt):
                    states = [tuple(np.ascontiguousarray(c_oracle.forward(ol, od, L)[:, ch]) for ch in (1, 2)) for ol, od in states]
                    for (first, count), (ol, od) in zip(case.runs, states):
                        _assert_reduce_is_checksum(rec[i, first:first + count], _k(ol), _k(od), ("step_n_trace", i, first))
                _assert_oracle_planes(case, planes, states, "step_n_trace")
            red = case.assert_reduce("reduce after step_n_trace", [(_k(ol), _k(od)) for ol, od in states] if exact else None)
            for f in FIELDS:
                assert np.array_equal(rec[-1][f], red[f]), f

        if family == "rotating":
            temps = case.big.reduce_temperature(L0)
            case.assert_rows_equal(temps, [s.reduce_temperature(L0) for s in case.shards], "reduce_temperature")
            assert np.isfinite(temps["mean"]).all() and (temps["min"] <= temps["max"]).all()
    finally:
        case.close()
    print(f"{family}-{precision}: {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("family", ("seam", "packed16", "generic"))
def test_first_step_from_an_unquantised_state_beyond_32_bits(amd, monkeypatch, hip, family):
    """init_random without `quantised` (float32 per-mille planes: the un-quantised draw), then one step in exact mode -
    step_first_stream, or step_generic on the narrow odd shape - against the C oracle started from the shards' downloaded
    initial states."""
    t0 = time.perf_counter()
    case = _Case(amd, monkeypatch, hip, family, "exact")
    try:
        info = case.big.kernel_info()
        assert ("first step: wave-strip" in info) == (family != "generic"), info
        case.each(lambda e: _init(e, SEED, quantised=False))
        states = _oracle_states(case.shards)
        assert all(len(np.unique(ol)) > 250 for ol, _ in states)            # un-quantised: more values than the 200 per-mille steps
        case.each(lambda e: e.step(L0))
        planes = case.assert_planes_equal("first step")
        states = [tuple(np.ascontiguousarray(c_oracle.forward(ol, od, L0)[:, ch]) for ch in (1, 2)) for ol, od in states]
        _assert_oracle_planes(case, planes, states, "first step")
        case.assert_reduce("reduce after the first step", [(_k(ol), _k(od)) for ol, od in states])
    finally:
        case.close()
    print(f"{family} first step: {time.perf_counter() - t0:.1f} s")


def test_agents_beyond_32_bits(amd, monkeypatch, hip):
    """The rotating-strip shape with 2 agents per world: init_random, policy_greedy, 3 x step_device_actions; agents and
    observations of the whole ensemble, compared at the probe worlds with the shards'."""
    t0 = time.perf_counter()
    case = _Case(amd, monkeypatch, hip, "rotating", "exact", N=2)
    try:
        case.each(lambda e: _init(e, SEED))
        L = L0
        for _ in range(3):
            case.each(lambda e: e.policy_greedy())
            case.each(lambda e: e.step_device_actions(L))
            L += DL
        case.assert_planes_equal("step_device_actions")
        idx, st = case.big.download_agents()
        obs = case.big.get_obs(L0)
        assert st.min() >= 0.0 and st.max() <= 1.0 and len(np.unique(st)) > 2      # the agents grazed
        for (first, count), s in zip(case.runs, case.shards):
            sidx, sst = s.download_agents()
            assert _bits(idx[first:first + count]) == _bits(sidx) and _bits(st[first:first + count]) == _bits(sst), first
            assert _bits(obs[first:first + count]) == _bits(s.get_obs(L0)), first
        case.assert_reduce("reduce after step_device_actions")
    finally:
        case.close()
    print(f"rotating with agents: {time.perf_counter() - t0:.1f} s")
