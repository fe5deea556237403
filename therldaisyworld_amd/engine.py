"""`Engine`: a thin NumPy-in / NumPy-out object over the C ABI (include/daisyworld_hip.h).

It owns one ``dw_handle`` (one HIP device, one stream).  All compute happens in the HIP library; this
class only marshals arrays and raises ``DaisyHipError`` on any failure.  The gym-style drop-in
``therldaisyworld_amd.RLDaisyWorld`` is built on it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import DwParams, DwTempStats, DwWorldStats

VON_NEUMANN_MASK = 0x0BA
MOORE_MASK = 0x1FF


def mask_bits(neighborhood: np.ndarray) -> int:
    """3x3 0/1 array -> the 9-bit row-major mask of dw_params.obs_mask."""
    nb = np.asarray(neighborhood)
    if nb.shape != (3, 3):
        raise ValueError("only kr=1 (3x3) observation neighbourhoods are supported "
                         "(the reference hard-codes 3, daisy_world_rl.py:258)")
    bits = 0
    for i, v in enumerate(nb.ravel()):
        if v:
            bits |= 1 << i
    return bits


def default_params(batch, height, width, n_agents) -> DwParams:
    p = DwParams()
    _ffi.check(_ffi.load().dw_default_params(C.byref(p), batch, height, width, n_agents))
    return p


def _mlp_episode_args(B, N, params, n_members, member_a, member_b, split):
    """What run_episode_mlp and run_episode_mlp_fitness pass alike: (parameter sets or None, their number, the two
    member maps as int32 or None, the split)."""
    if params is None:
        if n_members is None:
            raise ValueError("params=None needs n_members (the sets uploaded by an earlier call)")
        w, nm = None, int(n_members)
    else:
        w = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 1808)
        nm = w.shape[0]
    ma = None if member_a is None else np.ascontiguousarray(member_a, dtype=np.int32)
    mb = None if member_b is None else np.ascontiguousarray(member_b, dtype=np.int32)
    for m in (ma, mb):
        if m is not None and m.shape != (B,):
            raise ValueError(f"member maps must have shape {(B,)}")
    split = N // 2 if split is None else int(split)
    return w, nm, ma, mb, split


class Engine:
    def __init__(self, params: DwParams, lib_path=None):
        self._lib = _ffi.load(lib_path)
        self._h = C.c_void_p()
        self.params = DwParams()
        C.memmove(C.byref(self.params), C.byref(params), C.sizeof(DwParams))
        self._check(self._lib.dw_create(C.byref(self.params), C.byref(self._h)))
        p = self.params
        self.B, self.H, self.W, self.N = p.batch, p.height, p.width, p.n_agents

    def _check(self, rc):
        _ffi.check(rc, self._lib)                           # the message of THIS engine's library build

    # -- life cycle ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.dw_destroy(self._h)
            self._h = C.c_void_p()
        for blk in (getattr(self, "_pinned", None) or {}).values():   # (arrays handed out with reuse_buffers die with them)
            self._lib.dw_pinned_free(blk[0])
        self._pinned = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, params: DwParams):
        self._check(self._lib.dw_set_params(self._h, C.byref(params)))
        C.memmove(C.byref(self.params), C.byref(params), C.sizeof(DwParams))

    # -- state --------------------------------------------------------------------------------
    def _plane(self, a, dtype):
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.shape != (self.B, self.H, self.W):
            raise ValueError(f"plane shape {a.shape} != {(self.B, self.H, self.W)}")
        return a

    def upload_state(self, light, dark):
        light, dark = self._plane(light, np.float64), self._plane(dark, np.float64)
        self._check(self._lib.dw_upload_state_f64(self._h, _ffi.ptr_d(light), _ffi.ptr_d(dark)))

    def upload_state_f32(self, light, dark, quantised=False):
        light, dark = self._plane(light, np.float32), self._plane(dark, np.float32)
        self._check(self._lib.dw_upload_state_f32(self._h, _ffi.ptr_f(light), _ffi.ptr_f(dark), int(quantised)))

    def upload_agents(self, indices, states):
        idx = np.ascontiguousarray(indices, dtype=np.int32).reshape(self.B, self.N, 2)
        st = np.ascontiguousarray(states, dtype=np.float64).reshape(self.B, self.N)
        self._check(self._lib.dw_upload_agents(self._h, _ffi.ptr_i(idx), _ffi.ptr_d(st)))

    def download_agents(self):
        idx = np.empty((self.B, self.N, 2), dtype=np.int32)
        st = np.empty((self.B, self.N), dtype=np.float64)
        self._check(self._lib.dw_download_agents(self._h, _ffi.ptr_i(idx), _ffi.ptr_d(st)))
        return idx, st

    def init_random(self, seed: int, quantised: bool = False):
        """Device Philox initial state; quantised=True: covers rounded to 3 decimals, straight into the binary16
        planes (no float32 staging of the un-quantised state, no float64 first step)."""
        fn = self._lib.dw_init_random_quantised if quantised else self._lib.dw_init_random
        self._check(fn(self._h, C.c_uint64(seed & (2 ** 64 - 1))))

    def download_planes(self, which=_ffi.STATE_CURRENT):
        light = np.empty((self.B, self.H, self.W))
        dark = np.empty((self.B, self.H, self.W))
        self._check(self._lib.dw_download_planes(self._h, which, _ffi.ptr_d(light), _ffi.ptr_d(dark)))
        return light, dark

    def download_grid(self, L_init=0.75):
        grid = np.empty((self.B, 7, self.H, self.W))
        self._check(self._lib.dw_download_grid(self._h, float(L_init), _ffi.ptr_d(grid)))
        return grid

    def download_caches(self, L, temps=True, betas=True, growth=True, temp_effective=True):
        B, H, W = self.B, self.H, self.W
        t = np.empty((B, 3, H, W)) if temps else None
        b = np.empty((B, 3, H, W)) if betas else None
        g = np.empty((B, 2, H, W)) if growth else None
        e = np.empty((B, 1, H, W)) if temp_effective else None
        self._check(self._lib.dw_download_caches(self._h, float(L), _ffi.ptr_d(t), _ffi.ptr_d(b), _ffi.ptr_d(g),
                                           _ffi.ptr_d(e)))
        return t, b, g, e

    # -- hot path -----------------------------------------------------------------------------
    @staticmethod
    def _actions(action):
        """(b, n, 1) or (b, n) integer-valued array -> C-contiguous int32 (b, n)."""
        a = np.asarray(action)
        if a.ndim == 3:
            a = a[..., 0]
        if a.ndim != 2:
            raise ValueError(f"action must have shape (b, n, 1); got {np.shape(action)}")
        if not np.issubdtype(a.dtype, np.integer):
            ai = np.rint(a)
            if not np.array_equal(ai, a):
                raise ValueError("non-integral action codes are not supported")
            a = ai
        return np.ascontiguousarray(a, dtype=np.int32)

    def step(self, L, action=None):
        if action is None:
            self._check(self._lib.dw_step(self._h, None, 0, 0, float(L)))
        else:
            a = self._actions(action)
            self._check(self._lib.dw_step(self._h, _ffi.ptr_i(a), a.shape[0], a.shape[1], float(L)))

    def env_step(self, L, action=None):
        """step + get_obs + reward/done in one call with one synchronisation.  Returns
        (obs (B,N,7,3,3), reward (B,N,1), done (B,N,1) bool)."""
        obs = np.zeros((self.B, self.N, 7, 3, 3))
        reward = np.zeros((self.B, self.N, 1))
        done = np.zeros((self.B, self.N, 1), dtype=np.uint8)
        if action is None:
            a, ab, an = None, 0, 0
        else:
            a = self._actions(action)
            ab, an = a.shape
        self._check(self._lib.dw_env_step(self._h, _ffi.ptr_i(a), ab, an, float(L), _ffi.ptr_d(obs), _ffi.ptr_d(reward),
                                    _ffi.ptr_u8(done)))
        return obs, reward, done.astype(bool)

    def step_device_actions(self, L):
        self._check(self._lib.dw_step_device_actions(self._h, float(L)))

    def step_n(self, nsteps, L, dL, min_L, max_L, use_device_actions=False):
        Lc = C.c_double(float(L))
        self._check(self._lib.dw_step_n(self._h, int(nsteps), C.byref(Lc), float(dL), float(min_L), float(max_L),
                                  int(bool(use_device_actions))))
        return Lc.value

    def step_n_trace(self, L_schedule):
        """`len(L_schedule)` agent-free steps, step t with luminosity `L_schedule[t]`, and the per-step, per-world
        reductions of the whole run: an array of shape (n, B), dtype `_ffi.STATS_DTYPE`, whose row t is what `reduce()`
        would return after step t (`reserved` unspecified).  Recorded on the device, one download at the end."""
        Ls = np.ascontiguousarray(L_schedule, dtype=np.float64).reshape(-1)
        out = np.zeros((Ls.size, self.B), dtype=_ffi.STATS_DTYPE)
        self._check(self._lib.dw_step_n_trace(self._h, int(Ls.size), _ffi.ptr_d(Ls),
                                        out.ctypes.data_as(C.POINTER(DwWorldStats))))
        return out

    def step_n_trace_per_world(self, L, trace=True):
        """`len(L)` agent-free steps with a luminosity per WORLD: `L` is (n, B), world b takes step t at `L[t, b]`
        (`dw_step_n_trace_per_world`) - each world ends exactly where a one-world engine stepped with its column would.
        Returns the (n, B) records of `step_n_trace`, or None with `trace=False`.  Afterwards the engine has no single
        luminosity of the last step: `download_grid` / `get_obs` raise until a shared-L step or an upload."""
        Ls = np.ascontiguousarray(L, dtype=np.float64)
        if Ls.ndim != 2 or Ls.shape[1] != self.B:
            raise ValueError(f"per-world luminosities need shape (n, {self.B}), got {Ls.shape}")
        out = np.zeros(Ls.shape, dtype=_ffi.STATS_DTYPE) if trace else None
        self._check(self._lib.dw_step_n_trace_per_world(
            self._h, int(Ls.shape[0]), _ffi.ptr_d(Ls), out.ctypes.data_as(C.POINTER(DwWorldStats)) if trace else None))
        return out

    def step_n_trace_temperature(self, L_schedule, trace=True):
        """`len(L_schedule)` agent-free single steps that also record the per-world statistics of the local temperature
        field each step computes (`dw_step_n_trace_temperature`; the reference's `env.temp` after that step).
        `L_schedule` is 1-D (one luminosity per step, as `step_n_trace`) or (n, B) (one per step and world, as
        `step_n_trace_per_world`, and the engine is "per-world" afterwards).  Returns `(stats, temps)`: the (n, B) records
        of `step_n_trace` (None with `trace=False`) and (n, B) records of dtype `_ffi.TEMP_STATS_DTYPE` (mean, std, min,
        max in kelvin; std with ddof = 0).  The state afterwards is that of the cover-only trace calls, bit for bit."""
        Ls = np.ascontiguousarray(L_schedule, dtype=np.float64)
        if Ls.ndim == 2 and Ls.shape[1] != self.B or Ls.ndim not in (1, 2):
            raise ValueError(f"luminosities need shape (n,) or (n, {self.B}), got {Ls.shape}")
        n = int(Ls.shape[0])
        out = np.zeros((n, self.B), dtype=_ffi.STATS_DTYPE) if trace else None
        temps = np.zeros((n, self.B), dtype=_ffi.TEMP_STATS_DTYPE)
        self._check(self._lib.dw_step_n_trace_temperature(
            self._h, n, _ffi.ptr_d(Ls), int(Ls.ndim == 2), out.ctypes.data_as(C.POINTER(DwWorldStats)) if trace else None,
            temps.ctypes.data_as(C.POINTER(DwTempStats))))
        return out, temps

    def world_params(self):
        """The engine's own physics constants as one record of dtype `_ffi.WORLD_PARAMS_DTYPE` (`dw_world_params_of`): a
        row of the table `step_n_trace_ensemble` takes."""
        out = np.zeros((), dtype=_ffi.WORLD_PARAMS_DTYPE)
        self._check(self._lib.dw_world_params_of(self._h, out.ctypes.data_as(C.POINTER(_ffi.DwWorldParams))))
        return out

    def _world_table(self, worlds):
        """`worlds` as a contiguous (B,) array of `_ffi.WORLD_PARAMS_DTYPE`: a structured array with those fields, or a
        (B, 12) float64 array in the struct's order."""
        w = np.asarray(worlds)
        if w.dtype.names is not None:
            if set(w.dtype.names) != set(_ffi.WORLD_PARAM_NAMES):
                raise ValueError(f"per-world constants need the fields {_ffi.WORLD_PARAM_NAMES}, got {w.dtype.names}")
            tab = np.zeros(w.shape, dtype=_ffi.WORLD_PARAMS_DTYPE)
            for name in _ffi.WORLD_PARAM_NAMES:
                tab[name] = w[name]
        else:
            w = np.ascontiguousarray(w, dtype=np.float64)
            if w.ndim != 2 or w.shape[1] != len(_ffi.WORLD_PARAM_NAMES):
                raise ValueError(f"per-world constants need shape ({self.B}, {len(_ffi.WORLD_PARAM_NAMES)}), got {w.shape}")
            tab = w.view(_ffi.WORLD_PARAMS_DTYPE).reshape(-1)
        if tab.shape != (self.B,):
            raise ValueError(f"per-world constants need shape ({self.B},) records or ({self.B}, "
                             f"{len(_ffi.WORLD_PARAM_NAMES)}) values, got {np.shape(worlds)}")
        return np.ascontiguousarray(tab)

    def step_n_trace_ensemble(self, worlds, L, temperature=False, trace=True):
        """`len(L)` agent-free steps, world b with the physics constants `worlds[b]` (a structured array of dtype
        `_ffi.WORLD_PARAMS_DTYPE`, or (B, 12) float64 in the struct's order; `world_params()` is the engine's own row) at
        the luminosity `L[t, b]` (`dw_step_n_trace_ensemble`): each world ends exactly where a one-world engine with those
        constants would.  Returns the (n, B) records of `step_n_trace` (None with `trace=False`) - with
        `temperature=True` the pair `(records, temperature records)` of `step_n_trace_temperature`.  The engine's own
        params are unchanged; afterwards it is "per-world": `download_grid`, `get_obs`, `download_caches` and
        `reduce_temperature` raise until a shared-L step or an upload."""
        tab = self._world_table(worlds)
        Ls = np.ascontiguousarray(L, dtype=np.float64)
        if Ls.ndim != 2 or Ls.shape[1] != self.B:
            raise ValueError(f"per-world luminosities need shape (n, {self.B}), got {Ls.shape}")
        out = np.zeros(Ls.shape, dtype=_ffi.STATS_DTYPE) if trace else None
        temps = np.zeros(Ls.shape, dtype=_ffi.TEMP_STATS_DTYPE) if temperature else None
        self._check(self._lib.dw_step_n_trace_ensemble(
            self._h, int(Ls.shape[0]), tab.ctypes.data_as(C.POINTER(_ffi.DwWorldParams)), _ffi.ptr_d(Ls),
            out.ctypes.data_as(C.POINTER(DwWorldStats)) if trace else None,
            temps.ctypes.data_as(C.POINTER(DwTempStats)) if temperature else None))
        return (out, temps) if temperature else out

    def last_step_n_timing(self):
        """(ms spent in the fused step-pair launches of the last step_n call, their number, plane element bytes)."""
        ms, n, eb = C.c_float(0), C.c_int32(0), C.c_int32(0)
        self._check(self._lib.dw_last_step_n_timing(self._h, C.byref(ms), C.byref(n), C.byref(eb)))
        return ms.value, n.value, eb.value

    def update_agents(self, action):
        a = self._actions(action)
        self._check(self._lib.dw_update_agents(self._h, _ffi.ptr_i(a), a.shape[0], a.shape[1]))

    def upload_actions(self, action):
        a = self._actions(action)
        if a.shape != (self.B, self.N):
            raise ValueError(f"device action buffer needs shape {(self.B, self.N)}")
        self._check(self._lib.dw_upload_actions(self._h, _ffi.ptr_i(a)))

    def download_actions(self):
        a = np.empty((self.B, self.N), dtype=np.int32)
        self._check(self._lib.dw_download_actions(self._h, _ffi.ptr_i(a)))
        return a

    def forward(self, light, dark, L, want_caches=False):
        light, dark = self._plane(light, np.float64), self._plane(dark, np.float64)
        B, H, W = self.B, self.H, self.W
        grid = np.empty((B, 7, H, W))
        if want_caches:
            t, b, g, e = np.empty((B, 3, H, W)), np.empty((B, 3, H, W)), np.empty((B, 2, H, W)), np.empty((B, 1, H, W))
        else:
            t = b = g = e = None
        self._check(self._lib.dw_forward_f64(self._h, _ffi.ptr_d(light), _ffi.ptr_d(dark), float(L), _ffi.ptr_d(grid),
                                       _ffi.ptr_d(t), _ffi.ptr_d(b), _ffi.ptr_d(g), _ffi.ptr_d(e)))
        return (grid, t, b, g, e) if want_caches else grid

    def conv3x3(self, plane, kernel):
        """Toroidal 3x3 convolution of a (B,H,W) float64 plane on the device (ref ft_convolve)."""
        x = self._plane(plane, np.float64)
        k = np.ascontiguousarray(kernel, dtype=np.float64).reshape(9)
        out = np.empty_like(x)
        self._check(self._lib.dw_conv3x3_f64(self._h, _ffi.ptr_d(x), _ffi.ptr_d(k), _ffi.ptr_d(out)))
        return out

    def stage(self, stage, planes, L=0.0, kernel=None):
        """One stage of forward() on caller data, on the device (dw_stage_f64): `planes` = the stage's input
        planes, each (B,H,W); returns the list of its output planes."""
        n_in, n_out = _ffi.STAGE_IO[stage]
        if len(planes) != n_in:
            raise ValueError(f"stage {stage} takes {n_in} planes, got {len(planes)}")
        x = np.ascontiguousarray(np.stack([self._plane(a, np.float64) for a in planes]))
        out = np.empty((n_out, self.B, self.H, self.W))
        k = None if kernel is None else np.ascontiguousarray(kernel, dtype=np.float64).reshape(9)
        self._check(self._lib.dw_stage_f64(self._h, int(stage), _ffi.ptr_d(x), _ffi.ptr_d(out), float(L),
                                           _ffi.ptr_d(k) if k is not None else None))
        return list(out)

    def get_obs(self, L_init=0.75):
        obs = np.zeros((self.B, self.N, 7, 3, 3))
        if self.B * self.N:
            self._check(self._lib.dw_get_obs(self._h, float(L_init), _ffi.ptr_d(obs)))
        return obs

    def reward_done(self):
        reward = np.zeros((self.B, self.N, 1))
        done = np.zeros((self.B, self.N, 1), dtype=np.uint8)
        if self.B * self.N:
            self._check(self._lib.dw_get_reward_done(self._h, _ffi.ptr_d(reward), _ffi.ptr_u8(done)))
        return reward, done.astype(bool)

    def reduce(self):
        out = np.zeros(self.B, dtype=_ffi.STATS_DTYPE)
        self._check(self._lib.dw_reduce(self._h, out.ctypes.data_as(C.POINTER(DwWorldStats))))
        return out

    def reduce_temperature(self, L):
        """(B,) records of dtype `_ffi.TEMP_STATS_DTYPE`: mean, population std, min and max of the local temperature field
        `download_caches(L)` would return as `temps[:, 0]` - reduced on the device (`dw_reduce_temperature`), nothing but
        the 32 bytes per world comes down.  `L` is used as `download_caches` uses it."""
        out = np.zeros(self.B, dtype=_ffi.TEMP_STATS_DTYPE)
        self._check(self._lib.dw_reduce_temperature(self._h, float(L), out.ctypes.data_as(C.POINTER(DwTempStats))))
        return out

    # -- spatial frames -----------------------------------------------------------------------
    def _frame_spec(self, tile, worlds):
        """(`DwFrameSpec`, the array its list points into, (S, TH, TW)) for `tile` (an int or (tile_h, tile_w)) and
        `worlds` (None: all B in order).  What the library refuses (a tile that does not divide the grid, a world listed
        twice ...) is left to the library: the shape is then only a placeholder."""
        th, tw = (int(tile), int(tile)) if np.isscalar(tile) else (int(tile[0]), int(tile[1]))
        sel = None if worlds is None else np.ascontiguousarray(worlds, dtype=np.int32).reshape(-1)
        if sel is not None and sel.size == 0:
            raise ValueError("an empty selection of worlds: pass worlds=None for all of them")
        spec = _ffi.DwFrameSpec(th, tw, 0 if sel is None else int(sel.size),
                                None if sel is None else sel.ctypes.data_as(C.POINTER(C.c_int32)))
        S = self.B if sel is None else int(sel.size)
        return spec, sel, (S, max(self.H // th, 1) if th > 0 else 1, max(self.W // tw, 1) if tw > 0 else 1)

    def reduce_tiles(self, L, tile=(1, 1), worlds=None, cover=True, temperature=True):
        """One frame of the engine's state (`dw_reduce_tiles`): per tile of `tile` = (tile_h, tile_w) cells of each world in
        `worlds` (None: all), `cover` - records of dtype `_ffi.TILE_COVER_DTYPE`, the exact per-mille sums of light and dark
        cover of the CURRENT state - and `temperature` - the float64 mean in kelvin of the field `download_caches(L)` returns
        as `temps[:, 0]` (after a step: what the reference's `env.temp` holds).  Returns `(cover, temp)`, arrays of shape
        (S, H // tile_h, W // tile_w), None for what was not asked for.  At 1 x 1 tiles these are the planes and the field
        themselves, cell for cell and bit for bit."""
        spec, sel, shape = self._frame_spec(tile, worlds)
        cov = np.zeros(shape, dtype=_ffi.TILE_COVER_DTYPE) if cover else None
        tmp = np.zeros(shape, dtype=np.float64) if temperature else None
        self._check(self._lib.dw_reduce_tiles(
            self._h, float(L), C.byref(spec), cov.ctypes.data_as(C.POINTER(_ffi.DwTileCover)) if cover else None,
            _ffi.ptr_d(tmp) if temperature else None))
        return cov, tmp

    def step_n_frames(self, L_schedule, stride=1, tile=(1, 1), worlds=None, cover=True, temperature=True, trace=True):
        """`step_n_trace` with frames (`dw_step_n_frames`): `len(L_schedule)` agent-free steps, and at every `stride`-th
        step a frame as `reduce_tiles` describes it - `cover` of the state after that step, `temperature` of the field that
        step computes (the reference's `env.temp` after it).  Returns `(cover, temp, stats)`: (F, S, TH, TW) arrays with
        F = n // stride (None for what was not asked for) and the (n, B) records of `step_n_trace` (None with
        `trace=False`).  The state afterwards is that of `step_n_trace`, bit for bit."""
        Ls = np.ascontiguousarray(L_schedule, dtype=np.float64).reshape(-1)
        spec, sel, shape = self._frame_spec(tile, worlds)
        stride = int(stride)
        F = Ls.size // stride if stride >= 1 else 0
        cov = np.zeros((F, *shape), dtype=_ffi.TILE_COVER_DTYPE) if cover else None
        tmp = np.zeros((F, *shape), dtype=np.float64) if temperature else None
        out = np.zeros((Ls.size, self.B), dtype=_ffi.STATS_DTYPE) if trace else None
        self._check(self._lib.dw_step_n_frames(
            self._h, int(Ls.size), _ffi.ptr_d(Ls), C.byref(spec), stride,
            cov.ctypes.data_as(C.POINTER(_ffi.DwTileCover)) if cover else None, _ffi.ptr_d(tmp) if temperature else None,
            out.ctypes.data_as(C.POINTER(DwWorldStats)) if trace else None))
        return cov, tmp, out

    def policy_greedy(self, argmin=False):
        self._check(self._lib.dw_policy_greedy(self._h, _ffi.POLICY_ARGMIN if argmin else _ffi.POLICY_ARGMAX))

    def policy_per_agent(self, agent_mode):
        """agent_mode (N,) of POLICY_ARGMAX / POLICY_ARGMIN / POLICY_TABLE (keep the uploaded action)."""
        m = np.ascontiguousarray(agent_mode, dtype=np.int32)
        if m.shape != (self.N,):
            raise ValueError(f"agent_mode must have shape {(self.N,)}")
        self._check(self._lib.dw_policy_per_agent(self._h, _ffi.ptr_i(m)))

    def policy_mlp(self, params, agent_begin=0, agent_end=None, L_init=0.75):
        w = np.ascontiguousarray(params, dtype=np.float64).ravel()
        end = self.N if agent_end is None else int(agent_end)
        self._check(self._lib.dw_policy_mlp(self._h, _ffi.ptr_d(w), int(w.size), int(agent_begin), end, float(L_init)))

    def policy_mlp_population(self, params, world_member, agent_begin=0, agent_end=None, L_init=0.75):
        """params (P,1808); world_member (B,) int: which parameter set each world's agents use."""
        w = np.ascontiguousarray(params, dtype=np.float64)
        if w.ndim != 2 or w.shape[1] != 1808:
            raise ValueError("params must have shape (n_members, 1808)")
        m = np.ascontiguousarray(world_member, dtype=np.int32)
        if m.shape != (self.B,):
            raise ValueError(f"world_member must have shape {(self.B,)}")
        end = self.N if agent_end is None else int(agent_end)
        self._check(self._lib.dw_policy_mlp_population(self._h, _ffi.ptr_d(w), int(w.shape[0]), _ffi.ptr_i(m),
                                                 int(agent_begin), end, float(L_init)))

    def lifespan_reset(self):
        self._check(self._lib.dw_lifespan_reset(self._h))

    def lifespan_accumulate(self, threshold_k=5):
        self._check(self._lib.dw_lifespan_accumulate(self._h, int(threshold_k)))

    def lifespan_download(self):
        done_at = np.zeros(self.B, dtype=np.int32)
        agents = np.zeros((self.B, self.N, 1), dtype=np.int32)
        alive = C.c_int32(0)
        self._check(self._lib.dw_lifespan_download(self._h, _ffi.ptr_i(done_at), _ffi.ptr_i(agents) if self.N else None,
                                             C.byref(alive)))
        return done_at, agents, alive.value

    def snapshot_save(self, slot=0):
        """Device-side copy of the current state (planes, the retained previous state, agents, reductions) into one of
        the two slots."""
        self._check(self._lib.dw_snapshot_save_slot(self._h, int(slot)))

    def snapshot_restore(self, slot=0):
        self._check(self._lib.dw_snapshot_restore_slot(self._h, int(slot)))

    def run_episode(self, L_schedule, policy_mode, use_table=None, table=None, threshold_k=5, world_flags=True,
                    reuse_buffers=False):
        """K device-resident steps (one launch for H*W <= 4096, back-to-back launches otherwise).
        Returns (world_alive (K,B) bool, agent_ok (K,B,N) bool).  `table` entries: 0..8 an action, -1 / -2 the
        greedy / anti-greedy choice of that agent at that step.  world_flags=False: the per-step world
        reductions are not needed (world_alive is returned as None), which lets wide grids run step PAIRS in
        one fused launch with the agents' in-between step patched in (dw_agents_fused.hpp)."""
        Ls = np.ascontiguousarray(L_schedule, dtype=np.float64)
        K = Ls.shape[0]
        ut = None if use_table is None else np.ascontiguousarray(use_table, dtype=np.uint8)
        tb = None if table is None else np.ascontiguousarray(table, dtype=np.int8)
        if ut is not None and ut.shape != (K,):
            raise ValueError("use_table must have shape (K,)")
        if tb is not None and tb.shape != (K, self.B, self.N):
            raise ValueError(f"table must have shape {(K, self.B, self.N)}")
        # (the library writes every flag as 0 / 1: the uint8 arrays are returned as bool VIEWS, no second pass)
        # reuse_buffers=True: the flag arrays are this engine's own and are OVERWRITTEN by the next such call (a fresh
        # 256 KB array per chunk is a fresh mmap: ~60 page faults while the library copies into it) - for loops that
        # consume a chunk's flags before they run the next chunk
        if reuse_buffers:
            cache = self.__dict__.setdefault("_flag_buffers", {})
            key = (K, bool(world_flags))
            if key not in cache:
                cache.clear()
                cache[key] = (np.empty((K, self.B), dtype=np.uint8) if world_flags else None,
                              np.empty((K, self.B, self.N), dtype=np.uint8))
            alive, ok = cache[key]
        else:
            alive = np.empty((K, self.B), dtype=np.uint8) if world_flags else None
            ok = np.empty((K, self.B, self.N), dtype=np.uint8)
        self._check(self._lib.dw_run_episode(
            self._h, K, _ffi.ptr_d(Ls), int(policy_mode), _ffi.ptr_u8(ut),
            None if tb is None else tb.ctypes.data_as(C.POINTER(C.c_int8)), int(threshold_k), _ffi.ptr_u8(alive),
            _ffi.ptr_u8(ok) if self.N else None))
        return (None if alive is None else alive.view(np.bool_)), ok.view(np.bool_)

    def run_episode_trace(self, L_schedule, policy_mode, use_table=None, table=None, threshold_k=5, temperature=False):
        """`run_episode` that also records what `reduce()` would return after every step (`dw_run_episode_trace`): the
        daisy populations of an ensemble with grazing agents, in one device-resident run.  Returns (stats (K,B) of dtype
        `_ffi.STATS_DTYPE` with `reserved` 0, world_alive (K,B) bool, agent_ok (K,B,N) bool); flags, state and agents are
        `run_episode`'s for the same arguments, `world_alive == (stats["max_k"] > threshold_k)`, and the last row is
        `reduce()` after the call.

        `temperature=True` (`dw_run_episode_trace_temperature`): returns (stats, world_alive, agent_ok, temps), `temps`
        (K, B) records of dtype `_ffi.TEMP_STATS_DTYPE` - mean, population std, min and max of the local temperature
        field step t computes, from the state after its grazing and before its growth (the reference's `env.temp` after
        the t-th `env.step(action)`), float64 in every precision.  Everything else is unchanged, and the last row is
        `reduce_temperature(L_schedule[-1])` after the call, bit for bit."""
        Ls = np.ascontiguousarray(L_schedule, dtype=np.float64)
        K = Ls.shape[0]
        ut = None if use_table is None else np.ascontiguousarray(use_table, dtype=np.uint8)
        tb = None if table is None else np.ascontiguousarray(table, dtype=np.int8)
        if ut is not None and ut.shape != (K,):
            raise ValueError("use_table must have shape (K,)")
        if tb is not None and tb.shape != (K, self.B, self.N):
            raise ValueError(f"table must have shape {(K, self.B, self.N)}")
        stats = np.zeros((K, self.B), dtype=_ffi.STATS_DTYPE)
        alive = np.empty((K, self.B), dtype=np.uint8)
        ok = np.empty((K, self.B, self.N), dtype=np.uint8)
        if temperature:
            temps = np.zeros((K, self.B), dtype=_ffi.TEMP_STATS_DTYPE)
            self._check(self._lib.dw_run_episode_trace_temperature(
                self._h, K, _ffi.ptr_d(Ls), int(policy_mode), _ffi.ptr_u8(ut),
                None if tb is None else tb.ctypes.data_as(C.POINTER(C.c_int8)), int(threshold_k), _ffi.ptr_u8(alive),
                _ffi.ptr_u8(ok) if self.N else None, stats.ctypes.data_as(C.POINTER(DwWorldStats)),
                temps.ctypes.data_as(C.POINTER(DwTempStats))))
            return stats, alive.view(np.bool_), ok.view(np.bool_), temps
        self._check(self._lib.dw_run_episode_trace(
            self._h, K, _ffi.ptr_d(Ls), int(policy_mode), _ffi.ptr_u8(ut),
            None if tb is None else tb.ctypes.data_as(C.POINTER(C.c_int8)), int(threshold_k), _ffi.ptr_u8(alive),
            _ffi.ptr_u8(ok) if self.N else None, stats.ctypes.data_as(C.POINTER(DwWorldStats))))
        return stats, alive.view(np.bool_), ok.view(np.bool_)

    def run_episode_frames(self, L_schedule, policy_mode, use_table=None, table=None, threshold_k=5, stride=1, tile=(1, 1),
                           worlds=None, cover=True, temperature=True, agents=True, trace=True, temps=False):
        """`run_episode_trace` with pictures (`dw_run_episode_frames`): the K device-resident steps of an ensemble with
        grazing agents that also leave, at every `stride`-th step, a frame of the worlds in `worlds` (None: all) - `cover`
        and `temperature` as `reduce_tiles` returns them after that step (tiles of `tile` cells), `agents` as
        `download_agents` returns them after it, as records of dtype `_ffi.AGENT_FRAME_DTYPE` (`row`, `col`, `state`).
        Returns `(cover, temp, agents, ...)` - (F, S, TH, TW), (F, S, TH, TW) and (F, S, N) arrays with F = K // stride, None
        for what was not asked for - followed by `run_episode_trace`'s tuple `(stats, world_alive, agent_ok)` (`stats` None
        with `trace=False`), with `temps=True` that of `run_episode_trace(..., temperature=True)`.  State, flags and records
        are those calls', bit for bit."""
        Ls = np.ascontiguousarray(L_schedule, dtype=np.float64)
        K = Ls.shape[0]
        ut = None if use_table is None else np.ascontiguousarray(use_table, dtype=np.uint8)
        tb = None if table is None else np.ascontiguousarray(table, dtype=np.int8)
        if ut is not None and ut.shape != (K,):
            raise ValueError("use_table must have shape (K,)")
        if tb is not None and tb.shape != (K, self.B, self.N):
            raise ValueError(f"table must have shape {(K, self.B, self.N)}")
        spec, sel, shape = self._frame_spec(tile, worlds)
        stride = int(stride)
        F = K // stride if stride >= 1 else 0
        cov = np.zeros((F, *shape), dtype=_ffi.TILE_COVER_DTYPE) if cover else None
        tmp = np.zeros((F, *shape), dtype=np.float64) if temperature else None
        ag = np.zeros((F, shape[0], self.N), dtype=_ffi.AGENT_FRAME_DTYPE) if agents else None
        stats = np.zeros((K, self.B), dtype=_ffi.STATS_DTYPE) if trace else None
        trows = np.zeros((K, self.B), dtype=_ffi.TEMP_STATS_DTYPE) if temps else None
        alive = np.empty((K, self.B), dtype=np.uint8)
        ok = np.empty((K, self.B, self.N), dtype=np.uint8)
        self._check(self._lib.dw_run_episode_frames(
            self._h, K, _ffi.ptr_d(Ls), int(policy_mode), _ffi.ptr_u8(ut),
            None if tb is None else tb.ctypes.data_as(C.POINTER(C.c_int8)), int(threshold_k), _ffi.ptr_u8(alive),
            _ffi.ptr_u8(ok) if self.N else None, stats.ctypes.data_as(C.POINTER(DwWorldStats)) if trace else None,
            trows.ctypes.data_as(C.POINTER(DwTempStats)) if temps else None, C.byref(spec), stride,
            cov.ctypes.data_as(C.POINTER(_ffi.DwTileCover)) if cover else None, _ffi.ptr_d(tmp) if temperature else None,
            ag.ctypes.data_as(C.POINTER(_ffi.DwAgentFrame)) if agents else None))
        out = (cov, tmp, ag, stats, alive.view(np.bool_), ok.view(np.bool_))
        return out + (trows,) if temps else out

    def run_episode_ensemble(self, worlds, Ls, mode, use_table=None, table=None, threshold_k=5, trace=False,
                             temperature=False):
        """`run_episode` with the physics constants `worlds[b]` (as `step_n_trace_ensemble` takes them) and the luminosity
        column `Ls[:, b]` of world b (`dw_run_episode_ensemble`): `Ls` is (K, B).  Each world ends, and reports the flags,
        exactly as a one-world engine with those constants, that column and slice `[:, b]` of the table would after
        `run_episode`.  Returns (world_alive (K,B) bool, agent_ok (K,B,N) bool).  The engine's own params are unchanged;
        afterwards it is "per-world" as after `step_n_trace_ensemble`: `download_grid`, `get_obs`, `download_caches` and
        `reduce_temperature` raise until a shared-L step or an upload.

        `trace=True` and / or `temperature=True` (`dw_run_episode_ensemble_trace`): returns (world_alive, agent_ok, stats,
        temps) - `stats` (K, B) of dtype `_ffi.STATS_DTYPE`, the records `run_episode_trace` writes on that one-world
        engine, `temps` (K, B) of dtype `_ffi.TEMP_STATS_DTYPE`, its temperature rows (world b at `worlds[b]` and
        `Ls[t, b]`); the one not asked for is None and costs nothing.  Flags, state and agents are unchanged by either."""
        tab = self._world_table(worlds)
        L = np.ascontiguousarray(Ls, dtype=np.float64)
        if L.ndim != 2 or L.shape[1] != self.B:
            raise ValueError(f"per-world luminosities need shape (K, {self.B}), got {L.shape}")
        K = L.shape[0]
        ut = None if use_table is None else np.ascontiguousarray(use_table, dtype=np.uint8)
        tb = None if table is None else np.ascontiguousarray(table, dtype=np.int8)
        if ut is not None and ut.shape != (K,):
            raise ValueError("use_table must have shape (K,)")
        if tb is not None and tb.shape != (K, self.B, self.N):
            raise ValueError(f"table must have shape {(K, self.B, self.N)}")
        alive = np.empty((K, self.B), dtype=np.uint8)
        ok = np.empty((K, self.B, self.N), dtype=np.uint8)
        if trace or temperature:
            stats = np.zeros((K, self.B), dtype=_ffi.STATS_DTYPE) if trace else None
            temps = np.zeros((K, self.B), dtype=_ffi.TEMP_STATS_DTYPE) if temperature else None
            self._check(self._lib.dw_run_episode_ensemble_trace(
                self._h, K, tab.ctypes.data_as(C.POINTER(_ffi.DwWorldParams)), _ffi.ptr_d(L), int(mode), _ffi.ptr_u8(ut),
                None if tb is None else tb.ctypes.data_as(C.POINTER(C.c_int8)), int(threshold_k), _ffi.ptr_u8(alive),
                _ffi.ptr_u8(ok) if self.N else None,
                None if stats is None else stats.ctypes.data_as(C.POINTER(DwWorldStats)),
                None if temps is None else temps.ctypes.data_as(C.POINTER(DwTempStats))))
            return alive.view(np.bool_), ok.view(np.bool_), stats, temps
        self._check(self._lib.dw_run_episode_ensemble(
            self._h, K, tab.ctypes.data_as(C.POINTER(_ffi.DwWorldParams)), _ffi.ptr_d(L), int(mode), _ffi.ptr_u8(ut),
            None if tb is None else tb.ctypes.data_as(C.POINTER(C.c_int8)), int(threshold_k), _ffi.ptr_u8(alive),
            _ffi.ptr_u8(ok) if self.N else None))
        return alive.view(np.bool_), ok.view(np.bool_)

    def run_episode_mlp(self, L_schedule, params, member_a=None, member_b=None, split=None, L_init=0.75,
                        reuse_buffers=False, n_members=None, trace=False, temperature=False):
        """K device-resident steps with MLP policies: agents [0, split) of world b use parameter set
        member_a[b], agents [split, N) member_b[b].  Returns (reward (K,B,N,1) float64, done (K,B,N,1) bool)
        exactly as K calls of env.step would (ref step :486-492).

        `params=None`: the parameter sets of the last call that passed them are still on the device and are used again
        (pass `n_members`).  `reuse_buffers=True`: the returned arrays are views of page-locked buffers owned by this
        engine (no staging copy on the way back) and are OVERWRITTEN by the next call with reuse_buffers=True - for
        harnesses that consume a chunk's rewards before they run the next one.  `reuse_buffers=1` selects a SECOND such
        buffer (True is buffer 0): a harness that runs chunk c + 1 while it still reads chunk c's rewards alternates.

        `trace=True` and / or `temperature=True` (`dw_run_episode_mlp_trace`): returns (reward, done, stats, temps) -
        `stats` (K, B) of dtype `_ffi.STATS_DTYPE`, what `reduce()` would return after every step (`reserved` 0), `temps`
        (K, B) of dtype `_ffi.TEMP_STATS_DTYPE`, the statistics of the temperature field step t computes (after its grazing,
        before its growth, at `L_schedule[t]`; float64 in every precision); the one not asked for is None and costs nothing.
        Rewards, done flags, state and agents are unchanged by either."""
        Ls = np.ascontiguousarray(L_schedule, dtype=np.float64)
        K = Ls.shape[0]
        w, nm, ma, mb, split = _mlp_episode_args(self.B, self.N, params, n_members, member_a, member_b, split)
        n = K * self.B * self.N
        if reuse_buffers is not False and reuse_buffers is not None and n:
            buf = self._pinned_block(9 * n, 0 if reuse_buffers is True else int(reuse_buffers))
            reward = np.frombuffer(buf, dtype=np.float64, count=n).reshape(K, self.B, self.N, 1)
            done = np.frombuffer(buf, dtype=np.uint8, count=n, offset=8 * n).reshape(K, self.B, self.N, 1)
        else:
            reward = np.empty((K, self.B, self.N, 1))              # (every element is written by the library; done: 0 / 1)
            done = np.empty((K, self.B, self.N, 1), dtype=np.uint8)
        if trace or temperature:
            stats = np.zeros((K, self.B), dtype=_ffi.STATS_DTYPE) if trace else None
            temps = np.zeros((K, self.B), dtype=_ffi.TEMP_STATS_DTYPE) if temperature else None
            self._check(self._lib.dw_run_episode_mlp_trace(
                self._h, K, _ffi.ptr_d(Ls), _ffi.ptr_d(w), nm, _ffi.ptr_i(ma), _ffi.ptr_i(mb), split, float(L_init),
                _ffi.ptr_d(reward), _ffi.ptr_u8(done),
                None if stats is None else stats.ctypes.data_as(C.POINTER(DwWorldStats)),
                None if temps is None else temps.ctypes.data_as(C.POINTER(DwTempStats))))
            return reward, done.view(np.bool_), stats, temps
        self._check(self._lib.dw_run_episode_mlp(self._h, K, _ffi.ptr_d(Ls), _ffi.ptr_d(w), nm, _ffi.ptr_i(ma),
                                           _ffi.ptr_i(mb), split, float(L_init), _ffi.ptr_d(reward), _ffi.ptr_u8(done)))
        return reward, done.view(np.bool_)

    def run_episode_mlp_counts(self, L_schedule, params, n_active, member_a=None, member_b=None, split=None, L_init=0.75,
                               n_members=None, trace=True):
        """`run_episode_mlp(..., trace=True)` with a number of agents per world (`dw_run_episode_mlp_counts`): in world b
        only agents [0, n_active[b]) exist - the others are neither observed nor stamped into channel 4, their state is set
        to 0, their reward is 0, their done flag True and their action 0.  Returns (reward (K,B,N,1) float64, done (K,B,N,1)
        bool, stats (K,B) of dtype `_ffi.STATS_DTYPE` or None without `trace`).  For world b the call leaves what an engine
        of one world with n_active[b] agents holds after the same steps, bit for bit.  The counts belong to this call, not
        to the engine: afterwards the absent agents are N - n_active[b] agents of state 0."""
        Ls = np.ascontiguousarray(L_schedule, dtype=np.float64)
        K = Ls.shape[0]
        w, nm, ma, mb, split = _mlp_episode_args(self.B, self.N, params, n_members, member_a, member_b, split)
        na = None if n_active is None else np.ascontiguousarray(n_active, dtype=np.int32)
        if na is not None and na.shape != (self.B,):
            raise ValueError(f"n_active must have shape {(self.B,)}")
        reward = np.empty((K, self.B, self.N, 1))
        done = np.empty((K, self.B, self.N, 1), dtype=np.uint8)
        stats = np.zeros((K, self.B), dtype=_ffi.STATS_DTYPE) if trace else None
        self._check(self._lib.dw_run_episode_mlp_counts(
            self._h, K, _ffi.ptr_d(Ls), _ffi.ptr_d(w), nm, _ffi.ptr_i(ma), _ffi.ptr_i(mb), split, _ffi.ptr_i(na),
            float(L_init), _ffi.ptr_d(reward), _ffi.ptr_u8(done),
            None if stats is None else stats.ctypes.data_as(C.POINTER(DwWorldStats))))
        return reward, done.view(np.bool_), stats

    # -- the fitness bookkeeping of an ES population on the device (ref daisy/evo/sges.py:160-176) --------------------
    def fitness_begin(self, worlds_per_member, half):
        """Zero the device-resident accumulators of a population's fitness episodes - `sum_reward` (P,), `done_at`
        (B, N), `running` (P,) all True - for P = B // worlds_per_member members, member m owning worlds
        [m * worlds_per_member, (m + 1) * worlds_per_member); `half`: the agents [0, half) of a world whose rewards count."""
        self._check(self._lib.dw_fitness_begin(self._h, int(worlds_per_member), int(half)))
        self._fitness_members = self.B // int(worlds_per_member)

    def fitness_account(self, rewards, dones):
        """Account a chunk of host arrays - rewards (K, B, N[, 1]) float64 (`reward * (reward > 0)`), dones the same shape,
        bool - exactly as `harness._population_chunk` does; returns its `(executed, finished)`."""
        r = np.ascontiguousarray(rewards, dtype=np.float64)
        K = r.shape[0] if r.ndim else 0
        d = np.ascontiguousarray(dones).astype(np.uint8, copy=False)
        if r.size != K * self.B * self.N or d.size != r.size:
            raise ValueError(f"rewards and dones must have shape {(K, self.B, self.N)} (a trailing axis of 1 is allowed)")
        executed, finished = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.dw_fitness_account(self._h, K, _ffi.ptr_d(r), _ffi.ptr_u8(d), C.byref(executed),
                                                 C.byref(finished)))
        return executed.value, bool(finished.value)

    def run_episode_mlp_fitness(self, L_schedule, params, member_a=None, member_b=None, split=None, L_init=0.75,
                                n_members=None):
        """`run_episode_mlp` whose rewards and done flags stay on the device and are accounted there
        (`dw_run_episode_mlp_fitness`): state, agents, actions and the resident parameter sets are left as `run_episode_mlp`
        leaves them; returns `(executed, finished)` of the chunk - the only bytes that come down."""
        Ls = np.ascontiguousarray(L_schedule, dtype=np.float64)
        w, nm, ma, mb, split = _mlp_episode_args(self.B, self.N, params, n_members, member_a, member_b, split)
        executed, finished = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.dw_run_episode_mlp_fitness(self._h, Ls.shape[0], _ffi.ptr_d(Ls), _ffi.ptr_d(w), nm, _ffi.ptr_i(ma),
                                                         _ffi.ptr_i(mb), split, float(L_init), C.byref(executed),
                                                         C.byref(finished)))
        return executed.value, bool(finished.value)

    def fitness_download(self):
        """`(sum_reward (P,) float64, done_at (B, N, 1) int32, running (P,) bool)` as they stand on the device."""
        P = getattr(self, "_fitness_members", 0)
        if not P:                                                # (the library says so itself: DW_ESTATE)
            self._check(self._lib.dw_fitness_download(self._h, None, None, None))
        sum_reward = np.zeros(P)
        done_at = np.zeros((self.B, self.N, 1), dtype=np.int32)
        running = np.zeros(P, dtype=np.uint8)
        self._check(self._lib.dw_fitness_download(self._h, _ffi.ptr_d(sum_reward), _ffi.ptr_i(done_at), _ffi.ptr_u8(running)))
        return sum_reward, done_at, running.view(np.bool_)

    def _pinned_block(self, nbytes, index=0):
        """Page-locked host buffer number `index` of at least nbytes owned by this engine (grown geometrically, freed by
        close())."""
        blocks = self.__dict__.setdefault("_pinned", {})
        have = blocks.get(index)
        if have is None or have[1] < nbytes:
            if have is not None:
                self._lib.dw_pinned_free(have[0])
                del blocks[index]
            size = max(int(nbytes), 2 * (have[1] if have else 0), 1 << 20)
            ptr = C.c_void_p()
            self._check(self._lib.dw_pinned_alloc(size, C.byref(ptr)))
            blocks[index] = (ptr, size, (C.c_ubyte * size).from_address(ptr.value))
        return blocks[index][2]

    # -- plumbing -----------------------------------------------------------------------------
    def set_stream(self, hip_stream_ptr: int):
        self._check(self._lib.dw_set_stream(self._h, C.c_void_p(hip_stream_ptr)))

    def sync(self):
        self._check(self._lib.dw_sync(self._h))

    def timer_start(self):
        self._check(self._lib.dw_timer_start(self._h))

    def timer_stop(self) -> float:
        ms = C.c_float(0)
        self._check(self._lib.dw_timer_stop(self._h, C.byref(ms)))
        return ms.value

    def device_planes(self, which=_ffi.STATE_CURRENT):
        lp, dp = C.c_void_p(), C.c_void_p()
        self._check(self._lib.dw_device_planes(self._h, which, C.byref(lp), C.byref(dp)))
        return lp.value, dp.value

    def kernel_info(self) -> str:
        buf = C.create_string_buffer(1024)
        self._check(self._lib.dw_kernel_info(self._h, buf, 1024))
        return buf.value.decode()

    def audit_tie_bound(self, L):
        """(max |gq32-gq64| in quanta, max error/bound, flagged cell-values, audited cell-values)."""
        out = np.zeros(4)
        self._check(self._lib.dw_audit_tie_bound(self._h, float(L), _ffi.ptr_d(out)))
        return float(out[0]), float(out[1]), int(out[2]), int(out[3])

    def last_fixup_count(self) -> int:
        v = C.c_uint64(0)
        self._check(self._lib.dw_last_fixup_count(self._h, C.byref(v)))
        return int(v.value)
