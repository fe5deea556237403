"""Episode harnesses on top of the drop-in environment.

``simulate_lifespan(env, agent)`` is the reference's lifespan harness
(``notebooks/greedy_longevity_abatement.ipynb`` cell 2:28-57): run an episode until every world's
biosphere is dead and return, per world, the number of steps it was alive and, per agent, the number of
steps its reward stayed >= 0.1.  Results and legacy-NumPy-RNG consumption are identical to running the
notebook's loop on the reference.

For scripted policies (``Greedy`` in any of its modes, or no agent) the loop does not call ``env.step`` per
step: whole chunks of steps run device-resident (``dw_run_episode``: policy, grazing, physics and the
per-step alive flags — one launch with the worlds in LDS for H*W <= 4096, back-to-back launches without
host round trips for larger worlds); the host only draws the policy's random numbers for the chunk in the
reference's order and post-processes the flags.  If the episode ends inside a chunk the chunk is replayed
from a device-side snapshot (``dw_snapshot_save/restore``) for exactly the remaining steps, so the
environment is left in the very state (grid, agents, L, step_count, RNG stream) the reference loop would
leave it in.
"""
from __future__ import annotations

import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _ffi
from .agents.greedy import Greedy

LIFESPAN_THRESHOLD_K = 5          # grid_done = max cover <= 0.005 (notebook cell 2:48)


def _count_true(flags):
    """Number of set flags along axis 0 of a (K, ...) array of 0 / 1 bytes (bool or uint8), as intp - `flags.sum(axis=0)`.
    Eight flags at a time: the bytes are summed as uint64 words (no byte can carry for K <= 255), 8x less work than
    NumPy's bool -> int64 reduction (137 -> 17 us for 32 x 1000 x 4 flags: a third of a chunk's host time on 8x8 worlds)."""
    K, rest = flags.shape[0], flags.shape[1:]
    n = int(np.prod(rest, dtype=np.int64))
    if 0 < K <= 255 and n and n % 8 == 0 and flags.flags.c_contiguous and flags.dtype.itemsize == 1:
        words = flags.view(np.uint8).reshape(K, n).view(np.uint64).sum(axis=0)
        return words.view(np.uint8).reshape(rest).astype(np.intp)
    return np.count_nonzero(flags, axis=0)


def _grid_done(env):
    """ref notebook cell 2:48: `env.grid[:, 1:3].max(axis=(1, 2, 3)) <= 0.005` per world.  On the drop-in
    environment the per-world maximum is a by-product of the step kernel (per-mille integer, `dw_reduce`):
    k <= 5 is the same predicate without materialising and downloading the 7-channel float64 grid
    (3.7 GB per step for 1000 worlds of 256x256)."""
    from .daisy_world_rl import RLDaisyWorld
    if isinstance(env, RLDaisyWorld) and (env._grid_m is None or not env._grid_m.dirty()):
        return env._engine.reduce()["max_k"] <= LIFESPAN_THRESHOLD_K
    return env.grid[:, 1:3, :, :].max(axis=(1, 2, 3)) <= 0.005


def _simulate_on_host(env, agent, obs, done_at, agents_done_at):
    """The notebook's loop (any environment / any callable agent), one `env.step` per step."""
    while True:
        action = agent(obs) if agent is not None else None
        obs, reward, done, info = env.step(action)
        grid_done = _grid_done(env)
        done_at += (1 - 1 * grid_done)
        agents_done_at += (1 - 1 * done)
        if grid_done.mean() == 1.0:
            return done_at, agents_done_at


def _policy_mode(agent):
    if agent is None:
        return _ffi.POLICY_ZEROS                      # ref step(None): action 0 for every agent
    if type(agent) is Greedy:
        return _ffi.POLICY_ARGMAX if agent.greedy else _ffi.POLICY_ARGMIN
    return None


def _luminosity_schedule(env, nsteps):
    """L of the next `nsteps` steps, WITHOUT touching env (ref update_L :463-473 replayed on copies)."""
    L, dL, sc, mn, mx = env.L, env.dL, env.step_count, env.min_L, env.max_L
    out = []
    for _ in range(nsteps):
        out.append(L)
        sc += 1
        if env.ramp_up_down and sc % env.ramp_period == 0:
            dL *= -1
            mn -= env.ddL
            mx += env.ddL
        L += dL
        L = max([min([L, mx]), mn])
    return out


def simulate_lifespan(env, agent, chunk=32, use_device_loop=True, obs=None, final_state=True):
    """`obs=None`: reset the environment first, as the notebook's harness does.  Pass the observations of
    a reset the caller has already done (e.g. `env.reset_synthetic(seed); obs = env.get_obs()` — the
    device-side initial state for ensembles too large to draw from the host's legacy RNG).

    `final_state=False`: the caller wants the lifespans only (a sweep that discards the environment).  The chunk in
    which the last biosphere dies is then NOT replayed from a snapshot for exactly the remaining steps, and no
    snapshots are taken: the lifespans are the same numbers, but the environment (grid, agents, L, step_count, and the
    legacy-RNG stream when the policy draws) is left at the END of that chunk, up to `chunk - 1` steps past the point
    the reference loop stops at."""
    if obs is None:
        obs = env.reset()
    B, N = obs.shape[0], obs.shape[1]
    done_at = np.zeros((B,), dtype=int)
    agents_done_at = np.zeros((B, N, 1), dtype=int)
    mode = _policy_mode(agent)
    supported = env.precision != "f64" and env.collision_mode == 0
    if not (use_device_loop and supported and mode is not None):
        return _simulate_on_host(env, agent, obs, done_at, agents_done_at)

    eng = env._engine
    # step 1 through the ordinary path: the initial state is not quantised (ref initialize_grid)
    action = agent(obs) if agent is not None else None
    obs, reward, done, _ = env.step(action)
    alive = eng.reduce()["max_k"] > LIFESPAN_THRESHOLD_K
    done_at += alive
    agents_done_at += (1 - 1 * done)
    if not alive.any():
        return done_at, agents_done_at

    K = int(chunk)

    host = _ffi.load_host() if type(agent) is Greedy else None

    def draws_in_c(state, steps, use_table, table):
        """`steps` calls' worth of the policy's draws (one coin per call, randint(9) for the batch on the random branch) from
        the legacy state `state` by the host helper (include/daisyworld_host.h: the same numbers, 4x faster than two NumPy
        calls per step); the advanced state goes back to NumPy.  False: not available, nothing consumed."""
        if host is None or state[0] != "MT19937":
            return False
        key = np.array(state[1], dtype=np.uint32)
        pos = C.c_int32(int(state[2]))
        rc = host.dw_mt19937_greedy_draws(key.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(pos), float(agent.epsilon), int(steps),
                                          B * N, None if use_table is None else use_table.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          None if table is None else table.ctypes.data_as(C.POINTER(C.c_int8)))
        if rc != 0:
            return False
        np.random.set_state((state[0], key, pos.value, state[3], state[4]))
        return True

    def draw_chunk():
        """The policy's draws for K steps, in the reference's order, and the generator's state before them (a 2.5 KB
        copy, 34 us: once per chunk - one per step was 16 ms of an 88 ms sweep of 1000 worlds of 256 x 256)."""
        rng_before = np.random.get_state() if agent is not None else None
        use_table = np.zeros(K, dtype=np.uint8)
        table = np.zeros((K, B, N), dtype=np.int8)
        # (a policy that never takes its random branch draws one coin per step: K scalar draws are cheaper than the state
        # exchange with the helper)
        if agent is not None and not (agent.epsilon > 0.0 and draws_in_c(rng_before, K, use_table, table)):
            for t in range(K):
                if not agent.draw_branch():
                    use_table[t] = 1
                    table[t] = agent.draw_random_actions(B, N)[..., 0]
        return rng_before, use_table, table

    def rewind_draws(rng_before, steps):
        """Leave the generator where the reference's loop leaves it: after the draws of `steps` steps of this chunk."""
        if rng_before is None:
            return
        scratch_ut, scratch_tb = np.zeros(max(steps, 1), dtype=np.uint8), np.zeros((max(steps, 1), B, N), dtype=np.int8)
        if agent.epsilon > 0.0 and draws_in_c(rng_before, steps, scratch_ut, scratch_tb):
            return
        np.random.set_state(rng_before)
        for _ in range(steps):
            if not agent.draw_branch():
                agent.draw_random_actions(B, N)

    # The device runs chunk c (a blocking C call that releases the GIL) on a worker thread while this thread draws the
    # policy's random numbers for chunk c + 1: an epsilon-greedy policy's legacy-RNG draws (32 x B x N integers per
    # chunk, 1.2 ms for 1000 worlds) otherwise sit between the chunks - 17 % of the `random` policy's sweep time.
    # The draws do not depend on the device's results; when the episode turns out to end in chunk c, the generator is
    # rewound to its state before chunk c and the draws of the executed steps are repeated.
    # (a policy that never takes its random branch draws one coin per step: nothing to overlap, and the hand-over to
    # the worker costs ~0.2 ms per chunk)
    pool = ThreadPoolExecutor(max_workers=1) if agent is not None and getattr(agent, "epsilon", 1.0) > 0.0 else None
    try:
        ahead = None
        while True:
            rng_before, use_table, table = ahead if ahead is not None else draw_chunk()
            ahead = None
            Ls = _luminosity_schedule(env, K)

            def on_device():
                if final_state:
                    eng.snapshot_save()
                # (the chunk's flags are summed below before the next chunk runs: the engine's own flag buffers are re-used)
                return eng.run_episode(Ls, mode, use_table, table, LIFESPAN_THRESHOLD_K, reuse_buffers=True)

            if pool is not None:
                pending = pool.submit(on_device)
                ahead = draw_chunk()
                alive_k, ok_k = pending.result()
            else:
                alive_k, ok_k = on_device()
            all_dead = ~alive_k.any(axis=1)
            ended = bool(all_dead.any())                       # also when the last world died on the chunk's last step
            executed = int(np.argmax(all_dead)) + 1 if ended else K
            done_at += _count_true(alive_k[:executed])
            agents_done_at += _count_true(ok_k[:executed])[..., None]
            if not final_state:
                executed = K                                   # the environment stays where the chunk ended
            elif executed < K:
                # the episode ended inside the chunk: replay exactly `executed` steps from the snapshot
                eng.snapshot_restore()
                eng.run_episode(Ls[:executed], mode, use_table[:executed], table[:executed], LIFESPAN_THRESHOLD_K)
            if ended:
                rewind_draws(rng_before, executed)
            for _ in range(executed):                          # host scalars of the environment
                env._L_pass = env.L
                env.L = env.update_L(env.L)
            env._invalidate()
            if ended:
                return done_at, agents_done_at
    finally:
        if pool is not None:
            pool.shutdown(wait=True)


def _advance_host_scalars(env, executed):
    """L, step_count and the ramp bookkeeping of `executed` steps the device has already taken."""
    for _ in range(executed):
        env._L_pass = env.L
        env.L = env.update_L(env.L)
    env._invalidate()


RAMP_ALIVE_THRESHOLD = 0.005      # the notebook's test for a living biosphere: max cover > 0.005


def dead_temperature(env, L):
    """The temperature of a lifeless planet at luminosity `L` (any shape), ((S L (1 - albedo_bare)) / sigma)^(1/4) in float64
    on the host - the reference's `dead_temp` (ref daisy_world_rl.py:407-408), the curve its figures hold the regulated
    mean temperature against."""
    L = np.asarray(L, dtype=np.float64)
    return ((env.S * L * (1 - env.albedo_bare)) / env.sigma) ** (1 / 4)


def _ramp_series(env, nsteps, run_trace, temperature=False):
    """The host side of `simulate_ramp`: the schedule of the next `nsteps` steps, ONE call `run_trace(L_schedule)` ->
    (n, B) records of dtype `_ffi.STATS_DTYPE` (the engine's `step_n_trace`), then the environment's scalars advanced as
    `nsteps` calls of `env.step()` would have.  `temperature`: `run_trace` returns (records, temperature records) - the
    engine's `step_n_trace_temperature`."""
    if env.n_agents:
        raise ValueError("simulate_ramp is for agent-free ensembles (n_agents == 0): with agents the reference's step(None) "
                         "still grazes with action 0 - use simulate_lifespan")
    n = int(nsteps)
    L = np.asarray(_luminosity_schedule(env, n), dtype=np.float64)
    stats, temps = run_trace(L) if temperature else (run_trace(L), None)
    _advance_host_scalars(env, n)
    return _series_dict(env, L, stats, temps)


def _series_dict(env, L, stats, temps=None):
    """What `simulate_ramp` and `simulate_luminosity_sweep` return, from the (n, B) records of a run - with the (n, B)
    temperature records of a `temperature=True` run, also its temperature curves."""
    cells = float(env.dim) * float(env.dim)
    max_cover = stats["max_k"] / 1000.0
    out = {"L": L,
           "mean_light": stats["sum_light_k"] / 1000.0 / cells,
           "mean_dark": stats["sum_dark_k"] / 1000.0 / cells,
           "max_cover": max_cover,
           "alive": max_cover > RAMP_ALIVE_THRESHOLD,
           "stats": stats}
    if temps is not None:
        out.update(mean_temp=temps["mean"], std_temp=temps["std"], min_temp=temps["min"], max_temp=temps["max"],
                   dead_temp=dead_temperature(env, L))
    return out


def simulate_ramp(env, nsteps, obs=None, temperature=False):
    """The time series of an agent-free ensemble over the next `nsteps` steps of its luminosity ramp - the curves of
    the reference's notebooks (daisy/notebook_helpers.py:50-54 appends `env.grid[:, 1].mean()` per step) without a host
    round trip per step: the per-step, per-world reductions are recorded on the device (`dw_step_n_trace`) and come
    down once.  `obs=None`: reset the environment first, as `simulate_lifespan` does.

    Returns a dict: `L` (n,) the luminosity each step used; `mean_light`, `mean_dark` (n, B) float64; `max_cover`
    (n, B); `alive` (n, B) bool, the notebook's `max > 0.005`; `stats` the raw (n, B) records (exact per-mille
    integers).  Afterwards `env.grid`, `env.step()`, `env.L`, `env.step_count` ... continue as if the steps had been
    taken one by one.

    `temperature=True`: the run also records the per-world statistics of the local temperature field every step
    computes - the reference's `env.temp.mean()` / `.std()` after each step (notebook_helpers.py:50-52, `run_q2_sims`) -
    through `dw_step_n_trace_temperature` (single steps plus one reduction each: slower than the cover-only run, same
    state afterwards).  The dict gains `mean_temp`, `std_temp`, `min_temp`, `max_temp` (n, B) in kelvin and `dead_temp`,
    the lifeless temperature at each step's luminosity (ref :407-408), with the shape of `L`."""
    if env.n_agents:
        raise ValueError("simulate_ramp is for agent-free ensembles (n_agents == 0): with agents the reference's step(None) "
                         "still grazes with action 0 - use simulate_grazing (the curves) or simulate_lifespan")
    if obs is None:
        env.reset()
    eng = env._ensure_engine()
    env._sync_to_device()
    if temperature:
        return _ramp_series(env, nsteps, eng.step_n_trace_temperature, temperature=True)
    return _ramp_series(env, nsteps, eng.step_n_trace)


def simulate_frames(env, nsteps, stride=1, tile=1, worlds=None, temperature=True, obs=None):
    """`simulate_ramp` with pictures: the next `nsteps` steps of an agent-free ensemble in ONE device-resident run
    (`dw_step_n_frames`) that also leaves, at every `stride`-th step, a frame of the worlds in `worlds` (None: all) - the
    image panels of the reference's figure (daisy/notebook_helpers.py `plot_grid` / `update_fig`:
    `tensor_to_image(env.grid[:, :3])`, `tensor_to_image(env.temp)`) reduced on the device to tiles of `tile` cells (an int
    or (tile_h, tile_w); 1: the planes and the field themselves).  `obs=None`: reset the environment first.

    Returns `simulate_ramp`'s dict for all `nsteps` steps plus: `frame_steps` (F,), `env.step_count` after each frame's
    step (F = nsteps // stride); `frame_L` (F,), that step's luminosity; `light`, `dark` (F, S, TH, TW), the mean cover of
    each tile - at 1 x 1 tiles `env.grid[:, 1]` and `env.grid[:, 2]` after that step; `cover`, the raw records (exact
    per-mille sums, dtype `_ffi.TILE_COVER_DTYPE`); `worlds` (S,); and with `temperature`: `temp` (F, S, TH, TW) in kelvin,
    the tile means of `env.temp` after that step (at 1 x 1 tiles `env.temp[:, 0]` bit for bit), and `frame_dead_temp` (F,).
    Afterwards `env.grid`, `env.step()`, `env.L`, `env.step_count` continue as if the steps had been taken one by one.
    With agents, take the steps with `env.step` and call `env._engine.reduce_tiles` after each."""
    if env.n_agents:
        raise ValueError("simulate_frames is for agent-free ensembles (n_agents == 0): with agents the reference's step(None) "
                         "still grazes with action 0 - step with env.step and call the engine's reduce_tiles after each step")
    if obs is None:
        env.reset()
    eng = env._ensure_engine()
    env._sync_to_device()
    n, stride = int(nsteps), int(stride)
    L = np.asarray(_luminosity_schedule(env, n), dtype=np.float64)
    step0 = int(env.step_count)
    cover, temp, stats = eng.step_n_frames(L, stride=stride, tile=tile, worlds=worlds, cover=True, temperature=bool(temperature),
                                           trace=True)
    _advance_host_scalars(env, n)
    out = _series_dict(env, L, stats)
    at = np.arange(stride - 1, n - n % stride, stride)          # the frames' steps within the run
    th, tw = (int(tile), int(tile)) if np.isscalar(tile) else (int(tile[0]), int(tile[1]))
    cells = float(th * tw)
    out.update(frame_steps=step0 + at + 1, frame_L=L[at],
               light=cover["sum_light_k"] / 1000.0 / cells, dark=cover["sum_dark_k"] / 1000.0 / cells, cover=cover,
               worlds=np.arange(int(env.batch_size)) if worlds is None else np.asarray(worlds, dtype=np.int64).reshape(-1))
    if temperature:
        out.update(temp=temp, frame_dead_temp=dead_temperature(env, L[at]))
    return out


def simulate_grazing(env, agent, nsteps, chunk=64, obs=None, temperature=False):
    """The `simulate_ramp` of an ensemble WITH agents: the time series of the daisy populations over the next `nsteps`
    steps while the agents graze - the curves of the reference's animations with an agent (daisy/notebook_helpers.py:
    218-223 `update_fig_agent`, rl_daisy_world.ipynb cells 12-16, greedy_longevity_abatement.ipynb cells 10-15 append
    `env.grid[:, 1].mean()` and `env.grid[:, 2].mean()` after every `env.step(action)`) - without a host round trip per
    step.  `agent`: `None` (the reference's `step(None)`: action 0) or a `Greedy` in any mode or epsilon.  `obs=None`:
    reset the environment first.

    The first step goes through `env.step` (the initial state is un-quantised); the remaining `nsteps - 1` run
    device-resident in chunks of `chunk` steps (`dw_run_episode_trace`: policy, grazing, physics, flags and the per-step,
    per-world reductions).  An epsilon-greedy policy's draws are taken from the legacy NumPy stream in the reference's
    order, for exactly `nsteps` steps: the generator ends where the reference's loop leaves it.

    Returns the dict of `simulate_ramp` (`L`, `mean_light`, `mean_dark`, `max_cover`, `alive`, `stats`) plus `agent_ok`
    (n, B, N) bool - reward >= 0.1 after the step - and `agents_alive` (n, B) int, their number per world.  Afterwards
    `env.grid`, `env.step()`, `env.L`, `env.step_count` continue as if `nsteps` calls of `env.step(agent(obs))` had been
    made.  Precision "f64", `collision_mode == 1` and any other callable agent: the same dict from a host loop, one
    `env.step` and one `reduce()` per step.

    `temperature=True`: the run also records the per-world statistics of the local temperature field every step computes
    from the grazed state - the reference's `env.temp.mean()` / `.std()` after each `env.step(action)`, the curves
    `update_fig_agent` appends next to `env.dead_temp` (notebook_helpers.py:210-223) - through
    `dw_run_episode_trace_temperature` (the first step and the host loop: `reduce_temperature` after the step).  The
    dict gains `mean_temp`, `std_temp`, `min_temp`, `max_temp` (n, B) in kelvin and `dead_temp` (n,); everything else,
    the state afterwards and the generator's final state are those of the cover-only run."""
    return _grazing_run(env, agent, nsteps, chunk, obs, temperature)


class _GrazingFrames:
    """The frames of a `_grazing_run`: step t of the run leaves a frame when (t + 1) % stride == 0."""

    def __init__(self, env, n, stride, tile, worlds, temperature):
        self.stride, self.tile, self.worlds, self.temperature = int(stride), tile, worlds, bool(temperature)
        if self.stride < 1:
            raise ValueError("stride must be at least 1")
        self.sel = None if worlds is None else np.asarray(worlds, dtype=np.int64).reshape(-1)
        self.at = np.arange(self.stride - 1, n - n % self.stride, self.stride)    # the frames' steps within the run
        self.cover, self.temp, self.agents = [], [], []

    def call(self, t, K, n):
        """(steps, stride) of the device call that starts at step t of the run: from a whole stride of the run on, `K` rounded
        down to a multiple of the stride (at least one stride), so that a frame never straddles a call; a call that starts
        elsewhere (behind the run's first step, which the host takes) ends at the next whole stride, with one frame there."""
        s, off = self.stride, t % self.stride
        if off:
            return min(s - off, n - t), s - off
        return min(max(K // s * s, s), n - t), s

    def host(self, eng, t, L_t, N):
        """Step t was taken by `env.step`: its frame, if it leaves one, from the on-demand calls."""
        if (t + 1) % self.stride:
            return
        cov, tmp = eng.reduce_tiles(L_t, tile=self.tile, worlds=self.worlds, cover=True, temperature=self.temperature)
        self.cover.append(cov[None])
        if self.temperature:
            self.temp.append(tmp[None])
        if N:
            idx, st = eng.download_agents()
            pick = slice(None) if self.sel is None else self.sel
            rec = np.zeros((1,) + st[pick].shape, dtype=_ffi.AGENT_FRAME_DTYPE)
            rec["row"][0], rec["col"][0], rec["state"][0] = idx[pick][..., 0], idx[pick][..., 1], st[pick]
            self.agents.append(rec)

    def device(self, cov, tmp, ag):
        self.cover.append(cov)
        if self.temperature:
            self.temp.append(tmp)
        if ag is not None:
            self.agents.append(ag)

    def into(self, out, env, step0, N):
        th, tw = (int(self.tile), int(self.tile)) if np.isscalar(self.tile) else (int(self.tile[0]), int(self.tile[1]))
        cells = float(th * tw)
        cover = np.concatenate(self.cover) if self.cover else np.zeros((0,), dtype=_ffi.TILE_COVER_DTYPE)
        out.update(frame_steps=step0 + self.at + 1, frame_L=out["L"][self.at],
                   light=cover["sum_light_k"] / 1000.0 / cells, dark=cover["sum_dark_k"] / 1000.0 / cells, cover=cover,
                   worlds=np.arange(int(env.batch_size)) if self.sel is None else self.sel)
        if self.temperature:
            out.update(temp=np.concatenate(self.temp) if self.temp else np.zeros((0,)),
                       frame_dead_temp=dead_temperature(env, out["L"][self.at]))
        if N:
            ag = np.concatenate(self.agents) if self.agents else np.zeros((0,), dtype=_ffi.AGENT_FRAME_DTYPE)
            out.update(agent_pos=np.stack([ag["row"], ag["col"]], axis=-1), agent_state=ag["state"])


def _grazing_run(env, agent, nsteps, chunk, obs, temperature, frames=None):
    """`simulate_grazing` and, with `frames` (stride, tile, worlds, temperature), `simulate_grazing_frames`: one loop, one
    policy handling."""
    n = int(nsteps)
    if n < 1:
        raise ValueError("nsteps must be at least 1")
    K = int(chunk)
    if K < 1:
        raise ValueError("chunk must be at least 1")
    if obs is None:
        obs = env.reset()
    B, N = int(env.batch_size), int(env.n_agents)
    step0 = int(env.step_count)
    fr = _GrazingFrames(env, n, *frames) if frames is not None else None
    L = np.zeros(n, dtype=np.float64)
    stats = np.zeros((n, B), dtype=_ffi.STATS_DTYPE)
    ok = np.zeros((n, B, N), dtype=bool)
    temps = np.zeros((n, B), dtype=_ffi.TEMP_STATS_DTYPE) if temperature else None

    def host_step(t, obs):
        """Step t as the notebook takes it; its row from `reduce()` and `done`."""
        action = agent(obs) if agent is not None else None
        L[t] = env.L
        obs, _, done, _ = env.step(action)
        row = env._engine.reduce()
        for f in ("max_k", "sum_light_k", "sum_dark_k"):
            stats[f][t] = row[f]
        if temperature:
            temps[t] = env._engine.reduce_temperature(L[t])
        if fr is not None:
            fr.host(env._engine, t, L[t], N)
        if N:
            ok[t] = ~np.asarray(done).reshape(B, N)
        return obs

    mode = _policy_mode(agent)
    on_device = env.precision != "f64" and env.collision_mode == 0 and mode is not None
    obs = host_step(0, obs)
    if not on_device:
        for t in range(1, n):
            obs = host_step(t, obs)
    else:
        eng = env._engine
        t = 1
        while t < n:
            k, stride = (min(K, n - t), 0) if fr is None else fr.call(t, K, n)
            use_table = np.zeros(k, dtype=np.uint8)
            table = np.zeros((k, B, N), dtype=np.int8)
            if agent is not None:                              # the reference's order: one coin per call, then the batch's actions
                for i in range(k):
                    if not agent.draw_branch():
                        use_table[i] = 1
                        table[i] = agent.draw_random_actions(B, N)[..., 0]
            Ls = np.asarray(_luminosity_schedule(env, k), dtype=np.float64)
            L[t:t + k] = Ls
            if fr is not None:
                res = eng.run_episode_frames(Ls, mode, use_table, table, LIFESPAN_THRESHOLD_K, stride=stride, tile=fr.tile,
                                             worlds=fr.worlds, cover=True, temperature=fr.temperature, agents=N > 0, trace=True,
                                             temps=bool(temperature))
                fr.device(*res[:3])
                stats[t:t + k], ok[t:t + k] = res[3], res[5]
                if temperature:
                    temps[t:t + k] = res[6]
            elif temperature:
                stats[t:t + k], _, ok[t:t + k], temps[t:t + k] = eng.run_episode_trace(Ls, mode, use_table, table,
                                                                                       LIFESPAN_THRESHOLD_K, temperature=True)
            else:
                stats[t:t + k], _, ok[t:t + k] = eng.run_episode_trace(Ls, mode, use_table, table, LIFESPAN_THRESHOLD_K)
            _advance_host_scalars(env, k)
            t += k
    out = _series_dict(env, L, stats, temps)
    out["agent_ok"] = ok
    out["agents_alive"] = ok.sum(axis=2)
    if fr is not None:
        fr.into(out, env, step0, N)
    return out


def simulate_grazing_frames(env, agent, nsteps, stride=1, tile=1, worlds=None, temperature=True, chunk=64, obs=None):
    """`simulate_grazing` with pictures: the reference's animation with an agent in it (daisy/notebook_helpers.py:180-258
    `update_fig_agent` redraws `env.grid[:, :3]`, `env.temp` and the agent channel `env.grid[:, 4]` after every
    `env.step(action)`) without a host round trip per step.  `agent`, `chunk` and `obs` are `simulate_grazing`'s, and so is
    the handling of the policy, an epsilon-greedy one's host-drawn table included.  Step t of the run leaves a frame of the
    worlds in `worlds` (None: all) when (t + 1) % stride == 0: F = nsteps // stride frames, reduced to tiles of `tile` cells
    (an int or (tile_h, tile_w); 1: the planes and the field themselves).

    The first step goes through `env.step` (its frame, if it leaves one, through `reduce_tiles` and `download_agents`); the
    others run device-resident (`dw_run_episode_frames`) in chunks of `chunk` steps rounded down to a multiple of `stride`
    (at least `stride`), so that a frame never straddles a call; with `stride > 1` the first device call ends at the
    run's first whole stride.

    Returns `simulate_grazing`'s dict plus `frame_steps` (F,), `env.step_count` after each frame's step; `frame_L` (F,);
    `light`, `dark` (F, S, TH, TW), the mean cover of each tile after that step; `cover`, the raw records; `worlds` (S,);
    `temp` (F, S, TH, TW) in kelvin, the tile means of `env.temp` after that step, and `frame_dead_temp` (F,) - unless
    `temperature=False`; and, with agents, `agent_pos` (F, S, N, 2), row and column, and `agent_state` (F, S, N), the energy
    store the reference writes into channel 4 at that position (an agent-free environment is served without the two).  The
    temperature CURVES of `simulate_grazing(temperature=True)` are not recorded here.  Precision "f64", `collision_mode == 1`
    and any other callable agent: the same dict from a host loop."""
    return _grazing_run(env, agent, nsteps, chunk, obs, False, frames=(stride, tile, worlds, temperature))


def simulate_luminosity_sweep(env, L_values, nsteps, obs=None, temperature=False):
    """The response of an agent-free ensemble to forcing in ONE run: world b is held at luminosity `L_values[b]` for
    `nsteps` steps (`len(L_values) == env.batch_size`) - the bifurcation diagram the reference's notebooks assemble from
    one run per luminosity (`run_q2_sims`, the `min_L` / `max_L` edits).  `L_values` may also be (nsteps, B): a schedule
    per world, e.g. half the worlds ramping up and half ramping down for the hysteresis loop.  The per-step, per-world
    reductions are recorded on the device (`dw_step_n_trace_per_world`) and come down once.  `obs=None`: reset first.

    Returns the dict of `simulate_ramp` with `L` of shape (n, B).  The reference's `env.L` is ONE number and has no
    meaning after such a run: `env.step()` and `env.grid` raise until `env.reset()` (the covers are available from
    `env._engine.download_planes()`, the last records from the returned series).

    `temperature=True`: as in `simulate_ramp` - the temperature curves of every world at its own luminosity
    (`mean_temp`, `std_temp`, `min_temp`, `max_temp`, `dead_temp`, each (n, B))."""
    if env.n_agents:
        raise ValueError("simulate_luminosity_sweep is for agent-free ensembles (n_agents == 0)")
    n = int(nsteps)
    L = np.asarray(L_values, dtype=np.float64)
    if L.ndim == 1:
        L = np.broadcast_to(L, (n, L.shape[0]))
    if L.ndim != 2 or L.shape != (n, int(env.batch_size)):
        raise ValueError(f"L_values needs shape ({int(env.batch_size)},) or ({n}, {int(env.batch_size)}), got {np.shape(L_values)}")
    L = np.ascontiguousarray(L)
    if obs is None:
        env.reset()
    eng = env._ensure_engine()
    env._sync_to_device()
    stats, temps = eng.step_n_trace_temperature(L) if temperature else (eng.step_n_trace_per_world(L), None)
    env._invalidate()
    env._per_world_L = True
    return _series_dict(env, L, stats, temps)


def simulate_parameter_sweep(env, params, nsteps, L_values=None, obs=None, temperature=False):
    """A sweep over physics constants in ONE run: world b steps with the constants `params` names - a dict from a member
    of `_ffi.WORLD_PARAM_NAMES` (`q2`, `gamma`, the albedos, `temp_optimal`, `dt`, ...) to a scalar or a length-B array;
    members not named keep the environment's attribute - the figures the reference's notebooks assemble from one run per
    value (`run_q2_sims`: the same ramp with `env.q2 = 0, q/64, q/8`).  `L_values=None`: every world follows the
    environment's own luminosity ramp, as `simulate_ramp` (and the environment's `L` advances with it); `(B,)` or
    `(nsteps, B)`: as `simulate_luminosity_sweep` reads them.  Recorded on the device (`dw_step_n_trace_ensemble`), one
    download.  `obs=None`: reset first.

    Returns the dict of `simulate_luminosity_sweep` (`L` of shape (n, B)) plus `params`, the (B,) table of dtype
    `_ffi.WORLD_PARAMS_DTYPE` the run used; with `temperature=True`, `dead_temp[:, b]` is the lifeless temperature of
    world b from its own `S`, `sigma` and `albedo_bare`.  As after `simulate_luminosity_sweep`, `env.step()` and `env.grid`
    raise until `env.reset()`."""
    if env.n_agents:
        raise ValueError("simulate_parameter_sweep is for agent-free ensembles (n_agents == 0)")
    n, B = int(nsteps), int(env.batch_size)
    unknown = sorted(set(params) - set(_ffi.WORLD_PARAM_NAMES))
    if unknown:
        raise ValueError(f"not a per-world constant: {unknown} (one of {_ffi.WORLD_PARAM_NAMES})")
    table = np.zeros(B, dtype=_ffi.WORLD_PARAMS_DTYPE)
    for name in _ffi.WORLD_PARAM_NAMES:
        value = np.asarray(params.get(name, getattr(env, name)), dtype=np.float64)
        if value.shape not in ((), (B,)):
            raise ValueError(f"params[{name!r}] needs a scalar or shape ({B},), got {value.shape}")
        table[name] = value
    ramp = L_values is None
    if not ramp:
        L = np.asarray(L_values, dtype=np.float64)
        if L.ndim == 1:
            L = np.broadcast_to(L, (n, L.shape[0]))
        if L.ndim != 2 or L.shape != (n, B):
            raise ValueError(f"L_values needs shape ({B},) or ({n}, {B}), got {np.shape(L_values)}")
    if obs is None:
        env.reset()
    if ramp:
        L = np.repeat(np.asarray(_luminosity_schedule(env, n), dtype=np.float64)[:, None], B, axis=1)
    L = np.ascontiguousarray(L)
    eng = env._ensure_engine()
    env._sync_to_device()
    res = eng.step_n_trace_ensemble(table, L, temperature=temperature)
    stats, temps = res if temperature else (res, None)
    if ramp:
        _advance_host_scalars(env, n)
    env._invalidate()
    env._per_world_L = True
    out = _series_dict(env, L, stats, temps)
    if temps is not None:
        out["dead_temp"] = ((table["S"] * L * (1 - table["albedo_bare"])) / table["sigma"]) ** (1 / 4)
    out["params"] = table
    return out


def _sweep_param_table(env, scenarios, worlds_per_scenario):
    """The (S * Bs,) table of dtype `_ffi.WORLD_PARAMS_DTYPE` of a scenario list: scenario s owns the contiguous block of
    worlds [s * Bs, (s + 1) * Bs); a member its `params` does not name keeps the environment's attribute."""
    Bs = int(worlds_per_scenario)
    table = np.zeros(len(scenarios) * Bs, dtype=_ffi.WORLD_PARAMS_DTYPE)
    for s, sc in enumerate(scenarios):
        params = sc.get("params") or {}
        unknown = sorted(set(params) - set(_ffi.WORLD_PARAM_NAMES))
        if unknown:
            raise ValueError(f"scenario {s}: not a per-world constant: {unknown} (one of {_ffi.WORLD_PARAM_NAMES})")
        for name in _ffi.WORLD_PARAM_NAMES:
            value = np.asarray(params.get(name, getattr(env, name)), dtype=np.float64)
            if value.shape not in ((), (Bs,)):
                raise ValueError(f"scenario {s}: params[{name!r}] needs a scalar or shape ({Bs},), got {value.shape}")
            table[name][s * Bs:(s + 1) * Bs] = value
    return table


def _sweep_action_table(scenarios, running, K, Bs, N):
    """The (K, S * Bs, N) int8 action table of one chunk, filled per block: -1 / -2 for the worlds of a greedy /
    anti-greedy scenario (the device takes that agent's choice), 0 for `agent=None` (ref step(None): action 0), and on a
    step at which an epsilon-greedy scenario's coin takes the random branch, that block's host-drawn codes 0..8.  The
    draws come from `np.random` in this order: step-major, within a step scenario-major, for each scenario with
    epsilon > 0 that is still running one `rand()` and, on the random branch, one `randint(9)` for the block
    (`Greedy.draw_branch` / `draw_random_actions`); a scenario with epsilon = 0, or one that has ended, draws nothing."""
    S = len(scenarios)
    table = np.zeros((K, S * Bs, N), dtype=np.int8)
    drawing = []
    for s, sc in enumerate(scenarios):
        agent = sc.get("agent")
        if agent is not None:
            table[:, s * Bs:(s + 1) * Bs] = -1 if agent.greedy else -2
            if agent.epsilon > 0.0 and running[s]:
                drawing.append((s, agent))
    for t in range(K if drawing else 0):
        for s, agent in drawing:
            if not agent.draw_branch():
                table[t, s * Bs:(s + 1) * Bs] = agent.draw_random_actions(Bs, N)[..., 0]
    return table


def _sweep_account(done_at, agents_done_at, running, alive_k, ok_k):
    """The notebook's counting and stopping rule (cell 2:46-57) applied per scenario to the flags of a chunk: alive_k
    (K, S * Bs) and ok_k (K, S * Bs, N) are added to done_at (S, Bs) and agents_done_at (S, Bs, N, 1) for the steps up to
    and including the one at which all of the SCENARIO's worlds are dead; from then on the scenario's counts are frozen
    (`running[s]` False, in place), whatever its worlds do while the other scenarios finish."""
    S, Bs = done_at.shape
    K = alive_k.shape[0]
    alive = np.asarray(alive_k, dtype=bool).reshape(K, S, Bs)
    all_dead = ~alive.any(axis=2)                                                  # (K, S)
    earlier = np.zeros((K, S), dtype=bool)
    earlier[1:] = np.logical_or.accumulate(all_dead, axis=0)[:-1]
    counted = running[None, :] & ~earlier                                          # the scenario still counts step t
    done_at += np.count_nonzero(alive & counted[:, :, None], axis=0)
    if agents_done_at.size:
        ok = np.asarray(ok_k, dtype=bool).reshape(K, S, Bs, -1)
        agents_done_at += np.count_nonzero(ok & counted[:, :, None, None], axis=0)[..., None]
    running &= ~all_dead.any(axis=0)


def simulate_lifespan_sweep(env, scenarios, worlds_per_scenario, chunk=32, obs=None):
    """The reference's lifespan table (notebooks/greedy_longevity_abatement.ipynb: policies x albedo settings, each an
    ensemble run until every biosphere is dead) - or a lifespan-versus-q2 / gamma / temp_optimal scan - as ONE
    device-resident run instead of one `reset()`, one configuration and one `simulate_lifespan` per scenario.

    `scenarios` is a list of `{"params": {member: value}, "agent": Greedy | None}`: `params` names members of
    `_ffi.WORLD_PARAM_NAMES` (a scalar, or one value per world of the block; members not named keep the environment's
    attribute), `agent` is a `Greedy` in any of its modes or None (ref step(None): action 0).  Scenario s owns the
    contiguous block of worlds [s * worlds_per_scenario, (s + 1) * worlds_per_scenario), and
    `env.batch_size == len(scenarios) * worlds_per_scenario`.  Every world follows the environment's own luminosity
    ramp; `agent_gamma`, the observation mask and the initial-state fields are the environment's and shared.
    `obs=None`: reset the environment first; or pass the observations of a reset already done (`reset_synthetic`).
    A scenario may carry `"n_agents": k` with 0 <= k <= env.n_agents: its worlds have the first k agents only - the states
    of the others are uploaded as 0 before step 1, which is exact for `Greedy` and None (they read channels 1 and 2 only,
    and an agent of state 0 never moves, grazes or revives); their `agents_done_at` entries are 0.

    The first step starts from the un-quantised state: the policies' actions from the reset observations (block by
    block), `dw_update_agents`, one step of `dw_step_n_trace_ensemble`, `dw_get_reward_done`.  Then chunks of `chunk`
    steps of `dw_run_episode_ensemble` with the action table filled per block (`_sweep_action_table`).  A scenario's
    counts stop at the step at which all of ITS worlds are dead (the notebook's rule, per scenario); the run ends when
    every scenario has ended.

    Returns `(done_at (S, Bs), agents_done_at (S, Bs, N, 1), params)`, `params` the (S * Bs,) table of constants the run
    used.  A scenario with epsilon = 0 (or no agent) gets exactly the counts `simulate_lifespan` gives for its block of
    worlds with those constants set on the environment; a scenario with epsilon > 0 draws from `np.random` in the order
    `_sweep_action_table` documents, not in the order of a separate run: statistically equivalent, not bit-equal.
    The caller gets lifespans only: the worlds stop at the end of the last chunk and have no common luminosity or
    constants, so `env.step()` and `env.grid` raise until `env.reset()` (as `simulate_lifespan(final_state=False)`
    leaves an environment that is of no further use)."""
    S, Bs = len(scenarios), int(worlds_per_scenario)
    if S < 1 or Bs < 1 or int(env.batch_size) != S * Bs:
        raise ValueError(f"env.batch_size ({int(env.batch_size)}) must be len(scenarios) * worlds_per_scenario ({S} * {Bs})")
    for s, sc in enumerate(scenarios):
        if sc.get("agent") is not None and type(sc["agent"]) is not Greedy:
            raise ValueError(f"scenario {s}: the agent must be a Greedy or None")
        if "n_agents" in sc and not 0 <= int(sc["n_agents"]) <= int(env.n_agents):
            raise ValueError(f"scenario {s}: n_agents ({sc['n_agents']}) outside 0..env.n_agents ({int(env.n_agents)})")
    if env.precision == "f64" or env.collision_mode != 0:
        raise ValueError("simulate_lifespan_sweep runs device-resident: precision 'exact' or 'fast', collision_mode 0")
    table = _sweep_param_table(env, scenarios, Bs)
    if obs is None:
        obs = env.reset()
    B, N = S * Bs, int(env.n_agents)
    if N and any("n_agents" in sc for sc in scenarios):
        states = np.array(env.agent_states, dtype=np.float64)
        for s, sc in enumerate(scenarios):
            if "n_agents" in sc:
                states[s * Bs:(s + 1) * Bs, int(sc["n_agents"]):] = 0.0
        env.agent_states = states                               # uploaded by _sync_to_device below, before step 1
    done_at = np.zeros((S, Bs), dtype=int)
    agents_done_at = np.zeros((S, Bs, N, 1), dtype=int)
    running = np.ones(S, dtype=bool)
    eng = env._ensure_engine()
    env._sync_to_device()
    # step 1: the initial state is not quantised (ref initialize_grid)
    if N:
        action = np.zeros((B, N, 1), dtype=np.int64)
        for s, sc in enumerate(scenarios):
            if sc.get("agent") is not None:
                action[s * Bs:(s + 1) * Bs] = sc["agent"](obs[s * Bs:(s + 1) * Bs])
        eng.update_agents(action)
    L1 = np.full((1, B), _luminosity_schedule(env, 1)[0], dtype=np.float64)
    stats = eng.step_n_trace_ensemble(table, L1)
    _, done = eng.reward_done()
    _advance_host_scalars(env, 1)
    env._per_world_L = True
    _sweep_account(done_at, agents_done_at, running, stats["max_k"] > LIFESPAN_THRESHOLD_K, ~done[None, ..., 0])
    K = int(chunk)
    while running.any():
        Ls = np.repeat(np.asarray(_luminosity_schedule(env, K), dtype=np.float64)[:, None], B, axis=1)
        actions = _sweep_action_table(scenarios, running, K, Bs, N)
        alive_k, ok_k = eng.run_episode_ensemble(table, Ls, _ffi.POLICY_TABLE, None, actions, LIFESPAN_THRESHOLD_K)
        _sweep_account(done_at, agents_done_at, running, alive_k, ok_k)
        _advance_host_scalars(env, K)
    return done_at, agents_done_at, table


def simulate_agent_count_sweep(env, agent, counts, worlds_per_count, chunk=64, max_steps=None, obs=None):
    """The reference's agent-count scan (notebooks/daisy_world_existential_risk_and_agency.ipynb, cells fd8ad489 ..
    227e4895: how long the biosphere lives with n_agents = 1, 31, .. 271 grazers on the 16x16 world, 10 worlds per count,
    under the trained MLP, the greedy and the anti-greedy policy) as ONE device-resident run instead of one environment,
    one `reset()` and one run per count.

    Block s owns the worlds [s * Bs, (s + 1) * Bs), Bs = `worlds_per_count`, and has the first `counts[s]` of the
    environment's agents; `env.batch_size == len(counts) * Bs` and `env.n_agents >= max(counts)`, else ValueError before
    anything is reset.  `agent` is an `MLP`, a `Greedy` with `epsilon == 0`, or None (ref step(None): action 0).

    An `MLP` runs in chunks of `chunk` steps of `dw_run_episode_mlp_counts` with every agent on the one parameter set: the
    absent agents are neither observed nor stamped into channel 4 of the grid the MLP reads, so a block is bit for bit an
    environment of `counts[s]` agents.  A `Greedy` or None is delegated to `simulate_lifespan_sweep` with `"n_agents"`
    scenarios (`max_steps` must then be None: that run has no step limit).  The notebook's rule holds per block
    (`_sweep_account`): a block's counts stop at the step at which all of its worlds have maximum cover <= 0.005; the run
    ends at the end of the chunk in which the last block ended, or after `max_steps` steps.

    Returns `(done_at (S, Bs), agents_done_at (S, Bs, N, 1), n_active (S * Bs,))`; entries of absent agents are 0.  As after
    `simulate_lifespan_sweep` the environment is of no further use until `reset()`."""
    from .agents.mlp import MLP
    counts = [int(c) for c in counts]
    S, Bs, N = len(counts), int(worlds_per_count), int(env.n_agents)
    if S < 1 or Bs < 1 or int(env.batch_size) != S * Bs:
        raise ValueError(f"env.batch_size ({int(env.batch_size)}) must be len(counts) * worlds_per_count ({S} * {Bs})")
    if min(counts) < 0 or max(counts) > N:
        raise ValueError(f"counts must lie in 0..env.n_agents ({N}), got {counts}")
    scripted = agent is None or (type(agent) is Greedy and agent.epsilon == 0)
    if not scripted and not isinstance(agent, MLP):
        raise ValueError("the agent must be an MLP, a Greedy with epsilon == 0, or None")
    n_active = np.repeat(np.asarray(counts, dtype=np.int32), Bs)
    if scripted:
        if max_steps is not None:
            raise ValueError("max_steps applies to an MLP: the scripted policies run until every block has ended")
        scenarios = [{"agent": agent, "n_agents": c} for c in counts]
        done_at, agents_done_at, _ = simulate_lifespan_sweep(env, scenarios, Bs, chunk=chunk, obs=obs)
        return done_at, agents_done_at, n_active
    K = int(chunk)
    if K < 1 or (max_steps is not None and int(max_steps) < 1):
        raise ValueError("chunk and max_steps must be at least 1")
    if N < 1:
        raise ValueError("an MLP needs env.n_agents >= 1")
    if env.precision == "f64" or env.collision_mode != 0:
        raise ValueError("simulate_agent_count_sweep runs device-resident: precision 'exact' or 'fast', collision_mode 0")
    if obs is None:
        env.reset()
    params = np.asarray(agent.get_parameters(), dtype=np.float64).reshape(1, 1808)
    done_at = np.zeros((S, Bs), dtype=int)
    agents_done_at = np.zeros((S, Bs, N, 1), dtype=int)
    running = np.ones(S, dtype=bool)
    eng = env._ensure_engine()
    env._sync_to_device()
    steps = 0
    while running.any() and (max_steps is None or steps < int(max_steps)):
        k = K if max_steps is None else min(K, int(max_steps) - steps)
        Ls = np.asarray(_luminosity_schedule(env, k), dtype=np.float64)
        _, done, stats = eng.run_episode_mlp_counts(Ls, params if steps == 0 else None, n_active, split=N, L_init=env._L_pass,
                                                    n_members=1)
        _sweep_account(done_at, agents_done_at, running, stats["max_k"] > LIFESPAN_THRESHOLD_K, ~done[..., 0])
        _advance_host_scalars(env, k)
        steps += k
    return done_at, agents_done_at, n_active


def simulate_grazing_sweep(env, scenarios, worlds_per_scenario, nsteps, chunk=64, obs=None, temperature=False):
    """The population (and temperature) curves of several scenarios side by side from ONE device-resident run - the
    reference README's comparison of greedy, anti-greedy, random and no agents under light-and-dark and under neutral
    albedos, which shows when regulation breaks and why - instead of one environment, one configuration and one
    `simulate_grazing` per scenario.

    `scenarios`, `worlds_per_scenario` and `obs` are `simulate_lifespan_sweep`'s: scenario s owns the contiguous block of
    worlds [s * Bs, (s + 1) * Bs), and `env.batch_size == len(scenarios) * Bs`.  Every scenario runs exactly `nsteps`
    steps of the environment's own luminosity ramp: there is no stopping rule, as in `simulate_grazing`.

    The first step starts from the un-quantised state as in `simulate_lifespan_sweep` (the policies' actions block by
    block, `dw_update_agents`, one step of `dw_step_n_trace_ensemble`, which gives the first row of records and
    temperature rows, `dw_get_reward_done`); then chunks of `chunk` steps of `dw_run_episode_ensemble_trace` with the
    action table filled per block (`_sweep_action_table`, every scenario running).

    Returns a dict with every per-world entry reshaped to (n, S, Bs, ...): `L` (n,); `mean_light`, `mean_dark`,
    `max_cover`, `alive` and `stats` (n, S, Bs); `agent_ok` (n, S, Bs, N) bool and `agents_alive` (n, S, Bs) int; `params`,
    the (S * Bs,) table of constants the run used.  `temperature=True`: also `mean_temp`, `std_temp`, `min_temp`,
    `max_temp` (n, S, Bs) in kelvin and `dead_temp` (n, S, Bs), each world's lifeless temperature from its own `S`,
    `albedo_bare` and `sigma`.  Block s of every entry is what `simulate_grazing` returns for that block of worlds with the
    scenario's constants set on the environment when its epsilon is 0 (or it has no agent); a scenario with epsilon > 0
    draws in `_sweep_action_table`'s order: statistically equivalent, not bit-equal.  Afterwards the worlds have no
    common constants: `env.step()` and `env.grid` raise until `env.reset()`, as after `simulate_lifespan_sweep`."""
    S, Bs = len(scenarios), int(worlds_per_scenario)
    if S < 1 or Bs < 1 or int(env.batch_size) != S * Bs:
        raise ValueError(f"env.batch_size ({int(env.batch_size)}) must be len(scenarios) * worlds_per_scenario ({S} * {Bs})")
    for s, sc in enumerate(scenarios):
        if sc.get("agent") is not None and type(sc["agent"]) is not Greedy:
            raise ValueError(f"scenario {s}: the agent must be a Greedy or None")
    if env.precision == "f64" or env.collision_mode != 0:
        raise ValueError("simulate_grazing_sweep runs device-resident: precision 'exact' or 'fast', collision_mode 0")
    n, K = int(nsteps), int(chunk)
    if n < 1:
        raise ValueError("nsteps must be at least 1")
    if K < 1:
        raise ValueError("chunk must be at least 1")
    table = _sweep_param_table(env, scenarios, Bs)
    if obs is None:
        obs = env.reset()
    B, N = S * Bs, int(env.n_agents)
    L = np.zeros(n, dtype=np.float64)
    stats = np.zeros((n, B), dtype=_ffi.STATS_DTYPE)
    ok = np.zeros((n, B, N), dtype=bool)
    temps = np.zeros((n, B), dtype=_ffi.TEMP_STATS_DTYPE) if temperature else None
    running = np.ones(S, dtype=bool)
    eng = env._ensure_engine()
    env._sync_to_device()
    # step 1: the initial state is not quantised (ref initialize_grid)
    if N:
        action = np.zeros((B, N, 1), dtype=np.int64)
        for s, sc in enumerate(scenarios):
            if sc.get("agent") is not None:
                action[s * Bs:(s + 1) * Bs] = sc["agent"](obs[s * Bs:(s + 1) * Bs])
        eng.update_agents(action)
    L[0] = _luminosity_schedule(env, 1)[0]
    first = eng.step_n_trace_ensemble(table, np.full((1, B), L[0], dtype=np.float64), temperature=temperature)
    if temperature:
        stats[:1], temps[:1] = first
    else:
        stats[:1] = first
    _, done = eng.reward_done()
    if N:
        ok[0] = ~np.asarray(done).reshape(B, N)
    _advance_host_scalars(env, 1)
    env._per_world_L = True
    t = 1
    while t < n:
        k = min(K, n - t)
        Ls = np.asarray(_luminosity_schedule(env, k), dtype=np.float64)
        L[t:t + k] = Ls
        actions = _sweep_action_table(scenarios, running, k, Bs, N)
        _, ok[t:t + k], stats[t:t + k], rows = eng.run_episode_ensemble(
            table, np.repeat(Ls[:, None], B, axis=1), _ffi.POLICY_TABLE, None, actions, LIFESPAN_THRESHOLD_K, trace=True,
            temperature=temperature)
        if temperature:
            temps[t:t + k] = rows
        _advance_host_scalars(env, k)
        t += k
    out = _series_dict(env, L, stats, temps)
    if temperature:
        out["dead_temp"] = ((table["S"] * L[:, None] * (1 - table["albedo_bare"])) / table["sigma"]) ** (1 / 4)
    out["agent_ok"] = ok
    out["agents_alive"] = ok.sum(axis=2)
    for key, value in out.items():
        if key != "L":
            out[key] = value.reshape((n, S, Bs) + value.shape[2:])
    out["params"] = table
    return out


def _mlp_chunks(env, params, member_a, member_b, half, max_steps, chunk, after_chunk):
    """The step loop shared by the two fitness harnesses: chunks of steps device-resident
    (``dw_run_episode_mlp``), the reference's per-step float64 bookkeeping done by `after_chunk(rewards,
    dones) -> (executed, finished)` on the downloaded (K,B,N,1) rewards (already `reward * (reward > 0)`) and
    done flags of the chunk: it accounts for the steps up to and including the one that ends the episode, with
    every float64 sum accumulated in step order.  When the episode ends inside a chunk, the chunk is replayed
    from a device-side snapshot for exactly the executed steps, so the environment is left where the
    reference's loop leaves it.

    The device runs chunk c + 1 while this thread accounts for chunk c (a worker thread around the blocking C calls,
    which release the GIL): the bookkeeping - NumPy reductions in the reference's order over 4 MB of rewards per chunk
    for a population of 64 x 32 worlds - costs more than the chunk's kernel.  Chunk c + 1 does not depend on it except
    for "has the episode ended": its rewards go to the engine's second page-locked buffer, the state at its start to
    snapshot slot (c + 1) % 2, and when chunk c turns out to end the episode the speculative chunk is undone from the
    snapshots (slot c % 2 + a replay of the executed steps, or slot (c + 1) % 2 as it is when chunk c ran to its end).

    `after_chunk=None`: the bookkeeping is the device's (``dw_run_episode_mlp_fitness`` between `Engine.fitness_begin` and
    `Engine.fitness_download`, the caller's): the same loop, each chunk's call returns its `(executed, finished)` and nothing
    else comes down.  The speculative chunk's accounting changes nothing when chunk c ended the episode - no member runs
    any more - and the replay of the executed steps is the plain ``dw_run_episode_mlp``."""
    eng = env._engine
    n_members = np.asarray(params).reshape(-1, 1808).shape[0]
    if env.step_count >= max_steps:
        return
    env._sync_to_device()

    def on_device(c, Ls, L_init, first):
        if not first:                                    # (the first step starts from the un-quantised state: nothing to save,
            eng.snapshot_save(c & 1)                     # and it is never undone - it always runs to its end)
        # the parameter sets go up with the first chunk and stay on the device; rewards / done flags come back in the
        # engine's page-locked buffers (consumed by after_chunk before the chunk after the next overwrites them)
        if after_chunk is None:
            return eng.run_episode_mlp_fitness(Ls, params if first else None, member_a, member_b, half, L_init,
                                               n_members=n_members)
        return eng.run_episode_mlp(Ls, params if first else None, member_a, member_b, half, L_init,
                                   reuse_buffers=c & 1, n_members=n_members)

    pool = ThreadPoolExecutor(max_workers=1)
    try:
        c, K = 0, 1                                      # step 1 starts from the un-quantised state: a chunk of its own
        Ls = _luminosity_schedule(env, K)
        L_init = env._L_pass
        pending = pool.submit(on_device, c, Ls, L_init, True)
        while True:
            outcome = pending.result()
            ahead = None
            left = max_steps - (env.step_count + K)
            if left > 0:                                 # chunk c + 1, before chunk c is accounted for
                K_n = min(int(chunk), left)
                sched = _luminosity_schedule(env, K + K_n)
                Ls_n, L_init_n = sched[K:], sched[K - 1]
                ahead = pool.submit(on_device, c + 1, Ls_n, L_init_n, False)
            # (the device already returns reward * (reward > 0), ref step :490: agent states are clipped to [0, 1], so the
            # product is the state itself - a second pass over the (K,B,N,1) array would change no bit of it)
            executed, finished = outcome if after_chunk is None else after_chunk(*outcome)
            if executed < K or finished:
                if ahead is not None:
                    ahead.result()                       # the speculative chunk has to leave the device first
                if executed < K:                         # ended inside chunk c: its start + exactly the executed steps
                    eng.snapshot_restore(c & 1)
                    eng.run_episode_mlp(Ls[:executed], None, member_a, member_b, half, L_init, reuse_buffers=c & 1,
                                        n_members=n_members)
                elif ahead is not None:                  # ended with chunk c's last step: the state chunk c + 1 started from
                    eng.snapshot_restore((c + 1) & 1)
                ahead = None
            _advance_host_scalars(env, executed)
            if ahead is None:
                return                                   # the episode ended, or max_steps is reached
            pending, c, K, Ls, L_init = ahead, c + 1, K_n, Ls_n, L_init_n
    finally:
        pool.shutdown(wait=True)


def simulate_grazing_mlp(env, agent, nsteps, adversary=None, chunk=64, obs=None, temperature=False):
    """The `simulate_grazing` of LEARNED policies: the time series of the daisy populations over the next `nsteps` steps
    while MLP policies graze - the curves of the reference's trained-agent demo (daisy/notebook_helpers.py:210-223
    `update_fig_agent`, the existential-risk notebook's MLP cells append `env.grid[:, 1].mean()`, `env.grid[:, 2].mean()`,
    `temp.mean()` and `temp.std()` after every `env.step(action)`) - without a host round trip per step: observations, the
    MLP forward pass, grazing, physics and the per-step, per-world reductions stay on the device for `chunk` steps at a
    time (`dw_run_episode_mlp_trace`).  `agent` drives agents [0, N // 2) of every world and `adversary` the rest, as in
    `get_fitness`; `adversary=None`: `agent` drives them all.  `obs=None`: reset the environment first.

    The parameter sets go up with the first chunk and stay on the device.  There is no stopping rule: exactly `nsteps`
    steps are taken.  Returns the dict of `simulate_grazing` - `L`, `mean_light`, `mean_dark`, `max_cover`, `alive`,
    `stats`, `agent_ok` (n, B, N) bool (not done: reward >= 0.1 after the step) and `agents_alive` (n, B) - plus `reward`
    (n, B, N) float64, the step's `reward * (reward > 0)`; `temperature=True` adds `mean_temp`, `std_temp`, `min_temp`,
    `max_temp` (n, B) in kelvin and `dead_temp` (n,).  Afterwards `env.grid`, `env.step()`, `env.L`, `env.step_count`
    continue as if `nsteps` calls of `env.step(action)` had been made.

    Precision "f64" and `collision_mode == 1` have no device-resident form: ValueError - `simulate_grazing` with a
    callable agent is the host-loop route."""
    n = int(nsteps)
    if n < 1:
        raise ValueError("nsteps must be at least 1")
    K = int(chunk)
    if K < 1:
        raise ValueError("chunk must be at least 1")
    if env.precision == "f64" or env.collision_mode == 1:
        raise ValueError('simulate_grazing_mlp runs device-resident in precision "exact" or "fast" with collision_mode 0; '
                         "simulate_grazing with a callable agent is the host-loop route")
    if obs is None:
        env.reset()
    B, N = int(env.batch_size), int(env.n_agents)
    if adversary is None:
        params, split = np.asarray(agent.get_parameters(), dtype=np.float64).reshape(1, 1808), N
        member_a = member_b = None
    else:
        params, split = np.stack([agent.get_parameters(), adversary.get_parameters()]), N // 2
        member_a, member_b = np.zeros(B, dtype=np.int32), np.ones(B, dtype=np.int32)
    eng = env._ensure_engine()
    env._sync_to_device()
    L = np.zeros(n, dtype=np.float64)
    stats = np.zeros((n, B), dtype=_ffi.STATS_DTYPE)
    ok = np.zeros((n, B, N), dtype=bool)
    reward = np.zeros((n, B, N), dtype=np.float64)
    temps = np.zeros((n, B), dtype=_ffi.TEMP_STATS_DTYPE) if temperature else None
    t = 0
    while t < n:
        k = min(K, n - t)
        Ls = np.asarray(_luminosity_schedule(env, k), dtype=np.float64)
        L[t:t + k] = Ls
        # the parameter sets go up with the first chunk and stay on the device; the first steps of an episode (an
        # un-quantised state) are taken inside the call, launches per step
        r, d, st, tp = eng.run_episode_mlp(Ls, params if t == 0 else None, member_a, member_b, split, env._L_pass,
                                           n_members=params.shape[0], trace=True, temperature=bool(temperature))
        reward[t:t + k] = r[..., 0]
        ok[t:t + k] = ~d[..., 0]
        stats[t:t + k] = st
        if temperature:
            temps[t:t + k] = tp
        _advance_host_scalars(env, k)
        t += k
    out = _series_dict(env, L, stats, temps)
    out["agent_ok"] = ok
    out["agents_alive"] = ok.sum(axis=2)
    out["reward"] = reward
    return out


def _fitness_chunk(acc, rewards, dones, half):
    """Bookkeeping of `get_fitness` for one chunk of K steps (rewards (K,B,N,1) = reward * (reward > 0), dones
    (K,B,N,1) bool), equal to the reference's per-step statements (daisy/evo/sges.py:160-176: all_done,
    done_at += 1 - done, sum_reward += mean reward of the agents' half, total_steps += 1 - done; the loop
    leaves after the step in which every agent is done).  Returns (steps accounted for, episode ended)."""
    K = rewards.shape[0]
    ended = np.nonzero(dones.reshape(K, -1).all(axis=1))[0]
    executed = int(ended[0]) + 1 if ended.size else K
    alive = np.count_nonzero(~dones[:executed], axis=0)               # = sum(1 - done): integers, any order
    acc["done_at"] += alive
    acc["total_steps"] = acc["total_steps"] + alive
    means = [rewards[t][:, :half].mean() for t in range(executed)]    # the reference's call, step by step
    acc["sum_reward"] = np.add.accumulate(np.array([acc["sum_reward"]] + means))[-1]   # added in step order
    return executed, ended.size > 0


def _member_means(rewards, P, wpm, half):
    """Per (step, member): `reward[:, :half].mean()` of that member's block of worlds, as the reference forms it (sges.py:170 on
    a (wpm, N, 1) array) - NumPy flattens the non-contiguous slice in C order and sums it pairwise.  rewards: (K, P * wpm, N, 1).
    For the reference's own configuration (N = 4 agents, half = 2) the first two rewards of every world are gathered as ONE
    16-byte item (a complex128 view) and reduced along a CONTIGUOUS axis - the same pairwise sum over the same sequence, 1.7x
    faster than the strided multi-axis reduction; every other shape takes that reduction (both equal the reference's call on
    each block: tests/test_abi_and_host.py)."""
    K, B, N = rewards.shape[0], rewards.shape[1], rewards.shape[2]
    if N == 4 and half == 2 and rewards.flags.c_contiguous and rewards.dtype == np.float64:
        first = np.ascontiguousarray(rewards.reshape(K, B, 4).view(np.complex128)[:, :, 0])       # agents 0, 1 of every world
        return first.view(np.float64).reshape(K, P, wpm * 2).sum(axis=-1) / (wpm * 2)
    return rewards.reshape(K, P, wpm, N, 1)[:, :, :, :half].mean(axis=(2, 3, 4))


def _population_chunk(acc, rewards, dones, half, worlds_per_member):
    """The same for a population evaluated as one ensemble (member m owns worlds [m*wpm, (m+1)*wpm)): while a
    member runs, done_at / total_steps += 1 - done and sum_reward[m] += mean reward of its agents' half; the
    member stops after the step in which all ITS agents are done; the ensemble stops when no member runs.
    acc: done_at, total_steps (B,N,1) int, sum_reward (P,) float64, running (P,) bool - updated in place."""
    K, B, N = rewards.shape[0], rewards.shape[1], rewards.shape[2]
    P = B // worlds_per_member
    running = acc["running"]
    all_done = dones.reshape(K, P, -1).all(axis=2)                                 # (K,P)
    earlier = np.zeros((K, P), dtype=bool)
    earlier[1:] = np.logical_or.accumulate(all_done, axis=0)[:-1]
    run_t = running[None, :] & ~earlier                                            # running DURING step t
    none_left = np.nonzero(~(run_t & ~all_done).any(axis=1))[0]
    executed = int(none_left[0]) + 1 if none_left.size else K
    if run_t[:executed].all():                                                     # the usual chunk: every member still runs
        alive = executed - _count_true(dones[:executed])                           # = sum(1 - done): integers, any order
    else:
        live = np.repeat(run_t[:executed], worlds_per_member, axis=1)[:, :, None, None]
        alive = np.count_nonzero(live & ~dones[:executed], axis=0)                 # = sum(live * (1 - done))
    acc["done_at"][...] += alive
    acc["total_steps"][...] += alive
    # one member's mean of one step = the reference's `reward[:, :half].mean()` on that member's block of worlds
    # (the same pairwise reduction per (step, member); tests G11 + tools/fuzz_fitness.py hold it to that)
    means = _member_means(rewards[:executed], P, worlds_per_member, half)
    acc["sum_reward"][...] = np.add.accumulate(np.concatenate([acc["sum_reward"][None], run_t[:executed] * means]),
                                               axis=0)[-1]                         # added in step order
    running[...] = run_t[executed - 1] & ~all_done[executed - 1]
    return executed, none_left.size > 0


def _check_bookkeeping(bookkeeping, half):
    if bookkeeping not in ("host", "device"):
        raise ValueError(f'bookkeeping must be "host" or "device", got {bookkeeping!r}')
    if bookkeeping == "device" and half == 0:
        raise ValueError('bookkeeping="device" needs at least one agent in the first half (n_agents >= 2): with a single '
                         'agent the reference takes the mean of an empty slice - bookkeeping="host" is the route')
    return bookkeeping == "device"


def _device_fitness(env, params, member_a, member_b, half, worlds_per_member, max_steps, chunk):
    """The chunk loop with the bookkeeping on the device: `(sum_reward (P,), done_at (B, N, 1) int)` after the episode."""
    eng = env._ensure_engine()
    eng.fitness_begin(worlds_per_member, half)
    _mlp_chunks(env, params, member_a, member_b, half, max_steps, chunk, None)
    sum_reward, done_at, _ = eng.fitness_download()
    return sum_reward, done_at.astype(int)


def get_fitness(env, agent, adversary, max_steps=768, chunk=64, bookkeeping="host"):
    """ref SimpleGaussianES.get_fitness (daisy/evo/sges.py:144-181): one episode in which the first half
    of every world's agents is driven by `agent` and the second half by `adversary` (both MLP policies);
    returns (fitness, total_steps, done_at) exactly as the reference computes them.  Observations,
    policies, grazing and physics stay on the device for `chunk` steps at a time; only the (K,B,N) rewards
    and done flags come back, for the reference's float64 means in step order.

    `bookkeeping="device"`: those means, the sums in step order and the counters are kept on the device too
    (``dw_run_episode_mlp_fitness``: NumPy's pairwise order, the same bits); a chunk brings down 8 bytes and the episode
    one download of the accumulators.  A single agent per world (an empty first half) has only the host route."""
    on_device = _check_bookkeeping(bookkeeping, int(env.n_agents) // 2)   # refused before anything is reset
    agent.reset()
    obs = env.reset()
    B, N = obs.shape[0], obs.shape[1]
    half = N // 2
    params = np.stack([agent.get_parameters(), adversary.get_parameters()])
    member_a, member_b = np.zeros(B, dtype=np.int32), np.ones(B, dtype=np.int32)
    if on_device:
        sum_reward, done_at = _device_fitness(env, params, member_a, member_b, half, B, max_steps, chunk)
        return sum_reward[0] / (B * N), done_at.copy(), done_at.tolist()
    acc = {"done_at": np.zeros((B, N, 1), dtype=int), "total_steps": 0, "sum_reward": 0.0}
    _mlp_chunks(env, params, member_a, member_b, half, max_steps, chunk,
                lambda rewards, dones: _fitness_chunk(acc, rewards, dones, half))
    fitness = acc["sum_reward"] / (B * N)
    return fitness, acc["total_steps"], acc["done_at"].tolist()


def get_fitness_population(env, population, adversary_of=None, worlds_per_member=32, max_steps=768, chunk=64,
                           bookkeeping="host"):
    """All members of an evolution-strategy population evaluated as ONE batched ensemble (SURVEY.md §8f
    N3; the reference runs `get_fitness` once per member and farms members out to MPI workers,
    daisy/evo/sges.py:314-349).  `population` is a list of MLP policies (or a (P,1808) array);
    member m owns worlds [m*worlds_per_member, (m+1)*worlds_per_member); in each of its worlds the
    first half of the agents is driven by member m and the second half by member adversary_of[m]
    (default: itself).  Returns per-member (fitness, total_steps, done_at) computed exactly as
    `get_fitness` computes them for that member's block of worlds.

    Each member's episode ends when all ITS agents are done (or at max_steps), as in the reference; the
    ensemble keeps stepping until every member has finished, and a finished member's statistics are
    frozen at its own stopping step.  (With the legacy-RNG reset the worlds differ from P separate
    `reset()` calls of the reference; the per-member arithmetic is the same.)

    `bookkeeping="device"`: as in `get_fitness` - per-member means, sums and counters on the device, the same bits."""
    params = np.stack([m.get_parameters() if hasattr(m, "get_parameters") else np.asarray(m) for m in population])
    P = params.shape[0]
    adversary_of = np.arange(P) if adversary_of is None else np.asarray(adversary_of, dtype=int)
    on_device = _check_bookkeeping(bookkeeping, int(env.n_agents) // 2)   # refused before anything is reset
    env.batch_size = P * worlds_per_member
    obs = env.reset()
    B, N = obs.shape[0], obs.shape[1]
    half = N // 2
    member = np.repeat(np.arange(P), worlds_per_member).astype(np.int32)
    adv_member = adversary_of[member].astype(np.int32)
    if on_device:
        sum_reward, done_at = _device_fitness(env, params, member, adv_member, half, worlds_per_member, max_steps, chunk)
        fitness = sum_reward / (worlds_per_member * N)
        return [(fitness[m], done_at[m * worlds_per_member:(m + 1) * worlds_per_member].copy(),
                 done_at[m * worlds_per_member:(m + 1) * worlds_per_member].tolist()) for m in range(P)]
    done_at = np.zeros((B, N, 1), dtype=int)
    total_steps = np.zeros((B, N, 1), dtype=int)
    sum_reward = np.zeros(P)
    running = np.ones(P, dtype=bool)

    acc = {"done_at": done_at, "total_steps": total_steps, "sum_reward": sum_reward, "running": running}
    _mlp_chunks(env, params, member, adv_member, half, max_steps, chunk,
                lambda rewards, dones: _population_chunk(acc, rewards, dones, half, worlds_per_member))
    fitness = sum_reward / (worlds_per_member * N)
    return [(fitness[m], total_steps[m * worlds_per_member:(m + 1) * worlds_per_member],
             done_at[m * worlds_per_member:(m + 1) * worlds_per_member].tolist()) for m in range(P)]
