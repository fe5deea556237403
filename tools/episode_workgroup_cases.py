#!/usr/bin/env python3
"""The workgroup episode kernels (csrc/dw_episode.hpp: episode_small, episode_mlp) above 256 cells: ONE table of cases,
their deterministic inputs and their float64 oracle references, shared by tests/test_episode_workgroup_cases_cpu.py (keeps
the table honest on the oracle alone: worlds alive, agents grazing and dying, logit margins) and
tests/test_gpu_episode_workgroup.py (holds the kernels to these references).  Pure NumPy plus oracle/: no GPU code.

What the shapes are for - the kernels keep `wpb` worlds per 256-thread workgroup, `tpw = 256 / wpb` threads per world:
  C <= 256           wpb = 4, tpw = 64   one wave serves a world (covered by tests/test_gpu_episode_wave.py)
  256 < C <= 1024    wpb = 2, tpw = 128  two waves per world: reductions cross waves through LDS atomics, B odd leaves
                                         a workgroup with an invalid half that still crosses every barrier
  1024 < C <= 4096   wpb = 1, tpw = 256  four waves per world; 64 x 64 needs more than 64 KiB of dynamic LDS
  C > 4096           launches per step

Inputs of a case come from np.random.RandomState(seed of the case): planes np.round(rand * 0.4, 3), uniform agent
positions, agent states 0.5.  Protocol of every case (the GPU test's half is in brackets):
  1. [upload_state_f32(light, dark, quantised=True)]   the oracle world is built by set_initial_cover
  2. [upload_agents]
  3. one zero-action step at L0 = 0.94                  current and retained previous state are then quantised: the LDS
                                                        kernel takes every step of the call, the MLP one included
  4. the call under test.

References are cached per case in module dicts, their arrays read-only: the forms of one case (default,
DW_NO_EPISODE_KERNEL) and its run lengths (prefixes of one oracle run) share one reference.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constant_edge_cases as E  # noqa: E402
from oracle import c_oracle, daisy_oracle as O  # noqa: E402

WAVE, WORKGROUP, STEPWISE = "one wave per world", "workgroup (LDS)", "launches per step"
THRESHOLD_K = 5
L0 = 0.94
MAX_CELLS = 4096                                                 # episode_form / episode_mlp_form: C <= 4096
LDS_LIMIT = 160 * 1024
FIX_CAP = 240                                                    # kEpFixCap: the near-tie list of a world and step


def worlds_per_block(C):
    """worlds_per_block of dw_api.hip"""
    return 4 if C <= 256 else (2 if C <= 1024 else 1)


def threads_per_world(C):
    return 256 // worlds_per_block(C)


def episode_world_bytes(C, N):
    """episode_world_bytes of dw_episode.hpp: planes | agent states | idx, act | 8 reduction words | the near-tie list"""
    return (16 * C + N * 8 + N * 12 + 32 + 2 * FIX_CAP + 15) // 16 * 16


def episode_mlp_world_bytes(C, N):
    """episode_mlp_world_bytes of dw_episode.hpp: per agent state, idx, act and 128 doubles of network activations"""
    return (16 * C + N * (8 + 8 + 4 + 8 * 128) + 32 + 2 * FIX_CAP + 15) // 16 * 16


def largest_mlp_agents(C):
    """The largest N episode_mlp_form still hands to the workgroup kernel for worlds of C cells."""
    N = 0
    while episode_mlp_world_bytes(C, N + 1) * worlds_per_block(C) <= LDS_LIMIT:
        N += 1
    return N


def k_of(x):
    return np.rint(np.asarray(x) * 1000.0).astype(np.int64)


def _freeze(x):
    """The arrays of a cached reference are shared by every test that asks for it: read-only."""
    if isinstance(x, np.ndarray):
        x.flags.writeable = False
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _freeze(v)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# the oracle helpers of tests/test_gpu_episode_wave.py (copied: that file stays as it is)
# ---------------------------------------------------------------------------------------------------------------------
def oracle_env(light, dark, idx, st, L, agent_gamma=None, over=None):
    """Oracle environment (H x W through set_initial_cover) holding the given planes and agents; `over`: physics constants
    that differ from the defaults (the names of tools/constant_edge_cases.py)."""
    B, H, W = light.shape
    N = idx.shape[1]
    env = O.OracleDaisyWorldC(grid_dimension=max(H, W), n_agents=N, batch_size=B)
    if agent_gamma is not None:
        env.P.agent_gamma = agent_gamma
    for k, v in (over or {}).items():
        assert hasattr(env.P, k), k
        setattr(env.P, k, v)
    env.L = L
    env.set_initial_cover(np.array(light, dtype=np.float64), np.array(dark, dtype=np.float64))
    assert env.shape == (H, W)
    env.agent_indices = np.array(idx, dtype=np.int64)
    env.agent_states = np.array(st, dtype=np.float64).reshape(B, N, 1)
    return env


def oracle_step(env, L, action):
    """One reference step at luminosity L (ref :475-497).  Returns (reward, done, light, dark) - the covers as forward
    read them: after the agents grazed, which is the engine's retained previous state."""
    env.L = L
    kept = {}
    inner = env.forward

    def forward(grid):
        kept["light"], kept["dark"] = grid[:, O.CH_LIGHT].copy(), grid[:, O.CH_DARK].copy()
        return inner(grid)

    env.forward = forward
    try:
        _, reward, done, _ = env.step(np.asarray(action).reshape(env.P.batch_size, env.P.n_agents, 1).astype(np.int64))
    finally:
        del env.forward
    return reward, done, kept["light"], kept["dark"]


def resolve_codes(env, codes):
    """Table codes -> actions on the oracle: -1 / -2 are the greedy / anti-greedy choice of that agent
    (ref Greedy.__call__, agents/greedy.py:25-30, epsilon = 0)."""
    obs = env.get_obs(env.agent_indices)
    g1 = O.OracleGreedy(epsilon=0.0, greedy=True)(obs)
    g2 = O.OracleGreedy(epsilon=0.0, greedy=False)(obs)
    c = codes.astype(np.int64)[..., None]
    return np.where(c == -1, g1, np.where(c == -2, g2, c))


def max_k(env):
    return np.maximum(k_of(env.grid[:, 1]).max(axis=(1, 2)), k_of(env.grid[:, 2]).max(axis=(1, 2)))


def final_state(env, prev_light, prev_dark, reward, done, action):
    """Everything the engine can be asked for after the call, from the oracle."""
    kl, kd = k_of(env.grid[:, 1]), k_of(env.grid[:, 2])
    return {"light": kl, "dark": kd, "prev_light": k_of(prev_light), "prev_dark": k_of(prev_dark),
            "idx": env.agent_indices.copy(), "st": env.agent_states.copy(), "reward": reward.copy(), "done": done.copy(),
            "obs": env.get_obs(env.agent_indices), "action": np.asarray(action)[..., 0].astype(np.int64),
            "max_k": np.maximum(kl.max(axis=(1, 2)), kd.max(axis=(1, 2))).astype(np.uint32),
            "sum_light_k": kl.sum(axis=(1, 2)).astype(np.uint64), "sum_dark_k": kd.sum(axis=(1, 2)).astype(np.uint64)}


def quantise(env):
    """The protocol's step 3 on the oracle.  Returns the state the call under test starts from: per-mille planes, agent
    positions and states - the GPU test asserts the engine holds the same."""
    zeros = np.zeros((env.P.batch_size, env.P.n_agents, 1), dtype=np.int64)
    oracle_step(env, L0, zeros)
    return {"light": k_of(env.grid[:, 1]), "dark": k_of(env.grid[:, 2]), "idx": env.agent_indices.copy(),
            "st": env.agent_states[..., 0].copy()}


def start_inputs(shape, seed):
    """(light, dark, idx, st, rng) of a case: `rng` goes on to draw the case's action tables / parameter sets."""
    B, H, W, N = shape
    rng = np.random.RandomState(seed)
    light = np.round(rng.rand(B, H, W) * 0.4, 3)
    dark = np.round(rng.rand(B, H, W) * 0.4, 3)
    idx = np.stack([rng.randint(H, size=(B, N)), rng.randint(W, size=(B, N))], axis=-1).astype(np.int32)
    st = np.full((B, N), 0.5)
    return light, dark, idx, st, rng


# ---------------------------------------------------------------------------------------------------------------------
# A. dw_run_episode
# ---------------------------------------------------------------------------------------------------------------------
#           B, H,  W,    N       what it pins
SHAPES_A = [(5, 17, 17, 3),      # C = 289: the first shape beyond the wave form; wpb = 2, B odd: an invalid half
            (3, 32, 32, 5),      # C = 1024: the last wpb = 2 shape
            (3, 25, 41, 7),      # C = 1025: the first wpb = 1 shape, four waves per world, odd W
            (2, 3, 1365, 5),     # C = 4095: the minimal dimension with row wrap
            (2, 1365, 3, 5),     # ... and with column wrap
            (2, 63, 65, 4),      # C = 4095: just under the limit
            (3, 64, 64, 6),      # C = 4096: the limit; more than 64 KiB of dynamic LDS
            (2, 20, 20, 130)]    # N > tpw = 128: the agent loops take a second trip; agents meet on cells
CROWDED = (2, 20, 20, 130)
DISPATCH_A = (1, 17, 241, 2)     # C = 4097: launches per step
KS_A = (1, 2, 41)                # both ping-pong parities end a run
K_A = max(KS_A)
STARVE_STEPS = 20                # steps 1 .. 20 of argmin+use_table take the table (see inputs_a)
POLICIES = ("table", "argmin+use_table")
# frozen: chosen on the CPU so that every condition of tests/test_episode_workgroup_cases_cpu.py holds
SEEDS_A = {s: 3000 + i for i, s in enumerate(SHAPES_A)}

assert all(256 < s[1] * s[2] <= MAX_CELLS for s in SHAPES_A) and DISPATCH_A[1] * DISPATCH_A[2] == MAX_CELLS + 1
assert CROWDED[3] > threads_per_world(CROWDED[1] * CROWDED[2]) == 128


def schedule_a(K=K_A):
    """A gentle ramp through the daisies' comfortable range: worlds live, agents graze."""
    return 0.95 + 0.002 * np.arange(K, dtype=np.float64)


_INPUTS_A = {}


def inputs_a(shape):
    """The inputs of a case, a function of its seed alone: planes, agents, and the K_A-step tables every run length takes
    its first rows of - `codes` (K_A, B, N) int8 from -2 .. 8 and `use_table` (K_A,) uint8 for the policy
    argmin+use_table (step 0 anti-greedy, steps 1 .. STARVE_STEPS from the table: K = 2 holds one of each; a random 40 %
    of the rest), `moves` from 0 .. 8 for the
    float32-only mode (explicit moves: no decision rides on a float32 value)."""
    if shape not in _INPUTS_A:
        B, H, W, N = shape
        light, dark, idx, st, rng = start_inputs(shape, SEEDS_A[shape])
        codes = rng.randint(-2, 9, size=(K_A, B, N)).astype(np.int8)
        ut = (rng.rand(K_A) < 0.4).astype(np.uint8)
        ut[0], ut[1:STARVE_STEPS + 1] = 0, 1
        moves = rng.randint(9, size=(K_A, B, N)).astype(np.int8)
        # Random tables graze at every other step and nobody starves in 41 steps.  Agent 0 of world 0 is given moves that
        # never graze (5 .. 8 and the greedy codes become 1 .. 4): from a state of at most 1.0 it is dead - and, dead,
        # no longer moves - after twenty table steps, which is why use_table is set for steps 1 .. 20.
        for tab in (codes, moves):
            mine = tab[:, 0, 0]
            tab[:, 0, 0] = np.where(mine > 4, mine - 4, np.where(mine < 0, 4, mine))
        _INPUTS_A[shape] = _freeze({"light": light, "dark": dark, "idx": idx, "st": st, "codes": codes, "use_table": ut,
                                    "moves": moves})
    return _INPUTS_A[shape]


_REF_A = {}


def reference_a(shape, policy):
    """The oracle's K_A steps of a case under `policy`, computed once: `start` (the state after the quantising step),
    `alive` (K_A, B), `ok` (K_A, B, N), `reward` (K_A, B, N), `crowded` (K_A,) - two agents that moved share a cell -,
    `final[K]` for K in KS_A (what _compare_final compares after a run of K steps), `seconds`."""
    key = (shape, policy)
    if key in _REF_A:
        return _REF_A[key]
    assert policy in POLICIES
    t0 = time.perf_counter()
    B, H, W, N = shape
    inp = inputs_a(shape)
    env = oracle_env(inp["light"], inp["dark"], inp["idx"], inp["st"], L0)
    start = quantise(env)
    codes, ut = inp["codes"], (None if policy == "table" else inp["use_table"])
    Ls = schedule_a()
    alive, ok = np.zeros((K_A, B), dtype=bool), np.zeros((K_A, B, N), dtype=bool)
    rewards, crowded, final = np.zeros((K_A, B, N)), np.zeros(K_A, dtype=bool), {}
    for t in range(K_A):
        c = codes[t] if (ut is None or ut[t]) else np.full((B, N), -2, dtype=np.int8)      # POLICY_ARGMIN: anti-greedy
        action = resolve_codes(env, c)
        moved = env.agent_states[..., 0] - env.P.agent_gamma > 0.0                         # update_agents moves these
        reward, done, pl, pd = oracle_step(env, Ls[t], action)
        alive[t] = max_k(env) > THRESHOLD_K
        ok[t] = ~done[..., 0]
        rewards[t] = reward[..., 0]
        for b in range(B):
            cells = env.agent_indices[b, moved[b], 0] * W + env.agent_indices[b, moved[b], 1]
            crowded[t] |= len(np.unique(cells)) < len(cells)
        if t + 1 in KS_A:
            final[t + 1] = final_state(env, pl, pd, reward, done, action)
    ref = {"start": start, "alive": alive, "ok": ok, "reward": rewards, "crowded": crowded, "final": final,
           "max_k": max_k(env)}
    ref = _freeze(ref)
    ref["seconds"] = time.perf_counter() - t0
    _REF_A[key] = ref
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# agent-free dw_step_n on workgroup shapes
# ---------------------------------------------------------------------------------------------------------------------
STEP_N_SHAPES = [(5, 17, 17), (3, 25, 41), (2, 63, 65)]
STEP_N_AGENTS, STEP_N_STEPS = 3, 42                              # the first by the step kernel, 41 by episode_small
STEP_N_L, STEP_N_DL, STEP_N_RANGE = 0.9, 0.002, (0.75, 1.5)


def inputs_step_n(shape):
    """An UN-quantised float64 state (rand * 0.4, not rounded) and 3 agents per world, which the run must not touch."""
    B, H, W = shape
    rng = np.random.RandomState(4000 + 131 * H + W)
    light, dark = rng.rand(B, H, W) * 0.4, rng.rand(B, H, W) * 0.4
    idx = np.stack([rng.randint(H, size=(B, STEP_N_AGENTS)), rng.randint(W, size=(B, STEP_N_AGENTS))], axis=-1).astype(np.int32)
    return light, dark, idx, np.full((B, STEP_N_AGENTS), 0.5)


_REF_STEP_N = {}


def reference_step_n(shape):
    """(light, dark per-mille after STEP_N_STEPS steps, the luminosity c_oracle.step_n returns)"""
    if shape not in _REF_STEP_N:
        light, dark, _, _ = inputs_step_n(shape)
        L = c_oracle.step_n(light, dark, STEP_N_L, STEP_N_DL, STEP_N_STEPS, *STEP_N_RANGE)
        _REF_STEP_N[shape] = _freeze((k_of(light), k_of(dark), L))
    return _REF_STEP_N[shape]


# ---------------------------------------------------------------------------------------------------------------------
# the near-tie list overflow of ep_forward
# ---------------------------------------------------------------------------------------------------------------------
OVERFLOW_NAME = "To=800 g=2e-6"                                  # inadmissible: every cell of every step is flagged
#                 constants,     B, H,  W,  N
OVERFLOW_CASES = [(OVERFLOW_NAME, (3, 32, 32, 2)),               # wpb = 2: 1024 flagged cells per world, 240 listed
                  (OVERFLOW_NAME, (2, 40, 40, 2)),               # wpb = 1: 1600
                  (None, (3, 32, 32, 2))]                        # the defaults: a few near ties, the list never fills
OVERFLOW_K = 6
assert not any(E.BY_NAME[OVERFLOW_NAME]["admissible"]) and len(E.BY_NAME[OVERFLOW_NAME]["L"]) == OVERFLOW_K
assert all(s[1] * s[2] > FIX_CAP for _, s in OVERFLOW_CASES)


def overflow_schedule(name):
    """That case's own schedule (0.6 .. 1.7 in six steps); with the default constants nothing lives through it - no cover,
    no near tie to count -, so the defaults run over the first six steps of schedule_a."""
    return np.array(E.BY_NAME[name]["L"], dtype=np.float64) if name else schedule_a(OVERFLOW_K)


def overflow_constants(name):
    return dict(E.BY_NAME[name]["over"]) if name else {}


def inputs_overflow(name, shape):
    B, H, W, N = shape
    light, dark, idx, st, rng = start_inputs(shape, 5000 + H + (1 if name else 0))
    codes = rng.randint(-2, 9, size=(OVERFLOW_K, B, N)).astype(np.int8)
    return _freeze({"light": light, "dark": dark, "idx": idx, "st": st, "codes": codes})


_REF_OVERFLOW = {}


def reference_overflow(name, shape):
    """OVERFLOW_K table-policy steps over overflow_schedule(name) with the constants of `name` (None: the defaults): `start`,
    `alive`, `ok`, `final`, and `first` - the planes the run started from, which the CPU test wants changed."""
    key = (name, shape)
    if key in _REF_OVERFLOW:
        return _REF_OVERFLOW[key]
    t0 = time.perf_counter()
    B, H, W, N = shape
    inp = inputs_overflow(name, shape)
    env = oracle_env(inp["light"], inp["dark"], inp["idx"], inp["st"], L0, over=overflow_constants(name))
    start = quantise(env)
    Ls = overflow_schedule(name)
    alive, ok = np.zeros((OVERFLOW_K, B), dtype=bool), np.zeros((OVERFLOW_K, B, N), dtype=bool)
    for t in range(OVERFLOW_K):
        action = resolve_codes(env, inp["codes"][t])
        reward, done, pl, pd = oracle_step(env, Ls[t], action)
        alive[t] = max_k(env) > THRESHOLD_K
        ok[t] = ~done[..., 0]
    ref = _freeze({"start": start, "alive": alive, "ok": ok, "final": final_state(env, pl, pd, reward, done, action),
                   "max_k": max_k(env)})
    ref["seconds"] = time.perf_counter() - t0
    _REF_OVERFLOW[key] = ref
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# B. dw_run_episode_mlp
# ---------------------------------------------------------------------------------------------------------------------
#             B, H,  W,  N, split
SHAPES_B = [(3, 17, 17, 4, 2),      # four agents, but no longer the wave form
            (3, 32, 32, 9, 4),      # tpw = 128: ngrp = 8 agents per pass; N = ngrp + 1: the second pass has one live group
            (2, 25, 41, 5, 2),      # wpb = 1, ngrp = 16
            (2, 64, 64, 17, 8)]     # N = ngrp + 1 at the cell limit
LDS_EDGE_B = [(2, 64, 64, 93, 46),  # 163 152 B of 163 840
              (2, 32, 32, 62, 31)]  # 2 x 81 632 B
DISPATCH_B = [(1, 64, 64, 94, 47), (2, 32, 32, 63, 31)]          # one agent more: launches per step
KS_B = (3, 20)
K2_B = 5                                                         # the second chunk (params=None)
KS_EDGE_B = (3,)
MLP_AGENT_GAMMA = 0.005                                          # as tests/test_gpu_episode_wave.py: the agents move to the end
MARGIN = 1e-9
N_MEMBERS = 3
# frozen: the first seed from 6000 at which every condition of tests/test_episode_workgroup_cases_cpu.py holds
SEEDS_B = {(3, 17, 17, 4, 2): 6000, (3, 32, 32, 9, 4): 6000, (2, 25, 41, 5, 2): 6001, (2, 64, 64, 17, 8): 6000,
           (2, 64, 64, 93, 46): 6000, (2, 32, 32, 62, 31): 6000}

assert largest_mlp_agents(64 * 64) == 93 == LDS_EDGE_B[0][3] and largest_mlp_agents(32 * 32) == 62 == LDS_EDGE_B[1][3]
assert episode_mlp_world_bytes(4096, 93) == 163152 and episode_mlp_world_bytes(1024, 62) == 81632
assert all(e[3] + 1 == d[3] and e[1:3] == d[1:3] for e, d in zip(LDS_EDGE_B, DISPATCH_B))
assert SHAPES_B[1][3] == threads_per_world(1024) // 16 + 1 and SHAPES_B[3][3] == threads_per_world(4096) // 16 + 1


def ks_b(shape):
    return KS_EDGE_B if shape in LDS_EDGE_B else KS_B


def mlp_schedule(K, start=0):
    return 0.95 + 0.003 * np.arange(start, start + K, dtype=np.float64)


def members(B):
    """member_a / member_b: different sets for the two halves of every world"""
    return (np.arange(B) % N_MEMBERS).astype(np.int32), ((np.arange(B) + 1) % N_MEMBERS).astype(np.int32)


_INPUTS_B = {}


def inputs_b(shape):
    if shape not in _INPUTS_B:
        B, H, W, N, split = shape
        light, dark, idx, st, rng = start_inputs(shape[:4], SEEDS_B[shape])
        params = rng.randn(N_MEMBERS, 1808) * 0.3
        ma, mb = members(B)
        assert (ma != mb).any()
        _INPUTS_B[shape] = _freeze({"light": light, "dark": dark, "idx": idx, "st": st, "params": params, "member_a": ma,
                                    "member_b": mb})
    return _INPUTS_B[shape]


_REF_B = {}


def reference_b(shape):
    """The oracle's max(ks) + K2_B steps of a case with OracleMLP policies (agents [0, split) of world b: set
    member_a[b], the rest member_b[b]), computed once.  A run of K steps and its second chunk of K2_B steps are the
    steps [0, K) and [K, K + K2_B) of this one run: the schedule continues.  `reward` / `done` (T, B, N, 1), `action`
    (T, B, N), `swapped` (T, B, N) - what the OTHER half's parameter set of that world would have chosen from the same
    observation: where it differs, an agent handed the wrong set shows -, `margin` (T,) - the least distance of the two largest logits of a decision of that step: the device
    accumulates every dot product sequentially with fma, NumPy by matmul -, `final[t]` after t steps for every t a chunk
    ends at, `start`, `seconds`."""
    if shape in _REF_B:
        return _REF_B[shape]
    t0 = time.perf_counter()
    B, H, W, N, split = shape
    inp = inputs_b(shape)
    nets = [O.OracleMLP(p) for p in inp["params"]]
    env = oracle_env(inp["light"], inp["dark"], inp["idx"], inp["st"], L0, agent_gamma=MLP_AGENT_GAMMA)
    start = quantise(env)
    ends = sorted({K for K in ks_b(shape)} | {K + K2_B for K in ks_b(shape)})
    T = ends[-1]
    Ls = mlp_schedule(T)
    rewards, dones = np.zeros((T, B, N, 1)), np.zeros((T, B, N, 1), dtype=bool)
    actions, margin, final = np.zeros((T, B, N), dtype=np.int64), np.zeros(T), {}
    swapped = np.zeros((T, B, N), dtype=np.int64)
    obs = env.get_obs(env.agent_indices)
    for t in range(T):
        action = np.zeros((B, N, 1), dtype=np.int64)
        least = np.inf
        for b in range(B):
            for n in range(N):
                net, other = nets[inp["member_a"][b]], nets[inp["member_b"][b]]
                if n >= split:
                    net, other = other, net
                logits = net.forward(obs[b, n].reshape(63))
                swapped[t, b, n] = int(np.argmax(other.forward(obs[b, n].reshape(63))))
                top = np.sort(logits)
                least = min(least, top[-1] - top[-2])
                action[b, n, 0] = int(np.argmax(logits))
        margin[t], actions[t] = least, action[..., 0]
        reward, done, pl, pd = oracle_step(env, Ls[t], action)
        rewards[t], dones[t] = reward, done
        obs = env.get_obs(env.agent_indices)
        if t + 1 in ends:
            final[t + 1] = final_state(env, pl, pd, reward, done, action)
    ref = _freeze({"start": start, "reward": rewards, "done": dones, "action": actions, "swapped": swapped, "margin": margin,
                   "final": final})
    ref["seconds"] = time.perf_counter() - t0
    _REF_B[shape] = ref
    return ref
