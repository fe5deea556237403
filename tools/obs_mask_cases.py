#!/usr/bin/env python3
"""The agent kernels under observation masks other than the default (dw_params.obs_mask, the reference's
neighborhood_mode): ONE table of cases, their deterministic inputs and their float64 oracle references, shared by
tests/test_obs_mask_cases_cpu.py (keeps the table honest on the oracle alone: the mask changes decisions, worlds live,
agents graze, MLP margins) and tests/test_gpu_obs_masks.py (holds the kernels to these references).  Pure NumPy plus
oracle/: no GPU code.

A mask is 9 bits, row-major over the 3 x 3 patch (bit k = patch cell k, engine.mask_bits).  The greedy policies read the
cross cells 3, 1, 7, 5 (west, north, south, east) in that order: a masked candidate counts as 0.0, so np.argmin takes the
first masked one and np.argmax skips it.  The corners 0, 2, 6, 8 are visible to nothing but an MLP.

Protocol of every case (that of tools/episode_workgroup_cases.py, whose helpers are used): upload quantised planes and
agents drawn from RandomState(seed of the case), one zero-action step at L0, then the call under test - on the oracle
with `env.neighborhood = mask_array(mask)`.

The greedy policies of the exact cases: "argmax" and "argmin" are DW_POLICY_ARGMAX / DW_POLICY_ARGMIN with a use_table
that hands about a third of the steps (never the first, never the last) to the table of explicit codes - under a mask
that hides all four candidates a purely greedy agent walks west for ever (action 4) and never grazes, and the condition
"an agent grazes" could not hold; "table" is DW_POLICY_TABLE with codes -2 .. 8.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import episode_workgroup_cases as W  # noqa: E402
from oracle import daisy_oracle as O  # noqa: E402

WAVE, WORKGROUP, STEPWISE = W.WAVE, W.WORKGROUP, W.STEPWISE
PAIRS = "dw_step_n fuses step pairs"                             # kernel_info() of a handle whose plan allows step pairs
THRESHOLD_K, L0, MARGIN = W.THRESHOLD_K, W.L0, W.MARGIN
k_of = W.k_of

VON_NEUMANN, MOORE = 0x0BA, 0x1FF
MASKS = (0x1FF,      # Moore
         0x0B2,      # cross without west: the first candidate is masked
         0x09A,      # cross without east: the last candidate is masked
         0x155,      # corners and centre: every candidate masked, corners on
         0x1EF,      # everything but the centre
         0x010)      # centre only
GREEDY_MASKS = MASKS + (0x000,)                                  # nothing visible: an MLP would see all-equal logits
CANDIDATES = (3, 1, 7, 5)
CORNERS = (0, 2, 6, 8)


def mask_array(mask):
    """9-bit mask -> the 3 x 3 float64 0/1 array `env.neighborhood` holds (the inverse of engine.mask_bits)."""
    return np.array([(mask >> k) & 1 for k in range(9)], dtype=np.float64).reshape(3, 3)


def bits_of(array):
    """engine.mask_bits, restated: row-major, bit k = cell k."""
    return int(sum(1 << k for k, v in enumerate(np.asarray(array).ravel()) if v))


def hides_a_candidate(mask):
    return any(not (mask >> k) & 1 for k in CANDIDATES)


def shows_a_corner(mask):
    return any((mask >> k) & 1 for k in CORNERS)


_VN = mask_array(VON_NEUMANN)


def full_obs(env):
    """The un-masked observations of the oracle's agents (the mask is a plain product in get_obs)."""
    kept = env.neighborhood
    env.neighborhood = np.ones((3, 3))
    try:
        return env.get_obs(env.agent_indices)
    finally:
        env.neighborhood = kept


def greedy_actions(obs, codes):
    """Codes (B, N) -> actions (B, N, 1) on the observations `obs`: -1 / -2 the greedy / anti-greedy choice."""
    g1 = O.OracleGreedy(epsilon=0.0, greedy=True)(obs)
    g2 = O.OracleGreedy(epsilon=0.0, greedy=False)(obs)
    c = np.asarray(codes).astype(np.int64)[..., None]
    return np.where(c == -1, g1, np.where(c == -2, g2, c))


def masked_env(inp, mask, agent_gamma=None):
    env = W.oracle_env(inp["light"], inp["dark"], inp["idx"], inp["st"], L0, agent_gamma=agent_gamma)
    env.neighborhood = mask_array(mask)
    return env


# ---------------------------------------------------------------------------------------------------------------------
# 1 - 3. dw_run_episode and the record-keeping wave kernels
# ---------------------------------------------------------------------------------------------------------------------
#                B, H,  W,  N
WAVE_SHAPES = [(5, 3, 3, 2),         # every neighbour wraps
               (3, 5, 13, 4),
               (9, 4, 64, 4),
               (4, 8, 8, 64)]        # agents share cells
WORKGROUP_SHAPES = [(3, 17, 17, 3), (2, 25, 41, 5)]
WIDE_SHAPES = [(2, 40, 256, 3), (1, 70, 320, 2)]                 # launches per step; agent step pairs (agents_lookahead_patch)
SHAPES_1 = WAVE_SHAPES + WORKGROUP_SHAPES + WIDE_SHAPES
KS = (1, 65)                                                     # 65: one run crosses the 64-step segment seam
K_MAX = max(KS)
POLICIES = ("argmax", "argmin", "table")
RECORD_SHAPES = [(5, 3, 3, 2), (3, 5, 13, 4)]
RECORD_MASKS = (0x1FF, 0x0B2, 0x155)
# frozen: the first seed from 7000 at which every condition of tests/test_obs_mask_cases_cpu.py holds
SEEDS_1 = {(5, 3, 3, 2): 7001, (3, 5, 13, 4): 7001, (9, 4, 64, 4): 7000, (4, 8, 8, 64): 7000, (3, 17, 17, 3): 7000,
           (2, 25, 41, 5): 7000, (2, 40, 256, 3): 7001, (1, 70, 320, 2): 7004}


def form_of(shape):
    C = shape[1] * shape[2]
    return WAVE if C <= 256 and shape[3] <= 64 else (WORKGROUP if C <= W.MAX_CELLS else STEPWISE)


def masks_of_group(masks):
    """The masks of a group, and the default once: it ties the references to the ones the existing tests hold."""
    return tuple(masks) + (VON_NEUMANN,)


def schedule(K=K_MAX, start=0):
    return 0.95 + 0.002 * np.arange(start, start + K, dtype=np.float64)


_INPUTS_1 = {}


def inputs_1(shape):
    """Planes, agents, `codes` (K_MAX, B, N) int8 from -2 .. 8, `explicit` (the same with the greedy codes replaced by
    moves 5 .. 8: what "argmax" / "argmin" take at their table steps) and `use_table` (K_MAX,) uint8: about a third of
    the steps, step 63 among them, never the first nor the last (a K = 1 run and every run's last action are greedy)."""
    if shape not in _INPUTS_1:
        B, H, Wd, N = shape
        light, dark, idx, st, rng = W.start_inputs(shape, SEEDS_1[shape])
        codes = rng.randint(-2, 9, size=(K_MAX, B, N)).astype(np.int8)
        codes[0] = (-1 - np.arange(B * N) % 2).reshape(B, N)     # step 0: greedy and anti-greedy in turn (the K = 1 run decides)
        explicit = np.where(codes < 0, (codes + 7).astype(np.int8), codes).astype(np.int8)     # -2, -1 -> 5, 6
        ut = (rng.rand(K_MAX) < 0.33).astype(np.uint8)
        ut[0], ut[63], ut[K_MAX - 1] = 0, 1, 0
        _INPUTS_1[shape] = W._freeze({"light": light, "dark": dark, "idx": idx, "st": st, "codes": codes,
                                      "explicit": explicit, "use_table": ut})
    return _INPUTS_1[shape]


def call_of(shape, policy, K):
    """(policy mode name, use_table, table) of dw_run_episode for `policy`."""
    inp = inputs_1(shape)
    if policy == "table":
        return "TABLE", None, inp["codes"][:K]
    return policy.upper(), inp["use_table"][:K], inp["explicit"][:K]


def step_codes(shape, policy, t):
    inp = inputs_1(shape)
    if policy == "table":
        return inp["codes"][t]
    if inp["use_table"][t]:
        return inp["explicit"][t]
    return np.full(shape[::3], -1 if policy == "argmax" else -2, dtype=np.int8)


_REF_1 = {}


def reference_1(shape, mask, policy):
    """The oracle's K_MAX steps of a case: `start`, `alive` (K, B), `ok` (K, B, N), `action` (K, B, N), `final[K]` for K
    in KS, `differs` (K,) - a live agent's greedy decision of that step is not the one the von Neumann mask would have
    given on the same cells -, `grazed` (K,) - an agent's state rose at that step -, `seconds`."""
    key = (shape, mask, policy)
    if key in _REF_1:
        return _REF_1[key]
    t0 = time.perf_counter()
    B, H, Wd, N = shape
    inp = inputs_1(shape)
    env = masked_env(inp, mask)
    start = W.quantise(env)
    here = mask_array(mask)
    Ls = schedule()
    alive, ok = np.zeros((K_MAX, B), dtype=bool), np.zeros((K_MAX, B, N), dtype=bool)
    actions = np.zeros((K_MAX, B, N), dtype=np.int64)
    differs, grazed, final = np.zeros(K_MAX, dtype=bool), np.zeros(K_MAX, dtype=bool), {}
    for t in range(K_MAX):
        c = step_codes(shape, policy, t)
        obs = full_obs(env)
        action = greedy_actions(obs * here, c)
        other = greedy_actions(obs * _VN, c)
        before = env.agent_states[..., 0] - env.P.agent_gamma
        differs[t] = ((action != other)[..., 0] & (c < 0) & (before > 0.0)).any()
        reward, done, pl, pd = W.oracle_step(env, Ls[t], action)
        grazed[t] = (env.agent_states[..., 0] > before).any()
        alive[t] = W.max_k(env) > THRESHOLD_K
        ok[t] = ~done[..., 0]
        actions[t] = action[..., 0]
        if t + 1 in KS:
            final[t + 1] = W.final_state(env, pl, pd, reward, done, action)
    ref = W._freeze({"start": start, "alive": alive, "ok": ok, "action": actions, "differs": differs, "grazed": grazed,
                     "final": final})
    ref["seconds"] = time.perf_counter() - t0
    _REF_1[key] = ref
    return ref


# the ensemble call with constants of its own for every world: kind b % 4 of
ENSEMBLE_KINDS = ({}, {"q2": 0.0}, {"albedo_light": 0.8, "albedo_dark": 0.3, "gamma": 0.3}, {"temp_optimal": 290.0, "dt": 0.5})


def ensemble_constants(b):
    return dict(ENSEMBLE_KINDS[b % len(ENSEMBLE_KINDS)])


def ensemble_schedule(B, K=K_MAX):
    """(K, B): world b a little brighter than world b - 1."""
    return np.ascontiguousarray(schedule(K)[:, None] + 0.01 * np.arange(B)[None, :])


_REF_ENS = {}


def reference_ensemble(shape, mask):
    """K_MAX table steps of every world ALONE, on a one-world oracle with ensemble_constants(b) at the luminosities
    ensemble_schedule(B)[:, b]: `alive` (K, B), `ok` (K, B, N), `action` (K, B, N), `grazed` (K, B), and the final `light`, `dark` (per
    mille), `idx`, `st`, `reward`, `done`."""
    key = (shape, mask)
    if key in _REF_ENS:
        return _REF_ENS[key]
    t0 = time.perf_counter()
    B, H, Wd, N = shape
    inp = inputs_1(shape)
    Ls = ensemble_schedule(B)
    ref = {"alive": np.zeros((K_MAX, B), dtype=bool), "ok": np.zeros((K_MAX, B, N), dtype=bool),
           "action": np.zeros((K_MAX, B, N), dtype=np.int64), "light": np.zeros((B, H, Wd), dtype=np.int64),
           "dark": np.zeros((B, H, Wd), dtype=np.int64), "idx": np.zeros((B, N, 2), dtype=np.int64), "st": np.zeros((B, N)),
           "reward": np.zeros((B, N, 1)), "done": np.zeros((B, N, 1), dtype=bool), "grazed": np.zeros((K_MAX, B), dtype=bool)}
    for b in range(B):
        # the quantising step is the HANDLE's (its own constants): world b's constants act from the call on
        env = W.oracle_env(inp["light"][b:b + 1], inp["dark"][b:b + 1], inp["idx"][b:b + 1], inp["st"][b:b + 1], L0)
        env.neighborhood = mask_array(mask)
        W.quantise(env)
        for name, v in ensemble_constants(b).items():
            assert hasattr(env.P, name), name
            setattr(env.P, name, v)
        for t in range(K_MAX):
            action = greedy_actions(env.get_obs(env.agent_indices), inp["codes"][t, b:b + 1])
            before = env.agent_states[..., 0] - env.P.agent_gamma
            reward, done, _, _ = W.oracle_step(env, float(Ls[t, b]), action)
            ref["grazed"][t, b] = (env.agent_states[..., 0] > before).any()
            ref["alive"][t, b] = W.max_k(env)[0] > THRESHOLD_K
            ref["ok"][t, b] = ~done[0, :, 0]
            ref["action"][t, b] = action[0, :, 0]
        ref["light"][b], ref["dark"][b] = k_of(env.grid[0, 1]), k_of(env.grid[0, 2])
        ref["idx"][b], ref["st"][b] = env.agent_indices[0], env.agent_states[0, :, 0]
        ref["reward"][b], ref["done"][b] = reward[0], done[0]
    ref = W._freeze(ref)
    ref["seconds"] = time.perf_counter() - t0
    _REF_ENS[key] = ref
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# 4. dw_run_episode_mlp / dw_run_episode_mlp_trace
# ---------------------------------------------------------------------------------------------------------------------
#             B, H, W,  N, split
SHAPES_4 = [(3, 7, 9, 4, 2), (2, 3, 85, 1, 1),   # the wave form
            (2, 8, 8, 5, 2),                     # N = 5 takes the workgroup form
            (2, 17, 17, 4, 2)]                   # the workgroup form by its cells
K2 = 3                                           # the second chunk (params=None)
MLP_AGENT_GAMMA = W.MLP_AGENT_GAMMA
N_MEMBERS = W.N_MEMBERS
# frozen: the first seed from 7100 at which every condition of tests/test_obs_mask_cases_cpu.py holds
SEEDS_4 = {(3, 7, 9, 4, 2): 7101, (2, 3, 85, 1, 1): 7120, (2, 8, 8, 5, 2): 7101, (2, 17, 17, 4, 2): 7100}


def mlp_form_of(shape):
    return WAVE if shape[1] * shape[2] <= 256 and shape[3] <= 4 else WORKGROUP


_INPUTS_4 = {}


def inputs_4(shape):
    if shape not in _INPUTS_4:
        B, H, Wd, N, split = shape
        light, dark, idx, st, rng = W.start_inputs(shape[:4], SEEDS_4[shape])
        params = rng.randn(N_MEMBERS, 1808) * 0.3
        ma, mb = W.members(B)
        _INPUTS_4[shape] = W._freeze({"light": light, "dark": dark, "idx": idx, "st": st, "params": params, "member_a": ma,
                                      "member_b": mb})
    return _INPUTS_4[shape]


def _corner_stamped(env, here):
    """Some visible corner cell of some agent's patch holds an agent: channel 4 shows a stamped state there."""
    H, Wd = env.shape
    for b in range(env.agent_indices.shape[0]):
        cells = {(int(r), int(c)) for r, c in env.agent_indices[b]}
        for r, c in env.agent_indices[b]:
            for k in CORNERS:
                if here.ravel()[k] and ((int(r) + k // 3 - 1) % H, (int(c) + k % 3 - 1) % Wd) in cells:
                    return True
    return False


def mlp_decisions(nets, inp, split, obs):
    """(actions (B, N, 1), the least distance of the two largest logits) of one step's observations."""
    B, N = obs.shape[:2]
    action, least = np.zeros((B, N, 1), dtype=np.int64), np.inf
    for b in range(B):
        for n in range(N):
            net = nets[inp["member_a"][b]] if n < split else nets[inp["member_b"][b]]
            logits = net.forward(obs[b, n].reshape(63))
            top = np.sort(logits)
            least = min(least, top[-1] - top[-2])
            action[b, n, 0] = int(np.argmax(logits))
    return action, least


def _mlp_run(env, inp, split, Ls, masks_at, ends):
    """T oracle steps with OracleMLP policies; `masks_at`: {step: mask set before that step's decision}."""
    nets = [O.OracleMLP(p) for p in inp["params"]]
    T = len(Ls)
    B, N = env.agent_indices.shape[:2]
    rewards, dones = np.zeros((T, B, N, 1)), np.zeros((T, B, N, 1), dtype=bool)
    actions, margin, final = np.zeros((T, B, N), dtype=np.int64), np.zeros(T), {}
    differs, stamped, grazed = np.zeros(T, dtype=bool), np.zeros(T, dtype=bool), np.zeros(T, dtype=bool)
    for t in range(T):
        if t in masks_at:
            env.neighborhood = mask_array(masks_at[t])
        here = env.neighborhood
        obs = full_obs(env)
        action, margin[t] = mlp_decisions(nets, inp, split, obs * here)
        other, _ = mlp_decisions(nets, inp, split, obs * _VN)
        before = env.agent_states[..., 0] - env.P.agent_gamma
        differs[t] = ((action != other)[..., 0] & (before > 0.0)).any()
        stamped[t] = _corner_stamped(env, here)
        reward, done, pl, pd = W.oracle_step(env, Ls[t], action)
        grazed[t] = (env.agent_states[..., 0] > before).any()
        rewards[t], dones[t], actions[t] = reward, done, action[..., 0]
        if t + 1 in ends:
            final[t + 1] = W.final_state(env, pl, pd, reward, done, action)
    return {"reward": rewards, "done": dones, "action": actions, "margin": margin, "final": final, "differs": differs,
            "stamped": stamped, "grazed": grazed}


_REF_4 = {}


def reference_4(shape, mask):
    """K_MAX + K2 oracle steps with OracleMLP policies under `mask`: a run of K steps and its second chunk of K2 steps are
    the steps [0, K) and [K, K + K2) of this one run.  `reward` / `done` (T, B, N, 1), `action` (T, B, N), `margin` (T,),
    `differs` (T,) - a live agent's action is not the one its network takes on the von-Neumann-masked observation -,
    `stamped` (T,) - a visible corner cell holds an agent -, `grazed` (T,), `final[t]`, `start`, `max_k1`, `seconds`."""
    key = (shape, mask)
    if key in _REF_4:
        return _REF_4[key]
    t0 = time.perf_counter()
    inp = inputs_4(shape)
    env = masked_env(inp, mask, agent_gamma=MLP_AGENT_GAMMA)
    start = W.quantise(env)
    ends = sorted({K for K in KS} | {K + K2 for K in KS})
    ref = _mlp_run(env, inp, shape[4], schedule(ends[-1]), {}, ends)
    ref["start"] = start
    ref = W._freeze(ref)
    ref["seconds"] = time.perf_counter() - t0
    _REF_4[key] = ref
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# 5. per-step calls
# ---------------------------------------------------------------------------------------------------------------------
SHAPES_5 = [(3, 9, 13, 4), (2, 40, 256, 3)]
SEEDS_5 = {(3, 9, 13, 4): 7235, (2, 40, 256, 3): 7295}             # frozen likewise, from 7200
AGENT_RANGE = (1, 3)                                             # policy_mlp_population: agents [1, 3) only


ROTATIONS = (0, 1, 2)


def per_agent_modes(N, rotation=0):
    """dw_policy_per_agent: agent n argmax (0) / argmin (1) / keeps the uploaded action (2), in turn.  The call is made
    once per rotation, so that every agent takes every mode: with N = 3 a single call has one argmax and one argmin agent
    per world, too few for each mode to meet a decision the mask changes under every mask."""
    return ((np.arange(N) + rotation) % 3).astype(np.int32)


_INPUTS_5 = {}


def inputs_5(shape):
    """Quantised planes for the protocol's start; `upload_light` / `upload_dark`: an UN-quantised float32 state as it is
    uploaded, `raw_light` / `raw_dark`: the float64 values the handle then holds - it keeps float32 PER-MILLE values
    (f32nat_to_permille: x * 1000.f) and reads them as k / 1000.0, which the GPU test asserts from download_planes -;
    agents, three parameter sets, a member per world, and the actions uploaded before dw_policy_per_agent (9 + n: no
    policy writes such a code)."""
    if shape not in _INPUTS_5:
        B, H, Wd, N = shape
        light, dark, idx, st, rng = W.start_inputs(shape, SEEDS_5[shape])
        up_l, up_d = (rng.rand(B, H, Wd) * 0.4).astype(np.float32), (rng.rand(B, H, Wd) * 0.4).astype(np.float32)
        raw_l = (up_l * np.float32(1000.0)).astype(np.float64) / 1000.0
        raw_d = (up_d * np.float32(1000.0)).astype(np.float64) / 1000.0
        params = rng.randn(N_MEMBERS, 1808) * 0.3
        member = ((np.arange(B) + 1) % N_MEMBERS).astype(np.int32)
        kept = np.tile(9 + np.arange(N), (B, 1)).astype(np.int32)
        _INPUTS_5[shape] = W._freeze({"light": light, "dark": dark, "idx": idx, "st": st, "raw_light": raw_l,
                                      "raw_dark": raw_d, "upload_light": up_l, "upload_dark": up_d, "params": params, "member": member, "kept": kept})
    return _INPUTS_5[shape]


_REF_5 = {}


def reference_5(shape, mask, quantised):
    """What the per-step calls must give on one state: `obs` (B, N, 7, 3, 3), `argmax` / `argmin` (B, N), `per_agent`
    (one (B, N) per rotation of per_agent_modes), `mlp` (B, N) with parameter set 0, `population` (B, N) - agents [1, 3) of
    world b by set member[b], the rest kept -, `margin`, `start` (quantised only), and `differs`: per call, whether some
    action is not the one the von Neumann mask gives on the same cells - "argmax", "argmin", "per_agent argmax" /
    "per_agent argmin" (the agents in that mode, over the rotations), "mlp", "population".
    quantised=False: the state is the raw upload itself (the grid of set_initial_cover: un-rounded temperatures, no agent
    stamps)."""
    key = (shape, mask, quantised)
    if key in _REF_5:
        return _REF_5[key]
    B, H, Wd, N = shape
    inp = inputs_5(shape)
    here = mask_array(mask)
    if quantised:
        env = masked_env(inp, mask)
        start = W.quantise(env)
    else:
        env = W.oracle_env(inp["raw_light"], inp["raw_dark"], inp["idx"], inp["st"], L0)
        env.neighborhood = here
        start = None
    full = full_obs(env)
    obs = full * here
    nets = [O.OracleMLP(p) for p in inp["params"]]
    one = np.full((B, N), -1), np.full((B, N), -2)
    g1, g2 = greedy_actions(obs, one[0])[..., 0], greedy_actions(obs, one[1])[..., 0]
    v1, v2 = greedy_actions(full * _VN, one[0])[..., 0], greedy_actions(full * _VN, one[1])[..., 0]
    differs = {"argmax": bool((g1 != v1).any()), "argmin": bool((g2 != v2).any()), "per_agent argmax": False,
               "per_agent argmin": False, "mlp": False, "population": False}
    per_agent = []
    for rotation in ROTATIONS:
        modes = per_agent_modes(N, rotation)
        per_agent.append(np.where(modes == 0, g1, np.where(modes == 1, g2, inp["kept"])))
        differs["per_agent argmax"] |= bool((g1 != v1)[:, modes == 0].any())
        differs["per_agent argmin"] |= bool((g2 != v2)[:, modes == 1].any())
    mlp, population, least = np.zeros((B, N), dtype=np.int64), np.array(inp["kept"], dtype=np.int64), np.inf
    for b in range(B if mask else 0):                            # (nothing visible: all-equal logits, no MLP case)
        for n in range(N):
            for net, into in ((nets[0], mlp), (nets[inp["member"][b]], population)):
                if into is population and not AGENT_RANGE[0] <= n < AGENT_RANGE[1]:
                    continue
                logits = net.forward(obs[b, n].reshape(63))
                top = np.sort(logits)
                least = min(least, top[-1] - top[-2])
                into[b, n] = int(np.argmax(logits))
                differs["mlp" if into is mlp else "population"] |= int(np.argmax(net.forward((full * _VN)[b, n].reshape(63)))) != into[b, n]
    ref = W._freeze({"obs": obs, "argmax": g1, "argmin": g2, "per_agent": per_agent, "mlp": mlp, "population": population,
                     "start": start})
    ref.update(margin=least, differs=differs)
    _REF_5[key] = ref
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# 6. a mask change on a live handle
# ---------------------------------------------------------------------------------------------------------------------
CHANGES_GREEDY = [(VON_NEUMANN, 0x0B2), (0x09A, MOORE), (0x155, VON_NEUMANN)]     # (Moore is von Neumann to a greedy agent)
CHANGES_MLP = [(VON_NEUMANN, MOORE), (MOORE, 0x0B2), (0x155, 0x09A)]
CHANGE_GREEDY_SHAPE = (3, 5, 13, 4)
CHANGE_MLP_SHAPE = (3, 7, 9, 4, 2)
CHANGE_K1, CHANGE_K2 = 65, 7

_REF_6 = {}


def reference_change_greedy(first, second):
    """CHANGE_K1 table steps under `first`, then CHANGE_K2 under `second`, one oracle whose neighborhood changes between
    them: `alive`, `ok` (T, ...), `action` (T, B, N), `grazed` (T,), `final[CHANGE_K1]`, `final[T]`, `start`; `unchanged`: the actions
    had the mask stayed."""
    key = ("greedy", first, second)
    if key in _REF_6:
        return _REF_6[key]
    shape = CHANGE_GREEDY_SHAPE
    B, H, Wd, N = shape
    inp = inputs_1(shape)
    T = CHANGE_K1 + CHANGE_K2
    rng = np.random.RandomState(7300)
    codes = np.concatenate([inp["codes"], rng.randint(-2, 9, size=(CHANGE_K2, B, N)).astype(np.int8)])
    Ls = schedule(T)
    out = {}
    for name, masks in (("changed", (first, second)), ("unchanged", (first, first))):
        env = masked_env(inp, masks[0])
        start = W.quantise(env)
        alive, ok, final = np.zeros((T, B), dtype=bool), np.zeros((T, B, N), dtype=bool), {}
        actions, grazed = np.zeros((T, B, N), dtype=np.int64), np.zeros(T, dtype=bool)
        for t in range(T):
            if t == CHANGE_K1:
                env.neighborhood = mask_array(masks[1])
            action = greedy_actions(env.get_obs(env.agent_indices), codes[t])
            before = env.agent_states[..., 0] - env.P.agent_gamma
            reward, done, pl, pd = W.oracle_step(env, Ls[t], action)
            grazed[t] = (env.agent_states[..., 0] > before).any()
            alive[t], ok[t], actions[t] = W.max_k(env) > THRESHOLD_K, ~done[..., 0], action[..., 0]
            if t + 1 in (CHANGE_K1, T):
                final[t + 1] = W.final_state(env, pl, pd, reward, done, action)
        out[name] = {"start": start, "alive": alive, "ok": ok, "action": actions, "grazed": grazed, "final": final}
    ref = out["changed"]
    ref["codes"] = codes
    ref["unchanged"] = out["unchanged"]["action"]
    _REF_6[key] = ref = W._freeze(ref)
    return ref


def reference_change_mlp(first, second):
    """The same with OracleMLP policies (the second chunk runs with the parameter sets left on the device)."""
    key = ("mlp", first, second)
    if key in _REF_6:
        return _REF_6[key]
    shape = CHANGE_MLP_SHAPE
    inp = inputs_4(shape)
    T = CHANGE_K1 + CHANGE_K2
    out = {}
    for name, masks in (("changed", (first, second)), ("unchanged", (first, first))):
        env = masked_env(inp, masks[0], agent_gamma=MLP_AGENT_GAMMA)
        start = W.quantise(env)
        out[name] = _mlp_run(env, inp, shape[4], schedule(T), {CHANGE_K1: masks[1]}, (CHANGE_K1, T))
        out[name]["start"] = start
    ref = out["changed"]
    ref["unchanged"] = out["unchanged"]["action"]
    _REF_6[key] = ref = W._freeze(ref)
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# 7. the harness on a Moore drop-in
# ---------------------------------------------------------------------------------------------------------------------
SEED_7, B_7, STEPS_7 = 7400, 6, 40                               # frozen: the first seed from 7400 that meets the conditions

_REF_7 = {}


def reference_7():
    """The oracle loop simulate_grazing_mlp must reproduce: a reference-constructed 8 x 8 world with 4 agents and
    neighborhood_mode="moore", B_7 worlds, reset under np.random.seed(SEED_7); agents 0, 1 act by parameter vector 0,
    agents 2, 3 by vector 1 (RandomState(SEED_7).randn * 0.3).  `obs0`, `reward` / `ok` (T, B, N), the per-step reductions,
    `L` (T,), `grid`, `L_end`, `margin`, `differs`, `stamped`, `grazed` (T,)."""
    if _REF_7:
        return _REF_7
    params = np.random.RandomState(SEED_7).randn(2, 1808) * 0.3
    nets = [O.OracleMLP(p) for p in params]
    state = np.random.get_state()
    try:
        np.random.seed(SEED_7)
        env = O.OracleDaisyWorld.like_reference_ctor(grid_dimension=8, n_agents=4, neighborhood_mode="moore")
        env.P.batch_size = B_7
        obs = env.reset()
    finally:
        np.random.set_state(state)
    T, N = STEPS_7, 4
    ref = {"params": params, "obs0": obs.copy(), "reward": np.zeros((T, B_7, N)), "ok": np.zeros((T, B_7, N), dtype=bool),
           "max_k": np.zeros((T, B_7), dtype=np.uint32), "sum_light_k": np.zeros((T, B_7), dtype=np.uint64),
           "sum_dark_k": np.zeros((T, B_7), dtype=np.uint64), "L": np.zeros(T), "margin": np.zeros(T),
           "differs": np.zeros(T, dtype=bool), "stamped": np.zeros(T, dtype=bool), "grazed": np.zeros(T, dtype=bool)}
    inp = {"member_a": np.zeros(B_7, dtype=np.int32), "member_b": np.ones(B_7, dtype=np.int32)}
    for t in range(T):
        full = full_obs(env) if t else None                      # (the reset observation is the only one of the initial grid)
        action, ref["margin"][t] = mlp_decisions(nets, inp, N // 2, obs)
        if t:
            other, _ = mlp_decisions(nets, inp, N // 2, full * _VN)
            ref["differs"][t] = (action != other).any()
            ref["stamped"][t] = _corner_stamped(env, env.neighborhood)
        before = env.agent_states[..., 0] - env.P.agent_gamma
        ref["L"][t] = env.L
        obs, reward, done, _ = env.step(action)
        ref["grazed"][t] = (env.agent_states[..., 0] > before).any()
        ref["reward"][t], ref["ok"][t] = reward[..., 0], ~done[..., 0]
        kl, kd = k_of(env.grid[:, 1]), k_of(env.grid[:, 2])
        ref["max_k"][t] = np.maximum(kl.max(axis=(1, 2)), kd.max(axis=(1, 2)))
        ref["sum_light_k"][t], ref["sum_dark_k"][t] = kl.sum(axis=(1, 2)), kd.sum(axis=(1, 2))
    ref["grid"], ref["L_end"] = env.grid.copy(), env.L
    _REF_7.update(W._freeze(ref))
    return _REF_7


# ---------------------------------------------------------------------------------------------------------------------
# every exact reference of the table, for the CPU test and the timing line of the commit message
# ---------------------------------------------------------------------------------------------------------------------
CASES_1 = [(s, m, p) for s in SHAPES_1 for m in masks_of_group(GREEDY_MASKS) for p in POLICIES]
CASES_4 = [(s, m) for s in SHAPES_4 for m in masks_of_group(MASKS)]
CASES_5 = [(s, m, q) for s in SHAPES_5 for m in masks_of_group(GREEDY_MASKS) for q in (True, False)]
CASES_ENS = [(s, m) for s in RECORD_SHAPES for m in RECORD_MASKS]


if __name__ == "__main__":
    worst = (0.0, None)
    for case in CASES_1:
        worst = max(worst, (reference_1(*case)["seconds"], case))
    for case in CASES_4:
        worst = max(worst, (reference_4(*case)["seconds"], case))
    for case in CASES_ENS:
        worst = max(worst, (reference_ensemble(*case)["seconds"], case))
    print("largest reference: %.2f s %s" % worst)
