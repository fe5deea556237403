"""The one-wave-per-world episode kernels (csrc/dw_episode_wave.hpp: episode_wave, episode_mlp_wave) against the float64
oracle (run with ``-m gpu``), at the shapes, run lengths and agent counts the harness-level tests never reach:

  shapes      C = H*W below a wave (3x3), one off a wave boundary (63, 65, 255), on the kernel's limit (256), H != W,
              rows wider than a slot (W = 85), tall worlds (H = 85), B % 4 != 0;
  run length  K in {1, 63, 64, 65, 130}: the constants / action table are re-staged in LDS every 64 steps (kEwSeg), the
              flags are 64-bit masks written back per segment - K = 130 runs the segment loop three times;
  agents      N = 64 (every lane an agent) and N = 65 (the first count the wave kernel does not take);
  dispatch    every case asserts from ``kernel_info()`` which episode form it ran, and the long runs are repeated under
              DW_NO_EPISODE_WAVE (episode_small / episode_mlp, one workgroup per 1-4 worlds) and DW_NO_EPISODE_KERNEL
              (launches per step).

Everything compared is integer-valued or float64-exact in the contract (per-mille planes, positions, agent states,
flags, reductions, action codes, observations): every comparison is exact equality.  The oracle world is built through
``set_initial_cover``, so it is rectangular (tests/test_oracle_rect_cpu.py pins that generalisation without a GPU).

Protocol of every case: ``init_random(seed)``, one ``dw_step`` with zero actions (quantises the state; mirrored on the
oracle), then the call under test.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import c_oracle, daisy_oracle as O  # noqa: E402

WAVE, WORKGROUP, STEPWISE = "one wave per world", "workgroup (LDS)", "launches per step"
THRESHOLD_K = 5


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _k(x):
    return np.rint(np.asarray(x) * 1000.0).astype(np.int64)


def _engine(amd, B, H, W, N, precision, monkeypatch, switch=None, agent_gamma=None):
    """A handle created under exactly one (or none) of the DW_NO_EPISODE_* switches: they are read at creation."""
    from therldaisyworld_amd import _ffi
    for name in ("DW_NO_EPISODE_WAVE", "DW_NO_EPISODE_KERNEL"):
        monkeypatch.delenv(name, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")
    p = amd.default_params(B, H, W, N)
    p.precision = _ffi.PRECISION[precision]
    if agent_gamma is not None:
        p.agent_gamma = agent_gamma
    return amd.Engine(p)


def _oracle_like(eng, L):
    """Oracle environment (H x W through set_initial_cover) holding the engine's current (downloaded) state."""
    light, dark = eng.download_planes()
    idx, st = eng.download_agents()
    env = O.OracleDaisyWorldC(grid_dimension=max(eng.H, eng.W), n_agents=eng.N, batch_size=eng.B)
    env.P.agent_gamma = eng.params.agent_gamma
    env.L = L
    env.set_initial_cover(light, dark)
    assert env.shape == (eng.H, eng.W)
    env.agent_indices = idx.astype(np.int64)
    env.agent_states = st.reshape(eng.B, eng.N, 1).copy()
    return env


def _oracle_step(env, L, action):
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


def _resolve_codes(env, codes):
    """Table codes -> actions on the oracle: -1 / -2 are the greedy / anti-greedy choice of that agent
    (ref Greedy.__call__, agents/greedy.py:25-30, epsilon = 0)."""
    obs = env.get_obs(env.agent_indices)
    g1 = O.OracleGreedy(epsilon=0.0, greedy=True)(obs)
    g2 = O.OracleGreedy(epsilon=0.0, greedy=False)(obs)
    c = codes.astype(np.int64)[..., None]
    return np.where(c == -1, g1, np.where(c == -2, g2, c))


def _max_k(env):
    return np.maximum(_k(env.grid[:, 1]).max(axis=(1, 2)), _k(env.grid[:, 2]).max(axis=(1, 2)))


def _final_state(env, prev_light, prev_dark, reward, done, action):
    """Everything the engine can be asked for after the call, from the oracle."""
    kl, kd = _k(env.grid[:, 1]), _k(env.grid[:, 2])
    return {"light": kl, "dark": kd, "prev_light": _k(prev_light), "prev_dark": _k(prev_dark),
            "idx": env.agent_indices.copy(), "st": env.agent_states.copy(), "reward": reward.copy(), "done": done.copy(),
            "obs": env.get_obs(env.agent_indices), "action": np.asarray(action)[..., 0].astype(np.int64),
            "max_k": np.maximum(kl.max(axis=(1, 2)), kd.max(axis=(1, 2))).astype(np.uint32),
            "sum_light_k": kl.sum(axis=(1, 2)).astype(np.uint64), "sum_dark_k": kd.sum(axis=(1, 2)).astype(np.uint64)}


def _compare_final(eng, ref, L_last, what):
    from therldaisyworld_amd import _ffi
    gl, gd = eng.download_planes()
    assert np.array_equal(_k(gl), ref["light"]), f"{what}: light plane"
    assert np.array_equal(_k(gd), ref["dark"]), f"{what}: dark plane"
    pl, pd = eng.download_planes(_ffi.STATE_PREVIOUS)
    assert np.array_equal(_k(pl), ref["prev_light"]), f"{what}: previous light plane"
    assert np.array_equal(_k(pd), ref["prev_dark"]), f"{what}: previous dark plane"
    idx, st = eng.download_agents()
    assert np.array_equal(idx, ref["idx"]), f"{what}: agent positions"
    assert np.array_equal(st[..., None], ref["st"]), f"{what}: agent states"
    r_dev, d_dev = eng.reward_done()
    assert np.array_equal(r_dev, ref["reward"]) and np.array_equal(d_dev, ref["done"]), f"{what}: reward / done"
    s = eng.reduce()
    for f in ("max_k", "sum_light_k", "sum_dark_k"):
        assert np.array_equal(s[f], ref[f]), f"{what}: reduce() {f}"
    assert np.array_equal(eng.get_obs(L_last), ref["obs"]), f"{what}: observations"
    assert np.array_equal(eng.download_actions(), ref["action"]), f"{what}: action codes of the last step"


def _quantise(eng, L0):
    """The protocol's first step: zero actions from the un-quantised init_random state, mirrored on the oracle."""
    env = _oracle_like(eng, L0)
    zeros = np.zeros((eng.B, eng.N, 1), dtype=np.int64)
    eng.step(L0, zeros)
    _oracle_step(env, L0, zeros)
    return env


# ---------------------------------------------------------------------------------------------
# luminosity schedules
# ---------------------------------------------------------------------------------------------
L0 = 0.94


def _schedule(K):
    """The first K entries of ONE 130-step schedule: a gentle ramp through the daisies' comfortable range for 80 steps
    (worlds live, agents graze), then 0.1 per step up to L = 3 (T_eff ~ 400 K: beta < -30, every cover is gone within a
    few steps and the agents starve 0.05 per step) - the long runs end in death, the short ones are its prefixes."""
    t = np.arange(130, dtype=np.float64)
    Ls = np.where(t < 80, 0.95 + 0.002 * t, np.minimum(3.0, 0.95 + 0.002 * 79 + 0.1 * (t - 79)))
    return Ls[:K].copy()


# ---------------------------------------------------------------------------------------------
# A. dw_run_episode, exact mode, against the oracle
# ---------------------------------------------------------------------------------------------
#         B, H,  W,  N    what it pins
SHAPES = [(5, 3, 3, 2),       # the smallest legal world: 9 cells, 55 idle lanes, B % 4 != 0
          (6, 7, 9, 3),       # C = 63
          (3, 5, 13, 4),      # C = 65: one cell in the second slot
          (7, 3, 85, 5),      # C = 255, W > 64, H = 3
          (2, 85, 3, 5),      # the tall counterpart
          (9, 4, 64, 4),      # C = 256, non-square
          (1, 12, 12, 1),     # a lone world, a lone agent
          (4, 8, 8, 64),      # N = C = 64: every lane an agent, agents meet on cells
          (3, 16, 16, 64),    # N = 64 with four slots per lane
          (3, 12, 12, 65)]    # the first N beyond the wave kernel
KS_FULL = (1, 63, 64, 65, 130)


def _ks_of(shape):
    i = SHAPES.index(shape)
    return KS_FULL if i < 6 else ((65, 130) if shape[3] < 64 else (65,))


def _form_of(shape):
    return WORKGROUP if shape[3] > 64 else WAVE


CASES_A = [(s, K, pol) for s in SHAPES for K in _ks_of(s) for pol in ("table", "argmin+use_table")]
LONG_A = [(s, max(_ks_of(s))) for s in SHAPES]                  # K = 130 where the shape has it, 65 for N >= 64


def _inputs_a(shape, K, policy):
    """(codes (K, B, N) int8 from -2..8, use_table (K,) uint8 or None) - a function of the case alone."""
    B, H, W, N = shape
    rng = np.random.RandomState(1000 * SHAPES.index(shape) + K)
    codes = rng.randint(-2, 9, size=(K, B, N)).astype(np.int8)
    if policy == "table":
        return codes, None
    ut = (rng.rand(K) < 0.4).astype(np.uint8)
    ut[[t for t in (63, 64, 65) if t < K]] = 1                  # around the segment boundary
    return codes, ut


_REF_A = {}


def _reference_a(eng, env, shape, K, policy):
    """The oracle's K steps from the quantised state `env` holds - computed once per (shape, K, policy) and shared by the
    default, DW_NO_EPISODE_WAVE and DW_NO_EPISODE_KERNEL runs, which start from the same state (asserted)."""
    key = (shape, K, policy)
    start = (_k(env.grid[:, 1]), _k(env.grid[:, 2]), env.agent_indices.copy())
    if key in _REF_A:
        ref = _REF_A[key]
        assert all(np.array_equal(a, b) for a, b in zip(start, ref["start"])), "the shared reference starts elsewhere"
        return ref
    B, H, W, N = shape
    codes, ut = _inputs_a(shape, K, policy)
    Ls = _schedule(K)
    alive = np.zeros((K, B), dtype=bool)
    ok = np.zeros((K, B, N), dtype=bool)
    for t in range(K):
        c = codes[t] if (ut is None or ut[t]) else np.full((B, N), -2, dtype=np.int8)      # POLICY_ARGMIN: anti-greedy
        action = _resolve_codes(env, c)
        reward, done, pl, pd = _oracle_step(env, Ls[t], action)
        alive[t] = _max_k(env) > THRESHOLD_K
        ok[t] = ~done[..., 0]
    ref = _final_state(env, pl, pd, reward, done, action)
    ref.update(start=start, alive=alive, ok=ok)
    _REF_A[key] = ref
    return ref


def _assert_ends_in_death(ref, what):
    """Input conditions of the K = 130 cases, judged on the oracle's series alone: the run is alive well into its second
    segment and everything is dead at its end."""
    alive, ok = ref["alive"], ref["ok"]
    assert alive[70:].any(), f"{what}: no world alive at a step >= 70"
    assert not alive[-1].any(), f"{what}: a world is still alive at the end"
    assert ok[70:].any(), f"{what}: no agent ok at a step >= 70"
    assert not ok.all(), f"{what}: no agent has died"


def _run_a(amd, monkeypatch, shape, K, policy, switch, form):
    from therldaisyworld_amd import _ffi
    B, H, W, N = shape
    what = f"{shape} K={K} {policy} {switch or 'default'}"
    eng = _engine(amd, B, H, W, N, "exact", monkeypatch, switch)
    info = eng.kernel_info()
    assert f"; episode: {form}" in info, info
    eng.init_random(100 + SHAPES.index(shape))
    env = _quantise(eng, L0)
    ref = _reference_a(eng, env, shape, K, policy)
    if K == 130:
        _assert_ends_in_death(ref, what)
    codes, ut = _inputs_a(shape, K, policy)
    Ls = _schedule(K)
    if policy == "table":
        alive, ok = eng.run_episode(Ls, _ffi.POLICY_TABLE, None, codes, threshold_k=THRESHOLD_K)
    else:
        alive, ok = eng.run_episode(Ls, _ffi.POLICY_ARGMIN, ut, codes, threshold_k=THRESHOLD_K)
    for t in range(K):
        assert np.array_equal(alive[t], ref["alive"][t]), f"{what}: world_alive[{t}]"
        assert np.array_equal(ok[t], ref["ok"][t]), f"{what}: agent_ok[{t}]"
    _compare_final(eng, ref, Ls[-1], what)
    eng.close()


@pytest.mark.parametrize("shape,K,policy", CASES_A, ids=lambda v: str(v).replace(" ", ""))
def test_run_episode_exact_vs_oracle(amd, monkeypatch, shape, K, policy):
    _run_a(amd, monkeypatch, shape, K, policy, None, _form_of(shape))


@pytest.mark.parametrize("switch,form", [("DW_NO_EPISODE_WAVE", WORKGROUP), ("DW_NO_EPISODE_KERNEL", STEPWISE)])
@pytest.mark.parametrize("shape,K", LONG_A, ids=lambda v: str(v).replace(" ", ""))
def test_run_episode_exact_vs_oracle_other_forms(amd, monkeypatch, shape, K, switch, form):
    """The long table-driven runs again on the workgroup kernel (episode_small: its first rectangular and its first
    multi-segment-length runs) and as launches per step: the same oracle series."""
    _run_a(amd, monkeypatch, shape, K, "table", switch, form)


# ---------------------------------------------------------------------------------------------
# B. fast mode: float32 results are identical across kernel families
# ---------------------------------------------------------------------------------------------
def _outputs_fast(amd, monkeypatch, shape, K, switch, form):
    from therldaisyworld_amd import _ffi
    B, H, W, N = shape
    eng = _engine(amd, B, H, W, N, "fast", monkeypatch, switch)
    assert f"; episode: {form}" in eng.kernel_info(), eng.kernel_info()
    eng.init_random(100 + SHAPES.index(shape))
    eng.step(L0, np.zeros((B, N, 1), dtype=np.int64))
    codes = np.random.RandomState(7 + SHAPES.index(shape)).randint(9, size=(K, B, N)).astype(np.int8)   # explicit: 0..8
    Ls = _schedule(K)
    alive, ok = eng.run_episode(Ls, _ffi.POLICY_TABLE, None, codes, threshold_k=THRESHOLD_K)
    s = eng.reduce()
    out = {"alive": alive.copy(), "ok": ok.copy(), "obs": eng.get_obs(Ls[-1]), "action": eng.download_actions(),
           "max_k": s["max_k"].copy(), "sum_light_k": s["sum_light_k"].copy(), "sum_dark_k": s["sum_dark_k"].copy()}
    out["light"], out["dark"] = eng.download_planes()
    out["prev_light"], out["prev_dark"] = eng.download_planes(_ffi.STATE_PREVIOUS)
    out["idx"], out["st"] = eng.download_agents()
    out["reward"], out["done"] = eng.reward_done()
    eng.close()
    assert np.array_equal(out["action"], codes[-1])
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_run_episode_fast_equals_launches_per_step(amd, monkeypatch, shape):
    """The float32-only mode is not the oracle's arithmetic; the library's own invariant is that its results do not
    depend on the kernel family.  130 steps of explicit moves (no policy decision rides on a float32 value) through the
    default form and as launches per step: every output identical."""
    a = _outputs_fast(amd, monkeypatch, shape, 130, None, _form_of(shape))
    b = _outputs_fast(amd, monkeypatch, shape, 130, "DW_NO_EPISODE_KERNEL", STEPWISE)
    for name in a:
        assert np.array_equal(a[name], b[name]), f"{shape}: {name}"


# ---------------------------------------------------------------------------------------------
# C. dw_step_n without agents on wave shapes (kPolicySkipAgents on a handle that has agents)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(6, 7, 9), (3, 5, 13), (7, 3, 85), (9, 4, 64)], ids=lambda v: str(v).replace(" ", ""))
def test_step_n_on_wave_shapes_vs_c_oracle(amd, monkeypatch, shape):
    """131 agent-free steps from the un-quantised init_random state: the first by the step kernel, 130 by the episode
    kernel (three segments) with the agents skipped - planes and reductions bit-identical to the C oracle, the three
    agents of every world untouched, the returned luminosity the oracle's."""
    B, H, W = shape
    eng = _engine(amd, B, H, W, 3, "exact", monkeypatch)
    assert f"; episode: {WAVE}" in eng.kernel_info(), eng.kernel_info()
    eng.init_random(31 + H)
    light, dark = eng.download_planes()
    idx0, st0 = eng.download_agents()
    dL = 0.002                                                  # 0.9 -> 1.162: the daisies' comfortable range
    L = eng.step_n(131, 0.9, dL, 0.75, 1.5)
    Lo = c_oracle.step_n(light, dark, 0.9, dL, 131)
    assert L == Lo
    gl, gd = eng.download_planes()
    assert np.array_equal(_k(gl), _k(light)) and np.array_equal(_k(gd), _k(dark))
    assert _k(light).max() > THRESHOLD_K                        # (not a comparison of two dead worlds)
    s = eng.reduce()
    assert np.array_equal(s["sum_light_k"], _k(light).sum(axis=(1, 2)).astype(np.uint64))
    assert np.array_equal(s["sum_dark_k"], _k(dark).sum(axis=(1, 2)).astype(np.uint64))
    assert np.array_equal(s["max_k"], np.maximum(_k(light).max(axis=(1, 2)), _k(dark).max(axis=(1, 2))).astype(np.uint32))
    idx1, st1 = eng.download_agents()
    assert np.array_equal(idx0, idx1) and np.array_equal(st0, st1)
    eng.close()


# ---------------------------------------------------------------------------------------------
# D. dw_run_episode_mlp, exact mode, against the oracle with OracleMLP policies
# ---------------------------------------------------------------------------------------------
#             B, H,  W, N, split   (split = N // 2; N = 1: split = 1 - the adversary set [split, N) is empty - and 0)
MLP_SHAPES = [(3, 7, 9, 4, 2), (2, 5, 13, 3, 1), (5, 4, 64, 4, 2), (2, 3, 85, 1, 1), (2, 3, 85, 1, 0),
              (2, 8, 8, 5, 2)]                                  # N = 5: beyond the wave form (sixteen lanes per agent)
MLP_KS = (64, 65, 130)
MLP_K2 = 65                                                     # the second chunk (params=None): crosses a segment too
MARGIN = 1e-9
# Randomly drawn networks mostly repeat one move, and few of those graze: at the reference's decay of 0.05 per step
# their agents would be dead - and motionless - after 20 steps.  At 0.005 they move through both chunks (at most 196
# steps), their rewards change at every step, and the ones that never eat fall below the `done` threshold at step 181.
MLP_AGENT_GAMMA = 0.005


def _mlp_schedule(K, start=0):
    return 0.95 + 0.003 * np.arange(start, start + K, dtype=np.float64)


def _mlp_chunk(env, nets_a, nets_b, split, Ls, what):
    """K oracle steps with OracleMLP policies (agents [0, split) of world b: nets_a[b], the rest: nets_b[b]).  Asserts the
    input condition on the way: the device accumulates every dot product sequentially with fma, NumPy by matmul, so the
    two largest logits of every decision must be further apart than any such rounding difference."""
    B, N = env.P.batch_size, env.P.n_agents
    K = len(Ls)
    rewards, dones = np.zeros((K, B, N, 1)), np.zeros((K, B, N, 1), dtype=bool)
    obs = env.get_obs(env.agent_indices)
    least = np.inf
    for t in range(K):
        action = np.zeros((B, N, 1), dtype=np.int64)
        for b in range(B):
            for n in range(N):
                logits = (nets_a[b] if n < split else nets_b[b]).forward(obs[b, n].reshape(63))
                top = np.sort(logits)
                least = min(least, top[-1] - top[-2])
                action[b, n, 0] = int(np.argmax(logits))
        assert least > MARGIN, f"{what}: logit margin {least} at step {t}"
        kept = _oracle_step(env, Ls[t], action)
        rewards[t], dones[t] = kept[0], kept[1]
        obs = env.get_obs(env.agent_indices)
    return rewards, dones, _final_state(env, kept[2], kept[3], kept[0], kept[1], action)


@pytest.mark.parametrize("K", MLP_KS)
@pytest.mark.parametrize("shape", MLP_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_run_episode_mlp_exact_vs_oracle(amd, monkeypatch, shape, K):
    """K steps with three random parameter sets shared out per world (member_a / member_b differ per world), then 65
    more with the parameter sets still on the device (params=None): reward (K, B, N, 1) and done of every step, the final
    state after either chunk."""
    B, H, W, N, split = shape
    what = f"mlp {shape} K={K}"
    eng = _engine(amd, B, H, W, N, "exact", monkeypatch, agent_gamma=MLP_AGENT_GAMMA)
    info = eng.kernel_info()
    assert f"; mlp episode: {WAVE if N <= 4 else WORKGROUP}" in info, info
    rng = np.random.RandomState(500 + MLP_SHAPES.index(shape))
    params = rng.randn(3, 1808) * 0.3
    member_a = (np.arange(B) % 3).astype(np.int32)
    member_b = ((np.arange(B) + 1 + np.arange(B) // 3) % 3).astype(np.int32)
    assert (member_a != member_b).any()
    nets = [O.OracleMLP(p) for p in params]
    nets_a, nets_b = [nets[m] for m in member_a], [nets[m] for m in member_b]
    eng.init_random(200 + MLP_SHAPES.index(shape))
    env = _quantise(eng, L0)

    Ls = _mlp_schedule(K)
    r_ref, d_ref, ref = _mlp_chunk(env, nets_a, nets_b, split, Ls, what)
    reward, done = eng.run_episode_mlp(Ls, params, member_a, member_b, split=split)
    assert reward.shape == (K, B, N, 1)
    assert np.array_equal(reward, r_ref), f"{what}: reward"
    assert np.array_equal(done, d_ref), f"{what}: done"
    _compare_final(eng, ref, Ls[-1], what)

    Ls2 = _mlp_schedule(MLP_K2, K)
    r_ref, d_ref, ref = _mlp_chunk(env, nets_a, nets_b, split, Ls2, what + " second chunk")
    reward, done = eng.run_episode_mlp(Ls2, None, member_a, member_b, split=split, n_members=3)
    assert np.array_equal(reward, r_ref), f"{what}: reward of the second chunk"
    assert np.array_equal(done, d_ref), f"{what}: done of the second chunk"
    _compare_final(eng, ref, Ls2[-1], what + " second chunk")
    assert (r_ref[-1] > 0).any()                                # (agents lived, and moved, to the end)
    eng.close()
