"""The workgroup episode kernels (csrc/dw_episode.hpp: episode_small<EXACT>, episode_mlp<EXACT>; `workgroup (LDS)` in
``kernel_info()``) above 256 cells against the float64 oracle (run with ``-m gpu``) - the family the library runs for
24 x 24, 32 x 32 and 64 x 64 worlds, where a world is served by two waves (256 < C <= 1024, two worlds per workgroup) or
four (1024 < C <= 4096): its reductions cross waves through LDS atomics, its agent and MLP loops stride by 128 / 256
threads, and a workgroup can hold a half without a world.

The cases, their inputs and the oracle references are the table tools/episode_workgroup_cases.py (what each shape pins is
written there); tests/test_episode_workgroup_cases_cpu.py keeps that table honest without a GPU.  Protocol of every case:
``upload_state_f32(quantised=True)``, ``upload_agents``, one zero-action ``dw_step`` at L0 (mirrored on the oracle; the
state the call starts from is asserted equal to the oracle's), then the call under test.

  1  dw_run_episode, exact: K in {1, 2, 41} (both ping-pong parities end a run), policies table (codes -2 .. 8) and
     argmin+use_table; world_alive / agent_ok of every step and the whole final state
  2  the K = 41 table runs as launches per step (DW_NO_EPISODE_KERNEL) against the same references
  3  dw_run_episode, float32-only: the default form and launches per step give identical outputs
  4  agent-free dw_step_n from an un-quantised float64 upload, against c_oracle.step_n
  5  the near-tie list of ep_forward filled past kEpFixCap (inadmissible constants: every cell flagged), and not
  6  dw_run_episode_mlp, exact: K in {3, 20}, then 5 more steps with the parameter sets left on the device; N not a
     multiple of the agents per pass; at the 160 KiB LDS limit
  7  dw_run_episode_mlp, float32-only: identical outputs across the two forms
  8  one cell / one agent beyond the limits: launches per step

Everything compared is integer-valued or float64-exact in the contract: every comparison is exact equality.  Every test
first asserts from ``kernel_info()`` which form it runs.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import episode_workgroup_cases as W  # noqa: E402
from constant_edge_cases import ALL_SWITCHES  # noqa: E402

_ids = lambda v: str(v).replace(" ", "")  # noqa: E731


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _engine(amd, monkeypatch, shape, precision, switch=None, agent_gamma=None, over=None):
    """A handle created under exactly one (or none) of the library's switches: they are read at creation."""
    from therldaisyworld_amd import _ffi
    for name in ALL_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")
    p = amd.default_params(*shape[:4])
    p.precision = _ffi.PRECISION[precision]
    if agent_gamma is not None:
        p.agent_gamma = agent_gamma
    for k, v in (over or {}).items():
        setattr(p, k, v)
    return amd.Engine(p)


def _assert_form(eng, what, form):
    info = eng.kernel_info()
    assert f"; {what}: {form}" in info, info


def _begin(eng, inp, start=None):
    """Steps 1 to 3 of the protocol; `start`: the oracle's state after them, which the engine must hold."""
    B, N = eng.B, eng.N
    eng.upload_state_f32(inp["light"].astype(np.float32), inp["dark"].astype(np.float32), quantised=True)
    eng.upload_agents(inp["idx"], inp["st"])
    eng.step(W.L0, np.zeros((B, N, 1), dtype=np.int64))
    if start is not None:
        gl, gd = eng.download_planes()
        idx, st = eng.download_agents()
        assert np.array_equal(W.k_of(gl), start["light"]) and np.array_equal(W.k_of(gd), start["dark"]), "start planes"
        assert np.array_equal(idx, start["idx"]) and np.array_equal(st, start["st"]), "start agents"


def _compare_final(eng, ref, L_last, what):
    from therldaisyworld_amd import _ffi
    gl, gd = eng.download_planes()
    assert np.array_equal(W.k_of(gl), ref["light"]), f"{what}: light plane"
    assert np.array_equal(W.k_of(gd), ref["dark"]), f"{what}: dark plane"
    pl, pd = eng.download_planes(_ffi.STATE_PREVIOUS)
    assert np.array_equal(W.k_of(pl), ref["prev_light"]), f"{what}: previous light plane"
    assert np.array_equal(W.k_of(pd), ref["prev_dark"]), f"{what}: previous dark plane"
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


def _everything(eng, L_last):
    """Every output a float32-only run leaves, for the comparison of two forms"""
    from therldaisyworld_amd import _ffi
    s = eng.reduce()
    out = {"obs": eng.get_obs(L_last), "action": eng.download_actions(), "max_k": s["max_k"].copy(),
           "sum_light_k": s["sum_light_k"].copy(), "sum_dark_k": s["sum_dark_k"].copy()}
    out["light"], out["dark"] = eng.download_planes()
    out["prev_light"], out["prev_dark"] = eng.download_planes(_ffi.STATE_PREVIOUS)
    out["idx"], out["st"] = eng.download_agents()
    out["reward"], out["done"] = eng.reward_done()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2. dw_run_episode, exact mode, against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _run_a(amd, monkeypatch, shape, K, policy, switch, form):
    from therldaisyworld_amd import _ffi
    what = f"{shape} K={K} {policy} {switch or 'default'}"
    eng = _engine(amd, monkeypatch, shape, "exact", switch)
    _assert_form(eng, "episode", form)
    inp, ref = W.inputs_a(shape), W.reference_a(shape, policy)
    _begin(eng, inp, ref["start"])
    Ls, codes = W.schedule_a(K), inp["codes"][:K]
    if policy == "table":
        alive, ok = eng.run_episode(Ls, _ffi.POLICY_TABLE, None, codes, threshold_k=W.THRESHOLD_K)
    else:
        alive, ok = eng.run_episode(Ls, _ffi.POLICY_ARGMIN, inp["use_table"][:K], codes, threshold_k=W.THRESHOLD_K)
    for t in range(K):
        assert np.array_equal(alive[t], ref["alive"][t]), f"{what}: world_alive[{t}]"
        assert np.array_equal(ok[t], ref["ok"][t]), f"{what}: agent_ok[{t}]"
    _compare_final(eng, ref["final"][K], Ls[-1], what)
    eng.close()


@pytest.mark.parametrize("policy", W.POLICIES)
@pytest.mark.parametrize("K", W.KS_A)
@pytest.mark.parametrize("shape", W.SHAPES_A, ids=_ids)
def test_run_episode_exact_vs_oracle(amd, monkeypatch, shape, K, policy):
    _run_a(amd, monkeypatch, shape, K, policy, None, W.WORKGROUP)


@pytest.mark.parametrize("shape", W.SHAPES_A, ids=_ids)
def test_run_episode_exact_vs_oracle_launches_per_step(amd, monkeypatch, shape):
    """The same cached reference, the same start state (asserted), the library's other path."""
    _run_a(amd, monkeypatch, shape, W.K_A, "table", "DW_NO_EPISODE_KERNEL", W.STEPWISE)


# ---------------------------------------------------------------------------------------------------------------------
# 3. float32-only: results are identical across kernel families
# ---------------------------------------------------------------------------------------------------------------------
def _outputs_fast(amd, monkeypatch, shape, switch, form):
    from therldaisyworld_amd import _ffi
    eng = _engine(amd, monkeypatch, shape, "fast", switch)
    _assert_form(eng, "episode", form)
    inp = W.inputs_a(shape)
    _begin(eng, inp)
    Ls = W.schedule_a()
    alive, ok = eng.run_episode(Ls, _ffi.POLICY_TABLE, None, inp["moves"], threshold_k=W.THRESHOLD_K)
    out = _everything(eng, Ls[-1])
    out.update(alive=alive.copy(), ok=ok.copy())
    eng.close()
    assert np.array_equal(out["action"], inp["moves"][-1])
    return out


@pytest.mark.parametrize("shape", W.SHAPES_A, ids=_ids)
def test_run_episode_fast_equals_launches_per_step(amd, monkeypatch, shape):
    """The float32-only mode is not the oracle's arithmetic; the library's own invariant is that its results do not
    depend on the kernel family (section B of tests/test_gpu_episode_wave.py).  41 steps of explicit moves through
    episode_small<false> and as launches per step: every output identical."""
    a = _outputs_fast(amd, monkeypatch, shape, None, W.WORKGROUP)
    b = _outputs_fast(amd, monkeypatch, shape, "DW_NO_EPISODE_KERNEL", W.STEPWISE)
    assert a["max_k"].min() > W.THRESHOLD_K                      # (not a comparison of two dead worlds)
    for name in a:
        assert np.array_equal(a[name], b[name]), f"{shape}: {name}"


# ---------------------------------------------------------------------------------------------------------------------
# 4. agent-free dw_step_n (kPolicySkipAgents on a handle that has agents)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", W.STEP_N_SHAPES, ids=_ids)
def test_step_n_on_workgroup_shapes_vs_c_oracle(amd, monkeypatch, shape):
    """42 steps from an un-quantised float64 upload: the first by the step kernel, 41 by episode_small with the agents
    skipped - planes and reductions bit-identical to the C oracle, the returned luminosity the oracle's, the three agents
    of every world untouched."""
    eng = _engine(amd, monkeypatch, (*shape, W.STEP_N_AGENTS), "exact")
    _assert_form(eng, "episode", W.WORKGROUP)
    light, dark, idx0, st0 = W.inputs_step_n(shape)
    eng.upload_state(light, dark)
    eng.upload_agents(idx0, st0)
    L = eng.step_n(W.STEP_N_STEPS, W.STEP_N_L, W.STEP_N_DL, *W.STEP_N_RANGE)
    kl, kd, Lo = W.reference_step_n(shape)
    assert L == Lo
    gl, gd = eng.download_planes()
    assert np.array_equal(W.k_of(gl), kl) and np.array_equal(W.k_of(gd), kd)
    s = eng.reduce()
    assert np.array_equal(s["sum_light_k"], kl.sum(axis=(1, 2)).astype(np.uint64))
    assert np.array_equal(s["sum_dark_k"], kd.sum(axis=(1, 2)).astype(np.uint64))
    assert np.array_equal(s["max_k"], np.maximum(kl.max(axis=(1, 2)), kd.max(axis=(1, 2))).astype(np.uint32))
    idx1, st1 = eng.download_agents()
    assert np.array_equal(idx0, idx1) and np.array_equal(st0, st1)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the near-tie list of ep_forward, full and not
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", W.OVERFLOW_CASES, ids=_ids)
def test_near_tie_list_overflow(amd, monkeypatch, name, shape):
    """ep_forward lists a world's near-tie cells of a step - at most kEpFixCap = 240 of them, re-evaluated in float64
    after the cell loop by all threads of the world - and re-evaluates on the spot what no longer fits.  With the
    inadmissible constants every cell is flagged: 240 go through the list, the other 784 / 1360 of a world through the
    overflow branch, at every step.  dw_last_fixup_count is the number of CELLS re-evaluated in the call's LAST step (`nfix`
    is counted once per cell in either branch, red[3] is cleared after every step), summed over the worlds: exactly
    B * H * W there; with the default constants a few near ties per world - positive, and the list never fills."""
    from therldaisyworld_amd import _ffi
    B, H, Wd, N = shape
    what = f"{name} {shape}"
    eng = _engine(amd, monkeypatch, shape, "exact", over=W.overflow_constants(name))
    _assert_form(eng, "episode", W.WORKGROUP)
    inp, ref = W.inputs_overflow(name, shape), W.reference_overflow(name, shape)
    _begin(eng, inp, ref["start"])
    Ls = W.overflow_schedule(name)
    alive, ok = eng.run_episode(Ls, _ffi.POLICY_TABLE, None, inp["codes"], threshold_k=W.THRESHOLD_K)
    count = eng.last_fixup_count()
    print(what, "float64 re-evaluations of the last step:", count)
    assert np.array_equal(alive, ref["alive"]), f"{what}: world_alive"
    assert np.array_equal(ok, ref["ok"]), f"{what}: agent_ok"
    _compare_final(eng, ref["final"], Ls[-1], what)
    if name:
        assert count >= B * H * Wd and H * Wd > W.FIX_CAP, (what, count)
        assert count == B * H * Wd, (what, count)
    else:
        assert 0 < count < B * W.FIX_CAP, (what, count)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. dw_run_episode_mlp, exact mode, against the oracle with OracleMLP policies
# ---------------------------------------------------------------------------------------------------------------------
CASES_MLP = [(s, K) for s in W.SHAPES_B + W.LDS_EDGE_B for K in W.ks_b(s)]


@pytest.mark.parametrize("shape,K", CASES_MLP, ids=_ids)
def test_run_episode_mlp_exact_vs_oracle(amd, monkeypatch, shape, K):
    """K steps with three random parameter sets shared out per world (member_a != member_b), then 5 more with the
    parameter sets still on the device (params=None): reward and done of every step, the final state after either chunk."""
    B, H, Wd, N, split = shape
    what = f"mlp {shape} K={K}"
    eng = _engine(amd, monkeypatch, shape, "exact", agent_gamma=W.MLP_AGENT_GAMMA)
    _assert_form(eng, "mlp episode", W.WORKGROUP)
    inp, ref = W.inputs_b(shape), W.reference_b(shape)
    _begin(eng, inp, ref["start"])
    ma, mb = inp["member_a"], inp["member_b"]

    Ls = W.mlp_schedule(K)
    reward, done = eng.run_episode_mlp(Ls, inp["params"], ma, mb, split=split)
    assert reward.shape == (K, B, N, 1)
    assert np.array_equal(reward, ref["reward"][:K]), f"{what}: reward"
    assert np.array_equal(done, ref["done"][:K]), f"{what}: done"
    _compare_final(eng, ref["final"][K], Ls[-1], what)

    Ls2 = W.mlp_schedule(W.K2_B, K)
    reward, done = eng.run_episode_mlp(Ls2, None, ma, mb, split=split, n_members=W.N_MEMBERS)
    assert np.array_equal(reward, ref["reward"][K:K + W.K2_B]), f"{what}: reward of the second chunk"
    assert np.array_equal(done, ref["done"][K:K + W.K2_B]), f"{what}: done of the second chunk"
    _compare_final(eng, ref["final"][K + W.K2_B], Ls2[-1], what + " second chunk")
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. dw_run_episode_mlp, float32-only
# ---------------------------------------------------------------------------------------------------------------------
def _outputs_mlp_fast(amd, monkeypatch, shape, switch, form):
    B, H, Wd, N, split = shape
    eng = _engine(amd, monkeypatch, shape, "fast", switch, agent_gamma=W.MLP_AGENT_GAMMA)
    _assert_form(eng, "mlp episode", form)
    inp = W.inputs_b(shape)
    _begin(eng, inp)
    Ls = W.mlp_schedule(max(W.KS_B))
    reward, done = eng.run_episode_mlp(Ls, inp["params"], inp["member_a"], inp["member_b"], split=split)
    out = _everything(eng, Ls[-1])
    out.update(rewards=reward.copy(), dones=done.copy())
    eng.close()
    return out


@pytest.mark.parametrize("shape", W.SHAPES_B, ids=_ids)
def test_run_episode_mlp_fast_equals_launches_per_step(amd, monkeypatch, shape):
    """20 steps through episode_mlp<false> and as launches per step: every output identical (the planes are float32
    results that do not depend on the family, so neither do the observations the networks decide on)."""
    a = _outputs_mlp_fast(amd, monkeypatch, shape, None, W.WORKGROUP)
    b = _outputs_mlp_fast(amd, monkeypatch, shape, "DW_NO_EPISODE_KERNEL", W.STEPWISE)
    assert a["max_k"].min() > W.THRESHOLD_K and len(np.unique(a["action"])) > 1
    for name in a:
        assert np.array_equal(a[name], b[name]), f"{shape}: {name}"


# ---------------------------------------------------------------------------------------------------------------------
# 8. beyond the limits: dispatch only
# ---------------------------------------------------------------------------------------------------------------------
def test_a_world_of_4097_cells_runs_as_launches_per_step(amd, monkeypatch):
    eng = _engine(amd, monkeypatch, W.DISPATCH_A, "exact")
    _assert_form(eng, "episode", W.STEPWISE)
    _assert_form(eng, "mlp episode", W.STEPWISE)
    eng.close()


@pytest.mark.parametrize("shape,within", list(zip(W.DISPATCH_B, W.LDS_EDGE_B)), ids=_ids)
def test_one_agent_beyond_the_lds_limit_runs_as_launches_per_step(amd, monkeypatch, shape, within):
    """episode_mlp_form dispatches on episode_mlp_world_bytes(C, N) * wpb <= 160 KiB: the largest N within it is the
    workgroup form (run in section 6), one agent more is not."""
    eng = _engine(amd, monkeypatch, shape, "exact", agent_gamma=W.MLP_AGENT_GAMMA)
    _assert_form(eng, "mlp episode", W.STEPWISE)
    _assert_form(eng, "episode", W.WORKGROUP)                   # episode_small keeps no activations: it still fits
    eng.close()
    eng = _engine(amd, monkeypatch, (shape[0], *within[1:]), "exact", agent_gamma=W.MLP_AGENT_GAMMA)
    _assert_form(eng, "mlp episode", W.WORKGROUP)
    eng.close()
