"""The agent kernels under observation masks other than the default (`dw_params.obs_mask`, the reference's
neighborhood_mode) against the float64 oracle with `env.neighborhood` set to the same 3 x 3 array (run with ``-m gpu``).
With the default von Neumann mask all four greedy candidates are visible and the corners are not: the "masked candidate
counts as 0.0" side of every greedy select, and the float64 cell evaluation, double wrap and agent-stamp search of a
diagonal cell in the MLP observation builders, run only under the masks of this file.

The cases, their inputs and the oracle references are the table tools/obs_mask_cases.py;
tests/test_obs_mask_cases_cpu.py asserts without a GPU that each reference could not be met by a kernel that ignored the
mask.  Protocol of every case: ``upload_state_f32(quantised=True)``, ``upload_agents``, one zero-action ``dw_step`` at L0
(the state the call starts from is asserted equal to the oracle's), then the call under test with ``p.obs_mask = mask``.

  1  dw_run_episode, exact, K in {1, 65}, policies argmax / argmin (with use_table) / table, every form of every shape
  2  the same calls float32-only: bit-identical across the forms of a shape
  3  the record-keeping wave kernels: trace, temperature trace, ensemble (with and without records), frames
  4  dw_run_episode_mlp and dw_run_episode_mlp_trace with OracleMLP policies
  5  the per-step calls: policy_greedy, policy_per_agent, get_obs, policy_mlp, policy_mlp_population
  6  a mask change on a live handle (dw_set_params between two chunks; env.neighborhood between two steps)
  7  simulate_grazing_mlp on a neighborhood_mode="moore" drop-in

Everything compared is integer-valued or float64-exact in the contract: exact equality, but for the un-rounded
temperature channels of an un-quantised state in group 5 (see there).  Every test asserts from ``kernel_info()`` which
form it runs.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import obs_mask_cases as M  # noqa: E402
from constant_edge_cases import ALL_SWITCHES  # noqa: E402
from oracle import daisy_oracle as O  # noqa: E402

SWITCHES = ALL_SWITCHES + ("DW_NO_AGENT_FUSE", "DW_NO_AGENT_PREAPPLY")
FIELDS = ("max_k", "sum_light_k", "sum_dark_k")
_ids = lambda v: hex(v) if isinstance(v, int) and not isinstance(v, bool) else str(v).replace(" ", "")  # noqa: E731


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _engine(amd, monkeypatch, shape, precision, mask, switch=None, agent_gamma=None, over=None):
    """A handle with `obs_mask = mask`, created under exactly one (or none) of the library's switches."""
    from therldaisyworld_amd import _ffi
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")
    p = amd.default_params(*shape[:4])
    p.precision = _ffi.PRECISION[precision]
    p.obs_mask = mask
    if agent_gamma is not None:
        p.agent_gamma = agent_gamma
    for k, v in (over or {}).items():
        setattr(p, k, v)
    eng = amd.Engine(p)
    assert eng.params.obs_mask == mask
    return eng


def _assert_form(eng, what, form):
    info = eng.kernel_info()
    assert f"; {what}: {form}" in info, info


def _begin(eng, inp, start=None, worlds=slice(None)):
    """Steps 1 to 3 of the protocol; `start`: the oracle's state after them, which the engine must hold."""
    B, N = eng.B, eng.N
    eng.upload_state_f32(inp["light"][worlds].astype(np.float32), inp["dark"][worlds].astype(np.float32), quantised=True)
    eng.upload_agents(inp["idx"][worlds], inp["st"][worlds])
    eng.step(M.L0, np.zeros((B, N, 1), dtype=np.int64))
    if start is not None:
        gl, gd = eng.download_planes()
        idx, st = eng.download_agents()
        assert np.array_equal(M.k_of(gl), start["light"]) and np.array_equal(M.k_of(gd), start["dark"]), "start planes"
        assert np.array_equal(idx, start["idx"]) and np.array_equal(st, start["st"]), "start agents"


def _compare_final(eng, ref, L_last, what, obs=True):
    from therldaisyworld_amd import _ffi
    gl, gd = eng.download_planes()
    assert np.array_equal(M.k_of(gl), ref["light"]), f"{what}: light plane"
    assert np.array_equal(M.k_of(gd), ref["dark"]), f"{what}: dark plane"
    pl, pd = eng.download_planes(_ffi.STATE_PREVIOUS)
    assert np.array_equal(M.k_of(pl), ref["prev_light"]), f"{what}: previous light plane"
    assert np.array_equal(M.k_of(pd), ref["prev_dark"]), f"{what}: previous dark plane"
    idx, st = eng.download_agents()
    assert np.array_equal(idx, ref["idx"]), f"{what}: agent positions"
    assert np.array_equal(st[..., None], ref["st"]), f"{what}: agent states"
    r_dev, d_dev = eng.reward_done()
    assert np.array_equal(r_dev, ref["reward"]) and np.array_equal(d_dev, ref["done"]), f"{what}: reward / done"
    s = eng.reduce()
    for f in FIELDS:
        assert np.array_equal(s[f], ref[f]), f"{what}: reduce() {f}"
    if obs:                                                      # (a handle left "per-world" by the ensemble call has none)
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


def _mode(name):
    from therldaisyworld_amd import _ffi
    return getattr(_ffi, "POLICY_" + name)


# ---------------------------------------------------------------------------------------------------------------------
# the forms of a shape
# ---------------------------------------------------------------------------------------------------------------------
def _forms(shape):
    """[(switch, the episode form kernel_info() must name)] - the default first."""
    if shape in M.WAVE_SHAPES:
        return [(None, M.WAVE), ("DW_NO_EPISODE_WAVE", M.WORKGROUP), ("DW_NO_EPISODE_KERNEL", M.STEPWISE)]
    if shape in M.WORKGROUP_SHAPES:
        return [(None, M.WORKGROUP)]
    return [(None, M.STEPWISE), ("DW_NO_AGENT_FUSE", M.STEPWISE)]


def _assert_episode_form(eng, shape, form):
    _assert_form(eng, "episode", form)
    if shape in M.WIDE_SHAPES:                                   # the plan allows step pairs: with agents, runs of three and
        assert M.PAIRS in eng.kernel_info(), eng.kernel_info()   # more steps take agents_lookahead_patch unless switched off


RUNS_1 = [(s, sw, form, m, pol, K) for s in M.SHAPES_1 for sw, form in _forms(s) for m in M.masks_of_group(M.GREEDY_MASKS)
          for pol in M.POLICIES for K in M.KS]


# ---------------------------------------------------------------------------------------------------------------------
# 1. dw_run_episode, exact mode, against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,switch,form,mask,policy,K", RUNS_1, ids=_ids)
def test_run_episode_exact_vs_oracle(amd, monkeypatch, shape, switch, form, mask, policy, K):
    """Greedy choice under a mask, per form: one wave per world - ew_policy_action (dw_episode_wave.hpp:190) in
    episode_wave; workgroup - episode_small (dw_episode.hpp:245), also the wave shapes under DW_NO_EPISODE_WAVE; launches
    per step - policy_greedy (dw_agents.hpp:173; the wave shapes under DW_NO_EPISODE_KERNEL, the wide shapes under
    DW_NO_AGENT_FUSE) and, on the wide shapes by default, both candidate loops of agents_lookahead_patch
    (dw_agents_fused.hpp:138, :281: K = 65 is 31 step pairs with the next step's policy pre-applied, then three single
    steps' worth).  World and agent flags of every step, planes (current and previous), agents, reward / done, reduce(),
    get_obs and the last action codes, all equal to the oracle's."""
    what = f"{shape} {hex(mask)} K={K} {policy} {switch or 'default'}"
    eng = _engine(amd, monkeypatch, shape, "exact", mask, switch)
    _assert_episode_form(eng, shape, form)
    inp, ref = M.inputs_1(shape), M.reference_1(shape, mask, policy)
    _begin(eng, inp, ref["start"])
    mode, ut, table = M.call_of(shape, policy, K)
    Ls = M.schedule(K)
    alive, ok = eng.run_episode(Ls, _mode(mode), ut, table, threshold_k=M.THRESHOLD_K)
    for t in range(K):
        assert np.array_equal(alive[t], ref["alive"][t]), f"{what}: world_alive[{t}]"
        assert np.array_equal(ok[t], ref["ok"][t]), f"{what}: agent_ok[{t}]"
    _compare_final(eng, ref["final"][K], Ls[-1], what)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. float32-only: results are identical across the forms
# ---------------------------------------------------------------------------------------------------------------------
def _outputs_fast(amd, monkeypatch, shape, mask, policy, K, switch, form):
    eng = _engine(amd, monkeypatch, shape, "fast", mask, switch)
    _assert_episode_form(eng, shape, form)
    _begin(eng, M.inputs_1(shape))
    mode, ut, table = M.call_of(shape, policy, K)
    Ls = M.schedule(K)
    alive, ok = eng.run_episode(Ls, _mode(mode), ut, table, threshold_k=M.THRESHOLD_K)
    out = _everything(eng, Ls[-1])
    out.update(alive=alive.copy(), ok=ok.copy())
    eng.close()
    return out


@pytest.mark.parametrize("K", M.KS)
@pytest.mark.parametrize("policy", M.POLICIES)
@pytest.mark.parametrize("mask", M.masks_of_group(M.GREEDY_MASKS), ids=_ids)
@pytest.mark.parametrize("shape", M.SHAPES_1, ids=_ids)
def test_run_episode_fast_is_the_same_in_every_form(amd, monkeypatch, shape, mask, policy, K):
    """The float32-only instantiations of the kernels of group 1: ew_policy_action (dw_episode_wave.hpp:190) in
    episode_wave<false>, episode_small<false> (dw_episode.hpp:245), policy_greedy (dw_agents.hpp:173) and both candidate
    loops of agents_lookahead_patch<false> (dw_agents_fused.hpp:138, :281).  Float32 is not the oracle's arithmetic; the library's own invariant is
    that its results - here with greedy decisions riding on them - do not depend on the form: every output of every
    form of a shape is bit-identical to the default form's.  A workgroup shape has the one resident form and launches per
    step (DW_NO_EPISODE_KERNEL)."""
    forms = _forms(shape) + ([("DW_NO_EPISODE_KERNEL", M.STEPWISE)] if shape in M.WORKGROUP_SHAPES else [])
    outs = [_outputs_fast(amd, monkeypatch, shape, mask, policy, K, sw, form) for sw, form in forms]
    assert outs[0]["max_k"].max() > M.THRESHOLD_K                # (not a comparison of dead worlds)
    for (sw, _), other in zip(forms[1:], outs[1:]):
        for name in outs[0]:
            assert _bits(outs[0][name]) == _bits(other[name]), f"{shape} {hex(mask)} {policy} K={K}: {name} under {sw}"


# ---------------------------------------------------------------------------------------------------------------------
# 3. the record-keeping wave kernels
# ---------------------------------------------------------------------------------------------------------------------
K3, STRIDE3 = M.K_MAX, 2
_LOOPS = {}


def _per_step_loop(amd, monkeypatch, key, inp, actions, Ls, mask, worlds=slice(None), over=None):
    """The records' reference: `step` + `reduce` + `reduce_temperature` + `reduce_tiles` (1 x 1 tiles) + `download_agents`
    per step on a handle of its own, fed the oracle's actions - computed once per key.  `over`: constants set after the
    quantising step (which is the ensemble handle's own)."""
    if key in _LOOPS:
        return _LOOPS[key]
    from therldaisyworld_amd import _ffi
    B, H, Wd = inp["light"][worlds].shape
    N = inp["idx"].shape[1]
    eng = _engine(amd, monkeypatch, (B, H, Wd, N), "exact", mask)
    _begin(eng, inp, worlds=worlds)
    if over:
        p = amd.default_params(B, H, Wd, N)
        p.precision, p.obs_mask = _ffi.PRECISION["exact"], mask
        for k, v in over.items():
            setattr(p, k, v)
        eng.set_params(p)
    K = len(Ls)
    out = {"stats": np.zeros((K, B), dtype=_ffi.STATS_DTYPE), "temps": np.zeros((K, B), dtype=_ffi.TEMP_STATS_DTYPE),
           "cover": [], "temp": [], "agents": []}
    for t in range(K):
        eng.step(float(Ls[t]), actions[t][..., None])
        out["stats"][t], out["temps"][t] = eng.reduce(), eng.reduce_temperature(float(Ls[t]))
        if (t + 1) % STRIDE3 == 0:
            cov, tmp = eng.reduce_tiles(float(Ls[t]), tile=(1, 1))
            idx, st = eng.download_agents()
            out["cover"].append(cov), out["temp"].append(tmp), out["agents"].append((idx, st))
    eng.close()
    _LOOPS[key] = out
    return out


def _assert_rows(stats, temps, loop, what):
    if stats is not None:
        for f in FIELDS:
            assert np.array_equal(stats[f], loop["stats"][f]), f"{what}: stats {f}"
        assert not stats["reserved"].any()
    if temps is not None:
        assert _bits(temps) == _bits(loop["temps"]), f"{what}: temperature rows"


RECORD_CALLS = ("trace", "trace+temperature", "ensemble", "ensemble+records", "frames")


@pytest.mark.parametrize("call", RECORD_CALLS)
@pytest.mark.parametrize("mask", M.RECORD_MASKS, ids=_ids)
@pytest.mark.parametrize("shape", M.RECORD_SHAPES, ids=_ids)
def test_record_keeping_wave_kernels(amd, monkeypatch, shape, mask, call):
    """ew_policy_action (dw_episode_wave.hpp:190) as called by episode_wave_stats_pw (run_episode_trace),
    episode_wave_temp_pw (temperature=True), episode_wave_pw / episode_wave_ens_trace_pw (run_episode_ensemble without /
    with records, the handle's own constants in every row) and episode_wave_frames_pw (run_episode_frames, stride 2,
    1 x 1 tiles, all worlds): 65 table steps; flags and final state are group 1's oracle reference, the records those of the
    per-step loop."""
    what = f"{shape} {hex(mask)} {call}"
    B, H, Wd, N = shape
    eng = _engine(amd, monkeypatch, shape, "exact", mask)
    info = eng.kernel_info()
    for name in ("episode", "ensemble episode", "episode trace"):
        assert f"; {name}: {M.WAVE}" in info, info
    inp, ref = M.inputs_1(shape), M.reference_1(shape, mask, "table")
    _begin(eng, inp, ref["start"])
    Ls, codes = M.schedule(K3), inp["codes"]
    loop = _per_step_loop(amd, monkeypatch, (shape, mask), inp, ref["action"], Ls, mask)
    stats = temps = None
    mode = _mode("TABLE")
    if call == "trace":
        stats, alive, ok = eng.run_episode_trace(Ls, mode, None, codes, threshold_k=M.THRESHOLD_K)
    elif call == "trace+temperature":
        stats, alive, ok, temps = eng.run_episode_trace(Ls, mode, None, codes, threshold_k=M.THRESHOLD_K, temperature=True)
    elif call.startswith("ensemble"):
        tab, L2 = np.repeat(eng.world_params()[None], B), np.ascontiguousarray(np.repeat(Ls[:, None], B, axis=1))
        if call == "ensemble":
            alive, ok = eng.run_episode_ensemble(tab, L2, mode, None, codes, threshold_k=M.THRESHOLD_K)
        else:
            alive, ok, stats, temps = eng.run_episode_ensemble(tab, L2, mode, None, codes, threshold_k=M.THRESHOLD_K,
                                                               trace=True, temperature=True)
    else:
        cov, tmp, ag, stats, alive, ok, temps = eng.run_episode_frames(Ls, mode, None, codes, threshold_k=M.THRESHOLD_K,
                                                                       stride=STRIDE3, tile=(1, 1), temps=True)
        assert cov.shape == (K3 // STRIDE3, B, H, Wd) and ag.shape == (K3 // STRIDE3, B, N)
        for f in range(K3 // STRIDE3):
            assert _bits(cov[f]) == _bits(loop["cover"][f]), f"{what}: cover frame {f}"
            assert _bits(tmp[f]) == _bits(loop["temp"][f]), f"{what}: temperature frame {f}"
            idx, st = loop["agents"][f]
            assert np.array_equal(ag["row"][f], idx[..., 0]) and np.array_equal(ag["col"][f], idx[..., 1]), f"{what}: agent frame {f}"
            assert np.array_equal(ag["state"][f], st), f"{what}: agent states of frame {f}"
    assert np.array_equal(alive, ref["alive"]), f"{what}: world_alive"
    assert np.array_equal(ok, ref["ok"]), f"{what}: agent_ok"
    _assert_rows(stats, temps, loop, what)
    _compare_final(eng, ref["final"][K3], Ls[-1], what, obs=not call.startswith("ensemble"))
    eng.close()


@pytest.mark.parametrize("records", [False, True], ids=["flags", "records"])
@pytest.mark.parametrize("mask", M.RECORD_MASKS, ids=_ids)
@pytest.mark.parametrize("shape", M.RECORD_SHAPES, ids=_ids)
def test_ensemble_with_constants_per_world(amd, monkeypatch, shape, mask, records):
    """episode_wave_pw / episode_wave_ens_trace_pw with constants of its own for every world (M.ensemble_constants) and a
    luminosity column per world: every world ends, and reports flags, as a one-world oracle with those constants under the
    mask; the records are those of a per-step loop on one-world handles with those constants."""
    what = f"{shape} {hex(mask)} per-world constants"
    B, H, Wd, N = shape
    eng = _engine(amd, monkeypatch, shape, "exact", mask)
    _assert_form(eng, "ensemble episode", M.WAVE)
    inp, ref = M.inputs_1(shape), M.reference_ensemble(shape, mask)
    _begin(eng, inp)
    tab = np.repeat(eng.world_params()[None], B)
    for b in range(B):
        for name, v in M.ensemble_constants(b).items():
            tab[name][b] = v
    L2 = M.ensemble_schedule(B, K3)
    mode = _mode("TABLE")
    if records:
        alive, ok, stats, temps = eng.run_episode_ensemble(tab, L2, mode, None, inp["codes"], threshold_k=M.THRESHOLD_K,
                                                           trace=True, temperature=True)
        for b in range(B):
            loop = _per_step_loop(amd, monkeypatch, (shape, mask, b), inp, ref["action"][:, b:b + 1], L2[:, b], mask,
                                  worlds=slice(b, b + 1), over=M.ensemble_constants(b))
            _assert_rows(stats[:, b:b + 1], temps[:, b:b + 1], loop, f"{what}: world {b}")
    else:
        alive, ok = eng.run_episode_ensemble(tab, L2, mode, None, inp["codes"], threshold_k=M.THRESHOLD_K)
    assert np.array_equal(alive, ref["alive"]), f"{what}: world_alive"
    assert np.array_equal(ok, ref["ok"]), f"{what}: agent_ok"
    gl, gd = eng.download_planes()
    assert np.array_equal(M.k_of(gl), ref["light"]) and np.array_equal(M.k_of(gd), ref["dark"]), f"{what}: planes"
    idx, st = eng.download_agents()
    assert np.array_equal(idx, ref["idx"]) and np.array_equal(st, ref["st"]), f"{what}: agents"
    r_dev, d_dev = eng.reward_done()
    assert np.array_equal(r_dev, ref["reward"]) and np.array_equal(d_dev, ref["done"]), f"{what}: reward / done"
    assert np.array_equal(eng.download_actions(), ref["action"][-1]), f"{what}: action codes of the last step"
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. dw_run_episode_mlp / dw_run_episode_mlp_trace
# ---------------------------------------------------------------------------------------------------------------------
def _mlp_forms(shape):
    form = M.mlp_form_of(shape)
    return [(None, form)] + ([("DW_NO_EPISODE_KERNEL", M.STEPWISE)] if form == M.WAVE else [])


RUNS_4 = [(s, sw, form, m, K) for s in M.SHAPES_4 for sw, form in _mlp_forms(s) for m in M.masks_of_group(M.MASKS) for K in M.KS]


@pytest.mark.parametrize("shape,switch,form,mask,K", RUNS_4, ids=_ids)
def test_run_episode_mlp_exact_vs_oracle(amd, monkeypatch, shape, switch, form, mask, K):
    """The in-kernel observation builders: episode_mlp_wave (dw_episode_wave.hpp:474) on the wave shapes, episode_mlp
    (dw_episode.hpp:389) on N = 5 and on 17 x 17; under DW_NO_EPISODE_KERNEL the `observe` kernel feeds policy_mlp.  With
    the corners visible, lanes 0, 2, 6, 8 of a patch evaluate a diagonal neighbour in float64, wrap row and column at once
    and search the agent list for a stamp.  K steps with three parameter sets shared out per world, then K2 more with the
    sets still on the device (params=None): reward and done of every step, the final state after either chunk."""
    B, H, Wd, N, split = shape
    what = f"mlp {shape} {hex(mask)} K={K} {switch or 'default'}"
    eng = _engine(amd, monkeypatch, shape, "exact", mask, switch, agent_gamma=M.MLP_AGENT_GAMMA)
    _assert_form(eng, "mlp episode", form)
    inp, ref = M.inputs_4(shape), M.reference_4(shape, mask)
    _begin(eng, inp, ref["start"])
    ma, mb = inp["member_a"], inp["member_b"]
    Ls = M.schedule(K)
    reward, done = eng.run_episode_mlp(Ls, inp["params"], ma, mb, split=split, L_init=M.L0)
    assert reward.shape == (K, B, N, 1)
    assert np.array_equal(reward, ref["reward"][:K]), f"{what}: reward"
    assert np.array_equal(done, ref["done"][:K]), f"{what}: done"
    _compare_final(eng, ref["final"][K], Ls[-1], what)
    Ls2 = M.schedule(M.K2, K)
    reward, done = eng.run_episode_mlp(Ls2, None, ma, mb, split=split, L_init=Ls[-1], n_members=M.N_MEMBERS)
    assert np.array_equal(reward, ref["reward"][K:K + M.K2]), f"{what}: reward of the second chunk"
    assert np.array_equal(done, ref["done"][K:K + M.K2]), f"{what}: done of the second chunk"
    _compare_final(eng, ref["final"][K + M.K2], Ls2[-1], what + " second chunk")
    eng.close()


@pytest.mark.parametrize("shape,switch,form,mask,K", RUNS_4, ids=_ids)
def test_run_episode_mlp_trace_vs_oracle_and_loop(amd, monkeypatch, shape, switch, form, mask, K):
    """dw_run_episode_mlp_trace: on the wave shapes episode_mlp_wave_trace_pw (dw_episode_mlp_wave_trace_pw.hpp:124), the
    third copy of the observation builder.  Reward, done and final state are the oracle's, the cover and temperature rows
    those of the per-step loop (`step` with the oracle's actions + `reduce` + `reduce_temperature`)."""
    from therldaisyworld_amd import _ffi
    B, H, Wd, N, split = shape
    what = f"mlp trace {shape} {hex(mask)} K={K} {switch or 'default'}"
    eng = _engine(amd, monkeypatch, shape, "exact", mask, switch, agent_gamma=M.MLP_AGENT_GAMMA)
    _assert_form(eng, "mlp episode", form)
    inp, ref = M.inputs_4(shape), M.reference_4(shape, mask)
    _begin(eng, inp, ref["start"])
    Ls = M.schedule(K)
    reward, done, stats, temps = eng.run_episode_mlp(Ls, inp["params"], inp["member_a"], inp["member_b"], split=split,
                                                     L_init=M.L0, trace=True, temperature=True)
    assert np.array_equal(reward, ref["reward"][:K]), f"{what}: reward"
    assert np.array_equal(done, ref["done"][:K]), f"{what}: done"
    _compare_final(eng, ref["final"][K], Ls[-1], what)
    eng.close()
    key = ("mlp", shape, mask)
    if key not in _LOOPS:
        loop_eng = _engine(amd, monkeypatch, shape, "exact", mask, agent_gamma=M.MLP_AGENT_GAMMA)
        _begin(loop_eng, inp)
        rows = {"stats": np.zeros((M.K_MAX, B), dtype=_ffi.STATS_DTYPE), "temps": np.zeros((M.K_MAX, B), dtype=_ffi.TEMP_STATS_DTYPE)}
        Lall = M.schedule(M.K_MAX)
        for t in range(M.K_MAX):
            loop_eng.step(float(Lall[t]), ref["action"][t][..., None])
            rows["stats"][t], rows["temps"][t] = loop_eng.reduce(), loop_eng.reduce_temperature(float(Lall[t]))
        loop_eng.close()
        _LOOPS[key] = rows
    loop = {k: v[:K] for k, v in _LOOPS[key].items()}
    _assert_rows(stats, temps, loop, what)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the per-step calls
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantised", [True, False], ids=["quantised", "raw"])
@pytest.mark.parametrize("mask", M.masks_of_group(M.GREEDY_MASKS), ids=_ids)
@pytest.mark.parametrize("shape", M.SHAPES_5, ids=_ids)
def test_per_step_calls_vs_oracle(amd, monkeypatch, shape, mask, quantised):
    """policy_greedy (dw_agents.hpp:173) in both modes and through dw_policy_per_agent; `observe` (dw_agents.hpp:87)
    through get_obs, then policy_mlp and policy_mlp_population on agents [1, 3) - each against OracleGreedy / OracleMLP
    on the masked oracle observation.  quantised: after the protocol's zero-action step.  raw: straight after an
    un-quantised float32 upload (an exact float64 initial state has no device policy; the handle keeps float32 per-mille
    values, and the oracle is given what download_planes returns, as tests/test_gpu_episode_wave.py does) -
    policy_greedy<float> and observe<.., POST = false>, whose temperature channels are
    UN-rounded: the C oracle's pow() and the device's roots agree to a few 1e-16 relative there (oracle/daisy_oracle.py,
    OracleDaisyWorldC), so channels 3 .. 5 are compared to 1e-12 relative as tests/test_gpu_parity.py compares a reset's
    observations, the covers exactly; a decision is at least MARGIN = 1e-9 clear (asserted on the CPU)."""
    from therldaisyworld_amd import _ffi
    B, H, Wd, N = shape
    what = f"{shape} {hex(mask)} {'quantised' if quantised else 'raw'}"
    eng = _engine(amd, monkeypatch, shape, "exact", mask)
    inp, ref = M.inputs_5(shape), M.reference_5(shape, mask, quantised)
    if quantised:
        _begin(eng, inp, ref["start"])
    else:
        eng.upload_state_f32(inp["upload_light"], inp["upload_dark"], quantised=False)
        gl, gd = eng.download_planes()                           # (the reference was given what the handle holds)
        assert np.array_equal(gl, inp["raw_light"]) and np.array_equal(gd, inp["raw_dark"]), f"{what}: the state held"
        eng.upload_agents(inp["idx"], inp["st"])
    eng.policy_greedy(argmin=False)
    assert np.array_equal(eng.download_actions(), ref["argmax"]), f"{what}: policy_greedy argmax"
    eng.policy_greedy(argmin=True)
    assert np.array_equal(eng.download_actions(), ref["argmin"]), f"{what}: policy_greedy argmin"
    for rotation, want in zip(M.ROTATIONS, ref["per_agent"]):   # every agent takes every mode once
        eng.upload_actions(inp["kept"])
        modes = np.array([_ffi.POLICY_ARGMAX, _ffi.POLICY_ARGMIN, _ffi.POLICY_TABLE], dtype=np.int32)[M.per_agent_modes(N, rotation)]
        eng.policy_per_agent(modes)
        assert np.array_equal(eng.download_actions(), want), f"{what}: policy_per_agent, rotation {rotation}"
    obs = eng.get_obs(M.L0)
    if quantised:
        assert np.array_equal(obs, ref["obs"]), f"{what}: get_obs"
    else:
        assert np.array_equal(obs[:, :, :3], ref["obs"][:, :, :3]) and np.array_equal(obs[:, :, 6], ref["obs"][:, :, 6]), f"{what}: covers"
        np.testing.assert_allclose(obs[:, :, 3:6], ref["obs"][:, :, 3:6], rtol=1e-12, atol=0, err_msg=f"{what}: temperatures")
        assert np.array_equal(obs == 0.0, ref["obs"] == 0.0), f"{what}: what the mask zeroes"
    if mask:                                                     # (nothing visible: all-equal logits, no MLP case)
        eng.policy_mlp(inp["params"][0], L_init=M.L0)
        assert np.array_equal(eng.download_actions(), ref["mlp"]), f"{what}: policy_mlp"
        eng.upload_actions(inp["kept"])
        eng.policy_mlp_population(inp["params"], inp["member"], *M.AGENT_RANGE, L_init=M.L0)
        assert np.array_equal(eng.download_actions(), ref["population"]), f"{what}: policy_mlp_population"
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. a mask change on a live handle
# ---------------------------------------------------------------------------------------------------------------------
def _set_mask(eng, mask):
    from therldaisyworld_amd.engine import DwParams
    import ctypes as C
    p = DwParams()
    C.memmove(C.byref(p), C.byref(eng.params), C.sizeof(DwParams))
    p.obs_mask = mask
    eng.set_params(p)
    assert eng.params.obs_mask == mask


@pytest.mark.parametrize("first,second", M.CHANGES_GREEDY, ids=_ids)
def test_mask_change_between_two_greedy_chunks(amd, monkeypatch, first, second):
    """episode_wave: 65 table steps under `first`, dw_set_params with `second` on the live handle (its staging buffers are
    on the device), 7 more steps: both chunks equal an oracle whose neighborhood changed at the same step."""
    shape = M.CHANGE_GREEDY_SHAPE
    what = f"{shape} {hex(first)} -> {hex(second)}"
    eng = _engine(amd, monkeypatch, shape, "exact", first)
    _assert_form(eng, "episode", M.WAVE)
    ref = M.reference_change_greedy(first, second)
    _begin(eng, M.inputs_1(shape), ref["start"])
    K1, T = M.CHANGE_K1, M.CHANGE_K1 + M.CHANGE_K2
    Ls, mode = M.schedule(T), _mode("TABLE")
    alive, ok = eng.run_episode(Ls[:K1], mode, None, ref["codes"][:K1], threshold_k=M.THRESHOLD_K)
    assert np.array_equal(alive, ref["alive"][:K1]) and np.array_equal(ok, ref["ok"][:K1]), f"{what}: flags of the first chunk"
    _compare_final(eng, ref["final"][K1], Ls[K1 - 1], what + " first chunk")
    _set_mask(eng, second)
    alive, ok = eng.run_episode(Ls[K1:], mode, None, ref["codes"][K1:], threshold_k=M.THRESHOLD_K)
    assert np.array_equal(alive, ref["alive"][K1:]) and np.array_equal(ok, ref["ok"][K1:]), f"{what}: flags of the second chunk"
    _compare_final(eng, ref["final"][T], Ls[-1], what + " second chunk")
    eng.close()


@pytest.mark.parametrize("first,second", M.CHANGES_MLP, ids=_ids)
def test_mask_change_between_two_mlp_chunks(amd, monkeypatch, first, second):
    """episode_mlp_wave: 65 steps under `first`, dw_set_params with `second` while the handle keeps the parameter sets on
    the device, 7 more steps with params=None."""
    shape = M.CHANGE_MLP_SHAPE
    what = f"mlp {shape} {hex(first)} -> {hex(second)}"
    eng = _engine(amd, monkeypatch, shape, "exact", first, agent_gamma=M.MLP_AGENT_GAMMA)
    _assert_form(eng, "mlp episode", M.WAVE)
    inp, ref = M.inputs_4(shape), M.reference_change_mlp(first, second)
    _begin(eng, inp, ref["start"])
    K1, T = M.CHANGE_K1, M.CHANGE_K1 + M.CHANGE_K2
    Ls = M.schedule(T)
    ma, mb, split = inp["member_a"], inp["member_b"], shape[4]
    reward, done = eng.run_episode_mlp(Ls[:K1], inp["params"], ma, mb, split=split, L_init=M.L0)
    assert np.array_equal(reward, ref["reward"][:K1]) and np.array_equal(done, ref["done"][:K1]), f"{what}: first chunk"
    _compare_final(eng, ref["final"][K1], Ls[K1 - 1], what + " first chunk")
    _set_mask(eng, second)
    reward, done = eng.run_episode_mlp(Ls[K1:], None, ma, mb, split=split, L_init=Ls[K1 - 1], n_members=M.N_MEMBERS)
    assert np.array_equal(reward, ref["reward"][K1:]) and np.array_equal(done, ref["done"][K1:]), f"{what}: second chunk"
    _compare_final(eng, ref["final"][T], Ls[-1], what + " second chunk")
    eng.close()


@pytest.mark.parametrize("first,second", M.CHANGES_MLP, ids=_ids)
def test_dropin_neighborhood_assigned_between_steps(amd, first, second):
    """The drop-in reads `env.neighborhood` live (daisy_world_rl.py: `_param_key` :153, `_params` :159) and pushes
    dw_set_params when it changed: four greedy steps under `first`, `env.neighborhood = ...`, four more - observations
    (`observe<.., POST = true>`, dw_agents.hpp:87, mask test :103), rewards and grids equal an oracle whose neighborhood was
    changed at the same step.  The actions are OracleGreedy's on the ORACLE's observations (argmax and argmin in turn; the
    drop-in's are asserted equal to them at every step), so a wrong mask changes the course."""
    np.random.seed(9)
    env = amd.RLDaisyWorld(grid_dimension=8, n_agents=3)
    env.batch_size = 4
    env.neighborhood = M.mask_array(first)
    obs = env.reset()
    np.random.seed(9)
    ref = O.OracleDaisyWorld.like_reference_ctor(grid_dimension=8, n_agents=3)
    ref.P.batch_size = 4
    ref.neighborhood = M.mask_array(first)
    robs = ref.reset()
    np.testing.assert_allclose(obs, robs, rtol=1e-12, atol=0)
    for t in range(8):
        if t == 4:
            env.neighborhood = M.mask_array(second)
            ref.neighborhood = M.mask_array(second)
        a = O.OracleGreedy(epsilon=0.0, greedy=t % 2 == 0)(robs)
        obs, reward, done, _ = env.step(a)
        robs, rreward, rdone, _ = ref.step(a)
        assert np.array_equal(obs, robs), f"{hex(first)} -> {hex(second)}: observations of step {t}"
        assert np.array_equal(reward, rreward) and np.array_equal(done, rdone), f"rewards of step {t}"
    assert np.array_equal(env.grid, ref.grid)
    env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the harness on a Moore drop-in
# ---------------------------------------------------------------------------------------------------------------------
def test_simulate_grazing_mlp_on_a_moore_dropin(amd):
    """simulate_grazing_mlp on neighborhood_mode="moore" (8 x 8, 4 agents, 6 worlds, 40 steps in chunks of 16): the first
    step from the un-quantised reset state as launches per step (`observe` + policy_mlp), the rest by
    episode_mlp_wave_trace_pw (dw_episode_mlp_wave_trace_pw.hpp:124) - against the oracle loop with the same parameter
    vectors (agent: agents 0, 1; adversary: agents 2, 3)."""
    ref = M.reference_7()
    agent, adversary = amd.MLP(), amd.MLP()
    agent.set_parameters(ref["params"][0])
    adversary.set_parameters(ref["params"][1])
    np.random.seed(M.SEED_7)
    env = amd.RLDaisyWorld(grid_dimension=8, n_agents=4, neighborhood_mode="moore")
    env.batch_size = M.B_7
    obs = env.reset()
    np.testing.assert_allclose(obs, ref["obs0"], rtol=1e-12, atol=0)
    assert (obs[:, :, :, 0, 0] != 0).any()
    out = amd.simulate_grazing_mlp(env, agent, M.STEPS_7, adversary=adversary, chunk=16, obs=obs)
    assert "mlp episode: " + M.WAVE in env._engine.kernel_info() and env._engine.params.obs_mask == M.MOORE
    assert np.array_equal(out["reward"], ref["reward"]), "reward"
    assert np.array_equal(out["agent_ok"], ref["ok"]), "agent_ok"
    for f in FIELDS:
        assert np.array_equal(out["stats"][f], ref[f]), f
    assert np.array_equal(out["L"], ref["L"])
    assert np.array_equal(env.grid, ref["grid"]) and env.L == ref["L_end"] and env.step_count == M.STEPS_7
    env.close()
