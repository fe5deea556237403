"""GPU tests (``-m gpu``): every kernel family with the physics constants at the EDGES of what check_params admits -
dt < 0, dt = 0, a p that is no float32 value, p != 1, inadmissible tie chains (every cell redone in float64), a run that
crosses the admissibility boundary inside a step pair, gamma <= 0, q and q2 at and past each other, asymmetric and neutral
albedos, g = 0 and tiny g, luminosities far outside the ramp - from a quantised state that reaches covers of 1000, cells
with light + dark = 1000 and saturated / empty 3 x 3 patches.  The cases, states, shapes and families are the table
tools/constant_edge_cases.py; tests/test_constant_edges_cpu.py keeps that table honest without a GPU (the oracle is
finite and lively on every run used here, every case reaches its branch of csrc/dw_plan.hpp).

Every comparison of planes, reductions and flags in the exact mode is exact integer equality against the float64 oracle:
c_oracle for agent-free runs, oracle.daisy_oracle.OracleDaisyWorldC with the case's constants on its `P` (it hands all
twelve to the C oracle, OracleParams.from_obj) for runs with agents.  Every case asserts from ``kernel_info()`` which
family the handle's plan takes; the pair families also from ``last_step_n_timing()`` how many pairs were launched.

  A  exact mode: every case x every steady-state family (generic, tiled 16 / 32 / 64, the four wave-strip single-step
     forms, the four step-pair forms); the shrunk-queue cases again with the overflow fallbacks as the whole computation
  B  the first step from an un-quantised float64 / float32 state (step_generic<In, 3>, step_first_stream, packed)
  C  the per-world tables, one row per case, against the ORACLE per world (not against one-world handles: that link is
     tests/test_gpu_ensemble_params.py's): traced steps on a generic and a wave-strip shape, episodes with agents on the
     one-wave-per-world kernel and as launches per step; the full table (worlds_symmetric false) and its symmetric rows
  D  dw_run_episode with a shared set in its three forms
  E  the tie bound itself: error / bound < 1 on the admissible steps, every cell flagged on the inadmissible ones
  F  the float32-only mode: bit-identical planes across families, and one family per case anchored to the oracle at
     twice what profiles/constant_edges.json recorded (the project's rule: README table)
  G  the temperature reductions with three of the sets

The per-world tables hold the cases of at least four steps (one (n, B) luminosity array): 20 rows, 19 symmetric.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import constant_edge_cases as E  # noqa: E402
from oracle import c_oracle, daisy_oracle as O  # noqa: E402

FIELDS = ("max_k", "sum_light_k", "sum_dark_k")
WAVE, WORKGROUP, STEPWISE = "one wave per world", "workgroup (LDS)", "launches per step"
THRESHOLD_K = 5
L_RANGE = (0.0, 10.0)                                          # dw_step_n's clamp: wider than every schedule of the table
PROFILE = os.path.join(ROOT, "profiles", "constant_edges.json")


@pytest.fixture(scope="module")
def amd():
    import therldaisyworld_amd as t
    return t


def _clear_switches(monkeypatch, switches=None):
    """Exactly `switches` of the library's switches are set for the handles created from now on (read at creation)."""
    for name in E.ALL_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in (switches or {}).items():
        monkeypatch.setenv(name, value)


def _engine(amd, monkeypatch, shape, name, precision="exact", N=0, switches=None):
    """A handle with the constants of case `name` (None: the defaults), created under exactly `switches`."""
    from therldaisyworld_amd import _ffi
    _clear_switches(monkeypatch, switches)
    p = amd.default_params(*shape, N)
    p.precision = _ffi.PRECISION[precision]
    for k, v in (E.BY_NAME[name]["over"] if name else {}).items():
        setattr(p, k, v)
    return amd.Engine(p)


def _assert_family(eng, patterns, precision):
    info = eng.kernel_info()
    for pat in patterns:
        want = pat.format(prec=precision, exact="_exact" if precision == "exact" else "")
        assert want in info, (want, info)
    return info


def _upload_quantised(eng, light, dark):
    eng.upload_state_f32(light.astype(np.float32), dark.astype(np.float32), quantised=True)


def _reductions(kl, kd):
    return {"sum_light_k": kl.sum(axis=(1, 2)).astype(np.uint64), "sum_dark_k": kd.sum(axis=(1, 2)).astype(np.uint64),
            "max_k": np.maximum(kl.max(axis=(1, 2)), kd.max(axis=(1, 2))).astype(np.uint32)}


def _assert_state(eng, kl, kd, what):
    gl, gd = eng.download_planes()
    bad_l, bad_d = np.argwhere(E.k_of(gl) != kl), np.argwhere(E.k_of(gd) != kd)
    assert not len(bad_l) and not len(bad_d), (what, "planes", len(bad_l), bad_l[:4].tolist(), len(bad_d), bad_d[:4].tolist())
    s, ref = eng.reduce(), _reductions(kl, kd)
    for f in FIELDS:
        assert np.array_equal(s[f], ref[f]), (what, "reduce()", f, s[f].tolist(), ref[f].tolist())


@functools.lru_cache(maxsize=None)
def _start(shape):
    light, dark = E.start_state(*shape, E.seed_of(*shape))
    light.flags.writeable = dark.flags.writeable = False
    return light, dark


@functools.lru_cache(maxsize=None)
def _reference(name, shape):
    """The oracle's per-mille planes after every step of the case's schedule from the table's state: computed once per
    (case, shape), shared by the families of that shape, read-only."""
    out = []
    for a, b in E.oracle_run(c_oracle, name, *_start(shape)):
        ka, kb = E.k_of(a), E.k_of(b)
        ka.flags.writeable = kb.flags.writeable = False
        out.append((ka, kb))
    return out


def _run_schedule(eng, family, case):
    """The case's schedule through the family's own call: dw_step per step, or ONE dw_step_n for the pair families (the
    same luminosities: the schedule is accumulated as dw_step_n accumulates it)."""
    n = len(case["L"])
    if family.startswith("pairs"):
        L_end = eng.step_n(n, case["L0"], case["dL"], *L_RANGE)
        assert L_end == min(max(case["L_end"], L_RANGE[0]), L_RANGE[1]), (L_end, case["L_end"])
        assert eng.last_step_n_timing()[1] == E.pairs_of(n) >= 1
    else:
        for L in case["L"]:
            eng.step(L)


# ---------------------------------------------------------------------------------------------------------------------
# A. exact mode: every case x every steady-state family
# ---------------------------------------------------------------------------------------------------------------------
def _takes(family, name):
    """The pair families take the cases with a run of at least three steps: dw_step_n fuses no pair in a shorter one, and
    the worlds of the shorter cases (the defaults far outside the ramp) are dead by then."""
    return not family.startswith("pairs") or len(E.BY_NAME[name]["L"]) >= E.PAIR_MIN_STEPS


CASES_A = [(f, n) for f in E.FAMILY_NAMES for n in E.NAMES if _takes(f, n)]


def _exact_family(amd, monkeypatch, family, name, extra=None):
    _, shape, switches, patterns = E.BY_FAMILY[family]
    eng = _engine(amd, monkeypatch, shape, name, "exact", switches=dict(switches, **(extra or {})))
    info = _assert_family(eng, patterns, "exact")
    for k, v in (extra or {}).items():
        assert f"{k}={v}" in info, info
    _upload_quantised(eng, *_start(shape))
    _run_schedule(eng, family, E.BY_NAME[name])
    _assert_state(eng, *_reference(name, shape)[-1], f"{family} {name}")
    eng.close()


@pytest.mark.parametrize("family,name", CASES_A)
def test_exact_mode_every_family(amd, monkeypatch, family, name):
    _exact_family(amd, monkeypatch, family, name)


@pytest.mark.parametrize("name", E.QUEUE_CASES)
@pytest.mark.parametrize("family", E.QUEUE_FAMILIES)
def test_exact_mode_with_shrunk_queues(amd, monkeypatch, family, name):
    """Near-tie queues of two entries and no mismatch list: with every cell flagged (the inadmissible case) the overflow
    fallbacks are the whole computation."""
    _exact_family(amd, monkeypatch, family, name, E.QUEUE_SWITCHES)


# ---------------------------------------------------------------------------------------------------------------------
# B. the first step from an un-quantised state
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f64", "f32"])
@pytest.mark.parametrize("name", E.NAMES)
@pytest.mark.parametrize("family", [f[0] for f in E.FIRST_FAMILIES])
def test_first_step_from_an_unquantised_state(amd, monkeypatch, family, name, fmt):
    """Covers up to 1.0 in both species and the saturated patches, uploaded as float64 and as float32: step 1 (the
    first-step kernel with its own bound, derive_first_bound) and step 3 against the oracle started from the state the
    library holds (the download)."""
    _, shape, switches, has, has_not = next(f for f in E.FIRST_FAMILIES if f[0] == family)
    eng = _engine(amd, monkeypatch, shape, name, "exact", switches=switches)
    info = eng.kernel_info()
    assert has in info and (has_not is None or has_not not in info), info
    light, dark = E.first_state(*shape, E.seed_of(*shape))
    if fmt == "f64":
        eng.upload_state(light, dark)
    else:
        eng.upload_state_f32(light.astype(np.float32), dark.astype(np.float32), quantised=False)
    held = eng.download_planes()
    Ls = E.first_schedule(name)
    ref = E.oracle_run(c_oracle, name, *held, Ls)
    for t, L in enumerate(Ls):
        eng.step(L)
        if t in (0, len(Ls) - 1):
            _assert_state(eng, E.k_of(ref[t][0]), E.k_of(ref[t][1]), f"{family} {name} {fmt} step {t + 1}")
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# C. the per-world tables against the oracle
# ---------------------------------------------------------------------------------------------------------------------
TABLES = {"full": E.TABLE_CASES, "symmetric": E.TABLE_CASES_SYMMETRIC}


def _table(eng, names):
    """One row per case (dtype _ffi.WORLD_PARAMS_DTYPE) and the (TABLE_STEPS, B) luminosities: column b is case b's."""
    tab = np.repeat(eng.world_params()[None], len(names))
    for b, name in enumerate(names):
        for k, v in E.constants(name).items():
            tab[k][b] = v
    L = np.ascontiguousarray(np.array([E.table_schedule(n) for n in names]).T)
    sym = [E.BY_NAME[n]["symmetric"] for n in names]
    return tab, L, all(sym)


@pytest.mark.parametrize("kind", list(TABLES))
@pytest.mark.parametrize("hw,form", [((9, 50), "generic"), ((12, 256), "wave strips")])
def test_traced_steps_with_one_row_per_case(amd, monkeypatch, hw, form, kind):
    names = TABLES[kind]
    shape = (len(names), *hw)
    eng = _engine(amd, monkeypatch, shape, None, "exact")
    assert f"; per-world constants: {form}" in eng.kernel_info(), eng.kernel_info()
    tab, L, symmetric = _table(eng, names)
    assert symmetric == (kind == "symmetric")
    light, dark = _start(shape)
    _upload_quantised(eng, light, dark)
    tr = eng.step_n_trace_ensemble(tab, L)
    gl, gd = eng.download_planes()
    red = eng.reduce()
    for b, name in enumerate(names):
        run = E.oracle_run(c_oracle, name, light[b:b + 1], dark[b:b + 1], L[:, b])
        for t, (a, d) in enumerate(run):
            ref = _reductions(E.k_of(a), E.k_of(d))
            for f in FIELDS:
                assert tr[f][t, b] == ref[f][0], (name, "trace row", t, f, int(tr[f][t, b]), int(ref[f][0]))
        kl, kd = E.k_of(run[-1][0]), E.k_of(run[-1][1])
        assert np.array_equal(E.k_of(gl[b:b + 1]), kl) and np.array_equal(E.k_of(gd[b:b + 1]), kd), (name, "planes")
        ref = _reductions(kl, kd)
        for f in FIELDS:
            assert red[f][b] == ref[f][0], (name, "reduce()", f)
    eng.close()


def _oracle_env(name, light, dark, idx, st, L):
    """OracleDaisyWorldC holding (light, dark) and the agents, with the constants of case `name` (None: the defaults)."""
    B, H, W = light.shape
    env = O.OracleDaisyWorldC(grid_dimension=max(H, W), n_agents=idx.shape[1], batch_size=B)
    _set_constants(env, name)
    env.L = L
    env.set_initial_cover(light.copy(), dark.copy())
    assert env.shape == (H, W)
    env.agent_indices = idx.astype(np.int64).copy()
    env.agent_states = st.reshape(B, -1, 1).astype(np.float64).copy()
    return env


def _set_constants(env, name):
    for k, v in (E.constants(name) if name else E.defaults()).items():
        setattr(env.P, k, v)


def _oracle_steps(env, Ls, codes):
    """K reference steps with the table's codes (0 .. 8: explicit moves).  Returns (alive (K, B), ok (K, B, N))."""
    K, B, N = codes.shape
    alive, ok = np.zeros((K, B), dtype=bool), np.zeros((K, B, N), dtype=bool)
    for t in range(K):
        env.L = float(Ls[t])
        _, _, done, _ = env.step(codes[t].astype(np.int64)[..., None])
        kl, kd = E.k_of(env.grid[:, 1]), E.k_of(env.grid[:, 2])
        alive[t] = np.maximum(kl.max(axis=(1, 2)), kd.max(axis=(1, 2))) > THRESHOLD_K
        ok[t] = ~done[..., 0]
    return alive, ok


def _agents(B, N, H, W, seed):
    rng = np.random.RandomState(seed)
    idx = np.stack([rng.randint(H, size=(B, N)), rng.randint(W, size=(B, N))], axis=-1).astype(np.int32)
    return idx, np.ones((B, N))


def _codes(K, B, N, seed):
    """A fixed table of explicit moves: 0 .. 4 move, 5 .. 7 move and graze, 8 stays and grazes."""
    return np.random.RandomState(seed).randint(0, 9, size=(K, B, N)).astype(np.int8)


@pytest.mark.parametrize("kind", list(TABLES))
@pytest.mark.parametrize("switch,form", [(None, WAVE), ("DW_NO_EPISODE_WAVE", STEPWISE)])
def test_episodes_with_one_row_per_case(amd, monkeypatch, switch, form, kind):
    """dw_run_episode_ensemble (episode_wave_pw, and launches per step under DW_NO_EPISODE_WAVE) with 2 agents and a
    fixed action table: world b against a one-world oracle environment with case b's constants.  Protocol of
    tests/test_gpu_episode_wave.py: the uploaded state is quantised by one zero-action step - at the handle's own
    constants, the defaults - mirrored on the oracle."""
    from therldaisyworld_amd import _ffi
    names = TABLES[kind]
    B, N, K = len(names), E.EPISODE_AGENTS, E.TABLE_STEPS
    H, W = E.TABLE_EPISODE_SHAPE
    eng = _engine(amd, monkeypatch, (B, H, W), None, "exact", N=N, switches={switch: "1"} if switch else None)
    assert f"; ensemble episode: {form}" in eng.kernel_info(), eng.kernel_info()
    tab, L, symmetric = _table(eng, names)
    assert symmetric == (kind == "symmetric")
    light, dark = _start((B, H, W))
    idx, st = _agents(B, N, H, W, 41)
    eng.upload_state(light, dark)
    eng.upload_agents(idx, st)
    zeros = np.zeros((B, N, 1), dtype=np.int64)
    eng.step(E.TABLE_QUANTISE_L, zeros)
    codes = _codes(K, B, N, 43)
    alive, ok = eng.run_episode_ensemble(tab, L, _ffi.POLICY_TABLE, None, codes, threshold_k=THRESHOLD_K)
    gl, gd = eng.download_planes()
    gidx, gst = eng.download_agents()
    red = eng.reduce()
    q_light, q_dark = E.table_episode_state(c_oracle, B)
    for b, name in enumerate(names):
        env = _oracle_env(None, light[b:b + 1], dark[b:b + 1], idx[b:b + 1], st[b:b + 1], E.TABLE_QUANTISE_L)
        env.step(zeros[b:b + 1])
        assert np.array_equal(E.k_of(env.grid[:, 1]), E.k_of(q_light[b:b + 1]))       # the state the CPU test judged
        assert np.array_equal(E.k_of(env.grid[:, 2]), E.k_of(q_dark[b:b + 1]))
        _set_constants(env, name)
        ref_alive, ref_ok = _oracle_steps(env, L[:, b], codes[:, b:b + 1])
        kl, kd = E.k_of(env.grid[:, 1]), E.k_of(env.grid[:, 2])
        assert np.array_equal(E.k_of(gl[b:b + 1]), kl) and np.array_equal(E.k_of(gd[b:b + 1]), kd), (name, "planes")
        assert np.array_equal(gidx[b:b + 1], env.agent_indices), (name, "agent positions")
        assert np.array_equal(gst[b:b + 1, :, None], env.agent_states), (name, "agent states")
        assert np.array_equal(alive[:, b:b + 1], ref_alive) and np.array_equal(ok[:, b:b + 1], ref_ok), (name, "flags")
        ref = _reductions(kl, kd)
        for f in FIELDS:
            assert red[f][b] == ref[f][0], (name, "reduce()", f)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# D. dw_run_episode with a shared set, in its three forms
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _episode_reference(name):
    """The oracle's run of case `name` on EPISODE_SHAPE: the zero-action quantising step and EPISODE_K table steps -
    computed once, shared by the three forms."""
    B, H, W = E.EPISODE_SHAPE
    N, K = E.EPISODE_AGENTS, E.EPISODE_K
    light, dark = _start(E.EPISODE_SHAPE)
    idx, st = _agents(B, N, H, W, 51)
    Ls = E.episode_schedule(name)
    codes = _codes(K, B, N, 53)
    env = _oracle_env(name, light, dark, idx, st, Ls[0])
    env.L = Ls[0]
    env.step(np.zeros((B, N, 1), dtype=np.int64))
    alive, ok = _oracle_steps(env, Ls[1:], codes)
    return {"idx0": idx, "st0": st, "Ls": Ls, "codes": codes, "alive": alive, "ok": ok,
            "light": E.k_of(env.grid[:, 1]), "dark": E.k_of(env.grid[:, 2]), "idx": env.agent_indices.copy(),
            "st": env.agent_states.copy()}


@pytest.mark.parametrize("switch,form", [(None, WAVE), ("DW_NO_EPISODE_WAVE", WORKGROUP), ("DW_NO_EPISODE_KERNEL", STEPWISE)])
@pytest.mark.parametrize("name", E.EPISODE_CASES)
def test_run_episode_with_a_shared_set(amd, monkeypatch, name, switch, form):
    from therldaisyworld_amd import _ffi
    B, H, W = E.EPISODE_SHAPE
    N = E.EPISODE_AGENTS
    ref = _episode_reference(name)
    eng = _engine(amd, monkeypatch, E.EPISODE_SHAPE, name, "exact", N=N, switches={switch: "1"} if switch else None)
    assert f"; episode: {form}" in eng.kernel_info(), eng.kernel_info()
    eng.upload_state(*_start(E.EPISODE_SHAPE))
    eng.upload_agents(ref["idx0"], ref["st0"])
    eng.step(ref["Ls"][0], np.zeros((B, N, 1), dtype=np.int64))
    alive, ok = eng.run_episode(ref["Ls"][1:], _ffi.POLICY_TABLE, None, ref["codes"], threshold_k=THRESHOLD_K)
    what = f"{name} {form}"
    assert np.array_equal(alive, ref["alive"]), (what, "world_alive")
    assert np.array_equal(ok, ref["ok"]), (what, "agent_ok")
    _assert_state(eng, ref["light"], ref["dark"], what)
    idx, st = eng.download_agents()
    assert np.array_equal(idx, ref["idx"]), (what, "agent positions")
    assert np.array_equal(st[..., None], ref["st"]), (what, "agent states")
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# E. the bound itself
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.NAMES)
def test_tie_bound_holds_or_every_cell_is_flagged(amd, monkeypatch, name):
    """dw_audit_tie_bound before each of 5 steps on 4 x 64 x 64, at the luminosity of that step.  Admissible steps: the
    float32 error stays below the bound the tie test uses (ratio < 1: the bound is a proof, this is its condition;
    measured ratios: profiles/constant_edges.json, the worst 0.382 for gamma = 0).  Inadmissible steps: tie_lo < 0 makes the audit's tie test
    (|g - rint g| > thr with thr < 0) flag every cell value it audits - out[2] == out[3], both species of every cell."""
    _clear_switches(monkeypatch)
    rows = E.audit(amd, name)
    B, H, W = E.AUDIT_SHAPE
    for r in rows:
        print(name, r)
        assert r["audited"] == 2 * B * H * W
        if r["admissible"]:
            assert r["ratio"] < 1.0, (name, r)
        else:
            assert r["flagged"] == r["audited"], (name, r)


# ---------------------------------------------------------------------------------------------------------------------
# F. the float32-only mode
# ---------------------------------------------------------------------------------------------------------------------
FAST_CASES = [c["name"] for c in E.CASES if all(c["admissible"])]
_NO_EP, _PACK, _TILED, _SINGLE = {"DW_NO_EPISODE_KERNEL": "1"}, {"DW_PACK_MIN_STRIPS": "1"}, {"DW_KERNEL": "tiled"}, {"DW_NO_FUSE": "1"}
# groups of families on ONE shape: (label, switches, what kernel_info() must contain, the call that takes the steps)
FAST_GROUPS = {
    "4x8x8": ((4, 8, 8), [("generic", {}, "step_generic<fast>", "step"),
                          ("episode wave", {}, f"; episode: {WAVE}", "episode"),
                          ("episode workgroup", {"DW_NO_EPISODE_WAVE": "1"}, f"; episode: {WORKGROUP}", "episode"),
                          ("episode stepwise", _NO_EP, f"; episode: {STEPWISE}", "episode")]),
    "5x16x32": ((5, 16, 32), [("generic", {}, "step_generic<fast>", "step"),
                              ("strip-packed", dict(_PACK, **_SINGLE), "step_stream_fast<halo=packed>", "step"),
                              ("pairs-packed", dict(_PACK, **_NO_EP), "step_stream_fused2", "step_n")]),
    "2x20x64": ((2, 20, 64), [("tiled-16", {}, "step_tiled<TCQ=16", "step"),
                              ("strip-packed", dict(_PACK, **_SINGLE), "step_stream_fast<halo=packed>", "step")]),
    "2x20x128": ((2, 20, 128), [("tiled-32", {}, "step_tiled<TCQ=32", "step"),
                                ("strip-packed", dict(_PACK, **_SINGLE), "step_stream_fast<halo=packed>", "step")]),
    "2x12x256": ((2, 12, 256), [("tiled-64", _TILED, "step_tiled<TCQ=64", "step"),
                                ("strip-rotate", _SINGLE, "step_stream_fast<halo=rotate>", "step"),
                                ("pairs-rotating", _NO_EP, "step_stream_fused2", "step_n")]),
    "1x12x264": ((1, 12, 264), [("tiled-64", _TILED, "step_tiled<TCQ=64", "step"),
                                ("strip-general", _SINGLE, "step_stream_fast<halo=general>", "step"),
                                ("pairs-overlapped", _NO_EP, "step_stream_fused2", "step_n")]),
    "1x12x1024": ((1, 12, 1024), [("tiled-64", _TILED, "step_tiled<TCQ=64", "step"),
                                  ("strip-dpp-old", _SINGLE, "step_stream_fast<halo=dpp-old>", "step"),
                                  ("pairs-ring", _NO_EP, "step_stream_fused2", "step_n")]),
}


def _fast_planes(amd, monkeypatch, shape, name, member):
    """The planes after the case's schedule in the float32-only mode, the steps taken by `member`'s call; None where the
    call does not apply to a run this short."""
    from therldaisyworld_amd import _ffi
    label, switches, pattern, how = member
    case = E.BY_NAME[name]
    n = len(case["L"])
    if (how == "step_n" and n < E.PAIR_MIN_STEPS) or (how == "episode" and n < 2):
        return None
    B, H, W = shape
    N = E.EPISODE_AGENTS if how == "episode" else 0
    eng = _engine(amd, monkeypatch, shape, name, "fast", N=N, switches=switches)
    assert pattern in eng.kernel_info(), (label, eng.kernel_info())
    _upload_quantised(eng, *_start(shape))
    if how == "step_n":
        assert eng.step_n(n, case["L0"], case["dL"], *L_RANGE) == min(max(case["L_end"], L_RANGE[0]), L_RANGE[1])
        assert eng.last_step_n_timing()[1] == E.pairs_of(n)
    elif how == "episode":                                      # zero actions: the agents move and graze nothing
        eng.upload_agents(*_agents(B, N, H, W, 61))
        eng.step(case["L"][0], np.zeros((B, N, 1), dtype=np.int64))
        eng.run_episode(np.array(case["L"][1:]), _ffi.POLICY_TABLE, None, np.zeros((n - 1, B, N), dtype=np.int8),
                        threshold_k=THRESHOLD_K)
    else:
        for L in case["L"]:
            eng.step(L)
    planes = eng.download_planes()
    eng.close()
    return planes


@pytest.mark.parametrize("name", FAST_CASES)
@pytest.mark.parametrize("group", list(FAST_GROUPS))
def test_fast_mode_is_identical_across_families(amd, monkeypatch, group, name):
    """dw_physics.hpp: "all kernels produce bit-identical values whichever form they use" - held here as a condition, for
    every family of A and the three episode forms (zero actions), on the families that share a shape: the same state,
    case and schedule give the same planes, bit for bit."""
    shape, members = FAST_GROUPS[group]
    got = [(m[0], _fast_planes(amd, monkeypatch, shape, name, m)) for m in members]
    got = [(label, planes) for label, planes in got if planes is not None]
    first, base = got[0]
    for label, planes in got[1:]:
        for a, b, species in zip(planes, base, ("light", "dark")):
            diff = np.argwhere(a != b)
            assert not len(diff), (name, group, f"{label} against {first}", species, len(diff), diff[:4].tolist())


@functools.lru_cache(maxsize=None)
def _profile():
    with open(PROFILE) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("name", FAST_CASES)
def test_fast_mode_is_anchored_to_the_oracle(amd, monkeypatch, name):
    """Identical families can all share a wrong coefficient: one step of the single-step wave-strip kernel on 2 x 12 x 256
    from the table's state against the oracle - the largest deviation in quanta and the share of differing cell values,
    each asserted at twice what ONE GPU run recorded per case in profiles/constant_edges.json
    (tools/constant_edge_cases.py prints that file).  Measured there, of 12 288 cell values: none differs for 18 of the 20
    cases (dt < 0 and p != 1 among them: no magnification beyond a quantum), one value by one quantum - 0.0081 % - for
    the asymmetric albedos and for the defaults at L = 1.7."""
    _clear_switches(monkeypatch, {"DW_NO_FUSE": "1"})
    worst, share = E.anchor(amd, c_oracle, name)
    rec = _profile()[name]
    print(name, "max quanta", worst, "share", share, "recorded", rec["fast_max_quanta"], rec["fast_share"])
    assert worst <= 2 * rec["fast_max_quanta"], (name, worst, rec["fast_max_quanta"])
    assert share <= 2.0 * rec["fast_share"], (name, share, rec["fast_share"])


# ---------------------------------------------------------------------------------------------------------------------
# G. temperature reductions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", E.TEMPERATURE_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", E.TEMPERATURE_CASES)
def test_temperature_reductions(amd, monkeypatch, name, shape):
    """dw_reduce_temperature after a step against mean / std / min / max of the oracle's `temp` cache of that step, at
    the tolerances of tests/test_gpu_temperature.py (1e-12 relative per cell, the factor 2 for the summation; the std
    absolute against the world's maximum)."""
    L = E.BY_NAME[name]["L"][0]
    light, dark = _start(shape)
    out, caches = c_oracle.forward(light, dark, L, E.oracle_params(c_oracle, name), want_caches=True)
    temp = caches[:, 0]
    eng = _engine(amd, monkeypatch, shape, name, "exact")
    _upload_quantised(eng, light, dark)
    eng.step(L)
    rec = eng.reduce_temperature(L)
    _assert_state(eng, E.k_of(out[:, 1]), E.k_of(out[:, 2]), f"{name} {shape}")
    eng.close()
    mean, std = temp.mean(axis=(1, 2)), temp.std(axis=(1, 2))
    mn, mx = temp.min(axis=(1, 2)), temp.max(axis=(1, 2))
    np.testing.assert_allclose(rec["mean"], mean, rtol=2e-12, atol=0)
    np.testing.assert_allclose(rec["min"], mn, rtol=1e-12, atol=0)
    np.testing.assert_allclose(rec["max"], mx, rtol=1e-12, atol=0)
    assert (np.abs(rec["std"] - std) <= 2e-12 * mx).all(), (rec["std"], std)
