"""CPU tests of tools/fuzz_calls.py (no GPU, no library): the planner is deterministic, the seeds of
tests/test_gpu_call_sequences.py cover what they are chosen to cover, and the float64 model's bookkeeping is self-consistent.

The coverage conditions are conditions on the CHOSEN SEEDS, not measurements: a seed list that lets one of them fail is to be
replaced, never the condition.  A state class is the tuple the planner predicts for struct dw_handle: (current state
quantised?, stepped?, owner and format of the un-quantised upload, per-world L?, per-world constants?, agents present?,
slot 0 valid?, slot 1 valid?, MLP sets resident?).  Its first five members are what the library's preconditions and its
dispatch read together, and every operation kind is required from every one of their twelve combinations in which it is
admissible (574 pairs); the last four multiply that to more classes than 48 cases of a few seconds have operations, so
each of them is required in both of its values (and the restores across a change of the per-world marks, in both
directions).
"""
import collections
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tool():
    return _load("fuzz_calls", "tools", "fuzz_calls.py")


@pytest.fixture(scope="module")
def seeds():
    return _load("gpu_call_sequences", "tests", "test_gpu_call_sequences.py")


@pytest.fixture(scope="module")
def plans(tool, seeds):
    return [tool.plan_case(s) for s in seeds.ALL_SEEDS]


def test_plan_is_deterministic_per_seed(tool, seeds):
    for s in seeds.ALL_SEEDS[:6]:
        assert tool.digest(tool.plan_case(s)) == tool.digest(tool.plan_case(s))
    assert len({tool.digest(tool.plan_case(s)) for s in seeds.ALL_SEEDS[:6]}) == 6


def test_seed_lists_are_filed_by_precision(tool, seeds, plans):
    assert 0 < len(seeds.ALL_SEEDS) <= 48 and len(set(seeds.ALL_SEEDS)) == len(seeds.ALL_SEEDS)
    by = {p["seed"]: p for p in plans}
    assert all(by[s]["precision"] == "exact" for s in seeds.SEEDS_EXACT)
    assert all(by[s]["precision"] == "f64" for s in seeds.SEEDS_F64)
    assert all(by[s]["precision"] == "fast" and by[s]["twin"] and by[s]["B"] <= tool.TWIN_MAX_B for s in seeds.SEEDS_FAST)
    assert min(len(seeds.SEEDS_EXACT), len(seeds.SEEDS_F64), len(seeds.SEEDS_FAST)) >= 4
    assert sum(by[s]["twin"] for s in seeds.SEEDS_EXACT) >= 4           # the twin runs beside the oracle as well


def test_every_kind_is_planned_at_least_three_times(tool, plans):
    count = collections.Counter(op["kind"] for p in plans for op in p["ops"])
    assert not [(kd, count[kd]) for kd in tool.KINDS if count[kd] < 3]
    assert not [(kd, count[kd]) for kd in tool.REFUSALS if count[kd] < 2]
    assert not set(count) - set(tool.KINDS) - set(tool.REFUSALS)


def test_every_kind_is_planned_from_every_class_that_admits_it(tool, plans):
    need = {(kd, c) for kd in tool.KINDS for c in tool.CORE_CLASSES
            if any(tool.feasible(kd, c, n, pr) for n in (0, 2) for pr in ("exact", "f64", "fast"))}
    seen = {(op["kind"], op["cls"][:5]) for p in plans for op in p["ops"]}
    assert len(need) > 500
    assert not sorted(need - seen)
    assert not sorted((kd, c) for kd, c in seen - need if kd in tool.KINDS)     # nothing is planned where it is not admissible
    # the caller's L after a per-world-L run (lacks_shared_constants does not cover it): the caches succeed
    assert ("r_caches", (True, True, "none", True, False)) in seen
    # the other four members of the class, each in both values
    for member in (5, 6, 7, 8):
        assert {op["cls"][member] for p in plans for op in p["ops"] if op["kind"] in tool.CHANGING} == {False, True}
    # a slot saved in a per-world state restored into a shared-L state, and the reverse; with per-world constants too
    moves = {(op["slot_mode"], op["cls"][3:5]) for p in plans for op in p["ops"] if op["kind"].startswith("restore")}
    for saved, now in (((True, False), (False, False)), ((False, False), (True, False)), ((True, True), (False, False)),
                       ((False, False), (True, True))):
        assert (saved, now) in moves, (saved, now)


def test_shapes_switches_and_lengths(tool, plans):
    assert {(p["H"], p["W"]) for p in plans} == {s[0] for s in tool.SHAPES}
    assert {p["B"] for p in plans if (p["H"], p["W"]) == (8, 8)} == {5, 33}
    assert {p["N"] for p in plans if (p["H"], p["W"]) == (16, 16)} == {4, 6}
    for p in plans:
        assert sum(op["kind"] in tool.CHANGING for op in p["ops"]) >= 8, p["seed"]
    used = {name for p in plans for name in p["env"]}
    assert used >= {"DW_PACK_MIN_STRIPS", "DW_TEST_QUEUE_CAP", "DW_TEST_MISMATCH_CAP", "DW_TEST_TRACE_ROWS", "DW_TEST_FRAME_RING",
                    "DW_NO_EPISODE_WAVE", "DW_NO_EPISODE_KERNEL", "DW_NO_AGENT_FUSE", "DW_NO_SEAM_STRIPS"}
    assert any(not p["env"].get("DW_PACK_MIN_STRIPS") for p in plans)
    # the wave kernels' 64-step segment boundary inside a call; odd and even run lengths
    assert sum(len(op["Ls"]) >= 65 for p in plans for op in p["ops"] if op["kind"] in tool.EPISODES) >= 3
    assert {op["n"] for p in plans for op in p["ops"] if op["kind"] == "step_n"} >= set(range(1, 10))
    flags = {op["world_flags"] for p in plans for op in p["ops"] if op["kind"] in ("ep_greedy", "ep_anti", "ep_table")}
    assert flags == {False, True}
    assert any(op["kind"] == "ep_mlp_trace" and op["params"] is None for p in plans for op in p["ops"])


# ---- the model's bookkeeping ---------------------------------------------------------------------------------------------
SHARED_RUNS = ("step_n", "step_n_dev", "trace", "trace_temp", "frames", "ep_greedy", "ep_anti", "ep_table", "ep_trace",
               "ep_trace_temp", "ep_mlp", "ep_mlp_resident", "ep_mlp_trace")


def _bits(model, agents=True):
    parts = list(model.planes(False)) + (list(model.agents_now()) if agents else [])
    if model.S.stepped:
        parts += list(model.planes(True))
    return b"".join(np.ascontiguousarray(x).tobytes() for x in parts)


def _single_steps(tool, loop, op, exp):
    """The operation as single steps on the model `loop`: the records those steps leave, as the operation returns them."""
    kind, B = op["kind"], loop.B
    rows = collections.defaultdict(list)
    if kind in ("step_n", "step_n_dev"):
        Ls, L = [], op["L"]
        for _ in range(op["n"]):
            Ls.append(L)
            L = min(max(L + op["dL"], op["lo"]), op["hi"])
        L_end = L
    else:
        Ls = list(op["Ls"])
    if op.get("params") is not None:
        loop.mlp_sets = op["params"].copy()
    for t, L in enumerate(Ls):
        a = None
        if kind == "step_n_dev":
            a = op["a"]
        elif kind in tool.PLAIN_EPISODES and loop.N:
            if op["mode"] == "table" or (op["use_table"] is not None and op["use_table"][t]):
                a = loop._resolve(op["table"][t])
            else:
                a = loop._greedy(op["mode"] == "anti")
        elif kind.startswith("ep_mlp"):
            a = loop._mlp_actions(loop.mlp_sets, op.get("member_a"), op.get("member_b"), op["split"])
        loop.apply(dict(kind="step", L=float(L)) if a is None else dict(kind="step_act", L=float(L), a=a))
        rows["stats"].append(loop.stats())
        rows["temps"].append(loop.temp_on_demand(float(L)))
        if loop.N:
            reward, done = loop._rewards()
            rows["reward"].append(reward)
            rows["done"].append(done)
    for key in ("stats", "stats0", "temps", "reward", "done"):
        if exp.get(key) is not None:
            assert np.array_equal(exp[key], np.stack(rows["stats" if key == "stats0" else key])), (tool.describe(op), key)
    if exp.get("ok") is not None:
        assert np.array_equal(exp["ok"], ~np.stack(rows["done"])[..., 0])
    if exp.get("alive") is not None:
        assert np.array_equal(exp["alive"], np.stack(rows["stats"])["max_k"] > tool.THRESHOLD_K)
    if "L" in exp:
        assert exp["L"] == L_end


@pytest.mark.parametrize("which", [0, 1, 2])
def test_model_runs_equal_its_single_steps_and_restore_returns_the_saved_bytes(tool, seeds, which):
    """On three plans: every shared-L run and episode of the Model leaves the grids, agents and records that its single-step
    method leaves when driven in a loop; a restore returns the model to the bytes of the save; and after every operation the
    model is in the class the planner predicted."""
    by_size = sorted((tool.plan_case(s) for s in seeds.SEEDS_EXACT), key=lambda p: p["B"] * p["H"] * p["W"])
    plan = [p for p in by_size if p["N"]][which]
    loop = tool.Model(plan["H"], plan["W"], plan["B"], plan["N"], plan["precision"])
    saved = {}
    compared = collections.Counter()

    def on_op(m, op, exp):
        kind = op["kind"]
        if kind in SHARED_RUNS:
            _single_steps(tool, loop, op, exp)
            compared[kind] += 1
        else:
            loop.apply(op, tool.synthetic_state(plan, op))
        if kind in tool.CHANGING:
            assert _bits(m) == _bits(loop), tool.describe(op)
        if kind in ("save0", "save1"):
            saved[kind[-1]] = (_bits(m, m.S.agents), m.S.core(), m.S.agents)
        if kind in ("restore0", "restore1"):                   # (a slot saved before the agents came leaves them alone)
            assert (_bits(m, saved[kind[-1]][2]), m.S.core()) == saved[kind[-1]][:2]
            compared["restore"] += 1

    tool.dry_run(plan, on_op)
    assert sum(compared.values()) >= 3, compared
