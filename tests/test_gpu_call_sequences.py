"""GPU tests (``-m gpu``): slices of tools/fuzz_calls.py - random interleavings of every state-changing C ABI call on ONE
handle, everything compared after every operation.

  * exact and float64 precision against the float64 oracle model (planes, agents, reductions, flags, rewards, records and
    cover tiles exactly; temperature rows, tile means and caches to the bounds of tests/test_gpu_temperature.py,
    tests/test_gpu_frames.py and tests/test_gpu_parity.py), a third of the exact cases also against the twin;
  * the float32-only precision against the twin - B one-world engines without fused pairs, packing and episode kernels,
    driven by single steps - bit for bit, temperature rows included.

The seeds are chosen so that the coverage conditions of tests/test_call_sequences_cpu.py hold over their union: every
operation kind from every class of the handle's state it is admissible in.  A case plans 26 to 60 state-changing calls on
shapes of at most 22 400 cells and takes a few seconds, most of it the NumPy oracle.

Reduced sequences of the disagreements the seeds found are pinned by name at the end.
"""
import importlib.util
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEEDS_EXACT = [21, 155, 203, 225, 234, 321, 334, 383, 495, 646, 1098, 1427, 1536, 1657, 1771, 1856, 2055, 2316, 2517, 2565,
               2967, 2970]
SEEDS_F64 = [392, 1006, 1243, 1527, 2225, 2275]
SEEDS_FAST = [170, 204, 385, 418, 752, 797, 1177, 1435, 1553, 1626, 1922, 2120, 2575, 2654]
ALL_SEEDS = SEEDS_EXACT + SEEDS_F64 + SEEDS_FAST
assert len(ALL_SEEDS) <= 48


def load_tool():
    spec = importlib.util.spec_from_file_location("fuzz_calls", os.path.join(ROOT, "tools", "fuzz_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tool():
    return load_tool()


@pytest.fixture(autouse=True)
def _environment(monkeypatch, tool):
    """The DW_TEST_* caps of a plan are honoured only under DW_TEST_HOOKS; no switch of the caller's leaks into a case."""
    monkeypatch.setenv("DW_TEST_HOOKS", "1")
    for name in tool.SWITCHES + ("DW_KERNEL", "DW_STRIP_ROWS", "DW_TEST_FAIL_GROUP_ALLOC"):
        monkeypatch.delenv(name, raising=False)


def _case(tool, plan):
    log, t0 = [], time.perf_counter()
    ok, info = tool.run_case(plan["seed"], log, plan)
    print(f"seed {plan['seed']}: {time.perf_counter() - t0:.2f} s  {info}")
    assert ok, "\n".join(log)


@pytest.mark.parametrize("seed", SEEDS_EXACT)
def test_call_sequences_exact_vs_oracle_model(tool, seed):
    plan = tool.plan_case(seed)
    assert plan["precision"] == "exact"
    _case(tool, plan)


@pytest.mark.parametrize("seed", SEEDS_F64)
def test_call_sequences_f64_vs_oracle_model(tool, seed):
    plan = tool.plan_case(seed)
    assert plan["precision"] == "f64" and not plan["twin"]
    _case(tool, plan)


@pytest.mark.parametrize("seed", SEEDS_FAST)
def test_call_sequences_fast_vs_twin(tool, seed):
    plan = tool.plan_case(seed)
    assert plan["precision"] == "fast" and plan["twin"] and plan["B"] <= tool.TWIN_MAX_B
    _case(tool, plan)


# ---- pinned sequences ------------------------------------------------------------------------------------------------
def _covers(rng, B, H, W):
    return rng.rand(B, H, W) * 0.4 * (rng.rand(B, H, W) < 0.5), rng.rand(B, H, W) * 0.4 * (rng.rand(B, H, W) < 0.5)


@pytest.mark.parametrize("H,W", [(8, 8), (12, 12)])
def test_step_n_without_uploaded_agents_takes_the_step_kernels(tool, H, W):
    """dw_step_n(use_device_actions=0) makes no agent update at all, so - like dw_step without actions - it needs no agents on
    the handle.  (From a quantised state, worlds of up to 4096 cells went to the LDS episode kernels, whose precondition
    refused the run with DW_ESTATE "no agents uploaded": seed 15 of the first run, 8x8 B=33 N=4.)  One-wave and workgroup
    shapes; the same run from the un-quantised upload, whose first step was always a step kernel."""
    B, N, rng = 3, 2, np.random.RandomState(12)
    light, dark = _covers(rng, B, H, W)
    q = dict(light=np.round(light, 3).astype(np.float32), dark=np.round(dark, 3).astype(np.float32))
    ops = [dict(kind="upload_f32q", **q), dict(kind="step_n", n=4, L=0.9, dL=0.01, lo=0.72, hi=1.28),
           dict(kind="r_planes"), dict(kind="r_prev"), dict(kind="r_reduce"), dict(kind="r_grid", L=0.9),
           dict(kind="upload_f64", light=light, dark=dark), dict(kind="step_n", n=5, L=0.9, dL=0.01, lo=0.72, hi=1.28),
           dict(kind="r_planes"), dict(kind="r_prev"), dict(kind="r_reduce"), dict(kind="r_grid", L=0.9)]
    _case(tool, tool.explicit_plan(H, W, B, N, "exact", ops))


@pytest.mark.parametrize("H,W,switch", [(8, 8, None), (8, 8, "DW_NO_EPISODE_KERNEL")])
def test_refused_mlp_episode_keeps_the_resident_parameter_sets(tool, H, W, switch):
    """dw_run_episode_mlp on a handle whose last step took per-world luminosities is refused with DW_ESTATE - and must
    leave the parameter sets of the earlier call on the device: the later `params=None` episode acts with THEM.  (The
    refusal came after the new sets had been copied over the resident ones, and after `n_members` had been replaced.)
    In the one-wave and the launches-per-step form."""
    B, N, rng = 3, 2, np.random.RandomState(11)
    light, dark = _covers(rng, B, H, W)
    idx = np.stack([rng.randint(H, size=(B, N)), rng.randint(W, size=(B, N))], axis=-1).astype(np.int32)
    resident, other = rng.randn(1, 1808) * 0.5, rng.randn(2, 1808) * 0.5
    members = np.zeros(B, np.int32)
    ops = [dict(kind="upload_f64", light=light, dark=dark),
           dict(kind="upload_agents", idx=idx, st=np.ones((B, N))),
           dict(kind="step", L=0.95),
           dict(kind="step", L=0.96),
           dict(kind="ep_mlp", Ls=np.array([0.97, 0.98, 0.99]), split=1, n_members=1, params=resident),
           dict(kind="trace_pw", Ls=np.array([[1.0, 0.9, 1.1]])),
           dict(kind="x_ep_mlp", Ls=np.array([1.0, 1.0, 1.0]), params=other, n_members=2, split=1, member_a=members,
                member_b=members),
           dict(kind="r_planes"), dict(kind="r_agents"), dict(kind="r_reduce"),
           dict(kind="step", L=1.0),
           dict(kind="ep_mlp_resident", Ls=np.array([1.01, 1.02, 1.03, 1.04]), split=1, n_members=1, params=None),
           dict(kind="r_planes"), dict(kind="r_agents"), dict(kind="r_actions")]
    _case(tool, tool.explicit_plan(H, W, B, N, "exact", ops, env={switch: "1"} if switch else None))
