"""Keeps tools/episode_workgroup_cases.py honest, without a GPU: the references tests/test_gpu_episode_workgroup.py holds
the workgroup episode kernels to are only worth something if the oracle runs they come from are lively - worlds alive to
the end, agents that graze, agents that die and agents that do not, agents that meet on a cell where the case is there for
that, MLP decisions that no rounding order can turn - and cheap enough to be computed in a test.  The seeds of the table
were chosen here until every condition held, and are frozen.

Every condition is judged on the oracle's series alone.  The limit on a reference's time is a condition on the table too
(the GPU suite computes each of them once): the largest, 3 x 64 x 64 with 6 agents over 41 steps, takes about a second.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import episode_workgroup_cases as W  # noqa: E402

SECONDS = 10.0                                                   # "a few seconds", with room for a loaded machine
_ids = lambda v: str(v).replace(" ", "")  # noqa: E731


def test_the_table_is_what_the_kernels_dispatch_on():
    """The shapes sit where the table says: each side of the wpb thresholds, at the cell limit, one past it; the MLP edge
    cases at the largest N the LDS formula admits, the dispatch-only ones one agent beyond."""
    cells = sorted({s[1] * s[2] for s in W.SHAPES_A})
    assert cells == [289, 400, 1024, 1025, 4095, 4096]
    assert [W.worlds_per_block(c) for c in (256, 257, 1024, 1025, 4096)] == [4, 2, 2, 1, 1]
    assert sum(s[0] % W.worlds_per_block(s[1] * s[2]) != 0 for s in W.SHAPES_A) >= 2       # a workgroup with an invalid half
    assert W.episode_world_bytes(4096, 6) > 64 * 1024           # 64 x 64: the launch needs the raised dynamic-LDS limit
    for shape, beyond in zip(W.LDS_EDGE_B, W.DISPATCH_B):
        C = shape[1] * shape[2]
        wpb = W.worlds_per_block(C)
        assert W.episode_mlp_world_bytes(C, shape[3]) * wpb <= W.LDS_LIMIT < W.episode_mlp_world_bytes(C, beyond[3]) * wpb
    for shape in W.SHAPES_B + W.LDS_EDGE_B:
        assert 256 < shape[1] * shape[2] <= W.MAX_CELLS and 0 < shape[4] < shape[3]


def test_inputs_are_quantised_and_within_the_grid():
    for shape in W.SHAPES_A:
        inp = W.inputs_a(shape)
        B, H, Wd, N = shape
        for plane in (inp["light"], inp["dark"]):
            assert plane.shape == (B, H, Wd) and np.array_equal(plane, W.k_of(plane) / 1000.0) and plane.max() <= 0.4
        assert (inp["idx"] >= 0).all() and (inp["idx"][..., 0] < H).all() and (inp["idx"][..., 1] < Wd).all()
        assert (inp["st"] == 0.5).all()
        assert set(np.unique(inp["codes"])) == set(range(-2, 9)) and set(np.unique(inp["moves"])) == set(range(9))
        assert inp["use_table"][0] == 0 and inp["use_table"][1] == 1 and 0 < inp["use_table"].sum() < W.K_A


@pytest.mark.parametrize("policy", W.POLICIES)
@pytest.mark.parametrize("shape", W.SHAPES_A, ids=_ids)
def test_episode_references_are_lively(shape, policy):
    ref = W.reference_a(shape, policy)
    print(shape, policy, "reference seconds", round(ref["seconds"], 2))
    assert ref["seconds"] < SECONDS
    assert (ref["max_k"] > W.THRESHOLD_K).all() and ref["alive"].all(), "a world is dead at the last step"
    assert (np.diff(ref["reward"], axis=0) > 0).any(), "no agent's reward ever rises: nobody grazed"
    assert not ref["ok"][-1].all(), "no agent has died"
    assert ref["ok"][-1].any(), "no agent is ok at the end"
    assert sorted(ref["final"]) == list(W.KS_A)
    if shape == W.CROWDED:
        assert ref["crowded"].any(), "no step leaves two agents that moved on one cell"
        beyond = W.threads_per_world(shape[1] * shape[2])       # the agents of the loops' second trip: they graze too
        assert (np.diff(ref["reward"][:, :, beyond:], axis=0) > 0).any() and ref["ok"][-1][:, beyond:].any()
    # the shorter runs are not trivially equal to the long one
    assert not np.array_equal(ref["final"][1]["light"], ref["final"][2]["light"])
    assert not np.array_equal(ref["final"][2]["light"], ref["final"][W.K_A]["light"])


@pytest.mark.parametrize("shape", W.SHAPES_B + W.LDS_EDGE_B, ids=_ids)
def test_mlp_references_are_decided_and_lively(shape):
    ref = W.reference_b(shape)
    print(shape, "reference seconds", round(ref["seconds"], 2), "least margin", ref["margin"].min())
    assert ref["seconds"] < SECONDS
    assert (ref["margin"] > W.MARGIN).all(), ref["margin"].min()
    for K in W.ks_b(shape):                                      # every run: a first chunk and its second
        assert K in ref["final"] and K + W.K2_B in ref["final"]
        for lo, hi in ((0, K), (K, K + W.K2_B)):
            codes = set(np.unique(ref["action"][lo:hi]).tolist())
            assert len(codes) >= 3 and max(codes) > 4, (shape, lo, hi, codes)
        assert (ref["reward"][K + W.K2_B - 1] > 0).any() and (ref["reward"][K - 1] > 0).any()
    assert (np.diff(ref["reward"][..., 0], axis=0) > 0).any(), "no agent ever grazed"
    # the last agent - the lone live group of the last pass where N = agents per pass + 1 - decides differently with the
    # other half's parameter set, within the shortest run: handed the wrong set, or left out, it shows
    N, K = shape[3], min(W.ks_b(shape))
    assert (ref["action"][:K, :, N - 1] != ref["swapped"][:K, :, N - 1]).any(), "the last agent's set does not matter"
    assert (ref["action"][:K, :, 0] != ref["swapped"][:K, :, 0]).any(), "the first agent's set does not matter"


@pytest.mark.parametrize("name,shape", W.OVERFLOW_CASES, ids=_ids)
def test_overflow_references_are_alive_and_moving(name, shape):
    ref = W.reference_overflow(name, shape)
    print(name, shape, "reference seconds", round(ref["seconds"], 2), "max_k", ref["max_k"].tolist())
    assert ref["seconds"] < SECONDS
    assert (ref["max_k"] > W.THRESHOLD_K).all() and ref["alive"][-1].all()
    fin, start = ref["final"], ref["start"]
    assert not np.array_equal(fin["light"], start["light"]) and not np.array_equal(fin["dark"], start["dark"])
    if name:                                                     # the constants matter: the defaults end elsewhere
        other = W.reference_overflow(None, shape) if (None, shape) in W.OVERFLOW_CASES else None
        if other is not None:
            assert not np.array_equal(fin["light"], other["final"]["light"])


@pytest.mark.parametrize("shape", W.STEP_N_SHAPES, ids=_ids)
def test_step_n_references_are_alive(shape):
    light, dark, L = W.reference_step_n(shape)
    start = W.inputs_step_n(shape)
    assert not np.array_equal(start[0], W.k_of(start[0]) / 1000.0), "the upload is meant to be un-quantised"
    assert max(light.max(), dark.max()) > W.THRESHOLD_K
    assert L == pytest.approx(W.STEP_N_L + W.STEP_N_STEPS * W.STEP_N_DL, abs=1e-12)
