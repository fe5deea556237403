#!/usr/bin/env python3
"""The physics constants at the edges of what check_params admits: ONE table of constant sets, start states and kernel
families, shared by tests/test_constant_edges_cpu.py (keeps the table honest on the float64 oracle and on a host build of
csrc/dw_plan.hpp) and tests/test_gpu_constant_edges.py (holds every kernel family to the oracle with these sets).

A case is a set of overrides on the default constants plus the luminosity schedule it runs at: the same overrides appear
twice where two schedules reach different branches (p = 0.7 inside and below the comfortable range).  `admissible` is what
tie_chain() of dw_plan.hpp says per step of the schedule (one flag where it does not change), `symmetric` what
albedo_symmetric() says; the CPU test asserts both on the host build.

Not in the table, and to stay out: p = 2 and the defaults at L = 0.1 - the float64 oracle itself returns NaN there (the
fourth root of a negative radiative balance).

As a program (GPU box) it measures what nobody can assert beforehand, per case, and prints it as JSON:
  * tie_ratio / flagged_share: the worst float32 error over the tie bound (`audit_tie_bound`) after each of 5 steps on
    4 x 64 x 64, and the share of cell values the tie test flags, for the admissible cases;
  * fast_max_quanta / fast_share: the float32-only mode against the oracle after ONE step from the table's state on
    2 x 12 x 256 - the largest deviation in quanta and the share of differing cell values.

usage (GPU box): python tools/constant_edge_cases.py [--out profiles/constant_edges.json]"""
import os
import sys

import numpy as np

Q = 0.2 * 1000.0 / 5.67e-8                                       # the default q (ref daisy_world_rl.py:38)


def _case(name, over, L0, L1, n, admissible=True, symmetric=True):
    """The schedule is a linear ramp of n steps from L0 to L1, accumulated as dw_step_n accumulates it (L += dL in
    float64): `L` lists the luminosities of the steps, and dw_step_n(n, L0, dL, 0, 10) takes exactly those."""
    dL = (float(L1) - float(L0)) / (n - 1) if n > 1 else 0.0
    L, x = [], float(L0)
    for _ in range(n):
        L.append(x)
        x += dL
    adm = [bool(admissible)] * n if isinstance(admissible, (bool, int)) else [bool(a) for a in admissible]
    assert len(adm) == n
    return {"name": name, "over": dict(over), "L": L, "L0": float(L0), "dL": dL, "L_end": x, "admissible": adm,
            "symmetric": bool(symmetric)}


# name, overrides, ramp from .. to .. in n steps (4 to 7, odd and even counts: a pair-taking family also ends on a single
# step; shorter only where the world is dead after that), admissible (per step where it changes), symmetric
CASES = [
    _case("dt=-1", dict(dt=-1.0), 0.8, 1.2, 5),
    _case("dt=-0.5", dict(dt=-0.5), 1.2, 0.8, 6),
    _case("dt=0", dict(dt=0.0), 0.8, 1.4, 4),
    _case("p=0.7", dict(p=0.7), 0.6, 0.8, 7),
    # L = 0.1 gives NaN on the oracle from this table's saturated patches; at 0.12 it is finite and 1 + emin = 0.010
    _case("p=0.7 L=0.12", dict(p=0.7), 0.12, 0.12, 3, admissible=False),
    _case("p=0.7 dt=-1 L=0.12", dict(p=0.7, dt=-1.0), 0.12, 0.12, 5, admissible=False),
    _case("p=1.3", dict(p=1.3), 1.2, 1.2, 4),
    _case("To=800 g=2e-6", dict(temp_optimal=800.0, g=2e-6), 0.6, 1.7, 6, admissible=False),
    # crosses the boundary (admissible from L = 0.6): the step pair (0.5, 0.6) holds one step of each kind
    _case("To=600 g=8e-6 ramp", dict(temp_optimal=600.0, g=8e-6), 0.3, 0.8, 6,
          admissible=[False, False, False, True, True, True]),
    _case("gamma=0", dict(gamma=0.0), 0.8, 0.8, 5),
    _case("gamma=-0.1", dict(gamma=-0.1), 0.8, 0.8, 4),
    _case("q=0", dict(q=0.0), 0.8, 0.8, 5),
    _case("q=0 q2=0", dict(q=0.0, q2=0.0), 0.8, 0.8, 4),
    _case("q2=q", dict(q2=Q), 0.8, 0.8, 5),
    _case("q2=2q", dict(q2=2.0 * Q), 0.8, 1.2, 6),
    _case("albedo=0.3/0.9/0.05", dict(albedo_bare=0.3, albedo_light=0.9, albedo_dark=0.05), 0.6, 0.8, 5, symmetric=False),
    _case("S=1368", dict(S=1368.0), 0.6, 0.8, 6),
    _case("albedo=0.5/0.5/0.5", dict(albedo_bare=0.5, albedo_light=0.5, albedo_dark=0.5), 0.8, 0.8, 5),
    _case("g=0", dict(g=0.0), 0.3, 3.0, 6),
    _case("g=1e-9", dict(g=1e-9), 3.0, 0.3, 5),
    _case("g=0.05 To=310", dict(g=0.05, temp_optimal=310.0), 1.2, 1.2, 4),
    # the defaults outside the ramp: everything dies - two steps, at L = 3.0 one (its second changes 2 % of the values)
    _case("default L=0.3", dict(), 0.3, 0.3, 2),
    _case("default L=1.7", dict(), 1.7, 1.7, 2),
    _case("default L=3.0", dict(), 3.0, 3.0, 1),
]
NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}
DT_ZERO = "dt=0"
NEUTRAL = "albedo=0.5/0.5/0.5"

# the cases with a shrunk-queue interest: one inadmissible, one dt < 0
QUEUE_CASES = ["To=800 g=2e-6", "dt=-1"]
# the per-world tables hold one row per case of at least this many steps (one (n, B) luminosity array: its first TABLE_STEPS)
TABLE_STEPS = 4
TABLE_CASES = [c["name"] for c in CASES if len(c["L"]) >= TABLE_STEPS]
TABLE_CASES_SYMMETRIC = [n for n in TABLE_CASES if BY_NAME[n]["symmetric"]]
# dw_run_episode with a shared set
EPISODE_CASES = ["dt=-1", "p=0.7", "To=800 g=2e-6", "gamma=0", "albedo=0.3/0.9/0.05", "g=0", "p=0.7 dt=-1 L=0.12", "q2=2q"]
EPISODE_SHAPE, EPISODE_AGENTS, EPISODE_K = (4, 8, 8), 2, 6
TABLE_EPISODE_SHAPE = (8, 8)                                     # (B = the table's rows, 8, 8), 2 agents
TEMPERATURE_CASES = ["p=0.7", "albedo=0.3/0.9/0.05", "S=1368"]
TEMPERATURE_SHAPES = [(3, 9, 50), (2, 12, 256)]
AUDIT_SHAPE, AUDIT_STEPS = (4, 64, 64), 5
ANCHOR_SHAPE = (2, 12, 256)                                      # the float32-only mode's anchor to the oracle: one step

# kernel families of the steady state: name, (B, H, W), environment switches set before the handle is created (every
# other switch of ALL_SWITCHES is removed), what kernel_info() must contain.  The shapes are the smallest with a ragged last row strip
# (wave strips of 8 rows, tiles of 32 / 32 / 16 rows) and a column seam.
_NO_PAIRS = {"DW_NO_FUSE": "1"}
# dw_step_n keeps worlds of up to 4096 cells in LDS (the episode kernels) unless told not to: the pair families run under
_STEP_N = {"DW_NO_EPISODE_KERNEL": "1"}
FAMILIES = [
    ("generic-5x7", (3, 5, 7), {}, ["step_generic<{prec}>"]),
    ("generic-9x50", (2, 9, 50), {}, ["step_generic<{prec}>"]),
    ("tiled-16", (2, 20, 64), {}, ["step_tiled<TCQ=16"]),
    ("tiled-32", (2, 20, 132), {}, ["step_tiled<TCQ=32"]),
    ("tiled-64", (1, 20, 260), {"DW_KERNEL": "tiled"}, ["step_tiled<TCQ=64"]),
    ("strip-packed", (5, 16, 32), {"DW_NO_FUSE": "1", "DW_PACK_MIN_STRIPS": "1"}, ["step_stream_{prec}<halo=packed>"]),
    ("strip-rotate", (2, 12, 256), _NO_PAIRS, ["step_stream_{prec}<halo=rotate>"]),
    ("strip-dpp-old", (1, 12, 512), _NO_PAIRS, ["step_stream_{prec}<halo=dpp-old>"]),
    ("strip-general", (1, 12, 260), _NO_PAIRS, ["step_stream_{prec}<halo=general>"]),
    ("pairs-packed", (5, 16, 32), dict(_STEP_N, DW_PACK_MIN_STRIPS="1"), ["halo=packed", "step_stream_fused2{exact}"]),
    ("pairs-rotating", (2, 12, 256), _STEP_N, ["halo=rotate", "step_stream_fused2{exact}"]),
    ("pairs-overlapped", (1, 12, 264), _STEP_N, ["halo=general", "step_stream_fused2{exact}"]),
    ("pairs-ring", (1, 12, 1024), _STEP_N, ["halo=dpp-old", "step_stream_fused2{exact}"]),
]
FAMILY_NAMES = [f[0] for f in FAMILIES]
BY_FAMILY = {f[0]: f for f in FAMILIES}
PAIR_MIN_STEPS = 3                                               # dw_step_n fuses pairs in runs of three or more steps


def pairs_of(n):
    """Step pairs dw_step_n fuses in a run of n steps from a quantised state: the last one or two steps are single."""
    return (n - 1) // 2 if n >= PAIR_MIN_STEPS else 0
QUEUE_FAMILIES = [f[0] for f in FAMILIES if f[0].startswith(("tiled", "strip"))]
QUEUE_SWITCHES = {"DW_TEST_QUEUE_CAP": "2", "DW_TEST_MISMATCH_CAP": "0"}
# every switch a family or a test of these cases sets: removed from the environment before a handle's own are applied
ALL_SWITCHES = ("DW_NO_FUSE", "DW_PACK_MIN_STRIPS", "DW_KERNEL", "DW_TEST_QUEUE_CAP", "DW_TEST_MISMATCH_CAP",
                "DW_NO_EPISODE_WAVE", "DW_NO_EPISODE_KERNEL", "DW_STRIP_ROWS", "DW_NO_RING", "DW_NO_PACK", "DW_NO_SYM",
                "DW_FIRST_STEP_F64", "DW_FIRST_GENERIC", "DW_TILE_RPT", "DW_TEST_FORCE_RESCAN", "DW_TEST_FIRST_SLACK")
# the first step from an un-quantised state: name, shape, switches, what kernel_info() must contain / must not contain
FIRST_FAMILIES = [
    ("first-generic", (3, 5, 7), {}, "step_generic<exact>", "first step: wave-strip"),
    ("first-stream", (2, 12, 256), {}, "first step: wave-strip", None),
    ("first-stream-packed", (5, 16, 32), {"DW_PACK_MIN_STRIPS": "1"}, "first step: wave-strip", None),
]
# every (B, H, W) an agent-free run of a case starts from the table's state at (the CPU test checks the oracle on each)
STEP_SHAPES = sorted({f[1] for f in FAMILIES} | {AUDIT_SHAPE})
PHYSICS = ("p", "g", "S", "sigma", "gamma", "q", "q2", "dt", "albedo_bare", "albedo_light", "albedo_dark", "temp_optimal")


def defaults():
    return dict(p=1.0, g=0.003265, S=1000.0, sigma=5.67e-8, gamma=0.25, q=Q, q2=Q / 8.0, dt=1.0, albedo_bare=0.5,
                albedo_light=0.75, albedo_dark=0.25, temp_optimal=295.5)


def constants(name):
    """The twelve physics constants of a case."""
    d = defaults()
    d.update(BY_NAME[name]["over"])
    return d


def table_schedule(name):
    """The case's column of a per-world luminosity table: its first TABLE_STEPS steps."""
    return BY_NAME[name]["L"][:TABLE_STEPS]


def episode_schedule(name):
    """1 + EPISODE_K luminosities, the case's schedule cycled: the zero-action step that quantises the uploaded state,
    then the EPISODE_K steps of the call under test."""
    return np.resize(np.asarray(BY_NAME[name]["L"]), 1 + EPISODE_K).tolist()


TABLE_QUANTISE_L = 1.0


def table_episode_state(c_oracle, B):
    """What a per-world episode call starts from: the table's state on (B, *TABLE_EPISODE_SHAPE) after the zero-action
    step that quantises it - taken with the handle's OWN constants, the defaults, at TABLE_QUANTISE_L (zero actions move
    the agents and graze nothing)."""
    shape = (B, *TABLE_EPISODE_SHAPE)
    light, dark = start_state(*shape, seed_of(*shape))
    g = c_oracle.forward(light, dark, TABLE_QUANTISE_L, c_oracle.OracleParams.defaults())
    return np.ascontiguousarray(g[:, 1]), np.ascontiguousarray(g[:, 2])


def first_schedule(name):
    """The first-step kernels: steps 1 to 3 from an un-quantised state (compared after step 1 and after step 3) - step 1
    alone where the case's own run is a single step (the world is dead after it)."""
    return BY_NAME[name]["L"][:3]


def seed_of(B, H, W):
    return 9000 + 131 * H + 7 * W + B


_PATCHES = ((1000, 0), (0, 1000), (0, 0), (500, 500))            # fully light, fully dark, empty, 500 / 500


def start_state_k(B, H, W, seed):
    """The quantised start state in per-mille integers, (light, dark) of shape (B, H, W): random cells with covers up
    to 1000, a third of them with light + dark = 1000 exactly, a quarter of each species empty; and 3 x 3 patches that are
    fully light, fully dark, empty and 500 / 500, so that whole neighbourhoods are saturated or empty.  A world holds one
    patch per corner it has room for (H, W >= 6: four), world b starting with kind b % 4: every kind occurs (asserted), on
    the smallest grid spread over the worlds."""
    rng = np.random.RandomState(seed)
    light = np.rint(rng.rand(B, H, W) * 1000.0) * (rng.rand(B, H, W) > 0.25)
    dark = np.rint(rng.rand(B, H, W) * 1000.0) * (rng.rand(B, H, W) > 0.25)
    over = light + dark > 1000
    full = rng.rand(B, H, W) < 1.0 / 3.0
    dark = np.where(over | full, 1000.0 - light, dark)          # light + dark = 1000, light alone up to 1000
    swap = rng.rand(B, H, W) < 0.5                                # ... and dark alone up to 1000
    light, dark = np.where(swap, dark, light), np.where(swap, light, dark)
    # the patches sit in the corners of the grid (on the wrap-around seams, in the first and last row and column strip)
    corners = [(r0, c0) for r0 in ([0, H - 3] if H >= 6 else [0]) for c0 in ([0, W - 3] if W >= 6 else [0])]
    kinds = set()
    for b in range(B):
        for j, (r0, c0) in enumerate(corners):
            kind = (b + j) % 4
            light[b, r0:r0 + 3, c0:c0 + 3], dark[b, r0:r0 + 3, c0:c0 + 3] = _PATCHES[kind]
            kinds.add(kind)
    assert kinds == {0, 1, 2, 3}, "the grid and batch are too small for the four patches"
    assert light.max() == 1000 and dark.max() == 1000 and (light + dark).max() == 1000 and light.min() == 0
    return light.astype(np.int64), dark.astype(np.int64)


def start_state(B, H, W, seed):
    """start_state_k as covers: float64 multiples of 0.001, as np.round(., 3) leaves them."""
    kl, kd = start_state_k(B, H, W, seed)
    return kl / 1000.0, kd / 1000.0


def first_state(B, H, W, seed):
    """An UN-quantised float64 start state for the first-step kernels: each species 1.0 * rand() on 70 % of the cells
    (covers up to 1.0, their sum up to 2.0), with the four 3 x 3 patches of start_state (saturated, empty, half / half)."""
    rng = np.random.RandomState(seed + 1)
    light = 1.0 * rng.rand(B, H, W) * (rng.rand(B, H, W) < 0.7)
    dark = 1.0 * rng.rand(B, H, W) * (rng.rand(B, H, W) < 0.7)
    kl, kd = start_state_k(B, H, W, seed)
    patch = ((kl == 1000) & (kd == 0)) | ((kl == 0) & (kd == 1000)) | ((kl == 500) & (kd == 500))
    light, dark = np.where(patch, kl / 1000.0, light), np.where(patch, kd / 1000.0, dark)
    return light, dark


def oracle_params(c_oracle, name):
    return c_oracle.OracleParams.defaults(**BY_NAME[name]["over"])


def oracle_run(c_oracle, name, light, dark, L=None, params=None):
    """The float64 oracle from (light, dark) over the case's schedule (or `L`): the list of (light, dark) after every step,
    as the oracle leaves them (np.round(., 3))."""
    P = params or oracle_params(c_oracle, name)
    out = []
    for lum in (BY_NAME[name]["L"] if L is None else L):
        g = c_oracle.forward(light, dark, float(lum), P)
        light, dark = np.ascontiguousarray(g[:, 1]), np.ascontiguousarray(g[:, 2])
        out.append((light, dark))
    return out


def k_of(x):
    return np.rint(np.asarray(x) * 1000.0).astype(np.int64)


def changed_share(a, b):
    """Share of the cell values (both species) that differ between two (light, dark) pairs."""
    return (np.count_nonzero(k_of(a[0]) != k_of(b[0])) + np.count_nonzero(k_of(a[1]) != k_of(b[1]))) / (2.0 * a[0].size)


# ---- the measurements (GPU box) ------------------------------------------------------------------------------------
def _engine(amd, shape, name, precision, N=0):
    from therldaisyworld_amd import _ffi
    p = amd.default_params(*shape, N)
    p.precision = _ffi.PRECISION[precision]
    for k, v in BY_NAME[name]["over"].items():
        setattr(p, k, v)
    return amd.Engine(p)


def audit(amd, name):
    """(worst error / bound, flagged cell values, audited cell values, per-step admissibility as the audit saw it) over
    AUDIT_STEPS steps at the case's schedule (cycled) on AUDIT_SHAPE: the state is audited at the luminosity of the step
    it is about to take."""
    case = BY_NAME[name]
    eng = _engine(amd, AUDIT_SHAPE, name, "exact")
    light, dark = start_state(*AUDIT_SHAPE, seed_of(*AUDIT_SHAPE))
    eng.upload_state_f32(light.astype(np.float32), dark.astype(np.float32), quantised=True)
    rows = []
    for t in range(AUDIT_STEPS):
        i = t % len(case["L"])
        err, ratio, nf, n = eng.audit_tie_bound(case["L"][i])
        rows.append({"L": case["L"][i], "admissible": case["admissible"][i], "ratio": ratio, "err_quanta": err,
                     "flagged": nf, "audited": n})
        eng.step(case["L"][i])
    eng.close()
    return rows


def anchor(amd, c_oracle, name):
    """The float32-only mode against the oracle after ONE step from the table's state on ANCHOR_SHAPE (the single-step
    wave-strip kernel): (largest deviation in quanta, share of differing cell values)."""
    case = BY_NAME[name]
    light, dark = start_state(*ANCHOR_SHAPE, seed_of(*ANCHOR_SHAPE))
    eng = _engine(amd, ANCHOR_SHAPE, name, "fast")
    eng.upload_state_f32(light.astype(np.float32), dark.astype(np.float32), quantised=True)
    eng.step(case["L"][0])
    got = eng.download_planes()
    eng.close()
    ref = oracle_run(c_oracle, name, light, dark, case["L"][:1])[0]
    dl, dd = np.abs(k_of(got[0]) - k_of(ref[0])), np.abs(k_of(got[1]) - k_of(ref[1]))
    return int(max(dl.max(), dd.max())), (np.count_nonzero(dl) + np.count_nonzero(dd)) / (2.0 * dl.size)


def measure():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.setdefault("DW_NO_FUSE", "1")
    import therldaisyworld_amd as amd
    from oracle import c_oracle
    out = {"audit_shape": list(AUDIT_SHAPE), "audit_steps": AUDIT_STEPS, "anchor_shape": list(ANCHOR_SHAPE), "cases": {}}
    for case in CASES:
        name = case["name"]
        rows = audit(amd, name)
        adm = [r for r in rows if r["admissible"]]
        rec = {"over": case["over"], "L": case["L"], "admissible": case["admissible"],
               "tie_ratio": max((r["ratio"] for r in adm), default=None),
               "tie_err_quanta": max((r["err_quanta"] for r in adm), default=None),
               "flagged_share": (sum(r["flagged"] for r in adm) / sum(r["audited"] for r in adm)) if adm else None,
               "inadmissible_steps_all_flagged": all(r["flagged"] == r["audited"] for r in rows if not r["admissible"])}
        if case["admissible"][0]:
            rec["fast_max_quanta"], rec["fast_share"] = anchor(amd, c_oracle, name)
        out["cases"][name] = rec
    return out


if __name__ == "__main__":
    import argparse
    import json
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    text = json.dumps(measure(), indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
