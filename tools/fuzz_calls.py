#!/usr/bin/env python3
"""State-machine fuzz of EVERY state-changing C ABI call (through the Engine wrapper): random interleavings of the uploads,
the single steps and device policies, dw_step_n, the step series (dw_step_n_trace, _per_world, _temperature, _ensemble,
dw_step_n_frames), the episode loops (dw_run_episode, _trace[_temperature], _ensemble[_trace], _mlp[_trace]), both snapshot
slots, dw_set_params and the reads (planes, agents, reductions, temperature statistics, tiles, observations, the grid, the
caches, the stateless side computations) on ONE handle - what tools/fuzz_engine.py does for the nine calls of round 3.

Three separable parts:
  plan_case(seed)   pure Python / NumPy: shape, precision, switches and the whole list of operations with every argument,
                    drawn only where the predicted state of the handle admits them (plus deliberate refusals).  Every
                    planned operation is executed: nothing is dropped at run time.
  Model             the float64 reference: one OracleDaisyWorld per world, one method per operation (Reference.op_*),
                    no GPU code.  Twin is the same interface on B one-world engines driven by per-step primitives only:
                    the reference of the float32-only mode (bit for bit) and, in a third of the exact cases, of the
                    temperature rows and means.
  run_case(seed, log)  executes a plan on an Engine and compares after every operation.

usage: fuzz_calls.py [cases=30] [seed=1]"""
import copy
import hashlib
import os
import sys

os.environ.setdefault("DW_TEST_HOOKS", "1")     # the DW_TEST_* caps below are honoured only under it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

from oracle import daisy_oracle as O  # noqa: E402
from therldaisyworld_amd import _ffi  # noqa: E402  (importing the package needs no GPU)
import constant_edge_cases as CE  # noqa: E402

PHYS = _ffi.WORLD_PARAM_NAMES
_DEFAULT = O.Params()
DEFAULT_CONSTS = {n: float(getattr(_DEFAULT, n)) for n in PHYS}
# constant sets of tools/constant_edge_cases.py that stay finite on the oracle for every cover and every luminosity of
# the cases' range [0.7, 1.3] (no fourth root of a negative balance) and that all three precisions accept (g >= 0)
CONST_SETS = ["default", "gamma=0", "q2=2q", "S=1368", "albedo=0.3/0.9/0.05", "dt=-0.5", "g=0.05 To=310",
              "albedo=0.5/0.5/0.5"]
L_MIN, L_MAX = 0.7, 1.3
THRESHOLD_K = 5

# (H, W), the batches, the agent counts: the smallest shapes at which each kernel family is still reached
SHAPES = [((8, 8), (5, 33), (0, 1, 2, 3, 4)), ((16, 16), (3,), (4, 6)), ((5, 13), (3,), (2,)), ((12, 12), (3,), (3,)),
          ((24, 32), (19,), (0, 1, 2)), ((64, 64), (2,), (0, 1, 2, 3)), ((40, 256), (2,), (0, 1, 2, 3)),
          ((70, 320), (1,), (0, 1, 2))]
TWIN_MAX_B = 4
SWITCHES = ("DW_PACK_MIN_STRIPS", "DW_TEST_QUEUE_CAP", "DW_TEST_MISMATCH_CAP", "DW_TEST_TRACE_ROWS", "DW_TEST_FRAME_RING",
            "DW_NO_EPISODE_WAVE", "DW_NO_EPISODE_KERNEL", "DW_NO_AGENT_FUSE", "DW_NO_SEAM_STRIPS", "DW_NO_FUSE", "DW_NO_PACK")
TWIN_SWITCHES = {"DW_NO_FUSE": "1", "DW_NO_PACK": "1", "DW_NO_EPISODE_KERNEL": "1", "DW_NO_EPISODE_WAVE": "1"}

UPLOADS = ("upload_f64", "upload_f32", "upload_f32q", "init_random")
STATE_IN = UPLOADS + ("upload_agents", "upload_actions")
SINGLE = ("step", "step_act", "step_sub", "env_step", "greedy_step", "per_agent_step", "mlp_step", "mlp_pop_step",
          "update_agents")
RUNS = ("step_n", "step_n_dev", "trace", "trace_pw", "trace_temp", "trace_temp_pw", "trace_ens", "trace_ens_temp", "frames")
EPISODES = ("ep_greedy", "ep_anti", "ep_table", "ep_trace", "ep_trace_temp", "ep_ens", "ep_ens_trace", "ep_ens_trace_temp",
            "ep_mlp", "ep_mlp_resident", "ep_mlp_trace")
SNAPSHOTS = ("save0", "save1", "restore0", "restore1")
CONSTANTS = ("set_params", "set_precision")
CHANGING = STATE_IN + SINGLE + RUNS + EPISODES + SNAPSHOTS + CONSTANTS
READS = ("r_planes", "r_prev", "r_agents", "r_actions", "r_reduce", "r_temp", "r_tiles", "r_obs", "r_reward", "r_grid",
         "r_caches", "r_forward", "r_conv", "r_stage", "r_lifespan")
REFUSALS = ("x_obs", "x_grid", "x_ep_mlp", "x_caches", "x_temp", "x_tiles")
KINDS = CHANGING + READS
MLP_KINDS = ("mlp_step", "mlp_pop_step", "ep_mlp", "ep_mlp_resident", "ep_mlp_trace")
PLAIN_EPISODES = ("ep_greedy", "ep_anti", "ep_table", "ep_trace", "ep_trace_temp", "ep_ens", "ep_ens_trace",
                  "ep_ens_trace_temp")
NEED_AGENTS = ("step_act", "step_sub", "update_agents", "greedy_step", "per_agent_step", "step_n_dev", "upload_agents",
               "upload_actions", "ep_table") + MLP_KINDS
# the twelve classes of (current quantised?, stepped?, owner and format of the un-quantised upload, per-world L?,
# per-world constants?) a handle can be in
CORE_CLASSES = [(False, False, "cur:f64", False, False), (False, False, "cur:f32", False, False),
                (True, False, "none", False, False)] + \
               [(True, True, u, pl, pp) for u in ("prev:f64", "prev:f32", "none")
                for pl, pp in ((False, False), (True, False), (True, True))]


def k(x):
    return np.rint(np.asarray(x) * 1000.0)


def const_set(name):
    c = dict(DEFAULT_CONSTS)
    if name != "default":
        c.update({n: float(v) for n, v in CE.BY_NAME[name]["over"].items()})
    return c


# ======================================================================================================================
# the predicted bookkeeping of struct dw_handle
# ======================================================================================================================
class PState:
    """What the library's host code keeps per handle, as far as it decides what a call may do and what it evaluates."""

    def __init__(self, precision, n_agents):
        self.N = n_agents
        self.precision = precision
        self.have_state = False
        self.unq, self.fmt = None, "f64"         # owner of the un-quantised upload: None / "cur" / "prev"; its format
        self.stepped = self.perL = self.perP = False
        self.agents = False                      # agents uploaded (N > 0)
        self.slots = [None, None]                # what a snapshot slot restores of the above
        self.mlp = 0                             # parameter sets resident on the device
        self.fresh = False                       # stepped since the last upload, restore or dw_set_params
        self.actions = False                     # the device action buffer holds values the plan knows
        self.stats_ok = False                    # dw_reduce describes the current state

    def quantised(self):
        return self.unq != "cur"

    def lacks_L(self):
        return self.stepped and self.perL

    def lacks_P(self):
        return self.lacks_L() and self.perP

    def core(self):
        u = "none" if self.unq is None else f"{self.unq}:{self.fmt}"
        return (self.quantised(), self.stepped, u, self.lacks_L(), self.lacks_P())

    def cls(self):
        return self.core() + (self.agents, self.slots[0] is not None, self.slots[1] is not None, self.mlp > 0)

    # -- transitions (step_done, episode_done, state_arrived, the snapshot calls) ---------------------------------------
    def arrived(self, kind):
        self.have_state = True
        self.unq, self.fmt = {"upload_f64": ("cur", "f64"), "upload_f32": ("cur", "f32"), "init_random": ("cur", "f32"),
                              "upload_f32q": (None, self.fmt)}[kind]
        self.stepped = self.fresh = False
        self.slots = [None, None]
        self.stats_ok = True
        if kind == "init_random" and self.N:
            self.agents = True

    def steps(self, n, mode="shared"):
        for _ in range(n):
            self.unq = "prev" if self.unq == "cur" else None
        self.stepped = self.fresh = self.stats_ok = True
        self.perL, self.perP = mode != "shared", mode == "LP"

    def save(self, slot):
        self.slots[slot] = dict(unq=self.unq, fmt=self.fmt, stepped=self.stepped, perL=self.perL, perP=self.perP,
                                agents=self.agents, stats_ok=self.stats_ok)

    def restore(self, slot):
        s = self.slots[slot]
        self.unq, self.fmt, self.stepped, self.perL, self.perP = s["unq"], s["fmt"], s["stepped"], s["perL"], s["perP"]
        self.stats_ok = s["stats_ok"]
        self.fresh = False

    # -- which calls the state admits (the planner's rule: the library's preconditions, narrowed where a result could
    #    not be held to the references bit for bit) -------------------------------------------------------------------
    def admits(self, kind):
        N, q, ag = self.N, self.quantised(), self.agents
        if kind in UPLOADS:
            return True
        if not self.have_state:
            return False
        if kind in NEED_AGENTS and not N:
            return False
        if kind in ("upload_agents", "upload_actions", "set_params"):
            return True
        if kind == "set_precision":
            return self.precision != "fast"
        if kind in ("step_act", "step_sub", "update_agents", "step_n_dev"):
            return ag
        if kind == "env_step":
            return N == 0 or ag
        if kind in ("greedy_step", "per_agent_step"):     # (a device policy on a float32 upload sums in float32)
            return ag and q
        if kind in MLP_KINDS:                             # observations that are bit-exact: a quantised step pair
            ok = ag and q and self.stepped and self.fresh and not self.lacks_L()
            return ok and (kind != "ep_mlp_resident" or self.mlp > 0)
        if kind in PLAIN_EPISODES:
            return q and self.precision != "f64" and (N == 0 or ag)
        if kind in ("save0", "save1"):
            return q
        if kind in ("restore0", "restore1"):
            return self.slots[int(kind[-1])] is not None
        # reads
        if kind == "r_prev":
            return self.stepped
        if kind in ("r_agents", "r_reward"):
            return N > 0 and ag
        if kind == "r_actions":
            return N > 0 and self.actions
        if kind == "r_reduce":
            return q and self.stats_ok
        if kind == "r_lifespan":                          # (the agents' counters read the energy stores)
            return q and self.stats_ok and (N == 0 or ag)
        if kind in ("r_temp", "r_caches"):
            return not self.lacks_P()
        if kind == "r_tiles":
            return q or not self.lacks_P()
        if kind == "r_obs":
            return N > 0 and ag and not self.lacks_L()
        if kind == "r_grid":
            return not self.lacks_L()
        # deliberate refusals
        if kind == "x_grid":
            return self.lacks_L()
        if kind in ("x_obs", "x_ep_mlp"):
            return self.lacks_L() and N > 0 and ag
        if kind in ("x_caches", "x_temp", "x_tiles"):
            return self.lacks_P()
        return True                                        # the agent-free steps and runs, the stateless reads


def feasible(kind, core, n_agents=2, precision="exact"):
    """Can `kind` be admissible in the class `core` at all (with agents, snapshots and parameter sets at their best)?"""
    S = PState(precision, n_agents)
    S.have_state = True
    q, stepped, u, pl, pp = core
    S.unq, S.fmt = (None, "f64") if u == "none" else tuple(u.split(":"))
    S.stepped, S.perL, S.perP, S.fresh = stepped, pl, pp, stepped
    S.agents, S.mlp, S.actions, S.stats_ok = n_agents > 0, 1, True, True
    if S.unq != "cur":                                     # (an upload invalidates both slots)
        S.slots = [dict(), dict()]
    return S.admits(kind)


# ======================================================================================================================
# the planner
# ======================================================================================================================
class Planner:
    def __init__(self, seed):
        self.rng = rng = np.random.RandomState(seed)
        (self.H, self.W), Bs, Ns = SHAPES[int(rng.randint(len(SHAPES)))]
        self.B, self.N = int(rng.choice(Bs)), int(rng.choice(Ns))
        self.precision = str(rng.choice(["exact", "exact", "exact", "f64", "fast", "fast"]))
        if self.precision == "fast" and self.B > TWIN_MAX_B:
            self.precision = "exact"
        self.twin = self.precision == "fast" or (self.precision == "exact" and self.B <= TWIN_MAX_B and rng.rand() < 1 / 3)
        env = {}
        if rng.rand() < 0.5:
            env["DW_PACK_MIN_STRIPS"] = "1"
        if rng.rand() < 1 / 3:
            env["DW_TEST_QUEUE_CAP"] = str(int(rng.choice([1, 4, 16])))
            env["DW_TEST_MISMATCH_CAP"] = str(int(rng.choice([0, 1, 2])))
        if rng.rand() < 1 / 3:
            env["DW_TEST_TRACE_ROWS"] = str(int(rng.choice([2, 4])))
            env["DW_TEST_FRAME_RING"] = str(int(rng.choice([1, 2])))
        if rng.rand() < 0.25:
            env[str(rng.choice(["DW_NO_EPISODE_WAVE", "DW_NO_EPISODE_KERNEL", "DW_NO_AGENT_FUSE", "DW_NO_SEAM_STRIPS"]))] = "1"
        self.env = env
        self.S = PState(self.precision, self.N)
        self.consts = "default"
        self.L = float(rng.uniform(0.8, 1.2))
        self.ops = []
        self.n_changing = 0
        self.long_k_left = 1 if self.H * self.W <= 256 else 0
        self.nested = False

    # -- arguments ------------------------------------------------------------------------------------------------------
    def _L(self):
        self.L = float(np.clip(self.L + self.rng.uniform(-0.01, 0.02), 0.75, 1.25))
        return self.L

    def _sched(self, n, per_world=False):
        dL = float(self.rng.uniform(-0.005, 0.02))
        Ls = np.clip(self._L() + dL * np.arange(n), L_MIN, L_MAX)
        self.L = float(np.clip(Ls[-1], 0.75, 1.25))
        if not per_world:
            return Ls
        off = self.rng.uniform(-0.1, 0.1, size=self.B)
        return np.ascontiguousarray(np.clip(Ls[:, None] + off[None, :], L_MIN, L_MAX))

    def _cover(self):
        r, s = self.rng, (self.B, self.H, self.W)
        return r.rand(*s) * 0.4 * (r.rand(*s) < 0.5), r.rand(*s) * 0.4 * (r.rand(*s) < 0.5)

    def _actions(self, b=None, n=None):
        return self.rng.randint(9, size=(self.B if b is None else b, self.N if n is None else n)).astype(np.int32)

    def _table(self):
        names = [str(self.rng.choice(CONST_SETS)) for _ in range(self.B)]
        return names, np.array([[const_set(nm)[f] for f in PHYS] for nm in names], dtype=np.float64)

    def _K(self):
        if self.long_k_left and self.rng.rand() < 0.3:
            self.long_k_left -= 1
            return int(self.rng.randint(65, 71))
        return int(self.rng.randint(2, 10))

    def _mlp_sets(self, n):
        return self.rng.randn(n, 1808) * 0.5

    def _tile(self):
        if self.rng.rand() < 0.4:
            return (1, 1)
        dh = [d for d in range(1, self.H + 1) if self.H % d == 0]
        dw = [d for d in range(1, self.W + 1) if self.W % d == 0]
        return (int(self.rng.choice(dh)), int(self.rng.choice(dw)))

    def _worlds(self):
        if self.rng.rand() < 0.5:
            return None
        n = int(self.rng.randint(1, self.B + 1))
        return self.rng.permutation(self.B)[:n].astype(np.int32)

    def _episode_policy(self, kind, K):
        """mode, use_table, table of a scripted episode."""
        r, B, N = self.rng, self.B, self.N
        mode = {"ep_greedy": "greedy", "ep_anti": "anti", "ep_table": "table"}.get(
            kind, str(r.choice(["greedy", "anti", "table"] if N else ["greedy", "anti"])))
        use_table = table = None
        if mode == "table" or (N and r.rand() < 0.4):
            table = r.randint(-2, 9, size=(K, B, N)).astype(np.int8)
            if mode != "table":
                use_table = (r.rand(K) < 0.5).astype(np.uint8)
        return dict(mode=mode, use_table=use_table, table=table)

    # -- one operation -----------------------------------------------------------------------------------------------
    def emit(self, kind, force_n=None):
        """Draw the arguments of `kind`, record it with the class it is planned from, advance the predicted state."""
        S, r, B, N = self.S, self.rng, self.B, self.N
        assert S.admits(kind), (kind, S.cls())
        op = dict(kind=kind, cls=S.cls(), precision=S.precision, fresh_before=S.fresh)
        n = int(force_n or r.randint(1, 10))
        if kind in UPLOADS:
            if kind == "init_random":
                op["rseed"] = int(r.randint(1, 2 ** 31))
            else:
                light, dark = self._cover()
                if kind == "upload_f32q":
                    light, dark = np.round(light, 3), np.round(dark, 3)
                if kind != "upload_f64":
                    light, dark = light.astype(np.float32), dark.astype(np.float32)
                op.update(light=light, dark=dark)
            S.arrived(kind)
        elif kind == "upload_agents":
            op.update(idx=np.stack([r.randint(self.H, size=(B, N)), r.randint(self.W, size=(B, N))], axis=-1).astype(np.int32),
                      st=np.round(r.rand(B, N), 3))
            S.agents = True
            S.fresh = False                        # (the grid's agent stamps are those of the last step)
        elif kind == "upload_actions":
            op["a"] = self._actions()
            S.actions = True
        elif kind in ("step", "step_act", "step_sub", "env_step"):
            op["L"] = self._L()
            if kind == "step_act" or (kind == "env_step" and N and r.rand() < 0.7):
                op["a"] = self._actions()
            elif kind == "step_sub":
                op["a"] = self._actions(int(r.randint(1, B + 1)), int(r.randint(1, N + 1)))
            S.steps(1)
        elif kind == "greedy_step":
            op.update(L=self._L(), argmin=bool(r.randint(2)))
            S.steps(1)
            S.actions = True
        elif kind == "per_agent_step":
            op.update(L=self._L(), a=self._actions(), modes=r.choice([_ffi.POLICY_ARGMAX, _ffi.POLICY_ARGMIN, _ffi.POLICY_TABLE],
                                                                   size=N).astype(np.int32))
            S.steps(1)
            S.actions = True
        elif kind == "mlp_step":
            op.update(L=self._L(), params=self._mlp_sets(2), split=int(r.randint(0, N + 1)))
            S.steps(1)
            S.actions = True
        elif kind == "mlp_pop_step":
            P = int(r.randint(1, 4))
            op.update(L=self._L(), params=self._mlp_sets(P), member=r.randint(P, size=B).astype(np.int32))
            S.steps(1)
            S.actions = True
        elif kind == "update_agents":
            op["a"] = self._actions(int(r.randint(1, B + 1)), int(r.randint(1, N + 1)))
            S.stats_ok = S.fresh = False          # (grazing alone refreshes neither the reductions nor the grid's stamps)
        elif kind in ("step_n", "step_n_dev"):
            op.update(n=n, L=self._L(), dL=float(r.uniform(-0.005, 0.02)), lo=0.72, hi=1.28)
            if kind == "step_n_dev":
                op["a"] = self._actions()
                S.actions = True
            S.steps(n)
        elif kind in ("trace", "trace_temp"):
            op["Ls"] = self._sched(n)
            S.steps(n)
        elif kind in ("trace_pw", "trace_temp_pw"):
            op["Ls"] = self._sched(n, True)
            S.steps(n, "L")
        elif kind in ("trace_ens", "trace_ens_temp"):
            op["Ls"] = self._sched(n, True)
            op["sets"], op["tab"] = self._table()
            S.steps(n, "LP")
        elif kind == "frames":
            op.update(Ls=self._sched(n), stride=int(r.randint(1, 4)), tile=self._tile(), worlds=self._worlds(),
                      cover=bool(r.rand() < 0.8))
            op["temperature"] = bool(r.rand() < 0.7) or not op["cover"]
            S.steps(n)
        elif kind in PLAIN_EPISODES:
            K = self._K()
            op.update(self._episode_policy(kind, K))
            if kind.startswith("ep_ens"):
                op["Ls"] = self._sched(K, True)
                op["sets"], op["tab"] = self._table()
                S.steps(K, "LP")
            else:
                op["Ls"] = self._sched(K)
                op["world_flags"] = bool(r.rand() < 0.6)
                S.steps(K)
            if N:
                S.actions = True
        elif kind in ("ep_mlp", "ep_mlp_resident", "ep_mlp_trace"):
            K = self._K()
            op.update(Ls=self._sched(K), split=int(r.randint(0, N + 1)))
            nm = S.mlp if kind == "ep_mlp_resident" else int(r.randint(1, 4))
            op["n_members"] = nm
            op["params"] = None if kind == "ep_mlp_resident" or (kind == "ep_mlp_trace" and S.mlp and r.rand() < 0.3) \
                else self._mlp_sets(nm)
            if op["params"] is None:
                op["n_members"] = nm = S.mlp
            if nm > 1 or r.rand() < 0.5:
                op.update(member_a=r.randint(nm, size=B).astype(np.int32), member_b=r.randint(nm, size=B).astype(np.int32))
            if kind == "ep_mlp_trace":
                op["trace"] = bool(r.rand() < 0.7)
                op["temperature"] = bool(r.rand() < 0.6) or not op["trace"]
            S.mlp = nm
            S.steps(K)
            S.actions = True
        elif kind in ("save0", "save1"):
            S.save(int(kind[-1]))
        elif kind in ("restore0", "restore1"):
            sl = S.slots[int(kind[-1])]
            op["slot_mode"] = (sl["stepped"] and sl["perL"], sl["stepped"] and sl["perL"] and sl["perP"])
            S.restore(int(kind[-1]))
        elif kind == "set_params":
            self.consts = op["set"] = str(r.choice([c for c in CONST_SETS if c != self.consts]))
            S.fresh = False
        elif kind == "set_precision":
            S.precision = op["to"] = "f64" if S.precision == "exact" else "exact"
            S.fresh = False
        # ---- reads ----
        elif kind in ("r_temp", "r_obs", "r_grid", "r_caches", "x_obs", "x_grid", "x_caches", "x_temp"):
            op["L"] = float(r.uniform(0.8, 1.2))
        elif kind in ("r_tiles", "x_tiles"):
            cover = bool(S.quantised() and (S.lacks_P() or r.rand() < 0.8))
            temp = kind == "x_tiles" or (not S.lacks_P() and (not cover or r.rand() < 0.7))
            op.update(L=float(r.uniform(0.8, 1.2)), tile=self._tile(), worlds=self._worlds(), cover=cover, temperature=bool(temp))
        elif kind in ("r_forward", "r_conv", "r_stage"):
            light, dark = self._cover()
            op.update(light=light, dark=dark, L=float(r.uniform(0.8, 1.2)), kernel=r.rand(3, 3))
        elif kind == "x_ep_mlp":
            nm = int(r.randint(1, 3))
            op.update(Ls=self._sched(3), params=self._mlp_sets(nm), n_members=nm, split=N // 2,
                      member_a=np.zeros(B, np.int32), member_b=np.zeros(B, np.int32))
        op["post"] = S.cls()
        op["post_fresh"] = S.fresh
        op["consts"] = self.consts
        self.ops.append(op)
        if kind in CHANGING:
            self.n_changing += 1
            self._reads()
            if kind in SINGLE + RUNS + EPISODES and S.admits("save0") and r.rand() < 0.12:
                self.emit(f"save{int(r.randint(2))}")         # a slot that a later restore finds in another state
        return op

    def _reads(self, everything=False):
        S, r = self.S, self.rng
        can = [kd for kd in READS if S.admits(kd)]
        if not everything:
            can = list(r.permutation(can)[:int(r.randint(0, 4))])
        for kd in can:
            self.emit(kd)
        if self.nested:                                       # (the reads behind a restore that follows a refusal)
            return
        refused = False
        for kd in REFUSALS:
            if S.admits(kd) and (everything or r.rand() < 0.3):
                self.emit(kd)
                refused = True
        valid = [s for s in (0, 1) if S.slots[s] is not None]
        if refused and valid and r.rand() < 0.3:              # the refused call must have left the slots alone too
            self.nested = True
            self.emit(f"restore{int(r.choice(valid))}")
            self.nested = False

    # -- reaching a class --------------------------------------------------------------------------------------------
    def _pick(self, kinds):
        can = [kd for kd in kinds if self.S.admits(kd)]
        return str(self.rng.choice(can))

    SHARED_STEPS = ("step", "step_act", "step_sub", "env_step", "step_n", "step_n_dev", "trace", "trace_temp", "frames",
                    "greedy_step", "per_agent_step")
    MODE_STEPS = {"shared": SHARED_STEPS, "L": ("trace_pw", "trace_temp_pw"), "LP": ("trace_ens", "trace_ens_temp")}

    def goto(self, core):
        S = self.S
        if S.have_state and S.core() == core:
            return
        q, stepped, u, pl, pp = core
        mode = "LP" if pp else ("L" if pl else "shared")
        if u.startswith("cur") or u.startswith("prev"):
            self.emit("upload_f64" if u.endswith("f64") else self._pick(("upload_f32", "init_random")))
            if u.startswith("prev"):
                self.emit(self._pick(self.MODE_STEPS[mode]), force_n=1)
        elif not stepped:
            self.emit("upload_f32q")
        else:
            if not S.have_state:
                self.emit(self._pick(UPLOADS))
            if S.unq == "cur":
                self.emit(self._pick(self.SHARED_STEPS))
            kinds = self.MODE_STEPS[mode]
            if mode == "LP" and S.admits("ep_ens"):
                kinds = kinds + ("ep_ens", "ep_ens_trace", "ep_ens_trace_temp")
            if S.unq is not None or S.core() != core:
                self.emit(self._pick(kinds), force_n=None if S.unq is None else 2)

    def reach(self, kind, core):
        """The operations that make `kind` admissible in the class `core`; False when this case cannot get there."""
        S = self.S
        if not feasible(kind, core, self.N, S.precision):
            return False
        if kind in NEED_AGENTS or (self.N and kind in PLAIN_EPISODES + ("env_step",)):
            if not S.agents:
                if not S.have_state:
                    self.emit(self._pick(UPLOADS))
                if not S.agents:
                    self.emit("upload_agents")
        if kind == "ep_mlp_resident" and not S.mlp:
            if not self.reach("ep_mlp", CORE_CLASSES[-3]):
                return False
            self.emit("ep_mlp")
        self.goto(core)
        if kind in MLP_KINDS and not S.fresh and S.unq is None and S.stepped and not S.lacks_L():
            self.emit("step")
        if kind.startswith("restore") and S.quantised() and S.slots[int(kind[-1])] is None:
            self.emit(f"save{kind[-1]}")
        return S.core() == core and S.admits(kind)

    def plan(self):
        r = self.rng
        targets = [(kd, c) for kd in CHANGING for c in CORE_CLASSES if feasible(kd, c, self.N, self.precision)]
        order = r.permutation(len(targets))
        budget = int(r.randint(26, 40))
        if not self.N or r.rand() < 0.75:
            self.emit(self._pick(UPLOADS))
            if self.N and not self.S.agents:
                self.emit("upload_agents")
        else:                                               # a stretch without agents: the agent-free calls only
            self.emit(self._pick(("upload_f64", "upload_f32", "upload_f32q")))
        for i in order:
            if self.n_changing >= budget:
                break
            kind, core = targets[i]
            if self.reach(kind, core):
                self.emit(kind)
        self._reads(everything=True)
        return dict(seed=None, H=self.H, W=self.W, B=self.B, N=self.N, precision=self.precision, twin=bool(self.twin),
                    env=self.env, ops=self.ops)


def plan_case(seed):
    """The whole case as data: shape, precision, switches, and every operation with its arguments, the class of the
    handle's predicted state before (`cls`) and after (`post`) it.  Pure Python and NumPy; deterministic per seed."""
    plan = Planner(int(seed)).plan()
    plan["seed"] = int(seed)
    return plan


def digest(plan):
    """A hash of everything a plan holds (the determinism test)."""
    h = hashlib.sha1()

    def walk(x):
        if isinstance(x, dict):
            for key in sorted(x):
                h.update(str(key).encode())
                walk(x[key])
        elif isinstance(x, (list, tuple)):
            h.update(b"[")
            for v in x:
                walk(v)
        elif isinstance(x, np.ndarray):
            h.update(str(x.dtype).encode() + str(x.shape).encode() + np.ascontiguousarray(x).tobytes())
        else:
            h.update(repr(x).encode())
    walk(plan)
    return h.hexdigest()


def describe(op):
    bits = [op["kind"]]
    for key in ("n", "set", "to", "stride", "tile", "mode", "world_flags", "trace", "temperature", "n_members", "split"):
        if key in op:
            bits.append(f"{key}={op[key]}")
    if "Ls" in op:
        bits.append(f"steps={len(op['Ls'])}")
    if "params" in op and op["params"] is None:
        bits.append("params=None")
    return " ".join(bits)


# ======================================================================================================================
# the references: one method per operation, built on a few per-step primitives
# ======================================================================================================================
def _stats_rec(light, dark):
    """(B,) dw_world_stats records of (B, H, W) covers."""
    kl, kd = k(light), k(dark)
    out = np.zeros(light.shape[0], dtype=_ffi.STATS_DTYPE)
    out["max_k"] = np.maximum(kl.max(axis=(1, 2)), kd.max(axis=(1, 2)))
    out["sum_light_k"] = kl.sum(axis=(1, 2))
    out["sum_dark_k"] = kd.sum(axis=(1, 2))
    return out


def _temp_rec(field):
    """(B,) dw_temp_stats records of a (B, H, W) temperature field."""
    out = np.zeros(field.shape[0], dtype=_ffi.TEMP_STATS_DTYPE)
    out["mean"], out["std"] = field.mean(axis=(1, 2)), field.std(axis=(1, 2))
    out["min"], out["max"] = field.min(axis=(1, 2)), field.max(axis=(1, 2))
    return out


def _tiles_of(x, tile, sel, how):
    th, tw = tile
    x = x if sel is None else x[np.asarray(sel)]
    S, H, W = x.shape
    return getattr(x.reshape(S, H // th, th, W // tw, tw), how)(axis=(2, 4))


class Reference:
    """The bookkeeping every reference shares, and every operation spelled out in per-step primitives.  A subclass gives
    the primitives: _load, _init_random, _set_agents, _graze, _forward, _install / _uninstall, planes, agents_now, stats,
    obs, grid, tiles, temp_on_demand, caches, _save, _restore, _set_consts."""
    exact_floats = False                                   # are float64 results the engine's bytes (Twin) or close (Model)?

    def __init__(self, H, W, B, N, precision):
        self.H, self.W, self.B, self.N = H, W, B, N
        self.S = PState(precision, N)
        self.actions = None
        self.mlp_sets = None
        self.L_last = 0.0
        self.done_at = np.zeros(B, np.int32)
        self.agents_done_at = np.zeros((B, N, 1), np.int32)
        self.slot_L = [None, None]

    # -- policies, from the reference's own observations ------------------------------------------------------------------
    def _greedy(self, argmin):
        return O.OracleGreedy(epsilon=0.0, greedy=not argmin)(self.obs(0.9)).reshape(self.B, self.N).astype(np.int32)

    def _resolve(self, codes):
        a = codes.astype(np.int32)
        if (a < 0).any():
            a = np.where(a == -1, self._greedy(False), np.where(a == -2, self._greedy(True), a))
        return a.astype(np.int32)

    def _mlp_actions(self, sets, member_a, member_b, split):
        obs, a = self.obs(0.9), np.zeros((self.B, self.N), np.int32)
        for b in range(self.B):
            for lo, hi, m in ((0, split, member_a), (split, self.N, member_b)):
                if hi > lo:
                    net = O.OracleMLP(sets[0 if m is None else int(m[b])])
                    a[b, lo:hi] = net.get_action(obs[b, lo:hi])[:, 0]
        return a

    def _rewards(self):
        st = self.agents_now()[1].reshape(self.B, self.N, 1)
        reward = st * (st > 0)
        return reward, reward < 0.1

    # -- a step ------------------------------------------------------------------------------------------------------------
    def _step(self, Lv, a=None, mode="shared", want_temp=False):
        """One step of every world, world b at Lv[b]; `a`: a leading (ab, an) block of actions, or None (no agent update).
        Returns the temperature records of the field the step computes when asked."""
        if a is not None and self.N:
            self._graze(np.asarray(a))
        rec = self._forward(np.asarray(Lv, dtype=np.float64), want_temp)
        self.S.steps(1, mode)
        self.L_last = float(Lv[0])
        return rec

    def _run(self, Ls, mode="shared", policy=None, tab=None, want_temp=False):
        """A run of steps: Ls (n,) or (n, B); policy(t) -> actions of step t or None.  Returns the rows of the run."""
        Ls = np.asarray(Ls, dtype=np.float64)
        Lm = Ls if Ls.ndim == 2 else np.repeat(Ls[:, None], self.B, axis=1)
        out = dict(stats=[], temps=[], ok=[], reward=[], done=[])
        if tab is not None:
            self._install(tab)
        try:
            for t in range(Lm.shape[0]):
                a = policy(t) if policy else None
                if a is not None and self.N:
                    self.actions = np.asarray(a, dtype=np.int32).copy()
                out["temps"].append(self._step(Lm[t], a, mode, want_temp))
                out["stats"].append(self.stats())
                if self.N and self.S.agents:
                    reward, done = self._rewards()
                    out["reward"].append(reward)
                    out["done"].append(done)
        finally:
            if tab is not None:
                self._uninstall()
        res = dict(stats=np.stack(out["stats"]))
        if want_temp:
            res["temps"] = np.stack(out["temps"])
        if out["reward"]:
            res["reward"], res["done"] = np.stack(out["reward"]), np.stack(out["done"])
        return res

    # -- the operations ----------------------------------------------------------------------------------------------------
    def apply(self, op, eng_state=None):
        """What the call must return (a dict: only what is comparable), after updating the reference."""
        kind = op["kind"]
        S, B, N = self.S, self.B, self.N
        if kind in UPLOADS:
            if kind == "init_random":
                self._init_random(op["rseed"], eng_state)
            else:
                self._load(kind, op["light"], op["dark"], eng_state)
            S.arrived(kind)
            return {}
        if kind == "upload_agents":
            self._set_agents(op["idx"], op["st"])
            S.agents = True
            S.fresh = False
            return {}
        if kind == "upload_actions":
            self.actions = op["a"].copy()
            S.actions = True
            return {}
        if kind in ("step", "step_act", "step_sub"):
            self._step(np.full(B, op["L"]), op.get("a"))
            return {}
        if kind == "env_step":
            self._step(np.full(B, op["L"]), op.get("a"))
            res = dict(obs=self.obs(op["L"]))
            if N and S.agents:
                res["reward"], res["done"] = self._rewards()
            return res
        if kind == "greedy_step":
            self.actions = self._greedy(op["argmin"])
        elif kind == "per_agent_step":
            a, g0, g1 = op["a"].copy(), self._greedy(False), self._greedy(True)
            for n_, m in enumerate(op["modes"]):
                if m != _ffi.POLICY_TABLE:
                    a[:, n_] = (g1 if m == _ffi.POLICY_ARGMIN else g0)[:, n_]
            self.actions = a
        elif kind == "mlp_step":
            self.actions = self._mlp_actions(op["params"], np.zeros(B, int), np.ones(B, int), op["split"])
        elif kind == "mlp_pop_step":
            self.actions = self._mlp_actions(op["params"], op["member"], op["member"], N)
        if kind in ("greedy_step", "per_agent_step", "mlp_step", "mlp_pop_step"):
            S.actions = True
            self._step(np.full(B, op["L"]), self.actions)
            return {}
        if kind == "update_agents":
            self._graze(op["a"])
            S.stats_ok = S.fresh = False
            return {}
        if kind in ("step_n", "step_n_dev"):
            Ls, L = [], op["L"]
            for _ in range(op["n"]):
                Ls.append(L)
                L += op["dL"]
                L = op["hi"] if L > op["hi"] else L
                L = op["lo"] if L < op["lo"] else L
            if kind == "step_n_dev":
                self.actions = op["a"].copy()
                S.actions = True
                self._run(np.array(Ls), policy=lambda t: self.actions)
            else:
                self._run(np.array(Ls))
            return dict(L=L)
        if kind in ("trace", "trace_pw", "trace_temp", "trace_temp_pw", "trace_ens", "trace_ens_temp"):
            mode = "LP" if "ens" in kind else ("L" if kind.endswith("pw") else "shared")
            res = self._run(op["Ls"], mode, tab=op.get("tab"), want_temp="temp" in kind)
            return {key: res[key] for key in ("stats", "temps") if key in res}
        if kind == "frames":
            cov, tmp, rows = [], [], []
            for t, L in enumerate(op["Ls"]):
                self._step(np.full(B, L))
                rows.append(self.stats())
                if (t + 1) % op["stride"] == 0:
                    c, m = self.tiles(L, op["tile"], op["worlds"], op["cover"], op["temperature"])
                    cov.append(c)
                    tmp.append(m)
            res = dict(stats=np.stack(rows))
            if cov and op["cover"]:
                res["cover"] = np.stack(cov)
            if tmp and op["temperature"]:
                res["tmean"] = np.stack(tmp)
            return res
        if kind in PLAIN_EPISODES:
            greedy = {"greedy": False, "anti": True}

            def policy(t):
                if not N:
                    return None
                if op["mode"] == "table" or (op["use_table"] is not None and op["use_table"][t]):
                    return self._resolve(op["table"][t])
                return self._greedy(greedy[op["mode"]])
            ens = kind.startswith("ep_ens")
            res = self._run(op["Ls"], "LP" if ens else "shared", policy, tab=op.get("tab"), want_temp="temp" in kind)
            out = dict(alive=res["stats"]["max_k"] > THRESHOLD_K)
            if N:
                out["ok"] = ~res["done"][..., 0]
                S.actions = True
            if kind in ("ep_greedy", "ep_anti", "ep_table") and not op["world_flags"]:
                del out["alive"]
            if "trace" in kind:
                out["stats0"] = res["stats"]
            if "temp" in kind:
                out["temps"] = res["temps"]
            return out
        if kind in ("ep_mlp", "ep_mlp_resident", "ep_mlp_trace"):
            if op["params"] is not None:
                self.mlp_sets = op["params"].copy()
            sets = self.mlp_sets
            S.mlp = op["n_members"]
            res = self._run(op["Ls"], policy=lambda t: self._mlp_actions(sets, op.get("member_a"), op.get("member_b"), op["split"]),
                            want_temp=bool(op.get("temperature")))
            S.actions = True
            out = dict(reward=res["reward"], done=res["done"])
            if op.get("trace"):
                out["stats0"] = res["stats"]
            if op.get("temperature"):
                out["temps"] = res["temps"]
            return out
        if kind in ("save0", "save1"):
            s = int(kind[-1])
            self._save(s)
            self.slot_L[s] = self.L_last
            S.save(s)
            return {}
        if kind in ("restore0", "restore1"):
            s = int(kind[-1])
            self._restore(s, S.slots[s]["agents"])
            self.L_last = self.slot_L[s]
            S.restore(s)
            return {}
        if kind == "set_params":
            self._set_consts(const_set(op["set"]), S.precision)
            S.fresh = False
            return {}
        if kind == "set_precision":
            S.precision = op["to"]
            self._set_consts(None, S.precision)
            S.fresh = False
            return {}
        return self.read(op)

    def read(self, op):
        kind, S = op["kind"], self.S
        if kind == "r_planes":
            return dict(planes=self.planes(False), quantised=S.quantised())
        if kind == "r_prev":
            return dict(planes=self.planes(True), quantised=S.unq != "prev")
        if kind == "r_agents":
            idx, st = self.agents_now()
            return dict(idx=idx, st=st)
        if kind == "r_actions":
            return dict(a=self.actions)
        if kind == "r_reduce":
            return dict(stats=self.stats()[None])
        if kind == "r_reward":
            reward, done = self._rewards()
            return dict(reward=reward, done=done)
        if kind == "r_temp":
            return dict(temps=self.temp_on_demand(op["L"]))
        if kind == "r_tiles":
            c, m = self.tiles(op["L"], op["tile"], op["worlds"], op["cover"], op["temperature"])
            return dict(cover=c, tmean=m)
        if kind == "r_obs":
            return dict(obs=self.obs(op["L"]))
        if kind == "r_grid":
            return dict(grid=self.grid(op["L"]))
        if kind == "r_caches":
            return dict(caches=self.caches(op["L"]))
        if kind == "r_lifespan":
            alive = self.stats()["max_k"] > THRESHOLD_K
            self.done_at += alive
            if self.N and S.agents:
                self.agents_done_at += ~self._rewards()[1]
            return dict(done_at=self.done_at.copy(), agents_done_at=self.agents_done_at.copy() if S.agents else None,
                        n_alive=int(alive.sum()))
        return {}


def _physics_of(consts, light, dark, L):
    """The oracle's physics pass on (1, H, W) covers: the environment that holds the side-effect caches."""
    o = O.OracleDaisyWorld(grid_dimension=light.shape[-1], n_agents=0, batch_size=1)
    for n, v in consts.items():
        setattr(o.P, n, v)
    o.L = float(L)
    grid = np.zeros((1, 7) + light.shape[-2:])
    grid[:, 1], grid[:, 2] = light, dark
    o._physics(grid)
    return o


class Model(Reference):
    """The float64 reference: one OracleDaisyWorld per world (a world can have constants and a luminosity of its own)."""

    def __init__(self, H, W, B, N, precision="exact"):
        super().__init__(H, W, B, N, precision)
        self.w = [O.OracleDaisyWorld(grid_dimension=W, n_agents=N, batch_size=1) for _ in range(B)]
        for o in self.w:
            o.agent_indices = np.zeros((1, N, 2), dtype=np.int64)
            o.agent_states = np.zeros((1, N, 1))
        self.consts = dict(DEFAULT_CONSTS)
        self.prev = [None] * B                              # (light, dark) the last step read, after its grazing
        self.cache = [None] * B                             # the side-effect caches of the last step
        self.snap = [None, None]

    # -- primitives ------------------------------------------------------------------------------------------------------
    def _load(self, kind, light, dark, eng_state):
        if kind != "upload_f64":                            # float32 uploads: the doubles the library holds of them
            light, dark = eng_state["planes"]
        for b, o in enumerate(self.w):
            o.L = 1.0
            o.set_initial_cover(np.array(light[b:b + 1], dtype=np.float64), np.array(dark[b:b + 1], dtype=np.float64))
        self.prev, self.cache = [None] * self.B, [None] * self.B

    def _init_random(self, rseed, eng_state):
        self._load("init_random", None, None, eng_state)
        if self.N:
            self._set_agents(*eng_state["agents"])

    def _set_agents(self, idx, st):
        for b, o in enumerate(self.w):
            o.agent_indices = np.asarray(idx[b:b + 1], dtype=np.int64).copy()
            o.agent_states = np.asarray(st[b:b + 1], dtype=np.float64).reshape(1, self.N, 1).copy()

    def _graze(self, a):
        ab, an = a.shape
        for b, o in enumerate(self.w):
            o.update_agents(a[b:b + 1, :, None] if b < ab else np.zeros((0, an, 1), dtype=a.dtype))

    def _apply_consts(self, o, c):
        for n, v in c.items():
            setattr(o.P, n, v)

    def _install(self, tab):
        for b, o in enumerate(self.w):
            self._apply_consts(o, dict(zip(PHYS, tab[b])))

    def _uninstall(self):
        for o in self.w:
            self._apply_consts(o, self.consts)

    def _forward(self, Lv, want_temp):
        for b, o in enumerate(self.w):
            o.L = float(Lv[b])
            o.P.n_agents = self.N if self.S.agents else 0      # (no agents uploaded: nothing is stamped into the grid)
            self.prev[b] = (o.grid[:, 1].copy(), o.grid[:, 2].copy())
            o.grid = o.forward(o.grid)
            self.cache[b] = (o.temp, o.temp_light, o.temp_dark, o.beta, o.beta_l, o.beta_d, o.growth, o.temp_effective)
        return _temp_rec(np.concatenate([c[0][:, 0] for c in self.cache])) if want_temp else None

    def _set_consts(self, consts, precision):
        if consts is not None:
            self.consts = dict(consts)
            self._uninstall()

    def _save(self, s):
        self.snap[s] = copy.deepcopy(([o.grid for o in self.w], [o.agent_indices for o in self.w],
                                      [o.agent_states for o in self.w], self.prev, self.cache))

    def _restore(self, s, with_agents):
        grids, idx, st, prev, cache = copy.deepcopy(self.snap[s])
        for b, o in enumerate(self.w):
            o.grid = grids[b]
            if with_agents:
                o.agent_indices, o.agent_states = idx[b], st[b]
        self.prev, self.cache = prev, cache

    # -- views -----------------------------------------------------------------------------------------------------------
    def planes(self, previous):
        if previous:
            return np.concatenate([p[0] for p in self.prev]), np.concatenate([p[1] for p in self.prev])
        return np.concatenate([o.grid[:, 1] for o in self.w]), np.concatenate([o.grid[:, 2] for o in self.w])

    def agents_now(self):
        return (np.concatenate([o.agent_indices for o in self.w]).astype(np.int32),
                np.concatenate([o.agent_states for o in self.w])[..., 0])

    def stats(self):
        return _stats_rec(*self.planes(False))

    def obs(self, L):
        return np.concatenate([o.get_obs(o.agent_indices) for o in self.w])

    def grid(self, L):
        return np.concatenate([o.grid for o in self.w]) if self._derived_ok() else None

    def _derived_ok(self):
        """Do the oracle's grid and caches describe what the handle evaluates?  After a step with the current setting."""
        return self.S.fresh and self.S.quantised() and not self.S.lacks_L()

    def _field_env(self, L):
        """Per world, the caches the handle evaluates: the last step's, or - after a per-world-L run - the retained state
        at the caller's luminosity with the handle's constants."""
        S = self.S
        if not (S.fresh and S.stepped) or S.lacks_P():
            return None
        if not S.lacks_L():
            return self.cache
        out = []
        for b in range(self.B):
            o = _physics_of(self.consts, self.prev[b][0], self.prev[b][1], L)
            out.append((o.temp, o.temp_light, o.temp_dark, o.beta, o.beta_l, o.beta_d, o.growth, o.temp_effective))
        return out

    def temp_on_demand(self, L):
        env = self._field_env(L)
        return None if env is None else _temp_rec(np.concatenate([c[0][:, 0] for c in env]))

    def tiles(self, L, tile, sel, cover, temperature):
        c = m = None
        if cover:
            light, dark = self.planes(False)
            c = np.zeros(_tiles_of(light, tile, sel, "sum").shape, dtype=_ffi.TILE_COVER_DTYPE)
            c["sum_light_k"] = _tiles_of(k(light), tile, sel, "sum")
            c["sum_dark_k"] = _tiles_of(k(dark), tile, sel, "sum")
        if temperature:
            env = self._field_env(L)
            if env is not None:
                m = _tiles_of(np.concatenate([e[0][:, 0] for e in env]), tile, sel, "mean")
        return c, m

    def caches(self, L):
        env = self._field_env(L)
        if env is None:
            return None
        cat = lambda *i: np.concatenate([np.concatenate([e[j] for j in i], axis=1) for e in env])  # noqa: E731
        return cat(0, 1, 2), cat(3, 4, 5), cat(6), cat(7)

    def obs_comparable(self):
        return self._derived_ok()


class Twin(Reference):
    """B one-world engines of the same (H, W, N), created without fused pairs, packing and episode kernels, and driven by
    per-step primitives only: dw_step with host actions, dw_reduce, dw_reduce_temperature, dw_reduce_tiles.  World b takes
    its own luminosity column and, for the length of a per-world-constants operation, its own constants."""
    exact_floats = True

    def __init__(self, H, W, B, N, precision, amd):
        super().__init__(H, W, B, N, precision)
        self.amd = amd
        saved = {v: os.environ.pop(v, None) for v in SWITCHES}
        os.environ.update(TWIN_SWITCHES)
        try:
            self.e = []
            for b in range(B):
                p = amd.default_params(1, H, W, N)
                p.precision = _ffi.PRECISION[precision]
                p.world_offset = b
                self.e.append(amd.Engine(p))
        finally:
            for v in TWIN_SWITCHES:
                os.environ.pop(v, None)
            os.environ.update({v: x for v, x in saved.items() if x is not None})
        self.consts = dict(DEFAULT_CONSTS)

    def close(self):
        for e in self.e:
            e.close()

    def _params(self, e, consts, precision):
        p = _ffi.DwParams.from_buffer_copy(e.params)
        for n, v in consts.items():
            setattr(p, n, v)
        p.precision = _ffi.PRECISION[precision]
        return p

    def _load(self, kind, light, dark, eng_state):
        for b, e in enumerate(self.e):
            if kind == "upload_f64":
                e.upload_state(light[b:b + 1], dark[b:b + 1])
            else:
                e.upload_state_f32(light[b:b + 1], dark[b:b + 1], quantised=kind == "upload_f32q")

    def _init_random(self, rseed, eng_state):
        for e in self.e:
            e.init_random(rseed)

    def _set_agents(self, idx, st):
        for b, e in enumerate(self.e):
            e.upload_agents(idx[b:b + 1], st[b:b + 1])

    def _graze(self, a):
        ab, an = a.shape
        self._pending = [a[b:b + 1] if b < ab else np.zeros((0, an), np.int32) for b in range(self.B)]

    def _forward(self, Lv, want_temp):
        pending, self._pending = getattr(self, "_pending", None), None
        rec = np.zeros(self.B, dtype=_ffi.TEMP_STATS_DTYPE)
        for b, e in enumerate(self.e):
            e.step(float(Lv[b]), None if pending is None else pending[b])
            if want_temp:
                rec[b] = e.reduce_temperature(float(Lv[b]))[0]
        return rec if want_temp else None

    def apply(self, op, eng_state=None):
        if op["kind"] == "update_agents":                   # grazing alone
            ab, an = op["a"].shape
            for b, e in enumerate(self.e):
                e.update_agents(op["a"][b:b + 1] if b < ab else np.zeros((0, an), np.int32))
            self.S.stats_ok = self.S.fresh = False
            return {}
        return super().apply(op, eng_state)

    def _install(self, tab):
        for b, e in enumerate(self.e):
            e.set_params(self._params(e, dict(zip(PHYS, tab[b])), self.S.precision))

    def _uninstall(self):
        for e in self.e:
            e.set_params(self._params(e, self.consts, self.S.precision))

    def _set_consts(self, consts, precision):
        if consts is not None:
            self.consts = dict(consts)
        self._uninstall()

    def _save(self, s):
        for e in self.e:
            e.snapshot_save(s)

    def _restore(self, s, with_agents):
        for e in self.e:
            e.snapshot_restore(s)

    def planes(self, previous):
        got = [e.download_planes(_ffi.STATE_PREVIOUS if previous else _ffi.STATE_CURRENT) for e in self.e]
        return np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])

    def agents_now(self):
        got = [e.download_agents() for e in self.e]
        return np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])

    def stats(self):
        return np.concatenate([e.reduce() for e in self.e])

    def obs(self, L):
        return np.concatenate([e.get_obs(L) for e in self.e])

    def _shared(self):
        """The one-world engines evaluate with their own last luminosity: comparable while the handle has a shared one."""
        return not self.S.lacks_L()

    def grid(self, L):
        return np.concatenate([e.download_grid(L) for e in self.e]) if self._shared() else None

    def temp_on_demand(self, L):
        return np.concatenate([e.reduce_temperature(L) for e in self.e]) if self._shared() else None

    def tiles(self, L, tile, sel, cover, temperature):
        worlds = range(self.B) if sel is None else [int(b) for b in sel]
        temperature = temperature and self._shared()
        got = [self.e[b].reduce_tiles(L, tile, None, cover, temperature) for b in worlds] if cover or temperature else []
        return (np.concatenate([g[0] for g in got]) if cover else None,
                np.concatenate([g[1] for g in got]) if temperature else None)

    def caches(self, L):
        if not self._shared():
            return None
        got = [e.download_caches(L) for e in self.e]
        return tuple(np.concatenate([g[i] for g in got]) for i in range(4))

    def obs_comparable(self):
        return True


# ======================================================================================================================
# comparing
# ======================================================================================================================
def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _stats_equal(a, b):
    return all(np.array_equal(a[f], b[f]) for f in ("max_k", "sum_light_k", "sum_dark_k"))


def _temps_close(rec, ref):
    """tests/test_gpu_temperature.py::_assert_close_to_oracle."""
    ok = np.allclose(rec["mean"], ref["mean"], rtol=2e-12, atol=0) and np.allclose(rec["min"], ref["min"], rtol=1e-12, atol=0)
    ok = ok and np.allclose(rec["max"], ref["max"], rtol=1e-12, atol=0)
    return bool(ok and (np.abs(rec["std"] - ref["std"]) <= 2e-12 * ref["max"]).all())


def _caches_close(got, ref):
    """tests/test_gpu_parity.py::test_forward_matches_reference_fixture_g1."""
    t, b, g, e = got
    rt, rb, rg, re_ = ref
    return bool(np.allclose(t, rt, rtol=1e-12, atol=0) and np.allclose(e, re_, rtol=1e-12, atol=0)
                and np.allclose(b, rb, rtol=1e-9, atol=1e-12) and np.allclose(g, rg, rtol=1e-9, atol=1e-14))


def differences(got, exp, exact_floats, obs_ok=True):
    """Names of the entries of `exp` (None: not comparable) that `got` does not match."""
    bad = []
    for key, ref in exp.items():
        if ref is None or key == "quantised":
            continue
        g = got[key]
        if key == "planes":
            same = all(np.array_equal(k(x), k(y)) if exp["quantised"] else np.array_equal(x, y) for x, y in zip(g, ref))
        elif key == "stats":
            same = _stats_equal(g, ref)
        elif key == "stats0":
            same = _stats_equal(g, ref) and not g["reserved"].any()
        elif key == "temps":
            same = _bits(g) == _bits(ref) if exact_floats else _temps_close(g, ref)
        elif key == "tmean":
            same = _bits(g) == _bits(ref) if exact_floats else bool(np.allclose(g, ref, rtol=2e-12, atol=0))
        elif key == "caches":
            same = all(_bits(x) == _bits(y) for x, y in zip(g, ref)) if exact_floats else _caches_close(g, ref)
        elif key == "cover":
            same = np.array_equal(g["sum_light_k"], ref["sum_light_k"]) and np.array_equal(g["sum_dark_k"], ref["sum_dark_k"])
        elif key in ("obs", "grid"):
            same = not obs_ok or np.array_equal(g, ref)
        elif key in ("L", "n_alive"):
            same = g == ref
        else:
            same = np.array_equal(g, ref)
        if not same:
            bad.append(key)
    return bad


# ======================================================================================================================
# executing a plan
# ======================================================================================================================
POLICY = {"greedy": _ffi.POLICY_ARGMAX, "anti": _ffi.POLICY_ARGMIN, "table": _ffi.POLICY_TABLE}


def _dw_params(eng, consts, precision):
    p = _ffi.DwParams.from_buffer_copy(eng.params)
    for n, v in consts.items():
        setattr(p, n, v)
    p.precision = _ffi.PRECISION[precision]
    return p


def execute(eng, op, consts):
    """The Engine call(s) of one planned operation; what they return, under the keys the references use."""
    kind = op["kind"]
    if kind == "upload_f64":
        eng.upload_state(op["light"], op["dark"])
    elif kind in ("upload_f32", "upload_f32q"):
        eng.upload_state_f32(op["light"], op["dark"], quantised=kind == "upload_f32q")
    elif kind == "init_random":
        eng.init_random(op["rseed"])
    elif kind == "upload_agents":
        eng.upload_agents(op["idx"], op["st"])
    elif kind == "upload_actions":
        eng.upload_actions(op["a"])
    elif kind in ("step", "step_act", "step_sub"):
        eng.step(op["L"], op.get("a"))
    elif kind == "env_step":
        obs, reward, done = eng.env_step(op["L"], op.get("a"))
        return dict(obs=obs, reward=reward, done=done)
    elif kind == "greedy_step":
        eng.policy_greedy(argmin=op["argmin"])
        eng.step_device_actions(op["L"])
    elif kind == "per_agent_step":
        eng.upload_actions(op["a"])
        eng.policy_per_agent(op["modes"])
        eng.step_device_actions(op["L"])
    elif kind == "mlp_step":
        eng.policy_mlp(op["params"][0], 0, op["split"])
        eng.policy_mlp(op["params"][1], op["split"], eng.N)
        eng.step_device_actions(op["L"])
    elif kind == "mlp_pop_step":
        eng.policy_mlp_population(op["params"], op["member"])
        eng.step_device_actions(op["L"])
    elif kind == "update_agents":
        eng.update_agents(op["a"])
    elif kind in ("step_n", "step_n_dev"):
        if kind == "step_n_dev":
            eng.upload_actions(op["a"])
        return dict(L=eng.step_n(op["n"], op["L"], op["dL"], op["lo"], op["hi"], use_device_actions=kind == "step_n_dev"))
    elif kind == "trace":
        return dict(stats=eng.step_n_trace(op["Ls"]))
    elif kind == "trace_pw":
        return dict(stats=eng.step_n_trace_per_world(op["Ls"]))
    elif kind in ("trace_temp", "trace_temp_pw"):
        stats, temps = eng.step_n_trace_temperature(op["Ls"])
        return dict(stats=stats, temps=temps)
    elif kind == "trace_ens":
        return dict(stats=eng.step_n_trace_ensemble(op["tab"], op["Ls"]))
    elif kind == "trace_ens_temp":
        stats, temps = eng.step_n_trace_ensemble(op["tab"], op["Ls"], temperature=True)
        return dict(stats=stats, temps=temps)
    elif kind == "frames":
        cover, tmean, stats = eng.step_n_frames(op["Ls"], op["stride"], op["tile"], op["worlds"], op["cover"], op["temperature"])
        return dict(cover=cover, tmean=tmean, stats=stats)
    elif kind in ("ep_greedy", "ep_anti", "ep_table"):
        alive, ok = eng.run_episode(op["Ls"], POLICY[op["mode"]], op["use_table"], op["table"], THRESHOLD_K, op["world_flags"])
        return dict(alive=alive, ok=ok)
    elif kind in ("ep_trace", "ep_trace_temp"):
        out = eng.run_episode_trace(op["Ls"], POLICY[op["mode"]], op["use_table"], op["table"], THRESHOLD_K,
                                    temperature=kind == "ep_trace_temp")
        return dict(stats0=out[0], alive=out[1], ok=out[2], temps=out[3] if len(out) > 3 else None)
    elif kind in ("ep_ens", "ep_ens_trace", "ep_ens_trace_temp"):
        out = eng.run_episode_ensemble(op["tab"], op["Ls"], POLICY[op["mode"]], op["use_table"], op["table"], THRESHOLD_K,
                                       trace=kind != "ep_ens", temperature=kind == "ep_ens_trace_temp")
        return dict(alive=out[0], ok=out[1], stats0=out[2] if len(out) > 2 else None, temps=out[3] if len(out) > 2 else None)
    elif kind in ("ep_mlp", "ep_mlp_resident", "ep_mlp_trace", "x_ep_mlp"):
        out = eng.run_episode_mlp(op["Ls"], op["params"], op.get("member_a"), op.get("member_b"), op["split"],
                                  n_members=op["n_members"], trace=bool(op.get("trace")), temperature=bool(op.get("temperature")))
        return dict(reward=out[0], done=out[1], stats0=out[2] if len(out) > 2 else None, temps=out[3] if len(out) > 2 else None)
    elif kind in ("save0", "save1"):
        eng.snapshot_save(int(kind[-1]))
    elif kind in ("restore0", "restore1"):
        eng.snapshot_restore(int(kind[-1]))
    elif kind == "set_params":
        eng.set_params(_dw_params(eng, const_set(op["set"]), op["precision"]))
    elif kind == "set_precision":
        eng.set_params(_dw_params(eng, consts, op["to"]))
    # ---- reads ----
    elif kind == "r_planes":
        return dict(planes=eng.download_planes())
    elif kind == "r_prev":
        return dict(planes=eng.download_planes(_ffi.STATE_PREVIOUS))
    elif kind == "r_agents":
        idx, st = eng.download_agents()
        return dict(idx=idx, st=st)
    elif kind == "r_actions":
        return dict(a=eng.download_actions())
    elif kind == "r_reduce":
        return dict(stats=eng.reduce()[None])
    elif kind == "r_reward":
        reward, done = eng.reward_done()
        return dict(reward=reward, done=done)
    elif kind in ("r_temp", "x_temp"):
        return dict(temps=eng.reduce_temperature(op["L"]))
    elif kind in ("r_tiles", "x_tiles"):
        cover, tmean = eng.reduce_tiles(op["L"], op["tile"], op["worlds"], op["cover"], op["temperature"])
        return dict(cover=cover, tmean=tmean)
    elif kind in ("r_obs", "x_obs"):
        return dict(obs=eng.get_obs(op["L"]))
    elif kind in ("r_grid", "x_grid"):
        return dict(grid=eng.download_grid(op["L"]))
    elif kind in ("r_caches", "x_caches"):
        return dict(caches=eng.download_caches(op["L"]))
    elif kind == "r_lifespan":
        eng.lifespan_accumulate(THRESHOLD_K)
        done_at, agents_done_at, n_alive = eng.lifespan_download()
        return dict(done_at=done_at, agents_done_at=agents_done_at, n_alive=n_alive)
    elif kind == "r_forward":
        return dict(forward=eng.forward(op["light"], op["dark"], op["L"], want_caches=True))
    elif kind == "r_conv":
        return dict(conv=eng.conv3x3(op["light"], op["kernel"]))
    elif kind == "r_stage":
        return dict(stage=eng.stage(_ffi.STAGE_DENSITY, [op["light"], op["dark"]], kernel=O.daisy_kernel()))
    return {}


def stateless_differences(op, got, consts):
    """dw_forward_f64, dw_conv3x3_f64 and dw_stage_f64 on the caller's data, against the oracle's functions."""
    kind, bad = op["kind"], []
    if kind == "r_forward":
        grid, t, b, g, e = got["forward"]
        for w in range(grid.shape[0]):
            o = _physics_of(consts, op["light"][w:w + 1], op["dark"][w:w + 1], op["L"])
            new = np.round(np.clip(np.stack([op["light"][w], op["dark"][w]])[None] + o.P.dt * o.growth, 0, 1), 3)
            if not np.array_equal(k(grid[w, 1:3]), k(new[0])) or not np.array_equal(grid[w, 3], np.round(o.temp[0, 0], 3)):
                bad.append("forward grid")
            ref = (np.concatenate([o.temp, o.temp_light, o.temp_dark], axis=1), np.concatenate([o.beta, o.beta_l, o.beta_d], axis=1),
                   o.growth, o.temp_effective)
            if not _caches_close((t[w:w + 1], b[w:w + 1], g[w:w + 1], e[w:w + 1]), ref):
                bad.append("forward caches")
    elif kind == "r_conv":
        if not np.allclose(got["conv"], O.toroidal_conv3x3(op["light"], op["kernel"]), rtol=1e-12, atol=1e-15):
            bad.append("conv3x3")
    elif kind == "r_stage":
        ref = O.calculate_daisy_density(_DEFAULT, np.stack([op["light"], op["dark"]], axis=1))
        if not np.allclose(np.stack(got["stage"], axis=1), ref, rtol=1e-12, atol=1e-15):
            bad.append("stage")
    return sorted(set(bad))


def _identities(eng, op, got):
    """The documented byte identities between the calls of ONE handle."""
    kind, bad = op["kind"], []
    rows = got.get("stats0") if got.get("stats0") is not None else (got.get("stats") if kind != "r_reduce" else None)
    if rows is not None and len(rows) and not _stats_equal(rows[-1], eng.reduce()):
        bad.append("last record != dw_reduce")
    shared_temps = kind in ("trace_temp", "ep_trace_temp", "ep_mlp_trace", "ep_mlp", "ep_mlp_resident")
    if shared_temps and got.get("temps") is not None and np.ndim(op["Ls"]) == 1:
        if _bits(got["temps"][-1]) != _bits(eng.reduce_temperature(float(op["Ls"][-1]))):
            bad.append("last temperature row != dw_reduce_temperature")
    if kind == "r_tiles" and tuple(op["tile"]) == (1, 1):
        sel = slice(None) if op["worlds"] is None else np.asarray(op["worlds"])
        if op["cover"]:
            light, dark = eng.download_planes()
            if not (np.array_equal(got["cover"]["sum_light_k"], k(light)[sel]) and np.array_equal(got["cover"]["sum_dark_k"], k(dark)[sel])):
                bad.append("1x1 cover != planes")
        if op["temperature"] and _bits(got["tmean"]) != _bits(eng.download_caches(op["L"], betas=False, growth=False,
                                                                                    temp_effective=False)[0][:, 0][sel]):
            bad.append("1x1 temperature != caches")
    return bad


def synthetic_state(plan, op):
    """What stands in for the engine's downloads where no engine runs (the CPU tests of the Model's bookkeeping): the
    doubles of a float32 upload, a drawn state for dw_init_random."""
    B, H, W, N = plan["B"], plan["H"], plan["W"], plan["N"]
    if op["kind"] == "init_random":
        r = np.random.RandomState(op["rseed"] % (2 ** 32))
        planes = tuple((r.rand(B, H, W) * 0.2 * (r.rand(B, H, W) < 0.33)).astype(np.float32).astype(np.float64) for _ in range(2))
        idx = np.stack([r.randint(H, size=(B, N)), r.randint(W, size=(B, N))], axis=-1).astype(np.int32)
        return dict(planes=planes, agents=(idx, np.ones((B, N))))
    if op["kind"] in ("upload_f32", "upload_f32q"):
        return dict(planes=(op["light"].astype(np.float64), op["dark"].astype(np.float64)), agents=None)
    return None


def dry_run(plan, on_op=None):
    """The Model alone through a plan: returns it, after checking after every operation that it is in the class the plan
    predicted.  on_op(model, op, expected) sees every operation's result."""
    m = Model(plan["H"], plan["W"], plan["B"], plan["N"], plan["precision"])
    for op in plan["ops"]:
        if op["kind"] in REFUSALS:
            continue
        exp = m.apply(op, synthetic_state(plan, op))
        assert m.S.cls() == op["post"], (plan["seed"], describe(op), m.S.cls(), op["post"])
        assert m.S.fresh == op["post_fresh"], (plan["seed"], describe(op))
        if on_op:
            on_op(m, op, exp)
    return m


def explicit_plan(H, W, B, N, precision, ops, twin=False, env=None, seed=-1):
    """A plan from a hand-written list of operations (dicts of `kind` and its arguments, as plan_case draws them): the
    classes before and after each are filled in from the Model's own bookkeeping.  For pinned regression sequences."""
    plan = dict(seed=seed, H=H, W=W, B=B, N=N, precision=precision, twin=twin, env=dict(env or {}), ops=[dict(o) for o in ops])
    m, consts = Model(H, W, B, N, precision), "default"
    for op in plan["ops"]:
        op.update(cls=m.S.cls(), precision=m.S.precision, fresh_before=m.S.fresh)
        assert m.S.admits(op["kind"]), (describe(op), m.S.cls())
        if op["kind"] not in REFUSALS:
            m.apply(op, synthetic_state(plan, op))
        consts = op.get("set", consts)
        op.update(post=m.S.cls(), post_fresh=m.S.fresh, consts=consts)
    return plan


def _run_plan(plan, log, amd):
    seed, H, W, B, N = plan["seed"], plan["H"], plan["W"], plan["B"], plan["N"]
    p = amd.default_params(B, H, W, N)
    p.precision = _ffi.PRECISION[plan["precision"]]
    eng = amd.Engine(p)
    eng.lifespan_reset()
    refs = []
    if plan["precision"] != "fast":
        refs.append(Model(H, W, B, N, plan["precision"]))
    if plan["twin"]:
        refs.append(Twin(H, W, B, N, plan["precision"], amd))
    consts = dict(DEFAULT_CONSTS)
    done, ok = [], True

    def fail(what):
        nonlocal ok
        ok = False
        log.append(f"seed {seed} ({H}x{W} B={B} N={N} {plan['precision']}{' +twin' if plan['twin'] else ''} {plan['env']}): "
                   f"{what} after [{' > '.join(done[-6:])}]")

    for i, op in enumerate(plan["ops"]):
        kind = op["kind"]
        done.append(describe(op))
        if kind in REFUSALS:
            try:
                execute(eng, op, consts)
                fail(f"{kind} was not refused")
            except amd.DaisyHipError as e:
                if e.code == _ffi.DW_EHIP:                      # a failed HIP call: nothing more is started on this device
                    raise
                if e.code != _ffi.DW_ESTATE:
                    fail(f"{kind} refused with {e.code}, not DW_ESTATE")
            checks = [dict(kind=kd) for kd in ("r_planes", "r_agents", "r_reduce") if refs[0].S.admits(kd)]
        else:
            try:
                got = execute(eng, op, consts)
            except amd.DaisyHipError as e:
                if e.code == _ffi.DW_EHIP:
                    raise
                fail(f"{kind} raised {e}")
                break
            checks = []
            eng_state = None
            if kind in ("upload_f32", "upload_f32q", "init_random"):
                eng_state = dict(planes=eng.download_planes(),
                                 agents=eng.download_agents() if N and kind == "init_random" else None)
            if kind == "set_params":
                consts = const_set(op["set"])
            for ref in refs:
                exp = ref.apply(op, eng_state)
                if ref.S.cls() != op["post"]:
                    fail(f"{type(ref).__name__} is in class {ref.S.cls()}, the plan predicted {op['post']}")
                bad = differences(got, exp, ref.exact_floats, ref.obs_comparable())
                if bad:
                    fail(f"{kind} against {type(ref).__name__}: {bad}")
            bad = stateless_differences(op, got, consts) + _identities(eng, op, got)
            if bad:
                fail(f"{kind}: {bad}")
        for chk in checks:                                      # after a refusal: nothing has moved
            got = execute(eng, chk, consts)
            for ref in refs:
                bad = differences(got, ref.read(chk), ref.exact_floats)
                if bad:
                    fail(f"{chk['kind']} after the refused {kind} against {type(ref).__name__}: {bad}")
        if not ok:
            break
    info = (f"{H}x{W} B={B} N={N} {plan['precision']}{'+twin' if plan['twin'] else ''} ops={len(plan['ops'])} "
            f"changing={sum(o['kind'] in CHANGING for o in plan['ops'])} {plan['env']} :: {eng.kernel_info()[:40]}")
    if not ok:
        log.append(f"seed {seed} operations: " + " | ".join(f"{j}:{describe(o)}" for j, o in enumerate(plan["ops"][:len(done)])))
        log.append(f"seed {seed} kernel_info: {eng.kernel_info()}")
    for ref in refs:
        if isinstance(ref, Twin):
            ref.close()
    eng.close()
    return ok, info


def run_case(seed, log, plan=None):
    """Execute plan_case(seed) (or `plan`) on an Engine created under the plan's switches; compare after every operation."""
    import therldaisyworld_amd as amd
    plan = plan or plan_case(seed)
    saved = {v: os.environ.pop(v, None) for v in SWITCHES}
    os.environ.update(plan["env"])                              # (read by the library whenever a handle is created)
    try:
        return _run_plan(plan, log, amd)
    finally:
        for v in SWITCHES:
            os.environ.pop(v, None)
        os.environ.update({v: x for v, x in saved.items() if x is not None})


if __name__ == "__main__":
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    log, nbad = [], 0
    for i in range(cases):
        ok, info = run_case(seed * 10000 + i, log)
        nbad += not ok
        print("ok  " if ok else "FAIL", seed * 10000 + i, info, flush=True)
    for line in log:
        print(line)
    print(f"{cases - nbad}/{cases} cases identical")
    sys.exit(1 if nbad else 0)
