"""Event-based controller (fleet_event_based.py) on the GPU.

Every agent i holds a local MPC over the vehicles ``[i-1, i, i+1]`` clipped to the platoon
(:class:`LocalMpc` / :class:`LocalMpcGear`, fleet_event_based.py:26-376) with the trajectories of
the vehicles two places away as fixed data.  Per step, at most ``event_iters`` times: every agent
prices the current guesses (``eval_cost``) and solves its local problem; the agent with the largest
cost decrease above ``threshold`` overwrites the guesses of its local vehicles
(:class:`TrackingEventBasedCoordinator`, :413-646).

* :class:`EventSolver` owns one ``HVP_FORM_CENT`` handle and wraps the entry points of
  include/hvp_event.h: ``solve`` / ``evaluate`` (numpy) and the ``*_device`` forms of the batched
  closed loop (``hvp.sweep.run_point(controller="event")``).
* :func:`local_layout`, :func:`select_winner`, :func:`shift_guesses`, :func:`initial_guesses`:
  the coordinator's rules in plain numpy (what ``hvp_event_layout`` / ``_select`` / ``_shift``
  do on the device).
* The coordinator is a host drop-in for one platoon: per iteration one ``hvp_event_evaluate_batch``
  and one ``hvp_event_solve_batch`` over all n agents.
"""

from __future__ import annotations

import ctypes
import pickle
import time
from dataclasses import dataclass

import numpy as np

from . import _abi, tables
from .agent import MldAgent
from .batched import extrapolate
from .cent import DROPIN_MAX_NODES, cent_problem
from .env import EpisodeMonitor, PlatoonEnv
from .models import Platoon, Vehicle
from .params import ConstantSpacingPolicy, Params, Sim, SpacingPolicy

threshold = 10  # cost improvement must be more than this to consider communication (:23)
MAX_M = 3


# ---------------------------------------------------------------------- the rules in numpy
def local_layout(n: int, leader_index: int = 0) -> list[dict]:
    """Per agent of an n-vehicle platoon (fleet_event_based.py:700-723): ``lo`` (first local
    vehicle), ``m``, ``num_vehicles_in_front`` / ``_behind`` (0..2), ``rel_leader_index``
    (-1, 0, 1 or None) and ``leader`` (its local index, -1 for none)."""
    if n < 2:
        raise ValueError("the event-based controller needs n >= 2 vehicles")
    if not 0 <= leader_index < n:
        raise ValueError(f"leader_index {leader_index} outside 0..{n - 1}")
    out = []
    for i in range(n):
        lo, hi = max(i - 1, 0), min(i + 1, n - 1)
        rel = {leader_index - 1: -1, leader_index: 0, leader_index + 1: 1}.get(i)
        out.append({"lo": lo, "m": hi - lo + 1, "num_vehicles_in_front": min(i, 2),
                    "num_vehicles_behind": min(n - 1 - i, 2), "rel_leader_index": rel,
                    "leader": -1 if rel is None else leader_index - lo})
    return out


def select_winner(eval_costs, new_costs, threshold: float = threshold) -> int:
    """The winner of one iteration (:517-524): the first agent with the largest decrease
    ``eval - new`` that strictly exceeds ``threshold``; -1 when there is none.  ``inf`` marks an
    infeasible evaluation or solve.  No feasible solve at all raises RuntimeWarning."""
    ev = np.asarray(eval_costs, dtype=np.float64)
    nw = np.asarray(new_costs, dtype=np.float64)
    if not np.any(nw < np.inf):
        raise RuntimeWarning("No feasible solution found for any event based agent.")
    best, idx = -np.inf, -1
    with np.errstate(invalid="ignore"):
        dec = ev - nw  # inf - inf: NaN, which fails both comparisons as in the reference
    for i, d in enumerate(dec):
        if d > best and d > threshold:
            best, idx = d, i
    return idx


def shift_guesses(a: np.ndarray) -> np.ndarray:
    """on_timestep_end (:589-603): one sample on along the last axis, the last column repeated."""
    a = np.asarray(a)
    return np.concatenate((a[..., 1:], a[..., -1:]), axis=-1)


def initial_guesses(x, vehicles, N: int, ts: float, discrete_gears: bool):
    """on_episode_start (:620-635) for the platoon state x (2n,): constant-velocity states
    (n, 2, N+1), the inputs that hold each velocity (n, N) and the gears (n, N; zero without
    discrete gears)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = len(vehicles)
    xs = np.stack([extrapolate(x[2 * i], x[2 * i + 1], N, ts) for i in range(n)])
    us, gs = np.zeros((n, N)), np.zeros((n, N))
    for i, veh in enumerate(vehicles):
        v = float(x[2 * i + 1])
        if discrete_gears:
            j = veh.get_gear_from_velocity(v)
            gs[i] = j
            us[i] = veh.get_u_for_constant_vel(v, j)
        else:
            us[i] = veh.get_u_for_constant_vel(v)
    return xs, us, gs


def make_desc(items) -> ctypes.Array:
    """A host array of hvp_event_desc from (m, has_f2, has_b2, leader) tuples."""
    arr = (_abi.HvpEventDesc * max(1, len(items)))()
    for k, (m, f2, b2, lead) in enumerate(items):
        arr[k] = _abi.HvpEventDesc(int(m), int(bool(f2)), int(bool(b2)), int(lead))
    return arr


def platoon_desc(n: int, leader_index: int, P: int = 1) -> ctypes.Array:
    """The P n descriptors (instance b = p n + i) of P platoons, through hvp_event_layout."""
    one = (_abi.HvpEventDesc * n)()
    _abi.check(_abi.load().hvp_event_layout(n, leader_index, one), "hvp_event_layout")
    arr = (_abi.HvpEventDesc * (P * n))()
    for b in range(P * n):
        arr[b] = one[b % n]
    return arr


# ---------------------------------------------------------------------- the handle
@dataclass
class EventResult:
    u: np.ndarray       # (B, 3, N)
    x: np.ndarray       # (B, 3, 2, N+1)
    region: np.ndarray  # (B, 3, N)  -1 without a solution and for unused vehicle slots
    gear: np.ndarray    # (B, 3, N)
    cost: np.ndarray    # (B,)  inf when status != OPTIMAL
    status: np.ndarray  # (B,)
    nodes: np.ndarray   # (B,)
    iters: np.ndarray   # (B,)


class EventSolver:
    """One HVP_FORM_CENT handle for the local problems of the event-based controller."""

    def __init__(self, problem: _abi.HvpProblem, systems: list[_abi.HvpSystem], device: int = 0) -> None:
        self._lib = _abi.load()
        _abi.check(self._lib.hvp_event_validate(ctypes.byref(problem), 0, None), "hvp_event_validate")
        self.N = int(problem.N)
        self.problem = problem
        self.n_systems = len(systems)
        self.stride = _abi.event_params_stride(self.N)
        arr = (_abi.HvpSystem * len(systems))(*systems)
        h = ctypes.c_void_p()
        _abi.check(self._lib.hvp_create(ctypes.byref(h), ctypes.byref(problem), arr, len(systems), device), "hvp_create")
        self._h = h
        self.device = device

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.hvp_destroy(self._h)
            self._h = None

    def __del__(self) -> None:  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ device forms
    @staticmethod
    def _ptr(t):
        return ctypes.c_void_p(t.data_ptr() if t is not None else 0)

    def _stream(self, stream, dev):
        import torch

        return ctypes.c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)

    def alloc_outputs(self, B: int, device=None) -> dict:
        import torch

        dev = device or torch.device("cuda", self.device)
        N = self.N
        return {"u": torch.empty((B, MAX_M, N), dtype=torch.float64, device=dev),
                "x": torch.empty((B, MAX_M, 2, N + 1), dtype=torch.float64, device=dev),
                "region": torch.empty((B, MAX_M, N), dtype=torch.int8, device=dev),
                "gear": torch.empty((B, MAX_M, N), dtype=torch.int8, device=dev),
                "cost": torch.empty((B,), dtype=torch.float64, device=dev),
                "status": torch.empty((B,), dtype=torch.int32, device=dev),
                "nodes": torch.empty((B,), dtype=torch.int32, device=dev),
                "iters": torch.empty((B,), dtype=torch.int32, device=dev)}

    def _check(self, B, **tensors):
        import torch

        for name, (t, dt, shape) in tensors.items():
            if t is None:
                continue
            if not t.is_cuda or t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != shape:
                raise ValueError(f"{name} must be a contiguous CUDA {shape} tensor of dtype {dt}")
        del torch

    def solve_device(self, desc, sys_idx, params, max_nodes: int = 0, out: dict | None = None, stream=None) -> dict:
        """desc: host hvp_event_desc array (make_desc / platoon_desc); sys_idx (B, 3) int32,
        params (B, stride) float64 CUDA tensors.  Asynchronous on ``stream``."""
        import torch

        B = int(sys_idx.shape[0])
        self._check(B, sys_idx=(sys_idx, torch.int32, (B, MAX_M)), params=(params, torch.float64, (B, self.stride)))
        out = out or self.alloc_outputs(B, params.device)
        p = self._ptr
        rc = self._lib.hvp_event_solve_batch(self._h, B, desc, p(sys_idx), p(params), int(max_nodes), p(out["u"]),
                                             p(out["x"]), p(out["region"]), p(out["gear"]), p(out["cost"]),
                                             p(out["status"]), p(out["nodes"]), p(out["iters"]),
                                             self._stream(stream, params.device))
        _abi.check(rc, "hvp_event_solve_batch")
        return out

    def evaluate_device(self, desc, sys_idx, params, x_guess, u_guess, gear_guess=None, out: dict | None = None,
                        stream=None) -> dict:
        import torch

        B, N = int(sys_idx.shape[0]), self.N
        self._check(B, sys_idx=(sys_idx, torch.int32, (B, MAX_M)), params=(params, torch.float64, (B, self.stride)),
                    x_guess=(x_guess, torch.float64, (B, MAX_M, 2, N + 1)), u_guess=(u_guess, torch.float64, (B, MAX_M, N)),
                    gear_guess=(gear_guess, torch.int8, (B, MAX_M, N)))
        if out is None:
            out = {"cost": torch.empty(B, dtype=torch.float64, device=params.device),
                   "status": torch.empty(B, dtype=torch.int32, device=params.device)}
        p = self._ptr
        rc = self._lib.hvp_event_evaluate_batch(self._h, B, desc, p(sys_idx), p(params), p(x_guess), p(u_guess),
                                                p(gear_guess), p(out["cost"]), p(out["status"]),
                                                self._stream(stream, params.device))
        _abi.check(rc, "hvp_event_evaluate_batch")
        return out

    def gather_device(self, n: int, leader_index: int, x, vsys, xg, ug, gg, leader_x, sys_idx, params, x_guess, u_guess,
                      gear_guess=None, stream=None) -> None:
        P = int(x.shape[0])
        p = self._ptr
        rc = self._lib.hvp_event_gather(self._h, P, n, int(leader_index), p(x), p(vsys), p(xg), p(ug), p(gg), p(leader_x),
                                        p(sys_idx), p(params), p(x_guess), p(u_guess), p(gear_guess),
                                        self._stream(stream, x.device))
        _abi.check(rc, "hvp_event_gather")

    def select_device(self, n: int, ev: dict, sol: dict, xg, ug, gg, active, winner=None, threshold: float = threshold,
                      stream=None) -> None:
        P = int(active.shape[0])
        p = self._ptr
        rc = self._lib.hvp_event_select(self._h, P, n, float(threshold), p(ev["cost"]), p(ev["status"]), p(sol["cost"]),
                                        p(sol["status"]), p(sol["x"]), p(sol["u"]), p(sol["gear"] if gg is not None else None),
                                        p(xg), p(ug), p(gg), p(active), p(winner), self._stream(stream, active.device))
        _abi.check(rc, "hvp_event_select")

    def shift_device(self, n: int, xg, ug, gg=None, x=None, vsys=None, init: bool = False, stream=None) -> None:
        P = int(xg.shape[1])
        p = self._ptr
        rc = self._lib.hvp_event_shift(self._h, P, n, 1 if init else 0, p(x), p(vsys), p(xg), p(ug), p(gg),
                                       self._stream(stream, xg.device))
        _abi.check(rc, "hvp_event_shift")

    # ------------------------------------------------------------ host-array forms (synchronous)
    def _to(self, a, dtype):
        import torch

        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(torch.device("cuda", self.device))

    def solve(self, desc_items, sys_idx, params, max_nodes: int = 0) -> EventResult:
        """desc_items: (m, has_f2, has_b2, leader) per instance; sys_idx (B, 3); params (B, stride)."""
        import torch

        B = len(desc_items)
        out = self.solve_device(make_desc(desc_items), self._to(np.reshape(sys_idx, (B, MAX_M)), np.int32),
                                self._to(np.reshape(params, (B, self.stride)), np.float64), max_nodes)
        torch.cuda.synchronize(torch.device("cuda", self.device))
        h = {k: v.cpu().numpy() for k, v in out.items()}
        h["cost"] = np.where(h["status"] == _abi.OPTIMAL, h["cost"], np.inf)
        return EventResult(**h)

    def evaluate(self, desc_items, sys_idx, params, x_guess, u_guess, gear_guess=None):
        """(cost (B,) with inf for an infeasible guess, status (B,))."""
        import torch

        B, N = len(desc_items), self.N
        gg = None if gear_guess is None else self._to(np.reshape(gear_guess, (B, MAX_M, N)), np.int8)
        out = self.evaluate_device(make_desc(desc_items), self._to(np.reshape(sys_idx, (B, MAX_M)), np.int32),
                                   self._to(np.reshape(params, (B, self.stride)), np.float64),
                                   self._to(np.reshape(x_guess, (B, MAX_M, 2, N + 1)), np.float64),
                                   self._to(np.reshape(u_guess, (B, MAX_M, N)), np.float64), gg)
        torch.cuda.synchronize(torch.device("cuda", self.device))
        status = out["status"].cpu().numpy()
        return np.where(status == _abi.OPTIMAL, out["cost"].cpu().numpy(), np.inf), status


def pack_params(N: int, x0, x_f2=None, x_b2=None, leader_x=None) -> np.ndarray:
    """One instance's parameter block: x0 (m, 2) padded to 3 vehicles | x_f2 | x_b2 | leader_x."""
    K = 2 * (N + 1)
    out = np.zeros(_abi.event_params_stride(N))
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1)
    out[:len(x0)] = x0
    for k, blk in enumerate((x_f2, x_b2, leader_x)):
        if blk is not None:
            out[6 + k * K:6 + (k + 1) * K] = np.asarray(blk, dtype=np.float64).reshape(K)
    return out


def _pad(a: np.ndarray, m: int) -> np.ndarray:
    """(m, ...) -> (3, ...) with zeros."""
    out = np.zeros((MAX_M,) + a.shape[1:], dtype=a.dtype)
    out[:m] = a
    return out


_SOLVERS: dict = {}


def _shared_solver(problem, systems) -> EventSolver:
    key = (bytes(problem), tuple(bytes(s) for s in systems))
    s = _SOLVERS.get(key)
    if s is None:
        s = _SOLVERS[key] = EventSolver(problem, systems)
    return s


# ---------------------------------------------------------------------- the local MPCs
class LocalMpc:
    """Mpc for a vehicle, solving for states of vehicle in front and behind; local state is
    organised x = [x_front, x_me, x_back] (fleet_event_based.py:26-341)."""

    Q_x = Params.Q_x
    Q_u = Params.Q_u
    Q_du = Params.Q_du
    w = Params.w
    a_acc = Params.a_acc
    a_dec = Params.a_dec
    ts = Params.ts
    d_safe = Params.d_safe
    discrete_gears = False

    def __init__(self, N: int, systems: list[dict], num_vehicles_in_front: int, num_vehicles_behind: int,
                 spacing_policy: SpacingPolicy = ConstantSpacingPolicy(50), rel_leader_index: int | None = None,
                 quadratic_cost: bool = True, thread_limit: int | None = None, accel_cnstr_tightening: float = 0.0,
                 gears=None, max_nodes: int = DROPIN_MAX_NODES) -> None:
        self.n = len(systems)
        self.N = N
        self.thread_limit = thread_limit  # no CPU thread pool: kept for signature compatibility
        self.max_nodes = int(max_nodes)
        self.tables = self._tables(systems, gears)
        self.num_bin_vars = self._bin_vars(systems) * N
        self.leader_x = np.zeros((2, N + 1))
        self.x_f2 = np.zeros((2, N + 1))
        self.x_b2 = np.zeros((2, N + 1))
        self.x_pred = self.u_pred = self.regions_pred = self.gears_pred = None
        self.setup_cost_and_constraints(None, num_vehicles_in_front, num_vehicles_behind, spacing_policy,
                                        rel_leader_index, quadratic_cost, accel_cnstr_tightening)

    def _tables(self, systems, gears):
        return [tables.system_from_dict(s, None if gears is None else gears[i]) for i, s in enumerate(systems)]

    def _bin_vars(self, systems) -> int:
        return sum(len(s["S"]) for s in systems)

    def setup_cost_and_constraints(self, u, num_vehicles_in_front: int, num_vehicles_behind: int,
                                   spacing_policy: SpacingPolicy = ConstantSpacingPolicy(50),
                                   rel_leader_index: int | None = None, quadratic_cost: bool = True,
                                   accel_cnstr_tightening: float = 0.0) -> None:
        """fleet_event_based.py:72-291: the cost / constraint constants become the handle's problem
        and the boundary / leader layout the instance descriptor."""
        if not quadratic_cost:
            raise NotImplementedError("the event-based controller is quadratic only here: simulate() never builds "
                                      "the min_1_norm LocalMpc (DESIGN.md section 5e)")
        if rel_leader_index not in (None, -1, 0, 1):
            raise ValueError(f"rel leader index must be -1, 0, or 1. Got {rel_leader_index}.")
        f, b = int(num_vehicles_in_front), int(num_vehicles_behind)
        if not (0 <= f <= 2 and 0 <= b <= 2):
            raise ValueError("num_vehicles_in_front / num_vehicles_behind must be 0, 1 or 2")
        if self.n != 1 + min(f, 1) + min(b, 1):
            raise ValueError(f"{self.n} systems do not match {f} vehicle(s) in front and {b} behind")
        self.me = min(f, 1)  # local index of the agent's own vehicle
        lead = -1 if rel_leader_index is None else self.me - rel_leader_index
        if rel_leader_index is not None and not 0 <= lead < self.n:
            raise ValueError(f"rel_leader_index {rel_leader_index} names a vehicle outside the local problem")
        self.desc = (self.n, f == 2, b == 2, lead)
        self.spacing_policy = spacing_policy
        self.problem = cent_problem(self.N, spacing_policy, True, accel_cnstr_tightening, params=type(self))

    # ------------------------------------------------------------ parameters
    def _traj(self, a) -> np.ndarray:
        a = np.asarray(a, dtype=np.float64)
        if a.shape != (2, self.N + 1):
            raise ValueError(f"expected a (2, {self.N + 1}) trajectory, got {a.shape}")
        return a.copy()

    def set_leader_x(self, leader_x) -> None:
        self.leader_x = self._traj(leader_x)

    def set_x_f2(self, x_f2) -> None:
        self.x_f2 = self._traj(x_f2)

    def set_x_b2(self, x_b2) -> None:
        self.x_b2 = self._traj(x_b2)

    def params_for(self, x0) -> np.ndarray:
        _, f2, b2, lead = self.desc
        return pack_params(self.N, np.asarray(x0, dtype=np.float64).reshape(-1)[:2 * self.n],
                           self.x_f2 if f2 else None, self.x_b2 if b2 else None, self.leader_x if lead >= 0 else None)

    def _solver(self) -> EventSolver:
        return _shared_solver(self.problem, self.tables)

    def _sys(self) -> np.ndarray:
        return _pad(np.arange(self.n, dtype=np.int32), self.n)[None]

    # ------------------------------------------------------------ evaluation and solve
    def eval_cost(self, x: np.ndarray, u: np.ndarray, discrete_gears: bool = False, gears=None) -> float:
        """Cost of the fixed guesses x (2m, N+1), u (m, N) with optimal slacks, inf if infeasible
        (:308-327).  A departure from the reference's call shape: with discrete gears the reference
        fixes u_g alone and leaves the gear binaries to its solver, while the device evaluation
        fixes the gear of every step, so ``gears`` (m, N) must be passed then (ValueError without
        it; the coordinator passes its gear guesses).  INTEGRATION.md names this."""
        m, N = self.n, self.N
        xg = _pad(np.asarray(x, dtype=np.float64).reshape(m, 2, N + 1), m)
        ug = _pad(np.asarray(u, dtype=np.float64).reshape(-1, N)[:m], m)
        gg = None
        if discrete_gears:
            if gears is None:
                raise ValueError("eval_cost with discrete gears needs the gear guesses")
            gg = _pad(np.asarray(gears).reshape(m, N).astype(np.int8), m)[None]
        cost, _ = self._solver().evaluate([self.desc], self._sys(), self.params_for(xg[:, :, 0].reshape(-1))[None],
                                          xg[None], ug[None], gg)
        return float(cost[0])

    def solve_mpc(self, state, raises: bool = False):
        t0 = time.perf_counter()
        res = self._solver().solve([self.desc], self._sys(), self.params_for(state)[None], self.max_nodes)
        return self.absorb(res, 0, time.perf_counter() - t0, raises, state)

    def absorb(self, res: EventResult, b: int, run_time: float, raises: bool, state=None):
        m, N = self.n, self.N
        ok = int(res.status[b]) == _abi.OPTIMAL
        if not ok:
            if raises:
                raise RuntimeError(f"MPC for state {np.asarray(state).reshape(-1)} returned "
                                   f"{_abi.STATUS_NAMES.get(int(res.status[b]))}")
            x, u, cost = np.zeros((2 * m, N + 1)), np.zeros((m, N)), float("inf")
        else:
            x = res.x[b, :m].reshape(2 * m, N + 1).copy()
            u = res.u[b, :m].copy()
            cost = float(res.cost[b])
        self.x_pred, self.u_pred = x, u
        self.regions_pred = res.region[b, :m].copy()
        self.gears_pred = res.gear[b, :m].astype(float)
        info = {"x": x, "u": u, "cost": cost, "run_time": run_time, "nodes": int(res.nodes[b]),
                "bin_vars": self.num_bin_vars, "status": int(res.status[b])}
        return u[:, [0]], info


class LocalMpcGear(LocalMpc):
    """fleet_event_based.py:343-376: the pwa_friction model with gear binaries; every vehicle's table
    holds one mode per (gear, friction region) as :class:`hvp.cent.MpcGearCent`, the cost and the
    control box are on u_g.  ``solve_mpc -> [u_g0; gear0]``, ``info["u"] = vstack(u_g, gears)``."""

    discrete_gears = True

    def _tables(self, systems, gears):
        return [tables.gear_system_from_dict(s) for s in systems]

    def _bin_vars(self, systems) -> int:
        return sum(len(s["S"]) + len(Vehicle.b) for s in systems)

    def absorb(self, res: EventResult, b: int, run_time: float, raises: bool, state=None):
        ok = int(res.status[b]) == _abi.OPTIMAL
        if not ok and raises:
            raise RuntimeWarning(f"gear mpc for state {np.asarray(state).reshape(-1)} is infeasible.")
        _, info = LocalMpc.absorb(self, res, b, run_time, False, state)
        m = self.n
        if ok:
            u_g, gears = res.u[b, :m].copy(), res.gear[b, :m].astype(float)
        else:
            u_g, gears = np.zeros((m, self.N)), 6 * np.ones((m, self.N))  # mpc_gear.py:129-131
        info["u"] = np.vstack((u_g, gears))
        self.u_pred = info["u"]
        self.gears_pred = gears
        return np.vstack((u_g[:, [0]], gears[:, [0]])), info


# ---------------------------------------------------------------------- the coordinator
class TrackingEventBasedCoordinator(MldAgent):
    """fleet_event_based.py:413-646 for one platoon; all agents of an iteration in one batch."""

    def __init__(self, local_mpcs: list[LocalMpc], vehicles: list, ep_len: int, N: int, leader_x: np.ndarray,
                 discrete_gears: bool, ts: float, event_iters: int = 4, leader_index: int = 0) -> None:
        super().__init__(local_mpcs[0])
        self.n = len(local_mpcs)
        self.agents = [MldAgent(m) for m in local_mpcs]
        self.nx_l = Vehicle.nx_l
        self.nu_l = Vehicle.nu_l
        self.vehicles = vehicles
        self.num_iters = event_iters
        self.leader_x = leader_x
        self.ts = ts
        self.N = N
        self.discrete_gears = discrete_gears
        self.leader_index = leader_index
        self.state_guesses = [np.zeros((self.nx_l, N + 1)) for _ in range(self.n)]
        self.control_guesses = [np.zeros((self.nu_l, N)) for _ in range(self.n)]
        self.gear_guesses = [np.zeros((self.nu_l, N)) for _ in range(self.n)]
        self.solve_times = np.zeros((ep_len, 1))
        self.node_counts = np.zeros((ep_len, 1))
        self.temp_solve_time = 0
        self.temp_node_count = 0
        self.history: list[dict] = []  # per step: the winner of every iteration run, eval / new costs
        # one handle for the platoon: vehicle j's table is the one its own agent holds for it
        lay = local_layout(self.n, leader_index)
        for i, (mpc, L) in enumerate(zip(local_mpcs, lay)):
            if not isinstance(mpc, LocalMpc):
                raise TypeError("TrackingEventBasedCoordinator needs hvp.event.LocalMpc objects")
            want = (L["m"], L["num_vehicles_in_front"] == 2, L["num_vehicles_behind"] == 2, L["leader"])
            if mpc.desc != want or mpc.N != N:
                raise ValueError(f"local MPC {i} is not agent {i} of a platoon of {self.n} (leader {leader_index})")
            if bytes(mpc.problem) != bytes(local_mpcs[0].problem):
                raise ValueError("local MPCs must share the controller constants")
        self._lay = lay
        self._solver = EventSolver(local_mpcs[0].problem, [m.tables[m.me] for m in local_mpcs])
        self._sys = np.stack([_pad(np.arange(L["lo"], L["lo"] + L["m"], dtype=np.int32), L["m"]) for L in lay])
        self._desc = [m.desc for m in local_mpcs]

    # ------------------------------------------------------------ one iteration's batch
    def _batch(self, x: np.ndarray):
        n, N = self.n, self.N
        params, xg, ug, gg = [], [], [], []
        for i, L in enumerate(self._lay):
            lo, m = L["lo"], L["m"]
            mpc = self.agents[i].mpc
            if i > 1:
                mpc.set_x_f2(self.state_guesses[i - 2])
            if i < n - 2:
                mpc.set_x_b2(self.state_guesses[i + 2])
            params.append(mpc.params_for(x[lo:lo + m].reshape(-1)))
            xg.append(_pad(np.stack(self.state_guesses[lo:lo + m]), m))
            ug.append(_pad(np.vstack(self.control_guesses[lo:lo + m]), m))
            gg.append(_pad(np.vstack(self.gear_guesses[lo:lo + m]).astype(np.int8), m))
        return np.stack(params), np.stack(xg), np.stack(ug), np.stack(gg)

    def get_control(self, state, raises: bool = True):
        n = self.n
        x = np.asarray(state, dtype=np.float64).reshape(n, self.nx_l)
        step = {"winners": [], "eval": [], "new": []}
        for _ in range(self.num_iters):
            params, xg, ug, gg = self._batch(x)
            ev, _ = self._solver.evaluate(self._desc, self._sys, params, xg, ug, gg if self.discrete_gears else None)
            t0 = time.perf_counter()  # the agents' run time is the solve batch (its copies included), not the pricing
            res = self._solver.solve(self._desc, self._sys, params, self.agents[0].mpc.max_nodes)
            dt = time.perf_counter() - t0
            for i, a in enumerate(self.agents):  # every agent's solve is part of the one launch
                _, info = a.mpc.absorb(res, i, dt, False, x[self._lay[i]["lo"]:])
                a.record(info)
            new = np.array([a.get_predicted_cost() for a in self.agents])
            best_idx = select_winner(ev, new, threshold)  # RuntimeWarning without a feasible solve
            self.temp_solve_time += max(a.run_time for a in self.agents)
            self.temp_node_count = max(max(a.node_count for a in self.agents), self.temp_node_count)
            step["winners"].append(best_idx)
            step["eval"].append(ev)
            step["new"].append(new)
            if best_idx < 0:  # don't repeat the repetitions if no-one improved cost
                break
            L = self._lay[best_idx]
            a = self.agents[best_idx]
            for j in range(L["m"]):
                self.state_guesses[L["lo"] + j] = a.x_pred[2 * j:2 * j + 2, :].copy()
                self.control_guesses[L["lo"] + j] = a.u_pred[[j], :].copy()
                if self.discrete_gears:
                    self.gear_guesses[L["lo"] + j] = a.mpc.gears_pred[[j], :].copy()
        self.history.append(step)
        u0 = np.vstack([self.control_guesses[i][:, [0]] for i in range(n)])
        if self.discrete_gears:
            return np.vstack((u0, np.vstack([self.gear_guesses[i][:, [0]] for i in range(n)]))), {}
        return u0, {}

    # ------------------------------------------------------------ hooks
    def _set_leader(self, leader_x) -> None:
        for i in (self.leader_index - 1, self.leader_index, self.leader_index + 1):
            if 0 <= i < self.n:
                self.agents[i].mpc.set_leader_x(leader_x)

    def on_timestep_end(self, env, episode: int, timestep: int) -> None:
        self._set_leader(self.leader_x[:, timestep:timestep + self.N + 1])
        for i in range(self.n):
            self.state_guesses[i] = shift_guesses(self.state_guesses[i])
            self.control_guesses[i] = shift_guesses(self.control_guesses[i])
            if self.discrete_gears:
                self.gear_guesses[i] = shift_guesses(self.gear_guesses[i])
        self.solve_times[env.step_counter - 1, :] = self.temp_solve_time
        self.node_counts[env.step_counter - 1, :] = self.temp_node_count
        self.temp_solve_time = 0
        self.temp_node_count = 0

    def on_episode_start(self, env, episode: int, state) -> None:
        self._set_leader(self.leader_x[:, 0:self.N + 1])
        xs, us, gs = initial_guesses(np.asarray(env.x).reshape(-1), self.vehicles, self.N, self.ts, self.discrete_gears)
        for i in range(self.n):
            self.state_guesses[i] = xs[i]
            self.control_guesses[i] = us[[i]]
            if self.discrete_gears:
                self.gear_guesses[i] = gs[[i]]

    def extrapolate_position(self, initial_pos, initial_vel) -> np.ndarray:
        return extrapolate(float(np.asarray(initial_pos).reshape(-1)[0]), float(np.asarray(initial_vel).reshape(-1)[0]),
                           self.N, self.ts)


def simulate(sim: Sim, event_iters: int, save: bool = False, plot: bool = False, seed: int = 2,
             thread_limit: int | None = None, leader_index: int = 0):
    """Closed-loop run of the event-based controller (fleet_event_based.py:649-766)."""
    n, N, ep_len, ts = sim.n, sim.N, sim.ep_len, Params.ts
    leader_x = sim.leader_trajectory.get_leader_trajectory()
    if sim.vehicle_model_type == "pwa_gear":
        mpc_class, discrete_gears = LocalMpc, False
    elif sim.vehicle_model_type == "pwa_friction":
        mpc_class, discrete_gears = LocalMpcGear, True
    elif sim.vehicle_model_type == "nonlinear":
        raise NotImplementedError("LocalMpcNonlinearGear (nonlinear vehicle model) is out of scope (DESIGN.md)")
    else:
        raise ValueError(f"{sim.vehicle_model_type} is not a valid vehicle model type.")
    platoon = Platoon(n, vehicle_type=sim.vehicle_model_type, masses=sim.masses)
    systems = platoon.get_vehicle_system_dicts(ts)
    vehicles = platoon.get_vehicles()
    env = EpisodeMonitor(
        PlatoonEnv(n=n, platoon=platoon, leader_trajectory=sim.leader_trajectory, spacing_policy=sim.spacing_policy,
                   start_from_platoon=sim.start_from_platoon, leader_index=leader_index, ep_len=ep_len),
        max_episode_steps=ep_len,
    )
    mpcs = []
    for i, L in enumerate(local_layout(n, leader_index)):
        lo, m = L["lo"], L["m"]
        kw = {} if discrete_gears else {"gears": [tables.gears_of(v) for v in vehicles[lo:lo + m]]}
        mpcs.append(mpc_class(N, systems=systems[lo:lo + m], num_vehicles_in_front=L["num_vehicles_in_front"],
                              num_vehicles_behind=L["num_vehicles_behind"], rel_leader_index=L["rel_leader_index"],
                              spacing_policy=sim.spacing_policy, thread_limit=thread_limit, **kw))
    agent = TrackingEventBasedCoordinator(mpcs, vehicles=vehicles, ep_len=ep_len, N=N, leader_x=leader_x,
                                          discrete_gears=discrete_gears, ts=ts, event_iters=event_iters,
                                          leader_index=leader_index)
    agent.evaluate(env=env, episodes=1, seed=seed)
    X = env.observations[0].squeeze()
    U = env.actions[0].squeeze()
    R = env.rewards[0]
    if save:
        write_results(f"event_{event_iters}_{sim.id}_seed_{seed}.pkl", X, U, R, agent.solve_times, agent.node_counts,
                      env.unwrapped.viol_counter[0], leader_x)
    return X, U, R, agent, env


def write_results(path: str, X, U, R, solve_times, node_counts, violations, leader_x) -> None:
    """The seven objects of the reference's results file, in its order (:755-766)."""
    with open(path, "wb") as f:
        for obj in (X, U, R, solve_times, node_counts, violations, leader_x):
            pickle.dump(obj, f)
