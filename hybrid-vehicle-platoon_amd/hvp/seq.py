"""Sequential MLD controller: coordinator + ``simulate`` (fleet_seq_mld.py:296-545).

The local problem is the decentralised one (``LocalMpcMld`` / ``LocalMpcGear``, HVP_FORM_DECENT:
same parameter block, same role bits); only the source of the neighbour trajectories differs.  A
vehicle does not extrapolate its neighbours' measured states: per step the leader L solves first,
then the vehicles ahead of it (L-1 .. 0), then those behind it (L+1 .. n-1), and every vehicle
is handed

* the trajectory its neighbour on the leader's side solved in THIS step, as it is ("fresh"), and
* the other neighbour's trajectory of the PREVIOUS step shifted by one sample -- column 0
  dropped, the last column repeated, the last position then set to old p_N + ts * old v_N
  ("shifted"); before any prediction exists (the first step of an episode) the constant-velocity
  extrapolation of that neighbour's state, which is what ``on_episode_start`` sets.

The leader itself takes both neighbours shifted.  :func:`stage_blocks` is that rule in numpy;
``hvp_seq_stage_params`` (include/hvp_seq.h) is the same rule on the device for P platoons, which
the batched closed loop of ``hvp.sweep.run_point(controller="seq")`` runs between its stages.

The n solves of a step are a dependent chain, so here every stage is one ``hvp_solve_batch_host``
call of one instance on the platoon's handle; ``solve_times`` is the SUM of the agents' run
times (they run in series) and ``node_counts`` the max (fleet_seq_mld.py:404-409).
"""

from __future__ import annotations

import pickle
import time

import numpy as np

from .agent import MldAgent
from .batched import extrapolate
from .env import EpisodeMonitor, PlatoonEnv
from .models import Platoon, Vehicle
from .mpc import LocalMpcGear, LocalMpcMld
from .params import Params, Sim
from .tables import gears_of


def solve_order(n: int, leader_index: int) -> list[int]:
    """Vehicles in the order they solve within a step (fleet_seq_mld.py:336-386)."""
    return [leader_index] + list(range(leader_index - 1, -1, -1)) + list(range(leader_index + 1, n))


def stage_blocks(i: int, n: int, leader_index: int, x, xpred, first: bool, N: int, ts: float = 1.0):
    """Front and back neighbour blocks of vehicle i when its turn comes (the table in the module
    docstring).  x (..., 2n) the measured states; xpred (n, ..., 2, N+1) the prediction store:
    slot j holds the trajectory vehicle j solved last -- this step's if j solved before i, the
    previous step's otherwise (with ``first`` a slot whose vehicle has not solved yet is not
    read).  Returns (front, back), each (..., 2, N+1) or None where the vehicle has no such
    neighbour (a new array, never a view of xpred)."""
    x = np.asarray(x, dtype=np.float64)

    def fresh(j):
        return np.array(xpred[j], dtype=np.float64)

    def shifted(j):
        if first:
            return extrapolate(x[..., 2 * j], x[..., 2 * j + 1], N, ts)
        s = np.asarray(xpred[j], dtype=np.float64)
        out = np.concatenate((s[..., 1:], s[..., -1:]), axis=-1)
        out[..., 0, -1] = out[..., 0, -2] + ts * out[..., 1, -1]
        return out

    front = None if i == 0 else fresh(i - 1) if i > leader_index else shifted(i - 1)
    back = None if i == n - 1 else fresh(i + 1) if i < leader_index else shifted(i + 1)
    return front, back


class TrackingSequentialMldCoordinator(MldAgent):
    def __init__(self, local_mpcs: list, ep_len: int, N: int, leader_x: np.ndarray, ts: float,
                 leader_index: int = 0, order_forwards: bool = True) -> None:
        super().__init__(local_mpcs[0])
        self.n = len(local_mpcs)
        self.agents = [MldAgent(m) for m in local_mpcs]
        self.solve_times = np.zeros((ep_len, 1))
        self.node_counts = np.zeros((ep_len, 1))
        self.leader_x = leader_x
        self.nx_l = Vehicle.nx_l
        self.nu_l = Vehicle.nu_l
        self.ep_len = ep_len
        self.ts = ts
        self.N = N
        self.leader_index = leader_index
        self.forwards = order_forwards  # accepted and unused, as in the reference (:330)
        # slot j: the trajectory vehicle j solved last; _first until a whole step has been solved
        self._xpred = np.zeros((self.n, self.nx_l, N + 1))
        self._first = True
        # per step: the states x0 (n, 2) and every agent's x_pred (n, 2, N+1), u_pred, cost, region
        # sequence and HVP_* status
        self.history: list[dict] = []
        # one handle for the whole platoon (as hvp/decent.py), every stage a solve of one instance
        # on it.  Local MPCs without solver tables (any object with the MpcMld surface) are
        # solved through their own solve_mpc, as the reference's coordinator does.
        self._solver = None
        if all(getattr(m, "problem", None) is not None and hasattr(m, "table") for m in local_mpcs):
            from .solver import BatchSolver

            prob = local_mpcs[0].problem
            for m in local_mpcs[1:]:
                if bytes(m.problem) != bytes(prob):
                    raise ValueError("local MPCs must share the controller constants")
            self._solver = BatchSolver(prob, [m.table for m in local_mpcs])

    # ------------------------------------------------------------ control (n dependent stages)
    def _solve_stage(self, i: int, x_i: np.ndarray, raises: bool):
        a = self.agents[i]
        if self._solver is None:
            return a.get_control(x_i.reshape(self.nx_l, 1), raises)
        t0 = time.perf_counter()
        res = self._solver.solve(np.array([i], np.int32), np.array([a.mpc.role], np.int32), a.mpc.params_for(x_i)[None])
        ui, info = a.mpc.absorb(res, 0, time.perf_counter() - t0, raises, x_i)
        a.record(info)
        return ui, info

    def get_control(self, state: np.ndarray, raises: bool = True):
        x = np.asarray(state, dtype=np.float64).reshape(self.n, self.nx_l)
        u = [None] * self.n
        step = {"x0": x.copy(), "u_pred": [None] * self.n, "cost": np.zeros(self.n), "region": [None] * self.n,
                "status": np.zeros(self.n, dtype=np.int32)}
        for i in solve_order(self.n, self.leader_index):
            front, back = stage_blocks(i, self.n, self.leader_index, x.reshape(-1), self._xpred, self._first,
                                       self.N, self.ts)
            if front is not None:
                self.agents[i].mpc.set_x_front(front)
            if back is not None:
                self.agents[i].mpc.set_x_back(back)
            u[i], info = self._solve_stage(i, x[i], raises)
            self._xpred[i] = info["x"]
            step["u_pred"][i] = np.array(info["u"])
            step["cost"][i] = info["cost"]
            step["status"][i] = info.get("status", 0)
            region = getattr(self.agents[i].mpc, "regions_pred", None)
            step["region"][i] = None if region is None else np.array(region)
        self._first = False
        step["x_pred"] = self._xpred.copy()
        self.history.append(step)
        if u[0].shape[0] > self.nu_l:  # gear MPCs: continuous controls first, then the gears (:388-395)
            return np.vstack((np.vstack([ui[: self.nu_l] for ui in u]), np.vstack([ui[self.nu_l:] for ui in u]))), {}
        return np.vstack(u), {}

    # ------------------------------------------------------------ hooks
    def on_timestep_end(self, env, episode: int, timestep: int) -> None:
        self.agents[self.leader_index].mpc.set_leader_x(self.leader_x[:, timestep:timestep + self.N + 1])
        # the local MPCs are solved in series: the sum of their times, the worst node count
        self.solve_times[env.step_counter - 1, :] = sum(a.run_time for a in self.agents)
        self.node_counts[env.step_counter - 1, :] = max(a.node_count for a in self.agents)

    def on_episode_start(self, env, episode: int, state) -> None:
        self.agents[self.leader_index].mpc.set_leader_x(self.leader_x[:, 0:self.N + 1])
        x = np.asarray(env.x, dtype=np.float64).reshape(-1)
        for i in range(self.n):  # initial estimates, kept by the blocks no prediction replaces yet
            if i != 0:
                self.agents[i].mpc.set_x_front(
                    self.extrapolate_position_constant_vel(x[self.nx_l * (i - 1)], x[self.nx_l * (i - 1) + 1]))
            if i != self.n - 1:
                self.agents[i].mpc.set_x_back(
                    self.extrapolate_position_constant_vel(x[self.nx_l * (i + 1)], x[self.nx_l * (i + 1) + 1]))

    def extrapolate_position_constant_vel(self, initial_pos: float, initial_vel: float) -> np.ndarray:
        return extrapolate(initial_pos, initial_vel, self.N, self.ts)


def simulate(sim: Sim, save: bool = False, plot: bool = False, seed: int = 1, thread_limit: int | None = None,
             leader_index: int = 0, order_forwards: bool = True, verbose: bool = False):
    """Closed-loop run of the sequential controller (fleet_seq_mld.py:443-545)."""
    n, N, ep_len, ts = sim.n, sim.N, sim.ep_len, Params.ts
    leader_x = sim.leader_trajectory.get_leader_trajectory()
    if sim.vehicle_model_type not in ("pwa_gear", "pwa_friction"):
        raise NotImplementedError("the GPU path implements the pwa_gear (LocalMpcMld) and pwa_friction "
                                  "(LocalMpcGear) models; the nonlinear model is out of scope (DESIGN.md)")
    platoon = Platoon(n, vehicle_type=sim.vehicle_model_type, masses=sim.masses)
    systems = platoon.get_vehicle_system_dicts(ts)
    env = EpisodeMonitor(
        PlatoonEnv(n=n, platoon=platoon, leader_trajectory=sim.leader_trajectory, spacing_policy=sim.spacing_policy,
                   start_from_platoon=sim.start_from_platoon, real_vehicle_as_reference=sim.real_vehicle_as_reference,
                   ep_len=ep_len, leader_index=leader_index, quadratic_cost=sim.quadratic_cost),
        max_episode_steps=ep_len,
    )
    vehicles = platoon.get_vehicles()

    def local(i):
        kw = dict(quadratic_cost=sim.quadratic_cost, is_front=i == 0, is_leader=i == leader_index,
                  is_trailer=i == n - 1, thread_limit=thread_limit,
                  real_vehicle_as_reference=sim.real_vehicle_as_reference)
        if sim.vehicle_model_type == "pwa_friction":  # fleet_seq_mld.py:485-486
            return LocalMpcGear(N, systems[i], sim.spacing_policy, **kw)
        return LocalMpcMld(N, systems[i], sim.spacing_policy, gears=gears_of(vehicles[i]), **kw)

    mpcs = [local(i) for i in range(n)]
    agent = TrackingSequentialMldCoordinator(mpcs, ep_len=ep_len, N=N, leader_x=leader_x, ts=ts,
                                             leader_index=leader_index, order_forwards=order_forwards)
    agent.evaluate(env=env, episodes=1, seed=seed)
    X = env.observations[0].squeeze()
    U = env.actions[0].squeeze()
    R = env.rewards[0]
    if verbose:
        print(f"Return = {sum(R.squeeze())}")
        print(f"Violations = {env.unwrapped.viol_counter}")
        print(f"Run_times_sum: {sum(agent.solve_times)}")
    if save:
        with open(f"seq_{sim.id}_seed_{seed}.pkl", "wb") as f:
            for obj in (X, U, R, agent.solve_times, agent.node_counts, env.unwrapped.viol_counter[0], leader_x):
                pickle.dump(obj, f)
    return X, U, R, agent, env
