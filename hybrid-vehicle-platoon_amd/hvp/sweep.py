"""The n x N x seed sweep of the decentralised controller (configs[4], the reference's
n_sweep*.py loops over ``simulate(Sim_n_task_2(n, seed), save=True)``) as ONE job on the device;
``--controller seq`` sweeps the sequential controller (fleet_seq_mld.py, hvp/seq.py) and
``--controller event --event-iters K`` the event-based one (fleet_event_based.py, hvp/event.py)
instead.

Every (n, N) point runs its seeds as one batch of platoons in closed loop on the GPU -- the
neighbour predictions (hvp_decent_params_batch), the n local MIQPs of every platoon
(hvp_solve_batch) and PlatoonEnv.step (hvp_env_step_batch) per time step, ``ep_len`` steps --
with the task_2 setting of misc/common_controller_params.py:54-76: per-vehicle masses
U(700, 1000) drawn with ``np.random.seed(seed)``, constant-time spacing (10, 3), the
stop-and-go leader.  Each seed's episode is written as the reference's results file (7 pickles:
X, U, R, solve_times, node_counts, violations, leader_x; fleet_decent_mld.py:548-559), named as
the reference names it, so results_analysis/* reads a sweep directory unchanged.

Multi-GPU: one process per GPU (torch.distributed.run); every rank takes a contiguous share of
the seeds of EVERY point (``shard``), so each rank's work mixes the cheap and the expensive
points alike; no collective in the data path, a gather of the per-rank summaries at the end.
Within a GPU a point's seeds run as ``--streams`` blocks at once (a host thread and HIP stream
each, ``run_points``), so one block's kernels fill the CUs the other's level tails leave.

The sequential controller's n solves of a step are a dependent chain (leader, then the vehicles
ahead of it, then those behind; hvp/seq.py), so its batch runs n stages of S instances per step:
hvp_seq_stage_params (the neighbour blocks from the vehicle-major prediction store), then
hvp_solve_batch of vehicle i of every platoon, writing its trajectories straight into slot i of
that store; PlatoonEnv.step after the last stage.  Its files are ``seq_{sim.id}_seed_{s}.pkl``.

The event-based controller runs ``event_iters`` iterations per step, each four launches over the
S n agents of the batch -- hvp_event_gather (the agents' parameter blocks and guesses from the
vehicle-major guess store), hvp_event_evaluate_batch, hvp_event_solve_batch, hvp_event_select
(the winner rule, the guess update and the per-platoon ``active`` flag) -- with no host read; a
platoon nobody improved is still gathered and solved, it just cannot win.  hvp_event_shift after
the plant step.  Its files are ``event_{K}_{sim.id}_seed_{s}.pkl``.

    python -m hvp.sweep --out results/ [--n 5 10 15 20] [--N 5 10 15] [--seeds 100] [--ep-len 150]
                        [--controller {decent,seq,event}] [--leader-index K] [--event-iters K]
"""

from __future__ import annotations

import argparse
import json
import os
import pickle
import threading
import time

import numpy as np

from . import _abi, tables
from .env import derive_env_seed, initial_platoon_state
from .models import Platoon
from .params import Params, Sim_n_task_2


# run_points runs several run_point calls at once on host threads; the reference-style setup code
# draws from numpy's global generator, so that part is serialised
_RNG_LOCK = threading.Lock()


def shard(points, n_seeds: int, rank: int, world: int):
    """Work of `rank`: for every (n, N) point a contiguous block of the seeds 0..n_seeds-1 (the
    first n_seeds % world ranks get one more).  Together the ranks cover every (n, N, seed)
    exactly once."""
    base, extra = divmod(n_seeds, world)
    lo = rank * base + min(rank, extra)
    hi = lo + base + (1 if rank < extra else 0)
    return [(n, N, list(range(lo, hi))) for n, N in points if hi > lo]


def run_point(n: int, N: int, seeds, ep_len: int = 150, device: int = 0, out_dir: str | None = None,
              velocity_estimator: str = "none", warm_incumbent: bool = True, controller: str = "decent",
              leader_index: int | None = None, return_pred: bool = False, event_iters: int = 3) -> dict:
    """Closed-loop episodes of the decentralised (or, controller="seq", the sequential) controller
    for `seeds` (one platoon each) at (n, N), all on the device.  Returns per-seed X (T+1, 2n),
    U (T, n), R (T,), violations (T,), node_counts (T,), the step times and status_counts (local
    problems per HVP_* status; anything but optimal raises); writes the reference's results files
    if out_dir.  leader_index (seq only): None is vehicle 0 under the plain sim id, an index K
    also names the files ``..._lead_K`` as n_sweep_3.py's Sim_n_task_2(n, seed, leader_index) does.
    return_pred (seq only): also XPRED (T, n, S, 2, N+1), every vehicle's prediction of every step.
    controller="event": ``event_iters`` iterations per step (leader_index as for seq, the files'
    ``_lead_K`` id included); also returns WINNERS (T, event_iters, S): the winning agent of every
    iteration, -1 where nobody won or the platoon had stopped."""
    if controller not in ("decent", "seq", "event"):
        raise ValueError(f"controller must be 'decent', 'seq' or 'event', got {controller!r}")
    if controller == "decent" and (leader_index is not None or return_pred):
        raise ValueError("leader_index and return_pred are parameters of the seq path")
    if controller == "event" and return_pred:
        raise ValueError("return_pred is a parameter of the seq path")
    if controller == "seq" and velocity_estimator != "none":
        raise ValueError("the sequential controller has no velocity estimator (it observes no states)")
    if controller == "event" and velocity_estimator != "none":
        raise ValueError("the event-based controller has no velocity estimator (it observes no states)")
    if controller == "event" and (event_iters < 1 or n < 2):
        raise ValueError("the event-based controller needs event_iters >= 1 and n >= 2")
    lead = 0 if leader_index is None else int(leader_index)
    if not 0 <= lead < n:
        raise ValueError(f"leader_index {lead} outside 0..{n - 1}")
    import torch

    from .envdev import DeviceEnv
    from .solver import BatchSolver

    S, T = len(seeds), ep_len
    dev = torch.device("cuda", device)
    with _RNG_LOCK:  # Sim_n_task_2 and env.reset seed numpy's GLOBAL generator (params.py, env.py)
        sims = [Sim_n_task_2(n, seed=int(s), leader_index=leader_index, N=N) for s in seeds]
        x_init = np.stack([initial_platoon_state(n, derive_env_seed(int(s))).reshape(-1).astype(np.float64)
                           for s in seeds])
    leader_x = sims[0].leader_trajectory.get_leader_trajectory()  # (2, ep_len + 50), seed-independent
    if T + N + 1 > leader_x.shape[1]:  # Sim_n_task_2 builds the trajectory for its own ep_len (150)
        raise ValueError(f"ep_len {T} with N = {N} needs {T + N + 1} leader samples; the Sim_n_task_2 "
                         f"trajectory holds {leader_x.shape[1]} (ep_len <= {leader_x.shape[1] - N - 1})")
    systems, masses, fleet = [], [], []
    for sim in sims:
        pl = Platoon(n, vehicle_type="pwa_gear", masses=sim.masses)
        vehicles = pl.get_vehicles()
        fleet.append(vehicles)
        for i, d in enumerate(pl.get_vehicle_system_dicts(Params.ts)):
            systems.append(tables.system_from_dict(d, tables.gears_of(vehicles[i])))
        masses.append(sim.masses)
    B = S * n
    if controller == "event":
        from .cent import cent_problem
        from .event import EventSolver

        solver = EventSolver(cent_problem(N, sims[0].spacing_policy), systems, device=device)
    else:
        solver = BatchSolver(tables.problem(N, sims[0].spacing_policy), systems, device=device)
        solver.reserve(S if controller == "seq" else B)  # seq: one stage of S instances at a time
    lx = torch.from_numpy(np.ascontiguousarray(leader_x)).to(dev)
    x = torch.from_numpy(x_init).to(dev)
    env = DeviceEnv(solver, torch.tensor(masses, dtype=torch.float64, device=dev), leader_index=lead)
    X = torch.empty((T + 1, S, 2 * n), dtype=torch.float64, device=dev)
    U = torch.empty((T, S, n), dtype=torch.float64, device=dev)
    R = torch.empty((T, S), dtype=torch.float64, device=dev)
    V = torch.empty((T, S), dtype=torch.int32, device=dev)
    NODES = torch.empty((T, S), dtype=torch.int32, device=dev)
    X[0] = x
    u = torch.empty((S, n), dtype=torch.float64, device=dev)
    u_prev = None
    if controller == "seq":
        from .seq import solve_order

        order = solve_order(n, lead)
        # vehicle-major stores: stage i's solve writes vehicle i's outputs of every platoon into
        # slot i; xpred is the prediction store hvp_seq_stage_params reads (slot j: this step's
        # trajectory once stage j has run, the previous step's before)
        xpred = torch.zeros((n, S, 2, N + 1), dtype=torch.float64, device=dev)
        store = {k: torch.empty((n,) + tuple(v.shape), dtype=v.dtype, device=dev)
                 for k, v in solver.alloc_outputs(S, dev).items() if k != "x"}
        store["x"] = xpred
        stage_out = [{k: v[i] for k, v in store.items()} for i in range(n)]
        sys_v = (torch.arange(n, dtype=torch.int32, device=dev)[:, None]
                 + n * torch.arange(S, dtype=torch.int32, device=dev)[None, :]).contiguous()  # [i][p] = p n + i
        params = torch.empty((S, solver.params_stride), dtype=torch.float64, device=dev)
        roles = torch.empty(S, dtype=torch.int32, device=dev)
        # N > 8: every vehicle's previous sequence shifted by one step as a second initial incumbent
        # of its next search (pruning only).  The hint is indexed by batch position: one (S, N)
        # slice per vehicle, set before its stage
        hint = torch.full((n, S, N), -1, dtype=torch.int8, device=dev) if N > 8 and warm_incumbent else None
        codes = torch.arange(len(_abi.STATUS_NAMES), dtype=torch.int32, device=dev)
        counts = torch.zeros(len(_abi.STATUS_NAMES), dtype=torch.int64, device=dev)
        XPRED = torch.empty((T, n, S, 2, N + 1), dtype=torch.float64, device=dev) if return_pred else None
        rvar = bool(sims[0].real_vehicle_as_reference)

        def control(t, win):  # the n dependent stages of step t; nothing leaves the device
            for i in order:
                solver.seq_stage_params_device(i, x, xpred, win, leader_index=lead, real_vehicle_as_reference=rvar,
                                               first=t == 0, params=params, roles=roles)
                if hint is not None:
                    solver.set_region_hint(hint[i])
                solver.solve_device(sys_v[i], roles, params, stage_out[i], retry_overflow=N > 8)
                if hint is not None:
                    hint[i, :, :-1] = store["region"][i, :, 1:]
                    hint[i, :, -1] = store["region"][i, :, -1]
            u.copy_(store["u"][:, :, 0].t())
            counts.add_((store["status"].reshape(-1, 1) == codes).sum(dim=0))
            NODES[t] = store["nodes"].max(dim=0).values
            if return_pred:
                XPRED[t] = xpred
    elif controller == "event":
        from .event import initial_guesses, platoon_desc, threshold

        desc = platoon_desc(n, lead, S)  # host: instance b = p n + i
        vsys = torch.arange(B, dtype=torch.int32, device=dev).view(S, n).contiguous()
        # the guess store, vehicle-major as the seq path's prediction store
        # its episode-start values (on_episode_start) are the host rule's, uploaded once per episode:
        # the same numbers the host coordinator starts from, so the two agree bit for bit where two
        # agents' decreases tie (hvp_event_shift(init=1) is the same rule on the device)
        g0 = [initial_guesses(x_init[k], fleet[k], N, Params.ts, False) for k in range(S)]
        xg = torch.from_numpy(np.ascontiguousarray(np.stack([g[0] for g in g0], axis=1))).to(dev)
        ug = torch.from_numpy(np.ascontiguousarray(np.stack([g[1] for g in g0], axis=1))).to(dev)
        sys3 = torch.empty((B, 3), dtype=torch.int32, device=dev)
        params = torch.empty((B, solver.stride), dtype=torch.float64, device=dev)
        x_guess = torch.empty((B, 3, 2, N + 1), dtype=torch.float64, device=dev)
        u_guess = torch.empty((B, 3, N), dtype=torch.float64, device=dev)
        ev = {"cost": torch.empty(B, dtype=torch.float64, device=dev),
              "status": torch.empty(B, dtype=torch.int32, device=dev)}
        sol = solver.alloc_outputs(B, dev)
        active = torch.empty(S, dtype=torch.int32, device=dev)
        WINNERS = torch.empty((T, event_iters, S), dtype=torch.int32, device=dev)
        codes = torch.arange(len(_abi.STATUS_NAMES), dtype=torch.int32, device=dev)
        counts = torch.zeros(len(_abi.STATUS_NAMES), dtype=torch.int64, device=dev)
        nofeas = torch.zeros((), dtype=torch.int64, device=dev)

        def control(t, win):  # event_iters x (gather, evaluate, solve, select); nothing leaves the device
            active.fill_(1)
            NODES[t] = 0
            for it in range(event_iters):
                solver.gather_device(n, lead, x, vsys, xg, ug, None, win, sys3, params, x_guess, u_guess)
                solver.evaluate_device(desc, sys3, params, x_guess, u_guess, None, ev)
                solver.solve_device(desc, sys3, params, 0, sol)
                solver.select_device(n, ev, sol, xg, ug, None, active, WINNERS[t, it], threshold)
                # the reference stops iterating once nobody wins: a stopped platoon's later solves
                # are not part of its episode (statuses, node counts)
                live = WINNERS[t, it - 1] >= 0 if it else torch.ones(S, dtype=torch.bool, device=dev)
                lb = live.repeat_interleave(n)
                counts.add_(((sol["status"].reshape(-1, 1) == codes) & lb[:, None]).sum(dim=0))
                NODES[t] = torch.maximum(NODES[t], torch.where(live, sol["nodes"].view(S, n).max(dim=1).values,
                                                               torch.zeros_like(NODES[t])))
                nofeas.add_((WINNERS[t, it] == -2).sum())
            u.copy_(ug[:, :, 0].t())
    else:
        t_sys = torch.arange(B, dtype=torch.int32, device=dev)
        out = solver.alloc_outputs(B, dev)
        params = torch.empty((B, solver.params_stride), dtype=torch.float64, device=dev)
        roles = torch.empty(B, dtype=torch.int32, device=dev)
        bad = torch.zeros((), dtype=torch.int64, device=dev)
        x_prev = x.clone()
        # the previous step's sequences shifted by one step (last region repeated) as a second initial
        # incumbent of the next step's local searches (N > 8; pruning only, the answers do not change)
        hint = torch.full((B, N), -1, dtype=torch.int8, device=dev)
        if N > 8 and warm_incumbent:
            solver.set_region_hint(hint)

        def control(t, win):
            solver.decent_params_device(x, win, x_prev=x_prev, estimator=velocity_estimator, params=params,
                                        roles=roles)
            solver.solve_device(t_sys, roles, params, out, retry_overflow=N > 8)
            u.copy_(out["u"][:, 0].view(S, n))
            hint[:, :-1] = out["region"][:, 1:]
            hint[:, -1] = out["region"][:, -1]
            bad.add_((out["status"] != 0).sum())
            NODES[t] = out["nodes"].view(S, n).max(dim=1).values
            x_prev.copy_(x)
    step_s = np.zeros(T)
    for t in range(T):
        t0 = time.perf_counter()
        win = lx[:, t:t + N + 1].unsqueeze(0).expand(S, 2, N + 1).contiguous()
        control(t, win)
        st = env.step(x, u, lx[:, t].unsqueeze(0).expand(S, 2).contiguous(), u_prev=u_prev)
        u_prev = u.clone()
        R[t] = st["cost"]
        V[t] = st["viol"]
        U[t] = u
        X[t + 1] = x
        if controller == "event":
            solver.shift_device(n, xg, ug, None)
        torch.cuda.current_stream(dev).synchronize()  # this run's stream (run_points runs several at once)
        step_s[t] = time.perf_counter() - t0
    if controller in ("seq", "event"):
        status_counts = {_abi.STATUS_NAMES[k]: int(c) for k, c in enumerate(counts.cpu().tolist()) if c}
        if controller == "event" and int(nofeas.item()):
            raise RuntimeWarning("No feasible solution found for any event based agent.")
        if set(status_counts) - {_abi.STATUS_NAMES[_abi.OPTIMAL]}:
            raise RuntimeError(f"sweep point n={n} N={N} ({controller}): local problems not optimal: {status_counts}")
    else:
        if int(bad.item()):
            raise RuntimeError(f"sweep point n={n} N={N}: {int(bad.item())} local MIQPs not optimal")
        status_counts = {_abi.STATUS_NAMES[_abi.OPTIMAL]: T * B}  # `bad` counts every other status
    h = lambda a: a.cpu().numpy()  # noqa: E731
    Xh, Uh, Rh, Vh, Nh = h(X), h(U), h(R), h(V), h(NODES)
    res = {"n": n, "N": N, "seeds": list(seeds), "step_s": step_s, "X": Xh, "U": Uh, "R": Rh, "viol": Vh,
           "nodes": Nh, "leader_x": leader_x, "controller": controller, "status_counts": status_counts}
    if return_pred:
        res["XPRED"] = h(XPRED)
    if controller == "event":
        res["WINNERS"] = h(WINNERS)
    name = {"seq": "seq", "event": f"event_{event_iters}"}.get(controller, f"decent_vest_{velocity_estimator}")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        # the batch's step time is every seed's solve time (the reference records the slowest
        # agent of a step, fleet_decent_mld.py:336-339; here all agents of all seeds share a launch;
        # seq: the sum over the agents, fleet_seq_mld.py:404-408; here the n stages of the step)
        for k, (sim, s) in enumerate(zip(sims, seeds)):
            with open(os.path.join(out_dir, f"{name}_{sim.id}_seed_{s}.pkl"), "wb") as f:
                for obj in (Xh[:, k], Uh[:, k], Rh[:, k].reshape(T, 1, 1), step_s.reshape(T, 1),
                            Nh[:, k].reshape(T, 1).astype(float), Vh[:, k].astype(float), leader_x):
                    pickle.dump(obj, f)
    return res


def run_points(n: int, N: int, seeds, ep_len: int, device: int, out_dir, estimator: str, streams: int = 2,
               controller: str = "decent", leader_index: int | None = None, event_iters: int = 3):
    """run_point over `streams` blocks of the seeds at once, each block on its own host thread and
    HIP stream (the blocks are independent platoons; one block's kernels fill the GPU while the
    other's launches finish or synchronise).  Returns the per-block results and the wall time."""
    import torch

    seeds = list(seeds)
    kw = {"controller": controller, "leader_index": leader_index}
    if controller == "event":
        kw["event_iters"] = event_iters
    K = max(1, min(streams, len(seeds)))
    blocks = [seeds[len(seeds) * j // K:len(seeds) * (j + 1) // K] for j in range(K)]
    res, errs = [None] * K, []

    def work(j):
        try:
            stream = torch.cuda.Stream(torch.device("cuda", device))
            with torch.cuda.stream(stream):
                res[j] = run_point(n, N, blocks[j], ep_len, device, out_dir, estimator, **kw)
        except BaseException as e:  # noqa: BLE001 -- re-raised on the caller's thread
            errs.append(e)

    t0 = time.perf_counter()
    if K == 1:
        res[0] = run_point(n, N, blocks[0], ep_len, device, out_dir, estimator, **kw)
    else:
        th = [threading.Thread(target=work, args=(j,)) for j in range(K)]
        for h in th:
            h.start()
        for h in th:
            h.join()
    if errs:
        raise errs[0]
    return res, time.perf_counter() - t0


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, nargs="+", default=[5, 10, 15, 20])
    ap.add_argument("--N", type=int, nargs="+", default=[5, 10, 15])
    ap.add_argument("--seeds", type=int, default=100)
    ap.add_argument("--ep-len", type=int, default=150)
    ap.add_argument("--out", default=None, help="directory of the results files (none: summary only)")
    ap.add_argument("--estimator", default="none", choices=["none", "two_point", "sat"])
    ap.add_argument("--controller", default="decent", choices=["decent", "seq", "event"],
                    help="decent: fleet_decent_mld.py; seq: the sequential controller of fleet_seq_mld.py; "
                         "event: the event-based controller of fleet_event_based.py")
    ap.add_argument("--leader-index", type=int, default=None,
                    help="seq / event: the vehicle that tracks the leader trajectory (files get the _lead_K id)")
    ap.add_argument("--event-iters", type=int, default=3,
                    help="event only: iterations per step (n_sweep.py: sim_event(..., event_iters=3))")
    ap.add_argument("--streams", type=int, default=1,
                    help="seed blocks run concurrently per point (host threads / streams); measured 68 s vs 70 s "
                         "for the full grid, so 1 by default")
    args = ap.parse_args(argv)

    import torch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dist = None
    if world > 1:
        import torch.distributed as dist

        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    points = [(n, N) for N in args.N for n in args.n]
    t0 = time.perf_counter()
    summary = []
    for n, N, seeds in shard(points, args.seeds, rank, world):
        rs, wall = run_points(n, N, seeds, args.ep_len, local, args.out, args.estimator, args.streams,
                              args.controller, args.leader_index, args.event_iters)
        status_counts: dict = {}
        for r in rs:
            for k, c in r["status_counts"].items():
                status_counts[k] = status_counts.get(k, 0) + c
        R = np.concatenate([r["R"] for r in rs], axis=1)
        ep_s = wall if len(rs) > 1 else float(rs[0]["step_s"].sum())  # concurrent blocks: wall time incl. setup
        summary.append({"controller": args.controller, "n": n, "N": N, "seeds": len(seeds), "episode_s": ep_s,
                        "platoon_steps_per_s": len(seeds) * args.ep_len / ep_s,
                        "mean_return": float(R.sum(axis=0).mean()),
                        "violation_steps": int(sum((r["viol"] > 0).sum() for r in rs)),
                        "max_nodes": int(max(r["nodes"].max() for r in rs)), "status_counts": status_counts})
        print(json.dumps({"rank": rank, **summary[-1]}), flush=True)
    elapsed = time.perf_counter() - t0
    if dist:
        gathered = [None] * world
        dist.all_gather_object(gathered, {"rank": rank, "elapsed_s": elapsed, "points": summary})
        dist.destroy_process_group()
    else:
        gathered = [{"rank": rank, "elapsed_s": elapsed, "points": summary}]
    if rank == 0:
        total = sum(p["seeds"] for g in gathered for p in g["points"]) * args.ep_len
        print(json.dumps({"sweep": {"points": len(points), "seeds": args.seeds, "ep_len": args.ep_len, "ranks": world,
                                    "platoon_steps": total, "elapsed_s": max(g["elapsed_s"] for g in gathered),
                                    "platoon_steps_per_s": total / max(g["elapsed_s"] for g in gathered)}}),
              flush=True)


if __name__ == "__main__":
    main()
