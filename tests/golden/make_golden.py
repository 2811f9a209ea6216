#!/usr/bin/env python3
"""Regenerate the committed golden fixtures (TEST INFRASTRUCTURE).

The reference cannot run in this container (Gurobi / dmpcpwa absent; importing the reference
was refused by the environment), so the expected outputs come from the CPU
oracle (oracle/hvp_oracle.c: exhaustive region-sequence enumeration + certified QP solves).
Inputs follow the reference's own generators, restated in oracle/oracle.py:
env.reset init with the SeedSequence-derived seed (env.py:70-116), constant-velocity neighbour
predictions (fleet_decent_mld.py:421-428), the leader trajectories of misc/leader_trajectory.py
and the controller constants of misc/common_controller_params.py.

Files (numpy .npz, no pickles):
  decent_n10_N5.npz   configs[1]: n=10, N=5, mass 800, ConstantSpacing(50), seeds 0..9, t=0
  decent_n2_N5.npz    configs[0]: n=2, N=5, seeds 0..9
  decent_rollout_n4_N5.npz  mid-trajectory states: 6 steps along the MPC's own predictions
  task2_n5_N5.npz     Sim_n_task_2 flavour: masses U(700,1000), ConstantTime(10,3), stop-and-go leader
  variants_n4.npz     N = 3, 4, 6, 7; Q_du = 0.5; leader_index = 2; real_vehicle_as_reference
  hard_n10_N5.npz     configs[1] instances (seed, vehicle) at degenerate QP vertices: weakly active /
                      linearly dependent rows, where an interior-point solve stalls.  Found by
                      scanning bench seeds 0..5999 for disagreements between the two QP methods of
                      the lane (active set vs interior point); expected values from the oracle.
  sweep_n*_N{10,15}.npz  configs[4] (C5 sweep) horizons beyond exhaustive enumeration: t=0 states and
                      mid-rollout states; expected values from the oracle's branch and bound
                      (oracle_set_method(1), cross-checked against its enumeration at N <= 10 by
                      tests/test_oracle.py); "method" = 1 marks them (node counts not comparable)
  known_answers.json  constants derived from the reference source

  gear_n4_N5.npz, gear_n5_N8.npz  LocalMpcGear on the pwa_friction model ("model" = 1):
                      (gear, friction region) modes, oracle gear_friction_mld_system
  admm_local_N{5,10}.npz, admm_steps_n4_N5.npz  naive ADMM (configs[2]): local problems with
                      copies, and 3 closed-loop time steps x 4 ADMM iterations (oracle coordinator)
  admm_gear_local_N5.npz, admm_gear_steps_n4_N5.npz  naive ADMM on the pwa_friction model
                      (fleet_naive_admm.py:261-288 LocalMpcGear): local problems on the oracle's
                      gear_friction_mld_system and 3 closed-loop steps x 4 iterations
  gadmm_local_N{5,10}.npz, gadmm_steps_n4_N5.npz, gadmm_steps_n3_N10.npz  switching ADMM
                      (fleet_g_admm.py, configs[3]): every local QP of oracle coordinator runs
                      (sampled), and two time steps of the restated coordinator (warm starts,
                      rollouts, rounds of ADMM + switching) for several platoons
  cent_*.npz          centralised MLD (mpcs/cent_mld.py MpcMldCent, fleet_cent_mld.py): one MIQP per
                      platoon from the oracle's joint branch and bound (oracle_solve_cent, cross-checked
                      against its exhaustive joint enumeration by tests/test_cent.py); n = 2..8 at N = 5,
                      n = 3 at N = 10, n = 10 at N = 3, variants (real_vehicle_as_reference, leader
                      index, task_2 masses / ConstantTime / stop-and-go, Q_du), mid-rollout states,
                      the gear model (MpcGearCent, model = 1)
  cent_l1_*.npz       centralised min_1_norm (the MILP-vs-MIQP study's controller, "quadratic" = 0):
                      n = 3 at N = 5, 6, 8, 10, n = 4, Q_du, real_vehicle_as_reference, leader index 1,
                      the gear model (MpcGearCent)
  l1_long_*_N{9,10}.npz  min_1_norm at the MILP-vs-MIQP study's longer horizons (oracle branch
                      and bound, "method" = 1, "quadratic" = 0): t = 0 states, Q_du, a rollout
  l1_long_n4_N{11,12,13,16}.npz  the seed-0 platoon's four local MILPs at the horizons where the
                      templated device code changes path (l1_horizons; tests/test_horizons.py)
  admm_horizon_N{8,9,12,13,16}.npz, admm_l1_horizon_N{9,12}.npz  naive ADMM around the node-record
                      edge: the first-iteration local problems of the seed-0 platoon, at N = 12 also of
                      five platoons whose leader ends in the top regions (admm_horizons)
  admm_l1_*.npz       naive ADMM with min_1_norm (LocalMpcADMM(quadratic_cost=False)): local problems
                      (incl. ConstantTime spacing), 3 closed-loop steps at n = 4, N = 5, and configs[2]'s
                      size (n = 10, N = 10, 20 iterations, 2 steps; "admm_l1 n10")
  l1stall_n10_N10.npz the four n = 10, N = 10 min_1_norm platoons (seeds 20, 549, 617, 667) holding a
                      local MILP whose node LPs stalled the interior point (HVP_MAXITER on a feasible
                      problem); "exp_unique" marks the instances whose LP optimum is a unique vertex
  l1batch_n10_N10.npz the benchmark's n = 10, N = 10 min_1_norm platoons (seeds 0..255), one vehicle
                      (seed % 10) each: oracle status, cost and sequence only (no params)
  event_*.npz         joint optima (cent_* layout) whose contiguous blocks are the local problems of the
                      event-based controller at long horizons (event_fixtures; tests/test_event_horizons.py)
Run:  python tests/golden/make_golden.py [sweep | gear | admm | admm_l1 [n10] | admm_gear | gadmm | cent [n10 | l1] | configs admm|gadmm
                                          | l1 | l1_rollout | l1_long | l1stall | l1batch | event [file ...]
                                          | l1_horizons [N ...] | admm_horizons [N ...]]
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle as O  # noqa: E402
from instances import (decent_instances, fast_leader_platoons, fast_leader_window, leader_window,  # noqa: E402
                       split_params)


def stop_and_go(N: int, t: int, p=3000.0, vh=20.0, vl=10.0, vf=30.0, c0=30, c1=50, L=200):
    x = np.zeros((2, L))
    x[:, 0] = (p, vh)
    v = vh
    for k in range(L - 1):
        x[0, k + 1] = x[0, k] + v
        if c0 <= k < c1:
            v = vl
        elif k >= c1:
            v = vf
        x[1, k + 1] = v if k >= c0 else x[1, k]
    return x[:, t:t + N + 1]


def solve_set(systems, masses_idx, cfg, N, params, roles, quadratic=True):
    out = {k: [] for k in ("region", "u", "x", "cost", "nodes", "status", "certified")}
    for p, r, si in zip(params, roles, masses_idx):
        x0, xf, xb, xl = split_params(p, N)
        res = O.solve_miqp(systems[si], cfg, N, int(r), x0, xf, xb, xl, quadratic=quadratic)
        out["region"].append(res.sigma if res.status == 0 else np.full(N, -1))
        out["u"].append(res.u)
        out["x"].append(res.x)
        out["cost"].append(res.cost)
        out["nodes"].append(res.n_candidates)
        out["status"].append(res.status)
        out["certified"].append(res.best_certified)
    return {k: np.array(v) for k, v in out.items()}


def save(name, N, masses, cfg, params, roles, sys_idx, exp, method=0, model=0, quadratic=1):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, N=N, masses=np.asarray(masses, float), cfg=cfg.vector(), params=params,
                        roles=roles.astype(np.int32), sys=np.asarray(sys_idx, np.int32), method=method, model=model,
                        quadratic=quadratic, **{f"exp_{k}": v for k, v in exp.items()})
    cert = exp["certified"][exp["status"] == 0].mean() if (exp["status"] == 0).any() else 0
    print(f"{name}: {len(roles)} instances, optimal {int((exp['status'] == 0).sum())}, certified {cert:.3f}")


def decent_seeds(n, N, seeds, mass=800.0, cfg=None, system=None, quadratic=True):
    cfg = cfg or O.Cfg()
    P, R = [], []
    for s in seeds:
        p, r = decent_instances(O.env_initial_state(n, s), N, leader_window(N))
        P.append(p)
        R.append(r)
    params, roles = np.concatenate(P), np.concatenate(R)
    sys_idx = np.zeros(len(roles), np.int32)
    system = system or O.gear_pwa_system(mass)
    return params, roles, sys_idx, solve_set([system], sys_idx, cfg, N, params, roles, quadratic)


def l1_fixtures():
    """min_1_norm (quadratic_cost=False, fleet_decent_mld.py:73-76): the local MILP optima of the
    oracle, whose L1 path is checked against HiGHS milp on the reference's big-M MLD
    (tests/test_oracle.py).  Files l1_*.npz carry quadratic = 0."""
    N = 5
    params, roles, si, exp = decent_seeds(10, N, range(4), quadratic=False)
    save("l1_decent_n10_N5.npz", N, [800.0], O.Cfg(), params, roles, si, exp, quadratic=0)
    cfg = O.Cfg(Qdu=0.5)
    params, roles, si, exp = decent_seeds(4, N, range(3), cfg=cfg, quadratic=False)
    save("l1_variant_n4_N5_qdu.npz", N, [800.0], cfg, params, roles, si, exp, quadratic=0)
    for NN in (3, 7):
        params, roles, si, exp = decent_seeds(3, NN, range(2), quadratic=False)
        save(f"l1_variant_n3_N{NN}.npz", NN, [800.0], O.Cfg(), params, roles, si, exp, quadratic=0)
    P, R = [], []
    for s in range(2):
        p, r = decent_instances(O.env_initial_state(5, s), N, leader_window(N), leader_index=2)
        P.append(p)
        R.append(r)
        p, r = decent_instances(O.env_initial_state(5, s + 10), N, leader_window(N, 0, 3100.0),
                                real_vehicle_as_reference=True)
        P.append(p)
        R.append(r)
    params, roles = np.concatenate(P), np.concatenate(R)
    si = np.zeros(len(roles), np.int32)
    cfg = O.Cfg(d0=10.0, t0=3.0)  # time-headway spacing (task_2): t0 enters every position error
    exp = solve_set([O.gear_pwa_system(800.0)], si, cfg, N, params, roles, quadratic=False)
    save("l1_roles_n5_N5.npz", N, [800.0], cfg, params, roles, si, exp, quadratic=0)
    g = O.gear_friction_mld_system(800.0)
    params, roles, si, exp = decent_seeds(4, N, range(2), system=g, quadratic=False)
    exp["gear"] = g["gear"][exp["region"]]
    save("l1_gear_n4_N5.npz", N, [800.0], O.Cfg(), params, roles, si, exp, model=1, quadratic=0)


def l1_rollout():
    """min_1_norm along the platoon's own L1 trajectories: mid-episode states, where the LP optima
    sit on region edges and ties between sequences are likeliest."""
    params, roles, si, exp = rollout(4, 5, range(3), 8, quadratic=False)
    save("l1_rollout_n4_N5.npz", 5, [800.0], O.Cfg(), params, roles, si, exp, quadratic=0)


def l1_long():
    """min_1_norm at the longer horizons of the reference's MILP-vs-MIQP study (N = 5..10,
    results_analysis/analyse_results_MILP_MIQP.py:9-12): the oracle's branch and bound (its L1 path
    at N = 9 agrees with its exhaustive enumeration on the seed-0 platoon: same sequences and costs,
    2437 / 7104 / 1399 / 1416 sequences against 29 / 31 / 86 / 46 node LPs)."""
    O.set_method(O.METHOD_BNB)
    try:
        params, roles, si, exp = decent_seeds(4, 9, range(3), quadratic=False)
        save("l1_long_n4_N9.npz", 9, [800.0], O.Cfg(), params, roles, si, exp, method=1, quadratic=0)
        params, roles, si, exp = decent_seeds(5, 10, range(3), quadratic=False)
        save("l1_long_n5_N10.npz", 10, [800.0], O.Cfg(), params, roles, si, exp, method=1, quadratic=0)
        cfg = O.Cfg(Qdu=0.5)
        params, roles, si, exp = decent_seeds(4, 10, range(2), cfg=cfg, quadratic=False)
        save("l1_long_qdu_n4_N10.npz", 10, [800.0], cfg, params, roles, si, exp, method=1, quadratic=0)
        params, roles, si, exp = rollout(4, 10, range(2), 4, quadratic=False)
        save("l1_long_rollout_n4_N10.npz", 10, [800.0], O.Cfg(), params, roles, si, exp, method=1, quadratic=0)
    finally:
        O.set_method(O.METHOD_ENUMERATE)


L1_HORIZONS = (11, 12, 13, 16)


def l1_horizons(only=()):
    """min_1_norm at the horizons where the templated code changes path (tests/test_horizons.py):
    N = 11, 12 (naive-ADMM node records, 48-bit codes), 13 (neither) and 16 (HVP_MAX_N, the code word
    full).  The four local MILPs of the seed-0 platoon (n = 4) each, the oracle's branch and bound, one
    process per instance.  Files l1_long_n4_N{11,12,13,16}.npz in the l1_long_* layout.
    Generation (wall clock on 8 cores, the four instances in parallel): N = 11 11 s, N = 12 23 s,
    N = 13 46 s, N = 16 868 s (all four instances: under the 20 minutes that would have cut it to two)."""
    import time

    for N in (only or L1_HORIZONS):
        t0 = time.time()
        p, r = decent_instances(O.env_initial_state(4, 0), N, leader_window(N))
        exp = _l1_bnb_solve(N, p, r)
        save(f"l1_long_n4_N{N}.npz", N, [800.0], O.Cfg(), p, r, np.zeros(len(r), np.int32), exp, method=1,
             quadratic=0)
        print(f"  N = {N}: {time.time() - t0:.0f} s", flush=True)


def _l1_bnb_init():
    O.set_method(O.METHOD_BNB)


def _l1_bnb_case(job):
    """One min_1_norm oracle solve by branch and bound (worker of l1_stall / l1_batch)."""
    N, p, r = job
    x0, xf, xb, xl = split_params(p, N)
    return O.solve_miqp(O.gear_pwa_system(800.0), O.Cfg(), N, int(r), x0, xf, xb, xl, quadratic=False)


def _l1_bnb_solve(N, params, roles):
    """solve_set's dictionary for min_1_norm instances, the oracle's branch and bound on every core."""
    from multiprocessing import Pool

    with Pool(min(16, os.cpu_count() or 1), initializer=_l1_bnb_init) as pool:
        res = pool.map(_l1_bnb_case, [(N, p, r) for p, r in zip(params, roles)], chunksize=1)
    return {"region": np.array([r.sigma if r.status == 0 else np.full(N, -1) for r in res]),
            "u": np.array([r.u for r in res]), "x": np.array([r.x for r in res]),
            "cost": np.array([r.cost for r in res]), "nodes": np.array([r.n_candidates for r in res]),
            "status": np.array([r.status for r in res]), "certified": np.array([r.best_certified for r in res])}


L1_STALL_SEEDS = (20, 549, 617, 667)  # platoons holding (seed, vehicle) (20, 1), (549, 6), (617, 4), (667, 7)


def l1_stall():
    """The n = 10, N = 10 min_1_norm platoons in which one local MILP (a slow front vehicle, a much
    faster back vehicle: active w = 1e4 safe-distance hinges, a degenerate LP optimum) has node LPs on
    which the interior point of hvp_l1.h stalled short of its stop test.  Whole platoons, oracle branch
    and bound.  exp_unique: the oracle's u equals (1e-8) the vertex HiGHS returns for the oracle's own
    LP of the winning sequence; false where the LP optimum is a face, whose points all price alike."""
    from scipy.optimize import linprog

    n = N = 10
    P, R = [], []
    for s in L1_STALL_SEEDS:
        p, r = decent_instances(O.env_initial_state(n, s), N, leader_window(N))
        P.append(p)
        R.append(r)
    params, roles = np.concatenate(P), np.concatenate(R)
    exp = _l1_bnb_solve(N, params, roles)
    assert (exp["status"] == 0).all(), exp["status"]
    g = O.gear_pwa_system(800.0)
    unique = np.zeros(len(roles), bool)
    for j, (p, r) in enumerate(zip(params, roles)):
        x0, xf, xb, xl = split_params(p, N)
        _, q, _, A, b, G, h = O.export_qp(g, O.Cfg(), N, int(r), exp["region"][j], x0, xf, xb, xl, quadratic=False)
        # HiGHS's choice ("highs", here its dual simplex) finds the oracle's own vertex even where the
        # optimum is a face (seed 549, vehicle 6: every u within 0.54 prices alike); its interior point
        # lands elsewhere on a face, so unique = both agree with the oracle
        unique[j] = True
        for method in ("highs", "highs-ipm"):
            lp = linprog(q, A_ub=G, b_ub=h, A_eq=A, b_eq=b, bounds=[(None, None)] * len(q), method=method)
            assert lp.status == 0, (j, lp.message)
            unique[j] &= np.abs(lp.x[2 * N:3 * N] - exp["u"][j]).max() <= 1e-8  # z = [x_1 .. x_N | u | ...]
    exp["unique"] = unique
    save("l1stall_n10_N10.npz", N, [800.0], O.Cfg(), params, roles, np.zeros(len(roles), np.int32), exp, method=1,
         quadratic=0)
    print("faces (exp_unique false):", [(L1_STALL_SEEDS[j // n], j % n) for j in np.flatnonzero(~unique)])


def l1_batch():
    """One vehicle (seed % 10, bench.cpu_baseline's sampling rule) of each of the 256 benchmark platoons
    (seeds 0..255, n = 10, N = 10, min_1_norm): the oracle's status, cost and sequence.  No params:
    the tests rebuild them (decent_instances)."""
    n = N = 10
    seeds = np.arange(256)
    index = seeds * n + seeds % n  # into the 2560 instances in platoon order
    P, R = [], []
    for s in seeds:
        p, r = decent_instances(O.env_initial_state(n, int(s)), N, leader_window(N))
        P.append(p[s % n])
        R.append(r[s % n])
    exp = _l1_bnb_solve(N, np.array(P), np.array(R))
    assert (exp["status"] == 0).all(), np.flatnonzero(exp["status"] != 0)
    np.savez_compressed(os.path.join(HERE, "l1batch_n10_N10.npz"), N=N, n=n, seeds=seeds.astype(np.int32),
                        index=index.astype(np.int32), exp_status=exp["status"].astype(np.int32),
                        exp_cost=exp["cost"], exp_region=exp["region"].astype(np.int32))
    print(f"l1batch_n10_N10.npz: {len(seeds)} instances, optimal {int((exp['status'] == 0).sum())}")


def gear_model():
    """LocalMpcGear on pwa_friction (mpcs/mpc_gear.py, fleet_decent_mld.py:226-253): model = 1.
    N = 5 by exhaustive enumeration (~1e3 mode sequences per vehicle), N = 8 by the oracle's
    branch and bound."""
    g = O.gear_friction_mld_system(800.0)
    params, roles, si, exp = decent_seeds(4, 5, range(4), system=g)
    exp["gear"] = g["gear"][exp["region"]]
    save("gear_n4_N5.npz", 5, [800.0], O.Cfg(), params, roles, si, exp, model=1)
    O.set_method(O.METHOD_BNB)
    try:
        params, roles, si, exp = decent_seeds(5, 8, range(2), system=g)
        exp["gear"] = g["gear"][exp["region"]]
        save("gear_n5_N8.npz", 8, [800.0], O.Cfg(), params, roles, si, exp, method=1, model=1)
    finally:
        O.set_method(O.METHOD_ENUMERATE)


def rollout(n, N, seeds, steps, quadratic=True):
    """States along the platoon's own predicted trajectories (x_1 of every local solution)."""
    cfg = O.Cfg()
    sysd = O.gear_pwa_system(800.0)
    P, R = [], []
    for s in seeds:
        state = O.env_initial_state(n, s).astype(float)
        for t in range(steps):
            p, r = decent_instances(state, N, leader_window(N, t))
            P.append(p)
            R.append(r)
            exp = solve_set([sysd], np.zeros(n, int), cfg, N, p, r, quadratic)
            state = np.stack([exp["x"][i][:, 1] if exp["status"][i] == 0 else state[2 * i:2 * i + 2]
                              for i in range(n)]).reshape(-1)
    params, roles = np.concatenate(P), np.concatenate(R)
    sys_idx = np.zeros(len(roles), np.int32)
    return params, roles, sys_idx, solve_set([sysd], sys_idx, cfg, N, params, roles, quadratic)


def task2(n, N, seeds, t_list):
    cfg = O.Cfg(d0=10.0, t0=3.0)
    P, R, S, masses = [], [], [], []
    for s in seeds:
        rs = np.random.RandomState(s)
        m = rs.uniform(700, 1000, n)
        base = len(masses)
        masses.extend(m.tolist())
        state = O.env_initial_state(n, s).astype(float)
        for t in t_list:
            p, r = decent_instances(state, N, stop_and_go(N, t))
            P.append(p)
            R.append(r)
            S.append(base + np.arange(n))
    params, roles, sys_idx = np.concatenate(P), np.concatenate(R), np.concatenate(S)
    systems = [O.gear_pwa_system(m) for m in masses]
    return params, roles, sys_idx, masses, cfg, solve_set(systems, sys_idx, cfg, N, params, roles)


# (seed, vehicle) pairs of hard_n10_N5.npz (see the module docstring)
HARD = [(250, 3), (257, 1), (354, 7), (428, 3), (574, 8), (774, 2), (1048, 6), (1259, 2), (1322, 4), (1509, 1),
        (1700, 6), (1717, 2), (1726, 4), (1740, 3), (1873, 7), (2089, 6), (2120, 7), (2366, 0), (2660, 6),
        (2758, 8), (2998, 9), (3194, 1), (3307, 8), (3333, 1), (3377, 6), (3444, 1), (3451, 8), (3454, 3),
        (3651, 7), (3660, 7), (3757, 5), (4250, 9), (4273, 9), (4320, 6), (4346, 3), (4526, 6), (4818, 9),
        (4911, 5), (4980, 2), (4992, 7), (5021, 8), (5104, 2), (5169, 3), (5336, 7), (5380, 4), (5419, 4),
        (5561, 4), (5744, 6), (5890, 5)]


def hard_cases(N=5, n=10):
    P, R = [], []
    for s, v in HARD:
        p, r = decent_instances(O.env_initial_state(n, s), N, leader_window(N))
        P.append(p[v:v + 1])
        R.append(r[v:v + 1])
    params, roles = np.concatenate(P), np.concatenate(R)
    sys_idx = np.zeros(len(roles), np.int32)
    return params, roles, sys_idx, solve_set([O.gear_pwa_system(800.0)], sys_idx, O.Cfg(), N, params, roles)


def sweep():
    """C5 sweep points with N = 10, 15 (oracle branch and bound)."""
    O.set_method(O.METHOD_BNB)
    try:
        for n, N, seeds in ((5, 10, range(4)), (10, 10, range(3)), (20, 10, range(1)), (5, 15, range(3)),
                            (10, 15, range(2)), (15, 15, range(1)), (20, 15, range(1))):
            params, roles, si, exp = decent_seeds(n, N, seeds)
            save(f"sweep_n{n}_N{N}.npz", N, [800.0], O.Cfg(), params, roles, si, exp, method=1)
        params, roles, si, exp = rollout(5, 10, range(2), 5)
        save("sweep_rollout_n5_N10.npz", 10, [800.0], O.Cfg(), params, roles, si, exp, method=1)
    finally:
        O.set_method(O.METHOD_ENUMERATE)


def admm_fixtures():
    """Naive ADMM (fleet_naive_admm.py, configs[2]): local problems with copies (random y, z
    around the neighbours' predictions) and two closed-loop ADMM time steps of a 4-vehicle
    platoon, all from the oracle (full (x, u, s, copies) space, branch and bound)."""
    rng = np.random.default_rng(7)
    sysd = O.gear_pwa_system(800.0)
    for N, seeds in ((5, range(4)), (10, range(2))):
        P, R, X, U, XF, XB, C, S, REG = [], [], [], [], [], [], [], [], []
        for seed in seeds:
            n = 4
            st = O.env_initial_state(n, seed).astype(float)
            for i in range(n):
                pred = lambda j: O.constant_velocity_prediction(st[2 * j], st[2 * j + 1], N)  # noqa: E731
                zf = pred(i - 1) + rng.normal(0, 3, (2, N + 1)) if i > 0 else np.zeros((2, N + 1))
                zb = pred(i + 1) + rng.normal(0, 3, (2, N + 1)) if i < n - 1 else np.zeros((2, N + 1))
                yf = rng.normal(0, 2, (2, N + 1)) if i > 0 else np.zeros((2, N + 1))
                yb = rng.normal(0, 2, (2, N + 1)) if i < n - 1 else np.zeros((2, N + 1))
                if seed == 0:  # the first time step of the reference: y = z = 0
                    yf, zf, yb, zb = (np.zeros((2, N + 1)),) * 4
                xl = leader_window(N) if i == 0 else np.zeros((2, N + 1))
                p = O.admm_params(st[2 * i:2 * i + 2], yf, zf, yb, zb, xl)
                r = O.solve_admm_miqp(sysd, O.Cfg(), N, O.role_bits(i, n), 0.5, p)
                P.append(p); R.append(O.role_bits(i, n)); X.append(r.x); U.append(r.u); XF.append(r.x_front)
                XB.append(r.x_back); C.append(r.cost); S.append(r.status); REG.append(r.sigma)
        np.savez_compressed(os.path.join(HERE, f"admm_local_N{N}.npz"), N=N, rho=0.5, params=np.array(P),
                            roles=np.array(R, np.int32), exp_x=np.array(X), exp_u=np.array(U), exp_xf=np.array(XF),
                            exp_xb=np.array(XB), exp_cost=np.array(C), exp_status=np.array(S, np.int32),
                            exp_region=np.array(REG, np.int32))
        print(f"admm_local_N{N}.npz: {len(R)} instances")
    # closed-loop ADMM steps (the state advances by the local solutions' x_1)
    n, N, iters = 4, 5, 4
    coord = O.AdmmCoordinator(sysd, O.Cfg(), N, n)
    st = O.env_initial_state(n, 3).astype(float)
    states, us, xs = [], [], []
    for t in range(3):
        coord.set_leader_x(leader_window(N, t))
        u, hist = coord.step(st, iters)
        states.append(st.copy()); us.append(np.array([[r.u for r in res] for res in hist]))
        xs.append(np.array([[r.x for r in res] for res in hist]))
        st = np.concatenate([r.x[:, 1] for r in hist[-1]])
    np.savez_compressed(os.path.join(HERE, "admm_steps_n4_N5.npz"), N=N, n=n, iters=iters, rho=0.5,
                        states=np.array(states), exp_u=np.array(us), exp_x=np.array(xs))
    print("admm_steps_n4_N5.npz written")


def admm_l1_fixtures(big: bool = False):
    """Naive ADMM with min_1_norm (LocalMpcADMM(quadratic_cost=False), fleet_naive_admm.py:74-77):
    L1 tracking / input terms next to the quadratic ADMM terms of the copies, from the oracle
    (full (x, u, s, copies) space, branch and bound, KKT-certified QPs).
      admm_l1_local_N{5,10}.npz    local problems as admm_local_* (random y, z; seed 0: y = z = 0)
      admm_l1_local_ct_N5.npz      the same with ConstantTime(10, 3) spacing (t0 != 0: the back
                                   copy's position error involves its velocity, task_2's policy)
      admm_l1_steps_n4_N5.npz      3 closed-loop time steps x 4 ADMM iterations (oracle coordinator)
      admm_l1_steps_n10_N10.npz    (big) configs[2]'s size: n = 10, N = 10, 20 iterations, 2 steps"""
    import multiprocessing as mp

    sysd = O.gear_pwa_system(800.0)
    ctx = mp.get_context("spawn")
    with ctx.Pool(min(8, os.cpu_count() or 1)) as pool:
        if big:
            n, N, iters = 10, 10, 20
            coord = O.AdmmCoordinator(sysd, O.Cfg(), N, n, quadratic=False)
            st = O.env_initial_state(n, 0).astype(float)
            states, us, xs = [], [], []
            for t in range(2):
                coord.set_leader_x(leader_window(N, t))
                u, hist = coord.step(st, iters, pool=pool)
                states.append(st.copy()); us.append(np.array([[r.u for r in res] for res in hist]))
                xs.append(np.array([[r.x for r in res] for res in hist]))
                st = np.concatenate([r.x[:, 1] for r in hist[-1]])
                print(f"admm l1 step {t} done", flush=True)
            np.savez_compressed(os.path.join(HERE, f"admm_l1_steps_n{n}_N{N}.npz"), N=N, n=n, iters=iters, rho=0.5,
                                quadratic=0, states=np.array(states), exp_u=np.array(us), exp_x=np.array(xs),
                                exp_region=np.array([[r.sigma for r in hist[-1]]]))
            print(f"admm_l1_steps_n{n}_N{N}.npz written")
            return
        rng = np.random.default_rng(17)
        for name, N, seeds, cfg in (("admm_l1_local_N5", 5, range(4), O.Cfg()),
                                    ("admm_l1_local_N10", 10, range(2), O.Cfg()),
                                    ("admm_l1_local_ct_N5", 5, range(1, 3), O.Cfg(d0=10.0, t0=3.0))):
            P, R = [], []
            for seed in seeds:
                n = 4
                st = O.env_initial_state(n, seed).astype(float)
                for i in range(n):
                    pred = lambda j: O.constant_velocity_prediction(st[2 * j], st[2 * j + 1], N)  # noqa: E731
                    zf = pred(i - 1) + rng.normal(0, 3, (2, N + 1)) if i > 0 else np.zeros((2, N + 1))
                    zb = pred(i + 1) + rng.normal(0, 3, (2, N + 1)) if i < n - 1 else np.zeros((2, N + 1))
                    yf = rng.normal(0, 2, (2, N + 1)) if i > 0 else np.zeros((2, N + 1))
                    yb = rng.normal(0, 2, (2, N + 1)) if i < n - 1 else np.zeros((2, N + 1))
                    if seed == 0:  # the first time step of the reference: y = z = 0
                        yf, zf, yb, zb = (np.zeros((2, N + 1)),) * 4
                    xl = leader_window(N) if i == 0 else np.zeros((2, N + 1))
                    P.append(O.admm_params(st[2 * i:2 * i + 2], yf, zf, yb, zb, xl))
                    R.append(O.role_bits(i, n))
            res = pool.starmap(O.solve_admm_miqp, [(sysd, cfg, N, r, 0.5, p, 200, False) for r, p in zip(R, P)])
            np.savez_compressed(os.path.join(HERE, f"{name}.npz"), N=N, rho=0.5, quadratic=0, cfg=cfg.vector(),
                                params=np.array(P), roles=np.array(R, np.int32),
                                exp_x=np.array([r.x for r in res]), exp_u=np.array([r.u for r in res]),
                                exp_xf=np.array([r.x_front for r in res]), exp_xb=np.array([r.x_back for r in res]),
                                exp_cost=np.array([r.cost for r in res]),
                                exp_status=np.array([r.status for r in res], np.int32),
                                exp_cert=np.array([r.certified for r in res]),
                                exp_region=np.array([r.sigma for r in res], np.int32))
            print(f"{name}.npz: {len(R)} instances", flush=True)
        n, N, iters = 4, 5, 4
        coord = O.AdmmCoordinator(sysd, O.Cfg(), N, n, quadratic=False)
        st = O.env_initial_state(n, 3).astype(float)
        states, us, xs, regs = [], [], [], []
        for t in range(3):
            coord.set_leader_x(leader_window(N, t))
            u, hist = coord.step(st, iters, pool=pool)
            states.append(st.copy()); us.append(np.array([[r.u for r in res] for res in hist]))
            xs.append(np.array([[r.x for r in res] for res in hist]))
            regs.append(np.array([[r.sigma for r in res] for res in hist]))
            st = np.concatenate([r.x[:, 1] for r in hist[-1]])
        np.savez_compressed(os.path.join(HERE, "admm_l1_steps_n4_N5.npz"), N=N, n=n, iters=iters, rho=0.5,
                            quadratic=0, states=np.array(states), exp_u=np.array(us), exp_x=np.array(xs),
                            exp_region=np.array(regs, np.int32))
        print("admm_l1_steps_n4_N5.npz written")


ADMM_HORIZONS = (8, 9, 12, 13, 16)
ADMM_L1_HORIZONS = (9, 12)


def _admm_case(job):
    N, role, p, quadratic = job
    return O.solve_admm_miqp(O.gear_pwa_system(800.0), O.Cfg(), N, role, 0.5, p, 200, quadratic)


def admm_horizons(only=()):
    """Naive ADMM at the horizons around the node-record edge (tests/test_horizons.py): the local
    problems of the FIRST ADMM iteration of a time step (y = z = 0, fleet_naive_admm.py:379-419) of
    the seed-0 platoon (n = 4), in the admm_local_* layout.  admm_horizon_N{8,9,12,13,16}.npz
    (quadratic; N = 12 also holds the five fast_leader_platoons, "n_seed" = 4 marks where they start)
    and admm_l1_horizon_N{9,12}.npz (min_1_norm).  Generation (wall clock, 4 processes): quadratic
    under 1 / 1 / 7 / 3 / 5 s; min_1_norm 14 s and 32 s."""
    import time
    from multiprocessing import Pool

    with Pool(min(4, os.cpu_count() or 1)) as pool:
        for quadratic, horizons in ((True, ADMM_HORIZONS), (False, ADMM_L1_HORIZONS)):
            for N in horizons:
                if only and N not in only:
                    continue
                t0 = time.time()
                zero = np.zeros((2, N + 1))
                platoons = [(O.env_initial_state(4, 0).astype(float), leader_window(N))]
                if quadratic and N == 12:
                    platoons += [(st, fast_leader_window(N, st[0])) for st in fast_leader_platoons()]
                P, R = [], []
                for st, lead in platoons:
                    for i in range(4):
                        P.append(O.admm_params(st[2 * i:2 * i + 2], zero, zero, zero, zero, lead if i == 0 else zero))
                        R.append(O.role_bits(i, 4))
                res = pool.map(_admm_case, [(N, r, p, quadratic) for r, p in zip(R, P)], chunksize=1)
                name = f"admm_horizon_N{N}.npz" if quadratic else f"admm_l1_horizon_N{N}.npz"
                np.savez_compressed(os.path.join(HERE, name), N=N, rho=0.5, quadratic=int(quadratic), n_seed=4,
                                    cfg=O.Cfg().vector(), params=np.array(P), roles=np.array(R, np.int32),
                                    exp_x=np.array([r.x for r in res]), exp_u=np.array([r.u for r in res]),
                                    exp_xf=np.array([r.x_front for r in res]),
                                    exp_xb=np.array([r.x_back for r in res]),
                                    exp_cost=np.array([r.cost for r in res]),
                                    exp_status=np.array([r.status for r in res], np.int32),
                                    exp_cert=np.array([r.certified for r in res]),
                                    exp_region=np.array([r.sigma for r in res], np.int32))
                print(f"{name}: {len(R)} instances, optimal {sum(r.status == 0 for r in res)}, "
                      f"{time.time() - t0:.0f} s", flush=True)


def admm_gear_fixtures():
    """Naive ADMM with LocalMpcGear (fleet_naive_admm.py:261-288, selected for pwa_friction at
    :632-633): the local problem's modes are (gear, friction region) pairs (oracle
    gear_friction_mld_system, as for the decentralised gear fixtures); the same local-problem and
    closed-loop sets as admm_fixtures."""
    rng = np.random.default_rng(11)
    sysd = O.gear_friction_mld_system(800.0)
    N = 5
    P, R, X, U, XF, XB, C, S, REG = [], [], [], [], [], [], [], [], []
    for seed in range(3):
        n = 4
        st = O.env_initial_state(n, seed).astype(float)
        for i in range(n):
            pred = lambda j: O.constant_velocity_prediction(st[2 * j], st[2 * j + 1], N)  # noqa: E731
            zf = pred(i - 1) + rng.normal(0, 3, (2, N + 1)) if i > 0 else np.zeros((2, N + 1))
            zb = pred(i + 1) + rng.normal(0, 3, (2, N + 1)) if i < n - 1 else np.zeros((2, N + 1))
            yf = rng.normal(0, 2, (2, N + 1)) if i > 0 else np.zeros((2, N + 1))
            yb = rng.normal(0, 2, (2, N + 1)) if i < n - 1 else np.zeros((2, N + 1))
            if seed == 0:
                yf, zf, yb, zb = (np.zeros((2, N + 1)),) * 4
            xl = leader_window(N) if i == 0 else np.zeros((2, N + 1))
            p = O.admm_params(st[2 * i:2 * i + 2], yf, zf, yb, zb, xl)
            r = O.solve_admm_miqp(sysd, O.Cfg(), N, O.role_bits(i, n), 0.5, p)
            P.append(p); R.append(O.role_bits(i, n)); X.append(r.x); U.append(r.u); XF.append(r.x_front)
            XB.append(r.x_back); C.append(r.cost); S.append(r.status); REG.append(r.sigma)
    np.savez_compressed(os.path.join(HERE, "admm_gear_local_N5.npz"), N=N, rho=0.5, params=np.array(P),
                        roles=np.array(R, np.int32), exp_x=np.array(X), exp_u=np.array(U), exp_xf=np.array(XF),
                        exp_xb=np.array(XB), exp_cost=np.array(C), exp_status=np.array(S, np.int32),
                        exp_region=np.array(REG, np.int32), exp_gear=np.asarray(sysd["gear"])[np.array(REG)])
    print(f"admm_gear_local_N5.npz: {len(R)} instances")
    n, iters = 4, 4
    coord = O.AdmmCoordinator(sysd, O.Cfg(), N, n)
    st = O.env_initial_state(n, 3).astype(float)
    states, us, xs, gs = [], [], [], []
    for t in range(3):
        coord.set_leader_x(leader_window(N, t))
        u, hist = coord.step(st, iters)
        states.append(st.copy()); us.append(np.array([[r.u for r in res] for res in hist]))
        xs.append(np.array([[r.x for r in res] for res in hist]))
        gs.append(np.array([np.asarray(sysd["gear"])[r.sigma] for r in hist[-1]]))
        st = np.concatenate([r.x[:, 1] for r in hist[-1]])
    np.savez_compressed(os.path.join(HERE, "admm_gear_steps_n4_N5.npz"), N=N, n=n, iters=iters, rho=0.5,
                        states=np.array(states), exp_u=np.array(us), exp_x=np.array(xs), exp_gear=np.array(gs))
    print("admm_gear_steps_n4_N5.npz written")


def config_size_fixtures(which: str):
    """configs[2] and configs[3] at their own sizes: the oracle coordinators on
    t = 0 platoon states for two consecutive time steps (the state advances along the solution's
    x_1; the coordinator state -- naive ADMM's y, switching ADMM's previous solution -- carries
    over, fleet_naive_admm.py:357-359, fleet_g_admm.py:265-272).
      admm:  fleet_naive_admm n = 10, N = 10, 20 ADMM iterations, one seed  -> admm_steps_n10_N10.npz
      gadmm: fleet_g_admm n = 20, N = 10, 100 ADMM iterations, two seeds  -> gadmm_steps_n20_N10.npz"""
    if which == "admm":
        n, N, iters = 10, 10, 20
        sysd = O.gear_pwa_system(800.0)
        coord = O.AdmmCoordinator(sysd, O.Cfg(), N, n)
        st = O.env_initial_state(n, 0).astype(float)
        states, us, xs = [], [], []
        for t in range(2):
            coord.set_leader_x(leader_window(N, t))
            u, hist = coord.step(st, iters)
            states.append(st.copy()); us.append(np.array([[r.u for r in res] for res in hist]))
            xs.append(np.array([[r.x for r in res] for res in hist]))
            st = np.concatenate([r.x[:, 1] for r in hist[-1]])
            print(f"admm step {t} done", flush=True)
        np.savez_compressed(os.path.join(HERE, f"admm_steps_n{n}_N{N}.npz"), N=N, n=n, iters=iters, rho=0.5,
                            states=np.array(states), exp_u=np.array(us), exp_x=np.array(xs))
        print(f"admm_steps_n{n}_N{N}.npz written")
        return
    n, N, iters = 20, 10, 100
    systems = [O.gear_pwa_system(800.0) for _ in range(n)]
    co = O.GAdmmCoordinator(systems, O.Cfg(), N, admm_iters=iters)
    states, exp_u, exp_cost, exp_ws, exp_rounds, exp_seq, exp_runcost = [], [], [], [], [], [], []
    for seed in range(2):
        co.prev_u = None
        st = O.env_initial_state(n, seed).astype(float)
        for t in range(2):
            co.set_leader_traj(leader_window(N, t))
            u, c, runs = co.control(st)
            ws = next(k for k, r in enumerate(runs) if r is not None and r[1] == c)
            states.append(st.copy()); exp_u.append(u); exp_cost.append(c); exp_ws.append(ws + 1)
            exp_rounds.append([r[2]["rounds"] if r else -1 for r in runs] + [-1] * (2 - len(runs)))
            exp_seq.append([r[2]["sigma"] if r else np.full((n, N), -1) for r in runs] +
                           [np.full((n, N), -1)] * (2 - len(runs)))
            exp_runcost.append([r[1] if r else np.inf for r in runs] + [np.nan] * (2 - len(runs)))
            st = np.concatenate([runs[ws][2]["x"][i][:, 1] for i in range(n)])
            print(f"gadmm seed {seed} step {t} done", flush=True)
    name = f"gadmm_steps_n{n}_N{N}.npz"
    np.savez_compressed(os.path.join(HERE, name), N=N, n=n, iters=iters, rho=0.5, max_rounds=co.max_rounds,
                        steps=2, states=np.array(states), exp_u=np.array(exp_u), exp_cost=np.array(exp_cost),
                        exp_warm_start=np.array(exp_ws, np.int32), exp_rounds=np.array(exp_rounds, np.int32),
                        exp_seq=np.array(exp_seq, np.int32), exp_run_cost=np.array(exp_runcost))
    print(f"{name}: {len(states)} coordinator calls")


def gadmm_fixtures():
    """Switching ADMM (fleet_g_admm.py, configs[3]): the oracle's restated coordinator
    (oracle.py GAdmmCoordinator) on t = 0 platoon states; every local QP it solves is traced and
    a sample kept as local-problem fixtures; two consecutive time steps (the state advances
    along the winner's predicted x_1, the second step has both warm starts) as coordinator
    fixtures."""
    rng = np.random.default_rng(11)
    for N, n, iters, seeds in ((5, 4, 20, range(4)), (10, 3, 10, range(3))):
        systems = [O.gear_pwa_system(800.0) for _ in range(n)]
        co = O.GAdmmCoordinator(systems, O.Cfg(), N, admm_iters=iters)
        co.trace = []
        states, exp_u, exp_cost, exp_ws, exp_rounds, exp_seq, exp_runcost = [], [], [], [], [], [], []
        for seed in seeds:
            co.prev_u = None
            st = O.env_initial_state(n, seed).astype(float)
            for t in range(2):
                co.set_leader_traj(leader_window(N, t))
                u, c, runs = co.control(st)
                ws = next(k for k, r in enumerate(runs) if r is not None and r[1] == c)
                states.append(st.copy()); exp_u.append(u); exp_cost.append(c); exp_ws.append(ws + 1)
                exp_rounds.append([r[2]["rounds"] if r else -1 for r in runs] + [-1] * (2 - len(runs)))
                exp_seq.append([r[2]["sigma"] if r else np.full((n, N), -1) for r in runs] +
                               [np.full((n, N), -1)] * (2 - len(runs)))
                exp_runcost.append([r[1] if r else np.inf for r in runs] + [np.nan] * (2 - len(runs)))
                st = np.concatenate([runs[ws][2]["x"][i][:, 1] for i in range(n)])
        name = f"gadmm_steps_n{n}_N{N}.npz"
        np.savez_compressed(os.path.join(HERE, name), N=N, n=n, iters=iters, rho=0.5, max_rounds=co.max_rounds,
                            steps=2, states=np.array(states), exp_u=np.array(exp_u), exp_cost=np.array(exp_cost),
                            exp_warm_start=np.array(exp_ws, np.int32), exp_rounds=np.array(exp_rounds, np.int32),
                            exp_seq=np.array(exp_seq, np.int32), exp_run_cost=np.array(exp_runcost))
        print(f"{name}: {len(states)} coordinator calls")
        T = co.trace
        keep = np.sort(rng.choice(len(T), size=min(300, len(T)), replace=False))
        T = [T[k] for k in keep]
        roles = np.array([t[1] | (64 if t[2] else 0) for t in T], np.int32)
        np.savez_compressed(os.path.join(HERE, f"gadmm_local_N{N}.npz"), N=N, rho=0.5,
                            params=np.stack([t[3] for t in T]), roles=roles,
                            seq=np.stack([t[4] for t in T]).astype(np.int32),
                            exp_u=np.stack([t[5].u for t in T]), exp_x=np.stack([t[5].x for t in T]),
                            exp_xf=np.stack([t[5].x_front for t in T]), exp_xb=np.stack([t[5].x_back for t in T]),
                            exp_cost=np.array([t[5].cost for t in T]),
                            exp_status=np.array([t[5].status for t in T], np.int32),
                            exp_edge=np.array([t[5].switch for t in T], np.int64))
        print(f"gadmm_local_N{N}.npz: {len(T)} local QPs, {int((roles & 64).sum() // 64)} with a back copy")


def _cent_case(job):
    """One oracle solve of the centralised MIQP (worker of cent_fixtures)."""
    masses, model, cfg, N, x0, lead, leader_index, lsp = job[:8]
    quadratic = job[8] if len(job) > 8 else True
    systems = [O.gear_friction_mld_system(m) if model == 1 else O.gear_pwa_system(m) for m in masses]
    r = O.solve_cent(systems, cfg, N, x0, lead, leader_index, lsp, quadratic=quadratic)
    gear = np.array([systems[i]["gear"][r.sigma[i]] for i in range(len(masses))]) if r.status == 0 else None
    return r, gear


def cent_save(name, N, jobs, results, cfg, model=0):
    n = len(jobs[0][0])
    ok = [r.status == 0 for r, _ in results]
    np.savez_compressed(
        os.path.join(HERE, name), N=N, n=n, model=model, cfg=cfg.vector(),
        masses=np.array([j[0] for j in jobs], float), x0=np.array([np.reshape(j[4], (n, 2)) for j in jobs]),
        leader_x=np.array([j[5] for j in jobs]), leader_index=np.array([j[6] for j in jobs], np.int32),
        lsp=np.array([int(j[7]) for j in jobs], np.int32),
        exp_status=np.array([r.status for r, _ in results], np.int32),
        exp_region=np.array([r.sigma if r.status == 0 else np.full((n, N), -1) for r, _ in results], np.int32),
        exp_gear=np.array([g if g is not None else np.zeros((n, N), int) for _, g in results], np.int32),
        exp_u=np.array([r.u for r, _ in results]), exp_x=np.array([r.x for r, _ in results]),
        exp_cost=np.array([r.cost for r, _ in results]), exp_nodes=np.array([r.n_qps for r, _ in results], np.int32),
        quadratic=int(jobs[0][8]) if len(jobs[0]) > 8 else 1)
    print(f"{name}: {len(jobs)} platoons, optimal {sum(ok)}, QPs {[r.n_qps for r, _ in results]}", flush=True)


def cent_fixtures(big: bool = False):
    """Centralised MLD (configs: fleet_cent_mld.py): see the module docstring."""
    from multiprocessing import Pool

    def seeds_jobs(n, N, seeds, cfg=None, masses=None, model=0, leader_index=0, lsp=False, lead=None, quadratic=True):
        jobs = []
        for s in seeds:
            m = masses(s) if callable(masses) else [800.0] * n
            jobs.append((m, model, cfg or O.Cfg(), N, O.env_initial_state(n, s).astype(float),
                         leader_window(N) if lead is None else lead, leader_index, lsp, quadratic))
        return jobs

    def rollout_jobs(n, N, seeds, steps):
        jobs = []
        for s in seeds:
            st = O.env_initial_state(n, s).astype(float)
            for t in range(steps):
                job = ([800.0] * n, 0, O.Cfg(), N, st.copy(), leader_window(N, t), 0, False)
                jobs.append(job)
                r, _ = _cent_case(job)
                if r.status != 0:
                    break
                st = r.x[:, :, 1].reshape(-1)  # along the controller's own prediction
        return jobs

    rng_mass = lambda s: np.random.RandomState(s).uniform(700, 1000, 5).tolist()  # noqa: E731
    if big == "l1":
        # min_1_norm (the MILP of the reference's MILP-vs-MIQP study, fleet_cent_mld.py:137-175 with
        # Sim's n = 3 and N = 5..10): "quadratic" = 0.  N = 10 is left out: the oracle's joint
        # search did not finish one n = 3, N = 10 platoon in 75 minutes.  Files already present are
        # kept (the oracle takes minutes per N = 8 platoon).
        sets = [
            ("cent_l1_n3_N5.npz", 5, seeds_jobs(3, 5, range(4), quadratic=False), O.Cfg(), 0),
            ("cent_l1_n3_N6.npz", 6, seeds_jobs(3, 6, range(3), quadratic=False), O.Cfg(), 0),
            ("cent_l1_n3_N8.npz", 8, seeds_jobs(3, 8, range(2), quadratic=False), O.Cfg(), 0),
            ("cent_l1_n4_N5.npz", 5, seeds_jobs(4, 5, range(3), quadratic=False), O.Cfg(), 0),
            ("cent_l1_qdu_n3_N5.npz", 5, seeds_jobs(3, 5, range(2), cfg=O.Cfg(Qdu=0.5), quadratic=False),
             O.Cfg(Qdu=0.5), 0),
            ("cent_l1_lsp_n3_N5.npz", 5, seeds_jobs(3, 5, range(2), lsp=True, quadratic=False), O.Cfg(), 0),
            ("cent_l1_lead1_n3_N5.npz", 5, seeds_jobs(3, 5, range(2), leader_index=1, quadratic=False), O.Cfg(), 0),
            ("cent_l1_gear_n2_N4.npz", 4, seeds_jobs(2, 4, range(2), model=1, quadratic=False), O.Cfg(), 1),
        ]
    elif big:
        sets = [("cent_n10_N5.npz", 5, seeds_jobs(10, 5, range(4)), O.Cfg(), 0)]  # ~1.5 min per platoon
    else:
        sets = [
            ("cent_n2_N5.npz", 5, seeds_jobs(2, 5, range(10)), O.Cfg(), 0),
            ("cent_n4_N5.npz", 5, seeds_jobs(4, 5, range(6)), O.Cfg(), 0),
            ("cent_n6_N5.npz", 5, seeds_jobs(6, 5, range(4)), O.Cfg(), 0),
            ("cent_n8_N5.npz", 5, seeds_jobs(8, 5, range(1)), O.Cfg(), 0),
            ("cent_n3_N10.npz", 10, seeds_jobs(3, 10, range(2)), O.Cfg(), 0),
            ("cent_n10_N3.npz", 3, seeds_jobs(10, 3, range(4)), O.Cfg(), 0),
            ("cent_lsp_n4_N5.npz", 5, seeds_jobs(4, 5, range(3), lsp=True), O.Cfg(), 0),
            ("cent_lead2_n4_N5.npz", 5, seeds_jobs(4, 5, range(3), leader_index=2), O.Cfg(), 0),
            ("cent_qdu_n4_N5.npz", 5, seeds_jobs(4, 5, range(3), cfg=O.Cfg(Qdu=0.5)), O.Cfg(Qdu=0.5), 0),
            ("cent_task2_n5_N5.npz", 5, seeds_jobs(5, 5, range(3), cfg=O.Cfg(d0=10.0, t0=3.0), masses=rng_mass,
                                                   lead=stop_and_go(5, 29)), O.Cfg(d0=10.0, t0=3.0), 0),
            ("cent_rollout_n4_N5.npz", 5, rollout_jobs(4, 5, range(2), 4), O.Cfg(), 0),
            ("cent_gear_n3_N4.npz", 4, seeds_jobs(3, 4, range(3), model=1), O.Cfg(), 1),
        ]
    only = set(os.environ.get("CENT_ONLY", "").split(",")) - {""}
    sets = [x for x in sets if not only or x[0] in only]
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        pending = [[pool.apply_async(_cent_case, (j,)) for j in jobs] for _, _, jobs, _, _ in sets]
        for (name, N, jobs, cfg, model), futs in zip(sets, pending):  # each set saved as it completes
            cent_save(name, N, jobs, [f.get() for f in futs], cfg, model)


# event_* sets: (file, n, N, model, [(seed, leader_index), ...], wall-clock budget in seconds from the
# start of the run; the n = 5, N = 11 set: 20 minutes over all its seeds).  Oracle time per platoon when the
# sets were made (8 cores, all 22 solves in flight): N = 6 under 1 s; n = 3, N = 11 4-7 s; n = 3, N = 16
# 24 / 43 / 31 / 14 s; n = 4 4-17 s (N = 8), 29 / 36 s (N = 12), 74 s (N = 16); n = 5 16 / 65 s (N = 8) and
# 131 / 105 s (N = 11); the gear model 37 / 188 s.  Seeds known not to finish in 270 s are not listed
# (n = 3, N = 16: 0, 5; n = 4, N = 12 and 16: 0; n = 4, N = 16: 2; n = 5, N = 8: 0); n = 3, N = 16 seeds
# (4, leader 0) and (3, leader 1) finish in 161 / 132 s, n = 5, N = 11 seed 2 in 238 s, and are left
# out to keep the batches of the GPU test at two dozen wavefronts.
EVENT_SETS = (
    ("event_n3_N6.npz", 3, 6, 0, [(1, 0), (2, 1), (3, 2)], 600),
    ("event_n3_N11.npz", 3, 11, 0, [(1, 0), (3, 1), (2, 2)], 600),
    ("event_n3_N16.npz", 3, 16, 0, [(1, 0), (3, 0), (1, 1), (2, 2)], 900),
    ("event_n4_N8.npz", 4, 8, 0, [(1, 0), (3, 2), (2, 1)], 600),
    ("event_n4_N12.npz", 4, 12, 0, [(1, 0), (3, 1)], 600),
    ("event_n4_N16.npz", 4, 16, 0, [(1, 0)], 900),
    ("event_n5_N8.npz", 5, 8, 0, [(1, 0), (2, 3)], 600),
    ("event_n5_N11.npz", 5, 11, 0, [(1, 0), (3, 0)], 1200),
    ("event_gear_n4_N4.npz", 4, 4, 1, [(0, 0), (1, 2)], 600),
)


def _edge_steps(systems, r, tol=1e-6):
    """(vehicle, step) pairs of a joint optimum whose velocity sits on the friction edge alpha: the two
    modes that meet there (regions 3 and 4 of the gear PWA model, the two friction regions of a gear)
    share the gear, so their dynamics coincide at the edge and the sequences through either cost the
    same; which one a solver of a SUB-problem returns is its tie rule, not the optimum.  (At every other
    band edge the input gain changes with the gear: a step there is an active row, not a tie.)
    Platoons with such a step are left out of the event_* sets."""
    alpha = float(O.friction_pwa_system(800.0)["T"][0][0])  # the edge does not depend on the mass
    return [(i, k) for i in range(len(systems)) for k in range(1, r.x.shape[2] - 1)
            if abs(r.x[i, 1, k] - alpha) <= tol]


def event_fixtures(only=()):
    """Joint optima for the event-based controller's long-horizon checks (tests/test_event_horizons.py):
    the local problem over vehicles [lo, lo + m) of a centralised optimum, every other vehicle held at
    its optimal trajectory, is the local MIQP of include/hvp_event.h, so one joint optimum pins every
    contiguous block with m = 1, 2, 3.  Centralised fixtures in the cent_* layout (cent_save) with
    Cfg(d0 = 10, t0 = 3), per-vehicle masses RandomState(seed).uniform(700, 1000, 5)[:n] and the leader
    window leader_window(N, p0 = x0[2 L] + 30, v = 20); event_gear_n4_N4.npz on the (gear,
    friction-region) tables (model = 1).  A platoon that does not finish inside its set's budget, is not
    optimal or has a step on a band edge (_edge_steps) is reported and left out."""
    import time
    from multiprocessing import Pool

    cfg = O.Cfg(d0=10.0, t0=3.0)
    sets = [s for s in EVENT_SETS if not only or s[0] in only]
    t0 = time.time()
    pool = Pool(min(8, os.cpu_count() or 1))
    try:
        pending = []
        for name, n, N, model, platoons, _ in sets:
            jobs = []
            for seed, L in platoons:
                x0 = O.env_initial_state(n, seed).astype(float)
                masses = np.random.RandomState(seed).uniform(700, 1000, 5)[:n].tolist()
                jobs.append((masses, model, cfg, N, x0, leader_window(N, p0=x0[2 * L] + 30.0, v=20.0), L, False))
            pending.append((jobs, [pool.apply_async(_timed_cent_case, (j,)) for j in jobs]))
        for (name, n, N, model, platoons, budget), (jobs, futs) in zip(sets, pending):
            keep_jobs, keep_res = [], []
            for (seed, L), job, f in zip(platoons, jobs, futs):
                try:
                    (r, gear), dt = f.get(timeout=max(1.0, t0 + budget - time.time()))
                except Exception as e:  # multiprocessing.TimeoutError
                    print(f"  {name}: seed {seed}, leader {L}: not finished inside {budget} s ({type(e).__name__})", flush=True)
                    continue
                systems = [O.gear_friction_mld_system(m) if model == 1 else O.gear_pwa_system(m) for m in job[0]]
                edges = _edge_steps(systems, r) if r.status == 0 else []
                print(f"  {name}: seed {seed}, leader {L}: status {r.status}, {r.n_qps} QPs, {dt:.0f} s"
                      + (f", band-edge steps {edges}: left out" if edges else ""), flush=True)
                if r.status == 0 and not edges:
                    keep_jobs.append(job)
                    keep_res.append((r, gear))
            if keep_jobs:
                cent_save(name, N, keep_jobs, keep_res, cfg, model)  # each set saved as it completes
            else:
                print(f"{name}: no platoon finished; nothing written", flush=True)
    finally:
        pool.terminate()


def _timed_cent_case(job):
    import time

    t0 = time.time()
    return _cent_case(job), time.time() - t0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "event":
        event_fixtures(set(sys.argv[2:]))
        return
    if len(sys.argv) > 1 and sys.argv[1] == "cent":
        cent_fixtures(big=sys.argv[2] if len(sys.argv) > 2 else False)  # n10 | l1
        return
    if len(sys.argv) > 2 and sys.argv[1] == "configs":
        config_size_fixtures(sys.argv[2])
        return
    if len(sys.argv) > 1 and sys.argv[1] == "gadmm":
        gadmm_fixtures()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "admm":
        admm_fixtures()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "admm_l1":
        admm_l1_fixtures(big=len(sys.argv) > 2 and sys.argv[2] == "n10")
        return
    if len(sys.argv) > 1 and sys.argv[1] == "admm_gear":
        admm_gear_fixtures()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "sweep":
        sweep()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "gear":
        gear_model()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "l1":
        l1_fixtures()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "l1_long":
        l1_long()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "admm_horizons":
        admm_horizons([int(a) for a in sys.argv[2:]])
        return
    if len(sys.argv) > 1 and sys.argv[1] == "l1_horizons":
        l1_horizons([int(a) for a in sys.argv[2:]])
        return
    if len(sys.argv) > 1 and sys.argv[1] == "l1stall":
        l1_stall()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "l1batch":
        l1_batch()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "l1_rollout":
        l1_rollout()
        return
    N = 5
    params, roles, si, exp = hard_cases(N)
    save("hard_n10_N5.npz", N, [800.0], O.Cfg(), params, roles, si, exp)
    params, roles, si, exp = decent_seeds(10, N, range(10))
    save("decent_n10_N5.npz", N, [800.0], O.Cfg(), params, roles, si, exp)
    params, roles, si, exp = decent_seeds(2, N, range(10))
    save("decent_n2_N5.npz", N, [800.0], O.Cfg(), params, roles, si, exp)
    params, roles, si, exp = rollout(4, N, range(3), 6)
    save("decent_rollout_n4_N5.npz", N, [800.0], O.Cfg(), params, roles, si, exp)
    params, roles, si, masses, cfg, exp = task2(5, N, range(3), [0, 29, 31, 49, 52])
    save("task2_n5_N5.npz", N, masses, cfg, params, roles, si, exp)
    # variants: horizon, Q_du, leader index, real_vehicle_as_reference
    for NN in (3, 4, 6, 7):
        params, roles, si, exp = decent_seeds(4, NN, range(4))
        save(f"variant_n4_N{NN}.npz", NN, [800.0], O.Cfg(), params, roles, si, exp)
    cfg = O.Cfg(Qdu=0.5)
    params, roles, si, exp = decent_seeds(4, N, range(4), cfg=cfg)
    save("variant_n4_N5_qdu.npz", N, [800.0], cfg, params, roles, si, exp)
    P, R = [], []
    for s in range(4):
        p, r = decent_instances(O.env_initial_state(5, s), N, leader_window(N), leader_index=2)
        P.append(p)
        R.append(r)
        p, r = decent_instances(O.env_initial_state(5, s + 10), N, leader_window(N, 0, 3100.0),
                                real_vehicle_as_reference=True)
        P.append(p)
        R.append(r)
    params, roles = np.concatenate(P), np.concatenate(R)
    si = np.zeros(len(roles), np.int32)
    exp = solve_set([O.gear_pwa_system(800.0)], si, O.Cfg(), N, params, roles)
    save("variant_n5_N5_roles.npz", N, [800.0], O.Cfg(), params, roles, si, exp)

    # known answers derived from the reference's constants
    g = O.gear_pwa_system(800.0)
    ka = {
        "seed0_env_seed": O.env_seed(0),
        "env_init_n10_seed0": O.env_initial_state(10, 0).tolist(),
        "Ad22_m800": [float(a[1, 1]) for a in g["A"]],
        "Bd2_m800": [float(b[1]) for b in g["B"]],
        "cd2_m800": [float(c[1]) for c in g["c"]],
        "v_gear_lim": [9.235, 12.855, 16.93, 23.315, 32.47],
        "alpha": 22.92,
        "region_gear": [1, 2, 3, 4, 4, 5, 6],
        "survey_values": {"Ad22": [0.989256, 0.953444], "Bd2": [5.07125, 3.68125, 2.645, 2.00875, 2.00875, 1.4575,
                                                                 1.0475], "cd2": [-0.098, 0.722823],
                          "env_init_n10_seed0": [3000, 21, 2931, 22, 2808, 10, 2728, 16, 2603, 26, 2517, 22, 2454,
                                                 22, 2353, 28, 2235, 32, 2127, 31]},
    }
    with open(os.path.join(HERE, "known_answers.json"), "w") as f:
        json.dump(ka, f, indent=1)
    print("known_answers.json written")


if __name__ == "__main__":
    main()
