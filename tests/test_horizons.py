"""Every instantiated horizon N = 2..16 against the CPU oracle, through the C ABI.

hvp_solve_batch, hvp_evaluate_batch, hvp_gadmm_rollout and hvp_gadmm_solve dispatch on the horizon
(csrc/hvp_kernels.hip HVP_CASE(2) .. HVP_CASE(16)), and the templated code changes path with it:
  N <= 8    the lane path (256-thread blocks, the fused / refill kernels, the lane simplex of
            min_1_norm, 32-bit task codes);
  N >= 9    the 16-lane cooperative path (kCoop<N>), the region hint of decentralised solves;
  N <= 12   naive-ADMM node records on the cooperative path, node_prio's 48-bit code field, 256
            candidates per instance by default;
  N >= 13   no node records, 1024 candidates per instance;
  N = 16    the 4-bit-per-step region code fills its 64-bit word.
The other GPU tests run N = 3..8, 10 and 15 (decentralised), 5 and 10 (both ADMM schemes) only.

Bars (tests/test_gpu_parity.py _compare): status equal; region sequence and gear labels bit-exact;
cost 1e-9 relative to max(1, |c|); u 1e-6; x 1e-4.  The oracle runs its branch and bound
(O.set_method(O.METHOD_BNB)) live where that takes seconds; the slower min_1_norm and ADMM answers
come from fixtures (tests/golden/make_golden.py l1_horizons, admm_horizons).

The tests not marked gpu are the oracle-side conditions: the fast-leader instances do reach the top
regions at the last step, and the oracle reproduces the new fixtures.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle as O
from golden_io import load
from instances import decent_instances, fast_leader_platoons, fast_leader_window, leader_window, oracle_solve

GEAR_OF = np.array([1, 2, 3, 4, 4, 5, 6])
OVERFLOW_FREE = (12, 13)  # the horizons either side of default_capacity's 256 | 1024 edge


# ------------------------------------------------------------------ product-side builders
def _system():
    from hvp import tables
    from hvp.models import PwaGearVehicle

    veh = PwaGearVehicle(800)
    return tables.system_from_dict(veh.get_discrete_system(1), tables.gears_of(veh))


def _solver(N, **kw):
    from hvp import tables
    from hvp.solver import BatchSolver

    return BatchSolver(tables.problem(N, **kw), [_system()])


def _solve(s, params, roles):
    return s.solve(np.zeros(len(roles), np.int32), roles, params)


# ------------------------------------------------------------------ instances and oracle answers
@functools.lru_cache(maxsize=None)
def seed_batch(N: int):
    """The 12 local problems of the 4-vehicle platoons of seeds 0..2 (all four role patterns), then
    the 4 of seed 0 with leader_index = 2 and real_vehicle_as_reference."""
    P, R = [], []
    for seed in range(3):
        p, r = decent_instances(O.env_initial_state(4, seed), N, leader_window(N))
        P.append(p)
        R.append(r)
    p, r = decent_instances(O.env_initial_state(4, 0), N, leader_window(N), leader_index=2,
                            real_vehicle_as_reference=True)
    return np.concatenate(P + [p]), np.concatenate(R + [r])


@functools.lru_cache(maxsize=None)
def fast_batch(N: int):
    P, R = [], []
    for st in fast_leader_platoons():
        p, r = decent_instances(st, N, fast_leader_window(N, st[0]))
        P.append(p)
        R.append(r)
    return np.concatenate(P), np.concatenate(R)


def _arrays(ref) -> dict:
    return {"status": np.array([r.status for r in ref]), "region": np.array([r.sigma for r in ref]),
            "cost": np.array([r.cost for r in ref]), "u": np.array([r.u for r in ref]),
            "x": np.array([r.x for r in ref])}


@functools.lru_cache(maxsize=None)
def oracle_answers(kind: str, N: int, quadratic: bool = True) -> dict:
    """The oracle's branch and bound on seed_batch / fast_batch (min_1_norm: the first 12), once per
    session."""
    params, roles = seed_batch(N) if kind == "seed" else fast_batch(N)
    if not quadratic:
        params, roles = params[:12], roles[:12]
    O.set_method(O.METHOD_BNB)
    try:
        return _arrays(oracle_solve(O.gear_pwa_system(800.0), O.Cfg(), N, params, roles, quadratic=quadratic))
    finally:
        O.set_method(O.METHOD_ENUMERATE)


def _compare(res, exp, what=""):
    """The project's bars (module docstring) of a BatchResult against expected arrays."""
    st = exp["status"]
    assert np.array_equal(res.status, st), (what, res.status, st)
    for i in np.flatnonzero(st == 0):
        sig = exp["region"][i]
        assert list(res.region[i]) == list(sig), (what, i, res.region[i], sig, res.cost[i], exp["cost"][i])
        assert list(res.gear[i]) == list(GEAR_OF[sig]), (what, i)
        c = exp["cost"][i]
        assert abs(res.cost[i] - c) <= 1e-9 * max(1.0, abs(c)), (what, i, res.cost[i], c)
        assert np.abs(res.u[i] - exp["u"][i]).max() <= 1e-6, (what, i, res.u[i], exp["u"][i])
        assert np.abs(res.x[i] - exp["x"][i]).max() <= 1e-4, (what, i)


# ================================================================== 1. decentralised, quadratic cost
@pytest.mark.gpu
@pytest.mark.parametrize("N", range(2, 17))
def test_decent_branch_and_bound_matches_oracle(gpu_available, N):
    from hvp import _abi

    params, roles = seed_batch(N)
    exp = oracle_answers("seed", N)
    assert (exp["status"] == 0).all()
    _compare(_solve(_solver(N, method=_abi.METHOD_BNB), params, roles), exp, f"N={N}")


def test_candidate_count_is_the_enumeration_count():
    """O.candidates lists the velocity-feasible sequences the oracle's enumeration solves: its length
    is the enumeration's n_candidates (checked at N = 5; the N = 7 and 8 node counts below use it,
    where enumerating with every QP solved takes the oracle 3 s and 12 s)."""
    params, roles = seed_batch(5)
    sysd = O.gear_pwa_system(800.0)
    ref = oracle_solve(sysd, O.Cfg(), 5, params, roles)
    assert [r.n_candidates for r in ref] == [len(O.candidates(sysd, O.Cfg(), 5, p[:2])) for p in params]


@pytest.mark.gpu
@pytest.mark.parametrize("N", range(2, 9))
def test_decent_enumeration_matches_oracle(gpu_available, N):
    """N <= 8 by exhaustive enumeration: the same answers, and as many sequences solved as the
    oracle's enumeration lists."""
    from hvp import _abi

    params, roles = seed_batch(N)
    exp = oracle_answers("seed", N)
    res = _solve(_solver(N, method=_abi.METHOD_ENUMERATE), params, roles)
    _compare(res, exp, f"N={N}")
    sysd = O.gear_pwa_system(800.0)
    counts = [len(O.candidates(sysd, O.Cfg(), N, p[:2])) for p in params]
    assert list(res.nodes) == counts


@pytest.mark.gpu
@pytest.mark.parametrize("N", range(2, 17))
def test_decent_is_deterministic(gpu_available, N):
    """The 12 seeded instances twice on one handle: bit-equal outputs."""
    import torch

    from hvp import _abi

    params, roles = seed_batch(N)
    dev = torch.device("cuda", 0)
    tp, tr = torch.from_numpy(params[:12].copy()).to(dev), torch.from_numpy(roles[:12].copy()).to(dev)
    ts = torch.zeros(12, dtype=torch.int32, device=dev)
    s = _solver(N, method=_abi.METHOD_BNB)
    a = {k: v.clone() for k, v in s.solve_device(ts, tr, tp).items()}
    b = s.solve_device(ts, tr, tp)
    torch.cuda.synchronize()
    assert (a["status"] == 0).all()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("N", range(9, 17))
def test_decent_leaf_fallback(gpu_available, monkeypatch, N):
    """The cooperative path with the leaves' active-set solve capped at 2 steps (HVP_LEAF_GI_CAP, read
    at hvp_create): leaves go through the interior-point fallback and the answers stay the oracle's."""
    from hvp import _abi

    monkeypatch.setenv("HVP_LEAF_GI_CAP", "2")
    params, roles = seed_batch(N)
    s = _solver(N, method=_abi.METHOD_BNB)
    res = _solve(s, params, roles)
    assert s.stats().n_fallback > 0
    _compare(res, oracle_answers("seed", N), f"N={N}")


# ================================================================== 2. the top of the code word
@pytest.mark.parametrize("N", [12, 16])
def test_fast_leader_instances_end_in_the_top_regions(N):
    """The oracle-side condition of test_top_of_the_code_word: at least 4 instances whose optimal
    sequence has a region >= 4 at the last step and another region at step 0."""
    exp = oracle_answers("fast", N)
    assert (exp["status"] == 0).all()
    sig = exp["region"]
    top = (sig[:, N - 1] >= 4) & (sig[:, 0] != sig[:, N - 1])
    assert top.sum() >= 4, sig[:, [0, N - 1]]


@pytest.mark.gpu
@pytest.mark.parametrize("N", [12, 16])
def test_top_of_the_code_word(gpu_available, N):
    """fast_batch: the 20 local problems of five platoons whose leader reference runs ahead at 40 m/s.
    By the oracle the leading vehicles (instances 0, 4, 8, 12, 16) start in region 3 (18..21 m/s) and
    end, at k = N - 1, in region 5 at N = 12 (the top nibble of node_prio's 48-bit field) and in
    region 6 at N = 16 (bits 60..63 of the code word); the trailers (3, 7, ...) pass through regions
    4 and 5 early in the horizon and return to 3; the others stay in 3."""
    from hvp import _abi

    params, roles = fast_batch(N)
    exp = oracle_answers("fast", N)
    sig = exp["region"]
    top = (sig[:, N - 1] >= 4) & (sig[:, 0] != sig[:, N - 1])
    assert (exp["status"] == 0).all() and top.sum() >= 4, sig[:, [0, N - 1]]
    _compare(_solve(_solver(N, method=_abi.METHOD_BNB), params, roles), exp, f"N={N}")


@pytest.mark.gpu
@pytest.mark.parametrize("N", [9, 12, 13, 16])
def test_region_hint_keeps_the_answers(gpu_available, N):
    """hvp_set_region_hint on the cooperative path (decentralised solves take it from N = 9): the hinted
    sequence is packed step by step into the region code (hint_code, up to k = 15) and tried as a
    second incumbent.  Rows hinted with their own optimum, with another instance's optimum (usually
    infeasible or worse for them) and with no hint (-1) all keep the oracle's answers -- on the seeded
    batch and, at N = 12 and 16, on the instances that end in the top regions.  That the hint is read
    shows in the node counts against the same solve without one (at N = 16 the leaders that end in
    region 6 go from 158 and 94 nodes to 48 and 49)."""
    import torch

    from hvp import _abi

    batches = [("seed", seed_batch(N))] + ([("fast", fast_batch(N))] if N in (12, 16) else [])
    params = np.concatenate([b[1][0] for b in batches])
    roles = np.concatenate([b[1][1] for b in batches])
    exp = {k: np.concatenate([oracle_answers(b[0], N)[k] for b in batches]) for k in ("status", "region", "cost", "u", "x")}
    hint = exp["region"].astype(np.int8)
    hint[1::4] = hint[2::4]
    hint[3::4] = -1
    dev = torch.device("cuda", 0)
    s = _solver(N, method=_abi.METHOD_BNB)
    base = _solve_hinted(s, params, roles, dev)
    th = torch.from_numpy(hint).to(dev)
    s.set_region_hint(th)
    res = _solve_hinted(s, params, roles, dev)
    _compare(res, exp, f"N={N}")
    own = np.arange(len(roles)) % 2 == 0
    print(f"N = {N}: nodes without hint {base.nodes.tolist()}, with {res.nodes.tolist()}")
    # a row without a hint searches the same tree; a search that starts from its optimum as incumbent
    # prunes at least as much as one that has to find it, at the price of the one hinted leaf
    assert np.array_equal(res.nodes[3::4], base.nodes[3::4])
    assert res.nodes[own].sum() < base.nodes[own].sum(), (res.nodes[own].sum(), base.nodes[own].sum())


def _solve_hinted(s, params, roles, dev):
    """solve_device (the hint is a device tensor indexed by batch position) into a BatchResult."""
    import torch

    from hvp.solver import BatchResult

    out = s.solve_device(torch.zeros(len(roles), dtype=torch.int32, device=dev), torch.from_numpy(roles).to(dev),
                         torch.from_numpy(params).to(dev), retry_overflow=True)
    torch.cuda.synchronize()
    return BatchResult(**{k: v.cpu().numpy() for k, v in out.items()})


# ================================================================== 3. min_1_norm
L1_LIVE = (2, 4, 6, 8, 9)
L1_FIXTURE = (11, 12, 13, 16)


def _l1_case(N):
    """(params, roles, expected arrays) of a min_1_norm horizon: live, or its fixture."""
    if N in L1_LIVE:
        params, roles = seed_batch(N)
        return params[:12], roles[:12], oracle_answers("seed", N, False)
    fx = load(f"l1_long_n4_N{N}.npz")
    assert int(fx["N"]) == N and int(fx["quadratic"]) == 0 and int(fx["method"]) == 1
    exp = {k: fx[f"exp_{k}"] for k in ("status", "region", "cost", "u", "x")}
    return fx["params"], fx["roles"], exp


@pytest.mark.gpu
@pytest.mark.parametrize("N", L1_LIVE + L1_FIXTURE)
def test_l1_matches_oracle(gpu_available, N):
    """min_1_norm by branch and bound: the lane simplex up to N = 8 (the size its row table was cut
    for), the wave interior point from N = 9.  No horizon is refused."""
    from hvp import _abi

    params, roles, exp = _l1_case(N)
    assert (exp["status"] == 0).all()
    _compare(_solve(_solver(N, quadratic_cost=False, method=_abi.METHOD_BNB), params, roles), exp, f"N={N}")


@pytest.mark.gpu
@pytest.mark.parametrize("N", [2, 4, 6, 8])
def test_l1_refill_equals_grid_stride(gpu_available, monkeypatch, N):
    """The lane simplex through persistent waves against the grid-stride kernels (HVP_LP_REFILL=0):
    the same LPs by the same simplex, so the same trees and optima (tests/test_gpu_l1.py at N = 5)."""
    from hvp import _abi

    params, roles, exp = _l1_case(N)
    s = _solver(N, quadratic_cost=False, method=_abi.METHOD_BNB)
    a = _solve(s, params, roles)
    monkeypatch.setenv("HVP_LP_REFILL", "0")
    b = _solve(s, params, roles)
    _compare(b, exp, f"N={N}")
    assert np.array_equal(a.status, b.status) and np.array_equal(a.region, b.region)
    assert np.all(np.abs(a.cost - b.cost) <= 1e-12 * np.maximum(1, np.abs(b.cost)))
    assert np.abs(a.u - b.u).max() <= 1e-9
    assert np.array_equal(a.nodes, b.nodes)


def _l1_oracle_case(job):
    N, p, r = job
    O.set_method(O.METHOD_BNB)
    try:
        return oracle_solve(O.gear_pwa_system(800.0), O.Cfg(), N, p[None], [r], quadratic=False)[0]
    finally:
        O.set_method(O.METHOD_ENUMERATE)


@pytest.mark.parametrize("N", [11, 12, 13])
def test_oracle_reproduces_the_l1_fixture(N):
    """The fixtures the oracle re-solves in under a minute (12 s, 26 s and 53 s of CPU time; N = 16
    takes it a quarter of an hour), one freshly spawned process per instance (no fork of a process
    that may hold the GPU)."""
    import multiprocessing as mp
    import os

    fx = load(f"l1_long_n4_N{N}.npz")
    with mp.get_context("spawn").Pool(min(4, os.cpu_count() or 1)) as pool:
        ref = _arrays(pool.map(_l1_oracle_case, [(N, p, r) for p, r in zip(fx["params"], fx["roles"])], chunksize=1))
    assert np.array_equal(ref["status"], fx["exp_status"]) and np.array_equal(ref["region"], fx["exp_region"])
    assert np.all(np.abs(ref["cost"] - fx["exp_cost"]) <= 1e-12 * np.abs(fx["exp_cost"]))
    assert np.abs(ref["u"] - fx["exp_u"]).max() <= 1e-9


@pytest.mark.parametrize("N", L1_FIXTURE)
def test_l1_fixtures_hold_the_seed_platoon(N):
    fx = load(f"l1_long_n4_N{N}.npz")
    params, roles = seed_batch(N)
    assert (fx["exp_status"] == 0).all() and fx["exp_certified"].all()
    assert len(fx["roles"]) == 4  # the whole seed-0 platoon at every horizon
    assert np.array_equal(fx["params"], params[:4]) and np.array_equal(fx["roles"], roles[:4])


# ================================================================== 4. naive ADMM
ADMM_HORIZONS = (8, 9, 12, 13, 16)
ADMM_L1_HORIZONS = (9, 12)


def _admm_fixture(N, quadratic):
    return load(f"admm_horizon_N{N}.npz" if quadratic else f"admm_l1_horizon_N{N}.npz")


def _admm_platoons(N, quadratic):
    """(states (P, 8), leader windows (P, 2, N+1)) of a fixture: the seed-0 platoon, and at N = 12
    (quadratic) the five fast-leader platoons."""
    states = [O.env_initial_state(4, 0).astype(float)]
    leads = [leader_window(N)]
    if quadratic and N == 12:
        for st in fast_leader_platoons():
            states.append(st)
            leads.append(fast_leader_window(N, st[0]))
    return np.stack(states), np.stack(leads)


@pytest.mark.parametrize("N,quadratic", [(N, True) for N in ADMM_HORIZONS] + [(N, False) for N in ADMM_L1_HORIZONS])
def test_admm_fixture_is_the_first_iteration(N, quadratic):
    """The fixtures' parameter rows are those of a time step's first ADMM iteration (y = z = 0), every
    answer optimal and KKT-certified; at N = 12 the leaders of the fast platoons end in region >= 4."""
    fx = _admm_fixture(N, quadratic)
    states, leads = _admm_platoons(N, quadratic)
    zero = np.zeros((2, N + 1))
    rows = [O.admm_params(st[2 * i:2 * i + 2], zero, zero, zero, zero, lead if i == 0 else zero)
            for st, lead in zip(states, leads) for i in range(4)]
    assert np.array_equal(fx["params"], np.array(rows))
    assert list(fx["roles"]) == [O.role_bits(i, 4) for i in range(4)] * len(states)
    assert (fx["exp_status"] == 0).all() and fx["exp_cert"].all()
    if quadratic and N == 12:
        sig = fx["exp_region"][4::4]
        assert ((sig[:, N - 1] >= 4) & (sig[:, 0] != sig[:, N - 1])).sum() >= 4, sig


@pytest.mark.parametrize("N,quadratic,rows", [(N, True, slice(None)) for N in ADMM_HORIZONS] +
                         [(9, False, slice(None)), (12, False, slice(0, 1))])
def test_oracle_reproduces_the_admm_fixture(N, quadratic, rows):
    """Every fixture re-solved in full (1 to 25 s each; the min_1_norm one at N = 9 30 s), but for
    min_1_norm at N = 12: its leader only, the whole of it takes the oracle over a minute."""
    fx = _admm_fixture(N, quadratic)
    sysd = O.gear_pwa_system(800.0)
    for i in range(len(fx["roles"]))[rows]:
        r = O.solve_admm_miqp(sysd, O.Cfg(), N, int(fx["roles"][i]), float(fx["rho"]), fx["params"][i],
                              quadratic=quadratic)
        assert r.status == fx["exp_status"][i] and np.array_equal(r.sigma, fx["exp_region"][i])
        assert abs(r.cost - fx["exp_cost"][i]) <= 1e-12 * abs(fx["exp_cost"][i])
        assert np.abs(r.u - fx["exp_u"][i]).max() <= 1e-9


def _admm_iterations(N, quadratic, iters=3):
    """`iters` iterations of hvp_solve_admm_batch + hvp_admm_update on one handle; every iteration's
    parameter rows and outputs."""
    import torch

    from hvp import _abi
    from hvp.admm import AdmmEngine, admm_problem

    states, leads = _admm_platoons(N, quadratic)
    P = len(states)
    eng = AdmmEngine(admm_problem(N, 0.5, quadratic_cost=quadratic), [_system()], np.zeros(4 * P, np.int32),
                     [O.role_bits(i, 4) for i in range(4)] * P, 4, P)
    _abi.check(eng.solver._lib.hvp_set_node_records(eng.solver._h, 1), "hvp_set_node_records")
    eng.set_leader(leads)
    seen = []

    def keep(solver):
        torch.cuda.synchronize()
        seen.append({k: v.cpu().numpy().copy() for k, v in {**eng.out, "params": eng.params}.items()})
        seen[-1]["qp_iterations"] = int(solver.stats().qp_iterations)

    eng.step(states, iters, on_solve=keep)
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("N,quadratic", [(N, True) for N in ADMM_HORIZONS] + [(N, False) for N in ADMM_L1_HORIZONS])
def test_admm_across_the_node_record_edge(gpu_available, monkeypatch, N, quadratic):
    """HVP_FORM_ADMM at the lane path's last horizon (8), the first cooperative one (9), the last with
    node records (12), the first without (13) and HVP_MAX_N; min_1_norm (L1AdmmWave) at 9 and 12.
    The local problems of the first iteration equal the oracle's (the bars above, the copies to 1e-4
    as tests/test_admm.py); three iterations with the node records (default slots) and without
    (HVP_ADMM_NODE_SLOTS=0) agree in every iteration: regions equal, costs 1e-9 relative, controls
    1e-9 (the bar of test_node_records_keep_the_answers).  At 8, 13 and 16 there are no records (lane
    path; compiled out), so the two runs are bit-equal; at 9 and 12 the quadratic runs with records
    take fewer active-set iterations, which shows the records in use."""
    fx = _admm_fixture(N, quadratic)
    monkeypatch.delenv("HVP_ADMM_NODE_SLOTS", raising=False)
    warm = _admm_iterations(N, quadratic)
    monkeypatch.setenv("HVP_ADMM_NODE_SLOTS", "0")
    cold = _admm_iterations(N, quadratic)
    assert len(warm) == len(cold) == 3
    first = warm[0]
    assert np.array_equal(first["params"], fx["params"])
    ok = fx["exp_status"] == 0
    assert ok.all() and np.array_equal(first["status"], fx["exp_status"])
    assert np.array_equal(first["region"], fx["exp_region"])
    assert np.array_equal(first["gear"], GEAR_OF[fx["exp_region"]])
    ce = fx["exp_cost"]
    assert np.all(np.abs(first["cost"] - ce) <= 1e-9 * np.maximum(1.0, np.abs(ce))), np.abs(first["cost"] - ce).max()
    assert np.abs(first["u"] - fx["exp_u"]).max() <= 1e-6
    assert np.abs(first["x"] - fx["exp_x"]).max() <= 1e-4
    assert np.abs(first["x_front"] - fx["exp_xf"]).max() <= 1e-4
    assert np.abs(first["x_back"] - fx["exp_xb"]).max() <= 1e-4
    for it, (w, c) in enumerate(zip(warm, cold)):
        assert (w["status"] == 0).all() and (c["status"] == 0).all(), it
        assert np.array_equal(w["region"], c["region"]), it
        assert np.all(np.abs(w["cost"] - c["cost"]) <= 1e-9 * np.maximum(1.0, np.abs(c["cost"]))), it
        assert np.abs(w["u"] - c["u"]).max() <= 1e-9, it
    its = [sum(o["qp_iterations"] for o in run[1:]) for run in (warm, cold)]
    print(f"N = {N}, quadratic {quadratic}: QP iterations of iterations 2-3 with records {its[0]}, without {its[1]}")
    if not 9 <= N <= 12:
        # no records on the lane path or beyond N = 12: the same launches, so the same bits
        for w, c in zip(warm, cold):
            for k in w:
                assert np.array_equal(w[k], c[k]), (k, N)
    elif quadratic:
        # the records are in use: a node QP started from its own previous active set needs fewer steps
        assert its[0] < its[1], its


# ================================================================== 5. switching ADMM, evaluation
@pytest.mark.gpu
@pytest.mark.parametrize("N", [8, 9, 16])
def test_gadmm_rollout_and_solve_match_oracle(gpu_available, N):
    """hvp_gadmm_rollout then three ADMM iterations of hvp_gadmm_solve (+ hvp_gadmm_update) for 3
    platoons of 3 vehicles (seeds 0..2): the rolled-out sequences and trajectories are the oracle
    coordinator's, and every local QP -- the device's own parameter rows and sequences, re-solved by
    the oracle in the full (x, u, s, copies) space -- has the oracle's controls, trajectories, copies,
    cost and region-edge bits (the bars of tests/test_gadmm.py _check_local)."""
    import torch

    from hvp import _abi
    from hvp.gadmm import GAdmmEngine, gadmm_problem

    n = P = 3
    sysd = O.gear_pwa_system(800.0)
    co = O.GAdmmCoordinator([sysd] * n, O.Cfg(), N)
    states = np.stack([O.env_initial_state(n, seed).astype(float) for seed in range(P)])
    eng = GAdmmEngine(gadmm_problem(N, 0.5), [_system()] * n, n, P)
    eng.set_leader(leader_window(N))
    eng.params[:, :2] = torch.as_tensor(states.reshape(P * n, 2), device=eng.dev)
    eng.state.fill_(_abi.GADMM_LIVE)
    eng.rollout(0)
    torch.cuda.synchronize()
    assert (eng.state.cpu().numpy() & _abi.GADMM_FAILED == 0).all()
    seq, x = eng.seq.cpu().numpy(), eng.x.cpu().numpy()
    for b in range(P * n):
        i, x0 = b % n, states.reshape(P * n, 2)[b]
        X, sig = co.rollout(i, x0, np.full(N, co.u_const_vel(i, x0[1])))
        assert list(seq[b]) == list(sig), b
        assert np.abs(x[b] - X).max() <= 1e-9 * max(1.0, np.abs(X).max()), b
    eng.update(init=True)
    edges = 0
    for it in range(3):
        eng.solve()
        torch.cuda.synchronize()
        h = {k: getattr(eng, k).cpu().numpy() for k in ("params", "seq", "u", "x", "xf", "xb", "cost", "status", "edge")}
        for b in range(P * n):
            role, back = O.gadmm_role(b % n, n)
            r = O.solve_gadmm_qp(sysd, O.Cfg(), N, role, back, 0.5, h["params"][b], h["seq"][b])
            assert r.status == 0 and h["status"][b] == 0, (it, b, r.status, h["status"][b])
            assert abs(h["cost"][b] - r.cost) <= 1e-9 * max(1.0, abs(r.cost)), (it, b, h["cost"][b], r.cost)
            assert np.abs(h["u"][b] - r.u).max() <= 1e-6, (it, b)
            assert np.abs(h["x"][b] - r.x).max() <= 1e-6, (it, b)
            assert np.abs(h["xf"][b] - r.x_front).max() <= 1e-6, (it, b)
            assert np.abs(h["xb"][b] - r.x_back).max() <= 1e-9, (it, b)
            assert int(h["edge"][b].astype(np.uint32)) == r.switch, (it, b, hex(int(h["edge"][b])), hex(r.switch))
            edges += r.switch != 0
        eng.update()
    assert edges > 0.2 * 3 * P * n  # active region edges, up to step N - 1, are exercised


@pytest.mark.gpu
@pytest.mark.parametrize("N", [9, 13, 16])
def test_evaluate_prices_the_optima(gpu_available, N):
    """hvp_evaluate_batch on the cooperative horizons: the oracle's optimal (gear, u) of seed_batch
    costs the oracle's optimum to 1e-9 relative with its trajectory to 1e-9 max(1, |x|)
    (tests/test_evaluate.py's bars); and the solver's own optimum, priced, returns the solver's cost
    and trajectory to the same bars (one rollout and one cost sum in each kernel)."""
    from hvp import _abi

    params, roles = seed_batch(N)
    exp = oracle_answers("seed", N)
    s = _solver(N, method=_abi.METHOD_BNB)
    sysi = np.zeros(len(roles), np.int32)
    out = s.evaluate(sysi, roles, params, GEAR_OF[exp["region"]].astype(np.int8), exp["u"])
    assert (out["status"] == 0).all()
    assert np.all(np.abs(out["cost"] - exp["cost"]) <= 1e-9 * np.abs(exp["cost"]))
    assert np.all(np.abs(out["x"] - exp["x"]) <= 1e-9 * np.maximum(1.0, np.abs(exp["x"])))
    res = _solve(s, params, roles)
    _compare(res, exp, f"N={N}")
    own = s.evaluate(sysi, roles, params, res.gear, res.u)
    assert (own["status"] == 0).all()
    assert np.all(np.abs(own["cost"] - res.cost) <= 1e-9 * np.abs(res.cost))
    assert np.all(np.abs(own["x"] - res.x) <= 1e-9 * np.maximum(1.0, np.abs(res.x)))


# ================================================================== 6. the default capacity
@pytest.mark.gpu
@pytest.mark.parametrize("N", OVERFLOW_FREE)
def test_default_capacity_holds_the_batch(gpu_available, N):
    """Nothing reserved: default_capacity gives 256 nodes per instance and level up to N = 12 and 1024
    from N = 13.  No instance of seed_batch overflows, and the tree nodes of ALL levels together
    (hvp_stats.n_candidates, an upper bound of the widest level's high-water mark) stay below the
    one-level capacity."""
    import torch

    from hvp import _abi

    params, roles = seed_batch(N)
    B = len(roles)
    dev = torch.device("cuda", 0)
    s = _solver(N, method=_abi.METHOD_BNB)
    out = s.solve_device(torch.zeros(B, dtype=torch.int32, device=dev), torch.from_numpy(roles).to(dev),
                         torch.from_numpy(params).to(dev))
    torch.cuda.synchronize()
    st = s.stats()
    assert not (out["status"] == _abi.OVERFLOW).any()
    assert (out["status"] == _abi.OPTIMAL).all()
    assert st.capacity == (256 if N <= 12 else 1024) * B
    assert 0 < st.n_candidates < st.capacity, (st.n_candidates, st.capacity)
    assert np.array_equal(out["region"].cpu().numpy(), oracle_answers("seed", N)["region"])
