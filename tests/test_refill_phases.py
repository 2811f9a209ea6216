"""The refill kernel's instantiations by phase (hvp_lane.h k_bnb_bound_refill, launch_refill).

A launch of level N or of the dive list runs the LEAF instantiation (k a constant, no child code,
no pass-through stage), a launch of a level below N - 1 the UPPER one (no leaf write-back, no reuse
block), level N - 1 the kernel for every level.  HVP_REFILL_PHASES=0 sends every launch through
that one kernel, the code before.  Only unreachable code left the phased kernels, so every GPU case
asks for equality bit by bit: the default solve and the HVP_REFILL_PHASES=0 solve on the same
handle give torch.equal outputs and the same hvp_stats counts (n_candidates, qp_iterations,
n_fallback; n_spilled is printed: which reservation straddles a segment's end depends on the order
the waves reserve in, and two solves of one kernel differ in it too).  Against the host build of the algorithm (lib/libhvp_hostref.so) the bars
are test_refill_tables._check_against_hostref's.

The CPU test is of profiles/summarize.py: the instantiations share the short name
k_bnb_bound_refill, and their rows are merged (calls summed, averages weighted by calls).
"""

from __future__ import annotations

import csv
import importlib.util
import json
import os

import numpy as np
import pytest

from test_dive_reuse import (FIELDS, _as_result, _host_solve, _position_box_instances, _same_outputs, _tables,
                             _tie_instances)
from test_refill_cost_row import _hostref as _mixed_hostref
from test_refill_cost_row import _inputs as _mixed_inputs
from test_refill_tables import _check_against_hostref, _gear_pwa
from test_refill_uniform import _problem

gpu = pytest.mark.gpu

BATCHES = (1, 37, 300)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stats(solver):
    st = solver.stats()
    return (int(st.n_candidates), int(st.qp_iterations), int(st.n_fallback), int(st.n_spilled))


def _phased_and_not(monkeypatch, solver, sys_idx, roles, params, retry=False):
    """The default solve and the HVP_REFILL_PHASES=0 solve on the same handle: (outputs, stats) each."""
    import torch

    dev = torch.device("cuda", 0)
    ts, tr, tp = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (sys_idx, roles, params))
    runs = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("HVP_REFILL_PHASES", "0")
        else:
            monkeypatch.delenv("HVP_REFILL_PHASES", raising=False)
        out = solver.solve_device(ts, tr, tp, retry_overflow=retry)
        torch.cuda.synchronize()
        runs.append(({k: v.clone() for k, v in out.items()}, _stats(solver)))
    monkeypatch.delenv("HVP_REFILL_PHASES", raising=False)
    return runs


@gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("count", [1, 9])
@pytest.mark.parametrize("N", [2, 3, 5, 8])
def test_phased_against_one_kernel_and_host_build(gpu_available, monkeypatch, N, count, B):
    """Roles mixed lane by lane, one system (tables in LDS) and nine (the global-memory
    instantiations); a batch of 1, a partial wave, several waves.  N = 2: level 0 an upper level,
    level 1 the kernel for every level, level 2 a leaf level; N = 3: the smallest horizon with two
    upper levels.  (Which (N, STAGE) pairs have a LEAF / UPPER instantiation of their own is
    hvp_lane.h's kRefillLeafOk / kRefillUpperOk; the others launch the kernel for every level.)"""
    from hvp import tables
    from hvp.solver import BatchSolver

    params, roles = _mixed_inputs(N)
    sys_idx = (np.arange(len(roles)) % count).astype(np.int32)
    s = BatchSolver(tables.problem(N), list(_tables(count)))
    try:
        (on, st_on), (off, st_off) = _phased_and_not(monkeypatch, s, sys_idx[:B], roles[:B], params[:B])
    finally:
        s.close()
    print(f"N={N} count={count} B={B}: (n_candidates, qp_iterations, n_fallback, n_spilled) {st_on} phased, "
          f"{st_off} one kernel; nodes {int(on['nodes'].sum())}")
    _same_outputs(on, off)
    assert st_on[:3] == st_off[:3]
    ref = {k: v[:B] for k, v in _mixed_hostref(N, count).items()}
    _check_against_hostref(_as_result(on), ref)


@gpu
@pytest.mark.parametrize("count", [1, 9])
@pytest.mark.parametrize("N", [4, 6, 7])
def test_the_other_refill_horizons(gpu_available, monkeypatch, N, count):
    """The horizons between: their instantiations differ from N = 2, 3, 5 and 8's (UPPER alone at
    N = 4, LEAF alone at N = 6 and, with the tables in global memory, at N = 7).  300 instances,
    the two solves on one handle only."""
    from hvp import tables
    from hvp.solver import BatchSolver

    B = 300
    params, roles = _mixed_inputs(N)
    sys_idx = (np.arange(len(roles)) % count).astype(np.int32)
    s = BatchSolver(tables.problem(N), list(_tables(count)))
    try:
        (on, st_on), (off, st_off) = _phased_and_not(monkeypatch, s, sys_idx[:B], roles[:B], params[:B])
    finally:
        s.close()
    print(f"N={N} count={count}: {st_on} phased, {st_off} one kernel")
    _same_outputs(on, off)
    assert st_on[:3] == st_off[:3]
    assert (on["status"] == 0).any()


SWITCHES = (("HVP_DIVE_REUSE", "0"), ("HVP_PASS_THROUGH", "1"), ("HVP_SPLIT_LEVELS", "1"), ("HVP_SPLIT_LEVELS", "4"),
            ("HVP_ROOT_REFILL", "0"))


@gpu
@pytest.mark.parametrize("env", SWITCHES)
def test_with_every_switch_that_reaches_the_event(gpu_available, monkeypatch, env):
    """N = 5, 300 mixed-role instances.  Without the reuse (UPPER and LEAF next to a level N - 1 that
    skips its block), with pass-through nodes (RS_PASS in UPPER and at level N - 1, none at level
    N), one list and four buckets, and k_bnb_root in place of levels 0 and the dive list (levels
    1..N take the same choice): each solve equals the same-switch solve through the one kernel."""
    from hvp import tables
    from hvp.solver import BatchSolver

    N, B = 5, 300
    params, roles = _mixed_inputs(N)
    params, roles = params[:B], roles[:B]
    sys_idx = np.zeros(B, np.int32)
    monkeypatch.setenv(*env)
    s = BatchSolver(tables.problem(N), [_gear_pwa(800.0)])
    try:
        (on, st_on), (off, st_off) = _phased_and_not(monkeypatch, s, sys_idx, roles, params)
    finally:
        s.close()
    print(f"{env}: {st_on} phased, {st_off} one kernel")
    _same_outputs(on, off)
    assert st_on[:3] == st_off[:3]
    ref = {k: v[:B] for k, v in _mixed_hostref(N, 1).items()}
    _check_against_hostref(_as_result(on), ref)


@gpu
def test_full_buckets_spill(gpu_available, monkeypatch):
    """The smallest capacity at which one list per level fits, + 64 per bucket, four buckets:
    children spill into other segments (bnb_put_children from UPPER and from level N - 1), nothing
    overflows, and both solves are the default workspace's."""
    import torch

    from hvp import _abi, tables
    from hvp.solver import BatchSolver

    N, B = 5, 300
    params, roles = _mixed_inputs(N)
    params, roles = params[:B], roles[:B]
    sys_idx = np.zeros(B, np.int32)
    dev = torch.device("cuda", 0)
    ts, tr, tp = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (sys_idx, roles, params))

    def solver(cap=0):  # a fresh handle per capacity (hvp_reserve only ever grows a workspace)
        s = BatchSolver(tables.problem(N), [_gear_pwa(800.0)])
        if cap:
            s.reserve(B, cap)
        return s

    def overflows(cap):
        s = solver(cap)
        try:
            out = s.solve_device(ts, tr, tp)
            torch.cuda.synchronize()
            return bool((out["status"] == _abi.OVERFLOW).any())
        finally:
            s.close()

    s = solver()
    try:
        (plain, _), _ = _phased_and_not(monkeypatch, s, sys_idx, roles, params)
    finally:
        s.close()
    monkeypatch.setenv("HVP_SPLIT_LEVELS", "1")
    lo, hi = B, 16 * B
    assert not overflows(hi)
    while hi - lo > 64:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if overflows(mid) else (lo, mid)
    buckets = 4
    monkeypatch.setenv("HVP_SPLIT_LEVELS", str(buckets))
    s = solver(hi + 64 * buckets)
    try:
        (on, st_on), (off, st_off) = _phased_and_not(monkeypatch, s, sys_idx, roles, params)
    finally:
        s.close()
    print(f"capacity {hi + 64 * buckets}: {st_on} phased, {st_off} one kernel")
    # (which child spills depends on the order the waves reserve in: the count is not compared)
    assert st_on[3] > 0 and st_off[3] > 0, "the bucketed levels must have needed the spill at this capacity"
    _same_outputs(on, off)
    assert st_on[:3] == st_off[:3]
    _same_outputs(on, plain)


@gpu
def test_dead_leaf_slots_after_the_retry(gpu_available, monkeypatch):
    """Two slots per instance and level: reservations overflow and leave dead slots at level N,
    where LEAF writes leaf_stat = HVP_OVERFLOW.  The overflowed instances are the same with both
    kernels' dead-slot handling, and after the retry the answers are equal and the host build's."""
    import torch

    from hvp import _abi, tables
    from hvp.solver import BatchSolver

    N, B = 5, 300
    params, roles = _mixed_inputs(N)
    params, roles = params[:B], roles[:B]
    sys_idx = np.zeros(B, np.int32)
    s = BatchSolver(tables.problem(N), [_gear_pwa(800.0)])
    try:
        s.reserve(B, 2 * B)
        dev = torch.device("cuda", 0)
        raw = s.solve_device(torch.from_numpy(sys_idx).to(dev), torch.from_numpy(roles).to(dev),
                             torch.from_numpy(params).to(dev))
        torch.cuda.synchronize()
        over = (raw["status"] == _abi.OVERFLOW).cpu().numpy()
        assert over.any(), "the tiny workspace must overflow"
        (on, _), (off, _) = _phased_and_not(monkeypatch, s, sys_idx, roles, params, retry=True)
    finally:
        s.close()
    _same_outputs(on, off)
    ref = {k: v[:B] for k, v in _mixed_hostref(N, 1).items()}
    _check_against_hostref(_as_result(on), ref)


@gpu
def test_failed_leaves_and_an_infeasible_root(gpu_available, monkeypatch):
    """test_dive_reuse's platoons near p_max: leaves whose QP fails in LEAF go to the redo list
    and k_bnb_ipm (the same fallback count), a failed dive leaf raises no flag, and the instance
    whose root is infeasible (a dead slot at level 0, in UPPER) stays HVP_INFEASIBLE."""
    from hvp import _abi, tables
    from hvp.solver import BatchSolver

    params, roles = _position_box_instances()
    sys_idx = np.zeros(len(roles), np.int32)
    s = BatchSolver(tables.problem(5), [_gear_pwa(800.0)])
    try:
        (on, st_on), (off, st_off) = _phased_and_not(monkeypatch, s, sys_idx, roles, params)
    finally:
        s.close()
    print(f"{st_on} phased, {st_off} one kernel")
    _same_outputs(on, off)
    assert st_on[:3] == st_off[:3] and st_on[2] > 0, "these platoons need the interior-point fallback"
    res = _as_result(on)
    assert res.status[-1] == _abi.INFEASIBLE and res.nodes[-1] == 0
    assert (res.status[:-1] == _abi.OPTIMAL).any()
    _check_against_hostref(res, _host_solve(tables.problem(5), [_gear_pwa(800.0)], sys_idx, roles, params))


@gpu
def test_band_edge_ties(gpu_available, monkeypatch):
    """v0 on a band edge (test_dive_reuse's instances): sequences tie within 1e-9, and the winner
    is the enumeration's with either kernel."""
    from hvp import tables
    from hvp.solver import BatchSolver

    params, roles, winners = _tie_instances()
    sys_idx = np.zeros(len(roles), np.int32)
    s = BatchSolver(tables.problem(5), [_gear_pwa(800.0)])
    try:
        (on, st_on), (off, st_off) = _phased_and_not(monkeypatch, s, sys_idx, roles, params)
    finally:
        s.close()
    _same_outputs(on, off)
    assert st_on[:3] == st_off[:3]
    res = _as_result(on)
    assert (res.status == 0).all()
    assert np.array_equal(res.region, winners)
    _check_against_hostref(res, _host_solve(tables.problem(5), [_gear_pwa(800.0)], sys_idx, roles, params))


@gpu
def test_two_handles_alternating_on_two_streams(gpu_available, monkeypatch):
    """Two handles with different constants (w, tightening) and capacities, solved alternately on
    two streams, three times (test_refill_uniform's case): each phased solve's outputs are those of
    its handle's problem solved alone through the one kernel, bit for bit."""
    import torch

    from hvp.solver import BatchSolver

    N, B = 5, 300
    params, roles = _mixed_inputs(N)
    params, roles = np.ascontiguousarray(params[:B]), np.ascontiguousarray(roles[:B])
    dev = torch.device("cuda", 0)
    tp, tr = torch.from_numpy(params).to(dev), torch.from_numpy(roles).to(dev)
    ts = torch.zeros(B, dtype=torch.int32, device=dev)
    kinds = (dict(w=3.0e3, tightening=0.05), dict(w=2.0e4, tightening=0.11))
    caps = (32 * B, 48 * B)

    monkeypatch.setenv("HVP_REFILL_PHASES", "0")
    alone = []
    for kw in kinds:
        s = BatchSolver(_problem(N, **kw), [_gear_pwa(800.0)])
        try:
            alone.append(s.solve(np.zeros(B, np.int32), roles, params))
        finally:
            s.close()
    monkeypatch.delenv("HVP_REFILL_PHASES")
    assert (alone[0].status == 0).all() and (alone[1].status == 0).all()
    assert not np.array_equal(alone[0].u, alone[1].u)

    solvers = []
    for kw, cap in zip(kinds, caps):
        s = BatchSolver(_problem(N, **kw), [_gear_pwa(800.0)])
        s.reserve(B, cap)
        solvers.append(s)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()
    outs = []
    for _ in range(3):
        for i in (0, 1):
            streams[i].wait_stream(torch.cuda.current_stream(dev))
            outs.append((i, solvers[i].solve_device(ts, tr, tp, stream=streams[i])))
    torch.cuda.synchronize()
    for s in solvers:
        s.close()
    for i, out in outs:
        for k in FIELDS:
            assert np.array_equal(out[k].cpu().numpy(), getattr(alone[i], k)), (i, k)


@gpu
def test_one_handle_through_changing_descriptors(gpu_available, monkeypatch):
    """The refill kernel takes its workspace descriptor by value, built per solve (launch_bnb,
    dive_list_ws): nothing of an earlier solve's descriptor may reach a later one.  N = 5, 70
    mixed-role instances (a full wave and a partial one), one system, one handle: a default solve;
    one with HVP_SPLIT_LEVELS=1 (another level-list descriptor: one bucket per level); then
    reserve(4 * B), which raises max_batch past the handle's, so hvp_reserve frees every workspace
    array and the dive list and allocates them again at four times the size (the capacity and the
    dive list's capacity change with it: both descriptors differ whatever addresses come back);
    then a default solve again.  The first and the last solve are equal bit by bit with the same
    counts (this module's three; n_spilled is printed), and all three are the host build's."""
    import torch

    from hvp import tables
    from hvp.solver import BatchSolver

    N, B = 5, 70
    params, roles = _mixed_inputs(N)
    sys_idx = np.zeros(B, np.int32)
    dev = torch.device("cuda", 0)
    ts, tr, tp = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (sys_idx, roles[:B], params[:B]))

    def solve(s):
        out = s.solve_device(ts, tr, tp)
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in out.items()}, _stats(s)

    monkeypatch.delenv("HVP_SPLIT_LEVELS", raising=False)
    s = BatchSolver(tables.problem(N), [_gear_pwa(800.0)])
    try:
        first, st_first = solve(s)
        cap_first = int(s.stats().capacity)
        monkeypatch.setenv("HVP_SPLIT_LEVELS", "1")
        one_list, st_one = solve(s)
        monkeypatch.delenv("HVP_SPLIT_LEVELS")
        s.reserve(4 * B)
        last, st_last = solve(s)
        cap_last = int(s.stats().capacity)
    finally:
        s.close()
    print(f"capacity {cap_first} -> {cap_last}; (n_candidates, qp_iterations, n_fallback, n_spilled) {st_first} first, "
          f"{st_one} one list, {st_last} last")
    assert cap_last > cap_first, "reserve(4 * B) must have reallocated the workspace"
    _same_outputs(first, last)
    assert st_first[:3] == st_last[:3]
    ref = {k: v[:B] for k, v in _mixed_hostref(N, 1).items()}
    for out in (first, one_list, last):
        _check_against_hostref(_as_result(out), ref)


def _summarize():
    spec = importlib.util.spec_from_file_location("hvp_profiles_summarize", os.path.join(ROOT, "profiles", "summarize.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_summarize_merges_the_instantiations(tmp_path):
    """A made-up stats CSV of one stream's solve at N = 5: two LEAF launches, four UPPER ones and
    one of the kernel for every level, under three full names.  The summary has one
    k_bnb_bound_refill row with N + 2 = 7 calls and the call-weighted average; the counter pass,
    one row per launch, is averaged over all launches and not per full name."""
    S = _summarize()
    names = {ph: f"void hvp_k::k_bnb_bound_refill<5, true, {ph}>(int, hvp_system const*, int)" for ph in (0, 1, 2)}
    src = tmp_path / "prof"
    (src / "trace").mkdir(parents=True)
    (src / "occ").mkdir()
    rows = [(names[1], 2, 250_000.0), (names[2], 4, 300_000.0), (names[0], 1, 320_000.0),
            ("void hvp_k::k_bnb_key<5>(hvp_detail::Workspace, int, int, int)", 1, 4_000.0)]
    with open(src / "trace" / "run_kernel_stats.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs", "StdDev"])
        for name, calls, avg in rows:
            w.writerow([name, calls, calls * avg, avg, 0.0, avg, avg, 0.0])
    with open(src / "occ" / "run_counter_collection.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Kernel_Name", "Counter_Name", "Counter_Value"])
        for name, calls, _ in rows[:3]:
            for _ in range(calls):
                w.writerow([name, "SQ_WAVE_CYCLES", {1: 100.0, 2: 200.0, 0: 400.0}[int(name.split(", ")[2][0])]])
                w.writerow([name, "SQ_WAIT_ANY", 50.0])
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    assert S.summarize(str(src), "t00", "case", here=str(out_dir))["kernels"]["k_bnb_bound_refill"]["calls"] == 7
    meta = json.load(open(out_dir / "t00_case_summary.json"))
    k = meta["kernels"]["k_bnb_bound_refill"]
    assert k["calls"] == 7
    assert k["avg_ms"] == pytest.approx((2 * 0.25 + 4 * 0.3 + 0.32) / 7, rel=1e-12)
    assert k["SQ_WAVE_CYCLES"] == pytest.approx((2 * 100.0 + 4 * 200.0 + 400.0) / 7, rel=1e-12)
    assert k["wait_frac"] == pytest.approx(50.0 / k["SQ_WAVE_CYCLES"], rel=1e-12)
    assert meta["kernels"]["k_bnb_key"] == {"avg_ms": 0.004, "calls": 1}
    assert [n for n in meta["kernels"] if "refill" in n] == ["k_bnb_bound_refill"]
