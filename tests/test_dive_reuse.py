"""The greedy dive's leaf stands for its level-N copy (hvp_lane.h launch_bnb, Workspace::reuse).

The decentralised quadratic lane path solves every instance's dive leaf in the dive list, before
level 1.  No ancestor of that leaf is pruned before level N (each bound relaxes the leaf's QP, whose
cost is the incumbent until then), so level N used to list the same sequence and solve the same QP
again.  Now the refill event at level N - 1 leaves that child out where the dive leaf's QP
succeeded, and the dive entry takes its place in the tie rule (k_bnb_key, k_bnb_write,
k_bnb_finish) and in the per-instance counts.  HVP_DIVE_REUSE=0 solves the copy as before.

Every GPU case compares three solves: the default one, HVP_DIVE_REUSE=0 on the same handle, and the
host build of the algorithm (lib/libhvp_hostref.so), which keeps re-solving the leaf.  All output
arrays and hvp_stats.n_candidates are equal between the two GPU solves; status, regions, gears and
node counts are the host build's (cost to 1e-9 relative, u to 1e-6, x to 1e-4 as in
test_refill_tables.py); hvp_stats.qp_iterations, which counts the steps that ran, is strictly lower
with the reuse for the batches of 37 and 300.

The CPU test restates the premise on the host build: the dive's sequence is one of level N's nodes.
"""

from __future__ import annotations

import ctypes
import functools
import types

import numpy as np
import pytest

from test_refill_cost_row import _hostref as _mixed_hostref
from test_refill_cost_row import _inputs as _mixed_inputs
from test_refill_tables import _check_against_hostref, _gear_pwa, _systems

gpu = pytest.mark.gpu

BATCHES = (1, 37, 300)
FIELDS = ("status", "region", "gear", "nodes", "iters", "cost", "u", "x")
EDGE = 22.92  # the band edge between regions 3 and 4 of the gear PWA table


def _tables(count):
    return (_gear_pwa(800.0),) if count == 1 else _systems(count)


def _host_solve(prob, systems, sys_idx, roles, params):
    """hvp_hostref_solve_batch for any batch (the parametrised cases share test_refill_cost_row's)."""
    from hvp import _abi

    L = ctypes.CDLL(_abi.HOSTREF_PATH)
    B, N = len(roles), int(prob.N)
    S = (_abi.HvpSystem * len(systems))(*systems)
    out = dict(u=np.zeros((B, N)), x=np.zeros((B, 2, N + 1)), region=np.zeros((B, N), np.int8), cost=np.zeros(B),
               status=np.zeros(B, np.int32), nodes=np.zeros(B, np.int32), iters=np.zeros(B, np.int32))
    f = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = L.hvp_hostref_solve_batch(ctypes.byref(prob), S, B, f(sys_idx), f(roles), f(params), f(out["u"]),
                                   f(out["x"]), f(out["region"]), f(out["cost"]), f(out["status"]), f(out["nodes"]),
                                   f(out["iters"]), 8)
    assert rc == 0
    gear_tab = np.array([[s.gear[r] for r in range(16)] for s in systems])
    out["gear"] = np.where(out["region"] >= 0, gear_tab[sys_idx[:, None], np.maximum(out["region"], 0)], 0)
    return out


def _bnb_leaves(prob, table, role, prm):
    """(the dive converged, its sequence, level N's sequences) of one instance's search on the host
    build; sequences as tuples of regions."""
    from hvp import _abi

    L = ctypes.CDLL(_abi.HOSTREF_PATH)
    N = int(prob.N)
    ok, code = ctypes.c_int32(0), ctypes.c_uint64(0)
    cap = 1 << 14
    leaves = np.zeros(cap, np.uint64)
    prm = np.ascontiguousarray(prm, dtype=np.float64)
    n = L.hvp_hostref_bnb_leaves(ctypes.byref(prob), ctypes.byref(table), int(role), prm.ctypes.data_as(ctypes.c_void_p),
                                 ctypes.byref(ok), ctypes.byref(code), leaves.ctypes.data_as(ctypes.c_void_p), cap)
    assert 0 <= n <= cap
    seq = lambda c: tuple((int(c) >> (4 * k)) & 15 for k in range(N))  # noqa: E731
    return bool(ok.value), seq(code.value), [seq(c) for c in leaves[:n]]


def _on_and_off(monkeypatch, solver, sys_idx, roles, params, retry=False):
    """The default solve and the HVP_DIVE_REUSE=0 solve on the same handle: (outputs, stats) each."""
    import torch

    dev = torch.device("cuda", 0)
    ts, tr, tp = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (sys_idx, roles, params))
    runs = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("HVP_DIVE_REUSE", "0")
        else:
            monkeypatch.delenv("HVP_DIVE_REUSE", raising=False)
        out = solver.solve_device(ts, tr, tp, retry_overflow=retry)
        torch.cuda.synchronize()
        st = solver.stats()
        runs.append(({k: v.clone() for k, v in out.items()}, (int(st.n_candidates), int(st.qp_iterations),
                                                               int(st.n_fallback))))
    monkeypatch.delenv("HVP_DIVE_REUSE", raising=False)
    return runs


def _same_outputs(a, b):
    import torch

    assert set(a) == set(b) and set(FIELDS) <= set(a)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _as_result(out):
    return types.SimpleNamespace(**{k: v.cpu().numpy() for k, v in out.items()})


@gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("count", [1, 9])
@pytest.mark.parametrize("N", [2, 5, 8])
def test_reuse_against_resolve_and_host_build(gpu_available, monkeypatch, N, count, B):
    """Roles mixed lane by lane (test_refill_cost_row's batch), one system (tables in LDS) and nine
    (the global-memory instantiation); a batch of 1, a partial wave, several waves."""
    from hvp import tables
    from hvp.solver import BatchSolver

    params, roles = _mixed_inputs(N)
    sys_idx = (np.arange(len(roles)) % count).astype(np.int32)
    s = BatchSolver(tables.problem(N), list(_tables(count)))
    try:
        (on, st_on), (off, st_off) = _on_and_off(monkeypatch, s, sys_idx[:B], roles[:B], params[:B])
    finally:
        s.close()
    _same_outputs(on, off)
    print(f"N={N} count={count} B={B}: qp_iterations {st_on[1]} with reuse, {st_off[1]} without; "
          f"n_candidates {st_on[0]}, {st_off[0]}; nodes {int(on['nodes'].sum())}")
    assert st_on[0] == st_off[0], "n_candidates counts the tree's nodes"
    assert st_on[1] <= st_off[1]
    if B > 1:
        assert st_on[1] < st_off[1], "the reused leaves' steps did not run"
    ref = {k: v[:B] for k, v in _mixed_hostref(N, count).items()}
    _check_against_hostref(_as_result(on), ref)


# (gap between the three vehicles, the leader's speed, vehicle, the dive's sequence is the
# lexicographically smaller / larger of the tied ones): every vehicle at EDGE, N = 5.  Found on the
# CPU: the oracle's enumeration for the tied set, the host build for the dive's sequence.
TIES = (
    (25.0, EDGE, 2, "smaller"),        # (3,3,3,2,2) against (4,3,3,2,2)
    (40.0, EDGE, 2, "smaller"),        # (3,3,3,3,3) against (4,3,3,3,3)
    (60.0, EDGE, 2, "smaller"),        # (3,5,5,5,5) against (4,5,5,5,5)
    (25.0, EDGE, 1, "larger"),         # (3,4,4,4,4) among the 32 sequences over {3, 4}: (3,3,3,3,3) wins
    (25.0, EDGE - 0.5, 0, "larger"),
    (25.0, EDGE + 1.5, 1, "larger"),
)


@functools.lru_cache(maxsize=None)
def _tie_instances():
    """(params, roles, the enumeration's winners) of TIES, with the premise checked: the dive's
    sequence is within 1e-9 of the minimum, next to at least one other, on the stated side."""
    import oracle as O
    from hvp import tables
    from instances import decent_instances, leader_window, split_params

    N = 5
    sysd = O.gear_pwa_system(800.0)
    prob, table = tables.problem(N), _gear_pwa(800.0)
    P, R, W = [], [], []
    for gap, vl, i, side in TIES:
        state = np.array([3000.0, EDGE, 3000.0 - gap, EDGE, 3000.0 - 2 * gap, EDGE])
        params, roles = decent_instances(state, N, leader_window(N, v=vl))
        p, rl = np.ascontiguousarray(params[i]), int(roles[i])
        x0, xf, xb, xl = split_params(p, N)
        r = O.solve_miqp(sysd, O.Cfg(), N, rl, x0, xf, xb, xl, want_candidates=True)
        assert r.status == 0
        best = r.cand_obj.min()
        tied = sorted(tuple(int(v) for v in r.cand_sigma[t])
                      for t in np.flatnonzero(r.cand_obj <= best + 1e-9 * max(1.0, abs(best))))
        ok, dive, leaves = _bnb_leaves(prob, table, rl, p)
        assert ok and dive in tied and len(tied) >= 2, (gap, vl, i, dive, tied)
        assert (dive == tied[0]) == (side == "smaller"), (gap, vl, i, dive, tied[0])
        assert tuple(int(v) for v in r.sigma) == tied[0]
        P.append(p)
        R.append(rl)
        W.append(tied[0])
    return np.array(P), np.array(R, np.int32), np.array(W, np.int8)


@gpu
def test_ties_with_the_dive_sequence(gpu_available, monkeypatch):
    """v0 on a band edge: the dive's sequence ties with others within 1e-9.  Where it is the
    smallest the dive entry must win (no level-N leaf holds it any more); where it is not, a level-N
    leaf must win over it.  The winner is the enumeration's."""
    from hvp import tables
    from hvp.solver import BatchSolver

    params, roles, winners = _tie_instances()
    sys_idx = np.zeros(len(roles), np.int32)
    s = BatchSolver(tables.problem(5), [_gear_pwa(800.0)])
    try:
        (on, st_on), (off, st_off) = _on_and_off(monkeypatch, s, sys_idx, roles, params)
    finally:
        s.close()
    _same_outputs(on, off)
    assert st_on[0] == st_off[0] and st_on[1] < st_off[1]
    res = _as_result(on)
    assert (res.status == 0).all()
    assert np.array_equal(res.region, winners)
    _check_against_hostref(res, _host_solve(tables.problem(5), [_gear_pwa(800.0)], sys_idx, roles, params))


def _position_box_instances(N=5):
    """test_gpu_parity.py's vehicles near p_max (leaves the active-set method hands to the interior
    point, the dive's among them), and one with p_1 beyond p_max: no root node at all."""
    import oracle as O

    P, R = [], []
    for p0, v0, vl in [(9870, 30, 40), (9800, 25, 45), (9900, 20, 30), (9700, 35, 45), (9890, 22, 32), (9990, 20, 30)]:
        lead = np.stack([p0 + 60 + vl * np.arange(N + 1), np.full(N + 1, float(vl))])
        xb = O.constant_velocity_prediction(p0 - 80, v0, N)
        P.append(np.concatenate([[p0, v0], np.zeros(2 * (N + 1)), xb.ravel(), lead.ravel()]))
        R.append(O.role_bits(0, 2))
    return np.array(P, dtype=np.float64), np.array(R, np.int32)


@gpu
def test_failed_dive_leaf_is_solved_again(gpu_available, monkeypatch):
    """A dive leaf whose QP failed sets no incumbent and stands for nothing: its level-N copy is
    listed, raises the flag and goes to the interior point as before -- the same fallback count,
    statuses and costs as with the switch off.  The instance without a root stays HVP_INFEASIBLE."""
    from hvp import _abi, tables
    from hvp.solver import BatchSolver

    params, roles = _position_box_instances()
    sys_idx = np.zeros(len(roles), np.int32)
    s = BatchSolver(tables.problem(5), [_gear_pwa(800.0)])
    try:
        (on, st_on), (off, st_off) = _on_and_off(monkeypatch, s, sys_idx, roles, params)
    finally:
        s.close()
    _same_outputs(on, off)
    assert st_on[0] == st_off[0]
    assert st_on[2] == st_off[2] and st_off[2] > 0, "these platoons need the interior-point fallback"
    res = _as_result(on)
    assert res.status[-1] == _abi.INFEASIBLE and res.nodes[-1] == 0
    assert (res.status[:-1] == _abi.OPTIMAL).any()
    _check_against_hostref(res, _host_solve(tables.problem(5), [_gear_pwa(800.0)], sys_idx, roles, params))


@gpu
@pytest.mark.parametrize("env", [("HVP_SPLIT_LEVELS", "1"), ("HVP_SPLIT_LEVELS", "4"), ("HVP_PASS_THROUGH", "1"),
                                 ("HVP_ROOT_REFILL", "0")])
def test_with_the_other_switches(gpu_available, monkeypatch, env):
    """One list per level, four buckets, pass-through nodes (a level-(N-1) pass-through node leaves
    the child out as any other), and k_bnb_root in place of the dive list, where the reuse is
    silently off: the same outputs with and without HVP_DIVE_REUSE=0, and the unswitched default
    solve's."""
    from hvp import tables
    from hvp.solver import BatchSolver

    N, B = 5, 300
    params, roles = _mixed_inputs(N)
    params, roles = params[:B], roles[:B]
    sys_idx = np.zeros(B, np.int32)
    s = BatchSolver(tables.problem(N), [_gear_pwa(800.0)])
    try:
        (plain, st_plain), _ = _on_and_off(monkeypatch, s, sys_idx, roles, params)
        monkeypatch.setenv(*env)
        (on, st_on), (off, st_off) = _on_and_off(monkeypatch, s, sys_idx, roles, params)
    finally:
        s.close()
    _same_outputs(on, off)
    assert st_on[0] == st_off[0]
    if env[0] == "HVP_ROOT_REFILL":
        assert st_on[1] == st_off[1], "no dive list: nothing to reuse"
    else:
        assert st_on[1] < st_off[1]
    ref = {k: v[:B] for k, v in _mixed_hostref(N, 1).items()}
    _check_against_hostref(_as_result(on), ref)
    if env[0] == "HVP_PASS_THROUGH":  # (costs to rounding there: test_gpu_parity.py)
        assert st_on[0] < st_plain[0]
        for k in ("status", "region", "gear", "nodes"):
            assert np.array_equal(on[k].cpu().numpy(), plain[k].cpu().numpy()), k
    else:
        assert st_on[0] == st_plain[0]
        _same_outputs(on, plain)


@gpu
def test_small_workspace_after_the_retry(gpu_available, monkeypatch):
    """Two slots per instance and level (test_gpu_overflow.py): level N is shorter with the reuse,
    so other instances may overflow; after the retry of the overflowed ones the answers are the
    same, and the host build's."""
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
        assert (raw["status"] == _abi.OVERFLOW).any(), "the tiny workspace must overflow"
        (on, _), (off, _) = _on_and_off(monkeypatch, s, sys_idx, roles, params, retry=True)
    finally:
        s.close()
    _same_outputs(on, off)
    ref = {k: v[:B] for k, v in _mixed_hostref(N, 1).items()}
    _check_against_hostref(_as_result(on), ref)


def test_the_dive_sequence_is_a_level_n_node():
    """The claim the reuse rests on, on the host build, for 320 flagship instances (bench.py's
    first 32 platoons, n = 10, N = 5): every instance whose dive leaf converged has that sequence
    among its level-N nodes, exactly once.  No such instance may miss it."""
    import bench
    from hvp import tables

    N = 5
    params, roles = bench.make_inputs(range(32), 10, N)
    prob, table = tables.problem(N), _gear_pwa(800.0)
    dived = missing = 0
    for p, rl in zip(params, roles):
        ok, dive, leaves = _bnb_leaves(prob, table, int(rl), p)
        if not ok:
            continue
        dived += 1
        missing += leaves.count(dive) != 1
        assert len(set(leaves)) == len(leaves)
    assert dived >= len(roles) // 2, "the flagship instances dive"
    assert missing == 0, (missing, dived)
