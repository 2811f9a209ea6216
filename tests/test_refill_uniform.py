"""The refill kernel's block-scope copy of its uniform data (hvp_lane.h k_bnb_bound_refill, RefillUni):
the problem constants, the hoisted level list and its total, written to LDS once per block by its
first thread and read from there by the event at N >= 5 (kRefillUniMinN; shorter horizons keep the
by-value arguments).  The workspace descriptor and the claim pointer stay kernel arguments, and
the active-set trips read the constants from the argument too.

Against the host build of the same algorithm (lib/libhvp_hostref.so), as test_refill_tables.py:
status, regions, gears and per-instance node counts equal, cost to 1e-9 relative, u to 1e-6, x to
1e-4.

* The problem is not the default one: accel_cnstr_tightening != 0 (dec[k] and acc[k] differ per
  step), Q_du != 0 and another w, so a wrong index into the copy's constants changes answers.
* N = 2 (the arguments' path), 5, 8 (the copy); one system (tables staged in LDS, the barrier they
  already had) and nine (the global-memory instantiation, whose barrier is new at N >= 5); roles
  mixed lane by lane; batches of 1 (most blocks claim nothing), 37 (a partial wave) and 300
  instances (several waves, a second generation).
* Two handles with different constants and workspace capacities, solved alternately on two
  streams: the copy is per launch.  Every full solve also runs the dive list's level list.
* Two buckets at a capacity where a bucket spills: the level list in the copy then has two
  non-empty buckets (n[0], n[1], seg, nb and their total are read from LDS by the claim's slot
  arithmetic); cap, split and the spill's own counters are read from the descriptor argument as
  before.  A default solve's outputs.
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from test_refill_cost_row import _inputs as _mixed_inputs
from test_refill_tables import _check_against_hostref, _gear_pwa, _systems

pytestmark = pytest.mark.gpu

BATCHES = (1, 37, 300)
FIELDS = ("status", "region", "gear", "nodes", "iters", "cost", "u", "x")


def _problem(N, w=3.0e3, tightening=0.05, q_du=0.5):
    from hvp import tables
    from hvp.params import Params

    class P(Params):
        Q_du = q_du * np.eye(1)

    P.w = w
    prob = tables.problem(N, accel_cnstr_tightening=tightening, params=P)
    assert prob.accel_tightening != 0.0 or tightening == 0.0
    assert prob.Qdu == q_du and prob.w == w
    return prob


def _tables(count):
    return (_gear_pwa(800.0),) if count == 1 else _systems(count)


@functools.lru_cache(maxsize=None)
def _inputs(N):
    """The first 300 rows of test_refill_cost_row's batch: leaders, middles and trailers side by
    side in every wave (and among the first 37 lanes)."""
    params, roles = _mixed_inputs(N)
    B = max(BATCHES)
    params, roles = np.ascontiguousarray(params[:B]), np.ascontiguousarray(roles[:B])
    assert len(set(roles[:37].tolist())) == 3
    return params, roles


@functools.lru_cache(maxsize=None)
def _hostref(N, count):
    """The host build's answers for the 300 instances (an instance's answer does not depend on its
    batch, so the smaller batches are prefixes)."""
    from hvp import _abi

    L = ctypes.CDLL(_abi.HOSTREF_PATH)
    params, roles = _inputs(N)
    B = len(roles)
    systems = _tables(count)
    S = (_abi.HvpSystem * count)(*systems)
    sys_idx = (np.arange(B) % count).astype(np.int32)
    prob = _problem(N)
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


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("count", [1, 9])
@pytest.mark.parametrize("N", [2, 5, 8])
def test_against_host_build(gpu_available, N, count, B):
    from hvp.solver import BatchSolver

    params, roles = _inputs(N)
    sys_idx = (np.arange(len(roles)) % count).astype(np.int32)
    s = BatchSolver(_problem(N), list(_tables(count)))
    try:
        res = s.solve(sys_idx[:B], roles[:B], params[:B])
    finally:
        s.close()
    ref = {k: v[:B] for k, v in _hostref(N, count).items()}
    _check_against_hostref(res, ref)


def test_constants_reach_the_answers(gpu_available):
    """The premise of the cases above: against the default problem, the tightening, Q_du and w of
    _problem each change the host build's answers for this batch."""
    from hvp import _abi, tables

    N = 5
    ref = _hostref(N, 1)
    L = ctypes.CDLL(_abi.HOSTREF_PATH)
    params, roles = _inputs(N)
    B = len(roles)
    S = (_abi.HvpSystem * 1)(*_tables(1))
    sys_idx = np.zeros(B, np.int32)
    f = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for kw in (dict(tightening=0.0), dict(q_du=0.0), dict(w=1.0e4)):
        prob = _problem(N, **kw)
        out = dict(u=np.zeros((B, N)), x=np.zeros((B, 2, N + 1)), region=np.zeros((B, N), np.int8), cost=np.zeros(B),
                   status=np.zeros(B, np.int32), nodes=np.zeros(B, np.int32), iters=np.zeros(B, np.int32))
        rc = L.hvp_hostref_solve_batch(ctypes.byref(prob), S, B, f(sys_idx), f(roles), f(params), f(out["u"]),
                                       f(out["x"]), f(out["region"]), f(out["cost"]), f(out["status"]),
                                       f(out["nodes"]), f(out["iters"]), 8)
        assert rc == 0
        # (w weighs the safe-distance slacks: it moves the costs of this batch, not its inputs)
        assert np.abs(out["cost"] - ref["cost"]).max() > 1.0, kw
        assert "w" in kw or np.abs(out["u"] - ref["u"]).max() > 1e-4, kw
    assert tables.problem(N).Qdu == 0.0


def test_two_handles_alternating_on_two_streams(gpu_available):
    """Two handles with different constants (w, tightening) and workspace capacities, solved
    alternately on two streams, three times: each solve's outputs are those of its handle's
    problem solved alone, bit for bit."""
    import torch

    from hvp.solver import BatchSolver

    N, B = 5, 300
    params, roles = _inputs(N)
    dev = torch.device("cuda", 0)
    tp, tr = torch.from_numpy(params).to(dev), torch.from_numpy(roles).to(dev)
    ts = torch.zeros(B, dtype=torch.int32, device=dev)
    kinds = (dict(w=3.0e3, tightening=0.05), dict(w=2.0e4, tightening=0.11))
    caps = (32 * B, 48 * B)

    alone = []
    for kw in kinds:
        s = BatchSolver(_problem(N, **kw), list(_tables(1)))
        try:
            alone.append(s.solve(np.zeros(B, np.int32), roles, params))
        finally:
            s.close()
    assert (alone[0].status == 0).all() and (alone[1].status == 0).all()
    assert not np.array_equal(alone[0].u, alone[1].u)

    solvers = []
    for kw, cap in zip(kinds, caps):
        s = BatchSolver(_problem(N, **kw), list(_tables(1)))
        s.reserve(B, cap)
        solvers.append(s)
    assert solvers[0].stats().capacity != solvers[1].stats().capacity
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


def test_two_buckets_with_a_spill(gpu_available, monkeypatch):
    """N = 5, two buckets, the smallest capacity at which one list per level fits plus the
    straddling slots: a bucket spills, nothing overflows, and the outputs are a default solve's."""
    import torch

    from hvp import _abi
    from hvp.solver import BatchSolver

    N, B = 5, 300
    params, roles = _inputs(N)
    dev = torch.device("cuda", 0)
    tp, tr = torch.from_numpy(params).to(dev), torch.from_numpy(roles).to(dev)
    ts = torch.zeros(B, dtype=torch.int32, device=dev)

    def solver(cap=0):  # a fresh handle per capacity (hvp_reserve only ever grows a workspace)
        s = BatchSolver(_problem(N), list(_tables(1)))
        if cap:
            s.reserve(B, cap)
        return s

    def solve(s):
        out = s.solve_device(ts, tr, tp)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    s = solver()
    ref = solve(s)
    s.close()
    assert (ref["status"] == _abi.OPTIMAL).all()

    def overflows(cap):
        s = solver(cap)
        try:
            return bool((solve(s)["status"] == _abi.OVERFLOW).any())
        finally:
            s.close()

    monkeypatch.setenv("HVP_SPLIT_LEVELS", "1")
    lo, hi = B, 16 * B
    assert not overflows(hi)
    while hi - lo > 64:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if overflows(mid) else (lo, mid)
    buckets = 2
    monkeypatch.setenv("HVP_SPLIT_LEVELS", str(buckets))
    s = solver(hi + 64 * buckets)
    out = solve(s)
    assert s.stats().n_spilled > 0, "a bucket must have needed the spill at this capacity"
    s.close()
    for k in FIELDS:
        assert np.array_equal(out[k], ref[k]), k
