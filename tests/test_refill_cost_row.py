"""The refill kernel's batched event loads (hvp_lane.h k_bnb_bound_refill, hvp_ipm.h direct_cost
BATCH): the cost's whole parameter row loaded before the step loop whatever the lane's role, the
incumbent key fetched with it, and the claimed slot's node fields loaded together.

Against the host build of the same algorithm (lib/libhvp_hostref.so), as test_refill_tables.py:
status, regions, gears and per-instance node counts equal, cost to 1e-9 relative, u to 1e-6.

* Roles mixed lane by lane: the batch of bench.make_inputs reordered so that leader, middle and
  trailer rows alternate inside every 64 lanes (a wave's role branches all diverge), with one
  system (tables staged in LDS) and with nine (the global-memory instantiation).
* The blocks of the row a role does not read (x_front without TRACK_FRONT / SAFE_FRONT, x_back
  likewise, leader_x without TRACK_LEADER) are loaded now, and must stay unused: with NaN written
  into them every output is bit-equal to the clean batch's.  NaN, not a finite sentinel: the host
  build and the library before this change both pass it (no kernel of the solve reads such a block
  arithmetically).
* Dead slots and a full bucket: the small workspaces of test_gpu_overflow.py (a reservation that
  overflows leaves dead slots, whose fields the batched claim loads and must not look at; a bucket
  that spills) give a default solve's outputs.
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from test_refill_tables import _check_against_hostref, _gear_pwa, _systems

pytestmark = pytest.mark.gpu

PLATOONS = 64  # x 10 vehicles = 640 instances: three 256-lane blocks, ten waves
FIELDS = ("status", "region", "gear", "nodes", "iters", "cost", "u", "x")


def _tables(count):
    return (_gear_pwa(800.0),) if count == 1 else _systems(count)


def _unused_blocks(roles, N):
    """(B, stride) mask of the row's doubles the lane's role does not read."""
    from hvp import _abi

    K = 2 * (N + 1)
    m = np.zeros((len(roles), 2 + 3 * K), bool)
    m[:, 2:2 + K] = ((roles & (_abi.ROLE_TRACK_FRONT | _abi.ROLE_SAFE_FRONT)) == 0)[:, None]
    m[:, 2 + K:2 + 2 * K] = ((roles & (_abi.ROLE_TRACK_BACK | _abi.ROLE_SAFE_BACK)) == 0)[:, None]
    m[:, 2 + 2 * K:] = ((roles & _abi.ROLE_TRACK_LEADER) == 0)[:, None]
    return m


@functools.lru_cache(maxsize=None)
def _inputs(N, poison=False):
    """bench.make_inputs(range(64), 10, N) reordered: of every ten consecutive lanes the second is a
    leader, the fourth a trailer and the rest middle vehicles, each kind drawn in a fixed shuffled
    order (neighbouring lanes belong to different platoons)."""
    import bench

    params, roles = bench.make_inputs(range(PLATOONS), 10, N)
    roles = roles.astype(np.int32)
    rng = np.random.default_rng(7)
    idx = np.arange(len(roles)).reshape(PLATOONS, 10)
    lead, trail, mid = rng.permutation(idx[:, 0]), rng.permutation(idx[:, 9]), rng.permutation(idx[:, 1:9].ravel())
    order = np.empty((PLATOONS, 10), np.int64)
    order[:, 1], order[:, 3] = lead, trail
    order[:, [0, 2, 4, 5, 6, 7, 8, 9]] = mid.reshape(PLATOONS, 8)
    order = order.ravel()
    assert np.array_equal(np.sort(order), np.arange(len(roles)))
    params, roles = np.ascontiguousarray(params[order]), np.ascontiguousarray(roles[order])
    assert params.shape[1] == 2 + 6 * (N + 1)
    for w in range(0, len(roles), 64):  # every wave holds the three kinds, side by side
        assert len(set(roles[w:w + 64].tolist())) == 3
        assert (np.diff(roles[w:w + 64]) != 0).sum() >= 20
    if poison:
        m = _unused_blocks(roles, N)
        assert m[:, 2:].reshape(len(roles), 3, -1).all(axis=2).any(axis=0).all()  # each block somewhere
        params[m] = np.nan
    return params, roles


@functools.lru_cache(maxsize=None)
def _hostref(N, count, poison=False):
    from hvp import _abi, tables

    L = ctypes.CDLL(_abi.HOSTREF_PATH)
    params, roles = _inputs(N, poison)
    B = len(roles)
    systems = _tables(count)
    S = (_abi.HvpSystem * count)(*systems)
    sys_idx = (np.arange(B) % count).astype(np.int32)
    prob = tables.problem(N)
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


@functools.lru_cache(maxsize=None)
def _gpu(N, count, poison=False):
    from hvp import tables
    from hvp.solver import BatchSolver

    params, roles = _inputs(N, poison)
    sys_idx = (np.arange(len(roles)) % count).astype(np.int32)
    s = BatchSolver(tables.problem(N), list(_tables(count)))
    try:
        return s.solve(sys_idx, roles, params)
    finally:
        s.close()


@pytest.mark.parametrize("count", [1, 9])
@pytest.mark.parametrize("N", [2, 5, 8])
def test_roles_mixed_lane_by_lane(gpu_available, N, count):
    _check_against_hostref(_gpu(N, count), _hostref(N, count))


@pytest.mark.parametrize("count", [1, 9])
@pytest.mark.parametrize("N", [2, 5])
def test_unused_blocks_are_never_used(gpu_available, N, count):
    """NaN in every block of the row that the lane's role does not read changes no output bit: of
    the host build first (the premise), then of the library."""
    clean_h, pois_h = _hostref(N, count), _hostref(N, count, True)
    for k in FIELDS:
        assert np.array_equal(pois_h[k], clean_h[k]), ("host build", k)
    clean, pois = _gpu(N, count), _gpu(N, count, True)
    assert (clean.status == 0).any()
    for k in FIELDS:
        a, b = getattr(pois, k), getattr(clean, k)
        assert not np.isnan(a).any(), k
        assert np.array_equal(a, b), k


def test_dead_slots_and_full_bucket(gpu_available, monkeypatch):
    """N = 5, the mixed-role batch.  (1) Two nodes per instance and level: reservations overflow,
    the claims meet dead slots, the overflowed instances are reported and their re-solve gives the
    default answers.  (2) The smallest capacity at which one list per level fits plus the
    straddling slots, four buckets: children spill, nothing overflows.  Both equal a default
    solve bit for bit."""
    import torch

    from hvp import _abi, tables
    from hvp.solver import BatchSolver

    N = 5
    params, roles = _inputs(N)
    B = len(roles)
    dev = torch.device("cuda", 0)
    tp, tr = torch.from_numpy(params).to(dev), torch.from_numpy(roles).to(dev)
    ts = torch.zeros(B, dtype=torch.int32, device=dev)
    ref = _gpu(N, 1)
    assert (ref.status == _abi.OPTIMAL).all()

    def solver(cap):  # a fresh handle per capacity (hvp_reserve only ever grows a workspace)
        s = BatchSolver(tables.problem(N), list(_tables(1)))
        s.reserve(B, cap)
        return s

    def solve(s, retry=False):
        out = s.solve_device(ts, tr, tp, retry_overflow=retry)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    def same(out):
        for k in FIELDS:
            assert np.array_equal(out[k], getattr(ref, k)), k

    tiny = solver(2 * B)
    raw = solve(tiny)
    over = raw["status"] == _abi.OVERFLOW
    assert over.any(), "the tiny workspace must overflow"
    assert (raw["status"][~over] == _abi.OPTIMAL).all()
    assert np.array_equal(raw["region"][~over], ref.region[~over])
    same(solve(tiny, retry=True))
    tiny.close()

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
    buckets = 4
    monkeypatch.setenv("HVP_SPLIT_LEVELS", str(buckets))
    s = solver(hi + 64 * buckets)
    out = solve(s)
    assert s.stats().n_spilled > 0, "the bucketed levels must have needed the spill at this capacity"
    s.close()
    same(out)
