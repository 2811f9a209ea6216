"""The refill kernel's system tables (hvp_lane.h k_bnb_bound_refill): staged in LDS when the handle's
systems fit the cap (kRefillSysCap = 8), read from global memory otherwise.

Batches that MIX systems lane by lane, against the host build of the same algorithm
(lib/libhvp_hostref.so, hvp_hostref_solve_batch): regions, gears, status and per-instance node
counts equal -- the node counts also pin the child set a node's set-up now hands to its write-back
(it must be bnb_children's) -- and u, x, cost within test_gpu_parity.py's bars (cost 1e-9 relative,
u 1e-6, x 1e-4).
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SYS_CAP = 8      # hvp_lane.h kRefillSysCap
PLATOONS = 60    # x 10 vehicles = 600 instances: three 256-lane blocks, several 64-node generations
MASSES = (800.0, 1100.0)
EXTRA_MASSES = (650.0, 700.0, 900.0, 950.0, 1000.0, 1250.0)  # fill the handle past the cap


def _gear_pwa(mass):
    from hvp import tables
    from hvp.models import PwaGearVehicle

    veh = PwaGearVehicle(mass)
    return tables.system_from_dict(veh.get_discrete_system(1), tables.gears_of(veh))


@functools.lru_cache(maxsize=None)
def _systems(count):
    """3: the gear PWA vehicle at two masses and a (gear, friction region) mode table of >= 12
    modes; 9: the same three first, then six more gear PWA tables."""
    from hvp import tables
    from hvp.models import PwaFrictionVehicle, Vehicle

    # every gear's window stretched over the friction model's region boundary: 6 gears x 2 regions
    vh = [min(v + 20.0, 45.84) for v in Vehicle.vh]
    modes = tables.gear_system_from_dict(PwaFrictionVehicle(800.0).get_discrete_system(1), vh=vh)
    assert modes.n_regions >= 12
    out = [_gear_pwa(MASSES[0]), _gear_pwa(MASSES[1]), modes]
    if count > 3:
        out += [_gear_pwa(m) for m in EXTRA_MASSES]
    assert len(out) == count
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _inputs(N):
    import bench

    params, roles = bench.make_inputs(range(PLATOONS), 10, N)
    return np.ascontiguousarray(params), np.ascontiguousarray(roles.astype(np.int32))


@functools.lru_cache(maxsize=None)
def _hostref(N, count):
    """The host build's answers for the batch with sys[i] = i % count (computed once per case)."""
    from hvp import _abi, tables

    L = ctypes.CDLL(_abi.HOSTREF_PATH)
    params, roles = _inputs(N)
    B = len(roles)
    systems = _systems(count)
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
    out["sys"] = sys_idx
    return out


@functools.lru_cache(maxsize=None)
def _gpu(N, count):
    from hvp import tables
    from hvp.solver import BatchSolver

    params, roles = _inputs(N)
    sys_idx = (np.arange(len(roles)) % count).astype(np.int32)
    s = BatchSolver(tables.problem(N), list(_systems(count)))
    try:
        return s.solve(sys_idx, roles, params)
    finally:
        s.close()


def _check_against_hostref(res, ref):
    assert np.array_equal(res.status, ref["status"]), np.flatnonzero(res.status != ref["status"])[:8]
    ok = ref["status"] == 0
    assert ok.any()
    assert np.array_equal(res.region[ok], ref["region"][ok])
    assert np.array_equal(res.gear[ok], ref["gear"][ok])
    assert np.array_equal(res.nodes, ref["nodes"]), np.flatnonzero(res.nodes != ref["nodes"])[:8]
    c, ce = res.cost[ok], ref["cost"][ok]
    assert np.all(np.abs(c - ce) <= 1e-9 * np.maximum(1.0, np.abs(ce)))
    assert np.abs(res.u[ok] - ref["u"][ok]).max() <= 1e-6
    assert np.abs(res.x[ok] - ref["x"][ok]).max() <= 1e-4


@pytest.mark.parametrize("N", [2, 5, 8])
def test_mixed_systems_staged_tables(gpu_available, N):
    """Three systems in one handle, sys[i] = i % 3: neighbouring lanes index different tables of
    the LDS copy.  N = 8 also launches the kernel with the largest per-lane rows plus the tables."""
    ref = _hostref(N, 3)
    assert len(set(ref["sys"][:3])) == 3
    _check_against_hostref(_gpu(N, 3), ref)


@pytest.mark.parametrize("N", [2, 5, 8])
def test_more_systems_than_the_cap_read_global_memory(gpu_available, N):
    """SYS_CAP + 1 systems in the handle (the global-memory instantiation), sys[i] = i % 9: equal to
    the host build, and the instances that index the same table as in the three-system batch
    (i % 9 < 3) have that batch's answers and node counts, array by array."""
    count = SYS_CAP + 1
    res = _gpu(N, count)
    _check_against_hostref(res, _hostref(N, count))
    staged = _gpu(N, 3)
    same = np.flatnonzero(np.arange(len(res.status)) % count < 3)
    assert len(same) >= 190
    for k in ("status", "region", "gear", "nodes", "iters", "cost", "u", "x"):
        assert np.array_equal(getattr(res, k)[same], getattr(staged, k)[same]), k
