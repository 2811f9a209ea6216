"""The event-based kernels at long horizons and stage by stage (include/hvp_event.h).

Solve kernel.  The oracle has no event-based problem, but an exact reduction needs none: take the
oracle's optimum (x*, u*, sigma*) of a centralised MIQP of n vehicles and hold every vehicle
outside [lo, lo + m) at its optimal trajectory.  What is left is the local problem of hvp_event.h
over vehicles lo .. lo + m - 1 with x_f2 = x*[lo - 1] (lo > 0), x_b2 = x*[lo + m] (lo + m < n) and
leader = L - lo where the leader index falls inside the block; every other term of the joint
objective is a constant.  The local solve must therefore return sigma*, u*, x* of the block and
the numpy restatement of the local objective (test_event._objective) on them.  The fixtures
event_*.npz (tests/golden/make_golden.py event) are such joint optima up to N = 16, so the blocks
run k_event_bnb at V = m N up to 48 of 64 lanes: segments across lane 16 (V = 18, 22, 24), across
lane 32 (V = 33, 36), V = 32 exactly and V = 48, with no, one and both boundaries.

  CPU: the projection itself, with the oracle where it can solve the block (m = 1 with both
  boundaries: the decentralised MIQP; m = 2, 3 behind a fixed front vehicle: the centralised MIQP
  with real_vehicle_as_reference).
  GPU: every contiguous block of every stored platoon at the parity bar of DESIGN section 7, the
  output buffers pre-filled with sentinels (the slots of vehicles >= m are part of the contract).

Stage kernels.  hvp_event_gather / _select copy and compare, they do not compute: each is compared
element by element with a numpy restatement of the header's text, on inputs with a distinct value
per element, over a second thread block, every leader index and the winner rule's edge cases.
"""

from __future__ import annotations

import ctypes
import functools
import glob
import os
import time

import numpy as np
import pytest

import oracle as O
from golden_io import GOLDEN, load
from test_event import CFGS, _objective, _rows_hold, _same, _solver

EVENT = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "event_*.npz"))) + ["cent_gear_n3_N4.npz"]
SENT8, SENT32 = 0x55, 0x55555555


def _cfg(v) -> O.Cfg:
    v = np.asarray(v, dtype=float)
    return O.Cfg(Qx=tuple(v[0:4]), Qu=v[4], Qdu=v[5], w=v[6], a_acc=v[7], a_dec=v[8], ts=v[9], d_safe=v[10],
                 tight=v[11], d0=v[12], t0=v[13])


def _horizon(name) -> int:
    return int(load(name)["N"])


def _blocks(fx):
    """Every contiguous block [lo, lo + m), m = 1, 2, 3, of every stored platoon -- the blocks the
    agents' layout never produces included: (platoon, lo, m, (m, has_f2, has_b2, leader))."""
    n = int(fx["n"])
    out = []
    for p in range(len(fx["x0"])):
        assert fx["exp_status"][p] == 0 and not fx["lsp"][p]
        L = int(fx["leader_index"][p])
        for m in (1, 2, 3):
            for lo in range(n - m + 1):
                out.append((p, lo, m, (m, int(lo > 0), int(lo + m < n), L - lo if lo <= L < lo + m else -1)))
    return out


def _projection(fx, c, N, p, lo, m, desc):
    """The block's data and expected answer: (x0 (m, 2), x_f2, x_b2, leader_x (None where unused),
    sigma*, u*, x* of the block, the local objective on them)."""
    X, U = fx["exp_x"][p], fx["exp_u"][p]
    xf2 = X[lo - 1] if desc[1] else None
    xb2 = X[lo + m] if desc[2] else None
    xl = fx["leader_x"][p] if desc[3] >= 0 else None
    zero = np.zeros((2, N + 1))
    J = _objective(c, desc, X[lo:lo + m], U[lo:lo + m], zero if xf2 is None else xf2, zero if xb2 is None else xb2,
                   zero if xl is None else xl)
    return fx["x0"][p, lo:lo + m], xf2, xb2, xl, fx["exp_region"][p, lo:lo + m], U[lo:lo + m], X[lo:lo + m], J


# ====================================================================== CPU
def test_fixture_shapes():
    """The shapes the long-horizon checks rest on are all there: n = 3 at N = 6 with the leader on
    every vehicle, N = 11 and N = 16 (three platoons or more, a leader off vehicle 0); n = 4 at
    N = 8, 12, 16; n = 5 at N = 8 (two platoons or more); the gear model at n = 4."""
    have = {}
    for name in EVENT:
        fx = load(name)
        have[(int(fx["n"]), int(fx["N"]), int(fx["model"]))] = fx
        assert (fx["exp_status"] == 0).all(), name
        assert np.array_equal(fx["cfg"], (CFGS["time"] if name.startswith("event_") else CFGS["space"]).vector())
    assert sorted(have[(3, 6, 0)]["leader_index"].tolist()) == [0, 1, 2]
    assert (3, 11, 0) in have
    assert len(have[(3, 16, 0)]["x0"]) >= 3 and (have[(3, 16, 0)]["leader_index"] > 0).any()
    assert {(4, 8, 0), (4, 12, 0), (4, 16, 0), (4, 4, 1), (3, 4, 1)} <= set(have)
    assert len(have[(5, 8, 0)]["x0"]) >= 2
    descs = [(d, N) for (_, N, _), fx in have.items() for _, _, _, d in _blocks(fx)]
    assert {18, 32, 33, 36, 48} <= {d[0] * N for d, N in descs}  # lanes in use, any boundaries
    both = {m: max(N for d, N in descs if d[0] == m and d[1] and d[2]) for m in (1, 2, 3)}
    assert both[1] == 16 and both[2] == 16 and both[3] >= 8  # V = 16, 32 and 24 (33 with the n = 5, N = 11 set)


def test_validate_accepts_three_vehicles_at_the_longest_horizon():
    """hvp_event.h promises the single-wave search for V = m N <= 48 while hvp_event_validate refuses
    only m N > 64: through a handle the two cannot disagree (hvp_create caps N at HVP_MAX_N = 16),
    and the largest shape a handle allows, m = 3 at N = 16, is accepted."""
    from hvp import _abi
    from hvp.cent import cent_problem
    from hvp.event import make_desc

    lib = _abi.load()
    assert _abi.MAX_N == 16
    items = [(3, 1, 1, 1), (3, 0, 0, -1), (3, 0, 1, 2)]
    assert lib.hvp_event_validate(ctypes.byref(cent_problem(16)), len(items), make_desc(items)) == 0


def _oracle_projection(name):
    fx = load(name)
    N, model, c = int(fx["N"]), int(fx["model"]), _cfg(fx["cfg"])
    mk = O.gear_friction_mld_system if model == 1 else O.gear_pwa_system
    zero = np.zeros((2, N + 1))
    both = O.ROLE_SAFE_FRONT | O.ROLE_SAFE_BACK | O.ROLE_TRACK_FRONT | O.ROLE_TRACK_BACK
    checked = 0
    if N >= 8:  # beyond exhaustive enumeration of the region sequences
        O.set_method(O.METHOD_BNB)
    try:
        for p, lo, m, desc in _blocks(fx):
            x0, xf2, xb2, xl, sigma, u, x, J = _projection(fx, c, N, p, lo, m, desc)
            osys = [mk(float(mass)) for mass in fx["masses"][p, lo:lo + m]]
            if m == 1 and desc[1] and desc[2]:
                # the decentralised follower between x_f2 and x_b2, tracking the leader too where it is the leader
                role = both | (O.ROLE_TRACK_LEADER if desc[3] == 0 else 0)
                r = O.solve_miqp(osys[0], c, N, role, x0[0], xf2, xb2, zero if xl is None else xl)
            elif m >= 2 and desc[1] and not desc[2] and desc[3] < 0:
                # the centralised MIQP of the block behind the fixed vehicle lo - 1
                r = O.solve_cent(osys, c, N, x0.reshape(-1), xf2, 0, True)
            else:
                continue
            tag = (name, p, lo, m)
            assert r.status == 0, tag
            assert np.array_equal(np.reshape(r.sigma, (m, N)), sigma), (tag, r.sigma, sigma, r.cost, J)
            assert abs(r.cost - J) <= 1e-9 * abs(J), (tag, r.cost, J)
            assert np.abs(np.reshape(r.u, (m, N)) - u).max() <= 1e-6, tag
            assert np.abs(np.reshape(r.x, (m, 2, N + 1)) - x).max() <= 1e-4, tag
            checked += 1
    finally:
        O.set_method(O.METHOD_ENUMERATE)
    assert checked >= len(fx["x0"]), (name, checked)  # every platoon has at least one such block
    print(f"{name}: {checked} blocks re-solved by the oracle")


@pytest.mark.parametrize("name", [pytest.param(f, marks=pytest.mark.slow) if _horizon(f) >= 11 else f for f in EVENT])
def test_oracle_solves_the_projected_blocks(name):
    """The answer the GPU test expects is the oracle's: the blocks the oracle can state are solved
    by it as problems of their own and return the joint optimum's block (regions exact, cost 1e-9
    relative to the numpy objective, u 1e-6, x 1e-4)."""
    _oracle_projection(name)


# ====================================================================== GPU: the solve kernel
def _sentinel_outputs(s, B):
    import torch

    out = s.alloc_outputs(B)
    for t in out.values():
        if t.dtype == torch.float64:
            t.fill_(float("nan"))
        else:
            t.fill_(SENT8 if t.dtype == torch.int8 else SENT32)
    return out


def _solve_into_sentinels(s, items, sysv, params, max_nodes=0):
    """EventSolver.solve with the output buffers passed in pre-filled (alloc_outputs is torch.empty,
    and a fresh allocation is often zero already): (result with the raw cost, seconds)."""
    import torch

    from hvp.event import EventResult, make_desc

    B = len(items)
    out = _sentinel_outputs(s, B)
    desc = make_desc(items)
    sv, pv = s._to(np.reshape(sysv, (B, 3)), np.int32), s._to(np.reshape(params, (B, s.stride)), np.float64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.solve_device(desc, sv, pv, max_nodes, out)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return EventResult(**{k: v.cpu().numpy() for k, v in out.items()}), dt


def _pack_blocks(fx, c, N, blocks, sys_of):
    from hvp.event import pack_params

    items, sysv, params, refs = [], [], [], []
    for p, lo, m, desc in blocks:
        x0, xf2, xb2, xl, sigma, u, x, J = _projection(fx, c, N, p, lo, m, desc)
        items.append(desc)
        idx = np.zeros(3, np.int32)
        idx[:m] = [sys_of(p, v) for v in range(lo, lo + m)]
        sysv.append(idx)
        params.append(pack_params(N, x0, xf2, xb2, xl))
        refs.append((sigma, J, u, x))
    return items, np.stack(sysv), np.stack(params), refs


@pytest.mark.gpu
@pytest.mark.parametrize("name", EVENT)
def test_gpu_blocks_of_joint_optimum(gpu_available, name):
    """Every contiguous block of every stored platoon, one batch per fixture: status 0, regions and
    gears exact, cost 1e-9 relative to the numpy objective on the oracle's projection, u 1e-6,
    x 1e-4; the hard rows hold; hvp_event_evaluate_batch prices the returned (x, u, gear) at the
    same cost; whole platoons (m = n = 3) visit the oracle's number of QPs; for m < 3 every element
    of the unused slots is as the header says (u, x zero, region -1, gear 0) over the sentinels."""
    fx = load(name)
    N, n, model, c = int(fx["N"]), int(fx["n"]), int(fx["model"]), _cfg(fx["cfg"])
    s, _ = _solver(c, N, fx["masses"].reshape(-1), model)
    blocks = _blocks(fx)
    items, sysv, params, refs = _pack_blocks(fx, c, N, blocks, lambda p, v: p * n + v)
    res, dt = _solve_into_sentinels(s, items, sysv, params)
    ev, ev_status = s.evaluate(items, sysv, params, res.x, res.u, res.gear if model == 1 else None)
    for b, ((p, lo, m, desc), (sigma, J, u, x)) in enumerate(zip(blocks, refs)):
        tag = (name, p, lo, m)
        _same(res, b, m, sigma, J, u, x, tag)
        assert np.array_equal(res.gear[b, :m], fx["exp_gear"][p, lo:lo + m]), tag
        assert (res.gear[b, m:] == 0).all(), tag
        assert 0 < res.nodes[b] != SENT32 and 0 < res.iters[b] != SENT32, tag
        if m == n:
            assert res.nodes[b] == fx["exp_nodes"][p], (tag, res.nodes[b], fx["exp_nodes"][p])
        for j in range(m):
            _rows_hold(c, s.tables[sysv[b, j]], res.x[b, j], res.u[b, j], res.region[b, j], N)
            assert np.array_equal(res.x[b, j, :, 0], fx["x0"][p, lo + j]), tag
        assert ev_status[b] == 0 and abs(ev[b] - res.cost[b]) <= 1e-9 * abs(res.cost[b]), (tag, ev[b], res.cost[b])
    lanes = sorted({d[0] * N for _, _, _, d in blocks})
    print(f"{name}: {len(blocks)} blocks compared, V in {lanes}, solve batch {dt:.3f} s, "
          f"most QPs {int(res.nodes.max())}")


@pytest.mark.gpu
def test_gpu_node_cap_leaves_the_no_solution_outputs(gpu_available):
    """max_nodes = 1 on blocks that need more: HVP_MAXITER, cost 1e300, u zero, the
    constant-velocity trajectory, region -1, gear 0 -- and the unused slots zero -- over sentinels."""
    from hvp import _abi

    fx = load("event_n3_N6.npz")
    N, n, c = int(fx["N"]), int(fx["n"]), _cfg(fx["cfg"])
    s, _ = _solver(c, N, fx["masses"].reshape(-1))
    blocks = [bl for bl in _blocks(fx) if bl[0] == 1]  # one platoon: m = 1 (x3), 2 (x2), 3
    items, sysv, params, _ = _pack_blocks(fx, c, N, blocks, lambda p, v: p * n + v)
    full, _ = _solve_into_sentinels(s, items, sysv, params)
    assert (full.status == 0).all() and (full.nodes > 1).all(), full.nodes
    res, _ = _solve_into_sentinels(s, items, sysv, params, max_nodes=1)
    for b, (p, lo, m, desc) in enumerate(blocks):
        assert res.status[b] == _abi.MAXITER and res.cost[b] == 1e300, (b, res.status[b], res.cost[b])
        want = np.zeros((3, 2, N + 1))
        for j in range(m):
            p0, v0 = fx["x0"][p, lo + j]
            want[j] = [p0 + c.ts * v0 * np.arange(N + 1), np.full(N + 1, v0)]
        assert np.array_equal(res.x[b], want), (b, res.x[b], want)
        assert not res.u[b].any() and (res.region[b] == -1).all() and (res.gear[b] == 0).all(), b
        assert 1 <= res.nodes[b] != SENT32, (b, res.nodes[b])


@pytest.mark.gpu
def test_gpu_event_and_centralised_solves_share_one_handle(gpu_available):
    """hvp_event_solve_batch uses the DFS frames and tie rows of hvp_cent_solve_batch on the same
    handle.  Centralised and event solves interleaved on one handle (N = 5), batches growing and
    shrinking: the platoons of cent_n4_N5.npz against the fixture, and their blocks against the
    projection of the same optima."""
    from hvp import _abi
    from hvp.event import EventSolver
    from test_cent import _product

    fx = load("cent_n4_N5.npz")
    N, c = int(fx["N"]), _cfg(fx["cfg"])
    cs, sys_idx = _product(fx)
    es = EventSolver.__new__(EventSolver)  # the event entry points on the centralised solver's handle
    es._lib, es._h, es.N, es.problem, es.n_systems, es.device = cs._lib, cs._h, N, cs.problem, cs.n_systems, cs.device
    es.stride = _abi.event_params_stride(N)
    try:
        blocks = _blocks(fx)
        items, sysv, params, refs = _pack_blocks(fx, c, N, blocks, lambda p, v: int(sys_idx[p, v]))

        def cent(sel):
            res = cs.solve(sys_idx[sel], fx["x0"][sel], fx["leader_x"][sel], 0, False)
            for j, p in enumerate(sel):
                assert res.status[j] == 0 and np.array_equal(res.region[j], fx["exp_region"][p]), p
                assert abs(res.cost[j] - fx["exp_cost"][p]) <= 1e-9 * abs(fx["exp_cost"][p]), p
                assert np.abs(res.u[j] - fx["exp_u"][p]).max() <= 1e-6 and res.nodes[j] == fx["exp_nodes"][p], p

        def event(sel):
            res, _ = _solve_into_sentinels(es, [items[b] for b in sel], sysv[sel], params[sel])
            for j, b in enumerate(sel):
                _same(res, j, blocks[b][2], *refs[b], ("shared handle", blocks[b]))

        assert (fx["leader_index"] == 0).all() and not fx["lsp"].any()
        P, B = len(fx["x0"]), len(blocks)
        cent(np.arange(2))
        event(np.arange(B))          # grows the shared buffers past the centralised batch's
        cent(np.arange(P))
        event(np.arange(0, B, 3))    # new descriptors, a smaller batch
        cent(np.arange(P)[::-1])
        event(np.arange(B)[::-1])
    finally:
        es._h = None  # the handle is the centralised solver's to destroy


# ====================================================================== GPU: the coordinator's stages
@functools.lru_cache(maxsize=None)
def _stage_solver(N):
    return _solver(CFGS["space"], N, [800.0])[0]


def _distinct(rng, *shapes):
    """float64 arrays of the given shapes, no value used twice over all of them (none zero)."""
    sizes = [int(np.prod(sh)) for sh in shapes]
    vals = (rng.permutation(sum(sizes)) + 1.0) * 0.25
    out, at = [], 0
    for sh, k in zip(shapes, sizes):
        out.append(vals[at:at + k].reshape(sh).copy())
        at += k
    return out


def _gather_restated(P, n, N, leader, x, vsys, xg, ug, gg, lx):
    """hvp_event_gather as include/hvp_event.h words it (instance b = p n + i; agent i's vehicles
    [i-1, i, i+1] clipped to the platoon; stores vehicle-major)."""
    K = 2 * (N + 1)
    B = P * n
    sys3 = np.zeros((B, 3), np.int32)
    params = np.zeros((B, 6 + 3 * K))
    x_guess, u_guess = np.zeros((B, 3, 2, N + 1)), np.zeros((B, 3, N))
    gear_guess = np.zeros((B, 3, N), np.int8)
    for p in range(P):
        for i in range(n):
            b = p * n + i
            lo, hi = max(i - 1, 0), min(i + 1, n - 1)
            for j, v in enumerate(range(lo, hi + 1)):
                sys3[b, j] = vsys[p, v]
                params[b, 2 * j:2 * j + 2] = x[p, 2 * v:2 * v + 2]
                x_guess[b, j], u_guess[b, j] = xg[v, p], ug[v, p]
                if gg is not None:
                    gear_guess[b, j] = gg[v, p]
            if i >= 2:
                params[b, 6:6 + K] = xg[i - 2, p].reshape(K)
            if i + 2 < n:
                params[b, 6 + K:6 + 2 * K] = xg[i + 2, p].reshape(K)
            if leader - 1 <= i <= leader + 1:
                params[b, 6 + 2 * K:] = lx[p].reshape(K)
    return sys3, params, x_guess, u_guess, gear_guess


@pytest.mark.gpu
@pytest.mark.parametrize("P,n,N", [(53, 5, 3), (3, 2, 3), (3, 3, 3), (2, 4, 3), (2, 6, 3), (3, 3, 16)])
def test_gpu_gather_matches_restatement(gpu_available, P, n, N):
    """hvp_event_gather, every leader index, with and without the gear store, all five outputs
    pre-filled with sentinels: every element equals the restatement (unused slots zero; their sys
    entries a system index of the same platoon), gg = None leaves gear_guess untouched, and
    hvp_event_layout's descriptors name exactly the blocks that are filled.  (53, 5): 265 items,
    two thread blocks."""
    import torch

    from hvp.event import platoon_desc

    s = _stage_solver(N)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    K, B = 2 * (N + 1), P * n
    for leader in range(n):
        for with_gears in (True, False):
            rng = np.random.default_rng(100 * n + 10 * leader + with_gears)
            x, xg, ug, lx = _distinct(rng, (P, 2 * n), (n, P, 2, N + 1), (n, P, N), (P, 2, N + 1))
            vsys = (rng.permutation(B) + 7).astype(np.int32).reshape(P, n)
            gg = rng.integers(1, 7, (n, P, N)).astype(np.int8)
            sys3 = torch.full((B, 3), SENT32, dtype=torch.int32, device=dev)
            params = torch.full((B, s.stride), float("nan"), dtype=torch.float64, device=dev)
            x_guess = torch.full((B, 3, 2, N + 1), float("nan"), dtype=torch.float64, device=dev)
            u_guess = torch.full((B, 3, N), float("nan"), dtype=torch.float64, device=dev)
            gear_guess = torch.full((B, 3, N), SENT8, dtype=torch.int8, device=dev)
            s.gather_device(n, leader, t(x), t(vsys), t(xg), t(ug), t(gg) if with_gears else None, t(lx), sys3, params,
                            x_guess, u_guess, gear_guess)
            torch.cuda.synchronize()
            w_sys, w_params, w_x, w_u, w_g = _gather_restated(P, n, N, leader, x, vsys, xg, ug, gg if with_gears else None, lx)
            tag = (P, n, N, leader, with_gears)
            got_sys, got_params = sys3.cpu().numpy(), params.cpu().numpy()
            got_x = x_guess.cpu().numpy()
            assert np.array_equal(got_params, w_params), tag
            assert np.array_equal(got_x, w_x) and np.array_equal(u_guess.cpu().numpy(), w_u), tag
            assert np.array_equal(gear_guess.cpu().numpy(), w_g if with_gears else np.full((B, 3, N), SENT8, np.int8)), tag
            desc = platoon_desc(n, leader, P)
            for b in range(B):
                d, p = desc[b], b // n
                assert np.array_equal(got_sys[b, :d.m], w_sys[b, :d.m]), (tag, b)
                assert all(v in vsys[p] for v in got_sys[b, d.m:]), (tag, b, got_sys[b])
                used = [got_params[b, 6 + j * K:6 + (j + 1) * K] for j in range(3)]
                for blk, flag in zip(used, (d.has_f2, d.has_b2, d.leader >= 0)):
                    assert blk.all() if flag else not blk.any(), (tag, b)
                assert got_x[b, :d.m].all() and not got_x[b, d.m:].any(), (tag, b)
                assert got_params[b, :2 * d.m].all() and not got_params[b, 2 * d.m:6].any(), (tag, b)


def _select_rows(n):
    """Per-platoon inputs that hit each rule of the winner rule once, for n >= 2 agents:
    (eval cost, eval status, new cost, new status, active, winner).  Agents a < b carry the case, the
    rest a decrease of 5 (below the threshold of 10)."""
    inf, nan = np.inf, np.nan
    a, b = 0, n - 1
    a2 = n - 2  # a second placement, away from agent 0 where n allows

    def row(changes, active=1, want=-1, all_new_status=None):
        ev, nw = 50.0 + np.arange(n), 45.0 + np.arange(n)
        es, ns = np.zeros(n, np.int32), np.zeros(n, np.int32)
        for i, (e, est, w, wst) in changes.items():
            ev[i], es[i], nw[i], ns[i] = e, est, w, wst
        if all_new_status is not None:
            ns[:] = all_new_status
        return ev, es, nw, ns, active, want

    return [
        row({a: (110.0, 0, 100.0, 0)}),                                            # exactly the threshold: no win
        row({a2: (110.0 + 1e-9, 0, 100.0, 0)}, want=a2),                           # strictly more
        row({a: (120.0, 0, 100.0, 0), b: (220.0, 0, 200.0, 0)}, want=a),           # the first of equal decreases
        row({a: (120.0, 0, 100.0, 0), b: (300.0, 0, 100.0, 0)}, want=b),           # the largest, wherever it is
        row({a: (500.0, 0, 100.0, 0), b: (7.0, 1, 3.0, 0)}, want=b),               # eval status != 0 with a finite
                                                                                   # stored cost is inf: inf - finite
        row({a: (7.0, 1, 100.0, 0), b: (9.0, 2, 3.0, 0)}, want=a),                 # the first of two such
        row({a2: (1e9, 0, 1.0, 2)}),                                               # new status != 0, small stored cost
        row({}, all_new_status=2, want=-2),                                        # ... and never counts as feasible
        row({a: (1e300, 1, 1e300, 1), b: (80.0, 0, 60.0, 0)}, want=b),             # both infinite: NaN, skipped
        row({a: (nan, 0, nan, 0)}),                                                # NaN costs
        row({a2: (500.0, 0, nan, 0)}),
        row({i: (50.0, 0, 1e300, 1) for i in range(n)}, want=-2),                  # no feasible solve at all
        row({i: (50.0, 0, inf, 0) for i in range(n)}, want=-2),
        row({a: (120.0, 0, 100.0, 0), b: (300.0, 0, 100.0, 0)}, active=0),         # inactive: left alone
        row({a: (10.0, 0, 500.0, 0)}),                                             # a cost increase
    ]


@pytest.mark.gpu
@pytest.mark.parametrize("winner_given", [True, False])
@pytest.mark.parametrize("gears", [True, False])
@pytest.mark.parametrize("n", [2, 3, 5])
def test_gpu_select_matches_host_rule(gpu_available, n, gears, winner_given):
    """hvp_event_select over P = 70 platoons (two thread blocks), each with one row of _select_rows:
    the winners are hvp.event.select_winner's (-2 where it raises, -1 for an inactive platoon); the
    guess store changes only in vehicles lo .. lo + m - 1 of the winner, which take the winner's local
    slots, every other element bit-identical; active is cleared exactly where nobody won."""
    import torch

    from hvp.event import select_winner, threshold

    N, P = 3, 70
    s = _stage_solver(N)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    rows = _select_rows(n)
    pick = [(7 * p) % len(rows) for p in range(P)]  # every row in the first block, a mix in the second
    assert set(pick[:64]) == set(range(len(rows))) and len(set(pick[64:])) == P - 64
    ev, es, nw, ns = (np.stack([rows[k][j] for k in pick]) for j in range(4))
    active = np.array([rows[k][4] for k in pick], np.int32)
    want = np.empty(P, np.int32)
    for p, k in enumerate(pick):
        if not active[p]:
            want[p] = -1
            continue
        try:
            with np.errstate(invalid="ignore"):
                want[p] = select_winner(np.where(es[p] == 0, ev[p], np.inf), np.where(ns[p] == 0, nw[p], np.inf), threshold)
        except RuntimeWarning:
            want[p] = -2
        assert want[p] == rows[k][5], (k, want[p], rows[k][5])  # the rows do hit the rules they are named for
    rng = np.random.default_rng(n)
    xg, ug, x_sol, u_sol = _distinct(rng, (n, P, 2, N + 1), (n, P, N), (P * n, 3, 2, N + 1), (P * n, 3, N))
    gg = rng.integers(1, 4, (n, P, N)).astype(np.int8)
    gear_sol = rng.integers(4, 7, (P * n, 3, N)).astype(np.int8)
    w_xg, w_ug, w_gg = xg.copy(), ug.copy(), gg.copy()
    for p in range(P):
        i = want[p]
        if i < 0:
            continue
        lo, hi = max(i - 1, 0), min(i + 1, n - 1)
        for j, v in enumerate(range(lo, hi + 1)):
            w_xg[v, p], w_ug[v, p], w_gg[v, p] = x_sol[p * n + i, j], u_sol[p * n + i, j], gear_sol[p * n + i, j]
    d_xg, d_ug, d_gg, d_active = t(xg), t(ug), t(gg) if gears else None, t(active)
    winner = torch.full((P,), SENT32, dtype=torch.int32, device=dev) if winner_given else None
    s.select_device(n, {"cost": t(ev.reshape(-1)), "status": t(es.reshape(-1))},
                    {"cost": t(nw.reshape(-1)), "status": t(ns.reshape(-1)), "x": t(x_sol), "u": t(u_sol),
                     "gear": t(gear_sol)}, d_xg, d_ug, d_gg, d_active, winner, threshold)
    torch.cuda.synchronize()
    if winner_given:
        assert np.array_equal(winner.cpu().numpy(), want), (winner.cpu().numpy(), want)
    assert np.array_equal(d_active.cpu().numpy(), (active != 0) & (want >= 0))
    assert np.array_equal(d_xg.cpu().numpy(), w_xg) and np.array_equal(d_ug.cpu().numpy(), w_ug)
    if gears:
        assert np.array_equal(d_gg.cpu().numpy(), w_gg)
    assert (want >= 0).sum() >= 20 and (want == -2).sum() >= 10 and (active == 0).sum() >= 4
