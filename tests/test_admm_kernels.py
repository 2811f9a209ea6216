"""The ADMM bookkeeping kernels on their own: k_admm_update (hvp_admm_update), k_gadmm_update,
k_gadmm_switch and k_gadmm_rollout, each against a float64 NumPy restatement of the formulas of
include/hvp.h and of oracle.GAdmmCoordinator.rollout / u_const_vel / switch.

The coordinator runs of test_admm.py / test_gadmm.py reach these kernels only on the paths a
healthy closed loop takes.  Here the inputs are random (fixed seed, the workload's magnitudes:
p ~ 3e3, v in [5, 40], multipliers ~ 1e2) and cover what those runs never do: platoons that are not
live, velocities in no band, both edge bits at one step, edges at the state box, a restart over
non-zero multipliers, arbitrary warm starts, NULL outputs, one- and two-vehicle chains and vehicle
shards whose halo slots hold values no local solve produced.

Update kernels: every output is at most three additions, one multiply by 1/3 or 1/2 and one
y + rho (a - z), about ten roundings of 1.1e-16 S with S the largest magnitude among the inputs of
that entry's formula; the bar is |out - ref| <= 1e-12 S.  Entries that must not change are compared
bit for bit.
"""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

RHO = 0.5
LIVE, FAILED, CHANGED = 1, 2, 4
WORST = {}  # kernel -> worst error seen, in units of 1e-12 S (printed by each test)


def _rand_traj(rng, shape, N):
    """(..., 2, N+1) trajectories at the workload's magnitudes, flattened to (..., 2 (N+1))."""
    t = np.stack([3000.0 + rng.uniform(-200, 200, shape + (N + 1,)), rng.uniform(5, 40, shape + (N + 1,))], axis=-2)
    return t.reshape(shape + (2 * (N + 1),))


def _close(name, got, ref, scale):
    err = np.abs(got - ref) / (1e-12 * scale)
    WORST[name] = max(WORST.get(name, 0.0), float(err.max()))
    assert err.max() <= 1.0, (name, float(err.max()), np.unravel_index(int(err.argmax()), err.shape))


def _gear_table(sysd):
    from hvp import tables

    return tables.system_from_dict(sysd, list(sysd["gear"]))


def bounded_gear_pwa(mass: float) -> dict:
    """The 7-region gear model with regions 0 and 6 closed at the state box (vlo[0] = vmin,
    vhi[6] = vmax), so that a velocity can lie in no band."""
    s = O.gear_pwa_system(mass)
    lo, hi = O.region_bands(s)
    vmax, vmin = float(s["E"][2]), -float(s["E"][3])
    s["S"][0], s["T"][0] = [[0, 1], [0, -1]], [hi[0], -vmin]
    s["S"][6], s["T"][6] = [[0, 1], [0, -1]], [vmax, -lo[6]]
    return s


# ------------------------------------------------------------------ hvp_admm_update
def ref_admm_update(P, n, N, rho, x, xf, xb, y_front, y_back, params):
    """include/hvp.h hvp_admm_update: (z, y_front, y_back, params) and, per entry, the largest
    input magnitude of its formula (z_s, yf_s, yb_s; the params blocks share them)."""
    E = 2 * (N + 1)
    X, XF, XB = (a.reshape(P, n, E) for a in (x, xf, xb))
    z, zs = np.zeros((P, n, E)), np.zeros((P, n, E))
    for i in range(n):
        parts = [X[:, i]] + ([XF[:, i + 1]] if i + 1 < n else []) + ([XB[:, i - 1]] if i >= 1 else [])
        z[:, i] = sum(parts[1:], parts[0]) / len(parts)
        zs[:, i] = np.max(np.abs(parts), axis=0)
    yf, yb = y_front.reshape(P, n, E).copy(), y_back.reshape(P, n, E).copy()
    yfs, ybs = np.abs(yf), np.abs(yb)
    prm = params.reshape(P, n, -1).copy()
    for i in range(n):
        if i >= 1:
            yf[:, i] = yf[:, i] + rho * (XF[:, i] - z[:, i - 1])
            yfs[:, i] = np.maximum(np.maximum(yfs[:, i], np.abs(XF[:, i])), zs[:, i - 1])
            prm[:, i, 2:2 + E], prm[:, i, 2 + E:2 + 2 * E] = yf[:, i], z[:, i - 1]
        if i + 1 < n:
            yb[:, i] = yb[:, i] + rho * (XB[:, i] - z[:, i + 1])
            ybs[:, i] = np.maximum(np.maximum(ybs[:, i], np.abs(XB[:, i])), zs[:, i + 1])
            prm[:, i, 2 + 2 * E:2 + 3 * E], prm[:, i, 2 + 3 * E:2 + 4 * E] = yb[:, i], z[:, i + 1]
    return z, zs, yf, yfs, yb, ybs, prm


@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("N", [2, 5, 8])
def test_admm_update(gpu_available, n, N):
    import torch

    from hvp.admm import admm_problem
    from hvp.solver import BatchSolver

    P, E = 3, 2 * (N + 1)
    rng = np.random.default_rng(100 * N + n)
    solver = BatchSolver(admm_problem(N, RHO), [_gear_table(O.gear_pwa_system(800.0))])
    stride = solver.params_stride
    assert stride == 2 + 10 * (N + 1)
    x, xf, xb = (_rand_traj(rng, (P * n,), N) for _ in range(3))
    y_front, y_back = rng.normal(0, 100, (P * n, E)), rng.normal(0, 100, (P * n, E))
    params = rng.normal(0, 1e3, (P * n, stride))  # sentinels everywhere: what is not written must stay
    z, zs, yf, yfs, yb, ybs, prm = ref_admm_update(P, n, N, RHO, x, xf, xb, y_front, y_back, params)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    outs = []
    for with_z in (True, False):
        d = {k: t(v) for k, v in dict(x=x, xf=xf, xb=xb, yf=y_front, yb=y_back, prm=params).items()}
        dz = t(np.full((P * n, E), -7.0)) if with_z else None
        solver.admm_update(P, n, d["x"], d["xf"], d["xb"], d["yf"], d["yb"], d["prm"], dz)
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in d.items()} | ({"z": dz.cpu().numpy()} if with_z else {}))
    a, b = outs
    # z_out = NULL: identical params and multipliers; the inputs are never written
    for k in ("prm", "yf", "yb"):
        assert np.array_equal(a[k], b[k]), k
    for k, v in (("x", x), ("xf", xf), ("xb", xb)):
        assert np.array_equal(a[k], v), k
    if n == 1:  # a lone vehicle has no neighbour: nothing but z = x is written
        assert np.array_equal(a["prm"], params) and np.array_equal(a["yf"], y_front)
        assert np.array_equal(a["yb"], y_back) and np.array_equal(a["z"], x)
        return
    _close("admm_update", a["z"].reshape(P, n, E), z, zs)
    _close("admm_update", a["yf"].reshape(P, n, E)[:, 1:], yf[:, 1:], yfs[:, 1:])
    _close("admm_update", a["yb"].reshape(P, n, E)[:, :-1], yb[:, :-1], ybs[:, :-1])
    got = a["prm"].reshape(P, n, stride)
    before = params.reshape(P, n, stride)
    _close("admm_update", got[:, 1:, 2:2 + E], prm[:, 1:, 2:2 + E], yfs[:, 1:])
    _close("admm_update", got[:, 1:, 2 + E:2 + 2 * E], prm[:, 1:, 2 + E:2 + 2 * E], zs[:, :-1])
    _close("admm_update", got[:, :-1, 2 + 2 * E:2 + 3 * E], prm[:, :-1, 2 + 2 * E:2 + 3 * E], ybs[:, :-1])
    _close("admm_update", got[:, :-1, 2 + 3 * E:2 + 4 * E], prm[:, :-1, 2 + 3 * E:2 + 4 * E], zs[:, 1:])
    # the params copy of a multiplier is the multiplier itself
    assert np.array_equal(got[:, 1:, 2:2 + E], a["yf"].reshape(P, n, E)[:, 1:])
    assert np.array_equal(got[:, :-1, 2 + 2 * E:2 + 3 * E], a["yb"].reshape(P, n, E)[:, :-1])
    # what has no neighbour, x0 and leader_x: bit-unchanged
    assert np.array_equal(a["yf"].reshape(P, n, E)[:, 0], y_front.reshape(P, n, E)[:, 0])
    assert np.array_equal(a["yb"].reshape(P, n, E)[:, -1], y_back.reshape(P, n, E)[:, -1])
    assert np.array_equal(got[:, 0, 2:2 + 2 * E], before[:, 0, 2:2 + 2 * E])
    assert np.array_equal(got[:, -1, 2 + 2 * E:2 + 4 * E], before[:, -1, 2 + 2 * E:2 + 4 * E])
    assert np.array_equal(got[:, :, :2], before[:, :, :2])
    assert np.array_equal(got[:, :, 2 + 4 * E:], before[:, :, 2 + 4 * E:])
    print(f"hvp_admm_update n={n} N={N}: worst error {WORST['admm_update']:.2e} x 1e-12 S")


# ------------------------------------------------------------------ the switching-ADMM engine
def _engine(systems, n, P, N, lo=0, m=None):
    """A GAdmmEngine whose tensors the tests fill directly; lo / m: a vehicle shard, through a
    stub exchange object (no process group)."""
    from hvp.gadmm import GAdmmEngine, gadmm_problem

    ex = None if m is None else SimpleNamespace(lo=lo, m=m)
    return GAdmmEngine(gadmm_problem(N, RHO), [_gear_table(s) for s in systems], n, P, exchange=ex)


def _put(tensor, array):
    import torch

    tensor.copy_(torch.from_numpy(np.ascontiguousarray(array)).reshape(tensor.shape))


def ref_gadmm_update(P, n, lo, m, N, rho, x, xf, xb, params, state, init):
    """include/hvp.h hvp_gadmm_update: the new params and the per-entry input magnitude."""
    E = 2 * (N + 1)
    X, XF, XB = (a.reshape(P, n, E) for a in (x, xf, xb))

    def z(p, j):
        if init:
            return X[p, j].copy(), np.abs(X[p, j])
        parts = [X[p, j]] + ([XB[p, j - 1]] if j >= 1 else []) + ([XF[p, j + 1]] if j + 1 < n else [])
        return sum(parts[1:], parts[0]) / len(parts), np.max(np.abs(parts), axis=0)

    out, S = params.copy(), np.abs(params)

    def put(b, blk, val, scale):
        out[b, 2 + blk * E:2 + (blk + 1) * E] = val
        S[b, 2 + blk * E:2 + (blk + 1) * E] = scale

    def y(b, blk, a, zv, zsc):
        old = params[b, 2 + blk * E:2 + (blk + 1) * E]
        if init:
            put(b, blk, 0.0, 1.0)
        else:
            put(b, blk, old + rho * (a - zv), np.maximum(np.maximum(np.abs(old), np.abs(a)), zsc))

    for p in range(P):
        if not state[p] & LIVE:
            continue
        for i in range(lo, lo + m):
            b = p * m + i - lo
            zi, zis = z(p, i)
            put(b, 6, zi, zis)
            y(b, 5, X[p, i], zi, zis)
            if i >= 1:
                zm, zms = z(p, i - 1)
                put(b, 1, zm, zms)
                y(b, 0, XF[p, i], zm, zms)
            if i + 1 < n:
                zp, zps = z(p, i + 1)
                put(b, 3, zp, zps)
                y(b, 2, XB[p, i], zp, zps)
    return out, S


@pytest.mark.parametrize("n,lo,m", [(2, 0, 2), (3, 0, 3), (4, 0, 4), (4, 1, 2)],
                         ids=["n2", "n3", "n4", "n4-shard-lo1-m2"])
@pytest.mark.parametrize("N", [2, 5, 8])
def test_gadmm_update(gpu_available, n, lo, m, N):
    """Live, dead, live + changed and failed platoons; init = 0 and init = 1 over non-zero
    multipliers; unsharded and as the shard [1, 3) of 4 vehicles, whose neighbours' z come from
    the full-platoon slots, halo slots included (random values no local solve produced)."""
    import torch

    P, E = 4, 2 * (N + 1)
    rng = np.random.default_rng(1000 * N + 10 * n + lo)
    systems = [O.gear_pwa_system(800.0 + 100.0 * i) for i in range(n)]
    eng = _engine(systems, n, P, N, lo, m if m != n else None)
    assert (eng.lo, eng.m, eng.B, eng.stride) == (lo, m, P * m, 2 + 14 * (N + 1))
    state = np.array([LIVE, 0, LIVE | CHANGED, FAILED], dtype=np.int32)
    x, xf, xb = (_rand_traj(rng, (P * n,), N) for _ in range(3))
    params = rng.normal(0, 100, (P * m, eng.stride))  # every y block non-zero, every other block a sentinel
    for init in (0, 1):
        _put(eng.x, x), _put(eng.xf, xf), _put(eng.xb, xb), _put(eng.params, params), _put(eng.state, state)
        eng.update(init=bool(init))
        torch.cuda.synchronize()
        got = eng.params.cpu().numpy()
        ref, S = ref_gadmm_update(P, n, lo, m, N, RHO, x, xf, xb, params, state, init)
        for k, v in (("x", x), ("xf", xf), ("xb", xb)):
            assert np.array_equal(getattr(eng, k).cpu().numpy().reshape(P * n, E), v), k
        assert np.array_equal(eng.state.cpu().numpy(), state)
        g3, p3 = got.reshape(P, m, -1), params.reshape(P, m, -1)
        assert np.array_equal(g3[1], p3[1]) and np.array_equal(g3[3], p3[3])  # dead, failed: untouched
        assert not np.array_equal(g3[0], p3[0]) and not np.array_equal(g3[2], p3[2])
        # x0, leader_x, and the blocks of a side the vehicle does not have: bit-unchanged
        same = ref == params
        assert same[:, :2].all() and same[:, 2 + 4 * E:2 + 5 * E].all()
        assert np.array_equal(got[same], params[same])
        if init:  # z <- the x slot and every y <- 0, exactly
            assert np.array_equal(got, ref)
            for p in (0, 2):
                for j in range(m):
                    assert np.array_equal(g3[p, j, 2 + 6 * E:2 + 7 * E], x.reshape(P, n, E)[p, lo + j])
                    assert not g3[p, j, 2 + 5 * E:2 + 6 * E].any()
        else:
            _close("gadmm_update", got, ref, S)
    print(f"hvp_gadmm_update n={n} lo={lo} m={m} N={N}: worst error {WORST['gadmm_update']:.2e} x 1e-12 S")


# ------------------------------------------------------------------ hvp_gadmm_switch
@pytest.mark.parametrize("N", [5, 16])
def test_gadmm_switch(gpu_available, N):
    """Vehicle i of every platoon carries case i at every step k = 1..N-1: 0 lower bit only, 1 upper
    bit only, 2 both bits (the lower wins), 3 neither, 4 lower bit in region 0, 5 upper bit in region
    6 (no neighbour: no move).  Platoon 0 is live, platoon 1 failed (not live) with every bit set,
    platoon 2 live with only the cases that move nothing.  Half of the lanes also carry every bit
    the horizon does not use (N = 16: bits 30, 31 next to the 30 it uses) -- seq_0 never moves."""
    import torch

    P, n = 3, 6
    rng = np.random.default_rng(7 + N)
    systems = [O.gear_pwa_system((800.0, 1100.0)[i % 2]) for i in range(n)]
    eng = _engine(systems, n, P, N)
    assert eng.edge.dtype == torch.int32  # uint32 in the ABI
    used = np.uint32((1 << (2 * (N - 1))) - 1)
    lower = np.uint32(sum(1 << (2 * (k - 1)) for k in range(1, N)))
    upper = np.uint32(lower << np.uint32(1))
    assert lower | upper == used and (N != 16 or int(used).bit_length() == 30)
    case_bits = [lower, upper, lower | upper, np.uint32(0), lower, upper]
    seq = np.zeros((P, n, N), dtype=np.int8)
    edge = np.zeros((P, n), dtype=np.uint32)
    for p in range(P):
        for i, (rlo, rhi) in enumerate(((1, 6), (0, 5), (1, 5), (0, 6), (0, 0), (6, 6))):
            seq[p, i] = rng.integers(rlo, rhi + 1, N)
            seq[p, i, 0] = rng.integers(0, 7)
            edge[p, i] = case_bits[i] | (~used if (p + i) % 2 == 0 else np.uint32(0))
    edge[1] = np.uint32(0xFFFFFFFF)
    edge[2, :3] &= ~used  # the live platoon whose sequences must not change
    state = np.array([LIVE, FAILED, LIVE | FAILED], dtype=np.int32)
    _put(eng.seq, seq), _put(eng.edge, edge.view(np.int32)), _put(eng.state, state)
    eng.switch()
    torch.cuda.synchronize()
    got = eng.seq.cpu().numpy().reshape(P, n, N)
    st = eng.state.cpu().numpy()
    # the oracle's rule, element for element
    coord = O.GAdmmCoordinator(systems, O.Cfg(), N, rho=RHO)
    want = seq.copy()
    for p in (0, 2):
        for i in range(n):
            want[p, i] = coord.switch(i, seq[p, i].astype(np.int32), int(edge[p, i]))
    assert np.array_equal(got, want)
    # and the cases spelled out (adjacent regions of the 7-region chain share their edges)
    assert np.array_equal(got[:, :, 0], seq[:, :, 0])
    assert np.array_equal(got[0, 0, 1:], seq[0, 0, 1:] - 1)
    assert np.array_equal(got[0, 1, 1:], seq[0, 1, 1:] + 1)
    assert np.array_equal(got[0, 2, 1:], seq[0, 2, 1:] - 1)
    assert np.array_equal(got[0, 3:], seq[0, 3:])
    assert np.array_equal(got[1], seq[1]) and np.array_equal(got[2], seq[2])
    assert st.tolist() == [LIVE | CHANGED, FAILED, LIVE | FAILED]
    assert np.array_equal(eng.edge.cpu().numpy().view(np.uint32).reshape(P, n), edge)


# ------------------------------------------------------------------ hvp_gadmm_rollout
def _rollout_case(N, n, P, rng, lo=0, m=None):
    """Initial states and warm starts of P platoons of n vehicles of the bounded 7-region model:
    platoon 0 random; platoon 1 with vehicles exactly on shared band edges; platoon 2 with one
    vehicle within 1e-4 below vlo[0]; platoon 3 with one vehicle above vhi[6]."""
    m = n if m is None else m
    systems = [bounded_gear_pwa(800.0 + 150.0 * i) for i in range(n)]
    bands = [O.region_bands(s) for s in systems]
    x0 = np.stack([3000.0 + rng.uniform(-200, 200, (P, n)), rng.uniform(15, 30, (P, n))], axis=-1)
    i0, i1 = lo, lo + m - 1  # held vehicles
    x0[1, i0, 1] = bands[i0][0][3]  # = vhi[2]: the lower-index region 2 is the mode
    x0[1, i1, 1] = bands[i1][0][5]
    x0[2, i1, 1] = bands[i1][0][0] - 5e-5
    x0[3, i0, 1] = bands[i0][1][6] + 0.5
    u_prev = rng.uniform(-0.1, 0.25, (P, m, N))  # at most 0.6 m/s per step: every velocity stays in a band
    u_prev[1, :, :2] = 0.3  # off the band edge at once
    return systems, bands, x0, u_prev


@pytest.mark.parametrize("n,lo,m", [(3, 0, 3), (4, 1, 2)], ids=["n3", "n4-shard-lo1-m2"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("N", [2, 5, 8])
def test_gadmm_rollout(gpu_available, N, mode, n, lo, m):
    import torch

    P = 4
    rng = np.random.default_rng(50 * N + 7 * n + mode)
    systems, bands, x0, u_prev = _rollout_case(N, n, P, rng, lo, m)
    eng = _engine(systems, n, P, N, lo, m if m != n else None)
    coord = O.GAdmmCoordinator(systems, O.Cfg(), N, rho=RHO)
    state = np.array([LIVE, LIVE | CHANGED, LIVE, LIVE | CHANGED], dtype=np.int32)
    sent = -12345.0
    held = x0[:, lo:lo + m]
    params = rng.normal(0, 100, (P * m, eng.stride))
    params[:, :2] = held.reshape(P * m, 2)
    # the warm start the kernel must produce: constant-velocity throttle / u_prev shifted by one step
    u_ref = np.zeros((P, m, N))
    for p in range(P):
        for j in range(m):
            if mode == 1:
                u_ref[p, j] = np.concatenate([u_prev[p, j, 1:], u_prev[p, j, -1:]])
            elif p != 3 or j != 0:  # (3, first held): in no band even with the buffer
                u_ref[p, j] = coord.u_const_vel(lo + j, held[p, j, 1])
    results = {}
    for with_u in (True, False):
        _put(eng.x, np.full((P * n, 2, N + 1), sent)), _put(eng.seq, np.full((P * m, N), -1, dtype=np.int8))
        _put(eng.params, params), _put(eng.state, state)
        eng.prev_u = torch.from_numpy(u_prev.reshape(P * m, N)).to(eng.dev) if mode == 1 else None
        eng.u_ws = torch.full((P * m, N), sent, dtype=torch.float64, device=eng.dev) if with_u else None
        eng.rollout(mode)
        torch.cuda.synchronize()
        results[with_u] = (eng.x.cpu().numpy().reshape(P, n, 2, N + 1), eng.seq.cpu().numpy().reshape(P, m, N),
                           eng.state.cpu().numpy(), eng.u_ws.cpu().numpy().reshape(P, m, N) if with_u else None)
        assert np.array_equal(eng.params.cpu().numpy(), params)
    x, seq, st, u_ws = results[True]
    # u_ws = NULL: the same trajectories, sequences and flags
    assert np.array_equal(results[False][0][:2], x[:2]) and np.array_equal(results[False][1][:2], seq[:2])
    assert np.array_equal(results[False][2], st)
    # only the held vehicles' slots are written
    mask = np.ones(n, dtype=bool)
    mask[lo:lo + m] = False
    assert (x[:, mask] == sent).all()
    # platoons 2 and 3 fail (bit 1 set, bit 0 cleared, bit 2 kept), the others are not touched
    assert st.tolist() == [LIVE, LIVE | CHANGED, FAILED, FAILED | CHANGED]
    for p in (0, 1):
        for j in range(m):
            r = coord.rollout(lo + j, held[p, j], u_ref[p, j])
            assert r is not None, (p, j)
            X, sig = r
            # a constant-velocity rollout from a band edge stays on it to rounding, where the next
            # region is anyone's: only its first step is compared
            K = 1 if (mode == 0 and p == 1 and j in (0, m - 1)) else N
            assert np.array_equal(seq[p, j, :K], sig[:K]), (p, j, seq[p, j], sig)
            assert (np.abs(x[p, lo + j][:, :K + 1] - X[:, :K + 1]) <= 1e-9 * np.maximum(1.0, np.abs(X[:, :K + 1]))).all()
            assert np.abs(u_ws[p, j] - u_ref[p, j]).max() <= 1e-12 * max(1.0, np.abs(u_ref[p, j]).max()), (p, j)
            if mode == 1:
                assert np.array_equal(u_ws[p, j], u_ref[p, j])
    # exactly on a shared edge: the lower-index region
    assert seq[1, 0, 0] == 2 and seq[1, m - 1, 0] == 4
    if mode == 0:
        # within 1e-4 below vlo[0]: the throttle is that of region 0 (the buffer rule), then the
        # step's own lookup, which has no buffer, finds no band
        v = held[2, m - 1, 1]
        assert bands[lo + m - 1][0][0] - 1e-4 < v < bands[lo + m - 1][0][0]
        assert coord.rollout(lo + m - 1, held[2, m - 1], u_ref[2, m - 1]) is None
        assert np.abs(u_ws[2, m - 1] - u_ref[2, m - 1]).max() <= 1e-12 * np.abs(u_ref[2, m - 1]).max()
