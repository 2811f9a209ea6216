"""The sequential MLD controller (hvp.seq, fleet_seq_mld.py:296-545; hvp_seq_stage_params of
include/hvp_seq.h; hvp.sweep.run_point(controller="seq")).

The rule under test.  Per step the leader L solves first, then L-1 .. 0, then L+1 .. n-1.  Vehicle i
is handed, per neighbour, either that neighbour's trajectory of THIS step as it is (F, "fresh") or
its trajectory of the PREVIOUS step shifted (S): column 0 dropped, the last column repeated, the
last position then old p_N + ts * old v_N; on the first step of an episode S is the
constant-velocity extrapolation of the neighbour's state instead (C):

    vehicle   front block        back block
    leader    S of L-1 (L != 0)  S of L+1 (L != n-1)
    i < L     S of i-1 (i != 0)  F of i+1
    i > L     F of i-1           S of i+1 (i != n-1)

CPU: the numpy statement of the rule against a table written out here, the coordinator's order of
solves and bookkeeping on stub MPCs, the extension header's exports.  GPU: the stage kernel
against the numpy rule (exact), every local problem of a host episode against the CPU oracle in
isolation, the batched device closed loop against the host episode seed by seed.
"""

from __future__ import annotations

import functools
import glob
import os
import pickle
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the rule, restated for the tests
def order_of(n, L):
    return [L] + [L - 1 - k for k in range(L)] + list(range(L + 1, n))


def const_vel(p, v, N, ts):
    out = np.zeros((2, N + 1))
    out[0, 0], out[1, :] = p, v
    for k in range(N):
        out[0, k + 1] = out[0, k] + ts * v
    return out


def shift(s, ts):
    N = s.shape[1] - 1
    out = np.zeros_like(s)
    out[:, :N] = s[:, 1:]
    out[0, N] = s[0, N] + ts * s[1, N]
    out[1, N] = s[1, N]
    return out


def blocks_of(i, n, L, x0, prev, cur, N, ts):
    """(front, back) of vehicle i: prev / cur (n, 2, N+1) the predictions of the previous step
    (None on the first) and of this one; x0 (n, 2) this step's states.  None: no such neighbour."""
    def S(j):
        return const_vel(x0[j, 0], x0[j, 1], N, ts) if prev is None else shift(prev[j], ts)

    if i == L:
        return (S(i - 1) if i != 0 else None), (S(i + 1) if i != n - 1 else None)
    if i < L:
        return (S(i - 1) if i != 0 else None), cur[i + 1]
    return cur[i - 1], (S(i + 1) if i != n - 1 else None)


# ---------------------------------------------------------------- CPU
# (front, back) per leader index and vehicle for n = 4, written out from the table above:
# F<j> fresh of j, S<j> shifted of j (C<j>, constant velocity, on the first step), None: no block
RULE_N4 = {
    0: {0: (None, "S1"), 1: ("F0", "S2"), 2: ("F1", "S3"), 3: ("F2", None)},
    2: {2: ("S1", "S3"), 1: ("S0", "F2"), 0: (None, "F1"), 3: ("F2", None)},
    3: {3: ("S2", None), 2: ("S1", "F3"), 1: ("S0", "F2"), 0: (None, "F1")},
}


@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("L", [0, 2, 3])
def test_stage_blocks_rule(L, first):
    from hvp.seq import solve_order, stage_blocks

    n, N, ts = 4, 3, 0.5
    # distinct, exactly representable entries: slot j, row r (0 position, 1 velocity), column k
    xpred = np.array([[[1000.0 * (j + 1) + 100 * r + 7 * k for k in range(N + 1)] for r in range(2)]
                      for j in range(n)])
    x = np.array([900.0, 21, 800, 23, 700, 25, 600, 27])
    keep = xpred.copy()

    def want(tag):
        if tag is None:
            return None
        j = int(tag[1])
        s = xpred[j]
        if tag[0] == "F":
            return s
        if first:  # C: p, p + ts v, p + 2 ts v, p + 3 ts v; the velocity held
            p, v = x[2 * j], x[2 * j + 1]
            return np.array([[p, p + ts * v, p + 2 * ts * v, p + 3 * ts * v], [v, v, v, v]])
        # S: columns 1..N, then the last velocity again and the position old p_N + ts old v_N
        return np.array([[s[0, 1], s[0, 2], s[0, 3], s[0, 3] + ts * s[1, 3]], [s[1, 1], s[1, 2], s[1, 3], s[1, 3]]])

    assert solve_order(n, L) == list(RULE_N4[L])
    for i in range(n):
        got = stage_blocks(i, n, L, x, xpred, first, N, ts)
        for g, tag in zip(got, RULE_N4[L][i]):
            if tag is None:
                assert g is None
            else:
                assert g.shape == (2, N + 1) and np.array_equal(g, want(tag)), (L, first, i, tag)
                g[:] = -1  # a new array, never a view of the store
    assert np.array_equal(xpred, keep)


class _StubMpc:
    """A local MPC without the library: logs the setter and solve calls, returns canned results."""

    num_bin_vars = 0

    def __init__(self, i, N, log, gear=False):
        self.i, self.N, self.log, self.gear, self.calls = i, N, log, gear, 0

    def canned_x(self, call):
        return 100.0 * self.i + 10.0 * call + np.arange(2 * (self.N + 1), dtype=float).reshape(2, -1)

    def set_x_front(self, a):
        self.log.append(("front", self.i, np.array(a)))

    def set_x_back(self, a):
        self.log.append(("back", self.i, np.array(a)))

    def set_leader_x(self, a):
        self.log.append(("leader", self.i, np.array(a)))

    def solve_mpc(self, state, raises=True):
        self.calls += 1
        self.log.append(("solve", self.i, np.array(state)))
        u = np.full((1, self.N), 0.1 * (self.i + 1))
        if self.gear:
            u = np.vstack((u, np.full((1, self.N), float(self.i + 2))))
        info = {"x": self.canned_x(self.calls), "u": u, "cost": 1.0 + self.i, "run_time": 0.25 * (self.i + 1),
                "nodes": 10 + 3 * ((self.i + 2) % 4), "bin_vars": 0}
        return u[:, [0]], info


class _StubEnv:
    def __init__(self, x):
        self.x, self.step_counter = x, 0


@pytest.mark.parametrize("L", [0, 2])
def test_coordinator_order_and_bookkeeping(L):
    from hvp.seq import TrackingSequentialMldCoordinator

    n, N, ts = 4, 3, 1.0
    log = []
    mpcs = [_StubMpc(i, N, log) for i in range(n)]
    leader_x = np.stack([3000.0 + 20 * np.arange(12), np.full(12, 20.0)])
    co = TrackingSequentialMldCoordinator(mpcs, ep_len=3, N=N, leader_x=leader_x, ts=ts, leader_index=L,
                                          order_forwards=False)
    x = np.array([900.0, 21, 800, 23, 700, 25, 600, 27]).reshape(-1, 1)
    env = _StubEnv(x)
    co.on_episode_start(env, 0, x)
    assert [(k, i) for k, i, a in log if k == "leader"] == [("leader", L)]
    assert np.array_equal([a for k, i, a in log if k == "leader"][0], leader_x[:, :N + 1])
    preds = [None, None]  # the canned predictions of the previous and of this step
    for step in (1, 2):
        del log[:]
        u, _ = co.get_control(x)
        solves = [i for k, i, a in log if k == "solve"]
        assert solves == order_of(n, L)
        preds = [preds[1], np.stack([m.canned_x(step) for m in mpcs])]
        x0 = x.reshape(n, 2)
        # what every vehicle was handed last before its solve
        seen = {}
        for k, i, a in log:
            if k in ("front", "back"):
                seen[(k, i)] = a
            elif k == "solve":
                front, back = blocks_of(i, n, L, x0, preds[0], preds[1], N, ts)
                for side, want in (("front", front), ("back", back)):
                    if want is None:
                        assert (side, i) not in seen
                    else:
                        assert np.array_equal(seen[(side, i)], want), (step, side, i)
                assert np.array_equal(a.reshape(-1), x0[i])
        assert u.shape == (n, 1) and np.allclose(u[:, 0], [0.1 * (i + 1) for i in range(n)])
        env.step_counter = step
        co.on_timestep_end(env, 0, step)
        assert co.solve_times[step - 1, 0] == pytest.approx(sum(0.25 * (i + 1) for i in range(n)))  # the sum
        assert co.node_counts[step - 1, 0] == max(10 + 3 * ((i + 2) % 4) for i in range(n))  # the max
        assert np.array_equal([a for k, i, a in log if k == "leader"][-1], leader_x[:, step:step + N + 1])
    assert len(co.history) == 2 and np.array_equal(co.history[1]["x_pred"], preds[1])


def test_coordinator_stacks_gear_controls():
    from hvp.seq import TrackingSequentialMldCoordinator

    n, N = 3, 3
    co = TrackingSequentialMldCoordinator([_StubMpc(i, N, [], gear=True) for i in range(n)], ep_len=2, N=N,
                                          leader_x=np.zeros((2, 8)), ts=1.0, leader_index=1)
    u, _ = co.get_control(np.arange(2.0 * n).reshape(-1, 1))
    # the continuous controls of all vehicles first, then the gears (fleet_seq_mld.py:388-395)
    assert u.shape == (2 * n, 1)
    assert np.allclose(u[:, 0], [0.1, 0.2, 0.3, 2.0, 3.0, 4.0])


def _prototypes(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"^\s*(?:int|void|const char\s*\*)\s+(hvp_\w+)\s*\(", src, flags=re.M))


def test_seq_exports():
    import ctypes

    from hvp import _abi

    funcs = _prototypes("hvp_seq.h")
    assert funcs == {"hvp_seq_stage_params"} == set(_abi.EXPORTS_SEQ)
    # the extension leaves the ABI 5 table alone: EXPORTS is still exactly include/hvp.h
    assert set(_abi.EXPORTS) == _prototypes("hvp.h") - {"hvp_params_stride"}
    assert not funcs & set(_abi.EXPORTS) and _abi.ABI_VERSION == 5
    lib = _abi.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True).stdout
    for f in funcs:
        assert re.search(rf"\bT {f}\b", nm), f
        argt, rest = _abi.EXPORTS_SEQ[f]
        assert list(getattr(lib, f).argtypes) == list(argt) and getattr(lib, f).restype is rest
    # the prototype's 13 parameters, and argument errors before any device work
    assert len(_abi.EXPORTS_SEQ["hvp_seq_stage_params"][0]) == 13
    assert lib.hvp_seq_stage_params(None, 1, 4, 0, None, None, None, 0, 0, 0, None, None, None) == -1
    assert "null handle" in _abi.last_error()
    assert ctypes.sizeof(ctypes.c_void_p) == 8


def test_unknown_controller_raises_before_device_work():
    from hvp.sweep import run_point

    with pytest.raises(ValueError, match="controller"):
        run_point(4, 5, [0], ep_len=2, controller="bogus")
    with pytest.raises(ValueError, match="seq path"):
        run_point(4, 5, [0], ep_len=2, leader_index=2)  # the decentralised sweep has no leader choice
    with pytest.raises(ValueError, match="leader_index"):
        run_point(4, 5, [0], ep_len=2, controller="seq", leader_index=4)


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_stage_params_kernel_matches_host(gpu_available):
    """hvp_seq_stage_params against stage_blocks / tables.role_bits for every stage, exactly (ts = 1:
    the products are exact whether or not the compiler contracts them)."""
    import torch

    from hvp import tables
    from hvp.models import PwaGearVehicle
    from hvp.seq import stage_blocks
    from hvp.solver import BatchSolver

    P, n, N = 3, 4, 5
    K = 2 * (N + 1)
    veh = PwaGearVehicle(800)
    solver = BatchSolver(tables.problem(N), [tables.system_from_dict(veh.get_discrete_system(1), tables.gears_of(veh))])
    rng = np.random.default_rng(5)
    x = rng.uniform(5, 3000, (P, 2 * n))
    xpred = rng.uniform(5, 3000, (n, P, 2, N + 1))
    win = rng.uniform(5, 3000, (P, 2, N + 1))
    dev = torch.device("cuda", 0)
    xd, pd, wd = (torch.from_numpy(a).to(dev) for a in (x, xpred, win))
    zero = np.zeros((P, K))
    for L, rvar in ((0, False), (2, False), (3, False), (0, True)):
        for first in (True, False):
            for i in range(n):
                params, roles = solver.seq_stage_params_device(i, xd, pd, wd, leader_index=L,
                                                               real_vehicle_as_reference=rvar, first=first)
                torch.cuda.synchronize()
                params, roles = params.cpu().numpy(), roles.cpu().numpy()
                front, back = stage_blocks(i, n, L, x, xpred, first, N, 1.0)
                want = np.concatenate([x[:, 2 * i:2 * i + 2],
                                       zero if front is None else front.reshape(P, K),
                                       zero if back is None else back.reshape(P, K),
                                       win.reshape(P, K) if i == L else zero], axis=1)
                assert params.shape == (P, 2 + 3 * K) and np.array_equal(params, want), (L, first, i)
                assert roles.tolist() == [tables.role_bits(i == 0, i == n - 1, i == L, rvar)] * P, (L, first, i)
    for bad_i in (-1, n):  # the stage vehicle is checked before the launch
        with pytest.raises(Exception, match="stage vehicle"):
            solver.seq_stage_params_device(bad_i, xd, pd, wd)


N4 = dict(n=4, N=5, T=6)


@functools.lru_cache(maxsize=None)
def _host_episode(seed, L, n=4, N=5, T=6):
    """seq.simulate of the task_2 setting (one run per (seed, leader), shared by the tests)."""
    from hvp import seq
    from hvp.params import Sim_n_task_2

    sim = Sim_n_task_2(n, seed=seed, N=N)
    sim.ep_len = T
    X, U, R, agent, env = seq.simulate(sim, seed=seed, leader_index=L)
    return dict(sim=sim, X=np.asarray(X).reshape(T + 1, -1), U=np.asarray(U).reshape(T, -1),
                R=np.asarray(R).reshape(-1), viol=np.asarray(env.unwrapped.viol_counter[0]), agent=agent)


def _check_local_problems(agent, systems, cfg, n, N, L, leader_x, quadratic=True, ts=1.0):
    """Every local problem of the recorded episode, in solve order, against the oracle MIQP / MILP
    with the neighbour blocks rebuilt from the recorded predictions by blocks_of."""
    import oracle as O

    zero = np.zeros((2, N + 1))
    prev = None
    for t, h in enumerate(agent.history):
        cur = h["x_pred"]
        assert (h["status"] == 0).all()
        for i in order_of(n, L):
            front, back = blocks_of(i, n, L, h["x0"], prev, cur, N, ts)
            ref = O.solve_miqp(systems[i], cfg, N, O.role_bits(i, n, L), h["x0"][i],
                               zero if front is None else front, zero if back is None else back,
                               leader_x[:, t:t + N + 1] if i == L else zero, quadratic=quadratic)
            assert ref.status == 0
            assert abs(h["cost"][i] - ref.cost) <= 1e-9 * max(1.0, abs(ref.cost)), (t, i, h["cost"][i], ref.cost)
            if quadratic:  # LP minimisers are not unique: cost only
                assert h["region"][i].tolist() == ref.sigma.tolist(), (t, i)
                assert np.abs(h["u_pred"][i][0] - ref.u).max() <= 1e-6, (t, i)
        prev = cur


@pytest.mark.gpu
@pytest.mark.parametrize("L", [0, 3])
def test_seq_local_problems_match_oracle(gpu_available, L):
    import oracle as O
    from hvp import decent

    n, N, T = N4["n"], N4["N"], N4["T"]
    ep = _host_episode(0, L)
    sim = ep["sim"]
    assert len(ep["agent"].history) == T
    systems = [O.gear_pwa_system(m) for m in sim.masses]
    cfg = O.Cfg(d0=sim.spacing_policy.d0, t0=sim.spacing_policy.t0)
    _check_local_problems(ep["agent"], systems, cfg, n, N, L, sim.leader_trajectory.get_leader_trajectory())
    # not the decentralised rule: the same seed gives another episode
    _, Ud, _, _, _ = decent.simulate(sim, seed=0, leader_index=L)
    assert np.abs(np.asarray(Ud).reshape(T, -1) - ep["U"]).max() > 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("L", [None, 2])
def test_seq_point_matches_host_simulate(gpu_available, tmp_path, L):
    from hvp.sweep import run_point

    n, N, T, seeds = N4["n"], N4["N"], N4["T"], [0, 1, 2]
    res = run_point(n, N, seeds, ep_len=T, out_dir=str(tmp_path), controller="seq", leader_index=L,
                    return_pred=True)
    assert res["status_counts"] == {"OPTIMAL": T * n * len(seeds)}
    assert res["XPRED"].shape == (T, n, len(seeds), 2, N + 1)
    for k, s in enumerate(seeds):
        ep = _host_episode(s, L or 0)
        np.testing.assert_allclose(res["X"][:, k], ep["X"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(res["U"][:, k], ep["U"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(res["R"][:, k], ep["R"], rtol=1e-9)
        assert np.array_equal(res["viol"][:, k], ep["viol"])
    files = sorted(glob.glob(os.path.join(tmp_path, "*.pkl")))
    assert len(files) == len(seeds) == len(glob.glob(os.path.join(tmp_path, "seq_*_seed_*.pkl")))
    assert os.path.basename(files[0]) == f"seq_task_2_n_{n}_N_{N}" + ("" if L is None else f"_lead_{L}") + "_seed_0.pkl"
    with open(files[0], "rb") as f:  # results_analysis/perf_n.py:78-91
        X, U, R, solve_times, node_counts, violations, leader_state = (pickle.load(f) for _ in range(7))
        with pytest.raises(EOFError):
            pickle.load(f)
    assert X.shape == (T + 1, 2 * n) and U.shape == (T, n)
    assert np.isfinite(sum(R)[0, 0]) and min(solve_times)[0] > 0 and max(node_counts)[0] >= 1
    assert len(violations) == T and np.asarray(leader_state).shape[0] == 2


@pytest.mark.gpu
def test_seq_point_long_horizon(gpu_available):
    """N > 8, the branch-and-bound path: the device loop against the host episode, and the region
    hint (every vehicle's shifted previous sequence, one slice per stage) changes no episode."""
    from hvp.sweep import run_point

    n, N, T, seeds = 3, 10, 3, [0, 1]
    a = run_point(n, N, seeds, ep_len=T, controller="seq", warm_incumbent=True)
    b = run_point(n, N, seeds, ep_len=T, controller="seq", warm_incumbent=False)
    for k in ("X", "U", "R", "viol"):
        assert np.array_equal(a[k], b[k]), k
    assert a["status_counts"] == b["status_counts"] == {"OPTIMAL": T * n * len(seeds)}
    for k, s in enumerate(seeds):
        ep = _host_episode(s, 0, n, N, T)
        np.testing.assert_allclose(a["X"][:, k], ep["X"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(a["U"][:, k], ep["U"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(a["R"][:, k], ep["R"], rtol=1e-9)
        assert np.array_equal(a["viol"][:, k], ep["viol"])


@pytest.mark.gpu
def test_seq_gear_and_l1(gpu_available):
    import oracle as O
    from hvp import seq
    from hvp.params import Sim

    class ShortGear(Sim):
        n = 3
        N = 5
        ep_len = 3
        vehicle_model_type = "pwa_friction"

    n, N, T = 3, 5, 3
    X, U, R, agent, env = seq.simulate(ShortGear(), seed=3, leader_index=1)
    assert np.asarray(env.actions[0]).shape == (T, 2 * n, 1) and U.shape == (T, 2 * n)
    assert np.all(np.abs(U[:, :n]) <= 1 + 1e-9) and set(np.unique(U[:, n:]).astype(int)) <= set(range(1, 7))
    for t, h in enumerate(agent.history):  # the continuous controls first, then the gears
        assert np.array_equal(U[t, :n], [h["u_pred"][i][0, 0] for i in range(n)])
        assert np.array_equal(U[t, n:], [h["u_pred"][i][1, 0] for i in range(n)])
    with pytest.raises(NotImplementedError):
        class Nonlinear(ShortGear):
            vehicle_model_type = "nonlinear"

        seq.simulate(Nonlinear(), seed=3)

    class ShortL1(Sim):
        n = 3
        N = 5
        ep_len = 3
        quadratic_cost = False

    sim = ShortL1()
    X, U, R, agent, env = seq.simulate(sim, seed=2)
    assert len(agent.history) == T and not agent.agents[0].mpc.quadratic_cost
    _check_local_problems(agent, [O.gear_pwa_system(800.0)] * n, O.Cfg(), n, N, 0,
                          sim.leader_trajectory.get_leader_trajectory(), quadratic=False)
