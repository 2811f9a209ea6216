"""The event-based controller (hvp.event, fleet_event_based.py; include/hvp_event.h;
hvp.sweep.run_point(controller="event")).

CPU: the coordinator's rules in numpy (winner, shift, episode-start guesses, the per-agent
layout) against literal restatements of the reference, the results file, the extension's
prototypes and the argument errors that return before any device work.

GPU: the oracle has no event-based problem, so every term family of the local MIQP is pinned by an
exact reduction to one it solves -- no boundary = the centralised MIQP, the front boundary = the
centralised MIQP with real_vehicle_as_reference, both boundaries at m = 1 = the decentralised
follower -- and the combination by a term-by-term numpy restatement of the LocalMpc objective,
the exhaustive search, the evaluation kernel and feasible perturbations.  Parity bar (DESIGN
section 7): regions and gears exact, cost 1e-9 relative, u 1e-6, x 1e-4.
"""

from __future__ import annotations

import ctypes
import os
import pickle
import re
import subprocess
import warnings

import numpy as np
import pytest

import oracle as O
from golden_io import CfgParams
from instances import leader_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {"space": O.Cfg(), "time": O.Cfg(d0=10.0, t0=3.0)}  # ConstantSpacingPolicy(50), ConstantTimePolicy(10, 3)


# ====================================================================== CPU: the rules
def test_select_winner_rule():
    from hvp.event import select_winner

    inf = np.inf
    # strictly more than the threshold: a decrease of exactly 10 does not win
    assert select_winner([110.0, 50.0], [100.0, 45.0]) == -1
    assert select_winner([110.0 + 1e-9, 50.0], [100.0, 45.0]) == 0
    # the first of equal decreases
    assert select_winner([5.0, 120.0, 220.0, 1.0], [0.0, 100.0, 200.0, 0.5]) == 1
    # the largest decrease, wherever it is
    assert select_winner([120.0, 300.0, 130.0], [100.0, 100.0, 100.0]) == 1
    # inf - finite wins (and the first such)
    assert select_winner([500.0, inf, inf], [100.0, 3.0, 4.0]) == 1
    # new = inf never wins, with a finite or an infinite evaluation
    assert select_winner([1e9, inf, 50.0], [inf, inf, 45.0]) == -1
    assert select_winner([1e9, 80.0], [inf, 60.0]) == 1
    # nobody above the threshold: no winner (the coordinator stops iterating)
    assert select_winner([10.0, 20.0], [9.0, 19.0]) == -1
    # a cost increase never wins
    assert select_winner([10.0], [500.0]) == -1
    # no feasible solve at all
    with pytest.raises(RuntimeWarning):
        select_winner([1.0, inf], [inf, inf])
    # the threshold is the reference's
    import hvp.event as E

    assert E.threshold == 10


def test_shift_and_episode_start_guesses():
    from hvp.event import initial_guesses, shift_guesses
    from hvp.models import Platoon

    rng = np.random.default_rng(0)
    N = 4
    x = rng.normal(size=(2, N + 1))
    u = rng.normal(size=(1, N))
    # fleet_event_based.py:589-603, literally
    assert np.array_equal(shift_guesses(x), np.concatenate((x[:, 1:], x[:, -1:]), axis=1))
    assert np.array_equal(shift_guesses(u), np.concatenate((u[:, 1:], u[:, -1:]), axis=1))
    for model, gears in (("pwa_gear", False), ("pwa_friction", True)):
        pl = Platoon(3, vehicle_type=model, masses=[700.0, 850.0, 990.0])
        veh = pl.get_vehicles()
        state = np.array([3000.0, 21.0, 2900.0, 9.5, 2800.0, 33.0])
        xs, us, gs = initial_guesses(state, veh, N, 1.0, gears)
        for i in range(3):  # :620-646, literally
            want = np.zeros((2, N + 1))
            want[:, 0] = state[2 * i:2 * i + 2]
            for k in range(N):
                want[0, k + 1] = want[0, k] + 1.0 * want[1, k]
                want[1, k + 1] = want[1, k]
            assert np.array_equal(xs[i], want)
            v = state[2 * i + 1]
            if gears:
                j = veh[i].get_gear_from_velocity(v)
                assert np.array_equal(gs[i], j * np.ones(N))
                assert np.array_equal(us[i], veh[i].get_u_for_constant_vel(v, j) * np.ones(N))
            else:
                assert np.array_equal(us[i], veh[i].get_u_for_constant_vel(v) * np.ones(N))
                assert not gs[i].any()


def _reference_layout(n, leader_index):
    """fleet_event_based.py:700-723, literally: (systems slice, front, behind, rel)."""
    out = []
    for i in range(n):
        veh = [0, 1] if i == 0 else ([n - 2, n - 1] if i == n - 1 else [i - 1, i, i + 1])
        front = i if i < 2 else 2
        behind = (n - 1) - i if i > n - 3 else 2
        rel = -1 if i == leader_index - 1 else (0 if i == leader_index else (1 if i == leader_index + 1 else None))
        out.append((veh, front, behind, rel))
    return out


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6])
def test_local_layout_table(n):
    from hvp import _abi
    from hvp.event import local_layout, platoon_desc

    for lead in range(n):
        lay = local_layout(n, lead)
        desc = platoon_desc(n, lead, 2)  # hvp_event_layout, tiled for two platoons
        for i, (veh, front, behind, rel) in enumerate(_reference_layout(n, lead)):
            L = lay[i]
            assert list(range(L["lo"], L["lo"] + L["m"])) == veh
            assert (L["num_vehicles_in_front"], L["num_vehicles_behind"], L["rel_leader_index"]) == (front, behind, rel)
            # the local vehicle that tracks the leader: x_f1 / x_me / x_b1 for rel 1 / 0 / -1 (:146-165)
            me = veh.index(i)
            assert L["leader"] == (-1 if rel is None else me - rel)
            if rel is not None:
                assert veh[L["leader"]] == lead
            for p in range(2):
                d = desc[p * n + i]
                assert (d.m, d.has_f2, d.has_b2, d.leader) == (len(veh), int(front == 2), int(behind == 2), L["leader"])
    with pytest.raises(ValueError):
        local_layout(1)
    with pytest.raises(ValueError):
        local_layout(3, 3)
    assert _abi.load().hvp_event_layout(1, 0, (_abi.HvpEventDesc * 1)()) == -1


def test_results_file_round_trip(tmp_path):
    from hvp.event import write_results

    T, n = 4, 3
    rng = np.random.default_rng(1)
    objs = (rng.normal(size=(T + 1, 2 * n)), rng.normal(size=(T, n)), rng.normal(size=(T, 1, 1)),
            rng.random((T, 1)), rng.integers(1, 50, (T, 1)).astype(float), rng.integers(0, 2, T).astype(float),
            rng.normal(size=(2, T + 50)))
    path = tmp_path / "event_3_task_2_n_3_N_3_seed_0.pkl"
    write_results(str(path), *objs)
    with open(path, "rb") as f:  # the reader's order: X, U, R, solve_times, node_counts, violations, leader_x
        back = [pickle.load(f) for _ in range(7)]
        with pytest.raises(EOFError):
            pickle.load(f)
    for a, b in zip(objs, back):
        assert np.array_equal(a, b)


def _prototypes(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"^\s*(?:int|void|const char\s*\*)\s+(hvp_\w+)\s*\(", src, flags=re.M))


def test_event_exports():
    from hvp import _abi

    funcs = _prototypes("hvp_event.h")
    assert funcs == set(_abi.EXPORTS_EVENT)
    assert not funcs & (set(_abi.EXPORTS) | set(_abi.EXPORTS_SEQ)) and _abi.ABI_VERSION == 5
    lib = _abi.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True).stdout
    for f in funcs:
        assert re.search(rf"\bT {f}\b", nm), f
        argt, rest = _abi.EXPORTS_EVENT[f]
        assert list(getattr(lib, f).argtypes) == list(argt) and getattr(lib, f).restype is rest
    assert ctypes.sizeof(_abi.HvpEventDesc) == 16
    for N in (2, 5, 16):
        assert lib.hvp_event_params_stride(N) == _abi.event_params_stride(N) == 6 + 6 * (N + 1)


def test_argument_errors_before_any_device_work():
    """HVP_E_ARG (-1): m outside 1..3, a leader index >= m, m N > 64, a NULL required pointer, a
    problem that is not HVP_FORM_CENT; HVP_E_UNSUPPORTED (-3): a min_1_norm problem.  All on the
    host (this test runs without a GPU)."""
    from hvp import _abi, tables
    from hvp.cent import cent_problem
    from hvp.event import make_desc

    lib = _abi.load()
    ok = cent_problem(3)
    val = lambda prob, items: lib.hvp_event_validate(ctypes.byref(prob), len(items), make_desc(items))  # noqa: E731
    assert val(ok, [(1, 1, 1, -1), (2, 0, 1, 1), (3, 1, 1, 2), (3, 0, 0, -1)]) == 0
    for bad in ((0, 0, 0, -1), (4, 0, 0, 0), (-1, 0, 0, -1)):
        assert val(ok, [(2, 0, 0, 0), bad]) == -1 and "outside 1..3" in _abi.last_error()
    for bad in ((1, 1, 1, 1), (2, 0, 0, 2), (3, 0, 0, 3), (3, 0, 0, -2)):
        assert val(ok, [bad]) == -1 and "leader index" in _abi.last_error()
    assert val(cent_problem(22), [(2, 0, 0, 0)]) == 0
    assert val(cent_problem(22), [(2, 0, 0, 0), (3, 0, 0, 0)]) == -1 and "m N > 64" in _abi.last_error()
    assert lib.hvp_event_validate(ctypes.byref(ok), 2, None) == -1 and "null" in _abi.last_error()
    assert lib.hvp_event_validate(None, 0, None) == -1
    assert lib.hvp_event_validate(ctypes.byref(ok), -1, make_desc([(1, 0, 0, 0)])) == -1
    assert val(tables.problem(3), [(2, 0, 0, 0)]) == -1 and "HVP_FORM_CENT" in _abi.last_error()
    assert val(cent_problem(3, quadratic_cost=False), [(2, 0, 0, 0)]) == -3 and "quadratic" in _abi.last_error()
    # every handle-taking entry point refuses a null handle
    d = make_desc([(2, 0, 0, 0)])
    Z = None
    assert lib.hvp_event_solve_batch(Z, 1, d, Z, Z, 0, Z, Z, Z, Z, Z, Z, Z, Z, Z) == -1
    assert lib.hvp_event_evaluate_batch(Z, 1, d, Z, Z, Z, Z, Z, Z, Z, Z) == -1
    assert lib.hvp_event_gather(Z, 1, 3, 0, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z) == -1
    assert lib.hvp_event_select(Z, 1, 3, 10.0, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z) == -1
    assert lib.hvp_event_shift(Z, 1, 3, 0, Z, Z, Z, Z, Z, Z) == -1
    assert "null handle" in _abi.last_error()


def test_local_mpc_raises_like_the_reference():
    from hvp.event import LocalMpc
    from hvp.models import Platoon
    from hvp.sweep import run_point

    systems = Platoon(3, vehicle_type="pwa_gear").get_vehicle_system_dicts(1)
    with pytest.raises(ValueError, match="rel leader index must be -1, 0, or 1"):
        LocalMpc(3, systems, 1, 1, rel_leader_index=2)
    with pytest.raises(NotImplementedError):
        LocalMpc(3, systems, 1, 1, quadratic_cost=False)
    with pytest.raises(ValueError):
        LocalMpc(3, systems[:2], 1, 1)  # three local vehicles need three systems
    with pytest.raises(ValueError):
        LocalMpc(3, systems[:2], 0, 2, rel_leader_index=1)  # no vehicle in front to track the leader
    m = LocalMpc(3, systems, 2, 1, rel_leader_index=-1)
    assert m.desc == (3, True, False, 2) and m.me == 1
    assert LocalMpc(3, systems[:2], 0, 2, rel_leader_index=0).desc == (2, False, True, 0)
    assert LocalMpc(3, systems[:2], 2, 0, rel_leader_index=1).desc == (2, True, False, 0)
    with pytest.raises(ValueError, match="event_iters"):
        run_point(4, 3, [0], ep_len=2, controller="event", event_iters=0)


# ====================================================================== GPU
def _solver(cfg: O.Cfg, N: int, masses, model: int = 0, exhaustive: bool = False):
    """EventSolver with one table per entry of `masses` (the product's own table builders) and the
    oracle's system dicts of the same vehicles."""
    from hvp import tables
    from hvp.cent import cent_problem
    from hvp.event import EventSolver
    from hvp.models import PwaFrictionVehicle, PwaGearVehicle
    from hvp.params import ConstantTimePolicy

    cp = CfgParams(cfg.vector())
    prob = cent_problem(N, ConstantTimePolicy(cp.d0, cp.t0), accel_cnstr_tightening=cp.tight, params=cp,
                        exhaustive=exhaustive)
    tabs, osys = [], []
    for m in masses:
        if model == 1:
            tabs.append(tables.gear_system_from_dict(PwaFrictionVehicle(float(m)).get_discrete_system(float(cp.ts))))
            osys.append(O.gear_friction_mld_system(float(m)))
        else:
            veh = PwaGearVehicle(float(m))
            tabs.append(tables.system_from_dict(veh.get_discrete_system(float(cp.ts)), tables.gears_of(veh)))
            osys.append(O.gear_pwa_system(float(m)))
    s = EventSolver(prob, tabs)
    s.tables = tabs
    return s, osys


def _sys(idx):
    out = np.zeros(3, dtype=np.int32)
    out[:len(idx)] = idx
    return out


def _same(res, b, m, ref_sigma, ref_cost, ref_u, ref_x, tag):
    assert res.status[b] == 0, (tag, res.status[b])
    assert np.array_equal(res.region[b, :m], np.reshape(ref_sigma, (m, -1))), (tag, res.region[b, :m], ref_sigma,
                                                                                 res.cost[b], ref_cost)
    assert abs(res.cost[b] - ref_cost) <= 1e-9 * abs(ref_cost), (tag, res.cost[b], ref_cost)
    assert np.abs(res.u[b, :m] - np.reshape(ref_u, (m, -1))).max() <= 1e-6, tag
    assert np.abs(res.x[b, :m] - np.reshape(ref_x, (m, 2, -1))).max() <= 1e-4, tag
    assert not res.u[b, m:].any() and not res.x[b, m:].any() and (res.region[b, m:] == -1).all(), tag


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_gpu_no_boundary_equals_centralised(gpu_available, cfg):
    """Without boundary blocks the local problem is MpcMldCent's: a platoon of 3 seen by agent 1
    with the leader on vehicle 0, 1, 2 (rel 1, 0, -1) and a platoon of 2 seen by agents 0 and 1."""
    from hvp.event import local_layout, pack_params

    c, N = CFGS[cfg], 3
    masses = [800.0, 720.0, 950.0]
    s, osys = _solver(c, N, masses)
    items, sysv, params, refs = [], [], [], []
    for seed in (0, 1, 2):
        for n, agent, lead in ((3, 1, 0), (3, 1, 1), (3, 1, 2), (2, 0, 0), (2, 1, 0), (2, 0, 1), (2, 1, 1)):
            L = local_layout(n, lead)[agent]
            assert (L["lo"], L["m"]) == (0, n) and L["leader"] == lead
            x0 = O.env_initial_state(n, seed).astype(float)
            lw = leader_window(N, p0=x0[2 * lead] + 30.0, v=20.0)
            items.append((n, 0, 0, L["leader"]))
            sysv.append(_sys(range(n)))
            params.append(pack_params(N, x0, leader_x=lw))
            refs.append((n, O.solve_cent(osys[:n], c, N, x0, lw, lead)))
    res = s.solve(items, np.stack(sysv), np.stack(params))
    for b, (n, r) in enumerate(refs):
        assert r.status == 0
        _same(res, b, n, r.sigma, r.cost, r.u, r.x, (cfg, b))
        assert res.nodes[b] == r.n_qps, (cfg, b, res.nodes[b], r.n_qps)  # the oracle's exploration order


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_gpu_front_boundary_equals_real_vehicle_reference(gpu_available, cfg):
    """The agent n-1 problem with no adjacent leader (m = 2, front boundary) is the centralised
    MIQP of 2 vehicles with real_vehicle_as_reference and leader_x = x_f2 -- including an x_f2 so
    close that the boundary's safe row is active."""
    from hvp.event import pack_params

    c, N = CFGS[cfg], 3
    s, osys = _solver(c, N, [800.0, 910.0])
    items, sysv, params, refs = [], [], [], []
    for seed in (0, 3):
        x0 = O.env_initial_state(2, seed).astype(float)
        for gap, v in ((80.0, 20.0), (45.0, 12.0), (10.0, 5.0), (26.0, float(x0[1]) - 4.0)):
            xf2 = O.constant_velocity_prediction(x0[0] + gap, v, N)
            items.append((2, 1, 0, -1))
            sysv.append(_sys([0, 1]))
            params.append(pack_params(N, x0, x_f2=xf2))
            refs.append((gap, O.solve_cent(osys, c, N, x0, xf2, 0, True)))
    res = s.solve(items, np.stack(sysv), np.stack(params))
    active = 0
    for b, (gap, r) in enumerate(refs):
        assert r.status == 0
        _same(res, b, 2, r.sigma, r.cost, r.u, r.x, (cfg, b))
        xf2 = params[b][6:6 + 2 * (N + 1)].reshape(2, N + 1)
        active += bool((res.x[b, 0, 0, 2:] > xf2[0, 2:] - c.d_safe - 1e-6).any())
    assert active >= 2  # the soft safe row binds or is violated in some instances


@pytest.mark.gpu
def test_gpu_both_boundaries_m1_equals_decentralised_follower(gpu_available):
    """m = 1 with both boundaries is the decentralised follower's MIQP (x_front = x_f2,
    x_back = x_b2): 16 middle followers of n = 5 platoon states."""
    from hvp.event import pack_params

    N = 3
    role = O.ROLE_SAFE_FRONT | O.ROLE_SAFE_BACK | O.ROLE_TRACK_FRONT | O.ROLE_TRACK_BACK
    for cfg in sorted(CFGS):
        c = CFGS[cfg]
        s, osys = _solver(c, N, [800.0])
        items, params, refs = [], [], []
        zero = np.zeros((2, N + 1))
        for seed in range(6):
            x = O.env_initial_state(5, seed).astype(float)
            for i in (1, 2, 3):
                if len(items) == 16:
                    break
                # neighbours that close in on the follower in some instances (the back row binds)
                dv = (-3.0, 0.0, 4.0)[(seed + i) % 3]
                xf = O.constant_velocity_prediction(x[2 * i - 2], x[2 * i - 1] + dv, N)
                xb = O.constant_velocity_prediction(x[2 * i] - 30.0 + 10.0 * ((seed + i) % 3), x[2 * i + 3] - dv, N)
                items.append((1, 1, 1, -1))
                params.append(pack_params(N, x[2 * i:2 * i + 2], x_f2=xf, x_b2=xb))
                refs.append(O.solve_miqp(osys[0], c, N, role, x[2 * i:2 * i + 2], xf, xb, zero))
        assert len(items) == 16
        res = s.solve(items, np.zeros((16, 3), np.int32), np.stack(params))
        back_active = 0
        for b, r in enumerate(refs):
            assert r.status == 0
            _same(res, b, 1, r.sigma, r.cost, r.u, r.x, (cfg, b))
            xb = params[b][6 + 2 * (N + 1):6 + 4 * (N + 1)].reshape(2, N + 1)
            back_active += bool((xb[0, 2:] > res.x[b, 0, 0, 2:] - c.d_safe - 1e-6).any())
        assert back_active >= 1, cfg


def _objective(c: O.Cfg, desc, x, u, xf2, xb2, xl):
    """The LocalMpc objective (fleet_event_based.py:143-236) of x (m, 2, N+1), u (m, N) with every
    slack at its optimum max(0, .), term by term."""
    m, f2, b2, lead = desc
    Q = np.array(c.Qx, dtype=float).reshape(2, 2)
    q = lambda e: float(e @ Q @ e)  # noqa: E731
    sp = lambda xx: np.array([-c.t0 * xx[1] - c.d0, 0.0])  # noqa: E731  spacing(x): x_i - x_{i-1} - spacing(x_i)
    J = 0.0
    N = u.shape[1]
    for k in range(N + 1):
        X = [x[i, :, k] for i in range(m)]
        if lead >= 0:
            J += q(X[lead] - xl[:, k])
        for i in range(1, m):
            J += q(X[i] - X[i - 1] - sp(X[i]))
            J += c.w * max(0.0, X[i][0] - X[i - 1][0] + c.d_safe)
        if f2:
            J += q(X[0] - xf2[:, k] - sp(X[0]))
            J += c.w * max(0.0, X[0][0] - xf2[0, k] + c.d_safe)
        if b2:
            J += q(xb2[:, k] - X[m - 1] - sp(xb2[:, k]))
            J += c.w * max(0.0, xb2[0, k] - X[m - 1][0] + c.d_safe)
    J += c.Qu * float((u ** 2).sum()) + c.Qdu * float((np.diff(u, axis=1) ** 2).sum())
    return J


def _blocks(p, N):
    K = 2 * (N + 1)
    return [p[6 + j * K:6 + (j + 1) * K].reshape(2, N + 1) for j in range(3)]


def _rows_hold(c, tab, x, u, region, N):
    """The hard rows of one vehicle's trajectory: PWA dynamics of the returned regions, the region
    bands, the state / input boxes and the acceleration rows."""
    for k in range(N):
        r = int(region[k])
        v, vn = x[1, k], x[1, k + 1]
        assert tab.vlo[r] - 1e-7 <= v <= tab.vhi[r] + 1e-7
        assert abs(vn - (tab.a[r] * v + tab.b[r] * u[k] + tab.c[r])) <= 1e-8
        assert abs(x[0, k + 1] - (x[0, k] + tab.ts * v)) <= 1e-8
        assert tab.umin - 1e-7 <= u[k] <= tab.umax + 1e-7
        assert c.a_dec * c.ts - k * c.tight - 1e-7 <= vn - v <= c.a_acc * c.ts - k * c.tight + 1e-7
        assert tab.vmin - 1e-7 <= vn <= tab.vmax + 1e-7 and tab.pmin - 1e-6 <= x[0, k + 1] <= tab.pmax + 1e-6


EX_CAP = 5000  # QPs per instance of the exhaustive search of the whole agents at pwa_friction N = 5


def _episode_batches(model: str, N: int, seeds, n: int = 5, event_iters: int = 1):
    """The five agents' problems one step into an episode of the host coordinator, per seed:
    (coordinator, params, x_guess, u_guess, gear_guess)."""
    from hvp.event import simulate
    from hvp.params import Sim_n_task_2

    out = []
    for seed in seeds:
        sim = Sim_n_task_2(n, seed=seed, N=N)
        sim.vehicle_model_type = model
        sim.ep_len = 1
        _, _, _, agent, env = simulate(sim, event_iters, seed=seed)
        x = np.asarray(env.unwrapped.x, dtype=np.float64).reshape(n, 2)
        out.append((agent,) + agent._batch(x))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("model,N", [("pwa_gear", 3), ("pwa_gear", 5), ("pwa_friction", 3), ("pwa_friction", 5)])
def test_gpu_combined_terms(gpu_available, model, N, seed):
    """All five agents of an n = 5 platoon -- every (m, front, behind) configuration -- with the
    guesses one step into an episode, 8 seeds (one per case): the reported cost is the numpy
    restatement of the objective on the returned (x, u); every row holds; the exhaustive search
    returns the same regions and cost (the bounds with the boundary terms prune nothing optimal);
    evaluating the returned (x, u, gear) returns that cost; feasible perturbations of u never
    evaluate lower.

    The exhaustive search visits every reachable joint sequence and runs to its end on every
    instance of pwa_gear N = 3 and 5 and of pwa_friction N = 3.  On pwa_friction at N = 5 several
    gears are reachable per step and a 3-vehicle agent has them to the power 15 (the search ran
    into the 2M-QP default cap): there every agent gets EX_CAP QPs (one that does not finish reports
    HVP_MAXITER, never an answer, and is compared where it does finish), and the comparison is
    required in full on the sub-problems of the same platoon, guesses and boundary data that can
    finish: the three m = 1 problems with both boundaries (about 1e3 joint sequences each; an
    m = 2 problem has 1e5 to over 2e6 and took 15-140 s, two of sixteen not finishing at all)."""
    from hvp import _abi
    from hvp.event import EventSolver

    rng = np.random.default_rng(7)
    c = CFGS["time"]  # Sim_n_task_2's ConstantTimePolicy(10, 3) with the default weights
    gears = model == "pwa_friction"
    tried = accepted = compared = 0
    capped = (model, N) == ("pwa_friction", 5)
    for agent, params, xg, ug, gg in _episode_batches(model, N, [seed]):
        s = agent._solver
        desc, sysv = agent._desc, agent._sys
        assert {(d[0], d[1], d[2]) for d in desc} == {(2, False, True), (3, False, True), (3, True, True),
                                                      (3, True, False), (2, True, False)}
        res = s.solve(desc, sysv, params)
        ex_prob = _abi.HvpProblem.from_buffer_copy(bytes(s.problem))
        ex_prob.method = _abi.METHOD_ENUMERATE
        tabs = [m.tables[m.me] for m in (a.mpc for a in agent.agents)]
        exs = EventSolver(ex_prob, tabs)
        ex = exs.solve(desc, sysv, params, EX_CAP if capped else 0)
        ev, ev_status = s.evaluate(desc, sysv, params, res.x, res.u, res.gear if gears else None)
        for b, d in enumerate(desc):
            m = d[0]
            assert res.status[b] == 0 and ex.status[b] in ((0, 2) if capped else (0,)), (b, res.status[b], ex.status[b])
            xf2, xb2, xl = _blocks(params[b], N)
            J = _objective(c, d, res.x[b, :m], res.u[b, :m], xf2, xb2, xl)
            assert abs(res.cost[b] - J) <= 1e-9 * abs(J), (b, res.cost[b], J)
            for j in range(m):
                _rows_hold(c, tabs[sysv[b, j]], res.x[b, j], res.u[b, j], res.region[b, j], N)
                assert np.allclose(res.x[b, j, :, 0], params[b][2 * j:2 * j + 2])
            if ex.status[b] == 0:
                compared += 1
                assert np.array_equal(ex.region[b], res.region[b]), (b, ex.region[b], res.region[b], ex.cost[b], res.cost[b])
                assert abs(ex.cost[b] - res.cost[b]) <= 1e-9 * abs(res.cost[b]), (b, ex.cost[b], res.cost[b])
            else:
                assert ex.nodes[b] >= EX_CAP, (b, ex.nodes[b])
            assert ev_status[b] == 0 and abs(ev[b] - res.cost[b]) <= 1e-9 * abs(res.cost[b]), (b, ev[b], res.cost[b])
        # perturbed inputs, kept inside the hard rows step by step (the optimum usually sits on some
        # of them: a free perturbation is almost never feasible) and rolled out on the host through
        # the returned gears' modes; whatever the evaluation accepts costs no less than the optimum
        B = len(desc)
        xp, up = res.x.copy(), res.u.copy()
        for b, d in enumerate(desc):
            for j in range(d[0]):
                tab = tabs[sysv[b, j]]
                for k in range(N):
                    v = xp[b, j, 1, k]
                    cand = [r for r in range(tab.n_regions) if tab.vlo[r] <= v <= tab.vhi[r]
                            and (not gears or tab.gear[r] == res.gear[b, j, k])]
                    r = cand[0] if cand else int(res.region[b, j, k])
                    ar, br, cr = tab.a[r], tab.b[r], tab.c[r]
                    lo = max(tab.umin, (c.a_dec * c.ts - (ar - 1.0) * v - cr) / br)
                    hi = min(tab.umax, (c.a_acc * c.ts - (ar - 1.0) * v - cr) / br)
                    up[b, j, k] = min(max(res.u[b, j, k] + rng.normal(scale=0.02), lo), hi)
                    xp[b, j, 1, k + 1] = ar * v + br * up[b, j, k] + cr
                    xp[b, j, 0, k + 1] = xp[b, j, 0, k] + tab.ts * v
        assert np.abs(up - res.u).max() > 1e-3
        pv, pstat = s.evaluate(desc, sysv, params, xp, up, res.gear if gears else None)
        tried += B
        for b in range(B):
            if pstat[b] == 0:
                accepted += 1
                assert pv[b] >= res.cost[b] * (1.0 - 1e-9), (b, pv[b], res.cost[b])
        if capped:  # the sub-problems with both boundaries that the exhaustive search can finish
            from hvp.event import pack_params

            n = len(desc)
            x = params[:, :6]  # agent i's x0 block: the measured states of vehicles lo .. lo + m - 1
            meas = np.stack([x[0, 0:2]] + [x[i, 2:4] for i in range(1, n)])  # vehicle i is local 1 of agent i >= 1
            sub, sub_sys, sub_prm = [], [], []
            for lo, m in ((1, 1), (2, 1), (3, 1)):
                sub.append((m, 1, 1, -1))
                sub_sys.append(_sys(range(lo, lo + m)))
                sub_prm.append(pack_params(N, meas[lo:lo + m], x_f2=agent.state_guesses[lo - 1],
                                           x_b2=agent.state_guesses[lo + m]))
            sub_sys, sub_prm = np.stack(sub_sys), np.stack(sub_prm)
            r1, r2 = s.solve(sub, sub_sys, sub_prm), exs.solve(sub, sub_sys, sub_prm)
            for b, d in enumerate(sub):
                assert r1.status[b] == 0 and r2.status[b] == 0, (b, r1.status[b], r2.status[b], r2.nodes[b])
                assert np.array_equal(r1.region[b], r2.region[b]), (b, r1.region[b], r2.region[b])
                assert abs(r1.cost[b] - r2.cost[b]) <= 1e-9 * abs(r1.cost[b]), (b, r1.cost[b], r2.cost[b])
                xf2, xb2, xl = _blocks(sub_prm[b], N)
                J = _objective(c, d, r1.x[b, :d[0]], r1.u[b, :d[0]], xf2, xb2, xl)
                assert abs(r1.cost[b] - J) <= 1e-9 * abs(J), (b, r1.cost[b], J)
            print(f"sub-problems: exhaustive QPs {r2.nodes.tolist()}, branch and bound {r1.nodes.tolist()}")
    assert 2 * accepted >= tried, (accepted, tried)  # the projected perturbations mostly stay feasible
    print(f"exhaustive search compared on {compared} of {tried} whole agents ({model}, N = {N})")
    assert capped or compared == tried


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["pwa_gear", "pwa_friction"])
def test_gpu_evaluation(gpu_available, model):
    """hvp_event_evaluate_batch against the numpy restatement: consistent guesses (a solution
    shifted as on_timestep_end shifts it), a guess that leaves its own rollout -> inf, an
    acceleration violation -> inf, the constant-velocity start guesses -> finite."""
    from hvp.event import initial_guesses, local_layout, pack_params, shift_guesses

    N, n = 3, 5
    c = CFGS["time"]
    gears = model == "pwa_friction"
    agent, params, xg, ug, gg = _episode_batches(model, N, [1])[0]
    s, desc, sysv = agent._solver, agent._desc, agent._sys
    tabs = [m.tables[m.me] for m in (a.mpc for a in agent.agents)]

    def restated(b, prm, x, u, g):
        """eval_cost restated: rollout from the guess's column 0, inf when no
        mode holds v_k, a hard row fails or the rollout leaves the guess's states 1..N-1."""
        m = desc[b][0]
        xx = np.zeros((m, 2, N + 1))
        xx[:, :, 0] = x[b, :m, :, 0]
        for j in range(m):
            tab = tabs[sysv[b, j]]
            for k in range(N):
                p, v, uk = xx[j, 0, k], xx[j, 1, k], u[b, j, k]
                tol = 1e-9 * (1.0 + abs(v))
                cand = [r for r in range(tab.n_regions) if tab.vlo[r] - tol <= v <= tab.vhi[r] + tol
                        and (not gears or tab.gear[r] == g[b, j, k])]
                if not cand:
                    return np.inf
                r = cand[0]
                vn = tab.a[r] * v + tab.b[r] * uk + tab.c[r]
                pn = p + tab.ts * v
                if not tab.umin - 1e-9 * (1 + abs(uk)) <= uk <= tab.umax + 1e-9 * (1 + abs(uk)):
                    return np.inf
                if not c.a_dec * c.ts - 1e-9 * (1 + abs(vn - v)) <= vn - v <= c.a_acc * c.ts + 1e-9 * (1 + abs(vn - v)):
                    return np.inf
                if not (tab.vmin - 1e-9 * (1 + abs(vn)) <= vn <= tab.vmax + 1e-9 * (1 + abs(vn))
                        and tab.pmin - 1e-9 * (1 + abs(pn)) <= pn <= tab.pmax + 1e-9 * (1 + abs(pn))):
                    return np.inf
                if k + 1 < N and not (abs(x[b, j, 0, k + 1] - pn) <= 1e-6 * (1 + abs(x[b, j, 0, k + 1]))
                                      and abs(x[b, j, 1, k + 1] - vn) <= 1e-6 * (1 + abs(x[b, j, 1, k + 1]))):
                    return np.inf
                xx[j, :, k + 1] = (pn, vn)
        xf2, xb2, xl = _blocks(prm[b], N)
        return _objective(c, desc[b], xx, u[b, :m], xf2, xb2, xl)

    def check(prm, x, u, g, tag):
        cost, status = s.evaluate(desc, sysv, prm, x, u, g if gears else None)
        for b in range(n):
            J = restated(b, prm, x, u, g)
            assert (status[b] == 0) == bool(np.isfinite(J)), (tag, b, status[b], J)
            assert np.isinf(cost[b]) if np.isinf(J) else abs(cost[b] - J) <= 1e-9 * abs(J), (tag, b, cost[b], J)
        return cost, status

    # (a) consistent guesses: this step's solutions as they are, and the coordinator's guesses one
    # step in (shifted solutions: feasible unless the repeated last input breaks a row)
    res = s.solve(desc, sysv, params)
    cost, status = check(params, res.x, res.u, res.gear, "solved")
    assert (status == 0).all() and np.abs(cost - res.cost).max() <= 1e-9 * np.abs(res.cost).max()
    cost_s, status_s = check(params, xg, ug, gg, "shifted")
    assert (status_s == 0).any()
    xg, ug, gg = res.x, res.u, res.gear
    # the initial condition is the guess's own column 0, not the measured state in params
    moved = params.copy()
    moved[:, :6] += 1.0
    cost2, _ = s.evaluate(desc, sysv, moved, xg, ug, gg if gears else None)
    assert np.array_equal(cost, cost2)
    # (b) a guess whose state 1 is not the rollout's
    bad = xg.copy()
    bad[:, 0, 1, 1] += 0.01
    cost_b, status_b = check(params, bad, ug, gg, "left its rollout")
    assert np.isinf(cost_b).all() and (status_b == 1).all()
    # ... but the last state is free (it is defined by the shifted control)
    free = xg.copy()
    free[:, :, :, N] += 5.0
    cost_f, _ = s.evaluate(desc, sysv, params, free, ug, gg if gears else None)
    assert np.array_equal(cost_f, cost)
    # (c) an input that breaks the acceleration row at the last step (the step to x_N)
    hard = ug.copy()
    hard[:, 0, N - 1] = tabs[0].umax
    cost_a, _ = check(params, xg, hard, gg, "acceleration")
    assert np.isinf(cost_a).any()
    # (d) the episode-start guesses: constant velocity, finite
    x0 = O.env_initial_state(n, 2).astype(float)
    xs, us, gs = initial_guesses(x0, agent.vehicles, N, 1.0, gears)
    lay = local_layout(n, 0)
    p0, x0g, u0g, g0g = [], np.zeros((n, 3, 2, N + 1)), np.zeros((n, 3, N)), np.zeros((n, 3, N), np.int8)
    for i, L in enumerate(lay):
        lo, m = L["lo"], L["m"]
        x0g[i, :m], u0g[i, :m], g0g[i, :m] = xs[lo:lo + m], us[lo:lo + m], gs[lo:lo + m]
        p0.append(pack_params(N, x0[2 * lo:2 * (lo + m)], xs[i - 2] if i >= 2 else None, xs[i + 2] if i + 2 < n else None,
                              leader_window(N) if L["leader"] >= 0 else None))
    cost0, status0 = check(np.stack(p0), x0g, u0g, g0g, "episode start")
    assert (status0 == 0).all() and np.isfinite(cost0).all(), (status0, cost0)
    assert shift_guesses(xs).shape == xs.shape


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 2, 3])
def test_gpu_device_loop_matches_host_coordinator(gpu_available, n):
    """hvp.sweep.run_point(controller="event") against TrackingEventBasedCoordinator seed by seed
    (N = 3, event_iters = 3, ep_len = 6, 8 seeds): the same winner in every iteration, first
    controls equal to 1e-9, every local problem optimal.  n = 2 and 3: the clipped ends."""
    _device_loop_case(n, None)


@pytest.mark.gpu
@pytest.mark.parametrize("n,leader_index", [(5, 2), (4, 3)])
def test_gpu_device_loop_leader_not_first(gpu_available, n, leader_index):
    """The same comparison with the leader window on a vehicle other than 0 (gather's leader block
    for agents leader_index - 1 .. + 1, the layout's leader slot): a middle vehicle and the last."""
    _device_loop_case(n, leader_index)


def _device_loop_case(n, leader_index):
    from types import SimpleNamespace

    from hvp import tables
    from hvp.event import LocalMpc, TrackingEventBasedCoordinator, local_layout
    from hvp.models import Platoon
    from hvp.params import Params, Sim_n_task_2
    from hvp.sweep import run_point

    N, K, T, seeds = 3, 3, 6, list(range(8))
    lead = 0 if leader_index is None else leader_index
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dev = run_point(n, N, seeds, ep_len=T, controller="event", event_iters=K, leader_index=leader_index)
    assert set(dev["status_counts"]) == {"OPTIMAL"}
    solved = 0
    for k, seed in enumerate(seeds):
        # the host coordinator built as hvp.event.simulate builds it, driven step by step with the
        # states of the device episode: both sides then see the same numbers, so agents whose
        # decreases tie (two agents that find the same improvement of their shared vehicles) win
        # or lose alike; the plant itself is pinned in tests/test_envdev.py
        sim = Sim_n_task_2(n, seed=seed, leader_index=leader_index, N=N)
        platoon = Platoon(n, vehicle_type="pwa_gear", masses=sim.masses)
        systems, vehicles = platoon.get_vehicle_system_dicts(Params.ts), platoon.get_vehicles()
        mpcs = [LocalMpc(N, systems[L["lo"]:L["lo"] + L["m"]], L["num_vehicles_in_front"], L["num_vehicles_behind"],
                         sim.spacing_policy, L["rel_leader_index"],
                         gears=[tables.gears_of(v) for v in vehicles[L["lo"]:L["lo"] + L["m"]]])
                for L in local_layout(n, lead)]
        agent = TrackingEventBasedCoordinator(mpcs, vehicles, T, N, dev["leader_x"], False, Params.ts, K, lead)
        X = dev["X"][:, k]
        agent.on_episode_start(SimpleNamespace(x=X[0].reshape(-1, 1)), 0, X[0])
        for t in range(T):
            u, _ = agent.get_control(X[t].reshape(-1, 1))
            w = agent.history[t]["winners"]
            solved += n * len(w)
            w = w + [-1] * (K - len(w))  # the host stops at the first iteration nobody wins
            assert dev["WINNERS"][t, :, k].tolist() == w, (seed, t, dev["WINNERS"][t, :, k], w)
            assert np.abs(dev["U"][t, k] - u[:, 0]).max() <= 1e-9, (seed, t, dev["U"][t, k], u[:, 0])
            agent.on_timestep_end(SimpleNamespace(step_counter=t + 1), 0, t + 1)
        assert np.array_equal(dev["nodes"][:, k], agent.node_counts[:, 0].astype(int)), seed
    assert dev["status_counts"]["OPTIMAL"] == solved


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["pwa_gear", "pwa_friction"])
def test_gpu_shift_kernel_matches_host_rules(gpu_available, model):
    """hvp_event_shift against the numpy rules: the episode-start guesses (states exactly at
    ts = 1; the holding input to rounding, its formula is written on the discrete tables there) and
    the per-step shift exactly."""
    _shift_case(model, 4, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("n,P", [(4, 70), (2, 3)])
@pytest.mark.parametrize("model", ["pwa_gear", "pwa_friction"])
def test_gpu_shift_kernel_two_blocks_and_n2(gpu_available, model, n, P):
    """The same comparison over a second thread block (P n = 280 > 256 items) and at n = 2, the
    episode-start form and the per-step form each."""
    _shift_case(model, n, P)


def _shift_case(model, n, P):
    import torch

    from hvp import tables
    from hvp.cent import cent_problem
    from hvp.event import EventSolver, initial_guesses, shift_guesses
    from hvp.models import Platoon

    N = 3
    dev = torch.device("cuda", 0)
    gears = model == "pwa_friction"
    fleets = [Platoon(n, vehicle_type=model, masses=[700.0 + 60 * i + 11 * p for i in range(n)]) for p in range(P)]
    tabs = [tables.gear_system_from_dict(d) if gears else tables.system_from_dict(d, tables.gears_of(v))
            for pl in fleets for v, d in zip(pl.get_vehicles(), pl.get_vehicle_system_dicts(1))]
    s = EventSolver(cent_problem(N), tabs)
    x = np.stack([O.env_initial_state(n, p).astype(float) for p in range(P)])
    vsys = torch.arange(P * n, dtype=torch.int32, device=dev).view(P, n).contiguous()
    xg = torch.zeros((n, P, 2, N + 1), dtype=torch.float64, device=dev)
    ug = torch.zeros((n, P, N), dtype=torch.float64, device=dev)
    gg = torch.zeros((n, P, N), dtype=torch.int8, device=dev)
    s.shift_device(n, xg, ug, gg, x=torch.from_numpy(x).to(dev), vsys=vsys, init=True)
    torch.cuda.synchronize()
    for p in range(P):
        xs, us, _ = initial_guesses(x[p], fleets[p].get_vehicles(), N, 1.0, gears)
        assert np.array_equal(xg[:, p].cpu().numpy(), xs)
        assert np.abs(ug[:, p].cpu().numpy() - us).max() <= 1e-12 * np.abs(us).max()
        want_gear = [[fleets[p].get_vehicles()[i].get_gear_from_velocity(x[p, 2 * i + 1])] * N for i in range(n)]
        assert gg[:, p].cpu().tolist() == want_gear
    rng = np.random.default_rng(3)
    a, b = rng.normal(size=(n, P, 2, N + 1)), rng.normal(size=(n, P, N))
    g = rng.integers(1, 7, (n, P, N)).astype(np.int8)
    ta, tb, tg = (torch.from_numpy(v).to(dev) for v in (a, b, g))
    s.shift_device(n, ta, tb, tg)
    torch.cuda.synchronize()
    assert np.array_equal(ta.cpu().numpy(), shift_guesses(a))
    assert np.array_equal(tb.cpu().numpy(), shift_guesses(b))
    assert np.array_equal(tg.cpu().numpy(), shift_guesses(g))
