"""k_evaluate (hvp_evaluate_batch, MpcGear.evaluate_cost) against a plain longdouble restatement.

The kernel is a closed-form function of its inputs: roll the fixed (u, gear) out through the PWA
dynamics, check the rows of the MLD model, price the trajectory with the slacks at max(0, .).
``ref_evaluate`` restates exactly that in NumPy longdouble; the CPU tests pin it to the oracle's
optima (cost and trajectory), the GPU tests compare the kernel with it on whole batches that mix
systems, roles and verdicts, on one hand-made instance per row family, across the two regions that
share gear label 4, and with a control / an acceleration exactly on its bound.

A row is judged with the widening the header documents, 1e-9 * (1 + |value|).  A case whose verdict
changes between a widening of 1e-11, 1e-9 and 1e-7 is ambiguous (it sits on a row to rounding, where
the double-precision kernel and the longdouble reference may disagree) and is not compared; the
share of such cases is capped at 10 % per batch, and every batch must hold at least 20 % feasible
and 20 % infeasible counted cases.
"""

from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import pytest

import oracle as O
from instances import decent_instances, leader_window, split_params

LD = np.longdouble
OPTIMAL, INFEASIBLE = 0, 1
MASSES = (800.0, 1100.0)
CFG_A = O.Cfg()
CFG_B = O.Cfg(Qdu=0.5, tight=0.05, t0=0.5, d0=30.0)
CFGS = {"default": CFG_A, "qdu_tight_headway": CFG_B}
MODELS = {"gear_pwa": O.gear_pwa_system, "gear_friction": O.gear_friction_mld_system}
WIDENINGS = (1e-11, 1e-9, 1e-7)
# (leader_index, real_vehicle_as_reference) of the 4-vehicle platoons a batch is drawn from
SETUPS = ((0, False), (2, False), (0, True))


# ------------------------------------------------------------------ the reference
def _table(sysd: dict) -> SimpleNamespace:
    """The velocity-partitioned form of a system dict (include/hvp.h hvp_system), in longdouble."""
    n = len(sysd["S"])
    A = [np.asarray(sysd["A"][r], dtype=float) for r in range(n)]
    t = SimpleNamespace(n=n, ts=LD(A[0][0, 1]), gear=[int(g) for g in sysd["gear"]])
    t.a = [LD(A[r][1, 1]) for r in range(n)]
    t.b = [LD(np.asarray(sysd["B"][r], dtype=float).reshape(2)[1]) for r in range(n)]
    t.c = [LD(np.asarray(sysd["c"][r], dtype=float).reshape(2)[1]) for r in range(n)]
    t.vlo, t.vhi = O.region_bands(sysd)
    lo, hi = [-np.inf, -np.inf], [np.inf, np.inf]
    for row, e in zip(np.asarray(sysd["D"], dtype=float), np.asarray(sysd["E"], dtype=float).reshape(-1)):
        j = int(np.flatnonzero(row)[0])
        if row[j] > 0:
            hi[j] = min(hi[j], e / row[j])
        else:
            lo[j] = max(lo[j], e / row[j])
    t.pmin, t.vmin, t.pmax, t.vmax = lo[0], lo[1], hi[0], hi[1]
    t.umin, t.umax = -np.inf, np.inf
    for f, g in zip(np.asarray(sysd["F"], dtype=float).reshape(-1), np.asarray(sysd["G"], dtype=float).reshape(-1)):
        if f > 0:
            t.umax = min(t.umax, g / f)
        else:
            t.umin = max(t.umin, g / f)
    return t


def ref_evaluate(sysd, cfg, N, role, x0, xf, xb, xl, gears, u, quadratic=True, widen=1e-9) -> SimpleNamespace:
    """hvp_evaluate_batch of one instance in longdouble.  Returns status, cost (1e300 when
    infeasible), x (2, N+1) (NaN past the first step whose mode was not found, ``lost``) and
    ``rows``: (family, k, slack) of every row judged, slack >= 0 meaning satisfied exactly."""
    T = _table(sysd)
    xf, xb, xl = (np.asarray(a, dtype=float).reshape(2, N + 1) for a in (xf, xb, xl))
    wd = lambda val: LD(widen) * (1 + abs(val))  # noqa: E731
    x = np.full((2, N + 1), np.nan, dtype=LD)
    x[:, 0] = np.asarray(x0, dtype=float).reshape(2)
    rows, ok, lost = [], True, N

    def judge(name, k, slack, at):
        nonlocal ok
        rows.append((name, k, float(slack)))
        if slack < -wd(at):
            ok = False

    for k in range(N):
        p, v = x[0, k], x[1, k]
        # the mode: first region carrying the label whose closed band (widened) holds v_k
        r = next((m for m in range(T.n) if T.gear[m] == int(gears[k])
                  and T.vlo[m] - wd(v) <= v <= T.vhi[m] + wd(v)), None)
        if r is None:
            rows.append(("band", k, -np.inf))
            ok, lost = False, k
            break
        rows.append(("band", k, float(min(v - T.vlo[r], T.vhi[r] - v))))
        uk = LD(float(u[k]))
        judge("umin", k, uk - T.umin, uk)
        judge("umax", k, T.umax - uk, uk)
        vn = T.a[r] * v + T.b[r] * uk + T.c[r]
        dv = vn - v
        judge("dec", k, dv - (LD(cfg.a_dec) * LD(cfg.ts) + k * LD(cfg.tight)), dv)
        judge("acc", k, (LD(cfg.a_acc) * LD(cfg.ts) - k * LD(cfg.tight)) - dv, dv)
        pn = p + T.ts * v
        judge("vmin", k, vn - T.vmin, vn)
        judge("vmax", k, T.vmax - vn, vn)
        judge("pmin", k, pn - T.pmin, pn)
        judge("pmax", k, T.pmax - pn, pn)
        x[:, k + 1] = (pn, vn)
    out = SimpleNamespace(status=OPTIMAL if ok else INFEASIBLE, cost=1e300, x=x.astype(np.float64), lost=lost,
                          rows=rows)
    if not ok:
        return out
    # the objective term by term, as the oracle's direct_objective writes it
    Q = [LD(q) for q in cfg.Qx]
    d0, t0, w, ds = LD(cfg.d0), LD(cfg.t0), LD(cfg.w), LD(cfg.d_safe)
    if quadratic:
        stage = lambda ep, ev: Q[0] * ep * ep + (Q[1] + Q[2]) * ep * ev + Q[3] * ev * ev  # noqa: E731
    else:
        stage = lambda ep, ev: abs(Q[0] * ep) + abs(Q[3] * ev)  # noqa: E731
    J = LD(0)
    for k in range(N + 1):
        p, v = x[0, k], x[1, k]
        if role & O.ROLE_TRACK_FRONT:
            J += stage(p + t0 * v + d0 - xf[0, k], v - xf[1, k])
        if role & O.ROLE_TRACK_BACK:
            J += stage(xb[0, k] + t0 * xb[1, k] + d0 - p, xb[1, k] - v)
        if role & O.ROLE_TRACK_LEADER:
            J += stage(p - xl[0, k] + (t0 * v + d0 if role & O.ROLE_LEADER_SPACING else 0), v - xl[1, k])
        if role & O.ROLE_SAFE_FRONT:
            J += w * max(LD(0), p - xf[0, k] + ds)
        if role & O.ROLE_SAFE_BACK:
            J += w * max(LD(0), xb[0, k] + ds - p)
    ul = [LD(float(v)) for v in u]
    for k in range(N):
        J += LD(cfg.Qu) * ul[k] * ul[k] if quadratic else abs(LD(cfg.Qu) * ul[k])
        if k + 1 < N:
            du = ul[k + 1] - ul[k]
            J += LD(cfg.Qdu) * du * du if quadratic else abs(LD(cfg.Qdu) * du)
    out.cost = float(J)
    return out


def ref_lane(sysd, cfg, N, role, prm, gears, u, quadratic):
    """ref_evaluate of one parameter row at the three widenings: (the 1e-9 result, counted)."""
    x0, xf, xb, xl = split_params(np.asarray(prm, dtype=float), N)
    rs = [ref_evaluate(sysd, cfg, N, int(role), x0, xf, xb, xl, gears, u, quadratic, wdn) for wdn in WIDENINGS]
    return rs[1], len({r.status for r in rs}) == 1


# ------------------------------------------------------------------ the reference against the oracle
@pytest.mark.parametrize("quadratic", [True, False], ids=["l2", "l1"])
@pytest.mark.parametrize("cfg", list(CFGS), ids=list(CFGS))
@pytest.mark.parametrize("model", list(MODELS), ids=list(MODELS))
def test_reference_reproduces_the_oracle_optima(model, cfg, quadratic):
    """ref_evaluate(u*, gear*) of the oracle's optima: feasible, the oracle's cost to 1e-9 relative
    (the project's cost bar) and its trajectory to 1e-9.  All four roles of a 4-platoon, N = 2 and 5,
    seeds 0-2."""
    sysd, c = MODELS[model](800.0), CFGS[cfg]
    worst = 0.0
    O.set_method(O.METHOD_BNB)  # the same optima as the enumeration, in a fraction of its time
    try:
        worst = _self_check(sysd, c, quadratic)
    finally:
        O.set_method(O.METHOD_ENUMERATE)
    print(f"reference vs oracle, worst relative cost error {worst:.2e}")


def _self_check(sysd, c, quadratic) -> float:
    worst = 0.0
    for N in (2, 5):
        for seed in range(3):
            params, roles = decent_instances(O.env_initial_state(4, seed).astype(float), N, leader_window(N))
            for prm, role in zip(params, roles):
                x0, xf, xb, xl = split_params(prm, N)
                res = O.solve_miqp(sysd, c, N, int(role), x0, xf, xb, xl, quadratic=quadratic)
                assert res.status == 0
                ref = ref_evaluate(sysd, c, N, int(role), x0, xf, xb, xl, sysd["gear"][res.sigma], res.u, quadratic)
                assert ref.status == OPTIMAL, (N, seed, int(role), [r for r in ref.rows if r[2] < 0])
                assert abs(ref.cost - res.cost) <= 1e-9 * abs(res.cost), (N, seed, int(role), ref.cost, res.cost)
                assert np.abs(ref.x - res.x).max() <= 1e-9 * max(1.0, np.abs(res.x).max())
                worst = max(worst, abs(ref.cost - res.cost) / abs(res.cost))
    return worst


# ------------------------------------------------------------------ batches
@functools.lru_cache(maxsize=None)
def make_batch(model: str, cfg: str, quadratic: bool, N: int, seeds: tuple = (0, 1, 2)) -> SimpleNamespace:
    """One evaluate batch and its reference (computed once per session, shared by the CPU share
    test and the GPU comparison).  Per base instance -- every vehicle of the 4-platoons of SETUPS
    at the env's initial states of ``seeds``, masses mixed -- six (u, gear) inputs:
      0 the oracle's optimum (u*, gear*)        3 u uniform in the box, gear* kept
      1 u* + N(0, 0.05) clipped to the box      4 gear* with one step moved to the next label
      2 u* + N(0, 0.3) clipped                  5 one u_k set to umax + 1e-3
    in an order shuffled by the fixed seed, so neighbouring lanes differ in role, system and verdict."""
    c = CFGS[cfg]
    systems = [MODELS[model](m) for m in MASSES]
    rng = np.random.default_rng(1234)
    labels = sorted(set(int(g) for g in systems[0]["gear"]))
    O.set_method(O.METHOD_BNB)  # the same optima as the enumeration, in a fraction of its time
    try:
        lanes, nbase = [], 0
        for seed in seeds:
            for leader_index, rvr in SETUPS:
                state = O.env_initial_state(4, seed).astype(float)
                params, roles = decent_instances(state, N, leader_window(N), leader_index, rvr)
                for prm, role in zip(params, roles):
                    s = (nbase + nbase // 4) % 2
                    nbase += 1
                    x0, xf, xb, xl = split_params(prm, N)
                    res = O.solve_miqp(systems[s], c, N, int(role), x0, xf, xb, xl, quadratic=quadratic)
                    assert res.status == 0, (seed, leader_index, rvr, int(role))
                    us, gs = res.u.copy(), np.asarray(systems[s]["gear"])[res.sigma].astype(np.int8)
                    T = _table(systems[s])
                    box = lambda v: np.clip(v, T.umin, T.umax)  # noqa: E731
                    k5, k6 = int(rng.integers(N)), int(rng.integers(N))
                    g5, u6 = gs.copy(), us.copy()
                    g5[k5] = gs[k5] + 1 if gs[k5] < labels[-1] else gs[k5] - 1
                    u6[k6] = T.umax + 1e-3
                    for kind, (uu, gg) in enumerate(((us, gs), (box(us + rng.normal(0, 0.05, N)), gs),
                                                     (box(us + rng.normal(0, 0.3, N)), gs),
                                                     (rng.uniform(T.umin, T.umax, N), gs), (us, g5), (u6, gs))):
                        lanes.append((s, int(role), prm, gg, np.asarray(uu, dtype=float), kind))
    finally:
        O.set_method(O.METHOD_ENUMERATE)
    order = rng.permutation(len(lanes))
    lanes = [lanes[j] for j in order]
    b = SimpleNamespace(N=N, cfg=c, quadratic=quadratic, model=model, masses=MASSES, B=len(lanes))
    b.sys = np.array([l[0] for l in lanes], dtype=np.int32)
    b.roles = np.array([l[1] for l in lanes], dtype=np.int32)
    b.params = np.array([l[2] for l in lanes])
    b.gears = np.array([l[3] for l in lanes], dtype=np.int8)
    b.u = np.array([l[4] for l in lanes])
    b.kind = np.array([l[5] for l in lanes])
    refs = [ref_lane(systems[l[0]], c, N, l[1], l[2], l[3], l[4], quadratic) for l in lanes]
    b.ref = [r[0] for r in refs]
    b.counted = np.array([r[1] for r in refs])
    b.status = np.array([r.status for r in b.ref])
    return b


def batch_shares(b) -> tuple[float, float, float]:
    """(ambiguous, feasible, infeasible) shares of a batch; the last two over the counted cases."""
    return (float(np.mean(~b.counted)), float(np.sum(b.counted & (b.status == OPTIMAL))) / b.B,
            float(np.sum(b.counted & (b.status == INFEASIBLE))) / b.B)


# every (cost, config, model): at N = 5, but for min_1_norm on the gear-friction modes at N = 2 (the
# oracle's MILP over 11 modes takes seconds per instance from N = 5 on); N = 2 and 8 on two more;
# N = 10 (a second template instantiation, past the enumeration horizon) once.  Optima by the
# oracle's branch and bound.
BATCHES = [(m, c, q, 2 if (m, q) == ("gear_friction", False) else 5)
           for q in (True, False) for c in CFGS for m in MODELS] + [
    ("gear_pwa", "default", True, 2), ("gear_pwa", "qdu_tight_headway", True, 8),
    ("gear_friction", "default", True, 8, (0,))]
BATCH_N10 = ("gear_pwa", "default", True, 10, (0,))
ALL_BATCHES = BATCHES + [BATCH_N10]


def _bid(t):
    return f"{t[0]}-{t[1]}-{'l2' if t[2] else 'l1'}-N{t[3]}"


@pytest.mark.parametrize("spec", ALL_BATCHES, ids=_bid)
def test_batch_generator_shares(spec):
    """The generator meets the conditions the GPU comparison relies on: at most 10 % ambiguous
    cases, at least 20 % feasible and 20 % infeasible counted ones, and mixed neighbours."""
    b = make_batch(*spec)
    amb, feas, infeas = batch_shares(b)
    print(f"{_bid(spec)}: B = {b.B}, ambiguous {amb:.3f}, feasible {feas:.3f}, infeasible {infeas:.3f}")
    assert amb <= 0.10 and feas >= 0.20 and infeas >= 0.20, (amb, feas, infeas)
    # dense mixing: most neighbouring lanes differ in role, system or verdict
    assert np.mean(b.roles[1:] != b.roles[:-1]) > 0.5
    assert np.mean(b.sys[1:] != b.sys[:-1]) > 0.3
    assert np.mean(b.status[1:] != b.status[:-1]) > 0.3
    assert len(set(b.roles.tolist())) >= 6  # leader (with / without spacing), front, middle, trailer roles


# ------------------------------------------------------------------ the kernel
def _product(model: str, cfg: O.Cfg, quadratic: bool, N: int, masses=MASSES):
    """BatchSolver of the product's own tables for the oracle's (model, cfg)."""
    from golden_io import CfgParams
    from hvp import tables
    from hvp.models import PwaFrictionVehicle, PwaGearVehicle
    from hvp.params import ConstantTimePolicy
    from hvp.solver import BatchSolver

    cp = CfgParams(cfg.vector())
    prob = tables.problem(N, ConstantTimePolicy(cp.d0, cp.t0), quadratic, accel_cnstr_tightening=cp.tight, params=cp)
    systems = []
    for m in masses:
        if model == "gear_friction":
            systems.append(tables.gear_system_from_dict(PwaFrictionVehicle(float(m)).get_discrete_system(float(cp.ts))))
        else:
            veh = PwaGearVehicle(float(m))
            systems.append(tables.system_from_dict(veh.get_discrete_system(float(cp.ts)), tables.gears_of(veh)))
    return BatchSolver(prob, systems)


def _compare(out, refs, counted, N, what):
    """The issue's assertions of one evaluated batch against its references; returns the worst
    relative cost error and the worst x error in units of max(1, |x|)."""
    worst_c = worst_x = 0.0
    for i, (ref, cnt) in enumerate(zip(refs, counted)):
        x = out["x"][i]
        # the trajectory is the rollout whatever the verdict, up to the first step without a mode
        head = slice(0, ref.lost + 1)
        ex = np.abs(x[:, head] - ref.x[:, head]) / np.maximum(1.0, np.abs(ref.x[:, head]))
        worst_x = max(worst_x, float(ex.max()))
        assert ex.max() <= 1e-9, (what, i, "x", float(ex.max()))
        if not cnt:
            continue
        assert int(out["status"][i]) == ref.status, (what, i, "status", int(out["status"][i]), ref.status,
                                                     [r for r in ref.rows if r[2] < 1e-6])
        if ref.status == OPTIMAL:
            ec = abs(float(out["cost"][i]) - ref.cost) / abs(ref.cost)
            worst_c = max(worst_c, ec)
            assert ec <= 1e-9, (what, i, "cost", float(out["cost"][i]), ref.cost)
        else:
            assert float(out["cost"][i]) == 1e300, (what, i, float(out["cost"][i]))
    return worst_c, worst_x


@pytest.mark.gpu
@pytest.mark.parametrize("spec", ALL_BATCHES, ids=_bid)
def test_evaluate_batch_matches_reference(gpu_available, spec):
    """Whole batches through BatchSolver.evaluate: status wherever the reference's verdict is
    unambiguous, cost to 1e-9 relative where feasible and exactly 1e300 where not, x_out to
    1e-9 max(1, |x|); x_out = NULL changes neither cost nor status."""
    b = make_batch(*spec)
    amb, feas, infeas = batch_shares(b)
    assert amb <= 0.10 and feas >= 0.20 and infeas >= 0.20, (amb, feas, infeas)
    solver = _product(b.model, b.cfg, b.quadratic, b.N)
    out = solver.evaluate(b.sys, b.roles, b.params, b.gears, b.u)
    worst_c, worst_x = _compare(out, b.ref, b.counted, b.N, _bid(spec))
    print(f"{_bid(spec)}: B = {b.B}, ambiguous {amb:.3f}, feasible {feas:.3f}, infeasible {infeas:.3f}, "
          f"worst relative cost error {worst_c:.2e}, worst x error {worst_x:.2e}")
    nox = solver.evaluate(b.sys, b.roles, b.params, b.gears, b.u, want_x=False)
    assert "x" not in nox
    assert np.array_equal(nox["cost"], out["cost"]) and np.array_equal(nox["status"], out["status"])


# ------------------------------------------------------------------ hand-made instances
def _solve_u(T, r, v, dv):
    """u with a[r] v + b[r] u + c[r] - v = dv, solved in longdouble, rounded to double."""
    return float((LD(v) + LD(dv) - T.a[r] * LD(v) - T.c[r]) / T.b[r])


def _region_of(T, v, label=None):
    return next(m for m in range(T.n) if T.vlo[m] <= v <= T.vhi[m] and (label is None or T.gear[m] == label))


def _drive(sysd, N, v0, dvs):
    """(u, gears) that give the velocity steps dvs from v0, each step in the first region whose
    band holds its velocity."""
    T = _table(sysd)
    v, u, g = LD(v0), [], []
    for k in range(N):
        r = _region_of(T, v)
        uk = _solve_u(T, r, v, dvs[k])
        u.append(uk)
        g.append(T.gear[r])
        v = T.a[r] * v + T.b[r] * LD(uk) + T.c[r]
    return np.array(u), np.array(g, dtype=np.int8)


def _middle_params(N, p0, v0, gap=80.0, gap_back=None):
    """Parameter row and role of a middle vehicle whose neighbours drive at its speed `gap` ahead
    and `gap_back` (default: gap) behind."""
    xf = O.constant_velocity_prediction(p0 + gap, v0, N)
    xb = O.constant_velocity_prediction(p0 - (gap if gap_back is None else gap_back), v0, N)
    prm = np.concatenate([[p0, v0], xf.ravel(), xb.ravel(), np.zeros(2 * (N + 1))])
    return prm, O.role_bits(1, 3)


ROW_N = 5
ROW_CFG = O.Cfg(tight=0.05)


def _row_cases():
    """One instance per row family of the model: (name, violated row or None, parameter row, gears,
    u) twice -- the row violated by 1e-3, and the same instance 1e-3 inside it.  7-region gear
    model, m = 800, N = 5, accel tightening 0.05."""
    N, c = ROW_N, ROW_CFG
    sysd = O.gear_pwa_system(800.0)
    T = _table(sysd)
    acc = lambda k: c.a_acc * c.ts - k * c.tight  # noqa: E731
    cases = []

    def both(name, row, build):
        for sign, tag in ((+1, "violated"), (-1, "inside")):
            p0, v0, u, g = build(sign * 1e-3)
            prm, role = _middle_params(N, p0, v0)
            cases.append((f"{name}-{tag}", row if sign > 0 else None, prm, role, g, u))

    def u_below_umin(e):  # gear 5 at 25 m/s: even u < umin decelerates within the first step's accel row
        r = _region_of(T, 25.0)
        dv0 = float(T.a[r] * 25 + T.b[r] * (LD(T.umin) - LD(e)) + T.c[r] - 25)
        u, g = _drive(sysd, N, 25.0, [dv0] + [0.0] * (N - 1))
        u[0] = T.umin - e
        return 3000.0, 25.0, u, g

    def acc_last(e):  # only the per-step tightening makes the last step's acceleration too large
        u, g = _drive(sysd, N, 14.0, [0.0] * (N - 1) + [acc(N - 1) + e])
        return 3000.0, 14.0, u, g

    def dec_first(e):
        u, g = _drive(sysd, N, 30.0, [c.a_dec * c.ts - e] + [0.0] * (N - 1))
        return 3000.0, 30.0, u, g

    def v_above(e):  # x_0 is outside the state box's rows (k = 1..N): v_1 is the only one past vmax
        v0 = float(T.vmax) + 0.5 + e
        u, g = _drive(sysd, N, v0, [-0.5] * N)
        return 3000.0, v0, u, g

    def v_below(e):
        v0 = float(T.vmin) + 1.0
        u, g = _drive(sysd, N, v0, [0.0] * (N - 1) + [-1.0 - e])
        return 3000.0, v0, u, g

    def p_above(e):
        u, g = _drive(sysd, N, 20.0, [0.0] * N)
        return float(T.pmax) + e - 20.0 * N, 20.0, u, g

    both("u_below_umin", "umin", u_below_umin)
    both("acc_at_last_step", "acc", acc_last)
    both("dec_at_first_step", "dec", dec_first)
    both("v_above_vmax", "vmax", v_above)
    both("v_below_vmin", "vmin", v_below)
    both("p_above_pmax", "pmax", p_above)
    # a gear whose window does not hold v_0 / a label the table does not have; the twin is the
    # same instance with the right label
    u, g = _drive(sysd, N, 20.0, [0.0] * N)
    prm, role = _middle_params(N, 3000.0, 20.0)
    for name, label in (("gear_window_misses_v0", 2), ("gear_label_absent", 9)):
        bad = g.copy()
        bad[0] = label
        cases.append((f"{name}-violated", "band", prm, role, bad, u))
    cases.append(("gear-inside", None, prm, role, g, u))
    return sysd, cases


def test_row_cases_violate_exactly_one_row():
    """The hand-made instances are what they claim: the violated one misses exactly its own row
    family, at one step, by 1e-3, with every other row slack by at least 1e-3; its twin is feasible
    with every row slack by at least 1e-3 (the band rows included: the chosen speeds keep far
    from every band edge)."""
    sysd, cases = _row_cases()
    for name, row, prm, role, g, u in cases:
        x0, xf, xb, xl = split_params(prm, ROW_N)
        ref = ref_evaluate(sysd, ROW_CFG, ROW_N, role, x0, xf, xb, xl, g, u)
        bad = [(f, k, s) for f, k, s in ref.rows if s < 1e-3 * (1 - 1e-6)]
        if row is None:
            assert ref.status == OPTIMAL and not bad, (name, bad)
        else:
            assert ref.status == INFEASIBLE and len(bad) == 1 and bad[0][0] == row, (name, bad)
            if row != "band":
                assert abs(bad[0][2] + 1e-3) <= 1e-9, (name, bad)


@pytest.mark.gpu
def test_each_row_family_makes_its_instance_infeasible(gpu_available):
    """One violated row, whichever it is, gives HVP_INFEASIBLE and cost 1e300; the same instance
    with the violation removed is HVP_OPTIMAL at the reference cost."""
    sysd, cases = _row_cases()
    solver = _product("gear_pwa", ROW_CFG, True, ROW_N, masses=(800.0,))
    out = solver.evaluate(np.zeros(len(cases), np.int32), [c[3] for c in cases], np.array([c[2] for c in cases]),
                          np.array([c[4] for c in cases], dtype=np.int8), np.array([c[5] for c in cases]))
    for i, (name, row, prm, role, g, u) in enumerate(cases):
        x0, xf, xb, xl = split_params(prm, ROW_N)
        ref = ref_evaluate(sysd, ROW_CFG, ROW_N, role, x0, xf, xb, xl, g, u)
        if row is None:
            assert int(out["status"][i]) == OPTIMAL, name
            assert abs(float(out["cost"][i]) - ref.cost) <= 1e-9 * abs(ref.cost), (name, out["cost"][i], ref.cost)
        else:
            assert int(out["status"][i]) == INFEASIBLE and float(out["cost"][i]) == 1e300, (name, out["cost"][i])
        head = slice(0, ref.lost + 1)
        assert (np.abs(out["x"][i][:, head] - ref.x[:, head]) <= 1e-9 * np.maximum(1.0, np.abs(ref.x[:, head]))).all()


def _shared_label_cases(N=5):
    """Label 4 across alpha = vmax / 2, where regions 3 and 4 of the 7-region model meet: upwards,
    downwards, and from exactly alpha (the first region carrying the label, 3, is the mode)."""
    sysd = O.gear_pwa_system(800.0)
    T = _table(sysd)
    alpha = float(T.vhi[3])
    assert T.gear[3] == T.gear[4] == 4 and T.vlo[4] == alpha == float(T.vmax) / 2
    width = float(T.vhi[4]) - alpha
    cases = []
    for v0, dv in ((alpha - 2.5 * width / 4, width / 4), (alpha + 3.5 * width / 4, -width / 4), (alpha, width / 8)):
        u, g = _drive(sysd, N, v0, [dv] * N)
        assert (g == 4).all()
        prm, role = _middle_params(N, 3000.0, v0)
        cases.append((prm, role, g, u))
    return sysd, cases


def test_shared_label_cases_cross_alpha():
    sysd, cases = _shared_label_cases()
    T = _table(sysd)
    alpha = float(T.vhi[3])
    sides = []
    for prm, role, g, u in cases:
        x0, xf, xb, xl = split_params(prm, 5)
        ref = ref_evaluate(sysd, O.Cfg(), 5, role, x0, xf, xb, xl, g, u)
        assert ref.status == OPTIMAL and min(s for f, k, s in ref.rows if f != "band") >= 1e-3
        sides.append((ref.x[1, 0] < alpha, ref.x[1, -2] < alpha))
    assert sides[0] == (True, False) and sides[1] == (False, True) and cases[2][0][1] == alpha


@pytest.mark.gpu
def test_shared_gear_label_across_alpha(gpu_available):
    sysd, cases = _shared_label_cases()
    solver = _product("gear_pwa", O.Cfg(), True, 5, masses=(800.0,))
    out = solver.evaluate(np.zeros(len(cases), np.int32), [c[1] for c in cases], np.array([c[0] for c in cases]),
                          np.array([c[2] for c in cases], dtype=np.int8), np.array([c[3] for c in cases]))
    for i, (prm, role, g, u) in enumerate(cases):
        x0, xf, xb, xl = split_params(prm, 5)
        ref = ref_evaluate(sysd, O.Cfg(), 5, role, x0, xf, xb, xl, g, u)
        assert int(out["status"][i]) == OPTIMAL
        assert abs(float(out["cost"][i]) - ref.cost) <= 1e-9 * abs(ref.cost)
        assert (np.abs(out["x"][i] - ref.x) <= 1e-9 * np.maximum(1.0, np.abs(ref.x))).all()


def _on_bound_cases(N=5):
    """u_k = umax exactly, and steps whose dv equals a_acc ts (or a_dec ts) exactly -- u solved in
    longdouble and rounded to double, from 16 speeds each so that the double-precision dv falls on
    either side of its bound."""
    c = O.Cfg()
    sysd = O.gear_pwa_system(800.0)
    T = _table(sysd)
    cases = []
    for v0 in np.linspace(33.0, 37.0, 8):  # gear 6: full throttle stays inside the accel rows
        u, g = _drive(sysd, N, float(v0), [0.0] * N)
        u[1] = u[3] = float(T.umax)
        cases.append((float(v0), g, u))
    # the full acceleration is within the input box in gears 1-2, the full deceleration at speed
    speeds = [(v, c.a_acc * c.ts) for v in np.linspace(5.0, 12.0, 16)] + [
        (v, c.a_dec * c.ts) for v in np.concatenate([np.linspace(28.5, 32.0, 8), np.linspace(36.5, 37.5, 8)])]
    for j, (v0, bound) in enumerate(speeds):
        dvs = [0.0] * N
        dvs[j % N] = bound
        u, g = _drive(sysd, N, float(v0), dvs)
        cases.append((float(v0), g, u))
    # every third lane has the vehicle ahead, every other third the one behind, inside d_safe = 25:
    # one active and one inactive hinge, which a swapped or mis-signed hinge prices differently
    gaps = ((20.0, 80.0), (80.0, 22.0), (80.0, 80.0))
    return sysd, c, [(*_middle_params(N, 3000.0, v0, *gaps[j % 3]), g, u) for j, (v0, g, u) in enumerate(cases)]


def test_on_bound_cases_are_on_their_bound():
    sysd, c, cases = _on_bound_cases()
    for prm, role, g, u in cases:
        x0, xf, xb, xl = split_params(prm, 5)
        ref = ref_evaluate(sysd, c, 5, role, x0, xf, xb, xl, g, u)
        assert ref.status == OPTIMAL
        tight = [(f, k, s) for f, k, s in ref.rows if abs(s) <= 1e-12]
        assert tight and all(f in ("umax", "acc", "dec") for f, k, s in tight), tight


@pytest.mark.gpu
def test_equality_on_a_bound_is_feasible(gpu_available):
    sysd, c, cases = _on_bound_cases()
    solver = _product("gear_pwa", c, True, 5, masses=(800.0,))
    out = solver.evaluate(np.zeros(len(cases), np.int32), [k[1] for k in cases], np.array([k[0] for k in cases]),
                          np.array([k[2] for k in cases], dtype=np.int8), np.array([k[3] for k in cases]))
    for i, (prm, role, g, u) in enumerate(cases):
        x0, xf, xb, xl = split_params(prm, 5)
        ref = ref_evaluate(sysd, c, 5, role, x0, xf, xb, xl, g, u)
        assert int(out["status"][i]) == OPTIMAL, i
        assert abs(float(out["cost"][i]) - ref.cost) <= 1e-9 * abs(ref.cost)
