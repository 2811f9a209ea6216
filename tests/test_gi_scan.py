"""The active-set scan (csrc/hvp_gi.h gi_most_violated): which row the Goldfarb-Idnani step adds.

The rule, restated here in NumPy (_rule): the rows are looked at step by step -- the six V/U/A
rows of step k (ids 6(k-1) + {V_lo, V_hi, U_lo, U_hi, A_lo, A_hi}), then, from k = 2, its four
prefix rows (ids 6N + 4(k-2) + {P_lo, P_hi, SF, SB}).  Active rows are skipped.  A row is a
candidate when slack < -1e-11 * scale; a saturated soft row stands reversed (id | 256, slack and
bound negated).  Among the candidates the largest slack^2 / |c|^2 wins, compared cross-multiplied
and strictly, so of equal ones the first looked at wins.  The row's bound d (<= form) and its
U-row coefficient a come back with it.

CPU part: the host build's export hvp_hostref_gi_scan (the header compiled with -ffp-contract=off,
so the restatement's float64 arithmetic is the same bit for bit: id, d and a are compared for
equality) over lane QPs whose row data the cases set; and, since the host build shares the
header, its full solves of tests/instances.py against the oracle.

GPU part: role-mixed batches of the default problem at N = 2, 5, 8 (one and nine systems; 1, 37
and 300 instances: one lane, a partial wave, more than one block) and at N = 10 against the host
build: status, regions, gears and node counts equal, cost 1e-9 relative, u 1e-6, x 1e-4 (the
bars of test_refill_tables.py).  (At N = 10 most of the search's QPs are the wave-cooperative
solver's, hvp_coop.h, which has its own scan; the lane QPs of that unit inline this one.)
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

REV = 256
TOL = 1e-11
F_AM, F_VLO, F_VHI, F_ULO, F_UHI, F_HF, F_HB, F_COUNT = range(8)
HORIZONS = (2, 5, 8)
BIG = 1.0e6


# ---------------------------------------------------------------- the rule, restated

def _rows(N, data, y, sat):
    """(id, slack, nn, scale, d, a) of every row in the scan's order; Python floats throughout."""
    f = [float(v) for v in data]
    row = lambda fld, j: f[fld * N + j]  # noqa: E731
    v0, P1, ts, pmin, pmax = f[F_COUNT * N:F_COUNT * N + 5]
    dec = f[F_COUNT * N + 5:F_COUNT * N + 5 + N]
    acc = f[F_COUNT * N + 5 + N:F_COUNT * N + 5 + 2 * N]
    y = [float(v) for v in y]
    out = []
    yprev, cum = v0, 0.0
    for j in range(N):
        yk, a = y[j], row(F_AM, j)
        gv, gu, ga = yk, yk - a * yprev, yk - yprev
        nu, na = (1.0 + a * a, 2.0) if j else (1.0, 1.0)
        vl, vh, ul, uh, al, ah = row(F_VLO, j), row(F_VHI, j), row(F_ULO, j), row(F_UHI, j), dec[j], acc[j]
        cu, ca = (-a * v0, -v0) if j == 0 else (0.0, 0.0)
        su = 1.0 + abs(ul) + abs(a * yprev), 1.0 + abs(uh) + abs(a * yprev)
        out += [(6 * j + 0, gv - vl, 1.0, 1.0 + abs(vl), -vl, a),
                (6 * j + 1, vh - gv, 1.0, 1.0 + abs(vh), vh, a),
                (6 * j + 2, gu - ul, nu, su[0], cu - ul, a),
                (6 * j + 3, uh - gu, nu, su[1], uh - cu, a),
                (6 * j + 4, ga - al, na, 1.0 + abs(yprev), ca - al, a),
                (6 * j + 5, ah - ga, na, 1.0 + abs(yprev), ah - ca, a)]
        if j >= 1:
            m = j - 1
            cum += y[m]
            p, nn = P1 + ts * cum, ts * ts * (m + 1)
            sc, b = 1.0 + abs(p), 6 * N + 4 * m
            hf, hb = row(F_HF, m), row(F_HB, m)
            sfw, sbw = hf - p, p - hb
            satf, satb = (sat >> (2 * m)) & 1, (sat >> (2 * m + 1)) & 1
            out += [(b + 0, p - pmin, nn, sc, P1 - pmin, a),
                    (b + 1, pmax - p, nn, sc, pmax - P1, a),
                    ((b + 2) | REV, -sfw, nn, sc, P1 - hf, a) if satf else (b + 2, sfw, nn, sc, hf - P1, a),
                    ((b + 3) | REV, -sbw, nn, sc, hb - P1, a) if satb else (b + 3, sbw, nn, sc, P1 - hb, a)]
        yprev = yk
    return out


def _rule(N, data, y, active=(), sat=0):
    """(id, d, a) of the row the rule picks; (-1, 0.0, 0.0) when there is no candidate."""
    best = None
    for rid, slack, nn, scale, d, a in _rows(N, data, y, sat):
        if (rid & (REV - 1)) in active or not slack < -TOL * scale:
            continue
        v2 = slack * slack
        if best is None or v2 * best[2] > best[1] * nn:
            best = (rid, v2, nn, d, a)
    return (best[0], best[3], best[4]) if best else (-1, 0.0, 0.0)


def _family(N, rid):
    base = rid & (REV - 1)
    name = ("V_lo", "V_hi", "U_lo", "U_hi", "A_lo", "A_hi")[base % 6] if base < 6 * N else \
        ("P_lo", "P_hi", "SF", "SB")[(base - 6 * N) % 4]
    return name + ("_rev" if rid & REV else "")


# ---------------------------------------------------------------- the host build's scan

@functools.lru_cache(maxsize=None)
def _lib():
    from hvp import _abi

    L = ctypes.CDLL(_abi.HOSTREF_PATH)
    L.hvp_hostref_gi_scan.restype = ctypes.c_int
    L.hvp_hostref_gi_scan.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                      ctypes.c_ulonglong, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p]
    return L


@functools.lru_cache(maxsize=None)
def _lane(N, which=0):
    """(problem, system, role, parameter row) of one local problem of a benchmark platoon:
    which = 0 the leader, 1 a middle vehicle, 2 the trailer."""
    import bench
    from hvp import tables
    from hvp.models import PwaGearVehicle

    veh = PwaGearVehicle(800.0)
    table = tables.system_from_dict(veh.get_discrete_system(1), tables.gears_of(veh))
    params, roles = bench.make_inputs(range(1), 10, N)
    i = (0, 4, 9)[which]
    return tables.problem(N), table, int(roles[i]), np.ascontiguousarray(params[i])


def _scan(N, y, active=(), sat=0, data=None, which=0, code=0, K=0, interval=None):
    """The export: (id, d, a, the lane data the scan read)."""
    prob, table, role, prm = _lane(N, which)
    lo, hi = interval if interval is not None else (float(prm[1]), float(prm[1]))  # K = 0: the root's [v0, v0]
    y = np.ascontiguousarray(y, dtype=np.float64)
    act = np.ascontiguousarray(sorted(active), dtype=np.int32)
    din = None if data is None else np.ascontiguousarray(data, dtype=np.float64)
    dout = np.zeros(F_COUNT * N + 5 + 2 * N)
    rid, d, a = ctypes.c_int32(-7), ctypes.c_double(), ctypes.c_double()
    p = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = _lib().hvp_hostref_gi_scan(ctypes.byref(prob), ctypes.byref(table), role, p(prm), code, K, lo, hi, p(y),
                                    p(act) if len(act) else None, len(act), sat, None if din is None else p(din),
                                    p(dout), ctypes.byref(rid), ctypes.byref(d), ctypes.byref(a))
    assert rc == 0
    return rid.value, d.value, a.value, dout


def _same(N, y, active=(), sat=0, data=None, **kw):
    """Runs the export, checks it against the rule on the data it read and returns the id."""
    rid, d, a, dout = _scan(N, y, active, sat, data, **kw)
    if data is not None:
        assert np.array_equal(dout, np.asarray(data, dtype=np.float64))
    want = _rule(N, dout, y, set(active), sat)
    assert (rid, d, a) == want, (rid, d, a, want)
    return rid


def _loose(N, v=20.0):
    """Lane data no row of which is near its bound at y = v: every case tightens what it tests."""
    d = np.zeros(F_COUNT * N + 5 + 2 * N)
    r = d[:F_COUNT * N].reshape(F_COUNT, N)
    r[F_AM] = 0.9 + 0.01 * np.arange(N)
    r[F_VLO], r[F_VHI], r[F_ULO], r[F_UHI] = -BIG, BIG, -BIG, BIG
    r[F_HF], r[F_HB] = BIG, -BIG
    d[F_COUNT * N:F_COUNT * N + 5] = (v, 100.0, 1.0, -BIG, BIG)  # v0, P1, ts, pmin, pmax
    d[F_COUNT * N + 5:F_COUNT * N + 5 + N] = -BIG                # dec
    d[F_COUNT * N + 5 + N:] = BIG                                # acc
    return d


def _set(d, N, fld, j, x):
    d[:F_COUNT * N].reshape(F_COUNT, N)[fld, j] = x


# ---------------------------------------------------------------- CPU cases

@pytest.mark.parametrize("N", HORIZONS)
def test_lane_data_of_real_problems(N):
    """The lane QPs of a leader, a middle vehicle and a trailer (root relaxation and a fixed
    sequence), scanned at random points around v0."""
    rng = np.random.default_rng(100 + N)
    picked = set()
    for which in range(3):
        _, _, _, prm = _lane(N, which)
        for kw in (dict(), dict(code=sum(2 << (4 * k) for k in range(N)), K=N, interval=(0.0, -1.0))):
            for spread in (0.01, 0.5, 3.0, 15.0):
                for _ in range(12):
                    y = prm[1] + spread * rng.standard_normal(N)
                    picked.add(_same(N, y, which=which, **kw))
    assert len(picked) >= 4 and -1 not in picked or len(picked) >= 5


@pytest.mark.parametrize("N", HORIZONS)
def test_random_rows_every_family_wins(N):
    """Random bounds around a random y, random active sets and saturation bits: the export equals
    the rule every time, and every row family, both reversed soft rows included, wins somewhere."""
    rng = np.random.default_rng(N)
    won = set()
    ids = set()
    for trial in range(600):
        d = _loose(N)
        r = d[:F_COUNT * N].reshape(F_COUNT, N)
        y = 20.0 + 3.0 * rng.standard_normal(N)
        yprev = np.concatenate([[20.0], y[:-1]])
        p = 100.0 + np.cumsum(y)[:N - 1]
        tight = lambda n: np.where(rng.random(n) < 0.25, rng.normal(0.0, 1.0, n), BIG)  # noqa: E731
        r[F_VLO], r[F_VHI] = y - np.abs(tight(N)) * np.sign(tight(N)), y + tight(N)
        gu = y - r[F_AM] * yprev
        r[F_ULO], r[F_UHI] = gu - tight(N), gu + tight(N)
        d[F_COUNT * N + 5:F_COUNT * N + 5 + N] = (y - yprev) - tight(N)
        d[F_COUNT * N + 5 + N:] = (y - yprev) + tight(N)
        r[F_HF, :N - 1], r[F_HB, :N - 1] = p + tight(N - 1), p - tight(N - 1)
        if rng.random() < 0.3:
            d[F_COUNT * N + 3] = p.min() + rng.normal()
        if rng.random() < 0.3:
            d[F_COUNT * N + 4] = p.max() + rng.normal()
        sat = int(rng.integers(0, 1 << (2 * (N - 1)))) if rng.random() < 0.5 else 0
        nrows = 6 * N + 4 * (N - 1)
        active = set(rng.choice(nrows, size=int(rng.integers(0, min(N, 4) + 1)), replace=False).tolist())
        rid = _same(N, y, active, sat, d)
        assert (rid & (REV - 1)) not in active
        if rid >= 0:
            won.add(_family(N, rid))
            ids.add(rid & (REV - 1))
    assert won == {"V_lo", "V_hi", "U_lo", "U_hi", "A_lo", "A_hi", "P_lo", "P_hi", "SF", "SB", "SF_rev", "SB_rev"}
    assert len(ids) >= (6 * N + 4 * (N - 1)) // 2


@pytest.mark.parametrize("N", HORIZONS)
def test_all_rows_satisfied(N):
    d = _loose(N)
    y = np.full(N, 20.0)
    assert _same(N, y, data=d) == -1
    # on a bound, and inside it by less than the tolerance's width: no candidate either
    _set(d, N, F_VHI, N - 1, 20.0)
    assert _same(N, y, data=d) == -1
    _set(d, N, F_VHI, N - 1, 20.0 - 1e-10)  # 1e-11 * (1 + 20) = 2.1e-10 > 1e-10
    assert _same(N, y, data=d) == -1
    _set(d, N, F_VHI, N - 1, 20.0 - 1e-9)
    assert _same(N, y, data=d) == 6 * (N - 1) + 1


@pytest.mark.parametrize("N", HORIZONS)
def test_first_candidate_is_the_only_one(N):
    """One violated row and nothing else: it is chosen whatever its violation and norm are (the
    selection's first comparison is against the initial (0, 1) pair)."""
    y = np.full(N, 20.0)
    nrows = 6 * N + 4 * (N - 1)
    for eps in (1e-9, 1e-3, 1.0, 1e5):
        for rid in range(nrows):
            d = _loose(N)
            if rid < 6 * N:
                j, r = divmod(rid, 6)
                a = d[F_AM * N + j]
                val = (20.0, 20.0 - a * 20.0, 0.0)[r // 2]
                bound = val + (eps if r % 2 == 0 else -eps) * (1.0 + abs(val))
                if r < 4:
                    _set(d, N, (F_VLO, F_VHI, F_ULO, F_UHI)[r], j, bound)
                else:
                    d[F_COUNT * N + 5 + (N if r == 5 else 0) + j] = bound
            else:
                m, r = divmod(rid - 6 * N, 4)
                p = 100.0 + 20.0 * (m + 1)
                big = min(eps * (1.0 + p), 10.0) if r < 2 else eps * (1.0 + p)  # (a step moves p by 20)
                if r == 0:
                    d[F_COUNT * N + 3] = p + big
                elif r == 1:
                    d[F_COUNT * N + 4] = p - big
                else:
                    _set(d, N, F_HF if r == 2 else F_HB, m, p - big if r == 2 else p + big)
                if (r == 0 and m > 0) or (r == 1 and m + 1 < N - 1):
                    continue  # (positions grow: pmin binds the earlier steps too, pmax the later ones)
            assert _same(N, y, data=d) == rid, (eps, rid)


@pytest.mark.parametrize("N", HORIZONS)
def test_equal_violations_the_first_wins(N):
    y = np.full(N, 20.0)
    d = _loose(N)
    # V_hi of the first and of the last step, the same violation and norm
    _set(d, N, F_VHI, 0, 19.0)
    _set(d, N, F_VHI, N - 1, 19.0)
    assert _same(N, y, data=d) == 1
    # against A_hi of step 1 (norm 1: it carries the constant v0): slack 0 - acc = -1 as well
    d[F_COUNT * N + 5 + N] = -1.0
    assert _same(N, y, data=d) == 1
    _set(d, N, F_VHI, 0, BIG)
    assert _same(N, y, data=d) == 5
    # the violation is relative to the norm: A_hi of the last step has |c|^2 = 2
    d = _loose(N)
    d[F_COUNT * N + 5 + N + (N - 1)] = -4.0        # A_hi, last step: slack -4 -> 16 / 2 = 8
    _set(d, N, F_VLO, 0, 22.0)                     # V_lo, step 1: slack -2 -> 4 / 1: smaller
    assert _same(N, y, data=d) == 6 * (N - 1) + 5
    d[F_COUNT * N + 5 + N + (N - 1)] = -2.0        # 4 / 2 = 2 < 4
    assert _same(N, y, data=d) == 0
    # equal across norms, 16 / 4 against 4 / 1: the one looked at first, which for a prefix row
    # of step 2 against the last step's V_lo is the prefix row unless step 2 is the last step
    d = _loose(N)
    d[F_COUNT * N + 2] = 2.0                       # ts = 2: the prefix rows of step 2 have |c|^2 = 4
    _set(d, N, F_HF, 0, 100.0 + 2.0 * 20.0 - 4.0)  # SF, step 2: slack -4
    _set(d, N, F_VLO, N - 1, 22.0)                 # V_lo, last step: slack -2
    assert _same(N, y, data=d) == (6 * (N - 1) if N == 2 else 6 * N + 2)


@pytest.mark.parametrize("N", HORIZONS)
def test_both_rows_of_a_pair_violated(N):
    """A node whose interval is empty (vlo > vhi): both rows are candidates."""
    y = np.full(N, 20.0)
    j = N // 2
    d = _loose(N)
    _set(d, N, F_VLO, j, 23.0)
    _set(d, N, F_VHI, j, 18.0)
    assert _same(N, y, data=d) == 6 * j      # |20 - 23| > |18 - 20|
    _set(d, N, F_VLO, j, 21.0)
    assert _same(N, y, data=d) == 6 * j + 1
    _set(d, N, F_VLO, j, 22.0)
    assert _same(N, y, data=d) == 6 * j      # equal: the lower row is looked at first
    assert _same(N, y, active={6 * j}, data=d) == 6 * j + 1


@pytest.mark.parametrize("N", HORIZONS)
def test_active_rows_are_skipped(N):
    y = np.full(N, 20.0)
    d = _loose(N)
    _set(d, N, F_VHI, 0, 10.0)
    _set(d, N, F_ULO, N - 1, 20.0 - d[F_AM * N + N - 1] * 20.0 + 5.0)
    _set(d, N, F_HB, N - 2, 100.0 + 20.0 * (N - 1) + 1.0)
    a, b, c = 1, 6 * (N - 1) + 2, 6 * N + 4 * (N - 2) + 3
    assert _same(N, y, data=d) == a
    assert _same(N, y, active={a}, data=d) == b
    assert _same(N, y, active={a, b}, data=d) == c
    assert _same(N, y, active={a, b, c}, data=d) == -1
    assert _same(N, y, active={b}, data=d) == a


@pytest.mark.parametrize("N", HORIZONS)
def test_saturated_soft_rows_stand_reversed(N):
    y = np.full(N, 20.0)
    m = N - 2
    p = 100.0 + 20.0 * (m + 1)
    for r, fld, bit in ((2, F_HF, 2 * m), (3, F_HB, 2 * m + 1)):
        rid = 6 * N + 4 * m + r
        sgn = 1.0 if r == 2 else -1.0  # SF: p <= hf ; SB: p >= hb
        d = _loose(N)
        _set(d, N, fld, m, p - sgn * 3.0)           # violated by 3
        assert _same(N, y, data=d) == rid
        assert _same(N, y, sat=1 << bit, data=d) == -1          # saturated and still violated: no row
        _set(d, N, fld, m, p + sgn * 3.0)           # strictly satisfied by 3
        assert _same(N, y, data=d) == -1
        got, dd, _, _ = _scan(N, y, sat=1 << bit, data=d)
        assert got == rid | REV
        assert dd == (100.0 - (p + 3.0) if r == 2 else (p - 3.0) - 100.0)  # the reversed row's bound
        assert _same(N, y, sat=1 << bit, data=d) == rid | REV
        assert _same(N, y, active={rid}, sat=1 << bit, data=d) == -1
        _set(d, N, fld, m, p)                        # on the bound: neither copy
        assert _same(N, y, data=d) == -1 and _same(N, y, sat=1 << bit, data=d) == -1


@pytest.mark.parametrize("N", [2, 5])
def test_host_build_solves_against_the_oracle(N):
    """The host build shares the header, so the independent check of the whole active-set method
    is the oracle: the local MIQPs of two platoon states (tests/instances.py), status, sequence,
    cost 1e-9 relative, u 1e-6 (the bars of the parity tests)."""
    import oracle as O
    from hvp import _abi, tables
    from hvp.models import PwaGearVehicle
    from instances import decent_instances, leader_window, oracle_solve

    veh = PwaGearVehicle(800.0)
    table = tables.system_from_dict(veh.get_discrete_system(1), tables.gears_of(veh))
    P, R = zip(*(decent_instances(O.env_initial_state(4, seed), N, leader_window(N)) for seed in (0, 3)))
    params, roles = np.ascontiguousarray(np.concatenate(P)), np.ascontiguousarray(np.concatenate(R).astype(np.int32))
    B = len(roles)
    ref = oracle_solve(O.gear_pwa_system(800.0), O.Cfg(), N, params, roles)
    L = ctypes.CDLL(_abi.HOSTREF_PATH)
    S = (_abi.HvpSystem * 1)(table)
    f = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for method in (1, 2):  # enumeration, branch and bound
        prob = tables.problem(N)
        prob.method = method
        out = dict(u=np.zeros((B, N)), x=np.zeros((B, 2, N + 1)), region=np.zeros((B, N), np.int8), cost=np.zeros(B),
                   status=np.zeros(B, np.int32), nodes=np.zeros(B, np.int32), iters=np.zeros(B, np.int32))
        rc = L.hvp_hostref_solve_batch(ctypes.byref(prob), S, B, f(np.zeros(B, np.int32)), f(roles), f(params),
                                       f(out["u"]), f(out["x"]), f(out["region"]), f(out["cost"]), f(out["status"]),
                                       f(out["nodes"]), f(out["iters"]), 4)
        assert rc == 0
        assert out["iters"].sum() >= B  # the active-set method ran (steps: scans that chose a row)
        for i, r in enumerate(ref):
            assert int(out["status"][i]) == 0
            assert out["region"][i].tolist() == r.sigma.tolist(), (method, i)
            assert abs(out["cost"][i] - r.cost) <= 1e-9 * max(1.0, abs(r.cost)), (method, i)
            assert np.abs(out["u"][i] - r.u).max() <= 1e-6, (method, i)


# ---------------------------------------------------------------- GPU cases

BATCHES = (1, 37, 300)


@functools.lru_cache(maxsize=None)
def _gpu_inputs(N):
    from test_refill_cost_row import _inputs

    params, roles = _inputs(N)
    B = max(BATCHES)
    params, roles = np.ascontiguousarray(params[:B]), np.ascontiguousarray(roles[:B])
    assert len(set(roles[:37].tolist())) == 3  # leaders, middles and trailers within the partial wave
    return params, roles


def _gpu_tables(count):
    from test_refill_tables import _gear_pwa, _systems

    return (_gear_pwa(800.0),) if count == 1 else _systems(count)


@functools.lru_cache(maxsize=None)
def _gpu_hostref(N, count, B):
    """The host build's answers for the first B instances (computed once per case and shared)."""
    from hvp import _abi, tables

    L = ctypes.CDLL(_abi.HOSTREF_PATH)
    params, roles = _gpu_inputs(N)
    params, roles = params[:B], roles[:B]
    systems = _gpu_tables(count)
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


def _gpu_case(N, count, B):
    from hvp import tables
    from hvp.solver import BatchSolver
    from test_refill_tables import _check_against_hostref

    params, roles = _gpu_inputs(N)
    sys_idx = (np.arange(len(roles)) % count).astype(np.int32)
    s = BatchSolver(tables.problem(N), list(_gpu_tables(count)))
    try:
        res = s.solve(sys_idx[:B], roles[:B], params[:B])
    finally:
        s.close()
    full = _gpu_hostref(N, count, max(BATCHES) if N <= 8 else B)
    _check_against_hostref(res, {k: v[:B] for k, v in full.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("count", [1, 9])
@pytest.mark.parametrize("N", HORIZONS)
def test_gpu_against_host_build(gpu_available, N, count, B):
    _gpu_case(N, count, B)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 37])
def test_gpu_against_host_build_long_horizon(gpu_available, B):
    _gpu_case(10, 1, B)
