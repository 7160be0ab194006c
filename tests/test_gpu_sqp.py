"""GPU suite: the full SQP solve (include/cfnmpc.h: cfnmpc_solve_sqp / cfnmpc_fleet_solve_sqp).

The restatement's SQP is built here from the CPU restatement (oracle/cfnmpc_ref.c): cref.rti_step in a loop with x0 fixed,
res_step from the iterates, res_eq from cref.rk4_sens's Phi, res_ineq from the box, and the stop rule of the header.  The
converged point is the first output of the engine that does not depend on the QP route a row took, so the comparisons here
are tight whatever route (active set, dense head, interior point) each side used."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HOV = 15.777730167256925
TOL = 1e-9        # SQP tolerances of the parity tests
QP_TOL = 1e-11


def _inputs(oracle, B, N, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    x0 = oracle.sample_hover_x0(rng, B, scale=scale)
    yr, ye = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    return x0, np.repeat(yr[None], B, 0).copy(), np.repeat(ye[None], B, 0).copy()


def _start(x0, N, init):
    B = x0.shape[0]
    if init == "hover":
        return np.repeat(x0[:, None, :], N + 1, 1).copy(), np.full((B, N, 4), HOV)
    xr = np.zeros((B, N + 1, 13)); xr[:, :, 3] = 1.0
    return xr, np.zeros((B, N, 4))


def _residuals(cref, xo, uo, xn, un, x0, dt, u_min=0.0, u_max=22.0):
    """(res_step, res_eq, res_ineq) of one instance at w_j = (xn, un) after the step from (xo, uo)"""
    step = max(np.abs(xn - xo).max(), np.abs(un - uo).max())
    eq = np.abs(xn[0] - x0).max()
    for k in range(un.shape[0]):
        eq = max(eq, np.abs(xn[k + 1] - cref.rk4_sens(xn[k], un[k], dt)[0]).max())
    ineq = max(0.0, (u_min - un).max(), (un - u_max).max())
    return step, eq, ineq


def ref_sqp(cref, copts, x0, yref, yref_e, xr, ur, max_iter, tol):
    """The restatement's SQP (in place on xr, ur) -> status, sqp_iter, res [B][3], iterations run"""
    B = x0.shape[0]
    status = np.full(B, 2, dtype=np.int32); it = np.zeros(B, dtype=np.int32); res = np.zeros((B, 3))
    done = np.zeros(B, dtype=bool)
    ran = 0
    for j in range(1, max_iter + 1):
        idx = np.flatnonzero(~done)
        if idx.size == 0:
            break
        ran = j
        xa, ua = xr[idx].copy(), ur[idx].copy()
        sq, _, _, _ = cref.rti_step(copts, xa, ua, x0[idx].copy(), yref[idx].copy(), yref_e[idx].copy(), nthreads=0)
        for r, i in enumerate(idx):
            res[i] = _residuals(cref, xr[i], ur[i], xa[r], ua[r], x0[i], copts.dt, copts.u_min, copts.u_max)
            it[i] = j
            if sq[r] == 4:
                status[i], done[i] = 4, True
            elif res[i, 0] <= tol and res[i, 1] <= tol and res[i, 2] <= tol:
                status[i], done[i] = 0, True
            else:
                status[i] = 2
        xr[idx], ur[idx] = xa, ua
    return status, it, res, ran


def _gpu_sqp(B, x0, yref, yref_e, init, max_iter=100, sqp_tol=TOL, **kw):
    """a solver with options **kw (tol = the QP tolerance), one solve_sqp at sqp_tol"""
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    from crazyflie_nmpc_amd.solver import INIT_ACADOS, INIT_HOVER
    s = BatchSolver(B, default_opts(**kw))
    s.set_x0(x0); s.set_yref(yref, yref_e); s.init_iterate(INIT_HOVER if init == "hover" else INIT_ACADOS)
    n = s.solve_sqp(max_iter, sqp_tol, sqp_tol, sqp_tol)
    st, it, rs = s.sqp_stats()
    x, u = s.get_iterate()
    return s, n, st, it, rs, x, u


@pytest.mark.parametrize("init", ["acados", "hover"])
def test_sqp_matches_restatement_on_hover(oracle, cref, init):
    B, N = 192, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=21)
    s, n, st, it, rs, xg, ug = _gpu_sqp(B, x0, yref, yref_e, init, tol=QP_TOL)
    xr, ur = _start(x0, N, init)
    st_r, it_r, rs_r, n_r = ref_sqp(cref, cref.default_opts(tol=QP_TOL), x0, yref, yref_e, xr, ur, 100, TOL)
    # full steps without globalisation (acados' SQP takes them too): most rows converge, the rest are still moving (or
    # oscillating) after 100 iterations on both sides -- status 2, sqp_iter = max_iter
    conv = st_r == 0
    assert conv.sum() >= B // 2, np.unique(st_r, return_counts=True)
    assert set(np.unique(st_r)) <= {0, 2}
    assert np.array_equal(st, st_r), (np.flatnonzero(st != st_r), st[st != st_r], st_r[st != st_r])
    assert np.array_equal(it, it_r), (np.flatnonzero(it != it_r), it[it != it_r], it_r[it != it_r], rs[it != it_r], rs_r[it != it_r])
    assert n == n_r == it.max()
    # both sides stop at the same iteration, each within ~tol_step / (1 - rate) of the NLP point; the first steps are of size 16
    # (kRPM) from either start and carry the two sides' rounding differences up to 1e-6 before the linear contraction: 1.5e-8
    # measured on the inputs of the slowest converged rows
    assert np.abs(xg[conv] - xr[conv]).max() < 1e-7 and np.abs(ug[conv] - ur[conv]).max() < 1e-7
    assert (rs[conv] <= TOL).all(), rs[conv].max(0)
    assert np.abs(rs[conv] - rs_r[conv]).max() < 1e-8
    assert (it[~conv] == 100).all() and (rs[~conv].max(1) > TOL).all()


def test_sqp_converged_point_against_independent_referee(oracle):
    """At 16 converged rows the QP built at the GPU's final iterate (numpy oracle, sympy Jacobians) is solved exactly in
    extended precision: its step must be within 10 tol_step, its defects b_k within tol_eq."""
    B, N = 64, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=22, scale=1.0)
    s, n, st, it, rs, xg, ug = _gpu_sqp(B, x0, yref, yref_e, "hover", tol=QP_TOL)
    conv = np.flatnonzero(st == 0)
    assert conv.size >= 16
    for i in np.random.default_rng(0).choice(conv, 16, replace=False):
        qp = oracle.build_qp(xg[i], ug[i], x0[i], yref[i], yref_e[i])
        sol = oracle.solve_qp_refined(qp)
        step = max(np.abs(sol["dx"]).max(), np.abs(sol["du"]).max())
        assert step <= 10 * TOL, (i, step)
        assert max(np.abs(qp.b).max(), np.abs(qp.dx0).max()) <= TOL, i


def test_sqp_constrained_rows_route_independent(oracle):
    """scale 3: inputs on the box at the NLP solution.  The active-set route and the interior point alone reach the same
    point on every row that converged in both runs."""
    B, N = 128, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=23, scale=3.0)
    _s, _n, st_a, _it, rs_a, xa, ua = _gpu_sqp(B, x0, yref, yref_e, "hover", tol=QP_TOL)
    _s2, _n2, st_i, _it2, rs_i, xi, ui = _gpu_sqp(B, x0, yref, yref_e, "hover", tol=QP_TOL, active_set=0)
    both = (st_a == 0) & (st_i == 0)
    assert both.sum() >= 8, (np.unique(st_a, return_counts=True), np.unique(st_i, return_counts=True))
    on_box = (ua[both] <= 1e-9) | (ua[both] >= 22.0 - 1e-9)
    assert on_box.any(), "no input on the box at the solution: the test does not cover the constrained route"
    assert np.abs(xa[both] - xi[both]).max() < 1e-8 and np.abs(ua[both] - ui[both]).max() < 1e-8
    assert (rs_a[st_a == 0] <= TOL).all() and (rs_i[st_i == 0] <= TOL).all()


def test_sqp_frozen_rows_keep_their_iterate(oracle):
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B, N = 64, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=24, scale=1.0)
    s, n, st, it, rs, xg, ug = _gpu_sqp(B, x0, yref, yref_e, "hover", tol=QP_TOL)
    early = np.flatnonzero((st == 0) & (it < n))
    assert early.size > 0, (n, it)
    for j in sorted(set(it[early].tolist()))[:3]:
        s2 = BatchSolver(B, default_opts(tol=QP_TOL))
        s2.set_x0(x0); s2.set_yref(yref, yref_e); s2.init_iterate(INIT_HOVER)
        s2.solve(j)
        x2, u2 = s2.get_iterate()
        rows = early[it[early] == j]
        assert np.abs(xg[rows] - x2[rows]).max() <= 1e-12 and np.abs(ug[rows] - u2[rows]).max() <= 1e-12, j
    # max_iter = 1: exactly one RTI step, bitwise
    s1, n1, st1, it1, _r, x1, u1 = _gpu_sqp(B, x0, yref, yref_e, "hover", max_iter=1)
    s3 = BatchSolver(B)
    s3.set_x0(x0); s3.set_yref(yref, yref_e); s3.init_iterate(INIT_HOVER); s3.solve(1)
    x3, u3 = s3.get_iterate()
    assert n1 == 1 and (it1 == 1).all() and set(np.unique(st1)) <= {0, 2}
    assert np.array_equal(x1, x3) and np.array_equal(u1, u3)


def test_sqp_nan_row_stops_with_status_4(oracle):
    from crazyflie_nmpc_amd import BatchSolver
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B, N = 8, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=25)
    x0b = x0.copy(); x0b[5, 2] = np.nan
    s = BatchSolver(B)
    s.set_x0(x0b); s.set_yref(yref, yref_e); s.init_iterate(INIT_HOVER)
    xi, ui = s.get_iterate()
    n = s.solve_sqp()
    st, it, rs = s.sqp_stats()
    xo, uo = s.get_iterate()
    assert st[5] == 4 and it[5] == 1
    assert np.array_equal(np.isnan(xo[5]), np.isnan(xi[5])) and np.array_equal(uo[5], ui[5])
    assert np.array_equal(xo[5][~np.isnan(xo[5])], xi[5][~np.isnan(xi[5])])
    s2 = BatchSolver(B)
    s2.set_x0(x0); s2.set_yref(yref, yref_e); s2.init_iterate(INIT_HOVER)
    n2 = s2.solve_sqp()
    st2, it2, rs2 = s2.sqp_stats()
    x2, u2 = s2.get_iterate()
    ok = np.arange(B) != 5
    assert (st[ok] == 0).any() and np.array_equal(st[ok], st2[ok]) and np.array_equal(it[ok], it2[ok])
    assert np.array_equal(xo[ok], x2[ok]) and np.array_equal(uo[ok], u2[ok])
    assert np.array_equal(rs[ok], rs2[ok])


@pytest.mark.parametrize("variant", ["step_graph", "start_solve2", "box_stages", "cond_N2"])
def test_sqp_options_do_not_change_the_answer(oracle, variant):
    B, N = 64, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=26, scale=1.0)
    _s, _n, st, _it, _rs, xg, ug = _gpu_sqp(B, x0, yref, yref_e, "hover", tol=QP_TOL)
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    kw = {"step_graph": dict(step_graph=1), "start_solve2": dict(start_solve=2), "box_stages": {},
          "cond_N2": dict(cond_N2=10)}[variant]
    s = BatchSolver(B, default_opts(tol=QP_TOL, **kw))
    if variant == "box_stages":
        s.set_box_stages(np.zeros((B, N, 4)), np.full((B, N, 4), 22.0))
    s.set_x0(x0); s.set_yref(yref, yref_e); s.init_iterate(INIT_HOVER)
    s.solve_sqp(100, TOL, TOL, TOL)
    st2, _it2, rs2 = s.sqp_stats()
    x2, u2 = s.get_iterate()
    both = (st == 0) & (st2 == 0)
    assert both.sum() >= B // 4 and ((st == 0) == (st2 == 0)).mean() >= 0.9, (np.unique(st, return_counts=True), np.unique(st2, return_counts=True))
    assert np.abs(xg[both] - x2[both]).max() < 1e-8 and np.abs(ug[both] - u2[both]).max() < 1e-8
    assert (rs2[st2 == 0] <= TOL).all()


def test_fleet_sqp_mixed_horizons(oracle, cref):
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    horizons = np.array([30, 50, 100] * 16)[np.random.default_rng(27).permutation(48)]
    B, Nmax = horizons.size, 100
    x0, yref, yref_e = _inputs(oracle, B, Nmax, seed=27, scale=1.0)
    f = MixedHorizonFleet(horizons, tol=QP_TOL)
    f.set_x0(x0); f.set_yref(yref, yref_e); f.init_iterate(INIT_HOVER)
    n = f.solve_sqp(100, TOL, TOL, TOL)
    st, it, rs = f.sqp_stats()
    assert (st == 0).sum() >= B // 2 and n == it.max()
    for N, idx, xb, ub in f.bucket_iterates():
        xr, ur = _start(x0[idx], N, "hover")
        st_r, it_r, rs_r, _n = ref_sqp(cref, cref.default_opts(N=N, tol=QP_TOL), x0[idx].copy(), yref[idx, :N].copy(),
                                       yref_e[idx].copy(), xr, ur, 100, TOL)
        assert np.array_equal(st[idx], st_r) and np.array_equal(it[idx], it_r), N     # stats in fleet order
        c = st_r == 0
        assert np.abs(xb[c] - xr[c]).max() < 1e-8 and np.abs(ub[c] - ur[c]).max() < 1e-8, N
        assert np.abs(rs[idx][c] - rs_r[c]).max() < 1e-8, N


def test_sqp_argument_checks():
    from crazyflie_nmpc_amd import BatchSolver, _lib
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    L = _lib.lib()
    s = BatchSolver(4)
    f = MixedHorizonFleet([30, 50, 50, 100])
    n = C.c_int(-7)
    bad = [(0, 1e-6, 1e-6, 1e-6), (-3, 1e-6, 1e-6, 1e-6)]
    for pos in range(3):
        for v in (0.0, -1e-6, float("inf"), float("nan")):
            t = [1e-6, 1e-6, 1e-6]; t[pos] = v
            bad.append((10, *t))
    for args in bad:
        assert L.cfnmpc_solve_sqp(s._h, *args, C.byref(n), None) == -1, args
        assert L.cfnmpc_fleet_solve_sqp(f._h, *args, C.byref(n), None) == -1, args
    assert n.value == -7                                                # nothing written on a refusal
    assert L.cfnmpc_solve_sqp(None, 10, 1e-6, 1e-6, 1e-6, None, None) == -1
    assert L.cfnmpc_get_sqp_stats(None, None, None, None, 0, None) == -1
    assert L.cfnmpc_fleet_solve_sqp(None, 10, 1e-6, 1e-6, 1e-6, None, None) == -1
    assert L.cfnmpc_fleet_get_sqp_stats(None, None, None, None, 0, None) == -1
    assert L.cfnmpc_solve_sqp(s._h, 3, 1e-6, 1e-6, 1e-6, None, None) == 0   # n_iter may be NULL
