"""GPU suite: merit-function backtracking line search of the full SQP solve (include/cfnmpc.h: cfnmpc_set_sqp_globalization;
DESIGN.md section 5.17).

The reference is ls_ref / sqp_ls_ref of tests/test_sqp_ls_cpu.py, the algorithm of the header restated in numpy.  One iteration
is compared on the GPU's own data: w_{j-1} and mu from a globalised solve of j - 1 iterations, the candidate w^ from a full-step
solver set to w_{j-1} that takes one RTI step, w_j from a fresh globalised solve of j iterations.  Tolerances: 1e-9 max(1, |.|)
for iterates and residuals (the bound of the stored blocks, as in test_gpu_nlp_eval.py), step lengths exactly -- except on rows
whose test was decided by less than 1e-9 of the magnitude of its terms in the reference (ties: at most 5 % of the rows).  Every
comparison prints the figures it saw."""
import ctypes as C

import numpy as np
import pytest

from test_model_params_cpu import random_params
from test_sqp_ls_cpu import ALPHA_MIN, FIX, GOLDEN, fixture_inputs, ls_ref, make_data, n_trials, ties

pytestmark = pytest.mark.gpu
DT = 0.015
TOL = 1e-9        # SQP tolerances of the parity tests: no row converges within three iterations from these starts
QP_TOL = 1e-11
EINVAL = -1


def _inputs(oracle, B, N, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    x0 = oracle.sample_hover_x0(rng, B, scale=scale)
    yr, ye = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    return x0, np.repeat(yr[None], B, 0).copy(), np.repeat(ye[None], B, 0).copy()


def _maker(x0, yref, yref_e, configure=None, **kw):
    """-> make(globalised): a solver with the inputs, the options **kw and configure(solver) applied, at the hover start"""
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B = x0.shape[0]

    def make(globalised):
        s = BatchSolver(B, default_opts(**kw))
        if configure is not None:
            configure(s)
        s.set_x0(x0); s.set_yref(yref, yref_e); s.init_iterate(INIT_HOVER)
        if globalised:
            s.set_sqp_globalization("merit_backtracking")
        return s
    return make


def _one_iteration(make, data, j, prev, step_solver, what):
    """iteration j of a globalised solve against ls_ref.  prev = (w_{j-1}, mu_{j-1}, open rows) of the solve of j - 1 iterations (or
    the start); -> the same of the solve of j iterations, and the number of rows with alpha < 1"""
    (xw, uw), mu0, open_rows = prev
    B = xw.shape[0]
    step_solver.set_iterate(xw, uw)
    step_solver.solve(1)
    xh, uh = step_solver.get_iterate()
    failed = step_solver.stats()[0] == 4
    s = make(True)
    n = s.solve_sqp(j, TOL, TOL, TOL)
    st, it, rs = s.sqp_stats()
    al, mu, n_short, n_fail = s.sqp_ls_stats()
    xj, uj = s.get_iterate()
    al_r, mu_r, (xr, ur), rs_r, acc_r, mg = ls_ref((xw, uw), (xh, uh), mu0, data, failed=failed)
    rows = np.flatnonzero(open_rows)
    assert n == j and rows.size > 0 and (it[rows] == j).all(), (n, it)
    tie = ties(mg)[rows]
    diff = al[rows] != al_r[rows]
    print(f"{what}, iteration {j}: B {B}  rows {rows.size}  alpha < 1: {int((al_r[rows] < 1).sum())} (reference) "
          f"{int((al[rows] < 1).sum())} (GPU)  ties {int(tie.sum())}  alpha differs on {int(diff.sum())}  "
          f"no trial accepted: {int((~acc_r[rows]).sum())}")
    assert tie.sum() <= 0.05 * rows.size, tie.sum()
    assert not (diff & ~tie).any(), (rows[diff & ~tie], al[rows][diff & ~tie], al_r[rows][diff & ~tie])
    same = rows[~diff]
    e_mu = (np.abs(mu[rows] - mu_r[rows]) / np.maximum(np.abs(mu_r[rows]), 1e-300)).max()
    e_x = np.abs(xj[same] - xr[same]).max() / max(1.0, np.abs(xr[same]).max())
    e_u = np.abs(uj[same] - ur[same]).max() / max(1.0, np.abs(ur[same]).max())
    e_rs = np.abs(rs[same] - rs_r[same]).max(0)
    print(f"  mu rel {e_mu:.2e} (|mu| {np.abs(mu_r[rows]).max():.2e})  x {e_x:.2e}  u {e_u:.2e}  res step / eq / ineq {e_rs} "
          f"(|res| {np.abs(rs_r[same]).max(0)})")
    assert e_mu <= 1e-9, e_mu
    assert e_x <= 1e-9 and e_u <= 1e-9, (e_x, e_u)
    assert (e_rs <= 1e-9 * np.maximum(1.0, np.abs(rs_r[same]).max(0))).all(), e_rs
    step = np.maximum(np.abs(xh - xw).reshape(B, -1).max(1), np.abs(uh - uw).reshape(B, -1).max(1))
    assert np.abs(rs[same, 0] - step[same]).max() <= 1e-9 * max(1.0, step[same].max())    # the FULL step, whatever alpha
    # rows with alpha = 1 keep the step's candidate; the counters follow alpha
    full = same[al[same] == 1.0]
    assert np.abs(xj[full] - xh[full]).max(initial=0.0) <= 1e-9 and np.abs(uj[full] - uh[full]).max(initial=0.0) <= 1e-9
    assert ((al[rows] < 1.0) <= (n_short[rows] >= 1)).all() and (n_fail[rows] <= n_short[rows]).all()
    return ((xj, uj), mu, open_rows & (st == 2)), int((al[rows] < 1).sum())


def _start_of(make):
    s = make(False)
    x, u = s.get_iterate()
    return s, ((x, u), np.zeros(x.shape[0]), np.ones(x.shape[0], dtype=bool))


# ---- 1. the default is untouched ----------------------------------------------------------------------------------------------
def test_full_step_mode_and_rti_path_are_untouched(oracle):
    B, N = 65, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=61, scale=1.0)
    make = _maker(x0, yref, yref_e, tol=QP_TOL)
    a, b = make(False), make(False)
    b.set_sqp_globalization("full_step")
    assert a.sqp_globalization() == b.sqp_globalization() == ("full_step", 1e-4, 0.5, 2.0 ** -10)
    na, nb = a.solve_sqp(100, 1e-6, 1e-6, 1e-6), b.solve_sqp(100, 1e-6, 1e-6, 1e-6)
    assert na == nb
    for p, q in zip(a.sqp_stats() + a.get_iterate(), b.sqp_stats() + b.get_iterate()):
        assert np.array_equal(p, q)
    for s in (a, b):
        al, mu, ns, nf = s.sqp_ls_stats()
        assert (al == 1.0).all() and (mu == 0.0).all() and (ns == 0).all() and (nf == 0).all()
    # the RTI path ignores the setting
    c, d = make(True), make(False)
    assert c.sqp_globalization() == ("merit_backtracking", 1e-4, 0.5, 2.0 ** -10)
    c.solve(3); d.solve(3)
    for p, q in zip(c.get_iterate() + c.stats(), d.get_iterate() + d.stats()):
        assert np.array_equal(p, q)


# ---- 2. one iteration against the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [64, 1, 63, 65, 130])
def test_one_iteration_parity(oracle, B):
    N = 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=31, scale=3.0)
    make = _maker(x0, yref, yref_e, tol=QP_TOL)
    data = make_data(x0, yref, yref_e, oracle.Q_DIAG, oracle.R_DIAG, oracle.QN_DIAG, 0.0, 22.0, DT)
    stepper, prev = _start_of(make)
    for j in (1, 2, 3):
        prev, n_short = _one_iteration(make, data, j, prev, stepper, "hover start, scale 3")
    if B >= 63:
        assert n_short > 0, "no row with alpha < 1 in iteration 3: the test shows nothing"


# ---- 3. the outcome on the hard starts --------------------------------------------------------------------------------------------
def test_outcome_on_the_hard_starts(oracle):
    z = np.load(GOLDEN)
    x0, yref, yref_e, _xs, _us = fixture_inputs(oracle)
    make = _maker(x0, yref, yref_e, tol=FIX["qp_tol"])
    tol, cap = FIX["tol"], FIX["max_iter"]
    out = {}
    for glob in (False, True):
        s = make(glob)
        n = s.solve_sqp(cap, tol, tol, tol)
        st, it, rs = s.sqp_stats()
        s.eval_nlp()
        out[glob] = (st, it, rs, s.nlp_stats()[0], s.sqp_ls_stats(), n)
    st_f, st_g = out[False][0], out[True][0]
    it_g, rs_g, (al, mu, n_short, n_fail) = out[True][1], out[True][2], out[True][4]
    late = int(((z["status_ls"] == 0) & (z["sqp_iter_ls"] > cap - 15)).sum())
    want = int((z["status_ls"] == 0).sum()) - (1 + late)
    print(f"converged: full steps {int((st_f == 0).sum())} (fixture {int((z['status_full'] == 0).sum())}), line search "
          f"{int((st_g == 0).sum())} (fixture {int((z['status_ls'] == 0).sum())}, {late} of them in the last 15 iterations: at least "
          f"{want} wanted); iterations {out[False][5]} / {out[True][5]}")
    print(f"  n_short {n_short.tolist()}\n  n_fail {n_fail.tolist()}\n  alpha {al.tolist()}\n  sqp_iter {it_g.tolist()}")
    assert np.array_equal(st_f, z["status_full"]), (st_f, z["status_full"])
    assert (st_g == 0).sum() >= want, ((st_g == 0).sum(), want)
    assert (st_g[st_f == 0] == 0).all(), np.flatnonzero((st_f == 0) & (st_g != 0))
    both = (st_f == 0) & (st_g == 0)
    rel = np.abs(out[False][3][both] - out[True][3][both]) / np.abs(out[False][3][both])
    print(f"  cost of the rows converged both ways: relative difference {rel.max(initial=0.0):.2e}")
    assert (rel <= 1e-8).all(), rel
    assert (n_short >= 0).all() and (n_short <= it_g).all() and (n_fail <= n_short).all()
    assert ((al < 1.0) <= (n_short >= 1)).all() and (al[n_short == 0] == 1.0).all()
    assert (al <= 1.0).all() and (al >= ALPHA_MIN).all() and (np.log2(al) == np.round(np.log2(al))).all()
    assert (rs_g[st_g == 0] <= tol).all(), rs_g[st_g == 0].max(0)
    assert (mu >= 0).all() and np.isfinite(mu).all()


# ---- 4. the data in force ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["model_params", "weight_rows_scaled", "erk_steps_2", "stage_boxes", "start_solve_2", "cond_N2_10"])
def test_data_in_force(oracle, variant):
    B, N, j = 8, 20, 2
    x0, yref, yref_e = _inputs(oracle, B, N, seed=71, scale=3.0)
    rng = np.random.default_rng(72)
    kw, conf = dict(N=N, tol=QP_TOL), None
    d = dict(Qd=oracle.Q_DIAG, Rd=oracle.R_DIAG, QNd=oracle.QN_DIAG, lb=0.0, ub=22.0, erk_steps=1, params=None)
    if variant == "model_params":
        p = random_params(rng, B)
        conf = lambda s: s.set_model_params(p)
        d["params"] = p
    elif variant == "weight_rows_scaled":
        W = np.tile(oracle.W_DIAG, (B, 1)) * rng.uniform(0.5, 2.0, (B, 17))
        WN = np.tile(oracle.QN_DIAG, (B, 1)) * rng.uniform(0.5, 2.0, (B, 13))
        conf = lambda s: (s.set_weights_batch(W, WN), s.set_cost_scaling(DT, 1.0))
        d.update(Qd=DT * W[:, :13], Rd=DT * W[:, 13:], QNd=WN)
    elif variant == "erk_steps_2":
        conf = lambda s: s.set_erk_steps(2)
        d["erk_steps"] = 2
    elif variant == "stage_boxes":
        lb = rng.uniform(0.0, 6.0, (B, N, 4)); ub = rng.uniform(17.0, 22.0, (B, N, 4))
        lb[:, 0] = ub[:, 0] = oracle.HOV_W + rng.uniform(-1.0, 1.0, (B, 4))          # stage 0 pinned
        conf = lambda s: s.set_box_stages(lb, ub)
        d.update(lb=lb, ub=ub)
    elif variant == "start_solve_2":
        kw["start_solve"] = 2
    else:
        kw["cond_N2"] = 10
    make = _maker(x0, yref, yref_e, conf, **kw)
    data = make_data(x0, yref, yref_e, d["Qd"], d["Rd"], d["QNd"], d["lb"], d["ub"], DT, d["erk_steps"], d["params"])
    stepper, start = _start_of(make)
    s1 = make(True)
    s1.solve_sqp(j - 1, TOL, TOL, TOL)
    prev = (s1.get_iterate(), s1.sqp_ls_stats()[1], s1.sqp_stats()[0] == 2)
    _one_iteration(make, data, j, prev, stepper, variant)


# ---- 5. frozen rows ------------------------------------------------------------------------------------------------------------------
def test_frozen_rows_keep_their_iterate(oracle):
    B, N = 64, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=24, scale=1.0)
    make = _maker(x0, yref, yref_e, tol=QP_TOL)
    s = make(True)
    n = s.solve_sqp(100, TOL, TOL, TOL)
    st, it, _rs = s.sqp_stats()
    xg, ug = s.get_iterate()
    early = np.flatnonzero((st == 0) & (it < n))
    assert early.size > 0, (n, it)
    for j in sorted(set(it[early].tolist()))[:3]:
        s2 = make(True)
        assert s2.solve_sqp(j, TOL, TOL, TOL) == j
        x2, u2 = s2.get_iterate()
        rows = early[it[early] == j]
        assert np.array_equal(xg[rows], x2[rows]) and np.array_equal(ug[rows], u2[rows]), j   # w_{sqp_iter}, bit for bit


# ---- 6. a NaN row ----------------------------------------------------------------------------------------------------------------------
def test_nan_row_stops_with_status_4(oracle):
    B, N = 8, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=25)
    x0b = x0.copy(); x0b[5, 2] = np.nan
    s = _maker(x0b, yref, yref_e)(True)
    xi, ui = s.get_iterate()
    s.solve_sqp()
    st, it, rs = s.sqp_stats()
    al, mu, ns, nf = s.sqp_ls_stats()
    xo, uo = s.get_iterate()
    assert st[5] == 4 and it[5] == 1 and al[5] == 1.0 and ns[5] == 0 and nf[5] == 0          # kept its iterate: no search
    assert np.array_equal(np.isnan(xo[5]), np.isnan(xi[5])) and np.array_equal(uo[5], ui[5])
    assert np.array_equal(xo[5][~np.isnan(xo[5])], xi[5][~np.isnan(xi[5])])
    s2 = _maker(x0, yref, yref_e)(True)
    s2.solve_sqp()
    st2, it2, rs2 = s2.sqp_stats()
    x2, u2 = s2.get_iterate()
    ok = np.arange(B) != 5
    assert (st[ok] == 0).any() and np.array_equal(st[ok], st2[ok]) and np.array_equal(it[ok], it2[ok])
    assert np.array_equal(xo[ok], x2[ok]) and np.array_equal(uo[ok], u2[ok]) and np.array_equal(rs[ok], rs2[ok])
    for p, q in zip(s.sqp_ls_stats(), s2.sqp_ls_stats()):
        assert np.array_equal(p[ok], q[ok])


# ---- 7. fleet ------------------------------------------------------------------------------------------------------------------------
def test_fleet_equals_its_buckets(oracle):
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    horizons = np.array([30, 50, 100] * 4)[np.random.default_rng(81).permutation(12)]
    B, Nmax = horizons.size, 100
    x0, yref, yref_e = _inputs(oracle, B, Nmax, seed=82, scale=3.0)
    f = MixedHorizonFleet(horizons, tol=QP_TOL)
    f.set_x0(x0); f.set_yref(yref, yref_e); f.init_iterate(INIT_HOVER)
    assert f.sqp_globalization()[0] == "full_step"
    f.set_sqp_globalization("merit_backtracking")
    assert f.sqp_globalization() == ("merit_backtracking", 1e-4, 0.5, 2.0 ** -10)
    n = f.solve_sqp(30, 1e-6, 1e-6, 1e-6)
    st, it, rs = f.sqp_stats()
    al, mu, ns, nf = f.sqp_ls_stats()
    print(f"fleet: iterations {n}  status {st.tolist()}  n_short {ns.tolist()}  n_fail {nf.tolist()}")
    assert n == it.max() and (ns > 0).any()
    for N, idx, xb, ub in f.bucket_iterates():
        s = BatchSolver(idx.size, default_opts(N=N, tol=QP_TOL))
        s.set_x0(x0[idx]); s.set_yref(yref[idx, :N].copy(), yref_e[idx]); s.init_iterate(INIT_HOVER)
        s.set_sqp_globalization("merit_backtracking")
        s.solve_sqp(30, 1e-6, 1e-6, 1e-6)
        for p, q in zip((st, it, rs) + (al, mu, ns, nf), s.sqp_stats() + s.sqp_ls_stats()):
            assert np.array_equal(p[idx], q), N                                              # stats in fleet order
        x, u = s.get_iterate()
        assert np.array_equal(xb, x) and np.array_equal(ub, u), N


# ---- 8. argument checks ----------------------------------------------------------------------------------------------------------------
def test_argument_checks(oracle):
    from crazyflie_nmpc_amd import BatchSolver, _lib
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    L = _lib.lib()
    B = 4
    s = BatchSolver(B)
    f = MixedHorizonFleet([30, 50, 50, 100])
    assert L.cfnmpc_set_sqp_globalization(s._h, 1, 0.01, 0.7, 0.01) == 0
    assert s.sqp_globalization() == ("merit_backtracking", 0.01, 0.7, 0.01)
    bad = [(2, 0, 0, 0), (-1, 0, 0, 0), (1, 0.5, 0, 0), (1, -1e-4, 0, 0), (1, float("nan"), 0, 0), (1, 0, 1.0, 0), (1, 0, -0.5, 0),
           (1, 0, float("inf"), 0), (1, 0, 0, 1.5), (1, 0, 0, -0.1), (1, 0, 0, float("nan")),
           (1, 0, 0.5, 2.0 ** -33),          # T = 33
           (1, 0, 0.9, 0.03)]                # 0.9^33 = 0.0309 > 0.03: T = 34
    for args in bad:
        assert L.cfnmpc_set_sqp_globalization(s._h, *args) == EINVAL, args
        assert L.cfnmpc_fleet_set_sqp_globalization(f._h, *args) == EINVAL, args
    assert s.sqp_globalization() == ("merit_backtracking", 0.01, 0.7, 0.01)                  # nothing changed
    assert L.cfnmpc_set_sqp_globalization(s._h, 1, 0.0, 0.5, 2.0 ** -32) == 0                # T = 32 is allowed
    assert n_trials(0.5, 2.0 ** -32) == 32
    assert L.cfnmpc_set_sqp_globalization(s._h, 1, 0.0, 0.0, 1.0) == 0                       # alpha_min = 1: T = 0
    s.set_sqp_globalization("merit_backtracking")
    # stats: not before a solve, not with every pointer NULL
    al = np.empty(B); ns = np.empty(B, dtype=np.int32)
    pa, pn = al.ctypes.data_as(C.c_void_p), ns.ctypes.data_as(C.c_void_p)
    assert L.cfnmpc_get_sqp_ls_stats(s._h, pa, None, None, None, 0, None) == EINVAL
    assert L.cfnmpc_fleet_get_sqp_ls_stats(f._h, pa, None, None, None, 0, None) == EINVAL
    assert L.cfnmpc_get_sqp_globalization(s._h, None, None, None, None) == EINVAL
    x0, yref, yref_e = _inputs(oracle, B, 50, seed=91)
    s.set_x0(x0); s.set_yref(yref, yref_e); s.init_iterate(INIT_HOVER)
    w0 = s.workspace_bytes
    s.solve_sqp(5)
    assert s.workspace_bytes == w0 + B * (2 * 8 + 2 * 4)                                     # allocated at the first globalised solve
    assert L.cfnmpc_get_sqp_ls_stats(s._h, None, None, None, None, 0, None) == EINVAL
    assert L.cfnmpc_get_sqp_ls_stats(s._h, pa, None, pn, None, 0, None) == 0 and (al <= 1.0).all() and (ns >= 0).all()
    # the sensitivities belong to the last QP, which a globalised solve leaves behind: refused; allowed again after full steps / RTI
    assert L.cfnmpc_eval_sens_x0(s._h, 1e-6, None) == EINVAL
    s.solve(1)
    assert L.cfnmpc_eval_sens_x0(s._h, 1e-6, None) == 0
    s.set_sqp_globalization("full_step")
    s.solve_sqp(2)
    assert L.cfnmpc_eval_sens_x0(s._h, 1e-6, None) == 0
    with pytest.raises(ValueError):
        s.set_sqp_globalization("newton")
