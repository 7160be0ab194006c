"""CPU checks of the globalised SQP solve (include/cfnmpc.h: cfnmpc_set_sqp_globalization): the numpy
restatement of the merit-function backtracking line search the GPU tests compare against (ls_ref, one iteration for rows at once;
sqp_ls_ref, the whole solve around the CPU restatement's RTI step), the identity the search rests on, its outcome on the hard
starts against full steps (recorded in tests/golden/sqp_ls.npz, regenerated and compared here), the kernel's resources in the
built code and the new entry points.  No GPU needed.

Regenerate the fixture:  python tests/test_sqp_ls_cpu.py
"""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from test_nlp_eval_cpu import _consts, _f, nlp_ref_rows

GOLDEN = os.path.join(ROOT, "tests", "golden", "sqp_ls.npz")
ETA, REDUCTION, ALPHA_MIN, RHO = 1e-4, 0.5, 2.0 ** -10, 0.5      # the defaults of cfnmpc_set_sqp_globalization; rho is fixed
HOV = 15.777730167256925
# the fixture's configuration (the hard starts of DESIGN.md section 5.11: three times the disturbances, hover start)
FIX = dict(seed=23, B=32, N=50, scale=3.0, tol=1e-6, max_iter=100, qp_tol=1e-11)

vp, i32, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
SIGS = {
    "cfnmpc_set_sqp_globalization": "intcfnmpc_set_sqp_globalization(cfnmpc_solver*s,intmode,doubleeta,doublereduction,doublealpha_min);",
    "cfnmpc_get_sqp_globalization": "intcfnmpc_get_sqp_globalization(constcfnmpc_solver*s,int*mode,double*eta,double*reduction,"
                                    "double*alpha_min);",
    "cfnmpc_get_sqp_ls_stats": "intcfnmpc_get_sqp_ls_stats(cfnmpc_solver*s,double*alpha,double*mu,int*n_short,int*n_fail,"
                               "inton_device,void*stream);",
    "cfnmpc_fleet_set_sqp_globalization": "intcfnmpc_fleet_set_sqp_globalization(cfnmpc_fleet*f,intmode,doubleeta,doublereduction,"
                                          "doublealpha_min);",
    "cfnmpc_fleet_get_sqp_ls_stats": "intcfnmpc_fleet_get_sqp_ls_stats(cfnmpc_fleet*f,double*alpha,double*mu,int*n_short,int*n_fail,"
                                     "inton_device,void*stream);",
}
ARGTYPES = {
    "cfnmpc_set_sqp_globalization": [vp, i32, dbl, dbl, dbl],
    "cfnmpc_get_sqp_globalization": [vp, vp, vp, vp, vp],
    "cfnmpc_get_sqp_ls_stats": [vp, vp, vp, vp, vp, i32, vp],
    "cfnmpc_fleet_set_sqp_globalization": [vp, i32, dbl, dbl, dbl],
    "cfnmpc_fleet_get_sqp_ls_stats": [vp, vp, vp, vp, vp, i32, vp],
}


# ---- the algorithm, restated (public state order; rows at once) -----------------------------------------------------------------
def n_trials(reduction=REDUCTION, alpha_min=ALPHA_MIN):
    """T: the smallest integer with reduction^T <= alpha_min, the powers by repeated multiplication (as the library forms them)"""
    T, a = 0, 1.0
    while a > alpha_min:
        a *= reduction
        T += 1
    return T


def make_data(x0, yref, yref_e, Qd, Rd, QNd, lb, ub, dt, erk_steps=1, params=None):
    """the data in force, as cfnmpc_eval_nlp sees it: x0 [B, 13], yref [B, N, 17], yref_e [B, 13]; Qd [13] or [B, 13], Rd [4] or
    [B, 4], QNd [13] or [B, 13] (the weights TIMES the cost scaling); lb, ub scalars or anything that broadcasts to [B, N, 4];
    params [B, 8] or None"""
    x0 = np.asarray(x0, dtype=np.float64)
    B, N = x0.shape[0], np.asarray(yref).shape[1]
    return dict(x0=x0, yref=np.asarray(yref, dtype=np.float64), yref_e=np.asarray(yref_e, dtype=np.float64),
                Qd=np.broadcast_to(np.asarray(Qd, dtype=np.float64), (B, 13)), Rd=np.broadcast_to(np.asarray(Rd, dtype=np.float64), (B, 4)),
                QNd=np.broadcast_to(np.asarray(QNd, dtype=np.float64), (B, 13)),
                lb=np.broadcast_to(np.asarray(lb, dtype=np.float64), (B, N, 4)), ub=np.broadcast_to(np.asarray(ub, dtype=np.float64), (B, N, 4)),
                dt=float(dt), M=int(erk_steps), c=_consts(params, B, np.float64))


def take_rows(d, idx):
    """the data of the rows idx"""
    out = dict(d)
    for k in ("x0", "yref", "yref_e", "Qd", "Rd", "QNd", "lb", "ub"):
        out[k] = d[k][idx]
    out["c"] = [v[idx] for v in d["c"]]
    return out


def _phi(x, u, d):
    """Phi(x, u): M classic RK4 steps of dt / M; x [B, 13], u [B, 4] -> [B, 13]"""
    h = d["dt"] / d["M"]
    xs, uu, c = x.T, u.T, d["c"]
    for _ in range(d["M"]):
        k1 = _f(xs, uu, c); k2 = _f(xs + 0.5 * h * k1, uu, c); k3 = _f(xs + 0.5 * h * k2, uu, c); k4 = _f(xs + h * k3, uu, c)
        xs = xs + (h / 6) * (k1 + 2 * k2 + 2 * k3 + k4)
    return xs.T


def constraints(x, u, d):
    """-> c1 = |c(v)|_1, cinf = res_eq (max-norm over x_0 - x0 and the defects), res_ineq (max-norm of the box violation) [B] each;
    c(v) = (x_0 - x0, x_{k+1} - Phi(x_k, u_k), max(lb - u, 0) + max(u - ub, 0)).  A NaN sticks in all three."""
    B, N = u.shape[0], u.shape[1]
    e = np.abs(x[:, 0] - d["x0"])
    c1, cinf = e.sum(1), e.max(1)
    for k in range(N):
        e = np.abs(x[:, k + 1] - _phi(x[:, k], u[:, k], d))
        c1 = c1 + e.sum(1)
        cinf = np.maximum(cinf, e.max(1))
    c1 = c1 + (np.maximum(d["lb"] - u, 0.0) + np.maximum(u - d["ub"], 0.0)).reshape(B, -1).sum(1)
    ineq = np.maximum(0.0, np.maximum(d["lb"] - u, u - d["ub"]).reshape(B, -1).max(1))
    return c1, cinf, ineq


def cost_terms(x, u, dx, du, d, T=np.float64):
    """-> gd = grad J(w)'d, dHd = d'H d, gabs = sum of the |terms| of gd, [B] each, in the precision of T"""
    x, u, dx, du = (np.asarray(a, dtype=T) for a in (x, u, dx, du))
    N = u.shape[1]
    Qd, Rd, QNd = d["Qd"].astype(T)[:, None, :], d["Rd"].astype(T)[:, None, :], d["QNd"].astype(T)
    tx = Qd * (x[:, :N] - d["yref"][:, :, :13].astype(T)) * dx[:, :N]
    tu = Rd * (u - d["yref"][:, :, 13:].astype(T)) * du
    tn = QNd * (x[:, N] - d["yref_e"].astype(T)) * dx[:, N]
    gd = tx.sum((1, 2)) + tu.sum((1, 2)) + tn.sum(1)
    gabs = np.abs(tx).sum((1, 2)) + np.abs(tu).sum((1, 2)) + np.abs(tn).sum(1)
    dHd = (Qd * dx[:, :N] ** 2).sum((1, 2)) + (Rd * du ** 2).sum((1, 2)) + (QNd * dx[:, N] ** 2).sum(1)
    return gd, dHd, gabs


def ls_ref(w, w_hat, mu, d, eta=ETA, reduction=REDUCTION, alpha_min=ALPHA_MIN, failed=None):
    """One iteration's line search for B rows at once.  w = (x [B, N + 1, 13], u [B, N, 4]) = w_{j-1}, w_hat = the QP step's
    candidate, mu [B] the penalty so far (0 before iteration 1), d = make_data(...), failed [B] (bool; None: no row) = rows whose
    QP failed (status 4: the step kept the iterate, no search).
    -> alpha [B], mu [B], (x_j, u_j), res [B, 3] = (res_step = |w_hat - w|_inf, res_eq, res_ineq of w_j), accepted [B] (False: no
       trial was accepted, the row took alpha_T: one count of n_fail), margins [T + 1, B, 2] = per evaluated trial (lhs - rhs of
       the test, the magnitude of its terms |alpha gd| + alpha^2 dHd / 2 + mu (c1(trial) + c1(w))); NaN where not evaluated"""
    x, u = (np.asarray(a, dtype=np.float64) for a in w)
    xh, uh = (np.asarray(a, dtype=np.float64) for a in w_hat)
    B = x.shape[0]
    failed = np.zeros(B, dtype=bool) if failed is None else np.asarray(failed, dtype=bool)
    dx, du = xh - x, uh - u
    with np.errstate(all="ignore"):
        gd, dHd, _ = cost_terms(x, u, dx, du, d)
        c1w, _, _ = constraints(x, u, d)
        mu = np.array(mu, dtype=np.float64)
        cand = (gd + 0.5 * dHd) / ((1.0 - RHO) * c1w)
        up = (c1w > 0) & (cand > mu)                    # (a NaN keeps mu)
        mu[up] = cand[up]
        D = gd - mu * c1w
        T = n_trials(reduction, alpha_min)
        alpha = np.ones(B); accepted = np.ones(B, dtype=bool); open_ = ~failed
        res = np.empty((B, 3))
        res[:, 0] = np.maximum(np.abs(dx).reshape(B, -1).max(1), np.abs(du).reshape(B, -1).max(1))
        margins = np.full((T + 1, B, 2), np.nan)
        a = 1.0
        for t in range(T + 1):
            if t > 0:
                if not open_.any():
                    break
                a *= reduction
            xt, ut = (xh, uh) if t == 0 else (x + a * dx, u + a * du)
            c1t, cinf, ineq = constraints(xt, ut, d)
            if t == 0:
                res[:, 1], res[:, 2] = cinf, ineq
            lhs = a * gd + 0.5 * a * a * dHd + mu * (c1t - c1w)
            rhs = eta * a * D
            acc = lhs <= rhs                            # (a NaN fails it)
            margins[t, open_, 0] = (lhs - rhs)[open_]
            margins[t, open_, 1] = (np.abs(a * gd) + 0.5 * a * a * dHd + mu * (c1t + c1w))[open_]
            take = open_ & (acc | (t == T))
            alpha[take] = a
            accepted[take] = acc[take]
            res[take, 1], res[take, 2] = cinf[take], ineq[take]
            open_ = open_ & ~take
        short = alpha < 1.0
        xj, uj = xh.copy(), uh.copy()                   # (alpha = 1: the candidate, bit for bit)
        xj[short] = x[short] + alpha[short, None, None] * dx[short]
        uj[short] = u[short] + alpha[short, None, None] * du[short]
    return alpha, mu, (xj, uj), res, accepted, margins


def ties(margins, rel=1e-9):
    """rows with a test decided by less than rel times the magnitude of its terms at any evaluated trial"""
    with np.errstate(invalid="ignore"):
        return (np.abs(margins[:, :, 0]) < rel * margins[:, :, 1]).any(0)


def data_of_opts(copts, x0, yref, yref_e):
    """the data of the CPU restatement's options (uniform weights, scalar box, nominal model)"""
    W, WN = np.array(list(copts.W)), np.array(list(copts.WN))
    return make_data(x0, yref, yref_e, W[:13], W[13:], WN, copts.u_min, copts.u_max, copts.dt)


def sqp_ls_ref(cref, copts, x0, yref, yref_e, xr, ur, max_iter, tol, globalize=True, eta=ETA, reduction=REDUCTION,
               alpha_min=ALPHA_MIN):
    """The whole solve around the CPU restatement's RTI step (in place on xr, ur), the stop rule of cfnmpc_solve_sqp.
    globalize = False: full steps (ls_ref is not consulted).
    -> dict(status, sqp_iter, res [B, 3], ran, alpha, mu, n_short, n_fail)"""
    B = x0.shape[0]
    status = np.full(B, 2, dtype=np.int32); it = np.zeros(B, dtype=np.int32); res = np.zeros((B, 3))
    alpha = np.ones(B); mu = np.zeros(B); n_short = np.zeros(B, dtype=np.int32); n_fail = np.zeros(B, dtype=np.int32)
    done = np.zeros(B, dtype=bool)
    data = data_of_opts(copts, x0, yref, yref_e)
    ran = 0
    for j in range(1, max_iter + 1):
        idx = np.flatnonzero(~done)
        if idx.size == 0:
            break
        ran = j
        xa, ua = xr[idx].copy(), ur[idx].copy()
        sq, _, _, _ = cref.rti_step(copts, xa, ua, x0[idx].copy(), yref[idx].copy(), yref_e[idx].copy(), nthreads=0)
        dj = take_rows(data, idx)
        if globalize:
            al, m, (xa, ua), rs, acc, _ = ls_ref((xr[idx], ur[idx]), (xa, ua), mu[idx], dj, eta, reduction, alpha_min, failed=sq == 4)
            alpha[idx], mu[idx] = al, m
            n_short[idx] += al < 1.0
            n_fail[idx] += ~acc
        else:
            _, cinf, ineq = constraints(xa, ua, dj)
            step = np.maximum(np.abs(xa - xr[idx]).reshape(idx.size, -1).max(1), np.abs(ua - ur[idx]).reshape(idx.size, -1).max(1))
            rs = np.stack([step, cinf, ineq], 1)
        res[idx], it[idx] = rs, j
        conv = (rs <= tol).all(1)
        status[idx] = np.where(sq == 4, 4, np.where(conv, 0, 2))
        done[idx] = (sq == 4) | conv
        xr[idx], ur[idx] = xa, ua
    return dict(status=status, sqp_iter=it, res=res, ran=ran, alpha=alpha, mu=mu, n_short=n_short, n_fail=n_fail)


def fixture_inputs(oracle, B=FIX["B"], N=FIX["N"], seed=FIX["seed"], scale=FIX["scale"]):
    """x0, yref, yref_e and the hover start of the fixture's configuration"""
    rng = np.random.default_rng(seed)
    x0 = oracle.sample_hover_x0(rng, B, scale=scale)
    yr, ye = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    yref, yref_e = np.repeat(yr[None], B, 0).copy(), np.repeat(ye[None], B, 0).copy()
    return x0, yref, yref_e, np.repeat(x0[:, None, :], N + 1, 1).copy(), np.full((B, N, 4), HOV)


def generate(oracle, cref):
    """both solves of the fixture's configuration: the full-step loop of tests/test_gpu_sqp.py (ref_sqp) and sqp_ls_ref"""
    from test_gpu_sqp import ref_sqp
    x0, yref, yref_e, xs, us = fixture_inputs(oracle)
    copts = cref.default_opts(N=FIX["N"], tol=FIX["qp_tol"])
    xf, uf = xs.copy(), us.copy()
    st_f, it_f, _rs, _n = ref_sqp(cref, copts, x0, yref, yref_e, xf, uf, FIX["max_iter"], FIX["tol"])
    xl, ul = xs.copy(), us.copy()
    r = sqp_ls_ref(cref, copts, x0, yref, yref_e, xl, ul, FIX["max_iter"], FIX["tol"])
    both = (st_f == 0) & (r["status"] == 0)
    cost = lambda x, u: nlp_ref_rows(x[both], u[both], x0[both], yref[both], yref_e[both], oracle.Q_DIAG, oracle.R_DIAG,
                                     oracle.QN_DIAG, 0.0, 22.0, oracle.DT)[0]
    cf, cl = (cost(xf, uf), cost(xl, ul)) if both.any() else (np.zeros(0), np.zeros(0))
    return dict(status_full=st_f.astype(np.int32), sqp_iter_full=it_f.astype(np.int32), status_ls=r["status"].astype(np.int32),
                sqp_iter_ls=r["sqp_iter"].astype(np.int32)), r, (cf, cl)


@pytest.fixture(scope="module")
def outcome(oracle, cref):
    return generate(oracle, cref)


# ---- the restatement's own checks ---------------------------------------------------------------------------------------------
def test_trial_count():
    assert n_trials() == 10 and n_trials(0.5, 1.0) == 0 and n_trials(0.5, 0.3) == 2 and n_trials(0.9, 0.5) == 7
    assert n_trials(0.5, 2.0 ** -32) == 32 and n_trials(0.5, 2.0 ** -33) == 33


def test_cost_difference_identity(oracle):
    """J(w + a d) - J(w) = a gd + a^2 dHd / 2: the costs by nlp_ref_rows in np.longdouble (their difference is then exact to
    1e-19 |J|), gd and dHd by cost_terms in FP64, whose rounding is bounded by a few eps times the sum of the |terms|"""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("no extended precision on this platform")
    B, N = 6, 8
    rng = np.random.default_rng(41)
    x0 = oracle.sample_hover_x0(rng, B, scale=2.0)
    yr, ye = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    yref, yref_e = np.repeat(yr[None], B, 0).copy(), np.repeat(ye[None], B, 0).copy()
    x = np.repeat(x0[:, None, :], N + 1, 1) + 0.05 * rng.standard_normal((B, N + 1, 13))
    u = HOV + 3.0 * rng.standard_normal((B, N, 4))
    dx, du = 0.1 * rng.standard_normal(x.shape), 2.0 * rng.standard_normal(u.shape)
    Qd = oracle.Q_DIAG * (0.5 + rng.random((B, 13))); Rd = oracle.R_DIAG * (0.5 + rng.random((B, 4)))   # per-instance rows
    QNd = 1.3 * oracle.QN_DIAG
    d = make_data(x0, yref, yref_e, Qd, Rd, QNd, 0.0, 22.0, oracle.DT)
    gd, dHd, gabs = cost_terms(x, u, dx, du, d)
    LD = np.longdouble
    J = lambda xx, uu: nlp_ref_rows(xx, uu, x0, yref, yref_e, Qd, Rd, QNd, 0.0, 22.0, oracle.DT, T=LD)[0]
    J0 = J(x.astype(LD), u.astype(LD))
    for a in (1.0, 0.5, 0.125, 2.0 ** -10):
        dJ = J(x.astype(LD) + LD(a) * dx.astype(LD), u.astype(LD) + LD(a) * du.astype(LD)) - J0
        pred = a * gd + 0.5 * a * a * dHd
        err = np.abs(dJ - pred.astype(LD)).astype(np.float64)
        bound = 1e-13 * (a * gabs + 0.5 * a * a * dHd)
        print(f"alpha {a:.4g}: |dJ| {np.abs(dJ).max():.3e}  err {err.max():.2e}  bound {bound.min():.2e}")
        assert (err <= bound).all(), (a, err, bound)


def test_ls_ref_cases(oracle):
    """a feasible full step that lowers the cost is accepted at alpha = 1 with the iterate untouched; a failed row is not searched;
    a NaN row ends at alpha_T without an accepted trial"""
    B, N = 3, 6
    rng = np.random.default_rng(5)
    x0 = oracle.sample_hover_x0(rng, B, scale=1.0)
    yr, ye = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    yref, yref_e = np.repeat(yr[None], B, 0).copy(), np.repeat(ye[None], B, 0).copy()
    d = make_data(x0, yref, yref_e, oracle.Q_DIAG, oracle.R_DIAG, oracle.QN_DIAG, 0.0, 22.0, oracle.DT)
    def rollout(u):
        x = np.empty((B, N + 1, 13)); x[:, 0] = x0
        for k in range(N):
            x[:, k + 1] = _phi(x[:, k], u[:, k], d)
        return x
    u = np.full((B, N, 4), HOV + 1.0); x = rollout(u)
    uh = np.full((B, N, 4), HOV + 0.5); xh = rollout(uh)     # feasible, closer to the input reference
    xh[2, 3, 1] = np.nan
    al, mu, (xj, uj), res, acc, mg = ls_ref((x, u), (xh, uh), np.zeros(B), d, failed=np.array([False, True, False]))
    assert al[0] == 1.0 and acc[0] and np.array_equal(xj[0], xh[0]) and np.array_equal(uj[0], uh[0])
    assert res[0, 1] < 1e-13 and res[0, 2] == 0.0 and res[0, 0] == max(np.abs(xh[0] - x[0]).max(), 0.5)
    assert al[1] == 1.0 and acc[1] and np.isnan(mg[:, 1]).all()                      # no trial evaluated
    assert al[2] == ALPHA_MIN and not acc[2] and np.isnan(res[2, :2]).all() and res[2, 2] == 0.0 and np.isnan(xj[2]).any()
    assert not ties(mg)[0]


# ---- the outcome on the hard starts ---------------------------------------------------------------------------------------------
def test_line_search_converges_the_hard_starts(outcome):
    g, r, (cf, cl) = outcome
    full, ls = g["status_full"] == 0, g["status_ls"] == 0
    print(f"converged: full steps {full.sum()}, line search {ls.sum()} of {full.size}; n_short {r['n_short'].tolist()} "
          f"n_fail {r['n_fail'].tolist()}; sqp_iter {g['sqp_iter_ls'].tolist()}")
    assert set(np.unique(g["status_full"])) <= {0, 2} and set(np.unique(g["status_ls"])) <= {0, 2}
    assert full.sum() >= 1 and ls.sum() >= 4 * full.sum(), (full.sum(), ls.sum())
    assert (ls | ~full).all(), np.flatnonzero(full & ~ls)                            # none lost
    rel = np.abs(cf - cl) / np.abs(cf)
    print(f"cost of the rows converged both ways: relative difference {rel.max():.2e}")
    assert (rel <= 1e-8).all(), rel
    assert (r["res"][ls] <= FIX["tol"]).all()
    assert (r["n_short"] <= g["sqp_iter_ls"]).all() and (r["n_fail"] <= r["n_short"]).all()


def test_outcome_fixture_is_current(outcome):
    g = outcome[0]
    assert os.path.exists(GOLDEN), "tests/golden/sqp_ls.npz is missing: python tests/test_sqp_ls_cpu.py"
    z = np.load(GOLDEN)
    assert sorted(z.files) == sorted(g)
    for k in g:
        assert z[k].dtype == g[k].dtype and np.array_equal(z[k], g[k]), (k, z[k], g[k])


# ---- built code and entry points ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cfn_resource", os.path.join(ROOT, "tools", "resource.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    try:
        return mod.resource_table()
    except FileNotFoundError:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crazyflie_nmpc_amd", "csrc"), "-s", "ARCH=gfx950"])
        return mod.resource_table()


@pytest.mark.parametrize("name", ["k_sqp_ls", "k_sqp_ls_par"])
def test_ls_kernels_within_resources(table, name):
    assert name in table, sorted(table)
    r = table[name]
    assert r["unit"] == "cfnmpc_kernels"          # (the set of device units stays at four)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    assert r["vgpr"] <= 256 and r["occupancy"] >= 1, r
    assert r["lds"] <= 40960, r                   # four workgroups per compute unit (160 KB): one wavefront per SIMD


def _header():
    src = open(os.path.join(ROOT, "include", "cfnmpc.h")).read()
    return re.sub(r"\s+", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def test_entry_points_declared_exported_and_bound():
    src = _header()
    from crazyflie_nmpc_amd import _lib
    L = _lib.lib()
    for name, sig in SIGS.items():
        assert sig in src, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == ARGTYPES[name], name
    assert "#defineCFNMPC_SQP_FULL_STEP0" in src and "#defineCFNMPC_SQP_MERIT_BACKTRACKING1" in src
    assert L.cfnmpc_abi_version() == 9            # new entry points only: cfnmpc_opts and old signatures unchanged
    assert L.cfnmpc_opts_size() == ctypes.sizeof(_lib.Opts)
    # the setters refuse a NULL handle before they touch a device
    assert L.cfnmpc_set_sqp_globalization(None, 1, 0.0, 0.0, 0.0) == -1
    assert L.cfnmpc_get_sqp_globalization(None, None, None, None, None) == -1
    assert L.cfnmpc_get_sqp_ls_stats(None, None, None, None, None, 0, None) == -1
    assert L.cfnmpc_fleet_set_sqp_globalization(None, 1, 0.0, 0.0, 0.0) == -1
    assert L.cfnmpc_fleet_get_sqp_ls_stats(None, None, None, None, None, 0, None) == -1


def test_python_wrappers_and_defaults():
    from crazyflie_nmpc_amd import BatchSolver
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.solver import SQP_MODES
    assert SQP_MODES == ("full_step", "merit_backtracking")
    for cls in (BatchSolver, MixedHorizonFleet):
        sig = inspect.signature(cls.set_sqp_globalization)
        assert [sig.parameters[k].default for k in ("mode", "eta", "reduction", "alpha_min")] == ["merit_backtracking", 0, 0, 0]
        assert callable(cls.sqp_globalization) and callable(cls.sqp_ls_stats)


if __name__ == "__main__":
    import cfnmpc_oracle
    import cref
    cref.build()
    g, r, _c = generate(cfnmpc_oracle, cref)
    np.savez(GOLDEN, **g)
    print("full steps:", int((g["status_full"] == 0).sum()), "line search:", int((g["status_ls"] == 0).sum()), "->", GOLDEN)
