"""CPU checks of the heterogeneous fleet case: per-instance model parameters, per-instance weight
rows, cost scaling, erk_steps 2 and per-stage boxes in force TOGETHER, at the horizons where the engine's code paths change.
This file defines the case (het_case) and its reference (het_ref_step), both shared with tests/test_gpu_heterogeneous.py, and
checks on the reference alone that the composition collapses onto the references of the single features, that the case
exercises what it is meant to (constrained and free rows, every Riccati checkpoint class of every horizon, a referee that
converges on every compared row), and that the NLP and line-search references accept the composed data.  No new reference
mathematics: rk4_sens of test_model_params_cpu.py, oracle.qp_from_blocks / solve_qp_dense / solve_qp_refined, nlp_ref_rows of
test_nlp_eval_cpu.py, make_data / ls_ref / ties of test_sqp_ls_cpu.py.  No GPU needed."""
import numpy as np
import pytest

from test_model_params_cpu import NOMINAL, hover, random_params, rk4_sens
from test_nlp_eval_cpu import _consts, _f, _objective, nlp_ref_rows
from test_sqp_ls_cpu import ls_ref, make_data, take_rows, ties

DT = 0.015
EDGES = (5, 8, 17, 33, 40)       # minimum | a checkpoint stage that must not be used | one past the dense head | one past the
#                                  last checkpoint | smallest forward_split horizon, on the as_commit threshold
CHK = (4, 8, 12, 16, 24, 32)     # Riccati checkpoint stages (csrc/cfnmpc_ws.hpp: chk_stage)
B_HET = 130                      # two full 64-lane groups plus two rows; the last row-group block half full
ROWS = tuple(range(0, B_HET, 3))  # the 44 rows compared with the exact QP
SCALING = (2.0, 0.5)
ERK_STEPS = 2
SCALAR_BOX = (1.0, 21.0)
KICK = 1.0                       # m/s on the body velocity; part of the recipe (0.5 made the referee cycle on one N = 40 row)
LS_CASES = ((5, "stages"), (17, "stages"), (40, "stages"), (8, "scalar"))   # where the GPU file runs the line search


# ---- the case and its reference (shared with tests/test_gpu_heterogeneous.py) ----------------------------------------------------
def compose(oracle, p, W, WN, scaling, lb, ub, x0, erk_steps, box="stages", scalar_box=None):
    """the data of one heterogeneous problem set from its parts -> dict; regulation to (0, 0, 0.4) with each row's input
    reference hover(p_i), pre-step iterate x_k = x0, u_k = hover(p_i) clipped into the row's box"""
    B, N = lb.shape[0], lb.shape[1]
    yr, ye = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    yref, yref_e = np.repeat(yr[None], B, 0).copy(), np.repeat(ye[None], B, 0).copy()
    hov = hover(p)
    yref[:, :, 13:] = hov[:, None, None]
    x = np.repeat(x0[:, None, :], N + 1, 1).copy()
    u = np.clip(np.broadcast_to(hov[:, None, None], (B, N, 4)), lb, ub)
    return dict(B=B, N=N, box=box, scalar_box=scalar_box, p=p, W=W, WN=WN, scaling=tuple(scaling), erk_steps=int(erk_steps),
                lb=lb, ub=ub, x0=x0, yref=yref, yref_e=yref_e, x=x, u=u,
                Qd=scaling[0] * W[:, :13], Rd=scaling[0] * W[:, 13:], QNd=scaling[1] * WN)   # the effective (scaled) weights


def het_case(oracle, N, B=B_HET, box="stages"):
    """The heterogeneous case of horizon N, drawn from default_rng(1000 + N) in a fixed order: parameter rows, weight rows
    (default weights x log-uniform factors in [1/4, 4] per entry), the stage boxes lb ~ U(0, 4), ub ~ U(19, 22), hover-centred x0
    with N(0, 1) m/s on the body velocity.  box = "scalar": the same draws, then the scalar box [1, 21] (set through set_box)."""
    assert box in ("stages", "scalar")
    rng = np.random.default_rng(1000 + N)
    p = random_params(rng, B)
    W = oracle.W_DIAG * np.exp(rng.uniform(np.log(0.25), np.log(4.0), (B, 17)))
    WN = oracle.QN_DIAG * np.exp(rng.uniform(np.log(0.25), np.log(4.0), (B, 13)))
    lb = rng.uniform(0.0, 4.0, (B, N, 4))
    ub = rng.uniform(19.0, 22.0, (B, N, 4))
    if box == "scalar":
        lb, ub = np.full((B, N, 4), SCALAR_BOX[0]), np.full((B, N, 4), SCALAR_BOX[1])
    x0 = oracle.sample_hover_x0(rng, B, scale=1.0)
    x0[:, 7:10] += rng.normal(0, KICK, (B, 3))
    return compose(oracle, p, W, WN, SCALING, lb, ub, x0, ERK_STEPS, box, SCALAR_BOX if box == "scalar" else None)


def het_ref_step(oracle, case, i, x=None, u=None):
    """the exact QP of one RTI step of row i from the iterate (x, u) (None: the case's pre-step iterate): blocks by
    rk4_sens(x, u, p_i, DT, erk_steps), q, r and the bounds from the row's scaled weights and box
    -> (x + dx, u + du of oracle.solve_qp_dense, qp, oracle.solve_qp_refined(qp): the referee)"""
    c = case
    x = c["x"][i] if x is None else x
    u = c["u"][i] if u is None else u
    N = c["N"]
    A = np.empty((N, 13, 13)); Bm = np.empty((N, 13, 4)); b = np.empty((N, 13))
    for k in range(N):
        phi, A[k], Bm[k] = rk4_sens(x[k], u[k], c["p"][i], DT, c["erk_steps"])
        b[k] = phi - x[k + 1]
    Qd, Rd, QNd = c["Qd"][i], c["Rd"][i], c["QNd"][i]
    q = np.empty((N + 1, 13))
    q[:-1] = Qd * (x[:-1] - c["yref"][i, :, :13])
    q[-1] = QNd * (x[-1] - c["yref_e"][i])
    r = Rd * (u - c["yref"][i, :, 13:])
    qp = oracle.qp_from_blocks(A, Bm, b, q, r, c["x0"][i] - x[0], Qd, Rd, QNd, c["lb"][i] - u, c["ub"][i] - u)
    sol = oracle.solve_qp_dense(qp)
    return x + sol["dx"], u + sol["du"], qp, oracle.solve_qp_refined(qp)


def het_reference(oracle, cache, N, box):
    """the case (N, box) and the references of its compared rows, computed once per cache (a module-scoped dict)
    -> (case, {i: (xr, ur, qp, referee)})"""
    if (N, box) not in cache:
        case = het_case(oracle, N, box=box)
        cache[(N, box)] = (case, {i: het_ref_step(oracle, case, i) for i in ROWS})
    return cache[(N, box)]


def last_active(cls):
    """last stage with an input on its bound (cls [N][4], non-zero = active); -1: none"""
    st = np.flatnonzero((np.asarray(cls) != 0).any(axis=1))
    return int(st.max()) if st.size else -1


def kst_of(last, N):
    """start stage of the masked sweep (k_sens_mask) for a row whose last active stage is `last` >= 0: the smallest checkpoint
    above it that lies inside the horizon, else N"""
    for k in CHK:
        if last < k < N:
            return k
    return N


def chk_classes(N):
    """the checkpoint classes of horizon N: the checkpoints inside the horizon (kst can also be N itself: no checkpoint, the
    sweep starts from the terminal weight)"""
    return [k for k in CHK if k < N]


def nlp_args(case, rows=None):
    """the data arguments of nlp_ref_rows / _compare behind (x, u): x0, yref, yref_e and the keywords, for the rows `rows`"""
    r = slice(None) if rows is None else np.asarray(rows)
    c = case
    return (c["x0"][r], c["yref"][r], c["yref_e"][r]), dict(Qd=c["Qd"][r], Rd=c["Rd"][r], QNd=c["QNd"][r], lb=c["lb"][r], ub=c["ub"][r],
                                                            M=c["erk_steps"], params=c["p"][r])


def ls_data(case):
    """make_data of tests/test_sqp_ls_cpu.py on the composed data"""
    c = case
    return make_data(c["x0"], c["yref"], c["yref_e"], c["Qd"], c["Rd"], c["QNd"], c["lb"], c["ub"], DT, c["erk_steps"], c["p"])


def hover_start(case):
    """the iterate of init_iterate(INIT_HOVER) with the rows in force: x_k = x0, u_k = hover(p_i), NOT clipped into the box"""
    c = case
    return c["x"].copy(), np.broadcast_to(hover(c["p"])[:, None, None], c["u"].shape).copy()


@pytest.fixture(scope="module")
def het_cache():
    return {}


# ---- 1. the composed reference collapses onto the existing ones ------------------------------------------------------------------
def _qp_equal(a, b, tol):
    worst = 0.0
    for f in ("A", "B", "b", "q", "r", "lb", "ub", "dx0", "Qd", "Rd", "QNd"):
        worst = max(worst, float(np.abs(getattr(a, f) - getattr(b, f)).max()))
    assert worst <= tol, worst
    return worst


@pytest.mark.parametrize("N", [5, 17])
def test_collapses_onto_the_uniform_reference(oracle, N):
    """nominal parameters, uniform default weights, scaling (1, 1), scalar box [0, 22], M = 1: test_weights_cpu.ref_step.  The two
    differ in the model statement alone (oracle.rk4_sens against rk4_sens at the nominal row): 1e-13, the tolerance of
    test_model_params_cpu.test_reference_at_nominal_matches_oracle, on every entry of the QP; the two dense solutions of these QPs
    then agree as two QP solves do in this project (1e-8, with the referee behind it)."""
    from test_weights_cpu import agree, ref_step
    B = 4
    rng = np.random.default_rng(7 + N)
    x0 = oracle.sample_hover_x0(rng, B, scale=1.0)
    x0[:, 7:10] += rng.normal(0, KICK, (B, 3))
    W, WN = np.tile(oracle.W_DIAG, (B, 1)), np.tile(oracle.QN_DIAG, (B, 1))
    c = compose(oracle, np.tile(NOMINAL, (B, 1)), W, WN, (1.0, 1.0), np.zeros((B, N, 4)), np.full((B, N, 4), 22.0), x0, 1)
    assert np.array_equal(c["u"], np.full((B, N, 4), hover(NOMINAL))) and abs(hover(NOMINAL) - oracle.HOV_W) < 1e-14
    for i in range(B):
        xr, ur, qp, ref = het_ref_step(oracle, c, i)
        x1, u1, qp1 = ref_step(oracle, c["x"][i], c["u"][i], x0[i], c["yref"][i], c["yref_e"][i], oracle.W_DIAG, oracle.QN_DIAG)
        e_qp = _qp_equal(qp, qp1, 1e-13)
        e = agree(oracle, xr, ur, x1, u1, qp1, c["x"][i], c["u"][i], 1e-8)
        print(f"N {N} row {i}: QP data differ by {e_qp:.2e}, solutions by {e:.2e}")
        assert e <= 1e-8, (i, e)


@pytest.mark.parametrize("N", [5, 17])
def test_collapses_onto_the_model_parameter_reference(oracle, N):
    """parameter rows only (uniform weights, scaling (1, 1), scalar box [0, 22], M = 2): the formula of
    test_gpu_model_params._ref_step, which uses the same blocks: the same QP and the same dense solution, bit for bit"""
    from test_gpu_model_params import _ref_step
    B = 4
    rng = np.random.default_rng(17 + N)
    p = random_params(rng, B)
    x0 = oracle.sample_hover_x0(rng, B, scale=1.0)
    x0[:, 7:10] += rng.normal(0, KICK, (B, 3))
    W, WN = np.tile(oracle.W_DIAG, (B, 1)), np.tile(oracle.QN_DIAG, (B, 1))
    c = compose(oracle, p, W, WN, (1.0, 1.0), np.zeros((B, N, 4)), np.full((B, N, 4), 22.0), x0, 2)
    for i in range(B):
        xr, ur, qp, ref = het_ref_step(oracle, c, i)
        x1, u1, qp1 = _ref_step(oracle, c["x"][i], c["u"][i], x0[i], c["yref"][i], c["yref_e"][i], p[i], 2, oracle.W_DIAG, oracle.QN_DIAG)
        assert _qp_equal(qp, qp1, 0.0) == 0.0
        assert np.array_equal(xr, x1) and np.array_equal(ur, u1), i


def test_case_recipe(oracle):
    """the parts of het_case: shapes, ranges, the order of the draws (the scalar variant shares everything but the box), the
    weights as test_weights_cpu.random_rows forms them, the iterate inside the box"""
    a, b = het_case(oracle, 8), het_case(oracle, 8, box="scalar")
    for k in ("p", "W", "WN", "x0", "yref", "yref_e", "x"):
        assert np.array_equal(a[k], b[k]), k
    assert a["B"] == B_HET and a["lb"].shape == (B_HET, 8, 4) and ROWS[-1] == 129 and len(ROWS) == 44
    assert (a["lb"] >= 0).all() and (a["lb"] <= 4).all() and (a["ub"] >= 19).all() and (a["ub"] <= 22).all()
    assert (b["lb"] == 1.0).all() and (b["ub"] == 21.0).all() and b["scalar_box"] == (1.0, 21.0) and a["scalar_box"] is None
    for c in (a, b):
        f, fn = c["W"] / oracle.W_DIAG, c["WN"] / oracle.QN_DIAG
        assert f.min() >= 0.25 - 1e-12 and f.max() <= 4.0 + 1e-12 and fn.min() >= 0.25 - 1e-12 and fn.max() <= 4.0 + 1e-12
        assert np.array_equal(c["Qd"], 2.0 * c["W"][:, :13]) and np.array_equal(c["Rd"], 2.0 * c["W"][:, 13:])
        assert np.array_equal(c["QNd"], 0.5 * c["WN"])
        assert (c["u"] >= c["lb"]).all() and (c["u"] <= c["ub"]).all()
        assert np.array_equal(c["yref"][:, :, 13:], np.broadcast_to(hover(c["p"])[:, None, None], (B_HET, 8, 4)))
        assert np.array_equal(c["x"], np.repeat(c["x0"][:, None, :], 9, 1))
    rng = np.random.default_rng(1008)       # the first draw is random_params(rng, B)
    assert np.array_equal(a["p"], random_params(rng, B_HET))
    assert not np.array_equal(a["p"], het_case(oracle, 5)["p"])


# ---- 2. the case is a test at all ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", ["stages", "scalar"])
@pytest.mark.parametrize("N", EDGES)
def test_case_exercises_what_it_is_meant_to(oracle, het_cache, N, box):
    """On the reference alone, for the 44 compared rows: the referee reaches KKT <= 1e-12 on EVERY row (no row may be left out),
    at least a quarter of the rows have an input on its bound and at least two have none, and the last active stage of the
    constrained rows reaches into every checkpoint class the horizon has (kst_of: every checkpoint inside the horizon; rows whose
    last active stage lies behind the last such checkpoint, kst = N, are printed: at N = 33 that is stage 32 alone, which none
    of the 44 rows reaches with stage boxes)."""
    case, ref = het_reference(oracle, het_cache, N, box)
    kkt = np.array([ref[i][3]["kkt"] for i in ROWS])
    last = np.array([last_active(ref[i][3]["cls"]) for i in ROWS])
    dense = max(max(np.abs(ref[i][0] - (case["x"][i] + ref[i][3]["dx"])).max(), np.abs(ref[i][1] - (case["u"][i] + ref[i][3]["du"])).max())
                for i in ROWS)
    con = last >= 0
    classes = sorted({kst_of(l, N) for l in last[con]})
    print(f"N {N} box {box}: constrained / free {int(con.sum())} / {int((~con).sum())}  referee KKT {kkt.max():.1e}  "
          f"solves up to {max(ref[i][3]['solves'] for i in ROWS)}  last active stage {last[con].min()} .. {last[con].max()}  "
          f"kst classes {classes}  dense solve vs referee {dense:.1e}")
    assert (kkt <= 1e-12).all(), (np.array(ROWS)[kkt > 1e-12], kkt.max())
    assert con.sum() >= len(ROWS) / 4 and (~con).sum() >= 2, (con.sum(), (~con).sum())
    assert [k for k in classes if k < N] == chk_classes(N), (classes, chk_classes(N))


# ---- 3. the NLP and line-search references accept the composed data -------------------------------------------------------------
def test_nlp_reference_on_composed_data_against_finite_differences(oracle):
    """nlp_ref_rows with per-row Qd / Rd / QNd, per-stage lb / ub, params and erk_steps = 2 TOGETHER, on three rows of the N = 8
    case: on a dynamically feasible rollout gu is dJ/du of the single-shooting objective (central differences, h = 1e-5; the
    bound 1e-6 max(1, |g|) and its derivation are those of
    test_nlp_eval_cpu.test_reference_against_finite_differences_of_the_single_shooting_objective, |J| <= 3e4 included)."""
    N, h = 8, 1e-5
    c = het_case(oracle, N)
    rows = np.array([0, 64, 129])
    rng = np.random.default_rng(5)
    u = np.clip(hover(c["p"][rows])[:, None, None] + 2.0 * rng.standard_normal((3, N, 4)), c["lb"][rows] + 0.1, c["ub"][rows] - 0.1)
    cs = _consts(c["p"][rows], 3, np.float64)
    x = np.empty((3, N + 1, 13)); x[:, 0] = c["x0"][rows]
    hs = DT / ERK_STEPS
    for k in range(N):
        xs = x[:, k].T
        for _ in range(ERK_STEPS):
            k1 = _f(xs, u[:, k].T, cs); k2 = _f(xs + 0.5 * hs * k1, u[:, k].T, cs); k3 = _f(xs + 0.5 * hs * k2, u[:, k].T, cs)
            k4 = _f(xs + hs * k3, u[:, k].T, cs)
            xs = xs + (hs / 6) * (k1 + 2 * k2 + 2 * k3 + k4)
        x[:, k + 1] = xs.T
    (x0, yr, ye), kw = nlp_args(c, rows)
    cost, res, pi, gu = nlp_ref_rows(x, u, x0, yr, ye, kw["Qd"], kw["Rd"], kw["QNd"], kw["lb"], kw["ub"], DT, kw["M"], kw["params"])
    assert (res[:, 1] < 1e-13).all() and (res[:, 2] == 0.0).all()          # feasible rollouts inside their boxes
    for n, i in enumerate(rows):
        ci = [v[n] for v in cs]
        J = lambda uu, xx: _objective(oracle, uu, xx, yr[n], ye[n], kw["Qd"][n], kw["Rd"][n], kw["QNd"][n], DT, ERK_STEPS, ci)
        assert abs(cost[n] - J(u[n], x0[n])) <= 1e-12 * abs(cost[n]) and abs(cost[n]) <= 3e4
        g_fd = np.empty((N, 4))
        for k in range(N):
            for a in range(4):
                up, um = u[n].copy(), u[n].copy()
                up[k, a] += h; um[k, a] -= h
                g_fd[k, a] = (J(up, x0[n]) - J(um, x0[n])) / (2 * h)
        p_fd = np.empty(13)
        for j in range(13):
            xp, xm = x0[n].copy(), x0[n].copy()
            xp[j] += h; xm[j] -= h
            p_fd[j] = (J(u[n], xp) - J(u[n], xm)) / (2 * h)
        eg, ep = np.abs(gu[n] - g_fd).max(), np.abs(pi[n, 0] - p_fd).max()
        print(f"row {i}: |J| {abs(cost[n]):.3e}  |gu| {np.abs(gu[n]).max():.3e} err {eg:.2e}  |pi0| {np.abs(pi[n, 0]).max():.3e} err {ep:.2e}")
        assert eg <= 1e-6 * max(1.0, np.abs(gu[n]).max()), (i, eg)
        assert ep <= 1e-6 * max(1.0, np.abs(pi[n, 0]).max()), (i, ep)
        # the row's data matter: its neighbour's weights or parameters give another gradient
        o = rows[(n + 1) % 3]
        (_a, _b, _c), kwo = nlp_args(c, [o])
        g_w = nlp_ref_rows(x[n:n + 1], u[n:n + 1], x0[n:n + 1], yr[n:n + 1], ye[n:n + 1], kwo["Qd"], kwo["Rd"], kwo["QNd"], kw["lb"][n:n + 1],
                           kw["ub"][n:n + 1], DT, ERK_STEPS, kw["params"][n:n + 1])[3][0]
        g_p = nlp_ref_rows(x[n:n + 1], u[n:n + 1], x0[n:n + 1], yr[n:n + 1], ye[n:n + 1], kw["Qd"][n:n + 1], kw["Rd"][n:n + 1],
                           kw["QNd"][n:n + 1], kw["lb"][n:n + 1], kw["ub"][n:n + 1], DT, ERK_STEPS, kwo["params"])[3][0]
        assert np.abs(g_w - gu[n]).max() > 1e-3 and np.abs(g_p - gu[n]).max() > 1e-3


@pytest.mark.parametrize("N,box", LS_CASES)
def test_line_search_reference_on_composed_data(oracle, N, box):
    """make_data / ls_ref on the composed data, for the inputs of the GPU file's line-search test on the reference alone: from
    the hover start, iterations j = 1, 2 with the exact QP step as candidate, on the compared rows.  ties(...) stays under the
    5 % of the rows the GPU test allows; the step lengths are powers of the reduction and the penalty is finite."""
    case = het_case(oracle, N, box=box)
    rows = np.array(ROWS)
    d = take_rows(ls_data(case), rows)
    xs, us = hover_start(case)
    x, u, mu = xs[rows], us[rows], np.zeros(rows.size)
    for j in (1, 2):
        xh, uh = np.empty_like(x), np.empty_like(u)
        for n, i in enumerate(rows):
            _xr, _ur, _qp, ref = het_ref_step(oracle, case, i, x[n], u[n])
            assert ref["kkt"] <= 1e-12, (i, ref["kkt"])
            xh[n], uh[n] = x[n] + ref["dx"], u[n] + ref["du"]
        al, mu, (x, u), res, acc, mg = ls_ref((x, u), (xh, uh), mu, d)
        t = ties(mg)
        print(f"N {N} box {box} iteration {j}: alpha < 1 on {int((al < 1).sum())} of {rows.size} rows, ties {int(t.sum())}, "
              f"no trial accepted {int((~acc).sum())}, res eq / ineq {res[:, 1].max():.2e} / {res[:, 2].max():.2e}")
        assert t.sum() <= 0.05 * rows.size, t.sum()
        assert np.isfinite(mu).all() and (mu >= 0).all() and np.isfinite(res).all()
        assert (al <= 1.0).all() and (np.log2(al) == np.round(np.log2(al))).all()
