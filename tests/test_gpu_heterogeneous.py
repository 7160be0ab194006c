"""GPU suite: heterogeneous fleets.  Per-instance model parameters, per-instance weight rows, cost
scaling, erk_steps 2 and a box (per-stage or scalar) are in force TOGETHER on every solver of this file (_configure), at the
horizons where the engine's code paths change (tests/test_heterogeneous_cpu.py: EDGES), with 130 rows: two full 64-lane groups
plus two rows.  The case (het_case), its exact-QP reference (het_ref_step) and the checks that the case exercises what it is
meant to are in tests/test_heterogeneous_cpu.py; the references of the post-RTI evaluations are those of the features' own
suites, called with per-row data.  Every test prints the figures it saw."""
import numpy as np
import pytest

from test_gpu_nlp_eval import _compare
from test_gpu_sens import _check_against_ref, _engine
from test_gpu_sqp_ls import TOL as SQP_TOL
from test_gpu_sqp_ls import _maker, _one_iteration, _start_of
from test_heterogeneous_cpu import (B_HET, CHK, DT, EDGES, ERK_STEPS, LS_CASES, ROWS, SCALING, compose, het_case, het_reference, kst_of,
                                    last_active, ls_data, nlp_args)
from test_model_params_cpu import random_params
from test_nlp_eval_cpu import nlp_ref_rows
from test_weights_cpu import agree

pytestmark = pytest.mark.gpu
QP_TOL = 1e-11


def _configure(s, case, rows=None):
    """ALL of the heterogeneous data on a solver, fleet or multi-GPU fleet: parameter rows, weight rows, cost scaling,
    erk_steps and the box of the case (rows: the case's rows that the object holds, in its order; None: all)"""
    r = slice(None) if rows is None else np.asarray(rows)
    s.set_model_params(case["p"][r])
    s.set_weights_batch(case["W"][r], case["WN"][r])
    s.set_cost_scaling(*case["scaling"])
    s.set_erk_steps(case["erk_steps"])
    if case["box"] == "stages":
        s.set_box_stages(case["lb"][r], case["ub"][r])
    else:
        s.set_box(*case["scalar_box"])


def _solver(case, B=None, **kw):
    """a configured BatchSolver on the leading B rows of the case, at the case's pre-step iterate"""
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    B = case["B"] if B is None else B
    s = BatchSolver(B, default_opts(N=case["N"], tol=QP_TOL, **kw))
    _configure(s, case, np.arange(B))
    s.set_x0(case["x0"][:B]); s.set_yref(case["yref"][:B], case["yref_e"][:B]); s.set_iterate(case["x"][:B], case["u"][:B])
    return s


@pytest.fixture(scope="module")
def het_cache():
    return {}


def _ident(v):
    return ",".join(f"{k}={w}" for k, w in v.items()) or "default" if isinstance(v, dict) else str(v)


# ---- A. one RTI step against the exact QP -----------------------------------------------------------------------------------------
STEP_CASES = [(N, box, {}) for N in EDGES for box in ("stages", "scalar")] + [
    (40, "scalar", r) for r in (dict(as_passes=-1, forward_sweep=1),      # the monolithic k_as_w + the matrix-free k_forward_erk_par
                                dict(as_dense=1, forward_split=1), dict(as_dense=-1), dict(active_set=0), dict(step_graph=1))]


@pytest.mark.parametrize("N,box,route", STEP_CASES, ids=_ident)
def test_rti_step_matches_exact_qp(oracle, het_cache, N, box, route):
    """One RTI step of two solvers, B = 130 and B = 128, on the same leading rows: every compared row (range(0, B, 3)) has
    status 0 and agrees with the exact QP of ITS parameters, scaled weights and box (1e-8 on the active-set routes, 5e-6 for the
    interior point; oracle.solve_qp_refined is the referee); x_0 = x0 exactly and the box to 1e-9 on every row."""
    case, ref = het_reference(oracle, het_cache, N, box)
    tol = 5e-6 if route.get("active_set", 1) == 0 else 1e-8
    worst, n, n_con, n_feas = 0.0, 0, 0, 0
    for B in (B_HET, B_HET - 2):
        s = _solver(case, B, **route)
        s.solve(1)
        xg, ug = s.get_iterate()
        st, it, _res = s.stats()
        s.close()
        assert np.array_equal(xg[:, 0], case["x0"][:B])
        assert (ug >= case["lb"][:B] - 1e-9).all() and (ug <= case["ub"][:B] + 1e-9).all(), (B, (case["lb"][:B] - ug).max(), (ug - case["ub"][:B]).max())
        for i in ROWS:
            if i >= B:
                continue
            xr, ur, qp, _referee = ref[i]
            assert st[i] == 0, (B, i, st[i])
            e = agree(oracle, xg[i], ug[i], xr, ur, qp, case["x"][i], case["u"][i], tol)
            worst = max(worst, e)
            assert e <= tol, (B, i, e)
            n += 1
            n_con += int(it[i] > 0)
            n_feas += int(it[i] == 0)
    print(f"N {N} box {box} route {_ident(route)}: {n} compared, worst {worst:.2e}, constrained {n_con}, feasible {n_feas}")
    # (both kinds of rows are in: the shares of tests/test_heterogeneous_cpu.py, a quarter constrained and two free, per solver)
    assert n == 2 * len(ROWS) - 1 and n_con >= n // 4 and n_feas >= 2


# ---- B. row independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ah", [0, 1])
@pytest.mark.parametrize("box", ["stages", "scalar"])
@pytest.mark.parametrize("N", [8, 33])
def test_rows_independent_under_permutation(oracle, N, box, ah):
    """Permuting the 130 rows together with ALL their data permutes the outputs: bitwise with full-horizon sweeps, to 1e-9 with
    the active horizon (the head is a wave-level maximum).  A weight or parameter read from a wave-mate's row fails here even
    where parity on sampled rows would miss it."""
    case = het_case(oracle, N, box=box)
    perm = np.random.default_rng(90 + N + ah).permutation(B_HET)
    pc = dict(case)
    for k in ("p", "W", "WN", "lb", "ub", "x0", "yref", "yref_e", "x", "u"):
        pc[k] = case[k][perm]
    outs = []
    for c in (case, pc):
        s = _solver(c, active_horizon=ah)
        s.solve(1)
        outs.append(s.get_iterate() + tuple(s.stats()))
        s.close()
    (xa, ua, sa, ia, ra), (xb, ub, sb, ib, rb) = outs
    ex, eu = np.abs(xa[perm] - xb).max(), np.abs(ua[perm] - ub).max()
    print(f"N {N} box {box} active_horizon {ah}: constrained {int((ib > 0).sum())} of {B_HET}, status counts {np.bincount(sb)}, "
          f"|x| {ex:.2e} |u| {eu:.2e}")
    assert (ib > 0).sum() >= B_HET // 4 and (sb == 0).all()
    assert np.array_equal(sa[perm], sb)
    if ah == 0:
        assert np.array_equal(xa[perm], xb) and np.array_equal(ua[perm], ub) and np.array_equal(ia[perm], ib)
    else:
        assert ex <= 1e-9 and eu <= 1e-9, (ex, eu)
        assert ((ia[perm] > 0) == (ib > 0)).all()


# ---- C. NLP evaluation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,box", [(N, "stages") for N in EDGES] + [(8, "scalar")])
def test_nlp_evaluation(oracle, N, box):
    """k_nlp_eval_par with weight rows: cost, residuals, costates and reduced gradient against nlp_ref_rows on the composed data,
    at the hover iterate and after one RTI step (tolerances: _compare's own)"""
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    case = het_case(oracle, N, box=box)
    (x0, yref, yref_e), kw = nlp_args(case)
    s = _solver(case)
    s.init_iterate(INIT_HOVER)
    _compare(s, oracle, x0, yref, yref_e, f"box {box}, hover start", **kw)
    s.solve(1)
    _c, res, _pi, _gu = _compare(s, oracle, x0, yref, yref_e, f"box {box}, one RTI step", **kw)
    _x, u = s.get_iterate()
    on_box = ((u <= case["lb"] + 1e-9) | (u >= case["ub"] - 1e-9)).reshape(B_HET, -1).any(1)
    print(f"  rows with inputs on the box: {int(on_box.sum())} of {B_HET}; res_ineq {res[:, 2].max():.2e}")
    assert on_box.sum() >= B_HET // 4
    s.close()


# ---- D. SQP check and line search ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,box", LS_CASES)
def test_line_search_iterations(oracle, N, box):
    """iterations j = 1, 2 of a globalised solve against ls_ref on the composed data (k_sqp_check_par, k_sqp_ls_par with weight
    rows): the rule of tests/test_gpu_sqp_ls.py -- iterates to 1e-9, step lengths exactly off ties, ties at most 5 % of the rows"""
    case = het_case(oracle, N, box=box)
    make = _maker(case["x0"], case["yref"], case["yref_e"], lambda s: _configure(s, case), N=N, tol=QP_TOL)
    stepper, prev = _start_of(make)
    for j in (1, 2):
        prev, n_short = _one_iteration(make, ls_data(case), j, prev, stepper, f"heterogeneous N {N} box {box}")


def test_globalised_solve_converges_to_kkt_points(oracle):
    """One globalised solve to convergence at N = 17 (stage boxes): at least a quarter of the rows end with status 0, and
    nlp_ref_rows -- the CPU reference, not the engine -- at the returned iterate gives res_eq, res_ineq <= 1e-9 and
    res_stat <= 8e-7 on those rows: 1e-7 is test_gpu_nlp_eval.test_agreement_with_solve_sqp's bound at the same tolerances, the
    gradient is linear in the weights and 8 = 4 x 2 is the largest factor by which a row's scaled weights exceed the defaults.
    As seen on the MI355X: see DESIGN.md section 5.18."""
    N = 17
    case = het_case(oracle, N)
    make = _maker(case["x0"], case["yref"], case["yref_e"], lambda s: _configure(s, case), N=N, tol=QP_TOL)
    s = make(True)
    n = s.solve_sqp(100, SQP_TOL, SQP_TOL, SQP_TOL)
    st, it, rs = s.sqp_stats()
    x, u = s.get_iterate()
    s.close()
    conv = np.flatnonzero(st == 0)
    assert conv.size >= B_HET / 4, np.bincount(st, minlength=5)
    (x0, yref, yref_e), kw = nlp_args(case, conv)
    _cost, res, _pi, _gu = nlp_ref_rows(x[conv], u[conv], x0, yref, yref_e, kw["Qd"], kw["Rd"], kw["QNd"], kw["lb"], kw["ub"], DT, kw["M"],
                                        kw["params"])
    print(f"globalised solve, N {N}: iterations {n}, status counts {np.bincount(st, minlength=5)}, converged share "
          f"{conv.size / B_HET:.2f}; reference at the returned iterate: res_stat {res[:, 0].max():.3e} (row {conv[res[:, 0].argmax()]}), "
          f"res_eq {res[:, 1].max():.3e}, res_ineq {res[:, 2].max():.3e}")
    assert (res[:, 1] <= 1e-9).all() and (res[:, 2] <= 1e-9).all(), (res[:, 1].max(), res[:, 2].max())
    assert (res[:, 0] <= 8 * 1e-7).all(), (conv[res[:, 0] > 8e-7], res[:, 0].max())


# ---- E. sensitivities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,box", [(N, "scalar") for N in (5, 8, 9, 17, 24, 25, 33)] + [(17, "stages")])
def test_sensitivities(oracle, N, box):
    """solve(1) + eval_sens_x0 with all the data in force: every row against sens_ref on the engine's own blocks and active set
    with THAT row's scaled weights (test_gpu_sens._check_against_ref, its TOL); at least 20 % of the rows have an active input;
    rows whose masked sweep starts at a checkpoint AND rows whose sweep starts at N both occur."""
    case = het_case(oracle, N, box=box)
    s = _solver(case)
    s.solve(1)
    s.eval_sens_x0()
    du, dx, act = _engine(s)
    status, _, _ = s.stats()
    n = sum(_check_against_ref(s, du, dx, act, status, (case["Qd"][i], case["Rd"][i], case["QNd"][i]), rows=[i]) for i in range(B_HET))
    s.close()
    last = np.array([last_active(act[i]) for i in range(B_HET)])
    kst = np.array([kst_of(l, N) for l in last[last >= 0]])
    share = float((last >= 0).mean())
    print(f"N {N} box {box}: {n} rows checked, active share {share:.2f}, kst counts "
          f"{dict(zip(*(v.tolist() for v in np.unique(kst, return_counts=True))))}")
    assert n == B_HET, (n, np.bincount(status))                # (no row failed: a status-4 row holds NaN and is not compared)
    assert share >= 0.2, share
    assert (kst < N).any() and (kst == N).any(), np.unique(kst)
    assert set(kst[kst < N].tolist()) <= set(CHK)


def test_sensitivities_refused_after_each_setter(oracle):
    """after set_weights_batch, set_model_params, set_cost_scaling or set_erk_steps -- the others already in force -- a getter
    without a new evaluation is refused (the rule of tests/test_gpu_sens.py::test_refusals)"""
    from crazyflie_nmpc_amd.solver import CfnmpcError
    case = het_case(oracle, 8)
    s = _solver(case)
    rng = np.random.default_rng(3)
    changes = [lambda: s.set_weights_batch(case["W"][::-1].copy(), None), lambda: s.set_model_params(random_params(rng, B_HET)),
               lambda: s.set_cost_scaling(1.0, 3.0), lambda: s.set_erk_steps(3)]
    for change in changes:
        s.solve(1)
        s.eval_sens_x0()
        s.sens_x0(0)
        s.sens_active()
        change()
        with pytest.raises(CfnmpcError):
            s.sens_x0(0)
        with pytest.raises(CfnmpcError):
            s.sens_active()
    s.solve(1)
    s.eval_sens_x0()
    s.sens_x0(0)
    s.close()


# ---- F. fleet and multi -------------------------------------------------------------------------------------------------------------
def test_fleet_equals_its_buckets(oracle):
    """A MixedHorizonFleet of 26 vehicles with horizons from EDGES (shuffled), everything set through the fleet: solve(2),
    eval_nlp, eval_sens_x0 and a globalised solve_sqp(5) equal, bit for bit, single solvers per bucket given the same rows (the
    pattern of tests/test_gpu_sqp_ls.py::test_fleet_equals_its_buckets): every setter scatters to the right bucket rows when
    all are used at once.
    (This test found the unordered zero-fill of buffers allocated at first use: DESIGN.md section 5.18.)"""
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    rng = np.random.default_rng(2026)
    hz = np.resize(np.array(EDGES), 26)[rng.permutation(26)]
    B, Nmax, Nmin = hz.size, max(EDGES), min(EDGES)
    p = random_params(rng, B)
    W = oracle.W_DIAG * np.exp(rng.uniform(np.log(0.25), np.log(4.0), (B, 17)))
    WN = oracle.QN_DIAG * np.exp(rng.uniform(np.log(0.25), np.log(4.0), (B, 13)))
    lb = rng.uniform(0.0, 4.0, (B, Nmax, 4)); ub = rng.uniform(19.0, 22.0, (B, Nmax, 4))
    x0 = oracle.sample_hover_x0(rng, B, scale=1.0)
    x0[:, 7:10] += rng.normal(0, 1.0, (B, 3))
    case = compose(oracle, p, W, WN, SCALING, lb, ub, x0, ERK_STEPS)

    def run(o, sens_stages):
        o.init_iterate(INIT_HOVER)
        o.solve(2)
        out = list(o.stats())
        o.eval_nlp()
        out += list(o.nlp_stats())
        o.eval_sens_x0()
        out += [o.sens_x0(0, sens_stages)[0], o.sens_x0(0, sens_stages + 1)[1]]
        o.set_sqp_globalization("merit_backtracking")
        out.append(np.array(o.solve_sqp(5, SQP_TOL, SQP_TOL, SQP_TOL)))
        return out + list(o.sqp_stats()) + list(o.sqp_ls_stats())

    f = MixedHorizonFleet(hz, tol=QP_TOL)
    _configure(f, case)
    f.set_x0(x0); f.set_yref(case["yref"], case["yref_e"])
    assert f.Nmin == Nmin and f.Nmax == Nmax and len(f.buckets()) == len(EDGES)
    fo = run(f, Nmin)
    n_it = 0
    print(f"fleet: status {fo[0].tolist()}  qp_iter {fo[1].tolist()}  sqp status {fo[8].tolist()}  n_short {fo[13].tolist()}")
    assert (fo[1] > 0).sum() >= B // 4 and (fo[0] == 0).all()
    for N, idx, xb, ub_ in f.bucket_iterates():
        assert (hz[idx] == N).all()
        s = BatchSolver(idx.size, default_opts(N=N, tol=QP_TOL))
        sub = dict(case, lb=lb[:, :N], ub=ub[:, :N])
        _configure(s, sub, idx)
        s.set_x0(x0[idx]); s.set_yref(case["yref"][idx, :N].copy(), case["yref_e"][idx])
        so = run(s, Nmin)
        for k, (a, b) in enumerate(zip(fo, so)):
            if k == 7:
                n_it = max(n_it, int(b))                                                  # (iterations run: the longest bucket's)
                continue
            assert np.array_equal(a[idx], b), (N, k)
        x, u = s.get_iterate()
        assert np.array_equal(xb, x) and np.array_equal(ub_, u), N
        s.close()
    assert int(fo[7]) == n_it
    f.close()


@pytest.mark.parametrize("N,box", [(8, "scalar"), (33, "stages")])
def test_multi_equals_one_solver(oracle, N, box):
    """An in-process MultiGpuFleet over two shards of one device, everything set through cfnmpc_multi_*, against ONE solver of
    the 130 rows: RTI steps, eval_nlp and the sensitivities, bit for bit (full-horizon sweeps: a vehicle's arithmetic does not
    depend on its neighbours, as in tests/test_gpu_model_params.py::test_fleet_and_multi_match_single_solvers).
    (At [33-stages] this test found the unordered zero-fill of buffers allocated at first use: DESIGN.md section 5.18.)"""
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    from crazyflie_nmpc_amd.parallel import MultiGpuFleet
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    case = het_case(oracle, N, box=box)
    opts = default_opts(N=N, tol=QP_TOL, active_horizon=0)
    m, s = MultiGpuFleet(B_HET, [0, 0], opts), BatchSolver(B_HET, opts)
    assert [(lo, hi) for lo, hi, _d in m.shards()] == [(0, 65), (65, 130)]
    for o in (m, s):
        _configure(o, case)
        o.set_x0(case["x0"]); o.set_yref(case["yref"], case["yref_e"]); o.init_iterate(INIT_HOVER)
        o.solve(2)
    m.sync()
    xs, us = s.get_iterate()
    for a, b in zip(m.stats(), s.stats()):
        assert np.array_equal(a, b)
    for k in range(N):
        assert np.array_equal(m.get_u(k), us[:, k]) and np.array_equal(m.get_x(k + 1), xs[:, k + 1]), k
    m.eval_nlp(); s.eval_nlp()
    for a, b in zip(m.nlp_stats(), s.nlp_stats()):
        assert np.array_equal(a, b)
    m.eval_sens_x0(); s.eval_sens_x0()
    mu, _ = m.sens_x0(0, N)
    _, mx = m.sens_x0(0, N + 1)
    su, sx, act = _engine(s)
    print(f"multi N {N} box {box}: constrained {int((s.stats()[1] > 0).sum())} of {B_HET}, rows with an active input "
          f"{int((act != 0).any(axis=(1, 2)).sum())}, |du| differs by {np.abs(mu - su).max():.2e}, |dx| by {np.abs(mx - sx).max():.2e}")
    assert (s.stats()[1] > 0).sum() >= B_HET // 4
    assert np.array_equal(mu, su) and np.array_equal(mx, sx)
    m.close(); s.close()
