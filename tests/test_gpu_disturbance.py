"""GPU suite: per-instance disturbance model, disturbed plant and observer (include/cfnmpc.h: cfnmpc_set_disturbance,
cfnmpc_sim_dist, cfnmpc_estimate_disturbance).

The reference is the numpy restatement of tests/test_disturbance_cpu.py (f(x, u, p, d), complex-step Jacobians, M-step RK4
sensitivities, the observer), checked there against central differences and against the parameter row with more gravity.  One
RTI step is compared with oracle.qp_from_blocks + oracle.solve_qp_dense on those blocks, oracle.solve_qp_refined being the
referee where the two FP64 sides disagree (as tests/test_gpu_model_params.py does)."""
import numpy as np
import pytest

from test_disturbance_cpu import ND, observe, random_dist, rk4, rk4_sens
from test_gpu_model_params import _agree, _closed_loop, _inputs, _weights
from test_model_params_cpu import NOMINAL, hover, random_params

pytestmark = pytest.mark.gpu
DT = 0.015
QP_TOL = 1e-11


def _solver(B, M=1, p=None, d=None, **kw):
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    s = BatchSolver(B, default_opts(**kw))
    if M != 1:
        s.set_erk_steps(M)
    if p is not None:
        s.set_model_params(p)
    if d is not None:
        s.set_disturbance(d)
    return s


def _blocks(x, u, p, d, M):
    N = u.shape[0]
    A = np.empty((N, 13, 13)); Bm = np.empty((N, 13, 4)); b = np.empty((N, 13))
    for k in range(N):
        phi, A[k], Bm[k] = rk4_sens(x[k], u[k], p, d, DT, M)
        b[k] = phi - x[k + 1]
    return A, Bm, b


def _ref_step(oracle, x, u, x0, yref, yref_e, p, d, M, W, WN, u_min=0.0, u_max=22.0):
    A, Bm, b = _blocks(x, u, p, d, M)
    q = np.empty((x.shape[0], 13))
    q[:-1] = W[:13] * (x[:-1] - yref[:, :13])
    q[-1] = WN * (x[-1] - yref_e)
    r = W[13:] * (u - yref[:, 13:])
    qp = oracle.qp_from_blocks(A, Bm, b, q, r, x0 - x[0], W[:13], W[13:], WN, u_min - u, u_max - u)
    sol = oracle.solve_qp_dense(qp)
    return x + sol["dx"], u + sol["du"], qp


def _iterate(oracle, rng, B, N, p, seed):
    x0, yr, ye = _inputs(oracle, B, N, seed, scale=1.5)
    x = np.repeat(x0[:, None, :], N + 1, 1) + rng.normal(0, 0.05, (B, N + 1, 13))
    x[:, :, 3:7] /= np.linalg.norm(x[:, :, 3:7], axis=2, keepdims=True)
    u = hover(p)[:, None, None] + rng.normal(0, 2.0, (B, N, 4))
    return x0, yr, ye, x, u


def _lin(s, x0, yr, ye, x, u):
    s.set_x0(x0); s.set_yref(yr, ye); s.set_iterate(x, u)
    s.linearise_only()
    return s.get_linearisation()


def _rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


# ---- 1. blocks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("B,N", [(200, 50), (37, 5)])
def test_blocks_match_reference(oracle, B, N, M):
    """B = 200: the last wave partial; B = 37, N = 5: fewer instances than a wave, every interval in its own workgroup"""
    rng = np.random.default_rng(140 + M + N)
    p = random_params(rng, B)
    d = random_dist(rng, B)
    x0, yr, ye, x, u = _iterate(oracle, rng, B, N, p, 3 + M)
    s = _solver(B, M, p, d, N=N)
    assert np.array_equal(s.disturbance(), d)
    A, Bm, b = _lin(s, x0, yr, ye, x, u)
    for i in list(rng.choice(B - 8, 16, replace=False)) + list(range(B - 8, B)):
        Ar, Br, br = _blocks(x[i], u[i], p[i], d[i], M)
        assert np.abs(A[i] - Ar).max() <= 1e-12 * max(1.0, np.abs(Ar).max()), (i, np.abs(A[i] - Ar).max())
        assert np.abs(Bm[i] - Br).max() <= 1e-12 * max(1.0, np.abs(Br).max()), (i, np.abs(Bm[i] - Br).max())
        assert np.abs(b[i] - br).max() <= 1e-12 * max(1.0, np.abs(x[i]).max()), (i, np.abs(b[i] - br).max())


# ---- 2. gravity equivalence ------------------------------------------------------------------------------------------
def test_vertical_acceleration_is_more_gravity(oracle):
    B, N = 200, 50
    rng = np.random.default_rng(61)
    delta = rng.uniform(-1.0, 1.0, B)
    d = np.zeros((B, ND)); d[:, 2] = -delta
    pg = np.tile(NOMINAL, (B, 1)); pg[:, 0] += delta
    x0, yr, ye, x, u = _iterate(oracle, rng, B, N, pg, 5)
    dist = _lin(_solver(B, d=d), x0, yr, ye, x, u)              # (no parameter rows: the internal nominal table)
    grav = _lin(_solver(B, p=pg), x0, yr, ye, x, u)
    for a, b in zip(dist, grav):
        assert _rel(a, b) <= 1e-12, _rel(a, b)
    assert _rel(dist[2], _lin(_solver(B), x0, yr, ye, x, u)[2]) > 1e-4   # (and the rows matter)


# ---- 3. zero rows ----------------------------------------------------------------------------------------------------
def test_zero_rows_are_the_par_path(oracle):
    """Blocks: random parameter rows.  Closed loop: the loop of section 5.13 whose 1e-9 this bound is -- nominal rows, so that
    the model matches the plant of _closed_loop (oracle.rk4).  Measured: 3.0e-10 after 20 steps.  With RANDOM rows against that
    nominal plant (mass off by up to 30 %, two thirds of the rows at the box) the same 4e-11 after the first step doubles from
    step to step, 6.6e-7 after 20, with the interior point solved to 1e-8 or to 1e-11 alike: the loop amplifies, the kernels
    agree (blocks to 1e-13, two _par runs bitwise)."""
    B, N = 512, 50
    rng = np.random.default_rng(62)
    p = random_params(rng, B)
    x0, yr, ye, x, u = _iterate(oracle, rng, B, N, p, 21)
    par = _lin(_solver(B, p=p), x0, yr, ye, x, u)
    dst = _lin(_solver(B, p=p, d=np.zeros((B, ND))), x0, yr, ye, x, u)
    for a, b in zip(dst, par):
        assert _rel(a, b) <= 1e-13, _rel(a, b)
    pn = np.tile(NOMINAL, (B, 1))
    ra = _closed_loop(_solver(B, p=pn), oracle, x0, yr, ye, 20, 5)
    rb = _closed_loop(_solver(B, p=pn, d=np.zeros((B, ND))), oracle, x0, yr, ye, 20, 5)
    worst = 0.0
    for p_, q_ in zip(ra, rb):
        for v, w in zip(p_[:3], q_[:3]):
            worst = max(worst, np.abs(v - w).max())
    print(f"zero rows vs _par over 20 kicked steps: max |diff| = {worst:.3e}")
    assert worst <= 1e-9
    # back to NULL: bitwise the solver that never had rows (without and with parameter rows)
    for pp in (None, p):
        s = _solver(B, p=pp, d=random_dist(rng, B))
        s.set_disturbance(None)
        assert np.array_equal(s.disturbance(), np.zeros((B, ND)))
        rc = _closed_loop(s, oracle, x0, yr, ye, 6, 5)
        for p_, q_ in zip(_closed_loop(_solver(B, p=pp), oracle, x0, yr, ye, 6, 5), rc):
            for v, w in zip(p_, q_):
                assert np.array_equal(v, w)


# ---- 4. one RTI step per route ---------------------------------------------------------------------------------------
ROUTES = [dict(), dict(forward_sweep=1), dict(forward_split=1), dict(active_set=0), dict(M=2), dict(step_graph=1)]


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: ",".join(f"{k}={v}" for k, v in r.items()) or "default")
def test_rti_step_matches_reference(oracle, route):
    route = dict(route)
    M = route.pop("M", 1)
    graph = route.get("step_graph", 0)
    B, N = 1024, 50
    rng = np.random.default_rng(170)
    p = random_params(rng, B)
    d = random_dist(rng, B)
    x0, yr, ye = _inputs(oracle, B, N, 11, scale=1.5)
    yr[:, :, 13:] = hover(p)[:, None, None]
    x0[:, 7:10] += rng.normal(0, 1.5, (B, 3))                      # kicks: a good share of the rows hit the box
    x = np.repeat(x0[:, None, :], N + 1, 1)
    u = np.repeat(np.repeat(hover(p)[:, None, None], N, 1), 4, 2)
    s = _solver(B, M, p, tol=QP_TOL, **route)
    s.set_x0(x0); s.set_yref(yr, ye)
    if graph:
        # both parities of the step graph are captured with OTHER rows; the replay below must use the new ones
        s.set_disturbance(random_dist(rng, B))
        s.set_iterate(x, u)
        for _ in range(4):   # (two captures, two replays)
            s.solve(1)
    s.set_disturbance(d)
    s.set_iterate(x, u)
    s.solve(1)
    st, _, _ = s.stats()
    xg, ug = s.get_iterate()
    W, WN = _weights()
    rows = rng.choice(B, 24, replace=False)
    n_con = 0
    for i in rows:
        xr, ur, qp = _ref_step(oracle, x[i], u[i], x0[i], yr[i], ye[i], p[i], d[i], M, W, WN)
        n_con += int((ur <= 1e-9).any() or (ur >= 22.0 - 1e-9).any())
        assert st[i] == 0, (i, st[i])
        assert _agree(oracle, xg[i], ug[i], xr, ur, qp, x[i], u[i], 1e-8) <= 1e-8, i
    assert n_con >= 0.2 * len(rows), n_con


# ---- 5. row independence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ah", [0, 1])
def test_rows_independent_under_permutation(oracle, ah):
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B, N = 2048, 50
    rng = np.random.default_rng(190 + ah)
    p = random_params(rng, B)
    d = random_dist(rng, B)
    x0, yr, ye = _inputs(oracle, B, N, 12, scale=1.5)
    x0[:, 7:10] += rng.normal(0, 1.5, (B, 3))
    perm = rng.permutation(B)
    outs = []
    for pi in (np.arange(B), perm):
        s = _solver(B, p=p[pi], d=d[pi], active_horizon=ah, tol=QP_TOL)
        s.set_x0(x0[pi]); s.set_yref(yr[pi], ye[pi]); s.init_iterate(INIT_HOVER)
        s.solve(1)
        st, it, _ = s.stats()
        xg, ug = s.get_iterate()
        outs.append((xg, ug, st, it))
        s.close()
    (xa, ua, sa, ia), (xb, ub, sb, ib) = outs
    assert (ia[perm] > 0).sum() > B // 10                             # constrained rows are in
    assert np.array_equal(sa[perm], sb)
    if ah == 0:
        assert np.array_equal(xa[perm], xb) and np.array_equal(ua[perm], ub) and np.array_equal(ia[perm], ib)
    else:
        for k in (0, 1):
            assert np.abs(ua[perm][:, k] - ub[:, k]).max() < 1e-8
        assert np.abs(xa[perm][:, 4] - xb[:, 4]).max() < 1e-8
        assert ((ia[perm] > 0) == (ib > 0)).all()


# ---- 6. plant and observer -------------------------------------------------------------------------------------------
def test_sim_dist_matches_reference(oracle):
    import torch
    from crazyflie_nmpc_amd import sim
    B = 300
    rng = np.random.default_rng(18)
    p = random_params(rng, B)
    d = random_dist(rng, B)
    x = oracle.sample_hover_x0(rng, B, scale=1.5)
    u = hover(p)[:, None] + rng.normal(0, 2.0, (B, 4))
    for pp in (p, None):
        ref = np.stack([rk4(x[i], u[i], NOMINAL if pp is None else pp[i], d[i], 0.06, 4) for i in range(B)])
        xn = sim(x, u, 0.06, 4, params=pp, dist=d)
        assert np.abs(xn - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
        xt = sim(torch.tensor(x, device="cuda"), torch.tensor(u, device="cuda"), 0.06, 4,
                 params=None if pp is None else torch.tensor(pp, device="cuda"), dist=torch.tensor(d, device="cuda"))
        assert np.array_equal(xt.cpu().numpy(), xn)
    assert np.abs(sim(x, u, 0.06, 4, params=p, dist=np.zeros((B, ND))) - sim(x, u, 0.06, 4, params=p)).max() <= 1e-14 * 2.0


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_observer_matches_restatement_and_converges(oracle, device):
    import torch
    from crazyflie_nmpc_amd import estimate_disturbance, sim
    B, T = 300, DT
    rng = np.random.default_rng(19)
    p = random_params(rng, B)
    d_true = random_dist(rng, B)
    x = oracle.sample_hover_x0(rng, B, scale=1.0)

    def dev(a):
        return torch.tensor(a, device="cuda") if device else a

    def host(a):
        return a.cpu().numpy() if device else a

    for gain, steps, chained in ((0.7, 10, True), (0.5, 40, False)):
        d_g = dev(np.zeros((B, ND)))
        d_r = np.zeros((B, ND))
        xc = x.copy()
        for _ in range(steps):
            u = hover(p)[:, None] + rng.normal(0, 1.0, (B, 4))
            xn = sim(xc, u, T, 1, params=p, dist=d_true)
            out = estimate_disturbance(dev(xc), dev(u), dev(xn), d_g, T, 1, gain, 0.5 * gain + 0.25, params=dev(p))
            assert out is d_g                                                    # in place
            if chained:   # ten chained steps against the numpy restatement, fed the same measurements
                d_r = np.stack([observe(xc[i], u[i], xn[i], p[i], d_r[i], T, 1, gain, 0.5 * gain + 0.25) for i in range(B)])
                assert np.abs(host(d_g) - d_r).max() <= 1e-12 * max(1.0, np.abs(d_r).max())
            xc = xn
        if not chained:   # noise-free disturbed plant, gain 0.5 for both parts: 40 steps
            assert np.abs(host(d_g) - d_true).max() <= 1e-9, np.abs(host(d_g) - d_true).max()


# ---- 7. NLP consistency ----------------------------------------------------------------------------------------------
def test_nlp_residuals_and_sqp_follow_the_disturbed_dynamics(oracle):
    B, N, TOL = 48, 50, 1e-6
    rng = np.random.default_rng(23)
    p = random_params(rng, B)
    d = random_dist(rng, B)
    d[:, :3] = rng.choice([-1.0, 1.0], (B, 3)) * rng.uniform(0.5, 2.0, (B, 3))
    a_min = np.abs(d[:, :3]).max(axis=1).min()
    x0, yr, ye = _inputs(oracle, B, N, 31, scale=0.5)
    yr[:, :, 13:] = hover(p)[:, None, None]
    u = hover(p)[:, None, None] + rng.normal(0, 0.5, (B, N, 4))
    x = np.empty((B, N + 1, 13)); x[:, 0] = x0
    for i in range(B):
        for k in range(N):
            x[i, k + 1] = rk4(x[i, k], u[i, k], p[i], d[i], DT)
    for M in (1, 2):
        s = _solver(B, M, p, d)
        s.set_x0(x0); s.set_yref(yr, ye)
        xm = x
        if M == 2:
            xm = x.copy()
            for i in range(4):
                for k in range(N):
                    xm[i, k + 1] = rk4(xm[i, k], u[i, k], p[i], d[i], DT, 2)
        s.set_iterate(xm, u)
        s.eval_nlp()
        res = s.nlp_stats()[1]
        rows = slice(0, 4) if M == 2 else slice(None)
        assert res[rows, 1].max() <= 1e-12, res[rows, 1].max()
        s.set_disturbance(None)
        s.eval_nlp()
        # the velocity defect is dt R(q)' a_w to first order: its largest entry is at least dt |a_w|_2 / sqrt(3) > 0.5 dt |a_w|_inf
        assert s.nlp_stats()[1][rows, 1].min() >= 0.5 * DT * a_min
    # Full SQP solve.  Gauss-Newton steps do not converge under a sizeable world-frame acceleration: the numpy reference SQP (the QP
    # of oracle.qp_from_blocks on the reference blocks, full steps, 100 iterations, tolerances 1e-6) ends with status 2 on 19 of
    # the 48 rows above -- the same 19 rows as cfnmpc_solve_sqp -- on 3 of 32 rows with |a| in [0.1, 0.5] and on 1 of 32 with |a|
    # in [0.1, 0.3], whatever al is (a = 0, |al| <= 2: every row in at most 41 iterations).  So the draw is narrowed to where the
    # reference converges on every row: |a| in [0.05, 0.15] per axis, |al| <= 2, where it needs 7 .. 68 iterations.
    B, rng = 32, np.random.default_rng(23)
    p = random_params(rng, B)
    d = random_dist(rng, B, 0.15, 2.0)
    d[:, :3] = rng.choice([-1.0, 1.0], (B, 3)) * rng.uniform(0.05, 0.15, (B, 3))
    x0, yr, ye = _inputs(oracle, B, N, 31, scale=0.5)
    yr[:, :, 13:] = hover(p)[:, None, None]
    for mode in ("full_step", "merit_backtracking"):
        s = _solver(B, 1, p, d, tol=QP_TOL)
        s.set_sqp_globalization(mode)
        s.set_x0(x0); s.set_yref(yr, ye); s.set_iterate(np.repeat(x0[:, None, :], N + 1, 1), yr[:, :, 13:].copy())
        s.solve_sqp(100, TOL, TOL, TOL)
        st, it, rs = s.sqp_stats()
        print(f"solve_sqp {mode}: status counts {np.bincount(st, minlength=5).tolist()}, iterations {it.min()} .. {it.max()}")
        assert (st == 0).all(), (mode, st)
        xg, ug = s.get_iterate()
        for i in range(B):
            eq = max(np.abs(xg[i, k + 1] - rk4(xg[i, k], ug[i, k], p[i], d[i], DT)).max() for k in range(N))
            assert eq <= TOL and rs[i, 1] <= TOL, (i, eq, rs[i, 1])
        # the solve used the rows: under the undisturbed model the same iterate has a defect of the order dt |a|
        s.set_disturbance(None)
        s.eval_nlp()
        assert s.nlp_stats()[1][:, 1].min() >= 0.5 * DT * np.abs(d[:, :3]).max(axis=1).min()


# ---- 8. offset-free closed loop --------------------------------------------------------------------------------------
def test_offset_free_closed_loop():
    """256 vehicles in a constant wind with a torque bias (plant = sim(dist=d_true): a_x, a_y in +-[0.4, 0.8] m/s^2, a_z in
    +-[0, 0.3], al in +-[0, 1.5] rad/s^2), 200 steps of regulation from the reference point.  (a) the nominal controller keeps a
    constant position offset (a pure tracking least-squares cost has no integral action); (b) the controller fed every step by
    estimate_disturbance(gain 0.5) -> set_disturbance(device rows), starting from d^ = 0, removes it.
    Thresholds from the numpy reference loop on the CPU (the QP of oracle.qp_from_blocks on tests/test_disturbance_cpu.py's
    blocks, 200 steps, plant = rk4 with d_true, observer = observe) at four corner rows of the draw, |position error| at the end:
        d_true = ( 0.4,  0.4,  0  ;  0  ,  0  ,  0  ):   (a) 1.62e-2 m    (b) 2.6e-5 m
        d_true = ( 0.8, -0.8,  0.3;  1.5, -1.5,  1.5):   (a) 3.51e-2 m    (b) 3.9e-4 m
        d_true = (-0.8,  0.8, -0.3; -1.5,  1.5, -1.5):   (a) 3.47e-2 m    (b) 5.4e-4 m
        d_true = ( 0.4, -0.4,  0.3;  1.5,  1.5,  0  ):   (a) 2.16e-2 m    (b) 4.8e-4 m
    (the residue of (b) is the altitude: the input reference stays at the nominal hover speed, which a_z shifts).  So: every
    status 0, every row of (b) within 1 mm of the target, the median of (a) at least 1 cm and at least 10 x the maximum of (b)."""
    import torch
    from crazyflie_nmpc_amd import estimate_disturbance, sim
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B, N, STEPS = 256, 50, 200
    rng = np.random.default_rng(12)
    sg = lambda n: rng.choice([-1.0, 1.0], (B, n))   # noqa: E731
    d_true = np.concatenate([sg(2) * rng.uniform(0.4, 0.8, (B, 2)), sg(1) * rng.uniform(0.0, 0.3, (B, 1)),
                             sg(3) * rng.uniform(0.0, 1.5, (B, 3))], axis=1)
    yr1 = np.zeros((N, 17)); yr1[:, 2] = 0.4; yr1[:, 3] = 1.0; yr1[:, 13:] = hover(NOMINAL)
    yr = np.tile(yr1, (B, 1, 1))
    ye = np.tile(yr1[0, :13], (B, 1))
    x0 = ye.copy()
    dt_ = torch.tensor(d_true, device="cuda")
    err = {}
    for ctrl in ("nominal", "observer"):
        s = _solver(B)
        s.set_x0(x0); s.set_yref(yr, ye); s.init_iterate(INIT_HOVER)
        x = torch.tensor(x0, device="cuda")
        u0 = torch.empty((B, 4), dtype=torch.float64, device="cuda")
        dh = torch.zeros((B, ND), dtype=torch.float64, device="cuda")
        ok = True
        for _ in range(STEPS):
            s.set_x0(x)
            s.solve(1)
            s.get_u(0, out=u0)
            xn = sim(x, u0, DT, 1, dist=dt_)
            if ctrl == "observer":
                estimate_disturbance(x, u0, xn, dh, DT, 1, 0.5, 0.5)
                s.set_disturbance(dh)
            x = xn
            ok = ok and bool((s.stats()[0] == 0).all())
        assert ok
        err[ctrl] = np.linalg.norm(x[:, :3].cpu().numpy() - np.array([0.0, 0.0, 0.4]), axis=1)
        if ctrl == "observer":
            print("estimate error after %d steps: %.3e" % (STEPS, np.abs(dh.cpu().numpy() - d_true).max()))
        s.close()
    print("position error: nominal median %.3e min %.3e; observer max %.3e median %.3e" % (
        np.median(err["nominal"]), err["nominal"].min(), err["observer"].max(), np.median(err["observer"])))
    assert err["observer"].max() <= 1e-3
    assert np.median(err["nominal"]) >= max(1e-2, 10 * err["observer"].max())


# ---- 9. validation ---------------------------------------------------------------------------------------------------
def test_validation(oracle):
    from crazyflie_nmpc_amd import estimate_disturbance
    from crazyflie_nmpc_amd.solver import CfnmpcError
    B, N = 64, 50
    rng = np.random.default_rng(4)
    d = random_dist(rng, B)
    s = _solver(B, d=d)
    w0 = s.workspace_bytes
    for bad in (np.nan, np.inf, -np.inf):
        q = d.copy(); q[17, 3] = bad
        with pytest.raises(CfnmpcError):
            s.set_disturbance(q)
        assert np.array_equal(s.disturbance(), d)
    with pytest.raises(ValueError):
        s.set_disturbance(d[:, :5])
    s.set_disturbance(-d)                                               # (any sign)
    assert np.array_equal(s.disturbance(), -d) and s.workspace_bytes == w0
    assert w0 >= _solver(B).workspace_bytes + 8 * ND * B               # the table is counted from the first call
    with pytest.raises(CfnmpcError):
        s.start_factor(2)
    for kw in (dict(start_solve=2), dict(start_solve=3), dict(cond_N2=10)):
        f = _solver(B, **kw)
        with pytest.raises(CfnmpcError):
            f.set_disturbance(d)
        assert np.array_equal(f.disturbance(), np.zeros((B, ND)))
        f.set_disturbance(None)
    x = oracle.sample_hover_x0(rng, B, scale=1.0)
    u = np.full((B, 4), hover(NOMINAL))
    for ga, gw in ((0.0, 0.5), (0.5, 0.0), (1.5, 0.5), (0.5, -0.1), (np.nan, 0.5)):
        dd = d.copy()
        with pytest.raises(CfnmpcError):
            estimate_disturbance(x, u, x, dd, DT, 1, ga, gw)
        assert np.array_equal(dd, d)
    estimate_disturbance(x, u, x, d.copy(), DT, 1, 1.0, 1.0)


def test_sens_is_invalidated_and_matches_differences(oracle):
    from crazyflie_nmpc_amd.solver import CfnmpcError
    B, N = 64, 50
    rng = np.random.default_rng(6)
    p = random_params(rng, B)
    d = random_dist(rng, B)
    x0, yr, ye = _inputs(oracle, B, N, 6, scale=0.5)
    yr[:, :, 13:] = hover(p)[:, None, None]
    x = np.repeat(x0[:, None, :], N + 1, 1)
    u = np.repeat(yr[:, :1, 13:], N, 1).copy()
    s = _solver(B, 1, p, d, tol=QP_TOL)
    s.set_x0(x0); s.set_yref(yr, ye); s.set_iterate(x, u)
    s.solve(1)
    s.eval_sens_x0()
    s.set_disturbance(0.5 * d)                                          # new values: the evaluation no longer belongs to the data
    with pytest.raises(CfnmpcError):
        s.eval_sens_x0()
    with pytest.raises(CfnmpcError):
        s.sens_x0(0)
    s.set_iterate(x, u)
    s.solve(1)
    s.eval_sens_x0()
    du, _ = s.sens_x0(0)
    _, ug = s.get_iterate()
    free = np.flatnonzero(((ug > 1e-3) & (ug < 22.0 - 1e-3)).all(axis=(1, 2)))[:4]
    assert len(free) == 4
    eps = 1e-4
    fd = np.empty((B, 4, 13))
    for c in range(13):
        up = []
        for sgn in (1.0, -1.0):
            xe = x0.copy(); xe[:, c] += sgn * eps
            s.set_x0(xe); s.set_iterate(x, u)
            s.solve(1)
            up.append(s.get_u(0))
        fd[:, :, c] = (up[0] - up[1]) / (2 * eps)
    for i in free:
        assert np.abs(du[i] - fd[i]).max() <= 1e-5 * max(1.0, np.abs(fd[i]).max()), (i, np.abs(du[i] - fd[i]).max())


# ---- 10. fleet and multi ---------------------------------------------------------------------------------------------
def test_fleet_and_multi_match_single_solvers(oracle):
    import torch
    from crazyflie_nmpc_amd import BatchSolver, default_opts, parallel
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    rng = np.random.default_rng(29)
    B = 96
    hz = rng.choice([8, 17, 40], size=B)
    x0, yref, yref_e = _inputs(oracle, B, 40, 8, scale=1.5)
    f = MixedHorizonFleet(hz)
    singles = {n: (idx, _solver(len(idx), N=int(n))) for n, idx in f.buckets()}
    f.set_yref(yref, yref_e); f.set_x0(x0); f.init_iterate(INIT_HOVER)
    for n, (idx, s) in singles.items():
        s.set_yref(yref[idx, :n].copy(), yref_e[idx].copy()); s.set_x0(x0[idx].copy()); s.init_iterate(INIT_HOVER)
    x = x0.copy()
    for t in range(4):
        d = random_dist(rng, B)
        if t % 2:
            f.set_disturbance(torch.tensor(d, device="cuda"))           # through each bucket's staging, on its stream
        else:
            f.set_disturbance(d)
        assert np.array_equal(f.disturbance(), d)
        f.set_x0(x); f.solve(1)
        uf, xf = f.get_u(0), f.get_x(1)
        assert (f.stats()[0] == 0).all()
        for n, (idx, s) in singles.items():
            s.set_disturbance(d[idx].copy())
            s.set_x0(x[idx].copy()); s.solve(1)
            assert np.array_equal(s.get_u(0), uf[idx]) and np.array_equal(s.get_x(1), xf[idx])
        x = np.stack([rk4(x[i], uf[i], NOMINAL, d[i], DT) for i in range(B)])
    # the rows matter: without them the first bucket's step differs
    n, (idx, s) = next(iter(singles.items()))
    s.set_disturbance(None); s.set_x0(x0[idx].copy()); s.init_iterate(INIT_HOVER); s.solve(1)
    u_none = s.get_u(0)
    s.set_disturbance(d[idx].copy()); s.init_iterate(INIT_HOVER); s.solve(1)
    assert np.abs(s.get_u(0) - u_none).max() > 1e-3
    # multi, uniform horizon, two shards on device 0
    B2, N = 301, 50
    d2 = random_dist(rng, B2)
    x2, yr2, ye2 = _inputs(oracle, B2, N, 9, scale=1.4)
    opts = default_opts(active_horizon=0)
    m = parallel.MultiGpuFleet(B2, [0, 0], opts)
    s = BatchSolver(B2, opts)
    m.set_disturbance(d2); s.set_disturbance(d2)
    for o in (m, s):
        o.set_x0(x2); o.set_yref(yr2, ye2); o.init_iterate(INIT_HOVER)
    for t in range(3):
        m.set_x0(x2); s.set_x0(x2)
        m.solve(1); s.solve(1); m.sync()
        assert np.array_equal(m.get_u(0), s.get_u(0)) and np.array_equal(m.get_x(4), s.get_x(4))
        assert np.array_equal(m.stats()[1], s.stats()[1])
        x2 = np.stack([rk4(x2[i], s.get_u(0)[i], NOMINAL, d2[i], DT) for i in range(B2)])
    with pytest.raises(ValueError):
        m.set_disturbance(np.where(np.arange(ND) == 3, np.nan, d2))     # a bad row: refused as a whole
