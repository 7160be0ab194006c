"""GPU suite: per-instance model parameters (include/cfnmpc.h: cfnmpc_set_model_params, cfnmpc_sim_params; DESIGN.md
section 5.13).

The reference is the numpy restatement of tests/test_model_params_cpu.py (f(x, u, p), complex-step Jacobians, M-step RK4
sensitivities), checked there against the oracle at the nominal row and against central differences elsewhere.  One RTI
step is compared with oracle.qp_from_blocks + oracle.solve_qp_dense on those blocks, oracle.solve_qp_refined being the
referee where the two FP64 sides disagree (as tests/test_gpu_erk.py does)."""
import numpy as np
import pytest

from test_model_params_cpu import NOMINAL, hover, random_params, rk4, rk4_sens

pytestmark = pytest.mark.gpu
DT = 0.015
QP_TOL = 1e-11


def _inputs(oracle, B, N, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    x0 = oracle.sample_hover_x0(rng, B, scale=scale)
    yr, ye = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    return x0, np.repeat(yr[None], B, 0).copy(), np.repeat(ye[None], B, 0).copy()


def _solver(B, M=1, p=None, **kw):
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    s = BatchSolver(B, default_opts(**kw))
    if M != 1:
        s.set_erk_steps(M)
    if p is not None:
        s.set_model_params(p)
    return s


def _blocks(x, u, p, M):
    N = u.shape[0]
    A = np.empty((N, 13, 13)); Bm = np.empty((N, 13, 4)); b = np.empty((N, 13))
    for k in range(N):
        phi, A[k], Bm[k] = rk4_sens(x[k], u[k], p, DT, M)
        b[k] = phi - x[k + 1]
    return A, Bm, b


def _ref_step(oracle, x, u, x0, yref, yref_e, p, M, W, WN, u_min=0.0, u_max=22.0):
    A, Bm, b = _blocks(x, u, p, M)
    q = np.empty((x.shape[0], 13))
    q[:-1] = W[:13] * (x[:-1] - yref[:, :13])
    q[-1] = WN * (x[-1] - yref_e)
    r = W[13:] * (u - yref[:, 13:])
    qp = oracle.qp_from_blocks(A, Bm, b, q, r, x0 - x[0], W[:13], W[13:], WN, u_min - u, u_max - u)
    sol = oracle.solve_qp_dense(qp)
    return x + sol["dx"], u + sol["du"], qp


def _agree(oracle, xg, ug, xr, ur, qp, x, u, tol):
    e = max(np.abs(xg - xr).max(), np.abs(ug - ur).max())
    if e <= tol:
        return e
    ref = oracle.solve_qp_refined(qp)
    return max(np.abs(xg - (x + ref["dx"])).max(), np.abs(ug - (u + ref["du"])).max())


def _weights():
    from crazyflie_nmpc_amd import default_opts
    o = default_opts()
    return np.array(o.W), np.array(o.WN)


# ---- 1. blocks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3])
def test_blocks_match_reference(oracle, M):
    B, N = 200, 50                                   # (the last wave partial)
    rng = np.random.default_rng(40 + M)
    p = random_params(rng, B)
    x0, yr, ye = _inputs(oracle, B, N, 3 + M, scale=1.5)
    x = np.repeat(x0[:, None, :], N + 1, 1) + rng.normal(0, 0.05, (B, N + 1, 13))
    x[:, :, 3:7] /= np.linalg.norm(x[:, :, 3:7], axis=2, keepdims=True)
    u = hover(p)[:, None, None] + rng.normal(0, 2.0, (B, N, 4))
    s = _solver(B, M, p)
    s.set_x0(x0); s.set_yref(yr, ye); s.set_iterate(x, u)
    s.linearise_only()
    A, Bm, b = s.get_linearisation()
    for i in list(rng.choice(B - 8, 16, replace=False)) + list(range(B - 8, B)):
        Ar, Br, br = _blocks(x[i], u[i], p[i], M)
        assert np.abs(A[i] - Ar).max() <= 1e-12 * max(1.0, np.abs(Ar).max()), (i, np.abs(A[i] - Ar).max())
        assert np.abs(Bm[i] - Br).max() <= 1e-12 * max(1.0, np.abs(Br).max()), (i, np.abs(Bm[i] - Br).max())
        assert np.abs(b[i] - br).max() <= 1e-12 * max(1.0, np.abs(x[i]).max()), (i, np.abs(b[i] - br).max())


# ---- 2. nominal rows -------------------------------------------------------------------------------------------------
def _closed_loop(s, oracle, x0, yr, ye, steps, seed):
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    rng = np.random.default_rng(seed)
    s.set_x0(x0); s.set_yref(yr, ye); s.init_iterate(INIT_HOVER)
    x = x0.copy()
    out = []
    for j in range(steps):
        s.set_x0(x)
        s.solve(1)
        u0 = s.get_u(0)
        out.append((u0, s.get_u(1), s.get_x(4)) + tuple(s.stats()[:2]))
        x = np.stack([oracle.rk4(x[i], u0[i], DT) for i in range(x.shape[0])])
        if j % 3 == 1:
            x[:, 7:10] += rng.normal(0, 0.5, (x.shape[0], 3))
    return out


def test_nominal_rows_are_the_default(oracle):
    B, N = 512, 50
    x0, yr, ye = _inputs(oracle, B, N, 21, scale=1.5)
    rng = np.random.default_rng(2)
    x = np.repeat(x0[:, None, :], N + 1, 1) + rng.normal(0, 0.05, (B, N + 1, 13))
    u = 15.0 + rng.normal(0, 2.0, (B, N, 4))
    blocks = []
    for p in (None, np.tile(NOMINAL, (B, 1))):
        s = _solver(B, p=p)
        s.set_x0(x0); s.set_yref(yr, ye); s.set_iterate(x, u)
        s.linearise_only()
        blocks.append(s.get_linearisation())
    for a, b in zip(*blocks):
        assert np.abs(a - b).max() <= 1e-14 * np.abs(a).max()
    ra = _closed_loop(_solver(B), oracle, x0, yr, ye, 20, 5)
    rb = _closed_loop(_solver(B, p=np.tile(NOMINAL, (B, 1))), oracle, x0, yr, ye, 20, 5)
    worst, bitwise = 0.0, True
    for p_, q_ in zip(ra, rb):
        for v, w in zip(p_[:3], q_[:3]):
            worst = max(worst, np.abs(v - w).max())
            bitwise = bitwise and np.array_equal(v, w)
        assert np.array_equal(p_[4], q_[4])                         # QP solve counts
    print(f"nominal rows vs default over 20 steps: max |diff| = {worst:.3e}, bitwise = {bitwise}")
    # (measured 2.6e-10 absolute on u ~ 15 kRPM, not bitwise: k_linearise_par rounds a few products differently from the
    #  folded-constant kernel, 1e-16 relative, and 20 kicked closed-loop steps amplify that)
    assert worst <= 1e-9
    # back to NULL: the default kernels, bitwise
    s = _solver(B, p=random_params(rng, B))
    s.set_model_params(None)
    assert np.array_equal(s.model_params(), np.tile(NOMINAL, (B, 1)))
    rc = _closed_loop(s, oracle, x0, yr, ye, 20, 5)
    for p_, q_ in zip(ra, rc):
        for v, w in zip(p_, q_):
            assert np.array_equal(v, w)


# ---- 3. one RTI step per row -----------------------------------------------------------------------------------------
ROUTES = [dict(), dict(active_set=0), dict(forward_split=1), dict(as_dense=1), dict(as_dense=0), dict(M=2),
          dict(cond_N2=10), dict(step_graph=1)]


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: ",".join(f"{k}={v}" for k, v in r.items()) or "default")
def test_rti_step_matches_reference(oracle, route):
    route = dict(route)
    M = route.pop("M", 1)
    B, N = 1024, 50
    rng = np.random.default_rng(70)
    p = random_params(rng, B)
    x0, yr, ye = _inputs(oracle, B, N, 11, scale=1.5)
    yr[:, :, 13:] = hover(p)[:, None, None]
    x0[:, 7:10] += rng.normal(0, 1.5, (B, 3))                      # kicks: a good share of the rows hit the box
    x = np.repeat(x0[:, None, :], N + 1, 1)
    u = np.repeat(np.repeat(hover(p)[:, None, None], N, 1), 4, 2)
    s = _solver(B, M, p, tol=QP_TOL, **route)
    s.set_x0(x0); s.set_yref(yr, ye); s.set_iterate(x, u)
    s.solve(1)
    st, _, _ = s.stats()
    xg, ug = s.get_iterate()
    W, WN = _weights()
    rows = rng.choice(B, 24, replace=False)
    n_con = 0
    for i in rows:
        xr, ur, qp = _ref_step(oracle, x[i], u[i], x0[i], yr[i], ye[i], p[i], M, W, WN)
        n_con += int((ur <= 1e-9).any() or (ur >= 22.0 - 1e-9).any())
        assert st[i] == 0, (i, st[i])
        assert _agree(oracle, xg[i], ug[i], xr, ur, qp, x[i], u[i], 1e-8) <= 1e-8, i
    assert n_con >= 0.2 * len(rows), n_con


# ---- 4. row independence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ah", [0, 1])
def test_rows_independent_under_permutation(oracle, ah):
    """Permuting instances together with their parameters permutes every output (the pattern of
    tests/test_gpu_full_size.py::test_instances_are_independent_under_permutation): bitwise with full-horizon sweeps; with
    the active horizon the head is a wave-level maximum, so the solutions agree to rounding.  Constrained rows (compacted
    kernels) are part of it: a kernel that read a compact slot's or lane's parameters would fail here."""
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B, N = 2048, 50
    rng = np.random.default_rng(90 + ah)
    p = random_params(rng, B)
    x0, yr, ye = _inputs(oracle, B, N, 12, scale=1.5)
    x0[:, 7:10] += rng.normal(0, 1.5, (B, 3))
    perm = rng.permutation(B)
    outs = []
    for pi in (np.arange(B), perm):
        s = _solver(B, p=p[pi], active_horizon=ah, tol=QP_TOL)   # (kicked rows reach the interior point: solve it tightly)
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


# ---- 6. sim_params and hover -----------------------------------------------------------------------------------------
def test_sim_params_and_hover(oracle):
    from crazyflie_nmpc_amd import sim
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B = 300
    rng = np.random.default_rng(8)
    p = random_params(rng, B)
    x = oracle.sample_hover_x0(rng, B, scale=1.5)
    u = hover(p)[:, None] + rng.normal(0, 2.0, (B, 4))
    xn = sim(x, u, 0.06, 4, params=p)
    ref = np.stack([rk4(x[i], u[i], p[i], 0.06, 4) for i in range(B)])
    assert np.abs(xn - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    xnom = sim(x, u, 0.06, 4, params=np.tile(NOMINAL, (B, 1)))
    assert np.abs(xnom - sim(x, u, 0.06, 4)).max() <= 1e-14 * max(1.0, np.abs(xnom).max())
    s = _solver(B, p=p)
    s.set_x0(x); s.init_iterate(INIT_HOVER)
    _, ug = s.get_iterate()
    assert np.abs(ug - hover(p)[:, None, None]).max() <= 1e-12 * hover(p).max()
    assert np.array_equal(s.model_params(), p)


# ---- 9. validation ---------------------------------------------------------------------------------------------------
def test_validation_and_graph_update(oracle):
    from crazyflie_nmpc_amd.solver import INIT_HOVER, CfnmpcError
    B, N = 256, 50
    rng = np.random.default_rng(4)
    p = random_params(rng, B)
    s = _solver(B, p=p)
    for bad in (np.nan, 0.0, -1.0, np.inf):
        q = p.copy(); q[17, 3] = bad
        with pytest.raises(CfnmpcError):
            s.set_model_params(q)
        assert np.array_equal(s.model_params(), p)
    with pytest.raises(ValueError):
        s.set_model_params(p[:, :7])
    for ss in (2, 3):
        f = _solver(B, start_solve=ss)
        with pytest.raises(CfnmpcError):
            f.set_model_params(p)
        assert np.array_equal(f.model_params(), np.tile(NOMINAL, (B, 1)))
        f.set_model_params(None)
    # captured step graph: new values take effect in a replay of a graph captured BEFORE the update (one exec per parity of
    # the iterate buffers: two solves capture both, the third replays parity 0)
    x0, yr, ye = _inputs(oracle, B, N, 6, scale=1.0)
    p2 = random_params(np.random.default_rng(5), B)
    res = []
    for variant in ("graph", "plain"):
        g = _solver(B, p=p, step_graph=1 if variant == "graph" else 0)
        g.set_x0(x0); g.set_yref(yr, ye); g.init_iterate(INIT_HOVER)
        g.solve(1); g.solve(1)
        g.set_model_params(p2)
        g.solve(1); g.solve(1)
        res.append(g.get_iterate())
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    # ... and differ from what the old values give (the update is not a no-op)
    h = _solver(B, p=p, step_graph=1)
    h.set_x0(x0); h.set_yref(yr, ye); h.init_iterate(INIT_HOVER)
    for _ in range(4):
        h.solve(1)
    assert np.abs(h.get_iterate()[1] - res[0][1]).max() > 1e-6


# ---- 5. SQP ----------------------------------------------------------------------------------------------------------
def _ref_sqp(oracle, x0, yr, ye, p, xr, ur, max_iter, tol):
    """SQP on the numpy model (in place on xr, ur): one reference RTI step per iteration, the residuals and stop rule of
    cfnmpc_solve_sqp -> status, sqp_iter"""
    B = x0.shape[0]
    W, WN = _weights()
    status = np.full(B, 2, dtype=np.int32); it = np.zeros(B, dtype=np.int32)
    for i in range(B):
        for j in range(1, max_iter + 1):
            xn, un, _ = _ref_step(oracle, xr[i], ur[i], x0[i], yr[i], ye[i], p[i], 1, W, WN)
            step = max(np.abs(xn - xr[i]).max(), np.abs(un - ur[i]).max())
            eq = max([np.abs(xn[0] - x0[i]).max()] + [np.abs(xn[k + 1] - rk4(xn[k], un[k], p[i], DT)).max() for k in range(un.shape[0])])
            ineq = max(0.0, (0.0 - un).max(), (un - 22.0).max())
            xr[i], ur[i], it[i] = xn, un, j
            if step <= tol and eq <= tol and ineq <= tol:
                status[i] = 0
                break
    return status, it


def test_sqp_matches_reference(oracle):
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B, N, TOL, MAXIT = 12, 50, 1e-9, 60
    rng = np.random.default_rng(55)
    p = random_params(rng, B)
    x0, yr, ye = _inputs(oracle, B, N, 31, scale=1.0)
    yr[:, :, 13:] = hover(p)[:, None, None]
    s = _solver(B, p=p, tol=QP_TOL)
    s.set_x0(x0); s.set_yref(yr, ye); s.init_iterate(INIT_HOVER)
    s.solve_sqp(MAXIT, TOL, TOL, TOL)
    st, it, rs = s.sqp_stats()
    xg, ug = s.get_iterate()
    xr = np.repeat(x0[:, None, :], N + 1, 1).copy()
    ur = np.repeat(np.repeat(hover(p)[:, None, None], N, 1), 4, 2).copy()
    st_r, it_r = _ref_sqp(oracle, x0, yr, ye, p, xr, ur, MAXIT, TOL)
    # (full Gauss-Newton steps: part of the rows still oscillate at max_iter on both sides, status 2)
    assert (st_r == 0).sum() >= B // 3, st_r
    assert np.array_equal(st, st_r), (st, st_r)
    assert np.array_equal(it, it_r), (it, it_r)
    for i in np.flatnonzero(st == 0):   # the final iterate's defect under each row's OWN model
        eq = max(np.abs(xg[i, k + 1] - rk4(xg[i, k], ug[i, k], p[i], DT)).max() for k in range(N))
        assert eq <= TOL, (i, eq)
        assert rs[i, 1] <= TOL


# ---- 7. model mismatch, closed loop ----------------------------------------------------------------------------------
def test_model_mismatch_closed_loop():
    """512 vehicles whose plant mass is 0.8 - 1.3 x nominal (other parameters nominal), 200 steps through sim_params from
    the hover equilibrium at the reference.  Thresholds from the numpy reference loop on the CPU (the QP of
    oracle.qp_from_blocks on this file's blocks, 200 steps, plant = rk4 with the plant's row): the param-aware controller
    (its model = the plant, yref inputs = hover_speed) keeps the altitude error at 0.0 for mass 0.8 and 1.3; the nominal
    controller ends 8.9 cm (0.8) and 10.9 cm (1.3) off.  So: aware within 1 mm on every row; nominal median at least 10 x the
    aware median and above 1 cm."""
    import torch
    from crazyflie_nmpc_amd import hover_speed, sim
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B, N, STEPS = 512, 50, 200
    rng = np.random.default_rng(12)
    plant = np.tile(NOMINAL, (B, 1))
    plant[:, 1] *= rng.uniform(0.8, 1.3, B)
    yr1 = np.zeros((N, 17)); yr1[:, 2] = 0.4; yr1[:, 3] = 1.0
    ye = np.tile(yr1[0, :13], (B, 1))
    x0 = ye.copy()
    pt = torch.tensor(plant, device="cuda")
    err = {}
    for ctrl in ("aware", "nominal"):
        pc = plant if ctrl == "aware" else np.tile(NOMINAL, (B, 1))
        yr = np.tile(yr1, (B, 1, 1)); yr[:, :, 13:] = hover_speed(pc)[:, None, None]
        s = _solver(B, p=pc if ctrl == "aware" else None)
        s.set_x0(x0); s.set_yref(yr, ye); s.init_iterate(INIT_HOVER)
        x = torch.tensor(x0, device="cuda")
        u0 = torch.empty((B, 4), dtype=torch.float64, device="cuda")
        for _ in range(STEPS):
            s.set_x0(x)
            s.solve(1)
            s.get_u(0, out=u0)
            x = sim(x, u0, DT, 1, params=pt)
        assert (s.stats()[0] == 0).all()
        err[ctrl] = np.abs(x[:, 2].cpu().numpy() - 0.4)
        s.close()
    print("altitude error: aware max %.3e median %.3e; nominal median %.3e max %.3e" % (
        err["aware"].max(), np.median(err["aware"]), np.median(err["nominal"]), err["nominal"].max()))
    assert err["aware"].max() <= 1e-3
    assert np.median(err["nominal"]) >= max(1e-2, 10 * np.median(err["aware"]))


# ---- 8. fleet and multi ----------------------------------------------------------------------------------------------
def test_fleet_and_multi_match_single_solvers(oracle):
    """A mixed-horizon fleet with per-vehicle parameters (cfnmpc_fleet_set_model_params: rows scattered to the buckets)
    equals single solvers of each bucket's size and horizon on the same rows, bitwise; an in-process cfnmpc_multi over three
    shards on one device (cfnmpc_multi_set_model_params: rows split by shard) equals one solver, bitwise (full-horizon sweeps:
    a vehicle's arithmetic does not depend on its neighbours)."""
    from crazyflie_nmpc_amd import BatchSolver, default_opts, parallel
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    rng = np.random.default_rng(19)
    B = 333
    hz = rng.choice([30, 50, 100], size=B)
    p = random_params(rng, B)
    x0, yref, yref_e = _inputs(oracle, B, 100, 8, scale=1.5)
    yref[:, :, 13:] = hover(p)[:, None, None]
    f = MixedHorizonFleet(hz)
    f.set_model_params(p)
    singles = {n: (idx, _solver(len(idx), p=p[idx].copy(), N=int(n))) for n, idx in f.buckets()}
    f.set_yref(yref, yref_e); f.set_x0(x0); f.init_iterate(INIT_HOVER)
    for n, (idx, s) in singles.items():
        s.set_yref(yref[idx, :n].copy(), yref_e[idx].copy()); s.set_x0(x0[idx].copy()); s.init_iterate(INIT_HOVER)
    x = x0.copy()
    for t in range(3):
        f.set_x0(x); f.solve(1)
        uf, xf = f.get_u(0), f.get_x(1)
        assert (f.stats()[0] == 0).all()
        for n, (idx, s) in singles.items():
            s.set_x0(x[idx].copy()); s.solve(1)
            assert np.array_equal(s.get_u(0), uf[idx]) and np.array_equal(s.get_x(1), xf[idx])
        x = np.stack([rk4(x[i], uf[i], p[i], DT) for i in range(B)])
    # multi, uniform horizon, three shards on device 0
    B2, N = 1001, 50
    p2 = random_params(rng, B2)
    x2, yr2, ye2 = _inputs(oracle, B2, N, 9, scale=1.4)
    yr2[:, :, 13:] = hover(p2)[:, None, None]
    opts = default_opts(active_horizon=0)
    m = parallel.MultiGpuFleet(B2, [0, 0, 0], opts)
    s = BatchSolver(B2, opts)
    m.set_model_params(p2); s.set_model_params(p2)
    for o in (m, s):
        o.set_x0(x2); o.set_yref(yr2, ye2); o.init_iterate(INIT_HOVER)
    for t in range(3):
        m.set_x0(x2); s.set_x0(x2)
        m.solve(1); s.solve(1); m.sync()
        assert np.array_equal(m.get_u(0), s.get_u(0)) and np.array_equal(m.get_x(4), s.get_x(4))
        assert np.array_equal(m.stats()[1], s.stats()[1])
        x2 = np.stack([rk4(x2[i], s.get_u(0)[i], p2[i], DT) for i in range(B2)])
    with pytest.raises(ValueError):
        m.set_model_params(np.where(np.arange(8) == 3, -1.0, p2))   # a bad row: refused as a whole


# ---- 10. full size ---------------------------------------------------------------------------------------------------
def test_full_size_random_params(oracle):
    import torch
    from crazyflie_nmpc_amd import sim
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B, N, STEPS = 65536, 50, 10
    rng = np.random.default_rng(101)
    p = random_params(rng, B)
    x0, yr, ye = _inputs(oracle, B, N, 99, scale=1.0)
    W, WN = _weights()
    pt = torch.tensor(p, device="cuda")
    ok = {}
    for variant in ("default", "params"):
        yv = yr.copy()
        if variant == "params":
            yv[:, :, 13:] = hover(p)[:, None, None]
        s = _solver(B, p=p if variant == "params" else None, tol=QP_TOL)
        s.set_x0(x0); s.set_yref(yv, ye); s.init_iterate(INIT_HOVER)
        krng = np.random.default_rng(5)
        x = torch.tensor(x0, device="cuda")
        n_ok = 0
        for j in range(STEPS):
            x[:, 7:10] += torch.tensor(krng.normal(0, 0.3, (B, 3)), device="cuda")     # kicks
            s.set_x0(x)
            last = variant == "params" and j == STEPS - 1
            if last:
                xp, up = s.get_iterate()
                xc = x.cpu().numpy()
            s.solve(1)
            n_ok += int((s.stats()[0] == 0).sum())
            u0 = torch.tensor(s.get_u(0), device="cuda")
            x = sim(x, u0, DT, 1, params=pt if variant == "params" else None)
        ok[variant] = n_ok / (STEPS * B)
        if variant == "params":
            xg, ug = s.get_iterate()
            for i in rng.choice(B, 192, replace=False):
                xr, ur, qp = _ref_step(oracle, xp[i], up[i], xc[i], yv[i], ye[i], p[i], 1, W, WN)
                assert _agree(oracle, xg[i], ug[i], xr, ur, qp, xp[i], up[i], 1e-8) <= 1e-8, i
        s.close()
    print("ok fraction: default %.5f, random parameters %.5f" % (ok["default"], ok["params"]))
    assert abs(ok["params"] - ok["default"]) <= 0.005
