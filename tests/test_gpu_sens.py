"""GPU suite: solution sensitivities with respect to x0 (include/cfnmpc.h: cfnmpc_eval_sens_x0, cfnmpc_get_sens_x0,
cfnmpc_get_sens_active).

The reference is the numpy recursion of tests/test_sens_cpu.py (checked there against a dense referee on the condensed QP and
against central differences of the extended-precision QP solution), run on the engine's own blocks
(cfnmpc_debug_get_linearisation), weights and active set (cfnmpc_get_sens_active)."""
import ctypes as C

import numpy as np
import pytest

from test_sens_cpu import sens_ref

pytestmark = pytest.mark.gpu
DT = 0.015
# FP64 Riccati arithmetic on the GPU against numpy's drifts with the horizon: the start solve's own gains KR differ from numpy's
# by up to 7.7e-10 per stage at N = 100 (test_home_gains_against_numpy), the masked sweep by up to 2.7e-9 there
# (test_engine_matches_reference).  1e-9 holds to N = 50 and between routes that share their blocks.
TOL = 1e-8
ROUTE_TOL = 1e-9


def _solver(B, N=50, **kw):
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    return BatchSolver(B, default_opts(N=N, **kw))


def _setup(oracle, s, seed, scale):
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    rng = np.random.default_rng(seed)
    B, N = s.B, s.N
    x0 = oracle.sample_hover_x0(rng, B, scale=scale)
    yr, ye = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    s.set_yref(np.repeat(yr[None], B, 0), np.repeat(ye[None], B, 0))
    s.set_x0(x0)
    s.init_iterate(INIT_HOVER)
    return x0


def _weights(s, stage_scale=1.0, terminal_scale=1.0):
    W, WN = np.array(s.opts.W), np.array(s.opts.WN)
    return stage_scale * W[:13], stage_scale * W[13:], terminal_scale * WN


def _engine(s):
    """-> du [B][N][4][13], dx [B][N+1][13][13], act [B][N][4]"""
    du, _ = s.sens_x0(0, s.N)
    _, dx = s.sens_x0(0, s.N + 1)
    return du, dx, s.sens_active()


def _check_against_ref(s, du, dx, act, status, weights, rows=None):
    A, Bm, _b = s.get_linearisation()
    Qd, Rd, QNd = weights
    rows = range(s.B) if rows is None else rows
    n = 0
    for i in rows:
        if status[i] == 4:
            assert np.isnan(du[i]).all() and np.isnan(dx[i]).all()
            continue
        ru, rx = sens_ref(A[i], Bm[i], Qd, Rd, QNd, act[i])
        assert np.abs(du[i] - ru).max() <= TOL * max(1.0, np.abs(ru).max()), i
        assert np.abs(dx[i] - rx).max() <= TOL * max(1.0, np.abs(rx).max()), i
        assert np.array_equal(dx[i, 0], np.eye(13)), i
        assert np.all(du[i][act[i] != 0] == 0.0), i
        n += 1
    return n


def _kst(act, N):
    """start stage of the masked sweep (k_sens_mask): smallest checkpoint above the last active stage, else N; 0 = unlisted"""
    st = np.flatnonzero((np.asarray(act) != 0).any(axis=1))
    if st.size == 0:
        return 0, -1
    for c, k in enumerate(CHK):
        if k > st.max() and k < N:
            return k, c
    return N, -1


CHK = (4, 8, 12, 16, 24, 32)


def sens_ref_engine(A, B, Qd, Rd, QNd, act, K, Pchk):
    """the masked recursion over [0, kst) from the engine's own checkpoint (or QN), the engine's home gains K behind kst: what
    k_sens_factor + k_sens_fwd compute, isolated from the start solve's own rounding"""
    N = A.shape[0]
    act = np.asarray(act) != 0
    kst, c = _kst(act, N)
    Kt = -np.asarray(K, dtype=np.float64).copy()
    P = Pchk[c].copy() if c >= 0 else np.diag(QNd)
    for k in range(kst - 1, -1, -1):
        F = ~act[k]
        BF = B[k][:, F]
        Kt[k] = 0.0
        if F.any():
            S = np.diag(np.asarray(Rd)[F]) + BF.T @ P @ BF
            Kt[k][F] = -np.linalg.solve(S, BF.T @ P @ A[k])
        P = np.diag(Qd) + A[k].T @ P @ A[k] + A[k].T @ P @ BF @ Kt[k][F]
    du = np.zeros((N, 4, 13))
    dx = np.zeros((N + 1, 13, 13))
    dx[0] = np.eye(13)
    for k in range(N):
        du[k] = Kt[k] @ dx[k]
        dx[k + 1] = A[k] @ dx[k] + B[k] @ du[k]
    return du, dx


def _per_stage_err(a, b):
    """max over stages of |a_k - b_k| / max(1, |b_k|)"""
    ax = tuple(range(1, a.ndim))
    return float((np.abs(a - b).max(axis=ax) / np.maximum(1.0, np.abs(b).max(axis=ax))).max())


# ---- 1. engine against the numpy reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [20, 50, 100])
def test_engine_matches_reference(oracle, N):
    s = _solver(256, N)
    _setup(oracle, s, 10 + N, 3.0)
    s.solve(2)
    s.eval_sens_x0()
    du, dx, act = _engine(s)
    status, _, _ = s.stats()
    share = float((act != 0).any(axis=(1, 2)).mean())
    assert share >= 0.2, share
    assert _check_against_ref(s, du, dx, act, status, _weights(s)) >= 200
    # the new kernels alone, stage by stage: the reference on the engine's own blocks, checkpoints and home gains
    A, Bm, _b = s.get_linearisation()
    K, _d, Pchk, _st = s.get_factor()
    Qd, Rd, QNd = _weights(s)
    worst = 0.0
    for i in np.flatnonzero(status != 4):
        ru, rx = sens_ref_engine(A[i], Bm[i], Qd, Rd, QNd, act[i], K[i], Pchk[i])
        worst = max(worst, _per_stage_err(du[i], ru), _per_stage_err(dx[i], rx))
    print(f"N = {N}: engine vs reference on the engine's gains, per-stage relative {worst:.2e}")
    # (N <= 50: 1e-9; at N = 100 the masked sweep's FP64 rounding against numpy's reaches the start solve's own level, see
    #  test_home_gains_against_numpy and DESIGN.md section 5.14)
    assert worst <= (ROUTE_TOL if N <= 50 else TOL), worst
    # get(0, 1) (no sweep) and sub-ranges are slices of the one sweep
    u0, x0_ = s.sens_x0(0)
    assert np.array_equal(u0, du[:, 0]) and np.array_equal(x0_, dx[:, 0])
    u1, x1 = s.sens_x0(1)
    assert np.array_equal(u1, du[:, 1]) and np.array_equal(x1, dx[:, 1])
    u4, x4 = s.sens_x0(4, 3)
    assert np.array_equal(u4, du[:, 4:7]) and np.array_equal(x4, dx[:, 4:7])
    s.close()


def test_home_gains_against_numpy(oracle):
    """what bounds TOL: the start solve's gains KR (k_factor, no sensitivity code involved) against numpy's FP64 Riccati gains on
    the same blocks.  KR is the UNCONSTRAINED gain for every row (the active set only enters the sensitivity kernels), so every
    row that did not fail is compared"""
    s = _solver(256, 100)
    _setup(oracle, s, 110, 3.0)
    s.solve(2)
    s.eval_sens_x0()
    act = s.sens_active()
    status, _, _ = s.stats()
    A, Bm, _b = s.get_linearisation()
    K, _d, _P, _st = s.get_factor()
    Qd, Rd, QNd = _weights(s)
    worst = 0.0
    rows = [i for i in range(s.B) if status[i] != 4]
    assert len(rows) >= 200 and sum(act[i].any() for i in rows) >= 100
    for i in rows:   # numpy's Riccati gains, every stage, each normalised by its own largest entry
        P = np.diag(QNd)
        for k in range(s.N - 1, -1, -1):
            S = np.diag(Rd) + Bm[i, k].T @ P @ Bm[i, k]
            Kt = -np.linalg.solve(S, Bm[i, k].T @ P @ A[i, k])
            P = np.diag(Qd) + A[i, k].T @ P @ A[i, k] + A[i, k].T @ P @ Bm[i, k] @ Kt
            worst = max(worst, float(np.abs(-K[i, k] - Kt).max() / max(1.0, np.abs(Kt).max())))
    print(f"k_factor gains vs numpy (N = 100, kicks x 3, {len(rows)} rows, every stage): {worst:.2e} relative")
    assert worst <= TOL, worst
    s.close()


# ---- 2. engine against its own finite differences ----------------------------------------------------------------------------
def test_engine_matches_finite_differences(oracle):
    B, N, h = 32, 50, 1e-6
    s = _solver(B, N)
    x0 = _setup(oracle, s, 5, 2.0)
    s.solve(2)
    x_it, u_it = s.get_iterate()
    s.solve(1)
    s.eval_sens_x0()
    du, dx, act = _engine(s)
    # 27 replicas per row: x0, x0 +- h e_j, all from the same iterate, in one solver
    R = 27 * B
    r = _solver(R, N)
    yr, ye = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    r.set_yref(np.repeat(yr[None], R, 0), np.repeat(ye[None], R, 0))
    X0 = np.repeat(x0[:, None], 27, 1)
    for j in range(13):
        X0[:, 1 + 2 * j, j] += h
        X0[:, 2 + 2 * j, j] -= h
    r.set_iterate(np.repeat(x_it, 27, 0), np.repeat(u_it, 27, 0))
    r.set_x0(X0.reshape(R, 13))
    r.solve(1)
    r.eval_sens_x0()
    ract = r.sens_active().reshape(B, 27, N, 4)
    xs, us = r.get_iterate()
    xs = xs.reshape(B, 27, N + 1, 13); us = us.reshape(B, 27, N, 4)
    ok = excluded = 0
    for i in range(B):
        for j in range(13):
            if not all(np.array_equal(ract[i, m], act[i]) for m in (0, 1 + 2 * j, 2 + 2 * j)):
                excluded += 1
                continue
            fu = (us[i, 1 + 2 * j] - us[i, 2 + 2 * j]) / (2 * h)
            fx = (xs[i, 1 + 2 * j] - xs[i, 2 + 2 * j]) / (2 * h)
            for k, (a, b) in enumerate(((fu[0], du[i, 0, :, j]), (fu[1], du[i, 1, :, j]), (fx[4], dx[i, 4, :, j]))):
                assert np.abs(a - b).max() <= 1e-6 * max(1.0, np.abs(b).max()), (i, j, k)
            ok += 1
    print(f"finite differences: {ok} columns checked, {excluded} of {B * 13} excluded ({excluded / (B * 13):.1%}: active set "
          f"changed at +-h)")
    assert excluded <= 0.1 * B * 13, excluded
    s.close(); r.close()


# ---- 3. routes and options ---------------------------------------------------------------------------------------------------
def _boxes(B, N, seed):
    rng = np.random.default_rng(seed)
    lb = np.zeros((B, N, 4)); ub = np.full((B, N, 4), 22.0)
    ub[:, :, :] -= rng.uniform(0, 4, (B, N, 4))
    pin = rng.uniform(0, 1, B) < 0.25
    lb[pin, 0, :] = ub[pin, 0, :] = 14.0   # lb == ub pins of stage 0
    return lb, ub


ROUTES = {
    "default": {}, "as_dense_on": dict(as_dense=1), "as_dense_off": dict(as_dense=0),
    "forward_split": dict(as_dense=1, forward_split=1), "step_graph": dict(step_graph=1), "start_solve_3": dict(start_solve=3),
    "active_set_0": dict(active_set=0), "box_stages": {}, "cost_scaling": {}, "erk_3": {}, "params": {},
}


def _route(oracle, name, B=256, N=50):
    s = _solver(B, N, **ROUTES[name])
    _setup(oracle, s, 77, 2.5)
    w = _weights(s)
    if name == "box_stages":
        s.set_box_stages(*_boxes(B, N, 3))
    elif name == "cost_scaling":
        s.set_cost_scaling(DT, 1.0)
        w = _weights(s, DT, 1.0)
    elif name == "erk_3":
        s.set_erk_steps(3)
    elif name == "params":
        from test_model_params_cpu import random_params
        s.set_model_params(random_params(np.random.default_rng(5), B))
    s.solve(1)   # (one step from the same iterate: every route's QP has the same blocks)
    s.eval_sens_x0()
    du, dx, act = _engine(s)
    status, _, _ = s.stats()
    n = _check_against_ref(s, du, dx, act, status, w)
    return s, du, dx, act, n


@pytest.fixture(scope="module")
def default_route(oracle):
    s, du, dx, act, n = _route(oracle, "default")
    s.close()
    return du, dx, act


@pytest.mark.parametrize("name", list(ROUTES))
def test_routes_match_reference(oracle, name, default_route):
    s, du, dx, act, n = _route(oracle, name)
    assert n >= 200
    if name in ("as_dense_on", "as_dense_off", "forward_split", "step_graph", "start_solve_3", "active_set_0"):
        du0, dx0, act0 = default_route
        same = np.array([np.array_equal(act[i], act0[i]) and not np.isnan(du[i]).any() and not np.isnan(du0[i]).any()
                         for i in range(s.B)])
        assert same.mean() >= 0.8
        tol = TOL if name == "start_solve_3" else ROUTE_TOL   # (k_linfactor's gains are not k_factor's bit for bit)
        assert np.abs(du[same] - du0[same]).max() <= tol * max(1.0, np.abs(du0[same]).max())
        assert np.abs(dx[same] - dx0[same]).max() <= tol * max(1.0, np.abs(dx0[same]).max())
    if name == "box_stages":
        lb, ub = _boxes(s.B, s.N, 3)
        pin = lb[:, 0] == ub[:, 0]
        assert pin.any() and np.all(act[:, 0][pin] == -1)   # pinned inputs count as active
    s.close()


# ---- 4. after solve_sqp ------------------------------------------------------------------------------------------------------
def test_after_sqp(oracle):
    s = _solver(128, 30)
    _setup(oracle, s, 9, 1.5)
    s.solve_sqp(max_iter=50)
    st, _, _ = s.sqp_stats()
    s.eval_sens_x0()
    du, dx, act = _engine(s)
    conv = np.flatnonzero(st == 0)
    assert conv.size >= 16
    A, Bm, _b = s.get_linearisation()
    Qd, Rd, QNd = _weights(s)
    for i in conv:
        ru, rx = sens_ref(A[i], Bm[i], Qd, Rd, QNd, act[i])
        assert np.abs(du[i] - ru).max() <= TOL * max(1.0, np.abs(ru).max())
        assert np.abs(dx[i] - rx).max() <= TOL * max(1.0, np.abs(rx).max())
    s.close()


# ---- 5. side effects ---------------------------------------------------------------------------------------------------------
def _loop(oracle, with_sens, B=512, N=50, steps=20):
    from crazyflie_nmpc_amd import sim
    s = _solver(B, N)
    x = _setup(oracle, s, 21, 2.0)
    kicks = oracle.sample_hover_x0(np.random.default_rng(22), B, scale=2.0)
    cmds = []
    for t in range(steps):
        if t % 5 == 0:
            x[t % B::7] = kicks[t % B::7]
        s.set_x0(x)
        s.solve(1)
        if with_sens:
            s.eval_sens_x0()
            s.sens_x0(0); s.sens_x0(1); s.sens_x0(4)
        u0 = s.get_u(0)
        cmds.append(s.get_cmd()[0].copy())
        x = sim(x, u0, T=DT, steps=1)
    out = (s.get_iterate(), s.stats(), np.array(cmds))
    s.close()
    return out


def test_no_side_effects(oracle):
    (xa, ua), sa, ca = _loop(oracle, False)
    (xb, ub), sb, cb = _loop(oracle, True)
    assert np.array_equal(xa, xb) and np.array_equal(ua, ub) and np.array_equal(ca, cb)
    for a, b in zip(sa, sb):
        assert np.array_equal(a, b)


def test_repeated_eval_is_bitwise_equal(oracle):
    s = _solver(256, 50)
    _setup(oracle, s, 31, 2.5)
    s.solve(2)
    s.eval_sens_x0()
    a = _engine(s)
    s.eval_sens_x0()
    b = _engine(s)
    for p, q in zip(a, b):
        assert np.array_equal(p, q)
    s.close()


# ---- 8. validation -----------------------------------------------------------------------------------------------------------
def test_refusals(oracle):
    from crazyflie_nmpc_amd.solver import CfnmpcError, INIT_HOVER
    s = _solver(8, 20)
    _setup(oracle, s, 1, 1.0)
    L, h = s._L, s._h
    with pytest.raises(CfnmpcError):
        s.eval_sens_x0()                       # before any solve
    s.solve(1)
    for tol in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(CfnmpcError):
            s.eval_sens_x0(tol)
    with pytest.raises(CfnmpcError):
        s.sens_x0(0)                           # no evaluation yet
    with pytest.raises(CfnmpcError):
        s.sens_active()
    s.eval_sens_x0()
    du = np.empty((8, 21, 4, 13)); dx = np.empty((8, 21, 13, 13))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.cfnmpc_get_sens_x0(h, 0, 1, None, None, 0, None) != 0      # both NULL
    assert L.cfnmpc_get_sens_x0(h, -1, 1, p(du), p(dx), 0, None) != 0
    assert L.cfnmpc_get_sens_x0(h, 0, 0, p(du), p(dx), 0, None) != 0
    assert L.cfnmpc_get_sens_x0(h, 0, 22, None, p(dx), 0, None) != 0     # beyond N + 1
    assert L.cfnmpc_get_sens_x0(h, 20, 1, p(du), p(dx), 0, None) != 0    # du with stage N
    assert L.cfnmpc_get_sens_x0(h, 0, 21, None, p(dx), 0, None) == 0
    assert L.cfnmpc_get_sens_x0(h, 20, 1, None, p(dx), 0, None) == 0
    x_it, u_it = s.get_iterate()
    W, WN = np.array(s.opts.W), np.array(s.opts.WN)
    changes = [
        lambda: s.set_weights(W, WN), lambda: s.set_cost_scaling(1.0, 1.0), lambda: s.set_box(0.0, 22.0),
        lambda: s.set_box_stages(np.zeros((8, 20, 4)), np.full((8, 20, 4), 22.0)), lambda: s.set_model_params(None),
        lambda: s.set_erk_steps(1), lambda: s.set_iterate(x_it, u_it), lambda: s.init_iterate(INIT_HOVER),
    ]
    for change in changes:
        s.solve(1)
        s.eval_sens_x0()
        s.sens_x0(0)
        change()
        with pytest.raises(CfnmpcError):
            s.eval_sens_x0()
        with pytest.raises(CfnmpcError):
            s.sens_x0(0)
    s.set_box_stages(None, None)
    s.solve(1)
    s.eval_sens_x0()
    s.solve(1)                                 # a later solve invalidates the evaluation
    with pytest.raises(CfnmpcError):
        s.sens_x0(0)
    with pytest.raises(CfnmpcError):
        s.sens_active()
    s.close()
    for kw in (dict(cond_N2=5), dict(start_solve=2)):
        t = _solver(8, 20, **kw)
        _setup(oracle, t, 1, 1.0)
        t.solve(1)
        with pytest.raises(CfnmpcError):
            t.eval_sens_x0()
        t.close()


def test_nan_row(oracle):
    outs = []
    for bad in (False, True):
        s = _solver(64, 50)
        x0 = _setup(oracle, s, 41, 2.0)
        s.solve(1)
        if bad:
            x0[5] = np.nan
        s.set_x0(x0)
        s.solve(1)
        s.eval_sens_x0()
        outs.append(_engine(s) + (s.stats()[0],))
        s.close()
    (du0, dx0, a0, _st0), (du1, dx1, a1, st1) = outs
    assert st1[5] == 4 and np.isnan(du1[5]).all() and np.isnan(dx1[5]).all()
    keep = np.arange(64) != 5
    assert np.array_equal(du0[keep], du1[keep]) and np.array_equal(dx0[keep], dx1[keep])


# ---- 9. full size ------------------------------------------------------------------------------------------------------------
def test_full_size(oracle):
    import torch
    import bench
    B, steps = 65536, 4
    dev = torch.device("cuda", 0)
    res = []
    for with_sens in (False, True):
        f = bench.Fleet(B, dev, np.random.default_rng(0))
        for _ in range(steps):
            f.step()
            if with_sens:
                f.solver.eval_sens_x0()
                u0 = torch.empty((B, 4, 13), dtype=torch.float64, device=dev)
                x0 = torch.empty((B, 13, 13), dtype=torch.float64, device=dev)
                f.solver.sens_x0(0, out_u=u0, out_x=x0)
                u4, _x4 = f.solver.sens_x0(4)
        torch.cuda.synchronize()
        res.append((f.solver.get_iterate(), f.solver.stats(), f.u0.cpu().numpy()))
        if with_sens:
            act = f.solver.sens_active()
            listed = np.flatnonzero((act != 0).any(axis=(1, 2)))
            rng = np.random.default_rng(3)
            rows = np.unique(np.concatenate([rng.choice(B, 64, replace=False), rng.choice(listed, min(64, listed.size), replace=False)]))
            A, Bm, _b = f.solver.get_linearisation()
            Qd, Rd, QNd = _weights(f.solver)
            ug = u0.cpu().numpy()
            for i in rows:
                ru, _rx = sens_ref(A[i], Bm[i], Qd, Rd, QNd, act[i])
                assert np.abs(ug[i] - ru[0]).max() <= TOL * max(1.0, np.abs(ru[0]).max())
                assert np.abs(u4[i] - ru[4]).max() <= TOL * max(1.0, np.abs(ru[4]).max())
            assert listed.size > 0
            del A, Bm, _b
        f.close()
    (xa, ua), sa, ca = res[0]
    (xb, ub), sb, cb = res[1]
    assert np.array_equal(xa, xb) and np.array_equal(ua, ub) and np.array_equal(ca, cb)
    for a, b in zip(sa, sb):
        assert np.array_equal(a, b)


# ---- 7. acados-named drop-in -------------------------------------------------------------------------------------------------
def test_dropin(oracle):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from crazyflie_nmpc_amd import _lib
    _lib.lib()
    L = C.CDLL(os.path.join(root, "crazyflie_nmpc_amd", "libacados_solver_crazyflie.so"))
    vp = C.c_void_p
    L.ocp_nlp_out_create.restype = vp
    L.ocp_nlp_out_create.argtypes = [vp, vp]
    L.ocp_nlp_out_destroy.argtypes = [vp]
    L.ocp_nlp_out_destroy.restype = None
    L.ocp_nlp_eval_param_sens.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, vp]
    L.ocp_nlp_eval_param_sens.restype = None
    L.ocp_nlp_out_get.argtypes = [vp, vp, vp, C.c_int, C.c_char_p, vp]
    L.ocp_nlp_out_get.restype = None
    N = 50
    s = _solver(1, N)
    x0 = _setup(oracle, s, 61, 2.5)
    yr, ye = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    s.init_iterate(0)   # (acados_create's iterate)
    s.solve(1)
    s.eval_sens_x0()
    du, dx, _act = _engine(s)

    def read(out, k, field, n):
        v = np.empty(n)
        L.ocp_nlp_out_get(None, None, out, k, field, v.ctypes.data_as(vp))
        return v

    assert L.acados_create() == 0
    o = None
    try:
        xk = np.ascontiguousarray(x0[0])
        for f in (b"lbx", b"ubx"):
            assert L.ocp_nlp_constraints_model_set(None, None, None, 0, f, xk.ctypes.data_as(vp)) == 0
        for k in range(N):
            r = np.ascontiguousarray(yr[k])
            assert L.ocp_nlp_cost_model_set(None, None, None, k, b"yref", r.ctypes.data_as(vp)) == 0
        r = np.ascontiguousarray(ye)
        assert L.ocp_nlp_cost_model_set(None, None, None, N, b"yref", r.ctypes.data_as(vp)) == 0
        assert L.acados_solve() == 0
        u_before = [read(None, k, b"u", 4) for k in range(N)]
        x_before = [read(None, k, b"x", 13) for k in range(N + 1)]
        o = L.ocp_nlp_out_create(None, None)
        assert o
        assert np.isnan(read(o, 0, b"u", 4)).all()
        for j in range(13):
            L.ocp_nlp_eval_param_sens(None, b"ex", 0, j, o)
            for k in range(N):
                assert np.array_equal(read(o, k, b"u", 4), du[0, k, :, j]), (j, k)
            for k in range(N + 1):
                assert np.array_equal(read(o, k, b"x", 13), dx[0, k, :, j]), (j, k)
        for args in ((b"p", 0, 0), (b"ex", 1, 0), (b"ex", 0, 13), (b"ex", 0, -1)):
            L.ocp_nlp_eval_param_sens(None, *args, o)
            assert np.isnan(read(o, 3, b"u", 4)).all() and np.isnan(read(o, 3, b"x", 13)).all(), args
        for k in range(N):
            assert np.array_equal(read(None, k, b"u", 4), u_before[k])
        for k in range(N + 1):
            assert np.array_equal(read(None, k, b"x", 13), x_before[k])
    finally:
        if o:
            L.ocp_nlp_out_destroy(o)
        L.acados_free()
        s.close()


# ---- 6. fleet and multi ------------------------------------------------------------------------------------------------------
def _fleet_inputs(oracle, B, Nm, seed):
    rng = np.random.default_rng(seed)
    x0 = oracle.sample_hover_x0(rng, B, scale=2.5)
    yr, ye = oracle.regulation_yref(Nm, (0.0, 0.0, 0.4))
    return x0, np.repeat(yr[None], B, 0).copy(), np.repeat(ye[None], B, 0).copy()


def _host_sens(getter, h, stage, ns, B, with_u, *extra):
    du = np.empty((B, ns, 4, 13)) if with_u else None
    dx = np.empty((B, ns, 13, 13))
    rc = getter(h, stage, ns, None if du is None else du.ctypes.data_as(C.c_void_p), dx.ctypes.data_as(C.c_void_p), *extra)
    assert rc == 0, rc
    return du, dx


def test_fleet_equals_buckets(oracle):
    """the fleet's rows, in vehicle order, are its bucket solvers' rows bit for bit; range limited by the shortest horizon"""
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    hz = np.random.default_rng(3).choice([30, 50, 100], 160).astype(np.int32)
    B, Nm = len(hz), 100
    x0, yr, ye = _fleet_inputs(oracle, B, Nm, 4)
    f = MixedHorizonFleet(hz)
    f.set_x0(x0); f.set_yref(yr, ye); f.init_iterate(INIT_HOVER)
    f.solve(2)
    f.eval_sens_x0()
    L, Nmin = f._L, f.Nmin
    fu, _ = f.sens_x0(0, Nmin)
    _, fx = f.sens_x0(0, Nmin + 1)
    gu, gx = f.sens_x0(0)
    assert np.array_equal(gu, fu[:, 0]) and np.array_equal(gx, fx[:, 0])
    # device outputs take the other path of cfnmpc_fleet_get_sens_x0 (per-bucket staging + scatter)
    import torch
    tu = torch.empty((B, Nmin, 4, 13), dtype=torch.float64, device="cuda")
    tx = torch.empty((B, Nmin, 13, 13), dtype=torch.float64, device="cuda")
    f.sens_x0(0, Nmin, out_u=tu, out_x=tx)
    torch.cuda.synchronize()
    assert np.array_equal(tu.cpu().numpy(), fu) and np.array_equal(tx.cpu().numpy(), fx[:, :Nmin])
    for b, (N, idx) in enumerate(f.buckets()):
        sv = C.c_void_p()
        assert L.cfnmpc_fleet_bucket(f._h, b, None, None, C.byref(sv), None) == 0
        su, _ = _host_sens(L.cfnmpc_get_sens_x0, sv, 0, Nmin, len(idx), True, 0, None)
        _, sx = _host_sens(L.cfnmpc_get_sens_x0, sv, 0, Nmin + 1, len(idx), False, 0, None)
        assert np.array_equal(su, fu[idx]) and np.array_equal(sx, fx[idx]), N
    with pytest.raises(Exception):
        f.sens_x0(0, Nmin + 2)   # beyond the shortest horizon
    assert f.sens_x0(0, Nmin + 1)[0] is None   # (du: below the shortest horizon only)
    f.close()


def test_multi_two_shards(oracle):
    """contiguous shards: the multi's rows are its shard solvers' rows bit for bit; against ONE solver of the whole fleet the
    sensitivities agree to rounding where the active sets agree (the RTI iterates of the two batch sizes already differ in
    the last bits: engine kernels pick their work decomposition by batch)"""
    from crazyflie_nmpc_amd import default_opts
    from crazyflie_nmpc_amd.parallel import MultiGpuFleet
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B, N = 128, 50
    x0, yr, ye = _fleet_inputs(oracle, B, N, 5)
    m = MultiGpuFleet(B, [0, 0], opts=default_opts())
    m.set_x0(x0); m.set_yref(yr, ye); m.init_iterate(INIT_HOVER)
    m.solve(2); m.sync()
    m.eval_sens_x0()
    L = m._L
    mu, _ = m.sens_x0(0, N)
    _, mx = m.sens_x0(0, N + 1)
    for i in range(L.cfnmpc_multi_num_shards(m._h)):
        sv, lo, hi = C.c_void_p(), C.c_int(), C.c_int()
        assert L.cfnmpc_multi_shard(m._h, i, C.byref(sv), C.byref(lo), C.byref(hi), None, None) == 0
        n = hi.value - lo.value
        su, _ = _host_sens(L.cfnmpc_get_sens_x0, sv, 0, N, n, True, 0, None)
        _, sx = _host_sens(L.cfnmpc_get_sens_x0, sv, 0, N + 1, n, False, 0, None)
        assert np.array_equal(su, mu[lo.value:hi.value]) and np.array_equal(sx, mx[lo.value:hi.value]), i
    u4, x4 = m.sens_x0(4)
    assert np.array_equal(u4, mu[:, 4]) and np.array_equal(x4, mx[:, 4])
    s = _solver(B, N)
    s.set_x0(x0); s.set_yref(yr, ye); s.init_iterate(INIT_HOVER)
    s.solve(2)
    s.eval_sens_x0()
    su, _ = s.sens_x0(0, N)
    act = s.sens_active()
    # (the multi's active set: the shard solvers')
    same = []
    for i in range(L.cfnmpc_multi_num_shards(m._h)):
        sv, lo, hi = C.c_void_p(), C.c_int(), C.c_int()
        assert L.cfnmpc_multi_shard(m._h, i, C.byref(sv), C.byref(lo), C.byref(hi), None, None) == 0
        a = np.empty((hi.value - lo.value, N, 4), dtype=np.int8)
        assert L.cfnmpc_get_sens_active(sv, a.ctypes.data_as(C.c_void_p), 0, None) == 0
        same += [np.array_equal(a[r], act[lo.value + r]) for r in range(a.shape[0])]
    same = np.array(same)
    assert same.mean() >= 0.9
    assert np.abs(mu[same] - su[same]).max() <= ROUTE_TOL * max(1.0, np.abs(su[same]).max())
    s.close()


def test_multi_horizons(oracle):
    """mixed-horizon shards: the multi's rows, in the caller's order, are its shard fleets' rows bit for bit"""
    from crazyflie_nmpc_amd.parallel import MultiGpuFleet
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    hz = np.random.default_rng(6).choice([30, 50, 100], 120).astype(np.int32)
    B, Nm = len(hz), 100
    x0, yr, ye = _fleet_inputs(oracle, B, Nm, 7)
    m = MultiGpuFleet(B, [0, 0], horizons=hz)
    m.set_x0(x0); m.set_yref(yr, ye); m.init_iterate(INIT_HOVER)
    m.solve(2); m.sync()
    m.eval_sens_x0()
    L, Nmin = m._L, int(hz.min())
    mu, _ = m.sens_x0(0, Nmin)
    _, mx = m.sens_x0(0, Nmin + 1)
    seen = np.zeros(B, bool)
    for i in range(L.cfnmpc_multi_num_shards(m._h)):
        fl, cnt = C.c_void_p(), C.c_int()
        assert L.cfnmpc_multi_shard_fleet(m._h, i, C.byref(fl), C.byref(cnt), None, None, None) == 0
        idx = np.empty(cnt.value, dtype=np.int32)
        assert L.cfnmpc_multi_shard_fleet(m._h, i, None, None, idx.ctypes.data_as(C.c_void_p), None, None) == 0
        fu, _ = _host_sens(L.cfnmpc_fleet_get_sens_x0, fl, 0, Nmin, cnt.value, True, 0, None)
        _, fx = _host_sens(L.cfnmpc_fleet_get_sens_x0, fl, 0, Nmin + 1, cnt.value, False, 0, None)
        assert np.array_equal(fu, mu[idx]) and np.array_equal(fx, mx[idx]), i
        seen[idx] = True
    assert seen.all()
    g0, _ = m.sens_x0(0)
    assert np.array_equal(g0, mu[:, 0])
    with pytest.raises(Exception):
        m.sens_x0(0, Nmin + 2)
