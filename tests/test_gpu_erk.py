"""GPU suite: ERK sub-steps per shooting interval and stage-cost scaling (include/cfnmpc.h: cfnmpc_set_erk_steps /
cfnmpc_set_cost_scaling).

References are built here from the oracle's public functions: the M-step blocks by chaining cref.rk4_sens over dt / M
(A = A_M..A_1, B = sum_j A_M..A_{j+1} B_j, Phi = the last state), the QP of one RTI step by oracle.qp_from_blocks with those
blocks and the (scaled) weights, solved by oracle.solve_qp_dense, with oracle.solve_qp_refined as the referee where the two
FP64 sides disagree."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HOV = 15.777730167256925
DT = 0.015
QP_TOL = 1e-11


def _inputs(oracle, B, N, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    x0 = oracle.sample_hover_x0(rng, B, scale=scale)
    yr, ye = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    return x0, np.repeat(yr[None], B, 0).copy(), np.repeat(ye[None], B, 0).copy()


def _chain(cref, x, u, dt, M):
    A = np.eye(13)
    Bm = np.zeros((13, 4))
    xs = np.asarray(x, dtype=np.float64)
    for _ in range(M):
        xs, Aj, Bj = cref.rk4_sens(xs, u, dt / M)
        A = Aj @ A
        Bm = Aj @ Bm + Bj
    return xs, A, Bm


def _blocks(cref, x, u, M, dt=DT):
    """composed blocks of one instance's iterate: A [N][13][13], B [N][13][4], b [N][13]"""
    N = u.shape[0]
    A = np.empty((N, 13, 13)); Bm = np.empty((N, 13, 4)); b = np.empty((N, 13))
    for k in range(N):
        phi, A[k], Bm[k] = _chain(cref, x[k], u[k], dt, M)
        b[k] = phi - x[k + 1]
    return A, Bm, b


def _solver(B, M=1, scale=None, **kw):
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    s = BatchSolver(B, default_opts(**kw))
    if M != 1:
        s.set_erk_steps(M)
    if scale is not None:
        s.set_cost_scaling(*scale)
    return s


def _ref_step(cref, oracle, x, u, x0, yref, yref_e, M, W, WN, u_min=0.0, u_max=22.0, lb=None, ub=None):
    """one RTI step of one instance from iterate (x, u) with the composed M-step blocks -> (x_new, u_new, qp)"""
    A, Bm, b = _blocks(cref, x, u, M)
    W = np.asarray(W); WN = np.asarray(WN)
    q = np.empty((x.shape[0], 13))
    q[:-1] = W[:13] * (x[:-1] - yref[:, :13])
    q[-1] = WN * (x[-1] - yref_e)
    r = W[13:] * (u - yref[:, 13:])
    lo = (u_min if lb is None else lb) - u
    hi = (u_max if ub is None else ub) - u
    qp = oracle.qp_from_blocks(A, Bm, b, q, r, x0 - x[0], W[:13], W[13:], WN, lo, hi)
    sol = oracle.solve_qp_dense(qp)
    return x + sol["dx"], u + sol["du"], qp


def _agree(oracle, xg, ug, xr, ur, qp, x, u, tol):
    """engine iterate vs the dense solution; the refined referee decides where the two FP64 sides disagree"""
    e = max(np.abs(xg - xr).max(), np.abs(ug - ur).max())
    if e <= tol:
        return e
    ref = oracle.solve_qp_refined(qp)
    return max(np.abs(xg - (x + ref["dx"])).max(), np.abs(ug - (u + ref["du"])).max())


# ---- 1. linearisation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 3, 4])
@pytest.mark.parametrize("B,start", [(256, "hover"), (100, "random")])
def test_linearisation_matches_composed_blocks(cref, oracle, M, B, start):
    N = 50
    rng = np.random.default_rng(100 + M + B)
    x0, yr, ye = _inputs(oracle, B, N, 7 + M, scale=1.5)
    if start == "hover":
        x = np.repeat(x0[:, None, :], N + 1, 1) + rng.normal(0, 1e-2, (B, N + 1, 13))
        u = HOV + rng.normal(0, 1.0, (B, N, 4))
    else:
        x = np.repeat(x0[:, None, :], N + 1, 1) + rng.normal(0, 0.3, (B, N + 1, 13))
        x[:, :, 3:7] /= np.linalg.norm(x[:, :, 3:7], axis=2, keepdims=True)
        x[:, :, 10:13] += rng.normal(0, 3.0, (B, N + 1, 3))
        u = rng.uniform(0.0, 22.0, (B, N, 4))
    s = _solver(B, M)
    s.set_x0(x0); s.set_yref(yr, ye); s.set_iterate(x, u)
    s.linearise_only()
    A, Bm, b = s.get_linearisation()
    for i in rng.choice(B, 24, replace=False):
        Ar, Br, br = _blocks(cref, x[i], u[i], M)
        assert np.abs(A[i] - Ar).max() <= 1e-12 * max(1.0, np.abs(Ar).max()), (i, np.abs(A[i] - Ar).max())
        assert np.abs(Bm[i] - Br).max() <= 1e-12 * max(1.0, np.abs(Br).max()), (i, np.abs(Bm[i] - Br).max())
        assert np.abs(b[i] - br).max() <= 1e-12 * max(1.0, np.abs(x[i]).max()), (i, np.abs(b[i] - br).max())


# ---- 2. M = 1 is today -----------------------------------------------------------------------------------------------
def _closed_loop(s, oracle, x0, yr, ye, steps, seed):
    rng = np.random.default_rng(seed)
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    s.set_x0(x0); s.set_yref(yr, ye); s.init_iterate(INIT_HOVER)
    x = x0.copy()
    out = []
    for j in range(steps):
        s.set_x0(x)
        s.solve(1)
        u0 = s.get_u(0); u1 = s.get_u(1); x4 = s.get_x(4)
        out.append((u0, u1, x4) + tuple(s.stats()))
        x = np.stack([oracle.rk4(x[i], u0[i], DT) for i in range(x.shape[0])])
        if j % 3 == 1:
            x[:, 7:10] += rng.normal(0, 0.5, (x.shape[0], 3))     # kicks
    xi, ui = s.get_iterate()
    return out, xi, ui


def test_m1_is_bitwise_today(oracle):
    B, N = 1024, 50
    x0, yr, ye = _inputs(oracle, B, N, 21, scale=1.5)
    a = _solver(B)
    b = _solver(B)
    b.set_erk_steps(1)
    b.set_cost_scaling(1.0, 1.0)
    assert b.erk_steps == 1
    ra, xa, ua = _closed_loop(a, oracle, x0, yr, ye, 10, 5)
    rb, xb, ub = _closed_loop(b, oracle, x0, yr, ye, 10, 5)
    for p, q in zip(ra, rb):
        for v, w in zip(p, q):
            assert np.array_equal(v, w)
    assert np.array_equal(xa, xb) and np.array_equal(ua, ub)


# ---- 3. RTI parity at M = 2 ------------------------------------------------------------------------------------------
VARIANTS = [
    dict(active_set=1),
    dict(active_set=0),
    dict(active_set=1, as_dense=0),
    dict(active_set=1, as_dense=1, forward_sweep=1),
    dict(active_set=1, forward_sweep=2),
    dict(active_set=1, forward_split=1),
    dict(active_set=1, cond_N2=10),
    dict(active_set=1, step_graph=1),
    dict(active_set=1, _sbox=True),
]


def test_rti_parity_m2(cref, oracle):
    """every variant steps from the same iterate (variant 0's result of the step before); 12 sampled rows per step against
    the composed-block QP"""
    from crazyflie_nmpc_amd import default_opts
    B, N, M = 128, 50, 2
    x0, yr, ye = _inputs(oracle, B, N, 31, scale=2.0)
    W = np.array(default_opts().W); WN = np.array(default_opts().WN)
    rng = np.random.default_rng(9)
    lb = np.zeros((B, N, 4)); ub = np.full((B, N, 4), 22.0)
    ub[:, :5, :] = 20.0                                     # per-stage boxes of the _sbox variant
    sv = []
    for v in VARIANTS:
        v = dict(v)
        sbox = v.pop("_sbox", False)
        s = _solver(B, M, tol=QP_TOL, **v)          # (the interior point to a tight tolerance: its rows compare as well)
        s.set_yref(yr, ye)
        if sbox:
            s.set_box_stages(lb, ub)
        sv.append((s, sbox))
    x = np.repeat(x0[:, None, :], N + 1, 1).copy(); u = np.full((B, N, 4), HOV)
    xc = x0.copy()
    n_con = 0
    for j in range(10):
        rows = rng.choice(B, 12, replace=False)
        ref, ref_sb = {}, {}
        nxt = None
        for s, sbox in sv:
            s.set_x0(xc); s.set_iterate(x, u)
            s.solve(1)
            xg, ug = s.get_iterate()
            if nxt is None:
                nxt = (xg, ug)
                n_con += int(np.any((ug <= 1e-9) | (ug >= 22.0 - 1e-9), axis=(1, 2)).sum())
            for i in rows:
                d = ref_sb if sbox else ref
                if i not in d:
                    d[i] = _ref_step(cref, oracle, x[i], u[i], xc[i], yr[i], ye[i], M, W, WN,
                                     lb=lb[i] if sbox else None, ub=ub[i] if sbox else None)
                a, c, qp = d[i]
                e = _agree(oracle, xg[i], ug[i], a, c, qp, x[i], u[i], 5e-8)
                assert e <= 5e-8, (j, i, e, sbox, s.opts.active_set, s.opts.forward_sweep)
        x, u = nxt
        xc = np.stack([oracle.rk4(xc[i], u[i, 0], DT) for i in range(B)])
        xc[:, 7:10] += rng.normal(0, 0.8, (B, 3))
    assert n_con > 0                                        # some rows ran into the box


# ---- 4. forward sweeps agree -----------------------------------------------------------------------------------------
def test_forward_sweeps_agree_m3(oracle):
    B, N = 300, 50
    x0, yr, ye = _inputs(oracle, B, N, 41, scale=1.5)
    res = []
    for fs in (1, 2):
        s = _solver(B, 3, forward_sweep=fs, active_set=1)
        from crazyflie_nmpc_amd.solver import INIT_HOVER
        s.set_x0(x0); s.set_yref(yr, ye); s.init_iterate(INIT_HOVER)
        s.solve(1)
        res.append(s.get_iterate())
    assert np.abs(res[0][0] - res[1][0]).max() < 1e-9
    assert np.abs(res[0][1] - res[1][1]).max() < 1e-8


# ---- 5. SQP at M = 2 -------------------------------------------------------------------------------------------------
def test_sqp_m2_reaches_phi2(oracle):
    """(full-step SQP without globalisation: a few rows of a random set oscillate at any M -- the same rows at M = 1; the
    converged ones are checked)"""
    B, N, tol = 64, 50, 1e-8
    x0, yr, ye = _inputs(oracle, B, N, 51, scale=1.0)
    s = _solver(B, 2, tol=QP_TOL)
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    s.set_x0(x0); s.set_yref(yr, ye); s.init_iterate(INIT_HOVER)
    s.solve_sqp(100, tol, tol, tol)
    st, it, rs = s.sqp_stats()
    ok = np.flatnonzero(st == 0)
    assert ok.size >= 0.75 * B, st
    assert (rs[ok, 1] <= tol).all()
    x, u = s.get_iterate()
    d2 = d1 = 0.0
    for i in ok:
        for k in range(N):
            d2 = max(d2, np.abs(x[i, k + 1] - oracle.rk4(x[i, k], u[i, k], DT, steps=2)).max())
            d1 = max(d1, np.abs(x[i, k + 1] - oracle.rk4(x[i, k], u[i, k], DT, steps=1)).max())
    assert d2 <= tol, d2
    assert d1 > 100 * tol, d1                               # the option reaches k_sqp_check


# ---- 6. cost scaling -------------------------------------------------------------------------------------------------
def test_cost_scaling(cref, oracle):
    from crazyflie_nmpc_amd import default_opts
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B, N = 256, 50
    x0, yr, ye = _inputs(oracle, B, N, 61, scale=1.5)
    W = np.array(default_opts().W); WN = np.array(default_opts().WN)

    def run(s, steps=3):
        s.set_x0(x0); s.set_yref(yr, ye); s.init_iterate(INIT_HOVER)
        s.solve(steps)
        return s.get_iterate()

    a = _solver(B, scale=(DT, 1.0))
    b = _solver(B)
    b.set_weights(DT * W, WN)
    xa, ua = run(a); xb, ub = run(b)
    assert np.array_equal(xa, xb) and np.array_equal(ua, ub)
    # matches the restatement with scaled weights
    co = cref.default_opts(N=N, active_set=1, W=DT * W, WN=WN)
    xr = np.repeat(x0[:, None, :], N + 1, 1).copy(); ur = np.full((B, N, 4), HOV)
    for _ in range(3):
        cref.rti_step(co, xr, ur, x0.copy(), yr, ye, nthreads=0)
    assert max(np.abs(xa - xr).max(), np.abs(ua - ur).max()) < 1e-7
    # survives a later set_weights: scale (2, 3) then new weights == pre-scaled weights
    c = _solver(B, scale=(2.0, 3.0))
    c.set_weights(0.5 * W, 0.25 * WN)
    d = _solver(B)
    d.set_weights(2.0 * (0.5 * W), 3.0 * (0.25 * WN))
    xc, uc = run(c); xd, ud = run(d)
    assert np.array_equal(xc, xd) and np.array_equal(uc, ud)
    # changes the answer
    xu, uu = run(_solver(B))
    assert np.abs(ua[:, 0] - uu[:, 0]).max() > 1e-3


# ---- 7. fleet / multi / drop-in --------------------------------------------------------------------------------------
def test_fleet_m2_equals_buckets(oracle):
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    rng = np.random.default_rng(71)
    hz = rng.choice([30, 50, 100], 200).astype(np.int32)
    f = MixedHorizonFleet(hz)
    f.set_erk_steps(2)
    f.set_cost_scaling(DT, 1.0)
    B, Nm = len(hz), 100
    x0 = oracle.sample_hover_x0(rng, B, scale=1.5)
    yr, ye = oracle.regulation_yref(Nm, (0.0, 0.0, 0.4))
    yrf = np.repeat(yr[None], B, 0).copy(); yef = np.repeat(ye[None], B, 0).copy()
    f.set_x0(x0); f.set_yref(yrf, yef); f.init_iterate(INIT_HOVER)
    f.solve(2)
    for N, idx, xb, ub in f.bucket_iterates():
        s = _solver(len(idx), 2, scale=(DT, 1.0), N=N)
        s.set_x0(x0[idx]); s.set_yref(yrf[idx, :N].copy(), yef[idx]); s.init_iterate(INIT_HOVER)
        s.solve(2)
        xs, us = s.get_iterate()
        assert np.array_equal(xs, xb) and np.array_equal(us, ub), N


def test_multi_one_shard_equals_solver(oracle):
    from crazyflie_nmpc_amd.parallel import MultiGpuFleet
    from crazyflie_nmpc_amd import default_opts
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B, N = 128, 50
    x0, yr, ye = _inputs(oracle, B, N, 81, scale=1.5)
    m = MultiGpuFleet(B, [0], opts=default_opts())
    m.set_erk_steps(2); m.set_cost_scaling(DT, 1.0)
    m.set_x0(x0); m.set_yref(yr, ye); m.init_iterate(INIT_HOVER)
    m.solve(2); m.sync()
    s = _solver(B, 2, scale=(DT, 1.0))
    s.set_x0(x0); s.set_yref(yr, ye); s.init_iterate(INIT_HOVER)
    s.solve(2)
    assert np.array_equal(m.get_u(0), s.get_u(0))
    assert np.array_equal(m.get_x(4), s.get_x(4))


def test_dropin_settings(oracle):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from crazyflie_nmpc_amd import _lib
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    _lib.lib()
    L = C.CDLL(os.path.join(root, "crazyflie_nmpc_amd", "libacados_solver_crazyflie.so"))
    vp = C.c_void_p
    L.ocp_nlp_solver_opts_set.argtypes = [vp, vp, C.c_char_p, vp]
    L.ocp_nlp_solver_opts_set.restype = None
    N = 50
    x0, yr, ye = _inputs(oracle, 1, N, 91, scale=2.0)
    assert L.acados_create() == 0
    try:
        xk = np.ascontiguousarray(x0[0])
        for f in (b"lbx", b"ubx"):
            assert L.ocp_nlp_constraints_model_set(None, None, None, 0, f, xk.ctypes.data_as(vp)) == 0
        for k in range(N):
            r = np.ascontiguousarray(yr[0, k])
            assert L.ocp_nlp_cost_model_set(None, None, None, k, b"yref", r.ctypes.data_as(vp)) == 0
        r = np.ascontiguousarray(ye[0])
        assert L.ocp_nlp_cost_model_set(None, None, None, N, b"yref", r.ctypes.data_as(vp)) == 0
        ns = C.c_int(2)
        L.ocp_nlp_solver_opts_set(None, None, b"sim_method_num_steps", C.cast(C.pointer(ns), vp))
        sc = np.array([DT]); one = np.array([1.0])
        for k in range(N):
            assert L.ocp_nlp_cost_model_set(None, None, None, k, b"scaling", sc.ctypes.data_as(vp)) == 0
        assert L.ocp_nlp_cost_model_set(None, None, None, N, b"scaling", one.ctypes.data_as(vp)) == 0
        bad = np.array([0.0])
        assert L.ocp_nlp_cost_model_set(None, None, None, 3, b"scaling", bad.ctypes.data_as(vp)) == 1
        assert L.acados_cfnmpc_init_iterate(1) == 0
        assert L.acados_solve() == 0
        u = np.empty(4); x4 = np.empty(13)
        L.ocp_nlp_out_get(None, None, None, 0, b"u", u.ctypes.data_as(vp))
        L.ocp_nlp_out_get(None, None, None, 4, b"x", x4.ctypes.data_as(vp))
        s = _solver(1, 2, scale=(DT, 1.0))
        s.set_x0(x0); s.set_yref(yr, ye); s.init_iterate(INIT_HOVER)
        s.solve(1)
        assert np.array_equal(u, s.get_u(0)[0]) and np.array_equal(x4, s.get_x(4)[0])
        # disagreeing stage scalings: refused without solving
        sc2 = np.array([2 * DT])
        assert L.ocp_nlp_cost_model_set(None, None, None, 7, b"scaling", sc2.ctypes.data_as(vp)) == 0
        assert L.acados_solve() == 1
        assert L.ocp_nlp_cost_model_set(None, None, None, 7, b"scaling", sc.ctypes.data_as(vp)) == 0
        ns9 = C.c_int(9)
        L.ocp_nlp_solver_opts_set(None, None, b"sim_method_num_steps", C.cast(C.pointer(ns9), vp))
        assert L.acados_solve() == 1
    finally:
        L.acados_free()


# ---- 8. validation ---------------------------------------------------------------------------------------------------
def test_validation():
    from crazyflie_nmpc_amd.solver import CfnmpcError
    s = _solver(64, 3, scale=(0.5, 2.0))
    for n in (0, 9, -1):
        with pytest.raises(CfnmpcError):
            s.set_erk_steps(n)
    assert s.erk_steps == 3
    for a, b in ((0.0, 1.0), (1.0, 0.0), (-1.0, 1.0), (float("nan"), 1.0), (1.0, float("inf"))):
        with pytest.raises(CfnmpcError):
            s.set_cost_scaling(a, b)
    # the fused start solve keeps one step per interval: M > 1 refused
    for ss in (2, 3):
        f = _solver(256, start_solve=ss)
        with pytest.raises(CfnmpcError):
            f.set_erk_steps(2)
        assert f.erk_steps == 1
        f.set_erk_steps(1)


# ---- 9. full size ----------------------------------------------------------------------------------------------------
def test_full_size_m2(cref, oracle):
    from crazyflie_nmpc_amd import default_opts
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B, N, M = 65536, 50, 2
    x0, yr, ye = _inputs(oracle, B, N, 99, scale=1.0)
    s = _solver(B, M, tol=QP_TOL)
    s.set_x0(x0); s.set_yref(yr, ye); s.init_iterate(INIT_HOVER)
    W = np.array(default_opts().W); WN = np.array(default_opts().WN)
    rng = np.random.default_rng(5)
    xc = x0.copy()
    ok = 0
    rows = rng.choice(B, 64, replace=False)
    for j in range(20):
        s.set_x0(xc)
        last = j == 19
        if last:
            xp, up = s.get_iterate()
        s.solve(1)
        st, _, _ = s.stats()
        ok += int((st == 0).sum())
        u0 = s.get_u(0)
        if last:
            xg, ug = s.get_iterate()
            for i in rows:
                xr, ur, qp = _ref_step(cref, oracle, xp[i], up[i], xc[i], yr[i], ye[i], M, W, WN)
                assert _agree(oracle, xg[i], ug[i], xr, ur, qp, xp[i], up[i], 5e-8) <= 5e-8, i
        xc = np.asarray(cref.sim(xc, u0, DT, 1))
    assert ok / (20 * B) >= 0.99
