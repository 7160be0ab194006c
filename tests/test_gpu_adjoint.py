"""GPU suite: adjoint solution sensitivities (include/cfnmpc.h: cfnmpc_eval_adjoint, cfnmpc_get_adjoint,
cfnmpc_get_adjoint_cost and the fleet / multi entries; crazyflie_nmpc_amd/diff.py).

The reference is the numpy recursion of tests/test_adjoint_cpu.py (checked there against a dense KKT solve, central differences
of the extended-precision QP solution and the forward sensitivities), run on the engine's own blocks
(cfnmpc_debug_get_linearisation), weights, references, iterate and active set (cfnmpc_get_sens_active).

TOL: the worst per-stage relative error (DESIGN.md section 5.14's definition: max over stages of |a_k - b_k| / max(1, |b_k|))
of any output against adjoint_ref over the cases of test_against_reference (B = 256, kicks x 3, random gradients) was measured
on an MI355X as 9.8e-12 at N = 5, 1.6e-11 at N = 20 and 3.73e-10 at N = 50 (MEASURED_WORST); the bound is ten times the
worst, 3.73e-9.  By the same rule ID_TOL = 2.36e-11 for the identity with the engine's own sens_x0 (measured 2.36e-12,
MEASURED_ID; the unit loss: 5.5e-13).  One route is ill-conditioned enough for the reference's own FP64 rounding to matter
(weight rows with cost scaling (dt, 1): engine against numpy 1.5e-8, numpy against its extended-precision twin 5.2e-9); its
bound is ten times the reference's own rounding, measured inside the test (_check(ref_error=True))."""
import ctypes as C

import numpy as np
import pytest

from test_adjoint_cpu import adjoint_ref, gradients
from test_gpu_sens import _boxes, _fleet_inputs, _per_stage_err, _setup, _solver

pytestmark = pytest.mark.gpu
DT = 0.015
MEASURED_WORST, MEASURED_ID = 3.73e-10, 2.36e-12
TOL = 10 * MEASURED_WORST
ID_TOL = 10 * MEASURED_ID
STAGED = ("dq", "dr", "db", "dbox", "dyref")      # outputs with a stage axis
FLAT = ("dx0", "dW", "dWN", "dyref_e")


def _outputs(s):
    dx0, dq, dr, db, dbox = s.adjoint()
    dW, dWN, dyref, dyref_e = s.adjoint_cost()
    return dict(dx0=dx0, dq=dq, dr=dr, db=db, dbox=dbox, dW=dW, dWN=dWN, dyref=dyref, dyref_e=dyref_e)


def _eff_weights(s, stage_scale=1.0, terminal_scale=1.0):
    """-> effective rows Qd [B][13], Rd [B][4], QNd [B][13]"""
    W, WN = s.weights_batch()
    return stage_scale * W[:, :13], stage_scale * W[:, 13:], terminal_scale * WN


def _grads(s, seed, n_gx=None, n_gu=None):
    rng = np.random.default_rng(seed)
    n_gx = s.N + 1 if n_gx is None else n_gx
    n_gu = s.N if n_gu is None else n_gu
    return rng.normal(size=(s.B, n_gx, 13)), rng.normal(size=(s.B, n_gu, 4))


def _pad(g, n, w):
    out = np.zeros((n, w))
    if g is not None:
        out[:g.shape[0]] = g
    return out


def _reference(s, i, lin, weights, act, gx, gu, it, yr, scales=(1.0, 1.0), dtype=np.float64):
    A, Bm = lin
    Qd, Rd, QNd = (w[i] for w in weights)
    g_x = _pad(None if gx is None else gx[i], s.N + 1, 13)
    g_u = _pad(None if gu is None else gu[i], s.N, 4)
    r = adjoint_ref(A[i], Bm[i], Qd, Rd, QNd, act[i], g_x, g_u, dtype=dtype)
    r = {k: v.astype(np.float64) for k, v in r.items()}
    return gradients(r, act[i], Qd, Rd, QNd, it[0][i], it[1][i], yr[0][i], yr[1][i], *scales)


def _errors(out, ref, i):
    e = {k: _per_stage_err(out[k][i], ref[k]) for k in STAGED}
    e.update({k: float(np.abs(out[k][i] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())) for k in FLAT})
    return e


def _check(s, out, gx, gu, scales=(1.0, 1.0), rows=None, status=None, ref_error=False):
    """every output of both getters against the reference on the engine's own data -> (rows compared, worst error by output).
    ref_error: the bound is TOL or ten times the reference's own rounding -- its FP64 evaluation against its extended-precision
    one on the same data --, whichever is larger (the ill-conditioned routes)"""
    A, Bm, _b = s.get_linearisation()
    act = s.sens_active()
    weights = _eff_weights(s, *scales)
    it, yr = s.get_iterate(), s.yref()
    status = s.stats()[0] if status is None else status
    worst, own = {}, 0.0
    n = 0
    for i in (range(s.B) if rows is None else rows):
        if status[i] == 4:
            assert all(np.isnan(out[k][i]).all() for k in out), i
            continue
        ref = _reference(s, i, (A, Bm), weights, act, gx, gu, it, yr, scales)
        for k, e in _errors(out, ref, i).items():
            worst[k] = max(worst.get(k, 0.0), e)
        if ref_error and n < 32:
            ext = _reference(s, i, (A, Bm), weights, act, gx, gu, it, yr, scales, dtype=np.longdouble)
            own = max(own, max(_errors({k: v[None] for k, v in ref.items()}, ext, 0).values()))
        assert np.all(out["dbox"][i][act[i] == 0] == 0.0) and np.all(out["dr"][i][act[i] != 0] == 0.0), i
        assert np.all(out["dq"][i][0] == 0.0), i
        n += 1
    tol = max(TOL, 10 * own)
    print("worst per-stage relative error by output:", {k: f"{v:.2e}" for k, v in worst.items()},
          f"bound {tol:.2e}" + (f" (the reference's own rounding over 32 rows: {own:.2e})" if ref_error else ""))
    assert max(worst.values()) <= tol, (worst, tol)
    return n, worst


# ---- 1. engine against the numpy reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 20, 50])
def test_against_reference(oracle, N):
    s = _solver(256, N)
    _setup(oracle, s, 10 + N, 3.0)
    s.solve(2)
    s.eval_sens_x0()
    gx, gu = _grads(s, N)
    s.eval_adjoint(gx, gu)
    out = _outputs(s)
    share = float((s.sens_active() != 0).any(axis=(1, 2)).mean())
    assert share >= 0.2, share
    n, worst = _check(s, out, gx, gu)
    print(f"N = {N}: {n} rows, active share {share:.2f}, worst {max(worst.values()):.2e}")
    assert n >= 200
    s.close()


@pytest.fixture(scope="module")
def solved(oracle):
    """B = 256, N = 20, kicks x 3 after two steps, sensitivities evaluated: shared by the tests that only evaluate adjoints"""
    s = _solver(256, 20)
    _setup(oracle, s, 30, 3.0)
    s.solve(2)
    s.eval_sens_x0()
    yield s
    s.close()


def test_identity_with_sens_x0(solved):
    s = solved
    gx, gu = _grads(s, 2)
    s.eval_adjoint(gx, gu)
    dx0 = s.adjoint()[0]
    du, _ = s.sens_x0(0, s.N)
    _, dx = s.sens_x0(0, s.N + 1)
    want = np.einsum("bkij,bki->bj", dx, gx) + np.einsum("bkaj,bka->bj", du, gu)
    ok = ~np.isnan(want).any(axis=1)
    err = float((np.abs(dx0[ok] - want[ok]).max(axis=1) / np.maximum(1.0, np.abs(want[ok]).max(axis=1))).max())
    print(f"identity with sens_x0: {ok.sum()} rows, worst relative {err:.2e}")
    assert ok.sum() >= 200 and err <= ID_TOL, err


def test_unit_loss(solved):
    s = solved
    gu = np.zeros((s.B, 1, 4))
    gu[np.arange(s.B), 0, np.arange(s.B) % 4] = 1.0
    s.eval_adjoint(None, gu)
    dx0 = s.adjoint()[0]
    du0, _ = s.sens_x0(0)
    want = du0[np.arange(s.B), np.arange(s.B) % 4]
    ok = ~np.isnan(want).any(axis=1)
    err = float((np.abs(dx0[ok] - want[ok]).max(axis=1) / np.maximum(1.0, np.abs(want[ok]).max(axis=1))).max())
    print(f"unit loss: worst relative {err:.2e}")
    assert ok.sum() >= 200 and err <= ID_TOL, err


def test_zero_gradient(solved):
    s = solved
    s.eval_adjoint(np.zeros((s.B, s.N + 1, 13)), np.zeros((s.B, s.N, 4)))
    ok = s.stats()[0] != 4
    for k, v in _outputs(s).items():
        assert np.all(v[ok] == 0.0), k


def test_free_and_active_entries(solved):
    s = solved
    gx, gu = _grads(s, 4)
    s.eval_adjoint(gx, gu)
    out = _outputs(s)
    act = s.sens_active()
    ok = s.stats()[0] != 4
    assert (act[ok] != 0).sum() >= 100
    assert np.all(out["dbox"][ok][act[ok] == 0] == 0.0)
    assert np.all(out["dr"][ok][act[ok] != 0] == 0.0)
    assert np.abs(out["dbox"][ok][act[ok] != 0]).min() > 0.0    # (a random loss moves every bound's multiplier)


# ---- 2. finite differences through the engine --------------------------------------------------------------------------------
FD_W, FD_Y, FD_X = 2, (1, 2), 8     # the perturbed entries: W[2] (z), yref[stage 1][2], x0[8] (vby)


def _fd_setup(oracle, B=64, N=20, h=1e-6, solve=True):
    """7 replicas per row in one solver with per-vehicle weight rows: the base and +-h on one weight, one yref entry, one x0
    entry, all from the same stored iterate -> (solver r, dict of the replicas' inputs x0, W, WN, yref, yref_e).  solve: one
    step and the sensitivities are evaluated; else the rows and the stored iterate are set and nothing has run"""
    s = _solver(B, N)
    x0 = _setup(oracle, s, 5, 2.0)
    s.solve(2)
    x_it, u_it = s.get_iterate()
    yr, ye = s.yref()
    W, WN = s.weights_batch()
    s.close()
    R = 7 * B
    r = _solver(R, N)
    rep = lambda a: np.repeat(a[:, None], 7, 1)
    X0, Wr, Yr = rep(x0), rep(W), rep(yr)
    for m, sgn in ((1, 1.0), (2, -1.0)):
        Wr[:, m, FD_W] += sgn * h
        Yr[:, 2 + m, FD_Y[0], FD_Y[1]] += sgn * h
        X0[:, 4 + m, FD_X] += sgn * h
    sh = lambda a: np.ascontiguousarray(a.reshape((R,) + a.shape[2:]))
    inp = dict(x0=sh(X0), W=sh(Wr), WN=sh(rep(WN)), yref=sh(Yr), yref_e=sh(rep(ye)))
    r.set_weights_batch(inp["W"], inp["WN"])
    r.set_yref(inp["yref"], inp["yref_e"])
    r.set_iterate(sh(rep(x_it)), sh(rep(u_it)))     # (restores the stored iterate in every replica)
    r.set_x0(inp["x0"])
    if solve:
        r.solve(1)
        r.eval_sens_x0()
    return r, inp


def _fd_compare(r, gx, gu, grads, h=1e-6):
    """-> rows kept per perturbation; asserts the central difference of l = sum gx . x + gu . u against grads [B][3]"""
    B = r.B // 7
    act = r.sens_active().reshape(B, 7, r.N, 4)
    xs, us = r.get_iterate()
    loss = ((xs * gx).sum(axis=(1, 2)) + (us * gu).sum(axis=(1, 2))).reshape(B, 7)
    kept = []
    for c in range(3):
        same = np.array([np.array_equal(act[i, 0], act[i, 1 + 2 * c]) and np.array_equal(act[i, 0], act[i, 2 + 2 * c]) for i in range(B)])
        fd = (loss[:, 1 + 2 * c] - loss[:, 2 + 2 * c]) / (2 * h)
        err = np.abs(fd - grads[:, c]) / np.maximum(1.0, np.abs(grads[:, c]))
        print(f"finite differences, {('W', 'yref', 'x0')[c]}: {same.sum()} of {B} rows kept, worst relative {err[same].max():.2e}")
        assert err[same].max() <= 1e-5, (c, err[same].max())
        kept.append(int(same.sum()))
    return kept


def test_finite_differences_through_engine(oracle):
    r, _inp = _fd_setup(oracle)
    B = r.B // 7
    rng = np.random.default_rng(6)
    gx = np.repeat(rng.normal(size=(B, r.N + 1, 13)), 7, 0)
    gu = np.repeat(rng.normal(size=(B, r.N, 4)), 7, 0)
    r.eval_adjoint(gx, gu)
    dx0 = r.adjoint()[0][::7]
    dW, _dWN, dyref, _ = r.adjoint_cost()
    grads = np.stack([dW[::7, FD_W], dyref[::7, FD_Y[0], FD_Y[1]], dx0[:, FD_X]], axis=1)
    kept = _fd_compare(r, gx, gu, grads)
    assert min(kept) >= 48, kept     # at least 48 of the 64 rows keep their active set under every +-h
    r.close()


# ---- 3. routes and data ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["weight_rows_scaled", "box_stages", "as_dense", "after_sqp"])
def test_routes(oracle, name):
    B, N = 256, 20
    s = _solver(B, N, **(dict(as_dense=1) if name == "as_dense" else {}))
    _setup(oracle, s, 77, 1.5 if name == "after_sqp" else 2.5)
    scales = (1.0, 1.0)
    if name == "weight_rows_scaled":
        rng = np.random.default_rng(8)
        W, WN = s.weights_batch()
        s.set_weights_batch(W * rng.uniform(0.5, 2.0, W.shape), WN * rng.uniform(0.5, 2.0, WN.shape))
        s.set_cost_scaling(DT, 1.0)
        scales = (DT, 1.0)
    elif name == "box_stages":
        s.set_box_stages(*_boxes(B, N, 3))
    status = None
    if name == "after_sqp":
        s.solve_sqp(max_iter=50)     # (full steps: every row's iterate is its last QP's solution, converged or not)
        status = s.sqp_stats()[0]
        assert (status == 0).sum() >= 8
    else:
        s.solve(1)
    s.eval_sens_x0()
    gx, gu = _grads(s, 9)
    s.eval_adjoint(gx, gu)
    # (cost scaling (dt, 1) puts the terminal weight 67 times above the stage weights: FP64 rounding of either side grows)
    n, _ = _check(s, _outputs(s), gx, gu, scales, status=status, ref_error=name == "weight_rows_scaled")
    assert n >= 200
    if name == "box_stages":
        act = s.sens_active()
        pin = _boxes(B, N, 3)[0][:, 0] == _boxes(B, N, 3)[1][:, 0]
        assert pin.any() and np.all(act[:, 0][pin] == -1)
    s.close()


# ---- 4. shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["partial_wavefront", "first_stage_only", "gx_none", "gu_none"])
def test_shapes(oracle, case):
    B = 6 if case == "partial_wavefront" else 64
    s = _solver(B, 20)
    _setup(oracle, s, 12, 3.0)
    s.solve(2)
    s.eval_sens_x0()
    gx, gu = _grads(s, 13, *((1, 1) if case == "first_stage_only" else (None, None)))
    gx = None if case == "gx_none" else gx
    gu = None if case == "gu_none" else gu
    s.eval_adjoint(gx, gu)
    n, _ = _check(s, _outputs(s), gx, gu)
    assert n >= B - 2
    s.close()


# ---- 5. side effects ---------------------------------------------------------------------------------------------------------
def _loop(oracle, with_adj, B=512, N=20, steps=20):
    from crazyflie_nmpc_amd import sim
    s = _solver(B, N)
    x = _setup(oracle, s, 21, 2.0)
    kicks = oracle.sample_hover_x0(np.random.default_rng(22), B, scale=2.0)
    gu = np.ones((B, 1, 4))
    cmds = []
    for t in range(steps):
        if t % 5 == 0:
            x[t % B::7] = kicks[t % B::7]
        s.set_x0(x)
        s.solve(1)
        if with_adj:
            s.eval_sens_x0()
            s.eval_adjoint(None, gu)
        u0 = s.get_u(0)
        cmds.append(u0.copy())
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


def test_repeated_eval_is_bitwise_equal(solved):
    s = solved
    gx, gu = _grads(s, 14)
    s.eval_adjoint(gx, gu)
    a = _outputs(s)
    s.eval_adjoint(np.zeros_like(gx), None)   # (something else in between)
    s.eval_adjoint(gx, gu)
    b = _outputs(s)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_workspace_bytes_count_the_buffers(oracle):
    s = _solver(64, 20)
    _setup(oracle, s, 1, 1.0)
    s.solve(1)
    s.eval_sens_x0()
    before = s._L.cfnmpc_workspace_bytes(s._h)
    s.eval_adjoint(None, np.ones((64, 1, 4)))
    after = s._L.cfnmpc_workspace_bytes(s._h)
    assert after - before >= 8 * 64 * (21 * 13 + 20 * (4 + 13 + 4 + 17))
    s.eval_adjoint(None, np.ones((64, 1, 4)))
    assert s._L.cfnmpc_workspace_bytes(s._h) == after
    s.close()


# ---- 6. validation -----------------------------------------------------------------------------------------------------------
def test_refusals(oracle):
    from crazyflie_nmpc_amd.solver import CfnmpcError
    B, N = 8, 20
    s = _solver(B, N)
    _setup(oracle, s, 1, 1.0)
    gu = np.ones((B, 1, 4))
    with pytest.raises(CfnmpcError):
        s.eval_adjoint(None, gu)               # before any solve
    s.solve(1)
    with pytest.raises(CfnmpcError):
        s.eval_adjoint(None, gu)               # no eval_sens_x0
    s.eval_sens_x0()
    with pytest.raises(CfnmpcError):
        s.adjoint()                            # no evaluation yet
    with pytest.raises(CfnmpcError):
        s.adjoint_cost()
    with pytest.raises(CfnmpcError):
        s.eval_adjoint(np.ones((B, N + 2, 13)), None)     # n_gx > N + 1
    with pytest.raises(CfnmpcError):
        s.eval_adjoint(None, np.ones((B, N + 1, 4)))      # n_gu > N
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert s._L.cfnmpc_eval_adjoint(s._h, p(gu), 0, None, 0, 0, None) != 0   # n_gx = 0 with an array
    s.eval_adjoint(None, gu)                   # the refused calls left the solver usable
    ref = s.adjoint()[0]
    W, WN = np.array(s.opts.W), np.array(s.opts.WN)
    s.set_weights(W, WN)                       # data changed since the solve
    with pytest.raises(CfnmpcError):
        s.eval_adjoint(None, gu)
    with pytest.raises(CfnmpcError):
        s.adjoint()
    s.solve(1)
    s.eval_sens_x0()
    s.eval_adjoint(None, gu)
    assert np.isfinite(ref).all() and np.isfinite(s.adjoint()[0]).all()
    s.eval_sens_x0()                           # a new sensitivity evaluation: the adjoint belongs to the old one
    with pytest.raises(CfnmpcError):
        s.adjoint()
    s.eval_adjoint(None, gu)
    s.solve(1)                                 # a later solve invalidates the evaluation
    with pytest.raises(CfnmpcError):
        s.adjoint_cost()
    # a globalised SQP solve: the iterate is not the last QP's solution
    s.set_sqp_globalization("merit_backtracking")
    s.solve_sqp(max_iter=5)
    with pytest.raises(CfnmpcError):
        s.eval_sens_x0()
    with pytest.raises(CfnmpcError):
        s.eval_adjoint(None, gu)
    s.set_sqp_globalization("full_step")
    s.solve_sqp(max_iter=5)
    s.eval_sens_x0()
    s.eval_adjoint(None, gu)
    s.close()
    for kw in (dict(cond_N2=5), dict(start_solve=2)):
        t = _solver(B, N, **kw)
        _setup(oracle, t, 1, 1.0)
        t.solve(1)
        with pytest.raises(CfnmpcError):
            t.eval_adjoint(None, gu)
        t.solve(1)                             # ... and solves on
        assert (t.stats()[0] != 4).all()
        t.close()


def test_nan_row(oracle):
    outs = []
    gx, gu = None, None
    for bad in (False, True):
        s = _solver(64, 20)
        x0 = _setup(oracle, s, 41, 2.0)
        s.solve(1)
        if bad:
            x0[5] = np.nan
        s.set_x0(x0)
        s.solve(1)
        s.eval_sens_x0()
        if gx is None:
            gx, gu = _grads(s, 15)
        s.eval_adjoint(gx, gu)
        outs.append((_outputs(s), s.stats()[0]))
        s.close()
    (o0, _st0), (o1, st1) = outs
    assert st1[5] == 4
    keep = np.arange(64) != 5
    for k in o0:
        assert np.isnan(o1[k][5]).all(), k
        assert np.array_equal(o0[k][keep], o1[k][keep]), k


# ---- 7. fleet and multi ------------------------------------------------------------------------------------------------------
def _bucket_rows(L, sv, n, N):
    d0, dW, dWN = np.empty((n, 13)), np.empty((n, 17)), np.empty((n, 13))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.cfnmpc_get_adjoint(sv, p(d0), None, None, None, None, 0, None) == 0
    assert L.cfnmpc_get_adjoint_cost(sv, p(dW), p(dWN), None, None, 0, None) == 0
    return d0, dW, dWN


def test_fleet_equals_buckets(oracle):
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    hz = np.random.default_rng(3).choice([8, 17, 33], 96).astype(np.int32)
    B, Nm = len(hz), 33
    x0, yr, ye = _fleet_inputs(oracle, B, Nm, 4)
    f = MixedHorizonFleet(hz)
    f.set_x0(x0); f.set_yref(yr, ye); f.init_iterate(INIT_HOVER)
    f.solve(2)
    f.eval_sens_x0()
    rng = np.random.default_rng(5)
    n_g = f.Nmin
    gx, gu = rng.normal(size=(B, n_g, 13)), rng.normal(size=(B, n_g, 4))
    f.eval_adjoint(gx, gu)
    d0, dW, dWN = f.adjoint()
    assert np.isfinite(d0).mean() > 0.9 and np.abs(d0[np.isfinite(d0)]).max() > 0.0
    L = f._L
    for b, (N, idx) in enumerate(f.buckets()):
        sv = C.c_void_p()
        assert L.cfnmpc_fleet_bucket(f._h, b, None, None, C.byref(sv), None) == 0
        for a, want in zip(_bucket_rows(L, sv, len(idx), N), (d0, dW, dWN)):
            assert np.array_equal(a, want[idx], equal_nan=True), N
    # device tensors take the other path of the fleet's row movers
    import torch
    f.eval_adjoint(torch.from_numpy(gx).cuda(), torch.from_numpy(gu).cuda())
    torch.cuda.synchronize()
    for a, want in zip(f.adjoint(), (d0, dW, dWN)):
        assert np.array_equal(a, want, equal_nan=True)
    with pytest.raises(Exception):
        f.eval_adjoint(np.zeros((B, n_g + 1, 13)), None)   # beyond the shortest horizon
    f.close()


def test_multi_two_shards(oracle):
    from crazyflie_nmpc_amd import default_opts
    from crazyflie_nmpc_amd.parallel import MultiGpuFleet
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B, N = 128, 20
    x0, yr, ye = _fleet_inputs(oracle, B, N, 5)
    m = MultiGpuFleet(B, [0, 0], opts=default_opts(N=N))
    m.set_x0(x0); m.set_yref(yr, ye); m.init_iterate(INIT_HOVER)
    m.solve(2); m.sync()
    m.eval_sens_x0()
    rng = np.random.default_rng(6)
    gx, gu = rng.normal(size=(B, N, 13)), rng.normal(size=(B, N, 4))
    m.eval_adjoint(gx, gu)
    d0, dW, dWN = m.adjoint()
    assert np.abs(d0[np.isfinite(d0)]).max() > 0.0
    L = m._L
    for i in range(L.cfnmpc_multi_num_shards(m._h)):
        sv, lo, hi = C.c_void_p(), C.c_int(), C.c_int()
        assert L.cfnmpc_multi_shard(m._h, i, C.byref(sv), C.byref(lo), C.byref(hi), None, None) == 0
        for a, want in zip(_bucket_rows(L, sv, hi.value - lo.value, N), (d0, dW, dWN)):
            assert np.array_equal(a, want[lo.value:hi.value], equal_nan=True), i
    m.close()


# ---- 8. autograd -------------------------------------------------------------------------------------------------------------
def test_autograd_rti_step(oracle):
    import torch
    from crazyflie_nmpc_amd.diff import rti_step
    r, inp = _fd_setup(oracle, solve=False)
    B, N, R = r.B // 7, r.N, r.B
    dev = torch.device("cuda")
    # the replicas' own inputs as leaves: rti_step runs the step from the stored iterate
    leaves = [torch.tensor(inp[k], dtype=torch.float64, device=dev, requires_grad=True) for k in ("x0", "W", "WN", "yref", "yref_e")]
    x, u = rti_step(r, *leaves)
    assert tuple(x.shape) == (R, N + 1, 13) and tuple(u.shape) == (R, N, 4)
    wgt = torch.tensor(np.repeat(np.random.default_rng(7).normal(size=(B, 4)), 7, 0), dtype=torch.float64, device=dev)
    loss = (u[:, 0] * wgt).sum()
    loss.backward()
    torch.cuda.synchronize()
    # the gradients are those of the getters for the same loss
    # (autograd hands backward() the gradient of the whole u: the same array here, so that both sweeps start at the same stage)
    gu = np.zeros((R, N, 4)); gu[:, 0] = wgt.cpu().numpy()
    r.eval_adjoint(None, gu)
    dx0 = r.adjoint()[0]
    dW, dWN, dyref, dyref_e = r.adjoint_cost()
    for leaf, want in zip(leaves, (dx0, dW, dWN, dyref, dyref_e)):
        assert np.array_equal(leaf.grad.cpu().numpy(), want, equal_nan=True)
    # ... and one weight component agrees with the finite difference of the loss over the replicas
    gxz, guf = np.zeros((R, N + 1, 13)), gu
    grads = np.stack([dW[::7, FD_W], dyref[::7, FD_Y[0], FD_Y[1]], dx0[::7, FD_X]], axis=1)
    kept = _fd_compare(r, gxz, guf, grads)
    assert min(kept) >= 48, kept
    # backward() belongs to the solver's last rti_step
    x2, u2 = rti_step(r, *leaves)
    x3, u3 = rti_step(r, *leaves)
    with pytest.raises(RuntimeError):
        u2.sum().backward()
    r.close()
