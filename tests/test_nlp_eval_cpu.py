"""CPU checks of the NLP evaluation (include/cfnmpc.h: cfnmpc_eval_nlp): the numpy reference the GPU
tests compare against (nlp_ref) is refereed by finite differences of the single-shooting objective and by the same recursion
in extended precision, its kernel is in the built code within its resource ceiling, and the new entry points are declared,
exported and bound.  No GPU needed."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_model_params_cpu import NOMINAL, consts, random_params
from test_model_params_cpu import f as f_par
from test_model_params_cpu import rk4_sens as rk4_sens_par

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, i32 = ctypes.c_void_p, ctypes.c_int
SIGS = {
    "cfnmpc_eval_nlp": "intcfnmpc_eval_nlp(cfnmpc_solver*s,intkeep_multipliers,void*stream);",
    "cfnmpc_get_nlp_stats": "intcfnmpc_get_nlp_stats(cfnmpc_solver*s,double*cost,double*res,inton_device,void*stream);",
    "cfnmpc_get_nlp_multipliers": "intcfnmpc_get_nlp_multipliers(cfnmpc_solver*s,double*pi,double*gu,inton_device,void*stream);",
    "cfnmpc_fleet_eval_nlp": "intcfnmpc_fleet_eval_nlp(cfnmpc_fleet*f,void*stream);",
    "cfnmpc_fleet_get_nlp_stats": "intcfnmpc_fleet_get_nlp_stats(cfnmpc_fleet*f,double*cost,double*res,inton_device,void*stream);",
    "cfnmpc_multi_eval_nlp": "intcfnmpc_multi_eval_nlp(cfnmpc_multi*m);",
    "cfnmpc_multi_get_nlp_stats": "intcfnmpc_multi_get_nlp_stats(cfnmpc_multi*m,double*cost,double*res);",
}
ARGTYPES = {
    "cfnmpc_eval_nlp": [vp, i32, vp],
    "cfnmpc_get_nlp_stats": [vp, vp, vp, i32, vp],
    "cfnmpc_get_nlp_multipliers": [vp, vp, vp, i32, vp],
    "cfnmpc_fleet_eval_nlp": [vp, vp],
    "cfnmpc_fleet_get_nlp_stats": [vp, vp, vp, i32, vp],
    "cfnmpc_multi_eval_nlp": [vp],
    "cfnmpc_multi_get_nlp_stats": [vp, vp, vp],
}
SHIM = ("ocp_nlp_eval_cost", "ocp_nlp_eval_residuals", "ocp_nlp_get")


# ---- numpy reference, batched over the rows (external state order) ----------------------------------------------------------
def _f(x, u, c):
    """the model of test_model_params_cpu.f for rows at once: x [13, ...], u [4, ...], c = the eight derived constants, each a
    scalar or an array over the rows (x, u may be complex: complex-step Jacobians)"""
    g0, kt, ka, kb, kc, kwx, kwy, kwz = c
    q1, q2, q3, q4 = x[3], x[4], x[5], x[6]
    vx, vy, vz = x[7], x[8], x[9]
    wx, wy, wz = x[10], x[11], x[12]
    s1, s2, s3, s4 = u[0] * u[0], u[1] * u[1], u[2] * u[2], u[3] * u[3]
    return np.stack([
        vx * (2 * q1 * q1 + 2 * q2 * q2 - 1) - vy * (2 * q1 * q4 - 2 * q2 * q3) + vz * (2 * q1 * q3 + 2 * q2 * q4),
        vy * (2 * q1 * q1 + 2 * q3 * q3 - 1) + vx * (2 * q1 * q4 + 2 * q2 * q3) - vz * (2 * q1 * q2 - 2 * q3 * q4),
        vz * (2 * q1 * q1 + 2 * q4 * q4 - 1) - vx * (2 * q1 * q3 - 2 * q2 * q4) + vy * (2 * q1 * q2 + 2 * q3 * q4),
        -(q2 * wx) / 2 - (q3 * wy) / 2 - (q4 * wz) / 2,
        (q1 * wx) / 2 - (q4 * wy) / 2 + (q3 * wz) / 2,
        (q4 * wx) / 2 + (q1 * wy) / 2 - (q2 * wz) / 2,
        (q2 * wy) / 2 - (q3 * wx) / 2 + (q1 * wz) / 2,
        vy * wz - vz * wy + g0 * (2 * q1 * q3 - 2 * q2 * q4),
        vz * wx - vx * wz - g0 * (2 * q1 * q2 + 2 * q3 * q4),
        vx * wy - vy * wx - g0 * (2 * q1 * q1 + 2 * q4 * q4 - 1) + kt * (s1 + s2 + s3 + s4),
        ka * (s1 + s2 - s3 - s4) + kwx * (wy * wz),
        kb * (s1 - s2 - s3 + s4) + kwy * (wx * wz),
        kc * (s1 - s2 + s3 - s4) + kwz * (wx * wy),
    ])


def _consts(params, B, T):
    """derived constants per row ([8] arrays of B, dtype T) from parameter rows [B][8] (None: nominal), by consts() in FP64"""
    rows = np.tile(NOMINAL, (B, 1)) if params is None else np.asarray(params, dtype=np.float64).reshape(B, 8)
    c = np.array([consts(r) for r in rows])
    return [c[:, j].astype(T) for j in range(8)]


def _jac(x, u, c, T):
    """(df/dx [13, 13, B], df/du [13, 4, B]) by complex steps (f is a polynomial: exact to rounding), in the precision of T"""
    CT = np.complex128 if T is np.float64 else np.clongdouble
    hc = T(1e-40)
    xc, uc = x.astype(CT), u.astype(CT)
    A = np.empty((13, 13) + x.shape[1:], dtype=T); Bm = np.empty((13, 4) + x.shape[1:], dtype=T)
    for j in range(13):
        e = xc.copy(); e[j] += 1j * hc
        A[:, j] = _f(e, uc, c).imag / hc
    for j in range(4):
        e = uc.copy(); e[j] += 1j * hc
        Bm[:, j] = _f(xc, e, c).imag / hc
    return A, Bm


def _mm(a, b):
    return np.einsum("ij...,jk...->ik...", a, b)


def rk4_sens_rows(x, u, c, dt, M=1, T=np.float64):
    """M classic RK4 steps of dt / M with sensitivities for rows at once (the chaining of test_erk_cpu / rk4_sens of
    test_model_params_cpu): x [13, B], u [4, B] -> Phi [13, B], A [13, 13, B], B [13, 4, B]"""
    h = T(dt) / T(M)
    nb = x.shape[1]
    eye = np.repeat(np.eye(13, dtype=T)[:, :, None], nb, 2)
    xs, A, Bm = x.astype(T), eye.copy(), np.zeros((13, 4, nb), dtype=T)
    for _ in range(M):
        ks, kx, ku = [], [], []
        xt, Tx, Tu = xs, eye, np.zeros((13, 4, nb), dtype=T)
        for cc in (T(0.5), T(0.5), T(1.0), None):
            k = _f(xt, u, c)
            fx, fu = _jac(xt, u, c, T)
            dkx, dku = _mm(fx, Tx), _mm(fx, Tu) + fu
            ks.append(k); kx.append(dkx); ku.append(dku)
            if cc is not None:
                xt, Tx, Tu = xs + cc * h * k, eye + cc * h * dkx, cc * h * dku
        xn = xs + (h / 6) * (ks[0] + 2 * ks[1] + 2 * ks[2] + ks[3])
        Aj = eye + (h / 6) * (kx[0] + 2 * kx[1] + 2 * kx[2] + kx[3])
        Bj = (h / 6) * (ku[0] + 2 * ku[1] + 2 * ku[2] + ku[3])
        xs, A, Bm = xn, _mm(Aj, A), _mm(Aj, Bm) + Bj
    return xs, A, Bm


def nlp_ref_rows(x, u, x0, yref, yref_e, Qd, Rd, QNd, lb, ub, dt, erk_steps=1, params=None, T=np.float64):
    """nlp_ref for B rows at once: x [B, N + 1, 13], u [B, N, 4], x0 [B, 13], yref [B, N, 17], yref_e [B, 13]; Qd [13] or
    [B, 13], Rd [4] or [B, 4], QNd [13] or [B, 13] (the weights in force TIMES the cost scaling); lb, ub scalars or anything that
    broadcasts to [B, N, 4]; params [B, 8] or None -> cost [B], res [B, 3] (stat, eq, ineq), pi [B, N + 1, 13], gu [B, N, 4]"""
    x = np.asarray(x, dtype=T); u = np.asarray(u, dtype=T)
    B, N = u.shape[0], u.shape[1]
    x0 = np.asarray(x0, dtype=T); yref = np.asarray(yref, dtype=T); yref_e = np.asarray(yref_e, dtype=T)
    Qd = np.broadcast_to(np.asarray(Qd, dtype=T), (B, 13)); Rd = np.broadcast_to(np.asarray(Rd, dtype=T), (B, 4))
    QNd = np.broadcast_to(np.asarray(QNd, dtype=T), (B, 13))
    lb = np.broadcast_to(np.asarray(lb, dtype=T), (B, N, 4)); ub = np.broadcast_to(np.asarray(ub, dtype=T), (B, N, 4))
    c = _consts(params, B, T)
    pi = np.empty((B, N + 1, 13), dtype=T); gu = np.empty((B, N, 4), dtype=T)
    dN = x[:, N] - yref_e
    pi[:, N] = QNd * dN
    cost = 0.5 * (QNd * dN * dN).sum(1)
    r_eq = np.abs(x[:, 0] - x0).max(1)
    for k in range(N - 1, -1, -1):
        phi, A, Bm = rk4_sens_rows(x[:, k].T, u[:, k].T, c, dt, erk_steps, T)
        r_eq = np.maximum(r_eq, np.abs(x[:, k + 1] - phi.T).max(1))
        dx, du = x[:, k] - yref[:, k, :13], u[:, k] - yref[:, k, 13:]
        pi[:, k] = Qd * dx + np.einsum("ijb,bi->bj", A, pi[:, k + 1])
        gu[:, k] = Rd * du + np.einsum("ijb,bi->bj", Bm, pi[:, k + 1])
        cost = cost + 0.5 * (Qd * dx * dx).sum(1) + 0.5 * (Rd * du * du).sum(1)
    r_stat = np.abs(u - np.clip(u - gu, lb, ub)).reshape(B, -1).max(1)
    r_ineq = np.maximum(0.0, np.maximum(lb - u, u - ub).reshape(B, -1).max(1))
    return cost, np.stack([r_stat, r_eq, r_ineq], 1), pi, gu


def nlp_ref(x, u, x0, yref, yref_e, Qd, Rd, QNd, lb, ub, dt, erk_steps=1, params=None):
    """One instance: x [N + 1, 13], u [N, 4], x0 [13], yref [N, 17], yref_e [13], the effective weight diagonals, the box (scalars
    or [N, 4]), params [8] or None -> cost, res [3] = (res_stat, res_eq, res_ineq), pi [N + 1, 13], gu [N, 4] by the definitions
    of include/cfnmpc.h (cfnmpc_eval_nlp), with explicit A_k = dPhi/dx and B_k = dPhi/du (complex-step Jacobians through the
    RK4 stages)."""
    cost, res, pi, gu = nlp_ref_rows(np.asarray(x)[None], np.asarray(u)[None], np.asarray(x0)[None], np.asarray(yref)[None],
                                     np.asarray(yref_e)[None], Qd, Rd, QNd, lb, ub, dt, erk_steps,
                                     None if params is None else np.asarray(params)[None])
    return cost[0], res[0], pi[0], gu[0]


# ---- the reference's own checks -----------------------------------------------------------------------------------------------
def _iterates(oracle, B, N, seed, spread=1.0):
    """rough iterates around hover: not feasible, inputs partly on the box"""
    rng = np.random.default_rng(seed)
    x0 = oracle.sample_hover_x0(rng, B, scale=1.0)
    x = np.repeat(x0[:, None, :], N + 1, 1) + 0.05 * spread * rng.standard_normal((B, N + 1, 13))
    u = np.clip(oracle.HOV_W + 4.0 * spread * rng.standard_normal((B, N, 4)), 0.0, 22.0)
    yr, ye = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    return x, u, x0, np.repeat(yr[None], B, 0).copy(), np.repeat(ye[None], B, 0).copy()


def test_batched_model_is_the_parametrised_model_and_the_oracle(oracle):
    rng = np.random.default_rng(3)
    B = 6
    p = random_params(rng, B)
    x = rng.standard_normal((B, 13)); u = 10 + 5 * rng.random((B, 4))
    c = _consts(p, B, np.float64)
    fr = _f(x.T, u.T, c).T
    for i in range(B):
        assert np.array_equal(fr[i], f_par(x[i], u[i], p[i]))
    for M in (1, 3):
        phi, A, Bm = rk4_sens_rows(x.T, u.T, c, 0.015, M)
        for i in range(B):
            pr, Ar, Br = rk4_sens_par(x[i], u[i], p[i], 0.015, M)
            assert np.abs(phi[:, i] - pr).max() < 1e-14 and np.abs(A[:, :, i] - Ar).max() < 1e-13 and np.abs(Bm[:, :, i] - Br).max() < 1e-13
    # nominal row: the oracle's model, RK4 and (sympy) Jacobians
    cn = _consts(None, B, np.float64)
    phi, A, Bm = rk4_sens_rows(x.T, u.T, cn, oracle.DT, 1)
    fn = _f(x.T, u.T, cn)
    for i in range(B):
        assert np.abs(fn[:, i] - oracle.f_expl(x[i], u[i])).max() < 1e-12
        po, Ao, Bo = oracle.rk4_sens(x[i], u[i], oracle.DT)
        assert np.abs(phi[:, i] - po).max() < 1e-13 and np.abs(A[:, :, i] - Ao).max() < 1e-12 and np.abs(Bm[:, :, i] - Bo).max() < 1e-12


def _objective(oracle, u, x0, yref, yref_e, Qd, Rd, QNd, dt, M, c):
    """single-shooting objective J(u; x0): roll out with the sub-stepped RK4, sum the stage costs"""
    N = u.shape[0]
    h = dt / M
    x = x0.copy()
    J = 0.0
    for k in range(N):
        dx, du = x - yref[k, :13], u[k] - yref[k, 13:]
        J += 0.5 * (Qd * dx * dx).sum() + 0.5 * (Rd * du * du).sum()
        for _ in range(M):
            k1 = _f(x, u[k], c); k2 = _f(x + 0.5 * h * k1, u[k], c); k3 = _f(x + 0.5 * h * k2, u[k], c); k4 = _f(x + h * k3, u[k], c)
            x = x + (h / 6) * (k1 + 2 * k2 + 2 * k3 + k4)
    dN = x - yref_e
    return J + 0.5 * (QNd * dN * dN).sum()


@pytest.mark.parametrize("M", [1, 2])
def test_reference_against_finite_differences_of_the_single_shooting_objective(oracle, M):
    """Independent of any adjoint: on a dynamically feasible rollout gu is dJ/du and pi[0] is dJ/dx0 of J(u; x0).
    Central differences with step h = 1e-5 (inputs are O(16), states O(1)).  Error of the quotient: rounding eps |J| / h =
    2.2e-16 * |J| / 1e-5 = 2.2e-11 |J|, at most 7e-7 for |J| <= 3e4 (asserted below), and truncation h^2 |J'''| / 6 =
    1.7e-11 |J'''|, where each further derivative of the polynomial dynamics brings a factor O(10) at states of O(1):
    |J'''| ~ 1e2 |g|, i.e. 2e-9 |g|.  Tolerance 1e-6 * max(1, |g|_inf) covers the sum with |g| >= 1e2 and is still six orders
    below the gradients; the errors seen are printed."""
    N, dt, h = 12, oracle.DT, 1e-5
    rng = np.random.default_rng(11 + M)
    p = random_params(rng, 1)[0] if M == 2 else None
    c = [v[0] for v in _consts(None if p is None else p[None], 1, np.float64)]
    x0 = oracle.sample_hover_x0(rng, 1, scale=1.0)[0]
    u = np.clip(oracle.HOV_W + 3.0 * rng.standard_normal((N, 4)), 0.5, 21.5)
    yr, ye = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    Qd, Rd, QNd = 0.7 * oracle.Q_DIAG, 0.7 * oracle.R_DIAG, 1.3 * oracle.QN_DIAG
    x = np.empty((N + 1, 13)); x[0] = x0
    hs = dt / M
    for k in range(N):
        xs = x[k]
        for _ in range(M):
            k1 = _f(xs, u[k], c); k2 = _f(xs + 0.5 * hs * k1, u[k], c); k3 = _f(xs + 0.5 * hs * k2, u[k], c); k4 = _f(xs + hs * k3, u[k], c)
            xs = xs + (hs / 6) * (k1 + 2 * k2 + 2 * k3 + k4)
        x[k + 1] = xs
    cost, res, pi, gu = nlp_ref(x, u, x0, yr, ye, Qd, Rd, QNd, 0.0, 22.0, dt, M, p)
    J = lambda uu, xx: _objective(oracle, uu, xx, yr, ye, Qd, Rd, QNd, dt, M, c)
    assert res[1] < 1e-13 and res[2] == 0.0           # feasible rollout inside the box
    assert abs(cost - J(u, x0)) <= 1e-12 * abs(cost) and abs(cost) <= 3e4
    g_fd = np.empty((N, 4))
    for k in range(N):
        for a in range(4):
            up, um = u.copy(), u.copy()
            up[k, a] += h; um[k, a] -= h
            g_fd[k, a] = (J(up, x0) - J(um, x0)) / (2 * h)
    p_fd = np.empty(13)
    for j in range(13):
        xp, xm = x0.copy(), x0.copy()
        xp[j] += h; xm[j] -= h
        p_fd[j] = (J(u, xp) - J(u, xm)) / (2 * h)
    eg, ep = np.abs(gu - g_fd).max(), np.abs(pi[0] - p_fd).max()
    print(f"M={M}: |J| {abs(cost):.3e}  |gu| {np.abs(gu).max():.3e} err {eg:.2e}  |pi0| {np.abs(pi[0]).max():.3e} err {ep:.2e}")
    assert eg <= 1e-6 * max(1.0, np.abs(gu).max()), eg
    assert ep <= 1e-6 * max(1.0, np.abs(pi[0]).max()), ep


def test_natural_residual_cases():
    """|g| inside the box, zero on a bound with the gradient pointing outward, a pinned input counts as on a bound"""
    N = 2
    x = np.zeros((N + 1, 13)); x[:, 3] = 1.0
    yr = np.zeros((N, 17)); yr[:, 3] = 1.0
    ye = x[N].copy()
    Qd, QNd = np.zeros(13), np.zeros(13)
    Rd = np.ones(4)
    # cost is 1/2 |u - yref_u|^2 alone (pi = 0): g = u - yref_u
    u = np.array([[5.0, 0.0, 22.0, 7.0], [5.0, 0.0, 22.0, 7.0]])
    yr[:, 13:] = np.array([4.0, 3.0, 30.0, 7.5])      # g = u - yref_u = (1, -3, -8, -0.5)
    lb = np.zeros((N, 4)); ub = np.full((N, 4), 22.0)
    lb[:, 3] = ub[:, 3] = 7.0                          # pinned
    # x is a fixed point of nothing in particular: only res_stat is looked at
    cost, res, pi, gu = nlp_ref(x, u, x[0], yr, ye, Qd, Rd, QNd, lb, ub, 0.015)
    assert np.allclose(gu, u - yr[:, 13:]) and np.abs(pi).max() == 0.0
    # input 0 inside: |g| = 1; input 1 on the lower bound with g = -3 (wants up, inward): min(|g|, room) = 3; input 2 on the
    # upper bound with g = -8 (wants up, outward): 0; input 3 pinned: 0
    assert res[0] == 3.0
    u2 = u.copy(); u2[:, 1] = 10.0                     # now inside with g = 7, room to the lower bound 10: full gradient
    assert nlp_ref(x, u2, x[0], yr, ye, Qd, Rd, QNd, lb, ub, 0.015)[1][0] == 7.0
    assert cost == pytest.approx(0.5 * 2 * (1 + 9 + 64 + 0.25))


def test_fp64_recursion_against_extended_precision(oracle):
    """the FP64 recursion against the same recursion in np.longdouble on 12 rows: relative to the array's largest entry"""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("no extended precision on this platform")
    B, N = 12, 50
    x, u, x0, yref, yref_e = _iterates(oracle, B, N, seed=5)
    rng = np.random.default_rng(6)
    p = random_params(rng, B)
    args = (x, u, x0, yref, yref_e, oracle.Q_DIAG, oracle.R_DIAG, oracle.QN_DIAG, 0.0, 22.0, oracle.DT, 2, p)
    c64, r64, p64, g64 = nlp_ref_rows(*args)
    cld, rld, pld, gld = nlp_ref_rows(*args, T=np.longdouble)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    print(f"pi {rel(p64, pld):.2e}  gu {rel(g64, gld):.2e}  cost {rel(c64, cld):.2e}  res {rel(r64, rld):.2e}")
    assert rel(p64, pld) <= 1e-13 and rel(g64, gld) <= 1e-13
    assert rel(c64, cld) <= 1e-13 and rel(r64, rld) <= 1e-13


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


@pytest.mark.parametrize("name", ["k_nlp_eval", "k_nlp_eval_par"])
def test_nlp_kernels_within_resources(table, name):
    assert name in table, sorted(table)
    r = table[name]
    assert r["unit"] == "cfnmpc_kernels"          # (the set of device units stays at four)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["vgpr"] <= 256 and r["occupancy"] >= 1, r
    assert r["lds"] <= 40960, r                   # four wavefronts per compute unit (160 KB): one per SIMD at 65 536 instances


def _header(path=("include", "cfnmpc.h")):
    src = open(os.path.join(ROOT, *path)).read()
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
    assert L.cfnmpc_abi_version() == 9            # new entry points only: cfnmpc_opts and old signatures unchanged
    assert L.cfnmpc_opts_size() == ctypes.sizeof(_lib.Opts)
    assert "#defineCFNMPC_ABI_VERSION9" in src


def test_shim_entry_points_declared_and_exported():
    src = _header(("include", "acados_solver_crazyflie.h"))
    assert "voidocp_nlp_eval_cost(ocp_nlp_solver*solver,ocp_nlp_in*in,ocp_nlp_out*out);" in src
    assert "voidocp_nlp_eval_residuals(ocp_nlp_solver*solver,ocp_nlp_in*in,ocp_nlp_out*out);" in src
    assert "voidocp_nlp_get(ocp_nlp_config*config,ocp_nlp_solver*solver,constchar*field,void*value);" in src
    from crazyflie_nmpc_amd import _lib
    _lib.lib()                                     # (the shim links against the engine: load it first)
    shim = ctypes.CDLL(os.path.join(ROOT, "crazyflie_nmpc_amd", "libacados_solver_crazyflie.so"))
    for name in SHIM:
        assert hasattr(shim, name), name


def test_python_wrappers_exist():
    from crazyflie_nmpc_amd import BatchSolver
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.parallel import MultiGpuFleet
    sig = inspect.signature(BatchSolver.eval_nlp)
    assert sig.parameters["keep_multipliers"].default is False and sig.parameters["stream"].default is None
    assert callable(BatchSolver.nlp_stats) and callable(BatchSolver.nlp_multipliers)
    for cls in (MixedHorizonFleet, MultiGpuFleet):
        assert callable(getattr(cls, "eval_nlp")) and callable(getattr(cls, "nlp_stats"))
