"""CPU checks of the adjoint solution sensitivities (include/cfnmpc.h: cfnmpc_eval_adjoint, cfnmpc_get_adjoint,
cfnmpc_get_adjoint_cost): the numpy reference of the three sweeps the GPU tests compare against equals
a dense KKT solve with the active set fixed, central differences of the extended-precision QP solution and the forward
sensitivities of tests/test_sens_cpu.py; the new entry points are declared, exported and bound; the new kernels are in the built
code within their budgets while the default-path kernels keep the parent's figures.  No GPU needed.

Sign convention (csrc/cfnmpc_adj.hpp): with a the minimiser of the QP whose linear term is the loss gradient and whose
constraints are homogeneous, and (lam, mu) the multipliers of the recursion below,
    dl/dq_k = a^x_k, dl/dr_k = a^u_k, dl/dx0 = lam_0, dl/db_k = lam_{k+1}, dl/dbound_{k,a} = mu_{k,a} on active inputs,
    dl/dyref = -W a, dl/dW_j = sum_k a_{k,j} (z_{k,j} - yref_{k,j})."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from test_sens_cpu import hover_qps, sens_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGS = {
    "cfnmpc_eval_adjoint": "intcfnmpc_eval_adjoint(cfnmpc_solver*s,constdouble*gx,intn_gx,constdouble*gu,intn_gu,inton_device,"
                           "void*stream);",
    "cfnmpc_get_adjoint": "intcfnmpc_get_adjoint(cfnmpc_solver*s,double*dl_dx0,double*dl_dq,double*dl_dr,double*dl_db,"
                          "double*dl_dbox,inton_device,void*stream);",
    "cfnmpc_get_adjoint_cost": "intcfnmpc_get_adjoint_cost(cfnmpc_solver*s,double*dl_dW,double*dl_dWN,double*dl_dyref,"
                               "double*dl_dyref_e,inton_device,void*stream);",
    "cfnmpc_fleet_eval_adjoint": "intcfnmpc_fleet_eval_adjoint(cfnmpc_fleet*f,constdouble*gx,constdouble*gu,intn_g,inton_device,"
                                 "void*stream);",
    "cfnmpc_fleet_get_adjoint": "intcfnmpc_fleet_get_adjoint(cfnmpc_fleet*f,double*dl_dx0,double*dl_dW,double*dl_dWN,"
                                "inton_device,void*stream);",
    "cfnmpc_multi_eval_adjoint": "intcfnmpc_multi_eval_adjoint(cfnmpc_multi*m,constdouble*gx,constdouble*gu,intn_g);",
    "cfnmpc_multi_get_adjoint": "intcfnmpc_multi_get_adjoint(cfnmpc_multi*m,double*dl_dx0,double*dl_dW,double*dl_dWN);",
}
vp, i32 = ctypes.c_void_p, ctypes.c_int
ARGTYPES = {
    "cfnmpc_eval_adjoint": [vp, vp, i32, vp, i32, i32, vp],
    "cfnmpc_get_adjoint": [vp, vp, vp, vp, vp, vp, i32, vp],
    "cfnmpc_get_adjoint_cost": [vp, vp, vp, vp, vp, i32, vp],
    "cfnmpc_fleet_eval_adjoint": [vp, vp, vp, i32, i32, vp],
    "cfnmpc_fleet_get_adjoint": [vp, vp, vp, vp, i32, vp],
    "cfnmpc_multi_eval_adjoint": [vp, vp, vp, i32],
    "cfnmpc_multi_get_adjoint": [vp, vp, vp, vp],
}
NEW_KERNELS = ("k_adj_wuni", "k_adj_bwd", "k_adj_fwd", "k_adj_mult")
# figures of the default-path kernels on the parent commit (vgpr, agpr, scratch, lds): the RTI / SQP kernels are unchanged
# (the table of tests/test_poly_cpu.py)
PARENT = {
    "k_as": (256, 112, 0, 10880), "k_as_cst": (256, 144, 0, 8576), "k_as_dense": (256, 256, 84, 34944),
    "k_as_retry": (256, 140, 0, 8576), "k_as_sbox": (256, 148, 0, 8576), "k_as_solves": (256, 58, 0, 10880),
    "k_ascommit": (218, 0, 0, 0), "k_ascommit1": (255, 30, 0, 0), "k_factor": (250, 0, 0, 10880),
    "k_forward": (256, 74, 0, 13568), "k_forward_erk": (256, 242, 0, 13568), "k_forward_erk_par": (256, 256, 0, 13568),
    "k_forward_p1": (256, 22, 0, 13312), "k_forward_p1_erk": (256, 192, 0, 13312), "k_forward_p1_erk_par": (256, 212, 0, 13312),
    "k_forward_p1_par": (256, 22, 0, 13312), "k_forward_p2": (256, 72, 0, 13568), "k_forward_p2_erk": (256, 242, 0, 13568),
    "k_forward_p2_erk_par": (256, 256, 0, 13568), "k_forward_p2_par": (256, 62, 0, 13568), "k_forward_par": (256, 72, 0, 13568),
    "k_forward_rg": (256, 8, 0, 0), "k_forward_rg_sbox": (256, 22, 0, 0), "k_ipm": (256, 256, 464, 8576),
    "k_ipm_cst": (256, 256, 460, 8576), "k_ipm_list": (38, 0, 0, 4096), "k_ipm_rest": (256, 256, 532, 8576),
    "k_ipm_rest_cst": (256, 256, 528, 8576), "k_ipm_rest_sbox": (256, 256, 596, 8576), "k_ipm_sbox": (256, 256, 572, 8576),
    "k_linearise": (256, 237, 0, 40192), "k_linearise_clist": (256, 256, 196, 40192), "k_linearise_erk": (256, 256, 72, 40192),
    "k_linearise_erk_par": (256, 256, 180, 40192), "k_linearise_par": (256, 243, 84, 40192),
    "k_sqp_check": (256, 24, 0, 13568), "k_sqp_check_par": (256, 40, 0, 13568),
}
# the sensitivity kernels the adjoint shares sens_stage with keep theirs too (vgpr, agpr, scratch, lds)
PARENT_SENS = {"k_sens_factor": (182, 0, 0, 8576), "k_sens_fwd": (199, 0, 0, 0), "k_sens_mask": (36, 0, 0, 0), "k_sens_first": (22, 0, 0, 0)}


# ---- numpy reference of the three sweeps (public state order) ----------------------------------------------------------------
def _inv(M):
    """inverse of a small SPD matrix in M's own precision (numpy's LAPACK routines know float64 only)"""
    if M.dtype == np.float64:
        return np.linalg.inv(M)
    n = M.shape[0]
    T = np.concatenate([M.copy(), np.eye(n, dtype=M.dtype)], axis=1)
    for c in range(n):                    # Gauss-Jordan without pivoting: SPD
        T[c] = T[c] / T[c, c]
        for r in range(n):
            if r != c:
                T[r] = T[r] - T[r, c] * T[c]
    return T[:, n:]


def adjoint_ref(A, B, Qd, Rd, QNd, act, gx, gu, dtype=np.float64):
    """A [N][13][13], B [N][13][4], effective diagonal weights, act [N][4] (non-zero = active), gx [N+1][13], gu [N][4]
    -> dict(ax [N+1][13], au [N][4], lam [N+1][13], mu [N][4]).  dtype = np.longdouble: the same recursion in extended
    precision, the measure of this reference's own rounding"""
    N = A.shape[0]
    act = np.asarray(act) != 0
    A, B, Qd, Rd, QNd, gx, gu = (np.asarray(v, dtype=dtype) for v in (A, B, Qd, Rd, QNd, gx, gu))
    P = np.diag(QNd)
    Kt = np.zeros((N, 4, 13), dtype=dtype)
    Si = [None] * N
    for k in range(N - 1, -1, -1):        # masked gains (sens_ref's recursion) and S_FF^-1
        F = ~act[k]
        BF = B[k][:, F]
        if F.any():
            Si[k] = _inv(np.diag(Rd[F]) + BF.T @ P @ BF)
            Kt[k][F] = -Si[k] @ (BF.T @ P @ A[k])
        P = np.diag(Qd) + A[k].T @ P @ A[k] + A[k].T @ P @ BF @ Kt[k][F]
    p = gx[N].copy()
    kap = np.zeros((N, 4), dtype=dtype)
    for k in range(N - 1, -1, -1):        # 1. backward
        F = ~act[k]
        w = gu[k] + B[k].T @ p
        if F.any():
            kap[k][F] = -Si[k] @ w[F]
        p = gx[k] + A[k].T @ p + Kt[k].T @ np.where(F, w, dtype(0))
    ax = np.zeros((N + 1, 13), dtype=dtype)
    au = np.zeros((N, 4), dtype=dtype)
    for k in range(N):                    # 2. forward
        au[k] = Kt[k] @ ax[k] + kap[k]
        ax[k + 1] = A[k] @ ax[k] + B[k] @ au[k]
    lam = np.zeros((N + 1, 13), dtype=dtype)
    mu = np.zeros((N, 4), dtype=dtype)
    lam[N] = QNd * ax[N] + gx[N]
    for k in range(N - 1, -1, -1):        # 3. backward again
        mu[k] = Rd * au[k] + gu[k] + B[k].T @ lam[k + 1]
        lam[k] = Qd * ax[k] + gx[k] + A[k].T @ lam[k + 1]
    return dict(ax=ax, au=au, lam=lam, mu=mu)


def gradients(r, act, Qd, Rd, QNd, z_x, z_u, yref, yref_e, stage_scale=1.0, terminal_scale=1.0):
    """the gradient table: r = adjoint_ref(...) with the EFFECTIVE weights Qd, Rd, QNd; z = the QP's solution (the new iterate)
    -> dict of the outputs of cfnmpc_get_adjoint / cfnmpc_get_adjoint_cost (dW / dWN with respect to the unscaled weights)"""
    act = np.asarray(act) != 0
    N = r["au"].shape[0]
    a = np.concatenate([r["ax"][:N], r["au"]], axis=1)
    Wd = np.concatenate([Qd, Rd])
    z = np.concatenate([z_x[:N], z_u], axis=1)
    return dict(dx0=r["lam"][0], dq=r["ax"], dr=r["au"], db=r["lam"][1:], dbox=np.where(act, r["mu"], 0.0),
                dyref=-Wd * a, dyref_e=-QNd * r["ax"][N], dW=stage_scale * (a * (z - yref)).sum(axis=0),
                dWN=terminal_scale * r["ax"][N] * (z_x[N] - yref_e))


def dense_kkt(qp, act, gx, gu):
    """the same problem as one dense KKT system: min 1/2 a'Ha + g'a  s.t.  ax_0 = 0, ax_{k+1} = A ax_k + B au_k, au_active = 0
    -> (ax, au, lam, mu) with lam / mu MINUS the multipliers of the constraints written as C a = 0"""
    N = qp.N
    nx, nu = 13, 4
    nz = (N + 1) * nx + N * nu
    ix = lambda k: slice(k * nx, (k + 1) * nx)
    iu = lambda k: slice((N + 1) * nx + k * nu, (N + 1) * nx + (k + 1) * nu)
    H = np.zeros((nz, nz)); g = np.zeros(nz)
    for k in range(N):
        H[ix(k), ix(k)] = np.diag(qp.Qd); g[ix(k)] = gx[k]
        H[iu(k), iu(k)] = np.diag(qp.Rd); g[iu(k)] = gu[k]
    H[ix(N), ix(N)] = np.diag(qp.QNd); g[ix(N)] = gx[N]
    rows = []
    r = np.zeros((nx, nz)); r[:, ix(0)] = np.eye(nx); rows.append(r)
    for k in range(N):
        r = np.zeros((nx, nz)); r[:, ix(k + 1)] = np.eye(nx); r[:, ix(k)] = -qp.A[k]; r[:, iu(k)] = -qp.B[k]; rows.append(r)
    aidx = [(k, a) for k in range(N) for a in range(nu) if act[k, a]]
    for k, a in aidx:
        r = np.zeros((1, nz)); r[0, (N + 1) * nx + k * nu + a] = 1.0; rows.append(r)
    Cm = np.vstack(rows)
    m = Cm.shape[0]
    sol = np.linalg.solve(np.block([[H, Cm.T], [Cm, np.zeros((m, m))]]), np.concatenate([-g, np.zeros(m)]))
    z, nu_ = sol[:nz], sol[nz:]
    lam = -nu_[:(N + 1) * nx].reshape(N + 1, nx)
    mu = np.zeros((N, 4))
    for (k, a), v in zip(aidx, nu_[(N + 1) * nx:]):
        mu[k, a] = -v
    return z[:(N + 1) * nx].reshape(N + 1, nx), z[(N + 1) * nx:].reshape(N, nu), lam, mu


def _header():
    src = open(os.path.join(ROOT, "include", "cfnmpc.h")).read()
    return re.sub(r"\s+", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


@pytest.fixture(scope="module")
def table():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cfn_resource_adj", os.path.join(ROOT, "tools", "resource.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    try:
        return mod.resource_table()
    except FileNotFoundError:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crazyflie_nmpc_amd", "csrc"), "-s", "ARCH=gfx950"])
        return mod.resource_table()


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


# ---- 1. the reference against a dense KKT solve ------------------------------------------------------------------------------
@pytest.mark.parametrize("N,scale,seed", [(12, 1.0, 1), (20, 2.5, 2), (30, 3.0, 3)])
def test_reference_equals_dense_kkt(oracle, N, scale, seed):
    rng = np.random.default_rng(100 + seed)
    n_act = 0
    for qp in hover_qps(oracle, 4, N, scale, seed):
        act = oracle.solve_qp_refined(qp)["cls"] != 0
        n_act += int(act.any())
        gx, gu = rng.normal(size=(N + 1, 13)), rng.normal(size=(N, 4))
        r = adjoint_ref(qp.A, qp.B, qp.Qd, qp.Rd, qp.QNd, act, gx, gu)
        ax, au, lam, mu = dense_kkt(qp, act, gx, gu)
        for name, a, b in (("ax", r["ax"], ax), ("au", r["au"], au), ("lam", r["lam"], lam), ("mu", np.where(act, r["mu"], 0.0), mu)):
            assert _rel(a, b) <= 1e-9, (name, _rel(a, b))
        # self-checks of the recursion: mu vanishes on free inputs, au on active ones, ax_0 = 0
        assert np.abs(r["mu"][~act]).max() <= 1e-9 * max(1.0, np.abs(r["mu"]).max())
        assert np.all(r["au"][act] == 0.0) and np.all(r["ax"][0] == 0.0)
    if scale >= 2.5:
        assert n_act >= 1   # constrained QPs are covered


def test_extended_precision_twin(oracle):
    """the longdouble evaluation of adjoint_ref (the GPU tests' measure of the reference's own rounding) is the same recursion"""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("no extended precision on this platform")
    N = 20
    rng = np.random.default_rng(4)
    qp = hover_qps(oracle, 1, N, 2.5, 2)[0]
    act = oracle.solve_qp_refined(qp)["cls"] != 0
    gx, gu = rng.normal(size=(N + 1, 13)), rng.normal(size=(N, 4))
    r = adjoint_ref(qp.A, qp.B, qp.Qd, qp.Rd, qp.QNd, act, gx, gu)
    x = adjoint_ref(qp.A, qp.B, qp.Qd, qp.Rd, qp.QNd, act, gx, gu, dtype=np.longdouble)
    for k in r:
        assert x[k].dtype == np.longdouble and _rel(r[k], x[k].astype(np.float64)) <= 1e-10, k


# ---- 2. the gradient table against central differences of the exact QP solution ---------------------------------------------
def test_reference_equals_central_differences(oracle):
    """l = sum gx . dx + gu . du of oracle.solve_qp_refined under +-h on entries of dx0, b, q, r and the bound an active input
    sits on; only pairs whose classification did not change count.  4 QPs x (4 + 4 + 3 + 2) = 52 perturbations of the QP's
    continuous data and up to 2 bounds per constrained QP; at least 40 of the former and one bound must remain."""
    N, h = 20, 1e-6
    rng = np.random.default_rng(11)
    checked = bounds = constrained = 0
    for qp in hover_qps(oracle, 4, N, 2.5, 7):
        sol = oracle.solve_qp_refined(qp)
        act = sol["cls"] != 0
        constrained += int(act.any())
        gx, gu = rng.normal(size=(N + 1, 13)), rng.normal(size=(N, 4))
        r = adjoint_ref(qp.A, qp.B, qp.Qd, qp.Rd, qp.QNd, act, gx, gu)
        targets = [("dx0", (int(j),), r["lam"][0][j]) for j in rng.choice(13, 4, replace=False)]
        targets += [("b", (int(k), int(j)), r["lam"][k + 1][j]) for k, j in zip(rng.integers(0, N, 4), rng.integers(0, 13, 4))]
        targets += [("q", (int(k), int(j)), r["ax"][k][j]) for k, j in zip(rng.integers(0, N + 1, 3), rng.integers(0, 13, 3))]
        targets += [("r", (int(k), int(a)), r["au"][k][a]) for k, a in zip(rng.integers(0, N, 2), rng.integers(0, 4, 2))]
        for k, a in np.argwhere(act)[:2]:
            targets.append(("lb" if sol["cls"][k, a] == 1 else "ub", (int(k), int(a)), r["mu"][k][a]))
        for field, idx, grad in targets:
            arr = getattr(qp, field)
            keep = arr[idx]
            ls, same = [], True
            for sgn in (1.0, -1.0):
                arr[idx] = keep + sgn * h
                s2 = oracle.solve_qp_refined(qp)
                same = same and np.array_equal(s2["cls"], sol["cls"])
                ls.append(float((gx * s2["dx"]).sum() + (gu * s2["du"]).sum()))
            arr[idx] = keep
            if not same:
                continue
            fd = (ls[0] - ls[1]) / (2 * h)
            scale = max(1.0, np.abs(r["lam"]).max(), np.abs(r["ax"]).max(), np.abs(r["mu"]).max())
            assert abs(fd - grad) <= 1e-6 * scale, (field, idx, fd, grad)
            if field in ("lb", "ub"):
                bounds += 1
            else:
                checked += 1
    assert checked >= 40 and bounds >= 1 and constrained >= 1, (checked, bounds, constrained)


def test_cost_gradients_against_central_differences(oracle):
    """yref, W and WN enter the QP through q, r and the Hessian: rebuild the QP around the same linearisation point with one
    entry moved by +-h and compare the change of l with the table's dl/dyref, dl/dW, dl/dWN (classification unchanged)."""
    N, h = 12, 1e-6
    rng = np.random.default_rng(5)
    x0 = oracle.sample_hover_x0(np.random.default_rng(3), 1, scale=2.5)[0]
    yref, yref_e = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    yref = yref + 0.01 * rng.normal(size=yref.shape)
    xbar = np.tile(yref_e, (N + 1, 1)); ubar = np.full((N, 4), oracle.HOV_W)
    base = oracle.build_qp(xbar, ubar, x0, yref, yref_e)
    Qd0, Rd0, QNd0 = base.Qd.copy(), base.Rd.copy(), base.QNd.copy()

    def make(Qd, Rd, QNd, yr, ye):
        qp = oracle.qp_from_blocks(base.A, base.B, base.b, np.vstack([Qd * (xbar[:N] - yr[:, :13]), QNd * (xbar[N] - ye)]),
                                   Rd * (ubar - yr[:, 13:]), base.dx0, Qd, Rd, QNd, base.lb, base.ub)
        return qp

    qp = make(Qd0, Rd0, QNd0, yref, yref_e)
    sol = oracle.solve_qp_refined(qp)
    act = sol["cls"] != 0
    gx, gu = rng.normal(size=(N + 1, 13)), rng.normal(size=(N, 4))
    r = adjoint_ref(qp.A, qp.B, Qd0, Rd0, QNd0, act, gx, gu)
    G = gradients(r, act, Qd0, Rd0, QNd0, xbar + sol["dx"], ubar + sol["du"], yref, yref_e)
    W0 = np.concatenate([Qd0, Rd0])
    cases = [("W", (j,)) for j in (0, 4, 9, 12, 13, 16)] + [("WN", (j,)) for j in (2, 7)] + \
            [("yref", (3, 1)), ("yref", (0, 14)), ("yref", (11, 8)), ("yref_e", (5,))]
    checked = 0
    for name, idx in cases:
        ls, same = [], True
        for sgn in (1.0, -1.0):
            W, WN, yr, ye = W0.copy(), QNd0.copy(), yref.copy(), yref_e.copy()
            {"W": W, "WN": WN, "yref": yr, "yref_e": ye}[name][idx] += sgn * h
            s2 = oracle.solve_qp_refined(make(W[:13], W[13:], WN, yr, ye))
            same = same and np.array_equal(s2["cls"], sol["cls"])
            ls.append(float((gx * s2["dx"]).sum() + (gu * s2["du"]).sum()))
        if not same:
            continue
        fd = (ls[0] - ls[1]) / (2 * h)
        grad = {"W": G["dW"], "WN": G["dWN"], "yref": G["dyref"], "yref_e": G["dyref_e"]}[name][idx]
        assert abs(fd - grad) <= 1e-6 * max(1.0, abs(grad)), (name, idx, fd, grad)
        checked += 1
    assert checked >= 10, checked


# ---- 3. identity with the forward sensitivities ------------------------------------------------------------------------------
@pytest.mark.parametrize("N,scale,seed", [(12, 1.0, 1), (20, 2.5, 2)])
def test_identity_with_forward_sensitivities(oracle, N, scale, seed):
    rng = np.random.default_rng(seed)
    for qp in hover_qps(oracle, 3, N, scale, seed):
        act = oracle.solve_qp_refined(qp)["cls"] != 0
        gx, gu = rng.normal(size=(N + 1, 13)), rng.normal(size=(N, 4))
        r = adjoint_ref(qp.A, qp.B, qp.Qd, qp.Rd, qp.QNd, act, gx, gu)
        du, dx = sens_ref(qp.A, qp.B, qp.Qd, qp.Rd, qp.QNd, act)
        want = np.einsum("kij,ki->j", dx, gx) + np.einsum("kaj,ka->j", du, gu)
        assert _rel(r["lam"][0], want) <= 1e-11


# ---- 4. surface --------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_and_bound():
    src = _header()
    from crazyflie_nmpc_amd import _lib
    L = _lib.lib()
    for name, sig in SIGS.items():
        assert sig in src, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == ARGTYPES[name], name
    assert L.cfnmpc_abi_version() == 9 == _lib.ABI_VERSION


def test_python_surface():
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.parallel import MultiGpuFleet
    from crazyflie_nmpc_amd.solver import BatchSolver
    for cls, names in ((BatchSolver, ("eval_adjoint", "adjoint", "adjoint_cost")), (MixedHorizonFleet, ("eval_adjoint", "adjoint")),
                       (MultiGpuFleet, ("eval_adjoint", "adjoint"))):
        for m in names:
            assert callable(getattr(cls, m)), (cls, m)
    import inspect
    assert list(inspect.signature(BatchSolver.eval_adjoint).parameters)[1:] == ["gx", "gu", "stream"]
    pytest.importorskip("torch")
    from crazyflie_nmpc_amd import diff
    assert list(inspect.signature(diff.rti_step).parameters)[:6] == ["solver", "x0", "W", "WN", "yref", "yref_e"]
    import torch
    assert issubclass(diff._RtiStep, torch.autograd.Function)


def test_adjoint_kernels_resources(table):
    for k in NEW_KERNELS:
        assert k in table, k
        r = table[k]
        assert r["scratch"] == 0, (k, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (k, r)
        assert r["lds"] <= 16384, (k, r)
        assert r["occupancy"] >= 2, (k, r)


def test_default_kernels_keep_parent_figures(table):
    for k, (v, a, sc, lds) in {**PARENT, **PARENT_SENS}.items():
        r = table[k]
        assert (r["vgpr"], r["agpr"], r["scratch"], r["lds"]) == (v, a, sc, lds), (k, r)
    for k in ("k_sens_factor", "k_sens_fwd"):
        assert table[k]["occupancy"] >= table["k_factor"]["occupancy"] >= 2, (k, table[k])
