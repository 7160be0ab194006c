"""CPU checks of the solution sensitivities with respect to x0 (include/cfnmpc.h: cfnmpc_eval_sens_x0, cfnmpc_get_sens_x0,
cfnmpc_get_sens_active): the new entry points are declared, exported and bound, the new kernels are in
the built code within their budgets while the default-path kernels keep the parent's figures, and the numpy reference of the
masked Riccati recursion the GPU tests compare against equals a dense referee (condensed QP with the active set fixed) and
central differences of the extended-precision QP solution.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGS = {
    "cfnmpc_eval_sens_x0": "intcfnmpc_eval_sens_x0(cfnmpc_solver*s,doubleact_tol,void*stream);",
    "cfnmpc_get_sens_x0": "intcfnmpc_get_sens_x0(cfnmpc_solver*s,intstage,intn_stages,double*du,double*dx,inton_device,"
                          "void*stream);",
    "cfnmpc_get_sens_active": "intcfnmpc_get_sens_active(cfnmpc_solver*s,signedchar*act,inton_device,void*stream);",
    "cfnmpc_fleet_eval_sens_x0": "intcfnmpc_fleet_eval_sens_x0(cfnmpc_fleet*f,doubleact_tol,void*stream);",
    "cfnmpc_fleet_get_sens_x0": "intcfnmpc_fleet_get_sens_x0(cfnmpc_fleet*f,intstage,intn_stages,double*du,double*dx,"
                                "inton_device,void*stream);",
    "cfnmpc_multi_eval_sens_x0": "intcfnmpc_multi_eval_sens_x0(cfnmpc_multi*m,doubleact_tol);",
    "cfnmpc_multi_get_sens_x0": "intcfnmpc_multi_get_sens_x0(cfnmpc_multi*m,intstage,intn_stages,double*du,double*dx);",
}
vp, i32, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
ARGTYPES = {
    "cfnmpc_eval_sens_x0": [vp, dbl, vp],
    "cfnmpc_get_sens_x0": [vp, i32, i32, vp, vp, i32, vp],
    "cfnmpc_get_sens_active": [vp, vp, i32, vp],
    "cfnmpc_fleet_eval_sens_x0": [vp, dbl, vp],
    "cfnmpc_fleet_get_sens_x0": [vp, i32, i32, vp, vp, i32, vp],
    "cfnmpc_multi_eval_sens_x0": [vp, dbl],
    "cfnmpc_multi_get_sens_x0": [vp, i32, i32, vp, vp],
}
NEW_KERNELS = ("k_sens_mask", "k_sens_factor", "k_sens_fwd", "k_sens_first")
# figures of the default-path kernels on the parent commit (vgpr, agpr, scratch, lds): the RTI / SQP kernels are unchanged
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


# ---- numpy reference of the masked recursion (public state order) ------------------------------------------------------------
def sens_ref(A, B, Qd, Rd, QNd, act):
    """A [N][13][13], B [N][13][4], diagonal weights, act [N][4] (non-zero = active) -> (du [N][4][13], dx [N+1][13][13])"""
    N = A.shape[0]
    act = np.asarray(act) != 0
    P = np.diag(np.asarray(QNd, dtype=np.float64))
    Kt = np.zeros((N, 4, 13))
    for k in range(N - 1, -1, -1):
        F = ~act[k]
        BF = B[k][:, F]
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


def dense_referee(oracle, qp, act):
    """dV/dx0 = -H_FF^-1 Gam_F' Qbar dg/dx0, dX/dx0 = Gam dV/dx0 + dg/dx0 on the condensed QP with the active set fixed"""
    H, _h, Gam, _g = oracle.condense(qp)
    N = qp.N
    G0 = np.zeros(((N + 1) * 13, 13))
    G0[:13] = np.eye(13)
    for k in range(N):
        G0[(k + 1) * 13:(k + 2) * 13] = qp.A[k] @ G0[k * 13:(k + 1) * 13]
    Qbar = np.concatenate([np.tile(qp.Qd, N), qp.QNd])
    F = ~(np.asarray(act).reshape(-1) != 0)
    dV = np.zeros((N * 4, 13))
    dV[F] = -np.linalg.solve(H[np.ix_(F, F)], (Gam[:, F].T * Qbar) @ G0)
    dX = Gam @ dV + G0
    return dV.reshape(N, 4, 13), dX.reshape(N + 1, 13, 13)


def hover_qps(oracle, n, N, scale, seed):
    rng = np.random.default_rng(seed)
    x0s = oracle.sample_hover_x0(rng, n, scale=scale)
    yref, yref_e = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    out = []
    for x0 in x0s:
        xbar = np.tile(yref_e, (N + 1, 1))
        ubar = np.full((N, 4), oracle.HOV_W)
        out.append(oracle.build_qp(xbar, ubar, x0, yref, yref_e))
    return out


def _header():
    src = open(os.path.join(ROOT, "include", "cfnmpc.h")).read()
    return re.sub(r"\s+", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


@pytest.fixture(scope="module")
def table():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cfn_resource_sens", os.path.join(ROOT, "tools", "resource.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    try:
        return mod.resource_table()
    except FileNotFoundError:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crazyflie_nmpc_amd", "csrc"), "-s", "ARCH=gfx950"])
        return mod.resource_table()


def test_entry_points_declared_exported_and_bound():
    src = _header()
    from crazyflie_nmpc_amd import _lib
    L = _lib.lib()
    for name, sig in SIGS.items():
        assert sig in src, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == ARGTYPES[name], name
    assert L.cfnmpc_abi_version() == 9


def test_dropin_symbols_declared_and_exported():
    h = re.sub(r"\s+", "", re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "acados_solver_crazyflie.h")).read(), flags=re.S))
    assert "ocp_nlp_out*ocp_nlp_out_create(ocp_nlp_config*config,ocp_nlp_dims*dims);" in h
    assert "voidocp_nlp_out_destroy(void*out);" in h
    assert "voidocp_nlp_eval_param_sens(ocp_nlp_solver*solver,char*field,intstage,intindex,ocp_nlp_out*sens_out);" in h
    from crazyflie_nmpc_amd import _lib
    _lib.lib()
    shim = ctypes.CDLL(os.path.join(ROOT, "crazyflie_nmpc_amd", "libacados_solver_crazyflie.so"))
    for name in ("ocp_nlp_out_create", "ocp_nlp_out_destroy", "ocp_nlp_eval_param_sens"):
        assert hasattr(shim, name), name


def test_python_surface():
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.parallel import MultiGpuFleet
    from crazyflie_nmpc_amd.solver import BatchSolver
    for cls, names in ((BatchSolver, ("eval_sens_x0", "sens_x0", "sens_active")), (MixedHorizonFleet, ("eval_sens_x0", "sens_x0")),
                       (MultiGpuFleet, ("eval_sens_x0", "sens_x0"))):
        for m in names:
            assert callable(getattr(cls, m)), (cls, m)


def test_sens_kernels_resources(table):
    for k in NEW_KERNELS:
        assert k in table, k
        r = table[k]
        assert r["scratch"] == 0, (k, r)
        assert r["lds"] <= 16384, (k, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (k, r)
    for k in ("k_sens_factor", "k_sens_fwd"):
        assert table[k]["occupancy"] >= table["k_factor"]["occupancy"] >= 2, (k, table[k])


def test_default_kernels_keep_parent_figures(table):
    for k, (v, a, sc, lds) in PARENT.items():
        r = table[k]
        assert (r["vgpr"], r["agpr"], r["scratch"], r["lds"]) == (v, a, sc, lds), (k, r)


@pytest.mark.parametrize("N,scale,seed", [(12, 1.0, 1), (20, 2.5, 2), (30, 3.0, 3)])
def test_reference_equals_dense_referee(oracle, N, scale, seed):
    qps = hover_qps(oracle, 4, N, scale, seed)
    n_act = 0
    for qp in qps:
        sol = oracle.solve_qp_refined(qp)
        act = sol["cls"] != 0
        n_act += int(act.any())
        du, dx = sens_ref(qp.A, qp.B, qp.Qd, qp.Rd, qp.QNd, act)
        dV, dX = dense_referee(oracle, qp, act)
        assert np.abs(du - dV).max() <= 1e-10 * max(1.0, np.abs(dV).max())
        assert np.abs(dx - dX).max() <= 1e-10 * max(1.0, np.abs(dX).max())
        assert np.all(du[act] == 0.0)
    if scale >= 2.5:
        assert n_act >= 1   # constrained QPs are covered


def test_reference_equals_central_differences(oracle):
    N, h = 20, 1e-6
    qps = hover_qps(oracle, 6, N, 2.5, 7)
    checked = constrained = 0
    for qp in qps:
        sol = oracle.solve_qp_refined(qp)
        du, dx = sens_ref(qp.A, qp.B, qp.Qd, qp.Rd, qp.QNd, sol["cls"] != 0)
        dx0 = qp.dx0.copy()
        for j in range(13):
            res = []
            for sgn in (1.0, -1.0):
                qp.dx0 = dx0.copy()
                qp.dx0[j] += sgn * h
                res.append(oracle.solve_qp_refined(qp))
            qp.dx0 = dx0
            if not (np.array_equal(res[0]["cls"], sol["cls"]) and np.array_equal(res[1]["cls"], sol["cls"])):
                continue
            fu = (res[0]["du"] - res[1]["du"]) / (2 * h)
            fx = (res[0]["dx"] - res[1]["dx"]) / (2 * h)
            assert np.abs(fu - du[:, :, j]).max() <= 1e-6 * max(1.0, np.abs(du[:, :, j]).max())
            assert np.abs(fx - dx[:, :, j]).max() <= 1e-6 * max(1.0, np.abs(dx[:, :, j]).max())
            checked += 1
        constrained += int((sol["cls"] != 0).any())
    assert checked >= 13 * 4 and constrained >= 1
