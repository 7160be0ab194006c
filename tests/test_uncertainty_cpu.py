"""CPU checks of the uncertainty propagation and robust input-bound tightening (include/cfnmpc.h: cfnmpc_set_uncertainty,
cfnmpc_eval_uncertainty, cfnmpc_get_backoff, cfnmpc_get_uncertainty, cfnmpc_tighten_box): the numpy
reference of the covariance recursion the GPU tests compare against equals the same recursion in extended precision and the
product form X_k Sigma_0 X_k' with W = 0; the new entry points are declared, exported and bound; the new kernels are in the built
code without scratch at two waves per SIMD while the default-step kernels keep the parent's figures.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, i32, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
SIGS = {
    "cfnmpc_set_uncertainty": "intcfnmpc_set_uncertainty(cfnmpc_solver*s,constdouble*Sigma0,constdouble*W,inton_device,void*stream);",
    "cfnmpc_set_uncertainty_gain": "intcfnmpc_set_uncertainty_gain(cfnmpc_solver*s,intmode,constdouble*K,inton_device,void*stream);",
    "cfnmpc_eval_uncertainty": "intcfnmpc_eval_uncertainty(cfnmpc_solver*s,void*stream);",
    "cfnmpc_get_backoff": "intcfnmpc_get_backoff(cfnmpc_solver*s,double*beta,inton_device,void*stream);",
    "cfnmpc_get_uncertainty": "intcfnmpc_get_uncertainty(cfnmpc_solver*s,intstage,intn_stages,double*Sigma,double*std_x,"
                              "inton_device,void*stream);",
    "cfnmpc_tighten_box": "intcfnmpc_tighten_box(cfnmpc_solver*s,doublegamma,doublemin_width,int*n_clamped,inton_device,void*stream);",
    "cfnmpc_fleet_set_uncertainty": "intcfnmpc_fleet_set_uncertainty(cfnmpc_fleet*f,constdouble*Sigma0,constdouble*W,inton_device,void*stream);",
    "cfnmpc_fleet_set_uncertainty_gain": "intcfnmpc_fleet_set_uncertainty_gain(cfnmpc_fleet*f,intmode,constdouble*K,inton_device,void*stream);",
    "cfnmpc_fleet_eval_uncertainty": "intcfnmpc_fleet_eval_uncertainty(cfnmpc_fleet*f,void*stream);",
    "cfnmpc_fleet_get_backoff": "intcfnmpc_fleet_get_backoff(cfnmpc_fleet*f,double*beta,inton_device,void*stream);",
    "cfnmpc_fleet_get_uncertainty": "intcfnmpc_fleet_get_uncertainty(cfnmpc_fleet*f,intstage,intn_stages,double*Sigma,double*std_x,"
                                    "inton_device,void*stream);",
    "cfnmpc_fleet_tighten_box": "intcfnmpc_fleet_tighten_box(cfnmpc_fleet*f,doublegamma,doublemin_width,int*n_clamped,inton_device,void*stream);",
    "cfnmpc_multi_set_uncertainty": "intcfnmpc_multi_set_uncertainty(cfnmpc_multi*m,constdouble*Sigma0,constdouble*W);",
    "cfnmpc_multi_set_uncertainty_gain": "intcfnmpc_multi_set_uncertainty_gain(cfnmpc_multi*m,intmode,constdouble*K);",
    "cfnmpc_multi_eval_uncertainty": "intcfnmpc_multi_eval_uncertainty(cfnmpc_multi*m);",
    "cfnmpc_multi_get_backoff": "intcfnmpc_multi_get_backoff(cfnmpc_multi*m,double*beta);",
    "cfnmpc_multi_tighten_box": "intcfnmpc_multi_tighten_box(cfnmpc_multi*m,doublegamma,doublemin_width,int*n_clamped);",
}
ARGTYPES = {
    "set_uncertainty": [vp, vp, vp, i32, vp], "set_uncertainty_gain": [vp, i32, vp, i32, vp], "eval_uncertainty": [vp, vp],
    "get_backoff": [vp, vp, i32, vp], "get_uncertainty": [vp, i32, i32, vp, vp, i32, vp], "tighten_box": [vp, dbl, dbl, vp, i32, vp],
}
MULTI_ARGTYPES = {
    "set_uncertainty": [vp, vp, vp], "set_uncertainty_gain": [vp, i32, vp], "eval_uncertainty": [vp], "get_backoff": [vp, vp],
    "tighten_box": [vp, dbl, dbl, vp],
}
NEW_KERNELS = ("k_unc_prop", "k_unc_tighten", "k_unc_put_sym", "k_unc_put_gain")
# figures of the default-step kernels on the parent commit (vgpr, agpr, scratch, lds): the RTI / SQP kernels are unchanged
PARENT = {
    "k_as": (256, 112, 0, 10880), "k_as_cst": (256, 144, 0, 8576), "k_as_dense": (256, 256, 84, 34944),
    "k_as_retry": (256, 140, 0, 8576), "k_as_sbox": (256, 148, 0, 8576), "k_as_solves": (256, 58, 0, 10880),
    "k_ascommit": (218, 0, 0, 0), "k_ascommit1": (255, 30, 0, 0), "k_factor": (250, 0, 0, 10880),
    "k_forward": (256, 74, 0, 13568), "k_forward_p1": (256, 22, 0, 13312), "k_forward_p2": (256, 72, 0, 13568),
    "k_forward_rg": (256, 8, 0, 0), "k_forward_rg_sbox": (256, 22, 0, 0), "k_ipm": (256, 256, 464, 8576),
    "k_ipm_list": (38, 0, 0, 4096), "k_ipm_rest": (256, 256, 532, 8576), "k_ipm_rest_sbox": (256, 256, 596, 8576),
    "k_ipm_sbox": (256, 256, 572, 8576), "k_linearise": (256, 237, 0, 40192), "k_linearise_clist": (256, 256, 196, 40192),
    "k_sqp_check": (256, 24, 0, 13568),
}


# ---- numpy reference of the recursion (public state order) -------------------------------------------------------------------
def unc_ref(A, B, K, S0, W, dtype=np.float64):
    """A [N][13][13], B [N][13][4], K [N][4][13] or [4][13] (du = -K dx), S0, W [13][13]
    -> (Sigma [N+1][13][13], beta [N][4]): M = A - B K, Sigma+ = M Sigma M' + W, beta_a = sqrt((K Sigma K')_aa)"""
    N = A.shape[0]
    A, B, K, W = (np.asarray(v, dtype=dtype) for v in (A, B, K, W))
    if K.ndim == 2:
        K = np.repeat(K[None], N, 0)
    Sig = np.zeros((N + 1, 13, 13), dtype=dtype)
    beta = np.zeros((N, 4), dtype=dtype)
    Sig[0] = np.asarray(S0, dtype=dtype)
    for k in range(N):
        beta[k] = np.sqrt(np.maximum(np.einsum("al,lm,am->a", K[k], Sig[k], K[k]), 0))
        M = A[k] - B[k] @ K[k]
        Sig[k + 1] = M @ Sig[k] @ M.T + W
    return Sig, beta


def unc_ref_other_order(A, B, K, S0, W):
    """the same recursion with the products grouped the other way: Sigma+ = (A Sigma - B (K Sigma)) M' + W"""
    N = A.shape[0]
    Sig = np.zeros((N + 1, 13, 13))
    Sig[0] = S0
    for k in range(N):
        U = K[k] @ Sig[k]
        Y = A[k] @ Sig[k] - B[k] @ U
        Sig[k + 1] = Y @ (A[k] - B[k] @ K[k]).T + W
    return Sig


def random_cov(rng, n, std=(0.01,) * 3 + (0.01,) * 4 + (0.05,) * 3 + (0.05,) * 3):
    """n random symmetric positive definite [13][13] with the given standard deviations (public order: position 1 cm, attitude
    0.01, velocity 5 cm/s, rates 0.05 rad/s) and random correlations"""
    std = np.asarray(std)
    out = np.empty((n, 13, 13))
    for i in range(n):
        G = rng.standard_normal((13, 26))
        Cm = G @ G.T
        d = 1.0 / np.sqrt(np.diag(Cm))
        Cm = Cm * d[:, None] * d[None, :]
        S = Cm * std[:, None] * std[None, :]
        out[i] = 0.5 * (S + S.T)
    return out


def kicked_qps(oracle, n, N, seed, scale=1.0):
    """QPs around kicked hover iterates: state and input iterates perturbed per stage, so that the blocks differ by stage"""
    rng = np.random.default_rng(seed)
    yref, yref_e = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    out = []
    for x0 in oracle.sample_hover_x0(rng, n, scale=scale):
        xbar = oracle.sample_hover_x0(rng, N + 1, scale=0.5 * scale)
        ubar = oracle.HOV_W + rng.uniform(-2.0, 2.0, (N, 4))
        out.append(oracle.build_qp(xbar, ubar, x0, yref, yref_e))
    return out


def _stage_err(a, b):
    """max over stages of |a_k - b_k| / (largest entry of b_k)"""
    ax = tuple(range(1, a.ndim))
    den = np.maximum(np.abs(b).max(axis=ax), 1e-300)
    return float((np.abs(a - b).max(axis=ax) / den).max())


@pytest.mark.parametrize("N,seed", [(5, 1), (5, 2), (5, 3), (50, 4), (50, 5), (50, 6)])
def test_reference_against_extended_precision_and_product_form(oracle, N, seed):
    rng = np.random.default_rng(100 + seed)
    qp = kicked_qps(oracle, 1, N, seed)[0]
    K, _Si, _d = oracle._riccati_factor(qp, np.tile(qp.Rd, (N, 1)), qp.r)
    S0 = random_cov(rng, 1)[0]
    W = 0.01 * random_cov(rng, 1)[0]          # (0.1 std)^2
    Sig, beta = unc_ref(qp.A, qp.B, K, S0, W)
    # two FP64 orderings of the recursion, and FP64 against extended precision
    e_ord = _stage_err(unc_ref_other_order(qp.A, qp.B, K, S0, W), Sig)
    SigL, betaL = unc_ref(qp.A, qp.B, K, S0, W, dtype=np.longdouble)
    e_ld = max(_stage_err(Sig, SigL.astype(np.float64)), _stage_err(beta, betaL.astype(np.float64)))
    # W = 0: Sigma_k = X_k Sigma_0 X_k' with X_k = prod (A - B K)
    Sig0, beta0 = unc_ref(qp.A, qp.B, K, S0, np.zeros((13, 13)))
    X = np.eye(13)
    prod = np.empty_like(Sig0)
    for k in range(N + 1):
        prod[k] = X @ S0 @ X.T
        if k < N:
            X = (qp.A[k] - qp.B[k] @ K[k]) @ X
    e_prod = _stage_err(Sig0, prod)
    print(f"N = {N}: orderings {e_ord:.1e}, long double {e_ld:.1e}, product form {e_prod:.1e}")
    assert e_ord <= 1e-12 and e_ld <= 1e-12 and e_prod <= 1e-12
    # symmetric, positive, and the backoff is the standard deviation of K dx
    assert np.abs(Sig - Sig.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(Sig).max()
    assert (np.diagonal(Sig, axis1=1, axis2=2) > 0).all() and (beta > 0).all()
    # a constant user gain takes the [4][13] form
    Sc, bc = unc_ref(qp.A, qp.B, K[0], S0, W)
    Sr, br = unc_ref(qp.A, qp.B, np.repeat(K[:1], N, 0), S0, W)
    assert np.array_equal(Sc, Sr) and np.array_equal(bc, br)


def _header():
    src = open(os.path.join(ROOT, "include", "cfnmpc.h")).read()
    return re.sub(r"\s+", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


@pytest.fixture(scope="module")
def table():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cfn_resource_unc", os.path.join(ROOT, "tools", "resource.py"))
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
    for pre in ("cfnmpc_", "cfnmpc_fleet_"):
        for n, at in ARGTYPES.items():
            assert list(getattr(L, pre + n).argtypes) == at, pre + n
    for n, at in MULTI_ARGTYPES.items():
        assert list(getattr(L, "cfnmpc_multi_" + n).argtypes) == at, n
    assert "#defineCFNMPC_UNC_GAIN_RICCATI0" in src and "#defineCFNMPC_UNC_GAIN_USER1" in src
    assert L.cfnmpc_abi_version() == 9 == _lib.ABI_VERSION


def test_python_surface():
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.parallel import MultiGpuFleet
    from crazyflie_nmpc_amd.solver import BatchSolver
    names = ("set_uncertainty", "set_uncertainty_gain", "eval_uncertainty", "backoff", "uncertainty", "tighten_box")
    for cls in (BatchSolver, MixedHorizonFleet, MultiGpuFleet):
        for m in names:
            if cls is MultiGpuFleet and m == "uncertainty":   # (the full covariance: through the shards' solvers)
                continue
            assert callable(getattr(cls, m)), (cls, m)


def test_uncertainty_kernels_resources(table):
    for k in NEW_KERNELS:
        assert k in table, k
        r = table[k]
        assert r["scratch"] == 0 and r["lds"] == 0, (k, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (k, r)
        assert r["occupancy"] >= 2, (k, r)
    assert table["k_unc_prop"]["occupancy"] >= table["k_factor"]["occupancy"] >= 2


def test_default_kernels_keep_parent_figures(table):
    for k, (v, a, sc, lds) in PARENT.items():
        r = table[k]
        assert (r["vgpr"], r["agpr"], r["scratch"], r["lds"]) == (v, a, sc, lds), (k, r)
