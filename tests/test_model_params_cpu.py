"""CPU checks of the per-instance model parameters (include/cfnmpc.h: cfnmpc_set_model_params, cfnmpc_sim_params;
DESIGN.md section 5.13): the new entry points are declared, exported and bound, the ABI is unchanged, the _par kernels are in
the built code within their resource ceilings while the folded-constant kernels keep the figures of the parent commit, and
the numpy reference the GPU tests compare against (f(x, u, p), its Jacobians, M-step RK4 with sensitivities) is right.
No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGS = {
    "cfnmpc_set_model_params": "intcfnmpc_set_model_params(cfnmpc_solver*s,constdouble*p,inton_device,void*stream);",
    "cfnmpc_get_model_params": "intcfnmpc_get_model_params(cfnmpc_solver*s,double*p,inton_device,void*stream);",
    "cfnmpc_fleet_set_model_params": "intcfnmpc_fleet_set_model_params(cfnmpc_fleet*f,constdouble*p);",
    "cfnmpc_multi_set_model_params": "intcfnmpc_multi_set_model_params(cfnmpc_multi*m,constdouble*p);",
    "cfnmpc_sim_params": "intcfnmpc_sim_params(intbatch,constdouble*x,constdouble*u,constdouble*p,doubleT,intsteps,double*xn,"
                         "inton_device,void*stream);",
}
vp, i32, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
ARGTYPES = {
    "cfnmpc_set_model_params": [vp, vp, i32, vp],
    "cfnmpc_get_model_params": [vp, vp, i32, vp],
    "cfnmpc_fleet_set_model_params": [vp, vp],
    "cfnmpc_multi_set_model_params": [vp, vp],
    "cfnmpc_sim_params": [i32, vp, vp, vp, dbl, i32, vp, i32, vp],
}
FWD_PAR = ("k_forward_par", "k_forward_p1_par", "k_forward_p2_par", "k_cforward_par",
           "k_forward_erk_par", "k_forward_p1_erk_par", "k_forward_p2_erk_par", "k_cforward_erk_par")
# figures of the folded-constant kernels on the parent commit (vgpr, agpr, scratch, lds): the default path is unchanged
PARENT = {
    "k_linearise": (256, 237, 0, 40192), "k_linearise_erk": (256, 256, 72, 40192),
    "k_forward": (256, 74, 0, 13568), "k_forward_p1": (256, 22, 0, 13312), "k_forward_p2": (256, 72, 0, 13568),
    "k_cforward": (256, 82, 0, 13568), "k_forward_erk": (256, 242, 0, 13568), "k_forward_p1_erk": (256, 192, 0, 13312),
    "k_forward_p2_erk": (256, 242, 0, 13568), "k_cforward_erk": (256, 252, 0, 13568),
    "k_sqp_check": (256, 24, 0, 13568), "k_sim": (124, 0, 0, 0), "k_init_iterate": (12, 0, 0, 0),
}

NOMINAL = np.array([9.8066, 33e-3, 1.395e-5, 1.395e-5, 2.173e-5, 7.9379e-06, 3.25e-4, 0.0325])


# ---- numpy reference: f(x, u, p), Jacobians, M-step RK4 with sensitivities (external state order) --------------------------
def consts(p):
    """the eight derived constants, by the expressions of csrc/cfnmpc_model.hpp"""
    g0, mq, ixx, iyy, izz, cd, ct, arm = (float(v) for v in p)
    return (g0, ct / mq, -ct * arm / ixx, -ct * arm / iyy, -cd / izz,
            -(izz - iyy) / ixx, -(ixx - izz) / iyy, -(iyy - ixx) / izz)


def f(x, u, p):
    """export_ode_model.py:85-97 with the parameters of row p (x, u may be complex: complex-step Jacobians)"""
    g0, kt, ka, kb, kc, kwx, kwy, kwz = consts(p)
    q1, q2, q3, q4 = x[3], x[4], x[5], x[6]
    vx, vy, vz = x[7], x[8], x[9]
    wx, wy, wz = x[10], x[11], x[12]
    s1, s2, s3, s4 = u[0] * u[0], u[1] * u[1], u[2] * u[2], u[3] * u[3]
    return np.array([
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


def jac(x, u, p):
    """(df/dx [13][13], df/du [13][4]) by complex steps: f is a polynomial in (x, u), so these are exact to rounding"""
    hc = 1e-40
    x = np.asarray(x, dtype=np.complex128); u = np.asarray(u, dtype=np.complex128)
    A = np.empty((13, 13)); Bm = np.empty((13, 4))
    for c in range(13):
        e = x.copy(); e[c] += 1j * hc
        A[:, c] = f(e, u, p).imag / hc
    for c in range(4):
        e = u.copy(); e[c] += 1j * hc
        Bm[:, c] = f(x, e, p).imag / hc
    return A, Bm


def rk4_sens(x, u, p, dt=0.015, M=1):
    """M classic RK4 steps of dt / M and their sensitivities: (Phi, A = dPhi/dx, B = dPhi/du)"""
    h = dt / M
    xs = np.asarray(x, dtype=np.float64).copy()
    u = np.asarray(u, dtype=np.float64)
    A = np.eye(13); Bm = np.zeros((13, 4))
    for _ in range(M):
        Sx, Su = np.eye(13), np.zeros((13, 4))
        ks, kx, ku = [], [], []
        xt, Tx, Tu = xs, Sx, Su
        for c in (0.5, 0.5, 1.0, None):
            k = f(xt, u, p)
            fx, fu = jac(xt, u, p)
            dkx, dku = fx @ Tx, fx @ Tu + fu
            ks.append(k); kx.append(dkx); ku.append(dku)
            if c is not None:
                xt, Tx, Tu = xs + c * h * k, Sx + c * h * dkx, Su + c * h * dku
        xn = xs + (h / 6) * (ks[0] + 2 * ks[1] + 2 * ks[2] + ks[3])
        Aj = Sx + (h / 6) * (kx[0] + 2 * kx[1] + 2 * kx[2] + kx[3])
        Bj = Su + (h / 6) * (ku[0] + 2 * ku[1] + 2 * ku[2] + ku[3])
        xs, A, Bm = xn, Aj @ A, Aj @ Bm + Bj
    return xs, A, Bm


def rk4(x, u, p, dt, M=1):
    h = dt / M
    xs = np.asarray(x, dtype=np.float64).copy()
    for _ in range(M):
        k1 = f(xs, u, p); k2 = f(xs + 0.5 * h * k1, u, p); k3 = f(xs + 0.5 * h * k2, u, p); k4 = f(xs + h * k3, u, p)
        xs = xs + (h / 6) * (k1 + 2 * k2 + 2 * k3 + k4)
    return xs


def random_params(rng, B, nominal_g0=False):
    """rows drawn around the nominal one: mq +-30 %, inertias +-25 %, Ct / Cd +-15 %, l +-10 %, g0 9.8066 or 9.80665"""
    p = np.tile(NOMINAL, (B, 1))
    p[:, 0] = 9.8066 if nominal_g0 else rng.choice([9.8066, 9.80665], B)
    p[:, 1] *= rng.uniform(0.7, 1.3, B)
    p[:, 2:5] *= rng.uniform(0.75, 1.25, (B, 3))
    p[:, 5] *= rng.uniform(0.85, 1.15, B)
    p[:, 6] *= rng.uniform(0.85, 1.15, B)
    p[:, 7] *= rng.uniform(0.9, 1.1, B)
    return p


def hover(p):
    p = np.asarray(p)
    return np.sqrt((p[..., 1] * p[..., 0]) / (4 * p[..., 6]))


# ---- tests ---------------------------------------------------------------------------------------------------------------
def _header():
    src = open(os.path.join(ROOT, "include", "cfnmpc.h")).read()
    return re.sub(r"\s+", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


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


def test_entry_points_declared_exported_and_bound():
    src = _header()
    from crazyflie_nmpc_amd import _lib
    L = _lib.lib()
    for name, sig in SIGS.items():
        assert sig in src, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == ARGTYPES[name], name
    assert "#defineCFNMPC_NP8" in src


def test_abi_unchanged():
    from crazyflie_nmpc_amd import _lib
    L = _lib.lib()
    assert L.cfnmpc_abi_version() == 9
    assert L.cfnmpc_opts_size() == ctypes.sizeof(_lib.Opts)
    assert "#defineCFNMPC_ABI_VERSION9" in _header()


def test_python_surface():
    import inspect
    import crazyflie_nmpc_amd as cf
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.parallel import MultiGpuFleet
    assert tuple(cf.PARAM_NAMES) == ("g0", "mq", "Ixx", "Iyy", "Izz", "Cd", "Ct", "l")
    assert np.array_equal(cf.NOMINAL_PARAMS, NOMINAL)
    assert NOMINAL[7] == 65e-3 / 2                                 # the arm of the folded constants, exactly
    assert cf.hover_speed(NOMINAL) == np.sqrt((33e-3 * 9.8066) / (4 * 3.25e-4))
    assert np.array_equal(cf.hover_speed(np.tile(NOMINAL, (3, 1))), np.full(3, cf.hover_speed(NOMINAL)))
    for cls in (cf.BatchSolver, MixedHorizonFleet, MultiGpuFleet):
        assert inspect.signature(cls.set_model_params).parameters["p"].default is None
    assert callable(cf.BatchSolver.model_params)
    assert inspect.signature(cf.sim).parameters["params"].default is None


def test_par_kernels_resources(table):
    for k in ("k_linearise_par", "k_linearise_erk_par", "k_sqp_check_par", "k_sim_par", "k_init_iterate_par") + FWD_PAR:
        assert k in table, k
        r = table[k]
        assert r["unit"] == "cfnmpc_kernels", r
        assert r["occupancy"] >= 1 and r["vgpr"] <= 256 and not r.get("dynamic_stack"), (k, r)
    lin = table["k_linearise_par"]
    assert lin["scratch"] <= 96 and lin["lds"] <= 40960, lin
    for k in FWD_PAR:
        # (k_cforward_par, the one-step sweep of the partial-condensing path only: 20 B of scratch)
        assert table[k]["scratch"] <= (20 if k == "k_cforward_par" else 0) and table[k]["lds"] <= 13568, (k, table[k])
    for k in ("k_sim_par", "k_sqp_check_par"):
        assert table[k]["scratch"] == 0, (k, table[k])


def test_folded_kernels_keep_parent_figures(table):
    for k, (v, a, sc, lds) in PARENT.items():
        r = table[k]
        assert (r["vgpr"], r["agpr"], r["scratch"], r["lds"]) == (v, a, sc, lds), (k, r)


def test_reference_at_nominal_matches_oracle(oracle):
    rng = np.random.default_rng(3)
    for _ in range(4):
        x = oracle.sample_hover_x0(rng, 1, scale=1.5)[0]
        x[10:13] += rng.normal(0, 2.0, 3)
        u = oracle.HOV_W + rng.normal(0, 3.0, 4)
        assert np.abs(f(x, u, NOMINAL) - oracle.f_expl(x, u)).max() < 1e-13
        phi, A, Bm = rk4_sens(x, u, NOMINAL)
        phi_o, A_o, B_o = oracle.rk4_sens(x, u)
        assert np.abs(phi - phi_o).max() < 1e-13
        assert np.abs(A - A_o).max() < 1e-13 and np.abs(Bm - B_o).max() < 1e-13


@pytest.mark.parametrize("M", [1, 3])
def test_reference_sensitivities_at_random_params(oracle, M):
    rng = np.random.default_rng(20 + M)
    dt, eps = 0.015, 1e-5
    for p in random_params(rng, 3):
        x = oracle.sample_hover_x0(rng, 1, scale=1.5)[0]
        x[10:13] += rng.normal(0, 2.0, 3)
        u = hover(p) + rng.normal(0, 3.0, 4)
        phi, A, Bm = rk4_sens(x, u, p, dt, M)
        assert np.abs(phi - rk4(x, u, p, dt, M)).max() < 1e-13
        for c in range(13):
            e = np.zeros(13); e[c] = eps
            fd = (rk4(x + e, u, p, dt, M) - rk4(x - e, u, p, dt, M)) / (2 * eps)
            assert np.abs(A[:, c] - fd).max() < 1e-7, (c, np.abs(A[:, c] - fd).max())
        for c in range(4):
            e = np.zeros(4); e[c] = eps
            fd = (rk4(x, u + e, p, dt, M) - rk4(x, u - e, p, dt, M)) / (2 * eps)
            assert np.abs(Bm[:, c] - fd).max() < 1e-7, (c, np.abs(Bm[:, c] - fd).max())
        # the parameters matter: the same point under the nominal model moves elsewhere
        assert np.abs(phi - rk4(x, u, NOMINAL, dt, M)).max() > 1e-6
