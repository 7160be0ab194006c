"""CPU checks of the per-instance disturbance model, disturbed plant and observer (include/cfnmpc.h: cfnmpc_set_disturbance,
cfnmpc_sim_dist, cfnmpc_estimate_disturbance): the entry points are declared, exported and bound, the ABI
is unchanged, the _dst kernels are in the built code within their resource ceilings while the folded and _par kernels keep their
figures, and the numpy reference the GPU tests compare against is right: tests/test_model_params_cpu.py's f(x, u, p) wrapped
with the two disturbance terms (still a polynomial in (x, u): complex-step Jacobians stay exact), its M-step RK4 with
sensitivities, and a restatement of the observer.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import test_model_params_cpu as mp
from test_model_params_cpu import NOMINAL, _header, hover, random_params, table  # noqa: F401  (table: the fixture)

ND = 6
SIGS = {
    "cfnmpc_set_disturbance": "intcfnmpc_set_disturbance(cfnmpc_solver*s,constdouble*d,inton_device,void*stream);",
    "cfnmpc_get_disturbance": "intcfnmpc_get_disturbance(cfnmpc_solver*s,double*d,inton_device,void*stream);",
    "cfnmpc_sim_dist": "intcfnmpc_sim_dist(intbatch,constdouble*x,constdouble*u,constdouble*p,constdouble*d,doubleT,intsteps,"
                       "double*xn,inton_device,void*stream);",
    "cfnmpc_estimate_disturbance": "intcfnmpc_estimate_disturbance(intbatch,constdouble*x_prev,constdouble*u_prev,"
                                   "constdouble*x_meas,constdouble*p,double*d,doubleT,intsteps,doublegain_a,doublegain_w,"
                                   "inton_device,void*stream);",
    "cfnmpc_fleet_set_disturbance": "intcfnmpc_fleet_set_disturbance(cfnmpc_fleet*f,constdouble*d,inton_device,void*stream);",
    "cfnmpc_fleet_get_disturbance": "intcfnmpc_fleet_get_disturbance(cfnmpc_fleet*f,double*d,inton_device,void*stream);",
    "cfnmpc_multi_set_disturbance": "intcfnmpc_multi_set_disturbance(cfnmpc_multi*m,constdouble*d);",
}
vp, i32, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
ARGTYPES = {
    "cfnmpc_set_disturbance": [vp, vp, i32, vp],
    "cfnmpc_get_disturbance": [vp, vp, i32, vp],
    "cfnmpc_sim_dist": [i32, vp, vp, vp, vp, dbl, i32, vp, i32, vp],
    "cfnmpc_estimate_disturbance": [i32, vp, vp, vp, vp, vp, dbl, i32, dbl, dbl, i32, vp],
    "cfnmpc_fleet_set_disturbance": [vp, vp, i32, vp],
    "cfnmpc_fleet_get_disturbance": [vp, vp, i32, vp],
    "cfnmpc_multi_set_disturbance": [vp, vp],
}
LIN_DST = ("k_linearise_dst", "k_linearise_erk_dst")
FWD_DST = ("k_forward_dst", "k_forward_p1_dst", "k_forward_p2_dst")
FWD_ERK_DST = ("k_forward_erk_dst", "k_forward_p1_erk_dst", "k_forward_p2_erk_dst")
OTHER_DST = ("k_sqp_check_dst", "k_sqp_ls_dst", "k_nlp_eval_dst", "k_sim_dst", "k_dist_put", "k_dist_observe")
# scratch of k_linearise_dst as built (248 B), rounded up to 16 B; k_linearise_par: 84 B
LIN_DST_SCRATCH = 256


# ---- numpy reference: f(x, u, p, d) and what follows from it (external state order) ---------------------------------------
def rot(q):
    """R(q) of p' = R(q) v_b (csrc/cfnmpc_model.hpp: JacPoint::R); q may be complex"""
    q1, q2, q3, q4 = q
    return np.array([
        [2 * q1 * q1 + 2 * q2 * q2 - 1, -(2 * q1 * q4 - 2 * q2 * q3), 2 * q1 * q3 + 2 * q2 * q4],
        [2 * q1 * q4 + 2 * q2 * q3, 2 * q1 * q1 + 2 * q3 * q3 - 1, -(2 * q1 * q2 - 2 * q3 * q4)],
        [-(2 * q1 * q3 - 2 * q2 * q4), 2 * q1 * q2 + 2 * q3 * q4, 2 * q1 * q1 + 2 * q4 * q4 - 1]])


def f(x, u, p, d):
    """f(x, u, p) of tests/test_model_params_cpu.py with v_b' += R(q)' a_w, w' += al_b"""
    dx = mp.f(x, u, p)
    d = np.asarray(d, dtype=np.float64)
    dx[7:10] = dx[7:10] + rot(x[3:7]).T @ d[0:3]
    dx[10:13] = dx[10:13] + d[3:6]
    return dx


def jac(x, u, p, d):
    """(df/dx, df/du) by complex steps, exact to rounding"""
    hc = 1e-40
    x = np.asarray(x, dtype=np.complex128); u = np.asarray(u, dtype=np.complex128)
    A = np.empty((13, 13)); Bm = np.empty((13, 4))
    for c in range(13):
        e = x.copy(); e[c] += 1j * hc
        A[:, c] = f(e, u, p, d).imag / hc
    for c in range(4):
        e = u.copy(); e[c] += 1j * hc
        Bm[:, c] = f(x, e, p, d).imag / hc
    return A, Bm


def rk4(x, u, p, d, dt, M=1):
    h = dt / M
    xs = np.asarray(x, dtype=np.float64).copy()
    for _ in range(M):
        k1 = f(xs, u, p, d); k2 = f(xs + 0.5 * h * k1, u, p, d); k3 = f(xs + 0.5 * h * k2, u, p, d); k4 = f(xs + h * k3, u, p, d)
        xs = xs + (h / 6) * (k1 + 2 * k2 + 2 * k3 + k4)
    return xs


def rk4_sens(x, u, p, d, dt=0.015, M=1):
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
            k = f(xt, u, p, d)
            fx, fu = jac(xt, u, p, d)
            dkx, dku = fx @ Tx, fx @ Tu + fu
            ks.append(k); kx.append(dkx); ku.append(dku)
            if c is not None:
                xt, Tx, Tu = xs + c * h * k, Sx + c * h * dkx, Su + c * h * dku
        xn = xs + (h / 6) * (ks[0] + 2 * ks[1] + 2 * ks[2] + ks[3])
        Aj = Sx + (h / 6) * (kx[0] + 2 * kx[1] + 2 * kx[2] + kx[3])
        Bj = Su + (h / 6) * (ku[0] + 2 * ku[1] + 2 * ku[2] + ku[3])
        xs, A, Bm = xn, Aj @ A, Aj @ Bm + Bj
    return xs, A, Bm


def observe(x_prev, u_prev, x_meas, p, d, T, steps, gain_a, gain_w):
    """cfnmpc_estimate_disturbance for one row -> the new d"""
    e = np.asarray(x_meas) - rk4(x_prev, u_prev, p, d, T, steps)
    out = np.array(d, dtype=np.float64)
    out[0:3] += gain_a / T * (rot(np.asarray(x_prev)[3:7]) @ e[7:10])
    out[3:6] += gain_w / T * e[10:13]
    return out


def random_dist(rng, B, a_max=2.0, al_max=5.0):
    return np.concatenate([rng.uniform(-a_max, a_max, (B, 3)), rng.uniform(-al_max, al_max, (B, 3))], axis=1)


# ---- surface -----------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_and_bound():
    src = _header()
    from crazyflie_nmpc_amd import _lib
    L = _lib.lib()
    for name, sig in SIGS.items():
        assert sig in src, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == ARGTYPES[name], name
    assert "#defineCFNMPC_ND6" in src


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
    assert tuple(cf.DIST_NAMES) == ("ax", "ay", "az", "alx", "aly", "alz")
    for cls in (cf.BatchSolver, MixedHorizonFleet, MultiGpuFleet):
        assert inspect.signature(cls.set_disturbance).parameters["d"].default is None
    assert inspect.signature(cf.BatchSolver.set_disturbance).parameters["stream"].default is None
    assert callable(cf.BatchSolver.disturbance)
    assert inspect.signature(cf.sim).parameters["dist"].default is None
    sg = inspect.signature(cf.estimate_disturbance).parameters
    assert list(sg)[:4] == ["x_prev", "u_prev", "x_meas", "d"]
    assert (sg["T"].default, sg["steps"].default, sg["gain_a"].default, sg["gain_w"].default, sg["params"].default) == \
        (0.015, 1, 0.5, 0.5, None)


# ---- resources ---------------------------------------------------------------------------------------------------------------
def test_dst_kernels_resources(table):  # noqa: F811
    for k in LIN_DST + FWD_DST + FWD_ERK_DST + OTHER_DST:
        assert k in table, k
        r = table[k]
        assert r["unit"] == "cfnmpc_kernels", r
        assert r["occupancy"] >= 1 and r["vgpr"] <= 256 and not r.get("dynamic_stack"), (k, r)
    for k in LIN_DST:
        assert table[k]["lds"] <= 40960, (k, table[k])
    for k in FWD_DST + FWD_ERK_DST:
        assert table[k]["lds"] <= 13568, (k, table[k])
    for k in FWD_DST + ("k_sim_dst", "k_sqp_check_dst", "k_dist_put", "k_dist_observe"):
        assert table[k]["scratch"] == 0, (k, table[k])
    assert table["k_linearise_dst"]["scratch"] <= LIN_DST_SCRATCH, table["k_linearise_dst"]


def test_folded_and_par_kernels_keep_their_figures(table):  # noqa: F811
    for k, (v, a, sc, lds) in mp.PARENT.items():
        r = table[k]
        assert (r["vgpr"], r["agpr"], r["scratch"], r["lds"]) == (v, a, sc, lds), (k, r)
    mp.test_par_kernels_resources(table)


# ---- the reference -----------------------------------------------------------------------------------------------------------
def _point(oracle, rng, p):
    x = oracle.sample_hover_x0(rng, 1, scale=1.5)[0]
    x[10:13] += rng.normal(0, 2.0, 3)
    return x, hover(p) + rng.normal(0, 3.0, 4)


def test_reference_zero_disturbance_and_gravity(oracle):
    rng = np.random.default_rng(7)
    for p in random_params(rng, 4):
        x, u = _point(oracle, rng, p)
        assert np.array_equal(f(x, u, p, np.zeros(ND)), mp.f(x, u, p))
        delta = rng.uniform(-1.0, 1.0)
        pg = p.copy(); pg[0] += delta
        # a world-frame acceleration (0, 0, -delta) is delta more gravity
        assert np.abs(f(x, u, p, [0, 0, -delta, 0, 0, 0]) - mp.f(x, u, pg)).max() <= 1e-13
        assert np.abs(rk4(x, u, p, [0, 0, -delta, 0, 0, 0], 0.015, 3) - mp.rk4(x, u, pg, 0.015, 3)).max() <= 1e-13


@pytest.mark.parametrize("M", [1, 3])
def test_reference_sensitivities(oracle, M):
    rng = np.random.default_rng(30 + M)
    dt, eps = 0.015, 1e-5
    for p, d in zip(random_params(rng, 3), random_dist(rng, 3)):
        x, u = _point(oracle, rng, p)
        phi, A, Bm = rk4_sens(x, u, p, d, dt, M)
        assert np.abs(phi - rk4(x, u, p, d, dt, M)).max() < 1e-13
        for c in range(13):
            e = np.zeros(13); e[c] = eps
            fd = (rk4(x + e, u, p, d, dt, M) - rk4(x - e, u, p, d, dt, M)) / (2 * eps)
            assert np.abs(A[:, c] - fd).max() < 1e-7, (c, np.abs(A[:, c] - fd).max())
        for c in range(4):
            e = np.zeros(4); e[c] = eps
            fd = (rk4(x, u + e, p, d, dt, M) - rk4(x, u - e, p, d, dt, M)) / (2 * eps)
            assert np.abs(Bm[:, c] - fd).max() < 1e-7, (c, np.abs(Bm[:, c] - fd).max())
        # the pattern of A is that of the undisturbed model: the disturbance adds to d v' / d q only
        A0 = mp.rk4_sens(x, u, p, dt, M)[1]
        assert ((A != 0) <= (A0 != 0)).all()
        # the disturbance matters
        assert np.abs(phi - mp.rk4(x, u, p, dt, M)).max() > 1e-4


@pytest.mark.parametrize("gain,steps,tol", [(1.0, 10, 1e-10), (0.5, 40, 1e-9)])
def test_observer_restatement_converges(oracle, gain, steps, tol):
    """noise-free disturbed plant, random inputs, perturbed hover states: the estimate reaches the true row (plant and model
    are the same map, so it is a fixed point)"""
    rng = np.random.default_rng(11)
    T = 0.015
    worst = 0.0
    for p, d_true in zip(random_params(rng, 8), random_dist(rng, 8)):
        x = oracle.sample_hover_x0(rng, 1, scale=1.0)[0]
        d = np.zeros(ND)
        for _ in range(steps):
            u = hover(p) + rng.normal(0, 1.0, 4)
            xn = rk4(x, u, p, d_true, T, 1)
            d = observe(x, u, xn, p, d, T, 1, gain, gain)
            x = xn
        worst = max(worst, np.abs(d - d_true).max())
    print(f"observer gain {gain}: |d^ - d| = {worst:.2e} after {steps} steps")
    assert worst <= tol
