"""CPU checks of the differentiable plant rollouts (include/cfnmpc.h: cfnmpc_sim_rollout, cfnmpc_sim_rollout_vjp; DESIGN.md section
5.25): the entry points are declared, exported and bound, the ABI is unchanged, the new kernels are in the built code within their
recorded ceilings while every earlier kernel keeps its figures, and the reference the GPU tests compare against is right:

  (a) ref_vjp_cs: complex-step differentiation through the WHOLE numpy rollout, one complex rollout per input scalar (x0, u, the
      public parameter row, the disturbance row), all of them and all vehicles in one vectorised batch;
  (b) ref_vjp_rev: a numpy reverse sweep through RK4 with complex-step stage Jacobians with respect to (x, u, the eight derived
      constants, d), and the chain rule through derive_k's expressions at the end.

f below is tests/test_model_params_cpu.py's f with tests/test_disturbance_cpu.py's disturbance terms, restated over a leading
component axis so that the constants and the disturbance may be complex (mp.consts casts its row to float); the restatement is
checked against those two.  Error measure everywhere: per vehicle and output array, max |difference| / max(1, max |reference|),
the parameter gradient as gp * p (the gradient with respect to log p).  The stand-alone program tools/sim_vjp_check.cpp runs the
host-compiled reverse step on cases written here, under the host sanitizers.  No GPU needed."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import test_disturbance_cpu as dc
import test_model_params_cpu as mp
from test_model_params_cpu import NOMINAL, ROOT, _header, hover, table  # noqa: F401  (table: the fixture)

SIGS = {
    "cfnmpc_sim_rollout": "intcfnmpc_sim_rollout(intbatch,intL,constdouble*x0,constdouble*u,constdouble*p,constdouble*d,doubleT,"
                          "intsteps,double*xs,inton_device,void*stream);",
    "cfnmpc_sim_rollout_vjp": "intcfnmpc_sim_rollout_vjp(intbatch,intL,constdouble*xs,constdouble*u,constdouble*p,constdouble*d,"
                              "doubleT,intsteps,constdouble*gxs,double*gx0,double*gu,double*gp,double*gd,inton_device,void*stream);",
}
vp, i32, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
ARGTYPES = {
    "cfnmpc_sim_rollout": [i32, i32, vp, vp, vp, vp, dbl, i32, vp, i32, vp],
    "cfnmpc_sim_rollout_vjp": [i32, i32, vp, vp, vp, vp, dbl, i32, vp, vp, vp, vp, vp, i32, vp],
}
ROLLOUT = ("k_sim_rollout", "k_sim_rollout_par", "k_sim_rollout_dst")
VJP = ("k_sim_rollout_vjp", "k_sim_rollout_vjp_par", "k_sim_rollout_vjp_dst")
# ceilings of the new kernels, VGPRs + AGPRs of the unified file (512 per lane at one wave per SIMD): the figures of the build
# (128, 144, 198 | 388, 428, 493) rounded up to 8; no scratch, no LDS
VGPR_CEIL = {"k_sim_rollout": 128, "k_sim_rollout_par": 144, "k_sim_rollout_dst": 200,
             "k_sim_rollout_vjp": 392, "k_sim_rollout_vjp_par": 432, "k_sim_rollout_vjp_dst": 496}
ROWS = ("none", "p", "d", "pd")


# ---- the model over a leading component axis, complex-capable in every argument ---------------------------------------------
def derive(p):
    """the eight derived constants of rows p [8, ...] by derive_k's expressions (csrc/cfnmpc_model.hpp); p may be complex"""
    g0, mq, ixx, iyy, izz, cd, ct, arm = p
    return np.stack([g0 + 0 * mq, ct / mq, -ct * arm / ixx, -ct * arm / iyy, -cd / izz,
                     -(izz - iyy) / ixx, -(ixx - izz) / iyy, -(iyy - ixx) / izz])


def f(x, u, k, d):
    """mp.f with dc.f's disturbance terms: x [13, ...], u [4, ...], k [8, ...] derived constants, d [6, ...]"""
    g0, kt, ka, kb, kc, kwx, kwy, kwz = k
    q1, q2, q3, q4 = x[3], x[4], x[5], x[6]
    vx, vy, vz = x[7], x[8], x[9]
    wx, wy, wz = x[10], x[11], x[12]
    s1, s2, s3, s4 = u[0] * u[0], u[1] * u[1], u[2] * u[2], u[3] * u[3]
    R = dc.rot((q1, q2, q3, q4))
    ax, ay, az = d[0], d[1], d[2]
    return np.stack([
        vx * (2 * q1 * q1 + 2 * q2 * q2 - 1) - vy * (2 * q1 * q4 - 2 * q2 * q3) + vz * (2 * q1 * q3 + 2 * q2 * q4),
        vy * (2 * q1 * q1 + 2 * q3 * q3 - 1) + vx * (2 * q1 * q4 + 2 * q2 * q3) - vz * (2 * q1 * q2 - 2 * q3 * q4),
        vz * (2 * q1 * q1 + 2 * q4 * q4 - 1) - vx * (2 * q1 * q3 - 2 * q2 * q4) + vy * (2 * q1 * q2 + 2 * q3 * q4),
        -(q2 * wx) / 2 - (q3 * wy) / 2 - (q4 * wz) / 2,
        (q1 * wx) / 2 - (q4 * wy) / 2 + (q3 * wz) / 2,
        (q4 * wx) / 2 + (q1 * wy) / 2 - (q2 * wz) / 2,
        (q2 * wy) / 2 - (q3 * wx) / 2 + (q1 * wz) / 2,
        vy * wz - vz * wy + g0 * (2 * q1 * q3 - 2 * q2 * q4) + (R[0][0] * ax + R[1][0] * ay + R[2][0] * az),
        vz * wx - vx * wz - g0 * (2 * q1 * q2 + 2 * q3 * q4) + (R[0][1] * ax + R[1][1] * ay + R[2][1] * az),
        vx * wy - vy * wx - g0 * (2 * q1 * q1 + 2 * q4 * q4 - 1) + kt * (s1 + s2 + s3 + s4) + (R[0][2] * ax + R[1][2] * ay + R[2][2] * az),
        ka * (s1 + s2 - s3 - s4) + kwx * (wy * wz) + d[3],
        kb * (s1 - s2 - s3 + s4) + kwy * (wx * wz) + d[4],
        kc * (s1 - s2 + s3 - s4) + kwz * (wx * wy) + d[5],
    ])


def rk4_step(x, u, k, d, h):
    k1 = f(x, u, k, d); k2 = f(x + 0.5 * h * k1, u, k, d); k3 = f(x + 0.5 * h * k2, u, k, d); k4 = f(x + h * k3, u, k, d)
    return x + (h / 6) * (k1 + 2 * k2 + 2 * k3 + k4)


def rollout(x0, u, p, d, T, steps):
    """x0 [M, 13], u [M, L, 4], p [M, 8], d [M, 6] (any of them complex) -> xs [M, L + 1, 13]"""
    k = derive(np.moveaxis(p, -1, 0))
    dd = np.moveaxis(d, -1, 0)
    x = np.moveaxis(x0, -1, 0)
    out = [x]
    for t in range(u.shape[1]):
        ut = np.moveaxis(u[:, t], -1, 0)
        for _ in range(steps):
            x = rk4_step(x, ut, k, dd, T / steps)
        out.append(x)
    return np.moveaxis(np.stack(out), (0, 1), (1, 2))


def ref_vjp_cs(x0, u, p, d, gxs, T, steps):
    """(a): the gradient of sum(gxs * xs) with respect to (x0, u, p, d) by complex steps through the whole rollout
    -> (gx0 [B, 13], gu [B, L, 4], gp [B, 8], gd [B, 6])"""
    B, L = u.shape[0], u.shape[1]
    n = 13 + 4 * L + 8 + 6
    hc = 1e-30
    z = np.concatenate([x0, u.reshape(B, -1), p, d], axis=1).astype(np.complex128)   # [B, n]
    Z = np.repeat(z[:, None, :], n, axis=1)                                           # [B, n, n]: direction j perturbs entry j
    Z[:, np.arange(n), np.arange(n)] += 1j * hc
    Z = Z.reshape(B * n, n)
    xs = rollout(Z[:, :13], Z[:, 13:13 + 4 * L].reshape(B * n, L, 4), Z[:, 13 + 4 * L:21 + 4 * L], Z[:, 21 + 4 * L:], T, steps)
    g = (xs.imag.reshape(B, n, L + 1, 13) * gxs[:, None]).sum(axis=(2, 3)) / hc
    return g[:, :13], g[:, 13:13 + 4 * L].reshape(B, L, 4), g[:, 13 + 4 * L:21 + 4 * L], g[:, 21 + 4 * L:]


def _stage_jac(x, u, k, d):
    """complex-step Jacobians of f at points x [13, B] -> (fx [B, 13, 13], fu [B, 13, 4], fk [B, 13, 8], fd [B, 13, 6])"""
    hc = 1e-30
    out = []
    args = [x.astype(np.complex128), u.astype(np.complex128), k.astype(np.complex128), d.astype(np.complex128)]
    for a in range(4):
        cols = []
        for c in range(args[a].shape[0]):
            pert = [v.copy() if i == a else v for i, v in enumerate(args)]
            pert[a][c] += 1j * hc
            cols.append(f(*pert).imag / hc)          # [13, B]
        out.append(np.moveaxis(np.stack(cols), (0, 1, 2), (2, 1, 0)))   # [B, 13, ncols]
    return out


def ref_vjp_rev(x0, u, p, d, gxs, T, steps):
    """(b): reverse sweep through RK4, stage by stage, with complex-step stage Jacobians; the parameter gradient through the
    Jacobian of derive() (complex steps) at the end"""
    B, L = u.shape[0], u.shape[1]
    h = T / steps
    pT = np.moveaxis(p, -1, 0); dT = np.moveaxis(d, -1, 0)
    k = derive(pT)
    # forward: every sub-step's start state
    starts = []
    x = np.moveaxis(x0, -1, 0)
    for t in range(L):
        ut = np.moveaxis(u[:, t], -1, 0)
        for _ in range(steps):
            starts.append((x, ut, t))
            x = rk4_step(x, ut, k, dT, h)
    lam = gxs[:, L].copy()
    gu = np.zeros((B, L, 4)); gk = np.zeros((B, 8)); gd = np.zeros((B, 6))
    tv = lambda J, v: np.einsum("bij,bi->bj", J, v)   # noqa: E731  (J' v per vehicle)
    for n in range(len(starts) - 1, -1, -1):
        x, ut, t = starts[n]
        k1 = f(x, ut, k, dT); x2 = x + 0.5 * h * k1
        k2 = f(x2, ut, k, dT); x3 = x + 0.5 * h * k2
        k3 = f(x3, ut, k, dT); x4 = x + h * k3
        J = [_stage_jac(xx, ut, k, dT) for xx in (x, x2, x3, x4)]
        kb4 = h / 6 * lam
        kb3 = h / 3 * lam + h * tv(J[3][0], kb4)
        kb2 = h / 3 * lam + h / 2 * tv(J[2][0], kb3)
        kb1 = h / 6 * lam + h / 2 * tv(J[1][0], kb2)
        kbs = (kb1, kb2, kb3, kb4)
        lam = lam + sum(tv(J[i][0], kbs[i]) for i in range(4))
        gu[:, t] += sum(tv(J[i][1], kbs[i]) for i in range(4))
        gk += sum(tv(J[i][2], kbs[i]) for i in range(4))
        gd += sum(tv(J[i][3], kbs[i]) for i in range(4))
        if n % steps == 0:
            lam = lam + gxs[:, t]
    hc = 1e-30
    gp = np.empty((B, 8))
    for c in range(8):
        pc = pT.astype(np.complex128)
        pc[c] += 1j * hc * pT[c]            # a relative step: the entries span five decades
        gp[:, c] = (gk * np.moveaxis(derive(pc).imag, 0, -1)).sum(axis=1) / (hc * pT[c])
    return lam, gu, gp, gd


# ---- the draw of the issue and the error measure ---------------------------------------------------------------------------
def draw(seed, B, L):
    """p = nominal x U(0.8, 1.25) per entry, d = (U(+-2)^3, U(+-5)^3), position U(+-1), q = normalised (1, 0, 0, 0) + U(+-0.15),
    v U(+-1), w U(+-2), u = own hover speed + U(+-3), random gxs"""
    rng = np.random.default_rng(seed)
    p = NOMINAL * rng.uniform(0.8, 1.25, (B, 8))
    d = dc.random_dist(rng, B, 2.0, 5.0)
    x0 = np.empty((B, 13))
    x0[:, 0:3] = rng.uniform(-1, 1, (B, 3))
    q = np.array([1.0, 0, 0, 0]) + rng.uniform(-0.15, 0.15, (B, 4))
    x0[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    x0[:, 7:10] = rng.uniform(-1, 1, (B, 3))
    x0[:, 10:13] = rng.uniform(-2, 2, (B, 3))
    u = hover(p)[:, None, None] + rng.uniform(-3, 3, (B, L, 4))
    gxs = rng.uniform(-1, 1, (B, L + 1, 13))
    return dict(x0=x0, u=u, p=p, d=d, gxs=gxs)


def rows_of(c, rows):
    """(p, d) the model of a row combination uses: the nominal row / the zero row where the combination sets none"""
    B = c["x0"].shape[0]
    return (c["p"] if "p" in rows else np.tile(NOMINAL, (B, 1))), (c["d"] if "d" in rows else np.zeros((B, 6)))


@functools.lru_cache(maxsize=None)
def reference(seed, B, L, steps, rows, T=0.015):
    """the shared reference (a) of one shape and row combination -> (case, (gx0, gu, gp, gd)); computed once, never written to"""
    c = draw(seed, B, L)
    p, d = rows_of(c, rows)
    g = ref_vjp_cs(c["x0"], c["u"], p, d, c["gxs"], T, steps)
    for a in list(c.values()) + list(g):
        a.setflags(write=False)
    return c, g


def scaled_err(got, ref, scale=None):
    """per vehicle: max |got - ref| / max(1, max |ref|) over the trailing axes (scale: gp * p)"""
    B = ref.shape[0]
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if scale is not None:
        got, ref = got * scale, ref * scale
    num = np.abs(got - ref).reshape(B, -1).max(axis=1)
    return num / np.maximum(1.0, np.abs(ref).reshape(B, -1).max(axis=1))


def worst_err(got, ref, p):
    """worst scaled error over vehicles and the four output arrays (entries of `got` that are None are not compared)"""
    w = 0.0
    for i, (a, b) in enumerate(zip(got, ref)):
        if a is not None:
            w = max(w, float(scaled_err(a, b, p if i == 2 else None).max()))
    return w


# ---- surface and figures -----------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_and_bound():
    src = _header()
    from crazyflie_nmpc_amd import _lib
    L = _lib.lib()
    for name, sig in SIGS.items():
        assert sig in src, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == ARGTYPES[name], name


def test_abi_unchanged():
    from crazyflie_nmpc_amd import _lib
    L = _lib.lib()
    assert L.cfnmpc_abi_version() == 9
    assert L.cfnmpc_opts_size() == ctypes.sizeof(_lib.Opts)
    assert "#defineCFNMPC_ABI_VERSION9" in _header()


def test_python_surface():
    import inspect
    import crazyflie_nmpc_amd as cf
    from crazyflie_nmpc_amd import diff
    sg = inspect.signature(cf.sim_rollout).parameters
    assert list(sg) == ["x0", "u", "T", "steps", "out", "params", "dist"]
    assert (sg["T"].default, sg["steps"].default, sg["out"].default, sg["params"].default, sg["dist"].default) == (0.015, 1, None, None, None)
    sg = inspect.signature(cf.sim_rollout_vjp).parameters
    assert list(sg) == ["xs", "u", "gxs", "T", "steps", "params", "dist", "out"]
    assert (sg["T"].default, sg["steps"].default, sg["params"].default, sg["dist"].default, sg["out"].default) == (0.015, 1, None, None, None)
    assert "sim_rollout" in cf.__all__ and "sim_rollout_vjp" in cf.__all__
    for fn, first in ((diff.sim_rollout, ["x0", "u"]), (diff.sim_step, ["x", "u"])):
        sg = inspect.signature(fn).parameters
        assert list(sg) == first + ["params", "dist", "T", "steps"]
        assert (sg["params"].default, sg["dist"].default, sg["T"].default, sg["steps"].default) == (None, None, 0.015, 1)
    assert "sim_step(x0, u, p, d)" in diff.__doc__ and "one BatchSolver per step" in diff.__doc__


def test_new_kernels_resources(table):  # noqa: F811
    for k in ROLLOUT + VJP:
        assert k in table, k
        r = table[k]
        assert r["unit"] == "cfnmpc_kernels", r
        assert r["occupancy"] >= 1 and not r.get("dynamic_stack"), (k, r)
        assert r["scratch"] == 0 and r["lds"] == 0, (k, r)
        assert r["vgpr"] + r["agpr"] <= VGPR_CEIL[k], (k, r)


def test_earlier_kernels_keep_their_figures(table):  # noqa: F811
    for k, (v, a, sc, lds) in mp.PARENT.items():
        r = table[k]
        assert (r["vgpr"], r["agpr"], r["scratch"], r["lds"]) == (v, a, sc, lds), (k, r)
    mp.test_par_kernels_resources(table)
    dc.test_dst_kernels_resources(table)


# ---- the reference is right --------------------------------------------------------------------------------------------------
def test_restatement_is_the_suite_model():
    """f above against dc.f (mp.f with the disturbance terms), and the rollout against chained dc.rk4, row by row"""
    c = draw(3, 5, 3)
    k = derive(c["p"].T)
    for i in range(5):
        a = f(c["x0"][i], c["u"][i, 0], k[:, i], c["d"][i])
        b = dc.f(c["x0"][i], c["u"][i, 0], c["p"][i], c["d"][i])
        assert np.abs(a - b).max() <= 1e-13 * max(1.0, np.abs(b).max())
        assert np.array_equal(k[:, i], np.array(mp.consts(c["p"][i])))
    xs = rollout(c["x0"], c["u"], c["p"], c["d"], 0.015, 3)
    assert np.array_equal(xs[:, 0], c["x0"])
    for i in range(5):
        x = c["x0"][i]
        for t in range(3):
            x = dc.rk4(x, c["u"][i, t], c["p"][i], c["d"][i], 0.015, 3)
            assert np.abs(xs[i, t + 1] - x).max() <= 1e-13


@pytest.mark.parametrize("L,steps", [(1, 1), (2, 3), (7, 1), (20, 3)])
def test_two_references_agree(L, steps):
    worst = 0.0
    for rows in ("none", "pd"):
        c, ga = reference(11, 8, L, steps, rows)
        p, d = rows_of(c, rows)
        gb = ref_vjp_rev(c["x0"], c["u"], p, d, c["gxs"], 0.015, steps)
        worst = max(worst, worst_err(gb, ga, p))
    gpp = np.abs(ga[2] * p)
    print(f"(L, steps) = ({L}, {steps}): worst scaled error (a) vs (b) {worst:.2e}; |gp p| row maxima {gpp.max(axis=1).min():.3g} .. {gpp.max():.3g}")
    assert worst <= 1e-13


@pytest.mark.parametrize("steps", [1, 3])
def test_fixed_step_descent_on_the_disturbance_row_converges(steps):
    """B = 16 at rest at identity attitude, own mass known to the fit, L = 1, loss = sum (x1[7:13] - x1_logged[7:13])^2:
    d <- d - grad / (2 T^2) from d = 0.  x1[7:13] is d T + O(T^2) in d, so the step is the Gauss-Newton one up to O(T)."""
    rng = np.random.default_rng(5)
    B, T = 16, 0.015
    p = np.tile(NOMINAL, (B, 1)); p[:, 1] *= rng.uniform(0.8, 1.25, B)
    x0 = np.zeros((B, 13)); x0[:, 0:3] = rng.uniform(-1, 1, (B, 3)); x0[:, 3] = 1.0
    u = np.tile(hover(p)[:, None, None], (1, 1, 4))
    d_true = dc.random_dist(rng, B, 2.0, 5.0)
    logged = rollout(x0, u, p, d_true, T, steps)[:, 1]
    d = np.zeros((B, 6))
    course = []
    for _ in range(8):
        x1 = rollout(x0, u, p, d, T, steps)[:, 1]
        gxs = np.zeros((B, 2, 13)); gxs[:, 1, 7:13] = 2 * (x1[:, 7:13] - logged[:, 7:13])
        gd = ref_vjp_rev(x0, u, p, d, gxs, T, steps)[3]
        d = d - gd / (2 * T * T)
        course.append(np.abs(d - d_true).max())
    print(f"steps = {steps}: worst |d - d_true| per iteration " + " ".join(f"{e:.1e}" for e in course))
    assert course[-1] < 1e-12


# ---- the host-compiled reverse step under the host sanitizers ---------------------------------------------------------------
def test_sim_vjp_check_runs_clean_under_the_host_sanitizers(tmp_path):
    cases = []
    for (L, steps), rows in zip(((1, 1), (2, 3), (7, 1), (20, 3)), ("none", "p", "pd", "pd")):
        c, g = reference(11, 8, L, steps, rows)
        p, d = rows_of(c, rows)
        xs = rollout(c["x0"], c["u"], p, d, 0.015, steps)
        kind = {"none": 0, "p": 1, "pd": 2}[rows]
        for i in range(3):
            parts = [p[i], d[i], xs[i], c["u"][i], c["gxs"][i], g[0][i], g[1][i], g[2][i], g[3][i]]
            cases.append(f"{L} {steps} {kind} 0.015\n" + "\n".join(" ".join(repr(float(v)) for v in np.ravel(a)) for a in parts))
    path = tmp_path / "cases.txt"
    path.write_text(f"{len(cases)}\n" + "\n".join(cases) + "\n")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "crazyflie_nmpc_amd", "csrc"), "-s", "sim_vjp_check", f"OBJDIR={tmp_path}",
                        f"CASES={path}"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and f"sim_vjp_check ok: {len(cases)} cases" in r.stdout and "runtime error" not in r.stderr
