"""CPU checks of the device-side polynomial trajectory references (include/cfnmpc.h: cfnmpc_set_poly_library,
cfnmpc_set_poly_assignment, cfnmpc_set_yref_poly, cfnmpc_eval_poly, cfnmpc_get_yref): the numpy twin
crazyflie_nmpc_amd.trajectories.poly_rows -- what the GPU tests compare the kernel with -- against the reference's own
evaluator (tests/golden/poly.npz), against the model's identities, under placement, in the guard case and in closed loop on the
CPU restatement; the new entry points are declared, exported and bound; the new kernel is in the built code without scratch
while the default-step kernels keep the parent's figures.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from crazyflie_nmpc_amd import trajectories as tj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "poly.npz"))
NAMES = ("figure8", "takeoff", "figure8_takeoff_landing")
NOM = tj._NOMINAL_PARAMS
DT = 0.015


def gold_flat(name):
    g = GOLD
    return np.concatenate([g[name + "_pos"], g[name + "_vel"], g[name + "_acc"], g[name + "_yaw"][:, None], g[name + "_omega"]], 1)


def rows_at(tab, times, flags=0, place=None, params=None):
    """twin rows of ONE vehicle at arbitrary times (one call per time) -> (flat [m][13], rows [m][17])"""
    fl, rw = [], []
    for t in times:
        f, r = tj.poly_rows([tab], [0], place, float(t), 1, DT, flags, params)
        fl.append(f[0, 0]); rw.append(r[0, 0])
    return np.array(fl), np.array(rw)


def rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


# ---- 1. twin against the reference's evaluator -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_twin_against_golden(name):
    par = NOM.copy(); par[0] = 9.81               # the evaluator's gravity constant
    tab, t = GOLD[name + "_table"], GOLD[name + "_t"]
    gold = gold_flat(name)
    flat, rows = rows_at(tab, t, params=par[None])
    err = np.abs(flat - gold) / np.maximum(1.0, np.abs(gold))
    print(f"{name}: {len(t)} times, max error {err.max():.2e}")
    assert err.max() <= 1e-12
    assert np.isfinite(rows).all()
    # the grid in one call is the same evaluation
    ng = int(GOLD[name + "_grid"])
    f2, _ = tj.poly_rows([tab], [0], None, 0.0, ng, DT, 0, par[None])
    assert np.array_equal(f2[0], flat[:ng])


# ---- 2. model identities -----------------------------------------------------------------------------------------------------
def _bodies(flat, g0):
    """x_b, y_b, z_b of the flatness relations from flat rows, in plain numpy (independent of the twin's own expressions)"""
    acc, yaw = flat[:, 6:9], flat[:, 9]
    thr = acc + np.array([0, 0, g0])
    zb = thr / np.linalg.norm(thr, axis=1)[:, None]
    xw = np.stack([np.cos(yaw), np.sin(yaw), 0 * yaw], 1)
    yb = np.cross(zb, xw); yb /= np.linalg.norm(yb, axis=1)[:, None]
    return np.cross(yb, zb), yb, zb


@pytest.mark.parametrize("name", ["figure8", "figure8_takeoff_landing"])
def test_model_identities(oracle, name):
    tab = GOLD[name + "_table"]
    D = tab[:, 0].sum()
    t = np.random.default_rng(5).uniform(1e-4, D - 1e-4, 500)
    edges = np.cumsum(tab[:, 0])[:-1]
    t = t[np.abs(t[:, None] - edges[None]).min(1) > 3e-5]          # (the central difference must not straddle a piece boundary)
    flat, rows = rows_at(tab, t)
    h = 1e-5
    _f, rp = rows_at(tab, t + h)
    _f, rm = rows_at(tab, t - h)
    qdot_fd = (rp[:, 3:7] - rm[:, 3:7]) / (2 * h)
    xb, yb, zb = _bodies(flat, NOM[0])
    e_vel = e_acc = e_R = e_qd = e_qd_eval = 0.0
    for i in range(len(t)):
        row = rows[i]
        f = oracle.f_expl(row[:13], row[13:])
        R = rot(row[3:7])
        vb, om = row[7:10], row[10:13]
        e_vel = max(e_vel, np.abs(f[0:3] - flat[i, 3:6]).max())
        e_acc = max(e_acc, np.abs(R @ (f[7:10] + np.cross(om, vb)) - flat[i, 6:9]).max())
        e_R = max(e_R, np.abs(R - np.stack([xb[i], yb[i], zb[i]], 1)).max())
        e_qd = max(e_qd, np.abs(f[3:7] - qdot_fd[i]).max())
        row_e = row.copy(); row_e[12] = flat[i, 12]                # the evaluator's omega_z = z_b[2] dyaw
        e_qd_eval = max(e_qd_eval, np.abs(oracle.f_expl(row_e[:13], row_e[13:])[3:7] - qdot_fd[i]).max())
    print(f"{name}: {len(t)} times: vel {e_vel:.1e}, acc {e_acc:.1e}, R(q) {e_R:.1e}, qdot {e_qd:.1e}, qdot with the evaluator's omega_z {e_qd_eval:.1e}")
    assert e_vel <= 1e-13 and e_acc <= 1e-12 and e_R <= 1e-14 and e_qd <= 1e-8
    assert not e_qd_eval <= 1e-8, "the evaluator's omega_z is an approximation: the rows must use the exact rate"


# ---- 3. placement --------------------------------------------------------------------------------------------------------------
def _transform(rows, off, yaw0, ts):
    """unplaced rows -> placed rows by hand: positions rotated and shifted, attitude qz(yaw0) q, rates / ts, body velocity / ts"""
    out = rows.copy()
    c, s = np.cos(yaw0), np.sin(yaw0)
    out[:, 0] = c * rows[:, 0] - s * rows[:, 1] + off[0]
    out[:, 1] = s * rows[:, 0] + c * rows[:, 1] + off[1]
    out[:, 2] = rows[:, 2] + off[2]
    ch, sh = np.cos(yaw0 / 2), np.sin(yaw0 / 2)
    w, x, y, z = rows[:, 3], rows[:, 4], rows[:, 5], rows[:, 6]
    out[:, 3:7] = np.stack([ch * w - sh * z, ch * x - sh * y, ch * y + sh * x, ch * z + sh * w], 1)
    return out


def test_placement():
    tab = GOLD["figure8_table"]
    N = 40
    # time scale 1: a rotation about z and a shift leave body velocity, rates and speeds alone
    off, yaw0, t0 = (0.7, -1.2, 0.5), 2.3, 1.25
    _f, base = tj.poly_rows([tab], [0], None, 0.6, N, DT)
    _f, placed = tj.poly_rows([tab], [0], [[t0, 1.0, *off, yaw0]], 0.6 + t0, N, DT)
    err = np.abs(placed[0] - _transform(base[0], off, yaw0, 1.0)).max()
    print(f"placement (shift, rotation, start): {err:.1e}")
    assert err <= 1e-12
    # time scale 2: the path at half speed -- positions of tau = t / 2, velocities halved
    f1, _r = tj.poly_rows([tab], [0], None, 0.3, N, DT / 2)
    f2, _r = tj.poly_rows([tab], [0], [[0.0, 2.0, 0, 0, 0, 0]], 0.6, N, DT)
    assert np.abs(f2[0, :, 0:3] - f1[0, :, 0:3]).max() <= 1e-12
    assert np.abs(f2[0, :, 3:6] - f1[0, :, 3:6] / 2).max() <= 1e-12
    assert np.abs(f2[0, :, 6:9] - f1[0, :, 6:9] / 4).max() <= 1e-12
    # before the start and behind the end: held rows
    D = tab[:, 0].sum()
    hov = np.sqrt(NOM[1] * NOM[0] / (4 * NOM[6]))
    fb, rb = tj.poly_rows([tab], [0], [[10.0, 1.0, 1, 2, 3, 0.5]], 0.0, 4, DT)
    start = np.array([tab[0, 1], tab[0, 9], tab[0, 17]])
    c, s = np.cos(0.5), np.sin(0.5)
    want = np.array([c * start[0] - s * start[1] + 1, s * start[0] + c * start[1] + 2, start[2] + 3])
    assert np.abs(rb[0, :, 0:3] - want).max() <= 1e-15
    assert np.abs(rb[0, :, 3:7] - [np.cos(0.25), 0, 0, np.sin(0.25)]).max() <= 1e-15
    assert (rb[0, :, 7:13] == 0).all() and np.abs(rb[0, :, 13:] - hov).max() <= 1e-15 and (fb[0, :, 3:9] == 0).all()
    fe, re_ = tj.poly_rows([tab], [0], None, D + 1.0, 3, DT)
    last = tab[-1]
    end = [tj._horner(last[1 + 8 * a:9 + 8 * a], np.float64(last[0])) for a in range(3)]
    assert np.abs(re_[0, :, 0:3] - end).max() <= 1e-15 and (re_[0, :, 7:13] == 0).all()
    # LOOP over three periods: stage k is the row at the wrapped time tau - D floor(tau / D), accumulated D, bit for bit
    Dacc = 0.0
    for d in tab[:, 0]:
        Dacc = Dacc + d
    dtl = 0.11
    _f, rl = tj.poly_rows([tab], [0], None, 0.25, 200, dtl, tj.POLY_LOOP)
    tau = 0.25 + np.arange(200) * dtl
    assert tau[-1] > 3 * Dacc
    wrapped = np.where(tau >= Dacc, tau - Dacc * np.floor(tau / Dacc), tau)
    _f, ru = rows_at(tab, wrapped)
    assert np.array_equal(rl[0], ru)
    # a single-piece trajectory, B = 1, and a vehicle without a trajectory
    one = tab[3:4]
    f, r = tj.poly_rows([one], [0], None, 0.1, 5, DT)
    assert f.shape == (1, 5, 13) and r.shape == (1, 5, 17) and np.isfinite(r).all()
    f, r = tj.poly_rows([tab, one], [-1, 1, 0], None, 0.1, 5, DT)
    assert np.isnan(r[0]).all() and np.isnan(f[0]).all() and np.isfinite(r[1:]).all()


# ---- 4. guard ------------------------------------------------------------------------------------------------------------------
def free_fall_table():
    row = np.zeros(33)
    row[0] = 1.0
    row[17 + 2] = -0.5 * 9.8066          # z = -1/2 g0 t^2: thr = 0
    row[25] = 0.3; row[26] = 0.2         # yaw = 0.3 + 0.2 t
    row[1 + 1] = 0.4                     # x = 0.4 t
    return row[None]


def test_guard_free_fall():
    tab = free_fall_table()
    flat, rows = tj.poly_rows([tab], [0], None, 0.0, 60, DT)
    assert np.isfinite(rows).all() and np.isfinite(flat).all()
    hov = np.sqrt(NOM[1] * NOM[0] / (4 * NOM[6]))
    yaw = flat[0, :, 9]
    assert np.abs(rows[0, :, 3] - np.cos(yaw / 2)).max() <= 1e-15 and np.abs(rows[0, :, 6] - np.sin(yaw / 2)).max() <= 1e-15
    assert (rows[0, :, 4:6] == 0).all() and (rows[0, :, 10:12] == 0).all()
    assert np.abs(rows[0, :, 12] - 0.2).max() <= 1e-15 and np.abs(rows[0, :, 13:] - hov).max() <= 1e-15
    vel = flat[0, :, 3:6]
    vb = np.stack([np.cos(yaw) * vel[:, 0] + np.sin(yaw) * vel[:, 1], -np.sin(yaw) * vel[:, 0] + np.cos(yaw) * vel[:, 1], vel[:, 2]], 1)
    assert np.abs(rows[0, :, 7:10] - vb).max() <= 1e-15


# ---- 5. closed loop on the restatement -----------------------------------------------------------------------------------------
def test_closed_loop_consistent_beats_kinematic(cref):
    tab = GOLD["figure8_table"]
    N, steps = 50, 200
    place = [[0.0, 1.0, 0.0, 0.0, 0.5, 0.0]]
    opts = cref.default_opts(N=N)
    rms = {}
    for name, flags in (("consistent", 0), ("kinematic", tj.POLY_KINEMATIC)):
        _f, r0 = tj.poly_rows([tab], [0], place, 0.0, 1, DT, flags)
        x = r0[:, 0, :13].copy()
        xit = np.repeat(x[:, None, :], N + 1, 1).copy()
        uit = np.repeat(r0[:, :1, 13:], N, 1).copy()
        err = []
        for k in range(steps):
            flat, rows = tj.poly_rows([tab], [0], place, k * DT, N + 1, DT, flags)
            cref.rti_step(opts, xit, uit, x.copy(), np.ascontiguousarray(rows[:, :N]), np.ascontiguousarray(rows[:, N, :13]), nthreads=1)
            err.append(np.linalg.norm(x[0, :3] - flat[0, 0, :3]))
            x = cref.sim(x, uit[:, 0].copy(), T=DT, steps=1)
        e = np.array(err[60:])
        rms[name] = float(np.sqrt((e ** 2).mean()))
        print(f"{name}: RMS position error {1e3 * rms[name]:.3f} mm, maximum {1e3 * e.max():.3f} mm")
    assert rms["consistent"] <= 0.25 * rms["kinematic"]


# ---- 6. surface and resources --------------------------------------------------------------------------------------------------
vp, i32, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
SIGS = {
    "cfnmpc_set_poly_library": "intcfnmpc_set_poly_library(cfnmpc_solver*s,constdouble*pieces,constint*first,intn_traj,void*stream);",
    "cfnmpc_set_poly_assignment": "intcfnmpc_set_poly_assignment(cfnmpc_solver*s,constint*traj,constdouble*place,inton_device,void*stream);",
    "cfnmpc_set_yref_poly": "intcfnmpc_set_yref_poly(cfnmpc_solver*s,doublet,intflags,void*stream);",
    "cfnmpc_eval_poly": "intcfnmpc_eval_poly(cfnmpc_solver*s,doublet,intn_stages,intflags,double*flat,double*rows,inton_device,void*stream);",
    "cfnmpc_get_yref": "intcfnmpc_get_yref(cfnmpc_solver*s,double*yref,double*yref_e,inton_device,void*stream);",
    "cfnmpc_fleet_set_poly_library": "intcfnmpc_fleet_set_poly_library(cfnmpc_fleet*f,constdouble*pieces,constint*first,intn_traj,void*stream);",
    "cfnmpc_fleet_set_poly_assignment": "intcfnmpc_fleet_set_poly_assignment(cfnmpc_fleet*f,constint*traj,constdouble*place,inton_device,void*stream);",
    "cfnmpc_fleet_set_yref_poly": "intcfnmpc_fleet_set_yref_poly(cfnmpc_fleet*f,doublet,intflags,void*stream);",
    "cfnmpc_fleet_eval_poly": "intcfnmpc_fleet_eval_poly(cfnmpc_fleet*f,doublet,intflags,double*flat,double*rows,inton_device,void*stream);",
    "cfnmpc_multi_set_poly_library": "intcfnmpc_multi_set_poly_library(cfnmpc_multi*m,constdouble*pieces,constint*first,intn_traj);",
    "cfnmpc_multi_set_poly_assignment": "intcfnmpc_multi_set_poly_assignment(cfnmpc_multi*m,constint*traj,constdouble*place);",
    "cfnmpc_multi_set_yref_poly": "intcfnmpc_multi_set_yref_poly(cfnmpc_multi*m,doublet,intflags);",
}
ARGTYPES = {
    "cfnmpc_set_poly_library": [vp, vp, vp, i32, vp], "cfnmpc_set_poly_assignment": [vp, vp, vp, i32, vp],
    "cfnmpc_set_yref_poly": [vp, dbl, i32, vp], "cfnmpc_eval_poly": [vp, dbl, i32, i32, vp, vp, i32, vp],
    "cfnmpc_get_yref": [vp, vp, vp, i32, vp],
    "cfnmpc_fleet_set_poly_library": [vp, vp, vp, i32, vp], "cfnmpc_fleet_set_poly_assignment": [vp, vp, vp, i32, vp],
    "cfnmpc_fleet_set_yref_poly": [vp, dbl, i32, vp], "cfnmpc_fleet_eval_poly": [vp, dbl, i32, vp, vp, i32, vp],
    "cfnmpc_multi_set_poly_library": [vp, vp, vp, i32], "cfnmpc_multi_set_poly_assignment": [vp, vp, vp],
    "cfnmpc_multi_set_yref_poly": [vp, dbl, i32],
}
# figures of the default-step kernels on the parent commit (vgpr, agpr, scratch, lds): the table of tests/test_uncertainty_cpu.py
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


@pytest.fixture(scope="module")
def table():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cfn_resource_poly", os.path.join(ROOT, "tools", "resource.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    try:
        return mod.resource_table()
    except FileNotFoundError:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crazyflie_nmpc_amd", "csrc"), "-s", "ARCH=gfx950"])
        return mod.resource_table()


def test_entry_points_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "cfnmpc.h")).read()
    src = re.sub(r"\s+", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    from crazyflie_nmpc_amd import _lib
    L = _lib.lib()
    for name, sig in SIGS.items():
        assert sig in src, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == ARGTYPES[name], name
    for d in ("CFNMPC_POLY_NC33", "CFNMPC_NPLACE6", "CFNMPC_NFLAT13", "CFNMPC_POLY_LOOP1", "CFNMPC_POLY_KINEMATIC2"):
        assert "#define" + d in src, d
    assert L.cfnmpc_abi_version() == 9 == _lib.ABI_VERSION


def test_python_surface():
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.parallel import MultiGpuFleet
    from crazyflie_nmpc_amd.solver import BatchSolver
    for cls in (BatchSolver, MixedHorizonFleet, MultiGpuFleet):
        for m in ("set_poly_library", "set_poly_assignment", "set_yref_poly"):
            assert callable(getattr(cls, m)), (cls, m)
    for cls in (BatchSolver, MixedHorizonFleet):
        assert callable(cls.eval_poly), cls
    assert callable(BatchSolver.yref)


def test_poly_kernel_resources(table):
    r = table["k_poly_rows"]                      # the kernel of the control step: no scratch, no spills of either kind
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["occupancy"] >= 2, r
    r = table["k_poly_eval"]                      # its read-out twin: nothing in memory (two scalars are parked in vector lanes)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["occupancy"] >= 2, r
    assert table["k_poly_clamp_ids"]["scratch"] == 0


def test_default_kernels_keep_parent_figures(table):
    for k, (v, a, sc, lds) in PARENT.items():
        r = table[k]
        assert (r["vgpr"], r["agpr"], r["scratch"], r["lds"]) == (v, a, sc, lds), (k, r)
