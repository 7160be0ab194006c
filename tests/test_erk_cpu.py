"""CPU checks of the ERK sub-step and cost-scaling options (include/cfnmpc.h: cfnmpc_set_erk_steps / cfnmpc_set_cost_scaling;
DESIGN.md section 5.12): the new entry points are declared, exported and bound, the ABI is unchanged, the M > 1 kernels are in
the built code within their resource ceilings, and the chained reference the GPU tests compare against is right.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGS = {
    "cfnmpc_set_erk_steps": "intcfnmpc_set_erk_steps(cfnmpc_solver*s,intnum_steps);",
    "cfnmpc_erk_steps": "intcfnmpc_erk_steps(constcfnmpc_solver*s);",
    "cfnmpc_set_cost_scaling": "intcfnmpc_set_cost_scaling(cfnmpc_solver*s,doublestage_scale,doubleterminal_scale);",
    "cfnmpc_fleet_set_erk_steps": "intcfnmpc_fleet_set_erk_steps(cfnmpc_fleet*f,intnum_steps);",
    "cfnmpc_fleet_set_cost_scaling": "intcfnmpc_fleet_set_cost_scaling(cfnmpc_fleet*f,doublestage_scale,doubleterminal_scale);",
    "cfnmpc_multi_set_erk_steps": "intcfnmpc_multi_set_erk_steps(cfnmpc_multi*m,intnum_steps);",
    "cfnmpc_multi_set_cost_scaling": "intcfnmpc_multi_set_cost_scaling(cfnmpc_multi*m,doublestage_scale,doubleterminal_scale);",
}
ARGTYPES = {
    "cfnmpc_set_erk_steps": [ctypes.c_void_p, ctypes.c_int],
    "cfnmpc_erk_steps": [ctypes.c_void_p],
    "cfnmpc_set_cost_scaling": [ctypes.c_void_p, ctypes.c_double, ctypes.c_double],
    "cfnmpc_fleet_set_erk_steps": [ctypes.c_void_p, ctypes.c_int],
    "cfnmpc_fleet_set_cost_scaling": [ctypes.c_void_p, ctypes.c_double, ctypes.c_double],
    "cfnmpc_multi_set_erk_steps": [ctypes.c_void_p, ctypes.c_int],
    "cfnmpc_multi_set_cost_scaling": [ctypes.c_void_p, ctypes.c_double, ctypes.c_double],
}
ERK_KERNELS = ("k_linearise_erk", "k_forward_erk", "k_forward_p1_erk", "k_forward_p2_erk", "k_cforward_erk")


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


def test_abi_unchanged():
    from crazyflie_nmpc_amd import _lib
    L = _lib.lib()
    assert L.cfnmpc_abi_version() == 9
    assert L.cfnmpc_opts_size() == ctypes.sizeof(_lib.Opts)
    assert "#defineCFNMPC_ABI_VERSION9" in _header()
    assert "#defineCFNMPC_ERK_STEPS_MAX8" in _header()


def test_python_methods_and_defaults():
    import inspect
    from crazyflie_nmpc_amd import BatchSolver
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.parallel import MultiGpuFleet
    for cls in (BatchSolver, MixedHorizonFleet, MultiGpuFleet):
        assert callable(getattr(cls, "set_erk_steps"))
        sig = inspect.signature(cls.set_cost_scaling)
        assert (sig.parameters["stage"].default, sig.parameters["terminal"].default) == (1.0, 1.0)
    assert isinstance(BatchSolver.erk_steps, property)


def test_dropin_exports_solver_opts_set():
    so = os.path.join(ROOT, "crazyflie_nmpc_amd", "libacados_solver_crazyflie.so")
    L = ctypes.CDLL(so)
    assert hasattr(L, "ocp_nlp_solver_opts_set")
    h = open(os.path.join(ROOT, "include", "acados_solver_crazyflie.h")).read()
    h = re.sub(r"\s+", "", re.sub(r"/\*.*?\*/", "", h, flags=re.S))
    assert "voidocp_nlp_solver_opts_set(ocp_nlp_config*config,void*opts_,constchar*field,void*value);" in h


def test_erk_kernels_resources(table):
    for k in ERK_KERNELS:
        assert k in table, sorted(table)
        r = table[k]
        assert r["unit"] == "cfnmpc_kernels", r
        assert r["occupancy"] >= 1 and r["vgpr"] <= 256 and not r.get("dynamic_stack"), (k, r)
    assert table["k_linearise_erk"]["lds"] <= 40192            # the same tiles as k_linearise: four workgroups per CU
    assert table["k_linearise_erk"]["scratch"] <= 96, table["k_linearise_erk"]   # (72 B: DESIGN.md section 5.12)
    for k in ERK_KERNELS[1:]:
        assert table[k]["scratch"] == 0 and table[k]["vgpr_spill"] == 0, (k, table[k])
        assert table[k]["lds"] <= 13568, (k, table[k])
    # the one-step kernels keep their figures (M = 1 runs the code of the parent)
    assert table["k_linearise"]["scratch"] == 0 and table["k_forward"]["scratch"] == 0


def _chain(cref, x, u, dt, M):
    """M RK4 sensitivity steps of dt / M chained: Phi, A = A_M..A_1, B = sum_j A_M..A_{j+1} B_j"""
    A = np.eye(13)
    Bm = np.zeros((13, 4))
    xs = np.asarray(x, dtype=np.float64)
    for _ in range(M):
        xs, Aj, Bj = cref.rk4_sens(xs, u, dt / M)
        A = Aj @ A
        Bm = Aj @ Bm + Bj
    return xs, A, Bm


@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_chained_reference(cref, oracle, M):
    rng = np.random.default_rng(11 + M)
    dt = 0.015
    for _ in range(3):
        x = oracle.sample_hover_x0(rng, 1, scale=1.5)[0]
        x[10:13] += rng.normal(0, 2.0, 3)
        u = oracle.HOV_W + rng.normal(0, 3.0, 4)
        phi, A, Bm = _chain(cref, x, u, dt, M)
        assert np.abs(phi - oracle.rk4(x, u, dt, steps=M)).max() < 1e-12
        # central differences of oracle.rk4(steps=M) (step 1e-5: truncation and rounding errors both near 1e-11)
        eps = 1e-5
        Afd = np.empty((13, 13))
        Bfd = np.empty((13, 4))
        for c in range(13):
            e = np.zeros(13); e[c] = eps
            Afd[:, c] = (oracle.rk4(x + e, u, dt, steps=M) - oracle.rk4(x - e, u, dt, steps=M)) / (2 * eps)
        for c in range(4):
            e = np.zeros(4); e[c] = eps
            Bfd[:, c] = (oracle.rk4(x, u + e, dt, steps=M) - oracle.rk4(x, u - e, dt, steps=M)) / (2 * eps)
        assert np.abs(A - Afd).max() < 1e-9, np.abs(A - Afd).max()
        assert np.abs(Bm - Bfd).max() < 1e-9, np.abs(Bm - Bfd).max()
