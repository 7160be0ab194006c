"""CPU checks of the full SQP solve (include/cfnmpc.h: cfnmpc_solve_sqp): its convergence-check kernel
is in the built code without scratch, and the new entry points are declared, exported and bound.  No GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cfnmpc_solve_sqp", "cfnmpc_get_sqp_stats", "cfnmpc_fleet_solve_sqp", "cfnmpc_fleet_get_sqp_stats"]


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


def test_sqp_check_kernel_has_no_scratch(table):
    assert "k_sqp_check" in table, sorted(table)
    r = table["k_sqp_check"]
    assert r["unit"] == "cfnmpc_kernels"          # (the set of device units stays at four)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    assert r["occupancy"] >= 1, r
    assert r["vgpr"] <= 256 and r["lds"] <= 16384, r


def _header():
    src = open(os.path.join(ROOT, "include", "cfnmpc.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_sqp_entry_points_declared_exported_and_bound():
    src = _header()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
    from crazyflie_nmpc_amd import _lib
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name   # bound with argument types, not called blind
    assert L.cfnmpc_abi_version() == 9                       # new entry points only: cfnmpc_opts and old signatures unchanged


def test_sqp_signatures():
    src = re.sub(r"\s+", "", _header())   # (comments already stripped)
    assert ("intcfnmpc_solve_sqp(cfnmpc_solver*s,intmax_iter,doubletol_step,doubletol_eq,doubletol_ineq,int*n_iter,"
            "void*stream);") in src
    assert "intcfnmpc_get_sqp_stats(cfnmpc_solver*s,int*status,int*sqp_iter,double*res,inton_device,void*stream);" in src


def test_python_wrappers_exist():
    from crazyflie_nmpc_amd import BatchSolver
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    import inspect
    sig = inspect.signature(BatchSolver.solve_sqp)
    assert [sig.parameters[k].default for k in ("max_iter", "tol_step", "tol_eq", "tol_ineq")] == [100, 1e-6, 1e-6, 1e-6]
    for cls in (BatchSolver, MixedHorizonFleet):
        assert callable(getattr(cls, "solve_sqp")) and callable(getattr(cls, "sqp_stats"))
