"""Register / scratch budgets of the uniform-reference twins of the start solve's factorisation (k_factor_u, k_factor_wu; DESIGN.md
section 5.3), enforced on the code that was built -- the figures tools/resource.py reads from crazyflie_nmpc_amd/csrc/build/<unit>.res,
as tests/test_resource_budget.py does for the generic kernels.  The twins hold two reference values per lane over the whole sweep where
the generic kernels hold two per prefetched stage: they must stay at two waves per SIMD without touching scratch."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWINS = {"k_factor_u": "k_factor", "k_factor_wu": "k_factor_w"}


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


@pytest.mark.parametrize("twin", sorted(TWINS))
def test_twin_budget(table, twin):
    e, g = table[twin], table[TWINS[twin]]
    assert e["vgpr"] <= 256 and e["agpr"] <= g["agpr"] and e["scratch"] == 0 and e["occupancy"] >= 2, (twin, e, g)
    assert e["vgpr_spill"] == 0 and e["lds"] <= g["lds"], (twin, e, g)


def test_generic_kernels_keep_their_budget(table):
    for k in TWINS.values():
        e = table[k]
        assert e["vgpr"] <= 256 and e["scratch"] == 0 and e["occupancy"] >= 2, (k, e)
