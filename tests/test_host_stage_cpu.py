"""CPU check of the array tables of the solver-less batched calls (csrc/cfnmpc_stage.hpp): builds the
stand-alone program tools/host_stage_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer (make host_stage_check) and
runs it.  The program is plain C++ with its own main; nothing of it is loaded into Python.  No GPU needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_stage_check_runs_clean_under_the_host_sanitizers(tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "crazyflie_nmpc_amd", "csrc"), "-s", "host_stage_check", f"OBJDIR={tmp_path}"],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "host_stage_check ok" in r.stdout and "runtime error" not in r.stderr
