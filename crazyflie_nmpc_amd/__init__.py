"""crazyflie_nmpc_amd -- MI355X-native batched solve engine for the Crazyflie SQP-RTI hot path.

The product is `libcfnmpc.so` (hand-written HIP for gfx950 behind a C-ABI, include/cfnmpc.h and
include/acados_solver_crazyflie.h).  This package is the thin Python host side used by the
tests and bench.py: a ctypes binding (`_lib`), a batch solver object (`solver.BatchSolver`)
and a ROS-free mirror of the reference node's per-step protocol (`node`).
There is no CPU fallback: importing `_lib` fails loudly if the HIP library is missing.
"""
from .solver import DIST_NAMES, NOMINAL_PARAMS, PARAM_NAMES, BatchSolver, Opts, default_opts, ekf_aug_cov, ekf_aug_step, ekf_step, estimate, estimate_disturbance, hover_speed, sim, sim_rollout, sim_rollout_vjp  # noqa: F401

__all__ = ["BatchSolver", "Opts", "default_opts", "estimate", "sim", "NOMINAL_PARAMS", "PARAM_NAMES", "hover_speed", "DIST_NAMES",
           "estimate_disturbance", "sim_rollout", "sim_rollout_vjp", "ekf_step", "ekf_aug_step", "ekf_aug_cov"]
