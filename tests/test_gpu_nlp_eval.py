"""GPU suite: NLP cost, KKT residuals, costates and reduced gradient at the current iterate (include/cfnmpc.h: cfnmpc_eval_nlp;
DESIGN.md section 5.16).

The reference is nlp_ref (tests/test_nlp_eval_cpu.py: explicit A_k, B_k by complex-step Jacobians through the RK4 stages,
refereed there by finite differences of the single-shooting objective) run on the iterate read back with get_iterate and on
the same data.  Tolerance: the project pins the GPU's A, B, b against the oracle at 1e-12 (test_gpu_parity.py); carried through
13 entries x (N + 1) stages that is 6.6e-10 relative at N = 50, so 1e-9 * max(1, |ref|_inf) per array for pi, gu and res, and
1e-12 relative for the cost; at N = 100 the same product gives 1.3e-9.  Every comparison prints the figure it saw."""
import ctypes as C

import numpy as np
import pytest

from test_model_params_cpu import random_params
from test_nlp_eval_cpu import nlp_ref_rows

pytestmark = pytest.mark.gpu
DT = 0.015
EINVAL = -1


def _tol(N):
    return 1e-9 if N <= 50 else 13 * (N + 1) * 1e-12


def _inputs(oracle, B, N, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    x0 = oracle.sample_hover_x0(rng, B, scale=scale)
    yr, ye = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    return x0, np.repeat(yr[None], B, 0).copy(), np.repeat(ye[None], B, 0).copy()


def _solver(B, x0, yref, yref_e, **kw):
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    s = BatchSolver(B, default_opts(**kw))
    s.set_x0(x0); s.set_yref(yref, yref_e); s.init_iterate(INIT_HOVER)
    return s


def _compare(s, oracle, x0, yref, yref_e, what, Qd=None, Rd=None, QNd=None, lb=0.0, ub=22.0, M=1, params=None, keep=True):
    """eval_nlp on the solver's current iterate against nlp_ref on the iterate read back; -> (cost, res, pi, gu) of the GPU"""
    N = s.N
    Qd = oracle.Q_DIAG if Qd is None else Qd
    Rd = oracle.R_DIAG if Rd is None else Rd
    QNd = oracle.QN_DIAG if QNd is None else QNd
    s.eval_nlp(keep_multipliers=keep)
    cost, res = s.nlp_stats()
    x, u = s.get_iterate()
    cr, rr, pr, gr = nlp_ref_rows(x, u, x0, yref, yref_e, Qd, Rd, QNd, lb, ub, DT, M, params)
    tol = _tol(N)
    e_cost = np.abs(cost - cr) / np.abs(cr)
    e_res = np.abs(res - rr).max() / max(1.0, np.abs(rr).max())
    line = f"{what}: B {s.B} N {N}  cost rel {e_cost.max():.2e}  res {e_res:.2e} (|res| {np.abs(rr).max(0)})"
    pi = gu = None
    if keep:
        pi, gu = s.nlp_multipliers()
        e_pi = np.abs(pi - pr).max() / max(1.0, np.abs(pr).max())
        e_gu = np.abs(gu - gr).max() / max(1.0, np.abs(gr).max())
        line += f"  pi {e_pi:.2e} (|pi| {np.abs(pr).max():.2e})  gu {e_gu:.2e} (|gu| {np.abs(gr).max():.2e})"
    print(line)
    assert np.isfinite(cost).all() and np.isfinite(res).all()
    assert e_cost.max() <= 1e-12, e_cost.max()
    assert e_res <= tol, e_res
    if keep:
        assert e_pi <= tol and e_gu <= tol, (e_pi, e_gu)
    return cost, res, pi, gu


# ---- 1. parity with the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("B", [192, 1, 63, 65, 130])
def test_parity_with_reference(oracle, B, scale):
    N = 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=31 + B, scale=scale)
    s = _solver(B, x0, yref, yref_e)
    # no solve yet: the hover iterate (x_k = x0, u_k = hover): defects and gradients are large, nothing on the box
    _compare(s, oracle, x0, yref, yref_e, f"hover start, scale {scale}")
    s.solve(1)
    c, r, pi, gu = _compare(s, oracle, x0, yref, yref_e, f"one RTI step, scale {scale}")
    _x, u = s.get_iterate()
    on_box = ((u <= 0.0) | (u >= 22.0)).reshape(B, -1).any(1)
    print(f"  rows with inputs on the box: {on_box.sum()} of {B}")
    if scale == 3.0 and B >= 63:
        assert on_box.sum() >= (3 * B) // 4, on_box.sum()     # the coverage "inputs on the box": most rows saturate at this scale


# ---- 2. each option that changes the NLP ------------------------------------------------------------------------------------------
def test_per_instance_model_parameters(oracle):
    B, N = 130, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=41)
    p = random_params(np.random.default_rng(42), B)
    s = _solver(B, x0, yref, yref_e)
    s.set_model_params(p)
    _compare(s, oracle, x0, yref, yref_e, "model parameters, hover start", params=p)
    s.solve(1)
    _compare(s, oracle, x0, yref, yref_e, "model parameters, one RTI step", params=p)


def test_per_instance_weights_with_cost_scaling(oracle):
    B, N = 130, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=43)
    rng = np.random.default_rng(44)
    W = np.tile(oracle.W_DIAG, (B, 1)) * rng.uniform(0.5, 2.0, (B, 17))
    WN = np.tile(oracle.QN_DIAG, (B, 1)) * rng.uniform(0.5, 2.0, (B, 13))
    s = _solver(B, x0, yref, yref_e)
    s.set_weights_batch(W, WN)
    s.set_cost_scaling(DT, 1.0)
    kw = dict(Qd=DT * W[:, :13], Rd=DT * W[:, 13:], QNd=WN)
    _compare(s, oracle, x0, yref, yref_e, "weight rows x scaling (dt, 1), hover start", **kw)
    s.solve(1)
    _compare(s, oracle, x0, yref, yref_e, "weight rows x scaling (dt, 1), one RTI step", **kw)
    # uniform weights with the same scaling
    s2 = _solver(B, x0, yref, yref_e)
    s2.set_cost_scaling(DT, 1.0)
    s2.solve(1)
    _compare(s2, oracle, x0, yref, yref_e, "uniform weights x scaling (dt, 1)", Qd=DT * oracle.Q_DIAG, Rd=DT * oracle.R_DIAG)


def test_erk_steps_2(oracle):
    B, N = 130, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=45)
    s = _solver(B, x0, yref, yref_e)
    s.set_erk_steps(2)
    _compare(s, oracle, x0, yref, yref_e, "erk_steps 2, hover start", M=2)
    s.solve(1)
    _compare(s, oracle, x0, yref, yref_e, "erk_steps 2, one RTI step", M=2)


def test_erk_steps_3_with_model_parameters(oracle):
    """the sub-step recomputation beyond one extra step, on the _par kernel"""
    B, N = 65, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=46)
    p = random_params(np.random.default_rng(47), B)
    s = _solver(B, x0, yref, yref_e)
    s.set_erk_steps(3); s.set_model_params(p)
    s.solve(1)
    _compare(s, oracle, x0, yref, yref_e, "erk_steps 3 + model parameters", M=3, params=p)


def test_per_stage_boxes_with_pinned_stage_0(oracle):
    B, N = 130, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=48, scale=3.0)
    rng = np.random.default_rng(49)
    lb = rng.uniform(0.0, 6.0, (B, N, 4)); ub = rng.uniform(17.0, 22.0, (B, N, 4))
    lb[:, 0] = ub[:, 0] = oracle.HOV_W + rng.uniform(-1.0, 1.0, (B, 4))          # stage 0 pinned
    s = _solver(B, x0, yref, yref_e)
    s.set_box_stages(lb, ub)
    # the hover iterate violates nothing but sits off the pinned stage: res_ineq > 0 there
    c, r, pi, gu = _compare(s, oracle, x0, yref, yref_e, "stage boxes, hover start", lb=lb, ub=ub)
    assert (r[:, 2] > 0).all()
    s.solve(1)
    c, r, pi, gu = _compare(s, oracle, x0, yref, yref_e, "stage boxes, one RTI step", lb=lb, ub=ub)
    _x, u = s.get_iterate()
    assert np.abs(u[:, 0] - lb[:, 0]).max() <= 1e-9                               # the step honours the pin ...
    # ... and a pinned input adds nothing to res_stat whatever its gradient: res_stat is the largest entry over the other stages
    nat = np.abs(u - np.clip(u - gu, lb, ub))
    assert np.abs(nat[:, 0]).max() <= 1e-9 and np.abs(gu[:, 0]).max() > 1e-3
    assert np.abs(r[:, 0] - nat.reshape(B, -1).max(1)).max() <= 1e-12


# ---- 3. solvers without stored blocks -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(start_solve=2), dict(cond_N2=10)], ids=["start_solve2", "cond_N2_10"])
def test_solvers_without_stored_blocks(oracle, kw):
    B, N = 130, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=51, scale=1.0)
    s = _solver(B, x0, yref, yref_e, **kw)
    _compare(s, oracle, x0, yref, yref_e, f"{kw}, hover start")
    s.solve(1)
    _compare(s, oracle, x0, yref, yref_e, f"{kw}, one RTI step")


# ---- 4. agreement with solve_sqp ------------------------------------------------------------------------------------------------------
def test_agreement_with_solve_sqp(oracle):
    B, N = 64, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=22, scale=1.0)
    s = _solver(B, x0, yref, yref_e, tol=1e-11)
    s.solve_sqp(100, 1e-9, 1e-9, 1e-9)
    st, it, rs = s.sqp_stats()
    s.eval_nlp()
    cost, res = s.nlp_stats()
    conv = st == 0
    print(f"status 0: {conv.sum()} of {B}; res_stat of those: max {res[conv, 0].max() if conv.any() else None:.3e}; "
          f"|res_eq - sqp| {np.abs(res[:, 1] - rs[:, 1]).max():.2e}")
    assert conv.sum() >= 16, np.unique(st, return_counts=True)
    assert np.abs(res[:, 1] - rs[:, 1]).max() <= 1e-12
    assert np.array_equal(res[:, 2], rs[:, 2])
    assert (res[conv, 0] <= 1e-7).all(), res[conv, 0].max()
    # after ONE RTI step from the same start nothing is stationary yet
    s1 = _solver(B, x0, yref, yref_e, tol=1e-11)
    s1.solve(1)
    s1.eval_nlp()
    r1 = s1.nlp_stats()[1]
    print(f"one RTI step: res_stat min {r1[:, 0].min():.3e}")
    assert (r1[:, 0] > 1e-2).all(), r1[:, 0].min()


# ---- 5. evaluation disturbs nothing -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [0, 1])
def test_evaluation_disturbs_nothing(oracle, graph):
    B, N = 192, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=61, scale=3.0)
    out = []
    for with_eval in (False, True):
        s = _solver(B, x0, yref, yref_e, step_graph=graph)
        s.solve(1)
        if with_eval:
            s.eval_nlp(keep_multipliers=True)
            s.eval_nlp()
        s.solve(1)
        if with_eval:
            s.eval_nlp(keep_multipliers=True)
        s.solve(1)
        out.append(s.get_iterate() + s.stats())
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---- 6. getters -----------------------------------------------------------------------------------------------------------------------
def test_getters(oracle):
    import torch
    B, N = 65, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=62)
    s = _solver(B, x0, yref, yref_e)
    L, h, null = s._L, s._h, C.c_void_p(0)
    cost = np.empty(B); res = np.empty((B, 3)); pi = np.empty((B, N + 1, 13)); gu = np.empty((B, N, 4))
    pc, pr, pp, pg = (a.ctypes.data_as(C.c_void_p) for a in (cost, res, pi, gu))
    # before any evaluation
    assert L.cfnmpc_get_nlp_stats(h, pc, pr, 0, null) == EINVAL
    assert L.cfnmpc_get_nlp_multipliers(h, pp, pg, 0, null) == EINVAL
    assert L.cfnmpc_eval_nlp(h, 2, null) == EINVAL
    b0 = s.workspace_bytes
    s.solve(1)
    s.eval_nlp()
    assert s.workspace_bytes == b0                                   # cost and residuals live with the solver
    assert L.cfnmpc_get_nlp_stats(h, pc, pr, 0, null) == 0
    assert L.cfnmpc_get_nlp_stats(h, null, null, 0, null) == EINVAL    # both pointers NULL
    assert L.cfnmpc_get_nlp_multipliers(h, pp, pg, 0, null) == EINVAL  # the last evaluation kept none
    s.eval_nlp(keep_multipliers=True)
    NW = (B + 3) // 4 + 1                                              # workspace blocks of four rows, one spare
    assert s.workspace_bytes - b0 == 8 * (NW * (N + 1) * 52 + NW * N * 16)   # exactly the two buffers
    s.eval_nlp(keep_multipliers=True)
    assert s.workspace_bytes - b0 == 8 * (NW * (N + 1) * 52 + NW * N * 16)
    assert L.cfnmpc_get_nlp_multipliers(h, null, null, 0, null) == EINVAL
    assert L.cfnmpc_get_nlp_multipliers(h, pp, pg, 0, null) == 0
    assert L.cfnmpc_get_nlp_stats(h, pc, pr, 0, null) == 0
    # one pointer at a time
    pi1 = np.empty_like(pi); gu1 = np.empty_like(gu); c1 = np.empty_like(cost); r1 = np.empty_like(res)
    assert L.cfnmpc_get_nlp_multipliers(h, pi1.ctypes.data_as(C.c_void_p), null, 0, null) == 0
    assert L.cfnmpc_get_nlp_multipliers(h, null, gu1.ctypes.data_as(C.c_void_p), 0, null) == 0
    assert L.cfnmpc_get_nlp_stats(h, c1.ctypes.data_as(C.c_void_p), null, 0, null) == 0
    assert L.cfnmpc_get_nlp_stats(h, null, r1.ctypes.data_as(C.c_void_p), 0, null) == 0
    assert np.array_equal(pi1, pi) and np.array_equal(gu1, gu) and np.array_equal(c1, cost) and np.array_equal(r1, res)
    # on_device 1 (device tensors) and 2 (host, enqueued only)
    dc = torch.empty(B, dtype=torch.float64, device="cuda"); dr = torch.empty((B, 3), dtype=torch.float64, device="cuda")
    dp = torch.empty((B, N + 1, 13), dtype=torch.float64, device="cuda"); dg = torch.empty((B, N, 4), dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.cfnmpc_get_nlp_stats(h, C.c_void_p(dc.data_ptr()), C.c_void_p(dr.data_ptr()), 1, st) == 0
    assert L.cfnmpc_get_nlp_multipliers(h, C.c_void_p(dp.data_ptr()), C.c_void_p(dg.data_ptr()), 1, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(dc.cpu().numpy(), cost) and np.array_equal(dr.cpu().numpy(), res)
    assert np.array_equal(dp.cpu().numpy(), pi) and np.array_equal(dg.cpu().numpy(), gu)
    out = s.nlp_stats(out=(torch.empty_like(dc), torch.empty_like(dr)))
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), cost) and np.array_equal(out[1].cpu().numpy(), res)
    c2 = np.full(B, np.nan); r2 = np.full((B, 3), np.nan)
    assert L.cfnmpc_get_nlp_stats(h, c2.ctypes.data_as(C.c_void_p), r2.ctypes.data_as(C.c_void_p), 2, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(c2, cost) and np.array_equal(r2, res)
    p2 = np.full_like(pi, np.nan)
    assert L.cfnmpc_get_nlp_multipliers(h, p2.ctypes.data_as(C.c_void_p), null, 2, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(p2, pi)
    # the getters return the last evaluation's snapshot: a solve in between does not show
    s.solve(1)
    assert np.array_equal(s.nlp_stats()[0], cost)


# ---- 7. fleet and multi-GPU ----------------------------------------------------------------------------------------------------------
def test_fleet_and_multi(oracle):
    from crazyflie_nmpc_amd import default_opts, parallel
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B = 99
    hz = np.array([30, 50, 100])[np.arange(B) % 3]                      # interleaved
    x0, yref, yref_e = _inputs(oracle, B, 100, seed=71, scale=1.0)

    def single(idx, n):
        s = _solver(len(idx), x0[idx].copy(), yref[idx, :n].copy(), yref_e[idx].copy(), N=int(n))
        s.solve(1)
        s.eval_nlp()
        return s.nlp_stats() + s.get_iterate()

    def against_reference(cost, res, idx, n, xg, ug, what):
        cr, rr, _p, _g = nlp_ref_rows(xg, ug, x0[idx], yref[idx, :n], yref_e[idx], oracle.Q_DIAG, oracle.R_DIAG, oracle.QN_DIAG,
                                      0.0, 22.0, DT)
        e_c = (np.abs(cost[idx] - cr) / np.abs(cr)).max()
        e_r = np.abs(res[idx] - rr).max() / max(1.0, np.abs(rr).max())
        print(f"{what} N {n}: cost rel {e_c:.2e}  res {e_r:.2e}")
        assert e_c <= 1e-12 and e_r <= _tol(n)

    f = MixedHorizonFleet(hz)
    f.set_yref(yref, yref_e); f.set_x0(x0); f.init_iterate(INIT_HOVER)
    f.solve(1)
    f.eval_nlp()
    cost, res = f.nlp_stats()
    singles = {}
    for n, idx in f.buckets():
        c1, r1, xg, ug = single(idx, n)
        singles[n] = (idx, c1, r1, xg, ug)
        assert np.array_equal(cost[idx], c1) and np.array_equal(res[idx], r1)      # the caller's order, the per-solver results
        against_reference(cost, res, idx, n, xg, ug, "fleet")
    # the device-pointer path of the fleet getter (staging in bucket order, rows scattered on the device)
    import torch
    dc = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    dr = torch.full((B, 3), float("nan"), dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert f._L.cfnmpc_fleet_get_nlp_stats(f._h, C.c_void_p(dc.data_ptr()), C.c_void_p(dr.data_ptr()), 1, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(dc.cpu().numpy(), cost) and np.array_equal(dr.cpu().numpy(), res)
    assert f._L.cfnmpc_fleet_get_nlp_stats(f._h, C.c_void_p(0), C.c_void_p(0), 0, st) == EINVAL
    # multi: two shards on device 0, both create variants
    N = 50
    m = parallel.MultiGpuFleet(B, [0, 0], default_opts())
    m.set_x0(x0); m.set_yref(yref[:, :N].copy(), yref_e); m.init_iterate(INIT_HOVER)
    m.solve(1); m.sync()
    m.eval_nlp()
    cm, rm = m.nlp_stats()
    allidx = np.arange(B)
    c1, r1, xg, ug = single(allidx, N)
    assert np.array_equal(cm, c1) and np.array_equal(rm, r1)
    against_reference(cm, rm, allidx, N, xg, ug, "multi")
    mh = parallel.MultiGpuFleet(B, [0, 0], default_opts(), horizons=hz)
    mh.set_x0(x0); mh.set_yref(yref, yref_e); mh.init_iterate(INIT_HOVER)
    mh.solve(1); mh.sync()
    mh.eval_nlp()
    ch, rh = mh.nlp_stats()
    assert np.array_equal(ch, cost) and np.array_equal(rh, res)


# ---- 8. full size ----------------------------------------------------------------------------------------------------------------------
def test_full_size(oracle):
    B, N = 65536, 50
    x0, yref, yref_e = _inputs(oracle, B, N, seed=81, scale=1.0)
    s = _solver(B, x0, yref, yref_e)
    s.solve(1)
    st0, it0, rs0 = s.stats()
    s.eval_nlp()
    cost, res = s.nlp_stats()
    assert np.isfinite(cost).all() and np.isfinite(res).all() and (cost > 0).all() and (res >= 0).all()
    s.eval_nlp(keep_multipliers=True)
    c2, r2 = s.nlp_stats()
    assert np.array_equal(c2, cost) and np.array_equal(r2, res)      # kept multipliers change nothing of the rest
    pi, gu = s.nlp_multipliers()
    assert np.isfinite(pi).all() and np.isfinite(gu).all()
    st1, it1, rs1 = s.stats()
    assert np.array_equal(st0, st1) and np.array_equal(it0, it1) and np.array_equal(rs0, rs1)
    # spot rows against the reference (first, a wavefront boundary, last)
    rows = np.array([0, 63, 64, 4097, 65535])
    x, u = s.get_iterate()
    cr, rr, pr, gr = nlp_ref_rows(x[rows], u[rows], x0[rows], yref[rows], yref_e[rows], oracle.Q_DIAG, oracle.R_DIAG,
                                  oracle.QN_DIAG, 0.0, 22.0, DT)
    assert (np.abs(cost[rows] - cr) / np.abs(cr)).max() <= 1e-12
    assert np.abs(res[rows] - rr).max() <= 1e-9 * max(1.0, np.abs(rr).max())
    assert np.abs(pi[rows] - pr).max() <= 1e-9 * max(1.0, np.abs(pr).max())
    assert np.abs(gu[rows] - gr).max() <= 1e-9 * max(1.0, np.abs(gr).max())


# ---- acados-named drop-in ---------------------------------------------------------------------------------------------------------------
def test_shim_reports_cost_and_residuals(oracle):
    """ocp_nlp_eval_cost / ocp_nlp_eval_residuals / ocp_nlp_get of the batch-1 drop-in against a BatchSolver given the same step"""
    import os
    from crazyflie_nmpc_amd import _lib
    _lib.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shim = C.CDLL(os.path.join(root, "crazyflie_nmpc_amd", "libacados_solver_crazyflie.so"))
    N = 50
    x0, yref, yref_e = _inputs(oracle, 1, N, seed=91)
    dbl13 = C.c_double * 13
    shim.ocp_nlp_constraints_model_set.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_void_p]
    shim.ocp_nlp_cost_model_set.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_void_p]
    shim.ocp_nlp_get.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p]
    shim.ocp_nlp_eval_cost.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    shim.ocp_nlp_eval_residuals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    assert shim.acados_create() == 0
    try:
        xb = dbl13(*x0[0])
        for fld in (b"lbx", b"ubx"):
            shim.ocp_nlp_constraints_model_set(None, None, None, 0, fld, xb)
        for k in range(N):
            shim.ocp_nlp_cost_model_set(None, None, None, k, b"yref", (C.c_double * 17)(*yref[0, k]))
        shim.ocp_nlp_cost_model_set(None, None, None, N, b"yref", dbl13(*yref_e[0]))
        assert shim.acados_solve() == 0
        v = C.c_double(-7.0)
        shim.ocp_nlp_get(None, None, b"no_such_field", C.byref(v))
        assert v.value == -7.0                                          # untouched
        shim.ocp_nlp_eval_cost(None, None, None)
        shim.ocp_nlp_eval_residuals(None, None, None)
        got = []
        for fld in (b"cost_value", b"res_stat", b"res_eq", b"res_ineq"):
            shim.ocp_nlp_get(None, None, fld, C.byref(v))
            got.append(v.value)
    finally:
        shim.acados_free()
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    s = BatchSolver(1, default_opts())
    s.set_x0(x0); s.set_yref(yref, yref_e)
    s.solve(1)
    s.eval_nlp()
    cost, res = s.nlp_stats()
    assert got[0] == cost[0] and got[1:] == list(res[0])
