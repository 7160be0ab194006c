"""GPU suite: differentiable plant rollouts (include/cfnmpc.h: cfnmpc_sim_rollout, cfnmpc_sim_rollout_vjp; crazyflie_nmpc_amd.diff:
sim_rollout, sim_step).

The rollout is compared bit for bit with chained calls of the existing plant step.  The gradients are compared with reference (a)
of tests/test_sim_vjp_cpu.py (complex steps through the whole numpy rollout; checked there against an independent reverse sweep to
1.9e-15) in that file's error measure -- per vehicle and output array, max |difference| / max(1, max |reference|), the parameter
gradient as gp * p -- with the solver's own linearisation (a second GPU code path that shares only the model header), and, chained
behind the controller, with central differences of parent code (solve + sim).  Shapes: B = 1, 37 (a ragged wave), 300 (more than
one 256-lane block); L in {1, 2, 7, 20}; steps in {1, 3}; rows none / p / d / p + d."""
import ctypes as C

import numpy as np
import pytest

from test_disturbance_cpu import random_dist
from test_gpu_adjoint import FD_W, FD_X, FD_Y, _fd_setup
from test_gpu_disturbance import _iterate, _solver
from test_model_params_cpu import NOMINAL, hover, random_params
from test_sim_vjp_cpu import ROWS, draw, reference, rows_of, scaled_err, worst_err

pytestmark = pytest.mark.gpu
T = 0.015
EINVAL = -1


def _sel(c, rows):
    """(params, dist) as the Python calls take them for a row combination"""
    return (c["p"] if "p" in rows else None), (c["d"] if "d" in rows else None)


def _dev(a):
    import torch
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


# ---- 1. the rollout is the existing plant --------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("steps", [1, 3])
def test_rollout_is_the_existing_plant(rows, steps):
    import crazyflie_nmpc_amd as cf
    B, L = 300, 7
    c = draw(21, B, L)
    p, d = _sel(c, rows)
    xs = cf.sim_rollout(c["x0"], c["u"], T, steps, params=p, dist=d)
    assert xs.shape == (B, L + 1, 13) and np.array_equal(xs[:, 0], c["x0"])
    x = c["x0"]
    for t in range(L):
        x = cf.sim(x, np.ascontiguousarray(c["u"][:, t]), T, steps, params=p, dist=d)
        assert np.array_equal(xs[:, t + 1], x), t
    xd = cf.sim_rollout(_dev(c["x0"]), _dev(c["u"]), T, steps, params=_dev(p), dist=_dev(d))
    assert np.array_equal(xd.cpu().numpy(), xs)
    out = np.empty((B, L + 1, 13))
    assert cf.sim_rollout(c["x0"], c["u"], T, steps, out=out, params=p, dist=d) is out and np.array_equal(out, xs)


# ---- 2. gradients against reference (a) ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("B,L,steps", [(1, 1, 1), (37, 2, 3), (300, 7, 1), (64, 20, 3)])
def test_gradients_match_reference(B, L, steps, rows):
    import crazyflie_nmpc_amd as cf
    c, ref = reference(31, B, L, steps, rows)
    p, d = _sel(c, rows)
    pm, _dm = rows_of(c, rows)
    xs = cf.sim_rollout(c["x0"], c["u"], T, steps, params=p, dist=d)
    got = cf.sim_rollout_vjp(xs, c["u"], c["gxs"], T, steps, params=p, dist=d)
    assert (got[2] is None) == (p is None) and (got[3] is None) == (d is None)
    each = [None if g is None else float(scaled_err(g, r, pm if i == 2 else None).max()) for i, (g, r) in enumerate(zip(got, ref))]
    print(f"(B, L, steps) = ({B}, {L}, {steps}), rows {rows}: scaled error gx0, gu, gp p, gd = "
          + ", ".join("-" if e is None else f"{e:.2e}" for e in each))
    assert worst_err(got, ref, pm) <= 1e-12
    # device tensors: the same bits
    gd_ = cf.sim_rollout_vjp(_dev(xs), _dev(c["u"]), _dev(c["gxs"]), T, steps, params=_dev(p), dist=_dev(d))
    for a, b in zip(got, gd_):
        assert (a is None) == (b is None)
        assert a is None or np.array_equal(a, b.cpu().numpy())


# ---- 3. against the solver's own linearisation ---------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3])
def test_unit_cotangents_are_rows_of_the_linearisation(oracle, M):
    import crazyflie_nmpc_amd as cf
    B, N = 37, 5
    rng = np.random.default_rng(150 + M)
    p = random_params(rng, B)
    d = random_dist(rng, B)
    x0, yr, ye, x, u = _iterate(oracle, rng, B, N, p, 9 + M)
    s = _solver(B, M, p, d, N=N)
    s.set_x0(x0); s.set_yref(yr, ye); s.set_iterate(x, u)
    s.linearise_only()
    A, Bm, _b = s.get_linearisation()
    s.close()
    # one instance per (vehicle, stage, row i): L = 1 from (x_k, u_k) with gxs[:, 1] = e_i
    R = B * N * 13
    xk = np.repeat(x[:, :N].reshape(B * N, 13), 13, 0)
    uk = np.repeat(u.reshape(B * N, 1, 4), 13, 0)
    pk, dk = np.repeat(np.repeat(p, N, 0), 13, 0), np.repeat(np.repeat(d, N, 0), 13, 0)
    gxs = np.zeros((R, 2, 13)); gxs[np.arange(R), 1, np.arange(R) % 13] = 1.0
    xs = cf.sim_rollout(xk, uk, T, M, params=pk, dist=dk)
    gx0, gu, _gp, _gd = cf.sim_rollout_vjp(xs, uk, gxs, T, M, params=pk, dist=dk)
    ea = float(scaled_err(gx0.reshape(B * N, 13, 13), A.reshape(B * N, 13, 13)).max())
    eb = float(scaled_err(gu.reshape(B * N, 13, 4), Bm.reshape(B * N, 13, 4)).max())
    print(f"erk_steps = steps = {M}: rows of A {ea:.2e}, rows of B {eb:.2e}")
    assert ea <= 1e-12 and eb <= 1e-12


# ---- 4. structure --------------------------------------------------------------------------------------------------------------
def _call_vjp(L_, B, L, steps, Tv, xs, u, p, d, gxs, gx0, gu, gp, gd):
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    return L_.cfnmpc_sim_rollout_vjp(B, L, ptr(xs), ptr(u), ptr(p), ptr(d), Tv, steps, ptr(gxs), ptr(gx0), ptr(gu), ptr(gp), ptr(gd), 0, None)


def test_null_outputs_repeat_calls_and_stage_zero():
    import crazyflie_nmpc_amd as cf
    from crazyflie_nmpc_amd import _lib
    L_ = _lib.lib()
    B, L, steps = 37, 7, 3
    c = draw(41, B, L)
    xs = cf.sim_rollout(c["x0"], c["u"], T, steps, params=c["p"], dist=c["d"])
    full = cf.sim_rollout_vjp(xs, c["u"], c["gxs"], T, steps, params=c["p"], dist=c["d"])
    again = cf.sim_rollout_vjp(xs, c["u"], c["gxs"], T, steps, params=c["p"], dist=c["d"])
    for a, b in zip(full, again):
        assert np.array_equal(a, b)
    # NULL gu / gp / gd in every combination: what is written keeps its bits, also with the rows themselves NULL
    for mask in range(8):
        outs = [np.full((B, 13), np.nan)] + [np.full(s, np.nan) if mask >> i & 1 else None for i, s in enumerate(((B, L, 4), (B, 8), (B, 6)))]
        assert _call_vjp(L_, B, L, steps, T, xs, c["u"], c["p"], c["d"], c["gxs"], *outs) == 0
        for a, b in zip(outs, full):
            assert a is None or np.array_equal(a, b)
    xn = cf.sim_rollout(c["x0"], c["u"], T, steps)
    base = [np.empty((B, 13)), np.empty((B, L, 4)), np.empty((B, 8)), np.empty((B, 6))]
    assert _call_vjp(L_, B, L, steps, T, xn, c["u"], None, None, c["gxs"], *base) == 0     # gp at the nominal row, gd at the zero row
    only = np.empty((B, 13))
    assert _call_vjp(L_, B, L, steps, T, xn, c["u"], None, None, c["gxs"], only, None, None, None) == 0
    assert np.array_equal(only, base[0])
    nom = cf.sim_rollout_vjp(xn, c["u"], c["gxs"], T, steps, params=np.tile(NOMINAL, (B, 1)), dist=np.zeros((B, 6)))
    assert worst_err(base, nom, np.tile(NOMINAL, (B, 1))) <= 1e-12
    # a cotangent at stage 0 alone passes through
    g0 = np.zeros_like(c["gxs"]); g0[:, 0] = c["gxs"][:, 0]
    z = cf.sim_rollout_vjp(xs, c["u"], g0, T, steps, params=c["p"], dist=c["d"])
    assert np.array_equal(z[0], c["gxs"][:, 0])
    assert all(np.all(a == 0.0) for a in z[1:])


def test_refusals_write_nothing():
    from crazyflie_nmpc_amd import _lib
    L_ = _lib.lib()
    B, L = 5, 3
    c = draw(43, B, L)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    xs = np.full((B, L + 1, 13), 7.0)
    bad_p, bad_p2, bad_d = c["p"].copy(), c["p"].copy(), c["d"].copy()
    bad_p[2, 3] = 0.0; bad_p2[4, 1] = np.nan; bad_d[1, 5] = np.inf
    roll = dict(B=B, L=L, x0=c["x0"], u=c["u"], p=c["p"], d=c["d"], T=T, steps=1, xs=xs)
    bad = [dict(B=0), dict(B=-3), dict(L=0), dict(steps=0), dict(T=0.0), dict(T=-0.015), dict(T=float("nan")), dict(x0=None),
           dict(u=None), dict(p=bad_p), dict(p=bad_p2), dict(d=bad_d)]
    for kw in bad + [dict(xs=None)]:
        a = dict(roll, **kw)
        rc = L_.cfnmpc_sim_rollout(a["B"], a["L"], ptr(a["x0"]), ptr(a["u"]), ptr(a["p"]), ptr(a["d"]), a["T"], a["steps"], ptr(a["xs"]), 0, None)
        assert rc == EINVAL, kw
        assert np.all(xs == 7.0), kw
    good = np.empty((B, L + 1, 13))
    assert L_.cfnmpc_sim_rollout(B, L, ptr(c["x0"]), ptr(c["u"]), ptr(c["p"]), ptr(c["d"]), T, 1, ptr(good), 0, None) == 0
    outs = [np.full((B, 13), 7.0), np.full((B, L, 4), 7.0), np.full((B, 8), 7.0), np.full((B, 6), 7.0)]
    vjp = dict(B=B, L=L, xs=good, u=c["u"], p=c["p"], d=c["d"], T=T, steps=1, gxs=c["gxs"], gx0=outs[0])
    for kw in [k for k in bad if "x0" not in k] + [dict(xs=None), dict(gxs=None), dict(gx0=None)]:
        a = dict(vjp, **kw)
        rc = _call_vjp(L_, a["B"], a["L"], a["steps"], a["T"], a["xs"], a["u"], a["p"], a["d"], a["gxs"], a["gx0"], outs[1], outs[2], outs[3])
        assert rc == EINVAL, kw
        assert all(np.all(o == 7.0) for o in outs), kw


# ---- 5. autograd ---------------------------------------------------------------------------------------------------------------
def test_autograd_is_the_c_call():
    import torch
    import crazyflie_nmpc_amd as cf
    from crazyflie_nmpc_amd import diff
    B, L, steps = 37, 7, 3
    c = draw(51, B, L)
    leaves = [_dev(c[k]).requires_grad_() for k in ("x0", "u", "p", "d")]
    gxs = _dev(c["gxs"])
    xs = diff.sim_rollout(*leaves, T=T, steps=steps)
    assert tuple(xs.shape) == (B, L + 1, 13)
    assert np.array_equal(xs.detach().cpu().numpy(), cf.sim_rollout(c["x0"], c["u"], T, steps, params=c["p"], dist=c["d"]))
    (xs * gxs).sum().backward()
    torch.cuda.synchronize()
    want = cf.sim_rollout_vjp(xs.detach(), _dev(c["u"]), gxs, T, steps, params=_dev(c["p"]), dist=_dev(c["d"]))
    for leaf, w in zip(leaves, want):
        assert torch.equal(leaf.grad, w)
    with pytest.raises(RuntimeError):     # the stored rollout is released by the first backward()
        (xs * gxs).sum().backward()
    # without rows: only x0 and u have gradients; sim_step is L = 1
    x0, u = _dev(c["x0"]).requires_grad_(), _dev(c["u"][:, 0]).requires_grad_()
    x1 = diff.sim_step(x0, u, T=T, steps=steps)
    assert torch.equal(x1, diff.sim_rollout(x0, u.unsqueeze(1), T=T, steps=steps)[:, 1])
    assert np.array_equal(x1.detach().cpu().numpy(), cf.sim(c["x0"], np.ascontiguousarray(c["u"][:, 0]), T, steps))
    x1.sum().backward()
    assert x0.grad is not None and tuple(u.grad.shape) == (B, 4)
    with pytest.raises(ValueError):
        diff.sim_rollout(x0.float(), u.unsqueeze(1))


# ---- 6. chained behind the controller ------------------------------------------------------------------------------------------
def test_chain_with_the_controller(oracle):
    """loss = |x1[0:3] - target|^2 on the state the PLANT (own p, d rows) reaches after the controller's u_0: the leaf gradients
    through sim_step and rti_step against central differences of the same loss over the replicas of test_gpu_adjoint's harness,
    the forward side of which is solve + sim"""
    import torch
    import crazyflie_nmpc_amd as cf
    from crazyflie_nmpc_amd.diff import rti_step, sim_step
    h = 1e-6
    r, inp = _fd_setup(oracle, solve=False)
    B, N, R = r.B // 7, r.N, r.B
    rng = np.random.default_rng(61)
    rep = lambda a: np.ascontiguousarray(np.repeat(a, 7, 0))   # noqa: E731
    p, d = rep(NOMINAL * rng.uniform(0.8, 1.25, (B, 8))), rep(random_dist(rng, B))
    target = rep(inp["x0"][::7, 0:3] + rng.uniform(-0.5, 0.5, (B, 3)))
    leaves = [_dev(inp[k]).requires_grad_() for k in ("x0", "W", "WN", "yref", "yref_e")]
    u0 = rti_step(r, *leaves)[1][:, 0]
    x1 = sim_step(leaves[0], u0, _dev(p), _dev(d))
    ((x1[:, 0:3] - _dev(target)) ** 2).sum().backward()
    torch.cuda.synchronize()
    grads = np.stack([leaves[1].grad.cpu().numpy()[::7, FD_W], leaves[3].grad.cpu().numpy()[::7, FD_Y[0], FD_Y[1]],
                      leaves[0].grad.cpu().numpy()[::7, FD_X]], axis=1)
    # the same loss from parent code: the solver's new iterate (rti_step's forward pass is one solve) and the plant step
    un = np.ascontiguousarray(r.get_iterate()[1][:, 0])
    xn = cf.sim(inp["x0"], un, T, 1, params=p, dist=d)
    assert np.array_equal(xn, x1.detach().cpu().numpy())
    loss = ((xn[:, 0:3] - target) ** 2).sum(axis=1).reshape(B, 7)
    act = r.sens_active().reshape(B, 7, N, 4)
    kept = []
    for k in range(3):
        same = np.array([np.array_equal(act[i, 0], act[i, 1 + 2 * k]) and np.array_equal(act[i, 0], act[i, 2 + 2 * k]) for i in range(B)])
        fd = (loss[:, 1 + 2 * k] - loss[:, 2 + 2 * k]) / (2 * h)
        err = np.abs(fd - grads[:, k]) / np.maximum(1.0, np.abs(grads[:, k]))
        print(f"chain, {('W', 'yref', 'x0')[k]}: {same.sum()} of {B} rows kept, worst relative {err[same].max():.2e}, "
              f"largest |gradient| {np.abs(grads[same, k]).max():.2e}")
        assert err[same].max() <= 1e-5, (k, err[same].max())
        kept.append(int(same.sum()))
    assert min(kept) >= 48, kept
    r.close()


# ---- 7. identification ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 3])
def test_disturbance_descent_on_the_gpu(steps):
    """the fixed-step descent of tests/test_sim_vjp_cpu.py with diff.sim_step; the logged step comes from cfnmpc_sim_dist"""
    import torch
    import crazyflie_nmpc_amd as cf
    from crazyflie_nmpc_amd.diff import sim_step
    rng = np.random.default_rng(5)
    B = 16
    p = np.tile(NOMINAL, (B, 1)); p[:, 1] *= rng.uniform(0.8, 1.25, B)
    x0 = np.zeros((B, 13)); x0[:, 0:3] = rng.uniform(-1, 1, (B, 3)); x0[:, 3] = 1.0
    u = np.tile(hover(p)[:, None], (1, 4))
    d_true = random_dist(rng, B, 2.0, 5.0)
    logged = _dev(cf.sim(x0, u, T, steps, params=p, dist=d_true))
    x0_, u_, p_ = _dev(x0), _dev(u), _dev(p)
    d = torch.zeros((B, 6), dtype=torch.float64, device="cuda", requires_grad=True)
    course = []
    for _ in range(8):
        x1 = sim_step(x0_, u_, p_, d, T=T, steps=steps)
        ((x1[:, 7:13] - logged[:, 7:13]) ** 2).sum().backward()
        d = (d - d.grad / (2 * T * T)).detach().requires_grad_()
        course.append(float(np.abs(d.detach().cpu().numpy() - d_true).max()))
    print(f"steps = {steps}: worst |d - d_true| per iteration " + " ".join(f"{e:.1e}" for e in course))
    assert np.abs(d.detach().cpu().numpy() - d_true).max(axis=1).max() <= 1e-10
