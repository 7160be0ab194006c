"""Differentiable RTI step: torch autograd through the last QP of a BatchSolver.

    x, u = rti_step(solver, x0, W, WN, yref, yref_e)
    loss(u[:, 0]).backward()        # -> x0.grad, W.grad, WN.grad, yref.grad, yref_e.grad

The forward pass sets the rows, runs one RTI step from the solver's current iterate and evaluates the active set
(eval_sens_x0); the backward pass is one eval_adjoint with the incoming gradients.  In an RTI step the linearisation belongs to
the previous iterate, so A, B, b do not depend on this step's x0, weights or references: the gradient through the QP is the exact
gradient of the step with its active set held.  Everything stays on the device: no graph capture, no host copy of a trajectory.
The solver is state: backward() must run before the solver's data change or it solves again (it raises otherwise).

Differentiable plant: sim_rollout / sim_step are the RK4 plant of `sim` as autograd functions of the
state, the inputs and the per-vehicle parameter and disturbance rows; the backward pass is one sim_rollout_vjp (reverse mode
through RK4).  The one-step closed-loop chain, a loss on the state the VEHICLE reaches after the controller's first input:

    u = rti_step(solver, x0, W, WN, yref, yref_e)[1][:, 0]; x1 = sim_step(x0, u, p, d)
    loss(x1).backward()             # -> x0.grad (through controller and plant), W.grad, ..., p.grad, d.grad

A longer closed-loop chain takes one BatchSolver per step: each rti_step owns its solver's last QP until its backward() ran."""
from __future__ import annotations

import torch

from . import solver as _solver
from ._lib import NU, NX, NY


class _RtiStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, act_tol, x0, W, WN, yref, yref_e):
        args = [t.detach().contiguous() for t in (x0, W, WN, yref, yref_e)]
        solver.set_weights_batch(args[1], args[2])
        solver.set_x0(args[0])
        solver.set_yref(args[3], args[4])
        solver.solve(1)
        solver.eval_sens_x0(act_tol)
        x = torch.empty((solver.B, solver.N + 1, NX), dtype=torch.float64, device=x0.device)
        u = torch.empty((solver.B, solver.N, NU), dtype=torch.float64, device=x0.device)
        solver.get_iterate(out=(x, u))
        ctx.solver = solver
        ctx.token = solver._rti_step_token = object()
        ctx.set_materialize_grads(False)
        return x, u

    @staticmethod
    def backward(ctx, gx, gu):
        s = ctx.solver
        if getattr(s, "_rti_step_token", None) is not ctx.token:
            raise RuntimeError("rti_step: the solver has run another rti_step since this one; backward() belongs to its last QP")
        dev = torch.device("cuda", s._device if s._device is not None else torch.cuda.current_device())
        B, N = s.B, s.N
        if gx is None and gu is None:
            gu = torch.zeros((B, 1, NU), dtype=torch.float64, device=dev)
        s.eval_adjoint(None if gx is None else gx.contiguous(), None if gu is None else gu.contiguous())
        f64 = dict(dtype=torch.float64, device=dev)
        dx0 = torch.empty((B, NX), **f64)
        dW, dWN = torch.empty((B, NY), **f64), torch.empty((B, NX), **f64)
        dy, dye = torch.empty((B, N, NY), **f64), torch.empty((B, NX), **f64)
        s.adjoint(out=(dx0, None, None, None, None))
        s.adjoint_cost(out=(dW, dWN, dy, dye))
        return None, None, dx0, dW, dWN, dy, dye


def rti_step(solver, x0, W, WN, yref, yref_e, act_tol=1e-6):
    """One RTI step of `solver` (a BatchSolver) as a differentiable function of x0 [B, 13], the weight rows W [B, 17] and
    WN [B, 13] (unscaled, as set_weights_batch takes them), yref [B, N, 17] and yref_e [B, 13] -- float64 device tensors --
    -> (x [B, N + 1, 13], u [B, N, 4]), the new iterate.  The step starts from the solver's current iterate; the rows stay in
    force afterwards.  act_tol: eval_sens_x0's activity tolerance."""
    for t, sh in ((x0, (solver.B, NX)), (W, (solver.B, NY)), (WN, (solver.B, NX)), (yref, (solver.B, solver.N, NY)),
                  (yref_e, (solver.B, NX))):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == sh):
            raise ValueError(f"rti_step: expected a float64 device tensor of shape {sh}")
    return _RtiStep.apply(solver, float(act_tol), x0, W, WN, yref, yref_e)


class _SimRollout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, T, steps, x0, u, params, dist):
        x0_, u_ = x0.detach().contiguous(), u.detach().contiguous()
        p_ = None if params is None else params.detach().contiguous()
        d_ = None if dist is None else dist.detach().contiguous()
        xs = _solver.sim_rollout(x0_, u_, T=T, steps=steps, params=p_, dist=d_)
        ctx.save_for_backward(xs, u_, p_, d_)
        ctx.T, ctx.steps = T, steps
        return xs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gxs):
        xs, u_, p_, d_ = ctx.saved_tensors   # (released by the first backward(): a second one through the same graph raises)
        need = ctx.needs_input_grad   # (T, steps, x0, u, params, dist)
        B, L = u_.shape[0], u_.shape[1]
        f64 = dict(dtype=torch.float64, device=xs.device)
        gx0 = torch.empty((B, NX), **f64)
        gu = torch.empty((B, L, NU), **f64)
        gx0, gu, gp, gd = _solver.sim_rollout_vjp(xs, u_, gxs.contiguous(), T=ctx.T, steps=ctx.steps, params=p_, dist=d_,
                                                  out=(gx0, gu, None, None))
        return (None, None, gx0 if need[2] else None, gu if need[3] else None, gp if need[4] else None, gd if need[5] else None)


def sim_rollout(x0, u, params=None, dist=None, T=0.015, steps=1):
    """The open-loop plant rollout (solver.sim_rollout) as a once-differentiable function of x0 [B, 13], u [B, L, 4] and the
    optional rows params [B, 8], dist [B, 6] -- float64 device tensors -> xs [B, L + 1, 13], xs[:, 0] = x0.  backward() is one
    sim_rollout_vjp on the stored rollout; nothing is copied to the host."""
    B = x0.shape[0] if torch.is_tensor(x0) and x0.dim() == 2 else -1
    L = u.shape[1] if torch.is_tensor(u) and u.dim() == 3 else -1
    for t, sh, opt in ((x0, (B, NX), False), (u, (B, L, NU), False), (params, (B, _solver.NP), True), (dist, (B, _solver.ND), True)):
        if t is None and opt:
            continue
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == sh and B > 0 and L > 0):
            raise ValueError(f"sim_rollout: expected a float64 device tensor of shape {sh}")
    return _SimRollout.apply(float(T), int(steps), x0, u, params, dist)


def sim_step(x, u, params=None, dist=None, T=0.015, steps=1):
    """One plant step x [B, 13], u [B, 4] -> x_next [B, 13]: sim_rollout with L = 1."""
    if not (torch.is_tensor(u) and u.dim() == 2):
        raise ValueError("sim_step: expected u of shape (B, 4)")
    return sim_rollout(x, u.unsqueeze(1), params, dist, T, steps)[:, 1]
