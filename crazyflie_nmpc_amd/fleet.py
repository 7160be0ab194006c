"""Mixed-horizon fleets (BASELINE.json config C5: N in {30, 50, 100}, dt fixed at 15 ms).

Thin wrapper over the C-ABI's cfnmpc_fleet_* (include/cfnmpc.h): the library buckets the vehicles
by horizon (one solver per distinct N -- a solver's workspace is blocked by stage for one
horizon), keeps the caller's vehicle order at the boundary and solves the buckets concurrently.
A bucket is also the unit of multi-GPU balancing (parallel.shard_by_horizon deals buckets out by
sum N).  Arrays may be numpy (host) or torch device tensors, as for BatchSolver."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import NU, NX, NY
from .solver import NFLAT, SQP_MODES, PolyCalls, UncertaintyCalls, _arg, _check, _sqp_mode, default_opts, _launch_stream, _torch_device
from .synthetic import regulation_row


def _weight_rows(B, W, WN):
    """host rows of set_weights_batch -> ((pointer or None, keepalive), (pointer or None, keepalive))"""
    out = []
    for a, n in ((W, 17), (WN, 13)):
        if a is None:
            out.append((None, None))
            continue
        arr = np.ascontiguousarray(a, dtype=np.float64)
        if arr.shape != (B, n):
            raise ValueError(f"expected shape {(B, n)}, got {arr.shape}")
        out.append((arr.ctypes.data_as(C.c_void_p), arr))
    return out


class MixedHorizonFleet(UncertaintyCalls, PolyCalls):
    _unc_pre = "cfnmpc_fleet_"
    _unc_N = property(lambda self: self.Nmax)

    def __init__(self, horizons, **opt_kw):
        self._L = _lib.lib()
        self.horizons = np.ascontiguousarray(horizons, dtype=np.int32)
        self.B = len(self.horizons)
        self.opts = default_opts(**opt_kw)
        h = C.c_void_p()
        _check(self._L.cfnmpc_fleet_create(C.byref(h), self.B, self.horizons.ctypes.data_as(C.c_void_p), C.byref(self.opts)),
               "cfnmpc_fleet_create")
        self._h = h
        self._device = _torch_device()
        self.Nmin = self._L.cfnmpc_fleet_min_horizon(h)
        self.Nmax = self._L.cfnmpc_fleet_max_horizon(h)

    def close(self):
        if getattr(self, "_h", None):
            self._L.cfnmpc_fleet_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def workspace_bytes(self):
        return int(self._L.cfnmpc_fleet_workspace_bytes(self._h))

    def buckets(self):
        """-> [(N, fleet indices of the bucket's rows)] in ascending N"""
        out = []
        for b in range(self._L.cfnmpc_fleet_num_buckets(self._h)):
            n, c = C.c_int(0), C.c_int(0)
            _check(self._L.cfnmpc_fleet_bucket(self._h, b, C.byref(n), C.byref(c), None, None), "cfnmpc_fleet_bucket")
            idx = np.empty(c.value, dtype=np.int32)
            _check(self._L.cfnmpc_fleet_bucket(self._h, b, None, None, None, idx.ctypes.data_as(C.c_void_p)), "cfnmpc_fleet_bucket")
            out.append((n.value, idx))
        return out

    def bucket_iterates(self):
        """-> [(N, fleet indices, x [count][N+1][13], u [count][N][4])] per bucket: the persistent iterates (nlp_out of
        acados_mpc.cpp:77) through the buckets' own solvers (cfnmpc_fleet_bucket + cfnmpc_get_iterate), host arrays"""
        out = []
        for b in range(self._L.cfnmpc_fleet_num_buckets(self._h)):
            n, c, sv = C.c_int(0), C.c_int(0), C.c_void_p()
            _check(self._L.cfnmpc_fleet_bucket(self._h, b, C.byref(n), C.byref(c), C.byref(sv), None), "cfnmpc_fleet_bucket")
            idx = np.empty(c.value, dtype=np.int32)
            _check(self._L.cfnmpc_fleet_bucket(self._h, b, None, None, None, idx.ctypes.data_as(C.c_void_p)), "cfnmpc_fleet_bucket")
            x = np.empty((c.value, n.value + 1, NX)); u = np.empty((c.value, n.value, NU))
            _check(self._L.cfnmpc_get_iterate(sv, x.ctypes.data_as(C.c_void_p), u.ctypes.data_as(C.c_void_p), 0,
                                              _launch_stream(None, self._device)), "cfnmpc_get_iterate")
            out.append((n.value, idx, x, u))
        return out

    def set_regulation(self, xyz, uss):
        """xyz [B][3]: Regulation reference of every vehicle (acados_mpc.cpp:435-454)."""
        rows = np.stack([regulation_row(xyz[i], uss) for i in range(self.B)])
        self.set_yref(np.repeat(rows[:, None, :], self.Nmax, 1).copy(), rows[:, :13].copy())

    def set_yref(self, yref, yref_e):
        """yref [B][Nmax][17] (vehicle i uses rows 0..N_i-1), yref_e [B][13]"""
        p, dev, st, _k = _arg(yref, (self.B, self.Nmax, NY), device=self._device)
        pe, deve, _st, _k2 = _arg(yref_e, (self.B, NX), device=self._device)
        if dev != deve:
            raise ValueError("yref and yref_e must live on the same side")
        _check(self._L.cfnmpc_fleet_set_yref(self._h, p, pe, dev, st), "cfnmpc_fleet_set_yref")

    def eval_poly(self, t, flags=0, want_flat=True, want_rows=True):
        """-> (flat [B][Nmax][13], rows [B][Nmax][17]): every vehicle's own N stage rows of set_yref_poly, NaN behind its
        horizon and for vehicles without a trajectory; host arrays, None where not wanted"""
        fl = np.empty((self.B, self.Nmax, NFLAT)) if want_flat else None
        rw = np.empty((self.B, self.Nmax, NY)) if want_rows else None
        _check(self._L.cfnmpc_fleet_eval_poly(self._h, float(t), int(flags), None if fl is None else fl.ctypes.data_as(C.c_void_p),
                                              None if rw is None else rw.ctypes.data_as(C.c_void_p), 0, _launch_stream(None, self._device)),
               "cfnmpc_fleet_eval_poly")
        return fl, rw

    def set_x0(self, x0):
        p, dev, st, _k = _arg(x0, (self.B, NX), device=self._device)
        _check(self._L.cfnmpc_fleet_set_x0(self._h, p, dev, st), "cfnmpc_fleet_set_x0")

    def set_weights(self, W=None, WN=None):
        w = None if W is None else np.ascontiguousarray(W, dtype=np.float64)
        wn = None if WN is None else np.ascontiguousarray(WN, dtype=np.float64)
        _check(self._L.cfnmpc_fleet_set_weights(self._h, None if w is None else w.ctypes.data_as(C.c_void_p),
                                                None if wn is None else wn.ctypes.data_as(C.c_void_p)), "cfnmpc_fleet_set_weights")

    def set_box(self, u_min, u_max):
        _check(self._L.cfnmpc_fleet_set_box(self._h, float(u_min), float(u_max)), "cfnmpc_fleet_set_box")

    def set_erk_steps(self, n):
        _check(self._L.cfnmpc_fleet_set_erk_steps(self._h, int(n)), "cfnmpc_fleet_set_erk_steps")

    def set_cost_scaling(self, stage=1.0, terminal=1.0):
        _check(self._L.cfnmpc_fleet_set_cost_scaling(self._h, float(stage), float(terminal)), "cfnmpc_fleet_set_cost_scaling")

    def set_model_params(self, p=None):
        """per-vehicle model parameters, host array [B][NP] in the fleet's vehicle order; None: nominal"""
        if p is None:
            _check(self._L.cfnmpc_fleet_set_model_params(self._h, None), "cfnmpc_fleet_set_model_params")
            return
        pa = np.ascontiguousarray(p, dtype=np.float64)
        if pa.shape != (self.B, 8):
            raise ValueError(f"expected shape {(self.B, 8)}, got {pa.shape}")
        _check(self._L.cfnmpc_fleet_set_model_params(self._h, pa.ctypes.data_as(C.c_void_p)), "cfnmpc_fleet_set_model_params")

    def set_disturbance(self, d=None, stream=None):
        """per-vehicle disturbance rows [B][6] in the fleet's vehicle order (numpy or a device tensor); None: none"""
        if d is None:
            _check(self._L.cfnmpc_fleet_set_disturbance(self._h, None, 0, _launch_stream(stream, self._device)), "cfnmpc_fleet_set_disturbance")
            return
        pd, dev, st, _k = _arg(d, (self.B, 6), device=self._device)
        if stream:
            st = C.c_void_p(stream)
        _check(self._L.cfnmpc_fleet_set_disturbance(self._h, pd, dev, st), "cfnmpc_fleet_set_disturbance")

    def disturbance(self):
        """-> [B][6] rows in force, in the fleet's vehicle order (zeros while none are set)"""
        out = np.empty((self.B, 6))
        _check(self._L.cfnmpc_fleet_get_disturbance(self._h, out.ctypes.data_as(C.c_void_p), 0, None), "cfnmpc_fleet_get_disturbance")
        return out

    def set_weights_batch(self, W=None, WN=None):
        """per-vehicle cost weights, host arrays W [B][17] / WN [B][13] in the fleet's vehicle order; None, None: uniform"""
        pw, pn = _weight_rows(self.B, W, WN)
        _check(self._L.cfnmpc_fleet_set_weights_batch(self._h, pw[0], pn[0]), "cfnmpc_fleet_set_weights_batch")

    def set_box_stages(self, lb=None, ub=None):
        """per-stage / per-input boxes, host arrays [B][Nmax][4] (vehicle i uses rows 0..N_i-1); None, None: scalar box"""
        if lb is None and ub is None:
            _check(self._L.cfnmpc_fleet_set_box_stages(self._h, None, None), "cfnmpc_fleet_set_box_stages")
            return
        lb = np.ascontiguousarray(lb, dtype=np.float64); ub = np.ascontiguousarray(ub, dtype=np.float64)
        assert lb.shape == (self.B, self.Nmax, 4) and ub.shape == lb.shape
        _check(self._L.cfnmpc_fleet_set_box_stages(self._h, lb.ctypes.data_as(C.c_void_p), ub.ctypes.data_as(C.c_void_p)), "cfnmpc_fleet_set_box_stages")

    def get_cmd(self, cmd_vel=None, motvel=None):
        """Output stage of the reference node for the whole fleet (cfnmpc_fleet_get_cmd)."""
        if cmd_vel is None:
            cmd_vel = np.empty((self.B, 4))
        if motvel is None:
            if type(cmd_vel).__module__.startswith("torch"):
                import torch
                motvel = torch.empty((self.B, 4), dtype=torch.int32, device=cmd_vel.device)
            else:
                motvel = np.empty((self.B, 4), dtype=np.int32)
        p, dev, st, _k = _arg(cmd_vel, (self.B, 4), device=self._device)
        pm, devm, _s, _k2 = _arg(motvel, (self.B, 4), np.int32, device=self._device)
        assert dev == devm
        _check(self._L.cfnmpc_fleet_get_cmd(self._h, p, pm, dev, st), "cfnmpc_fleet_get_cmd")
        return cmd_vel, motvel

    def init_iterate(self, mode, stream=None):
        _check(self._L.cfnmpc_fleet_init_iterate(self._h, int(mode), _launch_stream(stream, self._device)), "cfnmpc_fleet_init_iterate")

    def solve(self, n_rti=1, stream=None):
        _check(self._L.cfnmpc_fleet_solve(self._h, int(n_rti), _launch_stream(stream, self._device)), "cfnmpc_fleet_solve")

    def solve_sqp(self, max_iter=100, tol_step=1e-6, tol_eq=1e-6, tol_ineq=1e-6, stream=None):
        """Full SQP solve of every vehicle at its own horizon (cfnmpc_fleet_solve_sqp); returns the iterations run by the
        longest-running bucket.  Per vehicle: sqp_stats()."""
        n = C.c_int(0)
        _check(self._L.cfnmpc_fleet_solve_sqp(self._h, int(max_iter), float(tol_step), float(tol_eq), float(tol_ineq), C.byref(n),
                                              _launch_stream(stream, self._device)), "cfnmpc_fleet_solve_sqp")
        return n.value

    def sqp_stats(self):
        """-> (status [B], sqp_iter [B], res [B, 3]) of the last solve_sqp, in the fleet's vehicle order"""
        st = np.empty(self.B, dtype=np.int32); it = np.empty(self.B, dtype=np.int32); rs = np.empty((self.B, 3))
        _check(self._L.cfnmpc_fleet_get_sqp_stats(self._h, st.ctypes.data_as(C.c_void_p), it.ctypes.data_as(C.c_void_p),
                                                  rs.ctypes.data_as(C.c_void_p), 0, _launch_stream(None, self._device)),
               "cfnmpc_fleet_get_sqp_stats")
        return st, it, rs

    def set_sqp_globalization(self, mode="merit_backtracking", eta=0, reduction=0, alpha_min=0):
        """BatchSolver.set_sqp_globalization for every bucket (cfnmpc_fleet_set_sqp_globalization)"""
        m = _sqp_mode(mode)
        _check(self._L.cfnmpc_fleet_set_sqp_globalization(self._h, m, float(eta), float(reduction), float(alpha_min)),
               "cfnmpc_fleet_set_sqp_globalization")
        self._sqp_glob = (SQP_MODES[m], float(eta) or 1e-4, float(reduction) or 0.5, float(alpha_min) or 2.0 ** -10)

    def sqp_globalization(self):
        """-> (mode, eta, reduction, alpha_min) in force (the last accepted setting; the defaults before one)"""
        return getattr(self, "_sqp_glob", (SQP_MODES[0], 1e-4, 0.5, 2.0 ** -10))

    def sqp_ls_stats(self):
        """-> (alpha [B], mu [B], n_short [B], n_fail [B]) of the last solve_sqp, in the fleet's vehicle order"""
        al = np.empty(self.B); mu = np.empty(self.B); ns = np.empty(self.B, dtype=np.int32); nf = np.empty(self.B, dtype=np.int32)
        _check(self._L.cfnmpc_fleet_get_sqp_ls_stats(self._h, al.ctypes.data_as(C.c_void_p), mu.ctypes.data_as(C.c_void_p),
                                                     ns.ctypes.data_as(C.c_void_p), nf.ctypes.data_as(C.c_void_p), 0,
                                                     _launch_stream(None, self._device)), "cfnmpc_fleet_get_sqp_ls_stats")
        return al, mu, ns, nf

    def get_u(self, stage, out=None):
        if out is None:
            out = np.empty((self.B, NU))
        p, dev, st, _k = _arg(out, (self.B, NU), device=self._device)
        _check(self._L.cfnmpc_fleet_get_u(self._h, int(stage), p, dev, st), "cfnmpc_fleet_get_u")
        return out

    def eval_nlp(self, stream=None):
        """cfnmpc_fleet_eval_nlp: NLP cost and KKT residuals at every bucket's current iterate (BatchSolver.eval_nlp; the
        multipliers have one shape per horizon: through the bucket's solver)"""
        _check(self._L.cfnmpc_fleet_eval_nlp(self._h, _launch_stream(stream, self._device)), "cfnmpc_fleet_eval_nlp")

    def nlp_stats(self):
        """-> (cost [B], res [B, 3] = res_stat, res_eq, res_ineq) of the last eval_nlp, in the fleet's vehicle order"""
        cost = np.empty(self.B); res = np.empty((self.B, 3))
        _check(self._L.cfnmpc_fleet_get_nlp_stats(self._h, cost.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p), 0,
                                                  _launch_stream(None, self._device)), "cfnmpc_fleet_get_nlp_stats")
        return cost, res

    def eval_sens_x0(self, act_tol=1e-6, stream=None):
        """cfnmpc_fleet_eval_sens_x0: sensitivities w.r.t. x0 of every bucket's last QP (BatchSolver.eval_sens_x0)"""
        _check(self._L.cfnmpc_fleet_eval_sens_x0(self._h, float(act_tol), _launch_stream(stream, self._device)),
               "cfnmpc_fleet_eval_sens_x0")

    def sens_x0(self, stage=0, n_stages=None, out_u=None, out_x=None):
        """-> (du, dx) in the fleet's vehicle order, shapes as BatchSolver.sens_x0; stages up to the shortest horizon Nmin
        (du is None if the range includes stage Nmin)"""
        from .solver import sens_x0_call
        return sens_x0_call(self, self.Nmin, self._L.cfnmpc_fleet_get_sens_x0, "cfnmpc_fleet_get_sens_x0", stage, n_stages,
                            out_u, out_x)

    def eval_adjoint(self, gx=None, gu=None, stream=None):
        """cfnmpc_fleet_eval_adjoint: adjoint sensitivities of every bucket's last QP, after eval_sens_x0.  gx [B, n_g, 13],
        gu [B, n_g, 4] (numpy or device tensors, one n_g <= Nmin; one of them may be None): the loss gradients for the
        stages [0, n_g), in the fleet's vehicle order"""
        if gx is None and gu is None:
            raise ValueError("gx or gu must be given")
        n_g = int((gx if gx is not None else gu).shape[1])
        px, pu, dev, st, keep = None, None, 0, None, []
        if gx is not None:
            px, dev, st, k = _arg(gx, (self.B, n_g, NX), device=self._device); keep.append(k)
        if gu is not None:
            pu, devu, st, k = _arg(gu, (self.B, n_g, NU), device=self._device); keep.append(k)
            if gx is not None and devu != dev:
                raise ValueError("gx and gu must both be host arrays or both device tensors")
            dev = devu
        if stream:
            st = C.c_void_p(stream)
        _check(self._L.cfnmpc_fleet_eval_adjoint(self._h, px, pu, n_g, dev, st), "cfnmpc_fleet_eval_adjoint")

    def adjoint(self):
        """-> (dl_dx0 [B, 13], dl_dW [B, 17], dl_dWN [B, 13]) of the last eval_adjoint, in the fleet's vehicle order (the
        per-stage outputs: through the buckets' solvers)"""
        d0, dW, dWN = np.empty((self.B, NX)), np.empty((self.B, NY)), np.empty((self.B, NX))
        vp = C.c_void_p
        _check(self._L.cfnmpc_fleet_get_adjoint(self._h, d0.ctypes.data_as(vp), dW.ctypes.data_as(vp), dWN.ctypes.data_as(vp), 0,
                                                _launch_stream(None, self._device)), "cfnmpc_fleet_get_adjoint")
        return d0, dW, dWN

    def get_x(self, stage, out=None):
        if out is None:
            out = np.empty((self.B, NX))
        p, dev, st, _k = _arg(out, (self.B, NX), device=self._device)
        _check(self._L.cfnmpc_fleet_get_x(self._h, int(stage), p, dev, st), "cfnmpc_fleet_get_x")
        return out

    def stats(self, out=None):
        """-> (status, qp_iter, res) [B]; `out` = three torch device tensors (int32, int32, float64)
        to keep them on the device"""
        if out is not None:
            st, it, rs = out
            ps, dev, strm, _a = _arg(st, (self.B,), np.int32, device=self._device)
            pi, _d, _s, _b = _arg(it, (self.B,), np.int32, device=self._device)
            pr, _d2, _s2, _c = _arg(rs, (self.B,), device=self._device)
            _check(self._L.cfnmpc_fleet_get_stats(self._h, ps, pi, pr, dev, strm), "cfnmpc_fleet_get_stats")
            return out
        st = np.empty(self.B, dtype=np.int32); it = np.empty(self.B, dtype=np.int32); rs = np.empty(self.B)
        _check(self._L.cfnmpc_fleet_get_stats(self._h, st.ctypes.data_as(C.c_void_p), it.ctypes.data_as(C.c_void_p),
                                              rs.ctypes.data_as(C.c_void_p), 0, _launch_stream(None, self._device)), "cfnmpc_fleet_get_stats")
        return st, it, rs
