"""Multi-GPU plumbing: NMPC instances are independent, so a batch shards
across ranks with NO data-path collective; torch.distributed (RCCL on GPUs, gloo in the CPU
tests) is used only to aggregate the report."""
from __future__ import annotations

import numpy as np

BASE_SEED = 20200103


def shard_seed(rank: int) -> int:
    """Every rank draws its own shard of the synthetic fleet."""
    return BASE_SEED + int(rank)


def shard_range(total: int, rank: int, world: int):
    """Contiguous index range of `rank` when `total` instances are split over `world` ranks."""
    base, rem = divmod(int(total), int(world))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_by_horizon(horizons, world: int):
    """Mixed-horizon batches (config C5): bucket by N (wave-homogeneous), then deal the buckets out so that sum(N_i) -- the
    cost model of a step -- is balanced (SURVEY.md section 8e "Partitioning").  The partitioner is the library's
    (cfnmpc_shard_by_horizon, host code: the same one cfnmpc_multi_create_horizons uses for its shards), so bench.py's ranks
    and an in-process MultiGpuFleet split a fleet identically.  Returns a list of ascending index arrays, one per rank."""
    import ctypes as C
    from . import _lib
    hz = np.ascontiguousarray(horizons, dtype=np.int32)
    of = np.empty(len(hz), dtype=np.int32)
    rc = _lib.lib().cfnmpc_shard_by_horizon(len(hz), hz.ctypes.data_as(C.c_void_p), int(world), of.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise ValueError(f"cfnmpc_shard_by_horizon failed with code {rc} (horizons must be >= 1, world >= 1)")
    return [np.nonzero(of == r)[0].astype(np.int64) for r in range(int(world))]


def aggregate_report(elapsed: float, sums, dist=None, device=None):
    """max-over-ranks of the timed region and sum-over-ranks of additive statistics.
    `dist` is torch.distributed (initialised) or None for a single process."""
    sums = np.asarray(sums, dtype=np.float64)
    if dist is None or not dist.is_initialized():
        return float(elapsed), sums
    # (a one-rank group still goes through the collectives: that is the smoke test of the backend under torchrun)
    import torch
    t = torch.tensor([elapsed], dtype=torch.float64, device=device)
    s = torch.tensor(sums, dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dist.all_reduce(s, op=dist.ReduceOp.SUM)
    return float(t.item()), s.cpu().numpy()


class MultiGpuFleet:
    """One fleet over several GPUs from ONE process (C-ABI cfnmpc_multi_*): contiguous shards, one
    solver + stream per shard, every shard's step launched before anyone waits.  Host arrays cover
    the whole fleet.  (bench.py keeps the one-process-per-GPU form the driver launches; this is the
    deployment form for a single controller process.)"""

    def __init__(self, total_batch, device_ids, opts=None, horizons=None):
        """horizons [total_batch] (optional): one horizon per vehicle -- config C5; the shards are then cfnmpc_fleets over the
        index sets of shard_by_horizon, host arrays use the fleet layouts (yref [B][Nmax][17], boxes [B][Nmax][4])."""
        import ctypes as C
        from . import _lib
        from .solver import _check, default_opts
        self._C, self._check = C, _check
        self._L = _lib.lib()
        self.B = int(total_batch)
        self.opts = opts if opts is not None else default_opts()
        ids = np.ascontiguousarray(device_ids, dtype=np.int32)
        h = C.c_void_p()
        self.mixed = horizons is not None
        if self.mixed:
            self.horizons = np.ascontiguousarray(horizons, dtype=np.int32)
            assert self.horizons.shape == (self.B,)
            self.N = int(self.horizons.max())       # row stride of yref / boxes
            _check(self._L.cfnmpc_multi_create_horizons(C.byref(h), len(ids), ids.ctypes.data_as(C.c_void_p), self.B,
                                                        self.horizons.ctypes.data_as(C.c_void_p), C.byref(self.opts)),
                   "cfnmpc_multi_create_horizons")
        else:
            self.N = int(self.opts.N)
            _check(self._L.cfnmpc_multi_create(C.byref(h), len(ids), ids.ctypes.data_as(C.c_void_p), self.B, C.byref(self.opts)),
                   "cfnmpc_multi_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.cfnmpc_multi_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def shards(self):
        """-> [(lo, hi, device)]; mixed horizons: [(vehicle indices, device)]"""
        C = self._C
        out = []
        if self.mixed:
            for i in range(self._L.cfnmpc_multi_num_shards(self._h)):
                cnt, dev = C.c_int(0), C.c_int(0)
                self._check(self._L.cfnmpc_multi_shard_fleet(self._h, i, None, C.byref(cnt), None, C.byref(dev), None), "cfnmpc_multi_shard_fleet")
                idx = np.empty(cnt.value, dtype=np.int32)
                self._check(self._L.cfnmpc_multi_shard_fleet(self._h, i, None, None, idx.ctypes.data_as(C.c_void_p), None, None), "cfnmpc_multi_shard_fleet")
                out.append((idx, dev.value))
            return out
        for i in range(self._L.cfnmpc_multi_num_shards(self._h)):
            lo, hi, dev = C.c_int(0), C.c_int(0), C.c_int(0)
            self._check(self._L.cfnmpc_multi_shard(self._h, i, None, C.byref(lo), C.byref(hi), C.byref(dev), None), "cfnmpc_multi_shard")
            out.append((lo.value, hi.value, dev.value))
        return out

    def _p(self, a, shape, dtype=np.float64):
        a = np.ascontiguousarray(a, dtype=dtype)
        assert a.shape == tuple(shape), (a.shape, shape)
        return a, a.ctypes.data_as(self._C.c_void_p)

    def set_x0(self, x0):
        a, p = self._p(x0, (self.B, 13))
        self._check(self._L.cfnmpc_multi_set_x0(self._h, p), "cfnmpc_multi_set_x0")

    def set_yref(self, yref, yref_e):
        a, p = self._p(yref, (self.B, self.N, 17)); b, q = self._p(yref_e, (self.B, 13))
        self._check(self._L.cfnmpc_multi_set_yref(self._h, p, q), "cfnmpc_multi_set_yref")

    def set_box(self, u_min, u_max):
        assert self._L.cfnmpc_multi_set_box(self._h, float(u_min), float(u_max)) == 0

    def set_erk_steps(self, n):
        rc = self._L.cfnmpc_multi_set_erk_steps(self._h, int(n))
        if rc != 0:
            raise ValueError(f"cfnmpc_multi_set_erk_steps failed with code {rc}")

    def set_model_params(self, p=None):
        """per-vehicle model parameters, host array [B][8] of the whole fleet; None: nominal"""
        import ctypes as C
        if p is None:
            rc = self._L.cfnmpc_multi_set_model_params(self._h, None)
        else:
            pa = np.ascontiguousarray(p, dtype=np.float64)
            if pa.shape != (self.B, 8):
                raise ValueError(f"expected shape {(self.B, 8)}, got {pa.shape}")
            rc = self._L.cfnmpc_multi_set_model_params(self._h, pa.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise ValueError(f"cfnmpc_multi_set_model_params failed with code {rc}")

    def set_disturbance(self, d=None):
        """per-vehicle disturbance rows, host array [B][6] of the whole fleet; None: none"""
        import ctypes as C
        if d is None:
            rc = self._L.cfnmpc_multi_set_disturbance(self._h, None)
        else:
            da = np.ascontiguousarray(d, dtype=np.float64)
            if da.shape != (self.B, 6):
                raise ValueError(f"expected shape {(self.B, 6)}, got {da.shape}")
            rc = self._L.cfnmpc_multi_set_disturbance(self._h, da.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise ValueError(f"cfnmpc_multi_set_disturbance failed with code {rc}")

    def set_poly_library(self, tables):
        """polynomial trajectory library for every shard (BatchSolver.set_poly_library); None or an empty list clears it"""
        from .solver import CfnmpcError, _poly_library_args
        pp, pf, n, _keep = _poly_library_args(tables)
        rc = self._L.cfnmpc_multi_set_poly_library(self._h, pp, pf, n)
        if rc != 0:
            raise CfnmpcError(f"cfnmpc_multi_set_poly_library failed with code {rc}")

    def set_poly_assignment(self, traj, place=None):
        """host arrays of the whole fleet: traj [B] int32 (-1 = none), place [B][6] or None"""
        from .solver import CfnmpcError
        _t, pt = self._p(traj, (self.B,), dtype=np.int32)
        _pl, pl = (None, None) if place is None else self._p(place, (self.B, 6))
        rc = self._L.cfnmpc_multi_set_poly_assignment(self._h, pt, pl)
        if rc != 0:
            raise CfnmpcError(f"cfnmpc_multi_set_poly_assignment failed with code {rc}")

    def set_yref_poly(self, t, flags=0):
        """every shard writes its vehicles' reference windows on the device (asynchronous, like solve)"""
        from .solver import CfnmpcError
        rc = self._L.cfnmpc_multi_set_yref_poly(self._h, float(t), int(flags))
        if rc != 0:
            raise CfnmpcError(f"cfnmpc_multi_set_yref_poly failed with code {rc}")

    def set_weights_batch(self, W=None, WN=None):
        """per-vehicle cost weights, host arrays W [B][17] / WN [B][13] of the whole fleet; None, None: uniform"""
        from .fleet import _weight_rows
        from .solver import CfnmpcError
        pw, pn = _weight_rows(self.B, W, WN)
        rc = self._L.cfnmpc_multi_set_weights_batch(self._h, pw[0], pn[0])
        if rc != 0:
            raise CfnmpcError(f"cfnmpc_multi_set_weights_batch failed with code {rc}")

    def set_cost_scaling(self, stage=1.0, terminal=1.0):
        rc = self._L.cfnmpc_multi_set_cost_scaling(self._h, float(stage), float(terminal))
        if rc != 0:
            raise ValueError(f"cfnmpc_multi_set_cost_scaling failed with code {rc}")

    def set_box_stages(self, lb=None, ub=None):
        """per-stage / per-input boxes [B][N][4] of the whole fleet; None, None: back to the scalar box"""
        if lb is None and ub is None:
            assert self._L.cfnmpc_multi_set_box_stages(self._h, None, None) == 0
            return
        a, p = self._p(lb, (self.B, self.N, 4)); b, q = self._p(ub, (self.B, self.N, 4))
        assert self._L.cfnmpc_multi_set_box_stages(self._h, p, q) == 0

    def init_iterate(self, mode):
        self._check(self._L.cfnmpc_multi_init_iterate(self._h, int(mode)), "cfnmpc_multi_init_iterate")

    def solve(self, n_rti=1):
        self._check(self._L.cfnmpc_multi_solve(self._h, int(n_rti)), "cfnmpc_multi_solve")

    def sync(self):
        self._check(self._L.cfnmpc_multi_sync(self._h), "cfnmpc_multi_sync")

    def eval_nlp(self):
        """cfnmpc_multi_eval_nlp: NLP cost and KKT residuals at every shard's current iterate (synchronous)"""
        self._check(self._L.cfnmpc_multi_eval_nlp(self._h), "cfnmpc_multi_eval_nlp")

    def nlp_stats(self):
        """-> (cost [B], res [B, 3] = res_stat, res_eq, res_ineq) of the last eval_nlp, host arrays in the caller's order"""
        vp = self._C.c_void_p
        cost = np.empty(self.B); res = np.empty((self.B, 3))
        self._check(self._L.cfnmpc_multi_get_nlp_stats(self._h, cost.ctypes.data_as(vp), res.ctypes.data_as(vp)), "cfnmpc_multi_get_nlp_stats")
        return cost, res

    def eval_sens_x0(self, act_tol=1e-6):
        """cfnmpc_multi_eval_sens_x0: sensitivities w.r.t. x0 of every shard's last QP (synchronous)"""
        self._check(self._L.cfnmpc_multi_eval_sens_x0(self._h, float(act_tol)), "cfnmpc_multi_eval_sens_x0")

    def sens_x0(self, stage=0, n_stages=None):
        """-> (du, dx) host arrays over the whole fleet in the caller's order, shapes as BatchSolver.sens_x0 (mixed horizons:
        stages up to the shortest horizon; du is None if the range includes the last stage)"""
        C = self._C
        Nlim = int(self.horizons.min()) if self.mixed else self.N
        ns = 1 if n_stages is None else int(n_stages)
        want_u = int(stage) + ns <= Nlim
        dx = np.empty((self.B, 13, 13) if n_stages is None else (self.B, ns, 13, 13))
        du = (np.empty((self.B, 4, 13) if n_stages is None else (self.B, ns, 4, 13))) if want_u else None
        self._check(self._L.cfnmpc_multi_get_sens_x0(self._h, int(stage), ns, None if du is None else du.ctypes.data_as(C.c_void_p),
                                                     dx.ctypes.data_as(C.c_void_p)), "cfnmpc_multi_get_sens_x0")
        return du, dx

    def eval_adjoint(self, gx=None, gu=None):
        """cfnmpc_multi_eval_adjoint: adjoint sensitivities of every shard's last QP, after eval_sens_x0 (synchronous).  Host
        arrays gx [B, n_g, 13], gu [B, n_g, 4] in the caller's order (one of them may be None), one n_g <= the shortest
        horizon"""
        if gx is None and gu is None:
            raise ValueError("gx or gu must be given")
        vp = self._C.c_void_p
        n_g = int(np.shape(gx if gx is not None else gu)[1])
        a = None if gx is None else self._p(gx, (self.B, n_g, 13))
        b = None if gu is None else self._p(gu, (self.B, n_g, 4))
        self._check(self._L.cfnmpc_multi_eval_adjoint(self._h, a[1] if a else vp(0), b[1] if b else vp(0), n_g), "cfnmpc_multi_eval_adjoint")

    def adjoint(self):
        """-> (dl_dx0 [B, 13], dl_dW [B, 17], dl_dWN [B, 13]) of the last eval_adjoint, host arrays in the caller's order"""
        vp = self._C.c_void_p
        d0, dW, dWN = np.empty((self.B, 13)), np.empty((self.B, 17)), np.empty((self.B, 13))
        self._check(self._L.cfnmpc_multi_get_adjoint(self._h, d0.ctypes.data_as(vp), dW.ctypes.data_as(vp), dWN.ctypes.data_as(vp)),
                    "cfnmpc_multi_get_adjoint")
        return d0, dW, dWN

    # ---- uncertainty propagation and bound tightening (BatchSolver.set_uncertainty ...; host arrays over the whole fleet, synchronous;
    # the full covariance is read through the shards' own solvers)
    def set_uncertainty(self, Sigma0=None, W=None):
        vp = self._C.c_void_p
        a = None if Sigma0 is None else self._p(Sigma0, (self.B, 13, 13))
        b = None if W is None else self._p(W, (self.B, 13, 13))
        self._check(self._L.cfnmpc_multi_set_uncertainty(self._h, a[1] if a else vp(0), b[1] if b else vp(0)), "cfnmpc_multi_set_uncertainty")

    def set_uncertainty_gain(self, mode="riccati", K=None):
        m = {"riccati": 0, "user": 1}.get(mode, mode)
        a = None if K is None else self._p(K, (self.B, 4, 13))
        self._check(self._L.cfnmpc_multi_set_uncertainty_gain(self._h, int(m), a[1] if a else self._C.c_void_p(0)), "cfnmpc_multi_set_uncertainty_gain")

    def eval_uncertainty(self):
        self._check(self._L.cfnmpc_multi_eval_uncertainty(self._h), "cfnmpc_multi_eval_uncertainty")

    def backoff(self):
        """-> beta [B][N][4] (mixed horizons: N the longest one, NaN behind a vehicle's own)"""
        beta = np.empty((self.B, self.N, 4))
        self._check(self._L.cfnmpc_multi_get_backoff(self._h, beta.ctypes.data_as(self._C.c_void_p)), "cfnmpc_multi_get_backoff")
        return beta

    def tighten_box(self, gamma, min_width=0.1):
        """-> n_clamped [B] (int32)"""
        n = np.empty(self.B, dtype=np.int32)
        self._check(self._L.cfnmpc_multi_tighten_box(self._h, float(gamma), float(min_width), n.ctypes.data_as(self._C.c_void_p)), "cfnmpc_multi_tighten_box")
        return n

    def get_u(self, stage):
        u = np.empty((self.B, 4))
        self._check(self._L.cfnmpc_multi_get_u(self._h, int(stage), u.ctypes.data_as(self._C.c_void_p)), "cfnmpc_multi_get_u")
        return u

    def get_x(self, stage):
        x = np.empty((self.B, 13))
        self._check(self._L.cfnmpc_multi_get_x(self._h, int(stage), x.ctypes.data_as(self._C.c_void_p)), "cfnmpc_multi_get_x")
        return x

    def get_cmd(self):
        c = np.empty((self.B, 4)); mv = np.empty((self.B, 4), dtype=np.int32)
        self._check(self._L.cfnmpc_multi_get_cmd(self._h, c.ctypes.data_as(self._C.c_void_p), mv.ctypes.data_as(self._C.c_void_p)), "cfnmpc_multi_get_cmd")
        return c, mv

    def stats(self):
        st = np.empty(self.B, dtype=np.int32); it = np.empty(self.B, dtype=np.int32); rs = np.empty(self.B)
        vp = self._C.c_void_p
        self._check(self._L.cfnmpc_multi_get_stats(self._h, st.ctypes.data_as(vp), it.ctypes.data_as(vp), rs.ctypes.data_as(vp)), "cfnmpc_multi_get_stats")
        return st, it, rs
