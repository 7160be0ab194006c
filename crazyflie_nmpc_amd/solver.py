"""Batch solver object over the C-ABI (include/cfnmpc.h).

Mirrors, for B instances, the calls the reference node makes on its single generated solver
(crazyflie_controller/src/acados_mpc.cpp): acados_create (:225) -> BatchSolver(...);
lbx/ubx (:581-582) -> set_x0; yref (:590-594) -> set_yref; acados_solve (:611) -> solve;
ocp_nlp_out_get u/x (:619-625) -> get_u / get_x; status -> stats.

Arrays may be numpy (host, copied) or torch CUDA/HIP tensors (device pointers are handed to
the library, the work is enqueued on torch's current stream).  torch is plumbing only.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import NU, NX, NY, Opts

INIT_ACADOS, INIT_HOVER = 0, 1
SQP_MODES = ("full_step", "merit_backtracking")   # CFNMPC_SQP_FULL_STEP, CFNMPC_SQP_MERIT_BACKTRACKING


def _sqp_mode(mode):
    """globalisation mode by name (or by its number, passed through for the library to judge)"""
    return SQP_MODES.index(mode) if mode in SQP_MODES else int(mode)

# per-instance model parameters (include/cfnmpc.h: cfnmpc_set_model_params), export_ode_model.py:33-42 order, l = arm length
NP = 8
PARAM_NAMES = ("g0", "mq", "Ixx", "Iyy", "Izz", "Cd", "Ct", "l")
NOMINAL_PARAMS = np.array([9.8066, 33e-3, 1.395e-5, 1.395e-5, 2.173e-5, 7.9379e-06, 3.25e-4, 0.0325])
# per-instance disturbance rows (include/cfnmpc.h: cfnmpc_set_disturbance): world-frame acceleration, body-frame angular acceleration
ND = 6
DIST_NAMES = ("ax", "ay", "az", "alx", "aly", "alz")


def hover_speed(params):
    """Per-row hover speed sqrt(mq g0 / (4 Ct)) in kRPM of parameter rows [..., NP] (the input part of yref)."""
    p = np.asarray(params, dtype=np.float64)
    return np.sqrt((p[..., 1] * p[..., 0]) / (4 * p[..., 6]))


class CfnmpcError(RuntimeError):
    pass


def _check(rc, what):
    if rc != 0:
        raise CfnmpcError(f"{what} failed with code {rc}")


def default_opts(**kw) -> Opts:
    o = Opts()
    _check(_lib.lib().cfnmpc_default_opts_v(C.byref(o), C.sizeof(o)), "cfnmpc_default_opts_v")
    for k, v in kw.items():
        if k in ("W", "WN"):
            arr = getattr(o, k)
            for i, x in enumerate(v):
                arr[i] = float(x)
        else:
            setattr(o, k, v)
    return o


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def _stream_ptr(a):
    import torch
    return C.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)


def _torch_device():
    """torch's current HIP device if its runtime is up (a solver lives on the device current at its creation), else None"""
    import sys
    torch = sys.modules.get("torch")
    try:
        if torch is not None and torch.cuda.is_available() and torch.cuda.is_initialized():
            return int(torch.cuda.current_device())
    except Exception:
        pass
    return None


def _launch_stream(stream, device=None):
    """Stream of a launch call: the caller's raw hipStream_t, else torch's CURRENT stream on the solver's device (the one
    the device-tensor setters enqueue on: a `with torch.cuda.stream(s):` block keeps setters and solve in one queue),
    else the default stream."""
    if stream:
        return C.c_void_p(stream)
    if device is not None:
        import sys
        torch = sys.modules.get("torch")
        try:
            if torch is not None and torch.cuda.is_initialized():
                return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        except Exception:
            pass
    return C.c_void_p(0)


def _torch_like(a, shape):
    import torch
    return torch.empty(shape, dtype=a.dtype, device=a.device)


def _arg(a, shape, dtype=np.float64, device=None):
    """-> (pointer, on_device, stream, keepalive).  Host arrays travel on the stream the launch calls use (torch's CURRENT
    stream on the solver's device, _launch_stream): inside `with torch.cuda.stream(s):` a numpy getter then waits for the
    solve enqueued on s, and a numpy setter cannot overtake it -- pool streams do not synchronise with stream 0."""
    if _is_torch(a):
        import torch
        want = {np.float64: torch.float64, np.int32: torch.int32}[dtype]
        if not a.is_cuda or a.dtype != want or not a.is_contiguous() or tuple(a.shape) != tuple(shape):
            raise ValueError(f"expected contiguous device tensor {shape} {want}, got {tuple(a.shape)} {a.dtype}")
        return C.c_void_p(a.data_ptr()), 1, _stream_ptr(a), a
    arr = np.ascontiguousarray(a, dtype=dtype)
    if arr.shape != tuple(shape):
        raise ValueError(f"expected shape {shape}, got {arr.shape}")
    return arr.ctypes.data_as(C.c_void_p), 0, _launch_stream(None, device), arr



def sens_x0_call(obj, N, fn, what, stage, n_stages, out_u, out_x):
    """shared body of BatchSolver.sens_x0 / MixedHorizonFleet.sens_x0 (fn: the C getter; N: the last stage of the range)"""
    ns = 1 if n_stages is None else int(n_stages)
    stage = int(stage)
    want_u = stage + ns <= N
    su = (obj.B, 4, NX) if n_stages is None else (obj.B, ns, 4, NX)
    sx = (obj.B, NX, NX) if n_stages is None else (obj.B, ns, NX, NX)
    if out_x is None:
        out_x = _torch_like(out_u, sx) if (out_u is not None and _is_torch(out_u)) else np.empty(sx)
    if want_u and out_u is None:
        out_u = _torch_like(out_x, su) if _is_torch(out_x) else np.empty(su)
    px, dev, st, _kx = _arg(out_x, sx, device=obj._device)
    pu = C.c_void_p(0)
    if want_u:
        pu, devu, _s, _ku = _arg(out_u, su, device=obj._device)
        if devu != dev:
            raise ValueError("out_u and out_x must both be host arrays or both device tensors")
    else:
        out_u = None
    _check(fn(obj._h, stage, ns, pu, px, dev, st), what)
    return out_u, out_x

UNC_GAIN_RICCATI, UNC_GAIN_USER = 0, 1


class UncertaintyCalls:
    """Uncertainty propagation and robust input-bound tightening (include/cfnmpc.h: cfnmpc_set_uncertainty ...; DESIGN.md section
    5.21), shared by BatchSolver and MixedHorizonFleet: _unc_pre is the C prefix, _unc_N the stage stride of beta (N, or the
    fleet's longest horizon; the covariance getter of a fleet reaches the shortest horizon, checked by the library)."""

    def _unc_fn(self, name):
        return getattr(self._L, self._unc_pre + name), self._unc_pre + name

    def set_uncertainty(self, Sigma0=None, W=None, stream=None):
        """Sigma0 [B][13][13]: covariance of the state estimate at stage 0; W [B][13][13]: covariance added per shooting
        interval (public state order; numpy or device tensors; None: zero).  Host arrays must be finite, symmetric and have a
        non-negative diagonal."""
        fn, what = self._unc_fn("set_uncertainty")
        if Sigma0 is not None and W is not None and _is_torch(Sigma0) != _is_torch(W):
            raise ValueError("Sigma0 and W must both be host arrays or both device tensors")
        ps, pw, dev, st, keep = None, None, 0, _launch_stream(stream, self._device), []
        if Sigma0 is not None:
            ps, dev, st, k = _arg(Sigma0, (self.B, NX, NX), device=self._device); keep.append(k)
        if W is not None:
            pw, dev, st, k = _arg(W, (self.B, NX, NX), device=self._device); keep.append(k)
        if stream:
            st = C.c_void_p(stream)
        _check(fn(self._h, ps, pw, dev, st), what)

    def set_uncertainty_gain(self, mode="riccati", K=None, stream=None):
        """Feedback gain of the propagation, in du = -K dx: "riccati" (the gains of the last solve's start solve) or "user"
        with one constant K [B][4][13] per instance (acados zoRO's fdbk_K_mat)."""
        fn, what = self._unc_fn("set_uncertainty_gain")
        m = {"riccati": UNC_GAIN_RICCATI, "user": UNC_GAIN_USER}.get(mode, mode)
        pk, dev, st = None, 0, _launch_stream(stream, self._device)
        if K is not None:
            pk, dev, st, _k = _arg(K, (self.B, NU, NX), device=self._device)
            if stream:
                st = C.c_void_p(stream)
        _check(fn(self._h, int(m), pk, dev, st), what)

    def eval_uncertainty(self, stream=None):
        """Propagates the covariance through the closed-loop linearisation of the last QP and keeps the backoffs (backoff())."""
        fn, what = self._unc_fn("eval_uncertainty")
        _check(fn(self._h, _launch_stream(stream, self._device)), what)

    def backoff(self, out=None):
        """-> beta [B][N][4]: 1-sigma standard deviation of the feedback's input correction (a fleet: [B][Nmax][4], NaN behind
        a vehicle's own horizon)"""
        fn, what = self._unc_fn("get_backoff")
        shape = (self.B, self._unc_N, NU)
        if out is None:
            out = np.empty(shape)
        p, dev, st, _k = _arg(out, shape, device=self._device)
        _check(fn(self._h, p, dev, st), what)
        return out

    def uncertainty(self, stage=0, n_stages=None, want_sigma=True, want_std=True):
        """-> (Sigma, std_x): the covariance [B][n][13][13] and the square roots of its diagonal [B][n][13] for the stages
        [stage, stage + n_stages) (n_stages = None: that one stage, without the stage axis); host arrays, None where not wanted"""
        fn, what = self._unc_fn("get_uncertainty")
        ns = 1 if n_stages is None else int(n_stages)
        sg = np.empty((self.B, ns, NX, NX)) if want_sigma else None
        sd = np.empty((self.B, ns, NX)) if want_std else None
        _check(fn(self._h, int(stage), ns, None if sg is None else sg.ctypes.data_as(C.c_void_p),
                  None if sd is None else sd.ctypes.data_as(C.c_void_p), 0, _launch_stream(None, self._device)), what)
        if n_stages is None:
            sg = None if sg is None else sg[:, 0]
            sd = None if sd is None else sd[:, 0]
        return sg, sd

    def tighten_box(self, gamma, min_width=0.1, stream=None):
        """lb' = lb + t, ub' = ub - t with t = min(gamma beta, (1 - min_width)(ub - lb) / 2) on the nominal box, in force from
        the next solve on; gamma = 0 puts the nominal box back.  -> n_clamped [B] (int32)"""
        fn, what = self._unc_fn("tighten_box")
        n = np.empty(self.B, dtype=np.int32)
        _check(fn(self._h, float(gamma), float(min_width), n.ctypes.data_as(C.c_void_p), 0, _launch_stream(stream, self._device)), what)
        return n


POLY_NC, NPLACE, NFLAT = 33, 6, 13
POLY_LOOP, POLY_KINEMATIC = 1, 2


def _poly_library_args(tables):
    """list of [n_i][33] tables (or None / empty: clear) -> (pieces pointer, first pointer, n_traj, keepalive)"""
    from .trajectories import poly_library
    if not tables:
        return None, None, 0, None
    pieces, first = poly_library(tables)
    return pieces.ctypes.data_as(C.c_void_p), first.ctypes.data_as(C.c_void_p), len(first) - 1, (pieces, first)


class PolyCalls:
    """Device-side polynomial trajectory references (include/cfnmpc.h: cfnmpc_set_poly_library ...), shared
    by BatchSolver and MixedHorizonFleet (_unc_pre is the C prefix).  The host twin of the kernel is trajectories.poly_rows."""

    def set_poly_library(self, tables, stream=None):
        """tables: list of [n_i][33] coefficient tables in the crazyflie_demo CSV format (trajectories.load_poly_csv); the id of
        a trajectory is its place in the list.  None or an empty list clears the library."""
        pp, pf, n, _keep = _poly_library_args(tables)
        _check(getattr(self._L, self._unc_pre + "set_poly_library")(self._h, pp, pf, n, _launch_stream(stream, self._device)),
               self._unc_pre + "set_poly_library")

    def set_poly_assignment(self, traj, place=None, stream=None):
        """traj [B] int32: trajectory id of every vehicle, -1 = none (its reference rows are left alone); place [B][6] =
        t_start [s], time_scale, ox, oy, oz [m], yaw0 [rad], None: [0, 1, 0, 0, 0, 0] everywhere.  numpy arrays are validated
        by the library; torch device tensors are taken as they are."""
        if place is not None and _is_torch(traj) != _is_torch(place):
            raise ValueError("traj and place must both be host arrays or both device tensors")
        pt, dev, st, _k = _arg(traj, (self.B,), dtype=np.int32, device=self._device)
        pl, _k2 = None, None
        if place is not None:
            pl, _d, _s, _k2 = _arg(place, (self.B, NPLACE), device=self._device)
        if stream:
            st = C.c_void_p(stream)
        _check(getattr(self._L, self._unc_pre + "set_poly_assignment")(self._h, pt, pl, dev, st), self._unc_pre + "set_poly_assignment")

    def set_yref_poly(self, t, flags=0, stream=None):
        """Writes the reference window of every vehicle with a trajectory, rows k = 0 .. N at the fleet times t + k dt, on the
        device; flags: POLY_LOOP | POLY_KINEMATIC.  Asynchronous."""
        _check(getattr(self._L, self._unc_pre + "set_yref_poly")(self._h, float(t), int(flags), _launch_stream(stream, self._device)),
               self._unc_pre + "set_yref_poly")


class BatchSolver(UncertaintyCalls, PolyCalls):
    _unc_pre = "cfnmpc_"
    _unc_N = property(lambda self: self.N)

    def __init__(self, batch: int, opts: Opts | None = None, **kw):
        self._L = _lib.lib()
        self.opts = opts if opts is not None else default_opts(**kw)
        self.B = int(batch)
        self.N = int(self.opts.N)
        h = C.c_void_p()
        _check(self._L.cfnmpc_create(C.byref(h), self.B, C.byref(self.opts)), "cfnmpc_create")
        self._h = h
        self._device = _torch_device()

    def close(self):
        if getattr(self, "_h", None):
            self._L.cfnmpc_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def workspace_bytes(self):
        return int(self._L.cfnmpc_workspace_bytes(self._h))

    # ---- inputs
    def set_x0(self, x0):
        p, dev, st, _k = _arg(x0, (self.B, NX), device=self._device)
        _check(self._L.cfnmpc_set_x0(self._h, p, dev, st), "cfnmpc_set_x0")

    def set_yref(self, yref, yref_e):
        p, dev, st, _k = _arg(yref, (self.B, self.N, NY), device=self._device)
        pe, deve, _st, _k2 = _arg(yref_e, (self.B, NX), device=self._device)
        if dev != deve:
            raise ValueError("yref and yref_e must live on the same side")
        _check(self._L.cfnmpc_set_yref(self._h, p, pe, dev, st), "cfnmpc_set_yref")

    def yref(self):
        """-> (yref [B][N][17], yref_e [B][13]): the reference windows in force, public order (cfnmpc_get_yref)"""
        y = np.empty((self.B, self.N, NY)); ye = np.empty((self.B, NX))
        _check(self._L.cfnmpc_get_yref(self._h, y.ctypes.data_as(C.c_void_p), ye.ctypes.data_as(C.c_void_p), 0,
                                       _launch_stream(None, self._device)), "cfnmpc_get_yref")
        return y, ye

    def eval_poly(self, t, n_stages, flags=0, want_flat=True, want_rows=True):
        """The evaluation of set_yref_poly for rows k = 0 .. n_stages - 1 without touching the references -> (flat
        [B][n_stages][13] = pos, vel, acc, yaw, omega as the reference's evaluator returns them, rows [B][n_stages][17]); host
        arrays, None where not wanted; NaN for vehicles without a trajectory."""
        fl = np.empty((self.B, int(n_stages), NFLAT)) if want_flat else None
        rw = np.empty((self.B, int(n_stages), NY)) if want_rows else None
        _check(self._L.cfnmpc_eval_poly(self._h, float(t), int(n_stages), int(flags), None if fl is None else fl.ctypes.data_as(C.c_void_p),
                                        None if rw is None else rw.ctypes.data_as(C.c_void_p), 0, _launch_stream(None, self._device)),
               "cfnmpc_eval_poly")
        return fl, rw

    def set_yref_windows(self, traj, mode, it, des_xyz, uss):
        """Device-side reference windows (NMPC::iteration state machine); all arguments are torch
        device tensors: traj [n_rows][17] float64 or None, mode / it [B] int32 (updated in place),
        des_xyz [B][3] float64."""
        import torch
        assert mode.is_cuda and it.is_cuda and des_xyz.is_cuda and mode.dtype == torch.int32 and it.dtype == torch.int32
        assert tuple(des_xyz.shape) == (self.B, 3) and des_xyz.is_contiguous() and des_xyz.dtype == torch.float64
        n_rows, tp = 0, None
        if traj is not None:
            assert traj.is_cuda and traj.dtype == torch.float64 and traj.is_contiguous() and traj.shape[1] == 17
            n_rows, tp = int(traj.shape[0]), C.c_void_p(traj.data_ptr())
        _check(self._L.cfnmpc_set_yref_windows(self._h, tp, n_rows, C.c_void_p(mode.data_ptr()), C.c_void_p(it.data_ptr()),
                                               C.c_void_p(des_xyz.data_ptr()), float(uss), _stream_ptr(mode)),
               "cfnmpc_set_yref_windows")

    def set_weights(self, W=None, WN=None):
        w = None if W is None else np.ascontiguousarray(W, dtype=np.float64)
        wn = None if WN is None else np.ascontiguousarray(WN, dtype=np.float64)
        _check(self._L.cfnmpc_set_weights(self._h, None if w is None else w.ctypes.data_as(C.c_void_p),
                                          None if wn is None else wn.ctypes.data_as(C.c_void_p)), "cfnmpc_set_weights")

    def set_box(self, u_min, u_max):
        _check(self._L.cfnmpc_set_box(self._h, float(u_min), float(u_max)), "cfnmpc_set_box")

    def set_erk_steps(self, n):
        """RK4 steps of dt / n per shooting interval (acados sim_method_num_steps), 1 <= n <= 8; default 1."""
        _check(self._L.cfnmpc_set_erk_steps(self._h, int(n)), "cfnmpc_set_erk_steps")

    @property
    def erk_steps(self):
        return int(self._L.cfnmpc_erk_steps(self._h))

    def set_cost_scaling(self, stage=1.0, terminal=1.0):
        """Effective weights stage * W (stages 0..N-1) and terminal * WN; newer acados uses (dt, 1)."""
        _check(self._L.cfnmpc_set_cost_scaling(self._h, float(stage), float(terminal)), "cfnmpc_set_cost_scaling")

    def set_model_params(self, p=None):
        """Per-instance model parameters [B][NP] (PARAM_NAMES order; numpy or a device tensor); None: back to the
        nominal model folded into the default kernels.  Every entry finite and > 0."""
        if p is None:
            _check(self._L.cfnmpc_set_model_params(self._h, None, 0, _launch_stream(None, self._device)), "cfnmpc_set_model_params")
            return
        pp, dev, st, _k = _arg(p, (self.B, NP), device=self._device)
        _check(self._L.cfnmpc_set_model_params(self._h, pp, dev, st), "cfnmpc_set_model_params")

    def model_params(self):
        """-> [B][NP] rows in force (the nominal row everywhere while none are set)"""
        out = np.empty((self.B, NP))
        _check(self._L.cfnmpc_get_model_params(self._h, out.ctypes.data_as(C.c_void_p), 0, None), "cfnmpc_get_model_params")
        return out

    def set_disturbance(self, d=None, stream=None):
        """Per-instance disturbance rows [B][ND] (DIST_NAMES order: a world-frame acceleration [m/s^2] and a body-frame angular
        acceleration [rad/s^2]; numpy or a device tensor); None: no disturbance.  Cheap enough for every control step: a device
        tensor is taken without a copy to the host or a synchronisation, and captured step graphs replay with the new values.
        stream: a raw hipStream_t instead of torch's current stream."""
        if d is None:
            _check(self._L.cfnmpc_set_disturbance(self._h, None, 0, _launch_stream(stream, self._device)), "cfnmpc_set_disturbance")
            return
        pd, dev, st, _k = _arg(d, (self.B, ND), device=self._device)
        if stream:
            st = C.c_void_p(stream)
        _check(self._L.cfnmpc_set_disturbance(self._h, pd, dev, st), "cfnmpc_set_disturbance")

    def disturbance(self):
        """-> [B][ND] rows in force (zeros while none are set)"""
        out = np.empty((self.B, ND))
        _check(self._L.cfnmpc_get_disturbance(self._h, out.ctypes.data_as(C.c_void_p), 0, _launch_stream(None, self._device)),
               "cfnmpc_get_disturbance")
        return out

    def set_weights_batch(self, W=None, WN=None):
        """Per-instance cost weights: W [B][17], WN [B][13] (numpy or device tensors; external order, unscaled -- the effective
        weights are the cost scaling's factors times the rows).  None, None: back to the uniform weights; one None: that
        part keeps what every row has.  Every entry finite, state / terminal weights >= 0, input weights > 0."""
        if W is None and WN is None:
            _check(self._L.cfnmpc_set_weights_batch(self._h, None, None, 0, _launch_stream(None, self._device)), "cfnmpc_set_weights_batch")
            return
        if W is not None and WN is not None and _is_torch(W) != _is_torch(WN):
            raise ValueError("W and WN must both be host arrays or both device tensors")
        pw, pn, dev, st, keep = None, None, 0, None, []
        if W is not None:
            pw, dev, st, k = _arg(W, (self.B, NY), device=self._device); keep.append(k)
        if WN is not None:
            pn, dev, st, k = _arg(WN, (self.B, NX), device=self._device); keep.append(k)
        _check(self._L.cfnmpc_set_weights_batch(self._h, pw, pn, dev, st), "cfnmpc_set_weights_batch")

    def weights_batch(self):
        """-> (W [B][17], WN [B][13]): the unscaled rows in force (the uniform weights everywhere while none are set)"""
        W, WN = np.empty((self.B, NY)), np.empty((self.B, NX))
        _check(self._L.cfnmpc_get_weights_batch(self._h, W.ctypes.data_as(C.c_void_p), WN.ctypes.data_as(C.c_void_p), 0, None),
               "cfnmpc_get_weights_batch")
        return W, WN

    def set_box_stages(self, lb=None, ub=None):
        """Per-stage, per-input box [B][N][4] (acados' "lbu" / "ubu" on individual stages); None, None: back to
        the scalar box."""
        if lb is None and ub is None:
            _check(self._L.cfnmpc_set_box_stages(self._h, None, None, 0, _launch_stream(None, self._device)), "cfnmpc_set_box_stages")
            return
        p, dev, st, _k = _arg(lb, (self.B, self.N, NU), device=self._device)
        pu, devu, _s, _k2 = _arg(ub, (self.B, self.N, NU), device=self._device)
        assert dev == devu
        _check(self._L.cfnmpc_set_box_stages(self._h, p, pu, dev, st), "cfnmpc_set_box_stages")

    def init_iterate(self, mode=INIT_ACADOS, stream=None):
        _check(self._L.cfnmpc_init_iterate(self._h, mode, _launch_stream(stream, self._device)), "cfnmpc_init_iterate")

    def set_iterate(self, x, u):
        p, dev, st, _k = _arg(x, (self.B, self.N + 1, NX), device=self._device)
        pu, devu, _s, _k2 = _arg(u, (self.B, self.N, NU), device=self._device)
        assert dev == devu
        _check(self._L.cfnmpc_set_iterate(self._h, p, pu, dev, st), "cfnmpc_set_iterate")

    # ---- solve
    def solve(self, n_rti=1, stream=None):
        """acados_solve() for the batch; `stream` is a raw hipStream_t (int) or None = default."""
        _check(self._L.cfnmpc_solve(self._h, int(n_rti), _launch_stream(stream, self._device)), "cfnmpc_solve")

    def solve_sqp(self, max_iter=100, tol_step=1e-6, tol_eq=1e-6, tol_ineq=1e-6, stream=None):
        """Full SQP solve (acados' nlp_solver_type 'SQP'; include/cfnmpc.h: cfnmpc_solve_sqp): RTI steps with x0, yref,
        weights and boxes fixed until every instance has converged (res_step <= tol_step, res_eq <= tol_eq,
        res_ineq <= tol_ineq), failed (QP status 4) or max_iter steps have run.  Defaults: acados' SQP defaults.
        Synchronises the stream.  Returns the number of iterations run; per instance: sqp_stats()."""
        n = C.c_int(0)
        _check(self._L.cfnmpc_solve_sqp(self._h, int(max_iter), float(tol_step), float(tol_eq), float(tol_ineq), C.byref(n),
                                        _launch_stream(stream, self._device)), "cfnmpc_solve_sqp")
        return n.value

    def sqp_stats(self):
        """-> (status [B] (0 converged, 2 max. iterations, 4 QP failure), sqp_iter [B], res [B, 3] = res_step, res_eq,
        res_ineq) of the last solve_sqp"""
        st = np.empty(self.B, dtype=np.int32); it = np.empty(self.B, dtype=np.int32); rs = np.empty((self.B, 3))
        _check(self._L.cfnmpc_get_sqp_stats(self._h, st.ctypes.data_as(C.c_void_p), it.ctypes.data_as(C.c_void_p),
                                            rs.ctypes.data_as(C.c_void_p), 0, _launch_stream(None, self._device)), "cfnmpc_get_sqp_stats")
        return st, it, rs

    def set_sqp_globalization(self, mode="merit_backtracking", eta=0, reduction=0, alpha_min=0):
        """Globalisation of solve_sqp (include/cfnmpc.h: cfnmpc_set_sqp_globalization): "full_step" (the default of a new solver)
        or "merit_backtracking", the l1 merit line search along every iteration's QP step; eta, reduction, alpha_min = 0 select
        the defaults 1e-4, 0.5, 2**-10.  Stays with the solver; solve() ignores it."""
        _check(self._L.cfnmpc_set_sqp_globalization(self._h, _sqp_mode(mode), float(eta), float(reduction), float(alpha_min)),
               "cfnmpc_set_sqp_globalization")

    def sqp_globalization(self):
        """-> (mode, eta, reduction, alpha_min) in force"""
        m = C.c_int(0); e = C.c_double(0); r = C.c_double(0); a = C.c_double(0)
        _check(self._L.cfnmpc_get_sqp_globalization(self._h, C.byref(m), C.byref(e), C.byref(r), C.byref(a)), "cfnmpc_get_sqp_globalization")
        return SQP_MODES[m.value], e.value, r.value, a.value

    def sqp_ls_stats(self):
        """-> (alpha [B], mu [B], n_short [B], n_fail [B]) of the last solve_sqp: step length of the last executed iteration,
        penalty, iterations with alpha < 1, iterations without an accepted trial"""
        al = np.empty(self.B); mu = np.empty(self.B); ns = np.empty(self.B, dtype=np.int32); nf = np.empty(self.B, dtype=np.int32)
        _check(self._L.cfnmpc_get_sqp_ls_stats(self._h, al.ctypes.data_as(C.c_void_p), mu.ctypes.data_as(C.c_void_p),
                                               ns.ctypes.data_as(C.c_void_p), nf.ctypes.data_as(C.c_void_p), 0,
                                               _launch_stream(None, self._device)), "cfnmpc_get_sqp_ls_stats")
        return al, mu, ns, nf

    def eval_nlp(self, keep_multipliers=False, stream=None):
        """NLP cost, KKT residuals and (keep_multipliers) costates / reduced gradient at the current iterate, from the data in
        force (include/cfnmpc.h: cfnmpc_eval_nlp); needs no solve and disturbs none.  Asynchronous on `stream`.  Read with
        nlp_stats() / nlp_multipliers()."""
        _check(self._L.cfnmpc_eval_nlp(self._h, 1 if keep_multipliers else 0, _launch_stream(stream, self._device)), "cfnmpc_eval_nlp")

    def nlp_stats(self, out=None):
        """-> (cost [B], res [B, 3] = res_stat, res_eq, res_ineq) of the last eval_nlp; `out` = two torch device tensors
        (float64) to keep them on the device (filled on torch's current stream)"""
        if out is not None:
            pc, dev, strm, _a = _arg(out[0], (self.B,), device=self._device)
            pr, _d, _s, _b = _arg(out[1], (self.B, 3), device=self._device)
            _check(self._L.cfnmpc_get_nlp_stats(self._h, pc, pr, dev, strm), "cfnmpc_get_nlp_stats")
            return out
        cost = np.empty(self.B); res = np.empty((self.B, 3))
        _check(self._L.cfnmpc_get_nlp_stats(self._h, cost.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p), 0,
                                            _launch_stream(None, self._device)), "cfnmpc_get_nlp_stats")
        return cost, res

    def nlp_multipliers(self):
        """-> (pi [B, N + 1, 13] costates in the public state order, gu [B, N, 4] reduced gradient dJ/du_k) of the last
        eval_nlp(keep_multipliers=True)"""
        pi = np.empty((self.B, self.N + 1, NX)); gu = np.empty((self.B, self.N, NU))
        _check(self._L.cfnmpc_get_nlp_multipliers(self._h, pi.ctypes.data_as(C.c_void_p), gu.ctypes.data_as(C.c_void_p), 0,
                                                  _launch_stream(None, self._device)), "cfnmpc_get_nlp_multipliers")
        return pi, gu

    def eval_sens_x0(self, act_tol=1e-6, stream=None):
        """Sensitivities of the last QP's solution with respect to x0 (include/cfnmpc.h: cfnmpc_eval_sens_x0): the active set
        of the current iterate (inputs within act_tol of a bound) and the masked Riccati gains.  Read with sens_x0()."""
        _check(self._L.cfnmpc_eval_sens_x0(self._h, float(act_tol), _launch_stream(stream, self._device)), "cfnmpc_eval_sens_x0")

    def sens_x0(self, stage=0, n_stages=None, out_u=None, out_x=None):
        """-> (du, dx): du_k/dx0 and dx_k/dx0 in the public state order, after eval_sens_x0.  n_stages = None: stage `stage`
        alone, du [B, 4, 13] and dx [B, 13, 13]; else stages [stage, stage + n_stages), du [B, n_stages, 4, 13] and
        dx [B, n_stages, 13, 13].  du is None if the range includes stage N.  out_u / out_x: numpy arrays or torch device
        tensors of those shapes (device tensors are filled on torch's current stream)."""
        return sens_x0_call(self, self.N, self._L.cfnmpc_get_sens_x0, "cfnmpc_get_sens_x0", stage, n_stages, out_u, out_x)

    def sens_active(self):
        """-> int8 [B, N, 4]: the active set of the last eval_sens_x0 (0 free, -1 lower bound, +1 upper bound)"""
        a = np.empty((self.B, self.N, NU), dtype=np.int8)
        _check(self._L.cfnmpc_get_sens_active(self._h, a.ctypes.data_as(C.c_void_p), 0, _launch_stream(None, self._device)),
               "cfnmpc_get_sens_active")
        return a

    def eval_adjoint(self, gx=None, gu=None, stream=None):
        """Adjoint sensitivities of the last QP (include/cfnmpc.h: cfnmpc_eval_adjoint), after eval_sens_x0: gx [B, n_gx, 13] =
        dl/dx_k for the stages k < n_gx <= N + 1, gu [B, n_gu, 4] = dl/du_k for k < n_gu <= N (numpy or torch device tensors;
        None or stages behind: zero).  Read with adjoint() / adjoint_cost()."""
        if gx is not None and gu is not None and _is_torch(gx) != _is_torch(gu):
            raise ValueError("gx and gu must both be host arrays or both device tensors")
        px, pu, nx, nu, dev, st, keep = None, None, 0, 0, 0, _launch_stream(stream, self._device), []
        if gx is not None:
            nx = int(gx.shape[1]) if len(gx.shape) == 3 else -1
            px, dev, st, k = _arg(gx, (self.B, nx, NX), device=self._device); keep.append(k)
        if gu is not None:
            nu = int(gu.shape[1]) if len(gu.shape) == 3 else -1
            pu, dev, st, k = _arg(gu, (self.B, nu, NU), device=self._device); keep.append(k)
        if stream:
            st = C.c_void_p(stream)
        _check(self._L.cfnmpc_eval_adjoint(self._h, px, nx, pu, nu, dev, st), "cfnmpc_eval_adjoint")

    def _adjoint_get(self, fn, what, shapes, out):
        """shared body of adjoint() / adjoint_cost(): out = None -> new host arrays; else a tuple of numpy arrays or torch device
        tensors of those shapes (None entries are not read; device tensors are filled on torch's current stream)"""
        if out is None:
            out = tuple(np.empty(sh) for sh in shapes)
        if len(out) != len(shapes):
            raise ValueError(f"expected {len(shapes)} outputs")
        ptrs, dev, st, keep = [], None, _launch_stream(None, self._device), []
        for o, sh in zip(out, shapes):
            if o is None:
                ptrs.append(None)
                continue
            if not _is_torch(o) and not (isinstance(o, np.ndarray) and o.dtype == np.float64 and o.flags.c_contiguous):
                raise ValueError("outputs must be contiguous float64 numpy arrays or torch device tensors")
            p, d, s_, k = _arg(o, sh, device=self._device)
            if dev is not None and d != dev:
                raise ValueError("outputs must all be host arrays or all device tensors")
            dev, st = d, s_
            ptrs.append(p); keep.append(k)
        _check(fn(self._h, *ptrs, dev or 0, st), what)
        return tuple(out)

    def adjoint(self, out=None):
        """-> (dl_dx0 [B, 13], dl_dq [B, N + 1, 13], dl_dr [B, N, 4], dl_db [B, N, 13], dl_dbox [B, N, 4]) of the last
        eval_adjoint: the gradients with respect to x0, the QP's linear cost terms, its defects and the bounds of the active
        inputs (public state order)."""
        B, N = self.B, self.N
        return self._adjoint_get(self._L.cfnmpc_get_adjoint, "cfnmpc_get_adjoint",
                                 ((B, NX), (B, N + 1, NX), (B, N, NU), (B, N, NX), (B, N, NU)), out)

    def adjoint_cost(self, out=None):
        """-> (dl_dW [B, 17], dl_dWN [B, 13], dl_dyref [B, N, 17], dl_dyref_e [B, 13]) of the last eval_adjoint; the weight
        gradients are with respect to the unscaled rows of weights_batch()."""
        B, N = self.B, self.N
        return self._adjoint_get(self._L.cfnmpc_get_adjoint_cost, "cfnmpc_get_adjoint_cost",
                                 ((B, NY), (B, NX), (B, N, NY), (B, NX)), out)

    def step_host(self, x0, yref, yref_e, stream=None):
        """cfnmpc_step_host: host arrays in (x0 [B,13], yref [B,N,17], yref_e [B,13]), one RTI step,
        host arrays out -> (u [B,N,4], x [B,N+1,13], status, qp_iter, res); one synchronisation."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64); yref = np.ascontiguousarray(yref, dtype=np.float64)
        yref_e = np.ascontiguousarray(yref_e, dtype=np.float64)
        assert x0.shape == (self.B, NX) and yref.shape == (self.B, self.N, NY) and yref_e.shape == (self.B, NX)
        u = np.empty((self.B, self.N, NU)); x = np.empty((self.B, self.N + 1, NX))
        st = np.empty(self.B, dtype=np.int32); it = np.empty(self.B, dtype=np.int32); rs = np.empty(self.B)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        _check(self._L.cfnmpc_step_host(self._h, vp(x0), vp(yref), vp(yref_e), vp(u), vp(x), vp(st), vp(it), vp(rs),
                                        _launch_stream(stream, self._device)), "cfnmpc_step_host")
        return u, x, st, it, rs

    def set_profiling(self, enable=True):
        _check(self._L.cfnmpc_set_profiling(self._h, int(bool(enable))), "cfnmpc_set_profiling")

    def get_profile(self):
        """-> (ms_linearise, ms_qp, n_steps): average kernel durations since the last call."""
        a = C.c_double(0); b = C.c_double(0); n = C.c_int(0)
        _check(self._L.cfnmpc_get_profile(self._h, C.byref(a), C.byref(b), C.byref(n)), "cfnmpc_get_profile")
        return a.value, b.value, n.value

    def get_profile_kernels(self):
        """-> (ms[6], n_steps): linearise | factor | forward | compaction | active set | interior point (averages)."""
        ms = (C.c_double * 6)(); n = C.c_int(0)
        _check(self._L.cfnmpc_get_profile_kernels(self._h, ms, C.byref(n)), "cfnmpc_get_profile_kernels")
        return [float(v) for v in ms], n.value

    def get_profile_steps(self, max_steps=4096):
        """-> array [n_steps][6]: the six kernel-group durations of every timed step (ms), not averaged."""
        ms = np.zeros((int(max_steps), 6)); n = C.c_int(0)
        _check(self._L.cfnmpc_get_profile_steps(self._h, ms.ctypes.data_as(C.c_void_p), int(max_steps), C.byref(n)), "cfnmpc_get_profile_steps")
        return ms[:n.value].copy()

    def linearise_only(self, stream=None):
        _check(self._L.cfnmpc_debug_linearise(self._h, _launch_stream(stream, self._device)), "cfnmpc_debug_linearise")

    def start_factor(self, mode, reps=1, stream=None):
        """Backward half of the start solve only (development / parity tests): mode 1 = k_linearise + k_factor,
        2 = the fused k_linfactor.  Returns the average duration of one repetition [ms]."""
        ms = C.c_double(0.0)
        _check(self._L.cfnmpc_debug_start_factor(self._h, int(mode), int(reps), C.byref(ms), _launch_stream(stream, self._device)),
               "cfnmpc_debug_start_factor")
        return ms.value

    def get_factor(self):
        """-> K [B][N][4][13], d [B][N][4], Pchk [B][6][13][13], status [B] of the last start solve (reference state order)"""
        K = np.empty((self.B, self.N, 4, NX)); d = np.empty((self.B, self.N, 4)); Pc = np.zeros((self.B, 6, NX, NX))
        st = np.empty(self.B, dtype=np.int32)
        _check(self._L.cfnmpc_debug_get_factor(self._h, K.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                               Pc.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p)), "cfnmpc_debug_get_factor")
        return K, d, Pc, st

    # ---- outputs
    def get_iterate(self, out=None):
        """-> (x [B, N + 1, 13], u [B, N, 4]); out: a pair of numpy arrays or torch device tensors of those shapes"""
        x, u = out if out is not None else (np.empty((self.B, self.N + 1, NX)), np.empty((self.B, self.N, NU)))
        px, dev, st, _k = _arg(x, (self.B, self.N + 1, NX), device=self._device)
        pu, devu, _s, _k2 = _arg(u, (self.B, self.N, NU), device=self._device)
        if dev != devu or (dev == 0 and not (x.flags.c_contiguous and u.flags.c_contiguous and x.dtype == u.dtype == np.float64)):
            raise ValueError("x and u must both be contiguous float64 host arrays or both device tensors")
        _check(self._L.cfnmpc_get_iterate(self._h, px, pu, dev, st), "cfnmpc_get_iterate")
        return x, u

    def get_u(self, stage, out=None):
        if out is None:
            out = np.empty((self.B, NU))
        p, dev, st, _k = _arg(out, (self.B, NU), device=self._device)
        _check(self._L.cfnmpc_get_u(self._h, int(stage), p, dev, st), "cfnmpc_get_u")
        return out

    def get_x(self, stage, out=None):
        if out is None:
            out = np.empty((self.B, NX))
        p, dev, st, _k = _arg(out, (self.B, NX), device=self._device)
        _check(self._L.cfnmpc_get_x(self._h, int(stage), p, dev, st), "cfnmpc_get_x")
        return out

    def get_cmd(self, cmd_vel=None, motvel=None):
        """Output stage of the reference node for the fleet on the device (cfnmpc_get_cmd):
        -> (cmd_vel [B][4] float64 = pitch deg, -roll deg, thrust PWM, yaw rate deg/s; motvel [B][4] int32).
        numpy arrays (host) or torch device tensors."""
        if cmd_vel is None:
            cmd_vel = np.empty((self.B, 4))
        if motvel is None:
            if _is_torch(cmd_vel):
                import torch
                motvel = torch.empty((self.B, 4), dtype=torch.int32, device=cmd_vel.device)
            else:
                motvel = np.empty((self.B, 4), dtype=np.int32)
        p, dev, st, _k = _arg(cmd_vel, (self.B, 4), device=self._device)
        pm, devm, _s, _k2 = _arg(motvel, (self.B, 4), dtype=np.int32, device=self._device)
        assert dev == devm
        _check(self._L.cfnmpc_get_cmd(self._h, p, pm, dev, st), "cfnmpc_get_cmd")
        return cmd_vel, motvel

    def stats(self):
        st = np.empty(self.B, dtype=np.int32); it = np.empty(self.B, dtype=np.int32); rs = np.empty(self.B)
        _check(self._L.cfnmpc_get_stats(self._h, st.ctypes.data_as(C.c_void_p), it.ctypes.data_as(C.c_void_p),
                                        rs.ctypes.data_as(C.c_void_p), 0, _launch_stream(None, self._device)), "cfnmpc_get_stats")
        return st, it, rs

    def get_linearisation(self):
        A = np.empty((self.B, self.N, NX, NX)); Bm = np.empty((self.B, self.N, NX, NU)); b = np.empty((self.B, self.N, NX))
        _check(self._L.cfnmpc_debug_get_linearisation(self._h, A.ctypes.data_as(C.c_void_p), Bm.ctypes.data_as(C.c_void_p),
                                                      b.ctypes.data_as(C.c_void_p)), "cfnmpc_debug_get_linearisation")
        return A, Bm, b

    def get_condensed(self, block):
        """Partial condensing (cond_N2 > 0): condensed block `block` of every instance after a fresh
        linearisation + pcond -> (H [B][w][w], D [B][13][w], m)."""
        N2 = int(self.opts.cond_N2)
        assert 0 < N2 < self.N
        mmax = -(-self.N // N2)
        w = 4 * mmax + 14
        H = np.zeros((self.B, w, w)); D = np.zeros((self.B, NX, w)); m = C.c_int(0)
        _check(self._L.cfnmpc_debug_get_condensed(self._h, int(block), H.ctypes.data_as(C.c_void_p), D.ctypes.data_as(C.c_void_p),
                                                  C.byref(m)), "cfnmpc_debug_get_condensed")
        wj = 4 * m.value + 14
        return (H.reshape(-1)[:self.B * wj * wj].reshape(self.B, wj, wj).copy(),      # (the library packs with the block's own w)
                D.reshape(-1)[:self.B * NX * wj].reshape(self.B, NX, wj).copy(), m.value)

    def list_counts(self):
        """-> (constrained rows listed, rows listed for the interior-point fall-back, listed rows with heads > 16 stages,
        late rows of a split forward sweep) of the last step"""
        c = np.zeros(4, dtype=np.int32)
        _check(self._L.cfnmpc_debug_get_list_counts(self._h, c.ctypes.data_as(C.c_void_p)), "cfnmpc_debug_get_list_counts")
        return tuple(int(v) for v in c)

    def yref_uniform(self):
        """-> True while the start solve reads every vehicle's stage reference once per step (set_yref found the rows of each
        vehicle equal over the stages); waits for a detection still on its way"""
        u = C.c_int(0)
        _check(self._L.cfnmpc_debug_get_yref_uniform(self._h, C.byref(u)), "cfnmpc_debug_get_yref_uniform")
        return bool(u.value)

    def heads(self):
        h = np.empty(self.B, dtype=np.int32)
        _check(self._L.cfnmpc_debug_get_head(self._h, h.ctypes.data_as(C.c_void_p)), "cfnmpc_debug_get_head")
        return h


def _call_args(x, arrays, rows=()):
    """arrays of one solver-less call on x's side: arrays = ((array or None, shape[, dtype]), ...), then the optional
    rows = ((rows [B][n] or None, n), ...) -> (pointers in that order, on_device, stream, keepalives); all torch device tensors
    (checked by _arg) or all numpy (converted, except None).  Host rows beside device tensors are uploaded: the kernels read
    device memory only."""
    dev, B = _is_torch(x), x.shape[0]
    if dev:
        import torch
        rows = [(r if r is None or _is_torch(r) else torch.as_tensor(np.ascontiguousarray(r, dtype=np.float64), device=x.device), n)
                for r, n in rows]
    ptrs, keep = [], []
    for a, sh, *dtype in (*arrays, *((r, (B, n)) for r, n in rows)):
        if a is None:
            ptrs.append(None)
            continue
        if not dev and _is_torch(a):
            raise ValueError("expected numpy arrays beside a numpy array")
        p, _d, _s, k = _arg(a, sh, *dtype)
        ptrs.append(p); keep.append(k)
    return ptrs, int(dev), _stream_ptr(x) if dev else None, keep


def _out_like(x, out, shape, what, dtype=np.float64):
    """an output array on x's side: the caller's (checked: written in place) or a new one"""
    if out is None:
        if not _is_torch(x):
            return np.empty(shape, dtype=dtype)
        import torch
        return torch.empty(shape, dtype={np.float64: torch.float64, np.int32: torch.int32}[dtype], device=x.device)
    if not _is_torch(x) and not (isinstance(out, np.ndarray) and out.dtype == dtype and out.flags.c_contiguous
                                 and out.shape == tuple(shape)):
        raise ValueError(f"{what}: expected a contiguous {np.dtype(dtype).name} array {tuple(shape)} (written in place)")
    return out


def sim(x, u, T=0.06, steps=4, out=None, params=None, dist=None):
    """Batched predictor / plant step (crazyflie_acados_sim_solve, acados_estimator.cpp:589).  params [B][NP]: each
    row's own model (cfnmpc_sim_params), e.g. a plant that differs from the controller's model.  dist [B][ND]: each row's
    disturbance (cfnmpc_sim_dist; with or without params).  numpy arrays or torch device tensors (host rows of params and dist
    beside device tensors are uploaded); out: an array [B][13] to write into."""
    L = _lib.lib()
    B = x.shape[0]
    out = _out_like(x, out, (B, NX), "out")
    (px, pu, po, pp, pd), dev, st, _keep = _call_args(x, ((x, (B, NX)), (u, (B, NU)), (out, (B, NX))), ((params, NP), (dist, ND)))
    tail = (float(T), int(steps), po, dev, st)
    if dist is not None:
        _check(L.cfnmpc_sim_dist(B, px, pu, pp, pd, *tail), "cfnmpc_sim_dist")
    elif params is not None:
        _check(L.cfnmpc_sim_params(B, px, pu, pp, *tail), "cfnmpc_sim_params")
    else:
        _check(L.cfnmpc_sim(B, px, pu, *tail), "cfnmpc_sim")
    return out


def sim_rollout(x0, u, T=0.015, steps=1, out=None, params=None, dist=None):
    """Open-loop rollout of the plant (cfnmpc_sim_rollout): x0 [B][13], u [B][L][4] -> xs [B][L + 1][13] with xs[:, 0] = x0 and
    xs[:, t + 1] = sim(xs[:, t], u[:, t], T, steps, params=params, dist=dist), bit for bit.  numpy arrays or torch device
    tensors, like sim; params [B][NP] and dist [B][ND] as there (host rows beside device tensors are uploaded)."""
    L_ = _lib.lib()
    B, L = x0.shape[0], u.shape[1]
    out = _out_like(x0, out, (B, L + 1, NX), "out")
    (px, pu, po, pp, pd), dev, st, _keep = _call_args(
        x0, ((x0, (B, NX)), (u, (B, L, NU)), (out, (B, L + 1, NX))), ((params, NP), (dist, ND)))
    _check(L_.cfnmpc_sim_rollout(B, L, px, pu, pp, pd, float(T), int(steps), po, dev, st), "cfnmpc_sim_rollout")
    return out


def sim_rollout_vjp(xs, u, gxs, T=0.015, steps=1, params=None, dist=None, out=None):
    """Gradient of a loss on a rollout (cfnmpc_sim_rollout_vjp): xs [B][L + 1][13] as sim_rollout returned it, u [B][L][4],
    gxs = dl/dxs [B][L + 1][13] -> (gx0 [B][13], gu [B][L][4], gp [B][NP], gd [B][ND]); gp / gd are None when params / dist
    is None.  out: (gx0, gu, gp, gd) arrays to write into, None entries are allocated."""
    L_ = _lib.lib()
    B, L = xs.shape[0], u.shape[1]
    o = tuple(out) if out is not None else (None, None, None, None)
    gx0 = _out_like(xs, o[0], (B, NX), "gx0")
    gu = _out_like(xs, o[1], (B, L, NU), "gu")
    gp = None if params is None else _out_like(xs, o[2], (B, NP), "gp")
    gd = None if dist is None else _out_like(xs, o[3], (B, ND), "gd")
    (pxs, pu, pg, p0, p1, p2, p3, pp, pd), dev, st, _keep = _call_args(
        xs, ((xs, (B, L + 1, NX)), (u, (B, L, NU)), (gxs, (B, L + 1, NX)), (gx0, (B, NX)), (gu, (B, L, NU)), (gp, (B, NP)),
             (gd, (B, ND))), ((params, NP), (dist, ND)))
    _check(L_.cfnmpc_sim_rollout_vjp(B, L, pxs, pu, pp, pd, float(T), int(steps), pg, p0, p1, p2, p3, dev, st),
           "cfnmpc_sim_rollout_vjp")
    return gx0, gu, gp, gd


def estimate_disturbance(x_prev, u_prev, x_meas, d, T=0.015, steps=1, gain_a=0.5, gain_w=0.5, params=None):
    """Disturbance observer (cfnmpc_estimate_disturbance), in place on d [B][ND]: the one-step prediction error of the disturbed
    model from (x_prev, u_prev) against x_meas, fed back with gains in (0, 1].  All torch device tensors or all numpy, like sim;
    feed d to BatchSolver.set_disturbance.  -> d"""
    L = _lib.lib()
    B = x_prev.shape[0]
    if d is None:
        raise ValueError("d: expected the rows [B][ND] to update in place")
    d = _out_like(x_prev, d, (B, ND), "d")
    (px, pu, pm, pd, pp), dev, st, _keep = _call_args(
        x_prev, ((x_prev, (B, NX)), (u_prev, (B, NU)), (x_meas, (B, NX)), (d, (B, ND))), ((params, NP),))
    _check(L.cfnmpc_estimate_disturbance(B, px, pu, pm, pp, pd, float(T), int(steps), float(gain_a), float(gain_w), dev, st),
           "cfnmpc_estimate_disturbance")
    return d


def ekf_step(x, P, u, z=None, r=None, Q=None, T=0.015, steps=1, gate=0.0, normalize=True, params=None, dist=None, out=None):
    """One extended Kalman filter step for every vehicle (cfnmpc_ekf_step; the rules are in include/cfnmpc.h): the estimate
    x [B][13] and its covariance P [B][13][13] through the RK4 plant of sim(x, u, T, steps, params=params, dist=dist) with process
    noise Q [B][13][13] (None: zero), then the sequential update with the measurement z [B][13] of variances r [B][13] (r < 0: the
    component is not measured; z = None: predict only) behind a gate of `gate` standard deviations per component (0: none).
    normalize: q <- q / |q| after an update.  numpy arrays or torch device tensors, like sim; out: (x, P, nis, counts) arrays to
    write into, None entries are allocated -- out = (x, P) updates the filter in place.
    -> (x [B][13], P [B][13][13], nis [B], counts [B][2] int32 = components used, rejected); (P, Q) are the (Sigma0, W) of
    BatchSolver.set_uncertainty."""
    L_ = _lib.lib()
    B = x.shape[0]
    if z is not None and r is None:
        raise ValueError("ekf_step: a measurement z needs its variances r")
    o = tuple(out) + (None,) * (4 - len(out)) if out is not None else (None, None, None, None)
    xn = _out_like(x, o[0], (B, NX), "x")
    Pn = _out_like(x, o[1], (B, NX, NX), "P")
    nis = _out_like(x, o[2], (B,), "nis")
    counts = _out_like(x, o[3], (B, 2), "counts", np.int32)
    (px, pP, pu, pQ, pz, pr, pxn, pPn, pn, pc, pp, pd), dev, st, _keep = _call_args(
        x, ((x, (B, NX)), (P, (B, NX, NX)), (u, (B, NU)), (Q, (B, NX, NX)), (z, (B, NX)), (r if z is not None else None, (B, NX)),
            (xn, (B, NX)), (Pn, (B, NX, NX)), (nis, (B,)), (counts, (B, 2), np.int32)), ((params, NP), (dist, ND)))
    flags = 1 if normalize else 0
    _check(L_.cfnmpc_ekf_step(B, px, pP, pu, pp, pd, float(T), int(steps), pQ, pz, pr, float(gate), flags, pxn, pPn, pn, pc, dev, st),
           "cfnmpc_ekf_step")
    return xn, Pn, nis, counts


EKF_NA = 16   # include/cfnmpc.h: CFNMPC_EKF_NA, 13 states + 3 disturbance slots


def ekf_aug_cov(P, sigma_d, B=None):
    """The augmented covariance Pa [B][16][16] of ekf_aug_step from a state covariance P [B][13][13] (or [13][13], shared) and the
    standard deviations sigma_d [3] (or [B][3]) of the three slots: blockdiag(P, diag(sigma_d^2)).  A slot that stays unused takes
    sigma_d = 0 (its row and column must be zero).  The batch is that of P or of sigma_d; when both are shared it is B, and
    without B the result is one matrix, [1][16][16].  numpy."""
    P = np.asarray(P, dtype=np.float64)
    sd = np.asarray(sigma_d, dtype=np.float64)
    n = P.shape[0] if P.ndim == 3 else (sd.shape[0] if sd.ndim == 2 else None)
    if n is not None and B is not None and int(B) != n:
        raise ValueError(f"ekf_aug_cov: B = {B} beside arrays for {n} vehicles")
    B = n if n is not None else (1 if B is None else int(B))
    Pa = np.zeros((B, EKF_NA, EKF_NA))
    Pa[:, :NX, :NX] = P
    Pa[:, np.arange(NX, EKF_NA), np.arange(NX, EKF_NA)] = np.broadcast_to(sd, (B, 3)) ** 2
    return Pa


def ekf_aug_step(x, d, Pa, u, sel, z=None, r=None, Q=None, Qd=None, T=0.015, steps=1, gate=0.0, normalize=True, params=None,
                 out=None, Pxx_out=None):
    """One step of the disturbance-augmented extended Kalman filter for every vehicle (cfnmpc_ekf_aug_step; the rules are in
    include/cfnmpc.h): ekf_step with the components sel [3] of the disturbance row d [B][ND] (entries of 0 .. 5, distinct; -1: the
    slot is unused) estimated jointly with the state x [B][13], under the covariance Pa [B][16][16] of (x, d[sel]) (ekf_aug_cov
    builds one).  The plant is sim(x, u, T, steps, params=params, dist=d); Q [B][13][13] is the state's process noise and
    Qd [B][3] the slots' random-walk variance per call (None: zero); z, r, gate, normalize as in ekf_step.  numpy arrays or torch
    device tensors, like ekf_step; sel is a host sequence.  out: (x, d, Pa, nis, counts) arrays to write into, None entries are
    allocated -- out = (x, d, Pa) updates the filter in place.  Pxx_out: an array [B][13][13] that receives the state block of
    the new covariance, the Sigma0 of BatchSolver.set_uncertainty.
    -> (x [B][13], d [B][ND], Pa [B][16][16], nis [B], counts [B][2] int32 = components used, rejected)"""
    L_ = _lib.lib()
    B = x.shape[0]
    if z is not None and r is None:
        raise ValueError("ekf_aug_step: a measurement z needs its variances r")
    sel_a = (C.c_int * 3)(*[int(v) for v in sel]) if len(sel) == 3 else None
    if sel_a is None:
        raise ValueError("ekf_aug_step: sel has three entries (-1: slot unused)")
    o = tuple(out) + (None,) * (5 - len(out)) if out is not None else (None,) * 5
    xn = _out_like(x, o[0], (B, NX), "x")
    dn = _out_like(x, o[1], (B, ND), "d")
    Pan = _out_like(x, o[2], (B, EKF_NA, EKF_NA), "Pa")
    nis = _out_like(x, o[3], (B,), "nis")
    counts = _out_like(x, o[4], (B, 2), "counts", np.int32)
    if Pxx_out is not None:
        Pxx_out = _out_like(x, Pxx_out, (B, NX, NX), "Pxx_out")
    (px, pd, pPa, pu, pQ, pQd, pz, pr, pxn, pdn, pPan, pPxx, pn, pc, pp), dev, st, _keep = _call_args(
        x, ((x, (B, NX)), (d, (B, ND)), (Pa, (B, EKF_NA, EKF_NA)), (u, (B, NU)), (Q, (B, NX, NX)), (Qd, (B, 3)), (z, (B, NX)),
            (r if z is not None else None, (B, NX)), (xn, (B, NX)), (dn, (B, ND)), (Pan, (B, EKF_NA, EKF_NA)),
            (Pxx_out, (B, NX, NX)), (nis, (B,)), (counts, (B, 2), np.int32)), ((params, NP),))
    flags = 1 if normalize else 0
    _check(L_.cfnmpc_ekf_aug_step(B, px, pd, pPa, pu, pp, C.cast(sel_a, C.c_void_p), float(T), int(steps), pQ, pQd, pz, pr, float(gate),
                                  flags, pxn, pdn, pPan, pPxx, pn, pc, dev, st), "cfnmpc_ekf_aug_step")
    return xn, dn, Pan, nis, counts


def estimate(meas, filt, u, dt=0.015, use_lpf=True, delay=0.06, steps=4):
    """Batched ESTIMATOR::predictor (acados_estimator.cpp:521-634) on torch device tensors:
    meas [B][9], filt [B][9] (updated in place), u [B][4] -> (x_est, x_pred) [B][13]."""
    import torch
    L = _lib.lib()
    B = meas.shape[0]
    for a, sh in ((meas, (B, 9)), (filt, (B, 9)), (u, (B, 4))):
        assert a.is_cuda and a.dtype == torch.float64 and a.is_contiguous() and tuple(a.shape) == sh
    x_est = torch.empty((B, NX), dtype=torch.float64, device=meas.device)
    x_pred = torch.empty_like(x_est)
    _check(L.cfnmpc_estimate(B, C.c_void_p(meas.data_ptr()), C.c_void_p(filt.data_ptr()), C.c_void_p(u.data_ptr()),
                             float(dt), int(bool(use_lpf)), float(delay), int(steps), C.c_void_p(x_est.data_ptr()),
                             C.c_void_p(x_pred.data_ptr()), _stream_ptr(meas)), "cfnmpc_estimate")
    return x_est, x_pred
