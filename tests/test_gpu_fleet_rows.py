"""GPU suite: the row staging of the fleet and multi-GPU layers.  Every cfnmpc_fleet_get_* /
cfnmpc_multi_get_* moves rows between the caller's vehicle order and the order of a bucket or shard; this file reads every
getter through host arrays and through device tensors, with all outputs and with each single output (the others NULL), into
prefilled arrays with a guard behind them, and compares bit for bit with the same getter of what lies below: the buckets' own
solvers (cfnmpc_fleet_bucket) for a fleet, one solver or one fleet fed the same data for a multi-GPU fleet.  Only copies are
under test: no tolerance anywhere.

The fleet has eleven vehicles in three buckets of unequal size, none contiguous in the fleet's order; N = 5 is the shortest
horizon a solver accepts, so its bucket has the smallest initial staging, and the sensitivity ranges read here exceed it.
All calls go through ctypes: the Python wrappers request every output."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HORIZONS = [5, 8, 8, 17, 5, 17, 8, 5, 5, 17, 8]
NMIN, NMAX = min(HORIZONS), max(HORIZONS)
BOX = (1.0, 21.0)        # the scalar box of tests/test_heterogeneous_cpu.py: with the 1 m/s kick some rows are constrained
QP_TOL = 1e-11
SQP_TOL = 1e-8
GUARD = 7                # elements behind every output array that no call may touch
FILL = {np.float64: -7.25e300, np.int32: -77777777}

# getter -> (name behind cfnmpc_[fleet_|multi_], leading arguments, outputs [(dtype, elements per vehicle)], may be NULL)
GETTERS = {
    "u": ("get_u", (NMIN - 1,), [(np.float64, 4)], (False,)),
    "x": ("get_x", (NMIN,), [(np.float64, 13)], (False,)),
    "cmd": ("get_cmd", (), [(np.float64, 4), (np.int32, 4)], (False, True)),
    "stats": ("get_stats", (), [(np.int32, 1), (np.int32, 1), (np.float64, 1)], (True, True, True)),
    "nlp_stats": ("get_nlp_stats", (), [(np.float64, 1), (np.float64, 3)], (True, True)),
    # du and dx of stages 0 .. Nmin-1: 5 x 221 doubles per vehicle against the 5 x 17 + 13 of the N = 5 bucket's first staging
    "sens": ("get_sens_x0", (0, NMIN), [(np.float64, NMIN * 52), (np.float64, NMIN * 169)], (True, True)),
    # dx up to stage Nmin (du does not exist there)
    "sens_last": ("get_sens_x0", (1, NMIN), [(np.float64, NMIN * 52), (np.float64, NMIN * 169)], (True, False)),
    "sqp_stats": ("get_sqp_stats", (), [(np.int32, 1), (np.int32, 1), (np.float64, 3)], (True, True, True)),
    "sqp_ls_stats": ("get_sqp_ls_stats", (), [(np.float64, 1), (np.float64, 1), (np.int32, 1), (np.int32, 1)], (True, True, True, True)),
}
AFTER_SQP = ("sqp_stats", "sqp_ls_stats")


def _masks(name):
    """all outputs, then each single output with the others NULL (outputs that must be given stay)"""
    _f, _pre, outs, nullable = GETTERS[name]
    if name == "sens_last":
        return [(False, True)]
    full = tuple(True for _ in outs)
    out = [full]
    for k in range(len(outs)):
        m = tuple(j == k or not nullable[j] for j in range(len(outs)))
        if m not in out:
            out.append(m)
    return out


CASES = [(g, m) for g in GETTERS for m in _masks(g)]
MULTI_CASES = [(g, m) for g, m in CASES if g not in AFTER_SQP]


def _id(v):
    return "".join("x" if b else "-" for b in v) if isinstance(v, tuple) else str(v)


def _data(B, Nmax, seed):
    """distinct x0, yref and weight rows per vehicle"""
    from crazyflie_nmpc_amd.synthetic import HOV_W, regulation_row, sample_hover_x0
    from crazyflie_nmpc_amd.solver import default_opts
    o = default_opts()
    rng = np.random.default_rng(seed)
    x0 = sample_hover_x0(rng, B, scale=1.0)
    x0[:, 7:10] += rng.normal(0, 1.0, (B, 3))
    rows = np.stack([regulation_row((0.1 * rng.uniform(-1, 1), 0.1 * rng.uniform(-1, 1), 0.4 + 0.01 * i), HOV_W) for i in range(B)])
    yref = np.repeat(rows[:, None, :], Nmax, 1) + 1e-3 * np.arange(Nmax)[None, :, None]   # (every stage row differs too)
    W = np.array(o.W[:]) * np.exp(rng.uniform(np.log(0.25), np.log(4.0), (B, 17)))
    WN = np.array(o.WN[:]) * np.exp(rng.uniform(np.log(0.25), np.log(4.0), (B, 13)))
    return dict(x0=x0, yref=np.ascontiguousarray(yref), yref_e=rows[:, :13].copy(), W=W, WN=WN)


def _feed(o, d, rows=None, N=None):
    """the data on a solver, fleet or multi-GPU fleet (rows: the vehicles it holds; N: its yref rows), then one RTI step from
    the hover start, eval_nlp and eval_sens_x0"""
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    r = slice(None) if rows is None else np.asarray(rows)
    N = d["yref"].shape[1] if N is None else N
    o.set_weights_batch(d["W"][r], d["WN"][r])
    o.set_box(*BOX)
    o.set_x0(d["x0"][r])
    o.set_yref(d["yref"][r, :N].copy(), d["yref_e"][r])
    o.init_iterate(INIT_HOVER)
    o.solve(1)
    o.eval_nlp()
    o.eval_sens_x0()


class _Out:
    """one output array of B rows, prefilled, with a guard behind it; host (numpy) or device (torch)"""

    def __init__(self, dtype, B, width, device):
        self.dtype, self.B, self.width = dtype, B, width
        n = B * width + GUARD
        if device:
            import torch
            self.t = torch.full((n,), FILL[dtype], dtype={np.float64: torch.float64, np.int32: torch.int32}[dtype], device="cuda")
            self.ptr = C.c_void_p(self.t.data_ptr())
        else:
            self.t = np.full(n, FILL[dtype], dtype=dtype)
            self.ptr = self.t.ctypes.data_as(C.c_void_p)

    def read(self):
        """-> (rows [B][width], guard untouched)"""
        a = self.t if isinstance(self.t, np.ndarray) else self.t.cpu().numpy()
        return a[:self.B * self.width].reshape(self.B, self.width).copy(), bool((a[self.B * self.width:] == FILL[self.dtype]).all())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(fn, h, name, mask, B, mode, pre=None):
    """one getter call -> (return code, [rows or None per output], every guard untouched).
    mode: 'multi' (no on_device / stream arguments), else the on_device value; 1 reads through device tensors"""
    _f, pre_, outs, _n = GETTERS[name]
    pre = pre_ if pre is None else pre
    bufs = [_Out(dt, B, w, mode == 1) if want else None for (dt, w), want in zip(outs, mask)]
    ptrs = [b.ptr if b else None for b in bufs]
    rc = fn(h, *pre, *ptrs) if mode == "multi" else fn(h, *pre, *ptrs, mode, _stream())
    got = [b.read() if b else (None, True) for b in bufs]
    return rc, [g[0] for g in got], all(g[1] for g in got)


def _same(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), k
        if a is not None:
            assert a.dtype == b.dtype and np.array_equal(a, b), (k, np.flatnonzero((a != b).any(axis=1)))


# ---- the fleet against its buckets' own solvers ----------------------------------------------------------------------------------
def _buckets(L, f):
    """-> [(N, solver handle, fleet indices)]"""
    out = []
    for b in range(L.cfnmpc_fleet_num_buckets(f._h)):
        n, c, sv = C.c_int(0), C.c_int(0), C.c_void_p()
        assert L.cfnmpc_fleet_bucket(f._h, b, C.byref(n), C.byref(c), C.byref(sv), None) == 0
        idx = np.empty(c.value, dtype=np.int32)
        assert L.cfnmpc_fleet_bucket(f._h, b, None, None, None, idx.ctypes.data_as(C.c_void_p)) == 0
        out.append((n.value, sv, idx))
    return out


def _from_buckets(L, bk, name, mask, B):
    """the same getter on every bucket's own solver (host arrays), its rows placed at the bucket's fleet indices"""
    fname, _pre, outs, _n = GETTERS[name]
    want = [np.full((B, w), FILL[dt], dtype=dt) if m else None for (dt, w), m in zip(outs, mask)]
    for _N, sv, idx in bk:
        rc, rows, ok = _call(getattr(L, "cfnmpc_" + fname), sv, name, mask, idx.size, 0)
        assert rc == 0 and ok, (name, mask, rc)
        for w, r in zip(want, rows):
            if w is not None:
                w[idx] = r
    for (dt, _w), w in zip(outs, want):
        assert w is None or not (w == FILL[dt]).any()      # (every fleet row belongs to a bucket)
    return want


@pytest.fixture(scope="module")
def fleet_records():
    """The whole run, once: one RTI step, eval_nlp, eval_sens_x0 through the fleet; every getter call of CASES on the fleet
    (host arrays and device tensors) beside its reference from the buckets; then a short globalised solve_sqp and its two
    getters (the sensitivities do not outlive a globalised solve, so they are read before it).
    -> {(getter, mask, mode): (return code, rows, guards untouched, reference)}, and the RTI statistics"""
    import torch
    from crazyflie_nmpc_amd import _lib
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    L = _lib.lib()
    B = len(HORIZONS)
    d = _data(B, NMAX, 11)
    f = MixedHorizonFleet(HORIZONS, tol=QP_TOL)
    bk = _buckets(L, f)
    assert [(n, idx.size) for n, _s, idx in bk] == [(5, 4), (8, 4), (17, 3)]
    assert all((np.diff(idx) > 1).any() for _n, _s, idx in bk)          # no bucket is contiguous in the fleet's order
    _feed(f, d)
    rec = {}

    def collect(names):
        for g, m in CASES:
            if g not in names:
                continue
            torch.cuda.synchronize()
            want = _from_buckets(L, bk, g, m, B)
            for mode in (0, 1):
                rec[(g, m, mode)] = _call(getattr(L, "cfnmpc_fleet_" + GETTERS[g][0]), f._h, g, m, B, mode) + (want,)

    collect([g for g in GETTERS if g not in AFTER_SQP])
    f.set_sqp_globalization("merit_backtracking")
    f.solve_sqp(4, SQP_TOL, SQP_TOL, SQP_TOL)
    collect(AFTER_SQP)
    torch.cuda.synchronize()
    f.close()
    return rec


def test_fleet_case_is_a_test(fleet_records):
    """the case has constrained and unconstrained rows, and no two vehicles share an output row (a row placed at a wrong index
    of its own bucket would otherwise compare equal)"""
    _rc, (st, it, _res), _ok, _want = fleet_records[("stats", (True, True, True), 0)]
    print(f"status {st[:, 0].tolist()}  qp_iter {it[:, 0].tolist()}")
    assert (st == 0).all() and (it > 0).any() and (it == 0).any()
    for g in ("x", "nlp_stats", "sens"):
        rows = fleet_records[(g, _masks(g)[0], 0)][3][0]
        assert len({r.tobytes() for r in rows}) == len(rows), g


@pytest.mark.parametrize("mode", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("getter,mask", CASES, ids=_id)
def test_fleet_getter_equals_its_buckets(fleet_records, getter, mask, mode):
    """cfnmpc_fleet_<getter> with the outputs of `mask` (the others NULL), host arrays or device tensors: return code 0, every
    requested element the bucket solver's own, bit for bit, and nothing written behind the arrays"""
    rc, got, guards, want = fleet_records[(getter, mask, mode)]
    assert rc == 0
    assert guards
    _same(got, want)


# ---- a multi-GPU fleet of two shards on device 0 against one solver / one fleet ----------------------------------------------------
def _multi_records(m, ref, ref_fn_prefix, B):
    from crazyflie_nmpc_amd import _lib
    import torch
    L = _lib.lib()
    rec = {}
    for g, mask in MULTI_CASES:
        torch.cuda.synchronize()
        want = _call(getattr(L, ref_fn_prefix + GETTERS[g][0]), ref._h, g, mask, B, 0)
        assert want[0] == 0 and want[2], (g, mask)
        rec[(g, mask)] = _call(getattr(L, "cfnmpc_multi_" + GETTERS[g][0]), m._h, g, mask, B, "multi") + (want[1],)
    return rec


@pytest.fixture(scope="module")
def multi_records():
    """uniform: N = 8, five vehicles in shards of 3 + 2, against one solver; mixed: the horizons of this file, against one
    fleet.  Full-horizon sweeps (active_horizon = 0): a vehicle's arithmetic does not depend on its neighbours
    (tests/test_gpu_heterogeneous.py::test_multi_equals_one_solver)."""
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.parallel import MultiGpuFleet
    out = {}
    opts = default_opts(N=8, tol=QP_TOL, active_horizon=0)
    d = _data(5, 8, 12)
    m, s = MultiGpuFleet(5, [0, 0], opts), BatchSolver(5, opts)
    assert [(lo, hi) for lo, hi, _d in m.shards()] == [(0, 3), (3, 5)]
    for o in (m, s):
        _feed(o, d)
    out["uniform"] = _multi_records(m, s, "cfnmpc_", 5)
    m.close(); s.close()
    B = len(HORIZONS)
    d = _data(B, NMAX, 11)
    m = MultiGpuFleet(B, [0, 0], default_opts(tol=QP_TOL, active_horizon=0), horizons=HORIZONS)
    f = MixedHorizonFleet(HORIZONS, tol=QP_TOL, active_horizon=0)
    assert sorted(np.concatenate([idx for idx, _d in m.shards()]).tolist()) == list(range(B))
    for o in (m, f):
        _feed(o, d)
    out["mixed"] = _multi_records(m, f, "cfnmpc_fleet_", B)
    m.close(); f.close()
    return out


@pytest.mark.parametrize("kind", ["uniform", "mixed"])
@pytest.mark.parametrize("getter,mask", MULTI_CASES, ids=_id)
def test_multi_getter_equals_one_solver_or_fleet(multi_records, kind, getter, mask):
    """cfnmpc_multi_<getter> (host arrays of the whole fleet) against the same getter of one solver (uniform shards) or one
    fleet (mixed shards) fed the same data, bit for bit; nothing written behind the arrays"""
    rc, got, guards, want = multi_records[kind][(getter, mask)]
    assert rc == 0
    assert guards
    _same(got, want)


# ---- on_device = 2 on a fleet: host arrays, synchronous ------------------------------------------------------------------------------
def test_fleet_reads_on_host_async_as_host():
    """cfnmpc_fleet_set_x0 / get_u / get_x / get_stats with on_device = CFNMPC_ON_HOST_ASYNC and numpy arrays: the same bits as
    with CFNMPC_ON_HOST, complete when the call returns (include/cfnmpc.h, `on_device`)."""
    from crazyflie_nmpc_amd import _lib
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    L = _lib.lib()
    B = len(HORIZONS)
    d = _data(B, NMAX, 13)
    res = {}
    for mode in (0, 2):
        f = MixedHorizonFleet(HORIZONS, tol=QP_TOL)
        f.set_box(*BOX)
        f.set_yref(d["yref"], d["yref_e"])
        x0 = d["x0"].copy()
        assert L.cfnmpc_fleet_set_x0(f._h, x0.ctypes.data_as(C.c_void_p), mode, _stream()) == 0
        x0[:] = 0.0                                   # (synchronous: the caller's array is free again)
        f.init_iterate(INIT_HOVER)
        f.solve(1)
        out = []
        for g in ("u", "stats"):
            rc, got, ok = _call(getattr(L, "cfnmpc_fleet_" + GETTERS[g][0]), f._h, g, _masks(g)[0], B, mode)
            assert rc == 0 and ok, (mode, g, rc)
            out += got
        rc, got, ok = _call(L.cfnmpc_fleet_get_x, f._h, "x", (True,), B, mode, pre=(0,))
        assert rc == 0 and ok and np.array_equal(got[0], d["x0"]), mode      # (x_0 of the iterate is the x0 that was set)
        res[mode] = out
        f.close()
    _same(res[2], res[0])
