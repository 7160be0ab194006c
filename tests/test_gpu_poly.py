"""GPU suite: device-side polynomial trajectory references (include/cfnmpc.h: cfnmpc_set_poly_library,
cfnmpc_set_poly_assignment, cfnmpc_set_yref_poly, cfnmpc_eval_poly, cfnmpc_get_yref).

References: what the reference's own evaluator returns (tests/golden/poly.npz) for cfnmpc_eval_poly's `flat`, and the numpy twin
crazyflie_nmpc_amd.trajectories.poly_rows (checked on the CPU in tests/test_poly_cpu.py against that evaluator and the model's
identities) for the 17-column rows.  Bounds: 1e-11 max(1, |reference|) -- FP64 rounding of a few hundred operations and of the
device's sincos / asin / atan2 against numpy's; an entry off by more than 1e-9 would be another piece of the polynomial."""
import ctypes as C
import os

import numpy as np
import pytest

from crazyflie_nmpc_amd import trajectories as tj

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "poly.npz"))
NAMES = ("figure8", "takeoff", "figure8_takeoff_landing")
TABLES = [GOLD[n + "_table"] for n in NAMES]
NOM = tj._NOMINAL_PARAMS
DT = 0.015
TOL, PIECE_TOL = 1e-11, 1e-9


def _solver(B, N=50, **kw):
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    return BatchSolver(B, default_opts(N=N, **kw))


def _gold_flat(name):
    g = GOLD
    return np.concatenate([g[name + "_pos"], g[name + "_vel"], g[name + "_acc"], g[name + "_yaw"][:, None], g[name + "_omega"]], 1)


def _relerr(a, ref):
    return np.abs(a - ref) / np.maximum(1.0, np.abs(ref))


def _report(what, err):
    i = np.unravel_index(np.argmax(err), err.shape)
    print(f"{what}: max error {err.max():.2e} at entry {tuple(int(v) for v in i)}")
    return float(err.max())


def _placements(rng, traj, t, N, tables=TABLES):
    """random placements: time scale in {0.5, 1, 2}, yaw0 up to +-pi, and start times such that the windows straddle the start,
    the end / the loop wrap, lie inside, many periods behind the end, or wholly before the start"""
    B = len(traj)
    place = np.zeros((B, 6))
    win = N * DT
    for i in range(B):
        ts = (0.5, 1.0, 2.0)[int(rng.integers(3))]
        D = tables[max(int(traj[i]), 0)][:, 0].sum() * ts
        kind = i % 5
        t0 = {0: t + 0.4 * win, 1: t - D + 0.5 * win, 2: t - rng.uniform(0.1, 0.8) * D, 3: t - 2.3 * D, 4: t + 10.0}[kind]
        place[i] = [t0, ts, rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(0.2, 1.5), rng.uniform(-np.pi, np.pi)]
    place[0, 5], place[B - 1, 5] = np.pi, -np.pi
    return place


# ---- 1. eval_poly against the reference's evaluator ----------------------------------------------------------------------------
def test_eval_poly_against_golden():
    B = 70                                        # one full wave plus six lanes
    s = _solver(B, N=5)
    par = np.tile(NOM, (B, 1)); par[:, 0] = 9.81  # the evaluator's gravity constant
    s.set_model_params(par)
    s.set_poly_library(TABLES)
    traj = (np.arange(B) % 3).astype(np.int32)
    s.set_poly_assignment(traj)
    grids = [int(GOLD[n + "_grid"]) for n in NAMES]
    worst = 0.0
    for ns in (min(grids), max(grids)):           # the shortest table's grid, then a window covering the others'
        flat, rows = s.eval_poly(0.0, ns)
        assert np.isfinite(flat).all() and np.isfinite(rows).all()
        for j, name in enumerate(NAMES):
            n = min(ns, grids[j])
            gold = _gold_flat(name)[:n]
            for i in np.nonzero(traj == j)[0][[0, -1]]:
                worst = max(worst, _report(f"{name} grid [{n}] vehicle {i}", _relerr(flat[i, :n], gold)))
            assert all(np.array_equal(flat[i], flat[j]) for i in np.nonzero(traj == j)[0])   # same table, same placement: same bits
    # the random and the boundary times, one call with one stage each
    for j, name in enumerate(NAMES):
        t, gold, ng = GOLD[name + "_t"], _gold_flat(name), grids[j]
        got = np.array([s.eval_poly(float(tt), 1, want_rows=False)[0][j, 0] for tt in t[ng:]])
        worst = max(worst, _report(f"{name} random and boundary times [{len(t) - ng}]", _relerr(got, gold[ng:])))
    assert worst <= TOL


# ---- 2. set_yref_poly -> get_yref against the twin ------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(70, 5), (70, 50), (1, 5), (1, 50)])
def test_set_yref_poly_against_twin(B, N):
    rng = np.random.default_rng(100 * N + B)
    s = _solver(B, N=N)
    par = np.tile(NOM, (B, 1)); par[:, 1] *= rng.uniform(0.8, 1.2, B)          # mass +- 20 %
    s.set_model_params(par)
    s.set_poly_library(TABLES)
    traj = rng.integers(0, 3, B).astype(np.int32)
    if B > 1:
        traj[[3, 17, 64, 69]] = -1
    t = 3.0
    place = _placements(rng, traj, t, N)
    sent_y, sent_e = rng.standard_normal((B, N, 17)), rng.standard_normal((B, 13))
    for flags in (0, tj.POLY_LOOP, tj.POLY_KINEMATIC):
        s.set_yref(sent_y, sent_e)
        s.set_poly_assignment(traj, place)
        s.set_yref_poly(t, flags)
        y, ye = s.yref()
        _f, rows = tj.poly_rows(TABLES, traj, place, t, N + 1, DT, flags, par)
        on = traj >= 0
        assert np.isfinite(y[on]).all() and np.isfinite(ye[on]).all()
        got = np.concatenate([y[on].reshape(on.sum(), -1), ye[on]], 1)
        want = np.concatenate([rows[on, :N].reshape(on.sum(), -1), rows[on, N, :13]], 1)
        assert np.abs(got - want).max() <= PIECE_TOL, "another piece of the polynomial"
        assert _report(f"B = {B}, N = {N}, flags {flags}", _relerr(got, want)) <= TOL
        # vehicles without a trajectory keep the sentinel bit for bit; a second call writes the same bits
        assert np.array_equal(y[~on], sent_y[~on]) and np.array_equal(ye[~on], sent_e[~on])
        s.set_yref_poly(t, flags)
        y2, ye2 = s.yref()
        assert np.array_equal(y, y2) and np.array_equal(ye, ye2)
    # the windows cover what they are meant to: held rows before the start and behind the end, live rows, a wrap
    tau = (t + np.arange(N + 1)[None] * DT - place[:, 0:1]) / place[:, 1:2]
    Dv = np.array([TABLES[max(int(j), 0)][:, 0].sum() for j in traj])[:, None]
    if B > 1:
        assert ((tau < 0).any(1) & (tau >= 0).any(1)).any() and ((tau < Dv).any(1) & (tau >= Dv).any(1)).any() and (tau > 2 * Dv).any()


# ---- 3. device arrays with bad values ---------------------------------------------------------------------------------------
def test_device_assignment_with_bad_values():
    import torch
    from crazyflie_nmpc_amd.solver import CfnmpcError
    B, N = 70, 5
    rng = np.random.default_rng(3)
    s = _solver(B, N=N)
    s.set_poly_library(TABLES)
    traj = rng.integers(0, 3, B).astype(np.int32)
    place = _placements(rng, traj, 1.0, N)
    place[:, 0] = 1.0 - rng.uniform(0.1, 0.5, B)          # live windows
    bad_id, bad_ts = [2, 9, 40, 66], [5, 11, 41, 69]
    traj[bad_id] = [3, -7, 1000000, -2147483648]
    place[bad_ts, 1] = [0.0, np.nan, -1.0, np.inf]
    sent_y, sent_e = rng.standard_normal((B, N, 17)), rng.standard_normal((B, 13))
    s.set_yref(sent_y, sent_e)
    # host arrays with these values are refused and change nothing
    with pytest.raises(CfnmpcError):
        s.set_poly_assignment(traj, place)
    s.set_yref_poly(1.0)
    y, ye = s.yref()
    assert np.array_equal(y, sent_y) and np.array_equal(ye, sent_e)          # (nobody is assigned yet)
    # device arrays are taken as they are
    s.set_poly_assignment(torch.as_tensor(traj, device="cuda"), torch.as_tensor(place, device="cuda"))
    s.set_yref_poly(1.0)
    torch.cuda.synchronize()
    y, ye = s.yref()
    clean_traj = traj.copy(); clean_traj[bad_id] = -1
    clean_place = place.copy(); clean_place[bad_ts, 1] = 1.0
    _f, rows = tj.poly_rows(TABLES, clean_traj, clean_place, 1.0, N + 1, DT)
    on = clean_traj >= 0
    assert np.isfinite(y[on]).all() and np.isfinite(ye[on]).all()
    assert np.array_equal(y[~on], sent_y[~on]) and np.array_equal(ye[~on], sent_e[~on])
    assert _report("bad ids and time scales", _relerr(y[on], rows[on, :N])) <= TOL and _relerr(ye[on], rows[on, N, :13]).max() <= TOL
    flat, rw = s.eval_poly(1.0, 3)
    assert np.isnan(rw[~on]).all() and np.isnan(flat[~on]).all() and np.isfinite(rw[on]).all()
    # a smaller library resets the ids it no longer has
    s.set_poly_library(TABLES[:1])
    s.set_yref(sent_y, sent_e)
    s.set_yref_poly(1.0)
    y, _ye = s.yref()
    gone = clean_traj != 0
    assert np.array_equal(y[gone], sent_y[gone]) and not np.array_equal(y[~gone], sent_y[~gone])
    s.set_poly_library(TABLES)                            # ... for good: the larger library does not bring them back
    s.set_yref(sent_y, sent_e)
    s.set_yref_poly(1.0)
    assert np.array_equal(s.yref()[0][gone], sent_y[gone])


# ---- 4. guard -------------------------------------------------------------------------------------------------------------------
def test_guard_free_fall():
    from test_poly_cpu import free_fall_table
    B, N = 3, 50
    s = _solver(B, N=N)
    tab = free_fall_table()
    s.set_poly_library([tab])
    s.set_poly_assignment(np.zeros(B, dtype=np.int32))
    s.set_yref_poly(0.0)
    y, ye = s.yref()
    flat, rows = tj.poly_rows([tab], np.zeros(B), None, 0.0, N + 1, DT)
    assert np.isfinite(y).all() and np.isfinite(ye).all()
    assert _relerr(y, rows[:, :N]).max() <= TOL and _relerr(ye, rows[:, N, :13]).max() <= TOL
    hov = np.sqrt(NOM[1] * NOM[0] / (4 * NOM[6]))
    assert (y[:, :, 4:6] == 0).all() and (y[:, :, 10:12] == 0).all() and np.abs(y[:, :, 13:] - hov).max() <= 1e-14
    assert np.abs(y[:, :, 12] - 0.2).max() <= 1e-15


# ---- 5. closed loop -------------------------------------------------------------------------------------------------------------
def test_closed_loop_tracks_and_matches_twin_and_graph():
    from crazyflie_nmpc_amd import sim
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B, N, steps = 24, 50, 150
    rng = np.random.default_rng(24)
    tab = TABLES[0]
    traj = np.zeros(B, dtype=np.int32)
    place = np.stack([-rng.uniform(0.0, 4.0, B), np.ones(B), rng.uniform(-2, 2, B), rng.uniform(-2, 2, B), rng.uniform(0.4, 1.0, B),
                      rng.uniform(-np.pi, np.pi, B)], 1)
    ref, _r = tj.poly_rows([tab], traj, place, 0.0, steps, DT)            # the path: positions at the control times
    _f, start = tj.poly_rows([tab], traj, place, 0.0, 1, DT)

    def loop(flags, source, **kw):
        s = _solver(B, N=N, **kw)
        s.set_poly_library([tab]); s.set_poly_assignment(traj, place)
        x = start[:, 0, :13].copy()
        s.set_x0(x); s.init_iterate(INIT_HOVER)
        err, U0 = [], []
        for k in range(steps):
            if source == "device":
                s.set_yref_poly(k * DT, flags)
            else:
                _f, rows = tj.poly_rows([tab], traj, place, k * DT, N + 1, DT, flags)
                s.set_yref(np.ascontiguousarray(rows[:, :N]), np.ascontiguousarray(rows[:, N, :13]))
            s.set_x0(x)
            s.solve(1)
            u0 = s.get_u(0)
            err.append(np.linalg.norm(x[:, :3] - ref[:, k, :3], axis=1))
            U0.append(u0.copy())
            x = sim(x, u0, T=DT, steps=1)
        assert (s.stats()[0] == 0).all()
        e = np.array(err[60:])
        return np.sqrt((e ** 2).mean(0)), np.array(U0)

    rms_c, u_dev = loop(0, "device")
    rms_k, _u = loop(tj.POLY_KINEMATIC, "device")
    print(f"RMS position error per vehicle: consistent {1e3 * rms_c.min():.3f} .. {1e3 * rms_c.max():.3f} mm, "
          f"kinematic {1e3 * rms_k.min():.3f} .. {1e3 * rms_k.max():.3f} mm, largest ratio {(rms_c / rms_k).max():.4f}")
    assert (rms_c <= 0.25 * rms_k).all()
    _r, u_twin = loop(0, "twin")
    du = np.abs(u_dev - u_twin).max()
    print(f"u0 against a solver fed the twin's rows through set_yref: {du:.2e}")
    assert du <= 1e-9
    _r, u_graph = loop(0, "device", step_graph=1)
    assert np.array_equal(u_graph, u_dev)


# ---- 6. layers ------------------------------------------------------------------------------------------------------------------
def _get_yref(L, handle, count, N):
    y = np.empty((count, N, 17)); ye = np.empty((count, 13))
    assert L.cfnmpc_get_yref(handle, y.ctypes.data_as(C.c_void_p), ye.ctypes.data_as(C.c_void_p), 0, None) == 0
    return y, ye


def _fleet_windows(L, fh):
    """[(N, indices in the fleet's order, yref, yref_e)] through the buckets' solvers"""
    out = []
    for b in range(L.cfnmpc_fleet_num_buckets(fh)):
        n, c, sv = C.c_int(0), C.c_int(0), C.c_void_p()
        assert L.cfnmpc_fleet_bucket(fh, b, C.byref(n), C.byref(c), C.byref(sv), None) == 0
        idx = np.empty(c.value, dtype=np.int32)
        assert L.cfnmpc_fleet_bucket(fh, b, None, None, None, idx.ctypes.data_as(C.c_void_p)) == 0
        out.append((n.value, idx, *_get_yref(L, sv, c.value, n.value)))
    return out


def test_layers_match_single_solvers():
    from crazyflie_nmpc_amd import _lib, default_opts
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.parallel import MultiGpuFleet
    L = _lib.lib()
    rng = np.random.default_rng(6)
    hz = np.tile([5, 8, 50], 9).astype(np.int32)
    B = len(hz)
    traj = rng.integers(0, 3, B).astype(np.int32)
    traj[[4, 20]] = -1
    t, flags = 2.0, tj.POLY_LOOP
    place = _placements(rng, traj, t, 8)
    single = {}
    for N in (5, 8, 50):
        s = _solver(B, N=N)
        s.set_poly_library(TABLES); s.set_poly_assignment(traj, place); s.set_yref_poly(t, flags)
        single[N] = s.yref()

    def check(windows, what):
        seen = np.zeros(B, dtype=int)
        for N, idx, y, ye in windows:
            assert np.array_equal(y, single[N][0][idx]) and np.array_equal(ye, single[N][1][idx]), (what, N)
            seen[idx] += 1
        assert (seen == 1).all(), what

    f = MixedHorizonFleet(hz)
    f.set_poly_library(TABLES); f.set_poly_assignment(traj, place); f.set_yref_poly(t, flags)
    check(_fleet_windows(L, f._h), "fleet")
    flat, rows = f.eval_poly(t, flags)
    for i in range(B):
        n = hz[i]
        assert np.isnan(rows[i, n:]).all() and np.isnan(flat[i, n:]).all()
        if traj[i] >= 0:
            assert np.array_equal(rows[i, :n], single[50][0][i, :n])
        else:
            assert np.isnan(rows[i]).all()
    # one process, two shards on one GPU: contiguous shards of one horizon ...
    m = MultiGpuFleet(B, [0, 0], default_opts(N=8))
    m.set_poly_library(TABLES); m.set_poly_assignment(traj, place); m.set_yref_poly(t, flags)
    assert L.cfnmpc_multi_sync(m._h) == 0
    wins = []
    for i in range(2):
        sv, lo, hi = C.c_void_p(), C.c_int(0), C.c_int(0)
        assert L.cfnmpc_multi_shard(m._h, i, C.byref(sv), C.byref(lo), C.byref(hi), None, None) == 0
        wins.append((8, np.arange(lo.value, hi.value), *_get_yref(L, sv, hi.value - lo.value, 8)))
    check(wins, "multi")
    # ... and shards that are mixed-horizon fleets
    mm = MultiGpuFleet(B, [0, 0], horizons=hz)
    mm.set_poly_library(TABLES); mm.set_poly_assignment(traj, place); mm.set_yref_poly(t, flags)
    assert L.cfnmpc_multi_sync(mm._h) == 0
    wins = []
    for i in range(2):
        fh, cnt = C.c_void_p(), C.c_int(0)
        assert L.cfnmpc_multi_shard_fleet(mm._h, i, C.byref(fh), C.byref(cnt), None, None, None) == 0
        sidx = np.empty(cnt.value, dtype=np.int32)
        assert L.cfnmpc_multi_shard_fleet(mm._h, i, None, None, sidx.ctypes.data_as(C.c_void_p), None, None) == 0
        wins += [(N, sidx[idx], y, ye) for N, idx, y, ye in _fleet_windows(L, fh)]
    check(wins, "multi, mixed horizons")


# ---- 7. lifetimes ---------------------------------------------------------------------------------------------------------------
def test_lifetimes_and_refusals(oracle):
    from crazyflie_nmpc_amd.solver import INIT_HOVER, CfnmpcError
    B, N = 9, 5
    s = _solver(B, N=N)
    with pytest.raises(CfnmpcError):
        s.set_yref_poly(0.0)                               # no library
    with pytest.raises(CfnmpcError):
        s.eval_poly(0.0, 2)
    before = s.workspace_bytes
    bad = TABLES[0].copy(); bad[2, 0] = 0.0
    for tabs in ([bad], [np.where(np.arange(33) == 7, np.nan, TABLES[1])], [TABLES[1]] * 1025):
        with pytest.raises(CfnmpcError):
            s.set_poly_library(tabs)
    assert s.workspace_bytes == before                     # (refused before anything is allocated)
    s.set_poly_library(TABLES)
    assert s.workspace_bytes > before
    with pytest.raises(CfnmpcError):
        s.set_poly_assignment(np.full(B, 3, dtype=np.int32))
    with pytest.raises(CfnmpcError):
        s.set_yref_poly(0.0, 4)                            # an unknown flag
    s.set_poly_assignment(np.zeros(B, dtype=np.int32))
    x0 = oracle.sample_hover_x0(np.random.default_rng(1), B)
    s.set_yref_poly(0.5); s.set_x0(x0); s.init_iterate(INIT_HOVER)
    s.solve(1)
    s.eval_uncertainty()
    s.set_yref_poly(0.515)                                 # the data of the next QP: as after set_yref
    with pytest.raises(CfnmpcError):
        s.eval_uncertainty()
    s.solve(1)
    s.eval_uncertainty()
    s.set_poly_library(None)                               # cleared
    with pytest.raises(CfnmpcError):
        s.set_yref_poly(0.0)
