"""GPU suite: per-instance cost weights (include/cfnmpc.h: cfnmpc_set_weights_batch).

The reference is the oracle, never the engine: oracle.qp_from_blocks on oracle.rk4_sens blocks with the row's own Qd, Rd, QNd,
solved by oracle.solve_qp_dense with oracle.solve_qp_refined as referee (tests/test_weights_cpu.py checks that reference
against the C restatement run with one row's weights in its Opts: 7e-13).  Weights: row i = default weights x a factor that is
log-uniform in [1/4, 4] per entry.  Inputs "kicked": hover-centred x0, regulation to (0, 0, 0.4), hover-initialised iterate, 3
closed-loop RTI steps with the rows in force, then N(0, 1) m/s on the body velocity."""
import numpy as np
import pytest

from test_weights_cpu import DT, agree, default_weights, random_rows, ref_step, regulation

pytestmark = pytest.mark.gpu
QP_TOL = 1e-11


def _solver(B, W=None, WN=None, M=1, **kw):
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    s = BatchSolver(B, default_opts(**kw))
    if M != 1:
        s.set_erk_steps(M)
    if W is not None or WN is not None:
        s.set_weights_batch(W, WN)
    return s


def _kicked(oracle, B, N, Wr, WNr, seed, kick=1.0, scale=1.0, **kw):
    """-> (x0 kicked, pre-step iterate x, u, yref, yref_e) after 3 closed-loop steps with the rows in force"""
    from crazyflie_nmpc_amd import sim
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    rng = np.random.default_rng(seed)
    x0 = oracle.sample_hover_x0(rng, B, scale=scale)
    yr, ye = regulation(oracle, B, N)
    s = _solver(B, Wr, WNr, tol=QP_TOL, **kw)
    s.set_x0(x0); s.set_yref(yr, ye); s.init_iterate(INIT_HOVER)
    x = x0.copy()
    for _ in range(3):
        s.set_x0(x); s.solve(1)
        x = sim(x, s.get_u(0), DT, 1)
    x[:, 7:10] += rng.normal(0, kick, (B, 3))
    xi, ui = s.get_iterate()
    s.close()
    return x, xi, ui, yr, ye


# ---- 1. one RTI step per row against the exact QP ----------------------------------------------------------------------
ROUTES = [dict(), dict(as_dense=1), dict(as_dense=-1), dict(as_passes=-1), dict(as_passes=-3), dict(forward_split=1),
          dict(forward_sweep=2), dict(as_warm=1), dict(step_graph=1), dict(active_horizon=0), dict(M=2), dict(sbox=1),
          dict(active_set=0)]
B1, B1P, N1 = 1024, 1022, 50
ROWS_A = 44          # random rows of the full solver
ROWS_P = [1015, 1016, 1017, 1018, 1019, 1020, 1021, 3]   # rows of the second solver: its last full wave and its partial last wave


@pytest.fixture(scope="module")
def step_case(oracle):
    Wr, WNr = random_rows(np.random.default_rng(70), B1)
    x0, x, u, yr, ye = _kicked(oracle, B1, N1, Wr, WNr, 11)
    rows = sorted(set(np.random.default_rng(1).choice(B1P, ROWS_A, replace=False).tolist()) | set(ROWS_P))
    return dict(Wr=Wr, WNr=WNr, x0=x0, x=x, u=u, yr=yr, ye=ye, rows=rows, ref={})


def _sbox(B, N):
    k = np.arange(N)
    lb = np.broadcast_to((1.0 + 0.5 * (k % 2))[None, :, None], (B, N, 4)).copy()
    ub = np.broadcast_to((21.0 - 0.5 * (k % 3))[None, :, None], (B, N, 4)).copy()
    return lb, ub


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: ",".join(f"{k}={v}" for k, v in r.items()) or "default")
def test_rti_step_matches_exact_qp(oracle, step_case, route):
    c = step_case
    route = dict(route)
    M = route.pop("M", 1)
    sbox = route.pop("sbox", 0)
    ipm = route.get("active_set", 1) == 0
    tol = 5e-6 if ipm else 1e-8
    W0, WN0 = default_weights()
    lb, ub = _sbox(B1, N1) if sbox else (None, None)
    out = {}
    for B in (B1, B1P):
        s = _solver(B, c["Wr"][:B], c["WNr"][:B], M, tol=QP_TOL, **route)
        if sbox:
            s.set_box_stages(lb[:B], ub[:B])
        s.set_x0(c["x0"][:B]); s.set_yref(c["yr"][:B], c["ye"][:B]); s.set_iterate(c["x"][:B], c["u"][:B])
        s.solve(1)
        out[B] = s.get_iterate() + tuple(s.stats())
        s.close()
    key = (M, sbox)
    ref = c["ref"].setdefault(key, {})
    worst, n_as, n_feas, n = 0.0, 0, 0, 0
    for i in c["rows"]:
        if i not in ref:
            bl, bu = (lb[i], ub[i]) if sbox else (0.0, 22.0)
            xr, ur, qp = ref_step(oracle, c["x"][i], c["u"][i], c["x0"][i], c["yr"][i], c["ye"][i], c["Wr"][i], c["WNr"][i], bl, bu, M)
            _, ud, _ = ref_step(oracle, c["x"][i], c["u"][i], c["x0"][i], c["yr"][i], c["ye"][i], W0, WN0, bl, bu, M)
            ref[i] = (xr, ur, qp, np.abs(ud[0] - ur[0]).max())
        xr, ur, qp, dw = ref[i]
        assert dw > 1e-3, (i, dw)                      # the weights matter on this row
        for B in ((B1P,) if i in ROWS_P else (B1,)) if i not in (1020, 1021) else (B1, B1P):
            xg, ug, st, it, res = out[B]
            assert st[i] == 0, (B, i, st[i])
            e = agree(oracle, xg[i], ug[i], xr, ur, qp, c["x"][i], c["u"][i], tol)
            worst = max(worst, e)
            assert e <= tol, (B, i, e)
            n += 1
            n_feas += int(it[i] == 0)
            n_as += int(it[i] > 0 and res[i] == 0.0)
    print(f"route {route or 'default'} M={M} sbox={sbox}: {n} compared, worst {worst:.2e}, feasible {n_feas}, active-set {n_as}")
    assert n >= 48
    assert n_feas >= 4
    if not ipm:
        assert n_as >= n // 4, (n_as, n)


# ---- 2. rows equal to the uniform weights are the uniform path, bitwise --------------------------------------------------
def _closed_loop(s, oracle, x0, yr, ye, steps, seed):
    from crazyflie_nmpc_amd import sim
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    rng = np.random.default_rng(seed)
    s.set_x0(x0); s.set_yref(yr, ye); s.init_iterate(INIT_HOVER)
    x = x0.copy()
    out = []
    for j in range(steps):
        s.set_x0(x)
        s.solve(1)
        u0 = s.get_u(0)
        out.append((u0, s.get_u(1), s.get_x(4)) + tuple(s.stats()[:2]))
        x = sim(x, u0, DT, 1)
        if j % 3 == 1:
            x[:, 7:10] += rng.normal(0, 0.5, (x.shape[0], 3))
    return out


def _same(ra, rb):
    for p_, q_ in zip(ra, rb):
        for v, w in zip(p_, q_):
            assert np.array_equal(v, w)


def test_uniform_rows_are_the_uniform_path_bitwise(oracle):
    B, N = 512, 50
    rng = np.random.default_rng(21)
    x0 = oracle.sample_hover_x0(rng, B, scale=1.5)
    yr, ye = regulation(oracle, B, N)
    W, WN = default_weights()
    ra = _closed_loop(_solver(B), oracle, x0, yr, ye, 20, 5)
    assert sum(int((r[4] > 0).sum()) for r in ra) > 0             # constrained rows are in
    _same(ra, _closed_loop(_solver(B, np.tile(W, (B, 1)), np.tile(WN, (B, 1))), oracle, x0, yr, ye, 20, 5))
    s = _solver(B, *random_rows(rng, B))
    s.set_weights_batch(None, None)
    _same(ra, _closed_loop(s, oracle, x0, yr, ye, 20, 5))
    # cost scaling and set_weights applied AFTER the rows, against a solver without rows given the same two calls
    res = []
    for rows in (False, True):
        s = _solver(B, np.tile(W, (B, 1)), np.tile(WN, (B, 1))) if rows else _solver(B)
        s.set_cost_scaling(DT, 1.0)
        s.set_weights(0.5 * W, 0.25 * WN)
        res.append(_closed_loop(s, oracle, x0, yr, ye, 20, 5))
    _same(*res)
    assert not np.array_equal(res[0][0][0], ra[0][0])


# ---- 3. row independence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ah,kick", [(0, 1.0), (1, 1.0), (0, 3.0)])
def test_rows_independent_under_permutation(oracle, ah, kick):
    """Permuting instances together with their weight rows permutes every output: a kernel that read a compact slot's row instead
    of the home instance's would fail here.  Kick 3 m/s: rows the active-set solves do not settle go through the interior-point
    fall-back twins (k_ipm_rest_w, res != 0) with NON-uniform rows; their wave-mates differ between the two runs, so they are
    compared to 5e-6 (the bound of the interior point at a tight tol, tests/test_gpu_parity.py), the others as for ah."""
    B, N = 2048, 50
    rng = np.random.default_rng(90 + ah + int(kick))
    Wr, WNr = random_rows(rng, B)
    x0, x, u, yr, ye = _kicked(oracle, B, N, Wr, WNr, 12, kick=kick, active_horizon=ah)
    perm = rng.permutation(B)
    outs = []
    for pi in (np.arange(B), perm):
        s = _solver(B, Wr[pi], WNr[pi], active_horizon=ah, tol=QP_TOL)
        s.set_x0(x0[pi]); s.set_yref(yr[pi], ye[pi]); s.set_iterate(x[pi], u[pi])
        s.solve(1)
        st, it, rs = s.stats()
        xg, ug = s.get_iterate()
        outs.append((xg, ug, st, it, rs))
        s.close()
    (xa, ua, sa, ia, ra), (xb, ub, sb, ib, rb) = outs
    n_ipm = int(((ib > 0) & (rb != 0.0) & (sb == 0)).sum())
    print(f"ah {ah} kick {kick}: constrained {(ib > 0).sum()}, interior-point rows {n_ipm}, status counts {np.bincount(sb)}")
    assert (ia[perm] > 0).sum() > B // 10
    assert n_ipm > 0                                              # (measured 11 / 12 / 284 rows: the fall-back twins are in)
    assert np.array_equal(sa[perm], sb)
    if kick > 1.0:
        ok = sb == 0
        ipm = ok & ((rb != 0.0) | (ra[perm] != 0.0))
        exact = ok & ~ipm
        assert np.array_equal(xa[perm][exact], xb[exact]) and np.array_equal(ua[perm][exact], ub[exact])
        assert np.abs(xa[perm][ipm] - xb[ipm]).max() <= 5e-6 and np.abs(ua[perm][ipm] - ub[ipm]).max() <= 5e-6
    elif ah == 0:
        assert np.array_equal(xa[perm], xb) and np.array_equal(ua[perm], ub) and np.array_equal(ia[perm], ib)
    else:
        for k in (0, 1):
            assert np.abs(ua[perm][:, k] - ub[:, k]).max() < 1e-8
        assert np.abs(xa[perm][:, 4] - xb[:, 4]).max() < 1e-8
        assert ((ia[perm] > 0) == (ib > 0)).all()


# ---- 4. setter semantics ---------------------------------------------------------------------------------------------
def _one_step(s, x0, yr, ye, it=None):
    """one RTI step from the iterate `it` = (x, u) (None: hover-initialised)"""
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    s.set_x0(x0); s.set_yref(yr, ye)
    if it is None:
        s.init_iterate(INIT_HOVER)
    else:
        s.set_iterate(*it)
    s.solve(1)
    return s.get_iterate()


def test_setter_semantics(oracle):
    import torch
    from crazyflie_nmpc_amd.solver import INIT_HOVER, CfnmpcError
    B, N = 256, 50
    rng = np.random.default_rng(4)
    Wr, WNr = random_rows(rng, B)
    W, WN = default_weights()
    x0, xk, uk, yr, ye = _kicked(oracle, B, N, Wr, WNr, 41)          # (the kicked state and iterate of the rows Wr, WNr)
    s = _solver(B)
    bytes0 = s.workspace_bytes
    for a, b in zip(s.weights_batch(), (np.tile(W, (B, 1)), np.tile(WN, (B, 1)))):
        assert np.array_equal(a, b)
    # round trip, NULL parts
    s.set_weights_batch(Wr, None)
    assert np.array_equal(s.weights_batch()[0], Wr) and np.array_equal(s.weights_batch()[1], np.tile(WN, (B, 1)))
    s.set_weights_batch(None, WNr)
    assert np.array_equal(s.weights_batch()[0], Wr) and np.array_equal(s.weights_batch()[1], WNr)
    assert s.workspace_bytes >= bytes0 + B * 32 * 8                           # cfnmpc_workspace_bytes counts the table
    base = _one_step(s, x0, yr, ye, (xk, uk))
    # bad rows are refused and leave the rows in force
    for bad, col in ((np.nan, 2), (np.inf, 2), (-1.0, 2), (0.0, 14), (-1.0, 15)):
        q = Wr.copy(); q[17, col] = bad
        with pytest.raises(CfnmpcError):
            s.set_weights_batch(q, None)
    for bad in (np.nan, np.inf, -1.0):
        q = WNr.copy(); q[B - 1, 5] = bad
        with pytest.raises(CfnmpcError):
            s.set_weights_batch(Wr, q)
    with pytest.raises(ValueError):
        s.set_weights_batch(Wr[:, :16], None)
    with pytest.raises(ValueError):
        s.set_weights_batch(None, WNr[:B - 1])
    assert np.array_equal(s.weights_batch()[0], Wr) and np.array_equal(s.weights_batch()[1], WNr)
    again = _one_step(s, x0, yr, ye, (xk, uk))
    assert np.array_equal(base[0], again[0]) and np.array_equal(base[1], again[1])
    # device tensors equal host arrays
    d = _solver(B)
    d.set_weights_batch(torch.tensor(Wr, device="cuda"), torch.tensor(WNr, device="cuda"))
    assert np.array_equal(d.weights_batch()[0], Wr) and np.array_equal(d.weights_batch()[1], WNr)
    dev = _one_step(d, x0, yr, ye, (xk, uk))
    assert np.array_equal(base[0], dev[0]) and np.array_equal(base[1], dev[1])
    # set_weights over rows replaces the part in every row
    s.set_weights(None, 2.0 * WN)
    assert np.array_equal(s.weights_batch()[0], Wr) and np.array_equal(s.weights_batch()[1], np.tile(2.0 * WN, (B, 1)))
    t = _solver(B, Wr, np.tile(2.0 * WN, (B, 1)))
    a, b = _one_step(s, x0, yr, ye, (xk, uk)), _one_step(t, x0, yr, ye, (xk, uk))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[1], base[1])
    # cost scaling before and after the rows = pre-scaled rows
    pre = _one_step(_solver(B, DT * Wr, 3.0 * WNr), x0, yr, ye, (xk, uk))
    for order in ("before", "after"):
        c = _solver(B)
        if order == "before":
            c.set_cost_scaling(DT, 3.0)
        c.set_weights_batch(Wr, WNr)
        if order == "after":
            c.set_cost_scaling(DT, 3.0)
        assert np.array_equal(c.weights_batch()[0], Wr)           # unscaled
        got = _one_step(c, x0, yr, ye, (xk, uk))
        assert np.array_equal(pre[0], got[0]) and np.array_equal(pre[1], got[1]), order
    # refused beside the fused start solve and partial condensing; nothing changes
    for kw in (dict(start_solve=2), dict(start_solve=3), dict(cond_N2=10)):
        f = _solver(B, **kw)
        with pytest.raises(CfnmpcError):
            f.set_weights_batch(Wr, WNr)
        assert np.array_equal(f.weights_batch()[0], np.tile(W, (B, 1)))
        f.close()
    # captured step graph: new rows take effect in a replay of a graph captured BEFORE the update
    W2, WN2 = random_rows(np.random.default_rng(5), B)
    res = []
    for variant in ("graph", "plain"):
        g = _solver(B, Wr, WNr, step_graph=1 if variant == "graph" else 0)
        g.set_x0(x0); g.set_yref(yr, ye); g.set_iterate(xk, uk)
        g.solve(1); g.solve(1)
        g.set_weights_batch(W2, WN2)
        g.solve(1); g.solve(1)
        res.append(g.get_iterate())
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    h = _solver(B, Wr, WNr, step_graph=1)
    h.set_x0(x0); h.set_yref(yr, ye); h.set_iterate(xk, uk)
    for _ in range(4):
        h.solve(1)
    assert np.abs(h.get_iterate()[1] - res[0][1]).max() > 1e-6


# ---- 6. sensitivities ------------------------------------------------------------------------------------------------
def test_sensitivities_use_the_rows(oracle):
    """eval_sens_x0 after a kicked step with rows against tests/test_sens_cpu.py::sens_ref on the engine's blocks and active
    set with the row's own Qd, Rd, QNd (1e-8 relative, the TOL of tests/test_gpu_sens.py); a change of weights afterwards
    invalidates the evaluation until the next solve."""
    from test_sens_cpu import sens_ref
    from crazyflie_nmpc_amd.solver import CfnmpcError
    B, N, TOL = 128, 50, 1e-8
    rng = np.random.default_rng(8)
    Wr, WNr = random_rows(rng, B)
    x0, xk, uk, yr, ye = _kicked(oracle, B, N, Wr, WNr, 43)
    s = _solver(B, Wr, WNr, tol=QP_TOL)
    _one_step(s, x0, yr, ye, (xk, uk))
    st = s.stats()[0]
    assert (st == 0).all()
    s.eval_sens_x0()
    du, _ = s.sens_x0(0, N)
    _, dx = s.sens_x0(0, N + 1)
    act = s.sens_active()
    A, Bm, _b = s.get_linearisation()
    assert (act.reshape(B, -1) != 0).any(axis=1).mean() >= 0.2
    for i in range(B):
        ru, rx = sens_ref(A[i], Bm[i], Wr[i, :13], Wr[i, 13:], WNr[i], act[i])
        assert np.abs(du[i] - ru).max() <= TOL * max(1.0, np.abs(ru).max()), i
        assert np.abs(dx[i] - rx).max() <= TOL * max(1.0, np.abs(rx).max()), i
    s.set_weights_batch(Wr, None)
    with pytest.raises(CfnmpcError):
        s.sens_x0(0)
    s.solve(1); s.eval_sens_x0()
    s.sens_x0(0)


# ---- 7. fleet and multi ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ah", [0, 1])
def test_fleet_and_multi_match_single_solvers(oracle, ah):
    """Rows in the caller's order give, per vehicle, the same u0 as a BatchSolver of that horizon given that vehicle's row:
    every object runs the kicked family itself (3 closed-loop steps with the rows in force, the velocity kick, one more step)
    on the same plant states, compared step by step."""
    from crazyflie_nmpc_amd import default_opts, parallel, sim
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.solver import INIT_HOVER, CfnmpcError
    rng = np.random.default_rng(19 + ah)
    B = 333
    hz = np.array([30, 50, 100])[np.arange(B) % 3]                  # interleaved
    Wr, WNr = random_rows(rng, B)
    x0 = oracle.sample_hover_x0(rng, B, scale=1.0)
    kick = rng.normal(0, 1.0, (B, 3))
    yref, yref_e = regulation(oracle, B, 100)

    def same(a, b):
        if ah == 0:
            assert np.array_equal(a, b)
        else:
            assert np.abs(a - b).max() <= 1e-8

    def single(idx, n):
        s = _solver(len(idx), Wr[idx].copy(), WNr[idx].copy(), N=int(n), active_horizon=ah)
        s.set_yref(yref[idx, :n].copy(), yref_e[idx].copy()); s.set_x0(x0[idx].copy()); s.init_iterate(INIT_HOVER)
        return s

    def loop(obj, parts, sync=False):
        """the kicked family on `obj`, the single solvers `parts` = [(idx, solver)] in lockstep -> u0 of the last step"""
        x = x0.copy()
        for t in range(4):
            if t == 3:
                x[:, 7:10] += kick
            obj.set_x0(x); obj.solve(1)
            if sync:
                obj.sync()
            u = obj.get_u(0)
            for idx, sv in parts:
                sv.set_x0(x[idx].copy()); sv.solve(1)
                same(sv.get_u(0), u[idx])
            x = sim(x, u, DT, 1)
        return x, u

    f = MixedHorizonFleet(hz, active_horizon=ah)
    f.set_weights_batch(Wr, WNr)
    f.set_yref(yref, yref_e); f.set_x0(x0); f.init_iterate(INIT_HOVER)
    buckets = [(idx, int(n)) for n, idx in f.buckets()]
    xk, uf = loop(f, [(idx, single(idx, n)) for idx, n in buckets])
    st, it = f.stats()[:2]
    assert (st == 0).all() and (it > 0).sum() > B // 10
    # a bad row in the LAST bucket leaves every bucket unchanged: the same step again gives the same inputs
    q = Wr.copy(); q[buckets[-1][0][-1], 13] = 0.0
    with pytest.raises(CfnmpcError):
        f.set_weights_batch(0.5 * q, None)
    g = MixedHorizonFleet(hz, active_horizon=ah)
    g.set_weights_batch(Wr, WNr)
    g.set_yref(yref, yref_e); g.set_x0(x0); g.init_iterate(INIT_HOVER)
    with pytest.raises(CfnmpcError):
        g.set_weights_batch(0.5 * q, None)
    assert np.array_equal(loop(g, [])[1], uf)
    # multi: two shards on device 0, uniform horizon and mixed horizons
    N = 50
    opts = default_opts(active_horizon=ah)
    m = parallel.MultiGpuFleet(B, [0, 0], opts)
    m.set_weights_batch(Wr, WNr)
    q = Wr.copy(); q[B - 1, 2] = np.nan
    with pytest.raises(CfnmpcError):
        m.set_weights_batch(q, WNr)                                # (refused as a whole: the rows above stay in force)
    m.set_x0(x0); m.set_yref(yref[:, :N].copy(), yref_e); m.init_iterate(INIT_HOVER)
    loop(m, [(idx, single(idx, N)) for idx in (np.arange(lo, min(lo + 111, B)) for lo in range(0, B, 111))], sync=True)
    mh = parallel.MultiGpuFleet(B, [0, 0], opts, horizons=hz)
    mh.set_weights_batch(Wr, WNr)
    q = WNr.copy(); q[B - 1, 0] = -1.0
    with pytest.raises(CfnmpcError):
        mh.set_weights_batch(Wr, q)
    mh.set_x0(x0); mh.set_yref(yref, yref_e); mh.init_iterate(INIT_HOVER)
    umh = loop(mh, [(idx, single(idx, n)) for idx, n in buckets], sync=True)[1]
    same(umh, uf)                                                  # (and so unchanged by the refused call)


# ---- 5. SQP ----------------------------------------------------------------------------------------------------------
def _gpu_sqp(Wr, WNr, x0, yr, ye, tol):
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    s = _solver(x0.shape[0], Wr, WNr, tol=QP_TOL)
    s.set_x0(x0); s.set_yref(yr, ye); s.init_iterate(INIT_HOVER)
    s.solve_sqp(100, tol, tol, tol)
    st, it, _ = s.sqp_stats()
    xg, ug = s.get_iterate()
    s.close()
    return st, it, xg, ug


def _referee(oracle, rows, xg, ug, x0, yr, ye, Wr, WNr, tol):
    for i in rows:
        xr, ur, qp = ref_step(oracle, xg[i], ug[i], x0[i], yr[i], ye[i], Wr[i], WNr[i])
        step = max(np.abs(xr - xg[i]).max(), np.abs(ur - ug[i]).max())
        if step > 10 * tol:   # (the FP64 dense solve against the extended-precision referee, as in test 1 and in the pattern test)
            ref = oracle.solve_qp_refined(qp)
            step = max(np.abs(ref["dx"]).max(), np.abs(ref["du"]).max())
        assert step <= 10 * tol, (i, step)
        assert max(np.abs(qp.b).max(), np.abs(qp.dx0).max()) <= tol, i


def test_sqp_with_rows_ends_with_status_0(oracle):
    """solve_sqp with weight rows on unkicked inputs (hover states of scale 0.25, where the full Gauss-Newton steps contract
    for every row: tests/test_weights_cpu.py::test_sqp_reference_counts) ends with status 0 on EVERY row, and at 8 sampled rows
    the QP built by the oracle at the returned point with the row's OWN weights has a step within 10 tol_step and defects within
    tol_eq (the bounds of tests/test_gpu_sqp.py::test_sqp_converged_point_against_independent_referee)."""
    from test_weights_cpu import sqp_case
    TOL = 1e-9
    Wr, WNr, x0, yr, ye = sqp_case(oracle, 0.25)
    st, it, xg, ug = _gpu_sqp(Wr, WNr, x0, yr, ye, TOL)
    print("scale 0.25: status counts", np.bincount(st), "max sqp_iter", it.max())
    assert (st == 0).all(), np.bincount(st)
    _referee(oracle, np.random.default_rng(0).choice(x0.shape[0], 8, replace=False), xg, ug, x0, yr, ye, Wr, WNr, TOL)


def test_sqp_with_rows_matches_restatement_at_scale_1(oracle, cref):
    """On the inputs of that referee test itself (scale 1) the issue's criterion "ends with status 0" is MISSED, with and
    without rows: full Gauss-Newton steps leave 9 of 64 rows oscillating at max_iter with the default weights and 35 of 64
    with the rows.  That is the iteration, not the engine: the C restatement run row by row with the
    row's weights in its Opts ends every row with the same status, and the converged rows after the same number of
    iterations give or take one (a convergence test that falls within rounding of tol at one iteration).  No row may end
    with a QP failure, and 8 converged rows pass the referee check."""
    from test_weights_cpu import ref_sqp, sqp_case
    TOL = 1e-9
    Wr, WNr, x0, yr, ye = sqp_case(oracle, 1.0)
    st, it, xg, ug = _gpu_sqp(Wr, WNr, x0, yr, ye, TOL)
    st_r, it_r = ref_sqp(cref, oracle, x0, yr, ye, Wr, WNr, 100, TOL)
    print("scale 1: status counts", np.bincount(st, minlength=5), "restatement", np.bincount(st_r, minlength=5))
    assert not (st == 4).any()
    assert np.array_equal(st, st_r), np.flatnonzero(st != st_r)
    conv = np.flatnonzero(st == 0)
    assert np.abs(it[conv] - it_r[conv]).max() <= 1, (it[conv], it_r[conv])
    assert conv.size >= 16
    _referee(oracle, np.random.default_rng(0).choice(conv, 8, replace=False), xg, ug, x0, yr, ye, Wr, WNr, TOL)


# ---- 8. full size ----------------------------------------------------------------------------------------------------
def test_full_size_with_rows(oracle, cref):
    """The pattern of tests/test_gpu_full_size.py::test_full_size_properties_and_spot_parity with weight rows: 65 536 instances
    (its inputs, seed 20200103), random rows (seed 71), default options -- the monolithic k_as twin at its real fleet size --,
    3 closed-loop steps through sim.  Spot parity on 192 rows (sample seed 1) against the C restatement called with B = 1 and
    that row's weights in its Opts, carried along from step to step; a second solver fed the same inputs returns bitwise the
    same iterate and statistics."""
    from crazyflie_nmpc_amd import sim
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B, N = 65536, 50
    x0 = oracle.sample_hover_x0(np.random.default_rng(20200103), B, scale=1.0)
    yref, yref_e = regulation(oracle, B, N)
    Wr, WNr = random_rows(np.random.default_rng(71), B)
    s, s2 = _solver(B, Wr, WNr), _solver(B, Wr, WNr)
    for o in (s, s2):
        o.set_x0(x0); o.set_yref(yref, yref_e); o.init_iterate(INIT_HOVER)
    x = x0.copy()
    idx = np.random.default_rng(1).choice(B, 192, replace=False)
    xr = np.repeat(x0[idx, None, :], N + 1, 1).copy(); ur = np.full((len(idx), N, 4), oracle.HOV_W)
    opts = [cref.default_opts(N, W=Wr[i], WN=WNr[i], tol=1e-8, active_set=1) for i in idx]
    for t in range(3):
        s.set_x0(x); s.solve(1)
        st, it, rs = s.stats()
        xg, ug = s.get_iterate()
        assert (st == 0).all(), np.bincount(st)
        assert np.abs(xg[:, 0, :] - x).max() < 1e-14
        assert ug.min() >= -1e-8 and ug.max() <= 22.0 + 1e-8
        frac = (it > 0).mean()
        print(f"step {t}: constrained fraction {frac:.4f}, of the sample {int((it[idx] > 0).sum())}")
        assert 0.02 < frac < 0.8, frac
        s2.set_x0(x); s2.solve(1)
        st2, it2, rs2 = s2.stats()
        x2, u2 = s2.get_iterate()
        assert np.array_equal(xg, x2) and np.array_equal(ug, u2)
        assert np.array_equal(st, st2) and np.array_equal(it, it2) and np.array_equal(rs, rs2)
        for r, i in enumerate(idx):
            st_r, it_r, _, _ = cref.rti_step(opts[r], xr[r:r + 1], ur[r:r + 1], x[i:i + 1].copy(), yref[i:i + 1].copy(),
                                             yref_e[i:i + 1].copy())
            assert st_r[0] == 0 and (it[i] > 0) == (it_r[0] > 0), (t, i, st_r, it[i], it_r)
        assert np.abs(ug[idx] - ur).max() < 1e-8 and np.abs(xg[idx] - xr).max() < 1e-8
        xr[:] = xg[idx]; ur[:] = ug[idx]
        x = sim(x, ug[:, 0, :].copy(), T=0.015, steps=1)
