"""GPU suite: stage-invariant references in the start solve's factorisation (Params.yuni).

cfnmpc_set_yref finds out on the device whether every vehicle's reference rows 1 .. N - 1 equal its row 0 bit for bit; if so the
_u twins of k_factor / k_factor_w read that row once per vehicle instead of once per stage.  Same operands, same order: the twins
must give the SAME BITS as the generic kernels, so every comparison here is numpy.array_equal, never a tolerance.

Workload of every case: per-vehicle different setpoints tiled over the stages, x0 = hover kicked with scale 2 (feasible rows and rows
settled by active-set solves side by side), hover-initialised iterate, three closed-loop RTI steps.  The generic kernel is reached by
moving one entry of the LAST vehicle's LAST stage by one ulp: the whole-fleet flag is then off, and all vehicles but the last see
the same data."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DT = 0.015
STEPS = 3


def _refs(B, N, seed):
    """-> (yref [B][N][17], yref_e [B][13], x0 [B][13]): one setpoint per vehicle, the same row at every stage"""
    from crazyflie_nmpc_amd.synthetic import HOV_W, regulation_row, sample_hover_x0
    rng = np.random.default_rng(seed)
    rows = np.stack([regulation_row((rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 0.4 + rng.uniform(-0.1, 0.1)),
                                    HOV_W * (1.0 + rng.uniform(-0.02, 0.02))) for _ in range(B)])
    yref = np.repeat(rows[:, None, :], N, 1).copy()
    return yref, rows[:, :13].copy(), sample_hover_x0(rng, B, scale=2.0)


def _one_ulp(yref):
    y = yref.copy()
    y[-1, -1, 2] = np.nextafter(y[-1, -1, 2], np.inf)
    return y


def _solver(B, N, weights=None, **kw):
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    s = BatchSolver(B, default_opts(N=N, **kw))
    if weights is not None:
        s.set_weights_batch(*weights)
    return s


def _step(s, x):
    """one closed-loop step -> (everything the step left, next plant state)"""
    from crazyflie_nmpc_amd import sim
    s.set_x0(x); s.solve(1)
    xi, ui = s.get_iterate()
    u0 = s.get_u(0).copy()
    st, it, rs = s.stats()
    return (xi.copy(), ui.copy(), u0, st.copy(), it.copy(), rs.copy()), sim(x, u0, DT, 1)


def _closed_loop(s, yref, yref_e, x0, want_uniform):
    """STEPS steps, then the start solve's factors of the iterate they left -> [step outputs ...] + [K, d, Pchk, status]"""
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    s.set_x0(x0); s.set_yref(yref, yref_e); s.init_iterate(INIT_HOVER)
    assert s.yref_uniform() == want_uniform
    out, x = [], x0.copy()
    for _ in range(STEPS):
        o, x = _step(s, x)
        out.append(o)
    assert s.yref_uniform() == want_uniform
    s.start_factor(1)
    assert s.yref_uniform() == want_uniform
    return out, s.get_factor()


def _same_bits(a, b, rows, what):
    for j, (p, q) in enumerate(zip(a, b)):
        assert np.array_equal(p[rows], q[rows], equal_nan=True), (what, j, int(np.sum(p[rows] != q[rows])))


def _twin_vs_generic(B, N, seed, weights=None, **kw):
    yref, yref_e, x0 = _refs(B, N, seed)
    sa, sb = _solver(B, N, weights, **kw), _solver(B, N, weights, **kw)
    try:
        steps_a, fac_a = _closed_loop(sa, yref, yref_e, x0, True)
        steps_b, fac_b = _closed_loop(sb, _one_ulp(yref), yref_e, x0, False)
    finally:
        sa.close(); sb.close()
    rows = slice(0, B - 1)
    for k, (a, b) in enumerate(zip(steps_a, steps_b)):
        _same_bits(a, b, rows, f"step {k}")
    _same_bits(fac_a, fac_b, rows, "factors")
    it = np.stack([o[4][rows] for o in steps_a]); st = np.stack([o[3][rows] for o in steps_a]); rs = np.stack([o[5][rows] for o in steps_a])
    n_feas, n_as, n_ipm = int((it == 0).sum()), int(((it > 0) & (rs == 0.0)).sum()), int(((it > 0) & (rs != 0.0)).sum())
    print(f"B {B} N {N}: {STEPS} steps x {B - 1} rows bitwise equal; feasible {n_feas}, active-set {n_as}, interior point {n_ipm}, "
          f"status != 0: {int((st != 0).sum())}")
    return n_feas, n_as


@pytest.mark.parametrize("B,N", [(7, 5), (67, 50), (260, 30)])
def test_twin_equals_generic_bitwise(B, N):
    n_feas, n_as = _twin_vs_generic(B, N, 100 + B)
    if B >= 67:
        assert n_feas > 0 and n_as > 0, (n_feas, n_as)   # both kinds of rows ran through the factors under test


def test_twin_equals_generic_bitwise_per_instance_weights():
    from test_weights_cpu import random_rows
    B, N = 67, 50
    n_feas, n_as = _twin_vs_generic(B, N, 7, weights=random_rows(np.random.default_rng(70), B))
    assert n_feas > 0 and n_as > 0, (n_feas, n_as)


def _windows_args(B, N, seed):
    """a tracking window per vehicle out of one trajectory (rows vary over the stages): torch device tensors"""
    import torch
    from crazyflie_nmpc_amd.synthetic import HOV_W, regulation_row
    n_rows = 3 * N + 8
    ph = np.linspace(0.0, 2 * np.pi, n_rows)
    traj = np.stack([regulation_row((0.2 * np.cos(p), 0.2 * np.sin(p), 0.4 + 0.05 * np.sin(2 * p)), HOV_W) for p in ph])
    it = np.random.default_rng(seed).integers(0, n_rows - N - 2, B).astype(np.int32)
    dev = torch.device("cuda:0")
    return (torch.from_numpy(traj).to(dev), torch.ones(B, dtype=torch.int32, device=dev), torch.from_numpy(it).to(dev),
            torch.zeros((B, 3), dtype=torch.float64, device=dev))


def test_flag_follows_the_data():
    """uniform -> set_yref with rows that vary -> uniform again (other setpoints) -> set_yref_windows: after each change one step of
    the long-lived solver equals, bit for bit, the step of a FRESH solver given the same references, iterate and x0 (a stale twin
    would read row 0 where the rows vary; stale rows would show in the third leg)."""
    import torch
    B, N = 67, 30
    y1, ye1, x0 = _refs(B, N, 31)
    y3, ye3, _ = _refs(B, N, 32)
    y2 = y1.copy()
    y2[:, :, :3] += np.linspace(0.0, 0.1, N)[None, :, None]           # a ramp over the stages, every vehicle
    traj, mode, it, des = _windows_args(B, N, 33)
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    s = _solver(B, N)
    fresh = []
    try:
        s.set_x0(x0); s.init_iterate(INIT_HOVER)
        x = x0.copy()
        legs = [("uniform", lambda q: q.set_yref(y1, ye1), True), ("varying", lambda q: q.set_yref(y2, ye1), False),
                ("uniform again", lambda q: q.set_yref(y3, ye3), True),
                ("windows", lambda q: q.set_yref_windows(traj, mode.clone(), it.clone(), des, 15.7777), False)]
        for name, put, want in legs:
            xi, ui = s.get_iterate()
            put(s)
            f = _solver(B, N)
            fresh.append(f)
            f.set_iterate(xi.copy(), ui.copy())
            put(f)
            torch.cuda.synchronize()
            assert s.yref_uniform() == want and f.yref_uniform() == want, name
            o, xn = _step(s, x)
            of, _ = _step(f, x)
            _same_bits(o, of, slice(None), name)
            assert s.yref_uniform() == want, name
            x = xn
    finally:
        s.close()
        for f in fresh:
            f.close()


def test_captured_step_follows_the_flag():
    """step_graph = 1: the references turn from uniform to varying and back between steps; every step of the captured solver equals
    the individually launched one bit for bit (two steps per leg: one per parity of the iterate buffers)."""
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B, N = 67, 30
    y1, ye1, x0 = _refs(B, N, 41)
    y2 = _one_ulp(y1)
    g, p = _solver(B, N, step_graph=1), _solver(B, N)
    try:
        for s in (g, p):
            s.set_x0(x0); s.init_iterate(INIT_HOVER)
        x = x0.copy()
        for leg, (y, want) in enumerate([(y1, True), (y2, False), (y1, True)]):
            for s in (g, p):
                s.set_yref(y, ye1)
            for j in range(2):
                og, xn = _step(g, x)
                op, _ = _step(p, x)
                _same_bits(og, op, slice(None), (leg, j))
                assert g.yref_uniform() == want and p.yref_uniform() == want, (leg, j)
                x = xn
    finally:
        g.close(); p.close()
