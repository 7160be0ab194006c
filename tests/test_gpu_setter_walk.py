"""GPU suite: a solver's setter history leaves no trace in its results.

A solver walked through a sequence of setter calls, with solves between them (tests/setter_walk.py: walk, run), must equal a
FRESH solver set directly to the final state (apply), bit for bit: the getters, three RTI steps from one iterate, the NLP
evaluation and the sensitivities.  What is in force comes from a model of the rules of include/cfnmpc.h (InForce), never from the
host code under test.  The first of the three steps is also held to the exact QP of the final state on twelve rows (1e-8, _agree of
tests/test_gpu_disturbance.py with oracle.solve_qp_refined as referee): "fresh" is anchored to the truth, and disturbance rows,
weight rows and stage boxes meet on the constrained-QP path.  tests/test_setter_walk_cpu.py checks on the CPU that the walk set
reaches the special cases and that the twelve rows are a test.

Bit equality is the criterion: a captured solver equals a plain one bit for bit (test_captured_step_graph_is_bit_identical), and
test_two_fresh_solvers_are_bit_equal below holds two fresh solvers with one state to it on every route before any walk runs.

A comparison at the end of a walk alone cannot see most of what it is after: nearly every setter invalidates the captured steps
and rewrites its table, so a later op covers an earlier op's missing invalidation or stale table.  Behind every setter op the
walked solver is therefore also held to a fresh solver set to the state so far (_checkpoint: two steps, bit for bit).

Measured on an MI355X: the control and all 26 walk cells pass; worst error against the exact QP 5.7e-9 (default, step_graph = 1,
as_dense = -1), 5.5e-9 (active_set = 0), 1.7e-9 (forward_split = 1); no difference in any bit, no defect found in the host code.
That the file can fail, on two builds with host logic made wrong on purpose: cfnmpc_set_cost_scaling without its
invalidate_graphs fails the step_graph = 1 walks that call it under uniform weights (N 8 seed 86, N 40 seed 99; with weight rows
in force the call rewrites the table a captured step reads, and nothing is stale) and no other cell; cfnmpc_set_model_params(NULL)
without the nominal upload under disturbance rows fails every cell of the three walks that hold params > dist > params(None)
(N 8 seed 5, N 40 seeds 23 and 40: ten cells, all five routes), each at the checkpoint behind that op, and no other.  With the
comparison at the end alone both wrong builds passed all cells."""
import numpy as np
import pytest

import setter_walk as sw
from test_gpu_disturbance import QP_TOL, _agree

pytestmark = pytest.mark.gpu
TOL = 1e-8
STEPS = 3
ROUTES = {"default": dict(), "step_graph=1": dict(step_graph=1), "active_set=0": dict(active_set=0), "as_dense=-1": dict(as_dense=-1),
          "forward_split=1,as_dense=1": dict(forward_split=1, as_dense=1)}
SPLIT = "forward_split=1,as_dense=1"      # N = 40 only: the shortest horizon forward_split = 1 accepts


def _cells():
    out = [("step_graph=1", N, seed) for N, seed in sw.walk_set()]
    for r in ROUTES:
        if r != "step_graph=1":
            out += [(r, N, seed) for N in sw.HORIZONS if not (r == SPLIT and N != 40) for seed in sw.widest_walks(N)]
    return out


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _solver(N, route, B=sw.B_WALK):
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    return BatchSolver(B, default_opts(N=N, tol=QP_TOL, **ROUTES[route]))


@pytest.fixture(scope="module")
def finals():
    """per walk, once: its ops, the model behind them, the inputs of the comparison and the exact QPs of the checked rows"""
    return {}


def _final(oracle, finals, N, seed):
    if (N, seed) not in finals:
        ops = sw.walk(seed, N)
        m = sw.replay(ops, sw.B_WALK, N)
        finals[(N, seed)] = (ops, m) + sw.final_reference(oracle, m, seed)
    return finals[(N, seed)]


def _hold_getters(s, m, who):
    """the getters of a solver against the model, exactly (polynomial reference rows: A and B exactly, the model to the bound of
    tests/test_gpu_poly.py) -> comparisons made"""
    W, WN = s.weights_batch()
    Wm, WNm = m.weights_batch()
    assert _bits(W, Wm) and _bits(WN, WNm), (who, "weights_batch")
    assert _bits(s.model_params(), m.model_params()), (who, "model_params")
    assert _bits(s.disturbance(), m.disturbance()), (who, "disturbance")
    assert s.erk_steps == m.erk, (who, "erk_steps")
    y, ye = s.yref()
    ym, yem, exact = m.yref()
    assert _bits(y[exact], ym[exact]) and _bits(ye[exact], yem[exact]), (who, "yref")
    if not exact.all():
        e = max(np.abs(y[~exact] - ym[~exact]).max(), np.abs(ye[~exact] - yem[~exact]).max())
        assert e <= 1e-11 * max(1.0, np.abs(ym[~exact]).max()), (who, "yref, polynomial rows", e)
    return 7


def _compare(oracle, a, b, m, inputs, ref, what):
    """steps 3 to 7 of the comparison -> (bit comparisons made, worst error against the exact QP, rows with an input on the box)"""
    from crazyflie_nmpc_amd import sim
    x0, x, u, _y, _ye = inputs
    n_bits = _hold_getters(a, m, what + ": walked") + _hold_getters(b, m, what + ": fresh")
    ya, yb = a.yref(), b.yref()
    assert _bits(ya[0], yb[0]) and _bits(ya[1], yb[1]), (what, "yref of the two solvers")
    n_bits += 2
    for s in (a, b):
        s.set_x0(x0); s.set_iterate(x, u)
    xk, worst, n_con = x0, 0.0, 0
    lb, ub = m.bounds()
    for step in range(STEPS):
        for s in (a, b):
            s.set_x0(xk); s.solve(1)
        (xa, ua), (xb, ub_) = a.get_iterate(), b.get_iterate()
        sa, sb = a.stats(), b.stats()
        assert _bits(xa, xb) and _bits(ua, ub_), (what, "iterate after step", step, int((xa != xb).any(axis=(1, 2)).sum()), "rows differ",
                                                  float(np.abs(xa - xb).max()), float(np.abs(ua - ub_).max()))
        for k, (p, q) in enumerate(zip(sa, sb)):
            assert _bits(p, q), (what, "stats", k, "after step", step)
        n_bits += 5
        if step == 0:
            for i, (xr, ur, qp, _referee) in ref.items():
                assert sa[0][i] == 0, (what, i, sa[0][i])
                e = _agree(oracle, xa[i], ua[i], xr, ur, qp, x[i], u[i], TOL)
                worst = max(worst, e)
                n_con += int(((ua[i] <= lb[i] + 1e-9) | (ua[i] >= ub[i] - 1e-9)).any())
                assert e <= TOL, (what, i, e)
        xk = sim(xk, a.get_u(0), T=sw.DT, steps=1, params=m.p, dist=m.d)
    for s in (a, b):
        s.eval_nlp()
    for k, (p, q) in enumerate(zip(a.nlp_stats(), b.nlp_stats())):
        assert _bits(p, q), (what, "nlp_stats", k)
    for s in (a, b):
        s.eval_sens_x0()
    (dua, _), (dub, _) = a.sens_x0(0, a.N), b.sens_x0(0, b.N)
    (_, dxa), (_, dxb) = a.sens_x0(0, a.N + 1), b.sens_x0(0, b.N + 1)
    assert _bits(dua, dub) and _bits(dxa, dxb), (what, "sens_x0")
    assert _bits(a.sens_active(), b.sens_active()), (what, "sens_active")
    return n_bits + 5, worst, n_con


def _checkpoint(oracle, a, route, m, seed, j, what):
    """Behind setter op j of a walk, while the model can state what is in force (no tightened box, polynomial rows written under
    the parameter rows in force): two RTI steps of the walked solver, one per parity of its captured steps, and of a fresh solver
    set to the state so far, from one x0 and iterate -- iterate and stats bit for bit.  An error that a later setter would cover
    (most of them invalidate the captured steps and rewrite a table) shows here.  The walked solver gets its x0 and iterate back.
    -> bit comparisons made"""
    if m.tight or not m.poly_follows_params():
        return 0
    x0, x, u, _y, _ye = sw.final_inputs(oracle, m, 1000 * seed + j)
    keep = a.get_iterate()
    b = _solver(m.N, route)
    try:
        b.set_x0(x0)
        sw.apply(b, m)
        for s in (a, b):
            s.set_x0(x0); s.set_iterate(x, u)
        for step in range(2):
            for s in (a, b):
                s.solve(1)
            (xa, ua), (xb, ub) = a.get_iterate(), b.get_iterate()
            assert _bits(xa, xb) and _bits(ua, ub), (what, "behind op", j, "step", step, "iterate", float(np.abs(xa - xb).max()),
                                                   float(np.abs(ua - ub).max()))
            for k, (p, q) in enumerate(zip(a.stats(), b.stats())):
                assert _bits(p, q), (what, "behind op", j, "step", step, "stats", k)
    finally:
        b.close()
    a.set_x0(a._walk_x0); a.set_iterate(*keep)
    return 10


# ---- the control: two fresh solvers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
def test_two_fresh_solvers_are_bit_equal(oracle, finals, route):
    """two fresh solvers given apply() with one state (that of the first walk of each horizon): the whole comparison, bit for bit"""
    for N in sw.HORIZONS:
        if route == SPLIT and N != 40:
            continue
        seed = sw.SEEDS[N][0]
        _ops, m, inputs, ref = _final(oracle, finals, N, seed)
        a, b = _solver(N, route), _solver(N, route)
        try:
            for s in (a, b):
                s.set_x0(inputs[0])
                sw.apply(s, m)
            n, worst, n_con = _compare(oracle, a, b, m, inputs, ref, f"control {route} N {N}")
        finally:
            a.close(); b.close()
        print(f"control, route {route}, N {N} (state of walk {seed}: {m.writer()}, {[k for k, v in m.features().items() if v]}): "
              f"{n} bit comparisons, worst error against the exact QP {worst:.2e}, {n_con} of {len(ref)} checked rows on the box")


# ---- the walks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,N,seed", _cells(), ids=lambda v: str(v))
def test_walked_solver_equals_fresh_solver(oracle, finals, route, N, seed):
    """Solver A runs walk (seed, N) (disturbance rows alternately as host arrays and device tensors), solver B is fresh and set to
    the final state; getters against the model, three RTI steps with the plant between them, eval_nlp and eval_sens_x0: A and B
    bit for bit; A's first step against the exact QP on the checked rows (1e-8).  Behind every setter op on the way A is also
    held to a fresh solver set to the state so far (_checkpoint).  Captured step graphs offer no count of their recaptures: a
    missed one shows as a difference."""
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    ops, m, inputs, ref = _final(oracle, finals, N, seed)
    what = f"walk {seed} N {N} route {route}"
    a, b = _solver(N, route), _solver(N, route)
    log = []
    try:
        a._walk_x0 = sw.start_state(oracle, seed, N)
        a.set_x0(a._walk_x0)
        a.init_iterate(INIT_HOVER)
        n_chk = [0, 0]

        def after(mk, j, op):
            c = _checkpoint(oracle, a, route, mk, seed, j, f"{what}, {sw.kind_of(op)}")
            n_chk[0] += c
            n_chk[1] += c > 0
        ma = sw.run(a, ops, log, after)
        assert not ma.tight and ma.poly_follows_params()
        b.set_x0(inputs[0])
        sw.apply(b, m)
        n, worst, n_con = _compare(oracle, a, b, m, inputs, ref, what)
    finally:
        print(f"{what}: ops run: {' '.join(k.replace('set_', '') for k in log)}")
        a.close(); b.close()
    print(f"{what}: final state {m.writer()} references, {[k for k, v in m.features().items() if v]}; {n_chk[1]} setter ops checked "
          f"on the way ({n_chk[0]} bit comparisons), {n} bit comparisons at the end, worst error "
          f"against the exact QP {worst:.2e} (bound {TOL:.0e}), {n_con} of {len(ref)} checked rows on the box")


# ---- one fleet ---------------------------------------------------------------------------------------------------------------------
def test_walked_fleet_equals_fresh_fleet(oracle):
    """The eleven-vehicle, three-bucket fleet of tests/test_gpu_fleet_rows.py through one sequence of the fleet setters -- stage
    boxes, disturbance, erk steps, weight rows, model parameters, cost scaling, each on and off once, solves between them, in an
    order the solver walks do not use: with everything on it equals a fresh fleet given the same data in another order, with
    everything off again it equals a fresh fleet that never had any; get_u, get_x and stats, bit for bit."""
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    from test_disturbance_cpu import random_dist
    from test_gpu_fleet_rows import BOX, HORIZONS, NMAX, NMIN, _data
    from test_model_params_cpu import random_params
    B = len(HORIZONS)
    d = _data(B, NMAX, 11)
    rng = np.random.default_rng(77)
    p, dist = random_params(rng, B), random_dist(rng, B)
    lb, ub = rng.uniform(0.0, 4.0, (B, NMAX, 4)), rng.uniform(19.0, 22.0, (B, NMAX, 4))

    def fleet():
        f = MixedHorizonFleet(HORIZONS, tol=QP_TOL)
        f.set_box(*BOX)
        f.set_x0(d["x0"]); f.set_yref(d["yref"], d["yref_e"]); f.init_iterate(INIT_HOVER)
        return f

    def outputs(f):
        f.set_x0(d["x0"]); f.init_iterate(INIT_HOVER)
        out = []
        for _ in range(2):
            f.solve(1)
            out += [f.get_u(0), f.get_u(NMIN - 1), f.get_x(1), f.get_x(NMIN)] + list(f.stats())
        return out

    on = [lambda f: f.set_box_stages(lb, ub), lambda f: f.set_disturbance(dist), lambda f: f.set_erk_steps(2),
          lambda f: f.set_weights_batch(d["W"], d["WN"]), lambda f: f.set_model_params(p), lambda f: f.set_cost_scaling(2.0, 0.5)]
    off = [lambda f: f.set_disturbance(None), lambda f: f.set_cost_scaling(1.0, 1.0), lambda f: f.set_model_params(None),
           lambda f: f.set_box_stages(None, None), lambda f: f.set_erk_steps(1), lambda f: f.set_weights_batch(None, None)]
    w, full, plain = fleet(), fleet(), fleet()
    try:
        for call in on:
            call(w); w.solve(1)
        for call in reversed(on):
            call(full)
        got, want = outputs(w), outputs(full)
        n = 0
        for k, (a, b) in enumerate(zip(got, want)):
            assert _bits(a, b), ("everything on", k)
            n += 1
        assert (got[4] == 0).all() and (got[5] > 0).any(), (got[4], got[5])       # (status 0; constrained rows are in)
        for call in off:
            call(w); w.solve(1)
        got, want = outputs(w), outputs(plain)
        for k, (a, b) in enumerate(zip(got, want)):
            assert _bits(a, b), ("everything off again", k)
            n += 1
        print(f"fleet: {n} bit comparisons; qp_iter with everything off {got[5].tolist()}")
    finally:
        w.close(); full.close(); plain.close()
