"""GPU suite: every reachable cell of the kernel-variant tables runs one RTI step.

The launchers of csrc/cfnmpc_kernels.hip look their kernel up in one table per family (linearisation, matrix-free forward
sweeps, constrained QP).  The features' own route tests walk one axis each; here the products run: model x erk x sweep for the
start solve, QP structure x box x weights for the constrained QPs, at the smallest shape that still exercises the indexing --
B = 67 (two 64-instance groups, the second nearly empty; 17 row-group waves, the last partly filled), N = 40 (the shortest
horizon forward_split = 1 accepts).

Every route over the same data solves the same QP, so the reference (tests/test_gpu_disturbance.py: _ref_step, _agree with
oracle.solve_qp_refined as referee, 1e-8 at the solver tol 1e-11) is computed once per data set for 12 seeded rows, always
rows 64 and 66 among them, and every route is also compared with every other route of its data set on those rows.

Data sets (inputs of test_gpu_disturbance.py::test_rti_step_matches_reference, seed 170 / _inputs seed 11, velocity kicks):
  start solve, kick N(0, 1.5) m/s on two rows of three (the unkicked third keeps rows without an active bound among the checked
    ones: their step is the forward sweep's result alone): model {folded constants, parameter rows, parameter + disturbance
    rows} x M {1, 2};
  constrained QP, kick N(0, 3) m/s on every row (rows the active-set solves leave to the interior-point fall-back: the CPU
    restatement predicts 5 of 67 for scalar box / uniform weights, row 19 of the checked ones among them), folded constants,
    M = 1: box {scalar, per stage} x weights {uniform, per instance}.
Share of the checked rows that touch the box in the reference (condition: >= 20 %; row seed 7 chosen on the CPU with the oracle
alone, SHARE below, asserted per data set): start solve 8 / 12 (folded constants) and 9 / 12 (parameter and disturbance rows),
constrained QP 11 / 12 (scalar box) and 12 / 12 (per-stage box).

The (Params, Args) families have no new case here: k_sqp_check / k_sqp_ls / k_nlp_eval run with the folded constants in
test_gpu_sqp.py, test_gpu_sqp_ls.py and test_gpu_nlp_eval.py, their _par forms in test_gpu_model_params.py (NLP residuals,
full SQP solve in both globalisation modes) and their _dst forms in
test_gpu_disturbance.py::test_nlp_residuals_and_sqp_follow_the_disturbed_dynamics."""
import numpy as np
import pytest

from test_disturbance_cpu import ND, random_dist
from test_gpu_disturbance import QP_TOL, _ref_step
from test_gpu_model_params import _agree, _inputs, _weights
from test_model_params_cpu import NOMINAL, hover, random_params
from test_weights_cpu import random_rows

pytestmark = pytest.mark.gpu
B, N = 67, 40
SEED, ROW_SEED = 170, 7
N_ROWS = 12
TOL = 1e-8          # two exact solves of one QP (smoke(), the features' route tests)

# ---- data sets -------------------------------------------------------------------------------------------------------
START_SETS = [("start", model, M) for model in ("nom", "par", "dst") for M in (1, 2)]
QP_SETS = [("qp", box, w) for box in ("scalar", "stages") for w in ("uniform", "rows")]
# number of the 12 checked rows with an input at its bound in the reference solution (CPU, oracle alone)
SHARE = {("start", "nom", 1): 8, ("start", "nom", 2): 8, ("start", "par", 1): 9, ("start", "par", 2): 9, ("start", "dst", 1): 9,
         ("start", "dst", 2): 9, ("qp", "scalar", "uniform"): 11, ("qp", "scalar", "rows"): 11, ("qp", "stages", "uniform"): 12,
         ("qp", "stages", "rows"): 12}


def checked_rows():
    rest = np.random.default_rng(ROW_SEED).choice(64, N_ROWS - 2, replace=False)
    return sorted(rest.tolist()) + [64, 66]


def stage_box():
    k = np.arange(N)
    lb = np.broadcast_to((1.0 + 0.5 * (k % 2))[None, :, None], (B, N, 4)).copy()
    ub = np.broadcast_to((21.0 - 0.5 * (k % 3))[None, :, None], (B, N, 4)).copy()
    return lb, ub


def make_data(oracle, key):
    """the seeded, velocity-kicked inputs of test_rti_step_matches_reference at (B, N); one draw order for every data set"""
    kind, a, b = key
    model, M = (a, b) if kind == "start" else ("nom", 1)
    rng = np.random.default_rng(SEED)
    p = random_params(rng, B)
    d = random_dist(rng, B)
    if model == "nom":
        p = np.tile(NOMINAL, (B, 1))
    if model != "dst":
        d = np.zeros((B, ND))
    x0, yr, ye = _inputs(oracle, B, N, 11, scale=1.5)
    yr[:, :, 13:] = hover(p)[:, None, None]
    kick = rng.normal(0, 1.5 if kind == "start" else 3.0, (B, 3))
    if kind == "start":
        kick[::3] = 0.0          # (rows the start solve alone decides: no input at the box, the forward sweep's result is the step)
    x0[:, 7:10] += kick
    x = np.repeat(x0[:, None, :], N + 1, 1)
    u = np.repeat(np.repeat(hover(p)[:, None, None], N, 1), 4, 2)
    W, WN = _weights()
    Wr, WNr = np.tile(W, (B, 1)), np.tile(WN, (B, 1))
    lb = ub = None
    if kind == "qp":
        if b == "rows":
            Wr, WNr = random_rows(rng, B)
        if a == "stages":
            lb, ub = stage_box()
    return dict(model=model, M=M, p=p, d=d, x0=x0, yr=yr, ye=ye, x=x, u=u, Wr=Wr, WNr=WNr, rows_w=kind == "qp" and b == "rows",
                lb=lb, ub=ub)


def reference(oracle, c):
    """-> {row: (x + dx, u + du, qp)} and the number of rows with an input at its bound"""
    ref, n_con = {}, 0
    for i in checked_rows():
        lo, hi = (0.0, 22.0) if c["lb"] is None else (c["lb"][i], c["ub"][i])
        xr, ur, qp = _ref_step(oracle, c["x"][i], c["u"][i], c["x0"][i], c["yr"][i], c["ye"][i], c["p"][i], c["d"][i], c["M"],
                               c["Wr"][i], c["WNr"][i], lo, hi)
        n_con += int((ur <= lo + 1e-9).any() or (ur >= hi - 1e-9).any())
        ref[i] = (xr, ur, qp)
    return ref, n_con


@pytest.fixture(scope="module")
def cases():
    return {}


def _case(oracle, cases, key):
    if key not in cases:
        c = make_data(oracle, key)
        c["ref"], c["n_con"] = reference(oracle, c)
        c["out"] = {}
        cases[key] = c
    return cases[key]


# ---- routes ----------------------------------------------------------------------------------------------------------
SWEEPS = [dict(forward_sweep=1, forward_split=-1), dict(forward_split=1), dict(forward_sweep=2)]
STRUCTURES = [dict(active_set=0), dict(as_passes=-1), dict(as_passes=-3, as_dense=-1), dict(as_passes=-3, as_dense=1)]
CELLS = [(k, r) for k in START_SETS for r in SWEEPS]
CELLS += [(k, dict(cond_N2=10)) for k in START_SETS if k[1] != "dst"]       # (no _dst twin: cfnmpc_set_disturbance refuses cond_N2)
CELLS += [(k, r) for k in QP_SETS for r in STRUCTURES]
CELLS += [(("qp", "scalar", "uniform"), dict(start_solve=2, active_set=a)) for a in (0, 1)]


def _id(cell):
    key, route = cell
    return "-".join(str(v) for v in key) + ":" + ",".join(f"{k}={v}" for k, v in route.items())


def _run(c, route):
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    s = BatchSolver(B, default_opts(N=N, tol=QP_TOL, **route))
    if c["M"] != 1:
        s.set_erk_steps(c["M"])
    if c["model"] != "nom":
        s.set_model_params(c["p"])
    if c["model"] == "dst":
        s.set_disturbance(c["d"])
    if c["rows_w"]:
        s.set_weights_batch(c["Wr"], c["WNr"])
    if c["lb"] is not None:
        s.set_box_stages(c["lb"], c["ub"])
    s.set_x0(c["x0"]); s.set_yref(c["yr"], c["ye"]); s.set_iterate(c["x"], c["u"])
    s.solve(1)
    out = s.get_iterate() + tuple(s.stats())
    s.close()
    return out


@pytest.mark.parametrize("cell", CELLS, ids=_id)
def test_cell_matches_reference_and_its_siblings(oracle, cases, cell):
    """One RTI step of one cell against the data set's reference and against the routes of the same data set that ran before.

    Measured on an MI355X, 40 cells: they agree with the reference to 1.7e-10 .. 5.2e-9 and with each other to <= 4.7e-9 (the
    largest: interior point, active_set = 0, against the active-set routes); interior-point fall-back rows (res > 0) in the
    active-set routes of the four QP data sets: 4 - 5, 5, 2, 5 of 67.
    The cell start-dst-2:forward_split=1 (parameter + disturbance rows x 2 RK4 sub-steps x split sweep: k_forward_p1_erk_dst +
    k_forward_p2_erk_dst, the product no route test had) found a miscompiled kernel: as first built, k_forward_p1_erk_dst read
    the high word of one model constant from a register nothing wrote (csrc/cfnmpc_kernels.hip: forward_body), row 3 was
    1.33e-2 from the reference, rows without an active bound up to 4.0e-2 and constrained rows up to 7.7 from the unsplit sweep
    of the same data, every status 0."""
    key, route = cell
    c = _case(oracle, cases, key)
    rows = checked_rows()
    assert c["n_con"] >= 0.2 * len(rows), c["n_con"]
    assert c["n_con"] == SHARE[key], (c["n_con"], SHARE[key])
    xg, ug, st, it, res = _run(c, route)
    worst = 0.0
    for i in rows:
        xr, ur, qp = c["ref"][i]
        assert st[i] == 0, (i, st[i])
        e = _agree(oracle, xg[i], ug[i], xr, ur, qp, c["x"][i], c["u"][i], TOL)
        worst = max(worst, e)
        assert e <= TOL, (i, e)
    n_fb = int(((it > 0) & (res > 0.0) & (st == 0)).sum())
    among = 0.0
    for other, (xo, uo) in c["out"].items():
        among = max(among, np.abs(xg[rows] - xo[rows]).max(), np.abs(ug[rows] - uo[rows]).max())
    print(f"{_id(cell)}: worst {worst:.2e}, among routes {among:.2e}, constrained {(it > 0).sum()}, res > 0 on {n_fb}, "
          f"status counts {np.bincount(st).tolist()}")
    assert among <= TOL, among
    if key[0] == "qp" and route.get("active_set", 1) == 1:
        assert n_fb >= 2, n_fb          # the interior-point fall-back kernel of the cell had rows to solve
    c["out"][_id(cell)] = (xg, ug)
