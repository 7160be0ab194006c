"""A fleet of any size tiled from 64 QPs whose exact RTI step is known (plain numpy, no GPU).

tests/test_gpu_large_fleet.py needs fleets of 20 483 rows in which EVERY row has a reference, and in which thousands of rows
take the interior-point fall-back; the dense exact QP costs 0.13 s per row on the CPU.  So the fleet is a seeded map tile[B]
onto D = 64 distinct rows at N = 40 (the shortest horizon forward_split accepts), and the reference (test_gpu_disturbance.
_ref_step, oracle.solve_qp_refined as referee exactly as test_gpu_model_params._agree uses it) is computed once per distinct
row and cached at module scope.

The distinct rows (nominal parameters, M = 1, default weights, the iterate held at x0 / hover, solver tol QP_TOL = 1e-11) are
chosen by what the CPU alone sees -- the oracle and cref.rti_step with active_set = 1, "the restatement" -- and the choice is
never revised because of what a GPU returns:

  16 fall-back   the restatement ends in the interior point (res > 0)
  32 active-set  it > 0, res == 0
   8 late        at rest at the reference, the z reference steps down by LATE_STEPS[j] from stage LATE_STAGE on: the QP solved
                 without the box first leaves [0, 22] at a stage >= 24 and is inside it on [0, 24) -- the rows part two of a
                 split forward sweep finds
   8 free        no input at a bound in the exact solution (the restatement's it == 0)

and a row of any kind is kept only if the restatement's step is within TOL / 5 = 2e-9 of the exact step after the referee: its QP is
conditioned well enough for two FP64 solvers to meet at TOL.  The fall-back, active-set and free rows come from a pool built like
test_gpu_variants.make_data (_inputs seed 11, scale 1.5, rng 170, velocity kicks N(0, 3) m/s, 160 rows: 21 fall-back rows, 19 of
them within 2e-9, rows 107 and 141 at 3.2e-9 and 5.5e-9; 134 active-set rows, all within 1.5e-9; 5 free rows); the free rows from
a second, calmer draw without kicks (FREE_SEED, scale 0.5: 30 of 32 free, within 1.3e-11); all 13 late candidates (steps of
0.7 .. 1.9 m) within 9.2e-10, first violations at stages 31 - 38.  tests/test_large_fleet_data_cpu.py recomputes the table."""
import numpy as np

from test_disturbance_cpu import ND, random_dist
from test_gpu_disturbance import QP_TOL, _ref_step
from test_gpu_model_params import _inputs, _weights
from test_model_params_cpu import NOMINAL, hover, random_params

N, D = 40, 64
TOL = 1e-8               # two exact solves of one QP (test_gpu_variants.TOL, smoke())
KEEP = TOL / 5           # the restatement against the exact step
POOL_ROWS, POOL_SEED, INPUT_SEED, KICK = 160, 170, 11, 3.0
FREE_ROWS, FREE_SEED, FREE_SCALE = 32, 12, 0.5
LATE_STAGE, SPLIT = 30, 24
KINDS = ("fallback", "active", "late", "free")
COUNT = dict(fallback=16, active=32, late=8, free=8)
# ---- the kept rows (indices into the pools; the first rows of each kind that meet the criteria, found on the CPU) ----
# (fall-back row 36 meets the criterion at 1.83e-9 only: too close to 2e-9 for a check another host's compiler has to reproduce, left out)
FALLBACK = (1, 3, 11, 18, 29, 40, 41, 44, 53, 63, 64, 88, 105, 112, 119, 133)
ACTIVE = (2, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15, 16, 17, 19, 20, 21, 22, 23, 25, 26, 27, 28, 30, 31, 32, 33, 34, 35, 37, 38, 39)
FREE = (1, 2, 3, 4, 5, 6, 7, 8)
LATE_STEPS = (0.7, 0.9, 1.1, 1.2, 1.4, 1.6, 1.7, 1.9)          # m, downward: first violations at stages 38, 36, 34, 33, 32, 32, 31, 31

# ---- the two fleets of tests/test_gpu_large_fleet.py: rows per kind (what they leave of B: free rows), seed of the map ----
B = 20483                # the last wave and the last 64-instance group ragged
# heavy: adds up to B, every row constrained.  68 % copies of the fall-back rows, not 40 %: the engine's monolithic kernels settle
# 5 - 6 of every 10 such copies by active-set solves where the restatement and the staged structure fall back (measured at 50 %:
# 4208 - 4875 of 10 242 listed by k_as*, 10 232 by the solves + commit structure), and the list has to pass 4 S with a margin
HEAVY = dict(fallback=14000, active=5459, late=1024)
LIGHT = dict(fallback=120, active=600, late=64)
FLEETS = {"heavy": (HEAVY, 31), "light": (LIGHT, 32)}


def pool():
    """the kicked pool: test_gpu_variants.make_data(("qp", "scalar", "uniform")) at POOL_ROWS rows, same draw order"""
    B = POOL_ROWS
    rng = np.random.default_rng(POOL_SEED)
    random_params(rng, B); random_dist(rng, B)          # (make_data's draws for the models this pool does not use)
    import cfnmpc_oracle as oracle
    x0, yr, ye = _inputs(oracle, B, N, INPUT_SEED, scale=1.5)
    yr[:, :, 13:] = hover(NOMINAL)
    x0[:, 7:10] += rng.normal(0, KICK, (B, 3))
    return x0, yr, ye


def free_pool():
    import cfnmpc_oracle as oracle
    x0, yr, ye = _inputs(oracle, FREE_ROWS, N, FREE_SEED, scale=FREE_SCALE)
    yr[:, :, 13:] = hover(NOMINAL)
    return x0, yr, ye


def late_pool(steps):
    """at rest at the reference; the z reference (terminal row included) lower by steps[j] from stage LATE_STAGE on"""
    import cfnmpc_oracle as oracle
    n = len(steps)
    x0, yr, ye = _inputs(oracle, n, N, 0, scale=0.0)
    yr[:, :, 13:] = hover(NOMINAL)
    for j, dz in enumerate(steps):
        yr[j, LATE_STAGE:, 2] -= dz
        ye[j, 2] -= dz
    return x0, yr, ye


def distinct_rows():
    """-> dict(x0 [D][13], yr [D][N][17], ye [D][13], kind [D] (index into KINDS)), kinds in blocks in the order of KINDS"""
    px, pyr, pye = pool()
    fx, fyr, fye = free_pool()
    lx, lyr, lye = late_pool(LATE_STEPS)
    fb, ac, fr = list(FALLBACK), list(ACTIVE), list(FREE)
    x0 = np.concatenate([px[fb], px[ac], lx, fx[fr]])
    yr = np.concatenate([pyr[fb], pyr[ac], lyr, fyr[fr]])
    ye = np.concatenate([pye[fb], pye[ac], lye, fye[fr]])
    kind = np.repeat(np.arange(4), [len(fb), len(ac), len(lx), len(fr)])
    return dict(x0=x0, yr=yr, ye=ye, kind=kind)


def iterate(x0):
    """the iterate every row starts from: the state held at x0, the inputs at hover"""
    B = x0.shape[0]
    return np.repeat(x0[:, None, :], N + 1, 1), np.full((B, N, 4), hover(NOMINAL))


def restatement(cref, x0, yr, ye):
    """one step of the CPU restatement with active_set = 1 at QP_TOL -> x, u, status, it, res"""
    x, u = iterate(x0)
    st, it, res, _ = cref.rti_step(cref.default_opts(N=N, tol=QP_TOL, active_set=1), x, u, x0.copy(), yr.copy(), ye.copy(), nthreads=1)
    return x, u, st, it, res


def exact_step(oracle, x0, yr, ye, u_min=0.0, u_max=22.0):
    """the dense exact QP of one row -> x + dx, u + du, qp"""
    x, u = iterate(x0[None])
    W, WN = _weights()
    return _ref_step(oracle, x[0], u[0], x0, yr, ye, NOMINAL, np.zeros(ND), 1, W, WN, u_min, u_max)


def first_violation(oracle, x0, yr, ye):
    """first stage at which the minimiser of the QP WITHOUT the box leaves [0, 22] (N if it never does)"""
    _, ur, _ = exact_step(oracle, x0, yr, ye, -1e9, 1e9)
    out = ((ur < 0.0) | (ur > 22.0)).any(axis=1)
    return int(np.argmax(out)) if out.any() else N


def touches_box(ur):
    return bool((ur <= 1e-9).any() or (ur >= 22.0 - 1e-9).any())


_cache = {}


def reference(oracle):
    """-> dict(rows = distinct_rows(), X [D][N+1][13], U [D][N][4] (dense exact QP), qp [D], refined {}); computed once"""
    if "ref" not in _cache:
        r = distinct_rows()
        n = r["x0"].shape[0]
        X = np.empty((n, N + 1, 13)); U = np.empty((n, N, 4)); qps = []
        for i in range(n):
            X[i], U[i], qp = exact_step(oracle, r["x0"][i], r["yr"][i], r["ye"][i])
            qps.append(qp)
        _cache["ref"] = dict(rows=r, X=X, U=U, qp=qps, refined={})
    return _cache["ref"]


def refined(oracle, ref, i):
    """the referee's step of distinct row i (extended precision), solved at most once"""
    if i not in ref["refined"]:
        sol = oracle.solve_qp_refined(ref["qp"][i])
        x, u = iterate(ref["rows"]["x0"][i][None])
        ref["refined"][i] = (x[0] + sol["dx"], u[0] + sol["du"])
    return ref["refined"][i]


def errors(oracle, ref, tile, xg, ug, tol=TOL):
    """every row of a fleet against the reference of its distinct row: the dense solution first; a distinct row with any copy
    above tol gets one refined solve and ALL its copies are compared with that instead -> err [B], spread [D] (largest
    difference between two copies of one distinct row, per entry), distinct rows that went to the referee"""
    err = np.maximum(np.abs(xg - ref["X"][tile]).max(axis=(1, 2)), np.abs(ug - ref["U"][tile]).max(axis=(1, 2)))
    sent = sorted(set(tile[err > tol].tolist()))
    for i in sent:
        m = tile == i
        xr, ur = refined(oracle, ref, i)
        err[m] = np.maximum(np.abs(xg[m] - xr).max(axis=(1, 2)), np.abs(ug[m] - ur).max(axis=(1, 2)))
    spread = np.zeros(ref["X"].shape[0])
    for i in np.unique(tile):
        m = tile == i
        spread[i] = max(np.ptp(xg[m], axis=0).max(), np.ptp(ug[m], axis=0).max())
    return err, spread, sent


def tile_map(B, seed, counts):
    """seeded map fleet row -> distinct row.  counts = {kind name: fleet rows of that kind}; what they leave of the B rows are
    copies of the free rows.  Inside a kind every distinct row gets its equal share (the first rows one more); the rows are then
    shuffled over the fleet."""
    kind = kinds()
    rest = B - sum(counts.values())
    assert rest >= 0
    counts = dict(counts)
    if rest:
        counts["free"] = counts.get("free", 0) + rest
    parts = []
    for name, n in counts.items():
        ids = np.flatnonzero(kind == KINDS.index(name))
        parts.append(ids[np.arange(n) % len(ids)])
    t = np.concatenate(parts)
    np.random.default_rng(seed).shuffle(t)
    assert t.shape == (B,)
    return t


def kinds():
    """kind [D] of the distinct rows (index into KINDS), without building them"""
    return np.repeat(np.arange(4), [len(FALLBACK), len(ACTIVE), len(LATE_STEPS), len(FREE)])
