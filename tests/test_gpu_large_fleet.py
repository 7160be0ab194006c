"""GPU suite: the large-fleet plan of the constrained-QP phase against the exact QP on EVERY row.

From 16 S instances on (S = the device's SIMD count, 1024 on an MI355X: 16 384 instances) resolve_plan (csrc/cfnmpc_plan.hpp)
runs code no small fleet reaches: ipm_listed = 1 -- the fall-back rows compacted into P.ilist2 by k_ipm_list (staged structure;
chunk <= 8 up to 8192 constrained rows, the general loop beyond) or by the atomicAdd of qp_wave<1> (monolithic k_as) --, the
k_ipm_rest* kernels as a grid-stride loop of at most S waves of four listed rows (more than 4 S listed rows: a second trip on
re-used LDS tiles), k_ascommit instead of k_ascommit1, sparse mode off once the constrained rows exceed S, the fused start
solve's second re-linearisation (k_linearise_clist, which = 1) and the late rows of a split forward sweep.  The full-size tests
compare properties, samples and routes with each other and never had more than a few hundred fall-back rows.

Here B = 20 483 (the last wave and the last 64-group ragged) and every row is a copy of one of the 64 distinct rows of
tests/large_fleet_data.py, whose exact RTI step is known (dense exact QP, oracle.solve_qp_refined as referee), N = 40, tol 1e-11:
  heavy fleet   HEAVY: 14 000 rows are copies of the 16 fall-back rows, the rest active-set and late rows -- every row constrained
                (> 8192: the long path of k_ipm_list), the fall-back list beyond 4 S rows on every active-set route (5705 - 13 947
                rows: two to four trips of the k_ipm_rest loop);
  light fleet   LIGHT: 784 constrained rows (<= S: sparse mode), 120 of them fall-back and 64 late rows, the others free rows.
Routes (ROUTES): the monolithic kernel, solves + commit, the dense structure with the split sweep and without, the fused start
solve, the interior point alone; and the same QP through the _sbox kernels (per-stage boxes all equal to [0, 22]) and the _w
twins (per-instance weights all equal to the uniform ones).  Per cell, one solve(1) from set_iterate:
  a. every status 0 and every one of the B rows within TOL = 1e-8 of its distinct row's reference (large_fleet_data.errors);
  b. the list counts prove the path (second loop trip, long list path | sparse mode, late rows);
  c. a second solve of the same solver from the same inputs is bitwise the first (iterate and all three statistics);
  d. every row within TOL of the same row in every earlier cell of the fleet.
test_small_fleet_same_rows puts the distinct rows alone into a B = 67 solver: a row that fails there is ill-conditioned, one that
fails only in (a) depends on the fleet's size.

Measured on an MI355X: see test_cell_matches_exact_qp_on_every_row."""
import numpy as np
import pytest

import large_fleet_data as L
from test_gpu_disturbance import QP_TOL

pytestmark = pytest.mark.gpu
B, N, TOL, FLEETS = L.B, L.N, L.TOL, L.FLEETS
# name, options, per-stage boxes, per-instance weights
ROUTES = [("mono", dict(as_passes=-1), False, False),
          ("commit", dict(as_passes=-3, as_dense=-1), False, False),
          ("dense-split", dict(as_passes=-3, as_dense=1), False, False),
          ("dense", dict(as_passes=-3, as_dense=1, forward_split=-1), False, False),
          ("fused", dict(start_solve=2), False, False),
          ("ipm", dict(active_set=0), False, False),
          ("sbox-mono", dict(as_passes=-1), True, False),
          ("sbox-default", dict(), True, False),
          ("w-mono", dict(as_passes=-1), False, True),
          ("w-commit", dict(as_passes=-3), False, True)]
CELLS = [(f, r) for f in FLEETS for r in ROUTES]


@pytest.fixture(scope="module")
def fleets():
    return {}


def _fleet(oracle, fleets, name):
    if name not in fleets:
        counts, seed = FLEETS[name]
        ref = L.reference(oracle)
        tile = L.tile_map(B, seed, counts)
        r = ref["rows"]
        x0 = r["x0"][tile]
        x, u = L.iterate(x0)
        fleets[name] = dict(ref=ref, tile=tile, x0=x0, yr=r["yr"][tile], ye=r["ye"][tile], x=x, u=u, lo=None, hi=None, cells=0)
    return fleets[name]


def _simds():
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


def _solver(n, opts, sbox, wrows):
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    from test_gpu_model_params import _weights
    s = BatchSolver(n, default_opts(N=N, tol=QP_TOL, **opts))
    if sbox:
        s.set_box_stages(np.zeros((n, N, 4)), np.full((n, N, 4), 22.0))
    if wrows:
        W, WN = _weights()
        s.set_weights_batch(np.tile(W, (n, 1)), np.tile(WN, (n, 1)))
    return s


def _step(s, f):
    s.set_x0(f["x0"]); s.set_iterate(f["x"], f["u"])
    s.solve(1)
    return s.get_iterate() + tuple(s.stats())


def _bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


@pytest.mark.parametrize("cell", CELLS, ids=lambda c: f"{c[0]}-{c[1][0]}")
def test_cell_matches_exact_qp_on_every_row(oracle, fleets, cell):
    """Measured on an MI355X (S = 1024), all 20 cells green.  counts = s.list_counts(): constrained rows listed, rows on the
    fall-back list, listed rows with heads > 16 stages, late rows.  worst = largest error of the 20 483 rows against the exact QP,
    spread = largest difference between two copies of one distinct row.

    heavy fleet                                                                    worst     spread    counts
      mono          k_as (atomicAdd list), k_ipm_rest                              2.22e-9   9.33e-10  (20483,  6615, 12355,    0)
      commit        k_as_solves, k_ascommit, k_as_retry, k_ipm_list, k_ipm_rest    2.22e-9   6.87e-11  (20483, 13947, 12355,    0)
      dense-split   k_forward_p1 | k_forward_p2, k_as_solves | k_as_dense, ...     2.22e-9   8.61e-10  (19459, 13689,  9944, 1024)
      dense         k_as_solves | k_as_dense, k_ascommit, ..., k_ipm_rest          2.22e-9   6.87e-11  (20483, 13947, 12355,    0)
      fused         k_linfactor, k_linearise_clist (0, 1), k_as_cst, k_ipm_rest_cst  2.21e-9 9.31e-10  (20483,  6615, 12355,    0)
      ipm           k_ipm                                                          6.62e-9   1.49e-9   (20483,     0, 12355,    0)
      sbox-mono, sbox-default   k_as_sbox, k_ipm_rest_sbox                         2.22e-9   9.34e-10  (20483,  5705, 12355,    0)
      w-mono        k_as_w, k_ipm_rest_w                                           2.22e-9   9.33e-10  (20483,  6615, 12355,    0)
      w-commit      k_as_solves_w, k_ascommit_w, k_as_retry_w, k_ipm_list, k_ipm_rest_w  2.22e-9  6.87e-11  (20483, 13947, 12355, 0)
    light fleet: worst 2.22e-9 (fused 2.21e-9, ipm 6.62e-9), spread 0 -- with one row per wave the copies of a distinct row are
    bitwise equal -- except ipm 1.49e-9; counts (784, 101, 334, 0) mono, fused, w-mono; (784, 139, 334, 0) commit, dense, w-commit;
    (720, 139, 206, 64) dense-split; (784, 93, 334, 0) both sbox cells; (784, 0, 334, 0) ipm.
    Among routes: <= 9.35e-10 between the active-set routes, 6.62e-9 against the interior point alone.  The worst row everywhere
    is a copy of distinct row 41 (an active-set row, 2.22e-9 in the B = 67 solver too: the dense reference's own accuracy); the
    referee was never called.  The second solve was bitwise the first in every cell, the atomicAdd-ordered lists of mono, fused and
    dense-split included: a row's result does not depend on its slot.  The monolithic kernels settle about half of the fall-back
    rows' copies themselves (6615 and 5705 of 14 000 listed), the staged structure lists 13 947.

    That the comparison sees the paths it names was checked once with two deliberately wrong builds, both inside their arrays:
    k_ipm_list's general loop listing the neighbouring slot's row failed heavy-commit and heavy-w-commit alone (worst 89 kRPM,
    every status still 0; heavy-mono, the light fleet and the small fleet green), and a k_ipm_rest loop whose later trips repeat
    the first failed every heavy active-set cell the same way (res > 0 on 4096 = 4 S rows)."""
    fleet, (route, opts, sbox, wrows) = cell
    f = _fleet(oracle, fleets, fleet)
    S = _simds()
    assert B >= 16 * S, (B, S)                                       # the plan under test: ipm_listed = 1
    s = _solver(B, opts, sbox, wrows)
    s.set_yref(f["yr"], f["ye"])
    xg, ug, st, it, res = _step(s, f)
    counts = s.list_counts()
    again = _step(s, f)
    counts2 = s.list_counts()
    s.close()
    # a. every row against its reference
    err, spread, sent = L.errors(oracle, f["ref"], f["tile"], xg, ug)
    # d. among the routes of this fleet: |new - any earlier cell| <= max(|new - lo|, |new - hi|), lo / hi the element-wise
    #    extremes of the earlier cells, with equality at one of them
    among = 0.0
    if f["lo"] is not None:
        among = max(max(np.abs(v - lo).max(), np.abs(v - hi).max()) for v, lo, hi in zip((xg, ug), f["lo"], f["hi"]))
    same = [np.array_equal(_bits(a), _bits(b)) for a, b in zip((xg, ug, st, it, res), again)]
    n_fb = int(((it > 0) & (res > 0.0)).sum())
    print(f"{fleet}-{route}: worst {err.max():.2e} (row {int(err.argmax())}, distinct {int(f['tile'][err.argmax()])}), "
          f"spread {spread.max():.2e} (distinct {int(spread.argmax())}), among routes {among:.2e}, counts {counts}, "
          f"constrained {int((it > 0).sum())}, res > 0 on {n_fb}, referee for {sent}, status {np.bincount(st).tolist()}, "
          f"second solve bitwise (x, u, status, it, res) {same}")
    assert (st == 0).all(), np.flatnonzero(st != 0)[:8]
    assert err.max() <= TOL, (int(err.argmax()), err.max())
    # b. the path ran
    active_set = opts.get("active_set", 1) == 1
    if fleet == "heavy":
        assert counts[0] > 8192, counts                               # the general loop of k_ipm_list; sparse mode off
        if active_set:
            assert counts[1] > 4 * S, counts                          # a second trip of the k_ipm_rest loop
    else:
        assert 0 < counts[0] <= S, counts                             # sparse mode
        if active_set:
            assert counts[1] > 0, counts
        if route == "dense-split":
            assert counts[3] > 0, counts                              # late rows of the split sweep
    # c. determinism
    assert counts2 == counts, (counts, counts2)
    assert all(same), same
    # d.
    assert among <= TOL, among
    if f["lo"] is None:
        f["lo"], f["hi"] = (xg.copy(), ug.copy()), (xg.copy(), ug.copy())
    else:
        for v, lo, hi in zip((xg, ug), f["lo"], f["hi"]):
            np.minimum(lo, v, out=lo); np.maximum(hi, v, out=hi)


def test_small_fleet_same_rows(oracle):
    """The 64 distinct rows alone (and rows 0 - 2 once more: B = 67), default route: the same TOL.  Measured: worst 2.22e-9 (distinct row 41),
    56 rows constrained, res > 0 on the 16 fall-back rows and one active-set row, no referee."""
    n = 67
    ref = L.reference(oracle)
    tile = np.arange(n) % L.D
    r = ref["rows"]
    f = dict(x0=r["x0"][tile], yr=r["yr"][tile], ye=r["ye"][tile])
    f["x"], f["u"] = L.iterate(f["x0"])
    s = _solver(n, {}, False, False)
    s.set_yref(f["yr"], f["ye"])
    xg, ug, st, it, res = _step(s, f)
    s.close()
    err, spread, sent = L.errors(oracle, ref, tile, xg, ug)
    kinds = [int(((it[:L.D] > 0) & (res[:L.D] > 0) & (r["kind"] == k)).sum()) for k in range(4)]
    print(f"small fleet: worst {err.max():.2e} (distinct {int(err.argmax()) % L.D}), constrained {int((it[:L.D] > 0).sum())}, "
          f"res > 0 per kind {kinds}, referee for {sent}")
    assert (st == 0).all(), st
    assert err.max() <= TOL, (int(err.argmax()), err.max())
    assert ((it[:L.D] > 0) == (r["kind"] != L.KINDS.index("free"))).all()
