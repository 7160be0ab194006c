"""CPU suite: the 64 distinct rows of tests/large_fleet_data.py are what its table says, by the oracle and the C restatement alone.

The GPU test built on them (tests/test_gpu_large_fleet.py) holds every one of 20 483 fleet rows to 1e-8 of its distinct row's exact
step; that bound is fair only if each distinct row's QP is conditioned well enough for two FP64 solvers to meet well inside it, and the
test's paths run only if the rows are of the kinds the fleets are mixed from.  Both are properties of the data, checked here without
a GPU."""
import numpy as np
import pytest

import large_fleet_data as L
from test_gpu_model_params import _agree


@pytest.fixture(scope="module")
def table(oracle, cref):
    ref = L.reference(oracle)
    r = ref["rows"]
    xc, uc, st, it, res = L.restatement(cref, r["x0"], r["yr"], r["ye"])
    x, u = L.iterate(r["x0"])
    err = np.array([_agree(oracle, xc[i], uc[i], ref["X"][i], ref["U"][i], ref["qp"][i], x[i], u[i], L.KEEP) for i in range(L.D)])
    return dict(ref=ref, rows=r, st=st, it=it, res=res, err=err)


def test_kinds_and_counts(table):
    r, st, it, res = table["rows"], table["st"], table["it"], table["res"]
    assert r["x0"].shape == (L.D, 13) and r["yr"].shape == (L.D, L.N, 17)
    assert np.array_equal(r["kind"], L.kinds())
    assert [int((r["kind"] == k).sum()) for k in range(4)] == [L.COUNT[n] for n in L.KINDS] == [16, 32, 8, 8]
    assert (st == 0).all(), st
    k = {n: r["kind"] == i for i, n in enumerate(L.KINDS)}
    assert ((it > 0) & (res > 0.0))[k["fallback"]].all()              # the restatement ends in the interior point
    assert ((it > 0) & (res == 0.0))[k["active"]].all()               # settled active-set solves
    assert ((it > 0) & (res == 0.0))[k["late"]].all()
    assert (it == 0)[k["free"]].all()
    # distinct: no two rows share their data (copies are the tile map's business)
    flat = np.concatenate([r["x0"], r["yr"].reshape(L.D, -1)], axis=1)
    assert len(np.unique(flat, axis=0)) == L.D


def test_restatement_meets_the_exact_step(table):
    """TOL / 5 = 2e-9 on all 64 rows, dense exact QP first, the referee where that disagrees"""
    err = table["err"]
    print("restatement against the exact step, worst per kind: " +
          ", ".join(f"{n} {err[table['rows']['kind'] == i].max():.2e}" for i, n in enumerate(L.KINDS)))
    assert (err <= L.KEEP).all(), (np.flatnonzero(err > L.KEEP), err.max())


def test_late_rows_leave_the_box_behind_the_split(oracle, table):
    r = table["rows"]
    late = np.flatnonzero(r["kind"] == L.KINDS.index("late"))
    first = [L.first_violation(oracle, r["x0"][i], r["yr"][i], r["ye"][i]) for i in late]
    print("late rows: first violation of the unbounded minimiser at stages", first)
    assert all(L.SPLIT <= k < L.N for k in first), first
    for i, dz in zip(late, L.LATE_STEPS):          # at rest at the reference, which steps down at LATE_STAGE
        assert np.array_equal(r["x0"][i], r["yr"][i, 0, :13]) and (r["x0"][i, 7:] == 0.0).all()
        assert (r["yr"][i, :L.LATE_STAGE, 2] == r["x0"][i, 2]).all()
        assert (r["yr"][i, L.LATE_STAGE:, 2] == r["x0"][i, 2] - dz).all() and r["ye"][i, 2] == r["x0"][i, 2] - dz


def test_share_at_the_box_and_free_rows(table):
    ref, r = table["ref"], table["rows"]
    touch = np.array([L.touches_box(ref["U"][i]) for i in range(L.D)])
    free = r["kind"] == L.KINDS.index("free")
    assert touch.sum() >= 0.2 * L.D, touch.sum()
    assert np.array_equal(touch, ~free)                               # every constrained row's exact solution is at a bound
    # free rows stay clear of the box: no rounding of the unconstrained minimiser makes them constrained
    assert ref["U"][free].min() >= 1.0 and ref["U"][free].max() <= 21.0, (ref["U"][free].min(), ref["U"][free].max())


def test_fleet_maps():
    kind = L.kinds()
    for name, (counts, seed) in L.FLEETS.items():
        t = L.tile_map(L.B, seed, counts)
        assert t.shape == (L.B,) and np.array_equal(t, L.tile_map(L.B, seed, counts))      # seeded
        n = {k: int((kind[t] == i).sum()) for i, k in enumerate(L.KINDS)}
        assert len(np.unique(t)) == (L.D if n["free"] else L.D - 8)                         # every distinct row of the kinds used
        assert all(n[k] == v for k, v in counts.items()), (n, counts)
        con = L.B - n["free"]
        if name == "heavy":
            assert n["free"] == 0 and n["fallback"] > 8192 and n["fallback"] >= 0.4 * L.B
        else:
            assert con <= 900 and n["fallback"] <= 150 and n["late"] >= 32 and n["free"] == L.B - con
        # copies of one distinct row are spread over the fleet, not one run of neighbours
        assert np.abs(np.diff(np.flatnonzero(t == t[0]))).max() > 4
