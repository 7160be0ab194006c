"""CPU checks of the setter walks (tests/setter_walk.py, run on the device by tests/test_gpu_setter_walk.py): the model InForce on
hand-written sequences for every special case of include/cfnmpc.h, with the expected values stated literally; the shape of the
walks; the coverage of the walk set (every op kind, every feature on and off in the final states, every ordered transition with a
solve on both sides), so that the GPU test cannot pass by not looking; and the referee conditions of the twelve checked rows of
every final state, on the oracle alone.  No GPU needed."""
from collections import Counter

import numpy as np
import pytest

import setter_walk as sw
from test_model_params_cpu import NOMINAL

B, N = 3, 2       # the model checks: three instances, two stages


def _model():
    return sw.InForce(B, N, W=np.arange(1.0, 18.0), WN=np.arange(101.0, 114.0))


def _rows(v, n):
    return np.tile(np.asarray(v, dtype=np.float64), (n, 1))


# ---- 1. the model on hand-written sequences ----------------------------------------------------------------------------------------
def test_model_weights_special_cases():
    W0, WN0 = np.arange(1.0, 18.0), np.arange(101.0, 114.0)
    Wr, WNr = 2.0 + np.arange(B * 17.0).reshape(B, 17), 3.0 + np.arange(B * 13.0).reshape(B, 13)
    m = _model()
    W, WN = m.weights_batch()                                           # no rows: the uniform weights everywhere
    assert np.array_equal(W, _rows(W0, B)) and np.array_equal(WN, _rows(WN0, B))
    m.set_weights_batch(None, WNr)                                      # (None, WN) without rows: W rows are the uniform W
    W, WN = m.weights_batch()
    assert np.array_equal(W, _rows(W0, B)) and np.array_equal(WN, WNr) and m.features()["weight rows"]
    m.set_weights_batch(Wr, None)                                       # (W, None) with rows: the WN rows stay
    W, WN = m.weights_batch()
    assert np.array_equal(W, Wr) and np.array_equal(WN, WNr)
    m.set_weights(W=10.0 * W0)                                          # set_weights with rows in force: that part in every row
    W, WN = m.weights_batch()
    assert np.array_equal(W, _rows(10.0 * W0, B)) and np.array_equal(WN, WNr)
    m.set_cost_scaling(2.0, 0.5)                                        # the rows stay unscaled; the scaling is a pair of its own
    assert np.array_equal(m.weights_batch()[0], _rows(10.0 * W0, B)) and m.scaling == (2.0, 0.5)
    assert np.array_equal(sw.row_data(m, 1)["Qd"], 20.0 * W0[:13]) and np.array_equal(sw.row_data(m, 1)["QNd"], 0.5 * WNr[1])
    m.set_weights_batch(None, None)                                     # back to uniform: the LAST set_weights, not the opts
    W, WN = m.weights_batch()
    assert np.array_equal(W, _rows(10.0 * W0, B)) and np.array_equal(WN, _rows(WN0, B)) and not m.features()["weight rows"]
    m.set_weights_batch(None, 7.0 * WNr)                                # no old rows come back: W rows are the uniform W again
    W, WN = m.weights_batch()
    assert np.array_equal(W, _rows(10.0 * W0, B)) and np.array_equal(WN, 7.0 * WNr)
    m.set_weights(WN=WN0)                                               # the other part alone
    W, WN = m.weights_batch()
    assert np.array_equal(W, _rows(10.0 * W0, B)) and np.array_equal(WN, _rows(WN0, B))


def test_model_params_and_disturbance_special_cases():
    p = NOMINAL * np.array([[1.1], [1.2], [1.3]])
    d = np.arange(B * 6.0).reshape(B, 6) - 4.0
    m = _model()
    assert np.array_equal(m.model_params(), _rows(NOMINAL, B)) and np.array_equal(m.disturbance(), np.zeros((B, 6)))
    m.set_model_params(p); m.set_disturbance(d); m.set_model_params(None)      # params > dist > params(None): nominal rows, dist stays
    assert np.array_equal(m.model_params(), _rows(NOMINAL, B)) and np.array_equal(m.disturbance(), d)
    assert not m.features()["parameter rows"] and m.features()["disturbance rows"]
    assert np.array_equal(sw.row_data(m, 2)["p"], NOMINAL) and np.array_equal(sw.row_data(m, 2)["d"], d[2])
    m.set_disturbance(None)                                                    # > dist(None): nothing left
    assert np.array_equal(m.disturbance(), np.zeros((B, 6))) and not any(m.features().values())
    m.set_model_params(p); m.set_model_params(None); m.set_disturbance(2.0 * d)  # params > params(None) > dist: nominal under the rows
    assert np.array_equal(m.model_params(), _rows(NOMINAL, B)) and np.array_equal(m.disturbance(), 2.0 * d)
    m.set_model_params(p); m.set_disturbance(None)                             # dist > params > dist(None): the parameter rows stay
    assert np.array_equal(m.model_params(), p) and np.array_equal(m.disturbance(), np.zeros((B, 6)))
    m.set_erk_steps(2); m.set_erk_steps(1)
    assert m.erk == 1 and not m.features()["erk steps"]
    m.set_erk_steps(3)
    assert sw.row_data(m, 0)["M"] == 3


def test_model_box_special_cases():
    lb, ub = np.full((B, N, 4), 1.5), np.full((B, N, 4), 20.5)
    m = _model()
    assert [a.tolist() for a in m.bounds()] == [np.full((B, N, 4), 0.0).tolist(), np.full((B, N, 4), 22.0).tolist()]
    m.set_box_stages(lb, ub); m.set_box(1.0, 21.0)                             # stages > set_box: the stage boxes stay in force
    assert np.array_equal(m.bounds()[0], lb) and np.array_equal(m.bounds()[1], ub) and m.box == (1.0, 21.0)
    m.set_box_stages(lb + 1.0, ub - 1.0)                                       # > stages again: the new arrays
    assert (m.bounds()[0] == 2.5).all() and (m.bounds()[1] == 19.5).all()
    m.set_box_stages(None, None)                                               # > (None, None): the scalar box set meanwhile
    assert (m.bounds()[0] == 1.0).all() and (m.bounds()[1] == 21.0).all() and not m.features()["stage boxes"]
    for back, want in ((lambda: m.set_box(2.0, 20.0), (2.0, 20.0)), (lambda: m.set_box_stages(None, None), (2.0, 20.0)),
                       (lambda: m.set_box_stages(lb, ub), (1.5, 20.5))):       # a tightened box and its three ways back
        m.tighten_box(3.0)
        assert m.tight
        back()
        assert not m.tight and (m.bounds()[0] == want[0]).all() and (m.bounds()[1] == want[1]).all()
    m.tighten_box(3.0); m.set_box(0.5, 21.5)                                   # nominal stage boxes: set_box puts THEM back
    assert not m.tight and (m.bounds()[0] == 1.5).all() and m.box == (0.5, 21.5)
    m.tighten_box(3.0); m.tighten_box(0.0)
    assert not m.tight


def test_model_reference_writers():
    y = np.arange(B * N * 17.0).reshape(B, N, 17)
    ye = -np.arange(B * 13.0).reshape(B, 13)
    yu = np.repeat(y[:, :1], N, 1)
    m = _model()
    m.set_yref(yu, ye)
    assert m.writer() == "uniform" and np.array_equal(m.yref()[0], yu) and np.array_equal(m.yref()[1], ye) and m.yref()[2].all()
    m.set_yref(y, ye)
    assert m.writer() == "varying" and np.array_equal(m.yref()[0], y)
    traj = np.arange(6 * 17.0).reshape(6, 17)
    m.set_yref_windows(traj, np.array([1, 0, 1]), np.array([0, 2, 3]), np.array([[1.0, 2.0, 3.0]] * 3), 15.5)
    yw, ywe, exact = m.yref()
    assert m.writer() == "windows" and exact.all()
    assert np.array_equal(yw[0], traj[0:2]) and np.array_equal(ywe[0], traj[2, :13])           # tracking: rows it .. it + N
    assert np.array_equal(yw[2], traj[3:5]) and np.array_equal(ywe[2], traj[5, :13])
    reg = [1.0, 2.0, 3.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 15.5, 15.5, 15.5, 15.5]
    assert yw[1].tolist() == [reg, reg] and ywe[1].tolist() == reg[:13]                        # regulation around des
    # polynomial rows: vehicles without a trajectory keep their rows bit for bit, the others follow the host twin
    tab = sw.poly_tables()
    place = np.tile([0.0, 1.0, 0.0, 0.0, 0.0, 0.0], (B, 1))
    m.set_model_params(NOMINAL * np.ones((B, 1)))
    m.set_yref_poly(np.array([0, -1, 2], dtype=np.int32), place, 1.0, 0)
    yp, ype, exact = m.yref()
    assert m.writer() == "poly" and exact.tolist() == [False, True, False] and m.poly_follows_params()
    assert np.array_equal(yp[1], yw[1]) and np.array_equal(ype[1], ywe[1])
    from crazyflie_nmpc_amd import trajectories as tj
    rows = tj.poly_rows(tab, [0, -1, 2], place, 1.0, N + 1, sw.DT, 0, None)[1]
    assert np.array_equal(yp[0], rows[0, :N]) and np.array_equal(ype[2], rows[2, N, :13]) and not np.array_equal(yp[0], yw[0])
    m.set_model_params(None)                  # the rows in force were written under other parameter rows: apply() could not
    assert not m.poly_follows_params()
    m.set_yref(y, ye)                         # every other writer replaces all of it
    assert m.writer() == "varying" and m.poly_follows_params() and np.array_equal(m.yref()[0], y)


class _Recorder:
    """stands in for a solver: records the setter calls of apply() into a model"""

    def __init__(self, B, N):
        self.m, self.calls, self.B, self.N = sw.InForce(B, N), [], B, N

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append(name)
            if name in ("set_poly_library", "set_poly_assignment"):
                self.__dict__[name] = (a, kw)
            elif name == "set_yref_poly":
                (traj, place), _ = self.__dict__["set_poly_assignment"]
                self.m.set_yref_poly(traj, place, *a)
            else:
                getattr(self.m, name)(*a, **kw)
        return call


@pytest.mark.parametrize("N_,seed", sw.walk_set())
def test_apply_states_the_whole_final_state(N_, seed, monkeypatch):
    """apply() on a recording stand-in (the windows' arrays stay on the host): a model fed its calls is in the walk's final state
    (every getter), each setter is called at most once, and features that are off get no call"""
    monkeypatch.setattr(sw, "_windows_call", lambda s, a: s.set_yref_windows(a["traj"], a["mode"], a["it"], a["des"], a["uss"]))
    m = sw.replay(sw.walk(seed, N_), sw.B_WALK, N_)
    r = _Recorder(sw.B_WALK, N_)
    sw.apply(r, m)
    for a, b in zip(r.m.weights_batch() + (r.m.model_params(), r.m.disturbance()) + r.m.yref() + r.m.bounds(),
                    m.weights_batch() + (m.model_params(), m.disturbance()) + m.yref() + m.bounds()):
        assert np.array_equal(a, b)
    assert (r.m.erk, r.m.scaling, r.m.box, r.m.writer()) == (m.erk, m.scaling, m.box, m.writer())
    assert max(Counter(r.calls).values()) == 1, r.calls
    off = {"weight rows": "set_weights_batch", "cost scaling": "set_cost_scaling", "erk steps": "set_erk_steps",
           "parameter rows": "set_model_params", "disturbance rows": "set_disturbance", "stage boxes": "set_box_stages"}
    for f, on in m.features().items():
        assert (off[f] in r.calls) == on, (f, r.calls)


# ---- 2. the shape of every walk ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N_,seed", sw.walk_set())
def test_walk_shape(N_, seed):
    ops = sw.walk(seed, N_)
    assert [sw.kind_of(o) for o in ops] == [sw.kind_of(o) for o in sw.walk(seed, N_)]          # (the seed fixes it)
    kinds = [sw.kind_of(o) for o in ops]
    n_set = sum(sw.is_setter(o) for o in ops)
    assert n_set <= sw.MAX_SETTERS, n_set
    assert kinds[0] in sw.WRITERS and kinds[0] != "set_yref_poly"
    solves = [i for i, k in enumerate(kinds) if k == "solve"]
    assert solves[1] == solves[0] + 1 and all(b > a + 1 for a, b in zip(solves[1:-1], solves[2:])), solves   # two, then singly
    assert kinds[-1] in ("solve", "read_only") and kinds.count("read_only") == 1 and kinds.count("solve_sqp") == 1
    assert kinds.count("tighten") <= 1
    for i, k in enumerate(kinds):
        if k in ("tighten", "read_only"):
            assert kinds[i - 1] == "solve", (k, kinds[i - 1])       # on the QP of the step just run, nothing changed since
    m = sw.replay(ops, sw.B_WALK, N_)
    assert not m.tight and m.poly_follows_params()
    if "tighten" in kinds:                                          # a way back follows, with a solve under the tightened box before it
        i = kinds.index("tighten")
        back = next(j for j in range(i + 1, len(ops)) if kinds[j] in ("set_box", "set_box_stages"))
        assert "solve" in kinds[i + 1:back]


# ---- 3. coverage of the walk set ---------------------------------------------------------------------------------------------------
def test_coverage_of_the_walk_set():
    kinds, hits, feats, writers = Counter(), {}, Counter(), Counter()
    print()
    for N_, seed in sw.walk_set():
        ops = sw.walk(seed, N_)
        kinds.update(sw.kind_of(o) for o in ops)
        t = sw.transitions(ops, sw.B_WALK, N_)
        for c in t:
            hits.setdefault(c, []).append((N_, seed))
        m = sw.replay(ops, sw.B_WALK, N_)
        feats.update((f, on) for f, on in m.features().items())
        writers[m.writer()] += 1
        print(f"walk N {N_:2d} seed {seed:3d}: {sum(sw.is_setter(o) for o in ops):2d} setter ops, {len(t)} transitions; final state: "
              f"{m.writer()} references, {', '.join(f for f, on in m.features().items() if on) or 'no rows'}, box {m.box}")
    print("op counts:", dict(sorted(kinds.items())))
    for c in sw.CHAINS:
        print(f"  transition {c}: walks {hits.get(c, [])}")
    print("features on / off in the final states:", {f: (feats[(f, True)], feats[(f, False)]) for f in sw.FEATURES}, dict(writers))
    print("widest walks:", {N_: sw.widest_walks(N_) for N_ in sw.HORIZONS})
    for k in sw.SETTERS + sw.EPISODES:
        assert kinds[k] >= 3, (k, kinds[k])
    for f in sw.FEATURES:
        assert feats[(f, True)] >= 2 and feats[(f, False)] >= 2, (f, feats[(f, True)], feats[(f, False)])
    for c in sw.CHAINS:
        assert hits.get(c), c
    assert len(sw.CHAINS) == 11 + 12 and all(len(sw.SEEDS[N_]) == 6 and len(set(sw.SEEDS[N_])) == 6 for N_ in sw.HORIZONS)


def test_transitions_need_a_solve_on_both_sides():
    """the detector on hand-written walks: the chain counts with a solve before, between and behind, and not without one"""
    P = ("set_model_params", dict(p=np.ones((B, 8))))
    P0, D, S = ("set_model_params", dict(p=None)), ("set_disturbance", dict(d=np.ones((B, 6)))), ("solve", {})
    name = "params > params(None) > dist"
    assert name in sw.transitions([S, P, S, P0, S, D, S], B, N)
    for ops in ([P, S, P0, S, D, S], [S, P, P0, S, D, S], [S, P, S, P0, D, S], [S, P, S, P0, S, D], [S, P, S, D, S, P0, S]):
        assert name not in sw.transitions(ops, B, N), [o[0] for o in ops]
    E = lambda n: ("set_erk_steps", dict(n=n))   # noqa: E731
    assert "erk 1 > 2 > 1" in sw.transitions([S, E(2), S, E(1), S], B, N)          # (a new solver runs one step per interval)
    assert "erk 1 > 2 > 1" not in sw.transitions([S, E(2), E(1), S], B, N)
    W = ("set_weights", dict(W=np.ones(17), WN=None))
    R = ("set_weights_batch", dict(W=np.ones((B, 17)), WN=None))
    CS = ("set_cost_scaling", dict(stage=2.0, terminal=1.0))
    assert "rows > set_weights > set_cost_scaling" in sw.transitions([S, R, S, W, S, CS, S], B, N)
    R0 = ("set_weights_batch", dict(W=None, WN=None))
    assert "rows > set_weights > set_cost_scaling" not in sw.transitions([S, R, S, R0, S, W, S, CS, S], B, N)   # (no rows in force)


# ---- 4. the referee conditions of every final state ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N_,seed", sw.walk_set())
def test_checked_rows_are_a_test(oracle, N_, seed):
    """The twelve checked rows (64 and 66 among them) of the final state, on the oracle alone, at the kick level KICK = 1.0 m/s of
    het_case with every third row calm: oracle.solve_qp_refined reaches KKT <= 1e-12 on every row, at least 20 % of the rows have
    an input on its bound in the reference and at least one has none.  (At N(0, 1.5) m/s, with offsets of 0.02 in the iterate or
    with a cost scaling of (dt, 1), the referee cycled on rows of three final states; with every row at scale 1 no checked row of
    several states stayed off the box.)"""
    m = sw.replay(sw.walk(seed, N_), sw.B_WALK, N_)
    (x0, x, u, _y, _ye), ref = sw.final_reference(oracle, m, seed)
    rows = sw.checked_rows()
    assert len(rows) == 12 and 64 in rows and 66 in rows and list(ref) == rows
    lb, ub = m.bounds()
    assert (u >= lb).all() and (u <= ub).all() and not np.array_equal(x[:, 0], x0)
    kkt = np.array([ref[i][3]["kkt"] for i in rows])
    on = np.array([bool(((ref[i][1] <= lb[i] + 1e-9) | (ref[i][1] >= ub[i] - 1e-9)).any()) for i in rows])
    dense = max(max(np.abs(ref[i][0] - (x[i] + ref[i][3]["dx"])).max(), np.abs(ref[i][1] - (u[i] + ref[i][3]["du"])).max()) for i in rows)
    print(f"\nN {N_} seed {seed} ({m.writer()} references; {', '.join(f for f, v in m.features().items() if v) or 'no rows'}): rows on the box "
          f"{int(on.sum())} of 12, referee KKT {kkt.max():.1e}, solves up to {max(ref[i][3]['solves'] for i in rows)}, "
          f"dense solve vs referee {dense:.1e}")
    assert (kkt <= 1e-12).all(), (np.array(rows)[kkt > 1e-12], kkt.max())
    assert on.sum() >= 0.2 * len(rows) and (~on).sum() >= 1, on
