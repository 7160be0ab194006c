"""GPU tests of the batched extended Kalman filter (include/cfnmpc.h: cfnmpc_ekf_step) against the numpy
twin of tests/test_ekf_cpu.py (ekf_ref, checked there): the prediction has the bits of cfnmpc_sim / cfnmpc_sim_params /
cfnmpc_sim_dist, covariance, update, gate, quaternion sign and normalisation follow the twin to 1e-9 -- the bound
tests/test_gpu_uncertainty.py holds the sibling covariance sweep to -- with the twin's counts exactly, the call works in place and
on host and device arrays with the same bits, a NaN stays in its own row, a 200-step filter run with dropouts and outliers ends
with a covariance cfnmpc_set_uncertainty accepts and the twin's estimate error, and the filter's output feeds the robust-tightening
chain of a solver.

Shapes: B in {1, 5, 67}: one row of a wavefront; a second wavefront with one row; past a 64-lane boundary (17 wavefronts, the last
with three rows).  Error measure: per vehicle and array, max |a - ref| / max(max |ref|, 1e-12)."""
import functools

import numpy as np
import pytest

import test_ekf_cpu as ec
from test_ekf_cpu import GATE, GATE_CASES, T, case, case_args, ekf_ref, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-9
SHAPES = [1, 5, 67]
ROWS = ec.ROWS


def _dev(a):
    import torch
    return None if a is None else torch.as_tensor(np.array(a), device="cuda")      # (a copy: the cases are read-only)


def _host(t):
    return tuple(a.cpu().numpy() for a in t)


def _step(c, on_device=False, normalize=True, out=None, **over):
    """crazyflie_nmpc_amd.ekf_step on a case -> numpy (x, P, nis, counts)"""
    from crazyflie_nmpc_amd import ekf_step
    a = dict(case_args(c), **over)
    kw = dict(T=a["T"], steps=a["steps"], gate=a["gate"], normalize=normalize)
    if on_device:
        return _host(ekf_step(_dev(c["x"]), _dev(c["P"]), _dev(c["u"]), z=_dev(a["z"]), r=_dev(a["r"]), Q=_dev(a["Q"]),
                              params=_dev(a["p"]), dist=_dev(a["d"]), out=out, **kw))
    return ekf_step(c["x"], c["P"], c["u"], z=a["z"], r=a["r"], Q=a["Q"], params=a["p"], dist=a["d"], out=out, **kw)


@functools.lru_cache(maxsize=None)
def _twin(seed, B, steps, rows, kind, gate=0.0, normalize=True, predict_only=False):
    """the twin's result of a case, computed once"""
    c = case(seed, B, steps, rows, kind, gate)
    a = case_args(c)
    if predict_only:
        a["z"] = a["r"] = None
    return ekf_ref(c["x"], c["P"], c["u"], normalize=normalize, **a)


def _errs(got, ref):
    return max(float(rel_err(got[0], ref[0]).max()), float(rel_err(got[1], ref[1]).max()), float(rel_err(got[2][:, None], ref[2][:, None]).max()))


def _same(a, b):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("B", SHAPES)
def test_predict_only_has_the_plant_steps_bits(B, steps, rows):
    from crazyflie_nmpc_amd import sim
    c = case(60 + B, B, steps, rows, "ten")
    a = case_args(c)
    x, P, nis, counts = _step(c, z=None, r=None)
    assert np.array_equal(x, sim(c["x"], c["u"], T=T, steps=steps, params=a["p"], dist=a["d"]))
    ref = _twin(60 + B, B, steps, rows, "ten", predict_only=True)
    e = float(rel_err(P, ref[1]).max())
    print(f"B {B}, steps {steps}, rows {rows}: P^- against the twin {e:.2e}, x^- {float(rel_err(x, ref[0]).max()):.2e}")
    assert e <= TOL
    assert not nis.any() and not counts.any() and counts.dtype == np.int32


@pytest.mark.parametrize("kind", ["ten", "pos", "all", "mixed", "flip"])
@pytest.mark.parametrize("B,steps,rows", [(1, 1, "none"), (5, 3, "p"), (5, 1, "d"), (67, 3, "pd"), (67, 1, "none")])
def test_full_step_against_the_twin(B, steps, rows, kind):
    c = case(70 + B, B, steps, rows, kind)
    worst = 0.0
    for normalize in (True, False):
        got = _step(c, normalize=normalize)
        ref = _twin(70 + B, B, steps, rows, kind, normalize=normalize)
        assert np.array_equal(got[3], ref[3])
        worst = max(worst, _errs(got, ref))
        if normalize:
            assert (np.abs(np.linalg.norm(got[0][:, 3:7], axis=1) - 1) <= 1e-15).all()
    print(f"B {B}, steps {steps}, rows {rows}, {kind}: worst error against the twin {worst:.2e}")
    assert worst <= TOL


@pytest.mark.parametrize("seed,B,steps,rows", GATE_CASES)
def test_gate_cases_against_the_twin(seed, B, steps, rows):
    c = case(seed, B, steps, rows, "mixed", GATE)
    got = _step(c)
    ref = _twin(seed, B, steps, rows, "mixed", GATE)
    assert np.array_equal(got[3], ref[3]) and ref[3][:, 1].sum() > 0
    e = _errs(got, ref)
    print(f"B {B}: gate cases, worst error against the twin {e:.2e}")
    assert e <= TOL


def test_in_place_host_device_and_repeated_calls_give_the_same_bits():
    import torch
    from crazyflie_nmpc_amd import ekf_step
    c = case(21, 67, 3, "pd", "mixed", GATE)
    a = case_args(c)
    base = _step(c)
    assert _same(base, _step(c))
    assert _same(base, _step(c, on_device=True))
    xh, Ph = np.array(c["x"]), np.array(c["P"])
    r = ekf_step(xh, Ph, c["u"], z=a["z"], r=a["r"], Q=a["Q"], params=a["p"], dist=a["d"], T=T, steps=3, gate=GATE, out=(xh, Ph))
    assert r[0] is xh and r[1] is Ph and _same(base, r)
    xd, Pd = _dev(c["x"]), _dev(c["P"])
    r = ekf_step(xd, Pd, _dev(c["u"]), z=_dev(a["z"]), r=_dev(a["r"]), Q=_dev(a["Q"]), params=_dev(a["p"]), dist=_dev(a["d"]), T=T,
                 steps=3, gate=GATE, out=(xd, Pd))
    torch.cuda.synchronize()
    assert r[0] is xd and _same(base, _host(r))


def test_a_nan_row_stays_alone():
    c = case(81, 5, 1, "pd", "all")
    base = _step(c, on_device=True)
    keep = [0, 1, 3, 4]
    for name in ("x", "z", "P"):
        bad = np.array(c[name])
        bad[(2, 4) if bad.ndim == 2 else (2, 4, 4)] = np.nan
        got = _step(dict(c, **{name: bad}), on_device=True)
        assert all(np.array_equal(g[keep], b[keep]) for g, b in zip(got, base)), name
        assert np.isnan(got[0][2]).any() and np.isnan(got[2][2]), name
        assert name == "z" or np.isnan(got[1][2]).any()      # (a NaN measurement meets the state and the NIS, not the covariance)


# ---- a filter run ------------------------------------------------------------------------------------------------------------
RUN_B, RUN_STEPS, RUN_GATE = 5, 200, 5.0
RUN_R = np.repeat([1e-3, 5e-3, -1.0, 2e-2], [3, 4, 3, 3]) ** 2 * np.repeat([1.0, 1.0, -1.0, 1.0], [3, 4, 3, 3])   # (v_b: not measured)
RUN_QSD = np.repeat([1e-4, 1e-4, 2e-2, 5e-2], [3, 4, 3, 3])


@functools.lru_cache(maxsize=None)
def _run_data():
    """the truth, the inputs and the measurements of the run: the RK4 plant with process noise from a perturbed hover, a mocap
    dropout (r[:7] < 0) every 11th step, a 0.5 m position outlier every 37th step"""
    rng = np.random.default_rng(90)
    B, n = RUN_B, RUN_STEPS
    c = ec.sv.draw(90, B, 1)
    p, d = c["p"], c["d"]
    k = ec.sv.derive(p.T); dd = d.T
    x = np.array(c["x0"]); x[:, 7:13] *= 0.2
    us = ec.sv.hover(p)[None, :, None] + rng.uniform(-0.3, 0.3, (n, B, 4))
    xs, zs, rs = [x], [], []
    for t in range(n):
        x = ec.sv.rk4_step(x.T, us[t].T, k, dd, T).T + RUN_QSD * rng.standard_normal((B, 13))
        z = x + np.sqrt(np.abs(RUN_R)) * rng.standard_normal((B, 13))
        r = np.tile(RUN_R, (B, 1))
        if t % 11 == 10:
            r[:, :7] = -1.0
        if t % 37 == 36:
            z[np.arange(B), rng.integers(0, 3, B)] += 0.5 * rng.choice([-1.0, 1.0], B)
        xs.append(x); zs.append(z); rs.append(r)
    x0 = xs[0] + ec.SIG0 * 0.5 * rng.standard_normal((B, 13))
    P0 = np.tile(np.diag(ec.SIG0 ** 2), (B, 1, 1))
    Q = np.tile(np.diag(RUN_QSD ** 2), (B, 1, 1))
    return dict(p=p, d=d, us=us, xs=np.array(xs), zs=np.array(zs), rs=np.array(rs), x0=x0, P0=P0, Q=Q)


def _run(step):
    """the filter over the run with step(x, P, u, z, r) -> (x, P, nis, counts) -> (final P, counts per step, v_b RMS error)"""
    D = _run_data()
    x, P = D["x0"], D["P0"]
    counts, err = [], []
    for t in range(RUN_STEPS):
        x, P, _nis, cn = step(x, P, D["us"][t], D["zs"][t], D["rs"][t])
        counts.append(np.array(cn))
        err.append(np.array(x)[:, 7:10] - D["xs"][t + 1][:, 7:10])
    return np.array(P), np.array(counts), float(np.sqrt(np.mean(np.square(err[20:]))))


def test_filter_run_with_dropouts_and_outliers():
    from crazyflie_nmpc_amd import BatchSolver, default_opts, ekf_step
    D = _run_data()
    ratios = []
    Pt, ct, et = _run(lambda x, P, u, z, r: ekf_ref(x, P, u, p=D["p"], d=D["d"], T=T, steps=1, Q=D["Q"], z=z, r=r, gate=RUN_GATE,
                                                     normalize=True, ratios=ratios))
    rt = np.array([v for _i, _j, v in ratios])
    assert not ((rt >= 0.9) & (rt <= 1.1)).any()          # (the twin's decisions are not at their threshold: the run is a fair referee)
    Pg, cg, eg = _run(lambda x, P, u, z, r: ekf_step(x, P, u, z=z, r=r, Q=D["Q"], T=T, steps=1, gate=RUN_GATE, normalize=True,
                                                      params=D["p"], dist=D["d"]))
    print(f"200 steps: v_b RMS error GPU {eg:.5f} m/s, twin {et:.5f} m/s; rejected {int(cg[:, :, 1].sum())}, "
          f"asymmetry of the final P {float(rel_err(Pg, np.swapaxes(Pg, 1, 2)).max()):.2e}")
    # every outlier (one position component of every vehicle every 37th step) was rejected, and nothing else: the twin's counts
    assert np.array_equal(cg, ct)
    out_steps = [t for t in range(RUN_STEPS) if t % 37 == 36]
    assert len(out_steps) == 5 and not any(t % 11 == 10 for t in out_steps)
    assert all((cg[t, :, 1] >= 1).all() for t in out_steps)
    # the final covariance, as returned, passes cfnmpc_set_uncertainty's host validation and has a positive diagonal
    assert (np.einsum("bii->bi", Pg) > 0).all()
    assert (np.abs(Pg - np.swapaxes(Pg, 1, 2)).reshape(RUN_B, -1).max(axis=1) <= 1e-12 * np.abs(Pg).reshape(RUN_B, -1).max(axis=1)).all()
    s = BatchSolver(RUN_B, default_opts(N=8))
    s.set_uncertainty(Pg, D["Q"])
    assert abs(eg - et) <= 0.01 * et


def test_the_filter_feeds_the_tightening_chain(oracle):
    """ekf_step -> set_x0 -> solve -> set_uncertainty(P_new, Q) -> eval_uncertainty -> backoff, on device tensors"""
    import torch
    from crazyflie_nmpc_amd import BatchSolver, default_opts, ekf_step
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B, N = 5, 8
    rng = np.random.default_rng(7)
    x = oracle.sample_hover_x0(rng, B, scale=0.5)
    yr, ye = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    P = ec.random_cov(rng, B, ec.SIG0)
    Q = ec.random_cov(rng, B, 0.02 * ec.SIG0)
    r = np.tile(np.where(RUN_R < 0, -1.0, RUN_R), (B, 1))
    z = x + np.sqrt(np.abs(r)) * rng.standard_normal((B, 13))
    u = np.full((B, 4), float(ec.sv.hover(ec.NOMINAL)))
    s = BatchSolver(B, default_opts(N=N))
    s.set_yref(np.repeat(yr[None], B, 0).copy(), np.repeat(ye[None], B, 0).copy())
    xn, Pn, _nis, counts = ekf_step(_dev(x), _dev(P), _dev(u), z=_dev(z), r=_dev(r), Q=_dev(Q), T=T, steps=1, gate=5.0)
    s.set_x0(xn)
    s.init_iterate(INIT_HOVER)
    s.solve(1)
    s.set_uncertainty(Pn, _dev(Q))
    s.eval_uncertainty()
    beta = s.backoff()
    torch.cuda.synchronize()
    assert (counts.cpu().numpy()[:, 0] == 10).all()
    assert beta.shape == (B, N, 4) and np.isfinite(beta).all() and (beta >= 0).all() and (beta > 0).any()
