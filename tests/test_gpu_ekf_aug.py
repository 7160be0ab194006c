"""GPU tests of the disturbance-augmented extended Kalman filter (include/cfnmpc.h: cfnmpc_ekf_aug_step)
against the numpy twin of tests/test_ekf_aug_cpu.py (ekf_aug_ref, checked there): state, disturbance row, augmented covariance,
its state block and the NIS follow the twin to 1e-9 -- the bound of this kernel family (tests/test_gpu_ekf.py,
tests/test_gpu_uncertainty.py) -- with the twin's counts exactly; the prediction has the bits of cfnmpc_sim_dist and leaves d alone;
without slots the call is cfnmpc_ekf_step on the disturbed model; it works in place and on host and device arrays with the same
bits; a NaN stays in its own row; the 300-step run of the CPU test comes out with the twin's decisions and estimates and a covariance
the host validation accepts; and its outputs feed a solver's disturbance row and robust-tightening chain.

Shapes: B in {1, 5, 67}: one row of a wavefront (three rows recompute without storing); a partly filled second block; several blocks
and a ragged tail.  steps in {1, 3}.  Error measure: rel_err of tests/test_ekf_cpu.py."""
import itertools

import numpy as np
import pytest

import test_ekf_aug_cpu as ea
import test_ekf_cpu as ec
from test_ekf_aug_cpu import GATE, GATE_CASES, SELS, T, case, case_args, ekf_aug_ref, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-9
KINDS = ["ten", "pos", "all", "mixed", "flip"]
# every selection with and without p, over the shapes and sub-step counts
COMBOS = [(sel, rows) + shape for (sel, rows), shape in zip(itertools.product(SELS, ["d", "pd"]),
                                                             [(1, 1), (5, 3), (67, 1), (67, 3), (5, 1), (1, 3), (67, 3), (5, 3)])]


def _dev(a):
    import torch
    return None if a is None else torch.as_tensor(np.array(a), device="cuda")      # (a copy: the cases are read-only)


def _host(t):
    return tuple(a.cpu().numpy() for a in t)


def _step(c, on_device=False, normalize=True, **over):
    """crazyflie_nmpc_amd.ekf_aug_step on a case -> numpy (x, d, Pa, nis, counts, Pxx)"""
    from crazyflie_nmpc_amd import ekf_aug_step
    a = dict(case_args(c), **over)
    B = c["x"].shape[0]
    kw = dict(T=a["T"], steps=a["steps"], gate=a["gate"], normalize=normalize)
    if on_device:
        import torch
        Pxx = torch.empty((B, 13, 13), dtype=torch.float64, device="cuda")
        out = ekf_aug_step(_dev(c["x"]), _dev(c["d"]), _dev(c["Pa"]), _dev(c["u"]), c["sel"], z=_dev(a["z"]), r=_dev(a["r"]), Q=_dev(a["Q"]),
                           Qd=_dev(a["Qd"]), params=_dev(a["p"]), Pxx_out=Pxx, **kw)
        return _host(out + (Pxx,))
    Pxx = np.empty((B, 13, 13))
    out = ekf_aug_step(c["x"], c["d"], c["Pa"], c["u"], c["sel"], z=a["z"], r=a["r"], Q=a["Q"], Qd=a["Qd"], params=a["p"], Pxx_out=Pxx, **kw)
    return out + (Pxx,)


def _twin(c, normalize=True, **over):
    a = dict(case_args(c), **over)
    return ekf_aug_ref(c["x"], c["d"], c["Pa"], c["u"], c["sel"], normalize=normalize, **a)


def _errs(got, ref):
    """worst error over x_new, d_new, Pa_new, Pxx_new and nis"""
    return max(float(rel_err(got[0], ref[0]).max()), float(rel_err(got[1], ref[1]).max()), float(rel_err(got[2], ref[2]).max()),
               float(rel_err(got[5], ref[2][:, :13, :13]).max()), float(rel_err(got[3][:, None], ref[3][:, None]).max()))


def _same(a, b):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


@pytest.mark.parametrize("sel,rows,B,steps", COMBOS, ids=str)
def test_full_step_against_the_twin(sel, rows, B, steps):
    worst = 0.0
    for kind in KINDS:
        c = case(70 + B, B, steps, rows, kind, sel)
        variants = [dict(), dict(Q=None, Qd=None)] + ([dict(Qd=None), dict(Q=None)] if kind == "ten" else [])
        for normalize, over in itertools.product((True, False), variants):
            got = _step(c, normalize=normalize, **over)
            ref = _twin(c, normalize=normalize, **over)
            assert np.array_equal(got[4], ref[4]) and got[4].dtype == np.int32
            assert np.array_equal(got[5], got[2][:, :13, :13])
            e = _errs(got, ref)
            worst = max(worst, e)
            assert e <= TOL, (kind, normalize, list(over), e)
            keep = [j for j in range(6) if j not in sel]
            assert np.array_equal(got[1][:, keep], c["d"][:, keep])
            if normalize:
                assert (np.abs(np.linalg.norm(got[0][:, 3:7], axis=1) - 1) <= 1e-15).all()
    print(f"sel {sel}, rows {rows}, B {B}, steps {steps}: worst error against the twin {worst:.2e}")


@pytest.mark.parametrize("seed,B,steps,rows,sel", GATE_CASES, ids=str)
def test_gate_cases_against_the_twin(seed, B, steps, rows, sel):
    """per-vehicle masks with the gate on: four consecutive vehicles of one wavefront differ in mask and rejections"""
    c = case(seed, B, steps, rows, "mixed", sel, GATE)
    got, ref = _step(c), _twin(c)
    assert np.array_equal(got[4], ref[4]) and ref[4][:, 1].sum() > 0
    e = _errs(got, ref)
    print(f"B {B}: gate cases, worst error against the twin {e:.2e}")
    assert e <= TOL


@pytest.mark.parametrize("rows", ["d", "pd"])
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_predict_only_has_the_plant_steps_bits(B, steps, rows):
    from crazyflie_nmpc_amd import sim
    sel = SELS[(B + steps) % len(SELS)]
    c = case(60 + B, B, steps, rows, "ten", sel)
    x, d, Pa, nis, counts, Pxx = _step(c, z=None, r=None)
    assert np.array_equal(x, sim(c["x"], c["u"], T=T, steps=steps, params=c["p"], dist=c["d"]))
    assert np.array_equal(d, c["d"])
    ref = _twin(c, z=None, r=None)
    e = float(rel_err(Pa, ref[2]).max())
    print(f"B {B}, steps {steps}, rows {rows}, sel {sel}: Pa^- against the twin {e:.2e}, x^- {float(rel_err(x, ref[0]).max()):.2e}")
    assert e <= TOL and np.array_equal(Pxx, Pa[:, :13, :13])
    assert not nis.any() and not counts.any() and counts.dtype == np.int32


@pytest.mark.parametrize("B,steps,kind,gate", [(5, 1, "ten", 0.0), (67, 3, "mixed", GATE), (1, 3, "all", 0.0)])
def test_without_slots_it_is_the_sibling_on_the_disturbed_model(B, steps, kind, gate):
    from crazyflie_nmpc_amd import ekf_step
    c = case(45, B, steps, "pd", kind, (-1, -1, -1), gate)
    x, d, Pa, nis, counts, Pxx = _step(c)
    xs, Ps, ns, cs = ekf_step(c["x"], np.ascontiguousarray(c["Pa"][:, :13, :13]), c["u"], z=c["z"], r=c["r"], Q=c["Q"], T=T, steps=steps,
                              gate=gate, params=c["p"], dist=c["d"])
    e = max(float(rel_err(x, xs).max()), float(rel_err(Pxx, Ps).max()), float(rel_err(nis[:, None], ns[:, None]).max()))
    print(f"B {B}, steps {steps}, {kind}: against ekf_step {e:.2e}")
    assert e <= TOL and np.array_equal(counts, cs) and np.array_equal(d, c["d"])
    assert not Pa[:, 13:, :].any() and not Pa[:, :, 13:].any()
    assert gate == 0.0 or cs[:, 1].sum() > 0


def test_in_place_host_device_and_repeated_calls_give_the_same_bits():
    import torch
    from crazyflie_nmpc_amd import ekf_aug_step
    seed, B, steps, rows, sel = GATE_CASES[1]
    c = case(seed, B, steps, rows, "mixed", sel, GATE)
    a = case_args(c)
    base = _step(c)
    assert _same(base, _step(c))
    assert _same(base, _step(c, on_device=True))
    assert np.array_equal(base[5], base[2][:, :13, :13])
    xh, dh, Ph = np.array(c["x"]), np.array(c["d"]), np.array(c["Pa"])
    r = ekf_aug_step(xh, dh, Ph, c["u"], sel, z=a["z"], r=a["r"], Q=a["Q"], Qd=a["Qd"], params=a["p"], T=T, steps=steps, gate=GATE,
                     out=(xh, dh, Ph))
    assert r[0] is xh and r[1] is dh and r[2] is Ph and _same(base[:5], r)
    xd, dd, Pd = _dev(c["x"]), _dev(c["d"]), _dev(c["Pa"])
    r = ekf_aug_step(xd, dd, Pd, _dev(c["u"]), sel, z=_dev(a["z"]), r=_dev(a["r"]), Q=_dev(a["Q"]), Qd=_dev(a["Qd"]), params=_dev(a["p"]),
                     T=T, steps=steps, gate=GATE, out=(xd, dd, Pd))
    torch.cuda.synchronize()
    assert r[0] is xd and r[1] is dd and r[2] is Pd and _same(base[:5], _host(r))


def test_a_nan_row_stays_alone():
    c = case(81, 5, 1, "pd", "all", (2, 3, 4))
    base = _step(c, on_device=True)
    keep = [0, 1, 3, 4]
    for name in ("x", "z", "Pa", "d"):
        bad = np.array(c[name])
        bad[(2, 4) if bad.ndim == 2 else (2, 4, 4)] = np.nan
        got = _step(dict(c, **{name: bad}), on_device=True)
        assert all(np.array_equal(g[keep], b[keep]) for g, b in zip(got, base)), name
        assert np.isnan(got[0][2]).any() and np.isnan(got[3][2]), name
        assert name == "z" or np.isnan(got[2][2]).any()      # (a NaN measurement meets the state and the NIS, not the covariance)


# ---- the 300-step run of tests/test_ekf_aug_cpu.py ----------------------------------------------------------------------------
@pytest.mark.parametrize("sel", ea.RUN_SELS, ids=str)
def test_closed_loop_run_against_the_twin(sel):
    from crazyflie_nmpc_amd import ekf_aug_step
    D = ea.run_data(sel)
    tw, _rt = ea.run_twin(sel)
    g = ea.run_filter(sel, lambda x, d, Pa, u, z, r: ekf_aug_step(x, d, Pa, u, sel, z=z, r=r, Q=D["Q"], Qd=D["Qd"], T=T, steps=1,
                                                                   gate=ea.RUN_GATE, normalize=True, params=D["p"]))
    idx = list(sel)
    ed = float(rel_err(g["d"][:, idx], tw["d"][:, idx]).max())
    print(f"sel {sel}: 300 steps: final d against the twin {ed:.2e}; v_b RMS error GPU {g['ev']:.5f} m/s, twin {tw['ev']:.5f} m/s; "
          f"rejected {int(g['counts'][:, :, 1].sum())}; asymmetry of the final Pa {float(rel_err(g['Pa'], np.swapaxes(g['Pa'], 1, 2)).max()):.2e}")
    assert np.array_equal(g["counts"], tw["counts"])
    assert ed <= 0.01 and abs(g["ev"] - tw["ev"]) <= 0.01 * tw["ev"]
    # the final covariance, as returned, passes the host validation of the next call (CFNMPC_EINVAL would raise)
    ekf_aug_step(g["x"], g["d"], g["Pa"], D["us"][0], sel, Q=D["Q"], Qd=D["Qd"], T=T, params=D["p"])
    assert (np.einsum("bii->bi", g["Pa"]) > 0).all()


def test_the_filter_feeds_the_disturbance_row_and_the_tightening_chain(oracle):
    """ekf_aug_step -> set_x0(x_new), set_disturbance(d_new) -> solve -> set_uncertainty(Pxx_new, Q) -> eval_uncertainty -> backoff, on
    device tensors"""
    import torch
    from crazyflie_nmpc_amd import BatchSolver, default_opts, ekf_aug_cov, ekf_aug_step
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    B, N, sel = 5, 8, (0, 1, 2)
    rng = np.random.default_rng(7)
    x = oracle.sample_hover_x0(rng, B, scale=0.5)
    yr, ye = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    Pa = ekf_aug_cov(ec.random_cov(rng, B, ec.SIG0), [0.5, 0.5, 0.5])
    Q = ec.random_cov(rng, B, 0.02 * ec.SIG0)
    r = np.tile(ea.RUN_R, (B, 1))
    z = x + np.sqrt(np.abs(r)) * rng.standard_normal((B, 13))
    u = np.full((B, 4), float(ec.sv.hover(ec.NOMINAL)))
    d = np.zeros((B, 6)); d[:, 3:] = 0.5
    s = BatchSolver(B, default_opts(N=N))
    s.set_yref(np.repeat(yr[None], B, 0).copy(), np.repeat(ye[None], B, 0).copy())
    Pxx = torch.empty((B, 13, 13), dtype=torch.float64, device="cuda")
    xn, dn, Pan, _nis, counts = ekf_aug_step(_dev(x), _dev(d), _dev(Pa), _dev(u), sel, z=_dev(z), r=_dev(r), Q=_dev(Q), T=T, steps=1,
                                             gate=5.0, Pxx_out=Pxx)
    s.set_x0(xn)
    s.set_disturbance(dn)
    s.init_iterate(INIT_HOVER)
    s.solve(1)
    s.set_uncertainty(Pxx, _dev(Q))
    s.eval_uncertainty()
    beta = s.backoff()
    torch.cuda.synchronize()
    assert (counts.cpu().numpy()[:, 0] == 10).all()
    dh = dn.cpu().numpy()
    assert np.array_equal(dh[:, 3:], d[:, 3:]) and dh[:, :3].any() and np.isfinite(dh).all()
    assert np.array_equal(s.disturbance(), dh)
    assert beta.shape == (B, N, 4) and np.isfinite(beta).all() and (beta >= 0).all() and (beta > 0).any()
