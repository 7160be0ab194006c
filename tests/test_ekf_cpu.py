"""CPU checks of the batched extended Kalman filter (include/cfnmpc.h: cfnmpc_ekf_step): the entry point
is declared, exported and bound, the ABI is unchanged, the new kernels are in the built code within their recorded ceilings while
every earlier kernel keeps its figures, the host validation refuses what the header says it refuses without touching the outputs,
and the numpy twin the GPU tests compare against (ekf_ref: the header's rules step for step, vectorised over the vehicles) is right:

  - its sub-step Jacobians chain to the complex-step Jacobian of the whole numpy rollout of tests/test_sim_vjp_cpu.py (f, derive)
    for the row kinds none / p / d / pd, to the forward sensitivities of tests/test_disturbance_cpu.py (stage Jacobians), and, for
    the nominal row, to oracle.rk4_sens;
  - with the gate off its sequential update is the joint Kalman update K = P H' (H P H' + R)^-1;
  - steps = 3 is three chained predictions of steps = 1;
  - the gate cases the GPU tests use keep every decision away from its threshold.

The stand-alone program tools/ekf_check.cpp runs the host-compiled plain-loop step on cases written here, under the host sanitizers.
Error measure everywhere: per vehicle and array, max |a - ref| / max(max |ref|, 1e-12).  No GPU needed."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import test_disturbance_cpu as dc
import test_sim_vjp_cpu as sv
from test_model_params_cpu import NOMINAL, ROOT, _header, table  # noqa: F401  (table: the fixture)

SIG = ("intcfnmpc_ekf_step(intbatch,constdouble*x,constdouble*P,constdouble*u,constdouble*p,constdouble*d,doubleT,intsteps,"
       "constdouble*Q,constdouble*z,constdouble*r,doublegate,intflags,double*x_new,double*P_new,double*nis,int*counts,"
       "inton_device,void*stream);")
vp, i32, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
ARGTYPES = [i32, vp, vp, vp, vp, vp, dbl, i32, vp, vp, vp, dbl, i32, vp, vp, vp, vp, i32, vp]
KERNELS = ("k_ekf", "k_ekf_par", "k_ekf_dst")
# ceilings of the new kernels, VGPRs + AGPRs of the unified file (512 per lane at one wave per SIMD): the figures of the build
# (394, 430, 474) rounded up to 8; no scratch, no LDS
VGPR_CEIL = {"k_ekf": 400, "k_ekf_par": 432, "k_ekf_dst": 480}
ROWS = sv.ROWS
EINVAL = -1
T = 0.015
# standard deviations of the test covariances and measurements, per state block p | q | v_b | w
SIG0 = np.repeat([0.05, 0.02, 0.2, 0.3], [3, 4, 3, 3])
SIGZ = np.repeat([1e-3, 1e-2, 0.1, 0.03], [3, 4, 3, 3])
MEASURED = {"ten": np.r_[0:7, 10:13], "pos": np.r_[0:3], "all": np.r_[0:13]}   # "ten": what the reference node measures (no v_b)


def rel_err(a, ref):
    """per vehicle: max |a - ref| / max(max |ref|, 1e-12) over the trailing axes -> [B]"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    B = ref.shape[0]
    return np.abs(a - ref).reshape(B, -1).max(axis=1) / np.maximum(np.abs(ref).reshape(B, -1).max(axis=1), 1e-12)


# ---- the numpy twin ------------------------------------------------------------------------------------------------------------
def substep(x, u, k, d, h):
    """one RK4 sub-step of every vehicle and its exact derivative, by complex steps through the sub-step: x [B, 13], u [B, 4],
    k [8, B] derived constants, d [6, B] -> (x+ [B, 13], A [B, 13, 13] = d x+ / d x)"""
    hc = 1e-30
    X = np.repeat(x.T[:, :, None], 13, axis=2).astype(np.complex128)     # [component, vehicle, direction]
    X[np.arange(13), :, np.arange(13)] += 1j * hc
    out = sv.rk4_step(X, u.T[:, :, None], k[:, :, None], d[:, :, None], h)
    return sv.rk4_step(x.T, u.T, k, d, h).T, np.moveaxis(out.imag / hc, 1, 0)


def predict_ref(x, P, u, p, d, T, steps, Q=None):
    """rule 1 -> (x^-, P^-, [A_0, .., A_{steps - 1}])"""
    k = sv.derive(np.moveaxis(p, -1, 0)); dd = np.moveaxis(d, -1, 0)
    x, P, As = np.array(x, dtype=np.float64), np.array(P, dtype=np.float64), []
    for _ in range(steps):
        x, A = substep(x, u, k, dd, T / steps)
        P = A @ P @ np.swapaxes(A, 1, 2)
        As.append(A)
    return x, (P if Q is None else P + Q), As


def update_ref(x, P, z, r, gate, normalize, ratios=None):
    """rules 2 - 4 on (x^-, P^-), vehicle by vehicle -> (x, P, nis, counts); ratios: a list that collects nu^2 / (gate^2 s) of
    every measured component when gate > 0"""
    B = x.shape[0]
    x, P, z = x.copy(), P.copy(), np.array(z, dtype=np.float64)
    nis, counts = np.zeros(B), np.zeros((B, 2), dtype=np.int32)
    for i in range(B):
        dot = 0.0
        for j in range(3, 7):
            if r[i, j] >= 0:
                dot += z[i, j] * x[i, j]
        if dot < 0:
            z[i, 3:7] = -z[i, 3:7]
        for j in range(13):
            if r[i, j] < 0:
                continue
            s = P[i, j, j] + r[i, j]
            nu = z[i, j] - x[i, j]
            if gate > 0:
                if ratios is not None:
                    ratios.append((i, j, nu * nu / (gate * gate * s)))
                if nu * nu > gate * gate * s:
                    counts[i, 1] += 1
                    continue
            col, row = P[i, :, j].copy(), P[i, j, :].copy()
            x[i] += col * nu / s
            P[i] -= np.outer(col, row) / s
            nis[i] += nu * nu / s
            counts[i, 0] += 1
        if normalize:
            q = x[i, 3:7]
            x[i, 3:7] = q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return x, P, nis, counts


def ekf_ref(x, P, u, p=None, d=None, T=T, steps=1, Q=None, z=None, r=None, gate=0.0, normalize=True, ratios=None):
    """cfnmpc_ekf_step in numpy -> (x_new, P_new, nis, counts)"""
    B = x.shape[0]
    p = np.tile(NOMINAL, (B, 1)) if p is None else p
    d = np.zeros((B, 6)) if d is None else d
    xm, Pm, _ = predict_ref(x, P, u, p, d, T, steps, Q)
    if z is None:
        return xm, Pm, np.zeros(B), np.zeros((B, 2), dtype=np.int32)
    return update_ref(xm, Pm, z, r, gate, normalize, ratios)


# ---- the cases of the CPU and GPU tests ----------------------------------------------------------------------------------------
def random_cov(rng, B, sig):
    """symmetric positive definite [B, 13, 13] with standard deviations about sig and correlations"""
    Lw = np.tril(rng.uniform(-0.3, 0.3, (B, 13, 13)), -1) + np.eye(13)
    Lw = Lw * (sig * rng.uniform(0.7, 1.3, (B, 13)))[:, :, None]
    S = Lw @ np.swapaxes(Lw, 1, 2)
    return 0.5 * (S + np.swapaxes(S, 1, 2))


def mixed_masks(B):
    """per-vehicle masks of measured components: vehicles 0 .. 3 all different (all 13 | the reference's ten | position | attitude
    and rates), then cycling with a shift"""
    sets = [np.r_[0:13], MEASURED["ten"], np.r_[0:3], np.r_[3:7, 10:13], np.r_[0:3, 7:10], np.r_[2:11]]
    m = np.zeros((B, 13), dtype=bool)
    for i in range(B):
        m[i, sets[i % len(sets)]] = True
    return m


@functools.lru_cache(maxsize=None)
def case(seed, B, steps, rows, kind, gate=0.0):
    """one call's inputs (never written to): the draw of tests/test_sim_vjp_cpu.py for (x, u, p, d), a random prior covariance and
    process noise, and a measurement of `kind`:
      "ten" / "pos" / "all": the components of MEASURED, noise of at most one standard deviation of the innovation each;
      "flip": "ten" with the quaternion measured at the other sign;
      "mixed": per-vehicle masks (mixed_masks); with gate > 0 some measured components are put 8 standard deviations out: in vehicle
               4 k + 0 none, 4 k + 1 its first, 4 k + 2 its last, 4 k + 3 its first two -- vehicles 1 and 3 have used and rejected
               components, four consecutive vehicles differ in mask and rejections"""
    c = sv.draw(seed, B, 1)
    rng = np.random.default_rng(1000 + seed)
    p, d = sv.rows_of(c, rows)
    x, u = c["x0"], c["u"][:, 0]
    P = random_cov(rng, B, SIG0)
    Q = random_cov(rng, B, 0.02 * SIG0)
    xm, Pm, _ = predict_ref(x, P, u, p, d, T, steps, Q)
    mask = mixed_masks(B) if kind == "mixed" else np.zeros((B, 13), dtype=bool)
    if kind != "mixed":
        mask[:, MEASURED["ten" if kind == "flip" else kind]] = True
    r = np.where(mask, (SIGZ * rng.uniform(0.5, 2.0, (B, 13))) ** 2, -1.0)
    sd = np.sqrt(np.einsum("bii->bi", Pm) + np.abs(r))
    cdev = rng.uniform(-1.0, 1.0, (B, 13))
    if kind == "mixed" and gate > 0:
        for i in range(B):
            js = np.flatnonzero(mask[i])
            out = {0: [], 1: js[:1], 2: js[-1:], 3: js[:2]}[i % 4]
            cdev[i, out] = 8.0 * np.sign(cdev[i, out])
    z = xm + cdev * sd
    if kind == "flip":
        z[:, 3:7] = -z[:, 3:7]
    out = dict(x=x, u=u, p=p, d=d, P=P, Q=Q, z=z, r=r, mask=mask, rows=rows, steps=steps, gate=gate)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def case_args(c):
    """the keyword arguments of ekf_ref / crazyflie_nmpc_amd.ekf_step a case stands for (p, d: None where the row kind sets none)"""
    return dict(p=c["p"] if "p" in c["rows"] else None, d=c["d"] if "d" in c["rows"] else None, T=T, steps=c["steps"], Q=c["Q"],
                z=c["z"], r=c["r"], gate=c["gate"])


GATE = 3.0
GATE_CASES = [(21, 5, 1, "pd"), (22, 67, 3, "none")]      # (seed, B, steps, rows) of the "mixed" cases with the gate on


# ---- surface and figures -------------------------------------------------------------------------------------------------------
def test_entry_point_declared_exported_and_bound():
    src = _header()
    from crazyflie_nmpc_amd import _lib
    L = _lib.lib()
    assert SIG in src
    assert "#defineCFNMPC_EKF_NORMALIZE_Q1" in src
    assert "cfnmpc_ekf_step" in _lib.SYMBOLS and hasattr(L, "cfnmpc_ekf_step")
    assert list(L.cfnmpc_ekf_step.argtypes) == ARGTYPES


def test_abi_unchanged():
    from crazyflie_nmpc_amd import _lib
    L = _lib.lib()
    assert L.cfnmpc_abi_version() == 9
    assert L.cfnmpc_opts_size() == ctypes.sizeof(_lib.Opts)
    assert "#defineCFNMPC_ABI_VERSION9" in _header()


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "cfnmpc.h"\nint main(void) { return cfnmpc_ekf_step(0, 0, 0, 0, 0, 0, 0.015, 1, 0, 0, 0, 0.0, '
                   'CFNMPC_EKF_NORMALIZE_Q, 0, 0, 0, 0, CFNMPC_ON_HOST, 0) == CFNMPC_EINVAL ? 0 : 1; }\n')
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_surface():
    import inspect
    import crazyflie_nmpc_amd as cf
    sg = inspect.signature(cf.ekf_step).parameters
    assert list(sg) == ["x", "P", "u", "z", "r", "Q", "T", "steps", "gate", "normalize", "params", "dist", "out"]
    assert [sg[k].default for k in list(sg)[3:]] == [None, None, None, 0.015, 1, 0.0, True, None, None, None]
    assert "ekf_step" in cf.__all__


def test_new_kernels_resources(table):  # noqa: F811
    for k in KERNELS:
        assert k in table, k
        e = table[k]
        assert e["unit"] == "cfnmpc_kernels", e
        assert e["occupancy"] >= 1 and not e.get("dynamic_stack"), (k, e)
        assert e["scratch"] == 0 and e["lds"] == 0, (k, e)
        assert e["vgpr"] + e["agpr"] <= VGPR_CEIL[k], (k, e)
    print({k: (table[k]["vgpr"], table[k]["agpr"]) for k in KERNELS})


def test_earlier_kernels_keep_their_figures(table):  # noqa: F811
    import test_resource_budget as rb
    sv.test_earlier_kernels_keep_their_figures(table)
    sv.test_new_kernels_resources(table)
    for k in rb.NO_SCRATCH:
        assert table[k]["scratch"] == 0, k
    for k, (v, a, scratch, occ, lds) in rb.BUDGET.items():
        e = table[k]
        assert e["vgpr"] <= v and e["agpr"] <= a and e["scratch"] <= scratch and e["occupancy"] >= occ and e["lds"] <= lds, (k, e)


# ---- host validation: every refusal comes before anything touches a device, and nothing is written ---------------------------
def _call(B=2, steps=1, T=T, gate=0.0, flags=1, edit=None, drop=(), on_device=0):
    """calls the entry point on a valid host case with one thing changed -> (return code, outputs untouched)"""
    from crazyflie_nmpc_amd import _lib
    L = _lib.lib()
    c = case(3, 2, 1, "pd", "ten")
    a = {k: np.array(c[k]) for k in ("x", "P", "u", "p", "d", "Q", "z", "r")}
    if edit:
        edit(a)
    outs = [np.full((2, 13), 7.0), np.full((2, 13, 13), 7.0), np.full(2, 7.0), np.full((2, 2), 7, dtype=np.int32)]
    names = ["x_new", "P_new", "nis", "counts"]
    ptr = lambda n, arr: None if n in drop else arr.ctypes.data_as(vp)   # noqa: E731
    rc = L.cfnmpc_ekf_step(B, ptr("x", a["x"]), ptr("P", a["P"]), ptr("u", a["u"]), ptr("p", a["p"]), ptr("d", a["d"]), T, steps,
                           ptr("Q", a["Q"]), ptr("z", a["z"]), ptr("r", a["r"]), gate, flags,
                           *(ptr(n, o) for n, o in zip(names, outs)), on_device, None)
    return rc, all((o == 7).all() for o in outs)


def _set(name, idx, v):
    def edit(a):
        a[name][idx] = v
    return edit


def _asym(name):
    def edit(a):
        a[name][1, 2, 5] += 1e-9 * np.abs(a[name][1]).max()
    return edit


@pytest.mark.parametrize("kw", [
    dict(B=0), dict(B=-3), dict(steps=0), dict(T=0.0), dict(T=-0.015), dict(T=float("nan")), dict(gate=-1.0), dict(gate=float("inf")),
    dict(gate=float("nan")), dict(flags=2), dict(flags=3), dict(flags=-1), dict(drop=("x",)), dict(drop=("P",)), dict(drop=("u",)),
    dict(drop=("x_new",)), dict(drop=("P_new",)), dict(drop=("r",)),
    dict(edit=_set("x", (1, 4), np.nan)), dict(edit=_set("u", (0, 1), np.inf)), dict(edit=_set("z", (1, 0), np.nan)),
    dict(edit=_set("r", (0, 12), np.inf)), dict(edit=_set("P", (1, 3, 3), -1e-9)), dict(edit=_set("P", (0, 2, 7), np.nan)),
    dict(edit=_asym("P")), dict(edit=_set("Q", (1, 0, 0), -1e-12)), dict(edit=_asym("Q")), dict(edit=_set("p", (1, 1), 0.0)),
    dict(edit=_set("p", (0, 6), -1.0)), dict(edit=_set("d", (1, 5), np.nan)),
], ids=lambda kw: ",".join(f"{k}={getattr(v, '__name__', v)}" for k, v in kw.items()))
def test_host_validation_refuses_and_writes_nothing(kw):
    rc, untouched = _call(**kw)
    assert rc == EINVAL and untouched


def test_device_argument_checks_come_before_the_launch():
    """the argument checks that do not read the arrays hold for device pointers too (nothing is launched: no device needed)"""
    for kw in (dict(B=0), dict(steps=0), dict(T=0.0), dict(gate=-1.0), dict(flags=2), dict(drop=("P_new",)), dict(drop=("r",))):
        rc, untouched = _call(on_device=1, **kw)
        assert rc == EINVAL and untouched, kw


# ---- the twin is right ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("steps", [1, 3])
def test_twin_jacobian_is_the_derivative_of_the_rollout(rows, steps):
    """the product of the twin's sub-step Jacobians against (a) complex steps through the whole numpy rollout of
    tests/test_sim_vjp_cpu.py and (b) the forward sensitivities of tests/test_disturbance_cpu.py (complex-step stage Jacobians)"""
    B = 6
    c = sv.draw(31, B, 1)
    p, d = sv.rows_of(c, rows)
    x, u = c["x0"], c["u"][:, 0]
    xm, _P, As = predict_ref(x, np.tile(np.eye(13), (B, 1, 1)), u, p, d, T, steps)
    A = functools.reduce(lambda acc, a: a @ acc, As)
    hc = 1e-30
    X = np.repeat(x[:, None, :], 13, axis=1).astype(np.complex128)
    X[:, np.arange(13), np.arange(13)] += 1j * hc
    rep = lambda a: np.repeat(a, 13, axis=0)   # noqa: E731
    xs = sv.rollout(X.reshape(B * 13, 13), rep(c["u"]), rep(p), rep(d), T, steps)[:, 1]
    Acs = np.swapaxes(xs.imag.reshape(B, 13, 13) / hc, 1, 2)
    assert np.array_equal(xs.real.reshape(B, 13, 13)[:, 0], xm)
    ea = rel_err(A, Acs).max()
    eb = 0.0
    for i in range(B):
        xi, Ai, _ = dc.rk4_sens(x[i], u[i], p[i], d[i], T, steps)
        eb = max(eb, rel_err(A[i:i + 1], Ai[None]).max(), rel_err(xm[i:i + 1], xi[None]).max())
    print(f"rows {rows}, steps {steps}: twin A against the rollout's complex-step Jacobian {ea:.2e}, against forward sensitivities {eb:.2e}")
    assert ea <= 1e-13 and eb <= 1e-12


def test_twin_jacobian_at_the_nominal_row_is_the_oracles(oracle):
    B = 4
    c = sv.draw(32, B, 1)
    x, u = c["x0"], c["u"][:, 0]
    xm, _P, As = predict_ref(x, np.tile(np.eye(13), (B, 1, 1)), u, np.tile(NOMINAL, (B, 1)), np.zeros((B, 6)), T, 1)
    for i in range(B):
        phi, A, _Bm = oracle.rk4_sens(x[i], u[i], dt=T)
        assert rel_err(As[0][i:i + 1], A[None]).max() <= 1e-12 and rel_err(xm[i:i + 1], phi[None]).max() <= 1e-13


@pytest.mark.parametrize("kind", ["ten", "pos", "all", "mixed"])
def test_sequential_update_is_the_joint_update(kind):
    """gate off, no normalisation: x, P and the NIS against K = P H' (H P H' + R)^-1 with np.linalg.solve, to 1e-12"""
    c = case(41, 8, 1, "pd", kind)
    a = case_args(c)
    xm, Pm, _ = predict_ref(c["x"], c["P"], c["u"], c["p"], c["d"], T, 1, c["Q"])
    x, P, nis, counts = ekf_ref(c["x"], c["P"], c["u"], normalize=False, **a)
    worst = 0.0
    for i in range(8):
        js = np.flatnonzero(c["r"][i] >= 0)
        H = np.eye(13)[js]
        S = H @ Pm[i] @ H.T + np.diag(c["r"][i, js])
        nu = c["z"][i, js] - xm[i, js]
        K = np.linalg.solve(S, H @ Pm[i]).T
        xj, Pj, nj = xm[i] + K @ nu, Pm[i] - K @ H @ Pm[i], nu @ np.linalg.solve(S, nu)
        worst = max(worst, rel_err(x[i:i + 1], xj[None]).max(), rel_err(P[i:i + 1], Pj[None]).max(), abs(nis[i] - nj) / nj)
        assert tuple(counts[i]) == (len(js), 0)
    print(f"{kind}: sequential against joint update {worst:.2e}")
    assert worst <= 1e-12


def test_three_sub_steps_are_three_chained_predictions():
    c = case(42, 5, 3, "pd", "ten")
    x3, P3, nis, counts = ekf_ref(c["x"], c["P"], c["u"], p=c["p"], d=c["d"], T=T, steps=3)
    x, P = c["x"], c["P"]
    for _ in range(3):
        x, P, _n, _c = ekf_ref(x, P, c["u"], p=c["p"], d=c["d"], T=T / 3, steps=1)
    assert np.array_equal(x, x3) and np.array_equal(P, P3)
    assert not nis.any() and not counts.any()


def test_symmetric_covariance_stays_symmetric_in_the_twin():
    c = case(43, 5, 1, "pd", "all")
    _x, P, _n, _c = ekf_ref(c["x"], c["P"], c["u"], **case_args(c))
    assert rel_err(P, np.swapaxes(P, 1, 2)).max() <= 1e-15
    assert (np.linalg.eigvalsh(0.5 * (P + np.swapaxes(P, 1, 2))) > 0).all()


def test_flipped_quaternion_measurement_is_the_same_measurement():
    c = case(44, 5, 1, "none", "flip")
    a = case_args(c)
    z2 = np.array(c["z"]); z2[:, 3:7] = -z2[:, 3:7]
    r1 = ekf_ref(c["x"], c["P"], c["u"], **a)
    r2 = ekf_ref(c["x"], c["P"], c["u"], **dict(a, z=z2))
    assert all(np.array_equal(p, q) for p, q in zip(r1, r2))
    assert (np.abs(np.linalg.norm(r1[0][:, 3:7], axis=1) - 1) <= 1e-15).all()


@pytest.mark.parametrize("seed,B,steps,rows", GATE_CASES)
def test_gate_cases_keep_their_distance_from_the_threshold(seed, B, steps, rows):
    c = case(seed, B, steps, rows, "mixed", GATE)
    ratios = []
    _x, _P, _n, counts = ekf_ref(c["x"], c["P"], c["u"], ratios=ratios, **case_args(c))
    rt = np.array([v for _i, _j, v in ratios])
    assert len(rt) == c["mask"].sum()
    assert not ((rt >= 0.9) & (rt <= 1.1)).any(), rt[(rt > 0.5) & (rt < 2.0)]
    assert (counts.sum(axis=1) == c["mask"].sum(axis=1)).all()
    assert ((counts[:, 0] > 0) & (counts[:, 1] > 0)).any()          # a vehicle with a used and a rejected component
    n = min(B, 4)
    assert list(counts[:n, 1]) == [0, 1, 1, 2][:n]
    for i in range(n):
        for j in range(i + 1, n):
            rej_i = {jj for ii, jj, v in ratios if ii == i and v > 1}
            rej_j = {jj for ii, jj, v in ratios if ii == j and v > 1}
            assert (c["mask"][i] != c["mask"][j]).any() and (rej_i != rej_j or not rej_i)
    print(f"B {B}: {int(counts[:, 0].sum())} used, {int(counts[:, 1].sum())} rejected; ratios used <= {rt[rt < 1].max():.3f}, rejected >= {rt[rt > 1].min():.3f}")


# ---- the host-compiled plain-loop step under the host sanitizers ------------------------------------------------------------
def test_ekf_check_runs_clean_under_the_host_sanitizers(tmp_path):
    cases = []
    todo = [(51, 1, "none", "ten", 0.0, 1, True), (52, 3, "p", "all", 0.0, 0, True), (53, 1, "pd", "flip", 0.0, 1, True),
            (21, 1, "pd", "mixed", GATE, 1, True), (54, 3, "pd", "pos", GATE, 1, False), (55, 3, "none", "ten", 0.0, 1, None)]
    for seed, steps, rows, kind, gate, flags, with_q in todo:      # with_q None: predict only
        c = case(seed, 5, steps, rows, kind, gate)
        a = case_args(c)
        if not with_q:
            a["Q"] = None
        if with_q is None:
            a["z"] = a["r"] = None
        x, P, nis, counts = ekf_ref(c["x"], c["P"], c["u"], normalize=bool(flags), **a)
        knd = {"none": 0, "p": 1, "pd": 2}[rows]
        for i in range(5):
            parts = [c["p"][i], c["d"][i], c["x"][i], c["P"][i], c["u"][i], c["Q"][i], c["z"][i], c["r"][i], x[i], P[i],
                     [nis[i], counts[i, 0], counts[i, 1]]]
            cases.append(f"{steps} {knd} {T!r} {gate!r} {flags} {int(bool(with_q))} {int(with_q is not None)}\n"
                         + "\n".join(" ".join(repr(float(v)) for v in np.ravel(q)) for q in parts))
    path = tmp_path / "cases.txt"
    path.write_text(f"{len(cases)}\n" + "\n".join(cases) + "\n")
    csrc = os.path.join(ROOT, "crazyflie_nmpc_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "-s", "ekf_check", f"OBJDIR={tmp_path}", f"CASES={path}"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and f"ekf_check ok: {len(cases)} cases" in r.stdout and "runtime error" not in r.stderr
    r = subprocess.run(["make", "-C", csrc, "-s", "ekf_check", f"OBJDIR={tmp_path}"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ekf_check ok: built-in checks" in r.stdout and "runtime error" not in r.stderr
