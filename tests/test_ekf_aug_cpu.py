"""CPU checks of the disturbance-augmented extended Kalman filter (include/cfnmpc.h: cfnmpc_ekf_aug_step):
the entry point is declared, exported and bound, the ABI is unchanged, k_ekf_aug is in the built code within its recorded ceiling
while every earlier kernel keeps its figures, the host validation refuses what the header says it refuses without touching the
outputs, and the numpy twin the GPU tests compare against (ekf_aug_ref: the header's rules step for step) is right:

  - the product of its F_s is the complex-step Jacobian of the whole numpy rollout of tests/test_sim_vjp_cpu.py with respect to
    (x, d[sel]);
  - with the gate off its sequential update is the joint Kalman update K = Pa H' (H Pa H' + R)^-1;
  - steps = 3 is three chained predictions of steps = 1;
  - with no slot in use its state block and state are ekf_ref's (tests/test_ekf_cpu.py);
  - the gate cases the GPU tests use keep every decision away from its threshold;
  - on a 300-step run with dropouts and outliers it ends consistent (e' Pdd^-1 e within the 0.999 quantile of chi-square with three
    degrees of freedom), rejects the outliers and nothing else, and estimates the disturbance better than the one-step observer's
    rule run on its own state estimates.

The stand-alone program tools/ekf_aug_check.cpp runs the host-compiled plain-loop step on cases written here, under the host
sanitizers.  Error measure everywhere: rel_err of tests/test_ekf_cpu.py.  No GPU needed."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import test_disturbance_cpu as dc
import test_ekf_cpu as ec
import test_sim_vjp_cpu as sv
from test_ekf_cpu import SIG0, SIGZ, MEASURED, T, rel_err
from test_model_params_cpu import NOMINAL, ROOT, _header, table  # noqa: F401  (table: the fixture)

SIG = ("intcfnmpc_ekf_aug_step(intbatch,constdouble*x,constdouble*d,constdouble*Pa,constdouble*u,constdouble*p,constint*sel,doubleT,"
       "intsteps,constdouble*Q,constdouble*Qd,constdouble*z,constdouble*r,doublegate,intflags,double*x_new,double*d_new,"
       "double*Pa_new,double*Pxx_new,double*nis,int*counts,inton_device,void*stream);")
vp, i32, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
ARGTYPES = [i32, vp, vp, vp, vp, vp, vp, dbl, i32, vp, vp, vp, vp, dbl, i32, vp, vp, vp, vp, vp, vp, i32, vp]
# ceiling of the new kernel, VGPRs + AGPRs of the unified file (512 per lane at one wave per SIMD): the figure of the build
# (506) rounded up to 8; no scratch, no LDS.  512 is also all a lane can have under __launch_bounds__(64),
# so this ceiling cannot fire on its own: what guards against register growth here is scratch == 0 (the next six registers spill)
VGPR_CEIL = {"k_ekf_aug": 512}
EINVAL = -1
NA = 16
SELS = [(0, 1, 2), (3, 4, 5), (2, 3, 4), (2, -1, -1)]
# standard deviations of the test covariances of the six disturbance components (world acceleration | angular acceleration)
SIGD = np.repeat([0.5, 2.0], [3, 3])


@pytest.fixture(autouse=True)
def _the_entry_point_is_there():
    """every test of this file, the checks of the twin included, is about cfnmpc_ekf_aug_step: a twin of a call the built library
    does not have is a reference of nothing, and none of them passes without it"""
    from crazyflie_nmpc_amd import _lib
    assert hasattr(_lib.lib(), "cfnmpc_ekf_aug_step")


# ---- the numpy twin ------------------------------------------------------------------------------------------------------------
def used_slots(sel):
    return [k for k in range(3) if sel[k] >= 0]


def substep_aug(x, u, k, d, h, sel):
    """one RK4 sub-step of every vehicle and F = [[A, G S], [0, I]] by complex steps through the sub-step with respect to
    (x, d[sel]): x [B, 13], u [B, 4], k [8, B], d [6, B] -> (x+ [B, 13], F [B, 16, 16])"""
    hc = 1e-30
    B = x.shape[0]
    X = np.repeat(x.T[:, :, None], NA, axis=2).astype(np.complex128)     # [component, vehicle, direction]
    D = np.repeat(d[:, :, None], NA, axis=2).astype(np.complex128)
    X[np.arange(13), :, np.arange(13)] += 1j * hc
    for s in used_slots(sel):
        D[sel[s], :, 13 + s] += 1j * hc
    out = sv.rk4_step(X, u.T[:, :, None], k[:, :, None], D, h)
    F = np.tile(np.eye(NA), (B, 1, 1))
    F[:, :13, :] = np.moveaxis(out.imag / hc, 1, 0)
    return sv.rk4_step(x.T, u.T, k, d, h).T, F


def predict_aug_ref(x, Pa, u, p, d, sel, T, steps, Q=None, Qd=None):
    """the predict rule -> (x^-, Pa^-, [F_0, .., F_{steps - 1}])"""
    k = sv.derive(np.moveaxis(p, -1, 0)); dd = np.moveaxis(d, -1, 0)
    x, Pa, Fs = np.array(x, dtype=np.float64), np.array(Pa, dtype=np.float64), []
    for _ in range(steps):
        x, F = substep_aug(x, u, k, dd, T / steps, sel)
        Pa = F @ Pa @ np.swapaxes(F, 1, 2)
        Fs.append(F)
    if Q is not None:
        Pa[:, :13, :13] += Q
    if Qd is not None:
        for s in used_slots(sel):
            Pa[:, 13 + s, 13 + s] += Qd[:, s]
    return x, Pa, Fs


def update_aug_ref(a, Pa, z, r, gate, normalize, ratios=None):
    """ekf_ref's update rules on (a^- [B, 16], Pa^-), vehicle by vehicle -> (a, Pa, nis, counts)"""
    B = a.shape[0]
    a, Pa, z = a.copy(), Pa.copy(), np.array(z, dtype=np.float64)
    nis, counts = np.zeros(B), np.zeros((B, 2), dtype=np.int32)
    for i in range(B):
        dot = 0.0
        for j in range(3, 7):
            if r[i, j] >= 0:
                dot += z[i, j] * a[i, j]
        if dot < 0:
            z[i, 3:7] = -z[i, 3:7]
        for j in range(13):
            if r[i, j] < 0:
                continue
            s = Pa[i, j, j] + r[i, j]
            nu = z[i, j] - a[i, j]
            if gate > 0:
                if ratios is not None:
                    ratios.append((i, j, nu * nu / (gate * gate * s)))
                if nu * nu > gate * gate * s:
                    counts[i, 1] += 1
                    continue
            col, row = Pa[i, :, j].copy(), Pa[i, j, :].copy()
            a[i] += col * nu / s
            Pa[i] -= np.outer(col, row) / s
            nis[i] += nu * nu / s
            counts[i, 0] += 1
        if normalize:
            q = a[i, 3:7]
            a[i, 3:7] = q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return a, Pa, nis, counts


def ekf_aug_ref(x, d, Pa, u, sel, p=None, T=T, steps=1, Q=None, Qd=None, z=None, r=None, gate=0.0, normalize=True, ratios=None):
    """cfnmpc_ekf_aug_step in numpy -> (x_new, d_new, Pa_new, nis, counts)"""
    B = x.shape[0]
    p = np.tile(NOMINAL, (B, 1)) if p is None else p
    xm, Pm, _ = predict_aug_ref(x, Pa, u, p, d, sel, T, steps, Q, Qd)
    if z is None:
        return xm, np.array(d), Pm, np.zeros(B), np.zeros((B, 2), dtype=np.int32)
    a = np.zeros((B, NA))
    a[:, :13] = xm
    for s in used_slots(sel):
        a[:, 13 + s] = d[:, sel[s]]
    a, Pn, nis, counts = update_aug_ref(a, Pm, z, r, gate, normalize, ratios)
    dn = np.array(d)
    for s in used_slots(sel):
        dn[:, sel[s]] = a[:, 13 + s]
    return a[:, :13].copy(), dn, Pn, nis, counts


# ---- the cases of the CPU and GPU tests ----------------------------------------------------------------------------------------
def random_cov_aug(rng, B, sel):
    """symmetric positive semi-definite [B, 16, 16] with correlations between the state and the slots; the rows and columns of
    unused slots are zero"""
    sig = np.concatenate([SIG0, [SIGD[s] if s >= 0 else 1.0 for s in sel]])
    Lw = np.tril(rng.uniform(-0.3, 0.3, (B, NA, NA)), -1) + np.eye(NA)
    Lw = Lw * (sig * rng.uniform(0.7, 1.3, (B, NA)))[:, :, None]
    S = Lw @ np.swapaxes(Lw, 1, 2)
    S = 0.5 * (S + np.swapaxes(S, 1, 2))
    for k in range(3):
        if sel[k] < 0:
            S[:, 13 + k, :] = 0.0
            S[:, :, 13 + k] = 0.0
    return S


@functools.lru_cache(maxsize=None)
def case(seed, B, steps, rows, kind, sel, gate=0.0):
    """one call's inputs (never written to), as tests/test_ekf_cpu.py's case: its draw for (x, u, p, d), a random augmented prior and
    process noise (Q, Qd), and a measurement of `kind` ("ten" / "pos" / "all" / "flip" / "mixed", with the outliers of "mixed" when
    gate > 0) around the AUGMENTED filter's own prediction.  rows: "d" (p = None, the nominal row) or "pd"."""
    c = sv.draw(seed, B, 1)
    rng = np.random.default_rng(2000 + seed)
    p = c["p"] if "p" in rows else None
    d, x, u = c["d"], c["x0"], c["u"][:, 0]
    Pa = random_cov_aug(rng, B, sel)
    Q = ec.random_cov(rng, B, 0.02 * SIG0)
    Qd = (0.05 * SIGD[np.maximum(sel, 0)] * rng.uniform(0.5, 2.0, (B, 3))) ** 2
    xm, Pm, _ = predict_aug_ref(x, Pa, u, np.tile(NOMINAL, (B, 1)) if p is None else p, d, sel, T, steps, Q, Qd)
    mask = ec.mixed_masks(B) if kind == "mixed" else np.zeros((B, 13), dtype=bool)
    if kind != "mixed":
        mask[:, MEASURED["ten" if kind == "flip" else kind]] = True
    r = np.where(mask, (SIGZ * rng.uniform(0.5, 2.0, (B, 13))) ** 2, -1.0)
    sd = np.sqrt(np.einsum("bii->bi", Pm)[:, :13] + np.abs(r))
    cdev = rng.uniform(-1.0, 1.0, (B, 13))
    if kind == "mixed" and gate > 0:
        for i in range(B):
            js = np.flatnonzero(mask[i])
            out = {0: [], 1: js[:1], 2: js[-1:], 3: js[:2]}[i % 4]
            cdev[i, out] = 8.0 * np.sign(cdev[i, out])
    z = xm + cdev * sd
    if kind == "flip":
        z[:, 3:7] = -z[:, 3:7]
    out = dict(x=x, u=u, p=p, d=d, Pa=Pa, Q=Q, Qd=Qd, z=z, r=r, mask=mask, rows=rows, steps=steps, gate=gate, sel=sel)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def case_args(c):
    """the keyword arguments of ekf_aug_ref a case stands for"""
    return dict(p=c["p"], T=T, steps=c["steps"], Q=c["Q"], Qd=c["Qd"], z=c["z"], r=c["r"], gate=c["gate"])


GATE = 3.0
GATE_CASES = [(21, 5, 1, "pd", (0, 1, 2)), (22, 67, 3, "d", (2, 3, 4))]      # (seed, B, steps, rows, sel) of the "mixed" cases with the gate on


# ---- surface and figures -------------------------------------------------------------------------------------------------------
def test_entry_point_declared_exported_and_bound():
    src = _header()
    from crazyflie_nmpc_amd import _lib
    L = _lib.lib()
    assert SIG in src
    assert "#defineCFNMPC_EKF_NA16" in src
    assert "cfnmpc_ekf_aug_step" in _lib.SYMBOLS and hasattr(L, "cfnmpc_ekf_aug_step")
    assert list(L.cfnmpc_ekf_aug_step.argtypes) == ARGTYPES


def test_abi_unchanged():
    from crazyflie_nmpc_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "cfnmpc_ekf_aug_step")
    assert L.cfnmpc_abi_version() == 9
    assert L.cfnmpc_opts_size() == ctypes.sizeof(_lib.Opts)
    assert "#defineCFNMPC_ABI_VERSION9" in _header()


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "cfnmpc.h"\nint main(void) { double Pa[CFNMPC_EKF_NA][CFNMPC_EKF_NA]; (void)Pa; '
                   'return cfnmpc_ekf_aug_step(0, 0, 0, 0, 0, 0, 0, 0.015, 1, 0, 0, 0, 0, 0.0, CFNMPC_EKF_NORMALIZE_Q, 0, 0, 0, 0, 0, 0, '
                   'CFNMPC_ON_HOST, 0) == CFNMPC_EINVAL ? 0 : 1; }\n')
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_surface():
    import inspect
    import crazyflie_nmpc_amd as cf
    sg = inspect.signature(cf.ekf_aug_step).parameters
    assert list(sg) == ["x", "d", "Pa", "u", "sel", "z", "r", "Q", "Qd", "T", "steps", "gate", "normalize", "params", "out", "Pxx_out"]
    assert [sg[k].default for k in list(sg)[5:]] == [None, None, None, None, 0.015, 1, 0.0, True, None, None, None]
    assert "ekf_aug_step" in cf.__all__ and "ekf_aug_cov" in cf.__all__
    P = ec.random_cov(np.random.default_rng(1), 2, SIG0)
    Pa = cf.ekf_aug_cov(P, [0.5, 0.0, 2.0])
    assert Pa.shape == (2, 16, 16) and np.array_equal(Pa[:, :13, :13], P)
    assert np.array_equal(Pa[:, 13:, 13:], np.tile(np.diag([0.25, 0.0, 4.0]), (2, 1, 1))) and not Pa[:, :13, 13:].any() and not Pa[:, 13:, :13].any()
    assert cf.ekf_aug_cov(P[0], [0.5, 0.0, 2.0]).shape == (1, 16, 16)      # (a shared P and shared deviations: one matrix ...)
    Pb = cf.ekf_aug_cov(P[0], [0.5, 0.0, 2.0], B=3)                        # (... or B copies of it)
    assert Pb.shape == (3, 16, 16) and all(np.array_equal(Pb[i], Pa[0]) for i in range(3))
    with pytest.raises(ValueError):
        cf.ekf_aug_cov(P, [0.5, 0.0, 2.0], B=3)


def test_new_kernel_resources(table):  # noqa: F811
    for k in VGPR_CEIL:
        assert k in table, k
        e = table[k]
        assert e["unit"] == "cfnmpc_kernels", e
        assert e["occupancy"] >= 1 and not e.get("dynamic_stack"), (k, e)
        assert e["scratch"] == 0 and e["lds"] == 0, (k, e)
        assert e["vgpr"] + e["agpr"] <= VGPR_CEIL[k], (k, e)
    print({k: (table[k]["vgpr"], table[k]["agpr"]) for k in VGPR_CEIL})


def test_earlier_kernels_keep_their_figures(table):  # noqa: F811
    assert "k_ekf_aug" in table
    ec.test_earlier_kernels_keep_their_figures(table)
    ec.test_new_kernels_resources(table)


# ---- host validation: every refusal comes before anything touches a device, and nothing is written ---------------------------
def _call(B=2, steps=1, T=T, gate=0.0, flags=1, edit=None, drop=(), on_device=0, sel=(2, -1, 4)):
    """calls the entry point on a valid host case with one thing changed -> (return code, outputs untouched)"""
    from crazyflie_nmpc_amd import _lib
    L = _lib.lib()
    c = case(3, 2, 1, "pd", "ten", (2, -1, 4))
    a = {k: np.array(c[k]) for k in ("x", "d", "Pa", "u", "p", "Q", "Qd", "z", "r")}
    if edit:
        edit(a)
    outs = [np.full((2, 13), 7.0), np.full((2, 6), 7.0), np.full((2, 16, 16), 7.0), np.full((2, 13, 13), 7.0), np.full(2, 7.0),
            np.full((2, 2), 7, dtype=np.int32)]
    names = ["x_new", "d_new", "Pa_new", "Pxx_new", "nis", "counts"]
    sel_a = (ctypes.c_int * 3)(*sel)
    ptr = lambda n, arr: None if n in drop else arr.ctypes.data_as(vp)   # noqa: E731
    rc = L.cfnmpc_ekf_aug_step(B, ptr("x", a["x"]), ptr("d", a["d"]), ptr("Pa", a["Pa"]), ptr("u", a["u"]), ptr("p", a["p"]),
                               None if "sel" in drop else ctypes.cast(sel_a, vp), T, steps, ptr("Q", a["Q"]), ptr("Qd", a["Qd"]),
                               ptr("z", a["z"]), ptr("r", a["r"]), gate, flags, *(ptr(n, o) for n, o in zip(names, outs)), on_device, None)
    return rc, all((o == 7).all() for o in outs)


_set, _asym = ec._set, ec._asym


def _slot_row(a):
    a["Pa"][1, 14, 3] = a["Pa"][1, 3, 14] = 1e-6      # (symmetric, but slot 1 is unused)


def _slot_diag(a):
    a["Pa"][0, 14, 14] = 1e-6


def _asym16(a):
    a["Pa"][1, 2, 15] += 1e-9 * np.abs(a["Pa"][1]).max()


@pytest.mark.parametrize("kw", [
    dict(sel=(6, 0, 1)), dict(sel=(0, -2, 1)), dict(sel=(3, 1, 3)), dict(sel=(0, 0, -1)), dict(drop=("sel",)),
    dict(edit=_slot_row), dict(edit=_slot_diag), dict(sel=(2, 3, -1)), dict(edit=_asym16), dict(edit=_asym("Pa")),
    dict(edit=_set("Qd", (1, 0), -1e-12)), dict(edit=_set("Qd", (0, 2), np.nan)), dict(edit=_set("Qd", (1, 2), np.inf)),
    dict(drop=("d",)), dict(drop=("d_new",)), dict(drop=("Pa_new",)), dict(drop=("r",)),
    dict(B=0), dict(B=-3), dict(steps=0), dict(T=0.0), dict(T=-0.015), dict(T=float("nan")), dict(gate=-1.0), dict(gate=float("inf")),
    dict(gate=float("nan")), dict(flags=2), dict(flags=3), dict(flags=-1), dict(drop=("x",)), dict(drop=("Pa",)), dict(drop=("u",)),
    dict(drop=("x_new",)),
    dict(edit=_set("x", (1, 4), np.nan)), dict(edit=_set("u", (0, 1), np.inf)), dict(edit=_set("z", (1, 0), np.nan)),
    dict(edit=_set("r", (0, 12), np.inf)), dict(edit=_set("Pa", (1, 3, 3), -1e-9)), dict(edit=_set("Pa", (0, 2, 7), np.nan)),
    dict(edit=_set("Pa", (0, 15, 15), -1e-9)), dict(edit=_set("Q", (1, 0, 0), -1e-12)), dict(edit=_asym("Q")),
    dict(edit=_set("p", (1, 1), 0.0)), dict(edit=_set("p", (0, 6), -1.0)), dict(edit=_set("d", (1, 5), np.nan)),
], ids=lambda kw: ",".join(f"{k}={getattr(v, '__name__', v)}" for k, v in kw.items()))
def test_host_validation_refuses_and_writes_nothing(kw):
    """(sel = (2, 3, -1): the case's Pa has a non-zero row for slot 2, which that selection leaves unused)"""
    rc, untouched = _call(**kw)
    assert rc == EINVAL and untouched


def test_the_qd_entry_of_an_unused_slot_is_ignored():
    """... by the validation as by the arithmetic: the call gets as far as the device (CFNMPC_EHIP where there is none)"""
    rc, _untouched = _call(edit=_set("Qd", (0, 1), -1.0))
    assert rc != EINVAL


def test_device_argument_checks_come_before_the_launch():
    """the argument checks that do not read the arrays, sel's among them (a host array in every call), hold for device pointers too
    (nothing is launched: no device needed)"""
    for kw in (dict(B=0), dict(steps=0), dict(T=0.0), dict(gate=-1.0), dict(flags=2), dict(drop=("Pa_new",)), dict(drop=("d_new",)),
               dict(drop=("d",)), dict(drop=("r",)), dict(drop=("sel",)), dict(sel=(6, 0, 1)), dict(sel=(0, -2, 1)), dict(sel=(3, 1, 3))):
        rc, untouched = _call(on_device=1, **kw)
        assert rc == EINVAL and untouched, kw


# ---- the twin is right ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sel", SELS, ids=str)
@pytest.mark.parametrize("rows", ["d", "pd"])
@pytest.mark.parametrize("steps", [1, 3])
def test_twin_jacobian_is_the_derivative_of_the_rollout(rows, steps, sel):
    """the product of the twin's F_s against complex steps through the whole numpy rollout of tests/test_sim_vjp_cpu.py with respect
    to (x, d[sel]); the bound tests/test_ekf_cpu.py holds A to"""
    B = 6
    c = sv.draw(31, B, 1)
    p, d = sv.rows_of(c, rows)
    x, u = c["x0"], c["u"][:, 0]
    xm, _P, Fs = predict_aug_ref(x, np.tile(np.eye(NA), (B, 1, 1)), u, p, d, sel, T, steps)
    F = functools.reduce(lambda acc, a: a @ acc, Fs)
    hc = 1e-30
    X = np.repeat(x[:, None, :], NA, axis=1).astype(np.complex128)      # [vehicle, direction, component]
    D = np.repeat(d[:, None, :], NA, axis=1).astype(np.complex128)
    X[:, np.arange(13), np.arange(13)] += 1j * hc
    for s in used_slots(sel):
        D[:, 13 + s, sel[s]] += 1j * hc
    rep = lambda a: np.repeat(a, NA, axis=0)   # noqa: E731
    xs = sv.rollout(X.reshape(B * NA, 13), rep(c["u"]), rep(p), D.reshape(B * NA, 6), T, steps)[:, 1]
    Fcs = np.tile(np.eye(NA), (B, 1, 1))
    Fcs[:, :13, :] = np.swapaxes(xs.imag.reshape(B, NA, 13) / hc, 1, 2)
    assert np.array_equal(xs.real.reshape(B, NA, 13)[:, 0], xm)
    ea = rel_err(F, Fcs).max()
    eg = rel_err(F[:, :13, 13:], Fcs[:, :13, 13:]).max()      # (the G block on its own scale: its entries are of order h)
    for k in range(3):
        assert (sel[k] >= 0) == bool(F[:, :13, 13 + k].any())
    print(f"rows {rows}, steps {steps}, sel {sel}: twin F against the rollout's complex-step Jacobian {ea:.2e}, its G block {eg:.2e}")
    assert ea <= 1e-13 and eg <= 1e-13


@pytest.mark.parametrize("kind", ["ten", "pos", "all", "mixed"])
def test_sequential_update_is_the_joint_update(kind):
    """gate off, no normalisation: a, Pa and the NIS against K = Pa H' (H Pa H' + R)^-1 with np.linalg.solve, to 1e-12"""
    B, sel = 8, (2, 3, 4)
    c = case(41, B, 1, "pd", kind, sel)
    xm, Pm, _ = predict_aug_ref(c["x"], c["Pa"], c["u"], c["p"], c["d"], sel, T, 1, c["Q"], c["Qd"])
    x, d, Pa, nis, counts = ekf_aug_ref(c["x"], c["d"], c["Pa"], c["u"], sel, normalize=False, **case_args(c))
    am = np.concatenate([xm, c["d"][:, list(sel)]], axis=1)
    worst = 0.0
    for i in range(B):
        js = np.flatnonzero(c["r"][i] >= 0)
        H = np.eye(NA)[js]
        S = H @ Pm[i] @ H.T + np.diag(c["r"][i, js])
        nu = c["z"][i, js] - am[i, js]
        K = np.linalg.solve(S, H @ Pm[i]).T
        aj, Pj, nj = am[i] + K @ nu, Pm[i] - K @ H @ Pm[i], nu @ np.linalg.solve(S, nu)
        got = np.concatenate([x[i], d[i, list(sel)]])
        worst = max(worst, rel_err(got[None], aj[None]).max(), rel_err(got[None, 13:], aj[None, 13:]).max(),
                    rel_err(Pa[i:i + 1], Pj[None]).max(), abs(nis[i] - nj) / nj)
        assert tuple(counts[i]) == (len(js), 0)
        assert np.array_equal(d[i, [0, 1, 5]], c["d"][i, [0, 1, 5]])
    print(f"{kind}: sequential against joint update {worst:.2e}")
    assert worst <= 1e-12


def test_three_sub_steps_are_three_chained_predictions():
    sel = (0, 1, 2)
    c = case(42, 5, 3, "pd", "ten", sel)
    x3, d3, P3, nis, counts = ekf_aug_ref(c["x"], c["d"], c["Pa"], c["u"], sel, p=c["p"], T=T, steps=3)
    x, P = c["x"], c["Pa"]
    for _ in range(3):
        x, _d, P, _n, _c = ekf_aug_ref(x, c["d"], P, c["u"], sel, p=c["p"], T=T / 3, steps=1)
    assert np.array_equal(x, x3) and np.array_equal(P, P3) and np.array_equal(d3, c["d"])
    assert not nis.any() and not counts.any()


@pytest.mark.parametrize("kind,gate", [("ten", 0.0), ("mixed", GATE)])
def test_without_slots_the_state_block_is_the_siblings(kind, gate):
    """sel = (-1, -1, -1) with zero slot rows: x, the state block, the NIS and the counts are ekf_ref's, to rounding (the
    zero rows take part in the twin's 16 x 16 products)"""
    sel = (-1, -1, -1)
    c = case(45, 6, 3, "pd", kind, sel, gate)
    assert not c["Pa"][:, 13:, :].any() and not c["Pa"][:, :, 13:].any()
    x, d, Pa, nis, counts = ekf_aug_ref(c["x"], c["d"], c["Pa"], c["u"], sel, **case_args(c))
    xr, Pr, nr, cr = ec.ekf_ref(c["x"], np.ascontiguousarray(c["Pa"][:, :13, :13]), c["u"], p=c["p"], d=c["d"], T=T, steps=3, Q=c["Q"],
                                z=c["z"], r=c["r"], gate=gate)
    assert rel_err(x, xr).max() <= 1e-14 and rel_err(Pa[:, :13, :13], Pr).max() <= 1e-14 and rel_err(nis[:, None], nr[:, None]).max() <= 1e-13
    assert np.array_equal(counts, cr) and np.array_equal(d, c["d"])
    assert not Pa[:, 13:, :].any() and not Pa[:, :, 13:].any()
    assert gate == 0.0 or cr[:, 1].sum() > 0


def test_symmetric_covariance_stays_symmetric_in_the_twin():
    sel = (3, 4, 5)
    c = case(43, 5, 1, "pd", "all", sel)
    _x, _d, Pa, _n, _c = ekf_aug_ref(c["x"], c["d"], c["Pa"], c["u"], sel, **case_args(c))
    assert rel_err(Pa, np.swapaxes(Pa, 1, 2)).max() <= 1e-15
    assert (np.linalg.eigvalsh(0.5 * (Pa + np.swapaxes(Pa, 1, 2))) > 0).all()


@pytest.mark.parametrize("seed,B,steps,rows,sel", GATE_CASES)
def test_gate_cases_keep_their_distance_from_the_threshold(seed, B, steps, rows, sel):
    c = case(seed, B, steps, rows, "mixed", sel, GATE)
    ratios = []
    _x, _d, _P, _n, counts = ekf_aug_ref(c["x"], c["d"], c["Pa"], c["u"], sel, ratios=ratios, **case_args(c))
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


# ---- the closed-loop case of the GPU test ------------------------------------------------------------------------------------
RUN_B, RUN_STEPS, RUN_GATE = 5, 300, 5.0
RUN_SELS = [(0, 1, 2), (2, 3, 4)]
RUN_R = np.where(np.isin(np.arange(13), MEASURED["ten"]), SIGZ ** 2, -1.0)      # the reference's ten components, SIGZ noise
RUN_QSD = np.repeat([1e-4, 1e-4, 2e-2, 5e-2], [3, 4, 3, 3])                     # the filter's process noise (the plant has none)
RUN_SIGD0 = np.repeat([1.0, 2.5], [3, 3])                                       # prior standard deviation of a slot
RUN_QD = 1e-8                                                                   # random-walk variance per step of a slot
CHI2_3_999 = 16.27
# seeds of the measurement noise, fixed so that the twin alone meets the checks below.  The components of d no slot estimates are
# an unmodelled disturbance here (with sel = (2, 3, 4): 2 m/s^2 sideways and 5 rad/s^2 about z, 0.075 rad/s per step against a gyro
# noise of 0.03), which brings valid innovations to 0.87 of the gate: of the seeds 204 .. 215 for that selection, 204, 209 and 211
# put one within 10 % of its threshold and 215 has a valid measurement rejected; the other eight pass like this one
RUN_SEED = {(0, 1, 2): 190, (2, 3, 4): 205}


@functools.lru_cache(maxsize=None)
def run_data(sel):
    """the truth, the inputs and the measurements of the run: the RK4 plant (tests/test_sim_vjp_cpu.py's rk4_step) from a perturbed
    hover under a constant per-vehicle disturbance row d, the ten measured components with SIGZ noise, a mocap dropout
    (r[:7] < 0) every 11th step and a 0.5 m position outlier every 37th.  The filter starts at d = 0 in all six components: the
    ones no slot estimates stay there, an unmodelled disturbance the process noise Q has to cover."""
    rng = np.random.default_rng(RUN_SEED[sel])
    B, n = RUN_B, RUN_STEPS
    c = sv.draw(190, B, 1)
    p, d = c["p"], c["d"]
    k = sv.derive(p.T); dd = d.T
    x = np.array(c["x0"]); x[:, 7:13] *= 0.2
    us = sv.hover(p)[None, :, None] + rng.uniform(-0.3, 0.3, (n, B, 4))
    xs, zs, rs, outl = [x], [], [], np.zeros((n, B), dtype=bool)
    for t in range(n):
        x = sv.rk4_step(x.T, us[t].T, k, dd, T).T
        z = x + np.sqrt(np.abs(RUN_R)) * rng.standard_normal((B, 13))
        r = np.tile(RUN_R, (B, 1))
        if t % 11 == 10:
            r[:, :7] = -1.0
        if t % 37 == 36:
            z[np.arange(B), rng.integers(0, 3, B)] += 0.5 * rng.choice([-1.0, 1.0], B)
            outl[t] = True
        xs.append(x); zs.append(z); rs.append(r)
    x0 = xs[0] + SIG0 * 0.5 * rng.standard_normal((B, 13))
    d0 = np.zeros_like(d)
    Pa0 = np.zeros((B, NA, NA))
    Pa0[:, np.arange(NA), np.arange(NA)] = np.concatenate([SIG0, RUN_SIGD0[list(sel)]]) ** 2
    Q = np.tile(np.diag(RUN_QSD ** 2), (B, 1, 1))
    Qd = np.full((B, 3), RUN_QD)
    out = dict(p=p, d=d, us=us, xs=np.array(xs), zs=np.array(zs), rs=np.array(rs), outl=outl, x0=x0, d0=d0, Pa0=Pa0, Q=Q, Qd=Qd)
    for a in out.values():
        a.setflags(write=False)
    return out


def run_filter(sel, step):
    """the filter over the run with step(x, d, Pa, u, z, r) -> (x, d, Pa, nis, counts)
    -> dict(x, d, Pa: the final ones; counts [n, B, 2]; xh [n, B, 13], dh [n, B, 6]: the estimates of every step; ev: RMS error of
    v_b after step 20)"""
    D = run_data(sel)
    x, d, Pa = D["x0"], D["d0"], D["Pa0"]
    counts, xh, dh = [], [], []
    for t in range(RUN_STEPS):
        x, d, Pa, _nis, cn = step(x, d, Pa, D["us"][t], D["zs"][t], D["rs"][t])
        counts.append(np.array(cn)); xh.append(np.array(x)); dh.append(np.array(d))
    xh, dh = np.array(xh), np.array(dh)
    ev = float(np.sqrt(np.mean(np.square(xh[20:, :, 7:10] - D["xs"][21:, :, 7:10]))))
    return dict(x=np.array(x), d=np.array(d), Pa=np.array(Pa), counts=np.array(counts), xh=xh, dh=dh, ev=ev)


@functools.lru_cache(maxsize=None)
def run_twin(sel):
    """the twin's run, computed once -> (run_filter's result, the gate ratios)"""
    D = run_data(sel)
    ratios = []
    out = run_filter(sel, lambda x, d, Pa, u, z, r: ekf_aug_ref(x, d, Pa, u, sel, p=D["p"], T=T, steps=1, Q=D["Q"], Qd=D["Qd"], z=z, r=r,
                                                              gate=RUN_GATE, normalize=True, ratios=ratios))
    return out, np.array([v for _i, _j, v in ratios])


def observer_rule(sel):
    """cfnmpc_estimate_disturbance's rule in numpy with both gains 1, run on the twin filter's own state estimates of the same
    data: x_prev = the filter's x of step t - 1, x_meas = its x of step t -> dh [n, B, 6]"""
    D = run_data(sel)
    tw, _ = run_twin(sel)
    k = sv.derive(D["p"].T)
    d = np.array(D["d0"])
    xprev, dh = D["x0"], []
    for t in range(RUN_STEPS):
        xhat = sv.rk4_step(xprev.T, D["us"][t].T, k, d.T, T).T
        e = tw["xh"][t] - xhat
        R = np.moveaxis(dc.rot(xprev[:, 3:7].T), -1, 0)      # [B, 3, 3]
        d = d.copy()
        d[:, 0:3] += np.einsum("bij,bj->bi", R, e[:, 7:10]) / T
        d[:, 3:6] += e[:, 10:13] / T
        dh.append(d)
        xprev = tw["xh"][t]
    return np.array(dh)


@pytest.mark.parametrize("sel", RUN_SELS, ids=str)
def test_closed_loop_run_is_consistent_and_beats_the_observer(sel):
    D = run_data(sel)
    tw, rt = run_twin(sel)
    assert not ((rt >= 0.9) & (rt <= 1.1)).any()          # (no decision at its threshold: the run is a fair referee for the GPU)
    idx = list(sel)
    e = tw["d"][:, idx] - D["d"][:, idx]
    Pdd = tw["Pa"][:, 13:, 13:]
    m = np.array([e[i] @ np.linalg.solve(Pdd[i], e[i]) for i in range(RUN_B)])
    # every outlier was rejected and nothing else
    rej = tw["counts"][:, :, 1]
    assert np.array_equal(rej > 0, D["outl"]) and (rej[D["outl"]] == 1).all()
    assert D["outl"].sum() == RUN_B * 8 and not any(t % 11 == 10 for t in range(RUN_STEPS) if t % 37 == 36)
    # the selected components against the one-step observer's rule on the same data
    ob = observer_rule(sel)
    rms_f = float(np.sqrt(np.mean(np.square(tw["dh"][-100:][:, :, idx] - D["d"][:, idx]))))
    rms_o = float(np.sqrt(np.mean(np.square(ob[-100:][:, :, idx] - D["d"][:, idx]))))
    print(f"sel {sel}: e' Pdd^-1 e = {np.round(m, 2)}, final |e| = {np.abs(e).max(axis=0)}, RMS error of d over the last 100 steps: "
          f"filter {rms_f:.4f}, observer rule {rms_o:.4f}; v_b RMS error {tw['ev']:.4f} m/s")
    assert (m <= CHI2_3_999).all()
    assert not tw["d"][:, [j for j in range(6) if j not in sel]].any()      # (no slot: left as they were)
    assert rms_f < rms_o


# ---- the host-compiled plain-loop step under the host sanitizers ------------------------------------------------------------
def test_ekf_aug_check_runs_clean_under_the_host_sanitizers(tmp_path):
    cases = []
    todo = [(51, 1, "d", "ten", 0.0, 1, True, (0, 1, 2)), (52, 3, "pd", "all", 0.0, 0, True, (3, 4, 5)),
            (53, 1, "pd", "flip", 0.0, 1, True, (2, 3, 4)), (21, 1, "pd", "mixed", GATE, 1, True, (0, 1, 2)),
            (54, 3, "pd", "pos", GATE, 1, False, (2, -1, -1)), (55, 3, "d", "ten", 0.0, 1, None, (-1, 5, 0)),
            (56, 1, "pd", "mixed", GATE, 1, True, (-1, -1, -1))]
    for seed, steps, rows, kind, gate, flags, with_q, sel in todo:      # with_q None: predict only
        B = 5
        c = case(seed, B, steps, rows, kind, sel, gate)
        a = case_args(c)
        if not with_q:
            a["Q"] = a["Qd"] = None
        if with_q is None:
            a["z"] = a["r"] = None
        x, d, Pa, nis, counts = ekf_aug_ref(c["x"], c["d"], c["Pa"], c["u"], sel, normalize=bool(flags), **a)
        p = np.tile(NOMINAL, (B, 1)) if c["p"] is None else c["p"]
        for i in range(B):
            parts = [p[i], c["d"][i], c["x"][i], c["Pa"][i], c["u"][i], c["Q"][i], c["Qd"][i], c["z"][i], c["r"][i], x[i], d[i], Pa[i],
                     [nis[i], counts[i, 0], counts[i, 1]]]
            cases.append(f"{steps} {T!r} {gate!r} {flags} {int(bool(with_q))} {int(bool(with_q))} {int(with_q is not None)} "
                         f"{sel[0]} {sel[1]} {sel[2]}\n" + "\n".join(" ".join(repr(float(v)) for v in np.ravel(q)) for q in parts))
    assert 30 <= len(cases) <= 40
    path = tmp_path / "cases.txt"
    path.write_text(f"{len(cases)}\n" + "\n".join(cases) + "\n")
    csrc = os.path.join(ROOT, "crazyflie_nmpc_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "-s", "ekf_aug_check", f"OBJDIR={tmp_path}", f"CASES={path}"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and f"ekf_aug_check ok: {len(cases)} cases" in r.stdout and "runtime error" not in r.stderr
    r = subprocess.run(["make", "-C", csrc, "-s", "ekf_aug_check", f"OBJDIR={tmp_path}"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ekf_aug_check ok: built-in checks" in r.stdout and "runtime error" not in r.stderr
