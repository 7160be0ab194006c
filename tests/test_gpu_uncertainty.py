"""GPU suite: uncertainty propagation and robust input-bound tightening (include/cfnmpc.h: cfnmpc_set_uncertainty,
cfnmpc_eval_uncertainty, cfnmpc_get_backoff, cfnmpc_get_uncertainty, cfnmpc_tighten_box).

The reference is the numpy recursion of tests/test_uncertainty_cpu.py (checked there against extended precision and the product
form), run on the engine's own blocks (cfnmpc_debug_get_linearisation) and gains (cfnmpc_debug_get_factor).  Iterates come from
a few kicked closed-loop steps, so that the blocks differ per row and stage."""
import ctypes as C

import numpy as np
import pytest

from test_uncertainty_cpu import random_cov, unc_ref

pytestmark = pytest.mark.gpu
DT = 0.015
EINVAL = -1
SHAPES = [(37, 5), (200, 50)]     # not a multiple of 4 or 64 and shorter than every checkpoint but one | the default horizon
TOL = 1e-9                        # the bound DESIGN.md section 5.14 holds the sibling sweep (k_sens_fwd) to for N <= 50
XTOL = 1e-8                       # against X_k Sigma_0 X_k' with the engine's own dx_k/dx0
U_MIN, U_MAX = 0.0, 22.0
GAMMA, MIN_WIDTH = 3.0, 0.1
KICK = 1.0                        # the bench's kick level (about 91 % of the rows unconstrained)
KICK_TIGHT = 1.0                  # test 4: the level at which >= 5 % of the rows sit at a tightened bound (see the test)


def _solver(B, N=50, **kw):
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    return BatchSolver(B, default_opts(N=N, **kw))


def _inputs(oracle, B, N, seed, scale):
    rng = np.random.default_rng(seed)
    x0 = oracle.sample_hover_x0(rng, B, scale=scale)
    kicks = oracle.sample_hover_x0(rng, B, scale=scale)
    yr, ye = oracle.regulation_yref(N, (0.0, 0.0, 0.4))
    return x0, kicks, np.repeat(yr[None], B, 0).copy(), np.repeat(ye[None], B, 0).copy()


def _loop(oracle, s, seed, scale=KICK, steps=10, every=20, configure=None):
    """a few closed-loop steps through the plant, one row in `every` kicked per step as in the bench's loop (steps = 3, every = 3:
    most rows freshly kicked); the last call is a solve.  -> the state that solve was given"""
    from crazyflie_nmpc_amd import sim
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    x, kicks, yr, ye = _inputs(oracle, s.B, s.N, seed, scale)
    s.set_yref(yr, ye)
    if configure:
        configure(s)
    s.set_x0(x)
    s.init_iterate(INIT_HOVER)
    for t in range(steps):
        s.set_x0(x)
        s.solve(1)
        if t == steps - 1:
            break
        x = sim(x, s.get_u(0), T=DT, steps=1)
        x[t::every] = kicks[t::every]
    return x


def _advance(s, x):
    from crazyflie_nmpc_amd import sim
    return sim(x, s.get_u(0), T=DT, steps=1)


def _step(s, x):
    """the next control step -> (x iterate, u iterate, status, qp_iter)"""
    s.set_x0(x)
    s.solve(1)
    xi, ui = s.get_iterate()
    st, it, _res = s.stats()
    return xi, ui, st, it


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def _cov(B, seed, w_scale=0.01):
    rng = np.random.default_rng(seed)
    S0 = random_cov(rng, B)
    return S0, w_scale * random_cov(rng, B)      # W = (0.1 std)^2


def _rel(a, ref):
    """per stage, relative to max(the stage's largest reference entry, 1e-12) -> the largest over the stages"""
    ax = tuple(range(1, a.ndim))
    return float((np.abs(a - ref).max(axis=ax) / np.maximum(np.abs(ref).max(axis=ax), 1e-12)).max())


def _tightened(beta, lb, ub, gamma=GAMMA, mw=MIN_WIDTH):
    """the documented rule in numpy -> (lb', ub', clamped)"""
    gb = gamma * beta
    cap = (1.0 - mw) * (ub - lb) / 2.0
    free = (lb != ub) & ~np.isnan(gb)
    cl = free & (gb > cap)
    t = np.where(free, np.where(cl, cap, gb), 0.0)
    return lb + t, ub - t, cl


def _check_against_numpy(s, K_user=None):
    """Sigma over [0, N + 1), std_x and beta against the numpy recursion on the engine's blocks -> the three maxima"""
    B, N = s.B, s.N
    A, Bm, _b = s.get_linearisation()
    K = s.get_factor()[0] if K_user is None else K_user
    status = s.stats()[0]
    S0, W = _cov(B, 5)
    s.set_uncertainty(S0, W)
    s.set_uncertainty_gain("riccati" if K_user is None else "user", K_user)
    s.eval_uncertainty()
    beta = s.backoff()
    Sig, sd = s.uncertainty(0, N + 1)
    worst = np.zeros(3)
    for i in range(B):
        if status[i] == 4:
            assert np.isnan(Sig[i]).all() and np.isnan(sd[i]).all() and np.isnan(beta[i]).all()
            continue
        rS, rb = unc_ref(A[i], Bm[i], K[i], S0[i], W[i])
        rsd = np.sqrt(np.diagonal(rS, axis1=1, axis2=2))
        worst = np.maximum(worst, [_rel(Sig[i], rS), _rel(sd[i], rsd), _rel(beta[i], rb)])
    return worst, (Sig, sd, beta)


# ---- 1. against numpy on the engine's own blocks -----------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", SHAPES)
def test_against_numpy_on_engine_blocks(oracle, B, N):
    s = _solver(B, N)
    _loop(oracle, s, 10 + N)
    K = s.get_factor()[0]
    assert np.abs(K[:, 0] - K[:, -1]).max() > 1e-3 and np.abs(K[0] - K[1]).max() > 1e-6   # gains differ per stage and row
    w_r, _ = _check_against_numpy(s)
    # a constant user gain per row: the row's first Riccati gain, perturbed
    rng = np.random.default_rng(3)
    Ku = K[:, 0] * (1.0 + 0.05 * rng.standard_normal((B, 4, 13)))
    w_u, _ = _check_against_numpy(s, Ku)
    print(f"B = {B}, N = {N}: Sigma / std_x / beta against numpy, per-stage relative: riccati {w_r}, user {w_u}")
    assert w_r.max() <= TOL and w_u.max() <= TOL, (w_r, w_u)
    s.close()


def test_against_numpy_with_disturbance_and_erk(oracle):
    """disturbance rows and erk_steps = 2 change the blocks only"""
    B, N = SHAPES[0]
    rng = np.random.default_rng(8)
    d = np.concatenate([rng.normal(0, 0.5, (B, 3)), rng.normal(0, 2.0, (B, 3))], axis=1)

    def configure(s):
        s.set_erk_steps(2)
        s.set_disturbance(d)
    s = _solver(B, N)
    _loop(oracle, s, 12, configure=configure)
    w, _ = _check_against_numpy(s)
    print(f"disturbance + erk_steps 2: {w}")
    assert w.max() <= TOL, w
    s.close()


@pytest.mark.parametrize("B,N", SHAPES)
def test_windows_are_slices_of_the_full_sweep(oracle, B, N):
    s = _solver(B, N)
    _loop(oracle, s, 14)
    S0, W = _cov(B, 6)
    s.set_uncertainty(S0, W)
    s.eval_uncertainty()
    Sig, sd = s.uncertainty(0, N + 1)
    for st, n in ((0, 1), (4, 1), (N, 1), (3, N - 2)):
        a, b = s.uncertainty(st, n)
        assert np.array_equal(a, Sig[:, st:st + n]) and np.array_equal(b, sd[:, st:st + n]), (st, n)
    a, b = s.uncertainty(2)                      # one stage, without the stage axis; one output only
    assert np.array_equal(a, Sig[:, 2]) and np.array_equal(b, sd[:, 2])
    assert s.uncertainty(2, want_std=False)[1] is None and np.array_equal(s.uncertainty(2, want_sigma=False)[1], sd[:, 2])
    # device outputs: the unchunked path
    import torch
    tS = torch.empty((B, N + 1, 13, 13), dtype=torch.float64, device="cuda")
    tb = torch.empty((B, N, 4), dtype=torch.float64, device="cuda")
    st_ = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert s._L.cfnmpc_get_uncertainty(s._h, 0, N + 1, C.c_void_p(tS.data_ptr()), None, 1, st_) == 0
    s.backoff(out=tb)
    torch.cuda.synchronize()
    assert np.array_equal(tS.cpu().numpy(), Sig) and np.array_equal(tb.cpu().numpy(), s.backoff())
    assert np.array_equal(Sig[:, 0], np.ascontiguousarray(S0))
    s.close()


# ---- 2. cross-check inside the engine ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", SHAPES)
def test_product_form_with_engine_sensitivities(oracle, B, N):
    s = _solver(B, N)
    _loop(oracle, s, 16)
    S0, _W = _cov(B, 7)
    s.set_uncertainty(S0, None)
    s.eval_uncertainty()
    s.eval_sens_x0()
    Sig, _ = s.uncertainty(0, N + 1, want_std=False)
    _, X = s.sens_x0(0, N + 1)
    free = ~(s.sens_active() != 0).any(axis=(1, 2)) & (s.stats()[0] != 4)
    assert free.mean() >= 0.75, free.mean()
    worst = 0.0
    for i in np.flatnonzero(free):
        ref = X[i] @ S0[i] @ X[i].transpose(0, 2, 1)
        worst = max(worst, _rel(Sig[i], ref))
    print(f"B = {B}, N = {N}: Sigma_k against X_k Sigma_0 X_k' on {int(free.sum())} unconstrained rows: {worst:.2e}")
    assert worst <= XTOL, worst
    s.close()


# ---- 3. zeros ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", SHAPES)
def test_zero_covariance_is_the_nominal_box(oracle, B, N):
    out = []
    for tighten in (True, False):
        s = _solver(B, N)
        x = _loop(oracle, s, 18)
        if tighten:
            s.set_uncertainty(None, None)
            s.eval_uncertainty()
            Sig, sd = s.uncertainty(0, N + 1)
            beta = s.backoff()
            assert not Sig.any() and not sd.any() and not beta.any()
            assert not s.tighten_box(GAMMA, MIN_WIDTH).any()
        x = _advance(s, x)
        if not tighten:
            s.set_box_stages(np.full((B, N, 4), U_MIN), np.full((B, N, 4), U_MAX))
        out.append(_step(s, x))
        s.close()
    assert _same(*out)


# ---- 4. tightening = explicit boxes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", SHAPES)
def test_tightening_equals_explicit_boxes(oracle, B, N):
    """KICK_TIGHT: with most rows freshly kicked (three steps, every third row kicked per step) the bench's kick level already
    puts 47 - 49 % of the status-0 rows at a tightened bound strictly inside the nominal box (measured, DESIGN.md section
    5.21), so the level was not raised"""
    S0, W = _cov(B, 9)
    out = []
    for explicit in (False, True):
        s = _solver(B, N)
        x = _loop(oracle, s, 20, scale=KICK_TIGHT, steps=3, every=3)
        s.set_uncertainty(S0, W)
        s.eval_uncertainty()
        beta = s.backoff()
        lbt, ubt, cl = _tightened(beta, np.full((B, N, 4), U_MIN), np.full((B, N, 4), U_MAX))
        if explicit:
            s.set_box_stages(lbt, ubt)
        else:
            ncl = s.tighten_box(GAMMA, MIN_WIDTH)
            assert not ncl.any() and not cl.any()    # 3 sigma against 6 kRPM of head-room: nothing clamps
        out.append(_step(s, _advance(s, x)))
        s.close()
    assert _same(*out)
    _xi, ui, st, _it = out[0]
    ok = st == 0
    b1 = beta[ok]
    print(f"B = {B}, N = {N}: 1-sigma backoffs {np.nanmin(b1):.3f} .. {np.nanmax(b1):.3f} kRPM")
    assert (ui[ok] >= lbt[ok] - 1e-9).all() and (ui[ok] <= ubt[ok] + 1e-9).all()
    moved = (lbt > U_MIN) & (ubt < U_MAX)
    at = moved & ((np.abs(ui - lbt) <= 1e-9) | (np.abs(ui - ubt) <= 1e-9))
    share = float(at[ok].any(axis=(1, 2)).mean())
    print(f"B = {B}, N = {N}, kicks x {KICK_TIGHT}: {share:.3f} of the status-0 rows have an input at a tightened bound")
    assert share >= 0.05, share


# ---- 5. the nominal box is kept ----------------------------------------------------------------------------------------------
def _tight_solver(oracle, B, N, seed=22, **kw):
    s = _solver(B, N, **kw)
    x = _loop(oracle, s, seed, scale=KICK_TIGHT, steps=3, every=3)
    S0, W = _cov(B, 9)
    s.set_uncertainty(S0, W)
    s.eval_uncertainty()
    return s, x


@pytest.mark.parametrize("B,N", SHAPES)
def test_nominal_box_is_kept(oracle, B, N):
    def run(action):
        s, x = _tight_solver(oracle, B, N)
        action(s)
        r = _step(s, _advance(s, x))
        s.close()
        return r
    once = run(lambda s: s.tighten_box(GAMMA, MIN_WIDTH))
    twice = run(lambda s: (s.tighten_box(GAMMA, MIN_WIDTH), s.tighten_box(GAMMA, MIN_WIDTH)))
    other = run(lambda s: (s.tighten_box(1.0, MIN_WIDTH), s.tighten_box(GAMMA, MIN_WIDTH)))
    assert _same(once, twice) and _same(once, other)          # every tightening starts from the nominal box
    scalar = run(lambda s: None)
    assert not _same(once, scalar)                            # (the tightened box does bind)
    assert _same(scalar, run(lambda s: (s.tighten_box(GAMMA, MIN_WIDTH), s.tighten_box(0.0, MIN_WIDTH))))
    assert _same(scalar, run(lambda s: (s.tighten_box(GAMMA, MIN_WIDTH), s.set_box(U_MIN, U_MAX))))
    assert _same(scalar, run(lambda s: (s.tighten_box(GAMMA, MIN_WIDTH), s.set_box_stages(None, None))))
    # a new set_box_stages replaces the nominal box; per-stage nominal boxes come back in place
    lb2, ub2 = np.full((B, N, 4), 1.0), np.full((B, N, 4), 21.0)
    ub2[:, 1::2] = 20.0

    def renewed(s):
        s.tighten_box(GAMMA, MIN_WIDTH)
        s.set_box_stages(lb2, ub2)
        s.tighten_box(GAMMA, MIN_WIDTH)

    def explicit(s):
        lbt, ubt, _ = _tightened(s.backoff(), lb2, ub2)
        s.set_box_stages(lbt, ubt)
    assert _same(run(renewed), run(explicit))
    nominal2 = run(lambda s: s.set_box_stages(lb2, ub2))
    assert _same(nominal2, run(lambda s: (renewed(s), s.tighten_box(0.0, 0.5))))
    assert _same(nominal2, run(lambda s: (renewed(s), s.set_box(U_MIN, U_MAX))))


# ---- 6. clamp and equalities -------------------------------------------------------------------------------------------------
def _dead_inputs(Bm):
    """[B][N][4]: the stage's column of B is exactly zero.  The rotor speeds enter the model only squared, so dPhi/du_a vanishes
    where the iterate's input a is 0 (an input the last solve left at the lower bound of the nominal box): the Riccati gain row
    of that input is then exactly zero, the linearised feedback does not use it and its backoff is 0"""
    return (Bm == 0.0).all(axis=2)


@pytest.mark.parametrize("gain", ["riccati", "user"])
@pytest.mark.parametrize("B,N", SHAPES)
def test_clamp_and_equalities(oracle, B, N, gain):
    """Sigma0 and W with std 10: every free entry whose input has any authority in the linearisation is clamped to exactly
    min_width of its nominal width, centred.  (W of the same size: with W = 0 the closed loop has contracted Sigma below the
    clamp by the late stages of N = 50.)  With a user gain that is every free entry; with the Riccati gains every free entry
    except those of _dead_inputs (measured at N = 50 in this loop: 3 of 39 200), which keep their nominal bounds."""
    S0 = random_cov(np.random.default_rng(4), B, std=(10.0,) * 13)
    lb, ub = np.full((B, N, 4), U_MIN), np.full((B, N, 4), U_MAX)
    out = []
    for explicit in (False, True):
        s = _solver(B, N)
        x = _loop(oracle, s, 24)
        lb[:, 0] = ub[:, 0] = s.get_u(1)           # stage 0 pinned (the input in flight)
        s.set_box_stages(lb, ub)
        x = _advance(s, x)
        s.set_x0(x); s.solve(1)
        s.set_uncertainty(S0, S0)
        if gain == "user":
            # one constant gain for every row (row 0's Riccati gain at stage 1; every input's row of it is of order 10)
            Ku = s.get_factor()[0][0, 1]
            assert np.abs(Ku).max(axis=1).min() > 1.0
            s.set_uncertainty_gain("user", np.repeat(Ku[None], B, 0))
            dead = np.zeros((B, N, 4), bool)
        else:
            dead = _dead_inputs(s.get_linearisation()[1])
        s.eval_uncertainty()
        beta = s.backoff()
        lbt, ubt, cl = _tightened(beta, lb, ub)
        if explicit:
            s.set_box_stages(lbt, ubt)
        else:
            ncl = s.tighten_box(GAMMA, MIN_WIDTH)
            print(f"B = {B}, N = {N}, {gain} gains: status after the pinned solve {np.bincount(s.stats()[0], minlength=5).tolist()}, "
                  f"smallest backoff of a live input {np.nanmin(beta[~dead]):.3g}, dead inputs {int(dead.sum())}, "
                  f"unclamped free entries {int((~cl[:, 1:]).sum())}")
            assert not np.isnan(beta).any()
            assert np.array_equal(cl[:, 1:], ~dead[:, 1:]) and not cl[:, 0].any()
            assert np.array_equal(ncl, (N - 1) * 4 - dead[:, 1:].sum(axis=(1, 2)))
        out.append(_step(s, _advance(s, x)))
        s.close()
    # every clamped entry: exactly min_width of the nominal width, centred; the pinned stage and the dead inputs keep their bounds
    w = ub - lb
    assert np.array_equal(lbt[:, 0], lb[:, 0]) and np.array_equal(ubt[:, 0], lb[:, 0])
    assert np.array_equal(lbt[dead], lb[dead]) and np.array_equal(ubt[dead], ub[dead])
    assert np.abs((ubt - lbt)[cl] - MIN_WIDTH * w[cl]).max() <= 1e-12
    assert np.abs((ubt + lbt)[cl] - (ub + lb)[cl]).max() <= 1e-12
    assert _same(*out)
    xi, ui, st, _it = out[0]
    assert (st != 4).all()
    assert np.abs(ui[:, 0] - lb[:, 0]).max() <= 1e-9
    assert (ui >= lbt - 1e-9).all() and (ui <= ubt + 1e-9).all()


@pytest.mark.parametrize("B,N", SHAPES)
def test_zero_backoff_only_without_input_authority(oracle, B, N):
    """Riccati gains, most rows freshly kicked: on every status-0 row the backoff is strictly positive, except -- exactly zero --
    where the stage's column of B is exactly zero (_dead_inputs); and the stored gains the sweep reads are numpy's Riccati gains
    on the same blocks (bound: the 1e-8 tests/test_gpu_sens.py::test_home_gains_against_numpy holds them to)."""
    s, _x = _tight_solver(oracle, B, N, seed=20)
    beta = s.backoff()
    A, Bm, _b = s.get_linearisation()
    K = s.get_factor()[0]
    ok = s.stats()[0] == 0
    dead = _dead_inputs(Bm)
    print(f"B = {B}, N = {N}: dead inputs {np.argwhere(dead).tolist()}, smallest live backoff {np.nanmin(beta[ok][~dead[ok]]):.3g}")
    assert ok.mean() >= 0.9
    assert np.array_equal(beta[ok] == 0.0, dead[ok]) and (beta[ok][~dead[ok]] > 0.0).all()
    if N == 50:
        assert dead[ok].any()                     # (this loop does leave an input at 0: the case is covered)
    W, WN = np.array(s.opts.W), np.array(s.opts.WN)
    worst = 0.0
    for i in np.flatnonzero(ok):
        P = np.diag(WN)
        for k in range(N - 1, -1, -1):
            Sm = np.diag(W[13:]) + Bm[i, k].T @ P @ Bm[i, k]
            Kt = np.linalg.solve(Sm, Bm[i, k].T @ P @ A[i, k])
            P = np.diag(W[:13]) + A[i, k].T @ P @ A[i, k] - A[i, k].T @ P @ Bm[i, k] @ Kt
            worst = max(worst, float(np.abs(K[i, k] - Kt).max() / max(1.0, np.abs(Kt).max())))
            assert not Kt[dead[i, k]].any()       # numpy's gain row of a dead input is exactly zero too
    print(f"B = {B}, N = {N}: stored gains against numpy's, every stage of {int(ok.sum())} rows: {worst:.2e}")
    assert worst <= 1e-8, worst
    s.close()


# ---- 7. refusals and validation ----------------------------------------------------------------------------------------------
def test_refusals_and_validation(oracle):
    B, N = 8, 20
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    s = _solver(B, N)
    L, h = s._L, s._h
    x, _k, yr, ye = _inputs(oracle, B, N, 1, 1.0)
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    s.set_yref(yr, ye); s.set_x0(x); s.init_iterate(INIT_HOVER)
    nc = np.zeros(B, dtype=np.int32)
    beta = np.empty((B, N, 4))
    assert L.cfnmpc_eval_uncertainty(h, None) == EINVAL                          # before any solve
    assert L.cfnmpc_tighten_box(h, 3.0, 0.1, p(nc), 0, None) == EINVAL           # without a backoff
    assert L.cfnmpc_get_backoff(h, p(beta), 0, None) == EINVAL
    s.solve(1)
    assert L.cfnmpc_tighten_box(h, 3.0, 0.1, p(nc), 0, None) == EINVAL           # before an evaluation
    S0, W = _cov(B, 2)
    s.set_uncertainty(S0, W)
    s.eval_uncertainty()
    b0 = s.backoff()
    S0_, _ = s.uncertainty(0)
    bad_sym = S0.copy(); bad_sym[3, 2, 5] *= 1.0 + 1e-9
    bad_nan = S0.copy(); bad_nan[1, 4, 4] = np.nan
    bad_inf = S0.copy(); bad_inf[1, 4, 6] = bad_inf[1, 6, 4] = np.inf
    bad_neg = S0.copy(); bad_neg[7] = 0.0; bad_neg[7, 2, 2] = -1e-9
    for bad in (bad_sym, bad_nan, bad_inf, bad_neg):
        assert L.cfnmpc_set_uncertainty(h, p(bad), p(W), 0, None) == EINVAL
        assert L.cfnmpc_set_uncertainty(h, p(S0), p(bad), 0, None) == EINVAL
    Kbad = np.zeros((B, 4, 13)); Kbad[2, 1, 3] = np.nan
    assert L.cfnmpc_set_uncertainty_gain(h, 1, p(Kbad), 0, None) == EINVAL
    assert L.cfnmpc_set_uncertainty_gain(h, 1, None, 0, None) == EINVAL
    assert L.cfnmpc_set_uncertainty_gain(h, 2, None, 0, None) == EINVAL
    for g, mw in ((-1.0, 0.1), (float("nan"), 0.1), (3.0, 0.0), (3.0, -0.1), (3.0, 1.5), (3.0, float("nan"))):
        assert L.cfnmpc_tighten_box(h, g, mw, p(nc), 0, None) == EINVAL
    Sg = np.empty((B, N + 1, 13, 13))
    assert L.cfnmpc_get_uncertainty(h, 0, 1, None, None, 0, None) == EINVAL
    assert L.cfnmpc_get_uncertainty(h, 0, N + 2, p(Sg), None, 0, None) == EINVAL
    assert L.cfnmpc_get_uncertainty(h, -1, 1, p(Sg), None, 0, None) == EINVAL
    # nothing changed: the same evaluation again gives the same bits
    s.eval_uncertainty()
    # new tables or another gain: the covariance getter waits for the next evaluation (it would sweep with the new inputs while
    # the stored backoff is the old evaluation's); the backoff stays
    for change in (lambda: s.set_uncertainty(S0, W), lambda: s.set_uncertainty_gain("riccati")):
        change()
        assert L.cfnmpc_get_uncertainty(h, 0, 1, p(Sg), None, 0, None) == EINVAL
        assert np.array_equal(s.backoff(), b0)
        s.eval_uncertainty()
    assert np.array_equal(s.backoff(), b0) and np.array_equal(s.uncertainty(0)[0], S0_)
    # a data change since the last solve: no evaluation, no covariance sweep -- the backoff stays (tighten_box may follow set_x0)
    s.set_x0(x)
    assert L.cfnmpc_eval_uncertainty(h, None) == EINVAL
    assert np.array_equal(s.backoff(), b0)
    assert L.cfnmpc_tighten_box(h, 3.0, 0.1, p(nc), 0, None) == 0
    assert L.cfnmpc_get_uncertainty(h, 0, 1, p(Sg), None, 0, None) == EINVAL     # (the box changed: not the last QP's data)
    s.solve(1)
    s.eval_uncertainty()
    s.set_weights(np.array(s.opts.W), np.array(s.opts.WN))
    assert L.cfnmpc_eval_uncertainty(h, None) == EINVAL
    xi, ui = s.get_iterate()
    s.set_iterate(xi, ui)                                                        # the backoff ends with the iterate
    assert L.cfnmpc_get_backoff(h, p(beta), 0, None) == EINVAL
    assert L.cfnmpc_tighten_box(h, 3.0, 0.1, p(nc), 0, None) == EINVAL
    s.close()
    for kw in (dict(cond_N2=5), dict(start_solve=2)):
        t = _solver(B, N, **kw)
        t.set_yref(yr, ye); t.set_x0(x); t.init_iterate(INIT_HOVER)
        t.solve(1)
        assert t._L.cfnmpc_eval_uncertainty(t._h, None) == EINVAL
        assert t._L.cfnmpc_tighten_box(t._h, 3.0, 0.1, None, 0, None) == EINVAL
        t.close()


@pytest.mark.parametrize("B,N", SHAPES)
def test_nan_row_keeps_its_nominal_box(oracle, B, N):
    outs = []
    for bad in (False, True):
        s = _solver(B, N)
        x = _loop(oracle, s, 26)
        x = _advance(s, x)
        if bad:
            x[5] = np.nan
        s.set_x0(x); s.solve(1)
        S0, W = _cov(B, 3)
        s.set_uncertainty(S0, W)
        s.eval_uncertainty()
        beta = s.backoff()
        Sig, sd = s.uncertainty(0, N + 1)
        dead = _dead_inputs(s.get_linearisation()[1])
        ncl = s.tighten_box(1e6, MIN_WIDTH)      # (everything clamps, where there is a backoff)
        outs.append((beta, Sig, sd, ncl, s.stats()[0], dead))
        s.close()
    (b0, S0_, d0, n0, _s0, dd0), (b1, S1, d1, n1, st1, _dd1) = outs
    assert st1[5] == 4 and np.isnan(b1[5]).all() and np.isnan(S1[5]).all() and np.isnan(d1[5]).all()
    assert n1[5] == 0 and np.array_equal(n0, N * 4 - dd0.sum(axis=(1, 2)))
    keep = np.arange(B) != 5
    assert np.array_equal(b0[keep], b1[keep]) and np.array_equal(S0_[keep], S1[keep]) and np.array_equal(n0[keep], n1[keep])
    # the box the failed row is left with: the next step (finite state again) is bitwise the step of a twin given the rule's boxes
    # explicitly, in which that row's are the nominal ones -- a tightened (clamped: a tenth of the width) box would bind
    res = []
    for explicit in (False, True):
        s = _solver(B, N)
        x = _advance(s, _loop(oracle, s, 26))
        xb = x.copy(); xb[5] = np.nan
        s.set_x0(xb); s.solve(1)
        s.set_uncertainty(*_cov(B, 3))
        s.eval_uncertainty()
        lbt, ubt, _cl = _tightened(s.backoff(), np.full((B, N, 4), U_MIN), np.full((B, N, 4), U_MAX), gamma=1e6)
        assert (lbt[5] == U_MIN).all() and (ubt[5] == U_MAX).all() and (ubt[6] - lbt[6] < 3.0).any()
        if explicit:
            s.set_box_stages(lbt, ubt)
        else:
            s.tighten_box(1e6, MIN_WIDTH)
        res.append(_step(s, x))
        s.close()
    assert _same(*res)


# ---- 8. row independence -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", SHAPES)
def test_rows_are_independent(oracle, B, N):
    """permuting the rows (states, covariances, user gains) permutes the outputs bit for bit -- on the rows whose blocks and gains
    the two solves left bitwise equal: a constrained row's QP solution depends in its last bits on the rows it shares a
    compacted wavefront with (they run their active-set solves in lock-step), and with it the next linearisation"""
    S0, W = _cov(B, 11)
    rng = np.random.default_rng(12)
    Ku = rng.standard_normal((B, 4, 13))
    perm = rng.permutation(B)
    x, _k, yr, ye = _inputs(oracle, B, N, 28, 2.0)
    outs, blocks = [], []
    for idx in (np.arange(B), perm):
        from crazyflie_nmpc_amd.solver import INIT_HOVER
        s = _solver(B, N)
        s.set_yref(yr, ye); s.set_x0(x[idx]); s.init_iterate(INIT_HOVER)
        s.solve(2)
        blocks.append(s.get_linearisation()[:2] + (s.get_factor()[0], s.stats()[0]))
        s.set_uncertainty(S0[idx], W[idx])
        res = ()
        for mode, K in (("riccati", None), ("user", Ku[idx])):
            s.set_uncertainty_gain(mode, K)
            s.eval_uncertainty()
            res += (s.backoff(),) + s.uncertainty(0, N + 1)
        res += (s.tighten_box(GAMMA, MIN_WIDTH),)
        outs.append(res)
        s.close()
    same = np.ones(B, bool)
    for a, b in zip(*blocks):
        same &= np.array([np.array_equal(a[perm][r], b[r]) for r in range(B)])
    print(f"B = {B}, N = {N}: rows with bitwise equal blocks, gains and status under the permutation: {int(same.sum())} of {B}")
    assert same.mean() >= 0.75, same.mean()
    for a, b in zip(*outs):
        assert np.array_equal(a[perm][same], b[same], equal_nan=True)


# ---- 9. fleet and multi ------------------------------------------------------------------------------------------------------
def _drive(o, x0, yr, ye, S0, W, sync=lambda: None):
    """solve(2), evaluate, tighten, one more step -> (beta, n_clamped, u0, status, qp_iter)"""
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    o.set_x0(x0); o.set_yref(yr, ye); o.init_iterate(INIT_HOVER)
    o.solve(2); sync()
    o.set_uncertainty(S0, W)
    o.eval_uncertainty()
    beta = o.backoff()
    ncl = o.tighten_box(GAMMA, MIN_WIDTH)
    o.set_x0(x0)
    o.solve(1); sync()
    st = o.stats()
    return beta, ncl, o.get_u(0), st[0], st[1]


def test_fleet_equals_its_buckets(oracle):
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    edges = (5, 8, 17, 33, 40)
    rng = np.random.default_rng(2027)
    hz = np.resize(np.array(edges), 26)[rng.permutation(26)].astype(np.int32)
    B, Nmax = hz.size, max(edges)
    x0, _k, yr, ye = _inputs(oracle, B, Nmax, 30, 2.0)
    S0, W = _cov(B, 13)
    f = MixedHorizonFleet(hz)
    fb, fn, fu, fs, fi = _drive(f, x0, yr, ye, S0, W)
    for i in range(B):
        assert np.isnan(fb[i, hz[i]:]).all() and not np.isnan(fb[i, :hz[i]]).any(), i
    # device arrays take the other path (per-bucket staging + scatter)
    import torch
    tb = torch.zeros((B, Nmax, 4), dtype=torch.float64, device="cuda")
    f.backoff(out=tb)
    torch.cuda.synchronize()
    assert np.array_equal(tb.cpu().numpy(), fb, equal_nan=True)
    f.eval_uncertainty()                         # (the tightening and the step ended the first evaluation)
    Sg, sd = f.uncertainty(0, f.Nmin + 1)
    assert np.array_equal(Sg[:, 0], S0)
    with pytest.raises(Exception):
        f.uncertainty(0, f.Nmin + 2)             # beyond the shortest horizon
    for N, idx in f.buckets():
        s = _solver(idx.size, N)
        sb, sn, su, ss, si = _drive(s, x0[idx], yr[idx, :N], ye[idx], S0[idx], W[idx])
        assert np.array_equal(sb, fb[idx, :N]) and np.array_equal(sn, fn[idx]), N
        assert np.array_equal(su, fu[idx]) and np.array_equal(ss, fs[idx]) and np.array_equal(si, fi[idx]), N
        s.close()
    f.close()


def test_multi_two_shards(oracle):
    from crazyflie_nmpc_amd import default_opts
    from crazyflie_nmpc_amd.parallel import MultiGpuFleet
    B, N = 74, 50
    x0, _k, yr, ye = _inputs(oracle, B, N, 32, 2.0)
    S0, W = _cov(B, 15)
    m = MultiGpuFleet(B, [0, 0], opts=default_opts())
    mb, mn, mu, ms, mi = _drive(m, x0, yr, ye, S0, W, sync=m.sync)
    assert not np.isnan(mb).any()
    for lo, hi, _dev in m.shards():
        s = _solver(hi - lo, N)
        r = slice(lo, hi)
        sb, sn, su, ss, si = _drive(s, x0[r], yr[r], ye[r], S0[r], W[r])
        assert np.array_equal(sb, mb[r]) and np.array_equal(sn, mn[r])
        assert np.array_equal(su, mu[r]) and np.array_equal(ss, ms[r]) and np.array_equal(si, mi[r])
        s.close()
    m.close()


def test_multi_horizons(oracle):
    from crazyflie_nmpc_amd.fleet import MixedHorizonFleet
    from crazyflie_nmpc_amd.parallel import MultiGpuFleet
    hz = np.random.default_rng(6).choice([5, 17, 40], 30).astype(np.int32)
    B, Nmax = len(hz), 40
    x0, _k, yr, ye = _inputs(oracle, B, Nmax, 34, 2.0)
    S0, W = _cov(B, 17)
    m = MultiGpuFleet(B, [0, 0], horizons=hz)
    mb, mn, mu, ms, mi = _drive(m, x0, yr, ye, S0, W, sync=m.sync)
    for i in range(B):
        assert np.isnan(mb[i, hz[i]:]).all() and not np.isnan(mb[i, :hz[i]]).any(), i
    seen = np.zeros(B, bool)
    for idx, _dev in m.shards():
        f = MixedHorizonFleet(hz[idx])
        Ns = int(hz[idx].max())
        fb, fn, fu, fs, fi = _drive(f, x0[idx], yr[idx, :Ns], ye[idx], S0[idx], W[idx])
        assert np.array_equal(fb, mb[idx, :Ns], equal_nan=True) and np.array_equal(fn, mn[idx])
        assert np.array_equal(fu, mu[idx]) and np.array_equal(fs, ms[idx]) and np.array_equal(fi, mi[idx])
        seen[idx] = True
        f.close()
    assert seen.all()
    m.close()


# ---- 10. no side effect ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("B,N", SHAPES)
def test_evaluation_alone_changes_nothing(oracle, B, N, graph):
    out = []
    for with_unc in (False, True):
        s = _solver(B, N, step_graph=graph)
        x = _loop(oracle, s, 36)
        if with_unc:
            S0, W = _cov(B, 19)
            before = s.get_linearisation() + (s.get_factor()[0],)
            s.set_uncertainty(S0, W)
            s.eval_uncertainty()
            s.backoff(); s.uncertainty(0, N + 1)
            assert _same(before, s.get_linearisation() + (s.get_factor()[0],))   # the stored blocks and gains are only read
        r = _step(s, _advance(s, x))
        out.append(r + _step(s, _advance(s, x)))
        s.close()
    assert _same(*out)


@pytest.mark.parametrize("B,N", SHAPES)
def test_tightened_values_replay_in_captured_graphs(oracle, B, N):
    """new tightened values over old ones are written in place: a solver with step_graph = 1 keeps replaying and equals the
    plain launches step for step"""
    out = []
    for graph in (0, 1):
        s, x = _tight_solver(oracle, B, N, step_graph=graph)
        res = ()
        for g in (GAMMA, 1.0, 2.0):
            s.tighten_box(g, MIN_WIDTH)
            x = _advance(s, x)
            res += _step(s, x)
            s.eval_uncertainty()
        out.append(res)
        s.close()
    assert _same(*out)
