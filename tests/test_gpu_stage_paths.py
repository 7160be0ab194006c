"""GPU tests of the two paths of the solver-less batched calls (csrc/cfnmpc_stage.hpp and staged_call):
sim, sim_rollout, sim_rollout_vjp, ekf_step, ekf_aug_step and estimate_disturbance give the same bits on numpy arrays -- staged
through the cached device scratch -- and on torch device tensors -- handed through --, for every combination of their optional
arrays; the numpy call leaves its inputs alone; caller-supplied outputs are written in place; the scratch serves calls of
different tables and sizes one after another; and a numpy sim with a wrongly shaped array raises before anything is written.

Shapes: the smallest at which staging can go wrong.  B in {1, 3, 257}: one lane; a partly filled group of the filter kernels' four
instances; one element past a block of 256 threads.  L in {1, 2} for the rollouts, steps in {1, 2}.  Nothing is compared against a
reference of the arithmetic (tests/test_gpu_sim_vjp.py, test_gpu_ekf.py, test_gpu_ekf_aug.py, test_gpu_disturbance.py do that):
every assertion here is bitwise equality of the two paths."""
import functools
import itertools

import numpy as np
import pytest

import test_ekf_aug_cpu as ea
import test_ekf_cpu as ec
import test_sim_vjp_cpu as sv
from test_ekf_cpu import SIG0, SIGZ

pytestmark = pytest.mark.gpu
T = 0.015
SEL = (4, -1, 0)          # two slots in use, out of order, and one unused
BS, STEPS, LS = [1, 3, 257], [1, 2], [1, 2]


@functools.lru_cache(maxsize=None)
def data(B):
    """valid inputs of every call for a batch of B (rollouts: L = 2, the calls take the first L inputs); never written to"""
    c = sv.draw(300 + B, B, 2)
    rng = np.random.default_rng(900 + B)
    D = dict(x=c["x0"], u=c["u"], p=c["p"], d=c["d"], gxs=c["gxs"], P=ec.random_cov(rng, B, SIG0), Q=ec.random_cov(rng, B, 0.02 * SIG0),
             Pa=ea.random_cov_aug(rng, B, SEL), Qd=(0.05 * rng.uniform(0.5, 2.0, (B, 3))) ** 2,
             z=c["x0"] + SIGZ * rng.uniform(-1.0, 1.0, (B, 13)),
             r=np.where(ec.mixed_masks(B), (SIGZ * rng.uniform(0.5, 2.0, (B, 13))) ** 2, -1.0),
             xm=c["x0"] + 0.01 * rng.uniform(-1.0, 1.0, (B, 13)))
    for a in D.values():
        a.setflags(write=False)
    return D


class Host:
    """the arrays of a numpy call: contiguous writable copies, remembered with a second copy to compare against afterwards"""
    def __init__(self):
        self.given = []

    def __call__(self, a):
        a = np.array(a, order="C")
        self.given.append((a, a.copy()))
        return a

    def fresh(self, a):
        return np.array(a, order="C")

    def new(self, shape, dtype=np.float64):
        return np.full(shape, 7, dtype=dtype)

    def unchanged(self):
        return all(np.array_equal(a, b) for a, b in self.given)


class Dev:
    """the arrays of a torch call: device copies"""
    def __call__(self, a):
        import torch
        return torch.as_tensor(np.array(a, order="C"), device="cuda")      # (a copy: the data is read-only)

    fresh = __call__

    def new(self, shape, dtype=np.float64):
        return self(np.full(shape, 7, dtype=dtype))


def _np(out):
    return tuple(a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy() for a in out)


def _opt(D, cv, on, name):
    return cv(D[name]) if name in on else None


# one function per call: (data, L, steps, the options in use, converter, caller-supplied outputs?) -> (outputs, what was passed as out)
def call_sim(D, L, steps, on, cv, own=False):
    from crazyflie_nmpc_amd import sim
    out = cv.new((len(D["x"]), 13)) if own else None
    return (sim(cv(D["x"]), cv(D["u"][:, 0]), T=T, steps=steps, out=out, params=_opt(D, cv, on, "p"), dist=_opt(D, cv, on, "d")),), (out,)


def call_rollout(D, L, steps, on, cv, own=False):
    from crazyflie_nmpc_amd import sim_rollout
    out = cv.new((len(D["x"]), L + 1, 13)) if own else None
    return (sim_rollout(cv(D["x"]), cv(D["u"][:, :L]), T=T, steps=steps, out=out, params=_opt(D, cv, on, "p"),
                        dist=_opt(D, cv, on, "d")),), (out,)


def call_vjp(D, L, steps, on, cv, own=False):
    from crazyflie_nmpc_amd import sim_rollout, sim_rollout_vjp
    B = len(D["x"])
    xs = sim_rollout(D["x"], np.ascontiguousarray(D["u"][:, :L]), T=T, steps=steps, params=D["p"] if "p" in on else None,
                     dist=D["d"] if "d" in on else None)
    out = (cv.new((B, 13)), cv.new((B, L, 4)), cv.new((B, 8)) if "p" in on else None, cv.new((B, 6)) if "d" in on else None) if own else None
    got = sim_rollout_vjp(cv(xs), cv(D["u"][:, :L]), cv(D["gxs"][:, :L + 1]), T=T, steps=steps, params=_opt(D, cv, on, "p"),
                          dist=_opt(D, cv, on, "d"), out=out)
    assert (got[2] is None) == ("p" not in on) and (got[3] is None) == ("d" not in on)
    return got, out or ()


def call_ekf(D, L, steps, on, cv, own=False):
    from crazyflie_nmpc_amd import ekf_step
    B = len(D["x"])
    out = (cv.new((B, 13)), cv.new((B, 13, 13)), cv.new((B,)), cv.new((B, 2), np.int32)) if own else None
    return ekf_step(cv(D["x"]), cv(D["P"]), cv(D["u"][:, 0]), z=_opt(D, cv, on, "z"), r=cv(D["r"]) if "z" in on else None,
                    Q=_opt(D, cv, on, "Q"), T=T, steps=steps, gate=0.0, params=_opt(D, cv, on, "p"), dist=_opt(D, cv, on, "d"),
                    out=out), out or ()


def call_aug(D, L, steps, on, cv, own=False):
    from crazyflie_nmpc_amd import ekf_aug_step
    B = len(D["x"])
    out = (cv.new((B, 13)), cv.new((B, 6)), cv.new((B, 16, 16)), cv.new((B,)), cv.new((B, 2), np.int32)) if own else None
    Pxx = cv.new((B, 13, 13)) if "Pxx" in on else None
    got = ekf_aug_step(cv(D["x"]), cv(D["d"]), cv(D["Pa"]), cv(D["u"][:, 0]), SEL, z=_opt(D, cv, on, "z"),
                       r=cv(D["r"]) if "z" in on else None, Q=_opt(D, cv, on, "Q"), Qd=_opt(D, cv, on, "Qd"), T=T, steps=steps, gate=0.0,
                       params=_opt(D, cv, on, "p"), out=out, Pxx_out=Pxx)
    return got + (Pxx,), out or ()


def call_observe(D, L, steps, on, cv, own=False):
    """(d is updated in place in every call: it does not go through the unchanged() list)"""
    from crazyflie_nmpc_amd import estimate_disturbance
    d = cv.fresh(D["d"])
    return (estimate_disturbance(cv(D["x"]), cv(D["u"][:, 0]), cv(D["xm"]), d, T=T, steps=steps, params=_opt(D, cv, on, "p")),), (d,)


CALLS = dict(sim=(call_sim, ("p", "d")), sim_rollout=(call_rollout, ("p", "d")), sim_rollout_vjp=(call_vjp, ("p", "d")),
             ekf_step=(call_ekf, ("p", "d", "Q", "z")), ekf_aug_step=(call_aug, ("p", "Q", "Qd", "z", "Pxx")),
             estimate_disturbance=(call_observe, ("p",)))


def _subsets(names):
    return [frozenset(s) for k in range(len(names) + 1) for s in itertools.combinations(names, k)]


def _same(a, b):
    assert len(a) == len(b)
    return all((p is None and q is None) or (p.dtype == q.dtype and np.array_equal(p, q, equal_nan=True)) for p, q in zip(a, b))


def _both(name, B, L, steps, on, own=False):
    """the call on numpy arrays and on device tensors -> (numpy results, device results as numpy); asserts on the way that the
    numpy call left its inputs alone and that caller-supplied outputs came back as the same objects"""
    fn = CALLS[name][0]
    h = Host()
    got_h, out_h = fn(data(B), L, steps, on, h, own)
    assert h.unchanged(), (name, sorted(on))
    got_d, out_d = fn(data(B), L, steps, on, Dev(), own)
    for got, out in ((got_h, out_h), (got_d, out_d)):
        assert all(o is None or o is g for g, o in zip(got, out)), (name, sorted(on))
    return _np(got_h), _np(got_d)


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("name", list(CALLS))
def test_numpy_and_device_calls_give_the_same_bits(name, B, steps):
    for L in (LS if "rollout" in name else [1]):
        for on in _subsets(CALLS[name][1]):
            a, b = _both(name, B, L, steps, on)
            assert _same(a, b), (name, B, L, steps, sorted(on))
            assert all(np.isfinite(p).all() for p in a if p is not None)
            if "ekf" in name:
                assert a[-2 if name == "ekf_aug_step" else -1].dtype == np.int32
                assert (a[3 if name == "ekf_aug_step" else 2] != 0).any() == ("z" in on)      # (the NIS: an update took place)


@pytest.mark.parametrize("name", list(CALLS))
def test_caller_outputs_are_written_in_place(name):
    B, L, steps, on = 3, 2, 2, frozenset(CALLS[name][1])
    base = _both(name, B, L, steps, on)[0]
    a, b = _both(name, B, L, steps, on, own=True)          # (asserts the identities)
    assert _same(a, base) and _same(b, base)


def test_scratch_serves_different_tables_one_after_another():
    """a large table, a small one, another large one, the small one again: the cached scratch grows, is reused without being
    freed, and every call's arrays lie where its own table puts them"""
    seq = [("ekf_aug_step", 257, 1), ("sim", 1, 1), ("sim_rollout_vjp", 257, 2), ("sim", 1, 1)]
    ref = [_both(name, B, L, 2, frozenset(CALLS[name][1]))[1] for name, B, L in seq]
    got = [CALLS[name][0](data(B), L, 2, frozenset(CALLS[name][1]), Host())[0] for name, B, L in seq]      # (back to back)
    for (name, B, L), g, r in zip(seq, got, ref):
        assert _same(_np(g), r), (name, B)


def test_numpy_sim_checks_its_shapes_before_anything_is_written():
    from crazyflie_nmpc_amd import sim
    D = data(3)
    x, u = np.array(D["x"]), np.array(D["u"][:, 0], order="C")
    for bad in (np.full((3, 12), 7.0), np.full((4, 13), 7.0), np.full((39,), 7.0), np.full((3, 13), 7.0, dtype=np.float32)):
        with pytest.raises(ValueError):
            sim(x, u, T=T, steps=1, out=bad)
        assert (bad == 7).all()
    out = np.full((3, 13), 7.0)
    for xa, ua in ((x[:, :12], u), (x, u[:, :3]), (x, np.array(D["u"][:, :2].reshape(3, 8)))):
        with pytest.raises(ValueError):
            sim(xa, ua, T=T, steps=1, out=out)
    assert (out == 7).all()
    assert sim(x, u, T=T, steps=1, out=out) is out and np.isfinite(out).all() and not (out == 7).all()
