"""Setter walks: a solver walked through a sequence of setter calls must equal a fresh solver set directly to the final state.

Shared by tests/test_setter_walk_cpu.py (the model, the coverage of the walk set and the referee conditions, no GPU) and
tests/test_gpu_setter_walk.py (the walks on the device).  No test functions here.

  InForce      a plain-Python model of what is in force on a solver, by the rules stated in include/cfnmpc.h alone: one method
               per setter, and what the getters must return.
  walk         (seed, N, B) -> a list of ops (name, arguments): at most 16 setter ops, with solve(1) calls, one read-only episode
               (eval_nlp, eval_sens_x0), one globalised solve_sqp(3) and at most one tightening episode in between.
  run / apply  the ops on a solver / the final state on a fresh solver, one call per feature in a fixed order.
  final_case   the exact QP of one RTI step of a row under a state (rk4_sens of tests/test_disturbance_cpu.py,
               oracle.qp_from_blocks / solve_qp_dense / solve_qp_refined, composed as het_ref_step and _ref_step compose them).

The values are drawn with the recipes the project has: random_params / hover (tests/test_model_params_cpu.py), the weight and box
draws of het_case (tests/test_heterogeneous_cpu.py), random_dist (tests/test_disturbance_cpu.py), random_cov
(tests/test_uncertainty_cpu.py), the window arguments of tests/test_gpu_yref_uniform.py, the tables of tests/golden/poly.npz."""
import os

import numpy as np

from test_disturbance_cpu import ND, random_dist, rk4_sens
from test_model_params_cpu import NOMINAL, hover, random_params
from test_uncertainty_cpu import random_cov

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.015
B_WALK = 67                      # two 64-instance groups, the second nearly empty; 17 row-group waves, the last partly filled
HORIZONS = (8, 40)               # the whole horizon inside the dense head | the shortest horizon forward_split = 1 accepts
MAX_SETTERS = 16
DEFAULT_BOX = (0.0, 22.0)
SQP_ITERS, SQP_TOL = 3, 1e-8
USS = 15.7777                    # the input reference of the windows (tests/test_gpu_yref_uniform.py)
N_CHECKED, ROW_SEED = 12, 7      # rows compared with the exact QP: 64 and 66 and ten seeded ones (tests/test_gpu_variants.py)
PERT_X, PERT_U = 0.002, 0.2      # the iterate of the final comparison: off x0 and off hover by N(0, .)
KICK = 1.0                       # m/s on the body velocity of two rows of three (het_case's level; every third row stays calm)
CALM = 0.1                       # scale of a calm row's offset from its reference (the others: 1, as in het_case)
# six seeds per horizon, fixed on the CPU by the conditions of tests/test_setter_walk_cpu.py
SEEDS = {8: (5, 30, 36, 75, 86, 129), 40: (23, 27, 35, 40, 99, 129)}

WRITERS = ("set_yref_uniform", "set_yref_varying", "set_yref_poly", "set_yref_windows")
SETTERS = ("set_weights", "set_weights_batch", "set_cost_scaling", "set_erk_steps", "set_model_params", "set_disturbance", "set_box",
           "set_box_stages") + WRITERS
EPISODES = ("solve", "read_only", "solve_sqp", "tighten")
FEATURES = ("weight rows", "cost scaling", "erk steps", "parameter rows", "disturbance rows", "stage boxes")


def poly_tables():
    g = np.load(os.path.join(ROOT, "tests", "golden", "poly.npz"))
    return [g[n + "_table"] for n in ("figure8", "takeoff", "figure8_takeoff_landing")]


def default_weights():
    from crazyflie_nmpc_amd import default_opts
    o = default_opts()
    return np.array(o.W[:]), np.array(o.WN[:])


def kind_of(op):
    name, a = op
    return "set_yref_" + a["kind"] if name == "set_yref" else name


def is_setter(op):
    """one of the at most 16 setter ops of a walk (a tightening episode counts as one)"""
    return kind_of(op) in SETTERS or op[0] == "tighten"


# ---- the model -------------------------------------------------------------------------------------------------------------------
class InForce:
    """What is in force on a solver of B instances and horizon N after the setters called so far (include/cfnmpc.h)."""

    def __init__(self, B, N, W=None, WN=None):
        self.B, self.N = B, N
        w, wn = default_weights() if W is None else (W, WN)
        self.W, self.WN = np.array(w, dtype=np.float64), np.array(wn, dtype=np.float64)   # uniform: opts or the last set_weights
        self.W_rows = self.WN_rows = None                                                 # per-instance rows, unscaled, or None
        self.scaling = (1.0, 1.0)
        self.erk = 1
        self.p = None
        self.d = None
        self.box = DEFAULT_BOX
        self.lb = self.ub = None
        self.tight = False
        self.base = None         # the last writer of every vehicle's references: (kind, arguments)
        self.poly = None         # set_yref_poly on top of it: (arguments, parameter rows in force at the call)

    # -- weights
    def set_weights(self, W=None, WN=None):
        """either part may be absent (unchanged); with rows in force each part given replaces that part in every row"""
        if W is not None:
            self.W = np.array(W, dtype=np.float64)
            if self.W_rows is not None:
                self.W_rows = np.tile(self.W, (self.B, 1))
        if WN is not None:
            self.WN = np.array(WN, dtype=np.float64)
            if self.WN_rows is not None:
                self.WN_rows = np.tile(self.WN, (self.B, 1))

    def set_weights_batch(self, W=None, WN=None):
        """None, None: back to the uniform weights; one None: that part keeps what every row has (the uniform values if no rows)"""
        if W is None and WN is None:
            self.W_rows = self.WN_rows = None
            return
        had = self.W_rows is not None
        self.W_rows = np.array(W, dtype=np.float64) if W is not None else (self.W_rows if had else np.tile(self.W, (self.B, 1)))
        self.WN_rows = np.array(WN, dtype=np.float64) if WN is not None else (self.WN_rows if had else np.tile(self.WN, (self.B, 1)))

    def set_cost_scaling(self, stage, terminal):
        self.scaling = (float(stage), float(terminal))

    def set_erk_steps(self, n):
        assert n in (1, 2, 3)
        self.erk = int(n)

    # -- model
    def set_model_params(self, p=None):
        self.p = None if p is None else np.array(p, dtype=np.float64)

    def set_disturbance(self, d=None):
        """host arrays or device tensors"""
        if d is not None and not isinstance(d, np.ndarray):
            d = d.cpu().numpy()
        self.d = None if d is None else np.array(d, dtype=np.float64)

    # -- boxes
    def set_box(self, u_min, u_max):
        """the scalar box; per-stage boxes stay in force until set_box_stages(None, None); a tightened box gives way to the nominal"""
        self.box = (float(u_min), float(u_max))
        self.tight = False

    def set_box_stages(self, lb=None, ub=None):
        assert (lb is None) == (ub is None)
        self.lb = None if lb is None else np.array(lb, dtype=np.float64)
        self.ub = None if ub is None else np.array(ub, dtype=np.float64)
        self.tight = False

    def tighten_box(self, gamma):
        self.tight = gamma > 0.0

    # -- references
    def set_yref(self, yref, yref_e):
        uniform = bool((yref == yref[:, :1]).all())
        self.base = ("uniform" if uniform else "varying", dict(yref=np.array(yref), yref_e=np.array(yref_e)))
        self.poly = None

    def set_yref_windows(self, traj, mode, it, des, uss):
        """mode 0: regulation rows around des; mode 1: rows it .. it + N of traj (this model takes no window that ends the track)"""
        assert ((mode == 0) | (mode == 1)).all() and (it[mode == 1] < traj.shape[0] - self.N).all()
        self.base = ("windows", dict(traj=np.array(traj), mode=np.array(mode), it=np.array(it), des=np.array(des), uss=float(uss)))
        self.poly = None

    def set_yref_poly(self, traj, place, t, flags):
        """vehicles with id -1 keep what they have; the rows of the others follow the parameter rows in force now"""
        assert self.base is not None
        self.poly = (dict(traj=np.array(traj), place=np.array(place), t=float(t), flags=int(flags)), None if self.p is None else self.p.copy())

    # -- what the getters return
    def weights_batch(self):
        if self.W_rows is None:
            return np.tile(self.W, (self.B, 1)), np.tile(self.WN, (self.B, 1))
        return self.W_rows.copy(), self.WN_rows.copy()

    def model_params(self):
        return np.tile(NOMINAL, (self.B, 1)) if self.p is None else self.p.copy()

    def disturbance(self):
        return np.zeros((self.B, ND)) if self.d is None else self.d.copy()

    def yref(self):
        """-> (yref, yref_e, exact [B]): exact rows are copies of what a setter was given; the others are the polynomial rows of
        the host twin trajectories.poly_rows, which the device follows to 1e-11 (tests/test_gpu_poly.py: TOL)"""
        B, N = self.B, self.N
        kind, a = self.base
        if kind == "windows":
            y = np.zeros((B, N + 1, 17))
            y[:, :, :3] = a["des"][:, None, :]
            y[:, :, 3] = 1.0
            y[:, :, 13:] = a["uss"]
            for i in np.flatnonzero(a["mode"] == 1):
                y[i] = a["traj"][a["it"][i]:a["it"][i] + N + 1]
            y, ye = y[:, :N].copy(), y[:, N, :13].copy()
        else:
            y, ye = a["yref"].copy(), a["yref_e"].copy()
        exact = np.ones(B, dtype=bool)
        if self.poly is not None:
            from crazyflie_nmpc_amd import trajectories as tj
            pa, par = self.poly
            _flat, rows = tj.poly_rows(poly_tables(), pa["traj"], pa["place"], pa["t"], N + 1, DT, pa["flags"], par)
            on = pa["traj"] >= 0
            y[on], ye[on] = rows[on, :N], rows[on, N, :13]
            exact = ~on
        return y, ye, exact

    def poly_follows_params(self):
        """the polynomial rows in force were written under the parameter rows in force now (apply() can then write them again)"""
        if self.poly is None:
            return True
        par = self.poly[1]
        return (par is None and self.p is None) or (par is not None and self.p is not None and np.array_equal(par, self.p))

    def features(self):
        return {"weight rows": self.W_rows is not None, "cost scaling": self.scaling != (1.0, 1.0), "erk steps": self.erk != 1,
                "parameter rows": self.p is not None, "disturbance rows": self.d is not None, "stage boxes": self.lb is not None}

    def writer(self):
        return "poly" if self.poly is not None else self.base[0]

    def bounds(self):
        """-> lb, ub [B][N][4] of the nominal box in force"""
        if self.lb is not None:
            return self.lb.copy(), self.ub.copy()
        return np.full((self.B, self.N, 4), self.box[0]), np.full((self.B, self.N, 4), self.box[1])

    def apply_op(self, op):
        name, a = op
        if name == "set_yref":
            self.set_yref(a["yref"], a["yref_e"])
        elif name == "tighten":
            self.tighten_box(a["gamma"])
        elif name in SETTERS:
            getattr(self, name)(**a)
        else:
            assert name in EPISODES, name


def replay(ops, B, N):
    """the model after the ops of a walk"""
    m = InForce(B, N)
    for op in ops:
        m.apply_op(op)
    return m


# ---- the walks -------------------------------------------------------------------------------------------------------------------
def _weight_rows(rng, B):
    W, WN = default_weights()
    return (W * np.exp(rng.uniform(np.log(0.25), np.log(4.0), (B, 17))), WN * np.exp(rng.uniform(np.log(0.25), np.log(4.0), (B, 13))))


def _stage_box(rng, B, N):
    return dict(lb=rng.uniform(0.0, 4.0, (B, N, 4)), ub=rng.uniform(19.0, 22.0, (B, N, 4)))


def _regulation(rng, B, N, varying):
    """a setpoint per vehicle near (0, 0, 0.4), the input reference at the nominal hover speed; varying: a ramp over the stages"""
    y = np.zeros((B, N, 17))
    y[:, :, :3] = (np.array([0.0, 0.0, 0.4]) + rng.uniform(-0.1, 0.1, (B, 3)))[:, None, :]
    y[:, :, 3] = 1.0
    y[:, :, 13:] = hover(NOMINAL)
    ye = y[:, 0, :13].copy()
    if varying:
        y[:, :, :3] += np.linspace(0.0, 0.1, N)[None, :, None]
    return dict(yref=y, yref_e=ye, kind="varying" if varying else "uniform")


def _windows(rng, B, N):
    """a tracking window per vehicle out of one circular trajectory, every fourth vehicle in regulation"""
    n_rows = 3 * N + 8
    ph = np.linspace(0.0, 2 * np.pi, n_rows)
    traj = np.zeros((n_rows, 17))
    traj[:, 0], traj[:, 1], traj[:, 2] = 0.2 * np.cos(ph), 0.2 * np.sin(ph), 0.4 + 0.05 * np.sin(2 * ph)
    traj[:, 3] = 1.0
    traj[:, 13:] = USS
    mode = np.ones(B, dtype=np.int32)
    mode[::4] = 0
    it = rng.integers(0, n_rows - N - 2, B).astype(np.int32)
    des = np.array([0.0, 0.0, 0.4]) + rng.uniform(-0.1, 0.1, (B, 3))
    return dict(traj=traj, mode=mode, it=it, des=des, uss=USS)


def _poly(rng, B):
    """a trajectory per vehicle, every fifth without one; unit time scale, small offsets around (0, 0, 0.4)"""
    traj = rng.integers(0, 3, B).astype(np.int32)
    traj[::5] = -1
    place = np.zeros((B, 6))
    place[:, 0] = rng.uniform(-0.5, 0.5, B)
    place[:, 1] = 1.0
    place[:, 2:4] = rng.uniform(-0.2, 0.2, (B, 2))
    place[:, 4] = rng.uniform(0.0, 0.4, B)
    place[:, 5] = rng.uniform(-np.pi, np.pi, B)
    return dict(traj=traj, place=place, t=float(rng.uniform(0.5, 3.0)), flags=int(rng.integers(0, 2)))


def _writer(rng, B, N, kind):
    if kind == "set_yref_poly":
        return ("set_yref_poly", _poly(rng, B))
    if kind == "set_yref_windows":
        return ("set_yref_windows", _windows(rng, B, N))
    return ("set_yref", _regulation(rng, B, N, kind == "set_yref_varying"))


def _family_model(rng, B):
    P = lambda: ("set_model_params", dict(p=random_params(rng, B)))   # noqa: E731
    D = lambda: ("set_disturbance", dict(d=random_dist(rng, B)))      # noqa: E731
    P0, D0 = ("set_model_params", dict(p=None)), ("set_disturbance", dict(d=None))
    return [[P(), D(), P0, D0], [P(), P0, D()], [D(), P(), D0], [D(), D(), P(), P()], [P(), D(), D0, P0, D()]][int(rng.integers(5))]


def _family_weights(rng, B):
    W, WN = default_weights()
    f = lambda n: np.exp(rng.uniform(np.log(0.25), np.log(4.0), n))   # noqa: E731
    R = lambda: ("set_weights_batch", dict(zip(("W", "WN"), _weight_rows(rng, B))))   # noqa: E731
    RW = lambda: ("set_weights_batch", dict(W=_weight_rows(rng, B)[0], WN=None))      # noqa: E731
    RN = lambda: ("set_weights_batch", dict(W=None, WN=_weight_rows(rng, B)[1]))      # noqa: E731
    R0 = ("set_weights_batch", dict(W=None, WN=None))
    SW = lambda k: ("set_weights", dict(W=W * f(17) if k != 2 else None, WN=WN * f(13) if k != 1 else None))   # noqa: E731
    CS = lambda: ("set_cost_scaling", dict(zip(("stage", "terminal"), [(2.0, 0.5), (0.5, 2.0), (4.0, 1.0), (1.0, 3.0)][int(rng.integers(4))])))   # noqa: E731
    k = int(rng.integers(3))
    return [[R(), SW(k), CS()], [R(), R0, RN()], [SW(0), RW(), SW(2), CS()], [CS(), RN(), SW(1), R0], [R(), CS(), R0, CS()]][int(rng.integers(5))]


def _family_box(rng, B, N):
    S = lambda: ("set_box_stages", _stage_box(rng, B, N))   # noqa: E731
    S0 = ("set_box_stages", dict(lb=None, ub=None))
    BX = lambda: ("set_box", dict(zip(("u_min", "u_max"), [(1.0, 21.0), (0.5, 21.5), (2.0, 20.0)][int(rng.integers(3))])))   # noqa: E731
    T = lambda: ("tighten", dict(S0=random_cov(rng, B), W=0.01 * random_cov(rng, B), gamma=3.0, min_width=0.1))   # noqa: E731
    back = [BX, lambda: S0, S][int(rng.integers(3))]
    return [[S(), BX(), S()], [S(), S0], [T(), back()], [S(), T(), back()], [BX(), S(), S0]][int(rng.integers(5))]


def _family_erk(rng):
    E = lambda n: ("set_erk_steps", dict(n=n))   # noqa: E731
    return [[E(2), E(1)], [E(2)], [E(3), E(2)], [E(3), E(1), E(2)], []][int(rng.integers(5))]


def walk(seed, N, B=B_WALK):
    """-> the ops of walk (seed, N): the families' op sequences merged at random (each keeps its own order); the first op is a
    writer of every vehicle's references.  Two solve(1) follow each other behind the first one to three setter ops, later ones
    come singly behind most setter ops, one always in front of a tightening episode and one at the end."""
    rng = np.random.default_rng([seed, N])
    kinds = list(rng.permutation(4)[:3])
    if WRITERS[kinds[0]] == "set_yref_poly":           # (polynomial rows leave vehicles without a trajectory alone: never first)
        kinds[0], kinds[1] = kinds[1], kinds[0]
    fams = [[_writer(rng, B, N, WRITERS[k]) for k in kinds], _family_model(rng, B), _family_weights(rng, B), _family_box(rng, B, N),
            _family_erk(rng)]
    first, fams[0] = fams[0][0], fams[0][1:]
    order = np.concatenate([np.full(len(f), j) for j, f in enumerate(fams)])
    order = order[rng.permutation(order.size)][:MAX_SETTERS - 2]
    taken = [0] * len(fams)
    setters = [first]
    for j in order:
        setters.append(fams[j][taken[j]])
        taken[j] += 1
    if replay(setters, B, N).tight:                    # a tightening episode cut off from its way back by the cap
        setters.append(("set_box_stages", dict(lb=None, ub=None)))
    n_first = int(rng.integers(1, 4))
    ops, n_solves = [], 0
    i_read, i_sqp = int(rng.integers(2, 7)), int(rng.integers(2, len(setters)))
    for j, s in enumerate(setters):
        if s[0] == "tighten" and (not ops or ops[-1][0] != "solve"):
            ops.append(("solve", {})); n_solves += 1
        ops.append(s)
        if j + 1 < n_first:
            continue
        if j + 1 == n_first:
            ops += [("solve", {}), ("solve", {})]; n_solves += 2
        elif rng.uniform() < 0.85 or s[0] == "tighten" or j + 1 == len(setters):
            ops.append(("solve", {})); n_solves += 1
        if ops[-1][0] == "solve" and i_read is not None and n_solves >= i_read:
            ops.append(("read_only", {})); i_read = None
        if j + 1 == i_sqp:
            ops += [("solve_sqp", {}), ("solve", {})]; n_solves += 1
    if i_read is not None:
        ops.append(("read_only", {}))
    return ops


def start_state(oracle, seed, N, B=B_WALK):
    """x0 of the walk's own solves: hover-centred with N(0, 1) m/s on the body velocity (het_case)"""
    rng = np.random.default_rng([seed, N, 1])
    x0 = oracle.sample_hover_x0(rng, B, scale=1.0)
    x0[:, 7:10] += rng.normal(0, 1.0, (B, 3))
    return x0


# ---- transitions and coverage ----------------------------------------------------------------------------------------------------
def _token(op):
    """(family, token) of a setter op"""
    name, a = op
    if name == "set_model_params":
        return "model", "P" if a["p"] is not None else "P0"
    if name == "set_disturbance":
        return "model", "D" if a["d"] is not None else "D0"
    if name == "set_weights_batch":
        return "weights", "R00" if a["W"] is None and a["WN"] is None else ("R0N" if a["W"] is None else "R")
    if name == "set_weights":
        return "weights", "SW"
    if name == "set_cost_scaling":
        return "weights", "CS"
    if name == "set_box":
        return "box", "BX"
    if name == "set_box_stages":
        return "box", "S" if a["lb"] is not None else "S0"
    if name == "tighten":
        return "box", "T"
    if name == "set_erk_steps":
        return "erk", "E%d" % a["n"]
    return "ref", {"set_yref_uniform": "yu", "set_yref_varying": "yv", "set_yref_poly": "yp", "set_yref_windows": "yw"}[kind_of(op)]


CHAINS = {"params > dist > params(None) > dist(None)": ("model", ["P", "D", "P0", "D0"]),
          "params > params(None) > dist": ("model", ["P", "P0", "D"]),
          "dist > params > dist(None)": ("model", ["D", "P", "D0"]),
          "rows > set_weights > set_cost_scaling": ("weights", ["R", "SW", "CS"]),
          "rows > batch(None, None) > batch(None, WN)": ("weights", ["R", "R00", "R0N"]),
          "stages > set_box > stages": ("box", ["S", "BX", "S"]),
          "stages > stages(None, None)": ("box", ["S", "S0"]),
          "tighten > set_box": ("box", ["T", "BX"]),
          "tighten > stages(None, None)": ("box", ["T", "S0"]),
          "tighten > stages": ("box", ["T", "S"]),
          "erk 1 > 2 > 1": ("erk", ["E1", "E2", "E1"])}
CHAINS.update({f"{a} > {b}": ("ref", [a, b]) for a in ("yu", "yv", "yp", "yw") for b in ("yu", "yv", "yp", "yw") if a != b})


def transitions(ops, B, N):
    """the chains of CHAINS a walk contains: consecutive ops of one family, with a solve(1) in front of the first (behind the
    family's previous op), between every two and behind the last"""
    solves = [i for i, op in enumerate(ops) if op[0] == "solve"]
    between = lambda lo, hi: any(lo < s < hi for s in solves)   # noqa: E731
    seqs = {"erk": [("E1", -1)]}                                # (a new solver runs one RK4 step per interval)
    m = InForce(B, N)
    for i, op in enumerate(ops):
        if is_setter(op):
            fam, tok = _token(op)
            if tok == "SW" and m.W_rows is None:
                tok = "SW-"                                     # (set_weights without rows in force is not the special case)
            seqs.setdefault(fam, []).append((tok, i))
        m.apply_op(op)
    hit = set()
    for name, (fam, chain) in CHAINS.items():
        seq = seqs.get(fam, [])
        for j in range(len(seq) - len(chain) + 1):
            part = seq[j:j + len(chain)]
            if [t for t, _ in part] != chain:
                continue
            pos = [i for _, i in part]
            lo = seq[j - 1][1] if j > 0 else -1
            ok = (pos[0] < 0 or between(lo, pos[0])) and all(between(a, b) for a, b in zip(pos[:-1], pos[1:])) and between(pos[-1], len(ops))
            if ok:
                hit.add(name)
    return hit


def walk_set():
    """-> [(N, seed)]: the twelve walks"""
    return [(N, seed) for N in HORIZONS for seed in SEEDS[N]]


def widest_walks(N, n=2):
    """the n walks of horizon N that contain the most chains of CHAINS (ties: the smaller seed)"""
    count = {seed: len(transitions(walk(seed, N), B_WALK, N)) for seed in SEEDS[N]}
    return sorted(SEEDS[N], key=lambda seed: (-count[seed], seed))[:n]


def checked_rows(B=B_WALK):
    rest = np.random.default_rng(ROW_SEED).choice(64, N_CHECKED - 2, replace=False)
    return sorted(rest.tolist()) + [64, 66]


# ---- the ops on a solver ---------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _windows_call(s, a):
    s.set_yref_windows(_dev(a["traj"]), _dev(a["mode"]), _dev(a["it"]), _dev(a["des"]), a["uss"])


def _poly_call(s, a):
    if not getattr(s, "_walk_library", False):
        s.set_poly_library(poly_tables())
        s._walk_library = True
    s.set_poly_assignment(a["traj"], a["place"])
    s.set_yref_poly(a["t"], a["flags"])


def run(s, ops, log=None, after=None):
    """the ops of a walk on a solver that has x0 and an iterate; disturbance rows go alternately as host arrays and as device
    tensors; after(model, index, op) is called behind every setter op.  -> the model after the walk"""
    m = InForce(s.B, s.N)
    n_dist = 0
    for j, op in enumerate(ops):
        name, a = op
        if name == "solve":
            s.solve(1)
        elif name == "read_only":
            s.eval_nlp()
            s.eval_sens_x0()
            s.nlp_stats(); s.sens_x0(0); s.sens_active()
        elif name == "solve_sqp":
            s.set_sqp_globalization("merit_backtracking")
            s.solve_sqp(SQP_ITERS, SQP_TOL, SQP_TOL, SQP_TOL)
        elif name == "tighten":
            s.set_uncertainty(a["S0"], a["W"])
            s.eval_uncertainty()
            s.tighten_box(a["gamma"], a["min_width"])
        elif name == "set_yref":
            s.set_yref(a["yref"], a["yref_e"])
        elif name == "set_yref_windows":
            _windows_call(s, a)
        elif name == "set_yref_poly":
            _poly_call(s, a)
        elif name == "set_disturbance":
            d = a["d"]
            if d is not None:
                n_dist += 1
                d = _dev(d) if n_dist % 2 == 0 else d
            s.set_disturbance(d)
        else:
            getattr(s, name)(**a)
        m.apply_op(op)
        if log is not None:
            log.append(kind_of(op))
        if after is not None and is_setter(op):
            after(m, j, op)
    return m


def apply(s, m):
    """the state m on a fresh solver: one call per feature in a fixed order, no call for a feature that is off"""
    W0, WN0 = default_weights()
    if m.erk != 1:
        s.set_erk_steps(m.erk)
    if m.p is not None:
        s.set_model_params(m.p)
    if m.d is not None:
        s.set_disturbance(m.d)
    if not (np.array_equal(m.W, W0) and np.array_equal(m.WN, WN0)):
        s.set_weights(m.W, m.WN)
    if m.W_rows is not None:
        s.set_weights_batch(m.W_rows, m.WN_rows)
    if m.scaling != (1.0, 1.0):
        s.set_cost_scaling(*m.scaling)
    if m.box != DEFAULT_BOX:
        s.set_box(*m.box)
    if m.lb is not None:
        s.set_box_stages(m.lb, m.ub)
    kind, a = m.base
    if kind == "windows":
        _windows_call(s, a)
    else:
        s.set_yref(a["yref"], a["yref_e"])
    if m.poly is not None:
        assert m.poly_follows_params()
        _poly_call(s, m.poly[0])


# ---- the final comparison: inputs and the exact QP -------------------------------------------------------------------------------
def final_inputs(oracle, m, seed):
    """x0 and a kicked, perturbed iterate for the comparison behind a walk: each vehicle around the first row of its reference
    (oracle.sample_hover_x0), two rows of three at scale 1 with KICK on the body velocity, every third row calm (scale CALM, no
    kick: rows whose step no bound touches); the iterate off x0 by N(0, PERT_X) (quaternions normalised) and off hover by
    N(0, PERT_U), inside the box -> x0, x, u, yref, yref_e"""
    B, N = m.B, m.N
    rng = np.random.default_rng([seed, N, 2])
    y, ye, _exact = m.yref()
    x0 = oracle.sample_hover_x0(rng, B, center=(0.0, 0.0, 0.0), scale=1.0)
    x0[::3] = oracle.sample_hover_x0(rng, x0[::3].shape[0], center=(0.0, 0.0, 0.0), scale=CALM)
    x0[:, :3] += y[:, 0, :3]
    kick = rng.normal(0, KICK, (B, 3))
    kick[::3] = 0.0
    x0[:, 7:10] += kick
    x = np.repeat(x0[:, None, :], N + 1, 1) + rng.normal(0, PERT_X, (B, N + 1, 13))
    x[:, :, 3:7] /= np.linalg.norm(x[:, :, 3:7], axis=2, keepdims=True)
    lb, ub = m.bounds()
    u = np.clip(hover(m.model_params())[:, None, None] + rng.normal(0, PERT_U, (B, N, 4)), lb, ub)
    return x0, x, u, y, ye


def final_case(oracle, m, x0, x, u, yref, yref_e):
    """the exact QP of one RTI step of ONE row under the state m (x0 [13], x [N + 1][13], u [N][4], yref [N][17], yref_e [13] and
    the row's own data in m: a dict p, d, Qd, Rd, QNd, lb, ub, M)
    -> (x + dx, u + du of oracle.solve_qp_dense, qp, oracle.solve_qp_refined(qp): the referee)"""
    N = u.shape[0]
    A = np.empty((N, 13, 13)); Bm = np.empty((N, 13, 4)); b = np.empty((N, 13))
    for k in range(N):
        phi, A[k], Bm[k] = rk4_sens(x[k], u[k], m["p"], m["d"], DT, m["M"])
        b[k] = phi - x[k + 1]
    Qd, Rd, QNd = m["Qd"], m["Rd"], m["QNd"]
    q = np.empty((N + 1, 13))
    q[:-1] = Qd * (x[:-1] - yref[:, :13])
    q[-1] = QNd * (x[-1] - yref_e)
    r = Rd * (u - yref[:, 13:])
    qp = oracle.qp_from_blocks(A, Bm, b, q, r, x0 - x[0], Qd, Rd, QNd, m["lb"] - u, m["ub"] - u)
    sol = oracle.solve_qp_dense(qp)
    return x + sol["dx"], u + sol["du"], qp, oracle.solve_qp_refined(qp)


def row_data(m, i):
    """the data of row i under the state m, for final_case"""
    W, WN = m.weights_batch()
    lb, ub = m.bounds()
    return dict(p=m.model_params()[i], d=m.disturbance()[i], Qd=m.scaling[0] * W[i, :13], Rd=m.scaling[0] * W[i, 13:],
                QNd=m.scaling[1] * WN[i], lb=lb[i], ub=ub[i], M=m.erk)


def final_reference(oracle, m, seed):
    """-> (inputs of final_inputs, {row: final_case(...)}) for the checked rows"""
    x0, x, u, y, ye = final_inputs(oracle, m, seed)
    return (x0, x, u, y, ye), {i: final_case(oracle, row_data(m, i), x0[i], x[i], u[i], y[i], ye[i]) for i in checked_rows(m.B)}
