"""Reference trajectories for the Tracking policy of the reference node.

* `load_traj_text`: the 17-column whitespace text format of crazyflie_controller/traj/*.txt
  (one row per 15 ms: x y z qw qx qy qz vbx vby vbz wx wy wz w1 w2 w3 w4), loader semantics of
  NMPC::readDataFromFile (acados_mpc.cpp:354-382): one row per line, row count = line count.
* `Figure8`: piecewise 7th-order polynomial trajectory in the crazyflie_demo CSV format
  (crazyflie_demo/scripts/figure8.csv; evaluation semantics of uav_trajectory.py:15-20 Horner,
  :97-105 piece lookup by cumulative duration).
* `figure8_reference`: SURVEY.md App. C synthesis of a 17-column NMPC reference from it
  (the reference repo has no figure-8 in crazyflie_controller/traj/, finding F6).
"""
from __future__ import annotations

import numpy as np

from .synthetic import HOV_W

TS = 0.015
USS_FILE = 15.7777  # hover speed as printed in the reference's trajectory files (helix_traj.txt:1)


def load_traj_text(path):
    rows = []
    with open(path) as f:
        for line in f:
            rows.append([float(t) for t in line.split()])
    return np.array(rows, dtype=np.float64)


def save_traj_text(path, traj):
    np.savetxt(path, traj, fmt="%.4f")


class Figure8:
    """rows: [duration, x^0..x^7, y^0..y^7, z^0..z^7, yaw^0..yaw^7] (ascending powers)."""

    def __init__(self, table):
        self.table = np.asarray(table, dtype=np.float64)
        assert self.table.ndim == 2 and self.table.shape[1] == 33
        self.duration = float(self.table[:, 0].sum())

    @staticmethod
    def _horner(p, t):
        x = 0.0
        for i in range(len(p)):
            x = x * t + p[len(p) - 1 - i]
        return x

    def eval(self, t):
        """-> (pos[3], yaw) at time t in [0, duration]"""
        assert 0.0 <= t <= self.duration + 1e-12
        cur = 0.0
        for row in self.table:
            if t < cur + row[0]:
                tt = t - cur
                return (np.array([self._horner(row[1:9], tt), self._horner(row[9:17], tt), self._horner(row[17:25], tt)]),
                        self._horner(row[25:33], tt))
            cur += row[0]
        row = self.table[-1]
        tt = row[0]
        return (np.array([self._horner(row[1:9], tt), self._horner(row[9:17], tt), self._horner(row[17:25], tt)]),
                self._horner(row[25:33], tt))


def figure8_reference(fig8: Figure8, z0=0.5, N=50, uss=USS_FILE):
    """Kinematic 17-column reference in the style of helix_traj.txt: positions
    sampled every 15 ms, identity attitude, zero velocities, hover speeds; N+1 copies of the last
    sample appended so that the Tracking window logic (rows iter..iter+N) can run to the end."""
    n = int(np.floor(fig8.duration / TS)) + 1
    rows = []
    for k in range(n):
        pos, _yaw = fig8.eval(min(TS * k, fig8.duration))
        rows.append([pos[0], pos[1], pos[2] + z0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, uss, uss, uss, uss])
    rows += [rows[-1]] * (N + 1)
    return np.array(rows, dtype=np.float64)


def tracking_window(traj, it, N=50):
    """Rows it..it+N of the trajectory as (yref [N][17], yref_e [13]) (acados_mpc.cpp:460-485)."""
    win = traj[it:it + N + 1]
    return win[:N].copy(), win[N, :13].copy()


def regulation_window(xyz, N=50, uss=HOV_W):
    row = np.zeros(17)
    row[0:3] = xyz
    row[3] = 1.0
    row[13:17] = uss
    return np.tile(row, (N, 1)), row[:13].copy()


# ---- device-side polynomial references (include/cfnmpc.h: cfnmpc_set_yref_poly) --------------------
POLY_NC = 33          # one piece: duration, x^0..x^7, y^0..y^7, z^0..z^7, yaw^0..yaw^7
NPLACE = 6            # placement row: t_start, time_scale, ox, oy, oz, yaw0
NFLAT = 13            # pos[3], vel[3], acc[3], yaw, omega[3]
POLY_LOOP, POLY_KINEMATIC = 1, 2
_NOMINAL_PARAMS = np.array([9.8066, 33e-3, 1.395e-5, 1.395e-5, 2.173e-5, 7.9379e-06, 3.25e-4, 0.0325])


def load_poly_csv(path):
    """-> [n_pieces][33]: a trajectory in the crazyflie_demo CSV format (one header line, then one piece per line:
    duration, x^0..x^7, y^0..y^7, z^0..z^7, yaw^0..yaw^7; a trailing comma is tolerated)."""
    tab = np.loadtxt(path, delimiter=",", skiprows=1, usecols=range(POLY_NC), ndmin=2)
    return np.ascontiguousarray(tab, dtype=np.float64)


def poly_library(tables):
    """-> (pieces [sum n_i][33], first [n_traj + 1] int32): the tables packed as cfnmpc_set_poly_library takes them"""
    tables = [np.asarray(t, dtype=np.float64).reshape(-1, POLY_NC) for t in tables]
    first = np.zeros(len(tables) + 1, dtype=np.int32)
    first[1:] = np.cumsum([len(t) for t in tables])
    pieces = np.concatenate(tables, axis=0) if tables else np.zeros((0, POLY_NC))
    return np.ascontiguousarray(pieces), first


def _horner(c, s):
    """Horner's rule on the coefficient list c [..., n] (ascending powers) at s, as uav_trajectory.py:15-20"""
    x = np.zeros_like(s)
    for i in range(c.shape[-1]):
        x = x * s + c[..., c.shape[-1] - 1 - i]
    return x


def _deriv(c):
    """the coefficient list (i + 1) c[i + 1] (uav_trajectory.py:23-24)"""
    return np.arange(1, c.shape[-1], dtype=np.float64) * c[..., 1:]


def poly_rows(tables, traj, place, t, n_stages, dt, flags=0, params=None):
    """Host twin of the device kernel k_poly_rows, operation for operation (the rules of include/cfnmpc.h).

    tables: list of [n_i][33] coefficient tables; traj [B] ids (-1: none); place [B][6] = t_start, time_scale, ox, oy, oz,
    yaw0 (None: [0, 1, 0, 0, 0, 0]); rows k = 0 .. n_stages - 1 at the fleet times t + k dt; params [B][8] model parameter rows
    (None: nominal).  -> (flat [B][n_stages][13], rows [B][n_stages][17]); NaN for vehicles without a trajectory."""
    traj = np.asarray(traj, dtype=np.int64).reshape(-1)
    B = traj.shape[0]
    place = np.tile([0.0, 1.0, 0.0, 0.0, 0.0, 0.0], (B, 1)) if place is None else np.asarray(place, dtype=np.float64).reshape(B, NPLACE)
    par = np.tile(_NOMINAL_PARAMS, (B, 1)) if params is None else np.asarray(params, dtype=np.float64).reshape(B, 8)
    flat = np.full((B, n_stages, NFLAT), np.nan)
    rows = np.full((B, n_stages, 17), np.nan)
    tq = t + np.arange(n_stages, dtype=np.float64) * dt
    with np.errstate(invalid="ignore", divide="ignore"):
        for tid, tab in enumerate(tables):
            sel = np.nonzero(traj == tid)[0]
            if sel.size == 0:
                continue
            tab = np.asarray(tab, dtype=np.float64).reshape(-1, POLY_NC)
            f, r = _poly_rows_one(tab, place[sel], par[sel], tq, flags)
            flat[sel], rows[sel] = f, r
    return flat, rows


def _poly_rows_one(tab, place, par, tq, flags):
    npc = tab.shape[0]
    cum = np.zeros(npc)
    edge = np.zeros(npc)
    c = 0.0
    for j in range(npc):                  # accumulated piece by piece, as Trajectory.eval does
        cum[j] = c
        c = c + tab[j, 0]
        edge[j] = c
    D = c
    ts = place[:, 1]
    ts = np.where(np.isfinite(ts) & (ts > 0.0), ts, 1.0)[:, None]
    tau = (tq[None, :] - place[:, 0:1]) / ts
    before = tau < 0.0
    after = tau >= D
    if flags & POLY_LOOP:
        w = tau - D * np.floor(tau / D)
        w = np.where(w < 0.0, 0.0, w)
        tau = np.where(after, w, tau)
        after = np.zeros_like(after)
    held = before | after
    idx = np.minimum((tau[..., None] >= edge).sum(-1), npc - 1)      # the first piece with tau < cum + duration (else the last)
    s = tau - cum[idx]
    idx = np.where(before, 0, np.where(after, npc - 1, idx))
    s = np.where(before, 0.0, np.where(after, tab[npc - 1, 0], s))
    co = tab[idx]                                                    # [b][k][33]
    ts2 = ts * ts
    ts3 = ts2 * ts
    p0, p1, p2, p3 = [], [], [], []
    for a in range(4):
        c0 = co[..., 1 + 8 * a:9 + 8 * a]
        c1 = _deriv(c0); c2 = _deriv(c1); c3 = _deriv(c2)
        p0.append(_horner(c0, s))
        p1.append(np.where(held, 0.0, _horner(c1, s) / ts))
        p2.append(np.where(held, 0.0, _horner(c2, s) / ts2))
        p3.append(np.where(held, 0.0, _horner(c3, s) / ts3))
    yaw0 = place[:, 5:6]
    c0y, s0y = np.cos(yaw0), np.sin(yaw0)

    def rz(vx, vy):
        return c0y * vx - s0y * vy, s0y * vx + c0y * vy
    px, py = rz(p0[0], p0[1])
    pos = np.stack([px + place[:, 2:3], py + place[:, 3:4], p0[2] + place[:, 4:5]], -1)
    vel = np.stack([*rz(p1[0], p1[1]), p1[2]], -1)
    acc = np.stack([*rz(p2[0], p2[1]), p2[2]], -1)
    jerk = np.stack([*rz(p3[0], p3[1]), p3[2]], -1)
    yaw = p0[3] + yaw0
    dyaw = p1[3]
    g0, mq, ct = par[:, 0:1], par[:, 1:2], par[:, 6:7]
    kt = ct / mq
    hov = np.sqrt((mq * g0) / (4 * ct)) + 0.0 * yaw
    cy, sy = np.cos(yaw), np.sin(yaw)
    thr = acc + np.stack([0.0 * yaw, 0.0 * yaw, g0 + 0.0 * yaw], -1)
    nthr = np.sqrt(thr[..., 0] * thr[..., 0] + thr[..., 1] * thr[..., 1] + thr[..., 2] * thr[..., 2])
    zb = thr / nthr[..., None]
    cx_, cy_, cz_ = -zb[..., 2] * sy, zb[..., 2] * cy, zb[..., 0] * sy - zb[..., 1] * cy       # z_b x x_w
    nc = np.sqrt(cx_ * cx_ + cy_ * cy_ + cz_ * cz_)
    yb = np.stack([cx_, cy_, cz_], -1) / nc[..., None]
    xb = np.stack([yb[..., 1] * zb[..., 2] - yb[..., 2] * zb[..., 1], yb[..., 2] * zb[..., 0] - yb[..., 0] * zb[..., 2],
                   yb[..., 0] * zb[..., 1] - yb[..., 1] * zb[..., 0]], -1)
    jz = jerk[..., 0] * zb[..., 0] + jerk[..., 1] * zb[..., 1] + jerk[..., 2] * zb[..., 2]
    hw = (jerk - jz[..., None] * zb) / nthr[..., None]
    dot = lambda a, b: a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]
    wx, wy = -dot(hw, yb), dot(hw, xb)
    wz_eval = zb[..., 2] * dyaw
    # exact body rate about z: -x_b . (h_w x x_w + z_b x dx_w) / |c|
    ex = -hw[..., 2] * sy - dyaw * (zb[..., 2] * cy)
    ey = hw[..., 2] * cy - dyaw * (zb[..., 2] * sy)
    ez = (hw[..., 0] * sy - hw[..., 1] * cy) + dyaw * (zb[..., 0] * cy + zb[..., 1] * sy)
    wz = -(xb[..., 0] * ex + xb[..., 1] * ey + xb[..., 2] * ez) / nc
    # attitude q = qz(yaw) qx(phi) qy(theta)
    zlx = cy * zb[..., 0] + sy * zb[..., 1]
    zly = -sy * zb[..., 0] + cy * zb[..., 1]
    theta = np.arcsin(np.clip(zlx, -1.0, 1.0))
    phi = np.arctan2(-zly, zb[..., 2])
    chz, shz = np.cos(0.5 * yaw), np.sin(0.5 * yaw)
    chx, shx = np.cos(0.5 * phi), np.sin(0.5 * phi)
    cht, sht = np.cos(0.5 * theta), np.sin(0.5 * theta)
    a_, b_, c_, d_ = chx * cht, shx * cht, chx * sht, shx * sht
    q = np.stack([chz * a_ - shz * d_, chz * b_ - shz * c_, chz * c_ + shz * b_, chz * d_ + shz * a_], -1)
    vb = np.stack([dot(xb, vel), dot(yb, vel), dot(zb, vel)], -1)
    spd = np.sqrt(nthr / (4 * kt))
    # level rows: held stages and the guard
    level = held | ~((thr[..., 2] > 0.1 * g0) & (nc >= 1e-3))
    zero = 0.0 * yaw
    q_l = np.stack([chz, zero, zero, shz], -1)
    vb_l = np.stack([cy * vel[..., 0] + sy * vel[..., 1], -sy * vel[..., 0] + cy * vel[..., 1], vel[..., 2]], -1)
    L = level[..., None]
    q = np.where(L, q_l, q)
    vb = np.where(L, vb_l, vb)
    om = np.where(L, np.stack([zero, zero, dyaw], -1), np.stack([wx, wy, wz], -1))
    om_f = np.where(L, np.stack([zero, zero, dyaw], -1), np.stack([wx, wy, wz_eval], -1))
    spd = np.where(level, hov, spd)
    flat = np.concatenate([pos, vel, acc, yaw[..., None], om_f], -1)
    if flags & POLY_KINEMATIC:
        q = np.stack([zero + 1.0, zero, zero, zero], -1)
        vb = np.zeros_like(vb)
        om = np.zeros_like(om)
        spd = hov
    rows = np.concatenate([pos, q, vb, om, np.repeat(spd[..., None], 4, -1)], -1)
    return flat, rows
