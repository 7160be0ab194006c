"""Generates tests/golden/poly.npz: the three piecewise-polynomial trajectories of the reference's crazyflie_demo/scripts
(figure8.csv, takeoff.csv, figure8withTakeoffAndLanding.csv) as coefficient tables, and what the REFERENCE'S OWN EVALUATOR
(crazyflie_demo/scripts/uav_trajectory.py, imported in place, never copied) returns for them: pos, vel, acc, yaw, omega.

    python tests/golden/make_golden_poly.py <checkout of the reference>

Sample times per table: every multiple of 0.015 s below the duration, 40 random times, and for every inner piece boundary
`cum` (accumulated in a Python loop, as Trajectory.eval does) cum itself and cum +- 1e-9.  The evaluator asserts t <= duration
and returns None at t == duration: every time stays strictly below it.

Keys per table NAME in (figure8, takeoff, figure8_takeoff_landing):
    NAME_table [n][33], NAME_t [m], NAME_grid (number of leading grid times), NAME_nbound (number of trailing boundary times),
    NAME_pos / _vel / _acc / _omega [m][3], NAME_yaw [m].
Only arrays are written."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = {"figure8": "figure8.csv", "takeoff": "takeoff.csv", "figure8_takeoff_landing": "figure8withTakeoffAndLanding.csv"}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CRAZYFLIE_REFERENCE")
    if not ref:
        raise SystemExit(__doc__)
    scripts = os.path.join(ref, "crazyflie_demo", "scripts")
    sys.path.insert(0, scripts)
    import uav_trajectory                      # the REFERENCE's evaluator, run in place
    rng = np.random.default_rng(20200522)
    out = {}
    for name, fn in FILES.items():
        path = os.path.join(scripts, fn)
        tr = uav_trajectory.Trajectory()
        tr.loadcsv(path)
        table = np.loadtxt(path, delimiter=",", skiprows=1, usecols=range(33), ndmin=2)
        dur = float(tr.duration)
        grid = []
        k = 0
        while 0.015 * k < dur:
            grid.append(0.015 * k)
            k += 1
        rnd = list(rng.uniform(0.0, dur * (1.0 - 1e-9), 40))
        bound = []
        cum = 0.0
        for row in table[:-1]:
            cum = cum + row[0]
            bound += [cum - 1e-9, cum, cum + 1e-9]
        t = np.array(grid + rnd + bound)
        assert (t >= 0).all() and (t < dur).all()
        res = [tr.eval(float(x)) for x in t]
        assert all(r is not None for r in res)
        out[name + "_table"] = table
        out[name + "_t"] = t
        out[name + "_grid"] = np.int64(len(grid))
        out[name + "_nbound"] = np.int64(len(bound))
        for f in ("pos", "vel", "acc", "omega"):
            out[name + "_" + f] = np.array([getattr(r, f) for r in res], dtype=np.float64)
        out[name + "_yaw"] = np.array([r.yaw for r in res], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "poly.npz"), **out)
    print("poly.npz written:", {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
