"""Time of the device-side polynomial references -> profiles/poly_time_65536.json.

65 536 instances, N = 50, the 10-piece figure-8 (tests/golden/poly.npz) as the library, every vehicle assigned with a random
placement.  In ONE process, each call between HIP events on the solver's stream, warmed up, median of `--reps`:
    set_yref_poly                       the new call (consistent rows; and with CFNMPC_POLY_KINEMATIC)
    set_yref_windows (Tracking)         the existing device path: one shared 17-column table, one phase per vehicle
    set_yref from a host array          the same per-vehicle rows [B][N][17] from pageable host memory: what a caller needs today
                                        for per-vehicle paths (upload + layout kernel; the host's time to PRODUCE the rows is not
                                        counted: the twin takes longer than the upload)
    one RTI step                        the bench's kicked hover fleet (bench.Fleet), for scale
The floor is the window's bytes (B (17 N + 13) doubles) at the fill rate the same process measures the way tools/hbm_rates.py
does.  python tools/poly_time.py [--batch 65536] [--reps 30] [--out profiles/poly_time_65536.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    return dict(median_ms=float(np.median(v)), mean_ms=float(np.mean(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), n=len(v))


def timed(torch, st, reps, call, warm=3):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        call()
        e1.record(st)
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return stats(out)


def run(B, reps, with_step):
    import torch
    from crazyflie_nmpc_amd import BatchSolver, default_opts
    from crazyflie_nmpc_amd import trajectories as tj
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    N, dt = 50, 0.015
    tab = np.load(os.path.join(ROOT, "tests", "golden", "poly.npz"))["figure8_table"]
    D = float(tab[:, 0].sum())
    rng = np.random.default_rng(0)
    s = BatchSolver(B, default_opts(N=N))
    traj = np.zeros(B, dtype=np.int32)
    place = np.stack([-rng.uniform(0.0, D, B), rng.choice([0.5, 1.0, 2.0], B), rng.uniform(-5, 5, B), rng.uniform(-5, 5, B),
                      rng.uniform(0.3, 2.0, B), rng.uniform(-np.pi, np.pi, B)], 1)
    s.set_poly_library([tab])
    s.set_poly_assignment(torch.as_tensor(traj, device=dev), torch.as_tensor(place, device=dev))
    out = {"batch": B, "N": N, "pieces": int(tab.shape[0]), "reps": reps}
    clock = [0.0]

    def poly(flags):
        def call():
            clock[0] += dt
            s.set_yref_poly(clock[0], flags)
        return call
    out["set_yref_poly"] = timed(torch, st, reps, poly(tj.POLY_LOOP))
    out["set_yref_poly_kinematic"] = timed(torch, st, reps, poly(tj.POLY_LOOP | tj.POLY_KINEMATIC))
    # the existing device path: one shared table, Tracking, a phase per vehicle
    table = torch.as_tensor(tj.figure8_reference(tj.Figure8(tab), N=N), device=dev)
    n_rows = int(table.shape[0])
    mode = torch.ones(B, dtype=torch.int32, device=dev)
    des = torch.zeros((B, 3), dtype=torch.float64, device=dev)
    it0 = torch.as_tensor(rng.integers(0, n_rows - N - 2 * reps - 8, B).astype(np.int32), device=dev)
    it = it0.clone()
    out["set_yref_windows_tracking"] = timed(torch, st, reps, lambda: s.set_yref_windows(table, mode, it, des, tj.USS_FILE))
    assert int(mode.min()) == 1, "every vehicle still tracks"
    # what a caller needs today for per-vehicle paths: the rows from the host
    sub = min(B, 2048)
    _f, rows = tj.poly_rows([tab], traj[:sub], place[:sub], 0.0, N + 1, dt, tj.POLY_LOOP)
    reps_h = -(-B // sub)
    yref = np.ascontiguousarray(np.tile(rows[:, :N], (reps_h, 1, 1))[:B])
    yref_e = np.ascontiguousarray(np.tile(rows[:, N, :13], (reps_h, 1))[:B])
    out["set_yref_from_host"] = timed(torch, st, max(3, reps // 3), lambda: s.set_yref(yref, yref_e), warm=2)
    # the floor: the window's bytes at the box's fill rate (tools/hbm_rates.py's measurement, 1 GiB)
    a = torch.empty((1 << 30) // 8, dtype=torch.float64, device=dev)
    fill = timed(torch, st, 10, lambda: a.fill_(1.0))
    rate = a.numel() * 8 / (fill["median_ms"] * 1e-3)
    nbytes = B * (17 * N + 13) * 8
    out["window_bytes"] = nbytes
    out["fill_rate_GBps"] = rate / 1e9
    out["floor_ms"] = nbytes / rate * 1e3
    del a
    if with_step:
        sys.path.insert(0, ROOT)
        import bench
        f = bench.Fleet(B, dev, np.random.default_rng(0))
        for _ in range(10):
            f.step()
        out["rti_step"] = timed(torch, st, reps, f.step, warm=2)
    out["ratio_poly_over_windows"] = out["set_yref_poly"]["median_ms"] / out["set_yref_windows_tracking"]["median_ms"]
    out["ratio_poly_over_floor"] = out["set_yref_poly"]["median_ms"] / out["floor_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = run(a.batch, a.reps, not a.no_step)
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
