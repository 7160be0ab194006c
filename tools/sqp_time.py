"""Full SQP solve at 65 536 hover instances: k_sqp_check's kernel time, wall time of one SQP solve
from a cold start (INIT_ACADOS) and from a warm closed-loop iterate, and the histograms of sqp_iter.

    python tools/sqp_time.py [--batch 65536] [--out DIR] [--profile profiles/NAME.json] [--globalization]

--globalization: the same two solves with the merit-function line search as well (results under
"merit_backtracking"), the trials per launch of the first iterations of the cold solve (per row and per wavefront: the loop of
k_sqp_ls runs until its slowest row is through), and k_sqp_ls's kernel times per launch beside k_sqp_check's from the same run.

The parent process never opens the GPU: it runs this script twice as a fresh child -- once plain (wall times, histograms),
once under `rocprofv3 --kernel-trace --stats` (kernel means; the wall times of that run are not used) -- and writes one JSON
with both, the box (host name, GPU name) included, to --profile when given."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from crazyflie_nmpc_amd import BatchSolver, sim
    from crazyflie_nmpc_amd.solver import INIT_ACADOS, INIT_HOVER
    from crazyflie_nmpc_amd.synthetic import regulation_row, sample_hover_x0
    torch.cuda.set_device(0)
    B, N = args.batch, 50
    rng = np.random.default_rng(1)
    x0 = sample_hover_x0(rng, B)
    row = regulation_row()
    yref = np.tile(row, (B, N, 1)); yref_e = np.tile(row[:13], (B, 1))
    s = BatchSolver(B)
    s.set_x0(x0); s.set_yref(yref, yref_e)
    out = {"batch": B, "N": N, "gpu": torch.cuda.get_device_name(0), "host": socket.gethostname(),
           "tolerances": [1e-6, 1e-6, 1e-6], "max_iter": 100}

    def timed_sqp():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = s.solve_sqp()
        ms = (time.perf_counter() - t0) * 1e3
        st, it, _rs = s.sqp_stats()
        hist = {int(k): int(v) for k, v in zip(*np.unique(it, return_counts=True))}
        stat = {int(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))}
        return ms, n, hist, stat

    # RTI step for scale (the SQP iteration IS one such step plus k_sqp_check and one read-back)
    s.init_iterate(INIT_HOVER); s.solve(5); torch.cuda.synchronize()
    t0 = time.perf_counter(); s.solve(args.reps * 5); torch.cuda.synchronize()
    out["rti_step_ms"] = (time.perf_counter() - t0) * 1e3 / (args.reps * 5)
    # cold start: acados' initial guess (x_k = [0,0,0,1,0..], u_k = 0), fixed x0
    cold = []
    for _ in range(args.reps):
        s.init_iterate(INIT_ACADOS)
        cold.append(timed_sqp())
    out["cold"] = {"ms": [c[0] for c in cold], "iters_run": cold[-1][1], "sqp_iter_hist": cold[-1][2], "status": cold[-1][3],
                   "ms_per_iter": min(c[0] for c in cold) / cold[-1][1]}
    # warm: the iterate of a closed loop (30 RTI steps, plant = the model, a kick on every 10th step) at its current state
    s.init_iterate(INIT_HOVER)
    x = x0.copy()
    for t in range(30):
        s.set_x0(x); s.solve(1)
        x = sim(x, s.get_u(0), T=0.015, steps=1)
        if t % 10 == 9:
            x[:, 10:13] += rng.uniform(-0.5, 0.5, (B, 3))
    s.set_x0(x)
    xs, us = s.get_iterate()
    warm = []
    for _ in range(args.reps):
        s.set_iterate(xs, us)
        warm.append(timed_sqp())
    out["warm"] = {"ms": [w[0] for w in warm], "iters_run": warm[-1][1], "sqp_iter_hist": warm[-1][2], "status": warm[-1][3],
                   "ms_per_iter": min(w[0] for w in warm) / warm[-1][1]}
    if args.globalization:
        s.set_sqp_globalization("merit_backtracking")
        g = {}
        cold = []
        for _ in range(args.reps):
            s.init_iterate(INIT_ACADOS)
            cold.append(timed_sqp())
        g["cold"] = {"ms": [c[0] for c in cold], "iters_run": cold[-1][1], "sqp_iter_hist": cold[-1][2], "status": cold[-1][3],
                     "ms_per_iter": min(c[0] for c in cold) / cold[-1][1]}
        al, mu, ns, nf = s.sqp_ls_stats()
        g["cold"].update(rows_with_short_steps=int((ns > 0).sum()), short_steps=int(ns.sum()), failed_searches=int(nf.sum()))
        warm = []
        for _ in range(args.reps):
            s.set_iterate(xs, us)
            warm.append(timed_sqp())
        g["warm"] = {"ms": [w[0] for w in warm], "iters_run": warm[-1][1], "sqp_iter_hist": warm[-1][2], "status": warm[-1][3],
                     "ms_per_iter": min(w[0] for w in warm) / warm[-1][1]}
        al, mu, ns, nf = s.sqp_ls_stats()
        g["warm"].update(rows_with_short_steps=int((ns > 0).sum()), short_steps=int(ns.sum()), failed_searches=int(nf.sum()))
        # trials of launch j of the cold solve: a solve capped at j iterations leaves the step length of iteration j (rows done
        # before it keep an earlier one and are left out); the wavefront's loop runs as many rounds as its slowest row
        trials = []
        for j in range(1, args.trial_iters + 1):
            s.init_iterate(INIT_ACADOS)
            s.solve_sqp(max_iter=j)
            _st, it, _rs = s.sqp_stats()
            al = s.sqp_ls_stats()[0]
            t = np.where(it == j, np.round(-np.log2(al)), 0).astype(np.int64)
            tw = np.pad(t, (0, (-B) % 64)).reshape(-1, 64).max(1)
            trials.append({"launch": j, "open_rows": int((it == j).sum()),
                           "row_trials_hist": {int(k): int(v) for k, v in zip(*np.unique(t[it == j], return_counts=True))},
                           "wave_rounds_hist": {int(k): int(v) for k, v in zip(*np.unique(tw, return_counts=True))},
                           "wave_rounds_mean": float(tw.mean())})
        g["trials_per_launch"] = trials
        out["merit_backtracking"] = g
        s.set_sqp_globalization("full_step")
    with open(os.path.join(args.out, "child_%s.json" % args.tag), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


def kernel_stats(d):
    paths = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not paths:
        return {}
    res = {}
    for r in csv.DictReader(open(paths[0])):
        name = r["Name"].split("(")[0].replace("cfn::", "")
        res[name] = {"calls": int(r["Calls"]), "mean_ms": float(r["AverageNs"]) / 1e6, "min_ms": float(r["MinNs"]) / 1e6,
                     "max_ms": float(r["MaxNs"]) / 1e6}
    return res


def kernel_calls(d, names):
    """per-launch durations [ms] of the named kernels, in launch order"""
    res = {n: [] for n in names}
    paths = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        return res
    rows = sorted(csv.DictReader(open(paths[0])), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].replace("cfn::", "")
        if name in res:
            res[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory of the children's results and the rocprofv3 output (default: a new "
                                                "temporary directory)")
    ap.add_argument("--profile", default=None, help="JSON to write the results to (e.g. profiles/sqp_time_65536.json)")
    ap.add_argument("--globalization", action="store_true", help="the solves with the merit-function line search as well")
    ap.add_argument("--trial-iters", type=int, default=12, help="launches of the cold solve whose trials are counted")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tag", default="plain")
    args = ap.parse_args()
    if args.out is None:
        args.out = tempfile.mkdtemp(prefix="sqp_time_")
    os.makedirs(args.out, exist_ok=True)
    if args.child:
        child(args)
        return
    me = [sys.executable, os.path.abspath(__file__), "--child", "--batch", str(args.batch), "--out", args.out]
    if args.globalization:
        me += ["--globalization", "--trial-iters", str(args.trial_iters)]
    subprocess.run(me + ["--reps", str(args.reps), "--tag", "plain"], check=True, timeout=900)
    prof_dir = os.path.join(args.out, "rocprof")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof_dir, "--"] + me +
                   ["--reps", "1", "--tag", "rocprof"], check=True, timeout=900)
    res = json.load(open(os.path.join(args.out, "child_plain.json")))
    ks = kernel_stats(prof_dir)
    res["kernels"] = ks
    res["k_sqp_check_mean_ms"] = ks.get("k_sqp_check", {}).get("mean_ms")
    res["target_k_sqp_check_ms"] = 0.25
    if args.globalization:
        # launch order of the profiled child (--reps 1): cold and warm solve, then the capped solves of 1 .. trial_iters iterations
        calls = kernel_calls(prof_dir, ("k_sqp_ls", "k_sqp_check"))
        ls = calls["k_sqp_ls"]
        g = res["merit_backtracking"]
        n_cold, n_warm = g["cold"]["iters_run"], g["warm"]["iters_run"]
        res["k_sqp_ls_ms"] = {"cold_solve": ls[:n_cold], "warm_solve": ls[n_cold:n_cold + n_warm],
                              "min": min(ls) if ls else None, "mean": sum(ls) / len(ls) if ls else None, "max": max(ls) if ls else None}
        res["k_sqp_check_ms"] = {"min": min(calls["k_sqp_check"], default=None), "calls": len(calls["k_sqp_check"])}
    if args.profile:
        with open(args.profile, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("gpu", "host", "rti_step_ms", "k_sqp_check_mean_ms")}))
    print("cold", res["cold"]); print("warm", res["warm"])


if __name__ == "__main__":
    main()
