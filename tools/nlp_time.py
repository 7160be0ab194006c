"""NLP evaluation at 65 536 hover instances: k_nlp_eval's kernel time with and without kept
multipliers beside k_sqp_check from the same run, the achieved memory rate against the 34-doubles-per-stage estimate, and the
wall time of one eval_nlp + nlp_stats.

    python tools/nlp_time.py [--batch 65536] [--out DIR] [--profile profiles/NAME.json]

The parent process never opens the GPU: it runs this script twice as a fresh child -- once plain (wall times), once under
`rocprofv3 --kernel-trace --stats` (kernel times, in a run of its own; the wall times of that run are not used) -- and writes
one JSON with both, the box (host name, GPU name) included, to --profile when given."""
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
    from crazyflie_nmpc_amd import BatchSolver
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    from crazyflie_nmpc_amd.synthetic import regulation_row, sample_hover_x0
    torch.cuda.set_device(0)
    B, N = args.batch, 50
    rng = np.random.default_rng(1)
    x0 = sample_hover_x0(rng, B)
    row = regulation_row()
    yref = np.tile(row, (B, N, 1)); yref_e = np.tile(row[:13], (B, 1))
    s = BatchSolver(B)
    s.set_x0(x0); s.set_yref(yref, yref_e); s.init_iterate(INIT_HOVER)
    out = {"batch": B, "N": N, "gpu": torch.cuda.get_device_name(0), "host": socket.gethostname()}
    s.solve(5); torch.cuda.synchronize()
    t0 = time.perf_counter(); s.solve(args.reps * 5); torch.cuda.synchronize()
    out["rti_step_ms"] = (time.perf_counter() - t0) * 1e3 / (args.reps * 5)

    def timed(keep, reps):
        s.eval_nlp(keep_multipliers=keep); torch.cuda.synchronize()      # (first call with keep: allocates)
        t0 = time.perf_counter()
        for _ in range(reps):
            s.eval_nlp(keep_multipliers=keep)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    out["eval_ms"] = timed(False, args.reps * 5)
    t0 = time.perf_counter(); cost, res = s.nlp_stats(); out["nlp_stats_ms"] = (time.perf_counter() - t0) * 1e3
    out["eval_keep_ms"] = timed(True, args.reps * 5)
    t0 = time.perf_counter(); s.nlp_multipliers(); out["nlp_multipliers_ms"] = (time.perf_counter() - t0) * 1e3
    out["res_max"] = [float(v) for v in res.max(0)]
    out["cost_mean"] = float(cost.mean())
    # k_sqp_check for the same run's comparison: two SQP iterations
    s.solve_sqp(2)
    # the options that change the kernel's work
    s.set_erk_steps(2); out["eval_erk2_ms"] = timed(False, args.reps); s.set_erk_steps(1)
    p = np.tile(np.array([9.8066, 33e-3, 1.395e-5, 1.395e-5, 2.173e-5, 7.9379e-06, 3.25e-4, 0.0325]), (B, 1))
    s.set_model_params(p); out["eval_par_ms"] = timed(False, args.reps); s.set_model_params(None)
    with open(os.path.join(args.out, "child_%s.json" % args.tag), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


def kernel_calls(d, names):
    """per kernel name: the durations [ms] of its dispatches in launch order (kernel trace)"""
    paths = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    res = {n: [] for n in names}
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
    ap.add_argument("--profile", default=None, help="JSON to write the results to (e.g. profiles/nlp_time_65536.json)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tag", default="plain")
    args = ap.parse_args()
    if args.out is None:
        args.out = tempfile.mkdtemp(prefix="nlp_time_")
    os.makedirs(args.out, exist_ok=True)
    if args.child:
        child(args)
        return
    me = [sys.executable, os.path.abspath(__file__), "--child", "--batch", str(args.batch), "--out", args.out]
    subprocess.run(me + ["--reps", str(args.reps), "--tag", "plain"], check=True, timeout=600)
    prof_dir = os.path.join(args.out, "rocprof")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof_dir, "--"] + me +
                   ["--reps", "1", "--tag", "rocprof"], check=True, timeout=600)
    res = json.load(open(os.path.join(args.out, "child_plain.json")))
    calls = kernel_calls(prof_dir, ("k_nlp_eval", "k_nlp_eval_par", "k_sqp_check"))
    # launch order of the child with --reps 1: 1 + 5 without multipliers, 1 + 5 with, then erk_steps 2 (1 + 1)
    ne = calls["k_nlp_eval"]
    res["kernels_ms"] = {"k_nlp_eval": ne[:6], "k_nlp_eval_keep": ne[6:12], "k_nlp_eval_erk2": ne[12:14],
                         "k_nlp_eval_par": calls["k_nlp_eval_par"], "k_sqp_check": calls["k_sqp_check"]}
    B, N = res["batch"], res["N"]
    gb = B * N * 34 * 8 / 1e9                       # the estimate's traffic: x 13, u 4, yref 17 per instance and stage
    gb_keep = gb + B * (N * 17 + 13) * 8 / 1e9      # + pi and g written
    if ne[:6]:
        res["k_nlp_eval_min_ms"] = min(ne[:6]); res["achieved_TBps"] = gb / min(ne[:6])
    if ne[6:12]:
        res["k_nlp_eval_keep_min_ms"] = min(ne[6:12]); res["achieved_keep_TBps"] = gb_keep / min(ne[6:12])
    if calls["k_sqp_check"]:
        res["k_sqp_check_min_ms"] = min(calls["k_sqp_check"])
    if args.profile:
        with open(args.profile, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: res.get(k) for k in ("gpu", "host", "rti_step_ms", "eval_ms", "eval_keep_ms", "k_nlp_eval_min_ms",
                                              "k_nlp_eval_keep_min_ms", "k_sqp_check_min_ms", "achieved_TBps", "eval_erk2_ms",
                                              "eval_par_ms")}))


if __name__ == "__main__":
    main()
