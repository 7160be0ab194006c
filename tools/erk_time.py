"""ERK sub-steps per shooting interval at 65 536 hover instances: wall time per closed-loop RTI step
(mean and slowest of the timed steps) and per-kernel means for M = 1, 2, 3, 4 RK4 steps per interval, all with the stage-cost
scaling (dt, 1) of newer acados, plus M = 1 unscaled (the bench workload).

    python tools/erk_time.py [--batch 65536] [--steps 20] [--out DIR] [--profile profiles/erk_time_65536.json]

The parent process never opens the GPU: it runs this script as a fresh child once plain (wall times) and once under
`rocprofv3 --kernel-trace --stats` (kernel means; the wall times of that run are not used) per configuration, and writes one
JSON with both, the box (host name, GPU name) included, to --profile when given."""
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
CONFIGS = [("M1", 1, False), ("M1_scaled", 1, True), ("M2_scaled", 2, True), ("M3_scaled", 3, True), ("M4_scaled", 4, True)]


def child(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from crazyflie_nmpc_amd import BatchSolver, sim
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    from crazyflie_nmpc_amd.synthetic import regulation_row, sample_hover_x0
    torch.cuda.set_device(0)
    B, N, dt = args.batch, 50, 0.015
    rng = np.random.default_rng(1)
    x0 = sample_hover_x0(rng, B)
    row = regulation_row()
    yref = np.tile(row, (B, N, 1)); yref_e = np.tile(row[:13], (B, 1))
    out = {"batch": B, "N": N, "gpu": torch.cuda.get_device_name(0), "host": socket.gethostname(), "configs": {}}
    for name, M, scaled in CONFIGS:
        if args.only and name != args.only:
            continue
        s = BatchSolver(B)
        s.set_erk_steps(M)
        if scaled:
            s.set_cost_scaling(dt, 1.0)
        s.set_x0(x0); s.set_yref(yref, yref_e); s.init_iterate(INIT_HOVER)
        x = x0.copy()
        ms = []
        ok = 0
        for t in range(args.warmup + args.steps):
            s.set_x0(x)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.solve(1)
            torch.cuda.synchronize()
            if t >= args.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
            st, _it, _r = s.stats()
            ok += int((st == 0).sum()) if t >= args.warmup else 0
            x = sim(x, s.get_u(0), T=dt, steps=1)
            if t % 10 == 9:
                x[:, 10:13] += rng.uniform(-0.5, 0.5, (B, 3))
        out["configs"][name] = {"erk_steps": M, "cost_scaling": [dt, 1.0] if scaled else [1.0, 1.0],
                                "step_ms_mean": float(np.mean(ms)), "step_ms_max": float(np.max(ms)),
                                "step_ms_min": float(np.min(ms)), "status0_fraction": ok / (B * args.steps)}
        s.close()
        del s
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="directory of the children's results and the rocprofv3 output (default: a new "
                                                "temporary directory)")
    ap.add_argument("--profile", default=None, help="JSON to write the results to (e.g. profiles/erk_time_65536.json)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--only", default=None)
    ap.add_argument("--tag", default="plain")
    args = ap.parse_args()
    if args.out is None:
        args.out = tempfile.mkdtemp(prefix="erk_time_")
    os.makedirs(args.out, exist_ok=True)
    if args.child:
        child(args)
        return
    me = [sys.executable, os.path.abspath(__file__), "--child", "--batch", str(args.batch), "--out", args.out]
    subprocess.run(me + ["--steps", str(args.steps), "--warmup", str(args.warmup), "--tag", "plain"], check=True, timeout=900)
    res = json.load(open(os.path.join(args.out, "child_plain.json")))
    for name, _M, _sc in CONFIGS:   # one profiled child per configuration: the kernel names are shared between them
        prof_dir = os.path.join(args.out, "rocprof_" + name)
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof_dir, "--"] + me +
                       ["--steps", "5", "--warmup", "2", "--only", name, "--tag", "rocprof_" + name], check=True, timeout=900)
        res["configs"][name]["kernels"] = kernel_stats(prof_dir)
    res["limit_ms"] = 15.0      # the reference's control period
    res["target_M2_ms"] = 6.0
    if args.profile:
        with open(args.profile, "w") as f:
            json.dump(res, f, indent=1)
    for name, c in res["configs"].items():
        print(name, {k: c[k] for k in ("step_ms_mean", "step_ms_max", "status0_fraction")},
              {k: round(v["mean_ms"], 4) for k, v in c.get("kernels", {}).items() if v["calls"] >= 5})


if __name__ == "__main__":
    main()
