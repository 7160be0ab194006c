"""Time of the adjoint solution sensitivities -> profiles/adj_time_65536.json.

65 536 instances in the bench's closed loop (bench.Fleet: hover regulation, staggered kicks, RK4 plant), kicks x 1 (the bench
workload) and x 2.  After 10 untimed RTI steps, per step of `--steps` more: the step itself, eval_sens_x0, then eval_adjoint for
a loss on u_0 only (gu [B][1][4]) and for a full-horizon loss (gx [B][N + 1][13], gu [B][N][4]) from device tensors, and the
reads of the per-vehicle gradients (dl_dx0, dl_dW, dl_dWN) into device tensors, each timed with HIP events on the fleet's
stream.  Also recorded: the share of rows with an active input and the workspace the adjoint buffers add.
--profile adds the kernel means next to k_factor's: one child run per workload under `rocprofv3 --kernel-trace --stats`, kept
apart from the timed runs.  The committed profile is the output of
    python tools/adj_time.py --profile [--batch 65536] [--steps 10] [--out profiles/adj_time_65536.json]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(B, steps, kick_scale):
    import torch
    import bench
    dev = torch.device("cuda", 0)
    f = bench.Fleet(B, dev, np.random.default_rng(0), kick_scale=kick_scale)
    s, N = f.solver, f.solver.N
    st = torch.cuda.current_stream(dev)
    for _ in range(10):
        f.step()
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *sh: torch.randn(sh, dtype=torch.float64, device=dev, generator=g)
    gu0, gxN, guN = rnd(B, 1, 4), rnd(B, N + 1, 13), rnd(B, N, 4)
    emp = lambda *sh: torch.empty(sh, dtype=torch.float64, device=dev)
    dx0, dW, dWN = emp(B, 13), emp(B, 17), emp(B, 13)
    bytes0 = None
    t = {k: [] for k in ("step", "eval_sens_x0", "eval_adjoint_u0", "eval_adjoint_full", "get_small")}
    shares = []
    for _ in range(steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        ev[0].record(st)
        f.step()
        ev[1].record(st)
        s.eval_sens_x0()
        if bytes0 is None:
            bytes0 = s.workspace_bytes
        ev[2].record(st)
        s.eval_adjoint(None, gu0)
        ev[3].record(st)
        s.eval_adjoint(gxN, guN)
        ev[4].record(st)
        s.adjoint(out=(dx0, None, None, None, None))
        s.adjoint_cost(out=(dW, dWN, None, None))
        ev[5].record(st)
        torch.cuda.synchronize()
        for i, k in enumerate(t):
            t[k].append(ev[i].elapsed_time(ev[i + 1]))
        shares.append(float((s.sens_active() != 0).any(axis=(1, 2)).mean()))
    # (the first timed step allocates the buffers inside its eval_adjoint: left out of the adjoint's figures)
    out = {k: dict(mean_ms=float(np.mean(v[1:] if k.startswith("eval_adjoint") else v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)))
           for k, v in t.items()}
    out["listed_share"] = dict(mean=float(np.mean(shares)), min=float(np.min(shares)), max=float(np.max(shares)))
    out["workspace_added_bytes"] = int(s.workspace_bytes - bytes0)
    f.close()
    return out


def kernel_stats(B, steps, kick_scale):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--batch", str(B), "--steps", str(steps),
               "--kick-scale", str(kick_scale)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        stats = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    name = row["Name"].split("(")[0].replace("cfn::", "")
                    if "adj" in name or "sens" in name or name in ("k_factor", "k_linearise"):
                        stats[name] = dict(calls=int(row["Calls"]), mean_us=float(row["AverageNs"]) / 1e3)
        return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kick-scale", type=float, default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adj_time_65536.json"))
    a = ap.parse_args()
    if a.child:
        run(a.batch, a.steps, a.kick_scale or 1.0)
        return
    res = {"batch": a.batch, "steps": a.steps, "workload": "bench.Fleet closed loop (hover, staggered kicks)", "runs": {}}
    for ks in ([a.kick_scale] if a.kick_scale else [1.0, 2.0]):
        r = run(a.batch, a.steps, ks)
        if a.profile:
            r["kernels"] = kernel_stats(a.batch, 3, ks)
        res["runs"][f"kicks_x{ks:g}"] = r
        print(json.dumps({f"kicks_x{ks:g}": r}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
