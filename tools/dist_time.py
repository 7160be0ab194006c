"""Step time with per-instance disturbance rows -> profiles/dist_time_65536.json.

65 536 hover instances in the kicked closed loop (plant = cfnmpc_sim_dist with each row's own disturbance where the variant has
one, velocity kicks every third step), 20 timed RTI steps per variant after 5 untimed ones.  The variants alternate in one
process, round by round:
  default        nothing set (the folded-constant kernels)
  par_nominal    every parameter row explicitly nominal (the _par kernels)
  dst_zero       zero disturbance rows (the _dst kernels, the arithmetic of par_nominal plus the disturbance terms)
  dst_random     random rows (|a| <= 2 m/s^2, |al| <= 5 rad/s^2), set once
  dst_random_set the same rows, cfnmpc_set_disturbance from a device array before EVERY step; the setter is timed on its own
                 (set_ms) beside the step
--profile adds the kernel means per variant: one child run per variant under `rocprofv3 --kernel-trace --stats` (10 steps after
5 untimed ones), kept apart from the timed runs.  The committed profile is the output of
    python tools/dist_time.py --profile [--batch 65536] [--rounds 3] [--out profiles/dist_time_65536.json]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANTS = "default,par_nominal,dst_zero,dst_random,dst_random_set"


def run(variant, B, steps, warm, d_rand, nominal):
    import torch
    from crazyflie_nmpc_amd import BatchSolver, default_opts, sim
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    from crazyflie_nmpc_amd.synthetic import regulation_row, sample_hover_x0
    N = 50
    rng = np.random.default_rng(1)
    x0 = sample_hover_x0(rng, B, scale=1.0)
    d = {"default": None, "par_nominal": None, "dst_zero": np.zeros((B, 6))}.get(variant, d_rand)
    s = BatchSolver(B, default_opts())
    if variant == "par_nominal":
        s.set_model_params(np.tile(nominal, (B, 1)))
    if d is not None:
        s.set_disturbance(d)
    row = regulation_row()
    s.set_x0(x0); s.set_yref(np.tile(row, (B, N, 1)), np.tile(row[:13], (B, 1))); s.init_iterate(INIT_HOVER)
    dev = torch.device("cuda:0")
    x = torch.tensor(x0, device=dev)
    dt = None if d is None else torch.tensor(d, device=dev)
    u0 = torch.empty((B, 4), dtype=torch.float64, device=dev)
    ms, set_ms, ok = [], [], 0
    for j in range(warm + steps):
        s.set_x0(x)
        torch.cuda.synchronize()
        ts = time.perf_counter()
        if variant == "dst_random_set":
            s.set_disturbance(dt)
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.solve(1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        st, _, _ = s.stats()
        s.get_u(0, out=u0)
        x = sim(x, u0, 0.015, 1, dist=dt) if dt is not None else sim(x, u0, 0.015, 1)
        if j % 3 == 1:
            x[:, 7:10] += 0.3 * torch.randn((B, 3), dtype=torch.float64, device=dev)
        if j >= warm:
            ms.append((t1 - t0) * 1e3)
            set_ms.append((t0 - ts) * 1e3)
            ok += int((st == 0).sum())
    s.close()
    return ms, set_ms, ok / (steps * B)


def profile(variant, B):
    """mean duration [ms] and calls per kernel of one variant (a child process under rocprofv3, 10 timed steps)"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--batch", str(B), "--rounds", "1", "--steps", "10",
               "--variants", variant, "--out", os.path.join(tmp, "t.json")]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        out = {}
        with open(stats[0]) as f:
            for r in csv.DictReader(f):
                name = r["Name"].split("(")[0].replace("cfn::", "")
                out[name] = {"mean_ms": round(float(r["AverageNs"]) * 1e-6, 4), "calls": int(r["Calls"])}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dist_time_65536.json"))
    ap.add_argument("--variants", default=VARIANTS)
    ap.add_argument("--profile", action="store_true", help="kernel means per variant from rocprofv3 child runs")
    a = ap.parse_args()
    from crazyflie_nmpc_amd import NOMINAL_PARAMS
    rng = np.random.default_rng(7)
    d_rand = np.concatenate([rng.uniform(-2.0, 2.0, (a.batch, 3)), rng.uniform(-5.0, 5.0, (a.batch, 3))], axis=1)
    variants = tuple(a.variants.split(","))
    res = {v: {"ms": [], "set_ms": [], "ok": []} for v in variants}
    for _ in range(a.rounds):
        for v in variants:
            ms, set_ms, ok = run(v, a.batch, a.steps, 5, d_rand, NOMINAL_PARAMS)
            res[v]["ms"] += ms
            res[v]["set_ms"] += set_ms
            res[v]["ok"].append(ok)
    out = {"batch": a.batch, "steps_per_round": a.steps, "rounds": a.rounds, "variants": {}}
    for v in variants:
        m = np.array(res[v]["ms"])
        out["variants"][v] = {"mean_ms": float(m.mean()), "median_ms": float(np.median(m)), "max_ms": float(m.max()),
                              "ok_fraction": float(np.mean(res[v]["ok"])), "ms": [round(t, 4) for t in m.tolist()]}
        if v == "dst_random_set":
            out["variants"][v]["set_median_ms"] = float(np.median(res[v]["set_ms"]))
    med = {v: out["variants"][v]["median_ms"] for v in variants}
    for v in variants:
        for base in ("default", "par_nominal"):
            if base in med and v != base and variants.index(v) > variants.index(base):
                out[f"ratio_{v}_vs_{base}_median"] = med[v] / med[base]
    if a.profile:
        out["kernel_ms"] = {v: profile(v, a.batch) for v in variants}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ("variants", "kernel_ms")}))
    for v in variants:
        print(v, {k: round(x, 4) for k, x in out["variants"][v].items() if k != "ms"})


if __name__ == "__main__":
    main()
