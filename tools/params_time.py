"""Step time with per-instance model parameters -> profiles/params_time_65536.json.

65 536 hover instances in the C3-style closed loop (plant = cfnmpc_sim_params with each row's own parameters, velocity kicks
every third step), 20 timed RTI steps per variant after 5 untimed ones.  The variants alternate in one process, round by round:
  default       no parameters set (the folded-constant kernels)
  nominal       every row explicitly nominal (the _par kernels, nominal values)
  random        random rows (mq +-30 %, inertias +-25 %, Ct / Cd +-15 %, l +-10 %)
  random_m2     the same with ERK M = 2
--profile adds the kernel means per variant: one child run per variant under `rocprofv3 --kernel-trace --stats` (10 steps after
5 untimed ones), kept apart from the timed runs.  The committed profile is the output of
    python tools/params_time.py --profile [--batch 65536] [--rounds 3] [--out profiles/params_time_65536.json]"""
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


def random_params(rng, B, nominal):
    p = np.tile(nominal, (B, 1))
    p[:, 1] *= rng.uniform(0.7, 1.3, B)
    p[:, 2:5] *= rng.uniform(0.75, 1.25, (B, 3))
    p[:, 5] *= rng.uniform(0.85, 1.15, B)
    p[:, 6] *= rng.uniform(0.85, 1.15, B)
    p[:, 7] *= rng.uniform(0.9, 1.1, B)
    return p


def run(variant, B, steps, warm, p_rand, nominal):
    import torch
    from crazyflie_nmpc_amd import BatchSolver, default_opts, hover_speed, sim
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    from crazyflie_nmpc_amd.synthetic import regulation_row, sample_hover_x0
    N = 50
    rng = np.random.default_rng(1)
    x0 = sample_hover_x0(rng, B, scale=1.0)
    p = {"default": None, "nominal": np.tile(nominal, (B, 1)), "random": p_rand, "random_m2": p_rand}[variant]
    plant = p if p is not None else np.tile(nominal, (B, 1))
    s = BatchSolver(B, default_opts())
    if variant == "random_m2":
        s.set_erk_steps(2)
    if p is not None:
        s.set_model_params(p)
    row = regulation_row()
    yr = np.tile(row, (B, N, 1))
    yr[:, :, 13:] = hover_speed(plant)[:, None, None]
    s.set_x0(x0); s.set_yref(yr, np.tile(row[:13], (B, 1))); s.init_iterate(INIT_HOVER)
    dev = torch.device("cuda:0")
    x = torch.tensor(x0, device=dev)
    pt = torch.tensor(plant, device=dev)
    u0 = torch.empty((B, 4), dtype=torch.float64, device=dev)
    ms, ok = [], 0
    for j in range(warm + steps):
        s.set_x0(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.solve(1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        st, _, _ = s.stats()
        s.get_u(0, out=u0)
        x = sim(x, u0, 0.015, 1, params=pt)
        if j % 3 == 1:
            x[:, 7:10] += 0.3 * torch.randn((B, 3), dtype=torch.float64, device=dev)
        if j >= warm:
            ms.append((t1 - t0) * 1e3)
            ok += int((st == 0).sum())
    s.close()
    return ms, ok / (steps * B)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "params_time_65536.json"))
    ap.add_argument("--variants", default="default,nominal,random,random_m2")
    ap.add_argument("--profile", action="store_true", help="kernel means per variant from rocprofv3 child runs")
    a = ap.parse_args()
    from crazyflie_nmpc_amd import NOMINAL_PARAMS
    p_rand = random_params(np.random.default_rng(7), a.batch, NOMINAL_PARAMS)
    variants = tuple(a.variants.split(","))
    res = {v: {"ms": [], "ok": []} for v in variants}
    for _ in range(a.rounds):
        for v in variants:
            ms, ok = run(v, a.batch, a.steps, 5, p_rand, NOMINAL_PARAMS)
            res[v]["ms"] += ms
            res[v]["ok"].append(ok)
    out = {"batch": a.batch, "steps_per_round": a.steps, "rounds": a.rounds, "variants": {}}
    for v in variants:
        m = np.array(res[v]["ms"])
        out["variants"][v] = {"mean_ms": float(m.mean()), "median_ms": float(np.median(m)), "max_ms": float(m.max()),
                              "ok_fraction": float(np.mean(res[v]["ok"])), "ms": [round(t, 4) for t in m.tolist()]}
    if "default" in variants:
        d = out["variants"]["default"]["median_ms"]
        for v in variants[1:]:
            out[f"ratio_{v}_vs_default_median"] = out["variants"][v]["median_ms"] / d
    if a.profile:
        out["kernel_ms"] = {v: profile(v, a.batch) for v in variants}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "variants"}))
    for v in variants:
        print(v, {k: round(x, 4) for k, x in out["variants"][v].items() if k != "ms"})


if __name__ == "__main__":
    main()
