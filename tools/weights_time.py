"""Step time with per-instance cost weights -> profiles/weights_time_<B>.json.

B hover instances in the closed loop with the bench's kicks (plant = cfnmpc_sim, N(0, 0.3) m/s on the body velocity every third
step), 20 timed RTI steps per variant and round after 5 untimed ones, device-synchronised.  The variants alternate inside one
process, round by round:
  none          no rows set (the uniform kernel arguments: the default step)
  uniform       every row = the uniform weights (the table and the _w twins, same QPs)
  random        random rows, default weights x a factor log-uniform in [1/4, 4] per entry (other QPs: recorded with the share of
                constrained rows, not a cost of the feature)
--parent DIR adds the A/B against a build of another commit (a checkout with its library built in DIR): per round two child
processes of DIR's package and one of this one, variant none each, alternating -- `parent_a` against `parent_b` is the spread
of the comparison, `child_none` against both is the comparison.
--profile adds the kernel means per variant: one child run per variant under `rocprofv3 --kernel-trace --stats`, kept apart
from the timed runs.
    python tools/weights_time.py [--batch 65536] [--rounds 3] [--parent DIR] [--profile]"""
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


def run(variant, B, steps, warm):
    import torch
    from crazyflie_nmpc_amd import BatchSolver, default_opts, sim
    from crazyflie_nmpc_amd.solver import INIT_HOVER
    from crazyflie_nmpc_amd.synthetic import regulation_row, sample_hover_x0
    N = 50
    rng = np.random.default_rng(1)
    x0 = sample_hover_x0(rng, B, scale=1.0)
    o = default_opts()
    s = BatchSolver(B, o)
    W, WN = np.array(o.W), np.array(o.WN)
    if variant == "uniform":
        s.set_weights_batch(np.tile(W, (B, 1)), np.tile(WN, (B, 1)))
    elif variant == "random":
        wr = np.random.default_rng(7)
        s.set_weights_batch(W * np.exp(wr.uniform(np.log(0.25), np.log(4.0), (B, 17))),
                            WN * np.exp(wr.uniform(np.log(0.25), np.log(4.0), (B, 13))))
    row = regulation_row()
    s.set_x0(x0); s.set_yref(np.tile(row, (B, N, 1)), np.tile(row[:13], (B, 1))); s.init_iterate(INIT_HOVER)
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    x = torch.tensor(x0, device=dev)
    u0 = torch.empty((B, 4), dtype=torch.float64, device=dev)
    ms, ok, con = [], 0, 0
    for j in range(warm + steps):
        s.set_x0(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.solve(1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        st, it, _ = s.stats()
        s.get_u(0, out=u0)
        x = sim(x, u0, 0.015, 1)
        if j % 3 == 1:
            x[:, 7:10] += 0.3 * torch.randn((B, 3), dtype=torch.float64, device=dev)
        if j >= warm:
            ms.append((t1 - t0) * 1e3)
            ok += int((st == 0).sum())
            con += int((it > 0).sum())
    s.close()
    return ms, ok / (steps * B), con / (steps * B)


def child(root, variant, B, steps):
    """one variant in a process of its own, with the package of `root` -> (ms, ok, constrained)"""
    root = os.path.abspath(root)
    env = dict(os.environ, PYTHONPATH=root)
    env.pop("CFNMPC_LIB", None)
    pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", variant, "--batch", str(B), "--steps", str(steps)],
                        capture_output=True, text=True, timeout=600, env=env, cwd=root)
    if pr.returncode != 0:
        raise RuntimeError(f"child run with the package of {root} failed ({pr.returncode}):\n{pr.stderr[-2000:]}")
    r = json.loads(pr.stdout.strip().splitlines()[-1])
    return r["ms"], r["ok"], r["con"]


def profile(variant, B):
    """mean duration [ms] and calls per kernel of one variant (a child process under rocprofv3, 10 timed steps)"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", variant, "--batch", str(B), "--steps", "10"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600,
                       env=dict(os.environ, PYTHONPATH=ROOT))
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--variants", default="none,uniform,random")
    ap.add_argument("--parent", default=None, help="checkout of another commit with its library built: same-call A/B of the default step")
    ap.add_argument("--profile", action="store_true", help="kernel means per variant from rocprofv3 child runs")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        ms, ok, con = run(a.child, a.batch, a.steps, 5)
        print(json.dumps({"ms": ms, "ok": ok, "con": con}))
        return
    sys.path.insert(0, ROOT)
    variants = tuple(a.variants.split(","))
    names = list(variants) + (["parent_a", "parent_b", "child_none"] if a.parent else [])
    res = {v: {"ms": [], "ok": [], "con": []} for v in names}
    for _ in range(a.rounds):
        todo = [(v, None) for v in variants]
        if a.parent:
            todo += [("parent_a", a.parent), ("child_none", ROOT), ("parent_b", a.parent)]
        for v, root in todo:
            ms, ok, con = run(v, a.batch, a.steps, 5) if root is None else child(root, "none", a.batch, a.steps)
            res[v]["ms"] += ms
            res[v]["ok"].append(ok)
            res[v]["con"].append(con)
    out = {"batch": a.batch, "steps_per_round": a.steps, "rounds": a.rounds, "variants": {}}
    for v in names:
        m = np.array(res[v]["ms"])
        out["variants"][v] = {"mean_ms": float(m.mean()), "median_ms": float(np.median(m)), "max_ms": float(m.max()),
                              "ok_fraction": float(np.mean(res[v]["ok"])), "constrained_fraction": float(np.mean(res[v]["con"])),
                              "ms": [round(t, 4) for t in m.tolist()]}
    med = {v: out["variants"][v]["median_ms"] for v in names}
    if "none" in med:
        for v in variants[1:]:
            out[f"ratio_{v}_vs_none_median"] = med[v] / med["none"]
    if a.parent:
        out["ratio_parent_b_vs_parent_a_median"] = med["parent_b"] / med["parent_a"]
        out["ratio_child_none_vs_parent_median"] = med["child_none"] / (0.5 * (med["parent_a"] + med["parent_b"]))
    if a.profile:
        out["kernel_ms"] = {v: profile(v, a.batch) for v in variants}
    path = a.out or os.path.join(ROOT, "profiles", f"weights_time_{a.batch}.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "variants"}))
    for v in names:
        print(v, {k: round(x, 4) for k, x in out["variants"][v].items() if k != "ms"})


if __name__ == "__main__":
    main()
