"""Time of the differentiable plant rollouts -> profiles/sim_vjp_65536.json.

65 536 vehicles, L = 50, T = 0.015, per-vehicle parameter and disturbance rows (the _dst twins: the most registers), device
tensors throughout.  In ONE process, between HIP events on torch's current stream, warmed up, ALTERNATING rollout / vjp, median of
`--reps`, for steps = 1 and steps = 3 (the recomputation of sub-step start states costs steps (steps - 1) / 2 forward sub-steps
per step):
    sim_rollout        k_sim_rollout_dst: reads x0, u, p, d, writes xs
    sim_rollout_vjp    k_sim_rollout_vjp_dst: reads xs, u, p, d, gxs, writes gx0, gu, gp, gd
    sim (L calls)      k_sim_dst of the same run, one call per step chained through torch tensors, for scale
Reports the vjp / rollout ratio and the achieved bytes per second over the ALGORITHMIC bytes (every array once) beside the fill
rate the same process measures the way tools/hbm_rates.py does.  The layout is instance-major, so a lane's accesses are 104-byte
runs: the ratio of the two rates is what that costs.
python tools/sim_vjp_time.py [--batch 65536] [--L 50] [--reps 20] [--out profiles/sim_vjp_65536.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    return dict(median_ms=float(np.median(v)), mean_ms=float(np.mean(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), n=len(v))


def timed_once(torch, st, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    call()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run(B, L, reps):
    import torch
    import crazyflie_nmpc_amd as cf
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    T = 0.015
    rng = np.random.default_rng(0)
    p = cf.NOMINAL_PARAMS * rng.uniform(0.8, 1.25, (B, 8))
    d = np.concatenate([rng.uniform(-2, 2, (B, 3)), rng.uniform(-5, 5, (B, 3))], axis=1)
    x0 = np.zeros((B, 13)); x0[:, 0:3] = rng.uniform(-1, 1, (B, 3))
    q = np.array([1.0, 0, 0, 0]) + rng.uniform(-0.15, 0.15, (B, 4))
    x0[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    x0[:, 7:10] = rng.uniform(-1, 1, (B, 3)); x0[:, 10:13] = rng.uniform(-2, 2, (B, 3))
    u = cf.hover_speed(p)[:, None, None] + rng.uniform(-3, 3, (B, L, 4))
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)   # noqa: E731
    x0, u, p, d = t(x0), t(u), t(p), t(d)
    gxs = t(rng.uniform(-1, 1, (B, L + 1, 13)))
    xs = torch.empty((B, L + 1, 13), dtype=torch.float64, device=dev)
    outs = (torch.empty((B, 13), dtype=torch.float64, device=dev), torch.empty((B, L, 4), dtype=torch.float64, device=dev),
            torch.empty((B, 8), dtype=torch.float64, device=dev), torch.empty((B, 6), dtype=torch.float64, device=dev))
    ut = [u[:, k].contiguous() for k in range(L)]
    xa, xb = torch.empty_like(x0), torch.empty_like(x0)
    out = {"batch": B, "L": L, "T": T, "reps": reps, "rows": "p + d"}
    # the fill rate of this box (tools/hbm_rates.py's measurement, 1 GiB)
    a = torch.empty((1 << 30) // 8, dtype=torch.float64, device=dev)
    for _ in range(3):
        a.fill_(1.0)
    fill = [timed_once(torch, st, lambda: a.fill_(1.0)) for _ in range(10)]
    rate = a.numel() * 8 / (float(np.median(fill)) * 1e-3)
    out["fill_rate_GBps"] = rate / 1e9
    del a
    ns = B * (L + 1) * 13
    bytes_roll = 8 * (B * 13 + B * L * 4 + B * 14 + ns)
    bytes_vjp = 8 * (2 * ns + B * L * 4 + B * 14 + B * 13 + B * L * 4 + B * 14)
    bytes_sim = 8 * L * B * (13 + 4 + 14 + 13)
    out["algorithmic_bytes"] = dict(sim_rollout=bytes_roll, sim_rollout_vjp=bytes_vjp, sim_calls=bytes_sim)
    for steps in (1, 3):
        def roll():
            cf.sim_rollout(x0, u, T, steps, out=xs, params=p, dist=d)

        def vjp():
            cf.sim_rollout_vjp(xs, u, gxs, T, steps, params=p, dist=d, out=outs)

        def sims():
            cur, nxt = x0, xa
            for k in range(L):
                cf.sim(cur, ut[k], T, steps, out=nxt, params=p, dist=d)
                cur, nxt = nxt, (xb if nxt is xa else xa)
        for _ in range(3):
            roll(); vjp(); sims()
        torch.cuda.synchronize()
        tr, tv, ts = [], [], []
        for _ in range(reps):
            tr.append(timed_once(torch, st, roll))
            tv.append(timed_once(torch, st, vjp))
            ts.append(timed_once(torch, st, sims))
        r = dict(sim_rollout=stats(tr), sim_rollout_vjp=stats(tv), sim_calls=stats(ts))
        r["ratio_vjp_over_rollout"] = r["sim_rollout_vjp"]["median_ms"] / r["sim_rollout"]["median_ms"]
        r["ratio_rollout_over_sim_calls"] = r["sim_rollout"]["median_ms"] / r["sim_calls"]["median_ms"]
        r["achieved_GBps"] = dict(sim_rollout=bytes_roll / (r["sim_rollout"]["median_ms"] * 1e-3) / 1e9,
                                  sim_rollout_vjp=bytes_vjp / (r["sim_rollout_vjp"]["median_ms"] * 1e-3) / 1e9,
                                  sim_calls=bytes_sim / (r["sim_calls"]["median_ms"] * 1e-3) / 1e9)
        r["fraction_of_fill_rate"] = {k: v / out["fill_rate_GBps"] for k, v in r["achieved_GBps"].items()}
        out[f"steps_{steps}"] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--L", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = run(a.batch, a.L, a.reps)
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
