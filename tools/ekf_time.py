"""Time of the batched extended Kalman filter step -> profiles/ekf_time.json.

4096 and 65 536 vehicles, T = 0.015, device tensors throughout, in ONE process, between HIP events on torch's current stream,
warmed up, ALTERNATING the calls, median of `--reps`, for steps = 1 and steps = 3 and for the three kernel twins (rows none | p |
p + d):
    ekf predict        k_ekf*: predict only (z = None), with Q
    ekf step           k_ekf*: predict and the update of the reference node's ten measured components, gate 5, normalisation
    sim                k_sim* of the same inputs and the same `steps`, for scale (the plant step alone)
Reports the achieved bytes per second of the full step over its ALGORITHMIC bytes (every array once: x, P, u, rows, Q, z, r in;
x, P, nis, counts out) beside the fill rate the same process measures the way tools/hbm_rates.py does.
python tools/ekf_time.py [--batches 4096,65536] [--reps 20] [--out profiles/ekf_time.json]"""
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


def run(B, reps, torch, cf, dev, st):
    T = 0.015
    rng = np.random.default_rng(0)
    p = cf.NOMINAL_PARAMS * rng.uniform(0.8, 1.25, (B, 8))
    d = np.concatenate([rng.uniform(-2, 2, (B, 3)), rng.uniform(-5, 5, (B, 3))], axis=1)
    x = np.zeros((B, 13)); x[:, 0:3] = rng.uniform(-1, 1, (B, 3))
    q = np.array([1.0, 0, 0, 0]) + rng.uniform(-0.15, 0.15, (B, 4))
    x[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    x[:, 7:10] = rng.uniform(-1, 1, (B, 3)); x[:, 10:13] = rng.uniform(-2, 2, (B, 3))
    u = cf.hover_speed(p)[:, None] + rng.uniform(-3, 3, (B, 4))
    sig = np.repeat([0.05, 0.02, 0.2, 0.3], [3, 4, 3, 3])
    Lw = (np.tril(rng.uniform(-0.3, 0.3, (B, 13, 13)), -1) + np.eye(13)) * sig[None, :, None]
    P = Lw @ np.swapaxes(Lw, 1, 2)
    Q = np.tile(np.diag((0.02 * sig) ** 2), (B, 1, 1))
    r = np.tile(np.repeat([1e-3, 1e-2, -1.0, 3e-2], [3, 4, 3, 3]) ** 2 * np.repeat([1.0, 1.0, -1.0, 1.0], [3, 4, 3, 3]), (B, 1))
    z = x + np.sqrt(np.abs(r)) * rng.standard_normal((B, 13))
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)   # noqa: E731
    x, u, p, d, P, Q, z, r = (t(a) for a in (x, u, p, d, P, Q, z, r))
    outs = (torch.empty_like(x), torch.empty_like(P), torch.empty(B, dtype=torch.float64, device=dev),
            torch.empty((B, 2), dtype=torch.int32, device=dev))
    xs = torch.empty_like(x)
    out = {"batch": B, "T": T, "reps": reps}
    for steps in (1, 3):
        for name, pp, dd in (("none", None, None), ("p", p, None), ("pd", p, d)):
            def predict():
                cf.ekf_step(x, P, u, Q=Q, T=T, steps=steps, params=pp, dist=dd, out=outs)

            def step():
                cf.ekf_step(x, P, u, z=z, r=r, Q=Q, T=T, steps=steps, gate=5.0, params=pp, dist=dd, out=outs)

            def sim():
                cf.sim(x, u, T, steps, out=xs, params=pp, dist=dd)
            for _ in range(3):
                predict(); step(); sim()
            torch.cuda.synchronize()
            tp, tf, ts = [], [], []
            for _ in range(reps):
                tp.append(timed_once(torch, st, predict))
                tf.append(timed_once(torch, st, step))
                ts.append(timed_once(torch, st, sim))
            rows = (8 if pp is not None else 0) + (6 if dd is not None else 0)
            nbytes = 8 * B * (13 + 169 + 4 + rows + 169 + 26 + 13 + 169 + 1 + 1)
            e = dict(ekf_predict=stats(tp), ekf_step=stats(tf), sim=stats(ts), algorithmic_bytes_step=nbytes)
            e["achieved_GBps_step"] = nbytes / (e["ekf_step"]["median_ms"] * 1e-3) / 1e9
            e["ratio_step_over_sim"] = e["ekf_step"]["median_ms"] / e["sim"]["median_ms"]
            out[f"steps_{steps}_{name}"] = e
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,65536")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import crazyflie_nmpc_amd as cf
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    # the fill rate of this box (tools/hbm_rates.py's measurement, 1 GiB)
    buf = torch.empty((1 << 30) // 8, dtype=torch.float64, device=dev)
    for _ in range(3):
        buf.fill_(1.0)
    fill = [timed_once(torch, st, lambda: buf.fill_(1.0)) for _ in range(10)]
    out = {"fill_rate_GBps": buf.numel() * 8 / (float(np.median(fill)) * 1e-3) / 1e9}
    del buf
    for B in (int(b) for b in a.batches.split(",")):
        out[f"batch_{B}"] = run(B, a.reps, torch, cf, dev, st)
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
