"""Time of the disturbance-augmented filter step -> profiles/ekf_aug_time.json.

4096 and 65 536 vehicles, T = 0.015, device tensors throughout, in ONE process, between HIP events on torch's current stream,
warmed up, ALTERNATING the calls, median of `--reps`, for steps = 1 and steps = 3 (per-vehicle parameter rows, sel = (0, 1, 2)):
    aug predict        k_ekf_aug: predict only (z = None), with Q and Qd
    aug step           k_ekf_aug: predict and the update of the reference node's ten measured components, gate 5, normalisation
    ekf step           k_ekf_dst: ekf_step(.., dist=d) on the same state, inputs, rows and measurement (the 13-state sibling)
No threshold: the figures and the same-run ratio aug step / ekf step are what DESIGN.md section 5.27 reports.
python tools/ekf_aug_time.py [--batches 4096,65536] [--reps 20] [--out profiles/ekf_aug_time.json]"""
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
    T, sel = 0.015, (0, 1, 2)
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
    Pa = cf.ekf_aug_cov(P, [0.5, 0.5, 0.5])
    Q = np.tile(np.diag((0.02 * sig) ** 2), (B, 1, 1))
    Qd = np.full((B, 3), 1e-6)
    r = np.tile(np.repeat([1e-3, 1e-2, -1.0, 3e-2], [3, 4, 3, 3]) ** 2 * np.repeat([1.0, 1.0, -1.0, 1.0], [3, 4, 3, 3]), (B, 1))
    z = x + np.sqrt(np.abs(r)) * rng.standard_normal((B, 13))
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)   # noqa: E731
    x, u, p, d, P, Pa, Q, Qd, z, r = (t(a) for a in (x, u, p, d, P, Pa, Q, Qd, z, r))
    nis = torch.empty(B, dtype=torch.float64, device=dev)
    counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
    outs = (torch.empty_like(x), torch.empty_like(P), nis, counts)
    outs_a = (torch.empty_like(x), torch.empty_like(d), torch.empty_like(Pa), nis, counts)
    Pxx = torch.empty_like(P)
    out = {"batch": B, "T": T, "reps": reps, "sel": list(sel)}
    for steps in (1, 3):
        def predict():
            cf.ekf_aug_step(x, d, Pa, u, sel, Q=Q, Qd=Qd, T=T, steps=steps, params=p, out=outs_a, Pxx_out=Pxx)

        def step():
            cf.ekf_aug_step(x, d, Pa, u, sel, z=z, r=r, Q=Q, Qd=Qd, T=T, steps=steps, gate=5.0, params=p, out=outs_a, Pxx_out=Pxx)

        def sibling():
            cf.ekf_step(x, P, u, z=z, r=r, Q=Q, T=T, steps=steps, gate=5.0, params=p, dist=d, out=outs)
        for _ in range(3):
            predict(); step(); sibling()
        torch.cuda.synchronize()
        tp, tf, ts = [], [], []
        for _ in range(reps):
            tp.append(timed_once(torch, st, predict))
            tf.append(timed_once(torch, st, step))
            ts.append(timed_once(torch, st, sibling))
        # every array once: x, d, Pa, u, p, Q, Qd, z, r in; x, d, Pa, Pxx, nis, counts out
        nbytes = 8 * B * (13 + 6 + 256 + 4 + 8 + 169 + 3 + 26 + 13 + 6 + 256 + 169 + 1 + 1)
        e = dict(aug_predict=stats(tp), aug_step=stats(tf), ekf_step=stats(ts), algorithmic_bytes_step=nbytes)
        e["achieved_GBps_step"] = nbytes / (e["aug_step"]["median_ms"] * 1e-3) / 1e9
        e["ratio_aug_step_over_ekf_step"] = e["aug_step"]["median_ms"] / e["ekf_step"]["median_ms"]
        out[f"steps_{steps}"] = e
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
    out = {}
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
