"""Time of the uncertainty propagation and the bound tightening -> profiles/unc_time_65536.json.

65 536 instances in the bench's closed loop (bench.Fleet: hover regulation, staggered kicks, RK4 plant).  After 10 untimed RTI
steps, per step of `--steps` more, each call timed with HIP events on the fleet's stream: the step under the scalar box, then
eval_uncertainty, the read of std_x over [0, N + 1] into a device tensor (one full sweep; the covariance itself too while it
fits: up to 4096 instances) and tighten_box(3, 0.1); every call has run once before the timed window, and the median is
reported beside mean, minimum and maximum.  A second pass times the step under the tightened (per-stage) boxes on the same
box, and a profiled pass gives the engine's own k_factor / forward-sweep durations (cfnmpc_set_profiling) in the same process.  The committed profile
is the output of
    python tools/unc_time.py [--batch 65536] [--steps 30] [--out profiles/unc_time_65536.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(v):
    return dict(median_ms=float(np.median(v)), mean_ms=float(np.mean(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), n=len(v))


def run(B, steps):
    import torch
    import bench
    from test_uncertainty_cpu import random_cov
    dev = torch.device("cuda", 0)
    f = bench.Fleet(B, dev, np.random.default_rng(0))
    s, N = f.solver, f.solver.N
    st = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(1)
    base = random_cov(rng, 64)
    S0 = torch.from_numpy(base[rng.integers(0, 64, B)]).to(dev)
    W = 0.01 * S0
    for _ in range(10):
        f.step()
    bytes0 = s.workspace_bytes
    s.set_uncertainty(S0, W)
    sd0 = torch.empty((B, N + 1, 13), dtype=torch.float64, device=dev)
    for _ in range(2):   # warm-up: every timed call once (first launches, buffer allocations), both box routes
        s.eval_uncertainty()
        s._L.cfnmpc_get_uncertainty(s._h, 0, N + 1, None, C.c_void_p(sd0.data_ptr()), 1, C.c_void_p(st.cuda_stream))
        s.tighten_box(3.0, 0.1)
        f.step()
        s.eval_uncertainty()
        s.tighten_box(0.0, 0.1)
        f.step()
    del sd0
    s.eval_uncertainty()
    nget = min(B, 4096)
    Sg = torch.empty((B, N + 1, 13, 13), dtype=torch.float64, device=dev) if nget == B else None
    sd = torch.empty((B, N + 1, 13), dtype=torch.float64, device=dev)
    t = {k: [] for k in ("step_scalar_box", "eval_uncertainty", "get_std_0_N1", "tighten_box")}
    clamped = 0
    for _ in range(steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        s.tighten_box(0.0, 0.1)                       # the scalar box back in force
        ev[0].record(st)
        f.step()
        ev[1].record(st)
        s.eval_uncertainty()
        ev[2].record(st)
        # (the getter before the tightening: a tightened box changes the QP's data and ends the evaluation)
        rc = s._L.cfnmpc_get_uncertainty(s._h, 0, N + 1, None if Sg is None else C.c_void_p(Sg.data_ptr()), C.c_void_p(sd.data_ptr()), 1,
                                         C.c_void_p(st.cuda_stream))
        ev[3].record(st)
        rc2 = s._L.cfnmpc_tighten_box(s._h, 3.0, 0.1, None, 1, C.c_void_p(st.cuda_stream))
        ev[4].record(st)
        assert rc == 0 and rc2 == 0, (rc, rc2)
        torch.cuda.synchronize()
        for i, k in enumerate(t):
            t[k].append(ev[i].elapsed_time(ev[i + 1]))
        clamped += int(s.tighten_box(3.0, 0.1).sum())
    out = {k: stats(v) for k, v in t.items()}
    out["clamped_entries"] = clamped
    out["workspace_added_bytes"] = int(s.workspace_bytes - bytes0)
    beta = s.backoff()
    out["backoff_1sigma_kRPM"] = dict(min=float(np.nanmin(beta)), median=float(np.nanmedian(beta)), max=float(np.nanmax(beta)))
    # the step under tightened (per-stage) boxes, re-tightened in place before every step
    tt = []
    for _ in range(steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(st)
        f.step()
        ev[1].record(st)
        s.eval_uncertainty()
        s._L.cfnmpc_tighten_box(s._h, 3.0, 0.1, None, 1, C.c_void_p(st.cuda_stream))
        torch.cuda.synchronize()
        tt.append(ev[0].elapsed_time(ev[1]))
    out["step_tightened_boxes"] = stats(tt)
    # the engine's own kernel groups under the scalar box, same process
    s.tighten_box(0.0, 0.1)
    f.step()
    s.set_profiling(True)
    for _ in range(steps):
        f.step()
    torch.cuda.synchronize()
    ms, n = s.get_profile_kernels()
    s.set_profiling(False)
    out["engine_kernels_ms"] = dict(zip(("linearise", "factor", "forward", "compaction", "active_set", "interior_point"), ms), steps=n)
    out["eval_over_k_factor"] = out["eval_uncertainty"]["median_ms"] / ms[1] if ms[1] > 0 else None
    out["tighten_over_forward"] = out["tighten_box"]["median_ms"] / ms[2] if ms[2] > 0 else None
    f.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unc_time_65536.json"))
    a = ap.parse_args()
    res = {"batch": a.batch, "steps": a.steps, "workload": "bench.Fleet closed loop (hover, staggered kicks x 1)", "run": run(a.batch, a.steps)}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
