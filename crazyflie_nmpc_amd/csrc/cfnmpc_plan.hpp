// cfnmpc_plan.hpp -- a solver's options resolved into one plan: every range check and refusal of cfnmpc_create and the ONE place
// where the kernel structure is chosen from fleet size, horizon and the device's SIMD count.  Plain C++,
// free of HIP: tools/host_plan_check.cpp runs a table of options -> plan or refusal through it under the host sanitizers
// (make host_plan_check, tests/test_host_plan_cpu.py).  Internal to the library.
#pragma once
#include "../../include/cfnmpc.h"

namespace cfn {

constexpr int PLAN_COND_MMAX = 10;   // longest condensed block; = COND_MMAX of cfnmpc_ws.hpp (asserted in cfnmpc_api.cpp)

// What cfnmpc_create copies into Params and the solver.  Nothing here owns anything.
struct Plan {
    // internal: 0 = monolithic k_as, -1 = every solve in one launch on the compact z store + commit, -2 = the monolithic
    // kernel's solves + commit, p > 0 = p single-solve passes
    int as_passes = 0;
    int as_dense = 0;        // head-condensed dense active-set solves (cfnmpc_asdense.hip) beside the solves + commit structure
    int forward_rg = 0;      // forward sweep of the start solve on the stored blocks (row groups)
    int fused = 0;           // start solve: 0 = stored blocks, 1 = k_linfactor, 2 = k_linfactor for the factorisation only
    int fwd_split = 0;       // split forward sweep, WANTED: 24 or 0 (it runs only if the second side stream exists)
    int ipm_listed = 0;      // fall-back rows compacted before the interior point
    int as_grid = 0;         // wavefronts per pass launch: two per SIMD of the device
    int as_sparse_max = 0;   // one constrained row per wave while they all fit at once: the SIMDs of the device
    int cond_N2 = 0, cond_M = 0, cond_rem = 0;   // partial condensing (cond_N2 normalised: 0 = off)
    int v4b = 1;             // home 4-vectors wave-blocked (the condensed kernels index theirs instance-major)
    int ab16 = 1;            // home A, B, b grouped by 16 blocks (cfnmpc_rg.hpp: abidx)
    int clist_chunks = 0;    // workgroups per 64-slot group of k_linearise_clist
    int chunks_all = 1, chunks_list = 10;   // workgroups per 64-instance group in the two linearisation passes
    int active_horizon = 0, active_set = 0, as_warm = 0;
    int use_graph = 0, reinit_failed = 0, overlap = 0;   // host side: captured step, cfnmpc_opts.reinit_failed, overlapped preparation
    int wants_side_streams = 0;   // the dense structure: k_as_solves (and part two of a split sweep) beside k_as_dense
};

// Q may be positive SEMI-definite (the reference's dynamic_reconfigure ranges start at 0.0,
// config/crazyflie_params.cfg:19-35): state weights >= 0, input weights > 0 (R must be definite:
// S = R + B'PB is what the Riccati recursion inverts); no NaN.
inline bool weights_ok(const double* W, const double* WN) {
    if (W) {
        for (int i = 0; i < 13; i++) if (!(W[i] >= 0.0)) return false;
        for (int i = 13; i < 17; i++) if (!(W[i] > 0.0)) return false;
    }
    if (WN) for (int i = 0; i < 13; i++) if (!(WN[i] >= 0.0)) return false;
    return true;
}

// Kernel choices that depend on how the fleet fills the device, in units of its SIMDs (S = 4 x compute units = wave slots at
// one wave per SIMD; MI355X: 1024) -- measured per horizon, profiles/r04_thresholds.md (tools/threshold_sweep.py):
//   * forward sweep on the stored blocks (row groups, B / 4 waves) instead of the matrix-free one (B / 64 waves of N
//     sequential stages): while B / 4 waves fit about twice on the SIMDs; the row-group sweep streams 240 N doubles per
//     instance, so long horizons leave it earlier (cross-over 7000 instances at N = 30 and 50, 5500 at N = 100);
//   * active-set solves + commit kernel instead of the monolithic kernel: while the ~8 % constrained rows make fewer
//     waves than there are SIMDs by a margin (roll-out = latency chain); re-measured after the 4-vector layout change:
//     N = 50: -3.5 % at 24 S, -0.5 % at 32 S, equal at 48 S; N = 100: -3.6 % up to 32 S, equal at 48 S; N = 30: +4.7 % from 24 S on;
//   * fall-back rows compacted before the interior point: from 16 S instances;
//   * head-condensed dense active-set solves (k_as_dense) for the rows with heads of at most 16 stages: below 18 S instances
//     (round 5, one box, A/B per size: 2 S +20.6 %, 4 S +8.5 %, 8 S +9.6 %, 12 S +1.8 %, 16 S +1.1 %, 20 S -1.8 %, 24 S -1.4 %,
//     28 S -0.5 %, 32 S -5 %: one row per wavefront and SIMD -- while the ~8 % constrained rows fit the SIMDs once the kernel lasts
//     as long as its hardest row, 50 - 90 us instead of 220; beyond that its ~47 us per row are rounds of waves and the four
//     rows per wavefront of k_as_solves / k_as win on throughput), profiles/r05_as_dense.md;
//   * split forward sweep (k_forward_p1 | k_forward_p2 beside the constrained rows' kernels): wherever that structure runs with the
//     matrix-free sweep (one box: 6144 instances +3.5 % against the unsplit matrix-free sweep and +2 % against the row-group one,
//     8192: +7.2 %, 12 288: +1.2 %, 16 384: +0.7 %; at 4096 the row-group sweep stays ahead, 7.33 against 6.75 M).
struct Choice { bool forward_rg, as_commit, ipm_listed, as_dense, forward_split; };
inline Choice choose_kernels(int batch, int N, int simds) {
    const long S = simds > 0 ? simds : 1024;
    Choice c;
    c.forward_rg = (long)batch < 6 * S;   // (round 5: 8 S -> 6 S for N <= 64 too -- the split matrix-free sweep beats the row-group one from 6 S on: 9.37 against 9.18 M at 6144 instances)
    c.as_commit = (long)batch < (N <= 40 ? 20 : 36) * S;
    c.ipm_listed = (long)batch >= 16 * S;
    c.as_dense = (long)batch < 18 * S;
    c.forward_split = true;
    return c;
}

// The caller's options (complete: cfnmpc_host.hpp, take_opts) for a fleet of `batch` instances on a device of `simds` SIMDs ->
// the plan, or CFNMPC_EINVAL with *out untouched.  `overlap`: the overlapped preparation of the development build (0 in the
// product).  Touches nothing but its arguments.
inline int resolve_plan(const cfnmpc_opts& o, int batch, int simds, int overlap, Plan* out) {
    if (!out || batch <= 0) return CFNMPC_EINVAL;
    if (o.N < 5 || o.N > 4096 || !(o.dt > 0) || !(o.u_max > o.u_min) || o.max_iter < 0 ||
        !(o.ah_margin >= 0.0 && o.ah_margin < 0.5) || o.ah_extra < 0) return CFNMPC_EINVAL;
    // QP parameters that would otherwise only show up as NaN / status 4 at run time
    if (!(o.tol > 0.0) || !(o.tau > 0.0 && o.tau < 1.0) || !(o.thr0 > 0.0) || !(o.lam0_min > 0.0) ||
        !(o.mu0_scale >= 0.0) || !(o.ipm_clip_viol >= 0.0) || !(o.ipm_clip_margin > 0.0 && o.ipm_clip_margin < 0.5) ||
        !(o.as_skip_viol >= 0.0)) return CFNMPC_EINVAL;
    if (!weights_ok(o.W, o.WN)) return CFNMPC_EINVAL;
    // partial condensing: cond_N2 blocks of at most PLAN_COND_MMAX stages; not combined with the overlapped preparation
    if (o.cond_N2 < 0 || o.cond_N2 > o.N) return CFNMPC_EINVAL;
    const int cond_N2 = (o.cond_N2 == 0 || o.cond_N2 == o.N) ? 0 : o.cond_N2;
    if (cond_N2 && ((o.N + cond_N2 - 1) / cond_N2 > PLAN_COND_MMAX || overlap)) return CFNMPC_EINVAL;
    Plan p;
    p.overlap = overlap ? 1 : 0;
    p.use_graph = o.step_graph ? 1 : 0;
    p.reinit_failed = o.reinit_failed ? 1 : 0;
    const Choice pick = choose_kernels(batch, o.N, simds);
    // the shooting intervals of a 64-instance group are independent: spread them over enough
    // workgroups to fill the 1024 SIMDs when the batch alone does not (a single instance then
    // linearises its 50 intervals in parallel instead of one after the other)
    {
        // k_linearise runs one wavefront per SIMD: a launch of groups x c workgroups takes ceil(groups c / SIMDs) rounds of
        // ceil(N / c) stages each (+ a prologue per workgroup) -- take the c that minimises it (rounding groups c UP past the
        // number of SIMDs would cost a whole second round: 255 groups x 5 chunks = 1275 workgroups ran 35 % slower than x 4)
        const int groups = (batch + 63) / 64;
        int c = 1;
        if (p.overlap) {
            c = 5;
            if (groups * c < simds) c = (simds + groups - 1) / groups;
        } else {
            double best = 1e300;
            for (int cc = 1; cc <= o.N; cc++) {
                const long rounds = ((long)groups * cc + simds - 1) / simds;
                const double cost = (double)rounds * ((o.N + cc - 1) / cc + 0.35);   // 0.35 stage-equivalents of prologue per workgroup
                if (cost < best - 1e-9) { best = cost; c = cc; }
            }
        }
        p.chunks_all = c < 1 ? 1 : (c > o.N ? o.N : c);
    }
    p.active_horizon = o.active_horizon ? 1 : 0;
    p.active_set = o.active_set ? 1 : 0;
    p.as_warm = (o.as_warm && o.active_set) ? 1 : 0;
    if (o.forward_sweep < 0 || o.forward_sweep > 2 || (o.step_graph && overlap) || (o.reinit_failed && overlap)) return CFNMPC_EINVAL;
#ifdef CFN_DEV   // (development builds: also -2 and 1..12, the instance-contiguous store / level-synchronous passes of round 3)
    if (o.as_passes < -3 || o.as_passes > 12) return CFNMPC_EINVAL;
#else
    if (o.as_passes != 0 && o.as_passes != -1 && o.as_passes != -3) return CFNMPC_EINVAL;
#endif
    p.as_passes = o.as_passes > 0 ? o.as_passes : (o.as_passes == -2 ? -1 : (o.as_passes == -3 ? -2 : 0));
    if (o.as_passes == 0 && pick.as_commit && o.start_solve != 2) p.as_passes = -2;   // small fleets: solves + commit kernel (measured); the commit kernel reads stored blocks
    p.as_grid = 2 * simds;   // pass launches: two wavefronts per SIMD of this device
    // one fall-back row per wave is as fast as four while those waves fit one per SIMD (1024 rows: 1.6 % of 65 536 instances,
    // 2.5 % fall back at three times the bench's disturbances): only large fleets pay the compaction's extra launch
    p.as_sparse_max = p.as_grid / 2;
    p.ipm_listed = pick.ipm_listed ? 1 : 0;
    // head-condensed dense active-set solves beside the solves + commit structure; scalar box, stored blocks
    if (o.as_dense < -1 || o.as_dense > 1 || o.start_solve < 0 || o.start_solve > 3 || o.forward_split < -1 || o.forward_split > 1) return CFNMPC_EINVAL;
    if (o.as_dense == 1 && (p.as_passes != -2 && o.as_passes != 0)) return CFNMPC_EINVAL;
    if (o.as_dense == 1 && o.as_passes == 0 && o.start_solve != 2 && !cond_N2) p.as_passes = -2;   // asked for: the structure it lives in
    p.as_dense = (p.as_passes == -2 && p.active_set && !p.as_warm && o.as_dense != -1 && (o.as_dense == 1 || pick.as_dense)) ? 1 : 0;
    // an EXPLICIT request that cannot be honoured is refused, not dropped (as_dense = 1 beside start_solve = 2, cond_N2, as_warm or
    // active_set = 0; forward_split = 1 outside the dense structure, with the row-group sweep, short horizons or the overlapped
    // preparation -- whose early pass would read the iterate while part two of the sweep is still writing it)
    if (o.as_dense == 1 && !p.as_dense) return CFNMPC_EINVAL;
    const bool split_ok = p.as_dense && !cond_N2 && o.start_solve != 2 && o.start_solve != 3 && o.N >= 40 && !overlap &&
                          o.forward_sweep != 2 && o.forward_split != -1;
    if (o.forward_split == 1 && !split_ok) return CFNMPC_EINVAL;
    // forward sweep on the stored blocks (row groups) below 6 S instances where the split matrix-free sweep takes over from there;
    // where it cannot run (short horizons, no dense structure, ...) the unsplit matrix-free sweep wins from 8 S on only
    // (an explicitly fused start solve stores no stage blocks: the automatic choice then stays with the matrix-free sweep)
    {
        const bool auto_rg = split_ok ? pick.forward_rg : (long)batch < 8L * simds;
        p.forward_rg = o.forward_sweep == 2 || (o.forward_sweep == 0 && auto_rg && o.start_solve != 2 && !(o.forward_split == 1)) ? 1 : 0;
    }
    // side streams of the rows with long heads and of part two of a split sweep (launch_qp_ipm); without them the kernels simply
    // run one after the other
    p.wants_side_streams = p.as_dense;
    // start solve: the fused kernel replaces k_linearise + k_factor where nothing but the constrained instances' QP kernels
    // reads the stage blocks afterwards (matrix-free forward sweep, monolithic active-set kernel, no partial condensing,
    // no overlapped preparation); per-stage boxes (cfnmpc_set_box_stages) switch a solver back at launch time
    {
        const bool can_fuse = !cond_N2 && !overlap && !p.forward_rg && p.as_passes == 0;
        if (o.start_solve == 2 && !can_fuse) return CFNMPC_EINVAL;
        if (o.start_solve == 3 && (cond_N2 || overlap)) return CFNMPC_EINVAL;
        p.fused = o.start_solve == 2 ? 1 : (o.start_solve == 3 ? 2 : 0);
        p.clist_chunks = o.N >= 10 ? 10 : o.N;
    }
    // split forward sweep: lives in the dense structure (two side streams), matrix-free sweep, horizons that reach well behind H
    p.fwd_split = (split_ok && !p.forward_rg && p.fused == 0 && (o.forward_split == 1 || pick.forward_split)) ? 24 : 0;
    p.cond_N2 = cond_N2;
    p.v4b = cond_N2 ? 0 : 1;
    p.cond_M = cond_N2 ? o.N / cond_N2 : 0;
    p.cond_rem = cond_N2 ? o.N % cond_N2 : 0;
    *out = p;
    return CFNMPC_OK;
}

}  // namespace cfn
