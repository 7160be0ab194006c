// cfnmpc_unc.hpp -- uncertainty propagation and robust input-bound tightening (cfnmpc_eval_uncertainty / cfnmpc_get_backoff /
// cfnmpc_get_uncertainty / cfnmpc_tighten_box).  Included at the end of cfnmpc_kernels.hip (its
// primitives, no device unit of its own).
//
// Zero-order robust optimisation: a state covariance carried along the horizon through the closed-loop linearisation of the last
// QP, and every input bound backed off by a multiple of the standard deviation of the feedback's input correction:
//     M_k = A_k - B_k K_k;   Sigma_{k+1} = M_k Sigma_k M_k' + W;   beta_{k,a} = sqrt((K_k Sigma_k K_k')_aa)      k = 0 .. N-1
// on the stored home blocks (AR, BR) and the home gains KR of the start solve -- or one constant user gain per instance --, in
// du = -K dx.  The forward, two-sided sibling of k_sens_fwd (cfnmpc_sens.hpp).  Kernels:
//   k_unc_prop     row groups (cfnmpc_ws.hpp), every row: lane i < 13 holds row i of Sigma_k.  Per stage
//                    U = K Sigma            lanes a < 4, one dotbc<13, 0> per column (as k_sens_fwd's u)
//                    beta_a^2 = U_a . K_a   lane-local in the lanes a < 4
//                    Y = A Sigma - B U      k_sens_fwd's inner body on Sigma's columns (A's 97-entry sparsity)
//                    M = A - B K            row i in lane i (the gain's entries broadcast from the lanes a < 4)
//                    Sigma+ = Y M' + W      13 rank1bc<13>: the entries of M are the broadcast source
//                  (169 + 182 + 52 + 169 broadcast FMAs and the 13 lane-local ones of beta: 585 FMAs per stage and wave).  One launch over [0, N) writes beta only
//                  (cfnmpc_eval_uncertainty); the getter's sweep over [0, stage + n_stages) writes Sigma and the square roots
//                  of its diagonal for the requested window, in the public state order.  Nothing of Sigma is kept between calls.
//   k_unc_tighten  one thread per [instance][stage][input]: nominal box + beta -> the per-stage box arrays in force and their
//                  compact copies, with the clamp, the equality rule and the per-instance count of clamped entries.
//   k_unc_put_sym / k_unc_put_gain   the caller's [B][13][13] / [B][4][13] arrays (public order) -> the tables below.
// Nothing here writes a field of Params except, in k_unc_tighten, the box arrays cfnmpc_set_box_stages owns.
#pragma once

namespace cfn {

// Sigma0 / W tables: a row-distributed 13 x 13 per instance, [wave][col j][inst & 3][row] (SZ_P per wave), internal order
__device__ __forceinline__ size_t unc_sym_at(int inst, int r, int c) { return (size_t)(inst >> 2) * SZ_P + (c * 4 + (inst & 3)) * 13 + r; }

__global__ __launch_bounds__(256) void k_unc_put_sym(int B, const double* __restrict__ src, double* __restrict__ tab) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)B * 169) return;
    const int i = (int)(e / 169), r = (int)(e % 169) / 13, c = (int)(e % 169) % 13;
    tab[unc_sym_at(i, int_of(r), int_of(c))] = src[e];
}
// user gain [B][4][13] (columns in the public order) -> KR's block layout with one stage per block
__global__ __launch_bounds__(256) void k_unc_put_gain(int B, const double* __restrict__ src, double* __restrict__ tab) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)B * 52) return;
    const int i = (int)(e / 52), a = (int)(e % 52) / 13, c = (int)(e % 52) % 13;
    tab[(size_t)(i >> 2) * SZ_K + (int_of(c) * 4 + (i & 3)) * 4 + a] = src[e];
}

// row L of an instance's table entry (nullptr: zero)
__device__ __forceinline__ void unc_ld_sym(const double* tab, const Lane& t, double (&S)[13]) {
    if (tab) {   // (wave-uniform)
        const gdouble* b = gm(tab) + (size_t)t.wave * SZ_P;
        SFOR(j, 0, 13, {
            const double v = b[(j * 4 + t.q) * 13 + imin(t.L, 12)];
            S[j] = t.L < 13 ? v : 0.0;
        });
    } else {
        SFOR(j, 0, 13, { S[j] = 0.0; });
    }
}

// the sweep over the stages [0, s0 + ns) for the rows [b0, b0 + nb) (wave-aligned: b0 % 4 == 0)
__global__ __launch_bounds__(64, 2) void k_unc_prop(Params P, UncArgs A) {
    Lane t;
    t.L = threadIdx.x & 15;
    t.row = threadIdx.x >> 4;
    t.q = t.row;
    t.wave = A.b0 / 4 + blockIdx.x;
    t.inst = t.wave * 4 + t.q;
    t.home = t.inst;
    t.valid = t.inst < P.B && t.inst < A.b0 + A.nb;
    t.wu = 0.0;
    const bool bad = t.valid && A.status[t.inst] == 4;
    const double nan = __builtin_nan("");
    const int kend = A.s0 + A.ns;           // last output stage + 1 (<= N + 1)
    const int kf = imin(kend, P.N);         // stages with a feedback law
    const size_t ob = (size_t)(t.inst - A.b0);
    const int eL = ext_of(imin(t.L, 12));
    double S[13];
    unc_ld_sym(A.S0, t, S);
    for (int k = 0; k < kf; k++) {
        double kr[13], ar[10], br[4];
        if (A.Ku) ld_cols4(blk(A.Ku, t, 1, 0, SZ_K), t, kr);   // (wave-uniform)
        else ld_cols4(blk(P.KR, t, P.N, k, SZ_K), t, kr);
        ld_ar(blkab(P, P.AR, t, k, SZ_A), t, ar);
        ld_rows4(blkab(P, P.BR, t, k, SZ_B), t, br);
        const bool out = t.valid && k >= A.s0 && t.L < 13;
        if (out && A.Sig) {
            double* sg = A.Sig + ((ob * A.ns + (k - A.s0)) * 13 + eL) * 13;
            SFOR(j, 0, 13, { sg[ext_of(j)] = bad ? nan : S[j]; });
        }
        if (out && A.sd) {
            double dg = 0.0;
            SFOR(j, 0, 13, { dg = (t.L == j) ? S[j] : dg; });
            A.sd[(ob * A.ns + (k - A.s0)) * 13 + eL] = bad ? nan : sqrt(fmax(dg, 0.0));
        }
        // U = K Sigma (lanes a < 4), beta^2 = diag(U K'), Y = A Sigma - B U
        double Y[13], b2 = 0.0;
        SFOR(j, 0, 13, {
            double acc = 0.0;
            dotbc<13, 0>(acc, kr, S[j]);
            b2 = __builtin_fma(acc, kr[j], b2);
            double u = -acc;
            settle(u);
            double vr[4];
            SFOR(a, 0, 4, { vr[a] = bc<a>(u); });
            double y = t.L < 3 ? S[j] : 0.0;
            dotbc<10, 3>(y, ar, S[j]);
            SFOR(a, 0, 4, { y = __builtin_fma(br[a], vr[a], y); });
            Y[j] = y;
        });
        if (A.beta && t.valid && t.L < 4) gm(A.beta)[i4(P, t, k, t.L)] = bad ? nan : sqrt(fmax(b2, 0.0));
        // (the last stage of a beta-only or short sweep forms a Sigma+ nobody reads: skipping it, by a break or a wave-uniform branch,
        //  costs the sweep 48 bytes of scratch per lane at two waves per SIMD -- 340 of a launch's 585 N FMAs are not worth that)
        // row i of M = A - B K (the gain's entries are the broadcast source)
        double M[13], nbr[4];
        SFOR(a, 0, 4, { nbr[a] = -br[a]; });
        SFOR(l, 0, 13, {
            double m = l < 3 ? (t.L == l ? 1.0 : 0.0) : ar[l < 3 ? 0 : l - 3];
            dotbc<4, 0>(m, nbr, kr[l]);
            M[l] = m;
        });
        // Sigma+ = Y M' + W: Sigma+[i][j] = W[i][j] + sum_l Y[i][l] * M[l]@lane(j)
        unc_ld_sym(A.W, lane_opaque(t), S);   // (W's row re-read per stage: 26 registers the sweep does not have at two waves per SIMD)
        SFOR(l, 0, 13, { rank1bc<13>(S, Y[l], M[l]); });
    }
    if (kend == P.N + 1 && t.valid && t.L < 13) {
        if (A.Sig) {
            double* sg = A.Sig + ((ob * A.ns + (P.N - A.s0)) * 13 + eL) * 13;
            SFOR(j, 0, 13, { sg[ext_of(j)] = bad ? nan : S[j]; });
        }
        if (A.sd) {
            double dg = 0.0;
            SFOR(j, 0, 13, { dg = (t.L == j) ? S[j] : dg; });
            A.sd[(ob * A.ns + (P.N - A.s0)) * 13 + eL] = bad ? nan : sqrt(fmax(dg, 0.0));
        }
    }
}

// lb' = lb + t, ub' = ub - t with t = min(gamma beta, (1 - min_width) (ub - lb) / 2); an equality entry (lb == ub) and an entry
// without a backoff (NaN: a row whose QP failed) keep the nominal values.  Every product and sum is rounded on its own, so that
// the same expressions in IEEE double arithmetic on the host give the same bits.
__global__ __launch_bounds__(256) void k_unc_tighten(Params P, TightenArgs A) {
#pragma clang fp contract(off)
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)P.B * P.N * 4) return;
    const int a = (int)(e & 3), k = (int)((e >> 2) % P.N), i = (int)((e >> 2) / P.N);
    const size_t idx = P.v4b ? (((size_t)(i >> 2) * P.N + k) * 4 + (i & 3)) * 4 + a : ((size_t)i * P.N + k) * 4 + a;
    const double lo = A.nlb ? A.nlb[idx] : A.u_min, hi = A.nub ? A.nub[idx] : A.u_max;
    const double gb = A.gamma * A.beta[idx];
    const double cap = (1.0 - A.min_width) * (hi - lo) / 2.0;
    double lt = lo, ht = hi;
    if (lo != hi && gb == gb) {
        const bool cl = gb > cap;
        const double tt = cl ? cap : gb;
        lt = lo + tt;
        ht = hi - tt;
        if (cl) atomicAdd(A.ncl + i, 1);
    }
    A.lbs[idx] = lt; A.ubs[idx] = ht;
    A.clbs[idx] = lt; A.cubs[idx] = ht;
}

void launch_unc_put_sym(int B, const double* src, double* tab, hipStream_t st) {
    hipLaunchKernelGGL(k_unc_put_sym, dim3((unsigned)(((long)B * 169 + 255) / 256)), dim3(256), 0, st, B, src, tab);
}
void launch_unc_put_gain(int B, const double* src, double* tab, hipStream_t st) {
    hipLaunchKernelGGL(k_unc_put_gain, dim3((unsigned)(((long)B * 52 + 255) / 256)), dim3(256), 0, st, B, src, tab);
}
void launch_unc_prop(const Params& P, const UncArgs& A, hipStream_t st) {
    hipLaunchKernelGGL(k_unc_prop, dim3((A.nb + 3) / 4), dim3(64), 0, st, P, A);
}
void launch_unc_tighten(const Params& P, const TightenArgs& A, hipStream_t st) {
    (void)hipMemsetAsync(A.ncl, 0, sizeof(int) * (size_t)P.B, st);
    hipLaunchKernelGGL(k_unc_tighten, dim3((unsigned)(((long)P.B * P.N * 4 + 255) / 256)), dim3(256), 0, st, P, A);
}

}  // namespace cfn
