// cfnmpc_adj.hpp -- adjoint solution sensitivities: the gradient of a caller's loss on the last QP's solution with respect to
// that QP's data (cfnmpc_eval_adjoint / cfnmpc_get_adjoint / cfnmpc_get_adjoint_cost).  Included at the
// end of cfnmpc_kernels.hip (its primitives and sens_stage of cfnmpc_sens.hpp, no device unit of its own).
//
// With the active set of cfnmpc_eval_sens_x0 held, the solution z = (x, u) of the QP is affine in its linear cost terms, x0, the
// defects b_k and the bounds the active inputs sit on.  For a loss l with gradients gx_k = dl/dx_k, gu_k = dl/du_k the vector
//     a = argmin  sum_k 1/2 a_k' W a_k + g_k' a_k   s.t.  ax_{k+1} = A_k ax_k + B_k au_k,  ax_0 = 0,  au_{k,active} = 0
// is dl/d(linear cost term), and the multipliers (lambda, mu) of that problem's constraints are the gradients with respect to
// the constraints' right-hand sides.  SIGN CONVENTION (this file, the C ABI and tests/test_adjoint_cpu.py: adjoint_ref):
//     dl/dq_k = +ax_k,  dl/dr_k = +au_k,  dl/dx0 = +lambda_0,  dl/db_k = +lambda_{k+1},  dl/dbound_{k,a} = +mu_{k,a} (active a)
//     dl/dyref_{k,j} = -W_j a_{k,j},   dl/dW_j = +scale sum_k a_{k,j} (z_{k,j} - yref_{k,j})        (W: the effective diagonal weight)
// Three sweeps, row groups (16 lanes per instance, four instances per wavefront), every row (and, for uniform weights, the
// one-wave copy k_adj_wuni in front of them):
//   k_adj_bwd   backward: the masked Riccati recursion (sens_stage) with the affine row p_k in lane 13,
//                   w = gu_k + B_k' p_{k+1},  kappa_k = -S_FF^{-1} w_F (0 on active inputs),  p_k = gx_k + A_k' p_{k+1} - K_k' w_F;
//               the start solve keeps no S^{-1} (factor_stage stores it for the interior-point corrector only), so the
//               cost-to-go is recomputed: from the Riccati checkpoint behind the row's last active stage AND the caller's last
//               non-zero gradient (Pchk, exact: nothing behind it is active and p is zero there), or from QN.  Keeps kappa.
//   k_adj_fwd   forward on the stored (A, B) and the masked (k < kst) or home gains:  au_k = -K_k ax_k + kappa_k,
//               ax_{k+1} = A_k ax_k + B_k au_k  (DPP broadcast FMAs, k_sens_fwd with one column).  Writes dl/dq, dl/dr and, lane j
//               owning component j, dl/dyref and the weight gradients, summed in the sweep's stage order (0 .. N - 1): no
//               atomics, two evaluations agree bit for bit.
//   k_adj_mult  backward: lambda_N = QN ax_N + gx_N,  mu_k = R au_k + gu_k + B_k' lambda_{k+1},
//               lambda_k = Q ax_k + gx_k + A_k' lambda_{k+1}.  The transposed products: lambda' rides as a ROW in lane 13 of the
//               row-distributed product (row) x A, (row) x B -- the instruction stream of factor_stage's steps (1), (2), no
//               reduction across lanes and no transpose.  Writes dl/dx0, dl/db, dl/dbox.
// Nothing here writes a field of Params: every output lives in the AdjArgs buffers (cfnmpc_ws.hpp) owned by the solver.
#pragma once

namespace cfn {

// stage at which the backward sweep of a row starts: the smallest Riccati checkpoint (< N) that is neither in front of the row's
// masked stages [0, kst) nor in front of a non-zero gradient (stages [0, ng)); else N (the terminal weight)
__device__ __forceinline__ int adj_start(const int N, const int kst, const int ng) {
    const int lo = imax(kst, ng);
    int ks = N;
    for (int c = N_CHK - 1; c >= 0; c--)
        if (chk_stage(c) >= lo && chk_stage(c) < N) ks = chk_stage(c);
    return ks;
}

// The row's effective weights in wtab's layout (cfnmpc_rg.hpp: WT_R, WT_QN; internal order): its row of the per-instance table,
// or the one uniform row k_adj_wuni copies out of the kernel arguments -- the select chains over P.W / P.WN (lane_wq, lane_wn)
// hold 60 scalar registers, which these sweeps do not have beside their pointers.
__device__ __forceinline__ const gwdouble* adj_wrow(const Params& P, const AdjArgs& A, int home) {
    return P.wtab ? wrow(P, home) : (const gwdouble*)(unsigned long long)A.wuni;
}
__global__ __launch_bounds__(64) void k_adj_wuni(Params P, AdjArgs A) {
    const int e = threadIdx.x;
    double v = 0.0;
    SFOR(j, 0, 13, { if (e == j) v = P.W[ext_of(j)]; });
    SFOR(a, 0, 4, { if (e == WT_R + a) v = P.W[13 + a]; });
    SFOR(j, 0, 13, { if (e == WT_QN + j) v = P.WN[ext_of(j)]; });
    if (e < WT_STRIDE) A.wuni[e] = v;
}

// the row-group lane of wavefront `blockIdx.x`; ic: the instance whose per-instance arrays the row reads (a padding row of the
// last wavefront aliases the wavefront's first row and stores nothing)
__device__ __forceinline__ Lane adj_lane(const Params& P, const AdjArgs& A, int& ic) {
    Lane t;
    t.L = threadIdx.x & 15;
    t.row = threadIdx.x >> 4;
    t.q = t.row;
    t.wave = blockIdx.x;
    t.inst = t.wave * 4 + t.q;
    t.home = t.inst;
    t.valid = t.inst < P.B;
    t.wu = adj_wrow(P, A, t.home)[WT_R + (t.L & 3)];
    ic = t.valid ? t.inst : t.wave * 4;
    return t;
}
// state / terminal weight of this lane's row (lane i < 13, 0 elsewhere)
__device__ __forceinline__ double adj_w13(const Params& P, const AdjArgs& A, const Lane& t, int off) {
    const double v = adj_wrow(P, A, t.home)[off + imin(t.L, 12)];
    return t.L < 13 ? v : 0.0;
}
__device__ __forceinline__ int adj_ng(const AdjArgs& A) { return imax(A.gx ? A.n_gx : 0, A.gu ? A.n_gu : 0); }

__global__ __launch_bounds__(64, 2) void k_adj_bwd(Params P, AdjArgs A) {
    __shared__ __attribute__((aligned(16))) double wtile[4][WT_TILE];
    __shared__ double btile[4][64];
    int ic;
    const Lane t = adj_lane(P, A, ic);
    const int N = P.N, ng = adj_ng(A);
    const int ks = adj_start(N, A.kst[ic], ng);
    int kmax = 0;
    for (int r = 0; r < 4; r++) kmax = imax(kmax, adj_start(N, A.kst[imin(t.wave * 4 + r, P.B - 1)], ng));
    const int eL = ext_of(imin(t.L, 12));
    const double is13 = t.L == 13 ? 1.0 : 0.0;
    // start: the checkpoint's cost-to-go with p = 0, or the terminal weight with p_N = gx_N
    double Pa[13];
    if (ks < N) {
        const gdouble* pc = gm(P.Pchk) + ((size_t)t.wave * N_CHK + chk_index(ks)) * SZ_PP;
        SFOR(j, 0, 13, {
            const double v = pc[pchk_at(j, t.q, imin(t.L, 12))];
            Pa[j] = t.L < 13 ? v : 0.0;
        });
    } else {
        const double wn = adj_w13(P, A, t, WT_QN);
        const bool gN = A.gx && A.n_gx == N + 1;
        const double* gp = A.gx + ((size_t)ic * A.n_gx + N) * 13;
        SFOR(j, 0, 13, {
            const double gv = gN ? gp[ext_of(j)] : 0.0;
            Pa[j] = (t.L == j) ? wn : (t.L == 13 ? gv : 0.0);
        });
    }
    const double wq = adj_w13(P, A, t, 0);
    const double rh = t.wu;
    // per-lane pointers and stage counts (vector registers: the sweep has them to spare, not the scalar ones)
    const int ngx = A.gx ? A.n_gx : 0, ngu = A.gu ? A.n_gu : 0;
    const double* gxl = A.gx + (size_t)ic * ngx * 13 + eL;
    const double* gul = A.gu + (size_t)ic * ngu * 4 + (t.L & 3);
    const unsigned* ml = reinterpret_cast<const unsigned*>(A.mask) + (size_t)ic * N;
    double* kl = A.kap + (size_t)t.inst * N * 4;
    for (int k = kmax - 1; k >= 0; k--) {
        double ar[10], br[4];
        ld_ar_raw(blkab(P, P.AR, t, k, SZ_A), t, ar);
        ld_rows4_raw(blkab(P, P.BR, t, k, SZ_B), t, br);
        const unsigned mw = ml[k];
        bool fa[4];
        SFOR(a, 0, 4, { fa[a] = ((mw >> (8 * a)) & 0xffu) != 0u; });
        double qv = 0.0, g = 0.0;
        if (k < ngx && t.L < 13) qv = gxl[(size_t)k * 13];
        if (k < ngu && t.L < 4) g = gul[(size_t)k * 4];
        double Pn[13], Kp[4];
        SFOR(j, 0, 13, { Pn[j] = Pa[j]; });
        sens_stage<true>(t, Pn, ar, br, fa, rh, wq, wtile[t.row], btile[t.row], Kp, is13, qv, g);
        const bool act = k < ks;
        SFOR(j, 0, 13, { Pa[j] = act ? Pn[j] : Pa[j]; });
        if (act && t.valid && t.L == 13) SFOR(a, 0, 4, { kl[(size_t)k * 4 + a] = -Kp[a]; });
    }
}

__global__ __launch_bounds__(64, 2) void k_adj_fwd(Params P, AdjArgs A) {
    int ic;
    const Lane t = adj_lane(P, A, ic);
    const double wq = adj_w13(P, A, t, 0), wn = adj_w13(P, A, t, WT_QN);
    const int N = P.N;
    const int kst = A.kst[ic];
    const int ks = adj_start(N, kst, adj_ng(A));
    const bool bad = A.status[ic] == 4;
    const double nan = __builtin_nan("");
    const int eL = ext_of(imin(t.L, 12));
    double* dq = A.dq + (size_t)t.inst * (N + 1) * 13 + eL;
    double* dr = A.dr + (size_t)t.inst * N * 4 + (t.L & 3);
    double* dy = A.dyref + (size_t)t.inst * N * 17;
    double* dye = A.dyref_e + (size_t)t.inst * 13 + eL;
    double* dwn = A.dWN + (size_t)t.inst * 13 + eL;
    double* dw = A.dW + (size_t)t.inst * 17;
    const double* kl = A.kap + (size_t)ic * N * 4 + (t.L & 3);
    const bool sx = t.valid && t.L < 13, su = t.valid && t.L < 4;
    double X = 0.0, accx = 0.0, accu = 0.0;   // lane j < 13: ax_j and its weight gradient; lane a < 4: that of input a
    for (int k = 0; k < N; k++) {
        double kr[13], ar[10], br[4];
        ld_cols4(blk(k < kst ? const_cast<double*>(A.K) : P.KR, t, N, k, SZ_K), t, kr);
        ld_ar(blkab(P, P.AR, t, k, SZ_A), t, ar);
        ld_rows4(blkab(P, P.BR, t, k, SZ_B), t, br);
        const gdouble* yb = blk(P.yref, t, N, k, SZ_Y) + t.q * 17;
        const double ex = ld13(blk(P.xit, t, N + 1, k, SZ_V13), t) - yb[imin(t.L, 12)];    // z_k - yref_k, states
        const double eu = gm(P.uit)[i4(P, t, k, t.L & 3)] - yb[13 + (t.L & 3)];            // ... inputs
        double kap = 0.0;
        if (k < ks && t.L < 4) kap = kl[(size_t)k * 4];
        if (sx) {
            dq[(size_t)k * 13] = bad ? nan : X;
            dy[(size_t)k * 17 + eL] = bad ? nan : -(wq * X);
        }
        accx += X * ex;
        double acc = 0.0;
        dotbc<13, 0>(acc, kr, X);
        double u = kap - acc;
        settle(u);
        if (su) {
            dr[(size_t)k * 4] = bad ? nan : u;
            dy[(size_t)k * 17 + 13 + t.L] = bad ? nan : -(t.wu * u);
        }
        accu += u * eu;
        double vr[4];
        SFOR(a, 0, 4, { vr[a] = bc<a>(u); });
        double xn = t.L < 3 ? X : 0.0;
        dotbc<10, 3>(xn, ar, X);
        SFOR(a, 0, 4, { xn += br[a] * vr[a]; });
        X = xn;
    }
    const double exN = ld13(blk(P.xit, t, N + 1, N, SZ_V13), t) - ld13(blk(P.yref_e, t, 1, 0, SZ_V13), t);
    if (sx) {
        dq[(size_t)N * 13] = bad ? nan : X;
        *dye = bad ? nan : -(wn * X);
        *dwn = bad ? nan : A.terminal_scale * (X * exN);
        dw[eL] = bad ? nan : A.stage_scale * accx;
    }
    if (su) dw[13 + t.L] = bad ? nan : A.stage_scale * accu;
}

__global__ __launch_bounds__(64, 2) void k_adj_mult(Params P, AdjArgs A) {
    int ic;
    const Lane t = adj_lane(P, A, ic);
    const int N = P.N;
    const bool bad = A.status[ic] == 4;
    const double nan = __builtin_nan("");
    const bool l13 = t.L == 13, st = t.valid && l13;
    // the row's weights in row form (every lane of the row holds all of them; lane 13 uses them)
    const gwdouble* wt = adj_wrow(P, A, t.home);
    double wq[13], wr[4];
    SFOR(j, 0, 13, { wq[j] = wt[j]; });
    SFOR(a, 0, 4, { wr[a] = wt[WT_R + a]; });
    const int eL = ext_of(imin(t.L, 12)), a4 = t.L & 3;
    // ax_k, au_k and the loss gradients are read lane-distributed (lane j: component j, one run per row) and handed to
    // lane 13's row form by DPP broadcasts
    const double* aq = A.dq + (size_t)ic * (N + 1) * 13 + eL;
    const double* au_ = A.dr + (size_t)ic * N * 4 + a4;
    const int ngx = A.gx ? A.n_gx : 0, ngu = A.gu ? A.n_gu : 0;
    const double* gxl = A.gx + (size_t)ic * ngx * 13 + eL;
    const double* gul = A.gu + (size_t)ic * ngu * 4 + a4;
    // lambda_N
    double Lm[13];
    {
        const double axv = aq[(size_t)N * 13];
        const double gxv = ngx == N + 1 ? gxl[(size_t)N * 13] : 0.0;
        const double lamv = wt[WT_QN + imin(t.L, 12)] * axv + gxv;      // lane j < 13: lambda_N[j]
        SFOR(j, 0, 13, {
            const double lam = bc<j>(lamv);
            Lm[j] = l13 ? lam : 0.0;
        });
    }
    const unsigned* ml = reinterpret_cast<const unsigned*>(A.mask) + (size_t)ic * N;
    double* db = A.db + (size_t)t.inst * N * 13;
    double* dbx = A.dbox + (size_t)t.inst * N * 4;
    for (int k = N - 1; k >= 0; k--) {
        double ar[10], br[4];
        ld_ar_raw(blkab(P, P.AR, t, k, SZ_A), t, ar);
        ld_rows4_raw(blkab(P, P.BR, t, k, SZ_B), t, br);
        const unsigned mw = ml[k];
        const double axv = aq[(size_t)k * 13], auv = au_[(size_t)k * 4];
        const double gxv = k < ngx ? gxl[(size_t)k * 13] : 0.0;
        const double guv = k < ngu ? gul[(size_t)k * 4] : 0.0;
        // lane 13: W = lambda_{k+1}' A_k, V = lambda_{k+1}' B_k (the other lanes: zero rows)
        double W[13], V[4];
        SFOR(j, 0, 3, { W[j] = Lm[j]; });
        SFOR(j, 3, 13, { W[j] = 0.0; });
        SFOR(a, 0, 4, { V[a] = 0.0; });
        dot3bc<6>(W[3], W[4], W[5], Lm, ar[0], ar[1], ar[2]);
        dot4bc<10>(W[6], W[7], W[8], W[9], Lm, ar[3], ar[4], ar[5], ar[6]);
        dot3bc<13>(W[10], W[11], W[12], Lm, ar[7], ar[8], ar[9]);
        dot4bc<13>(V[0], V[1], V[2], V[3], Lm, br[0], br[1], br[2], br[3]);
        SFOR(j, 0, 13, {
            const double lam = wq[j] * bc<j>(axv) + bc<j>(gxv) + W[j];
            if (st) db[(size_t)k * 13 + ext_of(j)] = bad ? nan : Lm[j];
            Lm[j] = l13 ? lam : 0.0;
        });
        SFOR(a, 0, 4, {
            const double mu = wr[a] * bc<a>(auv) + bc<a>(guv) + V[a];
            const bool active = ((mw >> (8 * a)) & 0xffu) != 0u;
            if (st) dbx[(size_t)k * 4 + a] = bad ? nan : (active ? mu : 0.0);
        });
    }
    if (st) SFOR(j, 0, 13, { A.dx0[(size_t)t.inst * 13 + ext_of(j)] = bad ? nan : Lm[j]; });
}

void launch_adjoint(const Params& P, const AdjArgs& A, hipStream_t st) {
    if (!P.wtab) hipLaunchKernelGGL(k_adj_wuni, dim3(1), dim3(64), 0, st, P, A);
    hipLaunchKernelGGL(k_adj_bwd, dim3(P.NW), dim3(64), 0, st, P, A);
    hipLaunchKernelGGL(k_adj_fwd, dim3(P.NW), dim3(64), 0, st, P, A);
    hipLaunchKernelGGL(k_adj_mult, dim3(P.NW), dim3(64), 0, st, P, A);
}

}  // namespace cfn
