// cfnmpc_sens.hpp -- solution sensitivities with respect to the initial state (cfnmpc_eval_sens_x0 / cfnmpc_get_sens_x0;
// DESIGN.md section 5.14).  Included at the end of cfnmpc_kernels.hip (its primitives, no device unit of its own).
//
// With the active set A of the last QP's solution held fixed, the solution is affine in x0; its Jacobian comes from the
// homogeneous Riccati recursion with the active inputs removed:
//     P_N = diag(QN);  k = N-1 .. 0:  S_FF = R_FF + B_F' P B_F,  K_k[F] = S_FF^{-1} (B'PA)_F,  K_k[A] = 0,
//                                     P = Q + A'PA - (A'PB)_F K_k[F]
//     X_0 = I;  U_k = -K_k X_k;  X_{k+1} = A_k X_k + B_k U_k       (du_k/dx0 = U_k, dx_k/dx0 = X_k)
// Three kernels:
//   k_sens_mask    lane per instance: the active set of the current iterate (mask [B][N][4]: 0 free, -1 lower, +1 upper),
//                  the work list of the rows with an active input (one ballot + one atomic per wave) and per row the stage
//                  kst below which its gains differ from the start solve's (0: none; else the smallest Riccati checkpoint
//                  behind its last active stage, or N);
//   k_sens_factor  row groups (cfnmpc_ws.hpp), listed rows only: the masked backward sweep over [0, kst) from the checkpoint's
//                  cost-to-go (Pchk: the unconstrained tail, exact because no input behind it is active) or from QN; the
//                  arithmetic of factor_stage without the affine row, the fixing weight of the active-set solves
//                   on the diagonal of R^ for active inputs and exact zeros for their gain rows;
//   k_sens_fwd     row groups, every row: the forward propagation of the 13 columns of X_k on the stored (A, B) and the
//                  masked (k < kst) or home gains KR, written in the public state order.
// Nothing here writes a field of Params: the outputs live in the SensArgs buffers (cfnmpc_ws.hpp) owned by the solver.
#pragma once

namespace cfn {


constexpr double SENS_FIX = 1e30;   // fixing weight of an active input: SENS_FIX * max(1, R_a) on the diagonal of R^

__global__ __launch_bounds__(64) void k_sens_mask(Params P, SensArgs A) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool valid = i < P.B;
    int last = -1;
    if (valid) {
        // uit / lbs / ubs in the home 4-vector layout (Params.v4b)
        const int rb = P.v4b ? (i >> 2) : i, s4n = P.v4b ? 16 : 4, q4 = P.v4b ? (i & 3) * 4 : 0;
        const double* ui = P.uit;
        for (int k = 0; k < P.N; k++) {
            const size_t base = ((size_t)rb * P.N + k) * s4n + q4;
            unsigned word = 0;
            for (int a = 0; a < 4; a++) {
                const double u = gm(ui)[base + a];
                const double lo = P.lbs ? gm(P.lbs)[base + a] : P.u_min;
                const double hi = P.ubs ? gm(P.ubs)[base + a] : P.u_max;
                const int m = (lo == hi || u - lo <= A.tol) ? -1 : (hi - u <= A.tol ? 1 : 0);
                if (m) last = k;
                word |= (unsigned)(unsigned char)(signed char)m << (8 * a);
            }
            reinterpret_cast<unsigned*>(A.mask)[(size_t)i * P.N + k] = word;
        }
    }
    const bool listed = last >= 0;
    int kst = 0;
    if (listed) {
        kst = P.N;
        for (int c = N_CHK - 1; c >= 0; c--)
            if (chk_stage(c) > last && chk_stage(c) < P.N) kst = chk_stage(c);   // (the checkpoints are written for stages < N)
    }
    if (valid) A.kst[i] = kst;
    const unsigned long long bal = __ballot(listed);
    if (bal) {
        int base = 0;
        if (threadIdx.x == 0) base = atomicAdd(A.cnt, __popcll(bal));
        base = __shfl(base, 0);
        if (listed) A.list[base + __popcll(bal & ((1ull << threadIdx.x) - 1ull))] = i;
    }
}

// index of the checkpoint at stage k (k one of chk_stage)
__device__ __forceinline__ int chk_index(int k) {
    int c = 0;
    SFOR(j, 0, N_CHK, { if (chk_stage(j) == k) c = j; });
    return c;
}

// One stage of the masked homogeneous recursion (factor_stage's arithmetic without the affine row).  Pa: lanes 0..12 row i
// of P_{k+1} -> P_k; fa[a]: input a of this row's instance is active (row-uniform); rh: R_a in lanes a < 4.  Returns the
// transposed gain in Kp (lane l < 13: K[a][l]), exact zeros for the active inputs.
// AFF (cfnmpc_adj.hpp): lane 13 carries an affine row p' as factor_stage's does -- qv: its linear state term in lanes j < 13,
// g: its linear input term in lanes a < 4; on exit lane 13 of Pa holds p_k' and lane 13 of Kp the feed-forward S_FF^{-1} rho_F
// (exact zeros on the active inputs).  Lanes 0..12 see the same instructions either way.
template <bool AFF = false>
__device__ __forceinline__ void sens_stage(const Lane& t, double (&Pa)[13], const double (&ar)[10], const double (&br)[4],
                                           const bool (&fa)[4], const double rh, const double wq, double* wt, double* sb,
                                           double (&Kp)[4], const double is13 = 0.0, const double qv = 0.0, const double g = 0.0) {
    // (1) W = Pa A (row form), (2) V = Pa B
    double W[13], V[4];
    SFOR(j, 0, 3, { W[j] = Pa[j]; });
    SFOR(j, 3, 13, { W[j] = 0.0; });
    dot3bc<6>(W[3], W[4], W[5], Pa, ar[0], ar[1], ar[2]);
    dot4bc<10>(W[6], W[7], W[8], W[9], Pa, ar[3], ar[4], ar[5], ar[6]);
    dot3bc<13>(W[10], W[11], W[12], Pa, ar[7], ar[8], ar[9]);
    // (3) transpose of W and the columns of B through the LDS tile
    __syncthreads();
    if (t.L < 13) {
        SFOR(j, 0, 13, { wt[t.L * WT_ROW + j] = W[j]; });
        SFOR(a, 0, 4, { sb[a * 16 + t.L] = br[a]; });
    }
    SFOR(a, 0, 4, { V[a] = 0.0; });
    dot4bc<13>(V[0], V[1], V[2], V[3], Pa, br[0], br[1], br[2], br[3]);
    __syncthreads();
    double bcl[13], Wt[13];
    SFOR(l, 0, 13, { bcl[l] = sb[(t.L & 3) * 16 + l]; });
    SFOR(l, 0, 13, { Wt[l] = wt[l * WT_ROW + imin(t.L, 12)]; });
    // (4) S = R^ + B'V (the fixing weight on the active inputs' diagonal), replicated; Cholesky between (5) and (6)
    double Srow[4];
    const int la = t.L & 3;
    const bool fl = la == 0 ? fa[0] : (la == 1 ? fa[1] : (la == 2 ? fa[2] : fa[3]));
    const double rhat = fl ? rh + SENS_FIX * fmax(1.0, rh) : rh;
    SFOR(c, 0, 4, { Srow[c] = (t.L == c) ? rhat : 0.0; });
    dot4bc<13>(Srow[0], Srow[1], Srow[2], Srow[3], bcl, V[0], V[1], V[2], V[3]);
    SFOR(c, 0, 4, { settle(Srow[c]); });
    double S[10], Si[10];
    SFOR(a, 0, 4, { SFOR(c, a, 4, { S[s4(a, c)] = bc<a>(Srow[c]); }); });
    SFOR(l, 0, 13, { pin(Wt[l]); });
    if (AFF) SFOR(l, 0, 13, { Wt[l] = t.L == 13 ? Pa[l] : Wt[l]; });
    Chol4 ch;
    chol4_pivot<0>(S, ch);
    // (5) M = Q + Wt A
    double M[13];
    SFOR(j, 0, 13, { M[j] = (t.L == j) ? wq : 0.0; });
    if (AFF) rank1bc<13>(M, is13, qv);
    SFOR(j, 0, 3, { M[j] += Wt[j]; });
    dot3bc<6>(M[3], M[4], M[5], Wt, ar[0], ar[1], ar[2]);
    chol4_pivot<1>(S, ch);
    dot4bc<10>(M[6], M[7], M[8], M[9], Wt, ar[3], ar[4], ar[5], ar[6]);
    chol4_pivot<2>(S, ch);
    dot3bc<13>(M[10], M[11], M[12], Wt, ar[7], ar[8], ar[9]);
    chol4_pivot<3>(S, ch);
    // (6) G' = Wt B
    double Gp[4];
    SFOR(a, 0, 4, { Gp[a] = 0.0; });
    dot4bc<13>(Gp[0], Gp[1], Gp[2], Gp[3], Wt, br[0], br[1], br[2], br[3]);
    if (AFF) rank1bc<4>(Gp, is13, g);
    chol4_finish(ch, Si);
    // (7) K' = G' Sinv, active columns exactly zero
    double nGp[4];
    SFOR(a, 0, 4, {
        double s = 0.0;
        SFOR(c, 0, 4, { s += Gp[c] * Si[s4(c, a)]; });
        Kp[a] = fa[a] ? 0.0 : s;
        nGp[a] = -Gp[a];
    });
    // (8) P <- M - G' K  (free inputs only)
    SFOR(j, 0, 13, { Pa[j] = M[j]; });
    upd4bc<0, 4>(Pa, Kp, nGp);
    upd4bc<4, 4>(Pa, Kp, nGp);
    upd4bc<8, 4>(Pa, Kp, nGp);
    upd4bc<12, 1>(Pa, Kp, nGp);
}

// masked backward sweep of the listed rows: four list slots per wavefront; a slot behind the list aliases the wave's first
// row and stores nothing
__global__ __launch_bounds__(64, 2) void k_sens_factor(Params P, SensArgs A) {
    __shared__ __attribute__((aligned(16))) double wtile[4][WT_TILE];
    __shared__ double btile[4][64];
    const int n = *A.cnt;
    const int w = blockIdx.x;
    if (w * 4 >= n) return;   // (wave-uniform)
    const int row = threadIdx.x >> 4;
    const bool valid = w * 4 + row < n;
    Lane t;
    t.L = threadIdx.x & 15;
    t.row = row;
    t.inst = A.list[valid ? w * 4 + row : w * 4];
    t.wave = t.inst >> 2;
    t.q = t.inst & 3;
    t.home = t.inst;
    t.valid = valid;
    t.wu = lane_wu(P, t.home, t.L & 3);
    const int kst = valid ? A.kst[t.inst] : 0;
    int kmax = 0;
    for (int r = 0; r < 4; r++)
        if (w * 4 + r < n) kmax = imax(kmax, A.kst[A.list[w * 4 + r]]);
    // start: the checkpoint's cost-to-go (home: packed) or the terminal weight
    double Pa[13];
    if (kst > 0 && kst < P.N) {
        const gdouble* pc = gm(P.Pchk) + ((size_t)t.wave * N_CHK + chk_index(kst)) * SZ_PP;
        SFOR(j, 0, 13, {
            const double v = pc[pchk_at(j, t.q, imin(t.L, 12))];
            Pa[j] = t.L < 13 ? v : 0.0;
        });
    } else {
        const double wn = lane_wn(P, t);
        SFOR(j, 0, 13, { Pa[j] = (t.L == j) ? wn : 0.0; });
    }
    const double wq = lane_wq(P, t);
    const double rh = t.wu;
    for (int k = kmax - 1; k >= 0; k--) {
        double ar[10], br[4];
        ld_ar_raw(blkab(P, P.AR, t, k, SZ_A), t, ar);
        ld_rows4_raw(blkab(P, P.BR, t, k, SZ_B), t, br);
        const unsigned mw = reinterpret_cast<const unsigned*>(A.mask)[(size_t)t.inst * P.N + k];
        bool fa[4];
        SFOR(a, 0, 4, { fa[a] = ((mw >> (8 * a)) & 0xffu) != 0u; });
        double Pn[13], Kp[4];
        SFOR(j, 0, 13, { Pn[j] = Pa[j]; });
        sens_stage(t, Pn, ar, br, fa, rh, wq, wtile[t.row], btile[t.row], Kp);
        const bool act = k < kst;
        SFOR(j, 0, 13, { Pa[j] = act ? Pn[j] : Pa[j]; });
        if (act && t.L < 13) {
            gdouble* kr = blk(A.K, t, P.N, k, SZ_K) + (t.L * 4 + t.q) * 4;
            SFOR(a, 0, 4, { kr[a] = Kp[a]; });
        }
    }
}

// forward propagation of the 13 columns of X_k over [0, s0 + ns) for the rows [b0, b0 + nb) (wave-aligned: b0 % 4 == 0)
__global__ __launch_bounds__(64, 2) void k_sens_fwd(Params P, SensArgs A) {
    Lane t;
    t.L = threadIdx.x & 15;
    t.row = threadIdx.x >> 4;
    t.q = t.row;
    t.wave = A.b0 / 4 + blockIdx.x;
    t.inst = t.wave * 4 + t.q;
    t.home = t.inst;
    t.valid = t.inst < P.B && t.inst < A.b0 + A.nb;
    t.wu = 0.0;
    const int kst = t.valid ? A.kst[t.inst] : 0;
    const bool bad = t.valid && A.status[t.inst] == 4;
    const double nan = __builtin_nan("");
    const int kend = A.s0 + A.ns;           // last output stage + 1 (<= N + 1)
    const int kf = imin(kend, P.N);         // stages with a feedback law
    const size_t ob = (size_t)(t.inst - A.b0);
    const int eL = ext_of(imin(t.L, 12));
    double X[13];
    SFOR(j, 0, 13, { X[j] = (t.L == j) ? 1.0 : 0.0; });
    for (int k = 0; k < kf; k++) {
        double kr[13], ar[10], br[4];
        ld_cols4(blk(k < kst ? A.K : P.KR, t, P.N, k, SZ_K), t, kr);
        ld_ar(blkab(P, P.AR, t, k, SZ_A), t, ar);
        ld_rows4(blkab(P, P.BR, t, k, SZ_B), t, br);
        const bool out = t.valid && k >= A.s0;
        double* du = (out && A.du && t.L < 4) ? A.du + ((ob * A.ns + (k - A.s0)) * 4 + t.L) * 13 : nullptr;
        double* dx = (out && A.dx && t.L < 13) ? A.dx + ((ob * A.ns + (k - A.s0)) * 13 + eL) * 13 : nullptr;
        double Xn[13];
        SFOR(j, 0, 13, {
            double acc = 0.0;
            dotbc<13, 0>(acc, kr, X[j]);
            double u = -acc;
            settle(u);
            if (du) du[ext_of(j)] = bad ? nan : u;
            if (dx) dx[ext_of(j)] = bad ? nan : X[j];
            double vr[4];
            SFOR(a, 0, 4, { vr[a] = bc<a>(u); });
            double xn = t.L < 3 ? X[j] : 0.0;
            dotbc<10, 3>(xn, ar, X[j]);
            SFOR(a, 0, 4, { xn += br[a] * vr[a]; });
            Xn[j] = xn;
        });
        SFOR(j, 0, 13, { X[j] = Xn[j]; });
    }
    if (kend == P.N + 1 && A.dx && t.valid && t.L < 13) {
        double* dx = A.dx + ((ob * A.ns + (P.N - A.s0)) * 13 + eL) * 13;
        SFOR(j, 0, 13, { dx[ext_of(j)] = bad ? nan : X[j]; });
    }
}

// get(0, 1): no sweep -- du_0/dx0 = -K_0 (masked or home gains, columns to the public order) and dx_0/dx0 = I, one thread per
// output element of the rows [b0, b0 + nb) (the same values as k_sens_fwd's first stage, bit for bit)
__global__ __launch_bounds__(256) void k_sens_first(Params P, SensArgs A) {
    const int wu = A.du ? 52 : 0, wx = A.dx ? 169 : 0;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)A.nb * (wu + wx)) return;
    const bool isu = e < (long)A.nb * wu;
    const long e2 = isu ? e : e - (long)A.nb * wu;
    const int w = isu ? wu : wx;
    const int r = (int)(e2 / w), c = (int)(e2 % w);
    const int inst = A.b0 + r;
    const bool bad = A.status[inst] == 4;
    double v;
    if (isu) {
        const int a = c / 13, l = int_of(c % 13);
        const int wave = inst >> 2, q = inst & 3;
        const double* kb = (A.kst[inst] > 0 ? A.K : P.KR) + ((size_t)wave * P.N) * SZ_K;
        v = -kb[(l * 4 + q) * 4 + a];
        A.du[e2] = bad ? __builtin_nan("") : v;
    } else {
        v = (c / 13 == c % 13) ? 1.0 : 0.0;
        A.dx[e2] = bad ? __builtin_nan("") : v;
    }
}

void launch_sens_eval(const Params& P, const SensArgs& A, hipStream_t st) {
    (void)hipMemsetAsync(A.cnt, 0, sizeof(int), st);
    hipLaunchKernelGGL(k_sens_mask, dim3((P.B + 63) / 64), dim3(64), 0, st, P, A);
    hipLaunchKernelGGL(k_sens_factor, dim3(P.NW), dim3(64), 0, st, P, A);
}

void launch_sens_fwd(const Params& P, const SensArgs& A, hipStream_t st) {
    if (A.s0 == 0 && A.ns == 1) {
        const long n = (long)A.nb * ((A.du ? 52 : 0) + (A.dx ? 169 : 0));
        hipLaunchKernelGGL(k_sens_first, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P, A);
        return;
    }
    hipLaunchKernelGGL(k_sens_fwd, dim3((A.nb + 3) / 4), dim3(64), 0, st, P, A);
}

}  // namespace cfn
