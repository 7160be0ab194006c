// cfnmpc_ekf.hpp -- batched extended Kalman filter on the engine's RK4 plant: state estimates with their covariance
// (cfnmpc_ekf_step; the rules are in include/cfnmpc.h), and its disturbance-augmented form with 13 states
// and three disturbance slots, one per lane of a 16-lane row (cfnmpc_ekf_aug_step, k_ekf_aug; section 5.27).
//
// Two parts, as cfnmpc_simvjp.hpp.  The first needs cfnmpc_model.hpp (through cfnmpc_simvjp.hpp's first part) only and compiles
// for the host as well (tools/ekf_check.cpp runs it under the host sanitizers): one instance's predict and update as plain loops,
// and ekf_decide, the skip / gate decision of one measured component, which the kernels share.  The second, the kernels, is
// compiled where cfnmpc_kernels.hip includes this file at its end (CFNMPC_EKF_KERNELS: its rk4_steps, ModelK and the row-group
// primitives of cfnmpc_rg.hpp; no device unit of its own and no field of Params: the call is solver-free like cfnmpc_sim).
//
// Predict, per RK4 sub-step s of h = T / steps:   A_s = d x_{s+1} / d x_s at (x_s, u; p, d),   P <- A_s P A_s',   x <- x_{s+1}
// and P += Q once per call.  Row i of A_s is the reverse sub-step of cfnmpc_simvjp.hpp seeded with e_i (lambda = A_s' e_i): the
// exact derivative of the discrete map.  Update: sequential over the measured components, in index order (a selector H and a
// diagonal R: the joint Kalman update), with a chi-square gate per component.
#pragma once
#include "cfnmpc_simvjp.hpp"

namespace cfn {

constexpr int EKF_NORMALIZE_Q = 1;   // include/cfnmpc.h: CFNMPC_EKF_NORMALIZE_Q

// One component j of the sequential update on the current (x, P): innovation variance s = P_jj + r_j, innovation nu = z_j - x_j;
// skip: not measured (r_j < 0); rej: measured, but outside the gate (gate > 0 and nu^2 > gate^2 s).  A NaN fails both tests: the
// component is used and the NaN spreads over the instance.
struct EkfDec {
    double s, nu;
    bool skip, rej;
};
__host__ __device__ __forceinline__ EkfDec ekf_decide(double pjj, double xj, double zj, double rj, double gate) {
    EkfDec e;
    e.s = pjj + rj;
    e.nu = zj - xj;
    e.skip = rj < 0.0;
    e.rej = gate > 0.0 && e.nu * e.nu > gate * gate * e.s;
    return e;
}

// ---- one instance as plain loops (host check; not used by the kernels below, which spread an instance over a 16-lane row) ----
template <class K>
__host__ __device__ inline void ekf_rk4_substep(double (&xc)[13], const double (&uc)[4], double h, const K& mk) {
    double k1[13], k2[13], k3[13], k4[13], xt[13];
    f_expl(xc, uc, k1, mk);
    for (int e = 0; e < 13; e++) xt[e] = xc[e] + 0.5 * h * k1[e];
    f_expl(xt, uc, k2, mk);
    for (int e = 0; e < 13; e++) xt[e] = xc[e] + 0.5 * h * k2[e];
    f_expl(xt, uc, k3, mk);
    for (int e = 0; e < 13; e++) xt[e] = xc[e] + h * k3[e];
    f_expl(xt, uc, k4, mk);
    for (int e = 0; e < 13; e++) xc[e] += (h / 6.0) * (k1[e] + 2 * k2[e] + 2 * k3[e] + k4[e]);
}
// A [13][13] = d x+ / d x of one sub-step from x, row by row
template <class K>
__host__ __device__ inline void ekf_substep_jac(const double (&x)[13], const double (&u)[4], double h, double* A, const K& mk) {
    for (int i = 0; i < 13; i++) {
        double lam[13], gu[4] = {0.0, 0.0, 0.0, 0.0};
        SimGrad G{};
        for (int e = 0; e < 13; e++) lam[e] = e == i ? 1.0 : 0.0;
        rk4_substep_vjp(x, u, h, lam, gu, G, mk);
        for (int e = 0; e < 13; e++) A[i * 13 + e] = lam[e];
    }
}
// x [13], P [13][13] in place; Q [13][13] or nullptr
template <class K>
__host__ __device__ inline void ekf_predict(double (&x)[13], double* P, const double (&u)[4], double T, int steps, const double* Q,
                                            const K& mk) {
    const double h = T / steps;
    for (int s = 0; s < steps; s++) {
        double A[169], Y[169];
        ekf_substep_jac(x, u, h, A, mk);
        for (int i = 0; i < 13; i++)
            for (int j = 0; j < 13; j++) {
                double acc = 0.0;
                for (int l = 0; l < 13; l++) acc += A[i * 13 + l] * P[l * 13 + j];
                Y[i * 13 + j] = acc;
            }
        for (int i = 0; i < 13; i++)
            for (int j = 0; j < 13; j++) {
                double acc = 0.0;
                for (int l = 0; l < 13; l++) acc += Y[i * 13 + l] * A[j * 13 + l];
                P[i * 13 + j] = acc;
            }
        ekf_rk4_substep(x, u, h, mk);
    }
    if (Q)
        for (int e = 0; e < 169; e++) P[e] += Q[e];
}
// quaternion sign, sequential update, optional normalisation; z is not written to.  counts = (used, rejected)
__host__ __device__ inline void ekf_update(double (&x)[13], double* P, const double* z_in, const double* r, double gate, int flags,
                                           double& nis, int (&counts)[2]) {
    double z[13];
    for (int j = 0; j < 13; j++) z[j] = z_in[j];
    double dot = 0.0;
    for (int j = 3; j < 7; j++)
        if (r[j] >= 0.0) dot += z[j] * x[j];
    if (dot < 0.0)
        for (int j = 3; j < 7; j++) z[j] = -z[j];
    nis = 0.0;
    counts[0] = 0; counts[1] = 0;
    for (int j = 0; j < 13; j++) {
        const EkfDec e = ekf_decide(P[j * 14], x[j], z[j], r[j], gate);
        if (e.skip) continue;
        if (e.rej) { counts[1]++; continue; }
        const double rs = 1.0 / e.s;
        double col[13], row[13];
        for (int a = 0; a < 13; a++) { col[a] = P[a * 13 + j]; row[a] = P[j * 13 + a]; }
        for (int a = 0; a < 13; a++) x[a] += (col[a] * e.nu) / e.s;
        for (int a = 0; a < 13; a++)
            for (int b = 0; b < 13; b++) P[a * 13 + b] -= (col[a] * row[b]) * rs;
        nis += e.nu * e.nu / e.s;
        counts[0]++;
    }
    if (flags & EKF_NORMALIZE_Q) {
        const double n = sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5] + x[6] * x[6]);
        for (int j = 3; j < 7; j++) x[j] = x[j] / n;
    }
}

// ---- the disturbance-augmented filter (cfnmpc_ekf_aug_step): a = [x; d[sel[0]], d[sel[1]], d[sel[2]]],
// NA = 16, one instance as plain loops.  F_s = [[A_s, G_s S], [0, I]]: row i < 13 is the reverse sub-step seeded with e_i, whose
// lam is row i of A_s and whose SimGrad::gd is row i of G_s = d x_{s+1} / d d; slot k takes column sel[k] of it (sel[k] < 0: a
// zero column).  The model always carries the disturbance row (DstK).
constexpr int EKF_NA = 16;   // include/cfnmpc.h: CFNMPC_EKF_NA

// F [16][16] of one sub-step from x
template <class K>
__host__ __device__ inline void ekf_aug_substep_jac(const double (&x)[13], const double (&u)[4], double h, const int (&sel)[3],
                                                    double* F, const K& mk) {
    for (int e = 0; e < EKF_NA * EKF_NA; e++) F[e] = 0.0;
    for (int i = 0; i < 13; i++) {
        double lam[13], gu[4] = {0.0, 0.0, 0.0, 0.0};
        SimGrad G{};
        for (int e = 0; e < 13; e++) lam[e] = e == i ? 1.0 : 0.0;
        rk4_substep_vjp(x, u, h, lam, gu, G, mk);
        for (int e = 0; e < 13; e++) F[i * EKF_NA + e] = lam[e];
        for (int k = 0; k < 3; k++) F[i * EKF_NA + 13 + k] = sel[k] >= 0 ? G.gd[sel[k]] : 0.0;
    }
    for (int k = 0; k < 3; k++) F[(13 + k) * EKF_NA + 13 + k] = 1.0;
}
// x [13], Pa [16][16] in place (d is constant: it is in mk); Q [13][13] or nullptr, Qd [3] or nullptr
template <class K>
__host__ __device__ inline void ekf_aug_predict(double (&x)[13], double* Pa, const double (&u)[4], const int (&sel)[3], double T,
                                                int steps, const double* Q, const double* Qd, const K& mk) {
    constexpr int n = EKF_NA;
    const double h = T / steps;
    for (int s = 0; s < steps; s++) {
        double F[n * n], Y[n * n];
        ekf_aug_substep_jac(x, u, h, sel, F, mk);
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) {
                double acc = 0.0;
                for (int l = 0; l < n; l++) acc += F[i * n + l] * Pa[l * n + j];
                Y[i * n + j] = acc;
            }
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) {
                double acc = 0.0;
                for (int l = 0; l < n; l++) acc += Y[i * n + l] * F[j * n + l];
                Pa[i * n + j] = acc;
            }
        ekf_rk4_substep(x, u, h, mk);
    }
    if (Q)
        for (int a = 0; a < 13; a++)
            for (int b = 0; b < 13; b++) Pa[a * n + b] += Q[a * 13 + b];
    if (Qd)
        for (int k = 0; k < 3; k++)
            if (sel[k] >= 0) Pa[(13 + k) * (n + 1)] += Qd[k];
}
// a [16] = (x, the three slots) and Pa [16][16] in place: ekf_update's rules with a 16-entry gain column; only the 13 state
// components are measured
__host__ __device__ inline void ekf_aug_update(double (&a)[EKF_NA], double* Pa, const double* z_in, const double* r, double gate,
                                               int flags, double& nis, int (&counts)[2]) {
    constexpr int n = EKF_NA;
    double z[13];
    for (int j = 0; j < 13; j++) z[j] = z_in[j];
    double dot = 0.0;
    for (int j = 3; j < 7; j++)
        if (r[j] >= 0.0) dot += z[j] * a[j];
    if (dot < 0.0)
        for (int j = 3; j < 7; j++) z[j] = -z[j];
    nis = 0.0;
    counts[0] = 0; counts[1] = 0;
    for (int j = 0; j < 13; j++) {
        const EkfDec e = ekf_decide(Pa[j * (n + 1)], a[j], z[j], r[j], gate);
        if (e.skip) continue;
        if (e.rej) { counts[1]++; continue; }
        const double rs = 1.0 / e.s;
        double col[n], row[n];
        for (int i = 0; i < n; i++) { col[i] = Pa[i * n + j]; row[i] = Pa[j * n + i]; }
        for (int i = 0; i < n; i++) a[i] += (col[i] * e.nu) / e.s;
        for (int i = 0; i < n; i++)
            for (int b = 0; b < n; b++) Pa[i * n + b] -= (col[i] * row[b]) * rs;
        nis += e.nu * e.nu / e.s;
        counts[0]++;
    }
    if (flags & EKF_NORMALIZE_Q) {
        const double nq = sqrt(a[3] * a[3] + a[4] * a[4] + a[5] * a[5] + a[6] * a[6]);
        for (int j = 3; j < 7; j++) a[j] = a[j] / nq;
    }
}

}  // namespace cfn

#ifdef CFNMPC_EKF_KERNELS
namespace cfn {

// One instance per 16-lane row (k_unc_prop's mapping, four instances per wavefront): lane i < 13 holds row i of P and, in the
// update, entry i of the state.  Per sub-step every lane of a row
//   - rebuilds row i of A_s by the reverse sub-step seeded with e_i (lanes 13 .. 15: the zero seed),
//   - forms Y = A_s P (13 dotbc<13>: 169 broadcast FMAs) and P <- Y A_s' (13 rank1bc<13>: 169 more),
//   - integrates the nominal sub-step with rk4_steps (every lane the whole state: the bits of k_sim / k_sim_par / k_sim_dst).
// The update broadcasts P_jj, x_j, z_j, r_j and row j of P from lane j: 13 broadcast FMAs per component and lane.  The skip and
// gate decisions are values that are uniform over a 16-lane row and written as selects: the four rows of a wavefront differ
// freely, and where the compiler turns a select into a branch the 16 lanes of a row still share one EXEC state, which is what a
// DPP row broadcast needs.  The predict (the asm primitives) is straight-line code under the full mask.  Rows behind the batch
// recompute the last instance and store nothing.
// x_new may be x, P_new may be P: a row reads all of its instance before it writes any of it.
template <bool PAR, bool DST>
__device__ __forceinline__ void ekf_body(const EkfArgs& A) {
    const int L = threadIdx.x & 15;
    const int inst = blockIdx.x * 4 + (threadIdx.x >> 4);
    const bool valid = inst < A.B;
    const size_t i = (size_t)imin(inst, A.B - 1);
    const int Lc = imin(L, 12);
    ModelK<PAR, DST> mk;
    if constexpr (DST) {
        mk = dst_k_rows(A.p, A.d, (int)i);
    } else if constexpr (PAR) {
        double pr[NPAR], kr[NK];
        SFOR(e, 0, NPAR, { pr[e] = A.p[i * NPAR + e]; });
        derive_k(pr, kr);
        SFOR(e, 0, 8, { mk.c[e] = kr[e]; });
    }
    double xc[13], uc[4], S[13];
    SFOR(e, 0, 13, { xc[e] = gm(A.x)[i * 13 + e]; });
    SFOR(e, 0, 4, { uc[e] = gm(A.u)[i * 4 + e]; });
    SFOR(j, 0, 13, {
        const double v = gm(A.P)[i * 169 + Lc * 13 + j];
        S[j] = L < 13 ? v : 0.0;
    });
    const double h = A.T / A.steps;
    for (int s = 0; s < A.steps; s++) {
        // the sub-step's start state behind a barrier: the reverse sub-step's three stage evaluations are not merged with the
        // ones of rk4_steps below, whose arithmetic stays the one k_sim compiles
        double xs[13], lam[13], gu[4] = {0.0, 0.0, 0.0, 0.0};
        SFOR(e, 0, 13, { xs[e] = xc[e]; opaque(xs[e]); });
        SFOR(e, 0, 13, { lam[e] = L == e ? 1.0 : 0.0; });
        SimGrad G{};
        rk4_substep_vjp(xs, uc, h, lam, gu, G, mk);   // lam: row L of A_s (gu, G: not read, not computed)
        double Y[13];
        SFOR(j, 0, 13, {
            double acc = 0.0;
            dotbc<13, 0>(acc, lam, S[j]);
            Y[j] = acc;
        });
        SFOR(j, 0, 13, { S[j] = 0.0; });
        SFOR(l, 0, 13, { rank1bc<13>(S, Y[l], lam[l]); });
        // (the plant step as k_sim compiles it, so that it rounds where k_sim rounds: a step count the compiler cannot see keeps
        //  rk4_steps' loop, with the terms of u formed in front of it and rounded on their own, and copies of u, h and the
        //  constants it cannot see through keep those terms apart from the ones the reverse sub-step above forms)
        int one = 1;
        asm volatile("" : "+s"(one));
        double uf[4], hf = h;
        ModelK<PAR, DST> mf = mk;
        SFOR(e, 0, 4, { uf[e] = uc[e]; opaque(uf[e]); });
        opaque(hf);
        if constexpr (PAR) SFOR(e, 0, 8, { opaque(mf.c[e]); });
        if constexpr (DST) SFOR(e, 0, ND, { opaque(mf.d[e]); });
        rk4_steps(xc, uf, hf, one, mf);
    }
    if (A.Q) SFOR(j, 0, 13, { S[j] += gm(A.Q)[i * 169 + Lc * 13 + j]; });   // (wave-uniform)
    double xi = pick(xc, L), nis = 0.0;
    int used = 0, rejected = 0;
    if (A.z) {   // (wave-uniform)
        const bool isq = L >= 3 && L <= 6;
        double zi = gm(A.z)[i * 13 + Lc];
        const double ri = gm(A.r)[i * 13 + Lc];
        // (P comes out of the asm primitives and is read through compiler-generated DPP from here on)
        SFOR(j, 0, 13, { settle(S[j]); });
        const double qt = (isq && ri >= 0.0) ? zi * xi : 0.0;
        const double dot = ((bc<3>(qt) + bc<4>(qt)) + bc<5>(qt)) + bc<6>(qt);
        zi = (isq && dot < 0.0) ? -zi : zi;
        SFOR(j, 0, 13, {
            const EkfDec e = ekf_decide(bc<j>(S[j]), bc<j>(xi), bc<j>(zi), bc<j>(ri), A.gate);
            const bool use = !e.skip && !e.rej;
            const double rs = 1.0 / e.s, pij = S[j];
            double row[13];
            SFOR(b, 0, 13, { row[b] = bc<j>(S[b]); });
            xi = use ? xi + (pij * e.nu) / e.s : xi;
            SFOR(b, 0, 13, {
                const double t = pij * row[b];
                S[b] = use ? __builtin_fma(-t, rs, S[b]) : S[b];
            });
            nis = use ? nis + e.nu * e.nu / e.s : nis;
            used += use ? 1 : 0;
            rejected += (!e.skip && e.rej) ? 1 : 0;
        });
        if (A.flags & EKF_NORMALIZE_Q) {
            const double qq = isq ? xi * xi : 0.0;
            const double n = sqrt(((bc<3>(qq) + bc<4>(qq)) + bc<5>(qq)) + bc<6>(qq));
            xi = isq ? xi / n : xi;
        }
    }
    if (valid && L < 13) {
        gm(A.xn)[i * 13 + L] = xi;
        SFOR(b, 0, 13, { gm(A.Pn)[i * 169 + L * 13 + b] = S[b]; });
    }
    if (valid && L == 0) {
        if (A.nis) gm(A.nis)[i] = nis;
        if (A.counts) { gm(A.counts)[i * 2] = used; gm(A.counts)[i * 2 + 1] = rejected; }
    }
}
__global__ __launch_bounds__(64) void k_ekf(EkfArgs A) { ekf_body<false, false>(A); }
__global__ __launch_bounds__(64) void k_ekf_par(EkfArgs A) { ekf_body<true, false>(A); }
__global__ __launch_bounds__(64) void k_ekf_dst(EkfArgs A) { ekf_body<true, true>(A); }

// the twin is chosen by the inputs alone, as launch_sim_rollout: d set: the disturbed twin (p or the nominal row); p alone: the
// parameter twin; else the folded constants
void launch_ekf(const EkfArgs& A, hipStream_t st) {
    const dim3 g((A.B + 3) / 4), b(64);
    if (A.d) hipLaunchKernelGGL(k_ekf_dst, g, b, 0, st, A);
    else if (A.p) hipLaunchKernelGGL(k_ekf_par, g, b, 0, st, A);
    else hipLaunchKernelGGL(k_ekf, g, b, 0, st, A);
}

// The disturbance-augmented filter (cfnmpc_ekf_aug_step): ekf_body's mapping with all 16 lanes of a row live -- lane L holds row L
// of the 16 x 16 Pa and, in the update, entry L of a = (x, slot 0, slot 1, slot 2).  Always the disturbed twin.  Per sub-step
//   - lane L < 13 rebuilds row L of F_s = [[A_s, G_s S], [0, I]]: lam from the reverse sub-step seeded with e_L, and g[k] = the
//     entry sel[k] of that sweep's gd (a wave-uniform select over the six; a zero for an unused slot; gk stays dead); lanes
//     13 .. 15 carry the zero seed and g[k] = (L == 13 + k): their rows of F_s, so that both products are uniform over the row,
//   - Y = F Pa: per column dotbc<13, 0> over lam plus dotbc<3, 13> over g (16 x 16 broadcast FMAs),
//   - Pa <- Y F': the 13 state columns take 16 rank1bc<13> (sources lam[l], then g[l - 13]); the slot columns are Y[13 + k],
//   - the nominal sub-step by ekf_body's recipe (the bits of k_sim_dst).
// The update is ekf_body's with a 16-entry gain column and 16 x 16 rank-one terms; j runs over the 13 measured components.
// d_new: lanes 13 + k store the used slots, lanes e < 6 copy the components no slot estimates.  x_new, d_new, Pa_new may be the
// inputs: a row reads all of its instance before it writes any of it (z, r, Q, Qd are no outputs).
__global__ __launch_bounds__(64) void k_ekf_aug(EkfAugArgs A) {
    const int L = threadIdx.x & 15;
    const int inst = blockIdx.x * 4 + (threadIdx.x >> 4);
    const bool valid = inst < A.B;
    const size_t i = (size_t)imin(inst, A.B - 1);
    const int Lc = imin(L, 12);
    const DstK mk = dst_k_rows(A.p, A.d, (int)i);
    double xc[13], uc[4], S[16];
    SFOR(e, 0, 13, { xc[e] = gm(A.x)[i * 13 + e]; });
    SFOR(e, 0, 4, { uc[e] = gm(A.u)[i * 4 + e]; });
    SFOR(j, 0, 16, { S[j] = gm(A.Pa)[i * 256 + L * 16 + j]; });
    double dsl = 0.0;   // lane 13 + k: the slot's component of d (0 for an unused slot)
    SFOR(k, 0, 3, {
        const double v = A.sel[k] >= 0 ? pick(mk.d, A.sel[k]) : 0.0;   // (wave-uniform)
        dsl = L == 13 + k ? v : dsl;
    });
    const double h = A.T / A.steps;
    for (int s = 0; s < A.steps; s++) {
        double xs[13], lam[13], g[3], gu[4] = {0.0, 0.0, 0.0, 0.0};
        SFOR(e, 0, 13, { xs[e] = xc[e]; opaque(xs[e]); });
        SFOR(e, 0, 13, { lam[e] = L == e ? 1.0 : 0.0; });
        SimGrad G{};
        rk4_substep_vjp(xs, uc, h, lam, gu, G, mk);   // lam: row L of A_s, G.gd: row L of G_s (gu, G.gk: not read, not computed)
        SFOR(k, 0, 3, {
            const double v = A.sel[k] >= 0 ? pick(G.gd, A.sel[k]) : 0.0;   // (wave-uniform)
            g[k] = L < 13 ? v : (L == 13 + k ? 1.0 : 0.0);
        });
        double Y[16];
        SFOR(j, 0, 16, {
            double acc = 0.0;
            dotbc<13, 0>(acc, lam, S[j]);
            dotbc<3, 13>(acc, g, S[j]);
            Y[j] = acc;
        });
        SFOR(j, 0, 13, { S[j] = 0.0; });
        SFOR(l, 0, 13, { rank1bc<13>(S, Y[l], lam[l]); });
        SFOR(k, 0, 3, { rank1bc<13>(S, Y[13 + k], g[k]); });
        SFOR(k, 0, 3, { S[13 + k] = Y[13 + k]; });
        // (the plant step as k_sim_dst compiles it: ekf_body's recipe)
        int one = 1;
        asm volatile("" : "+s"(one));
        double uf[4], hf = h;
        DstK mf = mk;
        SFOR(e, 0, 4, { uf[e] = uc[e]; opaque(uf[e]); });
        opaque(hf);
        SFOR(e, 0, 8, { opaque(mf.c[e]); });
        SFOR(e, 0, ND, { opaque(mf.d[e]); });
        rk4_steps(xc, uf, hf, one, mf);
    }
    if (A.Q) SFOR(j, 0, 13, {   // (wave-uniform)
        const double q = gm(A.Q)[i * 169 + Lc * 13 + j];
        S[j] += L < 13 ? q : 0.0;
    });
    if (A.Qd) SFOR(k, 0, 3, {
        const double q = gm(A.Qd)[i * 3 + k];
        S[13 + k] += (L == 13 + k && A.sel[k] >= 0) ? q : 0.0;
    });
    const double xl = pick(xc, L);
    double ai = L < 13 ? xl : dsl, nis = 0.0;
    int used = 0, rejected = 0;
    if (A.z) {   // (wave-uniform)
        const bool isq = L >= 3 && L <= 6;
        double zi = gm(A.z)[i * 13 + Lc];
        const double ri = gm(A.r)[i * 13 + Lc];
        SFOR(j, 0, 16, { settle(S[j]); });
        const double qt = (isq && ri >= 0.0) ? zi * ai : 0.0;
        const double dot = ((bc<3>(qt) + bc<4>(qt)) + bc<5>(qt)) + bc<6>(qt);
        zi = (isq && dot < 0.0) ? -zi : zi;
        SFOR(j, 0, 13, {
            const EkfDec e = ekf_decide(bc<j>(S[j]), bc<j>(ai), bc<j>(zi), bc<j>(ri), A.gate);
            const bool use = !e.skip && !e.rej;
            const double rs = 1.0 / e.s, pij = S[j];
            double row[16];
            SFOR(b, 0, 16, { row[b] = bc<j>(S[b]); });
            ai = use ? ai + (pij * e.nu) / e.s : ai;
            SFOR(b, 0, 16, {
                const double t = pij * row[b];
                S[b] = use ? __builtin_fma(-t, rs, S[b]) : S[b];
            });
            nis = use ? nis + e.nu * e.nu / e.s : nis;
            used += use ? 1 : 0;
            rejected += (!e.skip && e.rej) ? 1 : 0;
        });
        if (A.flags & EKF_NORMALIZE_Q) {
            const double qq = isq ? ai * ai : 0.0;
            const double n = sqrt(((bc<3>(qq) + bc<4>(qq)) + bc<5>(qq)) + bc<6>(qq));
            ai = isq ? ai / n : ai;
        }
    }
    if (valid) {
        if (L < 13) gm(A.xn)[i * 13 + L] = ai;
        SFOR(b, 0, 16, { gm(A.Pan)[i * 256 + L * 16 + b] = S[b]; });
        if (A.Pxx && L < 13) SFOR(b, 0, 13, { gm(A.Pxx)[i * 169 + L * 13 + b] = S[b]; });
        if (L < ND && L != A.sel[0] && L != A.sel[1] && L != A.sel[2]) gm(A.dn)[i * ND + L] = pick(mk.d, L);
        SFOR(k, 0, 3, { if (L == 13 + k && A.sel[k] >= 0) gm(A.dn)[i * ND + A.sel[k]] = ai; });
    }
    if (valid && L == 0) {
        if (A.nis) gm(A.nis)[i] = nis;
        if (A.counts) { gm(A.counts)[i * 2] = used; gm(A.counts)[i * 2 + 1] = rejected; }
    }
}

void launch_ekf_aug(const EkfAugArgs& A, hipStream_t st) {
    hipLaunchKernelGGL(k_ekf_aug, dim3((A.B + 3) / 4), dim3(64), 0, st, A);
}

}  // namespace cfn
#endif
