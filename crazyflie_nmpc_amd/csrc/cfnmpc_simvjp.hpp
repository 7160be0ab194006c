// cfnmpc_simvjp.hpp -- differentiable plant rollouts: the open-loop rollout of the RK4 plant and the reverse sweep through it
// (cfnmpc_sim_rollout / cfnmpc_sim_rollout_vjp).
//
// Two parts.  The first needs cfnmpc_model.hpp only and compiles for the host as well (tools/sim_vjp_check.cpp runs it under the
// host sanitizers): the transposed products of f with respect to the inputs, the eight derived constants and the disturbance row,
// the reverse of one RK4 sub-step, and the transpose of derive_k's Jacobian.  The second, the kernels, is compiled where
// cfnmpc_kernels.hip includes this file at its end (CFNMPC_SIMVJP_KERNELS: its rk4_steps, ModelK; no device unit of its own and
// no field of Params: the calls are solver-free like cfnmpc_sim).
//
// Reverse of one sub-step x+ = x + h/6 (k1 + 2 k2 + 2 k3 + k4), with lambda = dl/dx+ and Ji = (df/dx)(stage point i):
//     k4~ = h/6 lambda,   k3~ = h/3 lambda + h J4' k4~,   k2~ = h/3 lambda + h/2 J3' k3~,   k1~ = h/6 lambda + h/2 J2' k2~,
//     lambda <- lambda + sum_i Ji' ki~
// and every other argument a of f collects sum_i (df/da)(stage point i)' ki~.  df/du and the rotor columns of df/dk do not depend
// on the stage point (u is held over the interval), so they take the four ki~ summed; the gravity, gyroscopic and disturbance
// columns are taken point by point.
#pragma once
#include "cfnmpc_model.hpp"

namespace cfn {

// what a reverse sweep collects beside lambda: gk in the space of the eight derived constants (g0, KT, KA, KB, KC, KWX, KWY, KWZ),
// gd in the disturbance row's.  f is linear in both, so every K type collects both: the gradient at the nominal row (p = NULL) and
// at the zero row (d = NULL) needs no other kernel than the one the inputs select, and an output that is not asked for changes
// nothing in the others' arithmetic.
struct SimGrad {
    double gk[8];
    double gd[ND];
};

// the point-dependent columns of (df/dk)' v and (df/dd)' v at one stage point: gravity (-g0 R' e_z), the gyroscopic couplings, and
// R' a_w (whose a_z column is the gravity column with the sign turned: both are written from one product)
__host__ __device__ __forceinline__ void fk_point_t(const JacPoint& J, const double* __restrict__ v, SimGrad& G) {
    const double rz = J.R[6] * v[7] + J.R[7] * v[8] + J.R[8] * v[9];
    G.gk[0] -= rz;
    G.gk[5] += (J.w[1] * J.w[2]) * v[10];
    G.gk[6] += (J.w[0] * J.w[2]) * v[11];
    G.gk[7] += (J.w[0] * J.w[1]) * v[12];
    G.gd[0] += J.R[0] * v[7] + J.R[1] * v[8] + J.R[2] * v[9];
    G.gd[1] += J.R[3] * v[7] + J.R[4] * v[8] + J.R[5] * v[9];
    G.gd[2] += rz;
}

// the columns that do not depend on the stage point, for vs = the four stages' cotangent rows 9 .. 12 summed: (df/du)' (with the
// constants of this instance: ju_col holds the folded ones), the rotor columns of (df/dk)', and the body-rate rows of (df/dd)'
template <class K>
__host__ __device__ __forceinline__ void fu_t(const double* __restrict__ u, const double (&vs)[4], double* __restrict__ gu, SimGrad& G,
                                              const K& mk) {
    const double s1 = u[0] * u[0], s2 = u[1] * u[1], s3 = u[2] * u[2], s4 = u[3] * u[3];
    const double t = mk.kt() * vs[0], a = mk.ka() * vs[1], b = mk.kb() * vs[2], c = mk.kc() * vs[3];
    gu[0] += 2.0 * u[0] * (t + a + b + c);
    gu[1] += 2.0 * u[1] * (t + a - b - c);
    gu[2] += 2.0 * u[2] * (t - a - b + c);
    gu[3] += 2.0 * u[3] * (t - a + b - c);
    G.gk[1] += (s1 + s2 + s3 + s4) * vs[0];
    G.gk[2] += (s1 + s2 - s3 - s4) * vs[1];
    G.gk[3] += (s1 - s2 - s3 + s4) * vs[2];
    G.gk[4] += (s1 - s2 + s3 - s4) * vs[3];
    G.gd[3] += vs[1]; G.gd[4] += vs[2]; G.gd[5] += vs[3];
}

// Reverse of ONE RK4 sub-step of h from x (its start state): lam = dl/dx+ in, dl/dx out; gu and G are added to.  The stage points
// are rebuilt from x (three evaluations of f: k4 is not needed), then visited last to first with one Jacobian point alive.
template <class K>
__host__ __device__ __forceinline__ void rk4_substep_vjp(const double (&x)[13], const double (&u)[4], double h, double (&lam)[13],
                                                         double (&gu)[4], SimGrad& G, const K& mk) {
    double x2[13], x3[13], x4[13], kk[13];
    f_expl(x, u, kk, mk);
#pragma unroll
    for (int e = 0; e < 13; e++) x2[e] = x[e] + 0.5 * h * kk[e];
    f_expl(x2, u, kk, mk);
#pragma unroll
    for (int e = 0; e < 13; e++) x3[e] = x[e] + 0.5 * h * kk[e];
    f_expl(x3, u, kk, mk);
#pragma unroll
    for (int e = 0; e < 13; e++) x4[e] = x[e] + h * kk[e];
    JacPoint J;
    double kb[13], jt[13], acc[13], vs[4];
    // stage 4
#pragma unroll
    for (int e = 0; e < 13; e++) kb[e] = (h / 6.0) * lam[e];
    jac_point(x4, J);
    jtvp(J, kb, jt, mk);
    fk_point_t(J, kb, G);
#pragma unroll
    for (int e = 0; e < 4; e++) vs[e] = kb[9 + e];
#pragma unroll
    for (int e = 0; e < 13; e++) acc[e] = jt[e];
    // stage 3
#pragma unroll
    for (int e = 0; e < 13; e++) kb[e] = (h / 3.0) * lam[e] + h * jt[e];
    jac_point(x3, J);
    jtvp(J, kb, jt, mk);
    fk_point_t(J, kb, G);
#pragma unroll
    for (int e = 0; e < 4; e++) vs[e] += kb[9 + e];
#pragma unroll
    for (int e = 0; e < 13; e++) acc[e] += jt[e];
    // stage 2
#pragma unroll
    for (int e = 0; e < 13; e++) kb[e] = (h / 3.0) * lam[e] + 0.5 * h * jt[e];
    jac_point(x2, J);
    jtvp(J, kb, jt, mk);
    fk_point_t(J, kb, G);
#pragma unroll
    for (int e = 0; e < 4; e++) vs[e] += kb[9 + e];
#pragma unroll
    for (int e = 0; e < 13; e++) acc[e] += jt[e];
    // stage 1
#pragma unroll
    for (int e = 0; e < 13; e++) kb[e] = (h / 6.0) * lam[e] + 0.5 * h * jt[e];
    jac_point(x, J);
    jtvp(J, kb, jt, mk);
    fk_point_t(J, kb, G);
#pragma unroll
    for (int e = 0; e < 4; e++) vs[e] += kb[9 + e];
#pragma unroll
    for (int e = 0; e < 13; e++) lam[e] += acc[e] + jt[e];
    fu_t(u, vs, gu, G, mk);
}

// gp = (d derive_k / dp)' gk: the gradient with respect to the public row p = [g0, mq, Ixx, Iyy, Izz, Cd, Ct, l] from the one with
// respect to the eight derived constants (the hover-speed entry k[8] plays no part: no model function reads it)
__host__ __device__ inline void derive_k_t(const double* p, const double* gk, double* gp) {
    const double mq = p[1], ixx = p[2], iyy = p[3], izz = p[4], cd = p[5], ct = p[6], arm = p[7];
    const double rx = 1.0 / ixx, ry = 1.0 / iyy, rz = 1.0 / izz, rm = 1.0 / mq;
    gp[0] = gk[0];
    gp[1] = -gk[1] * ct * rm * rm;
    gp[2] = (gk[2] * ct * arm + gk[5] * (izz - iyy)) * rx * rx - gk[6] * ry + gk[7] * rz;
    gp[3] = (gk[3] * ct * arm + gk[6] * (ixx - izz)) * ry * ry + gk[5] * rx - gk[7] * rz;
    gp[4] = (gk[4] * cd + gk[7] * (iyy - ixx)) * rz * rz - gk[5] * rx + gk[6] * ry;
    gp[5] = -gk[4] * rz;
    gp[6] = gk[1] * rm - arm * (gk[2] * rx + gk[3] * ry);
    gp[7] = -ct * (gk[2] * rx + gk[3] * ry);
}

}  // namespace cfn

#ifdef CFNMPC_SIMVJP_KERNELS
namespace cfn {

// the constants (and, DST, the disturbance) of lane i: p [B][NPAR] (PAR; NULL = the nominal row), d [B][ND] (DST);
// pr: the parameter row the constants belong to (derive_k_t's point)
template <bool PAR, bool DST>
__device__ __forceinline__ ModelK<PAR, DST> rollout_k(const double* __restrict__ p, const double* __restrict__ d, int i,
                                                      double (&pr)[NPAR]) {
    ModelK<PAR, DST> mk;
    const double nom[NPAR] = {G0, MQ, IXX, IYY, IZZ, CD, CT, 0.0325};
    SFOR(e, 0, NPAR, { pr[e] = nom[e]; });
    if constexpr (PAR) {
        if (p) SFOR(e, 0, NPAR, { pr[e] = p[(size_t)i * NPAR + e]; });
        double kr[NK];
        derive_k(pr, kr);
        SFOR(e, 0, 8, { mk.c[e] = kr[e]; });
    }
    if constexpr (DST) SFOR(e, 0, ND, { mk.d[e] = d[(size_t)i * ND + e]; });
    return mk;
}

// Open-loop rollout, one instance per lane: xs[i][0] = x0[i], xs[i][t + 1] = rk4_steps(xs[i][t], u[i][t]) -- the function and the
// constant types of sim_body, so a step has the bits of k_sim / k_sim_par / k_sim_dst.
template <bool PAR, bool DST>
__device__ __forceinline__ void rollout_body(int B, int L, const double* __restrict__ x0, const double* __restrict__ u,
                                             const double* __restrict__ p, const double* __restrict__ d, double T, int steps,
                                             double* __restrict__ xs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    ModelK<PAR, DST> mk;
    if constexpr (DST) {
        mk = dst_k_rows(p, d, i);
    } else if constexpr (PAR) {
        double pr[NPAR], kr[NK];
        SFOR(e, 0, NPAR, { pr[e] = p[(size_t)i * NPAR + e]; });
        derive_k(pr, kr);
        SFOR(e, 0, 8, { mk.c[e] = kr[e]; });
    }
    double xc[13], uc[4];
    double* xo = xs + (size_t)i * (L + 1) * 13;
    const double* ui = u + (size_t)i * L * 4;
#pragma unroll
    for (int e = 0; e < 13; e++) { xc[e] = x0[(size_t)i * 13 + e]; xo[e] = xc[e]; }
    for (int t = 0; t < L; t++) {
#pragma unroll
        for (int e = 0; e < 4; e++) uc[e] = ui[(size_t)t * 4 + e];
        rk4_steps(xc, uc, T / steps, steps, mk);
#pragma unroll
        for (int e = 0; e < 13; e++) xo[(size_t)(t + 1) * 13 + e] = xc[e];
    }
}
__global__ __launch_bounds__(256) void k_sim_rollout(int B, int L, const double* __restrict__ x0, const double* __restrict__ u,
                          double T, int steps, double* __restrict__ xs) {
    rollout_body<false, false>(B, L, x0, u, nullptr, nullptr, T, steps, xs);
}
__global__ __launch_bounds__(256) void k_sim_rollout_par(int B, int L, const double* __restrict__ x0, const double* __restrict__ u,
                          const double* __restrict__ p, double T, int steps, double* __restrict__ xs) {
    rollout_body<true, false>(B, L, x0, u, p, nullptr, T, steps, xs);
}
__global__ __launch_bounds__(256) void k_sim_rollout_dst(int B, int L, const double* __restrict__ x0, const double* __restrict__ u,
                          const double* __restrict__ p, const double* __restrict__ d, double T, int steps, double* __restrict__ xs) {
    rollout_body<true, true>(B, L, x0, u, p, d, T, steps, xs);
}

// Reverse sweep, one instance per lane, t = L - 1 .. 0, sub-steps last to first.  The start state of sub-step s of step t is
// recomputed from the STORED xs[i][t] by s forward sub-steps (rk4_steps: the forward pass's own bits), so a step costs
// steps (steps - 1) / 2 forward sub-steps beside its `steps` reverse ones, and no state is kept per sub-step.  Every sum runs in
// this lane in the sweep's order: no atomics, two calls agree bit for bit.  gu / gp / gd may be NULL (skipped).
template <bool PAR, bool DST>
__device__ __forceinline__ void rollout_vjp_body(int B, int L, const double* __restrict__ xs, const double* __restrict__ u,
                                                 const double* __restrict__ p, const double* __restrict__ d, double T, int steps,
                                                 const double* __restrict__ gxs, double* __restrict__ gx0, double* __restrict__ gu,
                                                 double* __restrict__ gp, double* __restrict__ gd) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    double pr[NPAR];
    const ModelK<PAR, DST> mk = rollout_k<PAR, DST>(p, d, i, pr);
    const double h = T / steps;
    const double* xi = xs + (size_t)i * (L + 1) * 13;
    const double* gi = gxs + (size_t)i * (L + 1) * 13;
    const double* ui = u + (size_t)i * L * 4;
    SimGrad G;
    SFOR(e, 0, 8, { G.gk[e] = 0.0; });
    SFOR(e, 0, ND, { G.gd[e] = 0.0; });
    double lam[13];
#pragma unroll
    for (int e = 0; e < 13; e++) lam[e] = gi[(size_t)L * 13 + e];
    for (int t = L - 1; t >= 0; t--) {
        double xt[13], uc[4], gut[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int e = 0; e < 13; e++) xt[e] = xi[(size_t)t * 13 + e];
#pragma unroll
        for (int e = 0; e < 4; e++) uc[e] = ui[(size_t)t * 4 + e];
        for (int s = steps - 1; s >= 0; s--) {
            double xc[13];
#pragma unroll
            for (int e = 0; e < 13; e++) xc[e] = xt[e];
            if (s > 0) rk4_steps(xc, uc, h, s, mk);
            rk4_substep_vjp(xc, uc, h, lam, gut, G, mk);
        }
#pragma unroll
        for (int e = 0; e < 13; e++) lam[e] += gi[(size_t)t * 13 + e];
        if (gu) {
#pragma unroll
            for (int e = 0; e < 4; e++) gu[((size_t)i * L + t) * 4 + e] = gut[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 13; e++) gx0[(size_t)i * 13 + e] = lam[e];
    if (gp) {
        double gpr[NPAR];
        derive_k_t(pr, G.gk, gpr);
        SFOR(e, 0, NPAR, { gp[(size_t)i * NPAR + e] = gpr[e]; });
    }
    if (gd) SFOR(e, 0, ND, { gd[(size_t)i * ND + e] = G.gd[e]; });
}
__global__ __launch_bounds__(256) void k_sim_rollout_vjp(int B, int L, const double* __restrict__ xs, const double* __restrict__ u,
                          double T, int steps, const double* __restrict__ gxs, double* __restrict__ gx0, double* __restrict__ gu,
                          double* __restrict__ gp, double* __restrict__ gd) {
    rollout_vjp_body<false, false>(B, L, xs, u, nullptr, nullptr, T, steps, gxs, gx0, gu, gp, gd);
}
__global__ __launch_bounds__(256) void k_sim_rollout_vjp_par(int B, int L, const double* __restrict__ xs, const double* __restrict__ u,
                          const double* __restrict__ p, double T, int steps, const double* __restrict__ gxs,
                          double* __restrict__ gx0, double* __restrict__ gu, double* __restrict__ gp, double* __restrict__ gd) {
    rollout_vjp_body<true, false>(B, L, xs, u, p, nullptr, T, steps, gxs, gx0, gu, gp, gd);
}
__global__ __launch_bounds__(256) void k_sim_rollout_vjp_dst(int B, int L, const double* __restrict__ xs, const double* __restrict__ u,
                          const double* __restrict__ p, const double* __restrict__ d, double T, int steps,
                          const double* __restrict__ gxs, double* __restrict__ gx0, double* __restrict__ gu,
                          double* __restrict__ gp, double* __restrict__ gd) {
    rollout_vjp_body<true, true>(B, L, xs, u, p, d, T, steps, gxs, gx0, gu, gp, gd);
}

// p == NULL && d == NULL: the folded constants; d set: the disturbed twin (p or the nominal row); else the parameter twin
void launch_sim_rollout(int B, int L, const double* x0, const double* u, const double* p, const double* d, double T, int steps,
                        double* xs, hipStream_t st) {
    const dim3 g((B + 255) / 256), b(256);
    if (d) hipLaunchKernelGGL(k_sim_rollout_dst, g, b, 0, st, B, L, x0, u, p, d, T, steps, xs);
    else if (p) hipLaunchKernelGGL(k_sim_rollout_par, g, b, 0, st, B, L, x0, u, p, T, steps, xs);
    else hipLaunchKernelGGL(k_sim_rollout, g, b, 0, st, B, L, x0, u, T, steps, xs);
}
// the twin is chosen by the inputs alone, as above: every twin writes whichever of gu, gp, gd is asked for
void launch_sim_rollout_vjp(int B, int L, const double* xs, const double* u, const double* p, const double* d, double T, int steps,
                            const double* gxs, double* gx0, double* gu, double* gp, double* gd, hipStream_t st) {
    const dim3 g((B + 255) / 256), b(256);
    if (d) hipLaunchKernelGGL(k_sim_rollout_vjp_dst, g, b, 0, st, B, L, xs, u, p, d, T, steps, gxs, gx0, gu, gp, gd);
    else if (p) hipLaunchKernelGGL(k_sim_rollout_vjp_par, g, b, 0, st, B, L, xs, u, p, T, steps, gxs, gx0, gu, gp, gd);
    else hipLaunchKernelGGL(k_sim_rollout_vjp, g, b, 0, st, B, L, xs, u, T, steps, gxs, gx0, gu, gp, gd);
}

}  // namespace cfn
#endif
