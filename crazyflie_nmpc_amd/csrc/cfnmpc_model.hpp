// cfnmpc_model.hpp -- Crazyflie 13-state / 4-input model on the device (gfx950, FP64).
//
// Restates, for the GPU, the continuous dynamics of
//   crazyflie_controller/scripts/crazyflie_full_model/export_ode_model.py:33-102
// and the structure of its RK4 sensitivities.  State order (acados_mpc.cpp:117-131)
//   x = [ p(0..2) | q(3..6: w x y z) | v(7..9, body frame) | w(10..12, body rates) ],  u = kRPM(4).
//
// Nothing depends on p, q' depends on (q,w), v' on (q,v,w,u), w' on (w,u), p' on (q,v):
// influence graph  w -> q -> v -> p.  Hence d Phi / d x of ANY explicit RK scheme has the
// block pattern (rows x cols, blocks p,q,v,w)
//        p  q  v  w
//    p [ I  *  *  * ]
//    q [ 0  *  0  * ]        97 stored entries + 3 unit entries instead of 169,
//    v [ 0  *  *  * ]
//    w [ 0  0  0  * ]
// which the linearisation kernel writes and the Riccati kernels read in compact form.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <utility>

namespace cfn {

constexpr int NX = 13, NU = 4, NY = 17;

// export_ode_model.py:34-42
constexpr double G0 = 9.8066, MQ = 33e-3, IXX = 1.395e-5, IYY = 1.395e-5, IZZ = 2.173e-5,
                 CD = 7.9379e-06, CT = 3.25e-4, ARM = 65e-3 / 2;
constexpr double KWX = -(IZZ - IYY) / IXX, KWY = -(IXX - IZZ) / IYY, KWZ = -(IYY - IXX) / IZZ;
constexpr double KT = CT / MQ, KA = -CT * ARM / IXX, KB = -CT * ARM / IYY, KC = -CD / IZZ;

// ---- model constants (cfnmpc_set_model_params) ------------------------------------------------
// The model functions below take the eight constants they use through K: NomK folds the ones above at compile time (the
// default of every model function, so the folded-constant kernels compile to what they were without K); ParK holds one
// instance's own values, derived on the host (derive_k) from a parameter row p = [g0, mq, Ixx, Iyy, Izz, Cd, Ct, l] by the
// same expressions, so that the nominal row gives bit-identical constants.
constexpr int NPAR = 8;   // parameters per instance (include/cfnmpc.h: CFNMPC_NP)
constexpr int NK = 9;     // device rows per instance: g0, KT, KA, KB, KC, KWX, KWY, KWZ | hover speed sqrt(mq g0 / (4 Ct))
struct NomK {
    __host__ __device__ static constexpr double g0() { return G0; }
    __host__ __device__ static constexpr double kt() { return KT; }
    __host__ __device__ static constexpr double ka() { return KA; }
    __host__ __device__ static constexpr double kb() { return KB; }
    __host__ __device__ static constexpr double kc() { return KC; }
    __host__ __device__ static constexpr double kwx() { return KWX; }
    __host__ __device__ static constexpr double kwy() { return KWY; }
    __host__ __device__ static constexpr double kwz() { return KWZ; }
};
struct ParK {
    double c[8];   // g0, KT, KA, KB, KC, KWX, KWY, KWZ
    __host__ __device__ double g0() const { return c[0]; }
    __host__ __device__ double kt() const { return c[1]; }
    __host__ __device__ double ka() const { return c[2]; }
    __host__ __device__ double kb() const { return c[3]; }
    __host__ __device__ double kc() const { return c[4]; }
    __host__ __device__ double kwx() const { return c[5]; }
    __host__ __device__ double kwy() const { return c[6]; }
    __host__ __device__ double kwz() const { return c[7]; }
};
// ---- external disturbance (cfnmpc_set_disturbance) ----------------------------------------------
// A disturbance row d = [ax, ay, az | alx, aly, alz]: a_w = d[0:3] an acceleration in the WORLD frame [m/s^2], al_b = d[3:6] an
// angular acceleration in the BODY frame [rad/s^2]:   v_b' += R(q)' a_w,   w' += al_b   (R of p' = R(q) v_b, JacPoint::R).
// al_b adds nothing to df/dx; R(q)' a_w adds to d v_b' / d q only, the block gravity already occupies (-g0 R' e_z is the
// disturbance (0, 0, -g0)): the pattern of A is unchanged.  A K type that has dax() .. dlz() carries one instance's row next to
// its constants (DstK; DstKG in cfnmpc_kernels.hip reads it at its uses); for every other K the terms below are not compiled.
constexpr int ND = 6;     // include/cfnmpc.h: CFNMPC_ND
template <class K, class = void> struct has_dist : std::false_type {};
template <class K> struct has_dist<K, std::void_t<decltype(std::declval<const K&>().dax())>> : std::true_type {};
struct DstK : ParK {
    double d[ND];
    __host__ __device__ double dax() const { return d[0]; }
    __host__ __device__ double day() const { return d[1]; }
    __host__ __device__ double daz() const { return d[2]; }
    __host__ __device__ double dlx() const { return d[3]; }
    __host__ __device__ double dly() const { return d[4]; }
    __host__ __device__ double dlz() const { return d[5]; }
};
// every entry finite, any sign (cfnmpc_set_disturbance, cfnmpc_sim_dist, cfnmpc_estimate_disturbance)
inline bool dist_rows_ok(const double* d, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!(d[i] >= -1.7976931348623157e308 && d[i] <= 1.7976931348623157e308)) return false;   // (NaN fails both)
    return true;
}
// the nominal parameter row (export_ode_model.py:34-42; l = 0.0325 is ARM exactly)
constexpr double NOM_P[NPAR] = {G0, MQ, IXX, IYY, IZZ, CD, CT, 0.0325};
static_assert(NOM_P[7] == ARM, "nominal arm length");
// every entry finite and > 0 (cfnmpc_set_model_params, cfnmpc_sim_params)
inline bool model_params_ok(const double* p, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!(p[i] > 0.0 && p[i] <= 1.7976931348623157e308)) return false;   // (NaN fails both)
    return true;
}
// rows of cfnmpc_set_weights_batch, W [B][17] and / or WN [B][13]: every entry finite, state and terminal weights >= 0, input
// weights > 0 (NaN fails the comparisons)
inline bool weight_rows_ok(const double* W, const double* WN, size_t B) {
    const double big = 1.7976931348623157e308;
    if (W) for (size_t i = 0; i < B * 17; i++) if (!(W[i] >= 0.0 && W[i] <= big) || (i % 17 >= 13 && !(W[i] > 0.0))) return false;
    if (WN) for (size_t i = 0; i < B * 13; i++) if (!(WN[i] >= 0.0 && WN[i] <= big)) return false;
    return true;
}
// p[NPAR] -> k[NK] (the expressions of the constants above, term for term)
__host__ __device__ inline void derive_k(const double* p, double* k) {
    const double g0 = p[0], mq = p[1], ixx = p[2], iyy = p[3], izz = p[4], cd = p[5], ct = p[6], arm = p[7];
    k[0] = g0;
    k[1] = ct / mq; k[2] = -ct * arm / ixx; k[3] = -ct * arm / iyy; k[4] = -cd / izz;
    k[5] = -(izz - iyy) / ixx; k[6] = -(ixx - izz) / iyy; k[7] = -(iyy - ixx) / izz;
    k[8] = sqrt((mq * g0) / (4 * ct));
}

// ---- compact pattern of A = d Phi / d x -------------------------------------------------
__host__ __device__ constexpr int blk(int i) { return i < 3 ? 0 : (i < 7 ? 1 : (i < 10 ? 2 : 3)); }
// 0: structural zero, 1: unit entry (p-block diagonal), 2: stored
__host__ __device__ constexpr int a_kind(int r, int c) {
    const int br = blk(r), bc = blk(c);
    if (bc == 0) return (r == c) ? 1 : 0;
    if (bc == 1) return (br <= 2) ? 2 : 0;
    if (bc == 2) return (br == 0 || br == 2) ? 2 : 0;
    return 2;
}
__host__ __device__ constexpr int a_idx(int r, int c) {  // row-major rank among stored entries
    int n = 0;
    for (int i = 0; i < NX; i++)
        for (int j = 0; j < NX; j++) {
            if (i == r && j == c) return n;
            if (a_kind(i, j) == 2) n++;
        }
    return n;
}
constexpr int A_NNZ = a_idx(NX - 1, NX - 1) + 1;  // 97
static_assert(A_NNZ == 97, "pattern of dPhi/dx");

// packed symmetric 13x13 (upper, row-major): index of (i,j), any order of i,j
__host__ __device__ constexpr int sidx(int i, int j) {
    const int a = i < j ? i : j, b = i < j ? j : i;
    return a * NX - (a * (a - 1)) / 2 + (b - a);
}
constexpr int S_NNZ = 91;
// packed symmetric 4x4
__host__ __device__ constexpr int s4(int i, int j) {
    const int a = i < j ? i : j, b = i < j ? j : i;
    return a * 4 - (a * (a - 1)) / 2 + (b - a);
}

// ---- continuous dynamics ----------------------------------------------------------------
// (f_expl, jac_point and jtvp also compile for the host, with the K types' accessors: the reverse RK4 sub-step of
//  cfnmpc_simvjp.hpp is checked there under the host sanitizers, tools/sim_vjp_check.cpp)
template <class K = NomK>
__host__ __device__ __forceinline__ void f_expl(const double* __restrict__ x, const double* __restrict__ u,
                                       double* __restrict__ dx, const K& mk = K()) {
    const double q1 = x[3], q2 = x[4], q3 = x[5], q4 = x[6];
    const double vbx = x[7], vby = x[8], vbz = x[9];
    const double wx = x[10], wy = x[11], wz = x[12];
    const double w1 = u[0], w2 = u[1], w3 = u[2], w4 = u[3];
    dx[0] = vbx * (2 * q1 * q1 + 2 * q2 * q2 - 1) - vby * (2 * q1 * q4 - 2 * q2 * q3) + vbz * (2 * q1 * q3 + 2 * q2 * q4);
    dx[1] = vby * (2 * q1 * q1 + 2 * q3 * q3 - 1) + vbx * (2 * q1 * q4 + 2 * q2 * q3) - vbz * (2 * q1 * q2 - 2 * q3 * q4);
    dx[2] = vbz * (2 * q1 * q1 + 2 * q4 * q4 - 1) - vbx * (2 * q1 * q3 - 2 * q2 * q4) + vby * (2 * q1 * q2 + 2 * q3 * q4);
    dx[3] = -(q2 * wx) / 2 - (q3 * wy) / 2 - (q4 * wz) / 2;
    dx[4] = (q1 * wx) / 2 - (q4 * wy) / 2 + (q3 * wz) / 2;
    dx[5] = (q4 * wx) / 2 + (q1 * wy) / 2 - (q2 * wz) / 2;
    dx[6] = (q2 * wy) / 2 - (q3 * wx) / 2 + (q1 * wz) / 2;
    dx[7] = vby * wz - vbz * wy + mk.g0() * (2 * q1 * q3 - 2 * q2 * q4);
    dx[8] = vbz * wx - vbx * wz - mk.g0() * (2 * q1 * q2 + 2 * q3 * q4);
    // (rotor terms and gyroscopic couplings with the constants folded at compile time -- KT = Ct / mq, KA = -Ct l / Ixx, ...,
    //  KWX = -(Izz - Iyy) / Ixx, ...: the same products jvp() differentiates; a division by mq / Ixx / Iyy / Izz per
    //  evaluation cost k_linearise 16 FP64 divisions per shooting interval)
    const double s1 = w1 * w1, s2 = w2 * w2, s3 = w3 * w3, s4 = w4 * w4;
    dx[9] = vbx * wy - vby * wx - mk.g0() * (2 * q1 * q1 + 2 * q4 * q4 - 1) + mk.kt() * (s1 + s2 + s3 + s4);
    dx[10] = mk.ka() * (s1 + s2 - s3 - s4) + mk.kwx() * (wy * wz);
    dx[11] = mk.kb() * (s1 - s2 - s3 + s4) + mk.kwy() * (wx * wz);
    dx[12] = mk.kc() * (s1 - s2 + s3 - s4) + mk.kwz() * (wx * wy);
    if constexpr (has_dist<K>::value) {   // v_b' += R(q)' a_w, w' += al_b
        const double ax = mk.dax(), ay = mk.day(), az = mk.daz();
        dx[7] += (2 * q1 * q1 + 2 * q2 * q2 - 1) * ax + (2 * q1 * q4 + 2 * q2 * q3) * ay - (2 * q1 * q3 - 2 * q2 * q4) * az;
        dx[8] += -(2 * q1 * q4 - 2 * q2 * q3) * ax + (2 * q1 * q1 + 2 * q3 * q3 - 1) * ay + (2 * q1 * q2 + 2 * q3 * q4) * az;
        dx[9] += (2 * q1 * q3 + 2 * q2 * q4) * ax - (2 * q1 * q2 - 2 * q3 * q4) * ay + (2 * q1 * q1 + 2 * q4 * q4 - 1) * az;
        dx[10] += mk.dlx(); dx[11] += mk.dly(); dx[12] += mk.dlz();
    }
}

// Point data of df/dx at one RK stage point that is shared by all sensitivity columns:
// rotation matrix R(q) (= dp'/dv) and dp'/dq; everything else is linear in (q,v,w).
struct JacPoint {
    double q[4], v[3], w[3];
    double R[9];
    double Jpq[12];
};

__host__ __device__ __forceinline__ void jac_point(const double* __restrict__ x, JacPoint& J) {
    const double q1 = x[3], q2 = x[4], q3 = x[5], q4 = x[6];
    const double vx = x[7], vy = x[8], vz = x[9];
    J.q[0] = q1; J.q[1] = q2; J.q[2] = q3; J.q[3] = q4;
    J.v[0] = vx; J.v[1] = vy; J.v[2] = vz;
    J.w[0] = x[10]; J.w[1] = x[11]; J.w[2] = x[12];
    J.R[0] = 2 * q1 * q1 + 2 * q2 * q2 - 1; J.R[1] = -(2 * q1 * q4 - 2 * q2 * q3); J.R[2] = 2 * q1 * q3 + 2 * q2 * q4;
    J.R[3] = 2 * q1 * q4 + 2 * q2 * q3; J.R[4] = 2 * q1 * q1 + 2 * q3 * q3 - 1; J.R[5] = -(2 * q1 * q2 - 2 * q3 * q4);
    J.R[6] = -(2 * q1 * q3 - 2 * q2 * q4); J.R[7] = 2 * q1 * q2 + 2 * q3 * q4; J.R[8] = 2 * q1 * q1 + 2 * q4 * q4 - 1;
    J.Jpq[0] = 4 * q1 * vx - 2 * q4 * vy + 2 * q3 * vz; J.Jpq[1] = 4 * q2 * vx + 2 * q3 * vy + 2 * q4 * vz;
    J.Jpq[2] = 2 * q2 * vy + 2 * q1 * vz;               J.Jpq[3] = -2 * q1 * vy + 2 * q2 * vz;
    J.Jpq[4] = 4 * q1 * vy + 2 * q4 * vx - 2 * q2 * vz; J.Jpq[5] = 2 * q3 * vx - 2 * q1 * vz;
    J.Jpq[6] = 4 * q3 * vy + 2 * q2 * vx + 2 * q4 * vz; J.Jpq[7] = 2 * q1 * vx + 2 * q3 * vz;
    J.Jpq[8] = 4 * q1 * vz - 2 * q3 * vx + 2 * q2 * vy; J.Jpq[9] = 2 * q4 * vx + 2 * q1 * vy;
    J.Jpq[10] = -2 * q1 * vx + 2 * q4 * vy;             J.Jpq[11] = 4 * q4 * vz + 2 * q2 * vx + 2 * q3 * vy;
}

// out = (df/dx)(point) * s  for a direction s whose q-part / w-part may be structurally zero.
// s, out: 13 entries (s[0..2] is never read: nothing depends on position).
template <bool HQ, bool HW, class K = NomK>
__device__ __forceinline__ void jvp(const JacPoint& J, const double* __restrict__ s, double* __restrict__ o, const K& mk = K()) {
    const double q1 = J.q[0], q2 = J.q[1], q3 = J.q[2], q4 = J.q[3];
    const double vx = J.v[0], vy = J.v[1], vz = J.v[2];
    const double wx = J.w[0], wy = J.w[1], wz = J.w[2];
    const double sv0 = s[7], sv1 = s[8], sv2 = s[9];
    double o0 = J.R[0] * sv0 + J.R[1] * sv1 + J.R[2] * sv2;
    double o1 = J.R[3] * sv0 + J.R[4] * sv1 + J.R[5] * sv2;
    double o2 = J.R[6] * sv0 + J.R[7] * sv1 + J.R[8] * sv2;
    double o3 = 0, o4 = 0, o5 = 0, o6 = 0;
    double o7 = wz * sv1 - wy * sv2;
    double o8 = -wz * sv0 + wx * sv2;
    double o9 = wy * sv0 - wx * sv1;
    double o10 = 0, o11 = 0, o12 = 0;
    if (HQ) {
        const double a = s[3], b = s[4], c = s[5], d = s[6];
        o0 += J.Jpq[0] * a + J.Jpq[1] * b + J.Jpq[2] * c + J.Jpq[3] * d;
        o1 += J.Jpq[4] * a + J.Jpq[5] * b + J.Jpq[6] * c + J.Jpq[7] * d;
        o2 += J.Jpq[8] * a + J.Jpq[9] * b + J.Jpq[10] * c + J.Jpq[11] * d;
        o3 += 0.5 * (-wx * b - wy * c - wz * d);
        o4 += 0.5 * (wx * a + wz * c - wy * d);
        o5 += 0.5 * (wy * a - wz * b + wx * d);
        o6 += 0.5 * (wz * a + wy * b - wx * c);
        o7 += 2 * mk.g0() * (q3 * a - q4 * b + q1 * c - q2 * d);
        o8 += -2 * mk.g0() * (q2 * a + q1 * b + q4 * c + q3 * d);
        o9 += -4 * mk.g0() * (q1 * a + q4 * d);
        if constexpr (has_dist<K>::value) {   // d (R(q)' a_w) along the q-part: the rows of dR = (dR / dq) (a, b, c, d), transposed
            const double ax = mk.dax(), ay = mk.day(), az = mk.daz();
            const double d14 = q1 * d + q4 * a, d23 = q2 * c + q3 * b, d13 = q1 * c + q3 * a;
            const double d24 = q2 * d + q4 * b, d12 = q1 * b + q2 * a, d34 = q3 * d + q4 * c;
            o7 += 4 * (q1 * a + q2 * b) * ax + 2 * (d14 + d23) * ay + 2 * (d24 - d13) * az;
            o8 += 2 * (d23 - d14) * ax + 4 * (q1 * a + q3 * c) * ay + 2 * (d12 + d34) * az;
            o9 += 2 * (d13 + d24) * ax + 2 * (d34 - d12) * ay + 4 * (q1 * a + q4 * d) * az;
        }
    }
    if (HW) {
        const double a = s[10], b = s[11], c = s[12];
        o3 += 0.5 * (-q2 * a - q3 * b - q4 * c);
        o4 += 0.5 * (q1 * a - q4 * b + q3 * c);
        o5 += 0.5 * (q4 * a + q1 * b - q2 * c);
        o6 += 0.5 * (-q3 * a + q2 * b + q1 * c);
        o7 += -vz * b + vy * c;
        o8 += vz * a - vx * c;
        o9 += -vy * a + vx * b;
        o10 = mk.kwx() * (wz * b + wy * c);
        o11 = mk.kwy() * (wz * a + wx * c);
        o12 = mk.kwz() * (wy * a + wx * b);
    }
    o[0] = o0; o[1] = o1; o[2] = o2; o[3] = o3; o[4] = o4; o[5] = o5; o[6] = o6;
    o[7] = o7; o[8] = o8; o[9] = o9; o[10] = o10; o[11] = o11; o[12] = o12;
}

// out = (df/dx)(point)' v: the transposed product of jvp<true, true> at the same Jacobian point (reverse mode, k_nlp_eval).
// v, out: 13 entries; out[0..2] = 0 (nothing depends on position).
template <class K = NomK>
__host__ __device__ __forceinline__ void jtvp(const JacPoint& J, const double* __restrict__ v, double* __restrict__ o, const K& mk = K()) {
    const double q1 = J.q[0], q2 = J.q[1], q3 = J.q[2], q4 = J.q[3];
    const double vx = J.v[0], vy = J.v[1], vz = J.v[2];
    const double wx = J.w[0], wy = J.w[1], wz = J.w[2];
    const double p0 = v[0], p1 = v[1], p2 = v[2], a = v[3], b = v[4], c = v[5], d = v[6];
    const double g7 = 2 * mk.g0() * v[7], g8 = 2 * mk.g0() * v[8], g9 = 4 * mk.g0() * v[9];
    o[0] = 0; o[1] = 0; o[2] = 0;
    o[3] = J.Jpq[0] * p0 + J.Jpq[4] * p1 + J.Jpq[8] * p2 + 0.5 * (wx * b + wy * c + wz * d) + q3 * g7 - q2 * g8 - q1 * g9;
    o[4] = J.Jpq[1] * p0 + J.Jpq[5] * p1 + J.Jpq[9] * p2 + 0.5 * (-wx * a - wz * c + wy * d) - q4 * g7 - q1 * g8;
    o[5] = J.Jpq[2] * p0 + J.Jpq[6] * p1 + J.Jpq[10] * p2 + 0.5 * (-wy * a + wz * b - wx * d) + q1 * g7 - q4 * g8;
    o[6] = J.Jpq[3] * p0 + J.Jpq[7] * p1 + J.Jpq[11] * p2 + 0.5 * (-wz * a - wy * b + wx * c) - q2 * g7 - q3 * g8 - q4 * g9;
    o[7] = J.R[0] * p0 + J.R[3] * p1 + J.R[6] * p2 - wz * v[8] + wy * v[9];
    o[8] = J.R[1] * p0 + J.R[4] * p1 + J.R[7] * p2 + wz * v[7] - wx * v[9];
    o[9] = J.R[2] * p0 + J.R[5] * p1 + J.R[8] * p2 - wy * v[7] + wx * v[8];
    o[10] = 0.5 * (-q2 * a + q1 * b + q4 * c - q3 * d) + vz * v[8] - vy * v[9] + mk.kwy() * (wz * v[11]) + mk.kwz() * (wy * v[12]);
    o[11] = 0.5 * (-q3 * a - q4 * b + q1 * c + q2 * d) - vz * v[7] + vx * v[9] + mk.kwx() * (wz * v[10]) + mk.kwz() * (wx * v[12]);
    o[12] = 0.5 * (-q4 * a + q3 * b - q2 * c + q1 * d) + vy * v[7] - vx * v[8] + mk.kwx() * (wy * v[10]) + mk.kwy() * (wx * v[11]);
    if constexpr (has_dist<K>::value) {   // (d (R(q)' a_w) / dq)' v[7:10] = d (a_w' R(q) l) / dq, l = v[7:10]: Jpq's expressions at l
        const double ax = mk.dax(), ay = mk.day(), az = mk.daz();
        const double lx = v[7], ly = v[8], lz = v[9];
        o[3] += (4 * q1 * lx - 2 * q4 * ly + 2 * q3 * lz) * ax + (4 * q1 * ly + 2 * q4 * lx - 2 * q2 * lz) * ay + (4 * q1 * lz - 2 * q3 * lx + 2 * q2 * ly) * az;
        o[4] += (4 * q2 * lx + 2 * q3 * ly + 2 * q4 * lz) * ax + (2 * q3 * lx - 2 * q1 * lz) * ay + (2 * q4 * lx + 2 * q1 * ly) * az;
        o[5] += (2 * q2 * ly + 2 * q1 * lz) * ax + (4 * q3 * ly + 2 * q2 * lx + 2 * q4 * lz) * ay + (-2 * q1 * lx + 2 * q4 * ly) * az;
        o[6] += (-2 * q1 * ly + 2 * q2 * lz) * ax + (2 * q1 * lx + 2 * q3 * lz) * ay + (4 * q4 * lz + 2 * q2 * lx + 2 * q3 * ly) * az;
    }
}

// df/du column c (rows 9..12 only): d v'_z, d w'_x, d w'_y, d w'_z
__device__ __forceinline__ void ju_col(int c, const double* __restrict__ u, double* __restrict__ o4) {
    const double uc = 2.0 * u[c];
    const double sa = (c < 2) ? 1.0 : -1.0;             // w1 w2 | -w3 -w4
    const double sb = (c == 0 || c == 3) ? 1.0 : -1.0;  // w1 -w2 -w3 w4
    const double sc = (c == 0 || c == 2) ? 1.0 : -1.0;  // w1 -w2 w3 -w4
    o4[0] = KT * uc;
    o4[1] = KA * sa * uc;
    o4[2] = KB * sb * uc;
    o4[3] = KC * sc * uc;
}

// f(x, u) and (df/dx)(x) s + (df/du) du at one RK point, evaluated TOGETHER (export_ode_model.py:85-97 and its
// directional derivative, restated with shared sub-expressions: in this mapping a lane integrates one column only, so
// a Jacobian point kept for several columns -- cfnmpc_model.hpp: jac_point / jvp -- would be built for a single use).
//   xq[10] = q | v | w of the point, sq[10] = the direction's q | v | w parts (nothing depends on position);
//   rot[4] = the rotor terms of v_z', w' (functions of u only: constant over the interval), ju[4] = (df/du) du rows 9..12;
//   kk[13], dk[13]: slopes in EXTERNAL order.  With r = R(q) / 2:  p' = R v,  dp' = R dv + dR v.
template <class K = NomK>
__device__ __forceinline__ void lf_point(const double (&xq)[10], const double (&sq)[10], const double (&rot)[4],
                                         const double (&ju)[4], double (&kk)[13], double (&dk)[13], const K& mk = K()) {
    const double q1 = xq[0], q2 = xq[1], q3 = xq[2], q4 = xq[3], vx = xq[4], vy = xq[5], vz = xq[6];
    const double wx = xq[7], wy = xq[8], wz = xq[9];
    const double a = sq[0], b = sq[1], c = sq[2], d = sq[3], sx = sq[4], sy = sq[5], sz = sq[6];
    const double ox = sq[7], oy = sq[8], oz = sq[9];
    // r = R / 2
    const double t11 = q1 * q1 - 0.5;
    const double r0 = q2 * q2 + t11, r4 = q3 * q3 + t11, r8 = q4 * q4 + t11;
    const double p14 = q1 * q4, p13 = q1 * q3, p12 = q1 * q2;
    const double r1 = q2 * q3 - p14, r3 = q2 * q3 + p14;
    const double r2 = q2 * q4 + p13, r6 = q2 * q4 - p13;
    const double r5 = q3 * q4 - p12, r7 = q3 * q4 + p12;
    // dr = dR / 2 (the diagonal entries halved once more: they meet 2 v below)
    const double e1 = q1 * a;
    const double h0 = q2 * b + e1, h4 = q3 * c + e1, h8 = q4 * d + e1;
    const double d23 = q2 * c + q3 * b, d14 = q1 * d + q4 * a;
    const double d24 = q2 * d + q4 * b, d13 = q1 * c + q3 * a;
    const double d34 = q3 * d + q4 * c, d12 = q1 * b + q2 * a;
    const double dr1 = d23 - d14, dr3 = d23 + d14;
    const double dr2 = d24 + d13, dr6 = d24 - d13;
    const double dr5 = d34 - d12, dr7 = d34 + d12;
    const double v2x = 2.0 * vx, v2y = 2.0 * vy, v2z = 2.0 * vz;
    // position rows
    kk[0] = r0 * v2x + r1 * v2y + r2 * v2z;
    kk[1] = r3 * v2x + r4 * v2y + r5 * v2z;
    kk[2] = r6 * v2x + r7 * v2y + r8 * v2z;
    dk[0] = 2.0 * (r0 * sx + r1 * sy + r2 * sz + h0 * v2x + dr1 * vy + dr2 * vz);
    dk[1] = 2.0 * (r3 * sx + r4 * sy + r5 * sz + dr3 * vx + h4 * v2y + dr5 * vz);
    dk[2] = 2.0 * (r6 * sx + r7 * sy + r8 * sz + dr6 * vx + dr7 * vy + h8 * v2z);
    // quaternion rows (halved rates)
    const double hx = 0.5 * wx, hy = 0.5 * wy, hz = 0.5 * wz;
    const double gx = 0.5 * ox, gy = 0.5 * oy, gz = 0.5 * oz;
    kk[3] = -(q2 * hx + q3 * hy + q4 * hz);
    kk[4] = q1 * hx - q4 * hy + q3 * hz;
    kk[5] = q4 * hx + q1 * hy - q2 * hz;
    kk[6] = q2 * hy - q3 * hx + q1 * hz;
    dk[3] = -(b * hx + c * hy + d * hz + q2 * gx + q3 * gy + q4 * gz);
    dk[4] = a * hx - d * hy + c * hz + q1 * gx - q4 * gy + q3 * gz;
    dk[5] = d * hx + a * hy - b * hz + q4 * gx + q1 * gy - q2 * gz;
    dk[6] = b * hy - c * hx + a * hz + q2 * gy - q3 * gx + q1 * gz;
    // body velocity rows: v' = v x w - g0 R' e_z (+ thrust);  -G0 R[6..8] = -2 G0 r[6..8]
    kk[7] = vy * wz - vz * wy - (2.0 * mk.g0()) * r6;
    kk[8] = vz * wx - vx * wz - (2.0 * mk.g0()) * r7;
    kk[9] = vx * wy - vy * wx - (2.0 * mk.g0()) * r8 + rot[0];
    dk[7] = sy * wz + vy * oz - sz * wy - vz * oy - (2.0 * mk.g0()) * dr6;
    dk[8] = sz * wx + vz * ox - sx * wz - vx * oz - (2.0 * mk.g0()) * dr7;
    dk[9] = sx * wy + vx * oy - sy * wx - vy * ox - (4.0 * mk.g0()) * h8 + ju[0];
    // body rate rows
    kk[10] = mk.kwx() * (wy * wz) + rot[1];
    kk[11] = mk.kwy() * (wx * wz) + rot[2];
    kk[12] = mk.kwz() * (wx * wy) + rot[3];
    dk[10] = mk.kwx() * (oy * wz + wy * oz) + ju[1];
    dk[11] = mk.kwy() * (ox * wz + wx * oz) + ju[2];
    dk[12] = mk.kwz() * (ox * wy + wx * oy) + ju[3];
    if constexpr (has_dist<K>::value) {   // v_b' += R' a_w = 2 r' a_w and its derivative 2 dr' a_w (diagonal: dR / 2 = 2 h), w' += al_b
        const double ax = mk.dax(), ay = mk.day(), az = mk.daz();
        kk[7] += 2.0 * (r0 * ax + r3 * ay + r6 * az);
        kk[8] += 2.0 * (r1 * ax + r4 * ay + r7 * az);
        kk[9] += 2.0 * (r2 * ax + r5 * ay + r8 * az);
        dk[7] += 2.0 * (2.0 * h0 * ax + dr3 * ay + dr6 * az);
        dk[8] += 2.0 * (dr1 * ax + 2.0 * h4 * ay + dr7 * az);
        dk[9] += 2.0 * (dr2 * ax + dr5 * ay + 2.0 * h8 * az);
        kk[10] += mk.dlx(); kk[11] += mk.dly(); kk[12] += mk.dlz();
    }
}

}  // namespace cfn
