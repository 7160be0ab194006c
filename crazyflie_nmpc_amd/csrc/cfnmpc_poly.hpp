// cfnmpc_poly.hpp -- device-side polynomial trajectory references, one per vehicle (cfnmpc_set_poly_library /
// cfnmpc_set_poly_assignment / cfnmpc_set_yref_poly / cfnmpc_eval_poly).  Included at the end of
// cfnmpc_kernels.hip (its primitives, no device unit of its own).
//
// A library of piecewise 7th-order polynomial trajectories (the CSV format of crazyflie_demo/scripts/: one piece = duration and
// four ascending coefficient lists x, y, z, yaw), a trajectory id and a placement row per vehicle, and ONE kernel that writes every
// vehicle's reference window: the polynomial and its first three derivatives at each stage time, mapped through the flatness
// relations of this model to the 17-column row (the rules are in include/cfnmpc.h; crazyflie_nmpc_amd/trajectories.py:
// poly_rows is the numpy twin, operation for operation).
//   k_poly_rows    lane = instance, one wavefront = 64 consecutive instances = 16 workspace blocks, blockIdx.y = a chunk of the
//                  stages.  Per stage every lane evaluates its own row in registers (the piece lookup is a gather from the
//                  library in global memory: a few KB, resident in the L1 / L2), the 64 rows pass through one LDS tile, and the
//                  wave stores the tile element-wise: for a fixed stage the 16 blocks' rows are 16 runs of 68 contiguous
//                  doubles (Params.yref) or one run of 832 (yref_e) -- the read pattern of k_nlp_eval's el17, as stores.  A
//                  vehicle without a trajectory (id outside [0, n_traj)) owns no element of the tile: its rows keep their bits.
//   k_poly_eval    the same body with the public-order rows, and the evaluator's own quantities, into the caller's arrays
//                  [nb][ns][17] / [nb][ns][13]; NaN for a vehicle without a trajectory.
//   k_poly_clamp_ids  ids outside [0, n_traj) -> -1 (a smaller library).
// Every operation is rounded on its own (no contraction): the local time and the piece are then the twin's bit for bit, and
// Horner's rule is the reference evaluator's.  Nothing here writes a field of Params except yref / yref_e.
#pragma once

namespace cfn {

constexpr int POLY_NC = 33, NPLACE = 6, NFLAT = 13;

template <int n>
__device__ __forceinline__ double poly_horner(const double (&c)[n], double s) {
#pragma clang fp contract(off)
    double x = 0.0;
#pragma unroll
    for (int i = 0; i < n; i++) x = x * s + c[n - 1 - i];
    return x;
}

// EVAL = false: rows k = 0 .. N-1 -> P.yref, k = N -> P.yref_e (internal layout); EVAL = true: A.rows / A.flat (public order)
template <bool EVAL>
__device__ __forceinline__ void poly_body(const Params& P, const PolyArgs& A, double* tile, double* ftile, int* own) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const int loc = blockIdx.x * 64 + tid;          // row of this launch
    const int inst = A.b0 + loc;
    const bool valid = loc < A.nb && inst < P.B;
    int id = valid ? A.traj[inst] : -1;
    if (id < 0 || id >= A.n_traj) id = -1;          // (never indexes the library with an unchecked value)
    const bool on = id >= 0;
    own[tid] = EVAL ? (valid ? 1 : 0) : (on ? 1 : 0);
    double t0 = 0.0, ts = 1.0, ox = 0.0, oy = 0.0, oz = 0.0, yaw0 = 0.0;
    if (on && A.place) {
        const double* pl = A.place + (size_t)inst * NPLACE;
        t0 = pl[0]; ts = pl[1]; ox = pl[2]; oy = pl[3]; oz = pl[4]; yaw0 = pl[5];
    }
    if (!(ts > 0.0 && ts <= 1.7976931348623157e308)) ts = 1.0;
    const int p0 = on ? A.first[id] : 0, p1 = on ? A.first[id + 1] : 0;
    double D = 0.0;                                 // the trajectory's duration, piece by piece in table order
    for (int j = p0; j < p1; j++) D = D + A.pieces[(size_t)j * POLY_NC];
    double g0 = G0, kt = KT, hov = sqrt((MQ * G0) / (4 * CT));
    if (on && P.mpar) {
        const size_t S = ((size_t)P.NW + 1) * 4;
        g0 = P.mpar[inst]; kt = P.mpar[S + inst]; hov = P.mpar[(size_t)(NK - 1) * S + inst];
    }
    double s0y, c0y;
    sincos(yaw0, &s0y, &c0y);
    const double ts2 = ts * ts, ts3 = ts2 * ts;
    const double nan = __builtin_nan("");
    const int w0 = blockIdx.x * 16, N = P.N;
    const int k0 = blockIdx.y * A.kchunk, k1 = imin(k0 + A.kchunk, A.ns);
#pragma nounroll
    for (int k = k0; k < k1; k++) {
        // The row is built in three steps with the tile as this lane's parking space, so that few values are live at a time
        // (evaluated in one piece the body holds 104 coefficients and 30 results and spills at four waves per SIMD).
        const bool term = !EVAL && k == N;          // (uniform over the workgroup) the terminal row: 13 columns
        const int rs = term ? 13 : 17;              // this lane's row starts at tile[tid * rs]
        bool held = false;
        __syncthreads();                            // (the previous stage's tile has been stored)
        if (on) {
            // 1. local time, piece and piece time; value and three derivatives of x, y, z, yaw
            const double tq = A.t + (double)k * P.dt;
            double tau = (tq - t0) / ts;
            const bool before = tau < 0.0;
            bool after = tau >= D;
            if (after && (A.flags & 1)) {           // CFNMPC_POLY_LOOP
                tau = tau - D * floor(tau / D);
                if (tau < 0.0) tau = 0.0;
                after = false;
            }
            held = before || after;
            int j = p0;
            double cum = 0.0;
            for (; j < p1 - 1; j++) {               // the first piece with tau < cum + duration (else the last)
                const double d = A.pieces[(size_t)j * POLY_NC];
                if (tau < cum + d) break;
                cum = cum + d;
            }
            double s = tau - cum;
            if (before) { j = p0; s = 0.0; }
            if (after) { j = p1 - 1; s = A.pieces[(size_t)j * POLY_NC]; }
            const double* cf = A.pieces + (size_t)j * POLY_NC + 1;
#pragma nounroll
            for (int a = 0; a < 4; a++) {           // Horner on the coefficient lists (i + 1) c[i + 1], one axis at a time
                double c0[8], c1[7], c2[6], c3[5];
                SFOR(i, 0, 8, { c0[i] = cf[8 * a + i]; });
                SFOR(i, 0, 7, { c1[i] = (double)(i + 1) * c0[i + 1]; });
                SFOR(i, 0, 6, { c2[i] = (double)(i + 1) * c1[i + 1]; });
                SFOR(i, 0, 5, { c3[i] = (double)(i + 1) * c2[i + 1]; });
                tile[(4 * a + 0) * 64 + tid] = poly_horner(c0, s);
                tile[(4 * a + 1) * 64 + tid] = held ? 0.0 : poly_horner(c1, s) / ts;
                tile[(4 * a + 2) * 64 + tid] = held ? 0.0 : poly_horner(c2, s) / ts2;
                tile[(4 * a + 3) * 64 + tid] = held ? 0.0 : poly_horner(c3, s) / ts3;
            }
        }
        __syncthreads();
        double v0[4], v1[4], v2[4], v3[4];
        SFOR(a, 0, 4, {
            v0[a] = tile[(4 * a + 0) * 64 + tid]; v1[a] = tile[(4 * a + 1) * 64 + tid];
            v2[a] = tile[(4 * a + 2) * 64 + tid]; v3[a] = tile[(4 * a + 3) * 64 + tid];
        });
        __syncthreads();                            // (every lane has its sixteen values: the tile is free for the rows)
        double* row = tile + tid * rs;              // public column e of the row at row[rc(e)]
        auto rc = [&](int e) { return (EVAL || e >= 13) ? e : int_of(e); };
        if (on) {
            // 2. placement: Rz(yaw0), the offset, yaw0
            const double px = c0y * v0[0] - s0y * v0[1] + ox, py = s0y * v0[0] + c0y * v0[1] + oy, pz = v0[2] + oz;
            const double vx = c0y * v1[0] - s0y * v1[1], vy = s0y * v1[0] + c0y * v1[1], vz = v1[2];
            const double ax = c0y * v2[0] - s0y * v2[1], ay = s0y * v2[0] + c0y * v2[1], az = v2[2];
            const double jx = c0y * v3[0] - s0y * v3[1], jy = s0y * v3[0] + c0y * v3[1], jz = v3[2];
            const double yaw = v0[3] + yaw0, dyaw = v1[3];
            row[rc(0)] = px; row[rc(1)] = py; row[rc(2)] = pz;
            if constexpr (EVAL) {
                double* fl = ftile + tid * NFLAT;
                fl[0] = px; fl[1] = py; fl[2] = pz; fl[3] = vx; fl[4] = vy; fl[5] = vz; fl[6] = ax; fl[7] = ay; fl[8] = az; fl[9] = yaw;
            }
            double sy, cy;
            sincos(yaw, &sy, &cy);
            // 3. flatness
            const double tx = ax, ty = ay, tz = az + g0;
            const double nthr = sqrt(tx * tx + ty * ty + tz * tz);
            const double zx = tx / nthr, zy = ty / nthr, zz = tz / nthr;
            const double ccx = -zz * sy, ccy = zz * cy, ccz = zx * sy - zy * cy;      // c = z_b x x_w
            const double nc = sqrt(ccx * ccx + ccy * ccy + ccz * ccz);
            const double yx = ccx / nc, yy = ccy / nc, yz = ccz / nc;
            const double xx = yy * zz - yz * zy, xy = yz * zx - yx * zz, xz = yx * zy - yy * zx;   // x_b = y_b x z_b
            // level rows: held stages and the guard
            const bool level = held || !((tz > 0.1 * g0) && (nc >= 1e-3));
            const bool kin = (A.flags & 2) != 0;    // CFNMPC_POLY_KINEMATIC
            const double spd = (level || kin) ? hov : sqrt(nthr / (4 * kt));
            SFOR(e, 13, 17, { if (!term) row[e] = spd; });
            row[rc(7)] = kin ? 0.0 : (level ? cy * vx + sy * vy : xx * vx + xy * vy + xz * vz);
            row[rc(8)] = kin ? 0.0 : (level ? -sy * vx + cy * vy : yx * vx + yy * vy + yz * vz);
            row[rc(9)] = kin ? 0.0 : (level ? vz : zx * vx + zy * vy + zz * vz);
            const double jd = jx * zx + jy * zy + jz * zz;
            const double hx = (jx - jd * zx) / nthr, hy = (jy - jd * zy) / nthr, hz = (jz - jd * zz) / nthr;
            const double wx = -(hx * yx + hy * yy + hz * yz), wy = hx * xx + hy * xy + hz * xz;
            // exact body rate about z: -x_b . (h_w x x_w + z_b x dx_w) / |c|
            const double ex = -hz * sy - dyaw * (zz * cy);
            const double ey = hz * cy - dyaw * (zz * sy);
            const double ez = (hx * sy - hy * cy) + dyaw * (zx * cy + zy * sy);
            const double wz = -(xx * ex + xy * ey + xz * ez) / nc;
            row[rc(10)] = (level || kin) ? 0.0 : wx;
            row[rc(11)] = (level || kin) ? 0.0 : wy;
            row[rc(12)] = kin ? 0.0 : (level ? dyaw : wz);
            if constexpr (EVAL) {
                double* fl = ftile + tid * NFLAT;
                fl[10] = level ? 0.0 : wx; fl[11] = level ? 0.0 : wy; fl[12] = level ? dyaw : zz * dyaw;   // (the evaluator's omega_z)
            }
            // attitude q = qz(yaw) qx(phi) qy(theta)
            const double zlx = cy * zx + sy * zy, zly = -sy * zx + cy * zy;
            const double theta = asin(fmin(fmax(zlx, -1.0), 1.0)), phi = atan2(-zly, zz);
            double shz, chz, shx, chx, sht, cht;
            sincos(0.5 * yaw, &shz, &chz);
            sincos(0.5 * phi, &shx, &chx);
            sincos(0.5 * theta, &sht, &cht);
            const double qa = chx * cht, qb = shx * cht, qc = chx * sht, qd = shx * sht;
            row[rc(3)] = kin ? 1.0 : (level ? chz : chz * qa - shz * qd);
            row[rc(4)] = (level || kin) ? 0.0 : chz * qb - shz * qc;
            row[rc(5)] = (level || kin) ? 0.0 : chz * qc + shz * qb;
            row[rc(6)] = kin ? 0.0 : (level ? shz : chz * qd + shz * qa);
        } else if (EVAL) {                          // a vehicle without a trajectory: NaN
            SFOR(e, 0, 17, { row[e] = nan; });
            SFOR(e, 0, NFLAT, { ftile[tid * NFLAT + e] = nan; });
        }
        __syncthreads();
        // the tile, element-wise: lane l stores the elements l + 64 j.  (The lane index is made opaque per stage: the compiler would
        // otherwise keep the 17 element addresses of a stage -- loop invariants but for k -- in registers across the whole body.)
        int tl = tid;
        asm volatile("" : "+v"(tl));
        if constexpr (!EVAL) {
            if (term) {
                gdouble* dst = gm(P.yref_e) + (size_t)w0 * SZ_V13;
                SFOR(j, 0, 13, {
                    const int e = tl + 64 * j;
                    if (own[e / 13]) dst[e] = tile[e];
                });
            } else {
                char* base = (char*)(gm(P.yref) + ((size_t)w0 * N + k) * SZ_Y);   // (uniform) stage k of this wave's first block
                SFOR(j, 0, 17, {
                    const int e = tl + 64 * j, bk = e / SZ_Y;
                    const unsigned bo = ((unsigned)bk * (unsigned)(N * SZ_Y) + (unsigned)(e - bk * SZ_Y)) * 8u;
                    if (own[e / 17]) *(gdouble*)(base + bo) = tile[e];
                });
            }
        } else {
            const size_t r0 = (size_t)blockIdx.x * 64 * A.ns + k;
            if (A.rows) SFOR(j, 0, 17, {
                const int e = tl + 64 * j, o = e / 17;
                if (own[o]) A.rows[(r0 + (size_t)o * A.ns) * 17 + (e - o * 17)] = tile[e];
            });
            if (A.flat) SFOR(j, 0, NFLAT, {
                const int e = tl + 64 * j, o = e / NFLAT;
                if (own[o]) A.flat[(r0 + (size_t)o * A.ns) * NFLAT + (e - o * NFLAT)] = ftile[e];
            });
        }
    }
}

__global__ __launch_bounds__(64, 2) void k_poly_rows(Params P, PolyArgs A) {
    __shared__ double tile[64 * 17];
    __shared__ int own[64];
    poly_body<false>(P, A, tile, nullptr, own);
}
__global__ __launch_bounds__(64, 2) void k_poly_eval(Params P, PolyArgs A) {
    __shared__ double tile[64 * 17];
    __shared__ double ftile[64 * NFLAT];
    __shared__ int own[64];
    poly_body<true>(P, A, tile, ftile, own);
}
__global__ __launch_bounds__(256) void k_poly_clamp_ids(int B, int n_traj, int* __restrict__ traj) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B && (traj[i] < 0 || traj[i] >= n_traj)) traj[i] = -1;
}

// stages per workgroup: enough workgroups for about eight waves per SIMD on 1024 SIMDs, whatever the fleet size
static int poly_chunk(int nb, int ns) {
    const int groups = (nb + 63) / 64;
    int chunks = (8192 + groups - 1) / groups;
    chunks = chunks < 1 ? 1 : (chunks > ns ? ns : chunks);
    return (ns + chunks - 1) / chunks;
}
void launch_poly_rows(const Params& P, PolyArgs A, hipStream_t st) {
    A.b0 = 0; A.nb = P.B; A.ns = P.N + 1;
    A.kchunk = poly_chunk(A.nb, A.ns);
    hipLaunchKernelGGL(k_poly_rows, dim3((A.nb + 63) / 64, (A.ns + A.kchunk - 1) / A.kchunk), dim3(64), 0, st, P, A);
}
void launch_poly_eval(const Params& P, PolyArgs A, hipStream_t st) {
    A.kchunk = poly_chunk(A.nb, A.ns);
    hipLaunchKernelGGL(k_poly_eval, dim3((A.nb + 63) / 64, (A.ns + A.kchunk - 1) / A.kchunk), dim3(64), 0, st, P, A);
}
void launch_poly_clamp_ids(int B, int n_traj, int* traj, hipStream_t st) {
    hipLaunchKernelGGL(k_poly_clamp_ids, dim3((B + 255) / 256), dim3(256), 0, st, B, n_traj, traj);
}

}  // namespace cfn
