// cfnmpc_stage.hpp -- the arrays of one solver-less batched call (cfnmpc_sim*, cfnmpc_sim_rollout*, cfnmpc_ekf*_step,
// cfnmpc_estimate_disturbance): each array described once (Arr), and from that one list its place in a staging area and the
// area's size (Stage) -- the sum and the carving are one loop -- and the six calls' lists.  Plain C++, no HIP (tools/host_stage_check.cpp runs it under the
// host sanitizers); the driver that copies and launches is staged_call in cfnmpc_api.cpp.  Internal to the library; DESIGN.md
// section 5.19.1.
#pragma once
#include <cassert>
#include <cstddef>
#include <initializer_list>

#include "../../include/cfnmpc.h"

namespace cfn {

enum ArrDir { ARR_IN = 1, ARR_OUT = 2, ARR_INOUT = ARR_IN | ARR_OUT };

// One array of a call: n elements of esz bytes at the caller's p.  p = nullptr: an optional array that was not given -- it takes
// no room and the kernel gets nullptr -- unless `always`: an output the kernel writes in every call (nis, counts), which is
// staged whatever the caller passed and copied back only to a caller who asked.
struct Arr {
    void* p;
    size_t esz, n;
    int dir;
    bool always;
};
inline Arr arr_in(const double* p, size_t n) { return {const_cast<double*>(p), sizeof(double), n, ARR_IN, false}; }
inline Arr arr_out(double* p, size_t n) { return {p, sizeof(double), n, ARR_OUT, false}; }
inline Arr arr_inout(double* p, size_t n) { return {p, sizeof(double), n, ARR_INOUT, false}; }
inline Arr arr_out_always(double* p, size_t n) { return {p, sizeof(double), n, ARR_OUT, true}; }
inline Arr arr_out_always(int* p, size_t n) { return {p, sizeof(int), n, ARR_OUT, true}; }

constexpr int MAX_ARRS = 16;   // the widest call, cfnmpc_ekf_aug_step, has 15

// the arrays of one call as the launch takes them, in the order of the call's list
struct ArrPtrs {
    void* p[MAX_ARRS];
    double* d(int i) const { return static_cast<double*>(p[i]); }
    int* i(int k) const { return static_cast<int*>(p[k]); }
};

// The staging area of one call: the staged arrays one after another, each starting on a multiple of 8 bytes (as cfn::Layout).
struct Stage {
    int n = 0;
    Arr a[MAX_ARRS];
    size_t off[MAX_ARRS];
    size_t bytes = 0;

    Stage(std::initializer_list<Arr> arrs) {
        assert(arrs.size() <= (size_t)MAX_ARRS);
        for (const Arr& k : arrs) {
            a[n] = k;
            off[n] = bytes;
            if (staged(n)) bytes += (k.n * k.esz + 7) / 8 * 8;
            n++;
        }
    }
    bool staged(int i) const { return a[i].p || a[i].always; }
    size_t size(int i) const { return a[i].n * a[i].esz; }
    bool copy_in(int i) const { return a[i].p && (a[i].dir & ARR_IN); }
    bool copy_out(int i) const { return a[i].p && (a[i].dir & ARR_OUT); }
    // the arrays in the staging area at `base` (nullptr for one not staged), or the caller's own
    ArrPtrs at(void* base) const {
        ArrPtrs q{};
        for (int i = 0; i < n; i++) q.p[i] = staged(i) ? static_cast<char*>(base) + off[i] : nullptr;
        return q;
    }
    ArrPtrs own() const {
        ArrPtrs q{};
        for (int i = 0; i < n; i++) q.p[i] = a[i].p;
        return q;
    }
};

// The tables of the six calls, for a batch of B (rollouts: L steps); each enum names the arrays' places in its table.  Optional
// arrays are nullptr when not given.
struct SimArrs {
    enum { X, U, XN, P, D };
    static Stage of(size_t B, const double* x, const double* u, double* xn, const double* p, const double* d) {
        return {arr_in(x, B * 13), arr_in(u, B * 4), arr_out(xn, B * 13), arr_in(p, B * CFNMPC_NP), arr_in(d, B * CFNMPC_ND)};
    }
};
struct RolloutArrs {
    enum { X0, U, XS, P, D };
    static Stage of(size_t B, size_t L, const double* x0, const double* u, double* xs, const double* p, const double* d) {
        return {arr_in(x0, B * 13), arr_in(u, B * L * 4), arr_out(xs, B * (L + 1) * 13), arr_in(p, B * CFNMPC_NP), arr_in(d, B * CFNMPC_ND)};
    }
};
struct RolloutVjpArrs {
    enum { XS, GXS, U, P, D, GX0, GU, GP, GD };
    static Stage of(size_t B, size_t L, const double* xs, const double* gxs, const double* u, const double* p, const double* d,
                    double* gx0, double* gu, double* gp, double* gd) {
        const size_t ns = B * (L + 1) * 13, nu = B * L * 4, np = B * CFNMPC_NP, nd = B * CFNMPC_ND;
        return {arr_in(xs, ns), arr_in(gxs, ns), arr_in(u, nu), arr_in(p, np), arr_in(d, nd),
                arr_out(gx0, B * 13), arr_out(gu, nu), arr_out(gp, np), arr_out(gd, nd)};
    }
};
// (r is read with z only)
struct EkfArrs {
    enum { X, P, U, PAR, D, Q, Z, R, XN, PN, NIS, COUNTS };
    static Stage of(size_t B, const double* x, const double* P_, const double* u, const double* p, const double* d, const double* Q_,
                    const double* z, const double* r, double* xn, double* Pn, double* nis, int* counts) {
        const size_t nx = B * 13, nP = B * 169;
        return {arr_in(x, nx), arr_in(P_, nP), arr_in(u, B * 4), arr_in(p, B * CFNMPC_NP), arr_in(d, B * CFNMPC_ND), arr_in(Q_, nP),
                arr_in(z, nx), arr_in(z ? r : nullptr, nx), arr_out(xn, nx), arr_out(Pn, nP), arr_out_always(nis, B),
                arr_out_always(counts, 2 * B)};
    }
};
struct EkfAugArrs {
    enum { X, D, PA, U, PAR, Q, QD, Z, R, XN, DN, PAN, PXX, NIS, COUNTS };
    static Stage of(size_t B, const double* x, const double* d, const double* Pa, const double* u, const double* p, const double* Q_,
                    const double* Qd, const double* z, const double* r, double* xn, double* dn, double* Pan, double* Pxx, double* nis,
                    int* counts) {
        const size_t nx = B * 13, nP = B * 169, nA = B * CFNMPC_EKF_NA * CFNMPC_EKF_NA, nd = B * CFNMPC_ND;
        return {arr_in(x, nx), arr_in(d, nd), arr_in(Pa, nA), arr_in(u, B * 4), arr_in(p, B * CFNMPC_NP), arr_in(Q_, nP),
                arr_in(Qd, B * 3), arr_in(z, nx), arr_in(z ? r : nullptr, nx), arr_out(xn, nx), arr_out(dn, nd), arr_out(Pan, nA),
                arr_out(Pxx, nP), arr_out_always(nis, B), arr_out_always(counts, 2 * B)};
    }
};
struct DistObserveArrs {
    enum { XP, U, XM, D, P };
    static Stage of(size_t B, const double* x_prev, const double* u_prev, const double* x_meas, double* d, const double* p) {
        return {arr_in(x_prev, B * 13), arr_in(u_prev, B * 4), arr_in(x_meas, B * 13), arr_inout(d, B * CFNMPC_ND), arr_in(p, B * CFNMPC_NP)};
    }
};

}  // namespace cfn
