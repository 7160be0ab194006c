// cfnmpc_host.hpp -- what the host units (cfnmpc_api.cpp, cfnmpc_fleet.cpp, cfnmpc_multi.cpp) share: the error macros, the
// device guard, the reading of `on_device` and of the caller's options, and (cfnmpc_rows.hpp, free of HIP) the description of
// a per-vehicle array with the row movers of the fleet and multi-GPU layers.  Internal to the library; DESIGN.md section 5.19.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/cfnmpc.h"
#include "cfnmpc_rows.hpp"

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            std::fprintf(stderr, "cfnmpc: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_),   \
                         __FILE__, __LINE__);                                                       \
            return CFNMPC_EHIP;                                                                     \
        }                                                                                           \
    } while (0)
#define RC_TRY(x) do { int rc_ = (x); if (rc_ != CFNMPC_OK) return rc_; } while (0)

struct cfnmpc_solver;
struct cfnmpc_fleet;
namespace cfn {
// a stored backoff is there (cfnmpc_get_backoff / cfnmpc_tighten_box would accept): asked by the layers above BEFORE they touch
// the caller's arrays
bool unc_backoff_valid(const cfnmpc_solver* s);
bool fleet_backoff_valid(const cfnmpc_fleet* f);

// A solver, fleet or shard lives on the device that was current when it was created; every entry point that touches it makes
// that device current for the duration of the call (a caller that drives several GPUs from one thread may have another one
// selected).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) == hipSuccess && prev != device) switched = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// `on_device` argument: 0 host (synchronous), 2 host (enqueued only), anything else: device pointer
inline bool is_host(int on_device) { return on_device == CFNMPC_ON_HOST || on_device == CFNMPC_ON_HOST_ASYNC; }

// host arrays of cfnmpc_set_uncertainty, n matrices [13][13]: finite, symmetric to 1e-12 of the matrix' largest entry,
// non-negative diagonal (DIM = 16: the augmented covariance of cfnmpc_ekf_aug_step, by the same rule)
template <int DIM = 13>
inline bool unc_sym_ok(const double* S, size_t n) {
    for (size_t i = 0; i < n; i++) {
        const double* m = S + i * DIM * DIM;
        double big = 0.0;
        for (int e = 0; e < DIM * DIM; e++) {
            if (!(m[e] - m[e] == 0.0)) return false;   // (NaN, +-inf)
            const double a = m[e] < 0.0 ? -m[e] : m[e];
            if (a > big) big = a;
        }
        for (int r = 0; r < DIM; r++) {
            if (m[r * (DIM + 1)] < 0.0) return false;
            for (int c = r + 1; c < DIM; c++) {
                const double d = m[r * DIM + c] - m[c * DIM + r];
                if ((d < 0.0 ? -d : d) > 1e-12 * big) return false;
            }
        }
    }
    return true;
}
// cfnmpc_ekf_aug_step: sel [3] holds -1 (slot unused) or distinct entries of 0 .. 5
inline bool ekf_sel_ok(const int* sel) {
    for (int k = 0; k < 3; k++) {
        if (sel[k] < -1 || sel[k] >= CFNMPC_ND) return false;
        for (int l = 0; l < k; l++) if (sel[k] >= 0 && sel[k] == sel[l]) return false;
    }
    return true;
}
// ... and the rows and columns of its unused slots in n matrices Pa [16][16] are zero
inline bool ekf_unused_zero(const double* Pa, size_t n, const int* sel) {
    for (int k = 0; k < 3; k++) {
        if (sel[k] >= 0) continue;
        for (size_t i = 0; i < n; i++)
            for (int e = 0; e < 16; e++)
                if (Pa[i * 256 + (13 + k) * 16 + e] != 0.0 || Pa[i * 256 + e * 16 + 13 + k] != 0.0) return false;
    }
    return true;
}

// host arrays of cfnmpc_set_poly_library: every number finite, every duration > 0, first[0] = 0 and strictly increasing, within
// the limits of include/cfnmpc.h
inline bool poly_library_ok(const double* pieces, const int* first, int n_traj) {
    if (n_traj < 1 || n_traj > CFNMPC_POLY_MAX_TRAJ || first[0] != 0) return false;
    for (int j = 0; j < n_traj; j++) if (first[j + 1] <= first[j] || first[j + 1] > CFNMPC_POLY_MAX_PIECES) return false;
    const size_t n = (size_t)first[n_traj] * CFNMPC_POLY_NC;
    for (size_t i = 0; i < n; i++) {
        if (!(pieces[i] - pieces[i] == 0.0)) return false;   // (NaN, +-inf)
        if (i % CFNMPC_POLY_NC == 0 && !(pieces[i] > 0.0)) return false;
    }
    return true;
}
// host arrays of cfnmpc_set_poly_assignment for n vehicles: id in [-1, n_traj), time_scale finite and > 0, the rest finite
inline bool poly_assignment_ok(const int* traj, const double* place, size_t n, int n_traj) {
    for (size_t i = 0; i < n; i++) if (traj[i] < -1 || traj[i] >= n_traj) return false;
    if (place)
        for (size_t i = 0; i < n * CFNMPC_NPLACE; i++) {
            if (!(place[i] - place[i] == 0.0)) return false;
            if (i % CFNMPC_NPLACE == 1 && !(place[i] > 0.0)) return false;
        }
    return true;
}
// trajectories in the solver's library (0: none); a fleet's buckets all hold the same one
int poly_n_traj(const cfnmpc_solver* s);
int fleet_poly_n_traj(const cfnmpc_fleet* f);

// the options of a creator: the caller's (ABI guard: the first field is the size the caller's filler saw -- read BEFORE the
// struct is copied) or the defaults
inline int take_opts(const cfnmpc_opts* opts, cfnmpc_opts* o) {
    if (opts && opts->struct_size != (int)sizeof(cfnmpc_opts)) {
        std::fprintf(stderr, "cfnmpc: cfnmpc_opts of %d bytes handed to a library built for %d (ABI %d): rebuild against include/cfnmpc.h\n",
                     opts->struct_size, (int)sizeof(cfnmpc_opts), CFNMPC_ABI_VERSION);
        return CFNMPC_EINVAL;
    }
    if (opts) *o = *opts; else cfnmpc_default_opts(o);
    return CFNMPC_OK;
}

}  // namespace cfn
