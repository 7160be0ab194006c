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

namespace cfn {

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
