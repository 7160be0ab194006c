// Mixed-horizon fleets behind the C-ABI (include/cfnmpc.h, cfnmpc_fleet_*).
//
// The reference fixes its horizon when the solver is generated (generate_c_code.py:41-42) and
// owns one vehicle per process; BASELINE.json's config C5 runs N in {30, 50, 100} side by side.
// A cfnmpc_solver's workspace is blocked by stage for ONE horizon, so a fleet buckets its
// vehicles by N: one solver per distinct horizon, addressed through index lists.  Fleet-level
// arrays keep the caller's vehicle order; rows move between that order and the buckets in ONE
// place, fleet_io below: an entry point names its arrays as columns
// (cfnmpc_rows.hpp: Col) and the bucket call they go to or come from.
// Buckets are solved concurrently, each on its own stream forked from the caller's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

#include "../../include/cfnmpc.h"
#include "cfnmpc_host.hpp"
#include "cfnmpc_model.hpp"
#include "cfnmpc_sqp.h"

namespace {

using cfn::col;
using cfn::col_stages;
using cfn::Cols;
using cfn::Layout;
using cfn::Staged;

// dst bucket row r  <-  src fleet row idx[r]   (GATHER)
// dst fleet row idx[r]  <-  src bucket row r   (!GATHER)
// `len` elements of a row are moved; fleet rows are `fstride` elements apart, bucket rows `len`.
template <typename T, bool GATHER>
__global__ void k_rows(const T* __restrict__ src, T* __restrict__ dst, const int* __restrict__ idx, int count, int len,
                       long fstride) {
    const int r = blockIdx.y;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= count || e >= len) return;
    const long f = (long)idx[r] * fstride + e, b = (long)r * len + e;
    if (GATHER) dst[b] = src[f];
    else dst[f] = src[b];
}

template <typename T, bool GATHER>
void rows(T* fleet, T* stage, const int* idx, int count, int len, long fstride, hipStream_t st) {
    const int bx = len >= 256 ? 256 : 64;
    // blockIdx.y is limited to 65535: walk the bucket in slabs
    for (int r0 = 0; r0 < count; r0 += 65535) {
        const int n = std::min(65535, count - r0);
        T* s = stage + (long)r0 * len;
        hipLaunchKernelGGL((k_rows<T, GATHER>), dim3((len + bx - 1) / bx, n), dim3(bx), 0, st, GATHER ? fleet : s, GATHER ? s : fleet,
                           idx + r0, n, len, fstride);
    }
}

struct Bucket {
    int N = 0, count = 0;
    cfnmpc_solver* s = nullptr;
    std::vector<int> idx;       // fleet index of every bucket row
    int* d_idx = nullptr;
    void* d_stage = nullptr;    // staging in bucket order of device-pointer calls: n_stage bytes, grown on demand (staging())
    size_t n_stage = 0;
    hipStream_t st = nullptr;
    hipEvent_t done = nullptr;
};

}  // namespace

// (the fleet lives on the device that was current at cfnmpc_fleet_create, as its solvers do)
struct cfnmpc_fleet {
    int B = 0, Nmin = 0, Nmax = 0, device = 0;
    std::vector<Bucket> bk;       // ascending N (the order of cfnmpc_fleet_bucket)
    std::vector<int> order;       // bucket indices by decreasing work N x vehicles: launch order, stream priorities
    hipEvent_t fork = nullptr;
    std::vector<double> h_stage;  // host staging in bucket order (host-pointer calls)
};

namespace {

// run fn(bucket, stream) for every bucket on its own stream, forked from / joined to `user`
template <typename F>
int on_buckets(cfnmpc_fleet* f, hipStream_t user, F fn) {
    cfn::DeviceGuard dg(f->device);
    HIP_TRY(hipEventRecord(f->fork, user));
    for (int bi : f->order) {   // (heaviest bucket first)
        Bucket& b = f->bk[bi];
        HIP_TRY(hipStreamWaitEvent(b.st, f->fork, 0));
        RC_TRY(fn(b, b.st));
        HIP_TRY(hipEventRecord(b.done, b.st));
        HIP_TRY(hipStreamWaitEvent(user, b.done, 0));
    }
    return CFNMPC_OK;
}

// The bucket's device staging, at least `bytes` long.  The first allocation already holds the largest request of the step's
// calls (yref and yref_e: N x 17 + 13 doubles per vehicle), so those never reallocate; a longer request (a range of
// sensitivities) replaces the buffer once the bucket's stream -- the only one that uses it -- has drained.
int staging(Bucket& b, size_t bytes, hipStream_t st) {
    if (bytes <= b.n_stage) return CFNMPC_OK;
    if (b.d_stage) {
        HIP_TRY(hipStreamSynchronize(st));   // (an earlier call may still use the old buffer)
        (void)hipFree(b.d_stage);
        b.d_stage = nullptr;
        b.n_stage = 0;
    }
    const size_t want = std::max(bytes, sizeof(double) * (size_t)b.count * (b.N * 17 + 13));
    if (hipMalloc(&b.d_stage, want) != hipSuccess) return CFNMPC_ENOMEM;
    b.n_stage = want;
    return CFNMPC_OK;
}

// device arrays: the requested columns between the caller's arrays and the bucket's staging, one launch per column on `st`
template <bool GATHER>
void dev_rows(const Layout& L, const Bucket& b, hipStream_t st) {
    for (int i = 0; i < L.n; i++) {
        void* fl = L.c[i].p, *sg = L.at(b.d_stage, i);
        if (!fl) continue;
        if (L.c[i].esz == sizeof(double)) rows<double, GATHER>((double*)fl, (double*)sg, b.d_idx, b.count, (int)L.len[i], (long)L.stride[i], st);
        else rows<int, GATHER>((int*)fl, (int*)sg, b.d_idx, b.count, (int)L.len[i], (long)L.stride[i], st);
    }
}

// Every fleet-level array call.  The columns are laid out in the bucket's staging -- the fleet's host staging for host arrays
// (on_device 0 or 2: synchronous, bucket after bucket on the caller's stream), else the bucket's device staging, on the
// bucket's stream inside on_buckets -- and call(bucket, staged columns, on_device, stream) is the bucket's own setter / getter.
// WRITE: the rows are gathered from the caller's arrays before the call; else scattered to them after it.
template <bool WRITE, typename F>
int fleet_io(cfnmpc_fleet* f, int on_device, void* stream, Cols cols, F call) {
    if (cfn::is_host(on_device)) {
        cfn::DeviceGuard dg(f->device);
        for (Bucket& b : f->bk) {
            const Layout L(cols, b.count, b.N, f->Nmax);
            f->h_stage.resize((L.bytes + 7) / 8);
            void* base = f->h_stage.data();
            if (WRITE) cfn::move_rows<true>(L, base, b.idx.data(), b.count);
            RC_TRY(call(b, cfn::staged(L, base), (int)CFNMPC_ON_HOST, stream));
            if (!WRITE) cfn::move_rows<false>(L, base, b.idx.data(), b.count);
        }
        return CFNMPC_OK;
    }
    return on_buckets(f, (hipStream_t)stream, [&](Bucket& b, hipStream_t st) {
        const Layout L(cols, b.count, b.N, f->Nmax);
        RC_TRY(staging(b, L.bytes, st));
        if (WRITE) dev_rows<true>(L, b, st);
        RC_TRY(call(b, cfn::staged(L, b.d_stage), (int)CFNMPC_ON_DEVICE, (void*)st));
        if (!WRITE) dev_rows<false>(L, b, st);
        return (int)CFNMPC_OK;
    });
}
template <typename F>
int fleet_write(cfnmpc_fleet* f, int on_device, void* stream, Cols cols, F call) { return fleet_io<true>(f, on_device, stream, cols, call); }
template <typename F>
int fleet_read(cfnmpc_fleet* f, int on_device, void* stream, Cols cols, F call) { return fleet_io<false>(f, on_device, stream, cols, call); }

}  // namespace

extern "C" {

int cfnmpc_fleet_create(cfnmpc_fleet** out, int batch, const int* N_per_instance, const cfnmpc_opts* opts) {
    if (!out || batch < 1 || !N_per_instance) return CFNMPC_EINVAL;
    *out = nullptr;
    cfnmpc_opts o;
    RC_TRY(cfn::take_opts(opts, &o));
    const int cond_N2_req = o.cond_N2;
    if (cond_N2_req < 0) return CFNMPC_EINVAL;
    std::map<int, std::vector<int>> by_n;
    for (int i = 0; i < batch; i++) {
        if (N_per_instance[i] < 1) return CFNMPC_EINVAL;
        by_n[N_per_instance[i]].push_back(i);
    }
    cfnmpc_fleet* f = new cfnmpc_fleet;
    f->B = batch;
    f->Nmin = by_n.begin()->first;
    f->Nmax = by_n.rbegin()->first;
    int rc = CFNMPC_OK;
    if (hipGetDevice(&f->device) != hipSuccess || hipEventCreateWithFlags(&f->fork, hipEventDisableTiming) != hipSuccess) rc = CFNMPC_EHIP;
    for (auto& kv : by_n) {
        if (rc != CFNMPC_OK) break;
        f->bk.emplace_back();
        Bucket& b = f->bk.back();
        b.N = kv.first;
        b.count = (int)kv.second.size();
        b.idx = std::move(kv.second);
        o.N = b.N;
        // partial condensing applies per bucket: a bucket with no more than cond_N2 stages has nothing to condense
        // (cond_N2 >= N means "none", as for a single solver) instead of failing the whole fleet; a bucket whose
        // blocks would exceed the supported length is still refused by cfnmpc_create
        o.cond_N2 = (cond_N2_req > 0 && cond_N2_req < b.N) ? cond_N2_req : 0;
        rc = cfnmpc_create(&b.s, b.count, &o);
        if (rc != CFNMPC_OK) break;
        if (hipMalloc((void**)&b.d_idx, sizeof(int) * b.count) != hipSuccess) { rc = CFNMPC_ENOMEM; break; }
        if (hipMemcpy(b.d_idx, b.idx.data(), sizeof(int) * b.count, hipMemcpyHostToDevice) != hipSuccess ||
            hipEventCreateWithFlags(&b.done, hipEventDisableTiming) != hipSuccess) { rc = CFNMPC_EHIP; break; }
    }
    // Longest job first: the buckets run concurrently on their own streams, and the step lasts as long as the bucket with the
    // most work (N x vehicles: the N = 100 third of config C5 carries 55 % of the stage-steps) -- its launches go out first.
    // (Round 6 also gave the heavy bucket's stream the device's highest PRIORITY and the light one the lowest: +1.3 % in a fresh
    //  process, but -17 % inside bench.py's full run, where a dozen solvers' streams have been created and destroyed before --
    //  9.5 against 11.4 M RTI steps/s, A/B on one box, profiles/r06_notes.md section 7.  Plain streams.)
    if (rc == CFNMPC_OK) {
        f->order.resize(f->bk.size());
        for (size_t i = 0; i < f->bk.size(); i++) f->order[i] = (int)i;
        std::stable_sort(f->order.begin(), f->order.end(), [&](int a, int b) {
            return (long)f->bk[a].N * f->bk[a].count > (long)f->bk[b].N * f->bk[b].count;
        });
        for (Bucket& b : f->bk)
            if (rc == CFNMPC_OK && hipStreamCreateWithFlags(&b.st, hipStreamNonBlocking) != hipSuccess) rc = CFNMPC_EHIP;
    }
    if (rc != CFNMPC_OK) { cfnmpc_fleet_free(f); return rc; }
    *out = f;
    return CFNMPC_OK;
}

int cfnmpc_fleet_free(cfnmpc_fleet* f) {
    if (!f) return CFNMPC_EINVAL;
    cfn::DeviceGuard dg(f->device);
    (void)hipDeviceSynchronize();
    for (Bucket& b : f->bk) {
        if (b.s) cfnmpc_free(b.s);
        if (b.d_idx) (void)hipFree(b.d_idx);
        if (b.d_stage) (void)hipFree(b.d_stage);
        if (b.st) (void)hipStreamDestroy(b.st);
        if (b.done) (void)hipEventDestroy(b.done);
    }
    if (f->fork) (void)hipEventDestroy(f->fork);
    delete f;
    return CFNMPC_OK;
}

int cfnmpc_fleet_batch(const cfnmpc_fleet* f) { return f ? f->B : CFNMPC_EINVAL; }
int cfnmpc_fleet_max_horizon(const cfnmpc_fleet* f) { return f ? f->Nmax : CFNMPC_EINVAL; }
int cfnmpc_fleet_min_horizon(const cfnmpc_fleet* f) { return f ? f->Nmin : CFNMPC_EINVAL; }
int cfnmpc_fleet_num_buckets(const cfnmpc_fleet* f) { return f ? (int)f->bk.size() : CFNMPC_EINVAL; }

int cfnmpc_fleet_bucket(const cfnmpc_fleet* f, int bucket, int* N, int* count, cfnmpc_solver** solver, int* index) {
    if (!f || bucket < 0 || bucket >= (int)f->bk.size()) return CFNMPC_EINVAL;
    const Bucket& b = f->bk[bucket];
    if (N) *N = b.N;
    if (count) *count = b.count;
    if (solver) *solver = b.s;
    if (index) std::copy(b.idx.begin(), b.idx.end(), index);
    return CFNMPC_OK;
}

unsigned long long cfnmpc_fleet_workspace_bytes(const cfnmpc_fleet* f) {
    unsigned long long t = 0;
    if (f) for (const Bucket& b : f->bk) t += cfnmpc_workspace_bytes(b.s);
    return t;
}

int cfnmpc_fleet_set_x0(cfnmpc_fleet* f, const double* x0, int on_device, void* stream) {
    if (!f || !x0) return CFNMPC_EINVAL;
    return fleet_write(f, on_device, stream, {col(x0, 13)},
                       [](Bucket& b, Staged p, int mode, void* st) { return cfnmpc_set_x0(b.s, p.d(0), mode, st); });
}

int cfnmpc_fleet_set_yref(cfnmpc_fleet* f, const double* yref, const double* yref_e, int on_device, void* stream) {
    if (!f || !yref || !yref_e) return CFNMPC_EINVAL;
    return fleet_write(f, on_device, stream, {col_stages(yref, 17), col(yref_e, 13)},
                       [](Bucket& b, Staged p, int mode, void* st) { return cfnmpc_set_yref(b.s, p.d(0), p.d(1), mode, st); });
}

int cfnmpc_fleet_set_weights(cfnmpc_fleet* f, const double* W, const double* WN) {
    if (!f) return CFNMPC_EINVAL;
    for (Bucket& b : f->bk) RC_TRY(cfnmpc_set_weights(b.s, W, WN));
    return CFNMPC_OK;
}

// (every bucket is created from the same options, so a value one bucket refuses the first one refuses: nothing changes)
int cfnmpc_fleet_set_erk_steps(cfnmpc_fleet* f, int num_steps) {
    if (!f) return CFNMPC_EINVAL;
    for (Bucket& b : f->bk) RC_TRY(cfnmpc_set_erk_steps(b.s, num_steps));
    return CFNMPC_OK;
}

int cfnmpc_fleet_set_cost_scaling(cfnmpc_fleet* f, double stage_scale, double terminal_scale) {
    if (!f) return CFNMPC_EINVAL;
    for (Bucket& b : f->bk) RC_TRY(cfnmpc_set_cost_scaling(b.s, stage_scale, terminal_scale));
    return CFNMPC_OK;
}

// per-instance model parameters: host rows in the fleet's vehicle order -> each bucket's order, each bucket's copy on its own
// stream (complete when the call returns).  The rows are validated as a whole first, so a bad row leaves every bucket
// unchanged.  A bucket refuses parameters only for options every bucket shares (start_solve 2 / 3), so the FIRST bucket
// refuses and nothing has changed either (cfnmpc_fleet_set_erk_steps relies on the same).
int cfnmpc_fleet_set_model_params(cfnmpc_fleet* f, const double* p) {
    if (!f) return CFNMPC_EINVAL;
    if (p && !cfn::model_params_ok(p, (size_t)f->B * CFNMPC_NP)) return CFNMPC_EINVAL;
    return fleet_write(f, CFNMPC_ON_HOST, nullptr, {col(p, CFNMPC_NP)},
                       [](Bucket& b, Staged q, int mode, void*) { return cfnmpc_set_model_params(b.s, q.d(0), mode, b.st); });
}

// per-instance disturbance rows, host or device (the rows of an observer: every control step).  Host rows are validated as a
// whole first; a bucket refuses rows only for options every bucket shares (start_solve 2 / 3) or, with cond_N2, in the buckets
// that condense -- checked by the first call on each bucket before anything of that bucket changes.
int cfnmpc_fleet_set_disturbance(cfnmpc_fleet* f, const double* d, int on_device, void* stream) {
    if (!f) return CFNMPC_EINVAL;
    if (d && cfn::is_host(on_device) && !cfn::dist_rows_ok(d, (size_t)f->B * CFNMPC_ND)) return CFNMPC_EINVAL;
    return fleet_write(f, on_device, stream, {col(d, CFNMPC_ND)},
                       [](Bucket& b, Staged q, int mode, void* st) { return cfnmpc_set_disturbance(b.s, q.d(0), mode, st); });
}

int cfnmpc_fleet_get_disturbance(cfnmpc_fleet* f, double* d, int on_device, void* stream) {
    if (!f || !d) return CFNMPC_EINVAL;
    return fleet_read(f, on_device, stream, {col(d, CFNMPC_ND)},
                      [](Bucket& b, Staged q, int mode, void* st) { return cfnmpc_get_disturbance(b.s, q.d(0), mode, st); });
}

// per-instance cost weights: host rows in the fleet's vehicle order -> each bucket's order.  Validated as a whole first, and a
// bucket refuses rows only for options every bucket shares (start_solve 2 / 3, cond_N2), so the FIRST bucket refuses and nothing
// has changed (as cfnmpc_fleet_set_model_params).
int cfnmpc_fleet_set_weights_batch(cfnmpc_fleet* f, const double* W, const double* WN) {
    if (!f) return CFNMPC_EINVAL;
    if (!cfn::weight_rows_ok(W, WN, (size_t)f->B)) return CFNMPC_EINVAL;
    return fleet_write(f, CFNMPC_ON_HOST, nullptr, {col(W, 17), col(WN, 13)},
                       [](Bucket& b, Staged p, int mode, void*) { return cfnmpc_set_weights_batch(b.s, p.d(0), p.d(1), mode, b.st); });
}

int cfnmpc_fleet_set_box(cfnmpc_fleet* f, double u_min, double u_max) {
    if (!f || !(u_max > u_min)) return CFNMPC_EINVAL;
    for (Bucket& b : f->bk) RC_TRY(cfnmpc_set_box(b.s, u_min, u_max));
    return CFNMPC_OK;
}

// per-stage / per-input boxes for a fleet: host arrays [B][Nmax][4] in the fleet's vehicle order (rows behind a vehicle's
// own horizon are ignored); NULL, NULL returns every bucket to the scalar box
int cfnmpc_fleet_set_box_stages(cfnmpc_fleet* f, const double* lb, const double* ub) {
    if (!f || ((lb == nullptr) != (ub == nullptr))) return CFNMPC_EINVAL;
    return fleet_write(f, CFNMPC_ON_HOST, nullptr, {col_stages(lb, 4), col_stages(ub, 4)},
                       [](Bucket& b, Staged p, int mode, void* st) { return cfnmpc_set_box_stages(b.s, p.d(0), p.d(1), mode, st); });
}

int cfnmpc_fleet_init_iterate(cfnmpc_fleet* f, int mode, void* stream) {
    if (!f) return CFNMPC_EINVAL;
    return on_buckets(f, (hipStream_t)stream, [&](Bucket& b, hipStream_t st) { return cfnmpc_init_iterate(b.s, mode, st); });
}

int cfnmpc_fleet_solve(cfnmpc_fleet* f, int n_rti, void* stream) {
    if (!f || n_rti < 1) return CFNMPC_EINVAL;
    return on_buckets(f, (hipStream_t)stream, [&](Bucket& b, hipStream_t st) { return cfnmpc_solve(b.s, n_rti, st); });
}

int cfnmpc_fleet_get_u(cfnmpc_fleet* f, int stage, double* u, int on_device, void* stream) {
    if (!f || !u || stage < 0 || stage >= f->Nmin) return CFNMPC_EINVAL;
    return fleet_read(f, on_device, stream, {col(u, 4)},
                      [&](Bucket& b, Staged p, int mode, void* st) { return cfnmpc_get_u(b.s, stage, p.d(0), mode, st); });
}

int cfnmpc_fleet_get_x(cfnmpc_fleet* f, int stage, double* x, int on_device, void* stream) {
    if (!f || !x || stage < 0 || stage > f->Nmin) return CFNMPC_EINVAL;
    return fleet_read(f, on_device, stream, {col(x, 13)},
                      [&](Bucket& b, Staged p, int mode, void* st) { return cfnmpc_get_x(b.s, stage, p.d(0), mode, st); });
}

int cfnmpc_fleet_get_cmd(cfnmpc_fleet* f, double* cmd_vel, int* motvel, int on_device, void* stream) {
    if (!f || !cmd_vel || f->Nmin < 4) return CFNMPC_EINVAL;   // the output stage reads u1 and x4
    return fleet_read(f, on_device, stream, {col(cmd_vel, 4), col(motvel, 4)},
                      [](Bucket& b, Staged p, int mode, void* st) { return cfnmpc_get_cmd(b.s, p.d(0), p.i(1), mode, st); });
}

int cfnmpc_fleet_get_stats(cfnmpc_fleet* f, int* status, int* qp_iter, double* res, int on_device, void* stream) {
    if (!f) return CFNMPC_EINVAL;
    return fleet_read(f, on_device, stream, {col(status, 1), col(qp_iter, 1), col(res, 1)},
                      [](Bucket& b, Staged p, int mode, void* st) { return cfnmpc_get_stats(b.s, p.i(0), p.i(1), p.d(2), mode, st); });
}

// Full SQP solve over the buckets: every bucket still running enqueues its iteration (step + check + read-back of its count of
// open rows) on its own stream, then the host waits for all of them -- one synchronisation per iteration for the fleet.  A
// bucket whose rows are all done launches nothing more (the one place a fleet's SQP solve saves work).
int cfnmpc_fleet_solve_sqp(cfnmpc_fleet* f, int max_iter, double tol_step, double tol_eq, double tol_ineq, int* n_iter, void* stream) {
    if (!f) return CFNMPC_EINVAL;
    for (Bucket& b : f->bk) RC_TRY(cfn::sqp_check_args(b.s, max_iter, tol_step, tol_eq, tol_ineq));   // nothing enqueued yet
    cfn::DeviceGuard dg(f->device);
    hipStream_t user = (hipStream_t)stream;
    HIP_TRY(hipEventRecord(f->fork, user));
    std::vector<char> running(f->bk.size(), 1);
    for (int bi : f->order) {
        Bucket& b = f->bk[bi];
        HIP_TRY(hipStreamWaitEvent(b.st, f->fork, 0));
        RC_TRY(cfn::sqp_begin(b.s, max_iter, tol_step, tol_eq, tol_ineq, b.st));
    }
    int ran = 0;
    for (int j = 1; j <= max_iter; j++) {
        for (int bi : f->order)
            if (running[bi]) RC_TRY(cfn::sqp_iterate(f->bk[bi].s, f->bk[bi].st));   // (heaviest bucket first)
        ran = j;
        bool any = false;
        for (int bi : f->order) {
            if (!running[bi]) continue;
            unsigned open = 0;
            RC_TRY(cfn::sqp_wait(f->bk[bi].s, &open));
            running[bi] = open > 0;
            any = any || open > 0;
        }
        if (!any) break;
    }
    // (every bucket's work has completed; the join keeps the caller's stream ordered behind it all the same)
    for (Bucket& b : f->bk) {
        HIP_TRY(hipEventRecord(b.done, b.st));
        HIP_TRY(hipStreamWaitEvent(user, b.done, 0));
    }
    if (n_iter) *n_iter = ran;
    return CFNMPC_OK;
}

int cfnmpc_fleet_get_sqp_stats(cfnmpc_fleet* f, int* status, int* sqp_iter, double* res, int on_device, void* stream) {
    if (!f) return CFNMPC_EINVAL;
    return fleet_read(f, on_device, stream, {col(status, 1), col(sqp_iter, 1), col(res, 3)},
                      [](Bucket& b, Staged p, int mode, void* st) { return cfn::sqp_get_stats(b.s, p.i(0), p.i(1), p.d(2), mode, st); });
}

int cfnmpc_fleet_set_sqp_globalization(cfnmpc_fleet* f, int mode, double eta, double reduction, double alpha_min) {
    if (!f || f->bk.empty()) return CFNMPC_EINVAL;
    // (the check does not depend on the bucket: the first refusal comes before anything has changed)
    for (Bucket& b : f->bk) RC_TRY(cfn::sqp_set_globalization(b.s, mode, eta, reduction, alpha_min));
    return CFNMPC_OK;
}

int cfnmpc_fleet_get_sqp_ls_stats(cfnmpc_fleet* f, double* alpha, double* mu, int* n_short, int* n_fail, int on_device, void* stream) {
    if (!f || (!alpha && !mu && !n_short && !n_fail)) return CFNMPC_EINVAL;
    return fleet_read(f, on_device, stream, {col(alpha, 1), col(mu, 1), col(n_short, 1), col(n_fail, 1)},
                      [](Bucket& b, Staged p, int mode, void* st) { return cfn::sqp_get_ls_stats(b.s, p.d(0), p.d(1), p.i(2), p.i(3), mode, st); });
}

// ---- NLP evaluation at every bucket's current iterate (include/cfnmpc.h: cfnmpc_eval_nlp) -------------
int cfnmpc_fleet_eval_nlp(cfnmpc_fleet* f, void* stream) {
    if (!f) return CFNMPC_EINVAL;
    return on_buckets(f, (hipStream_t)stream, [&](Bucket& b, hipStream_t st) { return cfnmpc_eval_nlp(b.s, 0, st); });
}

// rows in the fleet's vehicle order: cost [B], res [B][3]
int cfnmpc_fleet_get_nlp_stats(cfnmpc_fleet* f, double* cost, double* res, int on_device, void* stream) {
    if (!f || (!cost && !res)) return CFNMPC_EINVAL;
    return fleet_read(f, on_device, stream, {col(cost, 1), col(res, 3)},
                      [](Bucket& b, Staged p, int mode, void* st) { return cfnmpc_get_nlp_stats(b.s, p.d(0), p.d(1), mode, st); });
}

// ---- solution sensitivities with respect to x0 (include/cfnmpc.h: cfnmpc_eval_sens_x0) --------------
int cfnmpc_fleet_eval_sens_x0(cfnmpc_fleet* f, double act_tol, void* stream) {
    if (!f) return CFNMPC_EINVAL;
    return on_buckets(f, (hipStream_t)stream, [&](Bucket& b, hipStream_t st) { return cfnmpc_eval_sens_x0(b.s, act_tol, st); });
}

// rows in the fleet's vehicle order: du [B][n_stages][4][13], dx [B][n_stages][13][13]; the range is limited by the shortest
// horizon (dx up to stage Nmin, du below it)
int cfnmpc_fleet_get_sens_x0(cfnmpc_fleet* f, int stage, int n_stages, double* du, double* dx, int on_device, void* stream) {
    if (!f || stage < 0 || n_stages < 1 || (!du && !dx) || (long)stage + n_stages > f->Nmin + 1 ||
        (du && stage + n_stages > f->Nmin))
        return CFNMPC_EINVAL;
    return fleet_read(f, on_device, stream, {col(du, (size_t)n_stages * 52), col(dx, (size_t)n_stages * 169)},
                      [&](Bucket& b, Staged p, int mode, void* st) { return cfnmpc_get_sens_x0(b.s, stage, n_stages, p.d(0), p.d(1), mode, st); });
}

// ---- adjoint sensitivities (include/cfnmpc.h: cfnmpc_eval_adjoint) -----------------------------------
int cfnmpc_fleet_eval_adjoint(cfnmpc_fleet* f, const double* gx, const double* gu, int n_g, int on_device, void* stream) {
    // (stages [0, n_g) below the shortest horizon: a terminal gradient would sit at another stage in every bucket)
    if (!f || (!gx && !gu) || n_g < 1 || n_g > f->Nmin) return CFNMPC_EINVAL;
    return fleet_write(f, on_device, stream, {col(gx, (size_t)n_g * 13), col(gu, (size_t)n_g * 4)},
                       [&](Bucket& b, Staged p, int mode, void* st) { return cfnmpc_eval_adjoint(b.s, p.d(0), n_g, p.d(1), n_g, mode, st); });
}

int cfnmpc_fleet_get_adjoint(cfnmpc_fleet* f, double* dl_dx0, double* dl_dW, double* dl_dWN, int on_device, void* stream) {
    if (!f || (!dl_dx0 && !dl_dW && !dl_dWN)) return CFNMPC_EINVAL;
    return fleet_read(f, on_device, stream, {col(dl_dx0, 13), col(dl_dW, 17), col(dl_dWN, 13)},
                      [](Bucket& b, Staged p, int mode, void* st) {
                          RC_TRY(cfnmpc_get_adjoint(b.s, p.d(0), nullptr, nullptr, nullptr, nullptr, mode, st));
                          return cfnmpc_get_adjoint_cost(b.s, p.d(1), p.d(2), nullptr, nullptr, mode, st);
                      });
}

// ---- uncertainty propagation and bound tightening (include/cfnmpc.h: cfnmpc_eval_uncertainty) --------
// host arrays are validated as a whole first: a bad matrix leaves every bucket unchanged
int cfnmpc_fleet_set_uncertainty(cfnmpc_fleet* f, const double* Sigma0, const double* W, int on_device, void* stream) {
    if (!f) return CFNMPC_EINVAL;
    if (cfn::is_host(on_device) && ((Sigma0 && !cfn::unc_sym_ok(Sigma0, (size_t)f->B)) || (W && !cfn::unc_sym_ok(W, (size_t)f->B))))
        return CFNMPC_EINVAL;
    return fleet_write(f, on_device, stream, {col(Sigma0, 169), col(W, 169)},
                       [](Bucket& b, Staged p, int mode, void* st) { return cfnmpc_set_uncertainty(b.s, p.d(0), p.d(1), mode, st); });
}

int cfnmpc_fleet_set_uncertainty_gain(cfnmpc_fleet* f, int mode, const double* K, int on_device, void* stream) {
    if (!f || (mode != CFNMPC_UNC_GAIN_RICCATI && mode != CFNMPC_UNC_GAIN_USER) || (mode == CFNMPC_UNC_GAIN_USER && !K)) return CFNMPC_EINVAL;
    if (mode == CFNMPC_UNC_GAIN_RICCATI) K = nullptr;
    if (K && cfn::is_host(on_device))
        for (size_t i = 0; i < (size_t)f->B * 52; i++) if (!std::isfinite(K[i])) return CFNMPC_EINVAL;
    return fleet_write(f, on_device, stream, {col(K, 52)},
                       [&](Bucket& b, Staged p, int md, void* st) { return cfnmpc_set_uncertainty_gain(b.s, mode, p.d(0), md, st); });
}

int cfnmpc_fleet_eval_uncertainty(cfnmpc_fleet* f, void* stream) {
    if (!f) return CFNMPC_EINVAL;
    return on_buckets(f, (hipStream_t)stream, [&](Bucket& b, hipStream_t st) { return cfnmpc_eval_uncertainty(b.s, st); });
}

// beta [B][Nmax][4]: NaN behind a vehicle's own horizon (the whole array is filled first; all bits set is a NaN)
int cfnmpc_fleet_get_backoff(cfnmpc_fleet* f, double* beta, int on_device, void* stream) {
    if (!f || !beta || !cfn::fleet_backoff_valid(f)) return CFNMPC_EINVAL;   // (checked before the caller's array is touched)
    const size_t bytes = (size_t)f->B * f->Nmax * 4 * sizeof(double);
    if (cfn::is_host(on_device)) std::memset(beta, 0xff, bytes);
    else {
        cfn::DeviceGuard dg(f->device);
        HIP_TRY(hipMemsetAsync(beta, 0xff, bytes, (hipStream_t)stream));
    }
    return fleet_read(f, on_device, stream, {col_stages(beta, 4)},
                      [](Bucket& b, Staged p, int mode, void* st) { return cfnmpc_get_backoff(b.s, p.d(0), mode, st); });
}

int cfnmpc_fleet_get_uncertainty(cfnmpc_fleet* f, int stage, int n_stages, double* Sigma, double* std_x, int on_device, void* stream) {
    if (!f || stage < 0 || n_stages < 1 || (!Sigma && !std_x) || (long)stage + n_stages > f->Nmin + 1) return CFNMPC_EINVAL;
    return fleet_read(f, on_device, stream, {col(Sigma, (size_t)n_stages * 169), col(std_x, (size_t)n_stages * 13)},
                      [&](Bucket& b, Staged p, int mode, void* st) { return cfnmpc_get_uncertainty(b.s, stage, n_stages, p.d(0), p.d(1), mode, st); });
}

int cfnmpc_fleet_tighten_box(cfnmpc_fleet* f, double gamma, double min_width, int* n_clamped, int on_device, void* stream) {
    // (what a bucket would refuse is checked for all of them first: no bucket is tightened when another has no backoff)
    if (!f || !cfn::fleet_backoff_valid(f) || !std::isfinite(gamma) || !(gamma >= 0.0) || !(min_width > 0.0) || !(min_width <= 1.0))
        return CFNMPC_EINVAL;
    return fleet_read(f, on_device, stream, {col(n_clamped, 1)},
                      [&](Bucket& b, Staged p, int mode, void* st) { return cfnmpc_tighten_box(b.s, gamma, min_width, p.i(0), mode, st); });
}

// ---- device-side polynomial trajectory references (include/cfnmpc.h: cfnmpc_set_yref_poly) ------------
// the library to every bucket (validated first: a bad table leaves every bucket unchanged)
int cfnmpc_fleet_set_poly_library(cfnmpc_fleet* f, const double* pieces, const int* first, int n_traj, void* stream) {
    if (!f || n_traj < 0) return CFNMPC_EINVAL;
    if (n_traj > 0 && pieces && first && !cfn::poly_library_ok(pieces, first, n_traj)) return CFNMPC_EINVAL;
    return on_buckets(f, (hipStream_t)stream, [&](Bucket& b, hipStream_t st) { return cfnmpc_set_poly_library(b.s, pieces, first, n_traj, st); });
}

// traj [B], place [B][6] or NULL in the fleet's vehicle order; host arrays are validated as a whole first
int cfnmpc_fleet_set_poly_assignment(cfnmpc_fleet* f, const int* traj, const double* place, int on_device, void* stream) {
    if (!f || !traj) return CFNMPC_EINVAL;
    if (cfn::is_host(on_device) && !cfn::poly_assignment_ok(traj, place, (size_t)f->B, cfn::fleet_poly_n_traj(f))) return CFNMPC_EINVAL;
    return fleet_write(f, on_device, stream, {col(traj, 1), col(place, CFNMPC_NPLACE)},
                       [](Bucket& b, Staged p, int mode, void* st) { return cfnmpc_set_poly_assignment(b.s, p.i(0), p.d(1), mode, st); });
}

// every bucket writes its own N + 1 rows at the shared t and dt
int cfnmpc_fleet_set_yref_poly(cfnmpc_fleet* f, double t, int flags, void* stream) {
    if (!f || cfn::fleet_poly_n_traj(f) == 0) return CFNMPC_EINVAL;   // (no bucket has written when the call is refused)
    return on_buckets(f, (hipStream_t)stream, [&](Bucket& b, hipStream_t st) { return cfnmpc_set_yref_poly(b.s, t, flags, st); });
}

// flat [B][Nmax][13], rows [B][Nmax][17]: every vehicle's own N stage rows, NaN behind its horizon (the arrays are filled first;
// all bits set is a NaN)
int cfnmpc_fleet_eval_poly(cfnmpc_fleet* f, double t, int flags, double* flat, double* rows, int on_device, void* stream) {
    if (!f || cfn::fleet_poly_n_traj(f) == 0 || (!flat && !rows)) return CFNMPC_EINVAL;
    const size_t nf = (size_t)f->B * f->Nmax * CFNMPC_NFLAT * sizeof(double), nr = (size_t)f->B * f->Nmax * 17 * sizeof(double);
    if (cfn::is_host(on_device)) {
        if (flat) std::memset(flat, 0xff, nf);
        if (rows) std::memset(rows, 0xff, nr);
    } else {
        cfn::DeviceGuard dg(f->device);
        if (flat) HIP_TRY(hipMemsetAsync(flat, 0xff, nf, (hipStream_t)stream));
        if (rows) HIP_TRY(hipMemsetAsync(rows, 0xff, nr, (hipStream_t)stream));
    }
    return fleet_read(f, on_device, stream, {col_stages(flat, CFNMPC_NFLAT), col_stages(rows, 17)},
                      [&](Bucket& b, Staged p, int mode, void* st) { return cfnmpc_eval_poly(b.s, t, b.N, flags, p.d(0), p.d(1), mode, st); });
}

}  // extern "C"

namespace cfn {
int fleet_poly_n_traj(const cfnmpc_fleet* f) { return f && !f->bk.empty() ? poly_n_traj(f->bk[0].s) : 0; }
bool fleet_backoff_valid(const cfnmpc_fleet* f) {
    if (!f) return false;
    for (const Bucket& b : f->bk) if (!unc_backoff_valid(b.s)) return false;
    return true;
}
}  // namespace cfn
