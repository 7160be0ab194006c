// cfnmpc_multi.cpp -- one fleet across several GPUs of a node from ONE process (include/cfnmpc.h,
// cfnmpc_multi_*): the native counterpart of the per-rank sharding that bench.py does with one
// process per GPU.
//
// NMPC instances are independent (one vehicle per solver in the reference: acados_mpc.cpp:76-82), so
// a fleet splits into contiguous shards with NO data-path exchange between devices: shard i owns the
// vehicles [lo_i, hi_i) on device device_ids[i], with its own cfnmpc_solver and its own stream
// created on that device.  cfnmpc_multi_solve launches every shard's RTI step and returns without
// waiting, so all devices work concurrently; the getters wait for the shard they read.  Host arrays
// at this boundary cover the WHOLE fleet in the caller's order.  For device-resident I/O take the
// shard's solver (cfnmpc_multi_shard) and use the single-device API with that device's pointers.
// Device ids may repeat (several shards on one GPU: used by the tests on a one-GPU box).
//
// Mixed horizons (BASELINE.json config C5; cfnmpc_multi_create_horizons): the vehicles are bucketed by horizon and dealt
// out over the shards so that sum N_i -- the cost model of a step -- is balanced (cfnmpc_shard_by_horizon below, SURVEY.md
// section 8e "Partitioning"); a shard is then a cfnmpc_fleet (one solver per horizon bucket) over a NON-contiguous index set
// and the host arrays of the whole fleet are gathered / scattered per shard.
//
// Every entry point names what it does on a shard twice, for its solver (uniform) and for its fleet (mixed); the shards are
// walked, and the arrays moved, by for_shards and multi_io below.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../include/cfnmpc.h"
#include "cfnmpc_host.hpp"
#include "cfnmpc_model.hpp"

namespace {
using cfn::col;
using cfn::col_stages;
using cfn::Cols;
using cfn::Layout;
using cfn::Staged;

struct Shard {
    int device = 0, lo = 0, hi = 0;
    cfnmpc_solver* s = nullptr;   // uniform horizon: vehicles [lo, hi)
    cfnmpc_fleet* f = nullptr;    // mixed horizons: vehicles idx[0..count) (ascending), lo = hi = -1
    std::vector<int> idx;
    int Nmax = 0;                 // longest horizon of this shard's fleet
    hipStream_t st = nullptr;
    std::vector<double> h;        // host staging in shard order (mixed)
};
}  // namespace

struct cfnmpc_multi {
    int B = 0, N = 0;             // N: the common horizon, or the longest one of a mixed fleet (row stride of yref / boxes)
    int Nmin = 0;
    bool mixed = false;
    std::vector<Shard> sh;
};

// for calls that ENQUEUE transfers on the shards' streams (CFNMPC_ON_HOST_ASYNC): on the first failing shard the earlier
// shards' copies may still be reading / writing the caller's arrays -- wait for them before the error is returned
#define RC_TRY_SYNC(m, x) do { int rc_ = (x); if (rc_ != CFNMPC_OK) { (void)cfnmpc_multi_sync(m); return rc_; } } while (0)

namespace {

// what both creators check first
int check_shards(cfnmpc_multi** out, int n_shards, const int* device_ids, int total_batch) {
    if (!out || n_shards < 1 || !device_ids || total_batch < n_shards) return CFNMPC_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CFNMPC_EHIP;
    for (int i = 0; i < n_shards; i++) if (device_ids[i] < 0 || device_ids[i] >= ndev) return CFNMPC_EINVAL;
    return CFNMPC_OK;
}

// on_solver(shard) on every shard of a uniform fleet, on_fleet(shard) on every shard of a mixed one; `wait`: for all the
// shards' streams afterwards (also behind a failure)
template <typename FS, typename FF>
int for_shards(cfnmpc_multi* m, FS on_solver, FF on_fleet, bool wait = false) {
    int rc = CFNMPC_OK;
    for (Shard& s : m->sh) {
        rc = m->mixed ? on_fleet(s) : on_solver(s);
        if (rc != CFNMPC_OK) break;
    }
    if (!wait) return rc;
    const int rs = cfnmpc_multi_sync(m);
    return rc != CFNMPC_OK ? rc : rs;
}

// Host arrays of the whole fleet.  Uniform shards are contiguous: every column is handed over in place, from row `lo` on, and
// every shard's transfer (+ layout kernel) is ENQUEUED on its own stream first (CFNMPC_ON_HOST_ASYNC), then the shards are
// waited for -- the copies of different GPUs overlap instead of running one after the other.  Mixed shards stage their rows in
// shard order; the shard's fleet call is synchronous and waits for that shard only (the other shards keep working meanwhile).
// WRITE: the rows are gathered before the call, else scattered after it.
template <bool WRITE, typename FS, typename FF>
int multi_io(cfnmpc_multi* m, Cols cols, FS on_solver, FF on_fleet) {
    for (Shard& s : m->sh) {
        if (!m->mixed) {
            const Layout L(cols, s.hi - s.lo, m->N, m->N);
            RC_TRY_SYNC(m, on_solver(s, cfn::in_place(L, s.lo), (int)CFNMPC_ON_HOST_ASYNC));
            continue;
        }
        const Layout L(cols, s.idx.size(), s.Nmax, m->N);
        s.h.resize((L.bytes + 7) / 8);
        if (WRITE) cfn::move_rows<true>(L, s.h.data(), s.idx.data(), s.idx.size());
        RC_TRY_SYNC(m, on_fleet(s, cfn::staged(L, s.h.data()), (int)CFNMPC_ON_HOST));
        if (!WRITE) cfn::move_rows<false>(L, s.h.data(), s.idx.data(), s.idx.size());
    }
    return m->mixed ? (int)CFNMPC_OK : cfnmpc_multi_sync(m);
}
template <typename FS, typename FF>
int multi_write(cfnmpc_multi* m, Cols cols, FS on_solver, FF on_fleet) { return multi_io<true>(m, cols, on_solver, on_fleet); }
template <typename FS, typename FF>
int multi_read(cfnmpc_multi* m, Cols cols, FS on_solver, FF on_fleet) { return multi_io<false>(m, cols, on_solver, on_fleet); }

}  // namespace

extern "C" {

int cfnmpc_multi_create(cfnmpc_multi** out, int n_shards, const int* device_ids, int total_batch, const cfnmpc_opts* opts) {
    RC_TRY(check_shards(out, n_shards, device_ids, total_batch));
    cfnmpc_opts o;
    RC_TRY(cfn::take_opts(opts, &o));
    cfnmpc_multi* m = new cfnmpc_multi;
    m->B = total_batch;
    m->N = o.N;
    const int base = total_batch / n_shards, rem = total_batch % n_shards;
    int lo = 0, rc = CFNMPC_OK;
    for (int i = 0; i < n_shards && rc == CFNMPC_OK; i++) {
        Shard s;
        s.device = device_ids[i];
        s.lo = lo;
        s.hi = lo + base + (i < rem ? 1 : 0);
        lo = s.hi;
        cfn::DeviceGuard d(s.device);
        rc = cfnmpc_create(&s.s, s.hi - s.lo, &o);
        if (rc == CFNMPC_OK && hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking) != hipSuccess) rc = CFNMPC_EHIP;
        m->sh.push_back(s);
    }
    if (rc != CFNMPC_OK) { cfnmpc_multi_free(m); return rc; }
    *out = m;
    return CFNMPC_OK;
}

// The partitioner of mixed-horizon fleets (pure host code): vehicles in order of decreasing horizon (stable), each to the
// shard with the smallest sum N so far (ties: lowest shard) -- longest-processing-time-first; with a handful of distinct
// horizons every shard ends with its share of every bucket and sum N agrees to within one vehicle's horizon.
int cfnmpc_shard_by_horizon(int batch, const int* N_per_instance, int n_shards, int* shard_of) {
    if (batch < 0 || n_shards < 1 || (batch > 0 && (!N_per_instance || !shard_of))) return CFNMPC_EINVAL;
    for (int i = 0; i < batch; i++) if (N_per_instance[i] < 1) return CFNMPC_EINVAL;
    std::vector<int> order(batch);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return N_per_instance[a] > N_per_instance[b]; });
    std::vector<long long> load(n_shards, 0);
    for (int i : order) {
        const int r = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        shard_of[i] = r;
        load[r] += N_per_instance[i];
    }
    return CFNMPC_OK;
}

int cfnmpc_multi_create_horizons(cfnmpc_multi** out, int n_shards, const int* device_ids, int total_batch, const int* N_per_instance,
                                 const cfnmpc_opts* opts) {
    if (!N_per_instance) return CFNMPC_EINVAL;
    RC_TRY(check_shards(out, n_shards, device_ids, total_batch));
    std::vector<int> of(total_batch);
    RC_TRY(cfnmpc_shard_by_horizon(total_batch, N_per_instance, n_shards, of.data()));
    cfnmpc_opts o;
    RC_TRY(cfn::take_opts(opts, &o));
    cfnmpc_multi* m = new cfnmpc_multi;
    m->B = total_batch;
    m->mixed = true;
    m->N = *std::max_element(N_per_instance, N_per_instance + total_batch);
    m->Nmin = *std::min_element(N_per_instance, N_per_instance + total_batch);
    m->sh.resize(n_shards);
    for (int i = 0; i < total_batch; i++) m->sh[of[i]].idx.push_back(i);     // ascending within a shard
    int rc = CFNMPC_OK;
    std::vector<int> hz;
    for (int i = 0; i < n_shards && rc == CFNMPC_OK; i++) {
        Shard& s = m->sh[i];
        s.device = device_ids[i];
        s.lo = s.hi = -1;
        hz.resize(s.idx.size());
        for (size_t r = 0; r < s.idx.size(); r++) hz[r] = N_per_instance[s.idx[r]];
        s.Nmax = *std::max_element(hz.begin(), hz.end());
        cfn::DeviceGuard d(s.device);
        rc = cfnmpc_fleet_create(&s.f, (int)hz.size(), hz.data(), &o);
        if (rc == CFNMPC_OK && hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking) != hipSuccess) rc = CFNMPC_EHIP;
    }
    if (rc != CFNMPC_OK) { cfnmpc_multi_free(m); return rc; }
    *out = m;
    return CFNMPC_OK;
}

int cfnmpc_multi_shard_fleet(const cfnmpc_multi* m, int shard, cfnmpc_fleet** fleet, int* count, int* index, int* device, void** stream) {
    if (!m || !m->mixed || shard < 0 || shard >= (int)m->sh.size()) return CFNMPC_EINVAL;
    const Shard& s = m->sh[shard];
    if (fleet) *fleet = s.f;
    if (count) *count = (int)s.idx.size();
    if (index) std::copy(s.idx.begin(), s.idx.end(), index);
    if (device) *device = s.device;
    if (stream) *stream = (void*)s.st;
    return CFNMPC_OK;
}

int cfnmpc_multi_free(cfnmpc_multi* m) {
    if (!m) return CFNMPC_EINVAL;
    for (Shard& s : m->sh) {
        cfn::DeviceGuard d(s.device);
        if (s.st) { (void)hipStreamSynchronize(s.st); (void)hipStreamDestroy(s.st); }
        if (s.s) cfnmpc_free(s.s);
        if (s.f) cfnmpc_fleet_free(s.f);
    }
    delete m;
    return CFNMPC_OK;
}

int cfnmpc_multi_batch(const cfnmpc_multi* m) { return m ? m->B : CFNMPC_EINVAL; }
int cfnmpc_multi_num_shards(const cfnmpc_multi* m) { return m ? (int)m->sh.size() : CFNMPC_EINVAL; }

int cfnmpc_multi_shard(const cfnmpc_multi* m, int shard, cfnmpc_solver** solver, int* lo, int* hi, int* device, void** stream) {
    if (!m || m->mixed || shard < 0 || shard >= (int)m->sh.size()) return CFNMPC_EINVAL;   // mixed fleets: cfnmpc_multi_shard_fleet
    const Shard& s = m->sh[shard];
    if (solver) *solver = s.s;
    if (lo) *lo = s.lo;
    if (hi) *hi = s.hi;
    if (device) *device = s.device;
    if (stream) *stream = (void*)s.st;
    return CFNMPC_OK;
}

int cfnmpc_multi_sync(cfnmpc_multi* m) {
    if (!m) return CFNMPC_EINVAL;
    for (Shard& s : m->sh) {
        cfn::DeviceGuard d(s.device);
        if (hipStreamSynchronize(s.st) != hipSuccess) return CFNMPC_EHIP;
    }
    return CFNMPC_OK;
}

int cfnmpc_multi_set_x0(cfnmpc_multi* m, const double* x0) {
    if (!m || !x0) return CFNMPC_EINVAL;
    return multi_write(m, {col(x0, 13)},
                       [](Shard& s, Staged p, int mode) { return cfnmpc_set_x0(s.s, p.d(0), mode, s.st); },
                       [](Shard& s, Staged p, int mode) { return cfnmpc_fleet_set_x0(s.f, p.d(0), mode, s.st); });
}

// yref [B][N][17] of the whole fleet (N: the longest horizon; a mixed shard's fleet reads the first Nmax_shard rows of each
// vehicle).  (Uniform: two arrays through ONE staging buffer per shard: the second put is ordered behind the first on the
// shard's stream.)
int cfnmpc_multi_set_yref(cfnmpc_multi* m, const double* yref, const double* yref_e) {
    if (!m || !yref || !yref_e) return CFNMPC_EINVAL;
    return multi_write(m, {col_stages(yref, 17), col(yref_e, 13)},
                       [](Shard& s, Staged p, int mode) { return cfnmpc_set_yref(s.s, p.d(0), p.d(1), mode, s.st); },
                       [](Shard& s, Staged p, int mode) { return cfnmpc_fleet_set_yref(s.f, p.d(0), p.d(1), mode, s.st); });
}

int cfnmpc_multi_set_box(cfnmpc_multi* m, double u_min, double u_max) {
    if (!m) return CFNMPC_EINVAL;
    return for_shards(m, [&](Shard& s) { return cfnmpc_set_box(s.s, u_min, u_max); },
                      [&](Shard& s) { return cfnmpc_fleet_set_box(s.f, u_min, u_max); });
}

// [B][N][4] of the whole fleet; NULL, NULL: back to the scalar box
int cfnmpc_multi_set_box_stages(cfnmpc_multi* m, const double* lb, const double* ub) {
    if (!m || ((lb == nullptr) != (ub == nullptr))) return CFNMPC_EINVAL;
    return multi_write(m, {col_stages(lb, 4), col_stages(ub, 4)},
                       [](Shard& s, Staged p, int mode) { return cfnmpc_set_box_stages(s.s, p.d(0), p.d(1), mode, s.st); },
                       [](Shard& s, Staged p, int) { return cfnmpc_fleet_set_box_stages(s.f, p.d(0), p.d(1)); });
}

int cfnmpc_multi_set_weights(cfnmpc_multi* m, const double* W, const double* WN) {
    if (!m) return CFNMPC_EINVAL;
    return for_shards(m, [&](Shard& s) { return cfnmpc_set_weights(s.s, W, WN); },
                      [&](Shard& s) { return cfnmpc_fleet_set_weights(s.f, W, WN); });
}

int cfnmpc_multi_set_erk_steps(cfnmpc_multi* m, int num_steps) {
    if (!m) return CFNMPC_EINVAL;
    return for_shards(m, [&](Shard& s) { return cfnmpc_set_erk_steps(s.s, num_steps); },
                      [&](Shard& s) { return cfnmpc_fleet_set_erk_steps(s.f, num_steps); });
}

int cfnmpc_multi_set_cost_scaling(cfnmpc_multi* m, double stage_scale, double terminal_scale) {
    if (!m) return CFNMPC_EINVAL;
    return for_shards(m, [&](Shard& s) { return cfnmpc_set_cost_scaling(s.s, stage_scale, terminal_scale); },
                      [&](Shard& s) { return cfnmpc_fleet_set_cost_scaling(s.f, stage_scale, terminal_scale); });
}

int cfnmpc_multi_set_model_params(cfnmpc_multi* m, const double* p) {
    if (!m) return CFNMPC_EINVAL;
    if (p && !cfn::model_params_ok(p, (size_t)m->B * CFNMPC_NP)) return CFNMPC_EINVAL;   // (as a whole: no shard changes)
    return multi_write(m, {col(p, CFNMPC_NP)},
                       [](Shard& s, Staged q, int mode) { return cfnmpc_set_model_params(s.s, q.d(0), mode, s.st); },
                       [](Shard& s, Staged q, int) { return cfnmpc_fleet_set_model_params(s.f, q.d(0)); });
}

int cfnmpc_multi_set_disturbance(cfnmpc_multi* m, const double* d) {
    if (!m) return CFNMPC_EINVAL;
    if (d && !cfn::dist_rows_ok(d, (size_t)m->B * CFNMPC_ND)) return CFNMPC_EINVAL;   // (as a whole: no shard changes)
    return multi_write(m, {col(d, CFNMPC_ND)},
                       [](Shard& s, Staged q, int mode) { return cfnmpc_set_disturbance(s.s, q.d(0), mode, s.st); },
                       [](Shard& s, Staged q, int mode) { return cfnmpc_fleet_set_disturbance(s.f, q.d(0), mode, s.st); });
}

int cfnmpc_multi_set_weights_batch(cfnmpc_multi* m, const double* W, const double* WN) {
    if (!m) return CFNMPC_EINVAL;
    if (!cfn::weight_rows_ok(W, WN, (size_t)m->B)) return CFNMPC_EINVAL;   // (as a whole: no shard changes)
    return multi_write(m, {col(W, 17), col(WN, 13)},
                       [](Shard& s, Staged p, int mode) { return cfnmpc_set_weights_batch(s.s, p.d(0), p.d(1), mode, s.st); },
                       [](Shard& s, Staged p, int) { return cfnmpc_fleet_set_weights_batch(s.f, p.d(0), p.d(1)); });
}

int cfnmpc_multi_init_iterate(cfnmpc_multi* m, int mode) {
    if (!m) return CFNMPC_EINVAL;
    return for_shards(m, [&](Shard& s) { return cfnmpc_init_iterate(s.s, mode, s.st); },
                      [&](Shard& s) { return cfnmpc_fleet_init_iterate(s.f, mode, s.st); });
}

// asynchronous: every device gets its work before anyone waits
int cfnmpc_multi_solve(cfnmpc_multi* m, int n_rti) {
    if (!m || n_rti < 1) return CFNMPC_EINVAL;
    return for_shards(m, [&](Shard& s) { return cfnmpc_solve(s.s, n_rti, s.st); },
                      [&](Shard& s) { return cfnmpc_fleet_solve(s.f, n_rti, s.st); });
}

int cfnmpc_multi_get_u(cfnmpc_multi* m, int stage, double* u) {
    if (!m || !u || (m->mixed && (stage < 0 || stage >= m->Nmin))) return CFNMPC_EINVAL;
    return multi_read(m, {col(u, 4)},
                      [&](Shard& s, Staged p, int mode) { return cfnmpc_get_u(s.s, stage, p.d(0), mode, s.st); },
                      [&](Shard& s, Staged p, int mode) { return cfnmpc_fleet_get_u(s.f, stage, p.d(0), mode, s.st); });
}

int cfnmpc_multi_get_x(cfnmpc_multi* m, int stage, double* x) {
    if (!m || !x || (m->mixed && (stage < 0 || stage > m->Nmin))) return CFNMPC_EINVAL;
    return multi_read(m, {col(x, 13)},
                      [&](Shard& s, Staged p, int mode) { return cfnmpc_get_x(s.s, stage, p.d(0), mode, s.st); },
                      [&](Shard& s, Staged p, int mode) { return cfnmpc_fleet_get_x(s.f, stage, p.d(0), mode, s.st); });
}

int cfnmpc_multi_get_cmd(cfnmpc_multi* m, double* cmd_vel, int* motvel) {
    if (!m || !cmd_vel) return CFNMPC_EINVAL;
    return multi_read(m, {col(cmd_vel, 4), col(motvel, 4)},
                      [](Shard& s, Staged p, int mode) { return cfnmpc_get_cmd(s.s, p.d(0), p.i(1), mode, s.st); },
                      [](Shard& s, Staged p, int mode) { return cfnmpc_fleet_get_cmd(s.f, p.d(0), p.i(1), mode, s.st); });
}

int cfnmpc_multi_get_stats(cfnmpc_multi* m, int* status, int* qp_iter, double* res) {
    if (!m) return CFNMPC_EINVAL;
    return multi_read(m, {col(status, 1), col(qp_iter, 1), col(res, 1)},
                      [](Shard& s, Staged p, int mode) { return cfnmpc_get_stats(s.s, p.i(0), p.i(1), p.d(2), mode, s.st); },
                      [](Shard& s, Staged p, int mode) { return cfnmpc_fleet_get_stats(s.f, p.i(0), p.i(1), p.d(2), mode, s.st); });
}

// ---- NLP evaluation over the whole fleet (cfnmpc_eval_nlp per shard; host arrays in the caller's order, synchronous) ----------
int cfnmpc_multi_eval_nlp(cfnmpc_multi* m) {
    if (!m) return CFNMPC_EINVAL;
    return for_shards(m, [](Shard& s) { return cfnmpc_eval_nlp(s.s, 0, s.st); },
                      [](Shard& s) { return cfnmpc_fleet_eval_nlp(s.f, s.st); }, true);
}

int cfnmpc_multi_get_nlp_stats(cfnmpc_multi* m, double* cost, double* res) {
    if (!m || (!cost && !res)) return CFNMPC_EINVAL;
    return multi_read(m, {col(cost, 1), col(res, 3)},
                      [](Shard& s, Staged p, int mode) { return cfnmpc_get_nlp_stats(s.s, p.d(0), p.d(1), mode, s.st); },
                      [](Shard& s, Staged p, int mode) { return cfnmpc_fleet_get_nlp_stats(s.f, p.d(0), p.d(1), mode, s.st); });
}

// ---- solution sensitivities with respect to x0 (host arrays over the whole fleet, caller's order; synchronous) ---------------
int cfnmpc_multi_eval_sens_x0(cfnmpc_multi* m, double act_tol) {
    if (!m) return CFNMPC_EINVAL;
    return for_shards(m, [&](Shard& s) { return cfnmpc_eval_sens_x0(s.s, act_tol, s.st); },
                      [&](Shard& s) { return cfnmpc_fleet_eval_sens_x0(s.f, act_tol, s.st); }, true);
}

int cfnmpc_multi_get_sens_x0(cfnmpc_multi* m, int stage, int n_stages, double* du, double* dx) {
    const int Nlim = m ? (m->mixed ? m->Nmin : m->N) : 0;
    if (!m || stage < 0 || n_stages < 1 || (!du && !dx) || (long)stage + n_stages > Nlim + 1 || (du && stage + n_stages > Nlim))
        return CFNMPC_EINVAL;
    return multi_read(m, {col(du, (size_t)n_stages * 52), col(dx, (size_t)n_stages * 169)},
                      [&](Shard& s, Staged p, int mode) { return cfnmpc_get_sens_x0(s.s, stage, n_stages, p.d(0), p.d(1), mode, s.st); },
                      [&](Shard& s, Staged p, int mode) { return cfnmpc_fleet_get_sens_x0(s.f, stage, n_stages, p.d(0), p.d(1), mode, s.st); });
}

// ---- adjoint sensitivities (host arrays over the whole fleet, caller's order; synchronous) -----------------------------------
int cfnmpc_multi_eval_adjoint(cfnmpc_multi* m, const double* gx, const double* gu, int n_g) {
    const int Nlim = m ? (m->mixed ? m->Nmin : m->N) : 0;
    if (!m || (!gx && !gu) || n_g < 1 || n_g > Nlim) return CFNMPC_EINVAL;
    return multi_write(m, {col(gx, (size_t)n_g * 13), col(gu, (size_t)n_g * 4)},
                       [&](Shard& s, Staged p, int mode) { return cfnmpc_eval_adjoint(s.s, p.d(0), n_g, p.d(1), n_g, mode, s.st); },
                       [&](Shard& s, Staged p, int mode) { return cfnmpc_fleet_eval_adjoint(s.f, p.d(0), p.d(1), n_g, mode, s.st); });
}

int cfnmpc_multi_get_adjoint(cfnmpc_multi* m, double* dl_dx0, double* dl_dW, double* dl_dWN) {
    if (!m || (!dl_dx0 && !dl_dW && !dl_dWN)) return CFNMPC_EINVAL;
    return multi_read(m, {col(dl_dx0, 13), col(dl_dW, 17), col(dl_dWN, 13)},
                      [](Shard& s, Staged p, int mode) {
                          RC_TRY(cfnmpc_get_adjoint(s.s, p.d(0), nullptr, nullptr, nullptr, nullptr, mode, s.st));
                          return cfnmpc_get_adjoint_cost(s.s, p.d(1), p.d(2), nullptr, nullptr, mode, s.st);
                      },
                      [](Shard& s, Staged p, int mode) { return cfnmpc_fleet_get_adjoint(s.f, p.d(0), p.d(1), p.d(2), mode, s.st); });
}

// ---- uncertainty propagation and bound tightening (host arrays over the whole fleet, caller's order; synchronous) ------------
int cfnmpc_multi_set_uncertainty(cfnmpc_multi* m, const double* Sigma0, const double* W) {
    if (!m) return CFNMPC_EINVAL;
    if ((Sigma0 && !cfn::unc_sym_ok(Sigma0, (size_t)m->B)) || (W && !cfn::unc_sym_ok(W, (size_t)m->B))) return CFNMPC_EINVAL;   // (as a whole: no shard changes)
    // (uniform shards: both arrays pass through ONE staging buffer per shard -- the solver orders the second put behind the first)
    return multi_write(m, {col(Sigma0, 169), col(W, 169)},
                       [](Shard& s, Staged p, int mode) { return cfnmpc_set_uncertainty(s.s, p.d(0), p.d(1), mode, s.st); },
                       [](Shard& s, Staged p, int mode) { return cfnmpc_fleet_set_uncertainty(s.f, p.d(0), p.d(1), mode, s.st); });
}

int cfnmpc_multi_set_uncertainty_gain(cfnmpc_multi* m, int mode, const double* K) {
    if (!m || (mode != CFNMPC_UNC_GAIN_RICCATI && mode != CFNMPC_UNC_GAIN_USER) || (mode == CFNMPC_UNC_GAIN_USER && !K)) return CFNMPC_EINVAL;
    if (mode == CFNMPC_UNC_GAIN_RICCATI) K = nullptr;
    if (K) for (size_t i = 0; i < (size_t)m->B * 52; i++) if (!std::isfinite(K[i])) return CFNMPC_EINVAL;
    return multi_write(m, {col(K, 52)},
                       [&](Shard& s, Staged p, int md) { return cfnmpc_set_uncertainty_gain(s.s, mode, p.d(0), md, s.st); },
                       [&](Shard& s, Staged p, int md) { return cfnmpc_fleet_set_uncertainty_gain(s.f, mode, p.d(0), md, s.st); });
}

int cfnmpc_multi_eval_uncertainty(cfnmpc_multi* m) {
    if (!m) return CFNMPC_EINVAL;
    return for_shards(m, [](Shard& s) { return cfnmpc_eval_uncertainty(s.s, s.st); },
                      [](Shard& s) { return cfnmpc_fleet_eval_uncertainty(s.f, s.st); }, true);
}

// beta [B][N][4] (N: the longest horizon): NaN behind a vehicle's own horizon (filled first; all bits set is a NaN)
int cfnmpc_multi_get_backoff(cfnmpc_multi* m, double* beta) {
    if (!m || !beta) return CFNMPC_EINVAL;
    for (const Shard& s : m->sh)   // (checked before the caller's array is touched)
        if (m->mixed ? !cfn::fleet_backoff_valid(s.f) : !cfn::unc_backoff_valid(s.s)) return CFNMPC_EINVAL;
    if (m->mixed) std::memset(beta, 0xff, (size_t)m->B * m->N * 4 * sizeof(double));
    return multi_read(m, {col_stages(beta, 4)},
                      [](Shard& s, Staged p, int mode) { return cfnmpc_get_backoff(s.s, p.d(0), mode, s.st); },
                      [](Shard& s, Staged p, int mode) { return cfnmpc_fleet_get_backoff(s.f, p.d(0), mode, s.st); });
}

int cfnmpc_multi_tighten_box(cfnmpc_multi* m, double gamma, double min_width, int* n_clamped) {
    if (!m) return CFNMPC_EINVAL;
    for (const Shard& s : m->sh)   // (no shard is tightened when another has no backoff)
        if (m->mixed ? !cfn::fleet_backoff_valid(s.f) : !cfn::unc_backoff_valid(s.s)) return CFNMPC_EINVAL;
    return multi_read(m, {col(n_clamped, 1)},
                      [&](Shard& s, Staged p, int mode) { return cfnmpc_tighten_box(s.s, gamma, min_width, p.i(0), mode, s.st); },
                      [&](Shard& s, Staged p, int mode) { return cfnmpc_fleet_tighten_box(s.f, gamma, min_width, p.i(0), mode, s.st); });
}

// ---- device-side polynomial trajectory references (per shard; host arrays over the whole fleet, caller's order) ----------------
int cfnmpc_multi_set_poly_library(cfnmpc_multi* m, const double* pieces, const int* first, int n_traj) {
    if (!m || n_traj < 0) return CFNMPC_EINVAL;
    if (n_traj > 0 && pieces && first && !cfn::poly_library_ok(pieces, first, n_traj)) return CFNMPC_EINVAL;   // (as a whole: no shard changes)
    return for_shards(m, [&](Shard& s) { return cfnmpc_set_poly_library(s.s, pieces, first, n_traj, s.st); },
                      [&](Shard& s) { return cfnmpc_fleet_set_poly_library(s.f, pieces, first, n_traj, s.st); }, true);
}

int cfnmpc_multi_set_poly_assignment(cfnmpc_multi* m, const int* traj, const double* place) {
    if (!m || !traj || m->sh.empty()) return CFNMPC_EINVAL;
    const int n_traj = m->mixed ? cfn::fleet_poly_n_traj(m->sh[0].f) : cfn::poly_n_traj(m->sh[0].s);
    if (!cfn::poly_assignment_ok(traj, place, (size_t)m->B, n_traj)) return CFNMPC_EINVAL;   // (as a whole: no shard changes)
    return multi_write(m, {col(traj, 1), col(place, CFNMPC_NPLACE)},
                       [](Shard& s, Staged p, int mode) { return cfnmpc_set_poly_assignment(s.s, p.i(0), p.d(1), mode, s.st); },
                       [](Shard& s, Staged p, int mode) { return cfnmpc_fleet_set_poly_assignment(s.f, p.i(0), p.d(1), mode, s.st); });
}

// asynchronous on every shard's stream, like cfnmpc_multi_solve
int cfnmpc_multi_set_yref_poly(cfnmpc_multi* m, double t, int flags) {
    if (!m || m->sh.empty()) return CFNMPC_EINVAL;
    if ((m->mixed ? cfn::fleet_poly_n_traj(m->sh[0].f) : cfn::poly_n_traj(m->sh[0].s)) == 0) return CFNMPC_EINVAL;
    return for_shards(m, [&](Shard& s) { return cfnmpc_set_yref_poly(s.s, t, flags, s.st); },
                      [&](Shard& s) { return cfnmpc_fleet_set_yref_poly(s.f, t, flags, s.st); });
}

}  // extern "C"
