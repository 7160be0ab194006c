// cfnmpc_api.cpp -- C-ABI of the batch engine (include/cfnmpc.h) over the HIP kernels.
// Host side only: allocation of the SoA workspace, AoS<->SoA staging, kernel launches.
// There is no CPU fallback: without a usable HIP device cfnmpc_create() fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <utility>
#include <vector>

#include "../../include/cfnmpc.h"
#include "cfnmpc_host.hpp"
#include "cfnmpc_model.hpp"
#include "cfnmpc_plan.hpp"
#include "cfnmpc_stage.hpp"
#include "cfnmpc_ws.hpp"
#include "cfnmpc_sqp.h"
#ifdef CFN_DEV
#include "cfnmpc_dev.h"
#endif

struct cfnmpc_solver {
    cfn::Params P{};
    int device = 0;
    std::vector<void*> allocs;
    double* stage_buf = nullptr;  // device staging buffer for AoS transfers (largest AoS array)
    size_t stage_doubles = 0;
    // cfnmpc_step_host: pinned host mirror + device buffers of one step's inputs / outputs (lazy)
    double *h_io = nullptr, *d_io = nullptr;
    size_t io_doubles = 0;
    unsigned long long bytes = 0;
    // optional per-kernel timing with HIP events on the launch stream (cfnmpc_set_profiling)
    int profiling = 0;
    std::vector<hipEvent_t> ev;  // EV_PER_STEP events per timed RTI step: start | linearise | factor | forward | compaction | active set | end
    size_t ev_used = 0;
    // preparation-phase overlap (development builds, CFNMPC_OVERLAP=1; always 0 in the product): the linearisation for the NEXT
    // step is written to the alternate (AR, BR, b) set while the interior-point kernel still
    // reads the current one
    int overlap = 0;
    double *AR2 = nullptr, *BR2 = nullptr, *b2 = nullptr;
    hipStream_t aux = nullptr;   // low-priority stream of the early linearisation pass
    hipEvent_t ev_start = nullptr, ev_aux = nullptr; // start solve done (on the caller's stream) / early pass done (on aux)
    bool lin_valid = false;   // (P.AR, P.BR, P.b) hold the linearisation of the current iterate
    int chunks_all = 1, chunks_list = 10; // workgroups per 64-instance group in the two linearisation passes
    // captured step (cfnmpc_opts.step_graph): the launches of one RTI step as a hipGraph, one per parity of
    // the iterate buffers (kernel arguments are by value and the host swaps xit / xitn after every step)
    int use_graph = 0;
    hipStream_t cap = nullptr;   // capture stream
    hipGraphExec_t gexec[2] = {nullptr, nullptr};
    hipEvent_t glaunched[2] = {nullptr, nullptr};   // recorded behind the last launch of gexec[p]: waited for before that exec is destroyed
    bool gvalid[2] = {false, false};
    int parity = 0;   // which of the two argument sets the NEXT step uses
    // stage-invariant references (Params.yuni): cfnmpc_set_yref launches k_yref_uniform behind its k_put; the
    // verdict travels through yvaries (device word -> pinned host word, both allocated with the first call) with yuni_ev behind the
    // copy, and the first step that follows waits for it once (resolve_yuni).  Every other writer of P.yref clears the flag unasked.
    int *yvaries = nullptr, *h_yvaries = nullptr;
    hipEvent_t yuni_ev = nullptr;
    bool yuni_pending = false;   // a verdict is on its way
    int reinit_failed = 0;   // cfnmpc_opts.reinit_failed
    double *lbs_keep = nullptr, *ubs_keep = nullptr; // per-stage boxes (cfnmpc_set_box_stages), allocated at the first call
    double* box_blk[4] = {nullptr, nullptr, nullptr, nullptr};   // ... the four blocks behind them (home lb / ub, compact lb / ub); a failed attempt keeps what it got
    // full SQP solve (cfnmpc_solve_sqp): per-instance results and counters of k_sqp_check (sqp.j / max_iter / tolerances of the
    // running solve), the pinned word the host reads the count of open rows through, and the event it waits for
    cfn::SqpArgs sqp{};
    unsigned* h_sqp_cnt = nullptr;
    hipEvent_t sqp_ev = nullptr;
    // globalisation of the SQP solve (cfnmpc_set_sqp_globalization): the setting (mode, alpha_min; eta / reduction / T in ls),
    // k_sqp_ls's per-instance state (allocated at the first globalised solve), whether the RUNNING solve is globalised, and
    // what the last solve was (-1: none yet, else its mode) for cfnmpc_get_sqp_ls_stats
    int glob_mode = CFNMPC_SQP_FULL_STEP;
    double glob_alpha_min = 1.0 / 1024.0;
    cfn::LsArgs ls = {nullptr, nullptr, nullptr, nullptr, /* eta */ 1e-4, /* reduction */ 0.5, /* T */ 10};
    bool ls_active = false;
    int ls_last = -1;
    // stage-cost scaling (cfnmpc_set_cost_scaling): the weights as the caller set them; P.W = stage_scale * W_set,
    // P.WN = terminal_scale * WN_set
    double W_set[17] = {}, WN_set[13] = {};
    double stage_scale = 1.0, terminal_scale = 1.0;
    // per-instance model parameters (cfnmpc_set_model_params): the caller's rows [B][NPAR] while set (empty: nominal) and the
    // device block of derived constants P.mpar points to while set (allocated at the first call, kept for later ones)
    std::vector<double> mp_rows;
    double* mpar_buf = nullptr;
    // per-instance disturbance rows (cfnmpc_set_disturbance): the device table P.dist points to while set (allocated at the first
    // call, kept for later ones).  While set, P.mpar is set too: the caller's rows, or the nominal ones if there are none
    double* dist_buf = nullptr;
    // per-instance cost weights (cfnmpc_set_weights_batch): the caller's unscaled rows [B][17] / [B][13] while set (empty: the
    // uniform W_set / WN_set) and the device table P.wtab points to while set (allocated at the first call, kept for later ones)
    std::vector<double> w_rows, wn_rows;
    double* wtab_buf = nullptr;
    // solution sensitivities (cfnmpc_eval_sens_x0): what the last QP was (0: none, or its data changed since; 1: an RTI step;
    // 2: an SQP iteration, whose status is sqp.status), whether an evaluation belongs to it, the buffers (allocated at the
    // first evaluation) and the staging buffer of host reads
    int sens_src = 0;
    bool sens_valid = false;
    cfn::SensArgs sens{};
    double* sens_stage = nullptr;
    size_t sens_stage_doubles = 0;
    // adjoint sensitivities (cfnmpc_eval_adjoint): the buffers (allocated at the first evaluation; adj_gx / adj_gu hold the
    // gradients a caller hands over as host arrays) and whether an evaluation belongs to the sensitivity evaluation in force
    cfn::AdjArgs adj{};
    double *adj_gx = nullptr, *adj_gu = nullptr;
    bool adj_valid = false;
    // NLP evaluation (cfnmpc_eval_nlp): cost [B] and residuals [B][3] (allocated with the solver), costates and reduced gradient
    // (allocated at the first evaluation that keeps them), and what the last evaluation left (0: none yet, 1: cost and residuals,
    // 2: the multipliers too)
    cfn::NlpArgs nlp{};
    int nlp_state = 0;
    // uncertainty propagation and robust input-bound tightening (cfnmpc_eval_uncertainty / cfnmpc_tighten_box; DESIGN.md
    // section 5.21); every buffer is allocated at the first call that needs it
    struct Unc {
        double* stage = nullptr;     // staging of host arrays, [B][13][13] (the solver's own staging buffer may be shorter)
        double *S0 = nullptr, *W = nullptr, *K = nullptr;   // the tables (cfnmpc_ws.hpp: UncArgs) ...
        bool has_S0 = false, has_W = false;                 // ... and whether one is in force (NULL given: zero)
        int gain_mode = CFNMPC_UNC_GAIN_RICCATI;
        double* beta = nullptr;      // backoffs, home 4-vector layout
        bool beta_valid = false;     // until the next evaluation, cfnmpc_init_iterate or cfnmpc_set_iterate
        bool current = false;        // the evaluation belongs to the last QP (cfnmpc_get_uncertainty sweeps its blocks)
        bool inputs_moved = false;   // cfnmpc_set_x0 / cfnmpc_set_yref since the last solve
        int* ncl = nullptr;          // [B] clamped entries of the last tightening
        // the nominal box while a tightened one is in force: per-stage (the copies below, home layout) or the scalar box
        double *nom_lb = nullptr, *nom_ub = nullptr;
        bool tight = false, nom_stages = false;
    } unc;
    // device-side polynomial trajectory references (cfnmpc_set_poly_library / cfnmpc_set_yref_poly): the
    // library tables (at their limits), the assignment [B] and the placement rows [B][6], allocated together at the first call
    struct Poly {
        double* pieces = nullptr;
        int* first = nullptr;
        int n_traj = 0;
        int* traj = nullptr;
        double* place = nullptr;
        bool has_place = false;   // (NULL given: the identity placement for everybody)
    } poly;
};

namespace {

using cfn::DeviceGuard;
using cfn::is_host;

constexpr size_t MAX_PROFILED_STEPS = 4096;   // cfnmpc_get_profile resets the count
constexpr size_t EV_PER_STEP = 7;
template <typename T>
int dev_alloc(cfnmpc_solver* s, T** p, size_t count) {
    void* q = nullptr;
    if (hipMalloc(&q, count * sizeof(T)) != hipSuccess) return CFNMPC_ENOMEM;
    s->allocs.push_back(q);   // (before the memset: cfnmpc_free releases it on any later failure)
    if (hipMemset(q, 0, count * sizeof(T)) != hipSuccess) return CFNMPC_EHIP;
    // hipMemset of device memory only ENQUEUES the fill on the null stream.  Buffers allocated at first use (the sensitivity
    // arguments, the weight table, the line-search state, ...) are written right afterwards by kernels on the CALLER's stream; on
    // a non-blocking stream (the shards of cfnmpc_multi, the buckets of cfnmpc_fleet) those are not ordered behind the null
    // stream, and the fill could land on top of what they wrote.  Complete it here: allocations are off the step's path.
    if (hipStreamSynchronize(nullptr) != hipSuccess) return CFNMPC_EHIP;
    s->bytes += count * sizeof(T);
    *p = static_cast<T*>(q);
    return CFNMPC_OK;
}

// copy an AoS array [B][S][E] (external state order) from the caller into a workspace field
int put_field(cfnmpc_solver* s, const double* src, int on_device, int S, int E, int perm13, double* field,
              hipStream_t st) {
    const cfn::Params& P = s->P;
    const size_t n = (size_t)P.B * S * E;
    const double* dsrc = src;
    const bool host = is_host(on_device);
    if (host) {
        if (n > s->stage_doubles) return CFNMPC_EINVAL;
        HIP_TRY(hipMemcpyAsync(s->stage_buf, src, n * sizeof(double), hipMemcpyHostToDevice, st));
        dsrc = s->stage_buf;
    }
    cfn::launch_put(P.B, S, E, perm13, dsrc, field, st, E == 4 ? P.v4b : 0);
    HIP_TRY(hipGetLastError());
    // the staging buffer is reused: wait, unless the caller orders the next use on the same stream itself
    if (on_device == CFNMPC_ON_HOST) HIP_TRY(hipStreamSynchronize(st));
    return CFNMPC_OK;
}

// copy stages s0..s0+S-1 of a workspace field into the caller's AoS array [B][S][E]
int get_field(cfnmpc_solver* s, double* dst, int on_device, int S, int E, int perm13, int s0, int Stot,
              const double* field, hipStream_t st) {
    const cfn::Params& P = s->P;
    const size_t n = (size_t)P.B * S * E;
    double* ddst = dst;
    const bool host = is_host(on_device);
    if (host) {
        if (n > s->stage_doubles) return CFNMPC_EINVAL;
        ddst = s->stage_buf;
    }
    cfn::launch_get(P.B, S, E, perm13, s0, Stot, field, ddst, st, E == 4 ? P.v4b : 0);
    HIP_TRY(hipGetLastError());
    if (host) {
        HIP_TRY(hipMemcpyAsync(dst, ddst, n * sizeof(double), hipMemcpyDeviceToHost, st));
        if (on_device == CFNMPC_ON_HOST) HIP_TRY(hipStreamSynchronize(st));
    }
    return CFNMPC_OK;
}

// The flat getters: device arrays of the solver -> the caller's host or device arrays, one copy per output that was asked for
// (dst != nullptr) on `st`; complete on return for CFNMPC_ON_HOST.
struct Out { void* dst; const void* src; size_t bytes; };
int copy_out(std::initializer_list<Out> outs, int on_device, hipStream_t st) {
    const hipMemcpyKind kind = is_host(on_device) ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    for (const Out& o : outs)
        if (o.dst) HIP_TRY(hipMemcpyAsync(o.dst, o.src, o.bytes, kind, st));
    if (on_device == CFNMPC_ON_HOST) HIP_TRY(hipStreamSynchronize(st));
    return CFNMPC_OK;
}

// Host reads of per-row outputs that may exceed any one buffer (cfnmpc_get_sens_x0, cfnmpc_get_uncertainty): the rows in chunks
// of whole wavefronts through a staging buffer of at most 32 Mi doubles, allocated at the first such read.  `per`: doubles per
// row; chunk(b0, nb, stage) launches for the rows [b0, b0 + nb) into `stage` and enqueues its copies to the caller's arrays.
template <typename F>
int host_row_chunks(cfnmpc_solver* s, size_t per, F chunk) {
    const size_t B = s->P.B, cap_max = (size_t)1 << 25;
    // (rows longer than the ranges the buffer was sized for -- cfnmpc_eval_poly over many stages: a buffer for 64 of them replaces
    //  it; the old one stays with the solver until cfnmpc_free, a transfer in flight may still read it)
    const size_t floor = per * std::min(B, (size_t)4);
    if (!s->sens_stage || s->sens_stage_doubles < floor) {
        const size_t want = std::max(std::min(B * (size_t)(s->P.N + 1) * 221, cap_max), std::min(per * std::min(B, (size_t)64), cap_max));
        if (want < floor) return CFNMPC_ENOMEM;
        double* buf = nullptr;
        const int rc = dev_alloc(s, &buf, want);
        if (rc != CFNMPC_OK) return rc;
        s->sens_stage = buf;
        s->sens_stage_doubles = want;
    }
    size_t rows = s->sens_stage_doubles / per;
    rows = rows >= B ? B : (rows & ~(size_t)3);   // (fewer than four rows: the buffer holds them all)
    if (rows == 0) return CFNMPC_ENOMEM;   // (unreachable: the buffer holds four rows of the longest range)
    for (size_t b0 = 0; b0 < B; b0 += rows) RC_TRY(chunk(b0, std::min(rows, B - b0), s->sens_stage));
    return CFNMPC_OK;
}

using cfn::weights_ok;
static_assert(cfn::PLAN_COND_MMAX == cfn::COND_MMAX, "cfnmpc_plan.hpp states the longest condensed block of cfnmpc_ws.hpp");

// The environment of the development build (make DEV=1; the shipped library reads no environment variable).  Before the options
// are resolved (plan == nullptr): CFNMPC_OVERLAP, the overlapped preparation -- the next step's linearisation beside the
// constrained rows' kernels, double-buffered A / B / b; measured slower at every fleet size, since round 6
// an experiment and not an option of the product.  Behind it: CFNMPC_LIN_CHUNKS=a,b, CFNMPC_AS_PASSES (internal encoding) and
// CFNMPC_AS_GRID replace what the plan chose.  A forced scheduling drops the dense structure, which lives in the solves + commit
// one only, and is refused beside the fused start solve, which lives in the monolithic one.
int dev_env(cfn::Plan* plan) {
#ifdef CFN_DEV
    if (!plan) {
        const char* e = std::getenv("CFNMPC_OVERLAP");
        return e && std::atoi(e) ? 1 : 0;
    }
    if (const char* e = std::getenv("CFNMPC_LIN_CHUNKS")) {
        int a = 0, b = 0;
        if (std::sscanf(e, "%d,%d", &a, &b) == 2 && a > 0 && b > 0) { plan->chunks_all = a; plan->chunks_list = b; }
    }
    if (const char* e = std::getenv("CFNMPC_AS_PASSES")) {
        const int v = std::atoi(e);
        if (v >= -2 && v <= 12 && v != plan->as_passes) {
            if (plan->fused == 1) return CFNMPC_EINVAL;
            plan->as_passes = v;
            plan->as_dense = plan->wants_side_streams = plan->fwd_split = 0;
        }
    }
    if (const char* e = std::getenv("CFNMPC_AS_GRID")) {
        const int v = std::atoi(e);
        if (v > 0) { plan->as_grid = v; plan->as_sparse_max = v / 2; }
    }
#else
    (void)plan;
#endif
    return 0;
}

}  // namespace

extern "C" {

const char* cfnmpc_version(void) { return "cfnmpc 0.9 (gfx950; row-group Riccati with fused DPP broadcast FMAs, lane-per-instance linearisation and matrix-free forward sweep, primal-dual active-set QP solves; options: fused start solve (linearisation inside the factorisation), partial condensing, small-fleet forward sweep; device output stage; multi-GPU shards)"; }

void cfnmpc_default_opts(cfnmpc_opts* o) {
    // generate_c_code.py:41-42,63-84,109,133-134
    static const double W[CFNMPC_NY] = {120.0, 100.0, 100.0, 1e-3, 1e-3, 1e-3, 1e-3, 0.7, 1.0,
                                        4.0,   1e-5,  1e-5,  10.0, 0.06, 0.06, 0.06, 0.06};
    o->struct_size = (int)sizeof(cfnmpc_opts);
    o->N = 50;
    o->dt = 0.75 / 50;
    for (int i = 0; i < CFNMPC_NY; i++) o->W[i] = W[i];
    for (int i = 0; i < CFNMPC_NYN; i++) o->WN[i] = 50.0 * W[i];
    o->u_min = 0.0;
    o->u_max = 22.0;
    o->tol = 1e-8;
    o->max_iter = 50;
    o->tau = 0.995;
    o->thr0 = 1.0;
    o->lam0_min = 1e-2;
    o->mu0_scale = 0.1;
    o->active_horizon = 1;
    o->ah_margin = 0.10;
    o->ah_extra = 4;
    o->active_set = 1;
    o->forward_sweep = 0;
    o->cond_N2 = 0;
    o->step_graph = 0;
    o->as_passes = 0;
    o->ipm_clip_viol = 2.0;
    o->ipm_clip_margin = 0.05;
    o->as_skip_viol = 4.0;
    o->reinit_failed = 0;
    o->start_solve = 0;
    o->as_warm = 0;
    o->as_dense = 0;
    o->forward_split = 0;
}

int cfnmpc_default_opts_v(cfnmpc_opts* o, int sizeof_opts) {
    if (!o || sizeof_opts != (int)sizeof(cfnmpc_opts)) return CFNMPC_EINVAL;   // nothing is written into a struct of another size
    cfnmpc_default_opts(o);
    return CFNMPC_OK;
}
int cfnmpc_opts_size(void) { return (int)sizeof(cfnmpc_opts); }
int cfnmpc_abi_version(void) { return CFNMPC_ABI_VERSION; }

int cfnmpc_create(cfnmpc_solver** out, int batch, const cfnmpc_opts* opts) {
    if (!out || batch <= 0) return CFNMPC_EINVAL;
    // 1. the options -> the plan (cfnmpc_plan.hpp): every refusal happens here, before anything is owned
    cfnmpc_opts o;
    RC_TRY(cfn::take_opts(opts, &o));
    int device = 0, simds = 1024;   // SIMDs of the device the solver is created on
    hipDeviceProp_t prop;
    const bool have_device = hipGetDevice(&device) == hipSuccess;
    if (have_device && hipGetDeviceProperties(&prop, device) == hipSuccess) simds = 4 * prop.multiProcessorCount;
    cfn::Plan plan;
    RC_TRY(cfn::resolve_plan(o, batch, simds, dev_env(nullptr), &plan));
    RC_TRY(dev_env(&plan));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        std::fprintf(stderr, "cfnmpc: no HIP device available (this library has no CPU path)\n");
        return CFNMPC_EHIP;
    }
    if (!have_device) return CFNMPC_EHIP;
    // 2. the solver, with the plan copied into it and into the kernels' parameters
    cfnmpc_solver* s = new (std::nothrow) cfnmpc_solver();
    if (!s) return CFNMPC_ENOMEM;
    s->device = device;
    s->overlap = plan.overlap;
    s->use_graph = plan.use_graph;
    s->reinit_failed = plan.reinit_failed;
    s->chunks_all = plan.chunks_all;
    s->chunks_list = plan.chunks_list;
    cfn::Params& P = s->P;
    P.B = batch;
    P.NW = (batch + 3) / 4;
    P.N = o.N;
    P.dt = o.dt;
    for (int i = 0; i < 17; i++) P.W[i] = s->W_set[i] = o.W[i];
    for (int i = 0; i < 13; i++) P.WN[i] = s->WN_set[i] = o.WN[i];
    P.erk_steps = 1;
    P.u_min = o.u_min; P.u_max = o.u_max; P.tol = o.tol; P.tau = o.tau; P.thr0 = o.thr0;
    P.lam0_min = o.lam0_min; P.mu0_scale = o.mu0_scale; P.max_iter = o.max_iter;
    P.clip_viol = o.ipm_clip_viol; P.clip_margin = o.ipm_clip_margin; P.as_skip_viol = o.as_skip_viol;
    P.active_horizon = plan.active_horizon;
    P.ah_margin = o.ah_margin;
    P.ah_extra = o.ah_extra;
    P.active_set = plan.active_set;
    P.as_warm = plan.as_warm;
    P.as_passes = plan.as_passes;
    P.as_grid = plan.as_grid;
    P.as_sparse_max = plan.as_sparse_max;
    P.ipm_listed = plan.ipm_listed;
    P.as_dense = plan.as_dense;
    P.forward_rg = plan.forward_rg;
    P.fused = plan.fused;
    P.clist_chunks = plan.clist_chunks;
    P.cond_N2 = plan.cond_N2;
    P.cond_M = plan.cond_M;
    P.cond_rem = plan.cond_rem;
    P.ab16 = plan.ab16;
    P.v4b = plan.v4b;
    // 3. side streams, workspace, iterate: from here on every failure is cfnmpc_free(s)
    if (plan.wants_side_streams) {   // without them the kernels simply run one after the other
        hipStream_t side = nullptr;
        hipEvent_t ef = nullptr, ej = nullptr;
        if (hipStreamCreateWithFlags(&side, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&ef, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&ej, hipEventDisableTiming) == hipSuccess) {
            P.as_side = side; P.as_fork = ef; P.as_join = ej;
            hipStream_t side2 = nullptr;
            hipEvent_t ej2 = nullptr;
            if (hipStreamCreateWithFlags(&side2, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&ej2, hipEventDisableTiming) == hipSuccess) {
                P.as_side2 = side2; P.as_join2 = ej2;
            } else {
                if (side2) (void)hipStreamDestroy(side2);
                (void)hipGetLastError();
            }
        } else {
            if (side) (void)hipStreamDestroy(side);
            if (ef) (void)hipEventDestroy(ef);
            (void)hipGetLastError();
        }
    }
    // (without the second side stream -- its creation failed -- the sweep stays in one launch)
    P.fwd_split = P.as_side2 ? plan.fwd_split : 0;
    // one spare workspace block (index P.NW) parks the idle rows of compacted interior-point waves
    const size_t NW = P.NW + 1, N = P.N;
    int rc = CFNMPC_OK;
#define ALLOC(field, cnt) if (rc == CFNMPC_OK) rc = dev_alloc(s, &P.field, (size_t)(cnt))
    ALLOC(xit, NW * (N + 1) * cfn::SZ_V13); ALLOC(uit, NW * 4 * N * 4);
    ALLOC(xitn, NW * (N + 1) * cfn::SZ_V13); ALLOC(uitn, NW * 4 * N * 4); ALLOC(x0, NW * cfn::SZ_V13);
    ALLOC(yref, NW * N * cfn::SZ_Y); ALLOC(yref_e, NW * cfn::SZ_V13);
    // (the linearisation's home fields are laid out and written in groups of 16 blocks, P.ab16)
    const size_t NW16 = ((size_t)P.NW / 16 + 1) * 16;   // whole groups of 16 blocks, the spare block NW included (cfnmpc_rg.hpp: abidx)
    ALLOC(AR, NW16 * N * cfn::SZ_A); ALLOC(BR, NW16 * N * cfn::SZ_B); ALLOC(b, NW16 * N * cfn::SZ_V13);
    ALLOC(KR, NW * N * cfn::SZ_K); ALLOC(Sinv, NW * N * cfn::SZ_S);
    ALLOC(d, NW * 4 * N * 4); ALLOC(Pchk, NW * cfn::N_CHK * cfn::SZ_PP);
    ALLOC(v, NW * 4 * N * 4); ALLOC(tl, NW * 4 * N * 4); ALLOC(tu, NW * 4 * N * 4); ALLOC(ll, NW * 4 * N * 4);
    ALLOC(lu, NW * 4 * N * 4); ALLOC(rg, NW * 4 * N * 4); ALLOC(dva, NW * 4 * N * 4); ALLOC(dvc, NW * 4 * N * 4);
    ALLOC(Rh, NW * 4 * N * 4); ALLOC(g, NW * 4 * N * 4);
    ALLOC(cAR, NW * N * cfn::SZ_A); ALLOC(cBR, NW * N * cfn::SZ_B); ALLOC(cKR, NW * N * cfn::SZ_K);
    ALLOC(cSinv, NW * N * cfn::SZ_S); ALLOC(cd, NW * 4 * N * 4); ALLOC(cPchk, NW * cfn::N_CHK * cfn::SZ_P);
    ALLOC(cv, NW * 4 * N * 4); ALLOC(cuit, NW * 4 * N * 4); ALLOC(cGR, NW * N * cfn::SZ_K);
    ALLOC(cS, NW * N * cfn::SZ_S4); ALLOC(crho, NW * 4 * N * 4);
    if (P.fused == 1) ALLOC(cbv, NW * N * cfn::SZ_V13);
    ALLOC(cPs, NW * 32 * cfn::SZ_PA);
    ALLOC(status, NW * 4); ALLOC(iters, NW * 4); ALLOC(head, NW * 4); ALLOC(res, NW * 4); ALLOC(viol, NW * 4);
    ALLOC(ilist, NW * 4); ALLOC(ilist2, NW * 4); ALLOC(nipm, 64);
    ALLOC(blkcnt, ((size_t)(batch + 63) / 64) * cfn::BIN_STRIDE); ALLOC(rank, NW * 4); ALLOC(done, NW * 4);
    ALLOC(ascnt, 32); ALLOC(askst, NW * 4); ALLOC(asst, NW * 4); ALLOC(asok, NW * 4);
    ALLOC(czdx, NW * 4 * (N + 1) * 13);
    if (P.as_warm) { ALLOC(wcls, NW * 4 * N * 4); ALLOC(wvalid, NW * 4); }
    if (P.fwd_split) { ALLOC(fs_dx, ((size_t)(batch + 63) / 64) * 13 * 64); ALLOC(fs_st, ((size_t)(batch + 63) / 64) * 4 * 64); }
    if (P.as_passes != 0) ALLOC(aslist, (size_t)3 * 7 * NW * 4);
    if (P.cond_N2) ALLOC(cb, NW * 4 * (size_t)P.cond_N2 * cfn::cb_size(cfn::cond_mmax(P)));
    // full SQP solve (cfnmpc_solve_sqp): residuals, status, sqp_iter, done flags, the two counters of open rows
    if (rc == CFNMPC_OK) rc = dev_alloc(s, &s->sqp.res, (size_t)batch * 3);
    if (rc == CFNMPC_OK) rc = dev_alloc(s, &s->sqp.status, (size_t)batch);
    if (rc == CFNMPC_OK) rc = dev_alloc(s, &s->sqp.iter, (size_t)batch);
    if (rc == CFNMPC_OK) rc = dev_alloc(s, &s->sqp.done, (size_t)batch);
    if (rc == CFNMPC_OK) rc = dev_alloc(s, &s->sqp.cnt, 2);
    // NLP evaluation (cfnmpc_eval_nlp): cost and the three residuals
    if (rc == CFNMPC_OK) rc = dev_alloc(s, &s->nlp.cost, (size_t)batch);
    if (rc == CFNMPC_OK) rc = dev_alloc(s, &s->nlp.res, (size_t)batch * 3);
    if (s->overlap) {
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &s->AR2, NW16 * N * cfn::SZ_A);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &s->BR2, NW16 * N * cfn::SZ_B);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &s->b2, NW16 * N * cfn::SZ_V13);
        int lo = 0, hi = 0;  // lo = least priority (numerically greatest)
        if (rc == CFNMPC_OK && (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess ||
                                hipStreamCreateWithPriority(&s->aux, hipStreamNonBlocking, lo) != hipSuccess ||
                                hipEventCreateWithFlags(&s->ev_start, hipEventDisableTiming) != hipSuccess ||
                                hipEventCreateWithFlags(&s->ev_aux, hipEventDisableTiming) != hipSuccess))
            rc = CFNMPC_EHIP;
    }
#undef ALLOC
    s->stage_doubles = (size_t)batch * (N + 1) * 17;
    if (rc == CFNMPC_OK) rc = dev_alloc(s, &s->stage_buf, s->stage_doubles);
    if (rc != CFNMPC_OK) { cfnmpc_free(s); return rc; }
    // default iterate = what acados_create() leaves behind
    cfn::launch_init_iterate(P, CFNMPC_INIT_ACADOS, nullptr);
    if (hipDeviceSynchronize() != hipSuccess) { cfnmpc_free(s); return CFNMPC_EHIP; }
    *out = s;
    return CFNMPC_OK;
}

int cfnmpc_free(cfnmpc_solver* s) {
    if (!s) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    if (s->aux) { (void)hipStreamSynchronize(s->aux); (void)hipStreamDestroy(s->aux); }
    if (s->P.as_side2) {
        (void)hipStreamSynchronize((hipStream_t)s->P.as_side2);
        (void)hipStreamDestroy((hipStream_t)s->P.as_side2);
        (void)hipEventDestroy((hipEvent_t)s->P.as_join2);
    }
    if (s->P.as_side) {
        (void)hipStreamSynchronize((hipStream_t)s->P.as_side);
        (void)hipStreamDestroy((hipStream_t)s->P.as_side);
        (void)hipEventDestroy((hipEvent_t)s->P.as_fork);
        (void)hipEventDestroy((hipEvent_t)s->P.as_join);
    }
    for (int p = 0; p < 2; p++) {
        if (s->glaunched[p]) { (void)hipEventSynchronize(s->glaunched[p]); (void)hipEventDestroy(s->glaunched[p]); }
        if (s->gexec[p]) (void)hipGraphExecDestroy(s->gexec[p]);
    }
    if (s->cap) (void)hipStreamDestroy(s->cap);
    if (s->ev_start) (void)hipEventDestroy(s->ev_start);
    if (s->ev_aux) (void)hipEventDestroy(s->ev_aux);
    if (s->sqp_ev) (void)hipEventDestroy(s->sqp_ev);
    if (s->yuni_ev) { (void)hipEventSynchronize(s->yuni_ev); (void)hipEventDestroy(s->yuni_ev); }
    if (s->h_yvaries) (void)hipHostFree(s->h_yvaries);
    for (void* p : s->allocs) (void)hipFree(p);
    if (s->h_io) (void)hipHostFree(s->h_io);
    if (s->h_sqp_cnt) (void)hipHostFree(s->h_sqp_cnt);
    for (hipEvent_t e : s->ev) (void)hipEventDestroy(e);
    delete s;
    return CFNMPC_OK;
}

int cfnmpc_batch(const cfnmpc_solver* s) { return s ? s->P.B : CFNMPC_EINVAL; }
int cfnmpc_horizon(const cfnmpc_solver* s) { return s ? s->P.N : CFNMPC_EINVAL; }
unsigned long long cfnmpc_workspace_bytes(const cfnmpc_solver* s) { return s ? s->bytes : 0ull; }

int cfnmpc_set_x0(cfnmpc_solver* s, const double* x0, int on_device, void* stream) {
    if (!s || !x0) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    s->unc.inputs_moved = true;   // (cfnmpc_eval_uncertainty: the data of the next QP, no longer the last one's)
    return put_field(s, x0, on_device, 1, 13, 1, s->P.x0, (hipStream_t)stream);
}

// kernel arguments or the choice of a kernel changed (weights, box, Params.yuni): the captured steps hold the old ones
static void invalidate_graphs(cfnmpc_solver* s) { s->gvalid[0] = s->gvalid[1] = false; }

// ---- stage-invariant references (Params.yuni) ----------------------------------------------------------------------------------
static void set_yuni(cfnmpc_solver* s, int yuni) {
    s->yuni_pending = false;
    if (s->P.yuni != yuni) { s->P.yuni = yuni; invalidate_graphs(s); }
}
// a writer of P.yref other than cfnmpc_set_yref (windows, polynomial rows, cfnmpc_step_host): the rows vary, no detection
static void yref_rows_vary(cfnmpc_solver* s) { set_yuni(s, 0); }
// behind the k_put of cfnmpc_set_yref on `st`: does any instance's row k >= 1 differ from its row 0?  Nothing waits here.
static int detect_yuni(cfnmpc_solver* s, hipStream_t st) {
    if (!s->yvaries) RC_TRY(dev_alloc(s, &s->yvaries, 1));
    if (!s->h_yvaries) HIP_TRY(hipHostMalloc((void**)&s->h_yvaries, sizeof(int), hipHostMallocDefault));
    if (!s->yuni_ev) HIP_TRY(hipEventCreateWithFlags(&s->yuni_ev, hipEventDisableTiming));
    HIP_TRY(hipMemsetAsync(s->yvaries, 0, sizeof(int), st));
    cfn::launch_yref_uniform(s->P, s->yvaries, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(s->h_yvaries, s->yvaries, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(s->yuni_ev, st));
    s->yuni_pending = true;
    return CFNMPC_OK;
}
// in front of whatever launches the start solve's factorisation: the one wait for a verdict on its way (none per step)
static int resolve_yuni(cfnmpc_solver* s) {
    if (!s->yuni_pending) return CFNMPC_OK;
    HIP_TRY(hipEventSynchronize(s->yuni_ev));
    set_yuni(s, *s->h_yvaries ? 0 : 1);
    return CFNMPC_OK;
}

int cfnmpc_set_yref(cfnmpc_solver* s, const double* yref, const double* yref_e, int on_device, void* stream) {
    if (!s || !yref || !yref_e) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    s->unc.inputs_moved = true;
    int rc = put_field(s, yref, on_device, s->P.N, 17, 1, s->P.yref, (hipStream_t)stream);
    if (rc != CFNMPC_OK) return rc;
    // (the flag in force stays until the verdict is read: a caller that sends stage-invariant rows every step keeps its captured graphs)
    rc = detect_yuni(s, (hipStream_t)stream);
    if (rc != CFNMPC_OK) { yref_rows_vary(s); return rc; }
    return put_field(s, yref_e, on_device, 1, 13, 1, s->P.yref_e, (hipStream_t)stream);
}

int cfnmpc_set_yref_windows(cfnmpc_solver* s, const double* traj, int n_rows, int* mode, int* iter,
                            const double* des_xyz, double uss, void* stream) {
    if (!s || !mode || !iter || !des_xyz) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    if (n_rows > 0 && (!traj || n_rows < s->P.N + 1)) return CFNMPC_EINVAL;
    if (n_rows <= 0 && traj) return CFNMPC_EINVAL;
    s->unc.inputs_moved = true;
    yref_rows_vary(s);
    cfn::launch_windows(s->P, traj, n_rows > 0 ? n_rows : 0, mode, iter, des_xyz, uss, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return CFNMPC_OK;
}

int cfnmpc_get_yref(cfnmpc_solver* s, double* yref, double* yref_e, int on_device, void* stream) {
    if (!s || (!yref && !yref_e)) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    hipStream_t st = (hipStream_t)stream;
    // (two arrays through one staging buffer: the second layout kernel is ordered behind the first copy on the stream)
    if (yref) RC_TRY(get_field(s, yref, is_host(on_device) && yref_e ? (int)CFNMPC_ON_HOST_ASYNC : on_device, s->P.N, 17, 1, 0, s->P.N, s->P.yref, st));
    if (yref_e) RC_TRY(get_field(s, yref_e, on_device, 1, 13, 1, 0, 1, s->P.yref_e, st));
    return CFNMPC_OK;
}

// ---- device-side polynomial trajectory references ----------------------------------------------------
static_assert(CFNMPC_POLY_NC == 33 && CFNMPC_NPLACE == 6 && CFNMPC_NFLAT == 13, "polynomial reference rows");
// the tables, the assignment (-1 everywhere) and the placement rows, allocated together at the first call of the feature
static int ensure_poly(cfnmpc_solver* s) {
    if (s->poly.traj) return CFNMPC_OK;
    const size_t B = s->P.B;
    RC_TRY(dev_alloc(s, &s->poly.pieces, (size_t)CFNMPC_POLY_MAX_PIECES * CFNMPC_POLY_NC));
    RC_TRY(dev_alloc(s, &s->poly.first, (size_t)CFNMPC_POLY_MAX_TRAJ + 1));
    RC_TRY(dev_alloc(s, &s->poly.place, B * CFNMPC_NPLACE));
    int* t = nullptr;
    RC_TRY(dev_alloc(s, &t, B));
    HIP_TRY(hipMemset(t, 0xff, B * sizeof(int)));   // (-1)
    HIP_TRY(hipStreamSynchronize(nullptr));          // (as in dev_alloc: the fill is complete before a stream writes)
    s->poly.traj = t;
    return CFNMPC_OK;
}
static cfn::PolyArgs poly_args(const cfnmpc_solver* s, double t, int flags) {
    cfn::PolyArgs A{};
    A.pieces = s->poly.pieces; A.first = s->poly.first; A.n_traj = s->poly.n_traj;
    A.traj = s->poly.traj; A.place = s->poly.has_place ? s->poly.place : nullptr;
    A.t = t; A.flags = flags;
    return A;
}

int cfnmpc_set_poly_library(cfnmpc_solver* s, const double* pieces, const int* first, int n_traj, void* stream) {
    if (!s || n_traj < 0) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    hipStream_t st = (hipStream_t)stream;
    if (n_traj == 0 || !pieces || !first) {   // clears the library: every vehicle is without a trajectory
        s->poly.n_traj = 0;
        if (s->poly.traj) { cfn::launch_poly_clamp_ids(s->P.B, 0, s->poly.traj, st); HIP_TRY(hipGetLastError()); }
        return CFNMPC_OK;
    }
    if (!cfn::poly_library_ok(pieces, first, n_traj)) return CFNMPC_EINVAL;
    RC_TRY(ensure_poly(s));
    HIP_TRY(hipMemcpyAsync(s->poly.pieces, pieces, (size_t)first[n_traj] * CFNMPC_POLY_NC * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->poly.first, first, ((size_t)n_traj + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    cfn::launch_poly_clamp_ids(s->P.B, n_traj, s->poly.traj, st);   // (a smaller library: ids it no longer has -> -1)
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // (the caller's arrays may be temporaries)
    s->poly.n_traj = n_traj;
    return CFNMPC_OK;
}

int cfnmpc_set_poly_assignment(cfnmpc_solver* s, const int* traj, const double* place, int on_device, void* stream) {
    if (!s || !traj) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    hipStream_t st = (hipStream_t)stream;
    const size_t B = s->P.B;
    const bool host = is_host(on_device);
    if (host && !cfn::poly_assignment_ok(traj, place, B, s->poly.n_traj)) return CFNMPC_EINVAL;
    RC_TRY(ensure_poly(s));
    const hipMemcpyKind kind = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    HIP_TRY(hipMemcpyAsync(s->poly.traj, traj, B * sizeof(int), kind, st));
    if (place) HIP_TRY(hipMemcpyAsync(s->poly.place, place, B * CFNMPC_NPLACE * sizeof(double), kind, st));
    s->poly.has_place = place != nullptr;
    if (on_device == CFNMPC_ON_HOST) HIP_TRY(hipStreamSynchronize(st));
    return CFNMPC_OK;
}

int cfnmpc_set_yref_poly(cfnmpc_solver* s, double t, int flags, void* stream) {
    if (!s || s->poly.n_traj == 0 || !std::isfinite(t) || (flags & ~(CFNMPC_POLY_LOOP | CFNMPC_POLY_KINEMATIC))) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    s->unc.inputs_moved = true;
    yref_rows_vary(s);
    cfn::launch_poly_rows(s->P, poly_args(s, t, flags), (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return CFNMPC_OK;
}

int cfnmpc_eval_poly(cfnmpc_solver* s, double t, int n_stages, int flags, double* flat, double* rows, int on_device, void* stream) {
    if (!s || s->poly.n_traj == 0 || !std::isfinite(t) || (flags & ~(CFNMPC_POLY_LOOP | CFNMPC_POLY_KINEMATIC)) || n_stages < 1 ||
        n_stages > (1 << 20) || (!flat && !rows))
        return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    hipStream_t st = (hipStream_t)stream;
    cfn::PolyArgs A = poly_args(s, t, flags);
    A.ns = n_stages;
    const size_t B = s->P.B, nf = flat ? (size_t)n_stages * CFNMPC_NFLAT : 0, nr = rows ? (size_t)n_stages * 17 : 0;
    if (!is_host(on_device)) {
        A.flat = flat; A.rows = rows; A.b0 = 0; A.nb = (int)B;
        cfn::launch_poly_eval(s->P, A, st);
        HIP_TRY(hipGetLastError());
        return CFNMPC_OK;
    }
    // host arrays: rows in chunks through the staging buffer (host_row_chunks)
    RC_TRY(host_row_chunks(s, nf + nr, [&](size_t b0, size_t nb, double* stage) {
        A.b0 = (int)b0; A.nb = (int)nb;
        A.flat = flat ? stage : nullptr;
        A.rows = rows ? stage + nb * nf : nullptr;
        cfn::launch_poly_eval(s->P, A, st);
        HIP_TRY(hipGetLastError());
        if (flat) HIP_TRY(hipMemcpyAsync(flat + b0 * nf, A.flat, nb * nf * sizeof(double), hipMemcpyDeviceToHost, st));
        if (rows) HIP_TRY(hipMemcpyAsync(rows + b0 * nr, A.rows, nb * nr * sizeof(double), hipMemcpyDeviceToHost, st));
        return (int)CFNMPC_OK;
    }));
    if (on_device == CFNMPC_ON_HOST) HIP_TRY(hipStreamSynchronize(st));
    return CFNMPC_OK;
}

// the QP's data changed since the last solve: no sensitivities until the next one
static void invalidate_sens(cfnmpc_solver* s) { s->sens_src = 0; s->sens_valid = false; s->adj_valid = false; s->unc.current = false; }

// The four blocks of the per-stage boxes (home lb / ub, compact lb / ub; cfnmpc_set_box_stages, cfnmpc_tighten_box).
static int ensure_box_blocks(cfnmpc_solver* s) {
    cfn::Params& P = s->P;
    if (s->lbs_keep && P.clbs && P.cubs) return CFNMPC_OK;
    // allocated and initialised as a whole before any pointer is committed: a failure half-way (ENOMEM, a failed copy)
    // leaves the solver on the scalar box with nothing dangling (the blocks stay owned by s->allocs until cfnmpc_free)
    const size_t cnt = ((size_t)P.NW + 1) * 4 * P.N * 4;
    // (blocks a failed earlier attempt did get are kept in s->box_blk and reused: a retry allocates only what is missing)
    int rc = CFNMPC_OK;
    for (int q = 0; q < 4 && rc == CFNMPC_OK; q++)
        if (!s->box_blk[q]) rc = dev_alloc(s, &s->box_blk[q], cnt);
    if (rc != CFNMPC_OK) return rc;
    double *lk = s->box_blk[0], *uk = s->box_blk[1], *cl = s->box_blk[2], *cu = s->box_blk[3];
    // rows of the spare block (parked rows of compacted waves): a wide finite box
    std::vector<double> lo(4 * (size_t)P.N * 4, -1e30), hi(4 * (size_t)P.N * 4, 1e30);
    HIP_TRY(hipMemcpy(lk + (size_t)P.NW * 4 * P.N * 4, lo.data(), lo.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(uk + (size_t)P.NW * 4 * P.N * 4, hi.data(), hi.size() * 8, hipMemcpyHostToDevice));
    s->lbs_keep = lk; s->ubs_keep = uk; P.clbs = cl; P.cubs = cu;
    return CFNMPC_OK;
}

// A tightened box in force (cfnmpc_tighten_box) gives way to the nominal one, on `st`: per-stage nominal arrays are copied back
// in place (captured step graphs keep replaying), a scalar nominal box switches the route back (and invalidates them).
static int untighten(cfnmpc_solver* s, hipStream_t st) {
    cfn::Params& P = s->P;
    if (!s->unc.tight) return CFNMPC_OK;
    if (s->unc.nom_stages) {
        const size_t bytes = (size_t)P.NW * 4 * P.N * 4 * sizeof(double);
        HIP_TRY(hipMemcpyAsync(P.lbs, s->unc.nom_lb, bytes, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(P.ubs, s->unc.nom_ub, bytes, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(P.clbs, s->unc.nom_lb, bytes, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(P.cubs, s->unc.nom_ub, bytes, hipMemcpyDeviceToDevice, st));
    } else {
        if (P.lbs) { s->lbs_keep = P.lbs; s->ubs_keep = P.ubs; }
        P.lbs = P.ubs = nullptr;
        invalidate_graphs(s);
    }
    s->unc.tight = false;
    invalidate_sens(s);
    return CFNMPC_OK;
}

// Per-instance weight table (Params.wtab, layout: cfnmpc_ws.hpp) from the rows in force, scaling applied: uploaded in place on
// `st` and complete on return, so that a captured step graph (which holds the pointer) replays with the new values.
static int upload_weight_rows(cfnmpc_solver* s, hipStream_t st) {
    const cfn::Params& P = s->P;
    const size_t B = P.B, S = ((size_t)P.NW + 1) * 4;
    std::vector<double> tab(S * 32, 0.0);
    for (size_t i = 0; i < S; i++) {   // (padding rows and the spare block: the uniform weights)
        const double* w = i < B ? s->w_rows.data() + i * 17 : s->W_set;
        const double* wn = i < B ? s->wn_rows.data() + i * 13 : s->WN_set;
        double* r = tab.data() + i * 32;
        for (int j = 0; j < 13; j++) r[j] = s->stage_scale * w[cfn::ext_of(j)];
        for (int c = 0; c < 4; c++) r[13 + c] = s->stage_scale * w[13 + c];
        for (int j = 0; j < 13; j++) r[17 + j] = s->terminal_scale * wn[cfn::ext_of(j)];
    }
    HIP_TRY(hipMemcpyAsync(s->wtab_buf, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CFNMPC_OK;
}

int cfnmpc_set_weights(cfnmpc_solver* s, const double* W, const double* WN) {
    if (!s || (!W && !WN)) return CFNMPC_EINVAL;
    if (!weights_ok(W, WN)) return CFNMPC_EINVAL;   // validated as a whole before anything is copied
    // rows in force: what goes into every row obeys the rows' own rule (finite; weights_ok lets +inf through)
    if (s->P.wtab && !cfn::weight_rows_ok(W, WN, 1)) return CFNMPC_EINVAL;
    if (W) for (int i = 0; i < 17; i++) s->P.W[i] = s->stage_scale * (s->W_set[i] = W[i]);
    if (WN) for (int i = 0; i < 13; i++) s->P.WN[i] = s->terminal_scale * (s->WN_set[i] = WN[i]);
    invalidate_graphs(s);
    invalidate_sens(s);
    if (s->P.wtab) {   // "for all instances": each part given replaces that part in every row
        DeviceGuard dg(s->device);
        for (size_t i = 0; i < (size_t)s->P.B; i++) {
            if (W) std::copy_n(W, 17, s->w_rows.data() + i * 17);
            if (WN) std::copy_n(WN, 13, s->wn_rows.data() + i * 13);
        }
        return upload_weight_rows(s, nullptr);
    }
    return CFNMPC_OK;  // kernel arguments: take effect at the next cfnmpc_solve
}

int cfnmpc_set_weights_batch(cfnmpc_solver* s, const double* W, const double* WN, int on_device, void* stream) {
    if (!s) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    cfn::Params& P = s->P;
    // not covered: the fused start solve (k_linfactor's weight table is shared by the four rows of a wavefront), partial
    // condensing (one weight vector per workgroup), the development build's overlapped preparation
    if (P.fused || P.cond_N2 || s->overlap) return CFNMPC_EINVAL;
    if (!W && !WN) {   // back to the uniform weights (the kernel arguments)
        if (P.wtab) { P.wtab = nullptr; invalidate_graphs(s); }
        s->w_rows.clear(); s->wn_rows.clear();
        invalidate_sens(s);
        return CFNMPC_OK;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t B = P.B;
    std::vector<double> w, wn;
    if (W) w.resize(B * 17);
    if (WN) wn.resize(B * 13);
    if (is_host(on_device)) {
        if (W) std::copy_n(W, w.size(), w.data());
        if (WN) std::copy_n(WN, wn.size(), wn.data());
    } else {   // device rows: one copy to the host to validate them
        if (W) HIP_TRY(hipMemcpyAsync(w.data(), W, w.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        if (WN) HIP_TRY(hipMemcpyAsync(wn.data(), WN, wn.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (!cfn::weight_rows_ok(W ? w.data() : nullptr, WN ? wn.data() : nullptr, B)) return CFNMPC_EINVAL;
    if (!s->wtab_buf) {
        const int rc = dev_alloc(s, &s->wtab_buf, ((size_t)P.NW + 1) * 4 * 32);
        if (rc != CFNMPC_OK) return rc;
    }
    // a part not given keeps what every row has (the uniform values if no rows were set)
    const bool had = !s->w_rows.empty();
    std::vector<double> w_old = s->w_rows, wn_old = s->wn_rows;
    if (!W && !had) { w.resize(B * 17); for (size_t i = 0; i < B; i++) std::copy_n(s->W_set, 17, w.data() + i * 17); }
    if (!WN && !had) { wn.resize(B * 13); for (size_t i = 0; i < B; i++) std::copy_n(s->WN_set, 13, wn.data() + i * 13); }
    if (W || !had) s->w_rows = std::move(w);
    if (WN || !had) s->wn_rows = std::move(wn);
    const int rc = upload_weight_rows(s, st);
    if (rc != CFNMPC_OK) {   // (nothing in force changes: the kernels keep reading what they read before)
        s->w_rows = std::move(w_old); s->wn_rows = std::move(wn_old);
        return rc;
    }
    if (!P.wtab) { P.wtab = s->wtab_buf; invalidate_graphs(s); }   // other kernels from here on
    invalidate_sens(s);
    return CFNMPC_OK;
}

int cfnmpc_get_weights_batch(cfnmpc_solver* s, double* W, double* WN, int on_device, void* stream) {
    if (!s || (!W && !WN)) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    const size_t B = s->P.B;
    std::vector<double> w = s->w_rows, wn = s->wn_rows;
    if (w.empty()) {
        w.resize(B * 17); wn.resize(B * 13);
        for (size_t i = 0; i < B; i++) { std::copy_n(s->W_set, 17, w.data() + i * 17); std::copy_n(s->WN_set, 13, wn.data() + i * 13); }
    }
    if (is_host(on_device)) {
        if (W) std::copy_n(w.data(), w.size(), W);
        if (WN) std::copy_n(wn.data(), wn.size(), WN);
        return CFNMPC_OK;
    }
    hipStream_t st = (hipStream_t)stream;
    if (W) HIP_TRY(hipMemcpyAsync(W, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice, st));
    if (WN) HIP_TRY(hipMemcpyAsync(WN, wn.data(), wn.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // (the sources are host temporaries)
    return CFNMPC_OK;
}

int cfnmpc_set_cost_scaling(cfnmpc_solver* s, double stage_scale, double terminal_scale) {
    if (!s || !(std::isfinite(stage_scale) && stage_scale > 0) || !(std::isfinite(terminal_scale) && terminal_scale > 0))
        return CFNMPC_EINVAL;
    s->stage_scale = stage_scale;
    invalidate_sens(s);
    s->terminal_scale = terminal_scale;
    for (int i = 0; i < 17; i++) s->P.W[i] = stage_scale * s->W_set[i];
    for (int i = 0; i < 13; i++) s->P.WN[i] = terminal_scale * s->WN_set[i];
    invalidate_graphs(s);
    if (s->P.wtab) {   // rescales the rows in force
        DeviceGuard dg(s->device);
        return upload_weight_rows(s, nullptr);
    }
    return CFNMPC_OK;
}

int cfnmpc_set_erk_steps(cfnmpc_solver* s, int num_steps) {
    if (!s || num_steps < 1 || num_steps > CFNMPC_ERK_STEPS_MAX) return CFNMPC_EINVAL;
    // the fused start solve (k_linfactor, k_linearise_clist) integrates one step per interval; the development build's
    // overlapped preparation (k_linearise_list) likewise
    if (num_steps > 1 && (s->P.fused || s->overlap)) return CFNMPC_EINVAL;
    s->P.erk_steps = num_steps;
    invalidate_sens(s);
    s->lin_valid = false;
    invalidate_graphs(s);
    return CFNMPC_OK;
}

int cfnmpc_erk_steps(const cfnmpc_solver* s) { return s ? s->P.erk_steps : CFNMPC_EINVAL; }

static_assert(CFNMPC_NP == cfn::NPAR, "parameter row");
static_assert(CFNMPC_ND == cfn::ND, "disturbance row");
// the table of derived constants (s->mpar_buf, allocated here at first use) from the rows [B][NPAR], NULL = nominal rows:
// [NK][S] structure-of-arrays over every workspace row (padding rows and the spare block: nominal).  In place, in stream order,
// complete on return: a captured step graph (which holds the pointer) replays with the new values
static int upload_mpar(cfnmpc_solver* s, const double* rows, hipStream_t st) {
    const cfn::Params& P = s->P;
    const size_t B = P.B, S = ((size_t)P.NW + 1) * 4;
    std::vector<double> k((size_t)cfn::NK * S);
    for (size_t i = 0; i < S; i++) {
        double ki[cfn::NK];
        cfn::derive_k(rows && i < B ? rows + i * cfn::NPAR : cfn::NOM_P, ki);
        for (int j = 0; j < cfn::NK; j++) k[(size_t)j * S + i] = ki[j];
    }
    if (!s->mpar_buf) RC_TRY(dev_alloc(s, &s->mpar_buf, k.size()));
    HIP_TRY(hipMemcpyAsync(s->mpar_buf, k.data(), k.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CFNMPC_OK;
}
int cfnmpc_set_model_params(cfnmpc_solver* s, const double* p, int on_device, void* stream) {
    if (!s) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    cfn::Params& P = s->P;
    if (!p) {   // back to the folded constants (the default kernels)
        if (P.dist) {   // (the _dst kernels stay: they read the constants from the table, nominal rows from here on)
            if (!s->mp_rows.empty()) RC_TRY(upload_mpar(s, nullptr, (hipStream_t)stream));
            s->lin_valid = false;
        } else if (P.mpar) { P.mpar = nullptr; s->lin_valid = false; invalidate_graphs(s); }
        s->mp_rows.clear();
        invalidate_sens(s);
        return CFNMPC_OK;
    }
    // the fused start solve (k_linfactor, k_linearise_clist) and the development build's overlapped preparation
    // (k_linearise_list) integrate with the folded constants
    if (P.fused || s->overlap) return CFNMPC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const size_t B = P.B, n = B * cfn::NPAR;
    std::vector<double> rows(n);
    if (is_host(on_device)) {
        std::copy_n(p, n, rows.data());
    } else {   // device rows: one copy to the host to validate them
        HIP_TRY(hipMemcpyAsync(rows.data(), p, n * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (!cfn::model_params_ok(rows.data(), n)) return CFNMPC_EINVAL;
    RC_TRY(upload_mpar(s, rows.data(), st));
    if (!P.mpar) { P.mpar = s->mpar_buf; invalidate_graphs(s); }   // other kernels from here on
    s->lin_valid = false;
    s->mp_rows = std::move(rows);
    invalidate_sens(s);
    return CFNMPC_OK;
}

int cfnmpc_get_model_params(cfnmpc_solver* s, double* p, int on_device, void* stream) {
    if (!s || !p) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    const size_t B = s->P.B, n = B * cfn::NPAR;
    std::vector<double> nom;
    const double* src = s->mp_rows.data();
    if (s->mp_rows.empty()) {
        nom.resize(n);
        for (size_t i = 0; i < B; i++) std::copy_n(cfn::NOM_P, cfn::NPAR, nom.data() + i * cfn::NPAR);
        src = nom.data();
    }
    if (is_host(on_device)) { std::copy_n(src, n, p); return CFNMPC_OK; }
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(p, src, n * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // (src is a host temporary)
    return CFNMPC_OK;
}

int cfnmpc_set_disturbance(cfnmpc_solver* s, const double* d, int on_device, void* stream) {
    if (!s) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    cfn::Params& P = s->P;
    hipStream_t st = (hipStream_t)stream;
    if (!d) {   // back to the kernels in force before: _par while parameter rows are set, else the folded ones
        if (P.dist) {
            P.dist = nullptr;
            if (s->mp_rows.empty()) P.mpar = nullptr;
            s->lin_valid = false;
            invalidate_graphs(s);
        }
        invalidate_sens(s);
        return CFNMPC_OK;
    }
    // the fused start solve, the partial-condensing sweep and the development build's overlapped preparation have no _dst twins
    if (P.fused || P.cond_N2 || s->overlap) return CFNMPC_EINVAL;
    const size_t B = P.B, n = B * cfn::ND, S = ((size_t)P.NW + 1) * 4;
    const bool host = is_host(on_device);
    if (host && (!cfn::dist_rows_ok(d, n) || n > s->stage_doubles)) return CFNMPC_EINVAL;
    if (!s->dist_buf) RC_TRY(dev_alloc(s, &s->dist_buf, (size_t)cfn::ND * S));   // (zero: padding rows and the spare block stay so)
    if (!P.mpar && s->mp_rows.empty()) RC_TRY(upload_mpar(s, nullptr, st));      // (first rows without parameter rows: nominal table)
    // rows -> table in place, in stream order: no copy to the host, no synchronisation for a device array; a captured step graph
    // (which holds the pointer) replays with the new values
    const double* src = d;
    if (host) {
        HIP_TRY(hipMemcpyAsync(s->stage_buf, d, n * sizeof(double), hipMemcpyHostToDevice, st));
        src = s->stage_buf;
    }
    cfn::launch_dist_put((int)B, (int)S, src, s->dist_buf, st);
    HIP_TRY(hipGetLastError());
    if (on_device == CFNMPC_ON_HOST) HIP_TRY(hipStreamSynchronize(st));   // (the staging buffer is reused)
    if (!P.dist) { P.dist = s->dist_buf; P.mpar = s->mpar_buf; invalidate_graphs(s); }   // other kernels from here on
    s->lin_valid = false;
    invalidate_sens(s);
    return CFNMPC_OK;
}

int cfnmpc_get_disturbance(cfnmpc_solver* s, double* d, int on_device, void* stream) {
    if (!s || !d) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    const cfn::Params& P = s->P;
    hipStream_t st = (hipStream_t)stream;
    const size_t B = P.B, n = B * cfn::ND, S = ((size_t)P.NW + 1) * 4;
    const bool host = is_host(on_device);
    if (!P.dist) {   // none set: zero rows
        if (host) std::fill_n(d, n, 0.0);
        else HIP_TRY(hipMemsetAsync(d, 0, n * sizeof(double), st));
        return CFNMPC_OK;
    }
    if (host && n > s->stage_doubles) return CFNMPC_EINVAL;
    cfn::launch_dist_get((int)B, (int)S, P.dist, host ? s->stage_buf : d, st);
    HIP_TRY(hipGetLastError());
    if (host) {
        HIP_TRY(hipMemcpyAsync(d, s->stage_buf, n * sizeof(double), hipMemcpyDeviceToHost, st));
        if (on_device == CFNMPC_ON_HOST) HIP_TRY(hipStreamSynchronize(st));
    }
    return CFNMPC_OK;
}

int cfnmpc_set_box(cfnmpc_solver* s, double u_min, double u_max) {
    if (!s || !(u_max > u_min)) return CFNMPC_EINVAL;
    if (s->unc.tight) {   // a tightened box in force: the nominal one comes back (cfnmpc_tighten_box)
        // (no stream argument here: a tightening or a solve enqueued on a non-blocking stream -- fleet buckets, multi shards --
        //  is not ordered before the null stream; wait for the device, then restore and complete)
        DeviceGuard dg(s->device);
        HIP_TRY(hipDeviceSynchronize());
        RC_TRY(untighten(s, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    s->P.u_min = u_min;   // kernel arguments: take effect at the next cfnmpc_solve
    s->P.u_max = u_max;
    invalidate_sens(s);
    invalidate_graphs(s);
    return CFNMPC_OK;
}

int cfnmpc_set_box_stages(cfnmpc_solver* s, const double* lb, const double* ub, int on_device, void* stream) {
    if (!s || ((lb == nullptr) != (ub == nullptr))) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    cfn::Params& P = s->P;
    if (!lb) {                       // back to the scalar box of cfnmpc_set_box
        if (P.lbs) { s->lbs_keep = P.lbs; s->ubs_keep = P.ubs; }
        P.lbs = P.ubs = nullptr;
        s->unc.tight = false;        // (a tightened box goes with it: the scalar box is the nominal one from here on)
        invalidate_graphs(s);
        invalidate_sens(s);
        return CFNMPC_OK;
    }
    if (P.cond_N2) return CFNMPC_EINVAL;   // the condensed path has no per-stage boxes
    const size_t n = (size_t)P.B * P.N * 4;
    // host arrays are validated here (NaN fails too; lb = ub pins the input); DEVICE arrays are taken as they are -- a caller
    // that hands over device pointers is responsible for lb <= ub (an inverted box ends in status 4 for that vehicle)
    if (is_host(on_device))
        for (size_t i = 0; i < n; i++) if (!(lb[i] <= ub[i])) return CFNMPC_EINVAL;
    invalidate_sens(s);
    RC_TRY(ensure_box_blocks(s));
    // the caller's AoS order [inst][stage][4] -> the layout of the home 4-vectors (Params.v4b).  Both arrays are STAGED first
    // (in the compact box buffers: scratch of the QP kernels, rewritten by every solve that uses them) and the home pair is
    // overwritten only after both puts succeeded -- a failure leaves the previous lb AND ub in force, never a mixed box.
    hipStream_t st = (hipStream_t)stream;
    int rcp = put_field(s, lb, on_device, P.N, 4, 0, P.clbs, st);
    if (rcp == CFNMPC_OK) rcp = put_field(s, ub, on_device, P.N, 4, 0, P.cubs, st);
    if (rcp != CFNMPC_OK) return rcp;
    const size_t bytes = (size_t)P.NW * 4 * P.N * 4 * sizeof(double);   // (the spare block behind it keeps its wide box)
    HIP_TRY(hipMemcpyAsync(s->lbs_keep, P.clbs, bytes, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->ubs_keep, P.cubs, bytes, hipMemcpyDeviceToDevice, st));
    if (on_device == CFNMPC_ON_HOST) HIP_TRY(hipStreamSynchronize(st));   // synchronous form: complete when the call returns
    P.lbs = s->lbs_keep; P.ubs = s->ubs_keep;
    s->unc.tight = false;   // (the new arrays are the nominal box; a tightened one they replaced is gone)
    invalidate_graphs(s);
    return CFNMPC_OK;
}

int cfnmpc_get_cmd(cfnmpc_solver* s, double* cmd_vel, int* motvel, int on_device, void* stream) {
    if (!s || !cmd_vel) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    hipStream_t st = (hipStream_t)stream;
    const size_t B = s->P.B;
    if (!is_host(on_device)) {
        cfn::launch_postproc(s->P, cmd_vel, motvel, st);
        HIP_TRY(hipGetLastError());
        return CFNMPC_OK;
    }
    // host pointers: through the staging buffer ([B][4] doubles, then [B][4] ints)
    if (B * 6 > s->stage_doubles) return CFNMPC_EINVAL;
    double* dc = s->stage_buf;
    int* dm = (int*)(s->stage_buf + B * 4);
    cfn::launch_postproc(s->P, dc, dm, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cmd_vel, dc, B * 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (motvel) HIP_TRY(hipMemcpyAsync(motvel, dm, B * 4 * sizeof(int), hipMemcpyDeviceToHost, st));
    if (on_device == CFNMPC_ON_HOST) HIP_TRY(hipStreamSynchronize(st));
    return CFNMPC_OK;
}

int cfnmpc_init_iterate(cfnmpc_solver* s, int mode, void* stream) {
    if (!s || (mode != CFNMPC_INIT_ACADOS && mode != CFNMPC_INIT_HOVER)) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    cfn::launch_init_iterate(s->P, mode, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    if (s->P.as_warm) HIP_TRY(hipMemsetAsync(s->P.wvalid, 0, sizeof(int) * (size_t)s->P.B, (hipStream_t)stream));   // a new iterate: no set to start from
    s->lin_valid = false;
    invalidate_sens(s);
    s->unc.beta_valid = false;
    return CFNMPC_OK;
}

int cfnmpc_set_iterate(cfnmpc_solver* s, const double* x, const double* u, int on_device, void* stream) {
    if (!s || !x || !u) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    s->lin_valid = false;
    invalidate_sens(s);
    s->unc.beta_valid = false;
    if (s->P.as_warm) HIP_TRY(hipMemsetAsync(s->P.wvalid, 0, sizeof(int) * (size_t)s->P.B, (hipStream_t)stream));
    int rc = put_field(s, x, on_device, s->P.N + 1, 13, 1, s->P.xit, (hipStream_t)stream);
    if (rc != CFNMPC_OK) return rc;
    return put_field(s, u, on_device, s->P.N, 4, 0, s->P.uit, (hipStream_t)stream);
}

int cfnmpc_get_iterate(cfnmpc_solver* s, double* x, double* u, int on_device, void* stream) {
    if (!s || !x || !u) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    int rc = get_field(s, x, on_device, s->P.N + 1, 13, 1, 0, s->P.N + 1, s->P.xit, (hipStream_t)stream);
    if (rc != CFNMPC_OK) return rc;
    return get_field(s, u, on_device, s->P.N, 4, 0, 0, s->P.N, s->P.uit, (hipStream_t)stream);
}

}  // extern "C"

namespace {

// One RTI step (linearise -> QP -> full step) on `st`, the body of cfnmpc_solve's loop and one iteration of the full SQP solve.
// reinit: cfnmpc_opts.reinit_failed applies (cfnmpc_solve; not inside an SQP solve, whose failed rows stop instead).
// chk (may be NULL): the SQP solve's convergence check (in a globalised solve: the line search that contains it), launched
// behind the step's kernels and BEFORE the host swaps the iterate buffers (it reads both; the line search writes the new one);
// the launches of the step itself are the same with or without it.
// behind the step of an SQP iteration: the convergence check, or in a globalised solve the line search that contains it
void launch_sqp_close(cfnmpc_solver* s, const cfn::SqpArgs& chk, hipStream_t st) {
    if (s->ls_active) cfn::launch_sqp_ls(s->P, chk, s->ls, st);
    else cfn::launch_sqp_check(s->P, chk, st);
}

int rti_step(cfnmpc_solver* s, hipStream_t st, bool reinit, const cfn::SqpArgs* chk) {
    invalidate_sens(s);   // (until the step is through)
    s->unc.inputs_moved = false;
    RC_TRY(resolve_yuni(s));
    hipEvent_t* e = nullptr;
    if (s->profiling && s->ev_used < EV_PER_STEP * MAX_PROFILED_STEPS) {   // bounded: later steps go untimed
        while (s->ev.size() < s->ev_used + EV_PER_STEP) {
            hipEvent_t ne;
            HIP_TRY(hipEventCreate(&ne));
            s->ev.push_back(ne);
        }
        e = &s->ev[s->ev_used];
        s->ev_used += EV_PER_STEP;
    }
    if (reinit) { cfn::launch_reinit_failed(s->P, st); s->lin_valid = false; }
    if (!s->overlap && s->use_graph && !e) {
        // the step's launches replayed from a captured graph (one per parity of the iterate buffers)
        const int p = s->parity;
        bool ok = true;
        if (!s->gvalid[p]) {
            if (!s->cap) HIP_TRY(hipStreamCreateWithFlags(&s->cap, hipStreamNonBlocking));
            if (!s->glaunched[p]) HIP_TRY(hipEventCreateWithFlags(&s->glaunched[p], hipEventDisableTiming));
            if (s->gexec[p]) {   // a launch of the old exec may still be running (cfnmpc_solve is asynchronous)
                HIP_TRY(hipEventSynchronize(s->glaunched[p]));
                (void)hipGraphExecDestroy(s->gexec[p]);
                s->gexec[p] = nullptr;
            }
            hipGraph_t g = nullptr;
            ok = hipStreamBeginCapture(s->cap, hipStreamCaptureModeThreadLocal) == hipSuccess;
            if (ok) {
                if (s->P.fused != 1 || s->P.lbs) cfn::launch_linearise(s->P, s->chunks_all, s->cap);
                if (s->P.cond_N2) cfn::launch_qp_cond(s->P, s->cap);
                else cfn::launch_qp(s->P, s->cap);
                ok = hipStreamEndCapture(s->cap, &g) == hipSuccess && g != nullptr;   // (always ends the capture)
            }
            if (ok) ok = hipGraphInstantiate(&s->gexec[p], g, nullptr, nullptr, 0) == hipSuccess;
            if (g) (void)hipGraphDestroy(g);
            if (!ok) {
                // capture / instantiation failed: drop the capture stream (it may be left in an invalid capture
                // state) and fall back to individual launches for good -- this step runs on the plain path below
                (void)hipGetLastError();
                (void)hipStreamDestroy(s->cap);
                s->cap = nullptr;
                s->gexec[p] = nullptr;
                s->use_graph = 0;
                std::fprintf(stderr, "cfnmpc: step_graph capture failed, launching the step's kernels individually\n");
            } else {
                s->gvalid[p] = true;
            }
        }
        if (ok) {
            HIP_TRY(hipGraphLaunch(s->gexec[p], st));
            HIP_TRY(hipEventRecord(s->glaunched[p], st));
            if (chk) launch_sqp_close(s, *chk, st);
            std::swap(s->P.xit, s->P.xitn);
            std::swap(s->P.uit, s->P.uitn);
            s->parity ^= 1;
            s->lin_valid = false;
            s->sens_src = chk ? (s->ls_active ? 0 : 2) : 1;
            return CFNMPC_OK;
        }
    }
    if (!s->overlap) {
        // linearise -> QP, everything on the caller's stream
        if (e) HIP_TRY(hipEventRecord(e[0], st));
        if (s->P.fused != 1 || s->P.lbs) cfn::launch_linearise(s->P, s->chunks_all, st);   // (fused start solve: k_linfactor linearises)
        if (e) HIP_TRY(hipEventRecord(e[1], st));
        if (s->P.cond_N2) {
            cfn::launch_qp_cond(s->P, st);   // pcond -> condensed Riccati -> expand (-> interior point)
            if (e) for (int j = 2; j < 6; j++) HIP_TRY(hipEventRecord(e[j], st));   // (no per-kernel split on this path)
        } else {
            cfn::launch_qp(s->P, st, e ? e + 2 : nullptr);
        }
        if (e) HIP_TRY(hipEventRecord(e[6], st));
        if (chk) launch_sqp_close(s, *chk, st);
        std::swap(s->P.xit, s->P.xitn);   // the step's kernels wrote every instance's new iterate there
        std::swap(s->P.uit, s->P.uitn);
        s->parity ^= 1;
        s->lin_valid = false;   // the iterate moved
        // (cfnmpc_eval_sens_x0: the QP of this step -- not behind a line search: that QP belongs to w_{j-1}, the iterate is w_j)
        s->sens_src = chk ? (s->ls_active ? 0 : 2) : 1;
        return CFNMPC_OK;
    }
#ifdef CFN_DEV   // overlapped preparation: development builds only (CFNMPC_OVERLAP=1); s->overlap is 0 in the product
    // feedback phase on the linearisation prepared by the previous step ...
    if (!s->lin_valid) cfn::launch_linearise(s->P, s->chunks_all, st);
    if (e) HIP_TRY(hipEventRecord(e[0], st));
    cfn::launch_qp_start(s->P, st);
    HIP_TRY(hipEventRecord(s->ev_start, st));
    cfn::launch_qp_ipm(s->P, st);
    if (e) { for (int j = 1; j < 6; j++) HIP_TRY(hipEventRecord(e[j], st)); }   // (phases only on the overlapped path)
    // ... and preparation of the next step into the alternate set: an early pass over ALL
    // instances runs beside the interior-point kernel (the instances still inside it are
    // linearised around a stale iterate there and redone by the list pass afterwards)
    std::swap(s->P.xit, s->P.xitn);   // (host-side: kernel arguments are by value)
    std::swap(s->P.uit, s->P.uitn);
    cfn::Params Q = s->P;
    Q.AR = s->AR2; Q.BR = s->BR2; Q.b = s->b2;
    HIP_TRY(hipStreamWaitEvent(s->aux, s->ev_start, 0));
    cfn::launch_linearise(Q, s->chunks_all, s->aux);
    HIP_TRY(hipEventRecord(s->ev_aux, s->aux));
    HIP_TRY(hipStreamWaitEvent(st, s->ev_aux, 0));
    cfn::launch_linearise_list(Q, s->chunks_list, st);
    if (e) HIP_TRY(hipEventRecord(e[6], st));
    s->AR2 = s->P.AR; s->BR2 = s->P.BR; s->b2 = s->P.b;
    s->P.AR = Q.AR; s->P.BR = Q.BR; s->P.b = Q.b;
    s->lin_valid = true;
#endif
    return CFNMPC_OK;
}

}  // namespace

// ---- full SQP solve, per solver (cfnmpc_sqp.h): cfnmpc_solve_sqp and cfnmpc_fleet_solve_sqp drive these ----------------
namespace cfn {

int sqp_check_args(const cfnmpc_solver* s, int max_iter, double tol_step, double tol_eq, double tol_ineq) {
    if (!s || s->overlap || max_iter < 1) return CFNMPC_EINVAL;
    for (double t : {tol_step, tol_eq, tol_ineq})
        if (!(t > 0.0) || !std::isfinite(t)) return CFNMPC_EINVAL;
    return CFNMPC_OK;
}

int sqp_begin(cfnmpc_solver* s, int max_iter, double tol_step, double tol_eq, double tol_ineq, void* stream) {
    const int rc = sqp_check_args(s, max_iter, tol_step, tol_eq, tol_ineq);
    if (rc != CFNMPC_OK) return rc;
    DeviceGuard dg(s->device);
    if (!s->h_sqp_cnt) HIP_TRY(hipHostMalloc((void**)&s->h_sqp_cnt, 2 * sizeof(unsigned), hipHostMallocDefault));
    if (!s->sqp_ev) HIP_TRY(hipEventCreateWithFlags(&s->sqp_ev, hipEventDisableTiming));
    s->sqp.max_iter = max_iter;
    s->sqp.tol_step = tol_step; s->sqp.tol_eq = tol_eq; s->sqp.tol_ineq = tol_ineq;
    s->sqp.j = 0;
    // globalised solve: k_sqp_ls's state at the first one (iteration 1 ignores what an earlier solve left in it)
    if (s->glob_mode == CFNMPC_SQP_MERIT_BACKTRACKING && !s->ls.n_fail) {
        const size_t B = s->P.B;
        cfn::LsArgs a = s->ls;
        int rc2 = dev_alloc(s, &a.alpha, B);
        if (rc2 == CFNMPC_OK) rc2 = dev_alloc(s, &a.mu, B);
        if (rc2 == CFNMPC_OK) rc2 = dev_alloc(s, &a.n_short, B);
        if (rc2 == CFNMPC_OK) rc2 = dev_alloc(s, &a.n_fail, B);
        if (rc2 != CFNMPC_OK) return rc2;   // (what was allocated stays with the solver; the next solve allocates again)
        s->ls = a;
    }
    s->ls_active = s->glob_mode == CFNMPC_SQP_MERIT_BACKTRACKING;
    s->ls_last = s->glob_mode;
    // once per solve: both counters to zero (the check kernel of iteration j clears the counter of iteration j + 1 itself);
    // the done flags need no reset, iteration 1 ignores them
    HIP_TRY(hipMemsetAsync(s->sqp.cnt, 0, 2 * sizeof(unsigned), (hipStream_t)stream));
    return CFNMPC_OK;
}

// enqueues SQP iteration s->sqp.j + 1 (step + check) and the read-back of its count of open rows; records s->sqp_ev behind it
int sqp_iterate(cfnmpc_solver* s, void* stream) {
    DeviceGuard dg(s->device);
    hipStream_t st = (hipStream_t)stream;
    s->sqp.j++;
    const int rc = rti_step(s, st, false, &s->sqp);
    if (rc != CFNMPC_OK) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(s->h_sqp_cnt, s->sqp.cnt + (s->sqp.j & 1), sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(s->sqp_ev, st));
    return CFNMPC_OK;
}

// waits for the last enqueued iteration; *open = its rows not yet done
int sqp_wait(cfnmpc_solver* s, unsigned* open) {
    DeviceGuard dg(s->device);
    HIP_TRY(hipEventSynchronize(s->sqp_ev));
    *open = *(volatile unsigned*)s->h_sqp_cnt;
    return CFNMPC_OK;
}

int sqp_iterations(const cfnmpc_solver* s) { return s->sqp.j; }

int sqp_set_globalization(cfnmpc_solver* s, int mode, double eta, double reduction, double alpha_min) {
    if (!s || (mode != CFNMPC_SQP_FULL_STEP && mode != CFNMPC_SQP_MERIT_BACKTRACKING)) return CFNMPC_EINVAL;
    if (eta == 0.0) eta = 1e-4;
    if (reduction == 0.0) reduction = 0.5;
    if (alpha_min == 0.0) alpha_min = 1.0 / 1024.0;
    if (!(eta > 0.0 && eta < 0.5) || !(reduction > 0.0 && reduction < 1.0) || !(alpha_min > 0.0 && alpha_min <= 1.0))
        return CFNMPC_EINVAL;
    int T = 0;   // the smallest T with reduction^T <= alpha_min, the powers by repeated multiplication as in k_sqp_ls
    for (double a = 1.0; a > alpha_min; a *= reduction)
        if (++T > 32) return CFNMPC_EINVAL;
    s->glob_mode = mode;
    s->glob_alpha_min = alpha_min;
    s->ls.eta = eta; s->ls.reduction = reduction; s->ls.T = T;
    return CFNMPC_OK;
}

int sqp_get_ls_stats(cfnmpc_solver* s, double* alpha, double* mu, int* n_short, int* n_fail, int on_device, void* stream) {
    if (!s || s->ls_last < 0 || (!alpha && !mu && !n_short && !n_fail)) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    hipStream_t st = (hipStream_t)stream;
    const bool host = is_host(on_device);
    const size_t B = s->P.B;
    if (s->ls_last == CFNMPC_SQP_FULL_STEP) {   // full steps: alpha = 1, no penalty, nothing shortened (no buffer needed)
        if (host) {
            if (alpha) std::fill_n(alpha, B, 1.0);
            if (mu) std::fill_n(mu, B, 0.0);
            if (n_short) std::fill_n(n_short, B, 0);
            if (n_fail) std::fill_n(n_fail, B, 0);
            return CFNMPC_OK;
        }
        if (alpha) {
            const std::vector<double> one(B, 1.0);
            HIP_TRY(hipMemcpyAsync(alpha, one.data(), B * sizeof(double), hipMemcpyHostToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));   // (the source goes out of scope)
        }
        if (mu) HIP_TRY(hipMemsetAsync(mu, 0, B * sizeof(double), st));
        if (n_short) HIP_TRY(hipMemsetAsync(n_short, 0, B * sizeof(int), st));
        if (n_fail) HIP_TRY(hipMemsetAsync(n_fail, 0, B * sizeof(int), st));
        return CFNMPC_OK;
    }
    return copy_out({{alpha, s->ls.alpha, B * sizeof(double)}, {mu, s->ls.mu, B * sizeof(double)},
                     {n_short, s->ls.n_short, B * sizeof(int)}, {n_fail, s->ls.n_fail, B * sizeof(int)}}, on_device, st);
}

int sqp_get_stats(cfnmpc_solver* s, int* status, int* sqp_iter, double* res, int on_device, void* stream) {
    if (!s) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    const size_t B = s->P.B;
    return copy_out({{status, s->sqp.status, B * sizeof(int)}, {sqp_iter, s->sqp.iter, B * sizeof(int)}, {res, s->sqp.res, B * 3 * sizeof(double)}},
                    on_device, (hipStream_t)stream);
}

}  // namespace cfn

extern "C" {

int cfnmpc_solve(cfnmpc_solver* s, int n_rti, void* stream) {
    if (!s || n_rti < 1) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    hipStream_t st = (hipStream_t)stream;
    for (int it = 0; it < n_rti; it++) {
        const int rc = rti_step(s, st, s->reinit_failed != 0, nullptr);
        if (rc != CFNMPC_OK) return rc;
    }
    HIP_TRY(hipGetLastError());
    return CFNMPC_OK;
}

int cfnmpc_solve_sqp(cfnmpc_solver* s, int max_iter, double tol_step, double tol_eq, double tol_ineq, int* n_iter, void* stream) {
    int rc = cfn::sqp_begin(s, max_iter, tol_step, tol_eq, tol_ineq, stream);
    if (rc != CFNMPC_OK) return rc;
    for (int j = 1; j <= max_iter; j++) {
        unsigned open = 0;
        if ((rc = cfn::sqp_iterate(s, stream)) != CFNMPC_OK || (rc = cfn::sqp_wait(s, &open)) != CFNMPC_OK) return rc;
        if (open == 0) break;
    }
    if (n_iter) *n_iter = cfn::sqp_iterations(s);
    return CFNMPC_OK;
}

int cfnmpc_get_sqp_stats(cfnmpc_solver* s, int* status, int* sqp_iter, double* res, int on_device, void* stream) {
    return cfn::sqp_get_stats(s, status, sqp_iter, res, on_device, stream);
}

int cfnmpc_set_sqp_globalization(cfnmpc_solver* s, int mode, double eta, double reduction, double alpha_min) {
    return cfn::sqp_set_globalization(s, mode, eta, reduction, alpha_min);
}

int cfnmpc_get_sqp_globalization(const cfnmpc_solver* s, int* mode, double* eta, double* reduction, double* alpha_min) {
    if (!s || (!mode && !eta && !reduction && !alpha_min)) return CFNMPC_EINVAL;
    if (mode) *mode = s->glob_mode;
    if (eta) *eta = s->ls.eta;
    if (reduction) *reduction = s->ls.reduction;
    if (alpha_min) *alpha_min = s->glob_alpha_min;
    return CFNMPC_OK;
}

int cfnmpc_get_sqp_ls_stats(cfnmpc_solver* s, double* alpha, double* mu, int* n_short, int* n_fail, int on_device, void* stream) {
    return cfn::sqp_get_ls_stats(s, alpha, mu, n_short, n_fail, on_device, stream);
}

int cfnmpc_step_host(cfnmpc_solver* s, const double* x0, const double* yref, const double* yref_e, double* u,
                     double* x, int* status, int* qp_iter, double* res, void* stream) {
    if (!s || !x0 || !yref || !yref_e) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    hipStream_t st = (hipStream_t)stream;
    const cfn::Params& P = s->P;
    const size_t B = P.B, N = P.N;
    // layout of the I/O block (doubles): x0 | yref | yref_e || u | x | res | status, iters (as ints)
    const size_t n_x0 = B * 13, n_yr = B * N * 17, n_ye = B * 13, n_in = n_x0 + n_yr + n_ye;
    const size_t n_u = B * N * 4, n_x = B * (N + 1) * 13, n_res = B, n_int = B;   // 2 ints per double slot
    const size_t n_out = n_u + n_x + n_res + n_int, n_all = n_in + n_out;
    if (s->io_doubles < n_all) {
        if (s->h_io) (void)hipHostFree(s->h_io);
        s->h_io = nullptr;
        HIP_TRY(hipHostMalloc((void**)&s->h_io, n_all * sizeof(double), hipHostMallocDefault));
        int rc = dev_alloc(s, &s->d_io, n_all);
        if (rc != CFNMPC_OK) return rc;
        s->io_doubles = n_all;
    }
    double *h = s->h_io, *d = s->d_io;
    std::memcpy(h, x0, n_x0 * sizeof(double));
    std::memcpy(h + n_x0, yref, n_yr * sizeof(double));
    std::memcpy(h + n_x0 + n_yr, yref_e, n_ye * sizeof(double));
    HIP_TRY(hipMemcpyAsync(d, h, n_in * sizeof(double), hipMemcpyHostToDevice, st));
    cfn::launch_put(P.B, 1, 13, 1, d, P.x0, st);
    yref_rows_vary(s);   // (the shim's per-stage setter fills this array: no detection on the one-vehicle path)
    cfn::launch_put(P.B, P.N, 17, 1, d + n_x0, P.yref, st);
    cfn::launch_put(P.B, 1, 13, 1, d + n_x0 + n_yr, P.yref_e, st);
    int rc = cfnmpc_solve(s, 1, stream);
    if (rc != CFNMPC_OK) return rc;
    double* o = d + n_in;
    cfn::launch_get(P.B, P.N, 4, 0, 0, P.N, s->P.uit, o, st, P.v4b);
    cfn::launch_get(P.B, P.N + 1, 13, 1, 0, P.N + 1, s->P.xit, o + n_u, st);
    HIP_TRY(hipMemcpyAsync(o + n_u + n_x, s->P.res, B * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(o + n_u + n_x + n_res, s->P.status, B * sizeof(int), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync((int*)(o + n_u + n_x + n_res) + B, s->P.iters, B * sizeof(int), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h + n_in, o, n_out * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const double* ho = h + n_in;
    if (u) std::memcpy(u, ho, n_u * sizeof(double));
    if (x) std::memcpy(x, ho + n_u, n_x * sizeof(double));
    if (res) std::memcpy(res, ho + n_u + n_x, B * sizeof(double));
    const int* hi = (const int*)(ho + n_u + n_x + n_res);
    if (status) std::memcpy(status, hi, B * sizeof(int));
    if (qp_iter) std::memcpy(qp_iter, hi + B, B * sizeof(int));
    return CFNMPC_OK;
}

int cfnmpc_get_u(cfnmpc_solver* s, int stage, double* u, int on_device, void* stream) {
    if (!s || !u || stage < 0 || stage >= s->P.N) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    return get_field(s, u, on_device, 1, 4, 0, stage, s->P.N, s->P.uit, (hipStream_t)stream);
}

int cfnmpc_get_x(cfnmpc_solver* s, int stage, double* x, int on_device, void* stream) {
    if (!s || !x || stage < 0 || stage > s->P.N) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    return get_field(s, x, on_device, 1, 13, 1, stage, s->P.N + 1, s->P.xit, (hipStream_t)stream);
}

int cfnmpc_get_stats(cfnmpc_solver* s, int* status, int* qp_iter, double* res, int on_device, void* stream) {
    if (!s) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    const size_t B = s->P.B;
    return copy_out({{status, s->P.status, B * sizeof(int)}, {qp_iter, s->P.iters, B * sizeof(int)}, {res, s->P.res, B * sizeof(double)}},
                    on_device, (hipStream_t)stream);
}

// ---- NLP evaluation at the current iterate --------------------------------------------------------
int cfnmpc_eval_nlp(cfnmpc_solver* s, int keep_multipliers, void* stream) {
    if (!s || (keep_multipliers != 0 && keep_multipliers != 1)) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    cfn::NlpArgs& A = s->nlp;
    if (keep_multipliers && !A.gu) {   // costates in the x-iterate's layout, reduced gradient in the u-iterate's (spare block included)
        const size_t NW = (size_t)s->P.NW + 1, N = s->P.N;
        double *pi = nullptr, *gu = nullptr;
        int rc = dev_alloc(s, &pi, NW * (N + 1) * cfn::SZ_V13);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &gu, NW * 4 * N * 4);
        if (rc != CFNMPC_OK) return rc;   // (what was allocated stays with the solver; the next call allocates again)
        A.pi = pi; A.gu = gu;
    }
    cfn::NlpArgs a = A;
    if (!keep_multipliers) a.pi = a.gu = nullptr;
    cfn::launch_nlp_eval(s->P, a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    s->nlp_state = keep_multipliers ? 2 : 1;
    return CFNMPC_OK;
}

int cfnmpc_get_nlp_stats(cfnmpc_solver* s, double* cost, double* res, int on_device, void* stream) {
    if (!s || s->nlp_state == 0 || (!cost && !res)) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    const size_t B = s->P.B;
    return copy_out({{cost, s->nlp.cost, B * sizeof(double)}, {res, s->nlp.res, B * 3 * sizeof(double)}}, on_device, (hipStream_t)stream);
}

int cfnmpc_get_nlp_multipliers(cfnmpc_solver* s, double* pi, double* gu, int on_device, void* stream) {
    if (!s || s->nlp_state != 2 || (!pi && !gu)) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    const int N = s->P.N;
    if (pi) {
        const int rc = get_field(s, pi, on_device, N + 1, 13, 1, 0, N + 1, s->nlp.pi, (hipStream_t)stream);
        if (rc != CFNMPC_OK) return rc;
    }
    if (gu) return get_field(s, gu, on_device, N, 4, 0, 0, N, s->nlp.gu, (hipStream_t)stream);
    return CFNMPC_OK;
}

// ---- solution sensitivities with respect to x0 ---------------------------------------------------
int cfnmpc_eval_sens_x0(cfnmpc_solver* s, double act_tol, void* stream) {
    if (!s || !std::isfinite(act_tol) || !(act_tol > 0.0)) return CFNMPC_EINVAL;
    // partial condensing and the fused start solve (start_solve = 2) write no home blocks / gains / checkpoints
    if (s->P.cond_N2 || s->P.fused == 1 || s->sens_src == 0) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    cfn::SensArgs& A = s->sens;
    const size_t NW = (size_t)s->P.NW + 1, N = s->P.N, B = s->P.B;
    if (!A.K) {
        cfn::SensArgs a{};
        int rc = dev_alloc(s, &a.mask, B * N * 4);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &a.list, B);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &a.cnt, 1);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &a.kst, B);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &a.K, NW * N * cfn::SZ_K);
        if (rc != CFNMPC_OK) return rc;   // (what was allocated stays with the solver; the next call allocates again)
        A = a;
    }
    s->sens_valid = false;
    s->adj_valid = false;
    A.tol = act_tol;
    cfn::launch_sens_eval(s->P, A, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    s->sens_valid = true;
    return CFNMPC_OK;
}

int cfnmpc_get_sens_x0(cfnmpc_solver* s, int stage, int n_stages, double* du, double* dx, int on_device, void* stream) {
    if (!s || !s->sens_valid) return CFNMPC_EINVAL;
    const int N = s->P.N;
    if (stage < 0 || n_stages < 1 || (long)stage + n_stages > N + 1 || (!du && !dx) || (du && stage + n_stages > N))
        return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    hipStream_t st = (hipStream_t)stream;
    cfn::SensArgs A = s->sens;
    A.status = s->sens_src == 2 ? s->sqp.status : s->P.status;
    A.s0 = stage;
    A.ns = n_stages;
    const size_t B = s->P.B, nu = du ? (size_t)n_stages * 52 : 0, nx = dx ? (size_t)n_stages * 169 : 0;
    if (!is_host(on_device)) {
        A.du = du; A.dx = dx; A.b0 = 0; A.nb = (int)B;
        cfn::launch_sens_fwd(s->P, A, st);
        HIP_TRY(hipGetLastError());
        return CFNMPC_OK;
    }
    // host arrays: rows in chunks of whole wavefronts through the staging buffer (host_row_chunks)
    RC_TRY(host_row_chunks(s, nu + nx, [&](size_t b0, size_t nb, double* stage) {
        A.b0 = (int)b0; A.nb = (int)nb;
        A.du = du ? stage : nullptr;
        A.dx = dx ? stage + nb * nu : nullptr;
        cfn::launch_sens_fwd(s->P, A, st);
        HIP_TRY(hipGetLastError());
        if (du) HIP_TRY(hipMemcpyAsync(du + b0 * nu, A.du, nb * nu * sizeof(double), hipMemcpyDeviceToHost, st));
        if (dx) HIP_TRY(hipMemcpyAsync(dx + b0 * nx, A.dx, nb * nx * sizeof(double), hipMemcpyDeviceToHost, st));
        return (int)CFNMPC_OK;
    }));
    if (on_device == CFNMPC_ON_HOST) HIP_TRY(hipStreamSynchronize(st));
    return CFNMPC_OK;
}

int cfnmpc_get_sens_active(cfnmpc_solver* s, signed char* act, int on_device, void* stream) {
    if (!s || !act || !s->sens_valid) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    return copy_out({{act, s->sens.mask, (size_t)s->P.B * s->P.N * 4}}, on_device, (hipStream_t)stream);
}

// ---- adjoint solution sensitivities --------------------------------------------------------------
int cfnmpc_eval_adjoint(cfnmpc_solver* s, const double* gx, int n_gx, const double* gu, int n_gu, int on_device, void* stream) {
    // the sensitivity evaluation is the one source of the active set: whatever refuses or invalidates it refuses this call
    if (!s || !s->sens_valid) return CFNMPC_EINVAL;
    const size_t N = s->P.N, B = s->P.B;
    if ((gx && (n_gx < 1 || (size_t)n_gx > N + 1)) || (gu && (n_gu < 1 || (size_t)n_gu > N))) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    hipStream_t st = (hipStream_t)stream;
    cfn::AdjArgs& A = s->adj;
    if (!A.kap) {
        cfn::AdjArgs a{};
        int rc = dev_alloc(s, &a.kap, B * N * 4);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &a.wuni, 32);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &a.dq, B * (N + 1) * 13);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &a.dr, B * N * 4);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &a.dx0, B * 13);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &a.db, B * N * 13);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &a.dbox, B * N * 4);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &a.dW, B * 17);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &a.dWN, B * 13);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &a.dyref, B * N * 17);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &a.dyref_e, B * 13);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &s->adj_gx, B * (N + 1) * 13);
        if (rc == CFNMPC_OK) rc = dev_alloc(s, &s->adj_gu, B * N * 4);
        if (rc != CFNMPC_OK) return rc;   // (what was allocated stays with the solver; the next call allocates again)
        A = a;
    }
    s->adj_valid = false;
    A.gx = gx; A.gu = gu;
    A.n_gx = gx ? n_gx : 0; A.n_gu = gu ? n_gu : 0;
    if (is_host(on_device)) {   // (the solver's own copies: the sweeps read them after this call has returned)
        if (gx) {
            HIP_TRY(hipMemcpyAsync(s->adj_gx, gx, B * n_gx * 13 * sizeof(double), hipMemcpyHostToDevice, st));
            A.gx = s->adj_gx;
        }
        if (gu) {
            HIP_TRY(hipMemcpyAsync(s->adj_gu, gu, B * n_gu * 4 * sizeof(double), hipMemcpyHostToDevice, st));
            A.gu = s->adj_gu;
        }
    }
    A.mask = s->sens.mask; A.kst = s->sens.kst; A.K = s->sens.K;
    A.status = s->sens_src == 2 ? s->sqp.status : s->P.status;
    A.stage_scale = s->stage_scale; A.terminal_scale = s->terminal_scale;
    cfn::launch_adjoint(s->P, A, st);
    HIP_TRY(hipGetLastError());
    if (on_device == CFNMPC_ON_HOST) HIP_TRY(hipStreamSynchronize(st));   // (the caller's arrays are free again)
    s->adj_valid = true;
    return CFNMPC_OK;
}

int cfnmpc_get_adjoint(cfnmpc_solver* s, double* dl_dx0, double* dl_dq, double* dl_dr, double* dl_db, double* dl_dbox, int on_device,
                       void* stream) {
    if (!s || !s->adj_valid) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    const size_t N = s->P.N, B = s->P.B, d = sizeof(double);
    const cfn::AdjArgs& A = s->adj;
    return copy_out({{dl_dx0, A.dx0, B * 13 * d}, {dl_dq, A.dq, B * (N + 1) * 13 * d}, {dl_dr, A.dr, B * N * 4 * d},
                     {dl_db, A.db, B * N * 13 * d}, {dl_dbox, A.dbox, B * N * 4 * d}}, on_device, (hipStream_t)stream);
}

int cfnmpc_get_adjoint_cost(cfnmpc_solver* s, double* dl_dW, double* dl_dWN, double* dl_dyref, double* dl_dyref_e, int on_device,
                            void* stream) {
    if (!s || !s->adj_valid) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    const size_t N = s->P.N, B = s->P.B, d = sizeof(double);
    const cfn::AdjArgs& A = s->adj;
    return copy_out({{dl_dW, A.dW, B * 17 * d}, {dl_dWN, A.dWN, B * 13 * d}, {dl_dyref, A.dyref, B * N * 17 * d},
                     {dl_dyref_e, A.dyref_e, B * 13 * d}}, on_device, (hipStream_t)stream);
}

// ---- uncertainty propagation and robust input-bound tightening -----------------------------------
namespace {
// one table of cfnmpc_set_uncertainty: allocated at the first array, filled by one put kernel on `st`
int unc_put_table(cfnmpc_solver* s, const double* src, bool host, size_t per, size_t blk, double** tab, hipStream_t st) {
    const size_t B = s->P.B, n = B * per;
    if (!*tab) RC_TRY(dev_alloc(s, tab, (size_t)s->P.NW * blk));   // (zero: the padding rows stay so)
    const double* d = src;
    if (host) {
        if (!s->unc.stage) RC_TRY(dev_alloc(s, &s->unc.stage, B * 169));
        HIP_TRY(hipMemcpyAsync(s->unc.stage, src, n * sizeof(double), hipMemcpyHostToDevice, st));
        d = s->unc.stage;
    }
    if (per == 169) cfn::launch_unc_put_sym((int)B, d, *tab, st);
    else cfn::launch_unc_put_gain((int)B, d, *tab, st);
    HIP_TRY(hipGetLastError());
    return CFNMPC_OK;
}
cfn::UncArgs unc_args(const cfnmpc_solver* s) {
    cfn::UncArgs A{};
    A.S0 = s->unc.has_S0 ? s->unc.S0 : nullptr;
    A.W = s->unc.has_W ? s->unc.W : nullptr;
    A.Ku = s->unc.gain_mode == CFNMPC_UNC_GAIN_USER ? s->unc.K : nullptr;
    A.status = s->sens_src == 2 ? s->sqp.status : s->P.status;
    return A;
}
}  // namespace

}  // extern "C"
namespace cfn {
bool unc_backoff_valid(const cfnmpc_solver* s) { return s && s->unc.beta_valid; }
int poly_n_traj(const cfnmpc_solver* s) { return s ? s->poly.n_traj : 0; }
}
extern "C" {

int cfnmpc_set_uncertainty(cfnmpc_solver* s, const double* Sigma0, const double* W, int on_device, void* stream) {
    if (!s) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    hipStream_t st = (hipStream_t)stream;
    const size_t B = s->P.B;
    const bool host = is_host(on_device);
    // host arrays are validated as a whole before anything changes; device arrays are taken as they are
    if (host && ((Sigma0 && !cfn::unc_sym_ok(Sigma0, B)) || (W && !cfn::unc_sym_ok(W, B)))) return CFNMPC_EINVAL;
    // new inputs: the covariance getter would sweep with them while the stored beta is the old evaluation's -- it waits for the
    // next cfnmpc_eval_uncertainty (the backoff itself stays valid: it is what cfnmpc_tighten_box applies)
    s->unc.current = false;
    // each table's flag follows its own put, so that a failure of the second put (allocation, copy) leaves tables and flags agreeing
    s->unc.has_S0 = false;
    if (Sigma0) {
        RC_TRY(unc_put_table(s, Sigma0, host, 169, cfn::SZ_P, &s->unc.S0, st));
        s->unc.has_S0 = true;
        if (host && W) HIP_TRY(hipStreamSynchronize(st));   // (the staging buffer is reused)
    }
    s->unc.has_W = false;
    if (W) {
        RC_TRY(unc_put_table(s, W, host, 169, cfn::SZ_P, &s->unc.W, st));
        s->unc.has_W = true;
    }
    if (on_device == CFNMPC_ON_HOST) HIP_TRY(hipStreamSynchronize(st));
    return CFNMPC_OK;
}

int cfnmpc_set_uncertainty_gain(cfnmpc_solver* s, int mode, const double* K, int on_device, void* stream) {
    if (!s || (mode != CFNMPC_UNC_GAIN_RICCATI && mode != CFNMPC_UNC_GAIN_USER)) return CFNMPC_EINVAL;
    if (mode == CFNMPC_UNC_GAIN_RICCATI) { s->unc.gain_mode = mode; s->unc.current = false; return CFNMPC_OK; }
    if (!K) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)s->P.B * 52;
    const bool host = is_host(on_device);
    if (host)
        for (size_t i = 0; i < n; i++) if (!std::isfinite(K[i])) return CFNMPC_EINVAL;
    s->unc.current = false;   // (as cfnmpc_set_uncertainty)
    RC_TRY(unc_put_table(s, K, host, 52, cfn::SZ_K, &s->unc.K, st));
    if (on_device == CFNMPC_ON_HOST) HIP_TRY(hipStreamSynchronize(st));
    s->unc.gain_mode = mode;
    return CFNMPC_OK;
}

int cfnmpc_eval_uncertainty(cfnmpc_solver* s, void* stream) {
    if (!s) return CFNMPC_EINVAL;
    // partial condensing and the fused start solve (start_solve = 2) write no home blocks / gains; the blocks must be the last
    // QP's: a solve, and no change of its data since
    if (s->P.cond_N2 || s->P.fused == 1 || s->sens_src == 0 || s->unc.inputs_moved) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    if (!s->unc.beta) RC_TRY(dev_alloc(s, &s->unc.beta, (size_t)s->P.NW * 4 * s->P.N * 4));
    cfn::UncArgs A = unc_args(s);
    A.beta = s->unc.beta;
    A.s0 = 0; A.ns = s->P.N; A.b0 = 0; A.nb = s->P.B;
    s->unc.beta_valid = false;
    cfn::launch_unc_prop(s->P, A, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    s->unc.beta_valid = true;
    s->unc.current = true;
    return CFNMPC_OK;
}

int cfnmpc_get_backoff(cfnmpc_solver* s, double* beta, int on_device, void* stream) {
    if (!s || !beta || !s->unc.beta_valid) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    return get_field(s, beta, on_device, s->P.N, 4, 0, 0, s->P.N, s->unc.beta, (hipStream_t)stream);
}

int cfnmpc_get_uncertainty(cfnmpc_solver* s, int stage, int n_stages, double* Sigma, double* std_x, int on_device, void* stream) {
    if (!s || !s->unc.current) return CFNMPC_EINVAL;
    const int N = s->P.N;
    if (stage < 0 || n_stages < 1 || (long)stage + n_stages > N + 1 || (!Sigma && !std_x)) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    hipStream_t st = (hipStream_t)stream;
    cfn::UncArgs A = unc_args(s);
    A.s0 = stage;
    A.ns = n_stages;
    const size_t B = s->P.B, ng = Sigma ? (size_t)n_stages * 169 : 0, nd = std_x ? (size_t)n_stages * 13 : 0;
    if (!is_host(on_device)) {
        A.Sig = Sigma; A.sd = std_x; A.b0 = 0; A.nb = (int)B;
        cfn::launch_unc_prop(s->P, A, st);
        HIP_TRY(hipGetLastError());
        return CFNMPC_OK;
    }
    // host arrays: rows in chunks of whole wavefronts through the staging buffer of the sensitivities' host reads
    RC_TRY(host_row_chunks(s, ng + nd, [&](size_t b0, size_t nb, double* stage) {
        A.b0 = (int)b0; A.nb = (int)nb;
        A.Sig = Sigma ? stage : nullptr;
        A.sd = std_x ? stage + nb * ng : nullptr;
        cfn::launch_unc_prop(s->P, A, st);
        HIP_TRY(hipGetLastError());
        if (Sigma) HIP_TRY(hipMemcpyAsync(Sigma + b0 * ng, A.Sig, nb * ng * sizeof(double), hipMemcpyDeviceToHost, st));
        if (std_x) HIP_TRY(hipMemcpyAsync(std_x + b0 * nd, A.sd, nb * nd * sizeof(double), hipMemcpyDeviceToHost, st));
        return (int)CFNMPC_OK;
    }));
    if (on_device == CFNMPC_ON_HOST) HIP_TRY(hipStreamSynchronize(st));
    return CFNMPC_OK;
}

int cfnmpc_tighten_box(cfnmpc_solver* s, double gamma, double min_width, int* n_clamped, int on_device, void* stream) {
    if (!s || !s->unc.beta_valid || !std::isfinite(gamma) || !(gamma >= 0.0) || !(min_width > 0.0) || !(min_width <= 1.0))
        return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    cfn::Params& P = s->P;
    hipStream_t st = (hipStream_t)stream;
    const size_t B = P.B;
    if (!s->unc.ncl) RC_TRY(dev_alloc(s, &s->unc.ncl, B));
    if (gamma == 0.0) {   // the nominal box back in force (the scalar route again if it is scalar)
        RC_TRY(untighten(s, st));
        HIP_TRY(hipMemsetAsync(s->unc.ncl, 0, B * sizeof(int), st));
    } else {
        RC_TRY(ensure_box_blocks(s));
        const size_t cnt = (size_t)P.NW * 4 * P.N * 4;
        if (!s->unc.tight) {   // the box in force is the nominal one: remember it
            s->unc.nom_stages = P.lbs != nullptr;
            if (s->unc.nom_stages) {
                if (!s->unc.nom_lb) RC_TRY(dev_alloc(s, &s->unc.nom_lb, cnt));
                if (!s->unc.nom_ub) RC_TRY(dev_alloc(s, &s->unc.nom_ub, cnt));
                HIP_TRY(hipMemcpyAsync(s->unc.nom_lb, P.lbs, cnt * sizeof(double), hipMemcpyDeviceToDevice, st));
                HIP_TRY(hipMemcpyAsync(s->unc.nom_ub, P.ubs, cnt * sizeof(double), hipMemcpyDeviceToDevice, st));
            }
        }
        cfn::TightenArgs T{};
        T.nlb = s->unc.nom_stages ? s->unc.nom_lb : nullptr;
        T.nub = s->unc.nom_stages ? s->unc.nom_ub : nullptr;
        T.u_min = P.u_min; T.u_max = P.u_max;
        T.beta = s->unc.beta;
        T.gamma = gamma; T.min_width = min_width;
        T.lbs = P.lbs ? P.lbs : s->lbs_keep; T.ubs = P.ubs ? P.ubs : s->ubs_keep;
        T.clbs = P.clbs; T.cubs = P.cubs;
        T.ncl = s->unc.ncl;
        cfn::launch_unc_tighten(P, T, st);
        HIP_TRY(hipGetLastError());
        // new values over old ones in place: captured step graphs keep replaying; only the switch from the scalar route
        // invalidates them (as cfnmpc_set_box_stages does)
        if (!P.lbs) { P.lbs = s->lbs_keep; P.ubs = s->ubs_keep; invalidate_graphs(s); }
        s->unc.tight = true;
        invalidate_sens(s);   // (the box is part of the QP's data)
    }
    if (n_clamped) return copy_out({{n_clamped, s->unc.ncl, B * sizeof(int)}}, on_device, st);
    if (on_device == CFNMPC_ON_HOST) HIP_TRY(hipStreamSynchronize(st));
    return CFNMPC_OK;
}

namespace {
// Device scratch of the entry points that take host arrays without a solver (staged_call below), `need` doubles: cached per
// device and grown on demand (the estimator calls cfnmpc_sim at 66 Hz with batch 1, acados_estimator.cpp:589 -- no allocation
// per call); one caller at a time PER DEVICE (predictors on different GPUs run concurrently): `lock` is held by the caller
// until its transfers are complete
int host_scratch(size_t need, double** out, std::unique_lock<std::mutex>& lock) {
    static std::mutex mtx[64];
    static double* scratch[64] = {nullptr};
    static size_t cap[64] = {0};
    int devi = 0;
    HIP_TRY(hipGetDevice(&devi));
    if (devi < 0 || devi >= 64) return CFNMPC_EHIP;
    lock = std::unique_lock<std::mutex>(mtx[devi]);
    if (cap[devi] < need) {
        if (scratch[devi]) (void)hipFree(scratch[devi]);
        scratch[devi] = nullptr; cap[devi] = 0;
        if (hipMalloc((void**)&scratch[devi], need * 8) != hipSuccess) return CFNMPC_ENOMEM;
        cap[devi] = need;
    }
    *out = scratch[devi];
    return CFNMPC_OK;
}
using cfn::ArrPtrs;
// One solver-less call over the arrays of `t` (cfnmpc_stage.hpp).  Device arrays: the caller's pointers
// go to `launch` as they are, nothing is copied or waited for.  Host arrays (validated by the caller before this): staged in
// host_scratch -- in and in-out arrays up, launch, out and in-out arrays down -- and synchronised with the scratch still locked.
extern "C++" template <class Launch>
int staged_call(const cfn::Stage& t, int on_device, hipStream_t st, Launch&& launch) {
    if (!is_host(on_device)) {
        launch(t.own());
        HIP_TRY(hipGetLastError());
        return CFNMPC_OK;
    }
    std::unique_lock<std::mutex> lock;
    double* base = nullptr;
    RC_TRY(host_scratch(t.bytes / 8, &base, lock));
    const ArrPtrs a = t.at(base);
    for (int i = 0; i < t.n; i++)
        if (t.copy_in(i)) HIP_TRY(hipMemcpyAsync(a.p[i], t.a[i].p, t.size(i), hipMemcpyHostToDevice, st));
    launch(a);
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < t.n; i++)
        if (t.copy_out(i)) HIP_TRY(hipMemcpyAsync(t.a[i].p, a.p[i], t.size(i), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CFNMPC_OK;
}
// optional host rows p [B][NPAR] and d [B][ND] hold valid values (device rows are not looked at)
bool host_rows_ok(const double* p, const double* d, size_t B, int on_device) {
    return !is_host(on_device) || ((!p || cfn::model_params_ok(p, B * cfn::NPAR)) && (!d || cfn::dist_rows_ok(d, B * cfn::ND)));
}
// cfnmpc_sim (p = NULL: the folded constants), cfnmpc_sim_params (p [batch][NPAR]) and cfnmpc_sim_dist (d [batch][ND], p or NULL)
int sim_impl(int batch, const double* x, const double* u, const double* p, const double* d, double T, int steps, double* xn,
             int on_device, void* stream) {
    if (batch <= 0 || !x || !u || !xn || steps < 1 || !(T > 0)) return CFNMPC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const size_t B = batch;
    if (!host_rows_ok(p, d, B, on_device)) return CFNMPC_EINVAL;
    using K = cfn::SimArrs;
    return staged_call(K::of(B, x, u, xn, p, d), on_device, st, [&](const ArrPtrs& a) {
        cfn::launch_sim(batch, a.d(K::X), a.d(K::U), a.d(K::P), a.d(K::D), T, steps, a.d(K::XN), st);
    });
}
}  // namespace

int cfnmpc_sim(int batch, const double* x, const double* u, double T, int steps, double* xn, int on_device,
               void* stream) {
    return sim_impl(batch, x, u, nullptr, nullptr, T, steps, xn, on_device, stream);
}

int cfnmpc_sim_params(int batch, const double* x, const double* u, const double* p, double T, int steps, double* xn,
                      int on_device, void* stream) {
    if (!p) return CFNMPC_EINVAL;
    return sim_impl(batch, x, u, p, nullptr, T, steps, xn, on_device, stream);
}

int cfnmpc_sim_dist(int batch, const double* x, const double* u, const double* p, const double* d, double T, int steps,
                    double* xn, int on_device, void* stream) {
    if (!d) return CFNMPC_EINVAL;
    return sim_impl(batch, x, u, p, d, T, steps, xn, on_device, stream);
}

int cfnmpc_sim_rollout(int batch, int L, const double* x0, const double* u, const double* p, const double* d, double T, int steps,
                       double* xs, int on_device, void* stream) {
    if (batch <= 0 || L < 1 || !x0 || !u || !xs || steps < 1 || !(T > 0)) return CFNMPC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (!host_rows_ok(p, d, batch, on_device)) return CFNMPC_EINVAL;
    using K = cfn::RolloutArrs;
    return staged_call(K::of(batch, L, x0, u, xs, p, d), on_device, st, [&](const ArrPtrs& a) {
        cfn::launch_sim_rollout(batch, L, a.d(K::X0), a.d(K::U), a.d(K::P), a.d(K::D), T, steps, a.d(K::XS), st);
    });
}

int cfnmpc_sim_rollout_vjp(int batch, int L, const double* xs, const double* u, const double* p, const double* d, double T, int steps,
                           const double* gxs, double* gx0, double* gu, double* gp, double* gd, int on_device, void* stream) {
    if (batch <= 0 || L < 1 || !xs || !u || !gxs || !gx0 || steps < 1 || !(T > 0)) return CFNMPC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (!host_rows_ok(p, d, batch, on_device)) return CFNMPC_EINVAL;
    using K = cfn::RolloutVjpArrs;
    return staged_call(K::of(batch, L, xs, gxs, u, p, d, gx0, gu, gp, gd), on_device, st, [&](const ArrPtrs& a) {
        cfn::launch_sim_rollout_vjp(batch, L, a.d(K::XS), a.d(K::U), a.d(K::P), a.d(K::D), T, steps, a.d(K::GXS), a.d(K::GX0),
                                    a.d(K::GU), a.d(K::GP), a.d(K::GD), st);
    });
}

int cfnmpc_ekf_step(int batch, const double* x, const double* P, const double* u, const double* p, const double* d, double T,
                    int steps, const double* Q, const double* z, const double* r, double gate, int flags, double* x_new,
                    double* P_new, double* nis, int* counts, int on_device, void* stream) {
    if (batch <= 0 || steps < 1 || !(T > 0) || !x || !P || !u || !x_new || !P_new || (z && !r)) return CFNMPC_EINVAL;
    if (!(gate >= 0.0 && gate <= 1.7976931348623157e308) || (flags & ~CFNMPC_EKF_NORMALIZE_Q)) return CFNMPC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    cfn::EkfArgs A{};
    A.B = batch; A.steps = steps; A.flags = flags; A.T = T; A.gate = gate;
    const size_t B = batch, nx = B * 13, nu = B * 4;
    if (is_host(on_device)) {
        // host arrays: validated as a whole before anything runs (x, u, z, r, d: finite -- dist_rows_ok's rule)
        if (!cfn::dist_rows_ok(x, nx) || !cfn::dist_rows_ok(u, nu) || !cfn::unc_sym_ok(P, B) || (Q && !cfn::unc_sym_ok(Q, B))) return CFNMPC_EINVAL;
        if (z && (!cfn::dist_rows_ok(z, nx) || !cfn::dist_rows_ok(r, nx))) return CFNMPC_EINVAL;
        if (!host_rows_ok(p, d, B, on_device)) return CFNMPC_EINVAL;
    }
    using K = cfn::EkfArrs;
    return staged_call(K::of(B, x, P, u, p, d, Q, z, r, x_new, P_new, nis, counts), on_device, st, [&](const ArrPtrs& a) {
        A.x = a.d(K::X); A.P = a.d(K::P); A.u = a.d(K::U); A.p = a.d(K::PAR); A.d = a.d(K::D); A.Q = a.d(K::Q); A.z = a.d(K::Z);
        A.r = a.d(K::R); A.xn = a.d(K::XN); A.Pn = a.d(K::PN); A.nis = a.d(K::NIS); A.counts = a.i(K::COUNTS);
        cfn::launch_ekf(A, st);
    });
}

int cfnmpc_ekf_aug_step(int batch, const double* x, const double* d, const double* Pa, const double* u, const double* p, const int* sel,
                        double T, int steps, const double* Q, const double* Qd, const double* z, const double* r, double gate,
                        int flags, double* x_new, double* d_new, double* Pa_new, double* Pxx_new, double* nis, int* counts,
                        int on_device, void* stream) {
    if (batch <= 0 || steps < 1 || !(T > 0) || !x || !d || !Pa || !u || !sel || !x_new || !d_new || !Pa_new || (z && !r)) return CFNMPC_EINVAL;
    if (!(gate >= 0.0 && gate <= 1.7976931348623157e308) || (flags & ~CFNMPC_EKF_NORMALIZE_Q)) return CFNMPC_EINVAL;
    if (!cfn::ekf_sel_ok(sel)) return CFNMPC_EINVAL;   // (sel is a host array in every call)
    hipStream_t st = (hipStream_t)stream;
    cfn::EkfAugArgs A{};
    A.B = batch; A.steps = steps; A.flags = flags; A.T = T; A.gate = gate;
    for (int k = 0; k < 3; k++) A.sel[k] = sel[k];
    const size_t B = batch, nx = B * 13, nu = B * 4, nq = B * 3;
    if (is_host(on_device)) {
        // host arrays: validated as a whole before anything runs, by cfnmpc_ekf_step's rules (Pa: the same rule at size 16, and
        // zero rows and columns for the unused slots; Qd: finite, >= 0)
        if (!cfn::dist_rows_ok(x, nx) || !cfn::dist_rows_ok(u, nu) || !cfn::unc_sym_ok<16>(Pa, B) || !cfn::ekf_unused_zero(Pa, B, sel) ||
            (Q && !cfn::unc_sym_ok(Q, B))) return CFNMPC_EINVAL;
        if (Qd)
            for (size_t e = 0; e < nq; e++)
                if (sel[e % 3] >= 0 && !(Qd[e] >= 0.0 && Qd[e] <= 1.7976931348623157e308)) return CFNMPC_EINVAL;
        if (z && (!cfn::dist_rows_ok(z, nx) || !cfn::dist_rows_ok(r, nx))) return CFNMPC_EINVAL;
        if (!host_rows_ok(p, d, B, on_device)) return CFNMPC_EINVAL;
    }
    using K = cfn::EkfAugArrs;
    return staged_call(K::of(B, x, d, Pa, u, p, Q, Qd, z, r, x_new, d_new, Pa_new, Pxx_new, nis, counts), on_device, st,
                       [&](const ArrPtrs& a) {
        A.x = a.d(K::X); A.d = a.d(K::D); A.Pa = a.d(K::PA); A.u = a.d(K::U); A.p = a.d(K::PAR); A.Q = a.d(K::Q); A.Qd = a.d(K::QD);
        A.z = a.d(K::Z); A.r = a.d(K::R); A.xn = a.d(K::XN); A.dn = a.d(K::DN); A.Pan = a.d(K::PAN); A.Pxx = a.d(K::PXX);
        A.nis = a.d(K::NIS); A.counts = a.i(K::COUNTS);
        cfn::launch_ekf_aug(A, st);
    });
}

int cfnmpc_estimate_disturbance(int batch, const double* x_prev,const double* u_prev, const double* x_meas, const double* p,
                                double* d, double T, int steps, double gain_a, double gain_w, int on_device, void* stream) {
    if (batch <= 0 || !x_prev || !u_prev || !x_meas || !d || steps < 1 || !(T > 0)) return CFNMPC_EINVAL;
    if (!(gain_a > 0 && gain_a <= 1) || !(gain_w > 0 && gain_w <= 1)) return CFNMPC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (!host_rows_ok(p, d, batch, on_device)) return CFNMPC_EINVAL;
    using K = cfn::DistObserveArrs;
    return staged_call(K::of(batch, x_prev, u_prev, x_meas, d, p), on_device, st, [&](const ArrPtrs& a) {
        cfn::launch_dist_observe(batch, a.d(K::XP), a.d(K::U), a.d(K::XM), a.d(K::P), a.d(K::D), T, steps, gain_a, gain_w, st);
    });
}

int cfnmpc_estimate(int batch, const double* meas, double* filt, const double* u, double dt, int use_lpf, double delay,
                    int steps, double* x_est, double* x_pred, void* stream) {
    if (batch <= 0 || !meas || !filt || !u || !x_est || !x_pred || steps < 1 || !(delay > 0) || !(dt > 0))
        return CFNMPC_EINVAL;
    cfn::launch_estimate(batch, meas, filt, u, dt, use_lpf ? 1 : 0, delay, steps, x_est, x_pred, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return CFNMPC_OK;
}

int cfnmpc_set_profiling(cfnmpc_solver* s, int enable) {
    if (!s) return CFNMPC_EINVAL;
    s->profiling = enable ? 1 : 0;
    s->ev_used = 0;
    return CFNMPC_OK;
}

// per timed step: ms_steps [max_steps][6] (the six groups of cfnmpc_get_profile_kernels), *n_steps = steps written (<= max_steps;
// later timed steps are dropped); resets the count like cfnmpc_get_profile_kernels
int cfnmpc_get_profile_steps(cfnmpc_solver* s, double* ms_steps, int max_steps, int* n_steps) {
    if (!s || !ms_steps || max_steps < 0 || !n_steps) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    size_t n = s->ev_used / EV_PER_STEP;
    if (n > (size_t)max_steps) n = (size_t)max_steps;
    for (size_t i = 0; i < n; i++) {
        hipEvent_t* e = &s->ev[EV_PER_STEP * i];
        HIP_TRY(hipEventSynchronize(e[EV_PER_STEP - 1]));
        for (size_t j = 0; j + 1 < EV_PER_STEP; j++) {
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, e[j], e[j + 1]));
            ms_steps[i * (EV_PER_STEP - 1) + j] = t;
        }
    }
    *n_steps = (int)n;
    s->ev_used = 0;
    return CFNMPC_OK;
}

int cfnmpc_get_profile_kernels(cfnmpc_solver* s, double* ms, int* n_steps) {
    if (!s || !ms || !n_steps) return CFNMPC_EINVAL;
    const size_t n = s->ev_used / EV_PER_STEP;
    std::vector<double> per(n * (EV_PER_STEP - 1) + 1);
    int got = 0;
    const int rc = cfnmpc_get_profile_steps(s, per.data(), (int)n, &got);
    if (rc != CFNMPC_OK) return rc;
    for (size_t j = 0; j + 1 < EV_PER_STEP; j++) {
        double acc = 0.0;
        for (int i = 0; i < got; i++) acc += per[(size_t)i * (EV_PER_STEP - 1) + j];
        ms[j] = got ? acc / got : 0.0;
    }
    *n_steps = got;
    return CFNMPC_OK;
}

int cfnmpc_get_profile(cfnmpc_solver* s, double* ms_linearise, double* ms_qp, int* n_steps) {
    if (!s || !ms_linearise || !ms_qp || !n_steps) return CFNMPC_EINVAL;
    double ms[EV_PER_STEP - 1];
    const int rc = cfnmpc_get_profile_kernels(s, ms, n_steps);
    if (rc != CFNMPC_OK) return rc;
    const double a = ms[0], b = ms[1] + ms[2] + ms[3] + ms[4] + ms[5];
    // overlap: the QP phase comes first (events 0 -> 1..5), then the exposed linearisation (5 -> 6)
    *ms_linearise = s->overlap ? ms[5] : a;
    *ms_qp = s->overlap ? a : b;
    return CFNMPC_OK;
}

#ifdef CFN_PROF
extern "C++" { namespace cfn { void debug_prof_read(unsigned long long* out, int reset);
                               float debug_bench_sweep(const Params& P, int waves, int head, int reps, int which); } }
float cfnmpc_debug_bench_sweep(cfnmpc_solver* s, int waves, int head, int reps, int which) {
    return cfn::debug_bench_sweep(s->P, waves, head, reps, which);
}
extern "C++" { namespace cfn { void debug_dprof_read(unsigned long long* out, int reset); } }
int cfnmpc_debug_dprof(unsigned long long* out, int reset) { (void)hipDeviceSynchronize(); cfn::debug_dprof_read(out, reset); return 0; }
int cfnmpc_debug_prof(unsigned long long* out, int reset) { (void)hipDeviceSynchronize(); cfn::debug_prof_read(out, reset); return 0; }
#endif

#ifdef CFN_DEV
// EXPERIMENT: linearisation + backward factorisation of the start solve, either as the two
// kernels of the product (chunk = 0) or alternating in chunks of `chunk` stages going backward -- linearise stages
// [k, k + chunk), then factorise them (cost-to-go parked between the launches) -- so that the stage blocks might be
// consumed from the L2 / MALL.  `reps` repetitions; *ms = average duration of one pair (HIP events).  Same numbers
// either way (bitwise: the same arithmetic).  Leaves the solver ready for cfnmpc_solve.
int cfnmpc_debug_chunked_pair(cfnmpc_solver* s, int chunk, int reps, double* ms, void* stream) {
    if (!s || chunk < 0 || reps < 1 || !ms) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    hipStream_t st = (hipStream_t)stream;
    RC_TRY(resolve_yuni(s));
    cfn::Params P = s->P;
    if (chunk > 0 && !P.Ppark) {
        int rc = dev_alloc(s, &s->P.Ppark, ((size_t)P.NW + 1) * 13 * 64);
        if (rc != CFNMPC_OK) return rc;
        P.Ppark = s->P.Ppark;
    }
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, st));
    for (int r = 0; r < reps; r++) {
        if (chunk == 0) {
            cfn::launch_linearise(P, s->chunks_all, st);
            cfn::launch_factor_only(P, st);
        } else {
            for (int hi = P.N; hi > 0; hi -= chunk) {
                const int lo = hi - chunk > 0 ? hi - chunk : 0;
                cfn::Params Q = P;
                Q.lin_k0 = lo; Q.lin_k1 = hi; Q.fk_lo = lo; Q.fk_hi = hi;
                // the chunk's intervals spread over as many workgroups as the whole horizon gets normally
                int c = s->chunks_all < hi - lo ? s->chunks_all : hi - lo;
                cfn::launch_linearise(Q, c < 1 ? 1 : c, st);
                cfn::launch_factor_chunk(Q, st);
            }
        }
    }
    HIP_TRY(hipEventRecord(e1, st));
    HIP_TRY(hipEventSynchronize(e1));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *ms = t / reps;
    HIP_TRY(hipGetLastError());
    return CFNMPC_OK;
}

// sums of the start solve's gains, feed-forward terms and Riccati checkpoints (host side, exact order: equal sums for
// bitwise-equal arrays) -- checker of the chunked experiment
int cfnmpc_debug_checksum(cfnmpc_solver* s, double* out3) {
    if (!s || !out3) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    const cfn::Params& P = s->P;
    HIP_TRY(hipDeviceSynchronize());
    const size_t n[3] = {(size_t)P.NW * P.N * cfn::SZ_K, (size_t)P.NW * 4 * P.N * 4, (size_t)P.NW * cfn::N_CHK * cfn::SZ_PP};
    const double* src[3] = {P.KR, P.d, P.Pchk};
    for (int f = 0; f < 3; f++) {
        std::vector<double> h(n[f]);
        HIP_TRY(hipMemcpy(h.data(), src[f], n[f] * 8, hipMemcpyDeviceToHost));
        double acc = 0.0;
        for (size_t i = 0; i < n[f]; i++) acc += h[i] * (double)(1 + (i % 7));
        out3[f] = acc;
    }
    return CFNMPC_OK;
}
#endif   // CFN_DEV

// Start solve, backward half only, for parity tests and timing: mode 1 = k_linearise + k_factor, mode 2 = k_linfactor;
// `reps` repetitions timed with HIP events on `stream` (*ms = average per repetition; may be NULL).
int cfnmpc_debug_start_factor(cfnmpc_solver* s, int mode, int reps, double* ms, void* stream) {
    if (!s || (mode != 1 && mode != 2) || reps < 1) return CFNMPC_EINVAL;
    // k_factor / k_linfactor address the home 4-vectors in the wave-blocked layout (Params.v4b): a partial-condensing solver
    // keeps them instance-major and never runs these kernels -- refuse instead of reading and writing in the wrong layout
    if (s->P.cond_N2 || !s->P.v4b) return CFNMPC_EINVAL;
    if (mode == 2 && (s->P.mpar || s->P.dist || s->P.wtab)) return CFNMPC_EINVAL;   // (k_linfactor: folded model constants, no disturbance, uniform weights)
    DeviceGuard dg(s->device);
    invalidate_sens(s);   // (rewrites KR / Pchk: they no longer belong to the last QP)
    RC_TRY(resolve_yuni(s));
    hipStream_t st = (hipStream_t)stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess) return CFNMPC_EHIP;
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return CFNMPC_EHIP; }
    bool ok = hipEventRecord(e0, st) == hipSuccess;
    for (int r = 0; ok && r < reps; r++) {
        if (mode == 1) {
            cfn::launch_linearise(s->P, s->chunks_all, st);
            cfn::launch_factor_only(s->P, st);
        } else {
            cfn::launch_linfactor(s->P, st);
        }
    }
    float t = 0.f;
    ok = ok && hipEventRecord(e1, st) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&t, e0, e1) == hipSuccess;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (!ok) return CFNMPC_EHIP;
    if (ms) *ms = (double)t / reps;
    HIP_TRY(hipGetLastError());
    s->lin_valid = mode == 1;
    return CFNMPC_OK;
}

// What the start solve's backward sweep leaves behind, decoded into dense arrays in the EXTERNAL state order (host
// pointers, any may be NULL): gains K [B][N][4][13], feed-forward d [B][N][4], cost-to-go checkpoints Pchk [B][6][13][13]
// (stages 4, 8, 12, 16, 24, 32; only those below N are written by the kernels), status [B].
int cfnmpc_debug_get_factor(cfnmpc_solver* s, double* K, double* d, double* Pchk, int* status) {
    if (!s || s->P.cond_N2 || !s->P.v4b) return CFNMPC_EINVAL;   // (as cfnmpc_debug_start_factor)
    DeviceGuard dg(s->device);
    const cfn::Params& P = s->P;
    const size_t NW = P.NW, N = P.N, B = P.B;
    HIP_TRY(hipDeviceSynchronize());
    if (K) {
        std::vector<double> h(NW * N * cfn::SZ_K);
        HIP_TRY(hipMemcpy(h.data(), P.KR, h.size() * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < B; i++)
            for (size_t k = 0; k < N; k++) {
                const double* kb = h.data() + ((i / 4) * N + k) * cfn::SZ_K;
                for (int l = 0; l < 13; l++)
                    for (int a = 0; a < 4; a++) K[((i * N + k) * 4 + a) * 13 + cfn::ext_of(l)] = kb[(l * 4 + (i % 4)) * 4 + a];
            }
    }
    if (d) {
        std::vector<double> h(NW * 4 * N * 4);
        HIP_TRY(hipMemcpy(h.data(), P.d, h.size() * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < B; i++)
            for (size_t k = 0; k < N; k++)
                for (int a = 0; a < 4; a++)
                    d[(i * N + k) * 4 + a] = h[P.v4b ? (((i / 4) * N + k) * 4 + i % 4) * 4 + a : (i * N + k) * 4 + a];
    }
    if (Pchk) {
        std::vector<double> h(NW * cfn::N_CHK * cfn::SZ_PP);   // (packed triangle, cfnmpc_ws.hpp: pchk_at)
        HIP_TRY(hipMemcpy(h.data(), P.Pchk, h.size() * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < B; i++)
            for (int c = 0; c < cfn::N_CHK; c++) {
                if (cfn::chk_stage(c) >= (int)N) continue;   // no kernel fills a checkpoint at or behind the horizon's end: the caller's block stays untouched
                const double* pb = h.data() + ((i / 4) * cfn::N_CHK + c) * cfn::SZ_PP;
                for (int j = 0; j < 13; j++)
                    for (int r = 0; r < 13; r++)
                        Pchk[((i * cfn::N_CHK + c) * 13 + cfn::ext_of(r)) * 13 + cfn::ext_of(j)] = pb[cfn::pchk_at(j, (int)(i % 4), r)];
            }
    }
    if (status) HIP_TRY(hipMemcpy(status, P.status, B * sizeof(int), hipMemcpyDeviceToHost));
    return CFNMPC_OK;
}

#ifdef CFN_DEV
// development experiment (tools/sub_fleet_emul.py): the parts of one fused RTI step on separate streams.
// part 1: k_linfactor; part 2: everything behind it + the swap of the iterate buffers; flags bit 0: k_forward_half
int cfnmpc_debug_solve_part(cfnmpc_solver* s, int part, int flags, void* stream) {
    if (!s || s->P.fused != 1 || s->P.lbs) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    hipStream_t st = (hipStream_t)stream;
    if (part == 1) cfn::launch_linfactor(s->P, st);
    else {
        cfn::Params Q = s->P;
        Q.forward_half = flags & 1;
        cfn::launch_qp_start(Q, st, nullptr, true);
        cfn::launch_qp_ipm(Q, st);
        std::swap(s->P.xit, s->P.xitn);
        std::swap(s->P.uit, s->P.uitn);
        s->parity ^= 1;
    }
    HIP_TRY(hipGetLastError());
    return CFNMPC_OK;
}
#endif   // CFN_DEV

int cfnmpc_debug_linearise(cfnmpc_solver* s, void* stream) {
    if (!s) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    invalidate_sens(s);   // (rewrites AR / BR / b: they no longer belong to the last QP)
    cfn::launch_linearise(s->P, s->chunks_all, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    s->lin_valid = true;
    return CFNMPC_OK;
}

int cfnmpc_debug_get_linearisation(cfnmpc_solver* s, double* A, double* Bm, double* b) {
    // Decodes the row-distributed stage blocks (AR, BR, b) into dense arrays in the EXTERNAL
    // state order: A [B][N][13][13], Bm [B][N][13][4], b [B][N][13].
    if (!s || !A || !Bm || !b) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    const cfn::Params& P = s->P;
    const size_t NW = ((size_t)P.NW / 16 + 1) * 16, N = P.N, B = P.B;   // (whole groups of 16 blocks)
    std::vector<double> ha(NW * N * cfn::SZ_A), hb(NW * N * cfn::SZ_B), hv(NW * N * cfn::SZ_V13);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(ha.data(), P.AR, ha.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hb.data(), P.BR, hb.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hv.data(), P.b, hv.size() * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < B; i++) {
        const size_t w = i / 4, q = i % 4;
        for (size_t k = 0; k < N; k++) {
            const size_t bs = ((w / 16) * N + k) * 16 + w % 16;   // [group of 16 blocks][stage][block of the group]
            const double* ab = ha.data() + bs * cfn::SZ_A;
            const double* bb = hb.data() + bs * cfn::SZ_B;
            const double* vb = hv.data() + bs * cfn::SZ_V13;
            double* Ad = A + (i * N + k) * 169;
            double* Bd = Bm + (i * N + k) * 52;
            for (int r = 0; r < 13; r++) {  // internal row / column indices
                for (int cc = 0; cc < 13; cc++) {
                    double val;
                    if (cc < 3) val = (r == cc) ? 1.0 : 0.0;
                    else {
                        const int sl = cc - 3;
                        val = r < cfn::ar_n(sl) ? ab[4 * cfn::ar_pre(sl) + q * cfn::ar_n(sl) + r] : 0.0;
                    }
                    Ad[cfn::ext_of(r) * 13 + cfn::ext_of(cc)] = val;
                }
                for (int a = 0; a < 4; a++) Bd[cfn::ext_of(r) * 4 + a] = bb[(a * 4 + q) * 13 + r];
                b[(i * N + k) * 13 + cfn::ext_of(r)] = vb[q * 13 + r];
            }
        }
    }
    return CFNMPC_OK;
}

int cfnmpc_debug_get_condensed(cfnmpc_solver* s, int block, double* H, double* D, int* m_out) {
    if (!s || !H || !D || !s->P.cond_N2 || block < 0 || block >= s->P.cond_N2) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    const cfn::Params& P = s->P;
    cfn::launch_linearise(P, s->chunks_all, nullptr);
    cfn::launch_pcond(P, nullptr);
    HIP_TRY(hipDeviceSynchronize());
    const int m = cfn::cond_len(P, block), mu = 4 * m, w = cfn::cond_w(m);
    const size_t slot = cfn::cb_size(cfn::cond_mmax(P)), B = P.B;
    std::vector<double> h(slot);
    // internal -> external order of the 13 state entries of z = (dU, dx, 1) and of the rows of D
    auto zext = [&](int i) { return (i >= mu && i < mu + 13) ? mu + cfn::ext_of(i - mu) : i; };
    for (size_t i = 0; i < B; i++) {
        HIP_TRY(hipMemcpy(h.data(), P.cb + (i * P.cond_N2 + block) * slot, slot * sizeof(double), hipMemcpyDeviceToHost));
        double* Hi = H + i * (size_t)w * w;
        double* Di = D + i * (size_t)13 * w;
        for (int r = 0; r < w; r++)
            for (int c = 0; c <= r; c++) {
                const double v = h[(size_t)r * (r + 1) / 2 + c];
                Hi[zext(r) * w + zext(c)] = v;
                Hi[zext(c) * w + zext(r)] = v;
            }
        const double* d = h.data() + cfn::cond_tri(w);
        for (int r = 0; r < 13; r++)
            for (int c = 0; c < w; c++) Di[cfn::ext_of(r) * w + zext(c)] = d[r * w + c];
    }
    if (m_out) *m_out = m;
    return CFNMPC_OK;
}

int cfnmpc_debug_get_viol(cfnmpc_solver* s, double* viol) {   // largest bound violation of the unconstrained minimiser (0: feasible)
    if (!s || !viol) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(viol, s->P.viol, (size_t)s->P.B * sizeof(double), hipMemcpyDeviceToHost));
    return CFNMPC_OK;
}

int cfnmpc_debug_get_head(cfnmpc_solver* s, int* head) {
    if (!s || !head) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(head, s->P.head, (size_t)s->P.B * sizeof(int), hipMemcpyDeviceToHost));
    return CFNMPC_OK;
}

// Work-list counts of the last step's constrained-QP phase (host array of four ints): constrained rows the compaction listed |
// rows listed for the interior-point fall-back (fleets that compact them: >= 16 S instances; else 0) | listed rows with heads of
// more than 16 stages | LATE rows of a split forward sweep (first violation behind stage 24, appended to the list by part two).
int cfnmpc_debug_get_list_counts(cfnmpc_solver* s, int* counts) {
    if (!s || !counts) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    HIP_TRY(hipDeviceSynchronize());
    int h[64];
    HIP_TRY(hipMemcpy(h, s->P.nipm, sizeof h, hipMemcpyDeviceToHost));
    counts[0] = h[0]; counts[1] = s->P.ipm_listed ? h[cfn::NI_LISTED] : 0; counts[2] = h[cfn::NI_LONG16]; counts[3] = s->P.fwd_split ? h[cfn::NI_LATE] : 0;
    return CFNMPC_OK;
}

// Whether the start solve's factorisation reads every instance's reference row once (1: cfnmpc_set_yref found rows 1 .. N - 1 equal
// to row 0 bit for bit in every instance; 0: some row differs, or another writer filled the references).  Waits for a detection
// that is still on its way, as the next step would.
int cfnmpc_debug_get_yref_uniform(cfnmpc_solver* s, int* uniform) {
    if (!s || !uniform) return CFNMPC_EINVAL;
    DeviceGuard dg(s->device);
    RC_TRY(resolve_yuni(s));
    *uniform = s->P.yuni;
    return CFNMPC_OK;
}

}  // extern "C"
