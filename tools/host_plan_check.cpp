// host_plan_check.cpp -- stand-alone check of crazyflie_nmpc_amd/csrc/cfnmpc_plan.hpp (resolve_plan: the option check of
// cfnmpc_create and the choice of the kernel structure): plain C++, no GPU, no HIP call.  A table of
// (options, fleet size, horizon, SIMDs of the device) -> the plan or the refusal: the defaults by fleet size, both sides of every
// threshold of choose_kernels, the horizon limits and the refusals documented in include/cfnmpc.h.  Meant for the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host_plan_check.cpp -o host_plan_check
//   ./host_plan_check
// (make -C crazyflie_nmpc_amd/csrc host_plan_check; tests/test_host_plan_cpu.py builds and runs it the same way).  Built WITHOUT
// CFN_DEV: the product's as_passes values.
#include <cmath>
#include <cstdio>

#include "../crazyflie_nmpc_amd/csrc/cfnmpc_plan.hpp"

namespace {

int failures = 0;

// the values of cfnmpc_default_opts (cfnmpc_api.cpp; this program links no library) at horizon N
cfnmpc_opts opts(int N = 50) {
    static const double W[CFNMPC_NY] = {120.0, 100.0, 100.0, 1e-3, 1e-3, 1e-3, 1e-3, 0.7, 1.0, 4.0, 1e-5, 1e-5, 10.0, 0.06, 0.06, 0.06, 0.06};
    cfnmpc_opts o = {};
    o.struct_size = (int)sizeof(cfnmpc_opts);
    o.N = N;
    o.dt = 0.75 / 50;
    for (int i = 0; i < CFNMPC_NY; i++) o.W[i] = W[i];
    for (int i = 0; i < CFNMPC_NYN; i++) o.WN[i] = 50.0 * W[i];
    o.u_min = 0.0; o.u_max = 22.0; o.tol = 1e-8; o.max_iter = 50; o.tau = 0.995; o.thr0 = 1.0; o.lam0_min = 1e-2; o.mu0_scale = 0.1;
    o.active_horizon = 1; o.ah_margin = 0.10; o.ah_extra = 4; o.active_set = 1;
    o.ipm_clip_viol = 2.0; o.ipm_clip_margin = 0.05; o.as_skip_viol = 4.0;
    return o;
}
template <typename F>
cfnmpc_opts with(cfnmpc_opts o, F set) { set(o); return o; }
#define WITH(N, stmt) with(opts(N), [](cfnmpc_opts& o) { stmt; })

cfn::Plan resolved(int line, const cfnmpc_opts& o, int batch, int simds) {
    cfn::Plan p;
    if (cfn::resolve_plan(o, batch, simds, 0, &p) != CFNMPC_OK) { std::printf("FAILED line %d: refused\n", line); failures++; }
    return p;
}
// accepted, with this structure (as_passes in the internal encoding: 0 monolithic, -2 solves + commit)
void plan_is(int line, const cfnmpc_opts& o, int batch, int simds, int forward_rg, int as_passes, int as_dense, int fwd_split, int ipm_listed) {
    const cfn::Plan p = resolved(line, o, batch, simds);
    if (p.forward_rg != forward_rg || p.as_passes != as_passes || p.as_dense != as_dense || p.fwd_split != fwd_split || p.ipm_listed != ipm_listed ||
        p.wants_side_streams != as_dense || p.as_grid != 2 * simds || p.as_sparse_max != simds || p.ab16 != 1) {
        std::printf("FAILED line %d: forward_rg %d as_passes %d as_dense %d fwd_split %d ipm_listed %d side streams %d as_grid %d as_sparse_max %d\n", line,
                    p.forward_rg, p.as_passes, p.as_dense, p.fwd_split, p.ipm_listed, p.wants_side_streams, p.as_grid, p.as_sparse_max);
        failures++;
    }
}
// refused, and nothing written into the plan
void refused(int line, const cfnmpc_opts& o, int batch, int simds = 1024) {
    cfn::Plan p;
    p.as_grid = -77;
    if (cfn::resolve_plan(o, batch, simds, 0, &p) != CFNMPC_EINVAL || p.as_grid != -77) { std::printf("FAILED line %d: not refused\n", line); failures++; }
}
#define PLAN_IS(...) plan_is(__LINE__, __VA_ARGS__)
#define REFUSED(...) refused(__LINE__, __VA_ARGS__)
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

}  // namespace

int main() {
    const int S = 1024;   // MI355X: 256 compute units x 4 SIMDs
    //                          forward_rg  as_passes  as_dense  fwd_split  ipm_listed
    // ---- the defaults by fleet size, N = 50: one row per distinct plan
    PLAN_IS(opts(), 4096, S,         1,        -2,        1,        0,         0);
    PLAN_IS(opts(), 8192, S,         0,        -2,        1,       24,         0);
    PLAN_IS(opts(), 16384, S,        0,        -2,        1,       24,         1);
    PLAN_IS(opts(), 20480, S,        0,        -2,        0,        0,         1);
    PLAN_IS(opts(), 65536, S,        0,         0,        0,        0,         1);
    CHECK(resolved(__LINE__, opts(), 8192, S).chunks_all == 8);     // 128 groups x 8 chunks = one round of 1024 workgroups
    CHECK(resolved(__LINE__, opts(), 65536, S).chunks_all == 1);    // 1024 groups fill the device by themselves
    {
        const cfn::Plan p = resolved(__LINE__, opts(), 8192, S);
        CHECK(p.chunks_list == 10 && p.clist_chunks == 10 && p.fused == 0 && p.cond_N2 == 0 && p.cond_M == 0 && p.cond_rem == 0 && p.v4b == 1);
        CHECK(p.active_horizon == 1 && p.active_set == 1 && p.as_warm == 0 && p.use_graph == 0 && p.reinit_failed == 0 && p.overlap == 0);
    }
    // ---- both sides of every threshold of choose_kernels
    PLAN_IS(opts(), 6 * S - 1, S,    1,        -2,        1,        0,         0);   // 6 S: row-group sweep | split matrix-free sweep
    PLAN_IS(opts(), 6 * S, S,        0,        -2,        1,       24,         0);
    PLAN_IS(opts(30), 8 * S - 1, S,  1,        -2,        1,        0,         0);   // 8 S where the split cannot run (N < 40): row-group | unsplit matrix-free
    PLAN_IS(opts(30), 8 * S, S,      0,        -2,        1,        0,         0);
    PLAN_IS(opts(), 16 * S - 1, S,   0,        -2,        1,       24,         0);   // 16 S: fall-back rows compacted
    PLAN_IS(opts(), 16 * S, S,       0,        -2,        1,       24,         1);
    PLAN_IS(opts(), 18 * S - 1, S,   0,        -2,        1,       24,         1);   // 18 S: the dense structure (and the split sweep with it) ends
    PLAN_IS(opts(), 18 * S, S,       0,        -2,        0,        0,         1);
    PLAN_IS(opts(40), 20 * S - 1, S, 0,        -2,        0,        0,         1);   // 20 S, N <= 40: solves + commit | monolithic
    PLAN_IS(opts(40), 20 * S, S,     0,         0,        0,        0,         1);
    PLAN_IS(opts(41), 20 * S, S,     0,        -2,        0,        0,         1);   // ... N > 40: not yet
    PLAN_IS(opts(41), 36 * S - 1, S, 0,        -2,        0,        0,         1);   // 36 S, N > 40
    PLAN_IS(opts(41), 36 * S, S,     0,         0,        0,        0,         1);
    PLAN_IS(opts(), 36 * S - 1, S,   0,        -2,        0,        0,         1);
    PLAN_IS(opts(), 36 * S, S,       0,         0,        0,        0,         1);
    // ---- a device of another size: the thresholds move with its SIMDs
    PLAN_IS(opts(), 6 * 256 - 1, 256, 1,       -2,        1,        0,         0);
    PLAN_IS(opts(), 6 * 256, 256,    0,        -2,        1,       24,         0);
    PLAN_IS(opts(), 16 * 256, 256,   0,        -2,        1,       24,         1);
    PLAN_IS(opts(), 36 * 256, 256,   0,         0,        0,        0,         1);
    // ---- horizons
    PLAN_IS(opts(39), 8192, S,       0,        -2,        1,        0,         0);   // the split sweep needs 40 stages
    PLAN_IS(opts(40), 8192, S,       0,        -2,        1,       24,         0);
    REFUSED(opts(4), 4096);
    CHECK(resolved(__LINE__, opts(5), 4096, S).clist_chunks == 5);
    CHECK(resolved(__LINE__, opts(4096), 4096, S).clist_chunks == 10);
    REFUSED(opts(4097), 4096);
    // partial condensing: 0 and N are "off"; blocks of at most ten stages
    CHECK(resolved(__LINE__, WITH(50, o.cond_N2 = 50), 4096, S).cond_N2 == 0 && resolved(__LINE__, WITH(50, o.cond_N2 = 50), 4096, S).v4b == 1);
    {
        const cfn::Plan p = resolved(__LINE__, WITH(50, o.cond_N2 = 5), 4096, S);    // ceil(50 / 5) = 10
        CHECK(p.cond_N2 == 5 && p.cond_M == 10 && p.cond_rem == 0 && p.v4b == 0 && p.fwd_split == 0 && p.fused == 0);
        const cfn::Plan q = resolved(__LINE__, WITH(50, o.cond_N2 = 6), 4096, S);
        CHECK(q.cond_N2 == 6 && q.cond_M == 8 && q.cond_rem == 2 && q.v4b == 0);
    }
    REFUSED(WITH(51, o.cond_N2 = 5), 4096);                                          // ceil(51 / 5) = 11
    REFUSED(WITH(50, o.cond_N2 = -1), 4096);
    REFUSED(WITH(50, o.cond_N2 = 51), 4096);
    // ---- explicit requests that are honoured
    PLAN_IS(WITH(50, o.as_passes = -1), 4096, S,  1,  0,  0,  0,  0);                // monolithic kernel: no dense structure, no split
    PLAN_IS(WITH(50, o.as_passes = -1), 8192, S,  0,  0,  0,  0,  0);
    PLAN_IS(WITH(50, o.as_passes = -3), 65536, S, 0, -2,  0,  0,  1);
    PLAN_IS(WITH(50, o.as_dense = 1), 65536, S,   0, -2,  1, 24,  1);                // selects the solves + commit structure
    PLAN_IS(WITH(50, o.as_dense = -1), 7000, S,   1, -2,  0,  0,  0);                // (no dense structure: the row-group sweep until 8 S)
    PLAN_IS(WITH(50, o.forward_split = 1), 4096, S, 0, -2, 1, 24, 0);                // takes the matrix-free sweep with it
    PLAN_IS(WITH(50, o.forward_split = -1), 8192, S, 0, -2, 1, 0, 0);
    PLAN_IS(WITH(50, o.forward_sweep = 1), 4096, S, 0, -2, 1, 24, 0);
    PLAN_IS(WITH(50, o.forward_sweep = 2), 65536, S, 1, 0, 0, 0, 1);
    PLAN_IS(WITH(50, o.as_warm = 1), 8192, S,     0, -2,  0,  0,  0);                // the warm start: no dense structure
    CHECK(resolved(__LINE__, WITH(50, o.as_warm = 1), 8192, S).as_warm == 1);
    CHECK(resolved(__LINE__, WITH(50, o.as_warm = 1; o.active_set = 0), 8192, S).as_warm == 0);
    {
        const cfn::Plan p = resolved(__LINE__, WITH(50, o.start_solve = 2), 4096, S);   // fused: matrix-free sweep and monolithic kernel at any size
        CHECK(p.fused == 1 && p.forward_rg == 0 && p.as_passes == 0 && p.as_dense == 0 && p.fwd_split == 0);
        const cfn::Plan q = resolved(__LINE__, WITH(50, o.start_solve = 3), 8192, S);   // validation: the structure stays, the sweep is not split
        CHECK(q.fused == 2 && q.forward_rg == 0 && q.as_passes == -2 && q.as_dense == 1 && q.fwd_split == 0);
        const cfn::Plan g = resolved(__LINE__, WITH(50, o.step_graph = 1; o.reinit_failed = 7), 8192, S);
        CHECK(g.use_graph == 1 && g.reinit_failed == 1);
    }
    // ---- the refusals documented in include/cfnmpc.h
    REFUSED(WITH(50, o.as_passes = -2), 4096);    // (development build only)
    REFUSED(WITH(50, o.as_passes = 1), 4096);
    REFUSED(WITH(50, o.as_passes = 12), 4096);
    REFUSED(WITH(50, o.as_passes = -4), 4096);
    REFUSED(WITH(50, o.as_passes = 13), 4096);
    REFUSED(WITH(50, o.as_dense = 1; o.start_solve = 2), 8192);
    REFUSED(WITH(50, o.as_dense = 1; o.as_warm = 1), 8192);
    REFUSED(WITH(50, o.as_dense = 1; o.active_set = 0), 8192);
    REFUSED(WITH(50, o.as_dense = 1; o.as_passes = -1), 8192);
    REFUSED(WITH(50, o.as_dense = 2), 8192);
    REFUSED(WITH(50, o.as_dense = -2), 8192);
    REFUSED(WITH(39, o.forward_split = 1), 8192);
    REFUSED(WITH(50, o.forward_split = 1; o.forward_sweep = 2), 8192);
    REFUSED(WITH(50, o.forward_split = 1; o.start_solve = 2), 65536);
    REFUSED(WITH(50, o.forward_split = 1; o.start_solve = 3), 8192);
    REFUSED(WITH(50, o.forward_split = 1), 20480);                 // a fleet at which the dense structure is not chosen
    REFUSED(WITH(50, o.forward_split = 1; o.as_dense = -1), 8192);
    REFUSED(WITH(50, o.forward_split = 1; o.cond_N2 = 10), 8192);
    REFUSED(WITH(50, o.forward_split = 2), 8192);
    REFUSED(WITH(50, o.forward_sweep = 3), 8192);
    REFUSED(WITH(50, o.forward_sweep = -1), 8192);
    REFUSED(WITH(50, o.start_solve = 2; o.forward_sweep = 2), 65536);
    REFUSED(WITH(50, o.start_solve = 2; o.as_passes = -3), 65536);   // "as_passes other than 0 / -1" ...
    CHECK(resolved(__LINE__, WITH(50, o.start_solve = 2; o.as_passes = -1), 65536, S).fused == 1);   // ... and -1 itself is served
    REFUSED(WITH(50, o.start_solve = 2; o.cond_N2 = 10), 65536);
    REFUSED(WITH(50, o.start_solve = 3; o.cond_N2 = 10), 65536);
    REFUSED(WITH(50, o.start_solve = 4), 8192);
    REFUSED(WITH(50, o.start_solve = -1), 8192);
    REFUSED(WITH(50, o.W[0] = -1.0), 8192);       // a negative state weight
    REFUSED(WITH(50, o.W[13] = 0.0), 8192);       // a zero input weight
    REFUSED(WITH(50, o.W[5] = std::nan("")), 8192);
    REFUSED(WITH(50, o.WN[12] = std::nan("")), 8192);
    CHECK(resolved(__LINE__, WITH(50, o.W[3] = 0.0; o.WN[3] = 0.0), 8192, S).as_dense == 1);   // (Q may be semi-definite)
    REFUSED(WITH(50, o.tau = 1.0), 8192);
    REFUSED(WITH(50, o.ah_margin = 0.5), 8192);
    REFUSED(WITH(50, o.tol = 0.0), 8192);
    REFUSED(WITH(50, o.dt = 0.0), 8192);
    REFUSED(WITH(50, o.u_max = o.u_min), 8192);
    REFUSED(WITH(50, o.max_iter = -1), 8192);
    REFUSED(WITH(50, o.ipm_clip_margin = 0.5), 8192);
    REFUSED(opts(), 0);
    // ---- the two open items of ADVICE.md on option handling, AS THEY ARE TODAY: fixing one is an edit of its row
    // ADVICE.md, "forward_split=1 ... A mixed-horizon fleet ... now fails as a whole": the N = 30 bucket refuses the option
    REFUSED(WITH(30, o.forward_split = 1), 8192);
    // ADVICE.md, "as_dense=1 with as_passes=-3 and cond_N2>0 is accepted": against the header, with side streams the condensed
    // solver never uses (PLAN_IS checks wants_side_streams == as_dense)
    PLAN_IS(WITH(50, o.as_dense = 1; o.as_passes = -3; o.cond_N2 = 10), 8192, S, 0, -2, 1, 0, 0);
    CHECK(resolved(__LINE__, WITH(50, o.as_dense = 1; o.as_passes = -3; o.cond_N2 = 10), 8192, S).cond_M == 5);

    if (failures) { std::printf("host_plan_check: %d FAILED\n", failures); return 1; }
    std::printf("host_plan_check ok\n");
    return 0;
}
