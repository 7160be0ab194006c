// cfnmpc_sqp.h -- the full SQP solve (include/cfnmpc.h: cfnmpc_solve_sqp) per solver, in steps: what cfnmpc_solve_sqp
// (cfnmpc_api.cpp) runs for one solver and cfnmpc_fleet_solve_sqp (cfnmpc_fleet.cpp) interleaves over a fleet's buckets.
// Internal to the library; DESIGN.md section 5.11.
#pragma once
#include "../../include/cfnmpc.h"

namespace cfn {
// CFNMPC_EINVAL for the overlapped development mode, max_iter < 1, tolerances <= 0 or not finite
int sqp_check_args(const cfnmpc_solver* s, int max_iter, double tol_step, double tol_eq, double tol_ineq);
// validates, takes the tolerances and clears the counters of open rows (enqueued on `stream`)
int sqp_begin(cfnmpc_solver* s, int max_iter, double tol_step, double tol_eq, double tol_ineq, void* stream);
// enqueues the next SQP iteration on `stream`: the RTI step, k_sqp_check (k_sqp_ls in a globalised solve), the read-back of the count of open rows
int sqp_iterate(cfnmpc_solver* s, void* stream);
// waits for the last enqueued iteration (one event); *open = rows not yet done after it
int sqp_wait(cfnmpc_solver* s, unsigned* open);
// iterations enqueued since sqp_begin
int sqp_iterations(const cfnmpc_solver* s);
// globalisation (cfnmpc_set_sqp_globalization / cfnmpc_get_sqp_ls_stats): the setting is read by the next sqp_begin
int sqp_set_globalization(cfnmpc_solver* s, int mode, double eta, double reduction, double alpha_min);
int sqp_get_ls_stats(cfnmpc_solver* s, double* alpha, double* mu, int* n_short, int* n_fail, int on_device, void* stream);
int sqp_get_stats(cfnmpc_solver* s, int* status, int* sqp_iter, double* res, int on_device, void* stream);
}  // namespace cfn
