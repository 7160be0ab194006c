/* cfnmpc.h -- batch C-ABI of the MI355X-native Crazyflie SQP-RTI solve engine (libcfnmpc.so).
 *
 * This is the batch superset of the reference's generated-solver boundary.
 * One `cfnmpc_solver` owns B independent NMPC instances (the reference owns exactly one, as
 * process globals: crazyflie_controller/src/acados_mpc.cpp:76-82).  The acados-named drop-in
 * (acados_create / acados_solve / ocp_nlp_*_set / ocp_nlp_out_get) lives in
 * include/acados_solver_crazyflie.h and is this engine with B = 1.
 *
 * Conventions
 *   - plain C, no torch / hip types in signatures; `stream` is a hipStream_t passed as void*
 *     (NULL = the default stream);
 *   - all arrays are FP64, AoS in the reference node's layouts:
 *       x  : [B][13]  = xq yq zq qw qx qy qz vbx vby vbz wx wy wz   (acados_mpc.cpp:117-131)
 *       u  : [B][4]   = w1..w4 [kRPM]                               (acados_mpc.cpp:133-138)
 *       yref   : [B][N][17], yref_e : [B][13]                        (acados_mpc.cpp:584-594)
 *   - `on_device`: 0 (CFNMPC_ON_HOST) host memory, copied synchronously; 2 (CFNMPC_ON_HOST_ASYNC) host memory,
 *     transfer only enqueued on `stream`; any other value: device memory of the solver's GPU (no copy through
 *     the host).  A fleet (cfnmpc_fleet_*) takes the value 2 as host memory too but completes the transfer before it
 *     returns, as with 0;
 *   - every call returns 0 on success, a negative CFNMPC_E* code otherwise; solver *status*
 *     per instance follows acados: 0 success, 2 max. iterations, 4 QP failure.
 *   - a solver (or fleet) lives on the HIP device that is current when it is created; later calls
 *     may be made with any device current (they select the solver's device for their duration);
 *   - there is NO CPU fallback: if no HIP device is usable, cfnmpc_create fails.
 */
#ifndef CFNMPC_H
#define CFNMPC_H

#ifdef __cplusplus
extern "C" {
#endif

#define CFNMPC_NX 13
#define CFNMPC_NU 4
#define CFNMPC_NY 17
#define CFNMPC_NYN 13

#define CFNMPC_OK 0
#define CFNMPC_EINVAL (-1)  /* bad argument                              */
#define CFNMPC_EHIP (-2)    /* HIP runtime error / no device             */
#define CFNMPC_ENOMEM (-3)  /* device allocation failed                  */

/* values of the `on_device` argument of the array setters / getters */
#define CFNMPC_ON_HOST 0        /* host pointer; the call returns when the transfer is complete                       */
#define CFNMPC_ON_DEVICE 1      /* device pointer of the solver's GPU (any non-zero value other than 2 historically)   */
#define CFNMPC_ON_HOST_ASYNC 2  /* host pointer; the transfer is only ENQUEUED on `stream`: the caller keeps the array
                                   alive and synchronises the stream before it reads (getters) or reuses (setters) it --
                                   what cfnmpc_multi_* uses to overlap the I/O of its shards                            */

#define CFNMPC_INIT_ACADOS 0 /* x_k = [0,0,0,1,0..], u_k = 0 (generate_c_code.py:135) */
#define CFNMPC_INIT_HOVER 1  /* x_k = current x0, u_k = hover speed                                      */

typedef struct cfnmpc_solver cfnmpc_solver;

/* ABI guard.  cfnmpc_opts has grown with every round; a caller built against an older header (or a hand-written binding
 * that stops short of the last field) must be refused instead of being written past:
 *   - CFNMPC_ABI_VERSION changes whenever cfnmpc_opts or a signature below changes; cfnmpc_abi_version() returns the
 *     LIBRARY's value, cfnmpc_opts_size() its sizeof(cfnmpc_opts);
 *   - cfnmpc_default_opts_v(opts, sizeof *opts) fills `opts` only if the caller's size is the library's (CFNMPC_EINVAL
 *     otherwise, nothing written) -- what C callers and bindings should use; CFNMPC_DEFAULT_OPTS(&o) spells it;
 *   - every cfnmpc_opts starts with its own size (set by cfnmpc_default_opts*), and cfnmpc_create / cfnmpc_fleet_create /
 *     cfnmpc_multi_create* refuse (CFNMPC_EINVAL) an object whose struct_size is not the library's. */
#define CFNMPC_ABI_VERSION 9

/* Replaces the constants baked into the generated solver by
 * crazyflie_controller/scripts/crazyflie_full_model/generate_c_code.py:41-146. */
typedef struct cfnmpc_opts {
    int struct_size;     /* sizeof(cfnmpc_opts) as the filler saw it (ABI guard above); do not change             */
    int N;               /* horizon length, generate_c_code.py:42 (50); 5 <= N <= 4096 (FP64 Riccati: with an
                            iterate far from the reference over the whole horizon the costate grows with N and
                            the stationarity residual with it -- 1e-12 at N = 50, 2e-10 at 200, 3.5e-7 at 4096) */
    double dt;           /* shooting interval Tf/N, generate_c_code.py:41-42 (0.015)       */
    double W[CFNMPC_NY]; /* diag of stage weight W, generate_c_code.py:63-84               */
    double WN[CFNMPC_NYN]; /* diag of terminal weight W_e = 50 Q, generate_c_code.py:109   */
    double u_min, u_max; /* input box, generate_c_code.py:133-134 (0, 22)                  */
    double tol;          /* QP: max-norm tolerance on all residuals (1e-8)                 */
    int max_iter;        /* QP: interior-point iteration cap (50)                          */
    double tau;          /* QP: fraction to the boundary (0.995)                           */
    double thr0;         /* QP: slack floor of the starting point (1.0)                    */
    double lam0_min;     /* QP: complementarity floor of the starting point (1e-2)         */
    double mu0_scale;    /* QP: starting complementarity = max(lam0_min, mu0_scale * largest
                            bound violation of the unconstrained minimiser) (0.1)          */
    int active_horizon;  /* QP: 1 = interior-point sweeps only over the head of the horizon
                            whose inputs can saturate; the unconstrained tail keeps its
                            Riccati feedback law and is verified afterwards (exact); 0 = all
                            N stages in every sweep (default 1)                              */
    double ah_margin;    /* active horizon: an unconstrained input closer to a bound than this
                            fraction of (u_max - u_min) counts as 'tight' (0.10)              */
    int ah_extra;        /* active horizon: stages added after the last tight stage (4)       */
    int active_set;      /* QP: 1 (default) = solve the box-constrained QP by a primal-dual active-set
                            iteration first: guess the active input bounds from the unconstrained
                            minimiser, solve the equality-constrained QP (one Riccati factorisation
                            with the active inputs fixed), check signs of the multipliers and bounds
                            of the free inputs, repeat until the set is stationary -- which proves
                            the KKT conditions of the strictly convex QP, i.e. the exact solution
                            (typically 1-3 solves instead of 5-10 interior-point iterations).  Falls
                            back to the interior-point iteration if the set does not settle within
                            12 solves.  0 = interior point only (the reference's QP method class).
                            cfnmpc_get_stats reports active-set solves + interior-point iterations. */
    int forward_sweep;   /* start solve, forward sweep: 1 = matrix-free, one instance per lane (dx+ = A dx + B du + b
                            as the directional derivative of the RK4 map: fewest bytes, B / 64 wavefronts);
                            2 = on the stored (A, B, b), four instances per wavefront (16 x more wavefronts, a
                            shorter dependent chain per stage: faster while the fleet is too small to fill the
                            GPU); 0 (default) = by fleet size in waves per SIMD (2 below 6 S instances, S = the device's
                            SIMD count, 1024 on MI355X: measured cross-over against the split matrix-free sweep, profiles/r05_forward_split.md).  Same results to
                            rounding.                                                                        */
    int cond_N2;         /* QP: partial condensing (PARTIAL_CONDENSING_HPIPM, generate_c_code.py:140; acados'
                            qp_solver_cond_N, which the generator leaves at its default): 0 or N (default 0) =
                            none -- the Riccati sweeps run over the N original stages; 0 < cond_N2 < N =
                            the N stages are regrouped into cond_N2 blocks of consecutive stages (the first
                            N mod cond_N2 one stage longer; at most 10 stages per block), the interior states
                            of each block are eliminated exactly (`pcond`: a QP with cond_N2 stages, 13
                            states, 4 x block-length inputs), that QP is solved by the Riccati recursion with
                            one dense Cholesky factorisation per block -- interior point on the same
                            condensed blocks for the instances whose unconstrained minimiser leaves the box
                            -- and the solution is expanded through the original stage dynamics.  Same primal
                            solution (strictly convex QP); active_set / active_horizon do not apply.
                            Measured slower than the uncondensed path at every N2:
                            an option for parity with the reference's solver plan, not the default.        */
    int step_graph;      /* 1: cfnmpc_solve replays the launches of an RTI step from a captured hipGraph (one per
                            parity of the two iterate buffers; re-captured after cfnmpc_set_weights / _set_box)
                            instead of launching its 7-8 kernels one by one;
                            steps timed with cfnmpc_set_profiling are launched individually.  0 (default): the
                            kernels already run back to back (18 us of gaps per step at 4096 instances), the
                            graph saves about half of that.                          */
    int as_passes;       /* QP, active_set = 1: how the active-set solves of the constrained instances are scheduled.
                            -1: one monolithic kernel on a wave-blocked compact copy (four instances per wavefront stay
                            together until the slowest has settled, been rolled out and verified in-wave);
                            -3: the same kernel's solves only, followed by a COMMIT kernel: new iterate = the start
                            solve's candidate + delta -- head stages element-wise from the solve's own du / dx, the tail
                            through the closed loop of the unconstrained feedback law, whose inputs are verified against
                            the box there (rows whose tail leaves it are solved again over a longer head);
                            0 (default): -3 below 36 S instances (20 S for N <= 40; S = the device's SIMD count, 1024 on MI355X),
                            -1 beyond -- measured on MI355X, profiles/r04_thresholds.md, DESIGN.md section 5.5.  Same solves in
                            either mode; results agree to rounding.  Any other value: CFNMPC_EINVAL (round 3's level-synchronous
                            passes and instance-contiguous store, -2 / 1..12, were slower at every fleet size and live in the
                            development build only since ABI 9). */
    double ipm_clip_viol; /* QP, interior point: CLIPPED START when the unconstrained minimiser leaves the box by more than
                            this many box widths (2.0; 0 = never).  From such a point (vehicles far from their iterate's
                            trajectory: ~100 kRPM outside and more) the infeasible start spends 30 - 60 iterations at tiny
                            step lengths; instead the iteration starts inside the box -- inputs clipped to a margin of
                            ipm_clip_margin of the width -- with multipliers that absorb the gradient of the condensed QP
                            there (one forward + one backward costate sweep) and a complementarity floor scaled by it.
                            Captured fall-back QPs: 63 -> 22 iterations, none at the cap any more; ordinary QPs are
                            better served by the infeasible start (5 against 8 iterations), hence the threshold.          */
    double ipm_clip_margin; /* ... 0.05                                                                                   */
    double as_skip_viol; /* QP, active_set = 1: instances whose unconstrained minimiser leaves the box by more than this many
                            box widths skip the active-set iteration and go straight to the interior point (4.0; 0 = never).
                            Measured on the engine's closed loops at 2x / 3x the bench's disturbances: the iteration settles
                            for 68 - 71 % of the instances between 2 and 4 widths, 14 - 15 % between 4 and 8, 1 - 2 % beyond --
                            twelve futile solves per instance otherwise.                                                 */
    int reinit_failed;   /* 1: an instance whose previous RTI step ended in status 4 (QP failure: the factorisation around its
                            iterate is not positive definite / not finite) restarts the next step from x_k = its current x0,
                            u_k = the input reference of its stage, instead of re-linearising around the same iterate and failing
                            the same way for good.  0 (default): the reference's behaviour -- the node ignores the status and keeps
                            the iterate (acados_mpc.cpp:611-616).                                                        */
    int start_solve;     /* start solve (linearisation + backward Riccati factorisation of the unconstrained QP):
                            1 = two kernels with the stage blocks (A, B, b) stored in between (k_linearise writes 162 doubles
                            per instance and stage, k_factor reads them back -- half of the bytes an RTI step moves);
                            2 = FUSED (k_linfactor): the factorisation's wavefront linearises each stage itself on its way
                            backward (every lane integrates one sensitivity column, the columns reach the row form through
                            the LDS tile of the W transpose) and (A, B, b) never touch HBM; the constrained instances alone
                            are re-linearised straight into the compact store of their QP kernels (k_linearise_clist);
                            3 = validation: the fused kernel for the factorisation, the stored blocks for everything behind it;
                            0 (default) = 1: measured on MI355X the fused kernel takes the step's HBM traffic from 17.8 to 8.0 GB
                            and is bound by its vector instructions instead (k_linfactor 2.85 - 2.99 ms against 2.70 - 2.87 ms for
                            the pair).  2 is refused (CFNMPC_EINVAL) together with what reads the stored
                            blocks: cond_N2, forward_sweep = 2, as_passes other than 0 / -1; it switches the
                            automatic choices to the matrix-free forward sweep and the monolithic active-set kernel, and a solver
                            that is given per-stage boxes later runs the stored-block kernels while they are set.  Same results
                            to rounding (tests/test_gpu_linfactor.py). */
    int as_warm;         /* QP, active_set = 1: 1 = WARM START of the active set.  An instance whose previous RTI step ended in a
                            settled active-set solve starts its first solve from the union of that solve's final set and the
                            violations of today's unconstrained minimiser, instead of the violations alone (consecutive steps of
                            a constrained vehicle share most of their active set, and the reference never shifts its iterate --
                            acados_mpc.cpp:581-611 -- so the classes are taken stage for stage).  Exactness is untouched: whatever
                            the start, the iteration ends in a stationary classification, i.e. the KKT point of the strictly
                            convex QP; only the number of solves changes.  The state (4 N bytes + a flag per instance) is cleared by
                            cfnmpc_init_iterate / cfnmpc_set_iterate.  Read by the monolithic and the solves + commit kernels
                            (as_passes 0 / -1 / -3); the level-synchronous variants ignore it.  Default 0: see DESIGN.md section 5.5
                            for the measured solve histograms. */
    int as_dense;        /* QP, active_set = 1, solves + commit structure (as_passes 0 auto / -3): rows whose head is at most 16
                            stages long (99 % of the constrained rows of the bench workload) are solved on the HEAD-CONDENSED DENSE
                            QP -- the same active-set iteration on H = R + Gamma' Q Gamma of the head (4 x head inputs, the tail's
                            cost-to-go as terminal weight), inverted once per row, every solve then a system of the size of the
                            active set (csrc/cfnmpc_asdense.hip) -- instead of one Riccati factorisation + forward sweep over the
                            head per solve.  Same classification rule, same solve counts, same solutions to rounding (the reference's
                            own plan condenses too: PARTIAL_CONDENSING_HPIPM, generate_c_code.py:140).  1 = on (selects the solves +
                            commit structure), -1 = off, 0 (default) = by measurement.  Scalar box only
                            (while per-stage boxes are set the monolithic kernels run).  An explicit 1 that cannot be honoured --
                            together with as_warm, active_set = 0, cond_N2, start_solve = 2 or as_passes other than 0 / -3 -- is
                            refused (CFNMPC_EINVAL), not dropped. */
    int forward_split;   /* start solve, matrix-free forward sweep inside the as_dense structure: 1 = in TWO launches -- stages [0, 24)
                            with the classification of the instances over that window, the compaction, and stages [24, N) of every
                            instance BESIDE the constrained rows' kernels (their heads of at most 24 stages read nothing behind
                            stage 24; rows with longer heads follow the second part on its stream) -- half of the sweep's 50-stage
                            latency chain leaves the critical path of a small fleet's step.  An instance that is feasible over the
                            first window and leaves the box behind it joins the list late and is solved with the retry kernel.
                            Same SOLUTIONS (candidates bitwise; a row's head class and its violation measure -- what as_skip_viol
                            and ipm_clip_viol compare -- come from the first window only, so a row may take another route than
                            with the single launch: a retry over a longer head after the tail verification, the active-set
                            iteration instead of the interior point or the other way round; either route ends at the QP's one
                            solution, to its own accuracy).  -1 = off, 0 (default) = by measurement.  An explicit 1 that cannot
                            be honoured -- outside the as_dense structure, N < 40, forward_sweep = 2, cond_N2, start_solve 2 / 3 -- is
                            refused (CFNMPC_EINVAL). */
} cfnmpc_opts;

void cfnmpc_default_opts(cfnmpc_opts *opts);   /* unchecked: the caller's struct MUST be this header's */
int cfnmpc_default_opts_v(cfnmpc_opts *opts, int sizeof_opts);
int cfnmpc_opts_size(void);
int cfnmpc_abi_version(void);
#define CFNMPC_DEFAULT_OPTS(o) cfnmpc_default_opts_v((o), (int)sizeof(cfnmpc_opts))

/* acados_create() / acados_free() equivalents (acados_mpc.cpp:225,418) for B instances on the
 * calling thread's current HIP device. */
int cfnmpc_create(cfnmpc_solver **out, int batch, const cfnmpc_opts *opts);
int cfnmpc_free(cfnmpc_solver *s);
int cfnmpc_batch(const cfnmpc_solver *s);
int cfnmpc_horizon(const cfnmpc_solver *s);
/* bytes of device workspace held by the solver */
unsigned long long cfnmpc_workspace_bytes(const cfnmpc_solver *s);

/* ocp_nlp_constraints_model_set(.., 0, "lbx"/"ubx", x0) equivalent (acados_mpc.cpp:581-582) */
int cfnmpc_set_x0(cfnmpc_solver *s, const double *x0, int on_device, void *stream);
/* ocp_nlp_cost_model_set(.., k, "yref", ..) for k = 0..N (acados_mpc.cpp:590-594).  Behind the copy the solver checks on the device
 * whether every vehicle's rows 0 .. N-1 are one row (a setpoint): the start solve then reads it once per vehicle and step, with the
 * same results bit for bit.  The call itself does not wait for that verdict; the first step that follows does, once. */
int cfnmpc_set_yref(cfnmpc_solver *s, const double *yref, const double *yref_e, int on_device, void *stream);
/* Reference windows generated ON THE DEVICE with the reference node's state machine
 * (NMPC::iteration, acados_mpc.cpp:430-516) -- replaces the host-side fill of yref_sign and the
 * N+1 ocp_nlp_cost_model_set("yref") calls per step (:590-594) for fleets:
 *   mode[i] = 0 Regulation (rows = des_xyz[i], identity attitude, zeros, uss), 1 Tracking (rows
 *   iter[i]..iter[i]+N of traj, then ++iter[i]; becomes 2 once iter[i] >= n_rows - N, keeping the
 *   previous window for that step), 2 Position_Hold (xyz of the last trajectory row).
 * All pointers are DEVICE pointers: traj [n_rows][17] (may be NULL with n_rows = 0 if no instance
 * tracks), mode [B] / iter [B] (int, updated in place), des_xyz [B][3]. */
int cfnmpc_set_yref_windows(cfnmpc_solver *s, const double *traj, int n_rows, int *mode, int *iter,
                            const double *des_xyz, double uss, void *stream);
/* The windows in force, in the public order (the sibling of cfnmpc_set_yref): yref [B][N][17], yref_e [B][13]; either pointer may be
 * NULL, not both. */
int cfnmpc_get_yref(cfnmpc_solver *s, double *yref /*[B][N][17] or NULL*/, double *yref_e /*[B][13] or NULL*/, int on_device, void *stream);
/* Device-side polynomial trajectory references, one per vehicle.  A small LIBRARY of piecewise 7th-order
 * polynomial trajectories in the format of crazyflie_demo/scripts/ (figure8.csv; uav_trajectory.py evaluates it), a trajectory id
 * and a PLACEMENT row per vehicle, and one kernel that writes every vehicle's reference window straight into yref / yref_e: the
 * polynomial and its first three derivatives at each stage time, mapped through the flatness relations of this model.  No RTI
 * kernel, launch, option or default changes: a solver that never calls these runs the same step bit for bit.
 *   cfnmpc_set_poly_library: HOST arrays, validated as a whole before anything changes (every number finite, every duration > 0,
 *     first[0] = 0 and strictly increasing: CFNMPC_EINVAL otherwise).  Limits: CFNMPC_POLY_MAX_TRAJ trajectories and
 *     CFNMPC_POLY_MAX_PIECES pieces in total, refused beyond (CFNMPC_EINVAL).  n_traj = 0 or a NULL pointer clears the library.
 *     Replacing the library resets the assigned ids outside [0, n_traj) to -1.  The tables and the assignment are allocated at the
 *     first call of the feature (cfnmpc_workspace_bytes counts them from then on); the copy is complete on return.
 *   cfnmpc_set_poly_assignment: traj [B], id of every vehicle's trajectory or -1 = none; place [B][CFNMPC_NPLACE] or NULL =
 *     [0, 1, 0, 0, 0, 0] for every vehicle.  Host arrays are validated (id in [-1, n_traj), time_scale finite and > 0, the rest
 *     finite; CFNMPC_EINVAL changes nothing); device arrays are taken as they are: the kernel treats an id outside [0, n_traj) as -1
 *     and a time_scale that is not a positive finite number as 1, and never indexes the library with an unchecked value.
 *   cfnmpc_set_yref_poly: for every vehicle with an id >= 0 the stage rows k = 0 .. N-1 and the terminal row k = N (first 13
 *     columns) at the fleet times t + k dt (cfnmpc_opts.dt).  Vehicles with id -1 keep what cfnmpc_set_yref /
 *     cfnmpc_set_yref_windows gave them bit for bit: the three sources can be mixed in one fleet.  Its effect on solver state is
 *     that of cfnmpc_set_yref_windows; the values are written in place (captured step graphs keep replaying); asynchronous on
 *     `stream`.  CFNMPC_EINVAL without a library, for t not finite and for unknown flags.
 *   cfnmpc_eval_poly: the same evaluation into the caller's arrays for rows k = 0 .. n_stages-1 (all of them stage rows), without
 *     touching yref: flat [B][n_stages][CFNMPC_NFLAT] = pos, vel, acc, yaw, omega after placement -- the fields of
 *     uav_trajectory.py's TrajectoryOutput, with its own omega_z = z_b[2] dyaw --, rows [B][n_stages][17] in the public order
 *     (either may be NULL, not both).  Rows of vehicles with id -1 are NaN.  Host arrays go through the staging buffer of
 *     cfnmpc_get_sens_x0, in chunks of rows.
 * Rules (crazyflie_nmpc_amd/trajectories.py: poly_rows follows them operation for operation; every operation is rounded on its
 * own, so the host twin and the kernel choose the same piece bit for bit):
 *   local time    tau = ((t + k dt) - t_start) / time_scale; D = the trajectory's duration, accumulated piece by piece in table order.
 *   piece         uav_trajectory.py:97-105: the first piece with tau < cum + duration (the last one otherwise), piece time tau - cum.
 *   outside       tau < 0: held at the start.  tau >= D with CFNMPC_POLY_LOOP: tau -= D floor(tau / D) (a negative result: 0), then
 *                 the lookup; without the flag: held at the end, the last piece at its own duration.  A held row has position and yaw
 *                 of that point, zero derivatives, attitude qz(yaw), zero velocities and rates, the vehicle's hover speed.
 *   derivatives   pos / yaw, vel / dyaw, acc, jerk by Horner's rule on the coefficient lists (i + 1) p[i + 1], taken one to three
 *                 times (Polynomial.derivative); the d-th derivative is divided by time_scale^d.
 *   placement     pos, vel, acc and jerk are rotated by Rz(yaw0); yaw += yaw0; pos += (ox, oy, oz).
 *   flatness      with g0 and Ct / mq of the vehicle's parameter row (cfnmpc_set_model_params; the nominal constants otherwise):
 *                 thr = acc + (0, 0, g0), z_b = thr / |thr|, x_w = (cos yaw, sin yaw, 0), c = z_b x x_w, y_b = c / |c|, x_b = y_b x z_b,
 *                 h_w = (jerk - (jerk . z_b) z_b) / |thr|, omega = (-h_w . y_b, h_w . x_b, omega_z).  The evaluator's omega_z =
 *                 z_b[2] dyaw is an approximation (figure8.csv, yaw = 0: up to 0.11 rad/s from the attitude's body rate); flat
 *                 returns it, the rows carry the exact one, omega_z = -x_b . (h_w x x_w + z_b x dx_w) / |c| with
 *                 dx_w = dyaw (-sin yaw, cos yaw, 0): the quaternion rows of this model's ODE are then the reference's own qdot.
 *   attitude      [x_b y_b z_b] = Rz(yaw) Rx(phi) Ry(theta) with zl = Rz(-yaw) z_b, theta = asin(zl_x), phi = atan2(-zl_y, zl_z);
 *                 q = qz(yaw) qx(phi) qy(theta) (w, x, y, z): continuous in yaw, no division, no sign choice.
 *   the rest      v_b = [x_b y_b z_b]' vel; four equal speeds sqrt(|thr| / (4 Ct / mq)) = sqrt(mq |thr| / (4 Ct)).  Torque-consistent
 *                 rotor speeds need the snap and the yaw acceleration and are out of scope.
 *   guard         a stage with thr_z <= 0.1 g0 or |c| < 1e-3 is a LEVEL row: attitude qz(yaw), v_b = Rz(yaw)' vel, omega = (0, 0, dyaw)
 *                 (in flat too), hover speed.  A reference never contains NaN or Inf.
 *   CFNMPC_POLY_KINEMATIC   the helix-style row [pos, 1, 0, 0, 0, 0 x 6, hover speed x 4] from the same lookup and placement (flat is
 *                 unchanged): the two references through one call.
 * Disturbance rows are ignored: the reference is that of the undisturbed vehicle, as with cfnmpc_init_iterate's hover mode. */
#define CFNMPC_POLY_NC 33      /* one piece: duration, x^0..x^7, y^0..y^7, z^0..z^7, yaw^0..yaw^7 (ascending powers; figure8.csv) */
#define CFNMPC_NPLACE 6        /* placement row: t_start [s], time_scale (> 0), ox, oy, oz [m], yaw0 [rad] */
#define CFNMPC_NFLAT 13        /* pos[3], vel[3], acc[3], yaw, omega[3]: the fields of uav_trajectory.py's TrajectoryOutput */
#define CFNMPC_POLY_LOOP 1      /* flags */
#define CFNMPC_POLY_KINEMATIC 2
#define CFNMPC_POLY_MAX_TRAJ 1024
#define CFNMPC_POLY_MAX_PIECES 8192
int cfnmpc_set_poly_library(cfnmpc_solver *s, const double *pieces /*[first[n_traj]][33], HOST*/, const int *first /*[n_traj+1], HOST*/,
                            int n_traj, void *stream);
int cfnmpc_set_poly_assignment(cfnmpc_solver *s, const int *traj /*[B], -1 = none*/, const double *place /*[B][6] or NULL*/,
                               int on_device, void *stream);
int cfnmpc_set_yref_poly(cfnmpc_solver *s, double t, int flags, void *stream);
int cfnmpc_eval_poly(cfnmpc_solver *s, double t, int n_stages, int flags, double *flat /*[B][n_stages][13] or NULL*/,
                     double *rows /*[B][n_stages][17] or NULL*/, int on_device, void *stream);
/* ocp_nlp_cost_model_set(.., k, "W", ..) equivalent (acados_mpc.cpp:596-602, compiled out by
 * SET_WEIGHTS 0 in the reference): diagonal stage / terminal weights for ALL instances and
 * stages; either pointer may be NULL (unchanged).  State weights must be >= 0 (the reference's
 * dynamic_reconfigure ranges start at 0.0, config/crazyflie_params.cfg), input weights > 0; the
 * arrays are validated as a whole before anything is changed. */
int cfnmpc_set_weights(cfnmpc_solver *s, const double *W /*[17]*/, const double *WN /*[13]*/);
/* ocp_nlp_constraints_model_set(.., k, "lbu"/"ubu", ..) equivalent (acados_mpc.cpp:605-608, compiled
 * out by FIXED_U0 0 at :111) for the case the engine supports: ONE input box [u_min, u_max] for all
 * inputs, stages and instances (generate_c_code.py:133-134).  Takes effect at the next
 * cfnmpc_solve.  Per-stage, per-input boxes: cfnmpc_set_box_stages below. */
int cfnmpc_set_box(cfnmpc_solver *s, double u_min, double u_max);
/* Discretisation and cost scaling of the OCP, to match a given acados build.  A bad value returns
 * CFNMPC_EINVAL and changes nothing; both setters invalidate captured step graphs, as cfnmpc_set_weights does.
 *   cfnmpc_set_erk_steps: num_steps = M classic RK4 steps of dt / M per shooting interval (acados sim_method_num_steps),
 *     1 <= M <= CFNMPC_ERK_STEPS_MAX, default 1.  The linearisation, the matrix-free forward sweep and the SQP residual
 *     (cfnmpc_solve_sqp: res_eq) use Phi_M.  M > 1 is refused beside start_solve 2 or 3 (the fused start solve integrates one
 *     step per interval); every other option works with it.  cfnmpc_erk_steps returns M (CFNMPC_EINVAL for NULL).
 *   cfnmpc_set_cost_scaling: the stage cost of stages 0..N-1 is multiplied by stage_scale, the terminal cost by
 *     terminal_scale (both finite and > 0; default 1, 1).  It scales whatever W / WN are set, before and after later
 *     cfnmpc_set_weights calls: the effective weights are stage_scale * W and terminal_scale * WN.  Newer acados scales
 *     by (dt, 1). */
#define CFNMPC_ERK_STEPS_MAX 8
int cfnmpc_set_erk_steps(cfnmpc_solver *s, int num_steps);
int cfnmpc_erk_steps(const cfnmpc_solver *s);
int cfnmpc_set_cost_scaling(cfnmpc_solver *s, double stage_scale, double terminal_scale);
/* Per-instance model parameters: p [B][CFNMPC_NP], one row per instance in the order of
 * export_ode_model.py:33-42, [g0, mq, Ixx, Iyy, Izz, Cd, Ct, l] (l = arm length, in place of dq).  The nominal row is
 *   [9.8066, 33e-3, 1.395e-5, 1.395e-5, 2.173e-5, 7.9379e-06, 3.25e-4, 0.0325]
 * and gives bit for bit the constants the default kernels fold in.  The linearisation, the matrix-free forward sweeps, the
 * SQP residual (res_eq), cfnmpc_init_iterate's hover mode (sqrt(mq g0 / (4 Ct)) per instance) use each instance's row.
 *   cfnmpc_set_model_params: every entry finite and > 0, else CFNMPC_EINVAL and nothing changes (device arrays are copied
 *     to the host once to be checked).  p = NULL returns the solver to the folded constants.  Refused (CFNMPC_EINVAL) beside
 *     start_solve 2 or 3 (the fused start solve integrates with the folded constants).  Switching between NULL and
 *     parameters invalidates captured step graphs; new values over old ones are copied in place on `stream` and complete
 *     before the call returns, so the next solve or graph replay reads them.
 *   cfnmpc_get_model_params: the rows in force (the nominal row for every instance while none are set). */
#define CFNMPC_NP 8
int cfnmpc_set_model_params(cfnmpc_solver *s, const double *p /*[B][CFNMPC_NP] or NULL*/, int on_device, void *stream);
int cfnmpc_get_model_params(cfnmpc_solver *s, double *p /*[B][CFNMPC_NP]*/, int on_device, void *stream);
/* Per-instance external disturbance: d [B][CFNMPC_ND], one row per instance,
 *   d = [ax, ay, az | alx, aly, alz]:  a_w = d[0:3] an acceleration in the WORLD frame [m/s^2] (wind, a payload),
 *                                      al_b = d[3:6] an angular acceleration in the BODY frame [rad/s^2] (a torque bias),
 *   v_b' += R(q)' a_w,   w' += al_b      (R(q) the matrix of p' = R(q) v_b).
 * The linearisation, the matrix-free forward sweeps, the SQP residual and line search and cfnmpc_eval_nlp use each instance's row
 * on top of its model parameters (cfnmpc_set_model_params; nominal if none are set).  cfnmpc_init_iterate's hover mode and the
 * hover speed of a parameter row stay disturbance-blind: they are the hover of the undisturbed vehicle.
 *   cfnmpc_set_disturbance: made to be called every control step (the rows come from an observer, cfnmpc_estimate_disturbance):
 *     asynchronous on `stream`.  Host arrays are validated (every entry finite, any sign; else CFNMPC_EINVAL and nothing changes)
 *     and staged (CFNMPC_ON_HOST returns when the transfer is complete); DEVICE arrays are taken as they are, without a copy to the
 *     host and without synchronisation -- one small kernel.  New values over old ones are written in place: captured step graphs
 *     stay valid and replay with them; a sensitivity evaluation and a kept linearisation are invalidated, as by
 *     cfnmpc_set_model_params.  d = NULL returns the solver to the kernels in force before (folded constants, or per-instance
 *     parameters while those are set); switching between NULL and rows invalidates captured step graphs.  Refused
 *     (CFNMPC_EINVAL) beside start_solve 2 or 3 and beside cond_N2 > 0 (no disturbed twins of the fused start solve and of the
 *     condensed sweep); cfnmpc_debug_start_factor mode 2 is refused while rows are set.
 *   cfnmpc_get_disturbance: the rows in force (zeros while none are set). */
#define CFNMPC_ND 6
int cfnmpc_set_disturbance(cfnmpc_solver *s, const double *d /*[B][CFNMPC_ND] or NULL*/, int on_device, void *stream);
int cfnmpc_get_disturbance(cfnmpc_solver *s, double *d /*[B][CFNMPC_ND]*/, int on_device, void *stream);
/* Per-instance cost weights: W [B][17] and WN [B][13], one row per instance in the external order of
 * cfnmpc_opts.W / .WN, unscaled -- the effective weights of row i are stage_scale * W[i] and terminal_scale * WN[i], and a later
 * cfnmpc_set_cost_scaling rescales the rows in force.  The reference tunes the 17 Wdiag_* values per vehicle through each node's
 * dynamic_reconfigure server (acados_mpc.cpp:199-203, 274-290, 334-350).
 *   cfnmpc_set_weights_batch: every entry finite, state and terminal weights >= 0, input weights > 0; the arrays are validated as
 *     a whole before anything changes (CFNMPC_EINVAL, the previous weights stay in force; device arrays are copied to the host once
 *     to be checked).  W = NULL and WN = NULL returns to the uniform weights, i.e. the values of cfnmpc_opts or of the last
 *     cfnmpc_set_weights.  One NULL part: that part keeps what every row has (the uniform values if no rows were set).  While rows
 *     are in force, each part cfnmpc_set_weights is given replaces that part in every row.  Refused (CFNMPC_EINVAL) beside
 *     start_solve 2 or 3 and cond_N2 > 0 (their kernels stage one weight vector per wavefront / workgroup); with rows in force
 *     cfnmpc_debug_start_factor refuses mode 2.  Switching between uniform weights and rows invalidates captured step graphs; new
 *     rows over old ones are copied in place on `stream` and complete before the call returns, so the next solve or graph replay
 *     reads them.  Every change of weights invalidates a sensitivity evaluation; cfnmpc_eval_sens_x0 uses the rows.
 *     cfnmpc_workspace_bytes counts the table (256 bytes per instance, allocated at the first call).
 *     While rows are in force, cfnmpc_set_weights (finite entries only, then) and cfnmpc_set_cost_scaling rewrite the table in
 *     place on the null stream, block until that is done and may return CFNMPC_EHIP; like cfnmpc_set_weights_batch on a stream
 *     other than the solves' own, they must not overlap a solve in flight, which reads the table (without rows both calls only
 *     change the arguments of the next launch, as before).
 *   cfnmpc_get_weights_batch: the unscaled rows in force (the uniform values for every instance while none are set); either
 *     pointer may be NULL. */
int cfnmpc_set_weights_batch(cfnmpc_solver *s, const double *W /*[B][17] or NULL*/, const double *WN /*[B][13] or NULL*/,
                             int on_device, void *stream);
int cfnmpc_get_weights_batch(cfnmpc_solver *s, double *W /*[B][17] or NULL*/, double *WN /*[B][13] or NULL*/,
                             int on_device, void *stream);
/* Per-stage, per-input box: lb, ub [B][N][4] (what "lbu" / "ubu" on INDIVIDUAL stages set in acados -- the reference's
 * FIXED_U0 variant pins stage 0 to the input in flight, lbu = ubu = u1, acados_mpc.cpp:605-608).  lb[i] = ub[i] makes
 * that input an equality (the active-set solves keep it fixed whatever its multiplier's sign; the interior-point
 * fall-back needs lb < ub).  HOST arrays are validated (lb <= ub everywhere, no NaN: CFNMPC_EINVAL, nothing changed); DEVICE
 * arrays are taken as they are -- the caller guarantees lb <= ub (an inverted box ends in status 4 for that vehicle).  The
 * call is atomic: on any failure the previous boxes (both arrays) stay in force.  NULL, NULL returns to the scalar box of
 * cfnmpc_set_box.  Steps with per-stage boxes run
 * the row-group forward sweep and the monolithic QP kernels (instantiated for them); not with cond_N2. */
int cfnmpc_set_box_stages(cfnmpc_solver *s, const double *lb, const double *ub, int on_device, void *stream);

/* Iterate (the persistent nlp_out of acados_mpc.cpp:77): initial guess, save / restore. */
int cfnmpc_init_iterate(cfnmpc_solver *s, int mode, void *stream);
int cfnmpc_set_iterate(cfnmpc_solver *s, const double *x /*[B][N+1][13]*/, const double *u /*[B][N][4]*/, int on_device, void *stream);
int cfnmpc_get_iterate(cfnmpc_solver *s, double *x, double *u, int on_device, void *stream);

/* acados_solve() equivalent (acados_mpc.cpp:611): n_rti consecutive SQP-RTI steps
 * (linearise -> Riccati interior-point QP -> full step) for all B instances, asynchronous on
 * `stream`.  The reference calls it with one step. */
int cfnmpc_solve(cfnmpc_solver *s, int n_rti, void *stream);

/* Full SQP solve (acados' nlp_solver_type = 'SQP', the one alternative the reference's generator names next to SQP_RTI,
 * generate_c_code.py:146-147): iterates every instance to a converged NLP solution.  x0, yref, weights and boxes stay fixed
 * during the solve.  One SQP iteration is exactly one RTI step as cfnmpc_solve runs it (linearise at the iterate, solve the
 * QP, take the full step).  After iteration j every instance not yet done gets
 *   res_step = max-norm of w_j - w_{j-1} over all x_k and u_k -- the STATIONARITY measure of this solve: for the Gauss-Newton
 *              QP with Q, R > 0 the step is zero iff w is a KKT point (it is not acados' res_stat);
 *   res_eq   = max(|x_0 - x0|, max_k |x_{k+1} - Phi(x_k, u_k)|) at w_j, Phi = the engine's RK4 step over dt;
 *   res_ineq = the largest violation of the input box at w_j (the scalar box, or the per-stage boxes while they are set);
 * and is classified: status 4 if the QP of step j failed (the step keeps its iterate; done, sqp_iter = j); else status 0 if
 * res_step <= tol_step, res_eq <= tol_eq and res_ineq <= tol_ineq (done, sqp_iter = j, keeps w_j); else status 2 once
 * j = max_iter.  A QP status 2 (QP iteration cap) does not stop an instance.  A done instance is FROZEN: later iterations
 * still run it through the step's kernels but restore its iterate, so it leaves the solve with w_{sqp_iter}.  The loop ends
 * when every instance is done or after max_iter iterations; *n_iter (may be NULL) = iterations run.  One read of the count
 * of open instances (pinned memory, one event) per iteration; the call synchronises `stream`.  cfnmpc_opts.reinit_failed
 * does not apply inside the solve (failed instances stop instead).  CFNMPC_EINVAL: max_iter < 1, a tolerance <= 0 or not
 * finite, the overlapped preparation of development builds.  cfnmpc_get_stats keeps its meaning: the QP statistics of the
 * LAST executed step (an instance frozen before it included). */
int cfnmpc_solve_sqp(cfnmpc_solver *s, int max_iter, double tol_step, double tol_eq, double tol_ineq,
                     int *n_iter /* iterations run, may be NULL */, void *stream);
/* Per instance, of the last cfnmpc_solve_sqp: status (0 converged, 2 max. iterations, 4 QP failure), sqp_iter (the
 * iteration whose iterate the instance kept) and res [B][3] = res_step, res_eq, res_ineq at that iterate.  Any pointer may
 * be NULL; on_device as everywhere. */
int cfnmpc_get_sqp_stats(cfnmpc_solver *s, int *status, int *sqp_iter, double *res /*[B][3]: step, eq, ineq*/,
                         int on_device, void *stream);

/* Globalisation of cfnmpc_solve_sqp (acados: globalization = MERIT_BACKTRACKING beside nlp_solver_type = SQP; DESIGN.md section
 * 5.17).  CFNMPC_SQP_FULL_STEP (default) is the solve described above.  With CFNMPC_SQP_MERIT_BACKTRACKING every iteration j
 * searches along the step of its QP: w = w_{j-1}, w^ = the QP's candidate, d = w^ - w, per instance
 *   c(v)  = (x_0 - x0, the N defects x_{k+1} - Phi(x_k, u_k), the box violations max(lb - u, 0) + max(u - ub, 0)), c1 = |c|_1;
 *   gd    = sum_k s (W o (y_k - yref_k)).d_k + s_e (W_N o (x_N - yref_e)).d_xN,  dHd = sum_k s W.d_k^2 + s_e W_N.d_xN^2 at w
 *           (the data of cfnmpc_eval_nlp; the cost is a linear least-squares form: J(w + a d) - J(w) = a gd + a^2 dHd / 2);
 *   mu    = 0 at iteration 1; if c1(w) > 0: mu <- max(mu, (gd + dHd / 2) / ((1 - 0.5) c1(w))); it never decreases in a solve;
 *   D     = gd - mu c1(w);
 *   a_t   = reduction^t, t = 0 .. T, T the smallest integer with reduction^T <= alpha_min; the first t with
 *           a_t gd + a_t^2 dHd / 2 + mu (c1(w + a_t d) - c1(w)) <= eta a_t D is accepted (differences only: no trial evaluates
 *           the cost); without one the iteration takes a_T and counts in n_fail.  A NaN fails every comparison.
 * w_j = w + a d (a = 1: the candidate, bit for bit); res_eq and res_ineq are those of w_j; res_step stays |d|_inf, the FULL
 * step of the QP, so that a short step cannot pass for convergence.  An instance whose QP failed (status 4) kept its iterate
 * and is not searched; classification, frozen instances and sqp_iter are those of the full-step solve.
 * cfnmpc_set_sqp_globalization: eta, reduction, alpha_min = 0 select the defaults 1e-4, 0.5, 2^-10.  CFNMPC_EINVAL (nothing
 * changes): a mode other than the two, eta outside (0, 0.5), reduction outside (0, 1), alpha_min outside (0, 1], T > 32.  The
 * setting stays with the solver; cfnmpc_solve_sqp reads it, cfnmpc_solve does not.  cfnmpc_eval_sens_x0 is refused
 * (CFNMPC_EINVAL) after a globalised solve: the last QP belongs to w_{j-1}, not to the iterate the solve left.
 * cfnmpc_get_sqp_ls_stats, of the last cfnmpc_solve_sqp: alpha = step length of the instance's last executed iteration (1 after
 * a full-step solve), mu = its penalty, n_short = its iterations with alpha < 1, n_fail = those without an accepted trial.
 * Any pointer may be NULL, not all; CFNMPC_EINVAL before the first cfnmpc_solve_sqp.  The buffers (two doubles, two ints per
 * instance) are allocated at the first globalised solve (cfnmpc_workspace_bytes counts them from then on). */
#define CFNMPC_SQP_FULL_STEP 0
#define CFNMPC_SQP_MERIT_BACKTRACKING 1
int cfnmpc_set_sqp_globalization(cfnmpc_solver *s, int mode, double eta, double reduction, double alpha_min);
int cfnmpc_get_sqp_globalization(const cfnmpc_solver *s, int *mode, double *eta, double *reduction, double *alpha_min);
int cfnmpc_get_sqp_ls_stats(cfnmpc_solver *s, double *alpha /*[B]*/, double *mu /*[B]*/, int *n_short /*[B]*/,
                            int *n_fail /*[B]*/, int on_device, void *stream);

/* One complete control step from HOST buffers with a single synchronisation -- what the node
 * does per sample (acados_mpc.cpp:581-625: set lbx/ubx, N+1 yref rows, acados_solve(), read u/x):
 * x0 [B][13], yref [B][N][17], yref_e [B][13] in; one RTI step; the whole iterate out
 * (u [B][N][4], x [B][N+1][13]) with status, QP solve count and residual per instance.  The
 * transfers go through pinned staging memory owned by the solver, asynchronously on `stream`,
 * which is synchronised once before returning.  Any output pointer may be NULL. */
int cfnmpc_step_host(cfnmpc_solver *s, const double *x0, const double *yref, const double *yref_e,
                     double *u, double *x, int *status, int *qp_iter, double *res, void *stream);

/* ocp_nlp_out_get(.., stage, "u"/"x", ..) equivalents (acados_mpc.cpp:619-625) */
int cfnmpc_get_u(cfnmpc_solver *s, int stage, double *u /*[B][4]*/, int on_device, void *stream);
int cfnmpc_get_x(cfnmpc_solver *s, int stage, double *x /*[B][13]*/, int on_device, void *stream);
/* status (acados_solve() return value), QP iteration count, nlp_out->inf_norm_res stand-in
 * (max-norm residual of the last QP).  Any pointer may be NULL.
 * qp_iter: 0 = the unconstrained minimiser was feasible; otherwise the number of active-set solves of a row they settled (a row
 * of the large fleets' kernel that was solved AGAIN over a longer head -- its own or a wave-mate's tail had left the box -- counts
 * the solves of all attempts; the later ones start from the previous attempt's final set and take one or two), or
 * the interior-point ITERATIONS of a row that fell back (after 12 unsettled solves, or skipped by as_skip_viol; such a row runs
 * the interior point over all N stages) -- the two ranges overlap (twelve iterations are not twelve solves).  res tells them apart: exactly 0.0 for a row settled by active-set
 * solves (a stationary classification IS the KKT system), the interior point's final residual (> 0, <= tol at status 0)
 * for a row it solved.  These are the statistics of the last executed RTI step, also after cfnmpc_solve_sqp (its per-instance
 * NLP results: cfnmpc_get_sqp_stats). */
int cfnmpc_get_stats(cfnmpc_solver *s, int *status /*[B]*/, int *qp_iter /*[B]*/, double *res /*[B]*/, int on_device, void *stream);

/* Solution sensitivities with respect to the initial state (acados' ocp_nlp_eval_param_sens with field "ex", stage 0; DESIGN.md
 * section 5.14): the Jacobians du_k/dx0 [4][13] and dx_k/dx0 [13][13] of the last QP's solution -- the QP of the latest
 * cfnmpc_solve step or of the last iteration of cfnmpc_solve_sqp -- with its active set held fixed.  An input of the current
 * iterate within act_tol of its lower or upper bound is active (lb == ub: always); an active input has a zero derivative row.
 * A weakly active input (at its bound with a zero multiplier) has no derivative: the result is the one for the set detected.
 * Both axes are in the public state order (xq yq zq qw qx qy qz vbx vby vbz wx wy wz).  A row whose status is 4
 * (cfnmpc_get_stats after a solve, cfnmpc_get_sqp_stats after cfnmpc_solve_sqp) gets NaN in every entry.
 *   cfnmpc_eval_sens_x0: the active set and the gains of the masked Riccati recursion, on `stream`.  Writes nothing that a
 *     solve, getter or option reads; its buffers are allocated at the first call (cfnmpc_workspace_bytes counts them from
 *     then on).  CFNMPC_EINVAL: act_tol not finite or <= 0; no solve yet, or set_weights / set_cost_scaling / set_box /
 *     set_box_stages / set_model_params / set_erk_steps / set_iterate / init_iterate since the last one; cond_N2 > 0 or
 *     start_solve = 2 (no stored blocks).
 *   cfnmpc_get_sens_x0: stages [stage, stage + n_stages) of one forward sweep from stage 0, du [B][n_stages][4][13] and dx
 *     [B][n_stages][13][13] (either may be NULL, not both; du must be NULL if the range includes stage N;
 *     stage + n_stages <= N + 1).  (0, 1) is the feedback gain; (0, N + 1) the whole trajectory.  CFNMPC_EINVAL without an
 *     evaluation since the last solve or data change.  Host arrays go through one staging buffer per solver: with
 *     CFNMPC_ON_HOST_ASYNC, calls that overlap must be made on the same stream.
 *   cfnmpc_get_sens_active: the active set the evaluation used, act [B][N][4]: 0 free, -1 lower, +1 upper. */
int cfnmpc_eval_sens_x0(cfnmpc_solver *s, double act_tol, void *stream);
int cfnmpc_get_sens_x0(cfnmpc_solver *s, int stage, int n_stages, double *du /*[B][n_stages][4][13] or NULL*/,
                       double *dx /*[B][n_stages][13][13] or NULL*/, int on_device, void *stream);
int cfnmpc_get_sens_active(cfnmpc_solver *s, signed char *act /*[B][N][4]*/, int on_device, void *stream);

/* Adjoint solution sensitivities (acados' eval_solution_sens_adjoint for a whole fleet): the gradient of
 * a caller's loss l on the last QP's solution z = (x_0..x_N, u_0..u_{N-1}) with respect to that QP's data, with the active set
 * of cfnmpc_eval_sens_x0 held.  In an RTI step A_k, B_k, b_k belong to the previous iterate, so this is the exact gradient of
 * the RTI map on its active set.  One evaluation = three sweeps over the stored blocks, whatever the number of outputs read.
 *   cfnmpc_eval_adjoint: gx [B][n_gx][13] = dl/dx_k for the stages k < n_gx (<= N + 1), gu [B][n_gu][4] = dl/du_k for k < n_gu
 *     (<= N), public state order; gradients behind are zero, a NULL array is all zero.  Needs a valid cfnmpc_eval_sens_x0 of the
 *     same solve (the one source of the active set and of act_tol): CFNMPC_EINVAL wherever that call is refused or has been
 *     invalidated (no solve, data changed since, cond_N2 > 0, start_solve = 2, a globalised cfnmpc_solve_sqp) and for
 *     n_gx / n_gu outside their ranges.  Device arrays are read on `stream` (keep them until it has passed); host arrays are
 *     copied first.  Writes nothing that a solve, getter or option reads; its buffers are allocated at the first call
 *     (cfnmpc_workspace_bytes counts them from then on).  A row whose status is 4 gets NaN in every output.
 *   cfnmpc_get_adjoint (any output may be NULL), with q_k / r_k the linear cost terms of the QP, b_k its defects:
 *     dl_dx0 [B][13]; dl_dq [B][N + 1][13] and dl_dr [B][N][4] (dl_dr is exactly 0 on active inputs); dl_db [B][N][13];
 *     dl_dbox [B][N][4]: with respect to the bound an active input sits on, exactly 0 on free inputs.
 *   cfnmpc_get_adjoint_cost (any may be NULL): dl_dW [B][17] and dl_dWN [B][13] with respect to the UNSCALED weights
 *     (cfnmpc_get_weights_batch's rows, or the uniform ones: then the row of every vehicle with respect to its own copy);
 *     dl_dyref [B][N][17], dl_dyref_e [B][13].
 * CFNMPC_EINVAL for both getters without an evaluation since the last cfnmpc_eval_sens_x0. */
int cfnmpc_eval_adjoint(cfnmpc_solver *s, const double *gx /*[B][n_gx][13] or NULL*/, int n_gx /*<= N+1*/,
                        const double *gu /*[B][n_gu][4] or NULL*/, int n_gu /*<= N*/, int on_device, void *stream);
int cfnmpc_get_adjoint(cfnmpc_solver *s, double *dl_dx0 /*[B][13]*/, double *dl_dq /*[B][N+1][13]*/, double *dl_dr /*[B][N][4]*/,
                       double *dl_db /*[B][N][13]*/, double *dl_dbox /*[B][N][4]*/, int on_device, void *stream);
int cfnmpc_get_adjoint_cost(cfnmpc_solver *s, double *dl_dW /*[B][17]*/, double *dl_dWN /*[B][13]*/,
                            double *dl_dyref /*[B][N][17]*/, double *dl_dyref_e /*[B][13]*/, int on_device, void *stream);

/* Uncertainty propagation and robust input-bound tightening (zero-order robust optimisation, acados' zoRO custom update;
 * DESIGN.md section 5.21).  A state covariance is carried along the horizon through the closed-loop linearisation of the LAST QP
 * (the "last QP" rule of cfnmpc_eval_sens_x0: its stored blocks A_k, B_k), and every input bound is backed off by a multiple of
 * the standard deviation of the feedback's input correction.  All arrays are in the public state order.
 *   Inputs per instance: Sigma_0 [13][13], symmetric, the covariance of the state estimate at stage 0; W [13][13], symmetric,
 *     the covariance added per shooting interval.  NULL means zero.
 *   Feedback gain K_k in du = -K_k dx (sign and layout of cfnmpc_debug_get_factor's K [B][N][4][13]):
 *     CFNMPC_UNC_GAIN_RICCATI (default): the gains of the last solve's start solve (the feedback law of the unconstrained tail);
 *     CFNMPC_UNC_GAIN_USER: one constant [4][13] per instance, K [B][4][13] (acados zoRO's fdbk_K_mat).
 *   Recursion, with M_k = A_k - B_k K_k:   Sigma_{k+1} = M_k Sigma_k M_k' + W,  k = 0 .. N-1;
 *     backoff beta_{k,a} = sqrt((K_k Sigma_k K_k')_aa), k = 0 .. N-1, a = 0 .. 3 (1 sigma; the tightening applies the multiple).
 *     A row whose status is 4 gets NaN in Sigma, std_x and beta; the tightening leaves its box nominal.
 *   Tightening: lb'_{k,a} = lb_{k,a} + t, ub'_{k,a} = ub_{k,a} - t with t = min(gamma beta_{k,a}, (1 - min_width)(ub - lb) / 2):
 *     the tightened box keeps at least min_width of its nominal width and never inverts.  An equality entry (lb == ub) is left
 *     untouched.  n_clamped [B]: per instance, the entries the clamp limited.
 *   Nominal box: what cfnmpc_set_box or cfnmpc_set_box_stages last set; it is remembered, and every tightening starts from it,
 *     never from a tightened one.  Tightened boxes are in force from the next solve on, as per-stage boxes (the kernels of
 *     cfnmpc_set_box_stages).  gamma = 0, or a later cfnmpc_set_box / cfnmpc_set_box_stages, puts the then-current nominal box
 *     back in force (the scalar route again if it is scalar).  New tightened values are written over old ones in place: captured
 *     step graphs keep replaying; only a switch between the scalar and the per-stage route invalidates them.
 *   cfnmpc_set_uncertainty / cfnmpc_set_uncertainty_gain: HOST arrays are validated (finite; Sigma_0 and W symmetric to 1e-12
 *     of their largest entry with a non-negative diagonal; CFNMPC_EINVAL changes nothing); DEVICE arrays are taken as they are,
 *     one put kernel on `stream` (the rule of cfnmpc_set_disturbance).
 *   cfnmpc_eval_uncertainty: one sweep over [0, N) on `stream`, keeps beta.  Writes nothing that a solve reads.  CFNMPC_EINVAL:
 *     no solve yet; any change of the QP's data since the last solve (whatever invalidates cfnmpc_eval_sens_x0, and set_x0 /
 *     set_yref / set_yref_windows / set_yref_poly); cond_N2 > 0 or start_solve = 2 (no stored blocks).
 *   cfnmpc_get_backoff: beta [B][N][4].  The stored beta stays valid until the next cfnmpc_eval_uncertainty,
 *     cfnmpc_init_iterate or cfnmpc_set_iterate, so cfnmpc_tighten_box may come before or after the set_x0 of the next step.
 *   cfnmpc_get_uncertainty: one sweep over [0, stage + n_stages) writes Sigma [B][n_stages][13][13] and std_x [B][n_stages][13]
 *     (the square roots of its diagonal; either may be NULL, not both; stage + n_stages <= N + 1).  Nothing of Sigma is kept
 *     between calls.  CFNMPC_EINVAL without an evaluation since the last solve or data change.  Host arrays go through the
 *     staging buffer of cfnmpc_get_sens_x0, in chunks of rows.
 *   cfnmpc_tighten_box: CFNMPC_EINVAL without a valid beta, for gamma < 0 and for min_width outside (0, 1].
 * The buffers (tables, beta, nominal-box copy) are allocated at the first call that needs them; cfnmpc_workspace_bytes counts
 * them from then on. */
#define CFNMPC_UNC_GAIN_RICCATI 0
#define CFNMPC_UNC_GAIN_USER 1
int cfnmpc_set_uncertainty(cfnmpc_solver *s, const double *Sigma0 /*[B][13][13] or NULL*/, const double *W /*[B][13][13] or NULL*/,
                           int on_device, void *stream);
int cfnmpc_set_uncertainty_gain(cfnmpc_solver *s, int mode, const double *K /*[B][4][13], mode 1*/, int on_device, void *stream);
int cfnmpc_eval_uncertainty(cfnmpc_solver *s, void *stream);
int cfnmpc_get_backoff(cfnmpc_solver *s, double *beta /*[B][N][4]*/, int on_device, void *stream);
int cfnmpc_get_uncertainty(cfnmpc_solver *s, int stage, int n_stages, double *Sigma /*[B][n_stages][13][13] or NULL*/,
                           double *std_x /*[B][n_stages][13] or NULL*/, int on_device, void *stream);
int cfnmpc_tighten_box(cfnmpc_solver *s, double gamma, double min_width, int *n_clamped /*[B] or NULL*/, int on_device, void *stream);

/* NLP cost, KKT residuals, costates and reduced gradient at the CURRENT iterate w = (x_0..x_N, u_0..u_{N-1}) (DESIGN.md section
 * 5.16), from the data in force now and nothing else: x0, yref / yref_e, the uniform or per-instance weights times the cost
 * scaling (s, s_e), the scalar or per-stage box, the nominal or per-instance model parameters, erk_steps (Phi = that many RK4
 * steps over dt).  It needs no preceding solve, does not depend on the route the QP of a row took, and writes nothing that a
 * solve, getter or option reads.  Per instance:
 *   cost     = sum_{k<N} 1/2 s (y_k - yref_k)' W (y_k - yref_k) + 1/2 s_e (x_N - yref_e)' W_N (x_N - yref_e),  y_k = (x_k, u_k);
 *   pi_N     = s_e W_N (x_N - yref_e),  pi_k = s Q (x_k - yref_k^x) + A_k' pi_{k+1},  A_k = dPhi/dx (x_k, u_k): the costates that
 *              put the x-stationarity of stages 1..N at zero; pi_0 is the multiplier of x_0 = x0;
 *   g_k      = s R (u_k - yref_k^u) + B_k' pi_{k+1},  B_k = dPhi/du: the reduced gradient dJ/du_k along the trajectory;
 *   res_stat = max_{k,a} |u_{k,a} - clip(u_{k,a} - g_{k,a}, lb_{k,a}, ub_{k,a})|, the projected-gradient (natural) residual of the
 *              box: |g| for an input inside the box, zero for an input on a bound (lb = ub included) whose gradient points
 *              outward, continuous in between, no activity tolerance; it folds complementarity in (there is no res_comp);
 *   res_eq   = max(|x_0 - x0|, max_k |x_{k+1} - Phi(x_k, u_k)|),  res_ineq = largest box violation -- the formulas of
 *              cfnmpc_solve_sqp's res_eq / res_ineq.
 * A NaN in the iterate of a row sticks in every result of that row.
 *   cfnmpc_eval_nlp: asynchronous on `stream`.  keep_multipliers = 0 stores cost and the three residuals (4 doubles per
 *     instance); 1 additionally stores pi and g -- their two buffers are allocated at the first such call
 *     (cfnmpc_workspace_bytes counts them from then on: ((B + 3) / 4 + 1) * (544 N + 416) bytes together).
 *   cfnmpc_get_nlp_stats / cfnmpc_get_nlp_multipliers: the LAST evaluation's snapshot (no invalidation tracking: a solve or a
 *     change of data in between does not show).  pi in the public state order.  CFNMPC_EINVAL before any evaluation, for the
 *     multipliers when the last evaluation did not keep them, and when both pointers are NULL. */
int cfnmpc_eval_nlp(cfnmpc_solver *s, int keep_multipliers, void *stream);
int cfnmpc_get_nlp_stats(cfnmpc_solver *s, double *cost /*[B] or NULL*/, double *res /*[B][3]: stat, eq, ineq; or NULL*/,
                         int on_device, void *stream);
int cfnmpc_get_nlp_multipliers(cfnmpc_solver *s, double *pi /*[B][N+1][13] or NULL*/, double *gu /*[B][N][4] or NULL*/,
                               int on_device, void *stream);

/* Output stage of the reference node for the whole fleet, on the device (NMPC::iteration,
 * acados_mpc.cpp:619-670): from the current iterate (u0 = inputs of stage 0, u1 = stage 1, x4 =
 * state of stage 4) it forms what the node publishes per vehicle,
 *   motvel  [B][4] int32 : u0 truncated toward zero -- /crazyflie/acados_motvel, the int32 fields of
 *                          PropellerSpeedsStamped (msg/PropellerSpeedsStamped.msg:2-5, :637-640);
 *   cmd_vel [B][4] double: linear.x = pitch [deg] = +deg(theta), linear.y = roll [deg] = -deg(phi),
 *                          linear.z = thrust PWM = (int)((mean(u1)*1000 - 4070.3)/0.2685) (:421-425),
 *                          angular.z = yaw rate [deg/s] = deg(x4.wz); (phi, theta) from the normalised
 *                          quaternion of x4 with the node's formulas (:384-404, :645-668).
 * motvel may be NULL.  on_device as everywhere. */
int cfnmpc_get_cmd(cfnmpc_solver *s, double *cmd_vel /*[B][4]*/, int *motvel /*[B][4]*/, int on_device, void *stream);

/* Per-phase timing (the role of nlp_out->total_time, acados_mpc.cpp:616): when enabled,
 * cfnmpc_solve brackets its two phases (linearisation, QP) with HIP events on the launch stream;
 * cfnmpc_get_profile waits for them and returns the average durations [ms] over the RTI steps
 * since the last call (at most 4096 steps are timed between two calls), then resets.  */
int cfnmpc_set_profiling(cfnmpc_solver *s, int enable);
int cfnmpc_get_profile(cfnmpc_solver *s, double *ms_linearise, double *ms_qp, int *n_steps);
/* The same timed steps split per kernel group (seven events per step): ms[6] = linearisation | start solve backward
 * (k_factor) | start solve forward (k_forward / k_forward_rg + k_rank) | compaction (k_compact + k_scatter) |
 * active-set kernels (k_as, or the passes + commit + retry) | interior point for what they left (k_ipm_rest / k_ipm).
 * Partial-condensing steps report their phases in ms[0] / ms[5] only.  Resets like cfnmpc_get_profile
 * (call one of the two). */
int cfnmpc_get_profile_kernels(cfnmpc_solver *s, double *ms, int *n_steps);
/* ... and per timed step instead of averaged (the active-set kernels of a step in which a tail check fails take four times the
 * average: a mean hides what a deadline sees): ms_steps [max_steps][6], *n_steps = steps written; resets likewise */
int cfnmpc_get_profile_steps(cfnmpc_solver *s, double *ms_steps, int max_steps, int *n_steps);

/* crazyflie_acados_sim_solve() equivalent, batched (acados_estimator.cpp:573-593):
 * xn = RK4(x, u) over T seconds in `steps` sub-steps.  Stateless. */
int cfnmpc_sim(int batch, const double *x, const double *u, double T, int steps, double *xn, int on_device, void *stream);
/* The same with per-instance model parameters p [batch][CFNMPC_NP] (as cfnmpc_set_model_params): a plant or predictor that
 * differs from the controller's model.  Host arrays are validated (finite, > 0); device arrays are taken as they are. */
int cfnmpc_sim_params(int batch, const double *x, const double *u, const double *p, double T, int steps, double *xn,
                      int on_device, void *stream);
/* ... and with per-instance disturbance rows d [batch][CFNMPC_ND] (as cfnmpc_set_disturbance): the disturbed plant.  p as in
 * cfnmpc_sim_params, or NULL = the nominal row.  Host arrays are validated (d: finite); device arrays are taken as they are. */
int cfnmpc_sim_dist(int batch, const double *x, const double *u, const double *p, const double *d, double T, int steps,
                    double *xn, int on_device, void *stream);
/* Differentiable plant rollouts, solver-free like the calls above.
 *   cfnmpc_sim_rollout: the open-loop rollout xs[:,0] = x0, xs[:,t+1] = Phi(xs[:,t], u[:,t]; p, d), Phi = `steps` classic RK4
 *     steps over T.  Step t has the bits of cfnmpc_sim (p = d = NULL), cfnmpc_sim_params (p alone) or cfnmpc_sim_dist (d set; p or
 *     NULL = the nominal row) for (xs[:,t], u[:,t]).  The single plant step is L = 1.
 *   cfnmpc_sim_rollout_vjp: the gradient of a loss l on that rollout from gxs = dl/dxs (reverse mode through RK4; it reads the
 *     stored xs).  gx0 = dl/dx0 includes gxs[:,0]; gu = dl/du; gp = dl/dp with respect to the public parameter row (p = NULL: at the
 *     nominal row); gd = dl/dd (d = NULL: at the zero row).  gu, gp, gd may be NULL: not computed, the other outputs keep their
 *     bits.  No atomics: two calls agree bit for bit.
 * Any steps >= 1.  Device arrays: one launch on `stream`, no synchronisation.  Host arrays are validated (p: finite, > 0; d: finite)
 * and staged; the call returns when the results are in place.  CFNMPC_EINVAL (nothing written): batch <= 0, L < 1, steps < 1,
 * !(T > 0), a NULL x0 / u / xs / gxs / gx0, host rows that fail the validation. */
int cfnmpc_sim_rollout(int batch, int L, const double *x0 /*[B][13]*/, const double *u /*[B][L][4]*/,
                       const double *p /*[B][CFNMPC_NP] or NULL = nominal*/, const double *d /*[B][CFNMPC_ND] or NULL = none*/,
                       double T, int steps, double *xs /*[B][L+1][13]*/, int on_device, void *stream);
int cfnmpc_sim_rollout_vjp(int batch, int L, const double *xs /*[B][L+1][13], as returned above*/, const double *u,
                           const double *p, const double *d, double T, int steps, const double *gxs /*[B][L+1][13]*/,
                           double *gx0 /*[B][13]*/, double *gu /*[B][L][4] or NULL*/, double *gp /*[B][CFNMPC_NP] or NULL*/,
                           double *gd /*[B][CFNMPC_ND] or NULL*/, int on_device, void *stream);
/* Disturbance observer, stateless, one lane per instance: with x^ = Phi(x_prev, u_prev; p, d) (`steps` RK4 sub-steps over T, the
 * map of cfnmpc_sim_dist) and e = x_meas - x^,
 *   d[0:3] += gain_a / T * R(q_prev) e[7:10],      d[3:6] += gain_w / T * e[10:13]       (d [batch][CFNMPC_ND], in place).
 * Gains in (0, 1], else CFNMPC_EINVAL.  A constant disturbance is a fixed point (plant and model are the same map); gain 1 is
 * dead-beat up to O(T), smaller gains filter measurement noise.  Feed d to cfnmpc_set_disturbance (device arrays: no
 * synchronisation anywhere in the loop).  p [batch][CFNMPC_NP] or NULL = nominal.  The observer needs a full 13-state x_meas and has
 * no noise model and no covariance; cfnmpc_ekf_aug_step below estimates d jointly with the state, from a partial measurement. */
int cfnmpc_estimate_disturbance(int batch, const double *x_prev, const double *u_prev, const double *x_meas, const double *p,
                                double *d, double T, int steps, double gain_a, double gain_w, int on_device, void *stream);

/* Extended Kalman filter step for a fleet, solver-free: the state estimate and its covariance through the RK4 plant above and a
 * measurement of some or all of the 13 states.  Everything in the public state order.  Per instance:
 *   1. Predict.  h = T / steps; the state goes through `steps` classic RK4 sub-steps, the map of cfnmpc_sim (p = d = NULL),
 *      cfnmpc_sim_params (p alone) or cfnmpc_sim_dist (d set; p or NULL = the nominal row): with z = NULL, x_new has that call's
 *      bits.  The covariance goes through the exact derivative of each sub-step, A_s = d x_{s+1} / d x_s at (x_s, u; p, d) -- the
 *      derivative of the discrete RK4 map, not I + h df/dx --: P <- A_s P A_s', s = 0 .. steps - 1; then P^- = P + Q, once per
 *      call (the convention of W in cfnmpc_set_uncertainty: one array serves both).
 *   2. Quaternion sign.  If sum_{j = 3..6, r_j >= 0} z_j x^-_j < 0, z_3 .. z_6 are negated (q and -q are one attitude).
 *   3. Update, sequential, component j = 0 .. 12 in index order, on the current (x, P).  r_j < 0: not measured, skipped.  Else
 *      s = P_jj + r_j, nu = z_j - x_j; if gate > 0 and nu^2 > gate^2 s the component is rejected (counted, nothing changes); else
 *      x_i += P_ij nu / s,  P_ab -= (P_aj P_jb) / s,  nis += nu^2 / s, and it is counted as used.  The product P_aj P_jb is formed
 *      before it meets 1 / s: an exactly symmetric P stays exactly symmetric.  With the diagonal R = diag(r) this is the joint
 *      Kalman update.
 *   4. With CFNMPC_EKF_NORMALIZE_Q, and only in a call with z, q <- q / |q| after the update; P is left as it is.
 *   5. z = NULL (predict only): nis = 0, counts = (0, 0), no normalisation.
 *   6. A NaN in an instance's (device) inputs stays in that instance's outputs and touches no other instance.
 * x_new may be x and P_new may be P: an instance's inputs are read completely before its outputs are written.  nis [B] and
 * counts [B][2] = (used, rejected) may be NULL.  CFNMPC_EINVAL, with nothing written: batch <= 0, steps < 1, !(T > 0), gate negative
 * or not finite, unknown flags, a NULL x / P / u / x_new / P_new, z without r.  Host arrays are validated as a whole before anything
 * runs (x, u, z, r, d finite, r of any sign; P and Q by cfnmpc_set_uncertainty's rule for Sigma0 / W; p finite and > 0), staged,
 * and the call returns when the results are in place.  Device arrays are taken as they are: one launch on `stream`, no
 * synchronisation -- cfnmpc_ekf_step -> cfnmpc_set_x0 -> solve -> get_u never touches the host, and (P_new, Q) are the
 * (Sigma0, W) of cfnmpc_set_uncertainty. */
#define CFNMPC_EKF_NORMALIZE_Q 1   /* flags */
int cfnmpc_ekf_step(int batch,
    const double *x /*[B][13]*/, const double *P /*[B][13][13]*/, const double *u /*[B][4]*/,
    const double *p /*[B][CFNMPC_NP] or NULL = nominal*/, const double *d /*[B][CFNMPC_ND] or NULL = none*/,
    double T, int steps,
    const double *Q /*[B][13][13] or NULL = zero*/,
    const double *z /*[B][13] or NULL = predict only*/, const double *r /*[B][13]; required with z*/,
    double gate, int flags,
    double *x_new /*[B][13]*/, double *P_new /*[B][13][13]*/,
    double *nis /*[B] or NULL*/, int *counts /*[B][2] = used, rejected; or NULL*/,
    int on_device, void *stream);

/* Disturbance-augmented filter step, solver-free: cfnmpc_ekf_step with up to three components of the disturbance row estimated
 * jointly with the state, from the same measurement of some or all of the 13 states.  The augmented vector
 * is a = [x; d[sel[0]], d[sel[1]], d[sel[2]]] (CFNMPC_EKF_NA = 16 entries; the entry of an unused slot, sel[k] = -1, is 0) with the
 * covariance Pa [16][16].  sel [3] is a HOST array in every call.  Every rule of cfnmpc_ekf_step holds without change (the
 * quaternion sign, the sequential update in the order j = 0 .. 12 with its skip on r_j < 0 and its gate test, the product formed
 * before 1 / s, CFNMPC_EKF_NORMALIZE_Q, predict-only semantics, NaN isolation per instance), with x read as a[0:13] and P as Pa;
 * the model is always the disturbed one, the map of cfnmpc_sim_dist(x, u, p, d) (p or NULL = the nominal row).  What is new:
 *   1. Predict.  Per sub-step s, F_s = [[A_s, G_s S], [0, I]] with A_s as in cfnmpc_ekf_step, G_s = d x_{s+1} / d d at
 *      (x_s, u; p, d) -- the exact derivative of the discrete sub-step with respect to the disturbance row -- and S [6][3] the
 *      selector of the slots' columns (a zero column for an unused slot): Pa <- F_s Pa F_s', s = 0 .. steps - 1; d is constant.
 *      Then, once per call, Pa[0:13][0:13] += Q and Pa[13+k][13+k] += Qd[k] for the used slots (Qd: the variance of a random walk
 *      per call; the entry of an unused slot is ignored).  With z = NULL, x_new has the bits of cfnmpc_sim_dist(x, u, p, d) and
 *      d_new the bits of d.
 *   2. Update.  Only the 13 state components are measured: j = 0 .. 12, s = Pa_jj + r_j, nu = z_j - a_j, and for a used component
 *      a_i += Pa_ij nu / s for all 16 i,  Pa_ab -= (Pa_aj Pa_jb) / s for all 16 x 16 (a, b).
 *   3. Output.  x_new = a[0:13]; d_new is d with d_new[sel[k]] = a[13+k] for the used slots, every other component copied bit
 *      for bit; Pa_new; Pxx_new (may be NULL) = Pa_new[0:13][0:13] bit for bit, the Sigma0 of cfnmpc_set_uncertainty.  An unused
 *      slot takes no part: its row of F_s is the unit row and its column of G_s S is zero.
 * x_new may be x, d_new may be d and Pa_new may be Pa.  nis, counts as in cfnmpc_ekf_step.  CFNMPC_EINVAL, with nothing written:
 * what cfnmpc_ekf_step refuses (here x / d / Pa / u / sel / x_new / d_new / Pa_new must not be NULL), and a sel[k] outside
 * -1 .. CFNMPC_ND - 1 or repeated among the used slots.  Host arrays are validated as a whole before anything runs: as in
 * cfnmpc_ekf_step (Pa by the rule for P at size 16), the rows and columns of Pa that belong to unused slots must be zero, Qd finite
 * and >= 0 in the used slots' entries; then staged, and the call returns when the results are in place.  Device arrays are taken
 * as they are: one launch on `stream`, no synchronisation -- cfnmpc_ekf_aug_step -> cfnmpc_set_x0(x_new),
 * cfnmpc_set_disturbance(d_new) -> solve, and (Pxx_new, Q) -> cfnmpc_set_uncertainty never touch the host. */
#define CFNMPC_EKF_NA 16      /* 13 states + 3 disturbance slots */
int cfnmpc_ekf_aug_step(int batch,
    const double *x /*[B][13]*/, const double *d /*[B][CFNMPC_ND]*/, const double *Pa /*[B][16][16]*/,
    const double *u /*[B][4]*/, const double *p /*[B][CFNMPC_NP] or NULL = nominal*/,
    const int *sel /*[3], HOST: slot k estimates d[sel[k]], sel[k] in 0..5 and distinct, or -1 = slot unused*/,
    double T, int steps,
    const double *Q /*[B][13][13] or NULL*/, const double *Qd /*[B][3] or NULL: random-walk variance per slot*/,
    const double *z /*[B][13] or NULL = predict only*/, const double *r /*[B][13]; required with z*/,
    double gate, int flags,
    double *x_new /*[B][13]*/, double *d_new /*[B][CFNMPC_ND]*/, double *Pa_new /*[B][16][16]*/,
    double *Pxx_new /*[B][13][13] or NULL: the state block, as cfnmpc_set_uncertainty takes it*/,
    double *nis /*[B] or NULL*/, int *counts /*[B][2] or NULL*/, int on_device, void *stream);

/* ESTIMATOR::predictor() for a fleet (acados_estimator.cpp:521-634), DEVICE pointers only:
 * assembles the 13-state from mocap position, onboard Euler angles [deg, as published by the
 * driver; the pitch sign flip of :495 is applied inside] and gyro rates, estimates the world
 * velocity with the reference's low-pass filter (:356-368; the reference always takes this branch
 * because it passes the absolute start time as "elapsed time"; use_lpf = 0 selects the finite
 * difference), rotates it into the body frame (:414-440) and integrates the model over `delay`
 * with the latest inputs (:573-593).  meas [B][9] = x y z roll pitch yaw wx wy wz; filt [B][9] =
 * previous position, v[k-1], v[k-2] (updated in place); u [B][4]; outputs x_est, x_pred [B][13]. */
int cfnmpc_estimate(int batch, const double *meas, double *filt, const double *u, double dt, int use_lpf,
                    double delay, int steps, double *x_est, double *x_pred, void *stream);

/* Kernel-level access for parity tests (oracle comparison of the linearisation): copies the
 * stage blocks of the last linearisation as dense row-major arrays in the reference's state
 * order: A [B][N][13][13], Bm [B][N][13][4], b [B][N][13] (host pointers). */
int cfnmpc_debug_get_linearisation(cfnmpc_solver *s, double *A, double *Bm, double *b);
/* runs only the linearisation kernel */
int cfnmpc_debug_linearise(cfnmpc_solver *s, void *stream);
/* start solve, backward half only (parity tests of the fused kernel, timing): mode 1 = k_linearise + k_factor, 2 = k_linfactor;
 * `reps` repetitions, *ms (may be NULL) = average duration of one, HIP events on `stream` */
int cfnmpc_debug_start_factor(cfnmpc_solver *s, int mode, int reps, double *ms, void *stream);
/* what that sweep leaves behind, as dense host arrays in the reference's state order (any pointer may be NULL):
 * K [B][N][4][13], d [B][N][4], cost-to-go checkpoints Pchk [B][6][13][13] (stages 4, 8, 12, 16, 24, 32 below N), status [B] */
int cfnmpc_debug_get_factor(cfnmpc_solver *s, double *K, double *d, double *Pchk, int *status);
/* partial condensing (cond_N2 > 0): runs linearisation + pcond and copies condensed block `block`
 * of every instance to the host as dense arrays in the reference's state order, with
 * z = (dU (4 m), dx (13), 1), w = 4 m + 14, m = stages of that block:
 *   H [B][w][w] symmetric (cost 1/2 z'H z; the [w-1][w-1] entry is not defined), D [B][13][w]
 *   (dx at the start of the next block = D z).  *m_out receives m. */
int cfnmpc_debug_get_condensed(cfnmpc_solver *s, int block, double *H, double *D, int *m_out);
/* number of leading stages the last QP's interior-point sweeps covered, per instance [B] (host) */
int cfnmpc_debug_get_viol(cfnmpc_solver *s, double *viol /*[B]*/);
int cfnmpc_debug_get_head(cfnmpc_solver *s, int *head);
/* work-list counts of the last step (host, four ints): constrained rows listed | rows listed for the interior-point fall-back
 * (fleets that compact them; else 0) | listed rows with heads of more than 16 stages | late rows of a split forward sweep */
int cfnmpc_debug_get_list_counts(cfnmpc_solver *s, int *counts /*[4]*/);
/* *uniform = 1 while the start solve's factorisation reads every vehicle's stage reference once per step instead of once per stage:
 * the last writer of the references was cfnmpc_set_yref and every vehicle's rows 1 .. N - 1 equalled its row 0 bit for bit (the rows
 * may differ between vehicles); 0 otherwise.  The solver finds this out on the device behind cfnmpc_set_yref; the first step that
 * follows (or this call) waits for the verdict once.  The results are the same bits either way. */
int cfnmpc_debug_get_yref_uniform(cfnmpc_solver *s, int *uniform);

/* ---- mixed-horizon fleets (BASELINE.json config C5: N in {30, 50, 100} side by side) ----------
 * The reference fixes N when the solver is generated (generate_c_code.py:41-42; one process per
 * vehicle, acados_mpc.cpp:76-82).  A fleet takes one horizon PER VEHICLE, buckets the vehicles by
 * horizon (one cfnmpc_solver per distinct N) and keeps the caller's vehicle order at the
 * boundary: rows move between that order and the buckets on the device (device pointers) or on
 * the host (host pointers).  Buckets are solved concurrently, each on an internal stream forked
 * from and joined to `stream`.  opts->N is ignored.  Layouts:
 *     x0 [B][13];  yref [B][Nmax][17] (vehicle i uses rows 0..N_i-1), yref_e [B][13];
 *     get_u: stage < min N;  get_x: stage <= min N;  stats [B]. */
typedef struct cfnmpc_fleet cfnmpc_fleet;
int cfnmpc_fleet_create(cfnmpc_fleet **out, int batch, const int *N_per_instance /*[B]*/, const cfnmpc_opts *opts);
int cfnmpc_fleet_free(cfnmpc_fleet *f);
int cfnmpc_fleet_batch(const cfnmpc_fleet *f);
int cfnmpc_fleet_min_horizon(const cfnmpc_fleet *f);
int cfnmpc_fleet_max_horizon(const cfnmpc_fleet *f);
int cfnmpc_fleet_num_buckets(const cfnmpc_fleet *f);
/* bucket b (ascending N): its horizon, size, solver (owned by the fleet; for per-bucket calls such
 * as cfnmpc_get_iterate) and the fleet index of each of its rows [count].  Any pointer may be NULL. */
int cfnmpc_fleet_bucket(const cfnmpc_fleet *f, int bucket, int *N, int *count, cfnmpc_solver **solver, int *index);
unsigned long long cfnmpc_fleet_workspace_bytes(const cfnmpc_fleet *f);
int cfnmpc_fleet_set_x0(cfnmpc_fleet *f, const double *x0, int on_device, void *stream);
int cfnmpc_fleet_set_yref(cfnmpc_fleet *f, const double *yref, const double *yref_e, int on_device, void *stream);
int cfnmpc_fleet_set_weights(cfnmpc_fleet *f, const double *W /*[17]*/, const double *WN /*[13]*/);
int cfnmpc_fleet_set_box(cfnmpc_fleet *f, double u_min, double u_max);
/* cfnmpc_set_erk_steps / cfnmpc_set_cost_scaling for every bucket */
int cfnmpc_fleet_set_erk_steps(cfnmpc_fleet *f, int num_steps);
int cfnmpc_fleet_set_cost_scaling(cfnmpc_fleet *f, double stage_scale, double terminal_scale);
/* cfnmpc_set_model_params for a fleet: HOST array [B][CFNMPC_NP] in the fleet's vehicle order (NULL: nominal) */
int cfnmpc_fleet_set_model_params(cfnmpc_fleet *f, const double *p);
/* cfnmpc_set_disturbance for a fleet: [B][CFNMPC_ND] in the fleet's vehicle order (NULL: none), host or device like
 * cfnmpc_fleet_set_x0 (a device array goes through each bucket's staging on the bucket's stream); host rows are validated as a
 * whole first.  cfnmpc_fleet_get_disturbance: the rows in force. */
int cfnmpc_fleet_set_disturbance(cfnmpc_fleet *f, const double *d, int on_device, void *stream);
int cfnmpc_fleet_get_disturbance(cfnmpc_fleet *f, double *d, int on_device, void *stream);
/* cfnmpc_set_weights_batch for a fleet: HOST arrays [B][17] / [B][13] in the fleet's vehicle order, scattered to the buckets;
 * validated as a whole first (a bad row, or an option that refuses rows, leaves every bucket unchanged; an allocation or copy
 * failure in a later bucket does not undo the earlier ones, as with cfnmpc_fleet_set_model_params) */
int cfnmpc_fleet_set_weights_batch(cfnmpc_fleet *f, const double *W, const double *WN);
/* cfnmpc_set_box_stages for a fleet: HOST arrays [B][Nmax][4] in the fleet's vehicle order (rows behind a vehicle's own
 * horizon are ignored); NULL, NULL: back to the scalar box */
int cfnmpc_fleet_set_box_stages(cfnmpc_fleet *f, const double *lb, const double *ub);
int cfnmpc_fleet_init_iterate(cfnmpc_fleet *f, int mode, void *stream);
int cfnmpc_fleet_solve(cfnmpc_fleet *f, int n_rti, void *stream);
int cfnmpc_fleet_get_u(cfnmpc_fleet *f, int stage, double *u /*[B][4]*/, int on_device, void *stream);
int cfnmpc_fleet_get_x(cfnmpc_fleet *f, int stage, double *x /*[B][13]*/, int on_device, void *stream);
int cfnmpc_fleet_get_cmd(cfnmpc_fleet *f, double *cmd_vel /*[B][4]*/, int *motvel /*[B][4]*/, int on_device, void *stream);
int cfnmpc_fleet_get_stats(cfnmpc_fleet *f, int *status, int *qp_iter, double *res, int on_device, void *stream);
/* cfnmpc_solve_sqp for a fleet: every bucket still running takes its iteration on its own stream, then the host waits once;
 * a bucket whose instances are all done launches nothing more.  *n_iter = iterations of the longest-running bucket.
 * Synchronises `stream`. */
int cfnmpc_fleet_solve_sqp(cfnmpc_fleet *f, int max_iter, double tol_step, double tol_eq, double tol_ineq, int *n_iter,
                           void *stream);
/* cfnmpc_get_sqp_stats in the fleet's vehicle order: status [B], sqp_iter [B], res [B][3] */
int cfnmpc_fleet_get_sqp_stats(cfnmpc_fleet *f, int *status, int *sqp_iter, double *res, int on_device, void *stream);
/* cfnmpc_set_sqp_globalization on every bucket (checked before anything changes), cfnmpc_get_sqp_ls_stats in the fleet's
 * vehicle order */
int cfnmpc_fleet_set_sqp_globalization(cfnmpc_fleet *f, int mode, double eta, double reduction, double alpha_min);
int cfnmpc_fleet_get_sqp_ls_stats(cfnmpc_fleet *f, double *alpha, double *mu, int *n_short, int *n_fail, int on_device, void *stream);
/* Solution sensitivities w.r.t. x0 of every bucket's last QP (cfnmpc_eval_sens_x0), rows in the fleet's vehicle order.  The range
 * is limited by the shortest horizon: dx up to stage Nmin, du below it.  Host arrays (on_device 0 or 2) are filled
 * synchronously. */
int cfnmpc_fleet_eval_sens_x0(cfnmpc_fleet *f, double act_tol, void *stream);
int cfnmpc_fleet_get_sens_x0(cfnmpc_fleet *f, int stage, int n_stages, double *du /*[B][n_stages][4][13] or NULL*/,
                             double *dx /*[B][n_stages][13][13] or NULL*/, int on_device, void *stream);
/* Adjoint sensitivities of every bucket's last QP (cfnmpc_eval_adjoint), rows in the fleet's vehicle order: gx [B][n_g][13] and
 * gu [B][n_g][4] (either may be NULL, not both) for the stages [0, n_g), n_g <= the shortest horizon -- no terminal-stage
 * gradient, which would sit at another stage in every bucket.  The getter returns the per-vehicle outputs dl_dx0 [B][13],
 * dl_dW [B][17], dl_dWN [B][13] (any may be NULL, not all); the per-stage outputs are read from the bucket solvers
 * (cfnmpc_fleet_bucket).  A fleet's rows equal its bucket solvers' bit for bit. */
int cfnmpc_fleet_eval_adjoint(cfnmpc_fleet *f, const double *gx, const double *gu, int n_g, int on_device, void *stream);
int cfnmpc_fleet_get_adjoint(cfnmpc_fleet *f, double *dl_dx0, double *dl_dW, double *dl_dWN, int on_device, void *stream);
/* Uncertainty propagation and bound tightening on every bucket (cfnmpc_set_uncertainty ...), rows in the fleet's vehicle order.
 * Host arrays are validated as a whole first.  beta has [B][Nmax][4] with NaN behind a vehicle's own horizon;
 * cfnmpc_fleet_get_uncertainty's range is limited by the shortest horizon (stage + n_stages <= Nmin + 1). */
int cfnmpc_fleet_set_uncertainty(cfnmpc_fleet *f, const double *Sigma0, const double *W, int on_device, void *stream);
int cfnmpc_fleet_set_uncertainty_gain(cfnmpc_fleet *f, int mode, const double *K, int on_device, void *stream);
int cfnmpc_fleet_eval_uncertainty(cfnmpc_fleet *f, void *stream);
int cfnmpc_fleet_get_backoff(cfnmpc_fleet *f, double *beta /*[B][Nmax][4]*/, int on_device, void *stream);
int cfnmpc_fleet_get_uncertainty(cfnmpc_fleet *f, int stage, int n_stages, double *Sigma, double *std_x, int on_device, void *stream);
int cfnmpc_fleet_tighten_box(cfnmpc_fleet *f, double gamma, double min_width, int *n_clamped /*[B] or NULL*/, int on_device, void *stream);
/* The polynomial references for a fleet (cfnmpc_set_poly_library ...): the library goes to every bucket; traj [B] and place [B][6]
 * in the fleet's vehicle order (host arrays are validated as a whole first); every bucket writes its own N + 1 rows at the shared
 * t and dt.  cfnmpc_fleet_eval_poly evaluates every vehicle's own N stage rows: flat [B][Nmax][13], rows [B][Nmax][17], NaN behind a
 * vehicle's own horizon. */
int cfnmpc_fleet_set_poly_library(cfnmpc_fleet *f, const double *pieces, const int *first, int n_traj, void *stream);
int cfnmpc_fleet_set_poly_assignment(cfnmpc_fleet *f, const int *traj, const double *place, int on_device, void *stream);
int cfnmpc_fleet_set_yref_poly(cfnmpc_fleet *f, double t, int flags, void *stream);
int cfnmpc_fleet_eval_poly(cfnmpc_fleet *f, double t, int flags, double *flat /*[B][Nmax][13] or NULL*/,
                           double *rows /*[B][Nmax][17] or NULL*/, int on_device, void *stream);
/* cfnmpc_eval_nlp (keep_multipliers = 0) on every bucket, cfnmpc_get_nlp_stats in the fleet's vehicle order: cost [B], res [B][3]
 * (host arrays, on_device 0 or 2, are filled synchronously).  The multipliers have one shape per horizon: evaluate and read them
 * through the bucket's solver (cfnmpc_fleet_bucket). */
int cfnmpc_fleet_eval_nlp(cfnmpc_fleet *f, void *stream);
int cfnmpc_fleet_get_nlp_stats(cfnmpc_fleet *f, double *cost /*[B] or NULL*/, double *res /*[B][3] or NULL*/, int on_device,
                               void *stream);

/* ---- one fleet across several GPUs of a node, from ONE process --------------------------------
 * The reference owns one vehicle per process (acados_mpc.cpp:76-82); instances are independent, so a
 * fleet splits into contiguous shards with no exchange between devices: shard i
 * = vehicles [lo_i, hi_i) on HIP device device_ids[i] (ids may repeat), each with its own solver and
 * stream.  cfnmpc_multi_solve launches every shard's step and returns without waiting; getters wait
 * for what they read.  Host arrays cover the WHOLE fleet ([B][..] as in the single-device calls).
 * Device-resident I/O: take a shard's solver / stream with cfnmpc_multi_shard and use the
 * single-device calls with pointers of that device. */
typedef struct cfnmpc_multi cfnmpc_multi;
int cfnmpc_multi_create(cfnmpc_multi **out, int n_shards, const int *device_ids /*[n_shards]*/, int total_batch,
                        const cfnmpc_opts *opts);
/* Mixed horizons across GPUs (BASELINE.json config C5 "8 x MI355X, divergent-length stress"; SURVEY.md section 8e: "first
 * bucket by N, then balance buckets across GPUs by sum N_i"): one horizon PER VEHICLE; the vehicles are dealt out over the
 * shards by cfnmpc_shard_by_horizon, every shard is a cfnmpc_fleet (one solver per horizon bucket) over its -- NOT
 * contiguous -- index set.  Host arrays cover the whole fleet in the caller's order with the fleet layouts (yref
 * [B][Nmax][17], boxes [B][Nmax][4], get_u: stage < min N).  cfnmpc_multi_shard does not apply (CFNMPC_EINVAL); use
 * cfnmpc_multi_shard_fleet: the shard's fleet, its vehicle count and their indices [count] in the caller's order. */
int cfnmpc_multi_create_horizons(cfnmpc_multi **out, int n_shards, const int *device_ids /*[n_shards]*/, int total_batch,
                                 const int *N_per_instance /*[total_batch]*/, const cfnmpc_opts *opts);
int cfnmpc_multi_shard_fleet(const cfnmpc_multi *m, int shard, cfnmpc_fleet **fleet, int *count, int *index, int *device, void **stream);
/* The partitioner itself (pure host code, no device needed; also what bench.py's ranks use for `--workload mixed`):
 * vehicles in order of decreasing horizon, each to the shard with the smallest sum N so far (ties: lowest shard).
 * shard_of [batch] receives the shard of every vehicle; sum N of any two shards differs by at most one vehicle's horizon. */
int cfnmpc_shard_by_horizon(int batch, const int *N_per_instance, int n_shards, int *shard_of);
int cfnmpc_multi_free(cfnmpc_multi *m);
int cfnmpc_multi_batch(const cfnmpc_multi *m);
int cfnmpc_multi_num_shards(const cfnmpc_multi *m);
int cfnmpc_multi_shard(const cfnmpc_multi *m, int shard, cfnmpc_solver **solver, int *lo, int *hi, int *device, void **stream);
int cfnmpc_multi_set_x0(cfnmpc_multi *m, const double *x0 /*[B][13] host*/);
int cfnmpc_multi_set_yref(cfnmpc_multi *m, const double *yref /*[B][N][17] host*/, const double *yref_e /*[B][13] host*/);
int cfnmpc_multi_set_weights(cfnmpc_multi *m, const double *W, const double *WN);
int cfnmpc_multi_init_iterate(cfnmpc_multi *m, int mode);
int cfnmpc_multi_solve(cfnmpc_multi *m, int n_rti);   /* asynchronous on every shard's stream */
int cfnmpc_multi_sync(cfnmpc_multi *m);
int cfnmpc_multi_get_u(cfnmpc_multi *m, int stage, double *u /*[B][4] host*/);
int cfnmpc_multi_get_x(cfnmpc_multi *m, int stage, double *x /*[B][13] host*/);
int cfnmpc_multi_get_cmd(cfnmpc_multi *m, double *cmd_vel /*[B][4] host*/, int *motvel /*[B][4] host or NULL*/);
int cfnmpc_multi_get_stats(cfnmpc_multi *m, int *status, int *qp_iter, double *res);
/* cfnmpc_set_box / cfnmpc_set_box_stages (host arrays [B][N][4] of the whole fleet) for every shard */
int cfnmpc_multi_set_box(cfnmpc_multi *m, double u_min, double u_max);
int cfnmpc_multi_set_box_stages(cfnmpc_multi *m, const double *lb, const double *ub);
/* cfnmpc_set_erk_steps / cfnmpc_set_cost_scaling for every shard */
int cfnmpc_multi_set_erk_steps(cfnmpc_multi *m, int num_steps);
int cfnmpc_multi_set_cost_scaling(cfnmpc_multi *m, double stage_scale, double terminal_scale);
/* cfnmpc_set_model_params for every shard: HOST array [B][CFNMPC_NP] of the whole fleet (NULL: nominal) */
int cfnmpc_multi_set_model_params(cfnmpc_multi *m, const double *p);
/* cfnmpc_set_disturbance for every shard: HOST array [B][CFNMPC_ND] of the whole fleet (NULL: none), validated as a whole first */
int cfnmpc_multi_set_disturbance(cfnmpc_multi *m, const double *d);
/* cfnmpc_set_weights_batch for every shard (both create variants): HOST arrays [B][17] / [B][13] of the whole fleet; validated
 * as a whole first (a bad row leaves every shard unchanged; an allocation or copy failure in a later shard does not undo the
 * earlier ones) */
int cfnmpc_multi_set_weights_batch(cfnmpc_multi *m, const double *W, const double *WN);
/* Solution sensitivities w.r.t. x0 over the whole fleet (cfnmpc_eval_sens_x0 per shard): host arrays in the caller's order,
 * synchronous; for cfnmpc_multi_create_horizons the range is limited by the shortest horizon, as for a fleet. */
int cfnmpc_multi_eval_sens_x0(cfnmpc_multi *m, double act_tol);
int cfnmpc_multi_get_sens_x0(cfnmpc_multi *m, int stage, int n_stages, double *du /*host or NULL*/, double *dx /*host or NULL*/);
/* Adjoint sensitivities over the whole fleet (cfnmpc_eval_adjoint per shard; cfnmpc_fleet_eval_adjoint's arguments): host arrays
 * in the caller's order, synchronous; n_g <= the (shortest) horizon. */
int cfnmpc_multi_eval_adjoint(cfnmpc_multi *m, const double *gx, const double *gu, int n_g);
int cfnmpc_multi_get_adjoint(cfnmpc_multi *m, double *dl_dx0, double *dl_dW, double *dl_dWN);
/* Uncertainty propagation and bound tightening per shard (both create variants): host arrays of the whole fleet in the caller's
 * order, synchronous, validated as a whole first; beta [B][N][4] (N: the longest horizon; NaN behind a vehicle's own).  The full
 * covariance is read through the shards' solvers (cfnmpc_multi_shard / cfnmpc_multi_shard_fleet). */
int cfnmpc_multi_set_uncertainty(cfnmpc_multi *m, const double *Sigma0, const double *W);
int cfnmpc_multi_set_uncertainty_gain(cfnmpc_multi *m, int mode, const double *K);
int cfnmpc_multi_eval_uncertainty(cfnmpc_multi *m);
int cfnmpc_multi_get_backoff(cfnmpc_multi *m, double *beta /*[B][N][4] host*/);
int cfnmpc_multi_tighten_box(cfnmpc_multi *m, double gamma, double min_width, int *n_clamped /*[B] host or NULL*/);
/* cfnmpc_eval_nlp (keep_multipliers = 0) per shard and its results over the whole fleet (both create variants): host arrays in
 * the caller's order, synchronous */
int cfnmpc_multi_eval_nlp(cfnmpc_multi *m);
int cfnmpc_multi_get_nlp_stats(cfnmpc_multi *m, double *cost /*[B] host or NULL*/, double *res /*[B][3] host or NULL*/);

/* The polynomial references per shard (both create variants): the library to every shard; host arrays traj [B], place [B][6] or NULL
 * of the whole fleet in the caller's order, validated as a whole first; cfnmpc_multi_set_yref_poly is asynchronous on every shard's
 * stream, like cfnmpc_multi_solve. */
int cfnmpc_multi_set_poly_library(cfnmpc_multi *m, const double *pieces, const int *first, int n_traj);
int cfnmpc_multi_set_poly_assignment(cfnmpc_multi *m, const int *traj, const double *place);
int cfnmpc_multi_set_yref_poly(cfnmpc_multi *m, double t, int flags);

const char *cfnmpc_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CFNMPC_H */
