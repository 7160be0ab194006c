// cfnmpc_asdense_body.inc -- the body of k_as_dense, included once per kernel by cfnmpc_asdense.hip with AS_DENSE_WR defined: the
// source of the row's cost weights (WR_ARGS: the kernel arguments, k_as_dense; WR_TABLE: Params.wtab, k_as_dense_w).  Text
// instead of a function template: behind a call, however inlined, k_as_dense no longer compiles to the register and scratch
// figures the budget tests pin.
    __shared__ DenseLds S;
    const int lane = threadIdx.x;
    const int N = P.N;
    const int nipm = gm(P.nipm)[0], nbig = gm(P.nipm)[NI_LONG16];
    for (int slot = nbig + (int)blockIdx.x; slot < nipm; slot += (int)gridDim.x) {
#ifdef CFN_PROF
        unsigned long long dacc[6] = {0, 0, 0, 0, 0, 0}, dlast = wall_clock64();
        const unsigned long long dstart = dlast;
#endif
        const int inst = gm(P.ilist)[slot];
        const int head = gm(P.head)[inst];           // <= 16 (or N <= 16): guaranteed by the list order (k_scatter)
        const double viol = gm(P.viol)[inst];
        // rows far outside the box skip the active-set iteration (as qp_wave): straight to the interior point
        const bool try_as = viol > 0.0 && !(P.as_skip_viol > 0.0 && viol > P.as_skip_viol * (P.u_max - P.u_min));
        if (!try_as || head < 1 || head > 16) {
            if (lane == 0) gm(P.asst)[slot] = 0;
            continue;
        }
        int chk = -1;
        SFOR(c, 0, N_CHK, { if (head == chk_stage(c) && head < N) chk = c; });
        // every DPP row of the wave addresses the same instance (the stage matrices are broadcast sources inside a row)
        const Lane t = lane_indirect<AS_DENSE_WR>(P, inst, true);
        const Lane& t_ = t;
        // this lane's input (k_j, a_j): unconstrained minimiser and iterate, in flight during the build
        const size_t e4 = i4(P, t, imin(lane >> 2, head - 1), lane & 3);
        const double v0 = lane < 4 * head ? gm(P.v)[e4] : 0.0;
        const double uk = lane < 4 * head ? gm(P.uit)[e4] : 0.0;
        __syncthreads();
        dense_stage<AS_DENSE_WR>(P, lane_opaque(t), head, chk, S.G, S.pm);
        __syncthreads();
        DPROF(0)
        if (head > 8) dense_build<true, AS_DENSE_WR>(P, lane_opaque(t), head, chk, S);
        else dense_build<false, AS_DENSE_WR>(P, lane_opaque(t), head, chk, S);
        __syncthreads();
        DPROF(1)
        int solves;
        if (head <= 4) solves = dense_solve<1>(P, head, v0, uk, S);
        else if (head <= 8) solves = dense_solve<2>(P, head, v0, uk, S);
        else if (head <= 12) solves = dense_solve<3>(P, head, v0, uk, S);
        else solves = dense_solve<4>(P, head, v0, uk, S);
        DPROF(2)
        if (solves > 0) {
            // du of the head -> the compact slot's P.dva; dx_1 .. dx_head -> P.czdx (what k_ascommit reads)
            const double dl = S.cv[lane];
            if (lane < 4 * head) gm(P.dva)[(size_t)slot * N * 4 + lane] = dl;
            // the stage matrices once more (the H store is free again): staged with all loads in flight, then the sequential sweep
            __syncthreads();
            const Lane t = lane_opaque(t_);   // (the sweep's addresses stay inside it)
            {
                StageOps o[4];
                SFOR(b, 0, 4, { load_ops(P, t, imin(4 * b + t.row, head - 1), o[b]); });
                SFOR(b, 0, 4, {
                    const int k = 4 * b + t.row;
                    if (k < head) {
                        double* d = S.G + k * ST_BLK + t.L * ST_ROW;
                        SFOR(g, 0, 10, { d[g] = o[b].ac[g]; });
                        SFOR(a, 0, 4, { d[10 + a] = o[b].br[a]; });
                    }
                });
            }
            __syncthreads();
            double x = 0.0;
            StageOps o0, o1;
            lds_ops(S.G, t, 0, o0);
            auto step = [&](const StageOps& o, const int k) {
                double xn = t.L < 3 ? x : 0.0;
                dotbc<10, 3>(xn, o.ac, x);
                SFOR(a, 0, 4, { xn = __builtin_fma(o.br[a], S.cv[k * 4 + a], xn); });
                x = xn;
                if (t.row == 0 && t.L < 13) gm(P.czdx)[((size_t)slot * (N + 1) + k + 1) * 13 + t.L] = x;
            };
            for (int k = 0; k < head; k += 2) {
                lds_ops(S.G, t, imin(k + 1, head - 1), o1);
                step(o0, k);
                if (k + 1 >= head) break;
                lds_ops(S.G, t, imin(k + 2, head - 1), o0);
                step(o1, k + 1);
            }
        }
        if (lane == 0) {
            gm(P.asst)[slot] = solves > 0 ? 1 : 0;
            if (solves > 0) gm(P.iters)[inst] = solves;
        }
#ifdef CFN_PROF
        DPROF(3)
        if (lane == 0) {
            const unsigned long long tot = dlast - dstart;
            const unsigned long long old = atomicMax(&g_dprof[8], tot);
            if (tot > old) { for (int i = 0; i < 6; i++) g_dprof[i] = dacc[i]; g_dprof[11] = solves; g_dprof[12] = head; }
            atomicAdd(&g_dprof[9], tot); atomicAdd(&g_dprof[10], 1ull); atomicAdd(&g_dprof[13], (unsigned long long)solves);
            for (int i = 0; i < 6; i++) atomicAdd(&g_dprof[16 + i], dacc[i]);
        }
#endif
    }
