// host_stage_check.cpp -- stand-alone check of the array tables of the solver-less batched calls,
// crazyflie_nmpc_amd/csrc/cfnmpc_stage.hpp (Arr, Stage and the six calls' lists): plain C++, no GPU, no HIP call.  Builds every
// call's table for every present / absent combination of its optional arrays at B = 1, 3, 257 (rollouts: L = 1, 2) and checks
// alignment, that no two staged arrays overlap, the total, that an absent array maps to nullptr, that nis and counts have room
// even when the caller declined them -- and that the total is what the hand-written size expressions of the code before the
// tables gave (transcribed below, so that the layout is pinned to them and not to itself).  Then moves every array of two calls
// through a malloc'ed staging area of exactly the table's size.  Meant for the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host_stage_check.cpp -o host_stage_check
//   ./host_stage_check
// (make -C crazyflie_nmpc_amd/csrc host_stage_check; tests/test_host_stage_cpu.py builds and runs it the same way)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../crazyflie_nmpc_amd/csrc/cfnmpc_stage.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

using cfn::Stage;
static double some_d;   // stands for a caller's array where only the table is looked at: never read or written
static int some_i;
static double* D(unsigned mask, int bit) { return (mask >> bit) & 1 ? &some_d : nullptr; }
static int* I(unsigned mask, int bit) { return (mask >> bit) & 1 ? &some_i : nullptr; }
static const size_t NPAR = CFNMPC_NP, ND = CFNMPC_ND;

// one table: `doubles` is the size the hand-written expression gave; `always`: bit i set = array i is staged whatever was passed
static int check_table(const Stage& t, size_t doubles, unsigned always = 0) {
    CHECK(t.n <= cfn::MAX_ARRS);
    char* const base = reinterpret_cast<char*>(uintptr_t(4096));   // (an address to measure from: not dereferenced)
    const cfn::ArrPtrs q = t.at(base), own = t.own();
    size_t end = 0;
    for (int i = 0; i < t.n; i++) {
        const bool want = t.a[i].p || ((always >> i) & 1);
        CHECK(t.staged(i) == want && own.p[i] == t.a[i].p);
        if (!want) { CHECK(q.p[i] == nullptr && !t.copy_in(i) && !t.copy_out(i)); continue; }
        CHECK(q.p[i] == base + t.off[i] && t.off[i] % 8 == 0 && t.size(i) > 0);
        CHECK(t.off[i] + t.size(i) <= t.bytes);                     // (room, also for an output the caller declined)
        if (!t.a[i].p) CHECK(!t.copy_in(i) && !t.copy_out(i));
        for (int j = 0; j < i; j++)
            if (t.staged(j)) CHECK(t.off[j] + t.size(j) <= t.off[i] || t.off[i] + t.size(i) <= t.off[j]);
        if (t.off[i] + t.size(i) > end) end = t.off[i] + t.size(i);
    }
    CHECK(t.bytes == (end + 7) / 8 * 8 && t.bytes == doubles * 8);
    return 0;
}

// every array of `t` (given or always staged) through a staging area of exactly t.bytes and back, the caller's arrays of exactly
// their sizes: inputs arrive, outputs the "kernel" wrote come back, nothing lands on a neighbour
static int round_trip(Stage t) {
    for (int i = 0; i < t.n; i++)
        if (t.a[i].p) {
            t.a[i].p = std::malloc(t.size(i));
            std::memset(t.a[i].p, 0x10 + i, t.size(i));
        }
    char* const base = static_cast<char*>(std::malloc(t.bytes));
    std::memset(base, 0xEE, t.bytes);
    const cfn::ArrPtrs q = t.at(base);
    for (int i = 0; i < t.n; i++)
        if (t.copy_in(i)) std::memcpy(q.p[i], t.a[i].p, t.size(i));
    for (int i = 0; i < t.n; i++)                                    // the kernel: every staged pure output
        if (t.staged(i) && t.a[i].dir == cfn::ARR_OUT) std::memset(q.p[i], 0x80 + i, t.size(i));
    for (int i = 0; i < t.n; i++) {
        if (!t.staged(i)) continue;
        const unsigned char want = (unsigned char)((t.a[i].dir & cfn::ARR_IN ? 0x10 : 0x80) + i);
        for (size_t e = 0; e < t.size(i); e++) CHECK(static_cast<unsigned char*>(q.p[i])[e] == want);
        if (t.copy_out(i)) {
            std::memset(t.a[i].p, 0, t.size(i));
            std::memcpy(t.a[i].p, q.p[i], t.size(i));
        }
        if (t.a[i].p)
            for (size_t e = 0; e < t.size(i); e++) CHECK(static_cast<unsigned char*>(t.a[i].p)[e] == want);
    }
    std::free(base);
    for (int i = 0; i < t.n; i++) std::free(t.a[i].p);
    return 0;
}

int main() {
    static_assert(cfn::MAX_ARRS >= 15, "cfnmpc_ekf_aug_step has 15 arrays");
    int n_tables = 0;
    for (size_t B : {size_t(1), size_t(3), size_t(257)}) {
        const size_t nx = B * 13, nP = B * 169, nA = B * 256, np = B * NPAR, nd = B * ND, nq = B * 3;
        double* const a = &some_d;
        // cfnmpc_sim, cfnmpc_sim_params, cfnmpc_sim_dist -- options p, d
        for (unsigned m = 0; m < 4; m++, n_tables++) {
            const double *p = D(m, 0), *d = D(m, 1);
            if (check_table(cfn::SimArrs::of(B, a, a, a, p, d), B * (30 + (p ? NPAR : 0) + (d ? ND : 0)))) return 1;
        }
        // cfnmpc_estimate_disturbance -- option p
        for (unsigned m = 0; m < 2; m++, n_tables++) {
            const double* p = D(m, 0);
            const Stage t = cfn::DistObserveArrs::of(B, a, a, a, a, p);
            if (check_table(t, B * (30 + ND + (p ? NPAR : 0)))) return 1;
            CHECK(t.copy_in(cfn::DistObserveArrs::D) && t.copy_out(cfn::DistObserveArrs::D));   // d: in-out
        }
        for (size_t L : {size_t(1), size_t(2)}) {
            const size_t nu = B * L * 4, ns = B * (L + 1) * 13;
            // cfnmpc_sim_rollout -- options p, d
            for (unsigned m = 0; m < 4; m++, n_tables++) {
                const double *p = D(m, 0), *d = D(m, 1);
                if (check_table(cfn::RolloutArrs::of(B, L, a, a, a, p, d), nx + nu + ns + (p ? B * NPAR : 0) + (d ? B * ND : 0))) return 1;
            }
            // cfnmpc_sim_rollout_vjp -- options p, d, gu, gp, gd
            for (unsigned m = 0; m < 32; m++, n_tables++) {
                double *p = D(m, 0), *d = D(m, 1), *gu = D(m, 2), *gp = D(m, 3), *gd = D(m, 4);
                if (check_table(cfn::RolloutVjpArrs::of(B, L, a, a, a, p, d, a, gu, gp, gd),
                                2 * ns + nu + (p ? np : 0) + (d ? nd : 0) + nx + (gu ? nu : 0) + (gp ? np : 0) + (gd ? nd : 0))) return 1;
            }
        }
        const size_t nu = B * 4;
        // cfnmpc_ekf_step -- options p, d, Q, z (with r), and r without z (not read: no room), nis, counts (room in every case)
        for (unsigned m = 0; m < 128; m++, n_tables++) {
            using K = cfn::EkfArrs;
            double *p = D(m, 0), *d = D(m, 1), *Q = D(m, 2), *z = D(m, 3), *r = z ? a : D(m, 4), *nis = D(m, 5);
            const Stage t = K::of(B, a, a, a, p, d, Q, z, r, a, a, nis, I(m, 6));
            // (what is checked against is the table's own r: nullptr without z)
            CHECK((t.a[K::R].p != nullptr) == (z != nullptr));
            if (check_table(t, nx + nP + nu + (p ? np : 0) + (d ? nd : 0) + (Q ? nP : 0) + (z ? 2 * nx : 0) + nx + nP + 2 * B,
                            1u << K::NIS | 1u << K::COUNTS)) return 1;
            CHECK(t.copy_out(K::NIS) == (nis != nullptr) && t.copy_out(K::COUNTS) == (I(m, 6) != nullptr));
        }
        // cfnmpc_ekf_aug_step -- options p, Q, Qd, z (with r), Pxx, nis, counts
        for (unsigned m = 0; m < 128; m++, n_tables++) {
            using K = cfn::EkfAugArrs;
            double *p = D(m, 0), *Q = D(m, 1), *Qd = D(m, 2), *z = D(m, 3), *Pxx = D(m, 4), *nis = D(m, 5);
            const Stage t = K::of(B, a, a, a, a, p, Q, Qd, z, a, a, a, a, Pxx, nis, I(m, 6));
            if (check_table(t, nx + nd + nA + nu + (p ? np : 0) + (Q ? nP : 0) + (Qd ? nq : 0) + (z ? 2 * nx : 0) + nx + nd + nA +
                                   (Pxx ? nP : 0) + 2 * B, 1u << K::NIS | 1u << K::COUNTS)) return 1;
            CHECK(t.n == 15 && t.copy_out(K::PXX) == (Pxx != nullptr) && t.copy_out(K::NIS) == (nis != nullptr));
        }
    }
    // the widest call with everything given, and with the optional outputs declined; the in-out call
    double* const a = &some_d;
    if (round_trip(cfn::EkfAugArrs::of(3, a, a, a, a, a, a, a, a, a, a, a, a, a, a, &some_i))) return 1;
    if (round_trip(cfn::EkfAugArrs::of(3, a, a, a, a, nullptr, a, nullptr, a, a, a, a, a, nullptr, nullptr, nullptr))) return 1;
    if (round_trip(cfn::DistObserveArrs::of(257, a, a, a, a, a))) return 1;
    std::printf("host_stage_check ok (%d tables)\n", n_tables);
    return 0;
}
