// ekf_aug_check -- one instance's disturbance-augmented filter step (csrc/cfnmpc_ekf.hpp: ekf_aug_predict, ekf_aug_update, plain
// loops) and the host validation of its arrays (csrc/cfnmpc_host.hpp: unc_sym_ok<16>, ekf_sel_ok, ekf_unused_zero) compiled for the
// HOST and run under AddressSanitizer and UndefinedBehaviorSanitizer (make -C crazyflie_nmpc_amd/csrc ekf_aug_check [CASES=file]);
// plain C++ with its own main, nothing of it is loaded into Python and nothing of it runs on a GPU.
//
// Case file (text, written by tests/test_ekf_aug_cpu.py from its numpy twin):
//     n_cases
//     steps T gate flags has_Q has_Qd has_z sel0 sel1 sel2
//     p[8]   d[6]   x[13]   Pa[256]   u[4]   Q[169]   Qd[3]   z[13]   r[13]
//     x_new[13]   d_new[6]   Pa_new[256]   nis   used   rejected              (expected)
// Error measure per output array: max |difference| / max(max |expected|, 1e-12); bound 1e-12; the counts exactly, and the
// components of d no slot estimates bit for bit.  Without a file: a predict-only and a full step on fixed data, and the validators
// on what they must accept and refuse (for the sanitizers).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../crazyflie_nmpc_amd/csrc/cfnmpc_ekf.hpp"
#include "../crazyflie_nmpc_amd/csrc/cfnmpc_host.hpp"

using namespace cfn;

namespace {

struct Case {
    int steps, flags, has_Q, has_Qd, has_z, sel[3];
    double T, gate;
    std::vector<double> p, d, x, Pa, u, Q, Qd, z, r, xn, dn, Pan;
    double nis;
    int used, rejected;
};

DstK model(const Case& c) {
    DstK mk;
    double kr[NK];
    derive_k(c.p.data(), kr);
    for (int e = 0; e < 8; e++) mk.c[e] = kr[e];
    for (int e = 0; e < ND; e++) mk.d[e] = c.d[e];
    return mk;
}

// the step as the kernel arranges it: a = (x, d[sel]), predict, update, d_new = d with the used slots replaced
void step(const Case& c, double (&x)[13], double (&dn)[ND], std::vector<double>& Pa, double& nis, int (&counts)[2]) {
    const DstK mk = model(c);
    double u[4], a[EKF_NA];
    for (int e = 0; e < 13; e++) x[e] = c.x[e];
    for (int e = 0; e < 4; e++) u[e] = c.u[e];
    Pa = c.Pa;
    nis = 0.0;
    counts[0] = 0; counts[1] = 0;
    ekf_aug_predict(x, Pa.data(), u, c.sel, c.T, c.steps, c.has_Q ? c.Q.data() : nullptr, c.has_Qd ? c.Qd.data() : nullptr, mk);
    for (int e = 0; e < 13; e++) a[e] = x[e];
    for (int k = 0; k < 3; k++) a[13 + k] = c.sel[k] >= 0 ? c.d[c.sel[k]] : 0.0;
    if (c.has_z) ekf_aug_update(a, Pa.data(), c.z.data(), c.r.data(), c.gate, c.flags, nis, counts);
    for (int e = 0; e < 13; e++) x[e] = a[e];
    for (int e = 0; e < ND; e++) dn[e] = c.d[e];
    for (int k = 0; k < 3; k++)
        if (c.sel[k] >= 0) dn[c.sel[k]] = a[13 + k];
}

double err(const double* a, const double* ref, size_t n) {
    double num = 0, den = 1e-12;
    for (size_t i = 0; i < n; i++) {
        num = std::fmax(num, std::fabs(a[i] - ref[i]));
        den = std::fmax(den, std::fabs(ref[i]));
    }
    return num / den;
}

bool read(FILE* f, std::vector<double>& v, size_t n) {
    v.resize(n);
    for (size_t i = 0; i < n; i++)
        if (fscanf(f, "%lf", &v[i]) != 1) return false;
    return true;
}

int run_file(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) { fprintf(stderr, "ekf_aug_check: cannot open %s\n", path); return 2; }
    int n = 0;
    if (fscanf(f, "%d", &n) != 1 || n < 1) { fclose(f); fprintf(stderr, "ekf_aug_check: bad case file\n"); return 2; }
    double worst = 0;
    for (int ci = 0; ci < n; ci++) {
        Case c;
        if (fscanf(f, "%d %lf %lf %d %d %d %d %d %d %d", &c.steps, &c.T, &c.gate, &c.flags, &c.has_Q, &c.has_Qd, &c.has_z, &c.sel[0],
                   &c.sel[1], &c.sel[2]) != 10 || c.steps < 1 || c.steps > 64 || !ekf_sel_ok(c.sel)) {
            fclose(f); fprintf(stderr, "ekf_aug_check: bad header of case %d\n", ci); return 2;
        }
        std::vector<double> tail;
        if (!(read(f, c.p, NPAR) && read(f, c.d, ND) && read(f, c.x, 13) && read(f, c.Pa, 256) && read(f, c.u, 4) && read(f, c.Q, 169) &&
              read(f, c.Qd, 3) && read(f, c.z, 13) && read(f, c.r, 13) && read(f, c.xn, 13) && read(f, c.dn, ND) && read(f, c.Pan, 256) &&
              read(f, tail, 3))) {
            fclose(f); fprintf(stderr, "ekf_aug_check: case %d is short\n", ci); return 2;
        }
        c.nis = tail[0]; c.used = (int)tail[1]; c.rejected = (int)tail[2];
        if (!unc_sym_ok<16>(c.Pa.data(), 1) || !ekf_unused_zero(c.Pa.data(), 1, c.sel)) {
            fclose(f); printf("ekf_aug_check FAILED: case %d: the validation refuses the case's Pa\n", ci); return 1;
        }
        double x[13], dn[ND], nis = 0.0;
        int counts[2] = {0, 0};
        std::vector<double> Pa;
        step(c, x, dn, Pa, nis, counts);
        const double e4[4] = {err(x, c.xn.data(), 13), err(dn, c.dn.data(), ND), err(Pa.data(), c.Pan.data(), 256), err(&nis, &c.nis, 1)};
        for (int k = 0; k < 4; k++) {
            worst = std::fmax(worst, e4[k]);
            if (!(e4[k] <= 1e-12)) {
                fclose(f);
                printf("ekf_aug_check FAILED: case %d (steps %d), output %d: error %.3e > 1e-12\n", ci, c.steps, k, e4[k]);
                return 1;
            }
        }
        for (int e = 0; e < ND; e++)
            if (e != c.sel[0] && e != c.sel[1] && e != c.sel[2] && std::memcmp(&dn[e], &c.d[e], 8) != 0) {
                fclose(f); printf("ekf_aug_check FAILED: case %d: d[%d] is not copied bit for bit\n", ci, e); return 1;
            }
        if (counts[0] != c.used || counts[1] != c.rejected) {
            fclose(f);
            printf("ekf_aug_check FAILED: case %d: counts (%d, %d), expected (%d, %d)\n", ci, counts[0], counts[1], c.used, c.rejected);
            return 1;
        }
    }
    fclose(f);
    printf("ekf_aug_check ok: %d cases, worst error %.3e\n", n, worst);
    return 0;
}

int run_builtin() {
    Case c;
    c.steps = 3; c.flags = EKF_NORMALIZE_Q; c.has_Q = 1; c.has_Qd = 1; c.has_z = 0; c.T = 0.015; c.gate = 3.0;
    c.sel[0] = 2; c.sel[1] = -1; c.sel[2] = 4;
    c.p = {9.8066, 33e-3, 1.395e-5, 1.395e-5, 2.173e-5, 7.9379e-06, 3.25e-4, 0.0325};
    c.d = {0.3, -0.2, 0.5, 1.0, -2.0, 0.5};
    c.x = {0.1, -0.2, 0.3, 0.98, 0.1, -0.1, 0.05, 0.3, -0.2, 0.1, 0.5, -0.4, 0.3};
    c.u = {15.0, 16.0, 15.5, 16.5};
    c.Pa.assign(256, 0.0); c.Q.assign(169, 0.0);
    for (int e = 0; e < 13; e++) { c.Pa[e * 17] = 0.01 * (1 + e); c.Q[e * 14] = 1e-6; }
    c.Pa[13 * 17] = 0.25; c.Pa[15 * 17] = 1.0;   // (slot 1 is unused: its row and column stay zero)
    c.Qd = {1e-4, 7.0, 1e-3};                    // (the entry of the unused slot is ignored)
    c.z = c.x; c.z[0] += 0.01; c.z[1] += 5.0;   // the second component: far outside the gate
    for (int e = 3; e < 7; e++) c.z[e] = -c.z[e];   // the other sign of the same attitude
    c.r.assign(13, 1e-4); c.r[7] = c.r[8] = c.r[9] = -1.0;
    // the validators
    int bad1[3] = {0, 6, 1}, bad2[3] = {-2, 0, 1}, bad3[3] = {3, -1, 3}, good[3] = {-1, -1, -1};
    std::vector<double> asym = c.Pa, slot = c.Pa;
    asym[2 * 16 + 14] += 1e-6;
    slot[14 * 16 + 3] = 1e-300; slot[3 * 16 + 14] = 1e-300;
    if (ekf_sel_ok(bad1) || ekf_sel_ok(bad2) || ekf_sel_ok(bad3) || !ekf_sel_ok(good) || !ekf_sel_ok(c.sel) ||
        !unc_sym_ok<16>(c.Pa.data(), 1) || unc_sym_ok<16>(asym.data(), 1) || !unc_sym_ok<16>(slot.data(), 1) ||
        !ekf_unused_zero(c.Pa.data(), 1, c.sel) || ekf_unused_zero(slot.data(), 1, c.sel) || !unc_sym_ok(c.Q.data(), 1)) {
        printf("ekf_aug_check FAILED: the validators\n");
        return 1;
    }
    double x[13], dn[ND], nis = 0.0;
    int counts[2];
    std::vector<double> Pa;
    step(c, x, dn, Pa, nis, counts);
    if (nis != 0.0 || counts[0] != 0 || counts[1] != 0 || std::memcmp(dn, c.d.data(), sizeof dn) != 0) {
        printf("ekf_aug_check FAILED: predict-only statistics\n");
        return 1;
    }
    if (Pa[14 * 17] != 0.0 || !ekf_unused_zero(Pa.data(), 1, c.sel)) { printf("ekf_aug_check FAILED: the unused slot took part\n"); return 1; }
    c.has_z = 1;
    step(c, x, dn, Pa, nis, counts);
    double as = 0, big = 0;
    for (int a = 0; a < 16; a++)
        for (int b = 0; b < 16; b++) {
            if (!std::isfinite(Pa[a * 16 + b]) || !std::isfinite(x[a % 13])) { printf("ekf_aug_check FAILED: step not finite\n"); return 1; }
            as = std::fmax(as, std::fabs(Pa[a * 16 + b] - Pa[b * 16 + a]));
            big = std::fmax(big, std::fabs(Pa[a * 16 + b]));
        }
    const double qn = std::sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5] + x[6] * x[6]);
    if (!(as <= 1e-12 * big) || counts[0] != 9 || counts[1] != 1 || !(std::fabs(qn - 1.0) <= 1e-15) || !(nis > 0.0) || !(x[3] > 0.0) ||
        dn[1] != c.d[1] || dn[0] != c.d[0] || dn[3] != c.d[3] || dn[5] != c.d[5] || !ekf_unused_zero(Pa.data(), 1, c.sel) ||
        !unc_sym_ok<16>(Pa.data(), 1)) {
        printf("ekf_aug_check FAILED: built-in step: asymmetry %.3e of %.3e, counts (%d, %d), |q| - 1 = %.3e\n", as, big, counts[0],
               counts[1], qn - 1.0);
        return 1;
    }
    printf("ekf_aug_check ok: built-in checks, asymmetry %.3e of %.3e\n", as, big);
    return 0;
}

}  // namespace

int main(int argc, char** argv) { return argc > 1 ? run_file(argv[1]) : run_builtin(); }
