// ekf_check -- one instance's extended Kalman filter step (csrc/cfnmpc_ekf.hpp: ekf_predict, ekf_update, plain loops) compiled for
// the HOST and run under AddressSanitizer and UndefinedBehaviorSanitizer (make -C crazyflie_nmpc_amd/csrc ekf_check [CASES=file]);
// plain C++ with its own main, nothing of it is loaded into Python and nothing of it runs on a GPU.
//
// Case file (text, written by tests/test_ekf_cpu.py from its numpy twin):
//     n_cases
//     steps kind T gate flags has_Q has_z      kind 0: folded constants, 1: parameter row, 2: parameter row + disturbance row
//     p[8]   d[6]   x[13]   P[169]   u[4]   Q[169]   z[13]   r[13]
//     x_new[13]   P_new[169]   nis   used   rejected              (expected)
// Error measure per output array: max |difference| / max(max |expected|, 1e-12); bound 1e-12; the counts exactly.
// Without a file: a predict-only and a full step on fixed data: finite, symmetric, counts as expected (for the sanitizers).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../crazyflie_nmpc_amd/csrc/cfnmpc_ekf.hpp"

using namespace cfn;

namespace {

struct Case {
    int steps, kind, flags, has_Q, has_z;
    double T, gate;
    std::vector<double> p, d, x, P, u, Q, z, r, xn, Pn;
    double nis;
    int used, rejected;
};

template <class K>
void step(const Case& c, const K& mk, double (&x)[13], std::vector<double>& P, double& nis, int (&counts)[2]) {
    double u[4];
    for (int e = 0; e < 13; e++) x[e] = c.x[e];
    for (int e = 0; e < 4; e++) u[e] = c.u[e];
    P = c.P;
    nis = 0.0;
    counts[0] = 0; counts[1] = 0;
    ekf_predict(x, P.data(), u, c.T, c.steps, c.has_Q ? c.Q.data() : nullptr, mk);
    if (c.has_z) ekf_update(x, P.data(), c.z.data(), c.r.data(), c.gate, c.flags, nis, counts);
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

template <class F>
void with_model(const Case& c, F&& fn) {
    if (c.kind == 0) {
        fn(NomK());
        return;
    }
    DstK mk;
    double kr[NK];
    derive_k(c.p.data(), kr);
    for (int e = 0; e < 8; e++) mk.c[e] = kr[e];
    for (int e = 0; e < ND; e++) mk.d[e] = c.d[e];
    if (c.kind == 1) fn(static_cast<const ParK&>(mk));
    else fn(mk);
}

int run_file(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) { fprintf(stderr, "ekf_check: cannot open %s\n", path); return 2; }
    int n = 0;
    if (fscanf(f, "%d", &n) != 1 || n < 1) { fclose(f); fprintf(stderr, "ekf_check: bad case file\n"); return 2; }
    double worst = 0;
    for (int ci = 0; ci < n; ci++) {
        Case c;
        if (fscanf(f, "%d %d %lf %lf %d %d %d", &c.steps, &c.kind, &c.T, &c.gate, &c.flags, &c.has_Q, &c.has_z) != 7 || c.steps < 1 ||
            c.steps > 64 || c.kind < 0 || c.kind > 2) {
            fclose(f); fprintf(stderr, "ekf_check: bad header of case %d\n", ci); return 2;
        }
        std::vector<double> tail;
        if (!(read(f, c.p, NPAR) && read(f, c.d, ND) && read(f, c.x, 13) && read(f, c.P, 169) && read(f, c.u, 4) && read(f, c.Q, 169) &&
              read(f, c.z, 13) && read(f, c.r, 13) && read(f, c.xn, 13) && read(f, c.Pn, 169) && read(f, tail, 3))) {
            fclose(f); fprintf(stderr, "ekf_check: case %d is short\n", ci); return 2;
        }
        c.nis = tail[0]; c.used = (int)tail[1]; c.rejected = (int)tail[2];
        double x[13], nis = 0.0;
        int counts[2] = {0, 0};
        std::vector<double> P;
        with_model(c, [&](const auto& mk) { step(c, mk, x, P, nis, counts); });
        const double e3[3] = {err(x, c.xn.data(), 13), err(P.data(), c.Pn.data(), 169), err(&nis, &c.nis, 1)};
        for (int k = 0; k < 3; k++) {
            worst = std::fmax(worst, e3[k]);
            if (!(e3[k] <= 1e-12)) {
                fclose(f);
                printf("ekf_check FAILED: case %d (steps %d, kind %d), output %d: error %.3e > 1e-12\n", ci, c.steps, c.kind, k, e3[k]);
                return 1;
            }
        }
        if (counts[0] != c.used || counts[1] != c.rejected) {
            fclose(f);
            printf("ekf_check FAILED: case %d: counts (%d, %d), expected (%d, %d)\n", ci, counts[0], counts[1], c.used, c.rejected);
            return 1;
        }
    }
    fclose(f);
    printf("ekf_check ok: %d cases, worst error %.3e\n", n, worst);
    return 0;
}

int run_builtin() {
    Case c;
    c.steps = 3; c.kind = 0; c.flags = EKF_NORMALIZE_Q; c.has_Q = 1; c.has_z = 0; c.T = 0.015; c.gate = 3.0;
    c.x = {0.1, -0.2, 0.3, 0.98, 0.1, -0.1, 0.05, 0.3, -0.2, 0.1, 0.5, -0.4, 0.3};
    c.u = {15.0, 16.0, 15.5, 16.5};
    c.P.assign(169, 0.0); c.Q.assign(169, 0.0);
    for (int e = 0; e < 13; e++) { c.P[e * 14] = 0.01 * (1 + e); c.Q[e * 14] = 1e-6; }
    c.z = c.x; c.z[0] += 0.01; c.z[1] += 5.0;   // the second component: far outside the gate
    for (int e = 3; e < 7; e++) c.z[e] = -c.z[e];   // the other sign of the same attitude
    c.r.assign(13, 1e-4); c.r[7] = c.r[8] = c.r[9] = -1.0;
    double x[13], nis = 0.0;
    int counts[2];
    std::vector<double> P;
    step(c, NomK(), x, P, nis, counts);
    if (nis != 0.0 || counts[0] != 0 || counts[1] != 0) { printf("ekf_check FAILED: predict-only statistics\n"); return 1; }
    c.has_z = 1;
    step(c, NomK(), x, P, nis, counts);
    double asym = 0, big = 0;
    for (int a = 0; a < 13; a++)
        for (int b = 0; b < 13; b++) {
            if (!std::isfinite(P[a * 13 + b]) || !std::isfinite(x[a])) { printf("ekf_check FAILED: step not finite\n"); return 1; }
            asym = std::fmax(asym, std::fabs(P[a * 13 + b] - P[b * 13 + a]));
            big = std::fmax(big, std::fabs(P[a * 13 + b]));
        }
    const double qn = std::sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5] + x[6] * x[6]);
    if (!(asym <= 1e-12 * big) || counts[0] != 9 || counts[1] != 1 || !(std::fabs(qn - 1.0) <= 1e-15) || !(nis > 0.0) || !(x[3] > 0.0)) {
        printf("ekf_check FAILED: built-in step: asymmetry %.3e of %.3e, counts (%d, %d), |q| - 1 = %.3e\n", asym, big, counts[0],
               counts[1], qn - 1.0);
        return 1;
    }
    printf("ekf_check ok: built-in checks, asymmetry %.3e of %.3e\n", asym, big);
    return 0;
}

}  // namespace

int main(int argc, char** argv) { return argc > 1 ? run_file(argv[1]) : run_builtin(); }
