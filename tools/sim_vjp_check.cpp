// sim_vjp_check -- the reverse RK4 sub-step of csrc/cfnmpc_simvjp.hpp compiled for the HOST and run under AddressSanitizer and
// UndefinedBehaviorSanitizer (make -C crazyflie_nmpc_amd/csrc sim_vjp_check [CASES=file]); plain C++ with its own main, nothing
// of it is loaded into Python.  It sweeps a stored rollout backwards exactly as k_sim_rollout_vjp does (sub-step start states
// recomputed from xs[t]; rk4_substep_vjp; derive_k_t once at the end) and compares with the gradients a case file holds.
//
// Case file (text, written by tests/test_sim_vjp_cpu.py from its complex-step reference):
//     n_cases
//     L steps kind T            kind 0: folded constants, 1: parameter row, 2: parameter row + disturbance row
//     p[8]   d[6]   xs[(L+1)*13]   u[L*4]   gxs[(L+1)*13]
//     gx0[13]   gu[L*4]   gp[8]   gd[6]                    (expected)
// Error measure per output array: max |difference| / max(1, max |expected|), the parameter gradient as gp * p; bound 1e-12.
// Without a file: the transpose of derive_k's Jacobian against central differences of derive_k at the nominal row, and one
// reverse step on fixed data (for the sanitizers).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../crazyflie_nmpc_amd/csrc/cfnmpc_simvjp.hpp"

using namespace cfn;

namespace {

template <class K>
void rk4_host(double (&xc)[13], const double (&uc)[4], double h, int steps, const K& mk) {
    double k1[13], k2[13], k3[13], k4[13], xt[13];
    for (int s = 0; s < steps; s++) {
        f_expl(xc, uc, k1, mk);
        for (int e = 0; e < 13; e++) xt[e] = xc[e] + 0.5 * h * k1[e];
        f_expl(xt, uc, k2, mk);
        for (int e = 0; e < 13; e++) xt[e] = xc[e] + 0.5 * h * k2[e];
        f_expl(xt, uc, k3, mk);
        for (int e = 0; e < 13; e++) xt[e] = xc[e] + h * k3[e];
        f_expl(xt, uc, k4, mk);
        for (int e = 0; e < 13; e++) xc[e] += (h / 6.0) * (k1[e] + 2 * k2[e] + 2 * k3[e] + k4[e]);
    }
}

struct Case {
    int L, steps, kind;
    double T;
    std::vector<double> p, d, xs, u, gxs, gx0, gu, gp, gd;
};

template <class K>
void sweep(const Case& c, const K& mk, std::vector<double>& gx0, std::vector<double>& gu, std::vector<double>& gp,
           std::vector<double>& gd) {
    const double h = c.T / c.steps;
    SimGrad G{};
    double lam[13];
    for (int e = 0; e < 13; e++) lam[e] = c.gxs[(size_t)c.L * 13 + e];
    for (int t = c.L - 1; t >= 0; t--) {
        double xt[13], uc[4], gut[4] = {0, 0, 0, 0};
        for (int e = 0; e < 13; e++) xt[e] = c.xs[(size_t)t * 13 + e];
        for (int e = 0; e < 4; e++) uc[e] = c.u[(size_t)t * 4 + e];
        for (int s = c.steps - 1; s >= 0; s--) {
            double xc[13];
            for (int e = 0; e < 13; e++) xc[e] = xt[e];
            rk4_host(xc, uc, h, s, mk);
            rk4_substep_vjp(xc, uc, h, lam, gut, G, mk);
        }
        for (int e = 0; e < 13; e++) lam[e] += c.gxs[(size_t)t * 13 + e];
        for (int e = 0; e < 4; e++) gu[(size_t)t * 4 + e] = gut[e];
    }
    for (int e = 0; e < 13; e++) gx0[e] = lam[e];
    derive_k_t(c.p.data(), G.gk, gp.data());
    for (int e = 0; e < ND; e++) gd[e] = G.gd[e];
}

double err(const std::vector<double>& a, const std::vector<double>& ref, const double* scale = nullptr) {
    double num = 0, den = 1;
    for (size_t i = 0; i < ref.size(); i++) {
        const double s = scale ? scale[i] : 1.0;
        num = std::fmax(num, std::fabs(a[i] * s - ref[i] * s));
        den = std::fmax(den, std::fabs(ref[i] * s));
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
    if (!f) { fprintf(stderr, "sim_vjp_check: cannot open %s\n", path); return 2; }
    int n = 0;
    if (fscanf(f, "%d", &n) != 1 || n < 1) { fclose(f); fprintf(stderr, "sim_vjp_check: bad case file\n"); return 2; }
    double worst = 0;
    for (int ci = 0; ci < n; ci++) {
        Case c;
        if (fscanf(f, "%d %d %d %lf", &c.L, &c.steps, &c.kind, &c.T) != 4 || c.L < 1 || c.L > 4096 || c.steps < 1 || c.steps > 64 ||
            c.kind < 0 || c.kind > 2) {
            fclose(f); fprintf(stderr, "sim_vjp_check: bad header of case %d\n", ci); return 2;
        }
        const size_t ns = (size_t)(c.L + 1) * 13, nu = (size_t)c.L * 4;
        if (!(read(f, c.p, NPAR) && read(f, c.d, ND) && read(f, c.xs, ns) && read(f, c.u, nu) && read(f, c.gxs, ns) &&
              read(f, c.gx0, 13) && read(f, c.gu, nu) && read(f, c.gp, NPAR) && read(f, c.gd, ND))) {
            fclose(f); fprintf(stderr, "sim_vjp_check: case %d is short\n", ci); return 2;
        }
        std::vector<double> gx0(13), gu(nu), gp(NPAR), gd(ND);
        if (c.kind == 0) {
            sweep(c, NomK(), gx0, gu, gp, gd);
        } else {
            DstK mk;
            double kr[NK];
            derive_k(c.p.data(), kr);
            for (int e = 0; e < 8; e++) mk.c[e] = kr[e];
            for (int e = 0; e < ND; e++) mk.d[e] = c.d[e];
            if (c.kind == 1) sweep(c, static_cast<const ParK&>(mk), gx0, gu, gp, gd);
            else sweep(c, mk, gx0, gu, gp, gd);
        }
        const double e4[4] = {err(gx0, c.gx0), err(gu, c.gu), err(gp, c.gp, c.p.data()), err(gd, c.gd)};
        for (int k = 0; k < 4; k++) {
            worst = std::fmax(worst, e4[k]);
            if (!(e4[k] <= 1e-12)) {
                fclose(f);
                printf("sim_vjp_check FAILED: case %d (L %d, steps %d, kind %d), output %d: scaled error %.3e > 1e-12\n", ci, c.L,
                       c.steps, c.kind, k, e4[k]);
                return 1;
            }
        }
    }
    fclose(f);
    printf("sim_vjp_check ok: %d cases, worst scaled error %.3e\n", n, worst);
    return 0;
}

int run_builtin() {
    // (d derive_k / dp)' gk against central differences, at the nominal row
    double p[NPAR], gk[8], gp[NPAR];
    for (int e = 0; e < NPAR; e++) p[e] = NOM_P[e];
    for (int e = 0; e < 8; e++) gk[e] = 0.25 + 0.125 * e;
    derive_k_t(p, gk, gp);
    double worst = 0;
    for (int j = 0; j < NPAR; j++) {
        double pp[NPAR], pm[NPAR], kp[NK], km[NK];
        for (int e = 0; e < NPAR; e++) { pp[e] = p[e]; pm[e] = p[e]; }
        const double hh = 1e-6 * p[j];
        pp[j] += hh; pm[j] -= hh;
        derive_k(pp, kp); derive_k(pm, km);
        double fd = 0;
        for (int e = 0; e < 8; e++) fd += gk[e] * (kp[e] - km[e]) / (pp[j] - pm[j]);
        worst = std::fmax(worst, std::fabs(fd - gp[j]) * p[j] / std::fmax(1.0, std::fabs(gp[j]) * p[j]));
    }
    if (!(worst <= 1e-6)) { printf("sim_vjp_check FAILED: derive_k transpose against differences: %.3e\n", worst); return 1; }
    // one reverse step on fixed data
    double x[13] = {0.1, -0.2, 0.3, 0.98, 0.1, -0.1, 0.05, 0.3, -0.2, 0.1, 0.5, -0.4, 0.3}, u[4] = {15.0, 16.0, 15.5, 16.5};
    double lam[13], gu[4] = {0, 0, 0, 0};
    for (int e = 0; e < 13; e++) lam[e] = 1.0 - 0.1 * e;
    SimGrad G{};
    rk4_substep_vjp(x, u, 0.015, lam, gu, G, NomK());
    for (int e = 0; e < 13; e++)
        if (!std::isfinite(lam[e])) { printf("sim_vjp_check FAILED: reverse step not finite\n"); return 1; }
    printf("sim_vjp_check ok: built-in checks, derive_k transpose %.3e\n", worst);
    return 0;
}

}  // namespace

int main(int argc, char** argv) { return argc > 1 ? run_file(argv[1]) : run_builtin(); }
