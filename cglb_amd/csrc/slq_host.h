// Stochastic Lanczos quadrature from the scalars of a (preconditioned) CG run - host only, no HIP: the iterative exact-GP class
// (cglb_itergp_*, include/cglb_hip.h) turns the per-iteration rz_j = r_j^T P r_j and pAp_j = p_j^T K p_j of every probe column into the
// Lanczos tridiagonal of P^-1/2 K P^-1/2 started at the normalised probe, and e_1^T log(T) e_1 into its share of log|P^-1 K|.
//   gamma_j = rz_j / pAp_j,  beta_j = rz_{j+1} / rz_j
//   T[j][j] = 1 / gamma_j + beta_{j-1} / gamma_{j-1} (second term absent at j = 0),  T[j][j+1] = sqrt(beta_j) / gamma_j
// The eigen-solve is the implicit QL iteration on a symmetric tridiagonal; only the first components of the eigenvectors are carried.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

// Number of Lanczos steps column `col` of the logs supports: min(steps, lanczos_iter), cut at the first j whose gamma_j or rz_j is zero or
// not finite (a converged or broken-down column).  rz: [steps + 1][ld], pap: [steps][ld].
static inline int slq_usable_steps(const double* rz, const double* pap, int steps, int ld, int col, int lanczos_iter) {
    int J = steps < lanczos_iter ? steps : lanczos_iter;
    if (J < 0) J = 0;
    for (int j = 0; j < J; ++j) {
        const double r = rz[(int64_t)j * ld + col], q = pap[(int64_t)j * ld + col];
        const double gamma = r / q;
        if (!(r != 0.0) || !std::isfinite(r) || !(gamma != 0.0) || !std::isfinite(gamma)) return j;
    }
    return J;
}

// diag[J], off[J] (off[j] = T[j][j+1]; off[J-1] is not part of the J x J matrix and is left 0) of column `col`
static inline void slq_tridiagonal(const double* rz, const double* pap, int ld, int col, int J, std::vector<double>& diag, std::vector<double>& off) {
    diag.assign((size_t)J, 0.0);
    off.assign((size_t)J, 0.0);
    double gprev = 0.0, bprev = 0.0;
    for (int j = 0; j < J; ++j) {
        const double r = rz[(int64_t)j * ld + col];
        const double gamma = r / pap[(int64_t)j * ld + col];
        diag[j] = 1.0 / gamma + (j > 0 ? bprev / gprev : 0.0);
        const double beta = rz[(int64_t)(j + 1) * ld + col] / r;
        if (j + 1 < J) off[j] = std::sqrt(beta) / gamma;
        gprev = gamma;
        bprev = beta;
    }
}

// Eigenvalues of the symmetric tridiagonal (d[n], e[n] with e[j] = T[j][j+1], e[n-1] ignored) and the squared first components of its
// orthonormal eigenvectors: on return d holds the eigenvalues and w[k] = V[0][k]^2.  Implicit QL with Wilkinson shifts; returns 0, or 1 if
// an eigenvalue did not converge within 60 sweeps.
static inline int slq_eig_first_row(std::vector<double>& d, std::vector<double>& e, std::vector<double>& w) {
    const int n = (int)d.size();
    std::vector<double> z((size_t)n, 0.0);  // first row of the accumulated rotations
    if (n > 0) z[0] = 1.0;
    if (n > 0) e[n - 1] = 0.0;
    for (int l = 0; l < n; ++l) {
        int iter = 0, m;
        do {
            for (m = l; m < n - 1; ++m) {
                const double dd = std::fabs(d[m]) + std::fabs(d[m + 1]);
                if (std::fabs(e[m]) <= 2.220446049250313e-16 * dd) break;
            }
            if (m != l) {
                if (iter++ == 60) return 1;
                double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
                double r = std::hypot(g, 1.0);
                g = d[m] - d[l] + e[l] / (g + (g >= 0.0 ? std::fabs(r) : -std::fabs(r)));
                double s = 1.0, c = 1.0, p = 0.0;
                int i;
                for (i = m - 1; i >= l; --i) {
                    double f = s * e[i];
                    const double b = c * e[i];
                    r = std::hypot(f, g);
                    e[i + 1] = r;
                    if (r == 0.0) {  // recover from underflow
                        d[i + 1] -= p;
                        e[m] = 0.0;
                        break;
                    }
                    s = f / r;
                    c = g / r;
                    g = d[i + 1] - p;
                    r = (d[i] - g) * s + 2.0 * c * b;
                    p = s * r;
                    d[i + 1] = g + p;
                    g = c * r - b;
                    f = z[i + 1];
                    z[i + 1] = s * z[i] + c * f;
                    z[i] = c * z[i] - s * f;
                }
                if (r == 0.0 && i >= l) continue;
                d[l] -= p;
                e[l] = g;
                e[m] = 0.0;
            }
        } while (m != l);
    }
    w.resize((size_t)n);
    for (int k = 0; k < n; ++k) w[k] = z[k] * z[k];
    return 0;
}

// e_1^T log(T) e_1 = sum_k V[0][k]^2 log lambda_k.  *status: 0, 1 (no convergence) or 2 (an eigenvalue that is not positive).
static inline double slq_e1_log_e1(std::vector<double> diag, std::vector<double> off, int* status) {
    std::vector<double> w;
    int st = slq_eig_first_row(diag, off, w);
    double s = 0.0;
    for (size_t k = 0; k < diag.size(); ++k) {
        if (!(diag[k] > 0.0)) { if (st == 0) st = 2; continue; }
        s += w[k] * std::log(diag[k]);
    }
    if (status) *status = st;
    return s;
}

// (1 / t) sum_{i = 1..t} rz_0,i e_1^T log(T_i) e_1 over the probe columns 1 .. t of the logs (column 0 is the data column): the estimate of
// log|P^-1 K| = tr log(P^-1/2 K P^-1/2) from probes z_i ~ N(0, P), whose |P^-1/2 z_i|^2 is rz_0,i.
static inline double slq_logdet_correction(const double* rz, const double* pap, int steps, int t, int lanczos_iter, int* status) {
    const int ld = 1 + t;
    double sum = 0.0;
    int worst = 0;
    std::vector<double> diag, off;
    for (int i = 1; i <= t; ++i) {
        const int J = slq_usable_steps(rz, pap, steps, ld, i, lanczos_iter);
        if (J == 0) continue;
        slq_tridiagonal(rz, pap, ld, i, J, diag, off);
        int st = 0;
        sum += rz[i] * slq_e1_log_e1(diag, off, &st);
        if (st > worst) worst = st;
    }
    if (status) *status = worst;
    return t > 0 ? sum / t : 0.0;
}
