// Host half of the Lanczos variance cache of the iterative exact-GP class (cglb_itergp_var_cache, include/cglb_hip.h) - plain C++, no HIP.
// The Lanczos run on K = variance kappa(X, X) + noise I leaves T = tridiag(alpha, beta) of order J; K^-1 ~ Q T^-1 Q^T = R R^T with R = Q L^-T and
// T = L L^T, L lower bidiagonal:
//   d_0 = sqrt(alpha_0),  l_{j-1} = beta_{j-1} / d_{j-1},  d_j = sqrt(alpha_j - l_{j-1}^2)
// and the columns of R follow on the device from R_j = (Q_j - l_{j-1} R_{j-1}) / d_j.
#pragma once
#include <cmath>
#include <vector>

// Stop rule of the Lanczos run after step j (J = j + 1 columns so far): the requested rank is reached, or the Krylov space has closed
// (beta_j <= 1e-10 alpha_0; a beta that is not a number closes it as well).
static inline bool lanczos_stop(int j, int rank, double beta_j, double alpha_0) { return j + 1 >= rank || !(beta_j > 1e-10 * alpha_0); }

// diag[J] and sub[J] (sub[j] = L[j + 1][j]; sub[J - 1] is not part of the J x J factor and is left 0) of T = L L^T; alpha: [J], beta: [>= J - 1].
// Returns 0, or 1 + j at the first pivot alpha_j - l_{j-1}^2 that is not positive (not a number included).
static inline int lanczos_bidiag_factor(const double* alpha, const double* beta, int J, std::vector<double>& diag, std::vector<double>& sub) {
    diag.assign((size_t)(J > 0 ? J : 0), 0.0);
    sub.assign((size_t)(J > 0 ? J : 0), 0.0);
    double lprev = 0.0;
    for (int j = 0; j < J; ++j) {
        const double pivot = alpha[j] - lprev * lprev;
        if (!(pivot > 0.0) || !std::isfinite(pivot)) return 1 + j;
        diag[j] = std::sqrt(pivot);
        if (j + 1 < J) {
            sub[j] = beta[j] / diag[j];
            lprev = sub[j];
        }
    }
    return 0;
}
