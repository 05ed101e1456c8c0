#ifndef DMRGX_HOST_TRIDIAG_QL_HPP
#define DMRGX_HOST_TRIDIAG_QL_HPP
/** Eigenvalues of a small symmetric tridiagonal matrix and the FIRST component of every eigenvector, by the implicit QL iteration
    with Wilkinson shifts (EISPACK tql2 restricted to one row of the eigenvector matrix; TridiagQLVectors below keeps all of it).
    This is all a continued fraction needs:
    for the Lanczos matrix T of a start vector v, the spectral function of v has its poles at the eigenvalues of T with the weights
    |v|^2 z_k^2 (-dsf, EngineMeasurements.hpp: DynamicalStructureFactor::Run).  Orders are the number of Lanczos steps (~100):
    host work of microseconds. */
#include <cmath>
#include <vector>

namespace dmrgx_host {

/** d[0..n): diagonal, e[0..n-1): e[i] couples i and i+1 (further entries ignored).  On return d holds the eigenvalues (unsorted) and
    z[k] the first component of the normalised eigenvector of d[k].  false: an eigenvalue did not converge in 60 iterations. */
inline bool TridiagQLFirstRow(std::vector<double>& d, std::vector<double> e, std::vector<double>& z)
{
    const int n = (int)d.size();
    z.assign((size_t)n, 0.0);
    if (n == 0) return true;
    z[0] = 1.0;
    e.resize((size_t)n, 0.0);
    e[(size_t)n - 1] = 0.0;
    const double eps = 2.220446049250313e-16;
    for (int l = 0; l < n; ++l) {
        int iter = 0, m;
        do {
            for (m = l; m < n - 1; ++m) if (std::fabs(e[m]) <= eps * (std::fabs(d[m]) + std::fabs(d[m + 1]))) break;
            if (m == l) break;
            if (iter++ == 60) return false;
            double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
            double r = std::hypot(g, 1.0);
            g = d[m] - d[l] + e[l] / (g + std::copysign(r, g));
            double s = 1.0, c = 1.0, p = 0.0;
            int i;
            for (i = m - 1; i >= l; --i) {
                double f = s * e[i];
                const double b = c * e[i];
                r = std::hypot(f, g);
                e[i + 1] = r;
                if (r == 0.0) { d[i + 1] -= p; e[m] = 0.0; break; }      /* an exact split: start over on the smaller block */
                s = f / r; c = g / r;
                g = d[i + 1] - p;
                r = (d[i] - g) * s + 2.0 * c * b;
                p = s * r;
                d[i + 1] = g + p;
                g = c * r - b;
                f = z[i + 1];                                         /* the same rotation on the first row of the eigenvector matrix */
                z[i + 1] = s * z[i] + c * f;
                z[i] = c * z[i] - s * f;
            }
            if (r == 0.0 && i >= l) continue;
            d[l] -= p; e[l] = g; e[m] = 0.0;
        } while (m != l);
    }
    return true;
}

/** The same iteration with ALL eigenvectors (EISPACK tql2): on return d holds the eigenvalues (unsorted) and vec[k * n + i] component i
    of the normalised eigenvector of d[k] -- eigenvector-major, so that a rotation walks two contiguous rows.  T = S Theta S^T with
    S[i][k] = vec[k * n + i].  For the overlaps of other vectors with a kept Lanczos basis (-dsf_sites, EngineMeasurements.hpp:
    DynamicalCorrelations::Run), which need more of S than its first row.  Orders up to a few hundred: 3 n^3 flops, milliseconds.
    false: an eigenvalue did not converge in 60 iterations. */
inline bool TridiagQLVectors(std::vector<double>& d, std::vector<double> e, std::vector<double>& vec)
{
    const int n = (int)d.size();
    vec.assign((size_t)n * (size_t)n, 0.0);
    if (n == 0) return true;
    for (int i = 0; i < n; ++i) vec[(size_t)i * (size_t)n + (size_t)i] = 1.0;
    e.resize((size_t)n, 0.0);
    e[(size_t)n - 1] = 0.0;
    const double eps = 2.220446049250313e-16;
    for (int l = 0; l < n; ++l) {
        int iter = 0, m;
        do {
            for (m = l; m < n - 1; ++m) if (std::fabs(e[m]) <= eps * (std::fabs(d[m]) + std::fabs(d[m + 1]))) break;
            if (m == l) break;
            if (iter++ == 60) return false;
            double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
            double r = std::hypot(g, 1.0);
            g = d[m] - d[l] + e[l] / (g + std::copysign(r, g));
            double s = 1.0, c = 1.0, p = 0.0;
            int i;
            for (i = m - 1; i >= l; --i) {
                double f = s * e[i];
                const double b = c * e[i];
                r = std::hypot(f, g);
                e[i + 1] = r;
                if (r == 0.0) { d[i + 1] -= p; e[m] = 0.0; break; }      /* an exact split: start over on the smaller block */
                s = f / r; c = g / r;
                g = d[i + 1] - p;
                r = (d[i] - g) * s + 2.0 * c * b;
                p = s * r;
                d[i + 1] = g + p;
                g = c * r - b;
                double* zi = vec.data() + (size_t)i * (size_t)n;      /* the same rotation on columns i, i + 1 of S: rows i, i + 1 here */
                double* zj = zi + n;
                for (int k = 0; k < n; ++k) {
                    f = zj[k];
                    zj[k] = s * zi[k] + c * f;
                    zi[k] = c * zi[k] - s * f;
                }
            }
            if (r == 0.0 && i >= l) continue;
            d[l] -= p; e[l] = g; e[m] = 0.0;
        } while (m != l);
    }
    return true;
}

}  // namespace dmrgx_host
#endif
