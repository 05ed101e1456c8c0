// The host side of a thick-restart Lanczos cycle, shared by eigs.hip and eigs_orth.hip: the small symmetric eigenproblem and the
// Rayleigh-Ritz step on the coefficient rows the device recorded.  Internal, not part of the ABI.  Plain C++: no device code.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace dmrgx {

// all eigenpairs of the symmetric A (row-major order n, destroyed) by cyclic Jacobi: ascending values (equal ones in the order of their
// diagonal positions), vectors in the columns of Q (row-major n x n)
inline void jacobi_eigh(int n, std::vector<double>& A, std::vector<double>& w, std::vector<double>& Q)
{
    auto a = [&](int i, int j) -> double& { return A[(size_t)i * n + j]; };
    std::vector<double> U((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) U[(size_t)i * n + i] = 1.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < n; ++i) { diag += a(i, i) * a(i, i); for (int j = i + 1; j < n; ++j) off += a(i, j) * a(i, j); }
        if (off <= 1e-32 * (diag + off) || off == 0.0) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a(p, q);
                if (apq == 0.0) continue;
                const double tau = (a(q, q) - a(p, p)) / (2.0 * apq);
                const double t = (tau >= 0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                for (int k = 0; k < n; ++k) { const double x = a(k, p), y = a(k, q); a(k, p) = c * x - s * y; a(k, q) = s * x + c * y; }
                for (int k = 0; k < n; ++k) { const double x = a(p, k), y = a(q, k); a(p, k) = c * x - s * y; a(q, k) = s * x + c * y; }
                for (int k = 0; k < n; ++k) { double& x = U[(size_t)k * n + p]; double& y = U[(size_t)k * n + q]; const double u = x, v = y; x = c * u - s * v; y = s * u + c * v; }
            }
    }
    std::vector<int> idx(n);
    for (int i = 0; i < n; ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return a(x, x) < a(y, y); });
    w.resize(n);
    Q.assign((size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j) { w[j] = a(idx[j], idx[j]); for (int i = 0; i < n; ++i) Q[(size_t)i * n + j] = U[(size_t)i * n + idx[j]]; }
}

// Rayleigh-Ritz on the leading mm columns of a cycle's projected matrix.  The cycle began with kept.size() Ritz vectors, whose block is
// diag(kept); the later columns come from the coefficient rows the device recorded (hbuf: `row` doubles per step, slot m + 1 beta^2).
struct Ritz {
    std::vector<double> th, Q;      // ascending Ritz values, their vectors in the columns (row-major mm x mm)
    double resid;                   // residual estimate of the lowest pair: |beta_mm Q[mm - 1][0]|
};
inline Ritz ritz_of_leading(int mm, int m, int row, const std::vector<double>& hbuf, const std::vector<double>& kept)
{
    const int k = (int)kept.size();
    std::vector<double> A((size_t)mm * mm, 0.0);
    for (int j = 0; j < mm; ++j) for (int i = 0; i <= j; ++i) {
        const double v = j >= k ? hbuf[(size_t)j * row + i] : (i == j ? kept[j] : 0.0);
        A[(size_t)i * mm + j] = v; A[(size_t)j * mm + i] = v;
    }
    Ritz r;
    jacobi_eigh(mm, A, r.th, r.Q);
    r.resid = std::fabs(std::sqrt(std::max(0.0, hbuf[(size_t)(mm - 1) * row + m + 1])) * r.Q[(size_t)(mm - 1) * mm + 0]);
    return r;
}

}  // namespace dmrgx
