// Correction vectors of the planned superblock Hamiltonian: 1 / (sigma + i eta - H) v0 = X + i Y at one (sigma, eta), by conjugate
// gradients on the positive definite A = (H - sigma)^2 + eta^2 (Kuehner-White; the linear solve inside Jeckelmann's DDMRG).  An engine
// extension like the Lanczos and Chebyshev calls of lanczos.hip, in their idiom: the iteration lives on the device.
//   Y = -eta A^-1 v0,  X = (H - sigma) Y / eta;  <u, Y> = -sum_n <u|n><n|v0> eta / ((sigma - E_n)^2 + eta^2): a true Lorentzian.
// CG on A y = b, b = -eta v0, y_0 = 0, r_0 = p_0 = b.  Per iteration, on four pool vectors r, p, s, t (u = H s reuses t) and the caller's Y:
//   MatMult        : t = H p
//   s              : s = t - sigma p ; partial sums of s . s and p . p                         (reads 2 vectors, writes 1)
//   scalars 1      : alpha = rr / (s.s + eta^2 p.p) -- p.A p as a sum of squares, no third MatMult; not positive and finite -> dead
//   MatMult        : u = H s
//   residual       : r -= alpha (u - sigma s + eta^2 p) ; partial sums of r . r                (reads 4, writes 1)
//   scalars 2      : a non-finite sum -> dead, the iteration does not count; else it counts: beta = rr_new / rr, converged when
//                    rr_new <= tol^2 b.b, stopped when the count reaches max_it
//   direction      : only for an iteration that counted: y += alpha p ; p = r + beta p unless converged   (reads 3, writes 2)
// y takes alpha p in the direction kernel, after scalars 2 has seen rr_new: an iteration whose residual sum is not finite never
// reaches Y.  (r does take it -- r is scratch.)  Once the stop flag is set -- converged, dead or max_it reached -- the vector kernels
// return at once and the scalar stages change nothing: the MatMults that remain in the enqueued block run on the frozen p and s.
// After the loop: p = y, t = H p, s = t - sigma y = eta X, X = s / eta, u = H s, true residual |b - (u - sigma s + eta^2 y)| / |b|.
// The MatMult sees the pairs (p, t) and (s, t) only.  Iterations are enqueued in blocks of check_every; one small copy per block brings
// the scalars back.  Fixed grids, partials added in block order by one workgroup, no atomics: the same bits whatever check_every is.
// What this run shares with response.hip -- the scalar slots, the direction kernel, the decisions of scalars 1 and 2, the checks, the block
// loop, the stats -- is cg.h.
#include "cg.h"

namespace dmrgx {
namespace {

// the device scalars are the common ones; the overlaps <u_i, Y>, <u_i, X> follow from CG_NS on

// partial[b] = sum of x[e]^2 over block b's range (lanczos.hip strides the whole grid: other bits).  (x is the caller's: 8-byte loads)
__global__ void __launch_bounds__(RANGE_THREADS) cv_norm2_kernel(const double* __restrict__ x, int64_t n, double* __restrict__ partial)
{
    double acc = 0.0;
    for (int64_t e = range_first(); e < range_end(n); e += RANGE_THREADS) acc += x[e] * x[e];
    acc = block_sum<RANGE_THREADS>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// r = p = -eta v0, y = 0; a refused v0: exact zeros everywhere, whatever v0 holds
__global__ void __launch_bounds__(RANGE_THREADS) cv_start_kernel(const double* __restrict__ v0, double* __restrict__ r, double* __restrict__ p, double* __restrict__ y, int64_t n,
                                                                double eta, const double* __restrict__ S)
{
    const bool dead = S[CG_DEAD] != 0.0;
    for (int64_t e = range_first(); e < range_end(n); e += RANGE_THREADS) {
        const double b = dead ? 0.0 : -eta * v0[e];
        r[e] = b;
        p[e] = b;
        y[e] = 0.0;
    }
}

// s = t - sigma p; partial[b] = s . s, partial[gridDim.x + b] = p . p over block b.  (t, p, s: pool blocks, 16-byte pairs)
__global__ void __launch_bounds__(RANGE_THREADS) cv_s_kernel(const double* __restrict__ t, const double* __restrict__ p, double* __restrict__ s, int64_t n, double sigma,
                                                            const double* __restrict__ S, double* __restrict__ partial)
{
    if (S[CG_STOP] != 0.0) return;
    double2 tr[RANGE_PAIRS], pr[RANGE_PAIRS];
#pragma unroll
    for (int i = 0; i < RANGE_PAIRS; ++i) {
        const int64_t e = range_pair(i);
        tr[i] = load2<true>(t, e, n);
        pr[i] = load2<true>(p, e, n);
    }
    double ss = 0.0, pp = 0.0;
#pragma unroll
    for (int i = 0; i < RANGE_PAIRS; ++i) {
        const int64_t e = range_pair(i);
        double2 x;
        x.x = tr[i].x - sigma * pr[i].x;
        x.y = tr[i].y - sigma * pr[i].y;
        store2<true>(s, e, n, x);
        ss += x.x * x.x; ss += x.y * x.y;                        // (beyond n the registers hold zeros)
        pp += pr[i].x * pr[i].x; pp += pr[i].y * pr[i].y;
    }
    ss = block_sum<RANGE_THREADS>(ss);
    pp = block_sum<RANGE_THREADS>(pp);
    if (threadIdx.x == 0) { partial[blockIdx.x] = ss; partial[gridDim.x + blockIdx.x] = pp; }
}

// r -= alpha (u - sigma s + eta^2 p); partial[b] = r . r over block b
__global__ void __launch_bounds__(RANGE_THREADS) cv_residual_kernel(const double* __restrict__ u, const double* __restrict__ s, const double* __restrict__ p, double* __restrict__ r,
                                                                   int64_t n, double sigma, double eta2, const double* __restrict__ S, double* __restrict__ partial)
{
    if (S[CG_STOP] != 0.0) return;
    const double alpha = S[CG_ALPHA];
    double2 ur[RANGE_PAIRS], sr[RANGE_PAIRS], pr[RANGE_PAIRS], rr[RANGE_PAIRS];
#pragma unroll
    for (int i = 0; i < RANGE_PAIRS; ++i) {
        const int64_t e = range_pair(i);
        ur[i] = load2<true>(u, e, n);
        sr[i] = load2<true>(s, e, n);
        pr[i] = load2<true>(p, e, n);
        rr[i] = load2<true>(r, e, n);
    }
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < RANGE_PAIRS; ++i) {
        const int64_t e = range_pair(i);
        double2 x;
        x.x = rr[i].x - alpha * (ur[i].x - sigma * sr[i].x + eta2 * pr[i].x);
        x.y = rr[i].y - alpha * (ur[i].y - sigma * sr[i].y + eta2 * pr[i].y);
        store2<true>(r, e, n, x);
        acc += x.x * x.x; acc += x.y * x.y;
    }
    acc = block_sum<RANGE_THREADS>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// closing 1: s = t - sigma y = eta X (t = H y), X = s / eta when X is wanted; a refused v0: exact zeros.  (y, X: the caller's, 8-byte accesses)
__global__ void __launch_bounds__(RANGE_THREADS) cv_x_kernel(const double* __restrict__ t, const double* __restrict__ y, double* __restrict__ s, double* __restrict__ X, int64_t n,
                                                            double sigma, double eta, const double* __restrict__ S)
{
    const bool none = S[CG_NORM2] == 0.0;
    for (int64_t e = range_first(); e < range_end(n); e += RANGE_THREADS) {
        const double x = none ? 0.0 : t[e] - sigma * y[e];
        s[e] = x;
        if (X) X[e] = none ? 0.0 : x / eta;
    }
}

// closing 2: partial[b] = sum over block b of (b - A y)^2, b = -eta v0, A y = u - sigma s + eta^2 y (u = H s)
__global__ void __launch_bounds__(RANGE_THREADS) cv_true_residual_kernel(const double* __restrict__ v0, const double* __restrict__ u, const double* __restrict__ s, const double* __restrict__ y,
                                                                        int64_t n, double sigma, double eta, const double* __restrict__ S, double* __restrict__ partial)
{
    const bool none = S[CG_NORM2] == 0.0;
    double acc = 0.0;
    for (int64_t e = range_first(); e < range_end(n); e += RANGE_THREADS) {
        const double d = none ? 0.0 : -eta * v0[e] - (u[e] - sigma * s[e] + eta * eta * y[e]);
        acc += d * d;
    }
    acc = block_sum<RANGE_THREADS>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// One workgroup: the partials added in block order, then the scalar logic of the stage.
//   stage 0 (start):   |v0|^2; not a positive finite number (nor eta^2 |v0|^2) -> dead and stopped from the start, reported as 0
//   stage 1 (alpha):   s.s and p.p; a sum that is not finite, p.A p not positive and finite, or an alpha that is not -> dead, stopped
//   stage 2 (counted): r.r, cg_counted
//   stage 3 (closing): the squared true residual, cg_true_residual
// A stopped run passes stages 1 and 2 unchanged.
__global__ void __launch_bounds__(RANGE_THREADS) cv_scalar_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ S, int stage, double eta2, double tol2, int max_it)
{
    const double a = sum_partials<RANGE_THREADS>(partial, nblk), b = stage == 1 ? sum_partials<RANGE_THREADS>(partial + nblk, nblk) : 0.0;
    if (threadIdx.x != 0) return;
    if (stage == 0) {
        const double bb = eta2 * a;
        const bool ok = a > 0.0 && a < INFINITY && bb > 0.0 && bb < INFINITY;
        S[CG_NORM2] = ok ? a : 0.0;
        S[CG_BB] = ok ? bb : 0.0;
        S[CG_RR] = ok ? bb : 0.0;
        S[CG_DEAD] = ok ? 0.0 : 1.0;
        S[CG_STOP] = ok ? 0.0 : 1.0;
    } else if (stage == 1) {
        if (S[CG_STOP] != 0.0) return;
        const double den = a + eta2 * b, alpha = S[CG_RR] / den;
        cg_accept_alpha(S, den, alpha, a >= 0.0 && a < INFINITY && b >= 0.0 && b < INFINITY);
    } else if (stage == 2) cg_counted(S, a, tol2, max_it);
    else cg_true_residual(S, a);
}

}  // namespace
}  // namespace dmrgx

using namespace dmrgx;

extern "C" dmrgx_status dmrgx_kron_correction_vector(dmrgx_kron_plan* plan, const double* v0_dev, double sigma, double eta, double tol, int32_t max_it, int32_t check_every,
                                                     double* Y_dev, double* X_dev, int32_t nu, const double* U_dev, int64_t ldu,
                                                     double* norm2, double* im, double* re, dmrgx_cv_stats* stats, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!plan || !v0_dev || !Y_dev || !norm2 || !stats || (nu > 0 && (!im || (X_dev && !re)))) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_correction_vector: null argument");
    if (!(eta > 0.0 && eta < INFINITY) || !(fabs(sigma) < INFINITY))
        DMRGX_FAIL(DMRGX_ERR_ARG, "kron_correction_vector: sigma %g, eta %g: a finite sigma and a positive finite eta are needed", sigma, eta);
    CgRun run("kron_correction_vector", st);
    DMRGX_CHK(run.check(plan, tol, max_it, check_every, nu, U_dev, ldu));
    const int64_t n = run.n;
    const size_t nn = run.nn, u_span = run.u_span;
    if (spans_overlap(Y_dev, nn, v0_dev, nn) || spans_overlap(X_dev, nn, v0_dev, nn) || spans_overlap(Y_dev, nn, X_dev, nn) || spans_overlap(Y_dev, nn, U_dev, u_span) ||
        spans_overlap(X_dev, nn, U_dev, u_span))
        DMRGX_FAIL(DMRGX_ERR_ARG, "kron_correction_vector: Y or X overlaps v0, U or the other one");
    DMRGX_CHK(run.alloc(2, (size_t)CG_NS + 2 * (size_t)nu));
    const double tol2 = run.tol2, eta2 = eta * eta;
    const int nblk = run.nblk;
    double *const S = run.S, *const P = run.P, *const r = run.vec(0), *const p = run.vec(1), *const s = run.vec(2), *const t = run.vec(3);
    const dim3 grid((unsigned)nblk), block(RANGE_THREADS), one(1);

    hipLaunchKernelGGL(cv_norm2_kernel, grid, block, 0, st, v0_dev, n, P);
    hipLaunchKernelGGL(cv_scalar_kernel, one, block, 0, st, (const double*)P, nblk, S, 0, eta2, tol2, (int)max_it);
    hipLaunchKernelGGL(cv_start_kernel, grid, block, 0, st, v0_dev, r, p, Y_dev, n, eta, (const double*)S);
    DMRGX_HIP(hipGetLastError());
    DMRGX_CHK(run.iterate([&]() -> dmrgx_status {
        DMRGX_CHK(dmrgx_kron_apply(plan, p, t, st));
        hipLaunchKernelGGL(cv_s_kernel, grid, block, 0, st, (const double*)t, (const double*)p, s, n, sigma, (const double*)S, P);
        hipLaunchKernelGGL(cv_scalar_kernel, one, block, 0, st, (const double*)P, nblk, S, 1, eta2, tol2, (int)max_it);
        DMRGX_CHK(dmrgx_kron_apply(plan, s, t, st));
        hipLaunchKernelGGL(cv_residual_kernel, grid, block, 0, st, (const double*)t, (const double*)s, (const double*)p, r, n, sigma, eta2, (const double*)S, P);
        hipLaunchKernelGGL(cv_scalar_kernel, one, block, 0, st, (const double*)P, nblk, S, 2, eta2, tol2, (int)max_it);
        run.direction(r, p, Y_dev);
        return DMRGX_OK;
    }));
    // closing: X and the true residual of the returned Y, through the same two (x, y) pairs
    DMRGX_HIP(hipMemcpyAsync(p, Y_dev, nn * sizeof(double), hipMemcpyDeviceToDevice, st));
    DMRGX_CHK(dmrgx_kron_apply(plan, p, t, st));
    hipLaunchKernelGGL(cv_x_kernel, grid, block, 0, st, (const double*)t, (const double*)Y_dev, s, X_dev, n, sigma, eta, (const double*)S);
    DMRGX_CHK(dmrgx_kron_apply(plan, s, t, st));
    hipLaunchKernelGGL(cv_true_residual_kernel, grid, block, 0, st, v0_dev, (const double*)t, (const double*)s, (const double*)Y_dev, n, sigma, eta, (const double*)S, P);
    hipLaunchKernelGGL(cv_scalar_kernel, one, block, 0, st, (const double*)P, nblk, S, 3, eta2, tol2, (int)max_it);
    DMRGX_HIP(hipGetLastError());
    if (nu > 0) {
        DMRGX_CHK(dmrgx_vec_gram(nu, 1, n, U_dev, ldu, Y_dev, n, S + CG_NS, 1, 0, nullptr, st));
        if (X_dev) DMRGX_CHK(dmrgx_vec_gram(nu, 1, n, U_dev, ldu, X_dev, n, S + CG_NS + nu, 1, 0, nullptr, st));
    }
    DMRGX_CHK(run.finish(2, 2, stats));
    *norm2 = run.host[CG_NORM2];
    for (int32_t i = 0; i < nu; ++i) {
        im[i] = run.host[CG_NS + i];
        if (X_dev) re[i] = run.host[CG_NS + nu + i];
    }
    return DMRGX_OK;
}
