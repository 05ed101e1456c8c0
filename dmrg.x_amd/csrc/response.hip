// Static linear response of the planned superblock Hamiltonian: X with <p, X> = 0 and Q (H - sigma) Q X = Q v0, Q = 1 - p p^T / <p, p>, by
// conjugate gradients on the complement of p.  With p = psi and sigma = E0 the operator is positive definite there, and for any u
//   <u, X> = sum_{n>0} <u|n><n|v0> / (E_n - E0):  half the static susceptibility d<u>/dh_v.  No eta, no squared operator: one MatMult per
// iteration, the error bounded by residual / gap.  An engine extension in the idiom of corrvec.hip: the iteration lives on the device.
// CG on A x = b, A = Q (H - sigma) Q, b = Q v0 = v0 - coef p, x_0 = 0, r_0 = d_0 = b.  On four pool vectors r, d, t and q (a 16-byte
// aligned copy of the caller's p) and the caller's X, per iteration:
//   MatMult        : t = H d
//   dots           : s = t - sigma d, written over t ; partial sums of d . s and q . s                 (reads t, d, q ; writes t)
//   scalars 1      : d.A d = d . s, not positive and finite -> dead ; alpha = rr / d.A d ; gamma = q.s / q.q
//   residual       : r -= delta q + alpha (s - gamma q) ; partial sums of r . r and q . r            (reads t, q, r ; writes r)
//   scalars 2      : a non-finite sum -> dead, the iteration does not count; else it counts: beta = rr_new / rr, delta = q.r / q.q,
//                    converged when rr_new <= tol^2 b.b, stopped when the count reaches max_it
//   direction      : only for an iteration that counted: x += alpha d ; d = r + beta d unless converged   (reads r, d, x ; writes x, d)
// gamma q takes out what H - sigma leaves along p (p is an eigenvector to its own residual only); delta q takes out what the rounding
// of the previous residual update left along p: r stays orthogonal to p to one rounding, and no drift along p re-enters d.
// Per iteration that is 9 vector reads and 4 writes besides the MatMult: x once; t, d, r and q twice each -- alpha needs all of d . s before
// r may move, and beta all of r . r before d may, so each of the three passes has to see its operands again; s goes over t so that the
// residual pass reads one vector where it would read t and d.
// x takes alpha d in the direction kernel, after scalars 2 has seen rr_new: an iteration whose residual sum is not finite never reaches X.
// Once the stop flag is set -- converged, dead or max_it reached -- the vector kernels return at once and the scalar stages change
// nothing: the MatMults that remain in the enqueued block run on the frozen d.
// After the loop: <q, X> / q.q q leaves X, d = X, t = H d, s = t - sigma d, true residual |b - (s - gamma q)| / |b|; one dmrgx_vec_gram
// for the overlaps.  The MatMult sees the pair (d, t) only.  Iterations are enqueued in blocks of check_every; one small copy per block
// brings the scalars back.  Fixed grids, partials added in block order by one workgroup, no atomics: the same bits whatever check_every is.
#include "krylov.h"
#include <cmath>
#include <limits>

namespace dmrgx {
namespace {

// the device scalars; the overlaps <u_i, X> follow from RS_NS on
enum : int { RS_PP = 0, RS_COEF = 1, RS_VV = 2, RS_NORM2 = 3, RS_BB = 4, RS_RR = 5, RS_ALPHA = 6, RS_GAMMA = 7, RS_BETA = 8, RS_DELTA = 9, RS_ITER = 10, RS_CONV = 11,
             RS_DEAD = 12, RS_STOP = 13, RS_APPLY = 14, RS_NONE = 15, RS_TRUE2 = 16, RS_NS = 18 };

// partial[b], [nblk + b], [2 nblk + b] = p . p, p . v0, v0 . v0 over block b's range.  (p, v0 are the caller's: 8-byte loads)
__global__ void __launch_bounds__(RANGE_THREADS) rs_start_dots_kernel(const double* __restrict__ p, const double* __restrict__ v0, int64_t n, double* __restrict__ partial)
{
    double pp = 0.0, pv = 0.0, vv = 0.0;
    for (int64_t e = range_first(); e < range_end(n); e += RANGE_THREADS) {
        const double a = p[e], b = v0[e];
        pp += a * a;
        pv += a * b;
        vv += b * b;
    }
    pp = block_sum<RANGE_THREADS>(pp);
    pv = block_sum<RANGE_THREADS>(pv);
    vv = block_sum<RANGE_THREADS>(vv);
    if (threadIdx.x == 0) { partial[blockIdx.x] = pp; partial[gridDim.x + blockIdx.x] = pv; partial[2 * gridDim.x + blockIdx.x] = vv; }
}

// q = p, r = d = b = v0 - coef p, x = 0; partial[b] = b . b over block b.  A refused p: exact zeros everywhere, whatever p and v0 hold
__global__ void __launch_bounds__(RANGE_THREADS) rs_start_kernel(const double* __restrict__ p, const double* __restrict__ v0, double* __restrict__ q, double* __restrict__ r,
                                                                double* __restrict__ d, double* __restrict__ x, int64_t n, const double* __restrict__ S, double* __restrict__ partial)
{
    const bool dead = S[RS_DEAD] != 0.0;
    const double coef = S[RS_COEF];
    double acc = 0.0;
    for (int64_t e = range_first(); e < range_end(n); e += RANGE_THREADS) {
        const double pe = dead ? 0.0 : p[e], b = dead ? 0.0 : v0[e] - coef * pe;
        q[e] = pe;
        r[e] = b;
        d[e] = b;
        x[e] = 0.0;
        acc += b * b;
    }
    acc = block_sum<RANGE_THREADS>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// s = t - sigma d over t; partial[b] = d . s, partial[gridDim.x + b] = q . s over block b.  (t, d, q: pool blocks, 16-byte pairs)
__global__ void __launch_bounds__(RANGE_THREADS) rs_dots_kernel(double* __restrict__ t, const double* __restrict__ d, const double* __restrict__ q, int64_t n, double sigma,
                                                               const double* __restrict__ S, double* __restrict__ partial)
{
    if (S[RS_STOP] != 0.0) return;
    double2 tr[RANGE_PAIRS], dr[RANGE_PAIRS], qr[RANGE_PAIRS];
#pragma unroll
    for (int i = 0; i < RANGE_PAIRS; ++i) {
        const int64_t e = range_pair(i);
        tr[i] = load2<true>(t, e, n);
        dr[i] = load2<true>(d, e, n);
        qr[i] = load2<true>(q, e, n);
    }
    double ds = 0.0, qs = 0.0;
#pragma unroll
    for (int i = 0; i < RANGE_PAIRS; ++i) {
        const int64_t e = range_pair(i);
        double2 x;
        x.x = tr[i].x - sigma * dr[i].x;
        x.y = tr[i].y - sigma * dr[i].y;
        store2<true>(t, e, n, x);
        ds += dr[i].x * x.x; ds += dr[i].y * x.y;                // (beyond n the registers hold zeros)
        qs += qr[i].x * x.x; qs += qr[i].y * x.y;
    }
    ds = block_sum<RANGE_THREADS>(ds);
    qs = block_sum<RANGE_THREADS>(qs);
    if (threadIdx.x == 0) { partial[blockIdx.x] = ds; partial[gridDim.x + blockIdx.x] = qs; }
}

// r -= delta q + alpha (s - gamma q); partial[b] = r . r, partial[gridDim.x + b] = q . r over block b
__global__ void __launch_bounds__(RANGE_THREADS) rs_residual_kernel(const double* __restrict__ s, const double* __restrict__ q, double* __restrict__ r, int64_t n,
                                                                   const double* __restrict__ S, double* __restrict__ partial)
{
    if (S[RS_STOP] != 0.0) return;
    const double alpha = S[RS_ALPHA], gamma = S[RS_GAMMA], delta = S[RS_DELTA];
    double2 sr[RANGE_PAIRS], qr[RANGE_PAIRS], rr[RANGE_PAIRS];
#pragma unroll
    for (int i = 0; i < RANGE_PAIRS; ++i) {
        const int64_t e = range_pair(i);
        sr[i] = load2<true>(s, e, n);
        qr[i] = load2<true>(q, e, n);
        rr[i] = load2<true>(r, e, n);
    }
    double acc = 0.0, qa = 0.0;
#pragma unroll
    for (int i = 0; i < RANGE_PAIRS; ++i) {
        const int64_t e = range_pair(i);
        double2 x;
        x.x = (rr[i].x - delta * qr[i].x) - alpha * (sr[i].x - gamma * qr[i].x);
        x.y = (rr[i].y - delta * qr[i].y) - alpha * (sr[i].y - gamma * qr[i].y);
        store2<true>(r, e, n, x);
        acc += x.x * x.x; acc += x.y * x.y;
        qa += qr[i].x * x.x; qa += qr[i].y * x.y;
    }
    acc = block_sum<RANGE_THREADS>(acc);
    qa = block_sum<RANGE_THREADS>(qa);
    if (threadIdx.x == 0) { partial[blockIdx.x] = acc; partial[gridDim.x + blockIdx.x] = qa; }
}

// the iteration counted: x += alpha d, and d = r + beta d unless that iteration converged.  XVEC: the caller's x is 16-byte aligned
template <bool XVEC> __global__ void __launch_bounds__(RANGE_THREADS) rs_direction_kernel(const double* __restrict__ r, double* __restrict__ d, double* __restrict__ x, int64_t n,
                                                                                         const double* __restrict__ S)
{
    if (S[RS_APPLY] == 0.0) return;
    const double alpha = S[RS_ALPHA], beta = S[RS_BETA];
    const bool turn = S[RS_CONV] == 0.0;
    double2 rr[RANGE_PAIRS], dr[RANGE_PAIRS], xr[RANGE_PAIRS];
#pragma unroll
    for (int i = 0; i < RANGE_PAIRS; ++i) {
        const int64_t e = range_pair(i);
        if (turn) rr[i] = load2<true>(r, e, n);
        dr[i] = load2<true>(d, e, n);
        xr[i] = load2<XVEC>(x, e, n);
    }
#pragma unroll
    for (int i = 0; i < RANGE_PAIRS; ++i) {
        const int64_t e = range_pair(i);
        double2 v;
        v.x = xr[i].x + alpha * dr[i].x;
        v.y = xr[i].y + alpha * dr[i].y;
        store2<XVEC>(x, e, n, v);
        if (turn) {
            v.x = rr[i].x + beta * dr[i].x;
            v.y = rr[i].y + beta * dr[i].y;
            store2<true>(d, e, n, v);
        }
    }
}

// closing 1: partial[b] = q . x over block b.  (x: the caller's, 8-byte loads)
__global__ void __launch_bounds__(RANGE_THREADS) rs_qx_kernel(const double* __restrict__ q, const double* __restrict__ x, int64_t n, double* __restrict__ partial)
{
    double acc = 0.0;
    for (int64_t e = range_first(); e < range_end(n); e += RANGE_THREADS) acc += q[e] * x[e];
    acc = block_sum<RANGE_THREADS>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// closing 2: x -= delta q, d = x; a run without a right-hand side: exact zeros
__global__ void __launch_bounds__(RANGE_THREADS) rs_clean_kernel(const double* __restrict__ q, double* __restrict__ x, double* __restrict__ d, int64_t n, const double* __restrict__ S)
{
    const bool none = S[RS_NONE] != 0.0;
    const double delta = S[RS_DELTA];
    for (int64_t e = range_first(); e < range_end(n); e += RANGE_THREADS) {
        const double v = none ? 0.0 : x[e] - delta * q[e];
        x[e] = v;
        d[e] = v;
    }
}

// closing 3: partial[b] = q . (t - sigma d) over block b (t = H d, d = X)
__global__ void __launch_bounds__(RANGE_THREADS) rs_qs_kernel(const double* __restrict__ t, const double* __restrict__ d, const double* __restrict__ q, int64_t n, double sigma,
                                                             double* __restrict__ partial)
{
    double acc = 0.0;
    for (int64_t e = range_first(); e < range_end(n); e += RANGE_THREADS) acc += q[e] * (t[e] - sigma * d[e]);
    acc = block_sum<RANGE_THREADS>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// closing 4: partial[b] = sum over block b of (b - A x)^2, b = v0 - coef q, A x = t - sigma d - gamma q
__global__ void __launch_bounds__(RANGE_THREADS) rs_true_residual_kernel(const double* __restrict__ v0, const double* __restrict__ t, const double* __restrict__ d, const double* __restrict__ q,
                                                                        int64_t n, double sigma, const double* __restrict__ S, double* __restrict__ partial)
{
    const bool none = S[RS_NONE] != 0.0;
    const double coef = S[RS_COEF], gamma = S[RS_GAMMA];
    double acc = 0.0;
    for (int64_t e = range_first(); e < range_end(n); e += RANGE_THREADS) {
        const double z = none ? 0.0 : (v0[e] - coef * q[e]) - ((t[e] - sigma * d[e]) - gamma * q[e]);
        acc += z * z;
    }
    acc = block_sum<RANGE_THREADS>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// One workgroup: the partials added in block order, then the scalar logic of the stage.
//   stage 0 (p, v0):   p.p, p.v0, v0.v0; p.p not positive and finite, or a coefficient that is not finite -> dead, stopped, no right-hand side
//   stage 1 (b):       |Q v0|^2; at most 1e-24 v0.v0, or not positive and finite: v0 is a multiple of p to rounding -> converged at once
//   stage 2 (alpha):   d.s and q.s; a sum that is not finite, d.A d not positive and finite, or an alpha that is not -> dead, stopped
//   stage 3 (counted): r.r and q.r; not finite -> dead, stopped, the iteration does not count and x never sees it; else rr, beta,
//                      delta, the count, the convergence and max_it decisions.  RS_APPLY tells the direction kernel of THIS iteration
//                      whether it counted
//   stage 4 (q.x):     delta = q.x / q.q for the closing clean-up (0 when it is not finite)
//   stage 5 (q.s):     gamma = q.s / q.q of the closing MatMult (0 when it is not finite: the residual then tells)
//   stage 6 (closing): the squared true residual; not finite (an H that is not) -> dead, reported as infinity
// A stopped run passes stages 2 and 3 unchanged.
__global__ void __launch_bounds__(RANGE_THREADS) rs_scalar_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ S, int stage, double tol2, int max_it)
{
    const double a = sum_partials<RANGE_THREADS>(partial, nblk);
    const double b = (stage == 0 || stage == 2 || stage == 3) ? sum_partials<RANGE_THREADS>(partial + nblk, nblk) : 0.0;
    const double c = stage == 0 ? sum_partials<RANGE_THREADS>(partial + 2 * nblk, nblk) : 0.0;
    if (threadIdx.x != 0) return;
    if (stage == 0) {
        const double coef = b / a;
        const bool ok = a > 0.0 && a < INFINITY && fabs(coef) < INFINITY;
        S[RS_PP] = ok ? a : 0.0;
        S[RS_COEF] = ok ? coef : 0.0;
        S[RS_VV] = c;
        S[RS_DEAD] = ok ? 0.0 : 1.0;
        S[RS_STOP] = ok ? 0.0 : 1.0;
        S[RS_NONE] = ok ? 0.0 : 1.0;
        return;
    }
    if (stage == 1) {
        if (S[RS_DEAD] != 0.0) return;
        const bool finite = a >= 0.0 && a < INFINITY;
        const bool ok = finite && a > 0.0 && a > 1e-24 * S[RS_VV];
        S[RS_NORM2] = finite ? a : 0.0;
        S[RS_BB] = ok ? a : 0.0;
        S[RS_RR] = ok ? a : 0.0;
        if (!ok) { S[RS_CONV] = 1.0; S[RS_STOP] = 1.0; S[RS_NONE] = 1.0; }
        return;
    }
    if (stage == 4 || stage == 5) {
        const double pp = S[RS_PP], v = pp > 0.0 ? a / pp : 0.0;
        S[stage == 4 ? RS_DELTA : RS_GAMMA] = fabs(v) < INFINITY ? v : 0.0;
        return;
    }
    if (stage == 6) {
        const double bb = S[RS_BB];
        if (!(a >= 0.0 && a < INFINITY)) { S[RS_DEAD] = 1.0; S[RS_TRUE2] = INFINITY; }
        else S[RS_TRUE2] = bb > 0.0 ? a / bb : 0.0;
        return;
    }
    const bool stopped = S[RS_STOP] != 0.0;
    if (stage == 2) {
        if (stopped) return;
        const double alpha = S[RS_RR] / a, gamma = b / S[RS_PP];
        if (!(a > 0.0 && a < INFINITY && fabs(b) < INFINITY && alpha >= 0.0 && alpha < INFINITY && fabs(gamma) < INFINITY)) { S[RS_DEAD] = 1.0; S[RS_STOP] = 1.0; }
        else { S[RS_ALPHA] = alpha; S[RS_GAMMA] = gamma; }
        return;
    }
    S[RS_APPLY] = 0.0;
    if (stopped) return;
    const double delta = b / S[RS_PP];
    if (!(a >= 0.0 && a < INFINITY && fabs(delta) < INFINITY)) { S[RS_DEAD] = 1.0; S[RS_STOP] = 1.0; return; }
    const double it = S[RS_ITER] + 1.0;
    S[RS_BETA] = a / S[RS_RR];                                   // (rr > 0: an iteration that left rr = 0 converged and stopped the run)
    S[RS_DELTA] = delta;
    S[RS_RR] = a;
    S[RS_ITER] = it;
    S[RS_APPLY] = 1.0;
    if (a <= tol2 * S[RS_BB]) { S[RS_CONV] = 1.0; S[RS_STOP] = 1.0; }
    else if (it >= (double)max_it) S[RS_STOP] = 1.0;
}

}  // namespace
}  // namespace dmrgx

using namespace dmrgx;

extern "C" dmrgx_status dmrgx_kron_static_response(dmrgx_kron_plan* plan, const double* p_dev, const double* v0_dev, double sigma, double tol, int32_t max_it, int32_t check_every,
                                                   double* X_dev, int32_t nu, const double* U_dev, int64_t ldu, double* coef, double* norm2, double* chi,
                                                   dmrgx_cv_stats* stats, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!plan || !p_dev || !v0_dev || !X_dev || !coef || !norm2 || !stats || (nu > 0 && !chi)) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_static_response: null argument");
    if (!(fabs(sigma) < INFINITY)) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_static_response: sigma %g is not finite", sigma);
    if (!(tol >= 0.0) || tol >= 1.0) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_static_response: tol %g outside [0, 1)", tol);
    if (max_it < 1) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_static_response: max_it %d, at least one iteration is needed", max_it);
    if (check_every < 0) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_static_response: check_every %d is negative", check_every);
    if (nu < 0) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_static_response: nu %d is negative", nu);
    int64_t n = 0;
    DMRGX_CHK(whole_plan_states(plan, "kron_static_response", "iteration", &n));
    if (nu > 0 && (!U_dev || ldu < n)) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_static_response: U is null or ldu %lld is smaller than n_states %lld", (long long)ldu, (long long)n);
    const size_t nn = (size_t)n, u_span = nu > 0 ? (size_t)(nu - 1) * (size_t)ldu + nn : 0;
    if (spans_overlap(X_dev, nn, p_dev, nn) || spans_overlap(X_dev, nn, v0_dev, nn) || spans_overlap(X_dev, nn, U_dev, u_span))
        DMRGX_FAIL(DMRGX_ERR_ARG, "kron_static_response: X overlaps p, v0 or U");
    const double tol_ = tol > 0.0 ? tol : 1e-8, tol2 = tol_ * tol_;
    const int64_t ce = check_every > 0 ? check_every : 8;
    const int nblk = range_blocks(n);
    const size_t nscal = (size_t)RS_NS + (size_t)nu;
    const bool xvec = ((uintptr_t)X_dev & 15) == 0;

    DevBuf dR, dD, dT, dQ, dPartial;
    DevScalars dS;
    DMRGX_CHK(dR.alloc_f64(nn, st));
    DMRGX_CHK(dD.alloc_f64(nn, st));
    DMRGX_CHK(dT.alloc_f64(nn, st));
    DMRGX_CHK(dQ.alloc_f64(nn, st));
    DMRGX_CHK(dPartial.alloc_f64((size_t)3 * nblk, st));
    DMRGX_CHK(dS.alloc_zeroed(nscal, st));
    double* S = dS.dev();
    double* P = dPartial.as<double>();
    double* r = dR.as<double>();
    double* d = dD.as<double>();
    double* t = dT.as<double>();
    double* q = dQ.as<double>();
    const dim3 grid((unsigned)nblk), block(RANGE_THREADS), one(1);

    hipLaunchKernelGGL(rs_start_dots_kernel, grid, block, 0, st, p_dev, v0_dev, n, P);
    hipLaunchKernelGGL(rs_scalar_kernel, one, block, 0, st, (const double*)P, nblk, S, 0, tol2, (int)max_it);
    hipLaunchKernelGGL(rs_start_kernel, grid, block, 0, st, p_dev, v0_dev, q, r, d, X_dev, n, (const double*)S, P);
    hipLaunchKernelGGL(rs_scalar_kernel, one, block, 0, st, (const double*)P, nblk, S, 1, tol2, (int)max_it);
    DMRGX_HIP(hipGetLastError());
    std::vector<double> head(RS_NS), host(nscal);
    int64_t blocks = 0;
    for (;;) {
        for (int64_t k = 0; k < ce; ++k) {
            DMRGX_CHK(dmrgx_kron_apply(plan, d, t, st));
            hipLaunchKernelGGL(rs_dots_kernel, grid, block, 0, st, t, (const double*)d, (const double*)q, n, sigma, (const double*)S, P);
            hipLaunchKernelGGL(rs_scalar_kernel, one, block, 0, st, (const double*)P, nblk, S, 2, tol2, (int)max_it);
            hipLaunchKernelGGL(rs_residual_kernel, grid, block, 0, st, (const double*)t, (const double*)q, r, n, (const double*)S, P);
            hipLaunchKernelGGL(rs_scalar_kernel, one, block, 0, st, (const double*)P, nblk, S, 3, tol2, (int)max_it);
            if (xvec) hipLaunchKernelGGL(rs_direction_kernel<true>, grid, block, 0, st, (const double*)r, d, X_dev, n, (const double*)S);
            else hipLaunchKernelGGL(rs_direction_kernel<false>, grid, block, 0, st, (const double*)r, d, X_dev, n, (const double*)S);
            DMRGX_HIP(hipGetLastError());
        }
        ++blocks;
        DMRGX_CHK(dS.read(head, st));                                // the one place where the host looks at the device
        if (head[RS_STOP] != 0.0) break;
    }
    // closing: what rounding left of p in X goes, then the true residual of the returned X through the same (d, t) pair
    hipLaunchKernelGGL(rs_qx_kernel, grid, block, 0, st, (const double*)q, (const double*)X_dev, n, P);
    hipLaunchKernelGGL(rs_scalar_kernel, one, block, 0, st, (const double*)P, nblk, S, 4, tol2, (int)max_it);
    hipLaunchKernelGGL(rs_clean_kernel, grid, block, 0, st, (const double*)q, X_dev, d, n, (const double*)S);
    DMRGX_HIP(hipGetLastError());
    DMRGX_CHK(dmrgx_kron_apply(plan, d, t, st));
    hipLaunchKernelGGL(rs_qs_kernel, grid, block, 0, st, (const double*)t, (const double*)d, (const double*)q, n, sigma, P);
    hipLaunchKernelGGL(rs_scalar_kernel, one, block, 0, st, (const double*)P, nblk, S, 5, tol2, (int)max_it);
    hipLaunchKernelGGL(rs_true_residual_kernel, grid, block, 0, st, v0_dev, (const double*)t, (const double*)d, (const double*)q, n, sigma, (const double*)S, P);
    hipLaunchKernelGGL(rs_scalar_kernel, one, block, 0, st, (const double*)P, nblk, S, 6, tol2, (int)max_it);
    DMRGX_HIP(hipGetLastError());
    if (nu > 0) DMRGX_CHK(dmrgx_vec_gram(nu, 1, n, U_dev, ldu, X_dev, n, S + RS_NS, 1, 0, nullptr, st));
    DMRGX_CHK(dS.read(host, st));
    const double bb = host[RS_BB];
    *coef = host[RS_COEF];
    *norm2 = host[RS_NORM2];
    stats->iterations = (int32_t)host[RS_ITER];
    stats->converged = host[RS_CONV] != 0.0;
    stats->dead = host[RS_DEAD] != 0.0;
    stats->n_matvec = (int32_t)std::min<int64_t>(blocks * ce + 1, std::numeric_limits<int32_t>::max());
    stats->residual = bb > 0.0 ? std::sqrt(host[RS_RR] / bb) : 0.0;
    stats->true_residual = std::sqrt(host[RS_TRUE2]);
    for (int32_t i = 0; i < nu; ++i) chi[i] = host[RS_NS + i];
    return DMRGX_OK;
}
