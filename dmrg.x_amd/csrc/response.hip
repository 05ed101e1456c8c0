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
// What this run shares with corrvec.hip -- the scalar slots, the direction kernel, the decisions of scalars 1 and 2, the checks, the block
// loop, the stats -- is cg.h.
#include "cg.h"

namespace dmrgx {
namespace {

// this solver's device scalars, after the common ones; the overlaps <u_i, X> follow from RS_NS on
enum : int { RS_NONE = CG_NS, RS_PP, RS_DELTA, RS_COEF, RS_VV, RS_GAMMA, RS_NS };

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
    const bool dead = S[CG_DEAD] != 0.0;
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
    if (S[CG_STOP] != 0.0) return;
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
    if (S[CG_STOP] != 0.0) return;
    const double alpha = S[CG_ALPHA], gamma = S[RS_GAMMA], delta = S[RS_DELTA];
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
//   stage 3 (counted): r.r and q.r; cg_counted, and delta = q.r / q.q of an iteration that counted
//   stage 4 (q.x):     delta = q.x / q.q for the closing clean-up (0 when it is not finite)
//   stage 5 (q.s):     gamma = q.s / q.q of the closing MatMult (0 when it is not finite: the residual then tells)
//   stage 6 (closing): the squared true residual, cg_true_residual
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
        S[CG_DEAD] = ok ? 0.0 : 1.0;
        S[CG_STOP] = ok ? 0.0 : 1.0;
        S[RS_NONE] = ok ? 0.0 : 1.0;
        return;
    }
    if (stage == 1) {
        if (S[CG_DEAD] != 0.0) return;
        const bool finite = a >= 0.0 && a < INFINITY;
        const bool ok = finite && a > 0.0 && a > 1e-24 * S[RS_VV];
        S[CG_NORM2] = finite ? a : 0.0;
        S[CG_BB] = ok ? a : 0.0;
        S[CG_RR] = ok ? a : 0.0;
        if (!ok) { S[CG_CONV] = 1.0; S[CG_STOP] = 1.0; S[RS_NONE] = 1.0; }
        return;
    }
    if (stage == 4 || stage == 5) {
        const double pp = S[RS_PP], v = pp > 0.0 ? a / pp : 0.0;
        S[stage == 4 ? RS_DELTA : RS_GAMMA] = fabs(v) < INFINITY ? v : 0.0;
        return;
    }
    if (stage == 6) { cg_true_residual(S, a); return; }
    if (stage == 2) {
        if (S[CG_STOP] != 0.0) return;
        const double alpha = S[CG_RR] / a, gamma = b / S[RS_PP];
        if (cg_accept_alpha(S, a, alpha, fabs(b) < INFINITY && fabs(gamma) < INFINITY)) S[RS_GAMMA] = gamma;
        return;
    }
    // stage 3: a delta that is not finite kills the run as a sum that is not does -- cg_counted sees an r.r that is not finite
    const double delta = b / S[RS_PP];
    if (cg_counted(S, fabs(delta) < INFINITY ? a : INFINITY, tol2, max_it)) S[RS_DELTA] = delta;
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
    CgRun run("kron_static_response", st);
    DMRGX_CHK(run.check(plan, tol, max_it, check_every, nu, U_dev, ldu));
    const int64_t n = run.n;
    const size_t nn = run.nn;
    if (spans_overlap(X_dev, nn, p_dev, nn) || spans_overlap(X_dev, nn, v0_dev, nn) || spans_overlap(X_dev, nn, U_dev, run.u_span))
        DMRGX_FAIL(DMRGX_ERR_ARG, "kron_static_response: X overlaps p, v0 or U");
    DMRGX_CHK(run.alloc(3, (size_t)RS_NS + (size_t)nu));
    const double tol2 = run.tol2;
    const int nblk = run.nblk;
    double *const S = run.S, *const P = run.P, *const r = run.vec(0), *const d = run.vec(1), *const t = run.vec(2), *const q = run.vec(3);
    const dim3 grid((unsigned)nblk), block(RANGE_THREADS), one(1);

    hipLaunchKernelGGL(rs_start_dots_kernel, grid, block, 0, st, p_dev, v0_dev, n, P);
    hipLaunchKernelGGL(rs_scalar_kernel, one, block, 0, st, (const double*)P, nblk, S, 0, tol2, (int)max_it);
    hipLaunchKernelGGL(rs_start_kernel, grid, block, 0, st, p_dev, v0_dev, q, r, d, X_dev, n, (const double*)S, P);
    hipLaunchKernelGGL(rs_scalar_kernel, one, block, 0, st, (const double*)P, nblk, S, 1, tol2, (int)max_it);
    DMRGX_HIP(hipGetLastError());
    DMRGX_CHK(run.iterate([&]() -> dmrgx_status {
        DMRGX_CHK(dmrgx_kron_apply(plan, d, t, st));
        hipLaunchKernelGGL(rs_dots_kernel, grid, block, 0, st, t, (const double*)d, (const double*)q, n, sigma, (const double*)S, P);
        hipLaunchKernelGGL(rs_scalar_kernel, one, block, 0, st, (const double*)P, nblk, S, 2, tol2, (int)max_it);
        hipLaunchKernelGGL(rs_residual_kernel, grid, block, 0, st, (const double*)t, (const double*)q, r, n, (const double*)S, P);
        hipLaunchKernelGGL(rs_scalar_kernel, one, block, 0, st, (const double*)P, nblk, S, 3, tol2, (int)max_it);
        run.direction(r, d, X_dev);
        return DMRGX_OK;
    }));
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
    DMRGX_CHK(run.finish(1, 1, stats));
    *coef = run.host[RS_COEF];
    *norm2 = run.host[CG_NORM2];
    for (int32_t i = 0; i < nu; ++i) chi[i] = run.host[RS_NS + i];
    return DMRGX_OK;
}
