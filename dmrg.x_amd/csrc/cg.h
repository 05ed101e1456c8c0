// What the device-resident conjugate-gradient calls share (corrvec.hip, response.hip), on top of krylov.h: the scalar slots, the direction
// kernel, the scalar decisions of an iteration and the host side of a run.  Internal, not part of the ABI.  A solver keeps what is its own:
// the start, the two vector passes of an iteration, how alpha's denominator is formed, and the closing.  An iteration of either:
//   MatMult(s) ; pass 1 and its sums ; scalars 1: cg_accept_alpha ; pass 2 moves r, sums r . r ; scalars 2: cg_counted ; cg_direction_kernel
// Once CG_STOP is set -- converged, dead or max_it reached -- the vector kernels return at once and the scalar stages change nothing.
#pragma once
#include "krylov.h"
#include <cmath>
#include <limits>

namespace dmrgx {

// The device scalars every run has; a solver's own follow from CG_NS on, and the overlaps after those.  NORM2: what the call reports as
// norm2; BB: b . b; RR: r . r of the last iteration that counted; ITER: how many did; CONV, DEAD, STOP, APPLY: flags; TRUE2: |b - A x|^2 / b . b
enum : int { CG_NORM2 = 0, CG_BB, CG_RR, CG_ALPHA, CG_BETA, CG_ITER, CG_CONV, CG_DEAD, CG_STOP, CG_APPLY, CG_TRUE2, CG_NS };

// the iteration counted: x += alpha d, and d = r + beta d unless that iteration converged.  VEC: the caller's x is 16-byte aligned
template <bool VEC> __global__ void __launch_bounds__(RANGE_THREADS) cg_direction_kernel(const double* __restrict__ r, double* __restrict__ d, double* __restrict__ x, int64_t n,
                                                                                         const double* __restrict__ S)
{
    if (S[CG_APPLY] == 0.0) return;
    const double alpha = S[CG_ALPHA], beta = S[CG_BETA];
    const bool turn = S[CG_CONV] == 0.0;
    double2 rr[RANGE_PAIRS], dr[RANGE_PAIRS], xr[RANGE_PAIRS];
#pragma unroll
    for (int i = 0; i < RANGE_PAIRS; ++i) {
        const int64_t e = range_pair(i);
        if (turn) rr[i] = load2<true>(r, e, n);
        dr[i] = load2<true>(d, e, n);
        xr[i] = load2<VEC>(x, e, n);
    }
#pragma unroll
    for (int i = 0; i < RANGE_PAIRS; ++i) {
        const int64_t e = range_pair(i);
        double2 v;
        v.x = xr[i].x + alpha * dr[i].x;
        v.y = xr[i].y + alpha * dr[i].y;
        store2<VEC>(x, e, n, v);
        if (turn) {
            v.x = rr[i].x + beta * dr[i].x;
            v.y = rr[i].y + beta * dr[i].y;
            store2<true>(d, e, n, v);
        }
    }
}

// The scalar decisions, for thread 0 of a solver's one-workgroup scalar kernel.
// scalars 1 of a run that has not stopped: `den` = d . A d and `alpha` = rr / den as the solver formed them, `sums_ok` what it asks of its
// own sums.  A denominator that is not positive and finite, or an alpha that is not finite -> dead, stopped.  Returns whether alpha stands.
__device__ __forceinline__ bool cg_accept_alpha(double* __restrict__ S, double den, double alpha, bool sums_ok) {
    if (!(sums_ok && den > 0.0 && den < INFINITY && alpha >= 0.0 && alpha < INFINITY)) { S[CG_DEAD] = 1.0; S[CG_STOP] = 1.0; return false; }
    S[CG_ALPHA] = alpha;
    return true;
}

// scalars 2: `rr_new` = r . r after the residual moved.  A stopped run passes unchanged.  Not finite -> dead, stopped, the iteration does
// not count and x never sees it; else it counts: beta, rr, the count, converged when rr_new <= tol2 b . b, stopped when the count reaches
// max_it.  CG_APPLY tells the direction kernel of THIS iteration whether it counted, and so does the return value.
__device__ __forceinline__ bool cg_counted(double* __restrict__ S, double rr_new, double tol2, int max_it) {
    S[CG_APPLY] = 0.0;
    if (S[CG_STOP] != 0.0) return false;
    if (!(rr_new >= 0.0 && rr_new < INFINITY)) { S[CG_DEAD] = 1.0; S[CG_STOP] = 1.0; return false; }
    const double it = S[CG_ITER] + 1.0;
    S[CG_BETA] = rr_new / S[CG_RR];                              // (rr > 0: an iteration that left rr = 0 converged and stopped the run)
    S[CG_RR] = rr_new;
    S[CG_ITER] = it;
    S[CG_APPLY] = 1.0;
    if (rr_new <= tol2 * S[CG_BB]) { S[CG_CONV] = 1.0; S[CG_STOP] = 1.0; }
    else if (it >= (double)max_it) S[CG_STOP] = 1.0;
    return true;
}

// closing: `res2` = |b - A x|^2 of the returned x; not finite (an H that is not) -> dead, reported as infinity
__device__ __forceinline__ void cg_true_residual(double* __restrict__ S, double res2) {
    const double bb = S[CG_BB];
    if (!(res2 >= 0.0 && res2 < INFINITY)) { S[CG_DEAD] = 1.0; S[CG_TRUE2] = INFINITY; }
    else S[CG_TRUE2] = bb > 0.0 ? res2 / bb : 0.0;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// One run.  An entry point reads: its own checks, check(), its overlap test, alloc(), start, iterate(), closing, overlaps, finish().
struct CgRun {
    const char* const call;                                      // the entry point's name, as its messages spell it
    const hipStream_t st;
    int64_t n = 0, ce = 0, blocks = 0;
    size_t nn = 0, u_span = 0;                                   // n; the doubles from U's first to the end of its last row
    int nblk = 0;
    double tol2 = 0.0;
    DevBuf dVec[4], dPartial;
    DevScalars dS;
    double *S = nullptr, *P = nullptr;
    std::vector<double> host;                                    // every scalar, after finish()

    CgRun(const char* name, hipStream_t stream) : call(name), st(stream) {}

    // the arguments both calls check in the same words, and the defaults: tol 1e-8, check_every 8
    dmrgx_status check(dmrgx_kron_plan* plan, double tol, int32_t max_it, int32_t check_every, int32_t nu, const double* U_dev, int64_t ldu) {
        if (!(tol >= 0.0) || tol >= 1.0) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: tol %g outside [0, 1)", call, tol);
        if (max_it < 1) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: max_it %d, at least one iteration is needed", call, max_it);
        if (check_every < 0) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: check_every %d is negative", call, check_every);
        if (nu < 0) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: nu %d is negative", call, nu);
        DMRGX_CHK(whole_plan_states(plan, call, "iteration", &n));
        if (nu > 0 && (!U_dev || ldu < n)) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: U is null or ldu %lld is smaller than n_states %lld", call, (long long)ldu, (long long)n);
        nn = (size_t)n;
        u_span = nu > 0 ? (size_t)(nu - 1) * (size_t)ldu + nn : 0;
        const double tol_ = tol > 0.0 ? tol : 1e-8;
        tol2 = tol_ * tol_;
        ce = check_every > 0 ? check_every : 8;
        nblk = range_blocks(n);
        return DMRGX_OK;
    }
    // the four pool vectors vec(0..3), `sums` partial sums per workgroup, `nscal` scalars (zeroed)
    dmrgx_status alloc(int sums, size_t nscal) {
        for (DevBuf& v : dVec) DMRGX_CHK(v.alloc_f64(nn, st));
        DMRGX_CHK(dPartial.alloc_f64((size_t)sums * nblk, st));
        DMRGX_CHK(dS.alloc_zeroed(nscal, st));
        host.resize(nscal);
        S = dS.dev();
        P = dPartial.as<double>();
        return DMRGX_OK;
    }
    double* vec(int i) const { return dVec[i].as<double>(); }
    // an iteration's last launch; 16-byte pair accesses of the caller's x only where it allows them
    void direction(const double* r, double* d, double* x) const {
        const dim3 grid((unsigned)nblk), block(RANGE_THREADS);
        if (((uintptr_t)x & 15) == 0) hipLaunchKernelGGL(cg_direction_kernel<true>, grid, block, 0, st, r, d, x, n, (const double*)S);
        else hipLaunchKernelGGL(cg_direction_kernel<false>, grid, block, 0, st, r, d, x, n, (const double*)S);
    }
    // blocks of `ce` iterations, each enqueued by enqueue() -> dmrgx_status; one small copy per block brings the scalars back
    template <class F> dmrgx_status iterate(F&& enqueue) {
        std::vector<double> head(CG_NS);
        for (;;) {
            for (int64_t k = 0; k < ce; ++k) { DMRGX_CHK(enqueue()); DMRGX_HIP(hipGetLastError()); }
            ++blocks;
            DMRGX_CHK(dS.read(head, st));                            // the one place where the host looks at the device
            if (head[CG_STOP] != 0.0) return DMRGX_OK;
        }
    }
    // the final read, into `host`, and the stats; MatMults: mv_it per enqueued iteration, mv_closing after the loop
    dmrgx_status finish(int mv_it, int mv_closing, dmrgx_cv_stats* stats) {
        DMRGX_CHK(dS.read(host, st));
        const double bb = host[CG_BB];
        stats->iterations = (int32_t)host[CG_ITER];
        stats->converged = host[CG_CONV] != 0.0;
        stats->dead = host[CG_DEAD] != 0.0;
        stats->n_matvec = (int32_t)std::min<int64_t>(mv_it * blocks * ce + mv_closing, std::numeric_limits<int32_t>::max());
        stats->residual = bb > 0.0 ? std::sqrt(host[CG_RR] / bb) : 0.0;
        stats->true_residual = std::sqrt(host[CG_TRUE2]);
        return DMRGX_OK;
    }
};

}  // namespace dmrgx
