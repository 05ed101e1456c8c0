// dmrgx_eigs_lowest_orth: the lowest eigenpair of the planned superblock Hamiltonian on the complement of given vectors -- the lowest
// eigenpair of P H P, P = 1 - Qt Qt^T, with Qt a private orthonormalised copy of the caller's rows.  Excited states of one sector are
// found one after another, each with the states already found as Q: that resolves exact degeneracies, which one Krylov sequence cannot.
//
// Thick-restart Lanczos as in eigs.hip (the same restart rule -- keep ncv / 2 Ritz vectors and the residual direction --, a look at the
// Ritz pair after every step, |r| <= tol |theta|), on ONE basis allocation [Qt ; v_0 .. v_m] of rows with an even stride, so that every
// access is a 16-byte pair access.  Every w = H v_j is orthogonalised twice against ALL rows above it; the projected matrix T = V^T H V is
// what the two passes removed along the rows of V.  Per step, in the range layout of krylov.h (a workgroup keeps its 2048 elements of w
// in registers and lets the rows go past):
//   MatMult : w = H x                                                    (x = v_j, w: two fixed pool vectors -- the plan sees one pair)
//   pass 1  : partial sums of <row, w> for every row, and of <w, w>      (reads the rows once)
//   sums    : the partials of every row added in block order             (one workgroup per row)
//   pass 2  : w -= sum c1[k] row_k, stored; partial sums of <row, w>, <w, w>   (walks the rows twice: the subtraction has to be complete
//             before the first of the second dots can be taken; the second walk finds a workgroup's 16 KB per row in the caches)
//   sums
//   pass 3  : v_{j+1} = (w - sum c2[k] row_k) / beta into its row and into x, beta^2 = <w, w> - |c2|^2 taken by every workgroup from the
//             reduced sums (c2 is the refinement of an orthogonal vector: no cancellation); workgroup 0 records the step's column of T
// No atomics, every sum has one order: two runs give the same bits.  The host reads one row of coefficients per step (that read is the
// step's only synchronisation), solves the projected problem by Jacobi rotations and uploads the restart rotation, which is applied
// in place: a workgroup owns its range of every row.
#include "krylov.h"
#include "ritz.h"
#include <chrono>
#include <cmath>
#include <cstring>

namespace dmrgx {
namespace {

constexpr int EO_KC = 64, EO_MAX_NCV = 64, EO_MAX_KEEP = EO_MAX_NCV / 2, EO_THREADS = 256;

// dst[row][e] = src[row][e], e < n: the caller's 8-byte aligned rows into rows the kernels may read in pairs.  blockIdx.y: the row
__global__ void __launch_bounds__(RANGE_THREADS) eo_copy_rows_kernel(const double* __restrict__ src, int64_t lds, double* __restrict__ dst, int64_t ldd, int64_t n)
{
    const double* __restrict__ s = src + (int64_t)blockIdx.y * lds;
    double* __restrict__ d = dst + (int64_t)blockIdx.y * ldd;
    for (int64_t e = range_first(); e < range_end(n); e += RANGE_THREADS) d[e] = s[e];
}

// the random start vector of eigs.hip, in the range layout: element e takes value e of the seed's stream (splitmix_uniform, krylov.h)
__global__ void __launch_bounds__(RANGE_THREADS) eo_random_kernel(double* __restrict__ v, int64_t n, uint64_t seed)
{
    for (int64_t e = range_first(); e < range_end(n); e += RANGE_THREADS) v[e] = splitmix_uniform(seed, e);
}

// Passes 1 and 2.  SUB: w -= sum_{k < nk} c[k] B[k] first, and w is stored.  Then partial[k * gridDim.x + b] = <B[k], w> over block b's
// range for k < nk, and partial[nk * gridDim.x + b] = <w, w>.  w may be a row of the basis below the nk rows read (neither is written
// through the other).  Wave sums go to LDS per row and are added in wave order once per EO_KC rows: no barrier per row.
template <bool SUB> __global__ void __launch_bounds__(RANGE_THREADS) eo_dots_kernel(double* __restrict__ w, const double* __restrict__ B, int64_t ld, int nk, int64_t n,
                                                                                    const double* __restrict__ c, double* __restrict__ partial)
{
    __shared__ double red[EO_KC][RANGE_THREADS / 64];
    double2 wr[RANGE_PAIRS];
#pragma unroll
    for (int t = 0; t < RANGE_PAIRS; ++t) wr[t] = load2<true>(w, range_pair(t), n);
    if (SUB) {
        for (int k = 0; k < nk; ++k) {
            const double* __restrict__ row = B + (int64_t)k * ld;
            const double ck = c[k];
            double2 v[RANGE_PAIRS];
#pragma unroll
            for (int t = 0; t < RANGE_PAIRS; ++t) v[t] = load2<true>(row, range_pair(t), n);
#pragma unroll
            for (int t = 0; t < RANGE_PAIRS; ++t) { wr[t].x -= ck * v[t].x; wr[t].y -= ck * v[t].y; }
        }
#pragma unroll
        for (int t = 0; t < RANGE_PAIRS; ++t) store2<true>(w, range_pair(t), n, wr[t]);
    }
    for (int k0 = 0; k0 < nk; k0 += EO_KC) {
        const int kc = min(EO_KC, nk - k0);
        for (int kk = 0; kk < kc; ++kk) {
            const double* __restrict__ row = B + (int64_t)(k0 + kk) * ld;
            double2 v[RANGE_PAIRS];
#pragma unroll
            for (int t = 0; t < RANGE_PAIRS; ++t) v[t] = load2<true>(row, range_pair(t), n);
            double acc = 0.0;
#pragma unroll
            for (int t = 0; t < RANGE_PAIRS; ++t) { acc += v[t].x * wr[t].x; acc += v[t].y * wr[t].y; }
            acc = wave_sum(acc);
            if ((threadIdx.x & 63) == 0) red[kk][threadIdx.x >> 6] = acc;
        }
        __syncthreads();
        if ((int)threadIdx.x < kc) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < RANGE_THREADS / 64; ++i) s += red[threadIdx.x][i];
            partial[(int64_t)(k0 + threadIdx.x) * gridDim.x + blockIdx.x] = s;
        }
        __syncthreads();
    }
    double ww = 0.0;
#pragma unroll
    for (int t = 0; t < RANGE_PAIRS; ++t) { ww += wr[t].x * wr[t].x; ww += wr[t].y * wr[t].y; }      // (beyond n the registers hold zeros)
    ww = block_sum<RANGE_THREADS>(ww);
    if (threadIdx.x == 0) partial[(int64_t)nk * gridDim.x + blockIdx.x] = ww;
}

// block i: out[i] = the partials of sum i added in block order
__global__ void __launch_bounds__(EO_THREADS) eo_sums_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ out)
{
    const double s = sum_partials<EO_THREADS>(partial + (int64_t)blockIdx.x * nblk, nblk);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// Pass 3.  dst = (w - sum_{k < nk} c2[k] B[k]) / beta, and dst2 too unless it is null, with beta^2 = c2[nk] - |c2|^2 (c2[nk] = <w, w>) formed
// by every thread in the same order: one value for the whole grid; a beta^2 that is not above 1e-290 gives exact zeros.  Workgroup 0
// records what the caller asks for: coef[t] = c1[skip + t] + c2[skip + t], t < nk - skip (what both passes removed along the Lanczos
// rows: the step's column of the projected matrix), *beta2 = beta^2, norms[0] = c1[nk] (<w, w> before any projection), norms[1] = beta^2.
// dst may be w (each thread reads its elements before it writes them) or a row below the nk rows read.
__global__ void __launch_bounds__(RANGE_THREADS) eo_normalise_kernel(const double* w, const double* __restrict__ B, int64_t ld, int nk, int64_t n,
                                                                     const double* __restrict__ c1, const double* __restrict__ c2, int skip,
                                                                     double* __restrict__ coef, double* __restrict__ beta2, double* __restrict__ norms,
                                                                     double* dst, double* __restrict__ dst2)
{
    double s2 = c2[nk];
    for (int k = 0; k < nk; ++k) s2 -= c2[k] * c2[k];
    s2 = s2 > 0.0 ? s2 : 0.0;
    const double inv = s2 > 1e-290 ? 1.0 / sqrt(s2) : 0.0;
    if (blockIdx.x == 0) {
        if (coef) for (int t = threadIdx.x; t < nk - skip; t += RANGE_THREADS) coef[t] = c1[skip + t] + c2[skip + t];
        if (threadIdx.x == 0 && beta2) *beta2 = s2;
        if (threadIdx.x == 0 && norms) { norms[0] = c1[nk]; norms[1] = s2; }
    }
    double2 wr[RANGE_PAIRS];
#pragma unroll
    for (int t = 0; t < RANGE_PAIRS; ++t) wr[t] = load2<true>(w, range_pair(t), n);
    for (int k = 0; k < nk; ++k) {
        const double* __restrict__ row = B + (int64_t)k * ld;
        const double ck = c2[k];
        double2 v[RANGE_PAIRS];
#pragma unroll
        for (int t = 0; t < RANGE_PAIRS; ++t) v[t] = load2<true>(row, range_pair(t), n);
#pragma unroll
        for (int t = 0; t < RANGE_PAIRS; ++t) { wr[t].x -= ck * v[t].x; wr[t].y -= ck * v[t].y; }
    }
#pragma unroll
    for (int t = 0; t < RANGE_PAIRS; ++t) {
        const double2 q = inv != 0.0 ? double2{wr[t].x * inv, wr[t].y * inv} : double2{0.0, 0.0};
        store2<true>(dst, range_pair(t), n, q);
        if (dst2) store2<true>(dst2, range_pair(t), n, q);
    }
}

// The thick restart, in place: V[j] <- sum_{i < m} V[i] R[i * kk + j] for j < kk (the kept Ritz vectors), V[kk] <- V[m] (the residual
// direction), which also goes to x as the next MatMult's input.  A thread reads all m + 1 values of its pair before it writes any, and no
// other thread touches that pair.  m <= EO_MAX_NCV, kk <= EO_MAX_KEEP.
__global__ void __launch_bounds__(RANGE_THREADS) eo_restart_kernel(double* V, int64_t ld, int m, int kk, int64_t n, const double* __restrict__ R, double* __restrict__ x)
{
    __shared__ double rs[EO_MAX_NCV * EO_MAX_KEEP];
    for (int t = threadIdx.x; t < m * kk; t += RANGE_THREADS) rs[t] = R[t];
    __syncthreads();
    for (int t = 0; t < RANGE_PAIRS; ++t) {
        const int64_t e = range_pair(t);
        if (e >= n) continue;
        double2 acc[EO_MAX_KEEP];
#pragma unroll
        for (int j = 0; j < EO_MAX_KEEP; ++j) acc[j] = double2{0.0, 0.0};
        for (int i = 0; i < m; ++i) {
            const double2 v = load2<true>(V + (int64_t)i * ld, e, n);
#pragma unroll
            for (int j = 0; j < EO_MAX_KEEP; ++j) if (j < kk) { acc[j].x += v.x * rs[i * kk + j]; acc[j].y += v.y * rs[i * kk + j]; }
        }
        const double2 last = load2<true>(V + (int64_t)m * ld, e, n);
#pragma unroll
        for (int j = 0; j < EO_MAX_KEEP; ++j) if (j < kk) store2<true>(V + (int64_t)j * ld, e, n, acc[j]);
        store2<true>(V + (int64_t)kk * ld, e, n, last);
        store2<true>(x, e, n, last);
    }
}

// out = sum_{i < mm} y[i] V[i]: the Ritz vector
__global__ void __launch_bounds__(RANGE_THREADS) eo_combine_kernel(const double* __restrict__ V, int64_t ld, int mm, int64_t n, const double* __restrict__ y, double* __restrict__ out)
{
    double2 acc[RANGE_PAIRS];
#pragma unroll
    for (int t = 0; t < RANGE_PAIRS; ++t) acc[t] = double2{0.0, 0.0};
    for (int i = 0; i < mm; ++i) {
        const double* __restrict__ row = V + (int64_t)i * ld;
        const double yi = y[i];
        double2 v[RANGE_PAIRS];
#pragma unroll
        for (int t = 0; t < RANGE_PAIRS; ++t) v[t] = load2<true>(row, range_pair(t), n);
#pragma unroll
        for (int t = 0; t < RANGE_PAIRS; ++t) { acc[t].x += yi * v[t].x; acc[t].y += yi * v[t].y; }
    }
#pragma unroll
    for (int t = 0; t < RANGE_PAIRS; ++t) store2<true>(out, range_pair(t), n, acc[t]);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// One deflated solve: the device buffers and the launches of the passes
struct OrthRun {
    hipStream_t st;
    int64_t n = 0, ld = 0;
    int nblk = 0;
    DevBuf dB, dX, dW, dPartial, dC, dR;
    DevScalars dS;
    double *B = nullptr, *x = nullptr, *w = nullptr, *P = nullptr, *c1 = nullptr, *c2 = nullptr;

    dmrgx_status dots(bool sub, double* vec, int nk, double* out)
    {
        if (sub) hipLaunchKernelGGL(eo_dots_kernel<true>, dim3(nblk), dim3(RANGE_THREADS), 0, st, vec, (const double*)B, ld, nk, n, (const double*)c1, P);
        else hipLaunchKernelGGL(eo_dots_kernel<false>, dim3(nblk), dim3(RANGE_THREADS), 0, st, vec, (const double*)B, ld, nk, n, (const double*)nullptr, P);
        hipLaunchKernelGGL(eo_sums_kernel, dim3(nk + 1), dim3(EO_THREADS), 0, st, (const double*)P, nblk, out);
        DMRGX_HIP(hipGetLastError());
        return DMRGX_OK;
    }
    // CGS2 of `vec` against rows [0, nk) and the normalisation into dst (and dst2)
    dmrgx_status orthonormalise(double* vec, int nk, int skip, double* coef, double* beta2, double* norms, double* dst, double* dst2)
    {
        DMRGX_CHK(dots(false, vec, nk, c1));
        DMRGX_CHK(dots(true, vec, nk, c2));
        hipLaunchKernelGGL(eo_normalise_kernel, dim3(nblk), dim3(RANGE_THREADS), 0, st, (const double*)vec, (const double*)B, ld, nk, n, (const double*)c1, (const double*)c2, skip,
                           coef, beta2, norms, dst, dst2);
        DMRGX_HIP(hipGetLastError());
        return DMRGX_OK;
    }
};

}  // namespace
}  // namespace dmrgx

using namespace dmrgx;

extern "C" dmrgx_status dmrgx_eigs_lowest_orth(dmrgx_kron_plan* plan, const dmrgx_eigs_opts* opts, int32_t nq, const double* Q_dev, int64_t ldq,
                                               double* e, double* psi_dev, dmrgx_eigs_stats* stats, void* stream)
{
    if (!plan || !opts || !e || !psi_dev) DMRGX_FAIL(DMRGX_ERR_ARG, "eigs_lowest_orth: null argument");
    if (nq < 0) DMRGX_FAIL(DMRGX_ERR_ARG, "eigs_lowest_orth: nq %d is negative", nq);
    if (nq == 0) return dmrgx_eigs_lowest(plan, opts, e, psi_dev, stats, stream);
    if (opts->allgather || opts->allreduce_sum || opts->comm) DMRGX_FAIL(DMRGX_ERR_ARG, "eigs_lowest_orth: collectives (allgather / allreduce_sum / comm) are set: the deflated solve runs on one rank");
    if (opts->max_matvec > 0) DMRGX_FAIL(DMRGX_ERR_ARG, "eigs_lowest_orth: max_matvec %d: the deflated solve has no fixed-length mode", opts->max_matvec);
    int64_t n = 0;
    DMRGX_CHK(whole_plan_states(plan, "eigs_lowest_orth", "deflated solve", &n));
    if (!Q_dev || ldq < n) DMRGX_FAIL(DMRGX_ERR_ARG, "eigs_lowest_orth: Q is null or ldq %lld is smaller than n_states %lld", (long long)ldq, (long long)n);
    if (nq >= n) DMRGX_FAIL(DMRGX_ERR_ARG, "eigs_lowest_orth: nq %d leaves no complement in %lld states", nq, (long long)n);
    const auto t_begin = std::chrono::steady_clock::now();
    const int64_t space = n - nq;                                  // the dimension of the complement: the Krylov space never grows past it
    int m = opts->ncv > 0 ? opts->ncv : 16;
    m = (int)std::min<int64_t>(std::min(m, EO_MAX_NCV), space);
    m = (int)std::max<int64_t>(m, std::min<int64_t>(2, space));    // (a one-vector space cannot restart, as in eigs_lowest)
    const int max_it = opts->max_it > 0 ? opts->max_it : std::max<int>(100, (int)(2 * space / m));
    const double tol = opts->tol > 0 ? opts->tol : 1e-8;
    const int row = m + 2, max_rows = nq + m + 1;

    OrthRun R;
    R.st = (hipStream_t)stream;
    hipStream_t st = R.st;
    R.n = n; R.ld = (n + 1) & ~(int64_t)1; R.nblk = range_blocks(n);
    const int64_t ld = R.ld;
    DMRGX_CHK(R.dB.alloc_f64((size_t)max_rows * (size_t)ld, st));
    DMRGX_CHK(R.dX.alloc_f64((size_t)ld, st));
    DMRGX_CHK(R.dW.alloc_f64((size_t)ld, st));
    DMRGX_CHK(R.dPartial.alloc_f64((size_t)(max_rows + 1) * (size_t)R.nblk, st));
    DMRGX_CHK(R.dC.alloc_f64((size_t)2 * (size_t)(max_rows + 1), st));
    DMRGX_CHK(R.dR.alloc_f64((size_t)EO_MAX_NCV * EO_MAX_KEEP, st));
    // the scalars: per step a row of m + 2 (the column of T, slot m + 1: beta^2), then (|row|^2 before, after) of every row of Q, then of the start vector
    const size_t o_qn = (size_t)(m + 1) * row, o_start = o_qn + 2 * (size_t)nq, nscal = o_start + 2;
    DMRGX_CHK(R.dS.alloc_zeroed(nscal, st));
    R.B = R.dB.as<double>(); R.x = R.dX.as<double>(); R.w = R.dW.as<double>(); R.P = R.dPartial.as<double>();
    R.c1 = R.dC.as<double>(); R.c2 = R.c1 + (max_rows + 1);
    double* const S = R.dS.dev();
    double* const V = R.B + (int64_t)nq * ld;                      // the Lanczos rows
    auto Hrow = [&](int j) { return S + (size_t)j * row; };
    std::vector<double> host(nscal, 0.0);

    // ---- Qt: the caller's rows, orthonormalised row by row in row order (CGS2) ----------------------------------------------------------
    hipLaunchKernelGGL(eo_copy_rows_kernel, dim3(R.nblk, nq), dim3(RANGE_THREADS), 0, st, Q_dev, ldq, R.B, ld, n);
    DMRGX_HIP(hipGetLastError());
    for (int r = 0; r < nq; ++r) {
        double* qr = R.B + (int64_t)r * ld;
        DMRGX_CHK(R.orthonormalise(qr, r, r, nullptr, nullptr, S + o_qn + 2 * (size_t)r, qr, nullptr));
    }
    DMRGX_CHK(R.dS.read(host, st));
    for (int r = 0; r < nq; ++r) {
        const double before = host[o_qn + 2 * (size_t)r], after = host[o_qn + 2 * (size_t)r + 1];
        if (!(before > 0.0 && before < INFINITY)) DMRGX_FAIL(DMRGX_ERR_ARG, "eigs_lowest_orth: row %d of Q is zero or not finite", r);
        if (!(after >= 1e-20 * before))
            DMRGX_FAIL(DMRGX_ERR_ARG, "eigs_lowest_orth: row %d of Q is linearly dependent on the rows before it (norm %.3e of %.3e left after projection)", r, std::sqrt(std::max(after, 0.0)), std::sqrt(before));
    }

    // ---- start vector: the caller's or random, projected against Qt; v_0 into its row and into x -----------------------------------------
    int rejected = 0;
    for (int attempt = opts->use_initial ? 0 : 1; attempt < 2; ++attempt) {
        if (attempt == 0) hipLaunchKernelGGL(eo_copy_rows_kernel, dim3(R.nblk, 1), dim3(RANGE_THREADS), 0, st, (const double*)psi_dev, n, R.w, ld, n);
        else hipLaunchKernelGGL(eo_random_kernel, dim3(R.nblk), dim3(RANGE_THREADS), 0, st, R.w, n, opts->seed);
        DMRGX_HIP(hipGetLastError());
        DMRGX_CHK(R.orthonormalise(R.w, nq, nq, nullptr, nullptr, S + o_start, V, R.x));
        DMRGX_CHK(R.dS.read(host, st));
        const double raw = host[o_start], proj = host[o_start + 1];
        const bool ok = proj > 0.0 && proj < INFINITY && (attempt == 1 || proj >= std::max(opts->min_initial_norm2, 1e-20 * raw));
        if (ok) break;
        if (attempt == 1) DMRGX_FAIL(DMRGX_ERR_INTERNAL, "eigs_lowest_orth: the random start vector has no finite part outside span(Q) (squared norm %g)", proj);
        rejected = 1;
    }

    // ---- thick-restart Lanczos on the complement -----------------------------------------------------------------------------------------
    std::vector<double> kept, y((size_t)m, 0.0), hbuf((size_t)(m + 1) * row, 0.0), rot;
    int k = 0, n_matvec = 0, restarts = 0, converged = 0, mm = 0;
    double resid = 0.0, lambda = 0.0;
    while (true) {
        Ritz ritz;
        bool early = false;
        for (int j = k; j < m; ++j) {
            DMRGX_CHK(dmrgx_kron_apply(plan, R.x, R.w, st));
            ++n_matvec;
            DMRGX_CHK(R.orthonormalise(R.w, nq + j + 1, nq, Hrow(j), Hrow(j) + m + 1, nullptr, V + (int64_t)(j + 1) * ld, R.x));
            // the step's column of T: the one read-back, and the step's synchronisation
            DMRGX_HIP(hipMemcpyAsync(hbuf.data() + (size_t)j * row, Hrow(j), (size_t)row * sizeof(double), hipMemcpyDeviceToHost, st));
            DMRGX_HIP(hipStreamSynchronize(st));
            mm = j + 1;
            ritz = ritz_of_leading(mm, m, row, hbuf, kept);
            if (mm < m && ritz.resid <= tol * std::max(std::fabs(ritz.th[0]), 1e-300)) { early = true; break; }
        }
        lambda = ritz.th[0];
        resid = ritz.resid;
        std::fill(y.begin(), y.end(), 0.0);
        for (int i = 0; i < mm; ++i) y[i] = ritz.Q[(size_t)i * mm + 0];
        ++restarts;
        if (early) { converged = 1; break; }
        if (resid <= tol * std::max(std::fabs(lambda), 1e-300) || m == space) { converged = 1; break; }      // (m == space: the whole complement, exact)
        if (restarts >= max_it) break;
        // thick restart: keep the kk lowest Ritz vectors and the residual direction v_m
        const int kk = std::max(1, std::min(m / 2, m - 1));
        rot.assign((size_t)m * kk, 0.0);
        for (int i = 0; i < m; ++i) for (int j = 0; j < kk; ++j) rot[(size_t)i * kk + j] = ritz.Q[(size_t)i * m + j];
        DMRGX_HIP(h2d_async(R.dR.p, rot.data(), rot.size() * sizeof(double), st));
        hipLaunchKernelGGL(eo_restart_kernel, dim3(R.nblk), dim3(RANGE_THREADS), 0, st, V, ld, m, kk, n, (const double*)R.dR.as<double>(), R.x);
        DMRGX_HIP(hipGetLastError());
        DMRGX_HIP(hipStreamSynchronize(st));                       // (rot is rewritten by the next restart)
        kept.assign(ritz.th.begin(), ritz.th.begin() + kk);
        k = kk;
    }

    // ---- psi = V y, projected against Qt once more, normalised --------------------------------------------------------------------------
    DMRGX_HIP(h2d_async(R.dR.p, y.data(), (size_t)mm * sizeof(double), st));
    hipLaunchKernelGGL(eo_combine_kernel, dim3(R.nblk), dim3(RANGE_THREADS), 0, st, (const double*)V, ld, mm, n, (const double*)R.dR.as<double>(), R.w);
    DMRGX_HIP(hipGetLastError());
    DMRGX_CHK(R.dots(false, R.w, nq, R.c1));
    hipLaunchKernelGGL(eo_normalise_kernel, dim3(R.nblk), dim3(RANGE_THREADS), 0, st, (const double*)R.w, (const double*)R.B, ld, nq, n, (const double*)R.c1, (const double*)R.c1, nq,
                       (double*)nullptr, (double*)nullptr, (double*)nullptr, R.x, (double*)nullptr);
    DMRGX_HIP(hipGetLastError());
    DMRGX_HIP(hipMemcpyAsync(psi_dev, R.x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    DMRGX_HIP(hipStreamSynchronize(st));
    *e = lambda;
    if (stats) {
        stats->n_matvec = n_matvec; stats->n_restart = restarts; stats->converged = converged; stats->start_rejected = rejected; stats->residual = resid;
        stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    }
    if (!converged) DMRGX_FAIL(DMRGX_ERR_NOTCONV, "eigs_lowest_orth: not converged after %d restarts (residual %.3e)", restarts, resid);
    return DMRGX_OK;
}
