// Lanczos coefficients of the planned superblock Hamiltonian from a given start vector: the tridiagonal matrix behind a
// continued-fraction (Lanczos-vector) spectral function such as S(q, w).  An engine extension like the Gram calls: nothing in the
// reference computes dynamics.
//
// Plain three-term recursion, no basis kept and no reorthogonalisation: three vectors with rotating roles (q_{j-1}, q_j, w).  Per step
//   MatMult        : w = H q_j
//   pass 1         : w -= beta_{j-1} q_{j-1} ; partial sums of q_j . w            (reads 3 vectors, writes 1)
//   alpha          : alpha_j = sum of the partials in block order
//   pass 2         : w -= alpha_j q_j ; partial sums of w . w                     (reads 2, writes 1)
//   beta           : beta_j = sqrt(sum), the breakdown decision, 1 / beta_j
//   scale          : q_{j+1} = w / beta_j in place, or exact zeros once dead      (reads 1, writes 1)
// Every scalar the next kernel needs -- beta_{j-1}, alpha_j, 1/beta_j, the dead flag -- lives in a small device array, so the whole run
// is enqueued without looking at the device; one copy and one synchronisation at the end bring the coefficients back.  Fixed grids and
// fixed-order sums of block partials, no atomics: two runs give the same bits.
// dmrgx_kron_lanczos_basis, further down, is the same run with the basis kept and fully reorthogonalised.
// dmrgx_kron_chebyshev_moments, after it, is the Chebyshev recursion in the same idiom: moments in place of coefficients, no normalisation.
#include "krylov.h"
#include <cmath>

namespace dmrgx {
namespace {

constexpr int LZ_BLOCKS = 1024, LZ_THREADS = 256;
// the device scalars: S[LZ_COEF + j] = alpha_j, S[LZ_COEF + nsteps + j] = beta_j
enum : int { LZ_NORM2 = 0, LZ_DEAD = 1, LZ_SCALE = 2, LZ_DONE = 3, LZ_INV = 4, LZ_BETA_PREV = 5, LZ_ALPHA = 6, LZ_COEF = 8 };

// partial[b] = sum of x[e]^2 over e = b LZ_THREADS + thread, strided by the whole grid (corrvec.hip sums contiguous ranges: other bits)
__global__ void __launch_bounds__(LZ_THREADS) lz_norm2_kernel(const double* __restrict__ x, int64_t n, double* __restrict__ partial)
{
    double acc = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * LZ_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * LZ_THREADS) acc += x[e] * x[e];
    acc = block_sum<LZ_THREADS>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// w -= beta_{j-1} q_{j-1} ; partial[b] = q_j . w over block b
__global__ void __launch_bounds__(LZ_THREADS) lz_pass1_kernel(double* __restrict__ w, const double* __restrict__ qprev, const double* __restrict__ qcur,
                                                             int64_t n, const double* __restrict__ S, double* __restrict__ partial)
{
    const double bp = S[LZ_BETA_PREV];
    double acc = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * LZ_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * LZ_THREADS) {
        const double x = w[e] - bp * qprev[e];
        w[e] = x;
        acc += qcur[e] * x;
    }
    acc = block_sum<LZ_THREADS>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// w -= alpha_j q_j ; partial[b] = w . w over block b
__global__ void __launch_bounds__(LZ_THREADS) lz_pass2_kernel(double* __restrict__ w, const double* __restrict__ qcur, int64_t n,
                                                             const double* __restrict__ S, double* __restrict__ partial)
{
    const double a = S[LZ_ALPHA];
    double acc = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * LZ_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * LZ_THREADS) {
        const double x = w[e] - a * qcur[e];
        w[e] = x;
        acc += x * x;
    }
    acc = block_sum<LZ_THREADS>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// dst = src / beta, and dst2 too unless it is null; exact zeros when there is no next vector (whatever src holds).  src may be dst
// (the three-term run scales in place): neither is __restrict__.  dst2 is never src or dst.
__global__ void __launch_bounds__(LZ_THREADS) lz_scale_kernel(const double* src, double* dst, double* __restrict__ dst2, int64_t n, const double* __restrict__ S)
{
    const double inv = S[LZ_INV];
    for (int64_t e = (int64_t)blockIdx.x * LZ_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * LZ_THREADS) {
        const double q = inv != 0.0 ? src[e] * inv : 0.0;
        dst[e] = q;
        if (dst2) dst2[e] = q;
    }
}

// Thread 0 of a scalar kernel, step j alive with finite sums: beta_j = sqrt(s) and the breakdown decision against
// max(|alpha_i|, i <= j; beta_i, i < j), a = alpha_j.  The step counts; *inv = 1 / beta_j when there is a next vector, else the run is dead.
__device__ __forceinline__ double lz_decide_beta(double* __restrict__ S, double s, double a, int j, double tol, double* inv)
{
    const double scale = fmax(S[LZ_SCALE], fabs(a)), beta = sqrt(s);
    S[LZ_DONE] = (double)(j + 1);
    if (beta > tol * scale) { *inv = 1.0 / beta; S[LZ_SCALE] = fmax(scale, beta); S[LZ_BETA_PREV] = beta; }
    else { S[LZ_DEAD] = 1.0; S[LZ_BETA_PREV] = 0.0; }
    return beta;
}

// One workgroup: the partials added in block order, then the scalar logic of the stage.
//   stage 0 (start): norm2 = |v0|^2; not a positive finite number -> dead from the start, reported as 0 with no step done
//   stage 1 (alpha): alpha_j, 0 once dead; a NaN or infinite sum -> dead, step j not counted, alpha_j = 0
//   stage 2 (beta):  beta_j and the breakdown decision: beta_j <= tol * max(|alpha_i|, i <= j; beta_i, i < j) -> dead, steps done = j + 1;
//                    the beta of the breaking step is kept as measured, every later coefficient is 0 and no 1/beta is ever formed of it
__global__ void __launch_bounds__(LZ_THREADS) lz_reduce_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ S, int stage, int j, int nsteps, double tol)
{
    const double s = sum_partials<LZ_THREADS>(partial, nblk);
    if (threadIdx.x != 0) return;
    const bool dead = S[LZ_DEAD] != 0.0;
    if (stage == 0) {
        const bool ok = s > 0.0 && s < INFINITY;
        S[LZ_NORM2] = ok ? s : 0.0;
        S[LZ_DEAD] = ok ? 0.0 : 1.0;
        S[LZ_INV] = ok ? 1.0 / sqrt(s) : 0.0;
    } else if (stage == 1) {
        // a sum that is not a finite number ends the run before step j counts: steps done stays j, alpha_j and all that follows are 0
        const bool ok = !dead && fabs(s) < INFINITY;
        if (!dead && !ok) { S[LZ_DEAD] = 1.0; S[LZ_BETA_PREV] = 0.0; }
        const double a = ok ? s : 0.0;
        S[LZ_ALPHA] = a;
        S[LZ_COEF + j] = a;
    } else {
        double beta = 0.0, inv = 0.0;
        if (!dead && !(s >= 0.0 && s < INFINITY)) { S[LZ_DEAD] = 1.0; S[LZ_BETA_PREV] = 0.0; S[LZ_ALPHA] = 0.0; S[LZ_COEF + j] = 0.0; }      // likewise: step j does not count
        else if (!dead) beta = lz_decide_beta(S, s, S[LZ_ALPHA], j, tol, &inv);
        S[LZ_INV] = inv;
        S[LZ_COEF + nsteps + j] = beta;
    }
}


// ---- the basis-keeping, fully reorthogonalised run (dmrgx_kron_lanczos_basis) ---------------------------------------------------------
// Row j of V is q_j.  After the three-term step above (pass 1, alpha, pass 2 -- the same kernels), w is orthogonalised against all of
// q_0..q_j twice by classical Gram-Schmidt:  h = V_{0..j} w  (multi-dot, then one reduction per k),  w -= V_{0..j}^T h  (multi-axpy).
// alpha_j is everything removed along q_j (the three-term alpha plus h_j of both passes), beta_j = |w| after the second pass.
// Both kernels are streaming reads of V_{0..j} in the range layout of krylov.h: a workgroup keeps its piece of w in registers (8 doubles
// per thread) and lets the rows go past in 16-byte loads -- V_{0..j} and w are read once per kernel.
constexpr int LB_KC = 64;

// partial[k * gridDim.x + b] = sum over block b's range of V[k * ldv + e] * w[e],  k < nk.  Wave sums go to LDS per k and are added in
// wave order once per LB_KC rows, so that there is no barrier per row.
template <bool VEC> __global__ void __launch_bounds__(RANGE_THREADS) lb_multidot_kernel(const double* __restrict__ w, const double* __restrict__ V, int64_t ldv, int nk, int64_t n,
                                                                                        double* __restrict__ partial)
{
    __shared__ double red[LB_KC][RANGE_THREADS / 64];
    double2 wr[RANGE_PAIRS];
#pragma unroll
    for (int t = 0; t < RANGE_PAIRS; ++t) wr[t] = load2<true>(w, range_pair(t), n);      // (w: a pool block, 256-byte aligned)
    for (int k0 = 0; k0 < nk; k0 += LB_KC) {
        const int kc = min(LB_KC, nk - k0);
        for (int kk = 0; kk < kc; ++kk) {
            const double* __restrict__ row = V + (int64_t)(k0 + kk) * ldv;
            double2 v[RANGE_PAIRS];
#pragma unroll
            for (int t = 0; t < RANGE_PAIRS; ++t) v[t] = load2<VEC>(row, range_pair(t), n);
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
}

// block k: h[k] = the partials of row k added in block order
__global__ void __launch_bounds__(LZ_THREADS) lb_hreduce_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ h)
{
    const double s = sum_partials<LZ_THREADS>(partial + (int64_t)blockIdx.x * nblk, nblk);
    if (threadIdx.x == 0) h[blockIdx.x] = s;
}

// w -= sum_{k < nk} h[k] V[k];  NORM: partial[b] = w . w over block b's range afterwards
template <bool VEC, bool NORM> __global__ void __launch_bounds__(RANGE_THREADS) lb_multiaxpy_kernel(double* __restrict__ w, const double* __restrict__ V, int64_t ldv, int nk, int64_t n,
                                                                                                    const double* __restrict__ h, double* __restrict__ partial)
{
    double2 wr[RANGE_PAIRS];
#pragma unroll
    for (int t = 0; t < RANGE_PAIRS; ++t) wr[t] = load2<true>(w, range_pair(t), n);
    for (int k = 0; k < nk; ++k) {
        const double* __restrict__ row = V + (int64_t)k * ldv;
        const double hk = h[k];
        double2 v[RANGE_PAIRS];
#pragma unroll
        for (int t = 0; t < RANGE_PAIRS; ++t) v[t] = load2<VEC>(row, range_pair(t), n);
#pragma unroll
        for (int t = 0; t < RANGE_PAIRS; ++t) { wr[t].x -= hk * v[t].x; wr[t].y -= hk * v[t].y; }
    }
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < RANGE_PAIRS; ++t) {
        store2<true>(w, range_pair(t), n, wr[t]);
        if (NORM) { acc += wr[t].x * wr[t].x; acc += wr[t].y * wr[t].y; }      // (beyond n the registers hold zeros)
    }
    if (NORM) {
        acc = block_sum<RANGE_THREADS>(acc);
        if (threadIdx.x == 0) partial[blockIdx.x] = acc;
    }
}

// One workgroup: stage 2 of lz_reduce_kernel for the reorthogonalised step.  alpha_j = the three-term alpha + h_j of both passes;
// beta_j = sqrt of the partials added in block order; the same breakdown rule, the same end on a sum that is not a finite number.
__global__ void __launch_bounds__(LZ_THREADS) lb_beta_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ S, const double* __restrict__ h1,
                                                             const double* __restrict__ h2, int j, int nsteps, double tol)
{
    const double s = sum_partials<LZ_THREADS>(partial, nblk);
    if (threadIdx.x != 0) return;
    double beta = 0.0, inv = 0.0, a = 0.0;
    if (S[LZ_DEAD] == 0.0) {
        a = S[LZ_ALPHA] + h1[j] + h2[j];
        if (!(fabs(a) < INFINITY) || !(s >= 0.0 && s < INFINITY)) { S[LZ_DEAD] = 1.0; S[LZ_BETA_PREV] = 0.0; a = 0.0; }      // step j does not count
        else beta = lz_decide_beta(S, s, a, j, tol, &inv);
    }
    S[LZ_ALPHA] = a;
    S[LZ_COEF + j] = a;
    S[LZ_INV] = inv;
    S[LZ_COEF + nsteps + j] = beta;
}

// A run that a non-finite sum ended inside step j leaves q_j in row j although step j does not count: rows >= steps done are zeros.
// (After a breakdown that row holds zeros already; a run that went through has no such row.)
__global__ void __launch_bounds__(LZ_THREADS) lb_zero_uncounted_row_kernel(double* __restrict__ V, int64_t ldv, int64_t n, int nsteps, const double* __restrict__ S)
{
    const int done = (int)S[LZ_DONE];
    if (S[LZ_DEAD] == 0.0 || done >= nsteps) return;
    double* __restrict__ row = V + (int64_t)done * ldv;
    for (int64_t e = (int64_t)blockIdx.x * LZ_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * LZ_THREADS) row[e] = 0.0;
}


// ---- Chebyshev moments (dmrgx_kron_chebyshev_moments) ---------------------------------------------------------------------------------
// t_0 = v0, t_1 = Ht t_0, t_{n+1} = 2 Ht t_n - t_{n-1} with Ht = (H - centre) / half_width: no normalisation, no reorthogonalisation, two
// earlier vectors.  Per step
//   MatMult        : w = H x                                   (x = t_n and w are two fixed pool vectors)
//   step           : t_{n+1} = s (w - centre x) - t_{n-1}, s = 2 / half_width (1 / half_width and no t_{n-1} for t_1), into ring row
//                    (n + 1) % 32 and into x; partial sums of t_{n+1} . t_{n+1} and t_{n+1} . t_n     (reads 3 vectors, writes 2)
//   scalars        : the partials added in block order, the guard, mu_{2n+1} and mu_{2n+2}
// and once per 16 vectors one dmrgx_vec_gram of U against the 16 ring rows just completed.  The scalars and all moments live in one
// device array that is copied back once at the end.
constexpr int CB_RING = 32, CB_BLOCK = 16;
constexpr double CB_GUARD = 1.0 + 1e-6;
// S[CB_VALID] = number of valid vectors t_0 .. t_{valid-1} (0: v0 itself was refused); S[CB_MOM + m] = mu_diag[m], then the cross moments
enum : int { CB_NORM2 = 0, CB_DEAD = 1, CB_VALID = 2, CB_MU1 = 3, CB_MOM = 4 };

// x = row = v0, or exact zeros when v0 was refused.  (v0 is the caller's: 8-byte loads)
__global__ void __launch_bounds__(LZ_THREADS) cb_start_kernel(const double* __restrict__ v0, double* __restrict__ row, double* __restrict__ x, int64_t n, const double* __restrict__ S)
{
    const bool dead = S[CB_DEAD] != 0.0;
    for (int64_t e = (int64_t)blockIdx.x * LZ_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * LZ_THREADS) {
        const double v = dead ? 0.0 : v0[e];
        row[e] = v;
        x[e] = v;
    }
}

// One step of the recursion over the workgroup's RANGE_LEN contiguous elements (the last range is ragged: nothing at or past n is read or
// written).  FIRST: t_1 = (w - centre x) / half_width, the row of t_{-1} does not exist and is not read.  x, w, prev and next are 16-byte
// aligned (pool blocks; ring rows with an even leading dimension).  partial[b] = t_{n+1} . t_{n+1}, partial[gridDim.x + b] = t_{n+1} . t_n
// over block b.  Once the run is dead: zeros into next and x, whatever w and prev hold.
template <bool FIRST> __global__ void __launch_bounds__(LZ_THREADS) cb_step_kernel(const double* __restrict__ w, double* __restrict__ x, const double* __restrict__ prev,
                                                                                  double* __restrict__ next, int64_t n, double centre, double scale,
                                                                                  const double* __restrict__ S, double* __restrict__ partial)
{
    const bool dead = S[CB_DEAD] != 0.0;
    double2 t[RANGE_PAIRS], c[RANGE_PAIRS];
#pragma unroll
    for (int i = 0; i < RANGE_PAIRS; ++i) { t[i] = double2{0.0, 0.0}; c[i] = double2{0.0, 0.0}; }
    if (!dead) {
        double2 wr[RANGE_PAIRS], pr[RANGE_PAIRS];
#pragma unroll
        for (int i = 0; i < RANGE_PAIRS; ++i) {
            const int64_t e = range_pair(i);
            wr[i] = load2<true>(w, e, n);
            c[i] = load2<true>(x, e, n);
            if (!FIRST) pr[i] = load2<true>(prev, e, n);
        }
#pragma unroll
        for (int i = 0; i < RANGE_PAIRS; ++i) {
            t[i].x = scale * (wr[i].x - centre * c[i].x);
            t[i].y = scale * (wr[i].y - centre * c[i].y);
            if (!FIRST) { t[i].x -= pr[i].x; t[i].y -= pr[i].y; }
        }
    }
    double tt = 0.0, tc = 0.0;
#pragma unroll
    for (int i = 0; i < RANGE_PAIRS; ++i) {
        store2<true>(next, range_pair(i), n, t[i]);
        store2<true>(x, range_pair(i), n, t[i]);
        tt += t[i].x * t[i].x; tt += t[i].y * t[i].y;            // (beyond n the registers hold zeros)
        tc += t[i].x * c[i].x; tc += t[i].y * c[i].y;
    }
    tt = block_sum<RANGE_THREADS>(tt);
    tc = block_sum<RANGE_THREADS>(tc);
    if (threadIdx.x == 0) { partial[blockIdx.x] = tt; partial[gridDim.x + blockIdx.x] = tc; }
}

// One workgroup.  stage 0 (start): partial = the blocks' sums of v0^2; mu_0 = norm2, or the run is dead with no valid vector.
// stage 1 (step n, which made t_{n+1}): both sums in block order; the guard -- |t_{n+1}|^2 not finite or above (1 + 1e-6) mu_0, or a
// cross sum that is not finite -- ends the run with t_n the last valid vector; else mu_{2n+1} = 2 t_{n+1}.t_n - mu_1 (n = 0: mu_1 itself)
// and mu_{2n+2} = 2 t_{n+1}.t_{n+1} - mu_0.  The moments of a dead run stay the zeros the array was filled with.
__global__ void __launch_bounds__(LZ_THREADS) cb_scalar_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ S, int stage, int n)
{
    const double a = sum_partials<LZ_THREADS>(partial, nblk), b = stage ? sum_partials<LZ_THREADS>(partial + nblk, nblk) : 0.0;
    if (threadIdx.x != 0) return;
    if (stage == 0) {
        const bool ok = a > 0.0 && a < INFINITY;
        S[CB_NORM2] = ok ? a : 0.0;
        S[CB_DEAD] = ok ? 0.0 : 1.0;
        S[CB_VALID] = ok ? 1.0 : 0.0;
        S[CB_MOM] = ok ? a : 0.0;
        return;
    }
    if (S[CB_DEAD] != 0.0) return;
    const double mu0 = S[CB_NORM2];
    if (!(a >= 0.0 && a <= CB_GUARD * mu0) || !(fabs(b) < INFINITY)) { S[CB_DEAD] = 1.0; return; }
    const double mu1 = n ? S[CB_MU1] : b;
    if (n == 0) S[CB_MU1] = b;
    S[CB_VALID] = (double)(n + 2);
    S[CB_MOM + 2 * n + 1] = 2.0 * b - mu1;
    S[CB_MOM + 2 * n + 2] = 2.0 * a - mu0;
}

// Before the Gram call of the ring rows that hold t_{n0} .. t_{n0 + rows - 1}: the rows of vectors that are not valid -- the one the guard
// refused, and a refused v0 -- become exact zeros.  blockIdx.y: the row.  A run that is alive returns at once.
__global__ void __launch_bounds__(LZ_THREADS) cb_zero_invalid_rows_kernel(double* __restrict__ rows, int64_t ldr, int64_t n, int n0, const double* __restrict__ S)
{
    if (S[CB_DEAD] == 0.0 || n0 + (int)blockIdx.y < (int)S[CB_VALID]) return;
    double* __restrict__ row = rows + (int64_t)blockIdx.y * ldr;
    for (int64_t e = (int64_t)blockIdx.x * LZ_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * LZ_THREADS) row[e] = 0.0;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// vec: every row of V is 16-byte aligned
void lb_multidot(bool vec, int nblk, hipStream_t st, const double* w, const double* V, int64_t ldv, int nk, int64_t n, double* partial)
{
    const auto kernel = vec ? lb_multidot_kernel<true> : lb_multidot_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(nblk), dim3(RANGE_THREADS), 0, st, w, V, ldv, nk, n, partial);
}

void lb_multiaxpy(bool vec, bool norm, int nblk, hipStream_t st, double* w, const double* V, int64_t ldv, int nk, int64_t n, const double* h, double* partial)
{
    const auto kernel = vec ? (norm ? lb_multiaxpy_kernel<true, true> : lb_multiaxpy_kernel<true, false>) : (norm ? lb_multiaxpy_kernel<false, true> : lb_multiaxpy_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(nblk), dim3(RANGE_THREADS), 0, st, w, V, ldv, nk, n, h, partial);
}

// the end of both Lanczos calls: the one copy and synchronisation, then norm2, the steps done and the coefficients
dmrgx_status lz_read_out(const DevScalars& S, int32_t nsteps, double* norm2, double* alpha, double* beta, int32_t* nsteps_done, hipStream_t st)
{
    std::vector<double> host((size_t)LZ_COEF + 2 * (size_t)nsteps);
    DMRGX_CHK(S.read(host, st));
    *norm2 = host[LZ_NORM2];
    *nsteps_done = (int32_t)host[LZ_DONE];
    for (int32_t j = 0; j < nsteps; ++j) { alpha[j] = host[LZ_COEF + j]; beta[j] = host[LZ_COEF + nsteps + j]; }
    return DMRGX_OK;
}

}  // namespace
}  // namespace dmrgx

using namespace dmrgx;

extern "C" dmrgx_status dmrgx_kron_chebyshev_moments(dmrgx_kron_plan* plan, const double* v0_dev, double centre, double half_width, int32_t nsteps,
                                                     int32_t nu, const double* U_dev, int64_t ldu, double* norm2, double* mu_diag, double* mu_cross,
                                                     int32_t* nsteps_done, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!plan || !v0_dev || !norm2 || !mu_diag || !nsteps_done || (nu > 0 && !mu_cross)) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_chebyshev_moments: null argument");
    if (nsteps < 1) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_chebyshev_moments: nsteps %d, at least one step is needed", nsteps);
    if (!(half_width > 0.0 && half_width < INFINITY) || !(fabs(centre) < INFINITY))
        DMRGX_FAIL(DMRGX_ERR_ARG, "kron_chebyshev_moments: window centre %g, half width %g: a finite centre and a positive finite half width are needed", centre, half_width);
    if (nu < 0) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_chebyshev_moments: nu %d is negative", nu);
    int64_t n = 0;
    DMRGX_CHK(whole_plan_states(plan, "kron_chebyshev_moments", "recursion", &n));
    if (nu > 0 && (!U_dev || ldu < n)) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_chebyshev_moments: U is null or ldu %lld is smaller than n_states %lld", (long long)ldu, (long long)n);
    const int64_t K = nsteps, ldr = (n + 1) & ~(int64_t)1;      // ring rows 16-byte aligned
    const int nblk = range_blocks(n);
    const size_t ndiag = (size_t)(2 * K + 1), nscal = (size_t)CB_MOM + ndiag + (size_t)(K + 1) * (size_t)nu;

    DevBuf dX, dW, dRing, dPartial;
    DevScalars dS;
    DMRGX_CHK(dX.alloc_f64((size_t)n, st));
    DMRGX_CHK(dW.alloc_f64((size_t)n, st));
    DMRGX_CHK(dRing.alloc_f64((size_t)CB_RING * (size_t)ldr, st));
    DMRGX_CHK(dPartial.alloc_f64((size_t)std::max(LZ_BLOCKS, 2 * nblk), st));
    DMRGX_CHK(dS.alloc_zeroed(nscal, st));
    double* S = dS.dev();
    double* P = dPartial.as<double>();
    double* x = dX.as<double>();
    double* w = dW.as<double>();
    double* ring = dRing.as<double>();
    double* cross = S + CB_MOM + ndiag;                          // [nu][K + 1] on the device: a Gram call writes 16 columns of it

    // the cross moments of t_{n0} .. t_{n0 + rows - 1}, which fill one block of 16 ring rows from its first row on
    auto gram_block = [&](int64_t n0, int rows) -> dmrgx_status {
        double* first = ring + (n0 % CB_RING) * ldr;
        hipLaunchKernelGGL(cb_zero_invalid_rows_kernel, dim3((unsigned)std::min(nblk, LZ_BLOCKS), (unsigned)rows), dim3(LZ_THREADS), 0, st, first, ldr, n, (int)n0, (const double*)S);
        DMRGX_HIP(hipGetLastError());
        if (nu > 0) DMRGX_CHK(dmrgx_vec_gram(nu, rows, n, U_dev, ldu, first, ldr, cross + n0, K + 1, 0, nullptr, st));
        return DMRGX_OK;
    };

    hipLaunchKernelGGL(lz_norm2_kernel, dim3(LZ_BLOCKS), dim3(LZ_THREADS), 0, st, v0_dev, n, P);
    hipLaunchKernelGGL(cb_scalar_kernel, dim3(1), dim3(LZ_THREADS), 0, st, (const double*)P, LZ_BLOCKS, S, 0, 0);
    hipLaunchKernelGGL(cb_start_kernel, dim3(LZ_BLOCKS), dim3(LZ_THREADS), 0, st, v0_dev, ring, x, n, (const double*)S);
    DMRGX_HIP(hipGetLastError());
    for (int64_t j = 0; j < K; ++j) {                            // step j: t_{j+1} from x = t_j and ring row of t_{j-1}
        double* next = ring + ((j + 1) % CB_RING) * ldr;
        DMRGX_CHK(dmrgx_kron_apply(plan, x, w, st));
        if (j == 0) hipLaunchKernelGGL(cb_step_kernel<true>, dim3(nblk), dim3(RANGE_THREADS), 0, st, (const double*)w, x, (const double*)nullptr, next, n, centre, 1.0 / half_width, (const double*)S, P);
        else hipLaunchKernelGGL(cb_step_kernel<false>, dim3(nblk), dim3(RANGE_THREADS), 0, st, (const double*)w, x, (const double*)(ring + ((j - 1) % CB_RING) * ldr), next, n, centre, 2.0 / half_width, (const double*)S, P);
        hipLaunchKernelGGL(cb_scalar_kernel, dim3(1), dim3(LZ_THREADS), 0, st, (const double*)P, nblk, S, 1, (int)j);
        DMRGX_HIP(hipGetLastError());
        if ((j + 2) % CB_BLOCK == 0) DMRGX_CHK(gram_block(j + 2 - CB_BLOCK, CB_BLOCK));      // t_{j+1} completes a block of 16
    }
    if ((K + 1) % CB_BLOCK) DMRGX_CHK(gram_block((K + 1) / CB_BLOCK * CB_BLOCK, (int)((K + 1) % CB_BLOCK)));
    std::vector<double> host(nscal);
    DMRGX_CHK(dS.read(host, st));
    const int64_t valid = (int64_t)host[CB_VALID], D = std::max<int64_t>(valid - 1, 0);
    *norm2 = host[CB_NORM2];
    *nsteps_done = (int32_t)D;
    for (int64_t m = 0; m <= 2 * K; ++m) mu_diag[m] = host[CB_MOM + m];
    const double* hc = host.data() + CB_MOM + ndiag;
    for (int64_t r = 0; r <= K; ++r)
        for (int32_t i = 0; i < nu; ++i) mu_cross[r * nu + i] = hc[(int64_t)i * (K + 1) + r];
    return DMRGX_OK;
}

extern "C" dmrgx_status dmrgx_kron_lanczos_coeffs(dmrgx_kron_plan* plan, const double* v0_dev, int32_t nsteps, double breakdown_tol,
                                                  double* norm2, double* alpha, double* beta, int32_t* nsteps_done, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!plan || !v0_dev || !norm2 || !alpha || !beta || !nsteps_done) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_lanczos_coeffs: null argument");
    if (nsteps < 1) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_lanczos_coeffs: nsteps %d, at least one step is needed", nsteps);
    if (!(breakdown_tol >= 0.0) || breakdown_tol >= 1.0) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_lanczos_coeffs: breakdown_tol %g outside [0, 1)", breakdown_tol);
    int64_t n = 0;
    DMRGX_CHK(whole_plan_states(plan, "kron_lanczos_coeffs", "recursion", &n));
    const double tol = breakdown_tol > 0.0 ? breakdown_tol : 1e-7;

    DevBuf dQ, dPartial;
    DevScalars dS;
    DMRGX_CHK(dQ.alloc_f64((size_t)3 * n, st));
    DMRGX_CHK(dPartial.alloc_f64((size_t)LZ_BLOCKS, st));
    DMRGX_CHK(dS.alloc_zeroed((size_t)LZ_COEF + 2 * (size_t)nsteps, st));
    double* S = dS.dev();
    double* P = dPartial.as<double>();
    double* qprev = dQ.as<double>();
    double* qcur = qprev + n;
    double* w = qcur + n;
    DMRGX_HIP(zero_async(qprev, (size_t)n * sizeof(double), st));      // q_{-1} = 0 (beta_{-1} = 0 multiplies it)

    hipLaunchKernelGGL(lz_norm2_kernel, dim3(LZ_BLOCKS), dim3(LZ_THREADS), 0, st, v0_dev, n, P);
    hipLaunchKernelGGL(lz_reduce_kernel, dim3(1), dim3(LZ_THREADS), 0, st, (const double*)P, LZ_BLOCKS, S, 0, 0, nsteps, tol);
    hipLaunchKernelGGL(lz_scale_kernel, dim3(LZ_BLOCKS), dim3(LZ_THREADS), 0, st, v0_dev, qcur, (double*)nullptr, n, (const double*)S);
    DMRGX_HIP(hipGetLastError());
    for (int32_t j = 0; j < nsteps; ++j) {
        DMRGX_CHK(dmrgx_kron_apply(plan, qcur, w, st));
        hipLaunchKernelGGL(lz_pass1_kernel, dim3(LZ_BLOCKS), dim3(LZ_THREADS), 0, st, w, (const double*)qprev, (const double*)qcur, n, (const double*)S, P);
        hipLaunchKernelGGL(lz_reduce_kernel, dim3(1), dim3(LZ_THREADS), 0, st, (const double*)P, LZ_BLOCKS, S, 1, j, nsteps, tol);
        hipLaunchKernelGGL(lz_pass2_kernel, dim3(LZ_BLOCKS), dim3(LZ_THREADS), 0, st, w, (const double*)qcur, n, (const double*)S, P);
        hipLaunchKernelGGL(lz_reduce_kernel, dim3(1), dim3(LZ_THREADS), 0, st, (const double*)P, LZ_BLOCKS, S, 2, j, nsteps, tol);
        hipLaunchKernelGGL(lz_scale_kernel, dim3(LZ_BLOCKS), dim3(LZ_THREADS), 0, st, (const double*)w, w, (double*)nullptr, n, (const double*)S);
        DMRGX_HIP(hipGetLastError());
        double* t = qprev; qprev = qcur; qcur = w; w = t;               // three buffers, three (x, y) pairs: the plan patches its tables once each
    }
    return lz_read_out(dS, nsteps, norm2, alpha, beta, nsteps_done, st);
}

extern "C" dmrgx_status dmrgx_kron_lanczos_basis(dmrgx_kron_plan* plan, const double* v0_dev, int32_t nsteps, double breakdown_tol, double* V_dev, int64_t ldv,
                                                 double* norm2, double* alpha, double* beta, int32_t* nsteps_done, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!plan || !v0_dev || !V_dev || !norm2 || !alpha || !beta || !nsteps_done) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_lanczos_basis: null argument");
    if (nsteps < 1) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_lanczos_basis: nsteps %d, at least one step is needed", nsteps);
    if (!(breakdown_tol >= 0.0) || breakdown_tol >= 1.0) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_lanczos_basis: breakdown_tol %g outside [0, 1)", breakdown_tol);
    int64_t n = 0;
    DMRGX_CHK(whole_plan_states(plan, "kron_lanczos_basis", "recursion", &n));
    if (ldv < n) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_lanczos_basis: ldv %lld is smaller than n_states %lld", (long long)ldv, (long long)n);
    if (spans_overlap(V_dev, (size_t)(nsteps - 1) * (size_t)ldv + (size_t)n, v0_dev, (size_t)n)) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_lanczos_basis: V overlaps v0");
    const double tol = breakdown_tol > 0.0 ? breakdown_tol : 1e-7;
    const int nblk = range_blocks(n);
    const bool vec = ((uintptr_t)V_dev & 15) == 0 && (ldv & 1) == 0;      // every row 16-byte aligned

    // x = q_j and w = H q_j are fixed buffers: the plan sees one (x, y) pair for the whole run, and never a row of V
    DevBuf dX, dW, dPartial, dRowPartial, dH;
    DevScalars dS;
    DMRGX_CHK(dX.alloc_f64((size_t)n, st));
    DMRGX_CHK(dW.alloc_f64((size_t)n, st));
    DMRGX_CHK(dPartial.alloc_f64((size_t)std::max(LZ_BLOCKS, nblk), st));
    DMRGX_CHK(dRowPartial.alloc_f64((size_t)nsteps * (size_t)nblk, st));
    DMRGX_CHK(dH.alloc_f64((size_t)2 * (size_t)nsteps, st));
    DMRGX_CHK(dS.alloc_zeroed((size_t)LZ_COEF + 2 * (size_t)nsteps, st));
    double* S = dS.dev();
    double* P = dPartial.as<double>();
    double* RP = dRowPartial.as<double>();
    double* h1 = dH.as<double>();
    double* h2 = h1 + nsteps;
    double* x = dX.as<double>();
    double* w = dW.as<double>();

    hipLaunchKernelGGL(lz_norm2_kernel, dim3(LZ_BLOCKS), dim3(LZ_THREADS), 0, st, v0_dev, n, P);
    hipLaunchKernelGGL(lz_reduce_kernel, dim3(1), dim3(LZ_THREADS), 0, st, (const double*)P, LZ_BLOCKS, S, 0, 0, nsteps, tol);
    hipLaunchKernelGGL(lz_scale_kernel, dim3(LZ_BLOCKS), dim3(LZ_THREADS), 0, st, v0_dev, V_dev, x, n, (const double*)S);
    DMRGX_HIP(hipGetLastError());
    for (int32_t j = 0; j < nsteps; ++j) {
        const double* qcur = V_dev + (int64_t)j * ldv;
        const double* qprev = j ? V_dev + (int64_t)(j - 1) * ldv : qcur;      // beta_{-1} = 0 multiplies a finite vector
        const int nk = j + 1;
        DMRGX_CHK(dmrgx_kron_apply(plan, x, w, st));
        hipLaunchKernelGGL(lz_pass1_kernel, dim3(LZ_BLOCKS), dim3(LZ_THREADS), 0, st, w, qprev, qcur, n, (const double*)S, P);
        hipLaunchKernelGGL(lz_reduce_kernel, dim3(1), dim3(LZ_THREADS), 0, st, (const double*)P, LZ_BLOCKS, S, 1, j, nsteps, tol);
        hipLaunchKernelGGL(lz_pass2_kernel, dim3(LZ_BLOCKS), dim3(LZ_THREADS), 0, st, w, qcur, n, (const double*)S, P);
        for (int pass = 0; pass < 2; ++pass) {
            double* h = pass ? h2 : h1;                                       // entries [0, j] are rewritten every step; entry j is what the beta kernel reads
            lb_multidot(vec, nblk, st, w, V_dev, ldv, nk, n, RP);
            hipLaunchKernelGGL(lb_hreduce_kernel, dim3(nk), dim3(LZ_THREADS), 0, st, (const double*)RP, nblk, h);
            lb_multiaxpy(vec, pass == 1, nblk, st, w, V_dev, ldv, nk, n, h, P);      // the second pass leaves the partials of w . w
        }
        hipLaunchKernelGGL(lb_beta_kernel, dim3(1), dim3(LZ_THREADS), 0, st, (const double*)P, nblk, S, (const double*)h1, (const double*)h2, j, nsteps, tol);
        if (j + 1 < nsteps) hipLaunchKernelGGL(lz_scale_kernel, dim3(LZ_BLOCKS), dim3(LZ_THREADS), 0, st, (const double*)w, V_dev + (int64_t)(j + 1) * ldv, x, n, (const double*)S);
        DMRGX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(lb_zero_uncounted_row_kernel, dim3(LZ_BLOCKS), dim3(LZ_THREADS), 0, st, V_dev, ldv, n, nsteps, (const double*)S);
    DMRGX_HIP(hipGetLastError());
    return lz_read_out(dS, nsteps, norm2, alpha, beta, nsteps_done, st);
}
