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
#include "common.h"
#include <cmath>

namespace dmrgx {
namespace {

constexpr int LZ_BLOCKS = 1024, LZ_THREADS = 256;
// the device scalars: S[LZ_COEF + j] = alpha_j, S[LZ_COEF + nsteps + j] = beta_j
enum : int { LZ_NORM2 = 0, LZ_DEAD = 1, LZ_SCALE = 2, LZ_DONE = 3, LZ_INV = 4, LZ_BETA_PREV = 5, LZ_ALPHA = 6, LZ_COEF = 8 };

__device__ __forceinline__ double lz_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// the workgroup's sum of `v`, valid in thread 0 (wave sums added in wave order)
__device__ __forceinline__ double lz_block_sum(double v) {
    __shared__ double red[LZ_THREADS / 64];
    v = lz_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) for (int k = 0; k < LZ_THREADS / 64; ++k) t += red[k];
    return t;
}

// partial[b] = sum over block b's elements of x[e]^2
__global__ void __launch_bounds__(LZ_THREADS) lz_norm2_kernel(const double* __restrict__ x, int64_t n, double* __restrict__ partial)
{
    double acc = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * LZ_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * LZ_THREADS) acc += x[e] * x[e];
    acc = lz_block_sum(acc);
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
    acc = lz_block_sum(acc);
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
    acc = lz_block_sum(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// dst = src / beta, or exact zeros when there is no next vector (whatever src holds)
__global__ void __launch_bounds__(LZ_THREADS) lz_scale_kernel(const double* src, double* dst, int64_t n, const double* __restrict__ S)
{
    const double inv = S[LZ_INV];
    for (int64_t e = (int64_t)blockIdx.x * LZ_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * LZ_THREADS) dst[e] = inv != 0.0 ? src[e] * inv : 0.0;
}

// One workgroup: the partials added in block order, then the scalar logic of the stage.
//   stage 0 (start): norm2 = |v0|^2; not a positive finite number -> dead from the start, reported as 0 with no step done
//   stage 1 (alpha): alpha_j, 0 once dead; a NaN or infinite sum -> dead, step j not counted, alpha_j = 0
//   stage 2 (beta):  beta_j and the breakdown decision: beta_j <= tol * max(|alpha_i|, i <= j; beta_i, i < j) -> dead, steps done = j + 1;
//                    the beta of the breaking step is kept as measured, every later coefficient is 0 and no 1/beta is ever formed of it
__global__ void __launch_bounds__(LZ_THREADS) lz_reduce_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ S, int stage, int j, int nsteps, double tol)
{
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += LZ_THREADS) s += partial[b];
    s = lz_block_sum(s);
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
        else if (!dead) {
            const double scale = fmax(S[LZ_SCALE], fabs(S[LZ_ALPHA]));
            beta = sqrt(s);
            S[LZ_DONE] = (double)(j + 1);
            if (beta > tol * scale) { inv = 1.0 / beta; S[LZ_SCALE] = fmax(scale, beta); S[LZ_BETA_PREV] = beta; }
            else { S[LZ_DEAD] = 1.0; S[LZ_BETA_PREV] = 0.0; if (!(beta >= 0.0)) beta = 0.0; }
        }
        S[LZ_INV] = inv;
        S[LZ_COEF + nsteps + j] = beta;
    }
}

}  // namespace
}  // namespace dmrgx

using namespace dmrgx;

extern "C" dmrgx_status dmrgx_kron_lanczos_coeffs(dmrgx_kron_plan* plan, const double* v0_dev, int32_t nsteps, double breakdown_tol,
                                                  double* norm2, double* alpha, double* beta, int32_t* nsteps_done, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!plan || !v0_dev || !norm2 || !alpha || !beta || !nsteps_done) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_lanczos_coeffs: null argument");
    if (nsteps < 1) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_lanczos_coeffs: nsteps %d, at least one step is needed", nsteps);
    if (!(breakdown_tol >= 0.0) || breakdown_tol >= 1.0) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_lanczos_coeffs: breakdown_tol %g outside [0, 1)", breakdown_tol);
    dmrgx_kron_info I;
    DMRGX_CHK(dmrgx_kron_plan_info(plan, &I));
    if (I.vec_len != I.n_states || I.local_len != I.n_states)
        DMRGX_FAIL(DMRGX_ERR_ARG, "kron_lanczos_coeffs: the plan is striped over ranks (world_size > 1): the recursion has no collectives");
    const double tol = breakdown_tol > 0.0 ? breakdown_tol : 1e-7;
    const int64_t n = I.n_states;
    const size_t nscal = (size_t)LZ_COEF + 2 * (size_t)nsteps;

    DevBuf dQ, dPartial, dS;
    DMRGX_CHK(dQ.alloc_f64((size_t)3 * n, st));
    DMRGX_CHK(dPartial.alloc_f64((size_t)LZ_BLOCKS, st));
    DMRGX_CHK(dS.alloc(nscal * sizeof(double)));
    DMRGX_HIP(zero_async(dS.p, dS.bytes, st));
    double* S = dS.as<double>();
    double* P = dPartial.as<double>();
    double* qprev = dQ.as<double>();
    double* qcur = qprev + n;
    double* w = qcur + n;
    DMRGX_HIP(zero_async(qprev, (size_t)n * sizeof(double), st));      // q_{-1} = 0 (beta_{-1} = 0 multiplies it)

    hipLaunchKernelGGL(lz_norm2_kernel, dim3(LZ_BLOCKS), dim3(LZ_THREADS), 0, st, v0_dev, n, P);
    hipLaunchKernelGGL(lz_reduce_kernel, dim3(1), dim3(LZ_THREADS), 0, st, (const double*)P, LZ_BLOCKS, S, 0, 0, nsteps, tol);
    hipLaunchKernelGGL(lz_scale_kernel, dim3(LZ_BLOCKS), dim3(LZ_THREADS), 0, st, v0_dev, qcur, n, (const double*)S);
    DMRGX_HIP(hipGetLastError());
    for (int32_t j = 0; j < nsteps; ++j) {
        DMRGX_CHK(dmrgx_kron_apply(plan, qcur, w, st));
        hipLaunchKernelGGL(lz_pass1_kernel, dim3(LZ_BLOCKS), dim3(LZ_THREADS), 0, st, w, (const double*)qprev, (const double*)qcur, n, (const double*)S, P);
        hipLaunchKernelGGL(lz_reduce_kernel, dim3(1), dim3(LZ_THREADS), 0, st, (const double*)P, LZ_BLOCKS, S, 1, j, nsteps, tol);
        hipLaunchKernelGGL(lz_pass2_kernel, dim3(LZ_BLOCKS), dim3(LZ_THREADS), 0, st, w, (const double*)qcur, n, (const double*)S, P);
        hipLaunchKernelGGL(lz_reduce_kernel, dim3(1), dim3(LZ_THREADS), 0, st, (const double*)P, LZ_BLOCKS, S, 2, j, nsteps, tol);
        hipLaunchKernelGGL(lz_scale_kernel, dim3(LZ_BLOCKS), dim3(LZ_THREADS), 0, st, (const double*)w, w, n, (const double*)S);
        DMRGX_HIP(hipGetLastError());
        double* t = qprev; qprev = qcur; qcur = w; w = t;               // three buffers, three (x, y) pairs: the plan patches its tables once each
    }
    std::vector<double> host(nscal);
    DMRGX_HIP(hipMemcpyAsync(host.data(), S, nscal * sizeof(double), hipMemcpyDeviceToHost, st));
    DMRGX_HIP(hipStreamSynchronize(st));
    *norm2 = host[LZ_NORM2];
    *nsteps_done = (int32_t)host[LZ_DONE];
    for (int32_t j = 0; j < nsteps; ++j) { alpha[j] = host[LZ_COEF + j]; beta[j] = host[LZ_COEF + nsteps + j]; }
    return DMRGX_OK;
}
