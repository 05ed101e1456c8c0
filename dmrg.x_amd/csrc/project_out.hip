// One vector removed from a family of vectors: for every row a < nv of V, c_a = <v_a, p> / <p, p> and v_a -= c_a p.  What a dynamical
// measurement of an operator with a ground-state expectation value needs before its first MatMult: (D_b - <D_b>) psi for all bonds b at
// once (-dsf_dimer), without which the elastic line carries all the weight.  An engine extension in the idiom of lanczos.hip and
// corrvec.hip: the range layout of krylov.h, everything decided on the device, one copy and one synchronisation at the end.
//   dots          : workgroup b keeps its RANGE_LEN elements of p in registers, walks the nv rows and leaves partial[a][b]; row nv is <p, p>
//   coefficients  : ONE workgroup adds the partials in block order (a wave per row: lanes b, b + 64, .., then shuffle-down 32..1), divides,
//                   and decides: <p, p> not positive and finite -> every coefficient 0; a row whose dot is not finite -> that coefficient 0
//   update        : the same ranges, p again in registers: v_a[e] -= c_a p[e]; a row with c_a == 0 is not read at all
// Traffic: p twice, V twice read and once written -- rows are NOT spread over a second grid dimension, which would read p once per row.
// The sums are carried as unevaluated pairs (s, c) of doubles -- TwoProduct by fma, TwoSum, Ogita-Rump-Oishi's Dot2 -- through the thread,
// the wave, the workgroup, the partials and the division: c_a is the quotient of the two exact sums to a rounding or two, whatever the
// length.  A row that IS a multiple of p -- 3 p as stored -- comes back with the coefficient 3.0 itself and leaves only the rounding of
// its own elements behind; sums rounded to a double each cannot promise that (their quotient is one spacing off 3.0 in a good third of
// the cases, and the row then keeps 4u |p_e| of p).  The arithmetic is free: both passes wait for the memory.  So the single-value sums
// of krylov.h do not serve here; their ORDER does (lanes 32..1, waves 0..3, partials b, b + stride): fixed grids, no atomics, same bits.
#include "krylov.h"
#include <cmath>

namespace dmrgx {
namespace {

// The error-free transformations below hold for the IEEE operations as written: a product contracted into the sum that follows it
// (hipcc's default, -ffp-contract=fast, does that across statements) is a different sum.  The fused operations wanted are spelled fma().
#pragma clang fp contract(off)

// s + c, |c| small against |s|: a sum that has not been rounded yet
struct dd { double s, c; };

__device__ __forceinline__ dd dd_zero() { return dd{0.0, 0.0}; }
// a + b = s + e exactly (Knuth)
__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
// acc += x y, the product taken exactly
__device__ __forceinline__ void dd_fma(dd& acc, double x, double y) {
    const double h = x * y, l = fma(x, y, -h);
    double e;
    two_sum(acc.s, h, acc.s, e);
    acc.c += e + l;
}
__device__ __forceinline__ dd dd_add(dd a, dd b) {
    dd r;
    double e;
    two_sum(a.s, b.s, r.s, e);
    r.c = (a.c + b.c) + e;
    return r;
}
// the wave's sum, valid in lane 0: wave_sum's order
__device__ __forceinline__ dd dd_wave_sum(dd v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        dd w;
        w.s = __shfl_down(v.s, o, 64);
        w.c = __shfl_down(v.c, o, 64);
        v = dd_add(v, w);
    }
    return v;
}
__device__ __forceinline__ double dd_value(dd a) { return a.s + a.c; }

constexpr int PO_WAVES = RANGE_THREADS / 64;
constexpr int PO_COEF_THREADS = 1024;              // the one workgroup of the coefficient stage: 16 waves, a row each at a time

// partial[(a nblk + b)] = <v_a, p> over block b's range, a < nv; a == nv: <p, p>.  VEC: V, p 16-byte aligned and ldv even
template <bool VEC> __global__ void __launch_bounds__(RANGE_THREADS) po_dots_kernel(int nv, int64_t n, const double* __restrict__ V, int64_t ldv, const double* __restrict__ p,
                                                                                    double2* __restrict__ partial)
{
    __shared__ double2 red[2][PO_WAVES];                         // two rows in flight: one barrier per row
    double2 pr[RANGE_PAIRS];
#pragma unroll
    for (int i = 0; i < RANGE_PAIRS; ++i) pr[i] = load2<VEC>(p, range_pair(i), n);       // (beyond n: zeros)
    const int nblk = (int)gridDim.x;
    for (int a = 0; a <= nv; ++a) {
        const double* __restrict__ row = a < nv ? V + (int64_t)a * ldv : p;
        double2 vr[RANGE_PAIRS];
#pragma unroll
        for (int i = 0; i < RANGE_PAIRS; ++i) vr[i] = a < nv ? load2<VEC>(row, range_pair(i), n) : pr[i];
        dd acc = dd_zero();
#pragma unroll
        for (int i = 0; i < RANGE_PAIRS; ++i) { dd_fma(acc, vr[i].x, pr[i].x); dd_fma(acc, vr[i].y, pr[i].y); }
        acc = dd_wave_sum(acc);
        if ((threadIdx.x & 63) == 0) red[a & 1][threadIdx.x >> 6] = make_double2(acc.s, acc.c);
        __syncthreads();
        if (threadIdx.x == 0) {
            dd t = dd_zero();
            for (int k = 0; k < PO_WAVES; ++k) t = dd_add(t, dd{red[a & 1][k].x, red[a & 1][k].y});
            partial[(int64_t)a * nblk + blockIdx.x] = make_double2(t.s, t.c);
        }
    }
}

// row a of the partials added in block order by one wave, valid in lane 0
__device__ __forceinline__ dd po_row_sum(const double2* __restrict__ partial, int a, int nblk) {
    dd s = dd_zero();
    for (int b = threadIdx.x & 63; b < nblk; b += 64) { const double2 x = partial[(int64_t)a * nblk + b]; s = dd_add(s, dd{x.x, x.y}); }
    return dd_wave_sum(s);
}

// out[a] = c_a, a < nv; out[nv] = <p, p>; out[nv + 1] = the flag: <p, p> is not a positive finite number (then everything else is 0)
__global__ void __launch_bounds__(PO_COEF_THREADS) po_coef_kernel(int nv, int nblk, const double2* __restrict__ partial, double* __restrict__ out)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    dd pp = po_row_sum(partial, nv, nblk);                       // every wave for itself: no barrier
    pp.s = __shfl(pp.s, 0, 64);
    pp.c = __shfl(pp.c, 0, 64);
    double ps = pp.s + pp.c;                                     // <p, p> as ps + pc
    const double pc = pp.c - (ps - pp.s);
    const bool ok = ps > 0.0 && ps < INFINITY;
    if (wave == 0 && lane == 0) { out[nv] = ok ? ps : 0.0; out[nv + 1] = ok ? 0.0 : 1.0; }
    for (int a = wave; a < nv; a += PO_COEF_THREADS / 64) {
        const dd d = po_row_sum(partial, a, nblk);               // (lane 0 holds the sum; the other lanes divide what they have and store nothing)
        double c = 0.0;
        if (ok && fabs(dd_value(d)) < INFINITY) {
            // (ds + dc) / (ps + pc): one step of the long division on the exact remainder
            const double q = d.s / ps, r = fma(-q, ps, d.s) + (d.c - q * pc);
            c = q + r / ps;
            if (!(fabs(c) < INFINITY)) c = 0.0;
        }
        if (lane == 0) out[a] = c;
    }
}

// v_a[e] -= c_a p[e] over block b's range; c_a == 0 (a refused p, a row whose dot is not finite, a row orthogonal already): not touched
template <bool VEC> __global__ void __launch_bounds__(RANGE_THREADS) po_update_kernel(int nv, int64_t n, double* __restrict__ V, int64_t ldv, const double* __restrict__ p,
                                                                                      const double* __restrict__ coef)
{
    double2 pr[RANGE_PAIRS];
#pragma unroll
    for (int i = 0; i < RANGE_PAIRS; ++i) pr[i] = load2<VEC>(p, range_pair(i), n);
    for (int a = 0; a < nv; ++a) {
        const double c = coef[a];
        if (c == 0.0) continue;
        double* __restrict__ row = V + (int64_t)a * ldv;
        double2 vr[RANGE_PAIRS];
#pragma unroll
        for (int i = 0; i < RANGE_PAIRS; ++i) vr[i] = load2<VEC>(row, range_pair(i), n);
#pragma unroll
        for (int i = 0; i < RANGE_PAIRS; ++i) {
            vr[i].x = fma(-c, pr[i].x, vr[i].x);
            vr[i].y = fma(-c, pr[i].y, vr[i].y);
            store2<VEC>(row, range_pair(i), n, vr[i]);           // (beyond n nothing is stored)
        }
    }
}

}  // namespace
}  // namespace dmrgx

using namespace dmrgx;

extern "C" dmrgx_status dmrgx_vec_project_out(int32_t nv, int64_t len, double* V_dev, int64_t ldv, const double* p_dev, double* coef, double* p_norm2, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!V_dev || !p_dev || !coef || !p_norm2) DMRGX_FAIL(DMRGX_ERR_ARG, "vec_project_out: null argument");
    if (nv < 1) DMRGX_FAIL(DMRGX_ERR_ARG, "vec_project_out: nv %d, at least one row is needed", nv);
    if (len < 0) DMRGX_FAIL(DMRGX_ERR_ARG, "vec_project_out: len %lld is negative", (long long)len);
    if (ldv < len) DMRGX_FAIL(DMRGX_ERR_ARG, "vec_project_out: ldv %lld is smaller than len %lld", (long long)ldv, (long long)len);
    const size_t nn = (size_t)len, v_span = (size_t)(nv - 1) * (size_t)ldv + nn;
    if (spans_overlap(p_dev, nn, V_dev, v_span)) DMRGX_FAIL(DMRGX_ERR_ARG, "vec_project_out: p overlaps V");
    for (int32_t a = 0; a < nv; ++a) coef[a] = 0.0;
    *p_norm2 = 0.0;
    if (len == 0) return DMRGX_OK;
    const int nblk = range_blocks(len);
    const bool vec = (((uintptr_t)V_dev | (uintptr_t)p_dev) & 15) == 0 && (ldv & 1) == 0;

    DevBuf dPartial;
    DevScalars dOut;                                             // (poisoned like every f64 workspace: every entry is written before it is read)
    DMRGX_CHK(dPartial.alloc_f64((size_t)2 * (size_t)(nv + 1) * (size_t)nblk, st));
    DMRGX_CHK(dOut.buf.alloc_f64((size_t)nv + 2, st));
    double2* P = dPartial.as<double2>();
    double* out = dOut.dev();
    const dim3 grid((unsigned)nblk), block(RANGE_THREADS);
    if (vec) hipLaunchKernelGGL(po_dots_kernel<true>, grid, block, 0, st, (int)nv, len, (const double*)V_dev, ldv, p_dev, P);
    else hipLaunchKernelGGL(po_dots_kernel<false>, grid, block, 0, st, (int)nv, len, (const double*)V_dev, ldv, p_dev, P);
    hipLaunchKernelGGL(po_coef_kernel, dim3(1), dim3(PO_COEF_THREADS), 0, st, (int)nv, nblk, (const double2*)P, out);
    if (vec) hipLaunchKernelGGL(po_update_kernel<true>, grid, block, 0, st, (int)nv, len, V_dev, ldv, p_dev, (const double*)out);
    else hipLaunchKernelGGL(po_update_kernel<false>, grid, block, 0, st, (int)nv, len, V_dev, ldv, p_dev, (const double*)out);
    DMRGX_HIP(hipGetLastError());
    std::vector<double> host((size_t)nv + 1);
    DMRGX_CHK(dOut.read(host, st));
    for (int32_t a = 0; a < nv; ++a) coef[a] = host[(size_t)a];
    *p_norm2 = host[(size_t)nv];
    return DMRGX_OK;
}
