// Gram matrix of two families of long vectors on MFMA f64:  G[i][j] (=|+=) sum_{n < len} U[i][n] * V[j][n].
//
// The all-pairs correlation tables <O_i psi, O_j psi> are this product with a few hundred vectors of the superblock dimension:
// an "NT" GEMM with tiny M, N and K in the millions, which the grouped GEMM (NN, no split over K outside the MatMult's plan) cannot
// run.  Both families are stored with len contiguous, so both MFMA operands of v_mfma_f64_16x16x4_f64 are "row l&15, some k": the sum
// over k does not care which k a lane feeds as long as U and V agree, so lane l owns the contiguous run k0 + 4 (l>>4) + {0,1,2,3} of
// every 16-long chunk and feeds it MFMA by MFMA -- two 16-byte loads per operand row, no transposition, no LDS.
//
// One wave computes one output tile of at most 64 x 64 (16 accumulators) over one slice of len and writes it to a slab; a second
// kernel adds the slices of a tile in slice order (no atomics: the result repeats bit for bit, as slab_reduce_kernel's does).  Tile
// counts and the slice length come from the shape only.  When U and V are the same family only the tiles on and above the diagonal
// are computed and the reduction writes both G[i][j] and G[j][i]; inside a diagonal tile (i,j) and (j,i) see the same products in
// the same order, so G comes back bitwise symmetric.
#include "common.h"

namespace dmrgx {
namespace {

constexpr int GRAM_T = 64;                      // tile edge
constexpr int GRAM_KC = 16;                     // k per chunk: 4 MFMAs per accumulator
constexpr int64_t GRAM_MIN_SLICE = 1024;        // shortest slice worth a workgroup of its own
constexpr int64_t GRAM_TARGET_WAVES = 2048;     // slices x tiles aimed at: two waves per SIMD of a 256-CU part (a constant: shape-only tiling)

typedef double gram_acc __attribute__((ext_vector_type(4)));

struct GramShape {
    int32_t nu, nv, TN, sym, slices;
    int64_t len, ldu, ldv, slice_len;
};

// tile number -> (ti, tj); sym: the tiles with tj >= ti, row by row
__device__ inline void gram_tile_of(int32_t t, int32_t TN, int32_t sym, int32_t& ti, int32_t& tj)
{
    if (!sym) { ti = t / TN; tj = t - ti * TN; return; }
    ti = 0;
    while (t >= TN - ti) { t -= TN - ti; ++ti; }
    tj = ti + t;
}

// 4 contiguous doubles behind an 8-byte aligned pointer (pointers and leading dimensions are only 8-byte aligned)
__device__ inline void gram_load4(const double* p, double (&v)[4]) { __builtin_memcpy(v, p, 4 * sizeof(double)); }

template <bool FULL>
__device__ inline void gram_tile_body(const GramShape& g, const double* __restrict__ U, const double* __restrict__ V, int32_t ti, int32_t tj,
                                      int64_t kbeg, int64_t kend, double* __restrict__ out)
{
    const int lane = threadIdx.x, r16 = lane & 15, h = lane >> 4;
    const int mb_n = FULL ? 4 : (min(GRAM_T, g.nu - ti * GRAM_T) + 15) / 16, nb_n = FULL ? 4 : (min(GRAM_T, g.nv - tj * GRAM_T) + 15) / 16;
    // rows past nu / nv are clamped to the last row: computed, never stored
    const double* up[4];
    const double* vp[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        up[b] = U + (int64_t)min(ti * GRAM_T + 16 * b + r16, g.nu - 1) * g.ldu + 4 * h;
        vp[b] = V + (int64_t)min(tj * GRAM_T + 16 * b + r16, g.nv - 1) * g.ldv + 4 * h;
    }
    gram_acc acc[4][4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[mb][nb] = gram_acc{0.0, 0.0, 0.0, 0.0};

    double a[4][4], b[4][4];
    int64_t k = kbeg;
#pragma unroll 2
    for (; k + GRAM_KC <= kend; k += GRAM_KC) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (FULL || q < mb_n) gram_load4(up[q] + k, a[q]);
            if (FULL || q < nb_n) gram_load4(vp[q] + k, b[q]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
                    if (FULL || (mb < mb_n && nb < nb_n)) acc[mb][nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mb][r], b[nb][r], acc[mb][nb], 0, 0, 0);
    }
    if (k < kend) {
        // the len edge: nothing past kend is read (with ld > len the next doubles are someone else's), both operands are exact zeros there
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool in = k + 4 * h + r < kend;
                a[q][r] = (in && (FULL || q < mb_n)) ? up[q][k + r] : 0.0;
                b[q][r] = (in && (FULL || q < nb_n)) ? vp[q][k + r] : 0.0;
            }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
                    if (FULL || (mb < mb_n && nb < nb_n)) acc[mb][nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mb][r], b[nb][r], acc[mb][nb], 0, 0, 0);
    }
    // C/D map of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
            if (FULL || (mb < mb_n && nb < nb_n)) {
#pragma unroll
                for (int r = 0; r < 4; ++r) out[(16 * mb + h + 4 * r) * GRAM_T + 16 * nb + r16] = acc[mb][nb][r];
            }
}

// block t * slices + s: tile t over slice s -> slab[(t * slices + s) * 64 * 64 ...] (compact 64 x 64; the blocks of 16 rows / columns that
// lie wholly outside G are not written and never read)
__global__ void __launch_bounds__(64) gram_tile_kernel(GramShape g, const double* __restrict__ U, const double* __restrict__ V, double* __restrict__ slab)
{
    const int32_t t = (int32_t)(blockIdx.x / (uint32_t)g.slices), s = (int32_t)(blockIdx.x - (uint32_t)t * (uint32_t)g.slices);
    int32_t ti, tj;
    gram_tile_of(t, g.TN, g.sym, ti, tj);
    const int64_t kbeg = (int64_t)s * g.slice_len, kend = min(g.len, kbeg + g.slice_len);
    double* out = slab + (int64_t)blockIdx.x * (GRAM_T * GRAM_T);
    if (g.nu - ti * GRAM_T >= GRAM_T && g.nv - tj * GRAM_T >= GRAM_T) gram_tile_body<true>(g, U, V, ti, tj, kbeg, kend, out);
    else gram_tile_body<false>(g, U, V, ti, tj, kbeg, kend, out);
}

// G (=|+=) slice 0 + slice 1 + ... of every tile, in slice order; sym: an off-diagonal tile is written to both triangles
__global__ void __launch_bounds__(256) gram_reduce_kernel(GramShape g, const double* __restrict__ slab, double* __restrict__ G, int64_t ldg, int accumulate)
{
    int32_t ti, tj;
    gram_tile_of((int32_t)blockIdx.x, g.TN, g.sym, ti, tj);
    const int e = blockIdx.y * 256 + threadIdx.x, i = e / GRAM_T, j = e % GRAM_T;
    const int32_t gi = ti * GRAM_T + i, gj = tj * GRAM_T + j;
    if (gi >= g.nu || gj >= g.nv) return;
    const double* p = slab + (int64_t)blockIdx.x * g.slices * (GRAM_T * GRAM_T) + e;
    double sum = 0.0;
    for (int32_t s = 0; s < g.slices; ++s) sum += p[(int64_t)s * (GRAM_T * GRAM_T)];
    double* d = G + (int64_t)gi * ldg + gj;
    *d = accumulate ? *d + sum : sum;
    if (g.sym && ti != tj) {
        double* m = G + (int64_t)gj * ldg + gi;
        *m = accumulate ? *m + sum : sum;
    }
}

}  // namespace
}  // namespace dmrgx

using namespace dmrgx;

extern "C" dmrgx_status dmrgx_vec_gram(int32_t nu, int32_t nv, int64_t len, const double* U_dev, int64_t ldu, const double* V_dev, int64_t ldv,
                                       double* G_dev, int64_t ldg, int32_t accumulate, dmrgx_gram_report* report, void* stream)
{
    if (nu < 1 || nv < 1 || len < 0 || !G_dev || ldg < nv) DMRGX_FAIL(DMRGX_ERR_ARG, "vec_gram: bad argument (nu=%d nv=%d len=%lld ldg=%lld)", nu, nv, (long long)len, (long long)ldg);
    if (len > 0 && (!U_dev || !V_dev || ldu < len || ldv < len)) DMRGX_FAIL(DMRGX_ERR_ARG, "vec_gram: null family or leading dimension below len (len=%lld ldu=%lld ldv=%lld)", (long long)len, (long long)ldu, (long long)ldv);
    hipStream_t st = (hipStream_t)stream;
    GramShape g{};
    g.nu = nu; g.nv = nv; g.len = len; g.ldu = ldu; g.ldv = ldv;
    g.sym = (len > 0 && U_dev == V_dev && ldu == ldv && nu == nv) ? 1 : 0;
    const int64_t TM = (nu + GRAM_T - 1) / GRAM_T, TN = (nv + GRAM_T - 1) / GRAM_T;
    const int64_t tiles = g.sym ? TN * (TN + 1) / 2 : TM * TN;
    g.TN = (int32_t)TN;
    int64_t slices = 0;
    if (len > 0) {
        slices = std::min<int64_t>(std::max<int64_t>((GRAM_TARGET_WAVES + tiles - 1) / tiles, 1), (len + GRAM_MIN_SLICE - 1) / GRAM_MIN_SLICE);
        g.slice_len = (((len + slices - 1) / slices + GRAM_KC - 1) / GRAM_KC) * GRAM_KC;
        slices = (len + g.slice_len - 1) / g.slice_len;
    }
    g.slices = (int32_t)slices;
    if (tiles * std::max<int64_t>(slices, 1) >= (int64_t)1 << 31) DMRGX_FAIL(DMRGX_ERR_ARG, "vec_gram: %lld x %lld output tiles are more than one launch holds", (long long)TM, (long long)TN);
    const int64_t slab_doubles = tiles * slices * (GRAM_T * GRAM_T);
    if (report) *report = dmrgx_gram_report{(int32_t)tiles, (int32_t)slices, slab_doubles};
    if (len == 0 && accumulate) return DMRGX_OK;
    DevBuf slab;                                        // back to the pool on exit; recycling is stream-ordered
    if (slices > 0) {
        DMRGX_CHK(slab.alloc_f64((size_t)slab_doubles, st));
        hipLaunchKernelGGL(gram_tile_kernel, dim3((unsigned)(tiles * slices)), dim3(64), 0, st, g, U_dev, V_dev, slab.as<double>());
    }
    hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)tiles, GRAM_T * GRAM_T / 256), dim3(256), 0, st, g, (const double*)slab.as<double>(), G_dev, ldg, accumulate ? 1 : 0);
    DMRGX_HIP(hipGetLastError());
    return DMRGX_OK;
}
