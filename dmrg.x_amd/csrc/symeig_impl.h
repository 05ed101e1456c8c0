// What the three translation units of the batched symmetric eigensolver share -- symeig.hip (driver, WY factors, second phase),
// symeig_trid.hip (tridiagonalisation), symeig_dc.hip (divide and conquer): the tuning constants, the reductions of the kernels, and
// the entry points of the two phases the driver calls.  Included by those three files only; not part of the library's interface.
#pragma once
#include "symeig.h"
#include "ggemm.h"
#include <cfloat>
#include <cmath>

namespace dmrgx {
// A namespace of its own: krylov.h has a wave_sum in dmrgx too (a shuffle-down into lane 0; the one here is an xor all-reduce, and the bits
// of every caller depend on which one it gets) -- a file that included both would not compile its first call instead of picking one.
namespace symeig_impl {

#ifndef DMRGX_DC_LEAF
#define DMRGX_DC_LEAF 16
#endif
constexpr int DC_LEAF = DMRGX_DC_LEAF;                // largest leaf of the divide-and-conquer tree.  Measured (same box; Rdms per step of configs[1] /
                                                      // truncation of cfg4real): 32: 2.00 / 8.85 ms, 16: 1.84 / 8.60, 8: 1.90 / 8.62 -- a Jacobi leaf of 16 costs a
                                                      // quarter of one of 32, which is more than the extra merge level takes
#ifndef DMRGX_DC_LEAF_THREADS
#define DMRGX_DC_LEAF_THREADS 128
#endif
constexpr int DC_LEAF_THREADS = DMRGX_DC_LEAF_THREADS;     // (leaf of 32: one wave measured 2x slower than 256 threads; leaf of 16: 128 threads as fast as 256)
#ifndef DMRGX_WY_NB
#define DMRGX_WY_NB 64
#endif
constexpr int WY_NB = DMRGX_WY_NB;                    // reflectors per block of the back-transformation.  -DDMRGX_WY_NB=128 (T assembled from two 64-halves, half as
                                                      // many dependent GEMM steps) measured SLOWER on the same box: 9.03-9.07 vs 8.72-8.74 ms per create at m = 2048
constexpr int WY_SUB = 64;                            // its T factor is inverted in halves: T = [T1, -T1 (V1^T V2) T2; 0, T2]
constexpr int TRID_MAXM = 32;                         // matrices per launch of the tridiagonalisation: their descriptors travel in the kernel argument segment
constexpr int DC_NVEC = 10, DC_NINT = 10;             // per-position double / int arrays of the divide and conquer (SymEigWs::vecs, ::ints)

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// The same sum in every lane without the LDS crossbar (ds_bpermute costs ~100 cycles per step on the latency path of every column):
// lane bits 0, 1 by quad permutes, bits 2, 3 by row rotations (a rotation all-reduce: after +ror4 and +ror8 every lane of a row
// holds the row's sum), bits 4, 5 by the gfx950 row / half swaps.
#define DMRGX_DPP_ADD(a, CTRL)                                                                                                   \
    {                                                                                                                            \
        const int lo_ = __double2loint(a), hi_ = __double2hiint(a);                                                              \
        a += __hiloint2double(__builtin_amdgcn_update_dpp(0, hi_, CTRL, 0xf, 0xf, false), __builtin_amdgcn_update_dpp(0, lo_, CTRL, 0xf, 0xf, false)); \
    }
__device__ __forceinline__ double wave_sum_fast(double a)
{
    DMRGX_DPP_ADD(a, 0xb1);      // quad_perm [1,0,3,2]
    DMRGX_DPP_ADD(a, 0x4e);      // quad_perm [2,3,0,1]
    DMRGX_DPP_ADD(a, 0x124);     // row_ror:4
    DMRGX_DPP_ADD(a, 0x128);     // row_ror:8
    int lo = __double2loint(a), hi = __double2hiint(a);
    auto l16 = __builtin_amdgcn_permlane16_swap((unsigned)lo, (unsigned)lo, false, false);
    auto h16 = __builtin_amdgcn_permlane16_swap((unsigned)hi, (unsigned)hi, false, false);
    a = __hiloint2double((int)h16[0], (int)l16[0]) + __hiloint2double((int)h16[1], (int)l16[1]);
    lo = __double2loint(a); hi = __double2hiint(a);
    auto l32 = __builtin_amdgcn_permlane32_swap((unsigned)lo, (unsigned)lo, false, false);
    auto h32 = __builtin_amdgcn_permlane32_swap((unsigned)hi, (unsigned)hi, false, false);
    return __hiloint2double((int)h32[0], (int)l32[0]) + __hiloint2double((int)h32[1], (int)l32[1]);
}
// one-barrier block sum: `red` must not be in use by waves that have not passed a barrier since they last read it
template <int NW>
__device__ __forceinline__ double block_sum1(double v, double* red, int tid)
{
    v = wave_sum_fast(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += red[w];
    return s;
}
__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
// sum over the workgroup; `red` holds one slot per wave.  Two barriers: the first also publishes whatever the callers wrote to
// LDS before the call, the second makes the partial sums visible.
template <int NW>
__device__ __forceinline__ double block_sum(double v, double* red, int tid)
{
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += red[w];
    return s;
}
template <int NW>
__device__ __forceinline__ double block_max(double v, double* red, int tid)
{
    v = wave_max(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) s = fmax(s, red[w]);
    return s;
}

// boundaries of the tree's nodes at a depth: repeated halving of [0, n)
inline std::vector<int> tree_bounds(int n, int level)
{
    std::vector<int> b{0, n};
    for (int l = 0; l < level; ++l) {
        std::vector<int> nb;
        for (size_t i = 0; i + 1 < b.size(); ++i) { nb.push_back(b[i]); nb.push_back((b[i] + b[i + 1]) / 2); }
        nb.push_back(n);
        b.swap(nb);
    }
    return b;
}
template <class K> dmrgx_status set_dyn_lds(K kernel, size_t bytes)
{
    if (bytes > 64 * 1024) DMRGX_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return DMRGX_OK;
}

// Everywhere below: M, the matrices of order > 0 of the call; ws[i], where the factors of M[i] sit in the workspaces B (doubles), I (ints).

// ---- 1. symeig_trid.hip: A -> d, e, tau and the reflectors V^T -----------------------------------------------------------------------
struct TridRun {                                      // what trid_enqueue leaves for trid_status_to_pinned; lives to the end of the call
    DevBuf gran;                                      // status word (first 16 bytes) + granule buffers of the persistent rounds
    bool persistent = false;                          // persistent rounds were launched
    const double* prof = nullptr;                     // DMRGX_TRID_PROF (developer aid): the phase clocks of the first round's first matrix,
    int prof_n = 0;                                   // and its order
};
// Plans the persistent rounds and enqueues them, and the column launches of the matrices that take that path, on st; fills the report's
// tridiagonalisation fields.
dmrgx_status trid_enqueue(const std::vector<SymEigMat>& M, const std::vector<SymEigWs>& ws, double* B, hipStream_t st, SymEigReport& rep, TridRun& run);
// Queues the copy of the persistent rounds' status word to pinned memory behind what st holds so far, and points status_host at it (left
// alone when no round ran).
dmrgx_status trid_status_to_pinned(const TridRun& run, hipStream_t st, const int32_t*& status_host);

// ---- 2. symeig_dc.hip: d, e -> the spectra w, and the eigenvectors of T up to the root merge (children in Q1, merge matrix in U) -----------
struct DcLevel { size_t merge_off = 0; int nmerge = 0, nlmax = 0; GemmSet gemm; };      // the merges that produce one level of the trees
struct DcTables { std::vector<DcLevel> levels; size_t o_mats = 0, o_leaves = 0, o_merges = 0; int nleaves = 0; };      // (offsets in the packed upload)
// Adds the GEMMs of every merge below the roots to `gemms`, and the scheduled tile lists and the descriptor tables to `pk`
void dc_add_tables(const std::vector<SymEigMat>& M, const std::vector<SymEigWs>& ws, double* B, int32_t* I, GemmBatch& gemms, PackedUpload& pk, DcTables& t);
// Leaves, then level by level, on st against the uploaded tables (`gemms` bound to them)
dmrgx_status dc_launch(const DcTables& t, int nm, int nmax, const GemmBatch& gemms, const DevBuf& d_tab, hipStream_t st);

}  // namespace symeig_impl
}  // namespace dmrgx
