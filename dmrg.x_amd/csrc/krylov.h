// What the device-resident Krylov calls share: the workgroup sum in wave order, 16-byte pair accesses with a ragged tail, the range layout,
// the random start-vector stream, and the host-side checks and scalar array.  Internal, not part of the ABI.  Who uses what:
//   lanczos.hip                  all of it but the stream
//   corrvec.hip, response.hip    all of it but the stream, through cg.h, which adds what a conjugate-gradient run shares on top
//   eigs_orth.hip                the sums, pair accesses and range layout, the stream, whole_plan_states, DevScalars
//   eigs.hip                     the single-value sums and the stream (its random start vector is eigs_orth.hip's)
//   project_out.hip              the range layout, pair accesses and host side; its sums are pairs of doubles in the same order
//   lib.hip                      the single-value sums
//   states_expand.hip            spans_overlap
// The host side of a Lanczos restart cycle that eigs.hip and eigs_orth.hip share (Jacobi, Rayleigh-Ritz) is ritz.h.
// Every sum here has ONE order -- lanes by shuffle-down 32..1, waves 0..3, block partials b, b + THREADS, .. per thread -- and the bits
// of every caller depend on it.  Multi-value reductions (red[wave][i]) are deliberately not covered.
#pragma once
#include "common.h"

namespace dmrgx {

// the wave's sum of `v`, valid in lane 0
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// the workgroup's sum of `v`, valid in thread 0 (wave sums added in wave order).  Every thread of the workgroup calls it; it ends with
// a barrier, so the LDS is free again and it may be called back to back.
template <int THREADS> __device__ __forceinline__ double block_sum(double v) {
    __shared__ double red[THREADS / 64];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) for (int k = 0; k < THREADS / 64; ++k) t += red[k];
    __syncthreads();
    return t;
}

// partial[0 .. nblk) added in block order by one workgroup, valid in thread 0
template <int THREADS> __device__ __forceinline__ double sum_partials(const double* __restrict__ partial, int nblk) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += THREADS) s += partial[b];
    return block_sum<THREADS>(s);
}

// elements e, e + 1 of p (e even); beyond n: zeros, and nothing is read.  VEC: p + e is 16-byte aligned
template <bool VEC> __device__ __forceinline__ double2 load2(const double* __restrict__ p, int64_t e, int64_t n) {
    if (VEC && e + 1 < n) return *reinterpret_cast<const double2*>(p + e);
    double2 r;
    r.x = e < n ? p[e] : 0.0;
    r.y = e + 1 < n ? p[e + 1] : 0.0;
    return r;
}

template <bool VEC> __device__ __forceinline__ void store2(double* __restrict__ p, int64_t e, int64_t n, double2 v) {
    if (VEC && e + 1 < n) { *reinterpret_cast<double2*>(p + e) = v; return; }
    if (e < n) p[e] = v.x;
    if (e + 1 < n) p[e + 1] = v.y;
}

// The range layout: workgroup b of RANGE_THREADS threads owns the RANGE_LEN contiguous elements from b RANGE_LEN on, the last range
// ragged.  Kept in registers a thread holds 8 elements as RANGE_PAIRS pairs: pair i at range_pair(i), RANGE_THREADS pairs apart, so that a wave's
// loads are contiguous.  Walked element by element (the caller's 8-byte aligned vectors) a thread goes from range_first() in steps of
// RANGE_THREADS up to range_end(n).  A sum over a range is not the sum of a grid-strided kernel: see lz_norm2_kernel, cv_norm2_kernel.
constexpr int RANGE_THREADS = 256, RANGE_PAIRS = 4, RANGE_LEN = RANGE_THREADS * 2 * RANGE_PAIRS;
__device__ __forceinline__ int64_t range_first() { return (int64_t)blockIdx.x * RANGE_LEN + threadIdx.x; }
__device__ __forceinline__ int64_t range_pair(int i) { return (int64_t)blockIdx.x * RANGE_LEN + 2 * threadIdx.x + (int64_t)i * 2 * RANGE_THREADS; }
__device__ __forceinline__ int64_t range_end(int64_t n) {
    const int64_t end = (int64_t)(blockIdx.x + 1) * RANGE_LEN;
    return end < n ? end : n;
}
inline int range_blocks(int64_t n) { return (int)std::max<int64_t>(1, (n + RANGE_LEN - 1) / RANGE_LEN); }

// value `index` of the counter-based uniform(-1, 1) stream of `seed` (splitmix64 of seed + index + 1): the random start vectors.  A value
// depends on its index alone, whatever the kernel's loop looks like.
__device__ __forceinline__ double splitmix_uniform(uint64_t seed, int64_t index) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(index + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// *n = n_states of a plan that one rank holds whole; a striped plan is refused in the name of `call`, whose `noun` has no collectives
inline dmrgx_status whole_plan_states(dmrgx_kron_plan* plan, const char* call, const char* noun, int64_t* n) {
    dmrgx_kron_info I;
    DMRGX_CHK(dmrgx_kron_plan_info(plan, &I));
    if (I.vec_len != I.n_states || I.local_len != I.n_states)
        DMRGX_FAIL(DMRGX_ERR_ARG, "%s: the plan is striped over ranks (world_size > 1): the %s has no collectives", call, noun);
    *n = I.n_states;
    return DMRGX_OK;
}

// do `na` doubles at a and `nb` doubles at b share a byte?  (a null pointer or an empty span overlaps nothing)
inline bool spans_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na * sizeof(double), b0 = (uintptr_t)b, b1 = b0 + nb * sizeof(double);
    return a && b && na && nb && a0 < b1 && b0 < a1;
}

// The device scalars of a run: zeroed on the stream when made (never poisoned: flags live here), read back by one copy and one
// synchronisation.
struct DevScalars {
    DevBuf buf;
    dmrgx_status alloc_zeroed(size_t count, hipStream_t st) {
        DMRGX_CHK(buf.alloc(count * sizeof(double)));
        DMRGX_HIP(zero_async(buf.p, buf.bytes, st));
        return DMRGX_OK;
    }
    double* dev() const { return buf.as<double>(); }
    // the first host.size() scalars; returns once they are there
    dmrgx_status read(std::vector<double>& host, hipStream_t st) const {
        DMRGX_HIP(hipMemcpyAsync(host.data(), buf.p, host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        DMRGX_HIP(hipStreamSynchronize(st));
        return DMRGX_OK;
    }
};

}  // namespace dmrgx
