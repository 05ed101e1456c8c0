// libdmrgx_hip.so: library-level entry points (error reporting, device probe, plain GEMM wrapper).
#include "ggemm.h"
#include "krylov.h"
#include <algorithm>

namespace dmrgx {
static thread_local std::string g_last_error;
void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}
}  // namespace dmrgx

using namespace dmrgx;

extern "C" int32_t dmrgx_abi_version(void) { return DMRGX_ABI_VERSION; }

extern "C" const char* dmrgx_last_error(void) { return g_last_error.c_str(); }

extern "C" dmrgx_status dmrgx_device_count(int32_t* n)
{
    if (!n) DMRGX_FAIL(DMRGX_ERR_ARG, "device_count: null argument");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess || c <= 0) {
        *n = 0;
        DMRGX_FAIL(DMRGX_ERR_DEVICE, "no HIP device available (%s): the dmrgx hot path has no CPU fallback", hipGetErrorString(e));
    }
    *n = c;
    return DMRGX_OK;
}

extern "C" dmrgx_status dmrgx_stripe_bounds(int32_t n_right, int32_t world_size, int32_t rank, int32_t* c0, int32_t* c1)
{
    if (!c0 || !c1 || n_right < 0 || world_size <= 0 || rank < 0 || rank >= world_size) DMRGX_FAIL(DMRGX_ERR_ARG, "stripe_bounds: bad argument");
    *c0 = dmrgx::stripe_cut(n_right, world_size, rank);
    *c1 = dmrgx::stripe_cut(n_right, world_size, rank + 1);
    return DMRGX_OK;
}

extern "C" dmrgx_status dmrgx_stripe_bounds_of_block(int32_t n_right, int32_t world_size, int32_t rank, int32_t block, int32_t* c0, int32_t* c1)
{
    if (!c0 || !c1 || n_right < 0 || world_size <= 0 || rank < 0 || rank >= world_size || block < 0) DMRGX_FAIL(DMRGX_ERR_ARG, "stripe_bounds_of_block: bad argument");
    const int32_t j = dmrgx::stripe_of_rank(world_size, rank, block);
    *c0 = dmrgx::stripe_cut(n_right, world_size, j);
    *c1 = dmrgx::stripe_cut(n_right, world_size, j + 1);
    return DMRGX_OK;
}

static bool bad_gemm_task(const dmrgx_gemm_task& g)
{
    return g.M < 0 || g.N < 0 || g.K < 0 || (g.M && g.N && (!g.C || g.ldc < g.N)) || (g.M && g.N && g.K && (!g.A || !g.B || g.lda < g.K || g.ldb < g.N));
}

// checked tasks in one grouped launch: tasks with M == 0 or N == 0 are skipped, K == 0 writes C = 0 (or leaves it, accumulating)
static dmrgx_status run_gemm_tasks(int32_t count, const dmrgx_gemm_task* t, hipStream_t st)
{
    GemmBatch b;
    GemmSet s;
    for (int32_t i = 0; i < count; ++i)
        b.gemm(s, t[i].C, (int32_t)t[i].ldc, t[i].M, t[i].N, t[i].A, (int32_t)t[i].lda, t[i].B, (int32_t)t[i].ldb, t[i].K, t[i].accumulate ? 1 : 0);
    if (b.groups.empty()) return DMRGX_OK;
    DevBuf tab;
    PackedUpload pk;
    b.pack(pk); b.pack(s, pk);
    DMRGX_CHK(pk.upload(tab, st));
    b.bind(tab);
    return b.launch(s, tab, st);
}

extern "C" dmrgx_status dmrgx_dgemm_nn(int32_t M, int32_t N, int32_t K, const double* A, int64_t lda,
                                       const double* B, int64_t ldb, double* C, int64_t ldc, void* stream)
{
    const dmrgx_gemm_task g{M, N, K, 0, A, lda, B, ldb, C, ldc};
    if (bad_gemm_task(g)) DMRGX_FAIL(DMRGX_ERR_ARG, "dgemm_nn: bad argument (M=%d N=%d K=%d)", M, N, K);
    return run_gemm_tasks(1, &g, (hipStream_t)stream);
}

extern "C" dmrgx_status dmrgx_dgemm_batch(int32_t count, const dmrgx_gemm_task* t, void* stream)
{
    if (count < 0 || (count > 0 && !t)) DMRGX_FAIL(DMRGX_ERR_ARG, "dgemm_batch: bad argument");
    for (int32_t i = 0; i < count; ++i)
        if (bad_gemm_task(t[i])) DMRGX_FAIL(DMRGX_ERR_ARG, "dgemm_batch: bad task %d (M=%d N=%d K=%d)", i, t[i].M, t[i].N, t[i].K);
    return run_gemm_tasks(count, t, (hipStream_t)stream);
}

// 0: fine; else what is wrong with product q of group g (leading dimensions travel as int32 in the device tables)
static const char* bad_ggemm_group(const dmrgx_ggemm_group& g, int32_t* q_bad)
{
    *q_bad = -1;
    if (g.M < 0 || g.N < 0 || g.nprods < 0) return "negative size";
    if (g.nprods > 0 && !g.prods) return "null product list";
    const bool live = g.M > 0 && g.N > 0;
    if (live && (!g.C || g.ldc < g.N || g.ldc > INT32_MAX)) return "null C or ldc < N";
    for (int32_t q = 0; q < g.nprods; ++q) {
        const dmrgx_ggemm_prod& p = g.prods[q];
        *q_bad = q;
        if (p.kind != GPROD_GEMM && p.kind != GPROD_AXPY) return "unknown kind";
        if (p.kind == GPROD_AXPY) {
            if (live && (!p.B || p.ldb < g.N || p.ldb > INT32_MAX)) return "scaled copy: null source or ldb < N";
            continue;
        }
        if (p.K < 0) return "negative K";
        if (live && p.K > 0 && (!p.A || !p.B || p.lda < p.K || p.ldb < g.N || p.lda > INT32_MAX || p.ldb > INT32_MAX)) return "null operand, lda < K or ldb < N";
    }
    return nullptr;
}

extern "C" dmrgx_status dmrgx_ggemm_groups(int32_t count, const dmrgx_ggemm_group* groups, int32_t tiling, dmrgx_ggemm_report* report, void* stream)
{
    if (count < 0 || (count > 0 && !groups) || (tiling != 0 && tiling != 1)) DMRGX_FAIL(DMRGX_ERR_ARG, "ggemm_groups: bad argument (count=%d tiling=%d)", count, tiling);
    for (int32_t i = 0; i < count; ++i) {
        int32_t q = -1;
        if (const char* why = bad_ggemm_group(groups[i], &q))
            DMRGX_FAIL(DMRGX_ERR_ARG, "ggemm_groups: bad group %d (M=%d N=%d nprods=%d, product %d): %s", i, groups[i].M, groups[i].N, groups[i].nprods, q, why);
    }
    hipStream_t st = (hipStream_t)stream;
    GemmBatch b;
    GemmSet s;
    for (int32_t i = 0; i < count; ++i) {
        const dmrgx_ggemm_group& g = groups[i];
        if (g.M == 0 || g.N == 0) continue;
        const int32_t pb = (int32_t)b.prods.size();
        int32_t cost = 0, n_axpy = 0;
        // the scaled copies first, in their own order, then the GEMM products in theirs
        for (int32_t q = 0; q < g.nprods; ++q)
            if (g.prods[q].kind == GPROD_AXPY) { b.prods.push_back(GProd{nullptr, g.prods[q].B, 0, (int32_t)g.prods[q].ldb, 0, GPROD_AXPY, g.prods[q].alpha}); ++n_axpy; ++cost; }
        for (int32_t q = 0; q < g.nprods; ++q) {
            const dmrgx_ggemm_prod& p = g.prods[q];
            if (p.kind != GPROD_GEMM || p.K == 0) continue;
            b.prods.push_back(GProd{p.A, p.B, (int32_t)p.lda, (int32_t)p.ldb, p.K, GPROD_GEMM, 1.0});
            cost += ggemm_ksteps(p.K);
        }
        b.group(s, GGroup{g.C, (int32_t)g.ldc, g.M, g.N, pb, (int32_t)b.prods.size(), n_axpy, g.accumulate ? 1 : 0}, cost, tiling == 0);
    }
    if (report) {
        *report = dmrgx_ggemm_report{(int32_t)s.big.size(), (int32_t)s.small.size(), 0, 0, ggemm_slots(2), ggemm_slots(1)};
    }
    if (b.groups.empty()) return DMRGX_OK;
    DevBuf tab;
    PackedUpload pk;
    b.pack(pk); b.pack(s, pk);
    if (report) { report->entries_big = (int32_t)s.big.size(); report->entries_small = (int32_t)s.small.size(); }
    DMRGX_CHK(pk.upload(tab, st));
    b.bind(tab);
    return b.launch(s, tab, st);
}

extern "C" dmrgx_status dmrgx_malloc(void** p, size_t bytes)
{
    if (!p) DMRGX_FAIL(DMRGX_ERR_ARG, "malloc: null argument");
    *p = nullptr;
    if (bytes == 0) return DMRGX_OK;
    hipError_t e = dmrgx::pool_malloc(p, bytes);
    if (e != hipSuccess) { *p = nullptr; DMRGX_FAIL(DMRGX_ERR_MEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); }
    if (dmrgx::pool_poison()) {                       // (the engine's SectorMat values: f64 only; no stream here, so the null stream and a wait)
        DMRGX_HIP(dmrgx::poison_f64_async(*p, bytes, nullptr));
        DMRGX_HIP(hipStreamSynchronize(nullptr));
    }
    return DMRGX_OK;
}
extern "C" dmrgx_status dmrgx_mem_stats(size_t* in_use, size_t* cached, size_t* peak_in_use)
{
    dmrgx::pool_stats(in_use, cached, peak_in_use);
    return DMRGX_OK;
}
extern "C" dmrgx_status dmrgx_free(void* p) { if (p) DMRGX_HIP(dmrgx::pool_free(p)); return DMRGX_OK; }
extern "C" dmrgx_status dmrgx_memcpy_h2d(void* d, const void* s, size_t n, void* st)
{ if (n) DMRGX_HIP(dmrgx::h2d_async(d, s, n, (hipStream_t)st)); return DMRGX_OK; }
extern "C" dmrgx_status dmrgx_memcpy_d2h(void* d, const void* s, size_t n, void* st)
{ if (n) { DMRGX_HIP(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, (hipStream_t)st)); DMRGX_HIP(hipStreamSynchronize((hipStream_t)st)); } return DMRGX_OK; }
extern "C" dmrgx_status dmrgx_memcpy_d2d(void* d, const void* s, size_t n, void* st)
{ if (n) DMRGX_HIP(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, (hipStream_t)st)); return DMRGX_OK; }
extern "C" dmrgx_status dmrgx_memset_zero(void* d, size_t n, void* st)
{ if (n) DMRGX_HIP(dmrgx::zero_async(d, n, (hipStream_t)st)); return DMRGX_OK; }
extern "C" dmrgx_status dmrgx_stream_sync(void* st) { DMRGX_HIP(hipStreamSynchronize((hipStream_t)st)); return DMRGX_OK; }

// ---- <x, y> on the device (correlators: VecDot of the reference, include/DMRGBlockContainer.hpp:2291) ------------------
namespace dmrgx {
namespace {
constexpr int VDOT_BLOCKS = 512, VDOT_THREADS = 256;
__global__ void __launch_bounds__(VDOT_THREADS) vdot_partial_kernel(const double* __restrict__ x, const double* __restrict__ y, int64_t n, double* __restrict__ partial)
{
    double s = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * VDOT_THREADS + threadIdx.x; e < n; e += (int64_t)VDOT_BLOCKS * VDOT_THREADS) s += x[e] * y[e];
    s = block_sum<VDOT_THREADS>(s);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
}  // namespace
}  // namespace dmrgx

namespace dmrgx {
namespace {
__global__ void __launch_bounds__(64) vdot_final_kernel(const double* __restrict__ partial, double* __restrict__ out)
{
    if (threadIdx.x == 0) { double t = 0.0; for (int k = 0; k < VDOT_BLOCKS; ++k) t += partial[k]; out[0] = t; }    // same order as the host sum of dmrgx_dot
}
}  // namespace
}  // namespace dmrgx

extern "C" dmrgx_status dmrgx_dot_async(int64_t n, const double* x_dev, const double* y_dev, double* dev_out, void* stream)
{
    if (n < 0 || !dev_out || (n > 0 && (!x_dev || !y_dev))) DMRGX_FAIL(DMRGX_ERR_ARG, "dot_async: bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { DMRGX_HIP(zero_async(dev_out, sizeof(double), st)); return DMRGX_OK; }
    DevBuf part;                                      // returned to the pool on exit; recycling is stream-ordered
    DMRGX_CHK(part.alloc_f64(dmrgx::VDOT_BLOCKS, st));
    hipLaunchKernelGGL(dmrgx::vdot_partial_kernel, dim3(dmrgx::VDOT_BLOCKS), dim3(dmrgx::VDOT_THREADS), 0, st, x_dev, y_dev, n, part.as<double>());
    hipLaunchKernelGGL(dmrgx::vdot_final_kernel, dim3(1), dim3(64), 0, st, (const double*)part.as<double>(), dev_out);
    DMRGX_HIP(hipGetLastError());
    return DMRGX_OK;
}

extern "C" dmrgx_status dmrgx_dot(int64_t n, const double* x_dev, const double* y_dev, double* host_out, void* stream)
{
    if (n < 0 || !host_out || (n > 0 && (!x_dev || !y_dev))) DMRGX_FAIL(DMRGX_ERR_ARG, "dot: bad argument");
    *host_out = 0.0;
    if (n == 0) return DMRGX_OK;
    hipStream_t st = (hipStream_t)stream;
    DevBuf part;
    DMRGX_CHK(part.alloc_f64(dmrgx::VDOT_BLOCKS, st));
    hipLaunchKernelGGL(dmrgx::vdot_partial_kernel, dim3(dmrgx::VDOT_BLOCKS), dim3(dmrgx::VDOT_THREADS), 0, st, x_dev, y_dev, n, part.as<double>());
    DMRGX_HIP(hipGetLastError());
    std::vector<double> h(dmrgx::VDOT_BLOCKS);
    DMRGX_HIP(hipMemcpyAsync(h.data(), part.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    DMRGX_HIP(hipStreamSynchronize(st));
    double t = 0.0;
    for (double v : h) t += v;          // fixed order: reproducible
    *host_out = t;
    return DMRGX_OK;
}

// ---- many Frobenius inner products in one launch (correlators of operators living on one block: <psi|P (x) 1|psi> =
//      sum_k <P[IL(k)], X_k X_k^T>_F, so a table of correlators is one batch of 2-D dot products against the Gram blocks) -----
namespace dmrgx {
namespace {
struct Dot2dPiece { const double* a; const double* b; int64_t lda, ldb; int32_t nr, nc; };
__global__ void __launch_bounds__(256) dot2d_partial_kernel(const Dot2dPiece* __restrict__ pieces, double* __restrict__ partial)
{
    __shared__ double red[4];
    const Dot2dPiece t = pieces[blockIdx.x];
    double s = 0.0;
    const int64_t tot = (int64_t)t.nr * t.nc;
    for (int64_t e = threadIdx.x; e < tot; e += 256) { const int64_t i = e / t.nc, j = e % t.nc; s += t.a[i * t.lda + j] * t.b[i * t.ldb + j]; }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
// out[outs[o]] = sum of partial[first[o] .. first[o+1]) in piece order
__global__ void __launch_bounds__(256) dot2d_final_kernel(const double* __restrict__ partial, const int32_t* __restrict__ outs, const int32_t* __restrict__ first, int nout, double* __restrict__ out)
{
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= nout) return;
    double s = 0.0;
    for (int q = first[o]; q < first[o + 1]; ++q) s += partial[q];
    out[outs[o]] = s;
}
}  // namespace
}  // namespace dmrgx

extern "C" dmrgx_status dmrgx_dot2d_batch(int32_t count, const dmrgx_dot2d_task* tasks, double* dev_out, void* stream)
{
    if (count < 0 || (count > 0 && (!tasks || !dev_out))) DMRGX_FAIL(DMRGX_ERR_ARG, "dot2d_batch: bad argument");
    if (count == 0) return DMRGX_OK;
    hipStream_t st = (hipStream_t)stream;
    // pieces of at most ~64k elements, grouped by output index (stable: task order inside an output is kept)
    std::vector<int32_t> order(count);
    for (int32_t i = 0; i < count; ++i) {
        const dmrgx_dot2d_task& t = tasks[i];
        if (t.nr < 0 || t.nc < 0 || t.out < 0 || (t.nr && t.nc && (!t.a || !t.b || t.lda < t.nc || t.ldb < t.nc))) DMRGX_FAIL(DMRGX_ERR_ARG, "dot2d_batch: bad task %d", i);
        order[i] = i;
    }
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return tasks[x].out < tasks[y].out; });
    std::vector<dmrgx::Dot2dPiece> pieces;
    std::vector<int32_t> outs, first;
    for (int32_t r = 0; r < count; ++r) {
        const dmrgx_dot2d_task& t = tasks[order[r]];
        if (outs.empty() || outs.back() != t.out) { outs.push_back(t.out); first.push_back((int32_t)pieces.size()); }
        if (t.nr == 0 || t.nc == 0) continue;
        const int32_t rows_per = std::max<int32_t>(1, 65536 / t.nc);
        for (int32_t r0 = 0; r0 < t.nr; r0 += rows_per)
            pieces.push_back(dmrgx::Dot2dPiece{t.a + (int64_t)r0 * t.lda, t.b + (int64_t)r0 * t.ldb, t.lda, t.ldb, std::min(rows_per, t.nr - r0), t.nc});
    }
    first.push_back((int32_t)pieces.size());
    DevBuf tab, dpart;
    DMRGX_CHK(dpart.alloc_f64(std::max<size_t>(pieces.size(), 1), st));
    dmrgx::PackedUpload pk;
    const size_t opc = pk.add(pieces), oo = pk.add(outs), of = pk.add(first);
    DMRGX_CHK(pk.upload(tab, st));
    if (!pieces.empty()) hipLaunchKernelGGL(dmrgx::dot2d_partial_kernel, dim3((unsigned)pieces.size()), dim3(256), 0, st, dmrgx::packed_at<dmrgx::Dot2dPiece>(tab, opc), dpart.as<double>());
    hipLaunchKernelGGL(dmrgx::dot2d_final_kernel, dim3((unsigned)((outs.size() + 255) / 256)), dim3(256), 0, st, (const double*)dpart.as<double>(), (const int32_t*)dmrgx::packed_at<int32_t>(tab, oo), (const int32_t*)dmrgx::packed_at<int32_t>(tab, of),
                       (int)outs.size(), dev_out);
    DMRGX_HIP(hipGetLastError());
    return DMRGX_OK;
}
