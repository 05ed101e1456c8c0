// K3/K4: reduced density matrices of the superblock ground state and their full eigendecomposition.
//
// Replaces the rank-0 loop of GetTruncation (reference include/DMRGBlockContainer.hpp:1715-1775): for every
// KronBlock k, Psi = n_L x n_R row-major slice of psi (:1731), rho_L = Psi Psi^T, rho_R = Psi^T Psi (:1733-1734),
// then EigRDM_BlockDiag = all eigenpairs of each block by LAPACK (:1962-2003).  Here all 2*nblocks matrices are
// built by ONE launch of the grouped MFMA-f64 GEMM and diagonalised together on the device by the direct solver of
// symeig*.hip (tridiagonalisation, divide and conquer; rdm_solve_direct below): first the spectra, then -- once the
// caller has cut (dmrgx_rdm_select) -- the eigenvectors of the kept states.  A call with a sector above SYMEIG_MAX_N,
// or under DMRGX_RDM_SOLVER=jacobi, goes to the block-Jacobi iteration of rdm_jacobi.hip instead.  Sorting, the
// global m-cut and the stable re-sort by sector (:1795,1850-1853) stay on the host (caller), which fetches spectra
// with dmrgx_rdm_eigenvalues and asks for the kept eigenvectors with dmrgx_rdm_eigenvectors (== FillRotation_BlockDiag,
// :2006-2057).
#include "ggemm.h"
#include "rdm.h"
#include <cmath>
#include <memory>

namespace dmrgx {
namespace {

// A <- 0 on the padding, V <- identity.  Block Jacobi's requirements (the padding stays exactly decoupled there: rotations with
// a_pq == 0 are skipped, so the real eigenvectors are the columns [0,n) of V and the convergence norms only see the real matrix);
// the direct solver overwrites V and never looks at the padding, and is left with both (rdm.h, RDM_PAD)
__global__ void rdm_init_kernel(const MatDesc* __restrict__ mats, double* __restrict__ buf)
{
    const MatDesc m = mats[blockIdx.y];
    const int64_t tot = (int64_t)m.npad * m.npad;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(e / m.npad), j = (int)(e % m.npad);
        buf[m.v_off + e] = (i == j) ? 1.0 : 0.0;
        if (i >= m.n || j >= m.n) buf[m.a_off + e] = 0.0;       // (the second buffer is written whole by the first round)
    }
}

__global__ void __launch_bounds__(256) transpose_kernel(const TrTile* __restrict__ tiles, const double* __restrict__ in, double* __restrict__ out)
{
    __shared__ double t[32][33];
    const TrTile k = tiles[blockIdx.x];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int i = k.ti * 32 + r, j = k.tj * 32 + tx;
        t[r][tx] = (i < k.nr && j < k.nc) ? in[k.src + (int64_t)i * k.nc + j] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int j = k.tj * 32 + r, i = k.ti * 32 + tx;
        if (i < k.nr && j < k.nc) out[k.dst + (int64_t)j * k.nr + i] = t[tx][r];
    }
}

// out[c] = sum_i W[i*ld + c]^2 for c < ncols  (Rayleigh quotients: lambda_c = |Psi^T u_c|^2)
struct ColNormTask { int64_t w_off, out_off; int32_t nrows, ncols, ld, pad; };
__global__ void __launch_bounds__(256) colnorm_kernel(const ColNormTask* __restrict__ tasks, const double* buf, double* out)
{
    __shared__ double part[4][64];
    const ColNormTask t = tasks[blockIdx.y];
    const int c0 = blockIdx.x * 64;
    if (c0 >= t.ncols) return;
    const int col = c0 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
    double s = 0.0;
    if (col < t.ncols) for (int i = rg; i < t.nrows; i += 4) { const double v = buf[t.w_off + (int64_t)i * t.ld + col]; s += v * v; }
    part[rg][threadIdx.x & 63] = s;
    __syncthreads();
    if (rg == 0 && col < t.ncols) out[t.out_off + col] = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

// dst[r*ld + i] = V[i*npad + perm[r]]
__global__ void gather_vec_kernel(const double* __restrict__ V, int npad, int n, const int32_t* __restrict__ perm, int count, double* __restrict__ dst, int64_t ld)
{
    const int r = blockIdx.y;
    if (r >= count) return;
    const int col = perm[r];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[(int64_t)r * ld + i] = V[(int64_t)i * npad + col];
}

// the same for up to GATHER_MAX (matrix, destination) pairs in one launch; the descriptors travel in the kernel-argument segment
constexpr int GATHER_MAX = 48;
struct GatherOne { const double* V; const int32_t* perm; double* dst; int64_t ld; int32_t npad, n, count, pad; };
struct GatherArgs { GatherOne t[GATHER_MAX]; };
__global__ void gather_vec_batch_kernel(const GatherArgs a)
{
    const GatherOne g = a.t[blockIdx.z];
    for (int r = blockIdx.y; r < g.count; r += gridDim.y) {
        const int col = g.perm[r];
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += gridDim.x * blockDim.x) g.dst[(int64_t)r * g.ld + i] = g.V[(int64_t)i * g.npad + col];
    }
}

}  // namespace

bool rdm_trace() { static const bool on = getenv("DMRGX_RDM_TRACE") != nullptr; return on; }
void RdmStageClock::operator()(const char* name)
{
    if (!rdm_trace()) return;
    (void)hipStreamSynchronize(st);
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "[rdm] stage %-10s %8.3f ms\n", name, std::chrono::duration<double, std::milli>(t - t_prev).count());
    t_prev = t;
}

void rdm_transpose(const TrTile* d_tiles, size_t count, const double* in, double* out, hipStream_t st)
{
    if (count) hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)count), dim3(256), 0, st, d_tiles, in, out);
}

}  // namespace dmrgx

using namespace dmrgx;

// Pinned host blocks for those read-backs, recycled per host thread (hipHostMalloc / hipHostFree per truncation would cost more than the
// synchronisation they replace).
namespace {
struct PinnedCache { std::vector<std::pair<double*, size_t>> free; };      // (never freed: a thread-exit hipHostFree can run after the runtime's own teardown)
PinnedCache& pinned_cache() { static thread_local PinnedCache c; return c; }
double* pinned_take(size_t count, size_t* cap)
{
    auto& f = pinned_cache().free;
    for (size_t i = 0; i < f.size(); ++i) if (f[i].second >= count) { double* p = f[i].first; *cap = f[i].second; f.erase(f.begin() + (std::ptrdiff_t)i); return p; }
    double* p = nullptr;
    const size_t n = std::max<size_t>(count + count / 4, 4096);
    if (hipHostMalloc((void**)&p, n * sizeof(double), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    *cap = n;
    return p;
}
}  // namespace
dmrgx_rdm::~dmrgx_rdm()
{
    if (rq_host) pinned_cache().free.push_back({rq_host, rq_cap});
    if (check_event) (void)hipEventDestroy(check_event);
}

// The direct solver on the Gram matrices, first phase: the spectra are final (secular equations of the divide and conquer), ascending per
// matrix; the eigenvectors are formed by dmrgx_rdm_select for the states the caller keeps (or for all of them at the first request).
dmrgx_status dmrgx::rdm_solve_direct(dmrgx_rdm& P, hipStream_t st)
{
    const int nm = (int)P.mats.size();
    double* buf = P.buf.as<double>();
    std::vector<SymEigMat> sm;
    for (int mi = 0; mi < nm; ++mi) {
        const MatDesc& m = P.mats[mi];
        if (m.n > 0) sm.push_back(SymEigMat{m.n, m.npad, m.npad, 0, buf + m.a_off, buf + m.v_off, buf + P.ew_base + (P.diag_off[mi] - P.diag_base)});
    }
    DMRGX_CHK(symeig_batched(sm, st, P.symeig, P.deferred));
    P.stage("symeig");
    std::vector<double> ew((size_t)P.dtot);
    if (!ew.empty()) DMRGX_HIP(hipMemcpyAsync(ew.data(), buf + P.ew_base, ew.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    DMRGX_HIP(hipStreamSynchronize(st));
    if (const int32_t bad = symeig_deferred_timed_out(P.deferred)) {
        // the persistent tridiagonalisation did not get its partners: everything queued behind it ran on garbage.  Once more, by launches
        // (the density matrices themselves were only read).
        symeig_note_timeout(bad);
        P.deferred.dbuf.release(); P.deferred.ibuf.release(); P.deferred.pending = false;
        DMRGX_CHK(symeig_batched(sm, st, P.symeig, P.deferred));
        P.symeig.timed_out = bad;
        if (!ew.empty()) DMRGX_HIP(hipMemcpyAsync(ew.data(), buf + P.ew_base, ew.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        DMRGX_HIP(hipStreamSynchronize(st));
        if (symeig_deferred_timed_out(P.deferred)) DMRGX_FAIL(DMRGX_ERR_INTERNAL, "rdm_create: the tridiagonalisation by launches reported a persistent-kernel status");
    }
    std::vector<int32_t> allperm;
    for (int mi = 0; mi < nm; ++mi) {
        const MatDesc& m = P.mats[mi];
        const double* a = ew.data() + (P.diag_off[mi] - P.diag_base);
        P.eig[mi].resize(m.n); P.perm[mi].resize(m.n);
        for (int32_t r = 0; r < m.n; ++r) {
            const double v = a[m.n - 1 - r];
            if (!(v == v)) DMRGX_FAIL(DMRGX_ERR_NOTCONV, "rdm_create: density matrix %d (n = %d): the direct solver returned NaN", mi, m.n);
            P.eig[mi][r] = v; P.perm[mi][r] = m.n - 1 - r;      // r-th largest eigenvalue = column n - 1 - r
        }
        P.perm_off[mi] = (int64_t)allperm.size();
        allperm.insert(allperm.end(), P.perm[mi].begin(), P.perm[mi].end());
    }
    DMRGX_CHK(upload(P.d_perm, allperm, st));
    P.stage("spectra");
    return DMRGX_OK;
}

// side_mask == NULL: every matrix.  Layout of the shared regions, Psi^T and the Gram matrices, then one of the two solvers.
static dmrgx_status rdm_create_impl(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks, const int32_t* block_il,
                                    const int32_t* block_ir, const double* psi_dev, const uint8_t* side_mask, void* stream, dmrgx_rdm** out)
{
    hipStream_t st = (hipStream_t)stream;
    if (!left || !right || !block_il || !block_ir || !psi_dev || !out || nblocks <= 0) DMRGX_FAIL(DMRGX_ERR_ARG, "rdm_create: bad argument");
    *out = nullptr;
    std::unique_ptr<dmrgx_rdm> P(new (std::nothrow) dmrgx_rdm());
    if (!P) DMRGX_FAIL(DMRGX_ERR_MEM, "out of host memory");
    P->nblocks = nblocks; P->stage.st = st;
    // ---- solver: the direct one unless DMRGX_RDM_SOLVER=jacobi (process-wide; kept for comparison) or a sector is above SYMEIG_MAX_N
    static const bool want_dc = !(getenv("DMRGX_RDM_SOLVER") && std::string(getenv("DMRGX_RDM_SOLVER")) == "jacobi");
    bool use_dc = want_dc;
    // ---- layout of the regions both solvers see (dmrgx_rdm::buf in rdm.h) ---------------------------------------------------------
    int64_t total = 0;
    P->off.assign((size_t)nblocks + 1, 0);
    for (int32_t k = 0; k < nblocks; ++k) {
        const int32_t il = block_il[k], ir = block_ir[k];
        if (il < 0 || il >= left->nsec || ir < 0 || ir >= right->nsec) DMRGX_FAIL(DMRGX_ERR_OUTOFRANGE, "rdm_create: KronBlock %d out of range", k);
        const int32_t nl = left->size[il], nr = right->size[ir];
        if (std::max(nl, nr) > SYMEIG_MAX_N) use_dc = false;
        P->nl.push_back(nl); P->nr.push_back(nr);
        P->off[k + 1] = P->off[k] + (int64_t)nl * nr;
        for (int side = 0; side < 2; ++side) {
            MatDesc m{};                                      // (a2_off: rdm_jacobi.hip)
            const bool sel = !side_mask || ((side_mask[k] >> side) & 1);
            P->selected.push_back(sel ? 1 : 0);
            m.n = !sel ? 0 : side == 0 ? nl : nr;             // a matrix left to another rank is an empty matrix here
            m.npad = ((m.n + RDM_PAD - 1) / RDM_PAD) * RDM_PAD;
            m.nb = m.npad / DMRGX_JB;
            m.a_off = total; total += (int64_t)m.npad * m.npad;
            m.v_off = total; total += (int64_t)m.npad * m.npad;
            P->mats.push_back(m);
        }
    }
    const int64_t N = P->off[nblocks];
    P->solver = use_dc ? 0 : 1;
    const int nm = (int)P->mats.size();
    P->psiT_off = total; total += N;
    for (int mi = 0; mi < nm; ++mi) { P->diag_off.push_back(P->dtot); P->dtot += P->mats[mi].npad; }
    P->diag_base = total; total += P->dtot;
    P->rq_base = total; total += P->dtot;          // Rayleigh quotients, same indexing as the diagonals
    P->w_base = total; total += 2 * N;             // W = Psi^T V_L (n_R x n_L) and Psi V_R (n_L x n_R) per block
    P->ew_base = total; total += use_dc ? P->dtot : 0;   // eigenvalues as the direct solver returns them (ascending)
    for (auto& v : P->diag_off) v += P->diag_base;
    P->psi = psi_dev;
    P->eig.resize(nm); P->perm.resize(nm); P->perm_off.resize(nm); P->have.assign((size_t)nm, 0);
    DMRGX_CHK(P->buf.alloc_f64((size_t)total, st));
    double* buf = P->buf.as<double>();
    // ---- tables of the set-up (matrix descriptors, transposition tiles, the Gram GEMMs) in ONE upload ----------------------------------
    std::vector<TrTile> tt;
    GemmBatch gram;
    GemmSet gram_set;
    for (int32_t k = 0; k < nblocks; ++k) {
        const int32_t nl = P->nl[k], nr = P->nr[k];
        const double* Psi = psi_dev + P->off[k];
        const double* PsiT = buf + P->psiT_off + P->off[k];
        const MatDesc& mL = P->mats[2 * k];
        const MatDesc& mR = P->mats[2 * k + 1];
        if (P->selected[2 * k] || P->selected[2 * k + 1])
            for (int ti = 0; ti < (nl + 31) / 32; ++ti) for (int tj = 0; tj < (nr + 31) / 32; ++tj) tt.push_back(TrTile{P->off[k], P->psiT_off + P->off[k], nl, nr, ti, tj});
        if (P->selected[2 * k]) gram.gemm(gram_set, buf + mL.a_off, mL.npad, nl, nl, Psi, nr, PsiT, nl, nr);             // rho_L = Psi Psi^T  (:1733)
        if (P->selected[2 * k + 1]) gram.gemm(gram_set, buf + mR.a_off, mR.npad, nr, nr, PsiT, nl, Psi, nr, nl);         // rho_R = Psi^T Psi  (:1734)
    }
    PackedUpload pk;
    const size_t o_m = pk.add(P->mats), o_tt = pk.add(tt);
    gram.pack(pk); gram.pack(gram_set, pk);
    DMRGX_CHK(pk.upload(P->d_tables, st));
    gram.bind(P->d_tables);
    PackedUpload::view<MatDesc>(P->d_mats, P->d_tables, o_m, P->mats.size());
    hipLaunchKernelGGL(rdm_init_kernel, dim3(64, nm), dim3(256), 0, st, (const MatDesc*)P->d_mats.as<MatDesc>(), buf);
    DMRGX_HIP(hipGetLastError());
    P->stage("layout");
    // ---- Psi^T (read from psi, the caller's memory: distinct base pointers) and the 2*nblocks Gram matrices in one grouped GEMM launch
    rdm_transpose(packed_at<TrTile>(P->d_tables, o_tt), tt.size(), psi_dev, buf, st);
    DMRGX_HIP(hipGetLastError());
    DMRGX_CHK(gram.launch(gram_set, P->d_tables, st));
    P->stage("gram");
    DMRGX_CHK(use_dc ? rdm_solve_direct(*P, st) : rdm_solve_jacobi(*P, st));
    *out = P.release();
    return DMRGX_OK;
}

extern "C" dmrgx_status dmrgx_rdm_create(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks, const int32_t* block_il,
                                         const int32_t* block_ir, const double* psi_dev, void* stream, dmrgx_rdm** out)
{
    return rdm_create_impl(left, right, nblocks, block_il, block_ir, psi_dev, nullptr, stream, out);
}

// the hint is accepted for compatibility and never dereferenced (include/dmrgx.h)
extern "C" dmrgx_status dmrgx_rdm_create_warm(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks, const int32_t* block_il,
                                              const int32_t* block_ir, const double* psi_dev, const double* const* v0_rows, void* stream, dmrgx_rdm** out)
{
    return rdm_create_impl(left, right, nblocks, block_il, block_ir, psi_dev, nullptr, stream, out);
}

extern "C" dmrgx_status dmrgx_rdm_create_subset(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks, const int32_t* block_il,
                                                const int32_t* block_ir, const double* psi_dev, const uint8_t* side_mask, void* stream, dmrgx_rdm** out)
{
    if (!side_mask) DMRGX_FAIL(DMRGX_ERR_ARG, "rdm_create_subset: null side_mask");
    return rdm_create_impl(left, right, nblocks, block_il, block_ir, psi_dev, side_mask, stream, out);
}

// Eigenvalues as Rayleigh quotients of the finished eigenvectors: lambda = |Psi^T u|^2 (rho_L) / |Psi v|^2 (rho_R).  Relative accuracy ~eps
// instead of the c*n*eps*||rho|| of a rotated diagonal / a secular root, which matters for TruncErr = 1 - sum of kept eigenvalues
// (include/DMRGBlockContainer.hpp:1872-1875).  Who cuts on what: the block-Jacobi solver evaluates all columns and these quotients ARE the
// spectrum the caller cuts on (rdm_jacobi.hip); with the direct solver the caller has already cut on the D&C eigenvalues, and the quotients
// of the kept columns -- the last cols[mi] -- are only the independent check of rdm_verify.
dmrgx_status dmrgx::rdm_rayleigh_enqueue(dmrgx_rdm& P, const std::vector<int32_t>& cols, hipStream_t st, bool* any)
{
    double* buf = P.buf.as<double>();
    GemmBatch wgemm;                                // W = Psi^T V_L, Psi V_R
    GemmSet wset;
    std::vector<ColNormTask> cn;
    for (int32_t k = 0; k < P.nblocks; ++k) {
        const int32_t nl = P.nl[(size_t)k], nr = P.nr[(size_t)k];
        const double* Psi = P.psi + P.off[(size_t)k];
        const double* PsiT = buf + P.psiT_off + P.off[(size_t)k];
        for (int side = 0; side < 2; ++side) {             // W_L = Psi^T V_L: n_R x (columns of V_L), then W_R = Psi V_R: n_L x (columns of V_R)
            const size_t mi = (size_t)(2 * k + side);
            const MatDesc& m = P.mats[mi];
            const int32_t n = side ? nr : nl, rows = side ? nl : nr, c = P.selected[mi] ? cols[mi] : 0, c0 = n - c;
            if (c <= 0) continue;
            const int64_t w_off = P.w_base + 2 * P.off[(size_t)k] + (side ? (int64_t)nl * nr : 0);
            wgemm.gemm(wset, buf + w_off, c, rows, c, side ? Psi : PsiT, n, buf + m.v_off + c0, m.npad, n);
            cn.push_back(ColNormTask{w_off, P.rq_base + (P.diag_off[mi] - P.diag_base) + c0, rows, c, c, 0});
        }
    }
    *any = !cn.empty();
    if (cn.empty()) return DMRGX_OK;                    // (nothing selected on this rank)
    DevBuf dtab;
    PackedUpload pk;
    wgemm.pack(pk); wgemm.pack(wset, pk);
    const size_t o_c = pk.add(cn);
    DMRGX_CHK(pk.upload(dtab, st));
    wgemm.bind(dtab);
    DMRGX_HIP(zero_async(buf + P.rq_base, (size_t)P.dtot * sizeof(double), st));
    DMRGX_CHK(wgemm.launch(wset, dtab, st));
    int maxc = 1;
    for (auto& c : cn) maxc = std::max(maxc, c.ncols);
    hipLaunchKernelGGL(colnorm_kernel, dim3((maxc + 63) / 64, (unsigned)cn.size()), dim3(256), 0, st, (const ColNormTask*)packed_at<ColNormTask>(dtab, o_c), (const double*)buf, buf);
    DMRGX_HIP(hipGetLastError());
    return DMRGX_OK;
}

// counts == NULL: every eigenvector of every matrix
static dmrgx_status rdm_select_impl(dmrgx_rdm* R, const int32_t* counts, hipStream_t st)
{
    if (!R->deferred.pending) return DMRGX_OK;
    const int nm = (int)R->mats.size();
    std::vector<int32_t> cols((size_t)nm, 0), keep;
    for (int mi = 0; mi < nm; ++mi) {
        const int32_t n = R->mats[mi].n;
        if (n <= 0) continue;
        const int32_t c = counts ? counts[mi] : n;
        if (c < 0 || c > n) DMRGX_FAIL(DMRGX_ERR_ARG, "rdm_select: matrix (block %d, side %d) of order %d cannot keep %d states", mi / 2, mi % 2, n, c);
        cols[(size_t)mi] = c;
        keep.push_back(c);                               // (the direct solver saw the matrices of order > 0, in this order)
    }
    DMRGX_CHK(symeig_finish(R->deferred, keep, st));
    // The Rayleigh quotients of the finished columns are the second, independent route to the kept eigenvalues -- compared when the object
    // is destroyed, after the caller's own synchronisation (dmrgx_rdm_destroy returns DMRGX_ERR_NOTCONV on a mismatch).  Nothing waits here.
    bool any = false;
    DMRGX_CHK(rdm_rayleigh_enqueue(*R, cols, st, &any));
    if (!any) return DMRGX_OK;
    if (!R->rq_host) R->rq_host = pinned_take((size_t)R->dtot, &R->rq_cap);
    if (!R->rq_host) DMRGX_FAIL(DMRGX_ERR_MEM, "rdm_select: no pinned host memory for the verification read-back");
    DMRGX_HIP(hipMemcpyAsync(R->rq_host, R->buf.as<double>() + R->rq_base, (size_t)R->dtot * sizeof(double), hipMemcpyDeviceToHost, st));
    if (!R->check_event) DMRGX_HIP(hipEventCreateWithFlags(&R->check_event, hipEventDisableTiming));
    DMRGX_HIP(hipEventRecord(R->check_event, st));
    R->check_cols = cols; R->check_pending = true;
    for (int mi = 0; mi < nm; ++mi) if (R->selected[mi] && R->mats[mi].n > 0) R->have[(size_t)mi] = cols[(size_t)mi];
    return DMRGX_OK;
}

extern "C" dmrgx_status dmrgx_rdm_select(dmrgx_rdm* R, const int32_t* counts, void* stream)
{
    if (!R) DMRGX_FAIL(DMRGX_ERR_ARG, "rdm_select: bad argument");
    if (!R->deferred.pending && R->solver == 0 && counts) {
        // a second selection can only narrow what the first one formed
        for (size_t mi = 0; mi < R->mats.size(); ++mi)
            if (R->selected[mi] && R->mats[mi].n > 0 && counts[mi] > R->have[mi])
                DMRGX_FAIL(DMRGX_ERR_ARG, "rdm_select: the eigenvectors of matrix (block %d, side %d) were formed for %d states, %d asked", (int)mi / 2, (int)mi % 2, R->have[mi], counts[mi]);
    }
    return rdm_select_impl(R, counts, (hipStream_t)stream);
}

extern "C" dmrgx_status dmrgx_rdm_eigenvalues(const dmrgx_rdm* R, int32_t side, int32_t k, double* host_out)
{
    if (!R || !host_out || side < 0 || side > 1 || k < 0 || k >= R->nblocks) DMRGX_FAIL(DMRGX_ERR_ARG, "rdm_eigenvalues: bad argument");
    if (!R->selected[2 * k + side]) DMRGX_FAIL(DMRGX_ERR_ARG, "rdm_eigenvalues: the density matrix (block %d, side %d) was left to another rank", k, side);
    const auto& e = R->eig[2 * k + side];
    std::copy(e.begin(), e.end(), host_out);
    return DMRGX_OK;
}

extern "C" dmrgx_status dmrgx_rdm_eigenvectors(const dmrgx_rdm* R, int32_t side, int32_t k, int32_t count, double* dst_dev, int64_t ld, void* stream)
{
    if (!R || side < 0 || side > 1 || k < 0 || k >= R->nblocks || count < 0) DMRGX_FAIL(DMRGX_ERR_ARG, "rdm_eigenvectors: bad argument");
    const int mi = 2 * k + side;
    if (!R->selected[mi]) DMRGX_FAIL(DMRGX_ERR_ARG, "rdm_eigenvectors: the density matrix (block %d, side %d) was left to another rank", k, side);
    const MatDesc& m = R->mats[mi];
    if (count > m.n || (count > 0 && (!dst_dev || ld < m.n))) DMRGX_FAIL(DMRGX_ERR_ARG, "rdm_eigenvectors: count %d > n %d or bad destination", count, m.n);
    if (count == 0) return DMRGX_OK;
    // (a caller that never selected gets every eigenvector, formed at its first request: the one-phase behaviour)
    if (R->deferred.pending) DMRGX_CHK(rdm_select_impl(const_cast<dmrgx_rdm*>(R), nullptr, (hipStream_t)stream));
    if (count > R->have[(size_t)mi]) DMRGX_FAIL(DMRGX_ERR_ARG, "rdm_eigenvectors: %d eigenvectors asked of (block %d, side %d), dmrgx_rdm_select formed %d", count, k, side, R->have[(size_t)mi]);
    hipLaunchKernelGGL(gather_vec_kernel, dim3((m.n + 255) / 256, count), dim3(256), 0, (hipStream_t)stream,
                       R->buf.as<double>() + m.v_off, m.npad, m.n, R->d_perm.as<int32_t>() + R->perm_off[mi], count, dst_dev, ld);
    DMRGX_HIP(hipGetLastError());
    return DMRGX_OK;
}

extern "C" dmrgx_status dmrgx_rdm_eigenvectors_batch(const dmrgx_rdm* R, int32_t ntasks, const dmrgx_rdm_vec_task* tasks, void* stream)
{
    if (!R || ntasks < 0 || (ntasks > 0 && !tasks)) DMRGX_FAIL(DMRGX_ERR_ARG, "rdm_eigenvectors_batch: bad argument");
    hipStream_t st = (hipStream_t)stream;
    for (int32_t t = 0; t < ntasks; ++t) {
        const dmrgx_rdm_vec_task& q = tasks[t];
        if (q.side < 0 || q.side > 1 || q.k < 0 || q.k >= R->nblocks || q.count < 0) DMRGX_FAIL(DMRGX_ERR_ARG, "rdm_eigenvectors_batch: task %d: bad argument", t);
        const int mi = 2 * q.k + q.side;
        if (!R->selected[mi]) DMRGX_FAIL(DMRGX_ERR_ARG, "rdm_eigenvectors_batch: the density matrix (block %d, side %d) was left to another rank", q.k, q.side);
        const MatDesc& m = R->mats[mi];
        if (q.count > m.n || (q.count > 0 && (!q.dst_dev || q.ld < m.n))) DMRGX_FAIL(DMRGX_ERR_ARG, "rdm_eigenvectors_batch: task %d: count %d > n %d or bad destination", t, q.count, m.n);
    }
    if (R->deferred.pending) DMRGX_CHK(rdm_select_impl(const_cast<dmrgx_rdm*>(R), nullptr, st));
    for (int32_t t0 = 0; t0 < ntasks; t0 += GATHER_MAX) {
        GatherArgs a;
        int na = 0, nmax = 1, cmax = 1;
        for (int32_t t = t0; t < std::min(ntasks, t0 + GATHER_MAX); ++t) {
            const dmrgx_rdm_vec_task& q = tasks[t];
            const int mi = 2 * q.k + q.side;
            const MatDesc& m = R->mats[mi];
            if (q.count == 0) continue;
            if (q.count > R->have[(size_t)mi]) DMRGX_FAIL(DMRGX_ERR_ARG, "rdm_eigenvectors_batch: %d eigenvectors asked of (block %d, side %d), dmrgx_rdm_select formed %d", q.count, q.k, q.side, R->have[(size_t)mi]);
            a.t[na++] = GatherOne{R->buf.as<double>() + m.v_off, R->d_perm.as<int32_t>() + R->perm_off[mi], q.dst_dev, q.ld, m.npad, m.n, q.count, 0};
            nmax = std::max(nmax, m.n); cmax = std::max(cmax, q.count);
        }
        if (na == 0) continue;
        hipLaunchKernelGGL(gather_vec_batch_kernel, dim3((unsigned)((nmax + 255) / 256), (unsigned)std::min(cmax, 4096), (unsigned)na), dim3(256), 0, st, a);
        DMRGX_HIP(hipGetLastError());
    }
    return DMRGX_OK;
}

extern "C" dmrgx_status dmrgx_rdm_info(const dmrgx_rdm* R, dmrgx_rdm_report* out)
{
    if (!R || !out) DMRGX_FAIL(DMRGX_ERR_ARG, "rdm_info: bad argument");
    memset(out, 0, sizeof(*out));
    out->n_sweeps = R->sweeps;
    out->solver = R->solver;
    out->trid_persistent_matrices = R->symeig.persistent_matrices;
    out->trid_launch_matrices = R->symeig.launch_matrices;
    out->max_workgroups_per_matrix = R->symeig.max_workgroups_per_matrix;
    out->merge_levels = R->symeig.merge_levels;
    out->wy_blocks_max = R->symeig.wy_blocks_max;
    out->timed_out = R->symeig.timed_out;
    symeig_process_state(&out->process_timeouts, &out->persistent_off);
    return DMRGX_OK;
}

// Two independent routes to every kept eigenvalue: the secular equations of the divide and conquer (what the caller cut on) and the Rayleigh
// quotient |Psi^T u|^2 of the finished eigenvector.  They agree to round-off; a failed leaf or secular solve (a wrong root) or a broken
// eigenvector shows here instead of as a wrong truncation further down -- the counterpart of the reference's "all eigenpairs
// converged" check (include/DMRGBlockContainer.hpp:1987).
static dmrgx_status rdm_verify(dmrgx_rdm* R)
{
    if (!R->check_pending) return DMRGX_OK;
    R->check_pending = false;
    DMRGX_HIP(hipEventSynchronize(R->check_event));      // (only the read-back: work queued on the stream since is not waited for)
    for (size_t mi = 0; mi < R->mats.size(); ++mi) {
        const MatDesc& m = R->mats[mi];
        const int32_t c = R->selected[mi] ? R->check_cols[mi] : 0;
        if (m.n <= 0 || c <= 0) continue;
        const double* b = R->rq_host + (R->diag_off[mi] - R->diag_base);
        const double scale = std::fabs(R->eig[mi][0]);
        double worst = 0.0;
        bool bad = false;
        for (int32_t r = 0; r < c; ++r) { const double d = std::fabs(R->eig[mi][r] - b[m.n - 1 - r]); if (!(d <= worst)) worst = d; if (!(d == d)) bad = true; }
        if (bad || !(worst <= 1e-8 * scale + 1e-300))
            DMRGX_FAIL(DMRGX_ERR_NOTCONV, "rdm: density matrix (block %d, side %d, n = %d): the direct solver's eigenvalues and the Rayleigh quotients of its vectors differ by %.3e (largest eigenvalue %.3e)",
                       (int)mi / 2, (int)mi % 2, m.n, worst, scale);
    }
    return DMRGX_OK;
}

extern "C" dmrgx_status dmrgx_rdm_destroy(dmrgx_rdm* R)
{
    if (!R) return DMRGX_OK;
    // The verification of the selected eigenpairs is read here: it waits for the event behind its read-back only -- a caller that destroys the
    // object one step later (the engine does) never waits at all; the blocks go back to the pool and are recycled in stream order (pool.hip)
    const dmrgx_status rc = rdm_verify(R);
    delete R;
    return rc;
}
