// Batched symmetric eigensolver for the reduced density matrices -- see symeig.h.  Three phases, every one of them batched over
// all matrices of a truncation step (the reference hands each block to LAPACK on rank 0, include/DMRGBlockContainer.hpp:1962-2003):
//
//  1. Householder tridiagonalisation  A = Q T Q^T: symeig_trid.hip.
//  2. Tridiagonal divide and conquer: symeig_dc.hip.
//  3. Back-transformation  X = H_0 .. H_{n-3} Z  in blocks of 64 reflectors, compact-WY with T^-1 = striu(V^T V) + diag(1/tau):
//     T V^T is formed for all blocks at once, then two grouped GEMMs per block step.  Here, with the driver of the three:
//     symeig_batched queues 1, 2 and the WY factors of 3; symeig_finish the eigenvector GEMMs of 2's root merge and of 3.
//
// tools/proto_trid_dc.py is the numpy statement of exactly this data flow.
#include "symeig_impl.h"
#include <chrono>

namespace dmrgx {
using namespace symeig_impl;
namespace {
// dst (n x n, ld) = src^T for every matrix (V from V^T)
struct SqPair { const double* src; double* dst; int32_t n, lds, ldd, pad; };
__global__ void __launch_bounds__(256) transpose_sq_kernel(const SqPair* __restrict__ prs)
{
    __shared__ double t[32][33];
    const SqPair p = prs[blockIdx.z];
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    if (r0 >= p.n || c0 >= p.n) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) t[r][tx] = (r0 + r < p.n && c0 + tx < p.n) ? p.src[(int64_t)(r0 + r) * p.lds + c0 + tx] : 0.0;
    __syncthreads();
    for (int r = ty; r < 32; r += 8) if (c0 + r < p.n && r0 + tx < p.n) p.dst[(int64_t)(c0 + r) * p.ldd + r0 + tx] = t[tx][r];
}

// ---------------------------------------------------------------------------------------------------------------------------
// 3. compact-WY factor of a block of reflectors:  Tneg = -(striu(G) + diag(1 / tau))^-1,  G = V_b^T V_b  (64 x 64, row-major)
// ---------------------------------------------------------------------------------------------------------------------------
struct WyBlock { const double* G; const double* tau; double* Tneg; int32_t kb, ld, zero_below, pad; };      // one 64 x 64 diagonal sub-block; G and Tneg with row stride ld;
                                                                                                      // zero_below: rows of the (structurally zero) block under it to clear
__global__ void __launch_bounds__(WY_SUB) wy_tinv_kernel(const WyBlock* __restrict__ blocks)
{
    __shared__ double S[WY_SUB][WY_SUB + 1];          // upper triangle + diagonal: S; strictly lower triangle: T^T (T[r][c] at [c][r])
    const WyBlock b = blocks[blockIdx.x];
    const int c = threadIdx.x, kb = b.kb;
    for (int r = 0; r < WY_SUB; ++r) {
        double v = 0.0;
        if (r < kb && c < kb) {
            if (c > r) v = b.G[(int64_t)r * b.ld + c];
            else if (c == r) { const double t = b.tau[r]; v = t != 0.0 ? 1.0 / t : 1.0; }
        } else if (r == c) v = 1.0;
        if (c >= r) S[r][c] = v;
    }
    __syncthreads();
    // column c of S^-1 by back substitution (S upper triangular): t_c = 1 / S_cc;  t_r = -(sum_{l = r+1 .. c} S_rl t_l) / S_rr.
    // Thread c writes row c of the lower triangle only and reads the upper triangle, which nobody writes: no barrier in the loop.
    const double tcc = 1.0 / S[c][c];
    for (int r = WY_SUB - 2; r >= 0; --r) {
        if (r < c) {
            double acc = S[r][c] * tcc;
            for (int l = r + 1; l < c; ++l) acc += S[r][l] * S[c][l];
            S[c][r] = -acc / S[r][r];
        }
    }
    for (int r = 0; r < kb; ++r) {
        if (c >= kb) break;
        const double t = r < c ? S[c][r] : (r == c ? tcc : 0.0);
        b.Tneg[(int64_t)r * b.ld + c] = -t;
    }
    for (int r = 0; r < b.zero_below; ++r) b.Tneg[(int64_t)(WY_SUB + r) * b.ld + c] = 0.0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------
// Where the factors of every matrix sit in the workspaces of the call, and the sizes of the two (dtot doubles, itot int32)
std::vector<SymEigWs> workspace_layout(const std::vector<SymEigMat>& M, int64_t& dtot, int64_t& itot)
{
    std::vector<SymEigWs> ws(M.size());
    dtot = itot = 0;
    for (size_t i = 0; i < M.size(); ++i) {
        const int64_t n = M[i].n, nn = n * n;
        SymEigWs& w = ws[i];
        w.nblk = (int)((std::max<int64_t>(n - 2, 0) + WY_NB - 1) / WY_NB);
        w.depth = 0;
        while ((n + (1 << w.depth) - 1) / (1 << w.depth) > DC_LEAF) ++w.depth;
        w.VT = dtot; dtot += nn;
        w.Vc = dtot; dtot += nn;
        w.TV = dtot; dtot += nn;
        w.Q1 = dtot; dtot += nn;
        w.U = dtot; dtot += nn;
        w.y = dtot; dtot += 2 * n;
        w.d = dtot; dtot += n; w.e = dtot; dtot += n; w.tau = dtot; dtot += n; w.dcur = dtot; dtot += n;
        w.scale = dtot; dtot += 8;
        w.vecs = dtot; dtot += DC_NVEC * n;
        w.G = dtot; dtot += (int64_t)w.nblk * WY_NB * WY_NB;
        w.Tn = dtot; dtot += (int64_t)w.nblk * WY_NB * WY_NB;
        w.W = dtot; dtot += (int64_t)WY_NB * n;
        w.ints = itot; itot += DC_NINT * n;
    }
    return ws;
}

// 3a (independent of the eigenvectors): V = (V^T)^T, the Gram blocks, T factors and T V^T.  The GEMMs go to `gemms`, their scheduled tile
// lists and the tables of the two kernels above to `pk`.
struct WyTables { GemmSet gram, tv, t12a, t12b; size_t o_tp = 0, o_wyb = 0; unsigned nwyb = 0; };
void wy_add_tables(const std::vector<SymEigMat>& M, const std::vector<SymEigWs>& ws, double* B, GemmBatch& gemms, PackedUpload& pk, WyTables& t)
{
    const int nm = (int)M.size();
    std::vector<SqPair> tp(nm);
    std::vector<WyBlock> wyb;
    for (int i = 0; i < nm; ++i) {
        const int n = M[i].n;
        const SymEigWs& w = ws[i];
        tp[i] = SqPair{B + w.VT, B + w.Vc, n, n, n, 0};
        for (int b = 0; b < w.nblk; ++b) {
            const int b0 = b * WY_NB, kb = std::min(WY_NB, n - 2 - b0), r0 = b0 + 1;      // reflectors b0 .. b0+kb-1 live in rows >= b0+1
            double* G = B + w.G + (int64_t)b * WY_NB * WY_NB;
            double* Tn = B + w.Tn + (int64_t)b * WY_NB * WY_NB;
            gemms.gemm(t.gram, G, WY_NB, kb, kb, B + w.VT + (int64_t)b0 * n + r0, n, B + w.Vc + (int64_t)r0 * n + b0, n, n - r0);      // G = V_b^T V_b
            const int k1 = std::min(kb, WY_SUB), k2 = kb - k1;
            wyb.push_back(WyBlock{G, B + w.tau + b0, Tn, k1, WY_NB, k2, 0});
            if (k2 > 0) {
                wyb.push_back(WyBlock{G + (int64_t)WY_SUB * WY_NB + WY_SUB, B + w.tau + b0 + WY_SUB, Tn + (int64_t)WY_SUB * WY_NB + WY_SUB, k2, WY_NB, 0, 0});
                // Tneg12 = Tneg1 . G12 . Tneg2 (= -T12): P = G12 . Tneg2 parked in the unused lower-left block of G, then Tneg12 = Tneg1 . P
                double* Pm = G + (int64_t)WY_SUB * WY_NB;
                gemms.gemm(t.t12a, Pm, WY_NB, k1, k2, G + WY_SUB, WY_NB, Tn + (int64_t)WY_SUB * WY_NB + WY_SUB, WY_NB, k2);
                gemms.gemm(t.t12b, Tn + WY_SUB, WY_NB, k1, k2, Tn, WY_NB, Pm, WY_NB, k1);
            }
            gemms.gemm(t.tv, B + w.TV + (int64_t)b0 * n, n, kb, n, Tn, WY_NB, B + w.VT + (int64_t)b0 * n, n, kb);     // (T V^T)_b = Tneg_b . V_b^T
        }
    }
    for (GemmSet* s : {&t.t12a, &t.t12b, &t.gram, &t.tv}) gemms.pack(*s, pk);
    t.nwyb = (unsigned)wyb.size();
    if (wyb.empty()) wyb.push_back(WyBlock{nullptr, nullptr, nullptr, 0, 0, 0, 0});
    t.o_tp = pk.add(tp); t.o_wyb = pk.add(wyb);
}

// The WY factors (V^T, Gram matrix, T^-1 by one latency-bound workgroup per block, T12, T V^T) and the divide and conquer both
// need the tridiagonalisation only, and neither fills the chip: the WY chain goes to a second stream, forked from st here; the caller
// makes st wait for `done` in front of the back-transformation (m = 512: ~100 us per call; timeline in profiles/r04_rdm_timeline_m512.txt).
dmrgx_status wy_launch_beside(const WyTables& t, int nm, int nmax, const GemmBatch& gemms, const DevBuf& d_tab, hipStream_t st, hipEvent_t& done)
{
    static thread_local hipStream_t side = nullptr;            // (one per host thread: callers on different threads / devices do not share it)
    static thread_local hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    if (!side) {
        DMRGX_HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
        DMRGX_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
        DMRGX_HIP(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    }
    DMRGX_HIP(hipEventRecord(ev_fork, st));
    DMRGX_HIP(hipStreamWaitEvent(side, ev_fork, 0));
    const unsigned t32 = (unsigned)((nmax + 31) / 32);
    hipLaunchKernelGGL(transpose_sq_kernel, dim3(t32, t32, (unsigned)nm), dim3(256), 0, side, packed_at<SqPair>(d_tab, t.o_tp));
    DMRGX_HIP(hipGetLastError());
    DMRGX_CHK(gemms.launch(t.gram, d_tab, side));
    hipLaunchKernelGGL(wy_tinv_kernel, dim3(t.nwyb), dim3(WY_SUB), 0, side, packed_at<WyBlock>(d_tab, t.o_wyb));
    DMRGX_HIP(hipGetLastError());
    DMRGX_CHK(gemms.launch(t.t12a, d_tab, side));
    DMRGX_CHK(gemms.launch(t.t12b, d_tab, side));
    DMRGX_CHK(gemms.launch(t.tv, d_tab, side));
    DMRGX_HIP(hipEventRecord(ev_join, side));
    done = ev_join;
    return DMRGX_OK;
}
}  // namespace

// First phase (symeig.h).  The device sees the work in the order of this function.
dmrgx_status symeig_batched(const std::vector<SymEigMat>& mats_in, hipStream_t st, SymEigReport& rep, SymEigDeferred& deferred)
{
    rep = SymEigReport();
    deferred.status_host = nullptr;
    std::vector<SymEigMat> M;
    for (const SymEigMat& s : mats_in) {
        if (s.n < 0 || s.n > SYMEIG_MAX_N) DMRGX_FAIL(DMRGX_ERR_ARG, "symeig: matrix of order %d (supported: 0..%d)", s.n, SYMEIG_MAX_N);
        if (s.n > 0 && (!s.A || !s.X || !s.w || s.lda < s.n || s.ldx < s.n)) DMRGX_FAIL(DMRGX_ERR_ARG, "symeig: bad matrix descriptor");
        if (s.n > 0) M.push_back(s);
    }
    const int nm = (int)M.size();
    if (nm == 0) return DMRGX_OK;
    // developer aid (DMRGX_SYMEIG_TRACE): host clock at the milestones of the call, no synchronisation -- where the HOST spends its time
    static const bool host_trace = getenv("DMRGX_SYMEIG_TRACE") != nullptr;
    const auto ht0 = std::chrono::steady_clock::now();
    std::vector<std::pair<const char*, double>> hmarks;
    auto hmark = [&](const char* what) { if (host_trace) hmarks.push_back({what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - ht0).count()}); };

    // ---- workspace -----------------------------------------------------------------------------------------------------
    int64_t dtot = 0, itot = 0;
    const std::vector<SymEigWs> ws = workspace_layout(M, dtot, itot);
    int nmax = 0;
    for (int i = 0; i < nm; ++i) {
        nmax = std::max(nmax, M[i].n);
        rep.merge_levels = std::max(rep.merge_levels, ws[i].depth); rep.wy_blocks_max = std::max(rep.wy_blocks_max, ws[i].nblk);
    }
    DevBuf dbuf, ibuf;
    DMRGX_CHK(dbuf.alloc_f64((size_t)dtot, st));
    DMRGX_CHK(ibuf.alloc((size_t)itot * sizeof(int32_t)));
    double* B = dbuf.as<double>();
    int32_t* I = ibuf.as<int32_t>();
    hmark("workspace");

    // ---- 1. tridiagonalisation: queued before the host builds a single table -- the table building overlaps it ---------------------
    TridRun trid;
    DMRGX_CHK(trid_enqueue(M, ws, B, st, rep, trid));
    hmark("trid launched");

    // ---- the tables of 3a and 2 and every GEMM of the call (a GemmSet per dependent step), in one copy ----------------------------
    GemmBatch gemms;
    gemms.skip_empty_k = true;
    PackedUpload pk;
    WyTables wy;
    DcTables dc;
    wy_add_tables(M, ws, B, gemms, pk, wy);
    dc_add_tables(M, ws, B, I, gemms, pk, dc);
    gemms.pack(pk);
    hmark("tables built");
    DevBuf d_tab;
    DMRGX_CHK(pk.upload(d_tab, st));
    gemms.bind(d_tab);
    hmark("tables uploaded");

    // ---- the persistent rounds have had the table building and the upload to run in; their status word follows them to the caller ----
    DMRGX_CHK(trid_status_to_pinned(trid, st, deferred.status_host));

    // ---- 3a on the side stream, 2 on st, join ---------------------------------------------------------------------------------------
    hipEvent_t wy_done = nullptr;
    if (rep.wy_blocks_max > 0) DMRGX_CHK(wy_launch_beside(wy, nm, nmax, gemms, d_tab, st, wy_done));
    DMRGX_CHK(dc_launch(dc, nm, nmax, gemms, d_tab, st));
    if (wy_done) DMRGX_HIP(hipStreamWaitEvent(st, wy_done, 0));

    // ---- everything symeig_finish needs: the matrices, where their factors sit in the workspace, and the workspace itself ------------
    deferred.mats.clear();
    for (int i = 0; i < nm; ++i) deferred.mats.push_back(SymEigDeferred::Mat{M[i], ws[i]});
    deferred.dbuf.release(); deferred.ibuf.release();
    std::swap(deferred.dbuf.p, dbuf.p); std::swap(deferred.dbuf.bytes, dbuf.bytes);
    std::swap(deferred.ibuf.p, ibuf.p); std::swap(deferred.ibuf.bytes, ibuf.bytes);
    deferred.pending = true;
    hmark("all queued");
    if (host_trace) {
        fprintf(stderr, "[symeig host] %d matrices, nmax %d:", nm, nmax);
        for (const auto& hm : hmarks) fprintf(stderr, "  %s %.0f us", hm.first, hm.second);
        fprintf(stderr, "\n");
    }
    return DMRGX_OK;
}

// Second phase: the root merge's GEMM X[:, kept] = blockdiag(Q_a, Q_b) U[:, kept] and the blocked back-transformation
// X[:, kept] <- H_0 ... H_{n-3} X[:, kept], for the keep[i] largest eigenvalues (the last columns) of every matrix -- half of the flops of
// both, and GEMM launches half as wide, when a truncation keeps half of the states.
dmrgx_status symeig_finish(SymEigDeferred& d, const std::vector<int32_t>& keep, hipStream_t st)
{
    if (!d.pending) return DMRGX_OK;
    const int nm = (int)d.mats.size();
    if ((int)keep.size() != nm) DMRGX_FAIL(DMRGX_ERR_ARG, "symeig_finish: %d counts for %d matrices", (int)keep.size(), nm);
    double* B = d.dbuf.as<double>();
    GemmBatch gemms;
    gemms.skip_empty_k = true;
    int max_nblk = 0;
    GemmSet root;
    for (int i = 0; i < nm; ++i) {
        const SymEigDeferred::Mat& q = d.mats[(size_t)i];
        const int n = q.m.n, c = keep[(size_t)i];
        if (c < 0 || c > n) DMRGX_FAIL(DMRGX_ERR_ARG, "symeig_finish: matrix %d of order %d cannot keep %d eigenvectors", i, n, c);
        if (c > 0) max_nblk = std::max(max_nblk, q.ws.nblk);
        if (q.ws.depth < 1 || c == 0) continue;                  // (a single leaf: its eigenvectors are complete)
        const int mid = tree_bounds(n, 1)[1], c0 = n - c;
        double* X = q.m.X; const int ldx = q.m.ldx;
        const double* Qs = B + q.ws.Q1; const double* U = B + q.ws.U;        // the root's children live in Q[1] (ld n), its merge matrix in U (ld n)
        gemms.gemm(root, X + c0, ldx, mid, c, Qs, n, U + c0, n, mid);
        gemms.gemm(root, X + (int64_t)mid * ldx + c0, ldx, n - mid, c, Qs + (int64_t)mid * n + mid, n, U + (int64_t)mid * n + c0, n, n - mid);
    }
    std::vector<GemmSet> bt_w((size_t)max_nblk), bt_x((size_t)max_nblk);
    for (int s = 0; s < max_nblk; ++s) {
        for (int i = 0; i < nm; ++i) {
            const SymEigDeferred::Mat& q = d.mats[(size_t)i];
            const int b = q.ws.nblk - 1 - s, n = q.m.n, c = keep[(size_t)i];
            if (b < 0 || c == 0) continue;
            const int b0 = b * WY_NB, kb = std::min(WY_NB, n - 2 - b0), r0 = b0 + 1, c0 = n - c;
            double* X = q.m.X; const int ldx = q.m.ldx;
            gemms.gemm(bt_w[(size_t)s], B + q.ws.W, n, kb, c, B + q.ws.TV + (int64_t)b0 * n + r0, n, X + (int64_t)r0 * ldx + c0, ldx, n - r0);      // W = -(T V^T) X[:, kept]
            gemms.gemm(bt_x[(size_t)s], X + (int64_t)r0 * ldx + c0, ldx, n - r0, c, B + q.ws.Vc + (int64_t)r0 * n + b0, n, B + q.ws.W, n, kb, 1);   // X[:, kept] += V W
        }
    }
    if (!gemms.groups.empty()) {
        DevBuf d_tab;
        PackedUpload pk;
        gemms.pack(pk); gemms.pack(root, pk);
        for (int s = 0; s < max_nblk; ++s) { gemms.pack(bt_w[(size_t)s], pk); gemms.pack(bt_x[(size_t)s], pk); }
        DMRGX_CHK(pk.upload(d_tab, st));
        gemms.bind(d_tab);
        DMRGX_CHK(gemms.launch(root, d_tab, st));
        for (int s = 0; s < max_nblk; ++s) { DMRGX_CHK(gemms.launch(bt_w[(size_t)s], d_tab, st)); DMRGX_CHK(gemms.launch(bt_x[(size_t)s], d_tab, st)); }
    }
    // (the tables and the workspace go back to the stream-ordered pool: later users are ordered behind the launches above)
    d.dbuf.release(); d.ibuf.release();
    d.pending = false;
    return DMRGX_OK;
}

}  // namespace dmrgx
