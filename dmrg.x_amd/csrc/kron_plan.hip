// K1: matrix-free superblock Hamiltonian apply  y = H_sb x  on the target-Sz sector.
//
// Replaces KronSumConstructShell + MatMult_KronSumShell (reference src/DMRGKron.cpp:1706-1917).  The reference
// evaluates, for every row, sum_t a_t sum_l sum_r A_t[l,l'] B_t[r,r'] x[..] (unfactored, :1844-1864).  Here the
// same operator is applied in factored, operator-merged form per KronBlock k=(IL,IR):
//
//     Y_k = H_L[IL] X_k  +  X_k H_R[IR]^T  +  sum_g  Abar_g[IL->IL'] ( X_k' Bhat_g[IR->IR']^T )
//
// where g runs over groups of terms sharing one operator on one side (the side with fewer distinct operators),
// the other side's operators being pre-summed with their coefficients (Abar_g = sum_t a_t A_t) at plan time.
// Stage 1 computes T_{g,k} = X_k' Bhat^T, stage 2 accumulates all groups into Y_k; both stages are ONE launch
// each of the grouped MFMA-f64 GEMM (ggemm.hip) over host-built task tables, with operator zero-cells skipped
// and identity cells (new-site operators) turned into scaled copies.  X_k is the row-major n_L x n_R matrix at
// the KronBlock offset (reference include/DMRGKron.hpp:198-209, 603-612).
//
// Multi-GPU: the right index of every KronBlock is split into world_size contiguous stripes; rank r owns
// column stripe r of every Y_k.  A full vector is stored rank-major (segment r = all stripes of rank r), so one
// RCCL all-gather of equal-sized segments rebuilds x for the next apply.
#include "ggemm.h"
#include <algorithm>
#include <map>
#include <set>
#include <tuple>
#include <cstdlib>
#include <memory>
#include <new>

namespace dmrgx {

namespace {

struct NCell {              // normalised operator cell (transpose folded in)
    int32_t q, r0, c0, nr, nc, kind;
    double scale;
    const double* data;     // caller's device memory (only read during plan creation)
    int64_t ld;
    bool tr;                // element (i,j) of the cell is data[j*ld + i]
};

struct PCell {              // plan-owned cell: dense data lives in the arena at `off` (row-major, ld = nc)
    int32_t q, r0, c0, nr, nc, kind;
    double scale;
    int64_t off;
};

struct CopyTask {           // dst[i*ldd + j] = (round 0) / += (later rounds) a * src(i,j): every contribution covers its whole destination cell
    int64_t dst_off;        // arena element offset
    const double* src;
    int64_t lds;
    int32_t nr, nc, ldd, tr;
    double a;
    int32_t round;          // contributions to the same destination are applied in separate launches
};

struct CopyTile { int32_t task, ti, tj, pad; };

// The column segments of the intermediates T_{g,k} that no right-operator cell reaches are read by stage 2 as zeros: they are the only part of
// the arena that is zeroed (round 5; rounds 1-4 zeroed the whole arena -- 1.4 GB at m = 2048 -- and added every operator into it)
// (one rectangle per blockIdx.x, its chunks over blockIdx.y: a plan can hold far more rectangles than the grid's y limit of 65535)
struct ZeroRect { int64_t off; int32_t ld, nr, nc, pad; };
__global__ void __launch_bounds__(256) zero_rects_kernel(const ZeroRect* __restrict__ rects, double* __restrict__ arena)
{
    const ZeroRect r = rects[blockIdx.x];
    const int64_t n = (int64_t)r.nr * r.nc;
    for (int64_t e = (int64_t)blockIdx.y * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.y * 256) arena[r.off + (e / r.nc) * r.ld + e % r.nc] = 0.0;
}

__global__ void __launch_bounds__(256)
cell_copy_kernel(const CopyTile* __restrict__ tiles, const CopyTask* __restrict__ tasks, double* __restrict__ arena)
{
    __shared__ double buf[32][33];
    const CopyTile t = tiles[blockIdx.x];
    const CopyTask k = tasks[t.task];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const int i0 = t.ti * 32, j0 = t.tj * 32;
    double* dst = arena + k.dst_off;
    if (!k.tr) {
        for (int r = ty; r < 32; r += 8) {
            const int i = i0 + r, j = j0 + tx;
            if (i < k.nr && j < k.nc) { const double v = k.a * k.src[(size_t)i * k.lds + j]; double& o = dst[(size_t)i * k.ldd + j]; o = k.round == 0 ? v : o + v; }
        }
    } else {
        // dst(i,j) = src[j*lds + i]: read coalesced along i, transpose through LDS
        for (int r = ty; r < 32; r += 8) {
            const int j = j0 + r, i = i0 + tx;
            buf[r][tx] = (i < k.nr && j < k.nc) ? k.src[(size_t)j * k.lds + i] : 0.0;
        }
        __syncthreads();
        for (int r = ty; r < 32; r += 8) {
            const int i = i0 + r, j = j0 + tx;
            if (i < k.nr && j < k.nc) { const double v = k.a * buf[tx][r]; double& o = dst[(size_t)i * k.ldd + j]; o = k.round == 0 ? v : o + v; }
        }
    }
}

// striped <-> reference vector layout
struct LayoutSeg { int64_t ref_off, full_off; int32_t nrow, ncol, ref_ld, full_ld; };
__global__ void layout_copy_kernel(const LayoutSeg* __restrict__ segs, const double* __restrict__ src, double* __restrict__ dst, int to_striped)
{
    const LayoutSeg s = segs[blockIdx.y];
    const int64_t n = (int64_t)s.nrow * s.ncol;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / s.ncol, j = e % s.ncol;
        const int64_t a = s.ref_off + i * s.ref_ld + j, b = s.full_off + i * s.full_ld + j;
        if (to_striped) dst[b] = src[a]; else dst[a] = src[b];
    }
}

// Split-K fix-up: for every split output block, y_block += slab_0 + slab_1 + ... in fixed order (bit-reproducible,
// no atomics).  Slabs are compact M x N copies (ld = N) stored back to back in the arena.
struct RedTask { int64_t dst_off, slab_off; int32_t ldc, M, N, nslab; };
struct RedTile { int32_t task, chunk; };
constexpr int RED_CHUNK = 2048;
__global__ __launch_bounds__(256) void slab_reduce_kernel(const RedTile* __restrict__ tiles, const RedTask* __restrict__ tasks,
                                                          double* __restrict__ y, const double* __restrict__ arena)
{
    const RedTile t = tiles[blockIdx.x];
    const RedTask k = tasks[t.task];
    const uint32_t mn = (uint32_t)k.M * (uint32_t)k.N, N = (uint32_t)k.N;     // a split block has < 2^31 elements (host check)
    const double* sl = arena + k.slab_off;
    double* yb = y + k.dst_off;
    constexpr int NE = RED_CHUNK / 256;
    const uint32_t e0 = (uint32_t)t.chunk * RED_CHUNK + threadIdx.x;
    double v[NE];
    double* d[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const uint32_t e = min(e0 + (uint32_t)i * 256u, mn - 1);        // clamped: every lane loads, only valid ones store
        const uint32_t row = e / N, col = e - row * N;
        d[i] = yb + (size_t)row * k.ldc + col;
        v[i] = *d[i];
    }
    for (int s = 0; s < k.nslab; ++s) {                                  // slab-major: NE independent loads in flight per step,
        const double* p = sl + (size_t)s * mn;                           // each element still summed in slab order
#pragma unroll
        for (int i = 0; i < NE; ++i) v[i] += p[min(e0 + (uint32_t)i * 256u, mn - 1)];
    }
#pragma unroll
    for (int i = 0; i < NE; ++i) if (e0 + (uint32_t)i * 256u < mn) *d[i] = v[i];
}

// ---- diagonal of the superblock Hamiltonian (preconditioner of the generalized-Davidson solver) --------------------------
// diag(H)[(l, r) of KronBlock k] = sum_t dA_t[l] * dB_t[r] over the "diagonal terms": H_L (x) 1, 1 (x) H_R and every merged
// operator pair with sector shift 0 (the Sz Sz terms).  dA_t / dB_t are the diagonals of the plan's own operator copies.
struct DiagSrc { int64_t off; int32_t ld, n, round; int64_t dst; double scale; };     // off < 0: scaled identity
struct DiagSeg { int64_t out_off; int32_t nrow, ncol; int64_t l0, r0; };
__global__ void __launch_bounds__(256) diag_gather_kernel(const DiagSrc* __restrict__ src, int nsrc, int round, const double* __restrict__ arena, double* __restrict__ dvec)
{
    const int t = blockIdx.x;
    if (t >= nsrc) return;
    const DiagSrc s = src[t];
    if (s.round != round) return;
    for (int i = threadIdx.x; i < s.n; i += 256) dvec[s.dst + i] += s.off >= 0 ? arena[s.off + (int64_t)i * (s.ld + 1)] : s.scale;
}
__global__ void __launch_bounds__(256) diag_fill_kernel(const DiagSeg* __restrict__ segs, const double* __restrict__ dA, const double* __restrict__ dB,
                                                         int nterms, int64_t NL, int64_t NR, double* __restrict__ out)
{
    const DiagSeg s = segs[blockIdx.y];
    const int64_t n = (int64_t)s.nrow * s.ncol;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t l = e / s.ncol, r = e % s.ncol;
        double d = 0.0;
        for (int t = 0; t < nterms; ++t) d += dA[(int64_t)t * NL + s.l0 + l] * dB[(int64_t)t * NR + s.r0 + r];
        out[s.out_off + e] = d;
    }
}

}  // namespace
}  // namespace dmrgx

using namespace dmrgx;

// Bases selectable by a task-table entry: the plan's arena, the apply's x and y.
enum : int32_t { BASE_ARENA = 0, BASE_X = 1, BASE_Y = 2 };

namespace dmrgx {
// Task tables are built with element offsets + base selectors and patched into absolute pointers per apply by
// a tiny kernel, so the ggemm kernel itself only ever sees plain pointers.
struct RelProd { int64_t a_off, b_off; int32_t lda, ldb, K, kind; double alpha; int32_t a_base, b_base; };
struct RelGroup { int64_t c_off; int32_t c_base, ldc, M, N, prod_begin, prod_end, n_axpy, accumulate; };

__global__ void patch_tables_kernel(const RelProd* __restrict__ rp, GProd* __restrict__ gp, int np,
                                    const RelGroup* __restrict__ rg, GGroup* __restrict__ gg, int ng,
                                    double* arena, const double* x, double* y)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const double* bases[3] = {arena, x, y};
    if (i < np) {
        const RelProd r = rp[i];
        GProd g;
        g.A = bases[r.a_base] + r.a_off; g.B = bases[r.b_base] + r.b_off;
        g.lda = r.lda; g.ldb = r.ldb; g.K = r.K; g.kind = r.kind; g.alpha = r.alpha;
        gp[i] = g;
    }
    if (i < ng) {
        const RelGroup r = rg[i];
        GGroup g;
        g.C = const_cast<double*>(bases[r.c_base]) + r.c_off;
        g.ldc = r.ldc; g.M = r.M; g.N = r.N; g.prod_begin = r.prod_begin; g.prod_end = r.prod_end;
        g.n_axpy = r.n_axpy; g.accumulate = r.accumulate;
        gg[i] = g;
    }
}
}  // namespace dmrgx

struct DiagTables {                     // dmrgx_kron_diag
    std::vector<DiagSrc> src;           // where the diagonals of the operator copies sit in the arena
    std::vector<DiagSeg> segs;          // this rank's panels of every KronBlock
    int32_t terms = 0, rounds = 0;
    int64_t NL = 0, NR = 0;
};

struct dmrgx_kron_plan {
    dmrgx_kron_info info{};
    DevBuf arena;                       // operators + intermediates + split-K slabs
    DevBuf d_tables;                    // one upload holds every table below, addressed by its offset
    size_t o_rprods = 0, o_rgroups = 0; // relative tables (stage 1 then stage 2, one array)
    size_t o_tiles1 = 0, o_tiles2 = 0, o_red_tasks = 0, o_red_tiles = 0, o_layout = 0;
    int32_t nprods = 0, ngroups = 0, ntiles1 = 0, ntiles2 = 0, n_red_tiles = 0, nlayout = 0;
    template <class T> const T* table(size_t off) const { return packed_at<T>(d_tables, off); }
    // Patched (absolute-pointer) task tables, one set per (x, y) pair seen: a Lanczos solve applies the plan to the same
    // ncv+1 basis vectors cycle after cycle, so after the first cycle no apply has to re-patch (one launch less per step).
    struct Patched { const double* x = nullptr; double* y = nullptr; DevBuf prods, groups; };
    std::vector<std::unique_ptr<Patched>> patched;
    size_t patched_next = 0;            // round-robin victim once PATCHED_MAX sets exist
    static constexpr size_t PATCHED_MAX = 24;
    DiagTables diag;
    bool timing = false;                // per-stage HIP-event timing (dmrgx_kron_plan_timing)
    std::vector<hipEvent_t> ev;         // NEV events per recorded apply: before stage 1, between the stages, after stage 2; at most MAX_TIMED applies
    static constexpr size_t NEV = 3, MAX_TIMED = 4096;
    size_t ev_used = 0;
    ~dmrgx_kron_plan() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};

namespace {

// ---- validation --------------------------------------------------------------------------------------------------------------
inline int32_t world_of(const dmrgx_kron_desc* d) { return d->world_size <= 0 ? 1 : d->world_size; }

dmrgx_status normalise_op(const dmrgx_secop* op, const dmrgx_sectors& sec, const char* what, std::vector<NCell>& out)
{
    out.clear();
    if (!op) return DMRGX_OK;
    if (op->ncells < 0 || (op->ncells > 0 && !op->cells)) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: bad cell list", what);
    for (int32_t i = 0; i < op->ncells; ++i) {
        const dmrgx_cell& c = op->cells[i];
        NCell n{c.row_sector, c.r0, c.c0, c.nr, c.nc, c.kind, c.scale, c.data, c.ld, op->transposed != 0};
        if (n.tr) { n.q -= op->shift; std::swap(n.r0, n.c0); std::swap(n.nr, n.nc); }
        const int32_t qc = n.q + op->shift;
        if (n.q < 0 || n.q >= sec.nsec || qc < 0 || qc >= sec.nsec)
            DMRGX_FAIL(DMRGX_ERR_OUTOFRANGE, "%s: cell %d sector (%d -> %d) out of range [0,%d)", what, i, n.q, qc, sec.nsec);
        if (n.nr <= 0 || n.nc <= 0 || n.r0 < 0 || n.c0 < 0 || n.r0 + n.nr > sec.size[n.q] || n.c0 + n.nc > sec.size[qc])
            DMRGX_FAIL(DMRGX_ERR_OUTOFRANGE, "%s: cell %d rectangle [%d+%d, %d+%d) exceeds block %d x %d", what, i,
                       n.r0, n.nr, n.c0, n.nc, sec.size[n.q], sec.size[qc]);
        if (n.kind == DMRGX_CELL_IDENT) { if (n.nr != n.nc) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: identity cell %d not square", what, i); }
        else if (n.kind == DMRGX_CELL_DENSE) {
            if (!n.data || n.ld < (n.tr ? n.nr : n.nc)) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: dense cell %d has no data / bad ld", what, i);
        } else DMRGX_FAIL(DMRGX_ERR_ARG, "%s: cell %d has unknown kind %d", what, i, n.kind);
        out.push_back(n);
    }
    return DMRGX_OK;
}

// What validation hands to planning beside the descriptor itself.
struct Checked {
    std::map<std::pair<int32_t, int32_t>, int32_t> kmap;       // (IL, IR) -> KronBlock
    std::vector<std::vector<NCell>> Lops, Rops;
    std::vector<NCell> HL, HR;
};

dmrgx_status validate(const dmrgx_kron_desc* d, Checked& in)
{
    const int32_t W = world_of(d);
    if (d->rank < 0 || d->rank >= W) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_plan_create: rank %d outside world %d", d->rank, W);
    const dmrgx_sectors& SL = d->left;
    const dmrgx_sectors& SR = d->right;
    if (SL.nsec <= 0 || SR.nsec <= 0 || !SL.size || !SR.size) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_plan_create: empty sector table");
    for (int i = 0; i < SL.nsec; ++i) if (SL.size[i] <= 0) DMRGX_FAIL(DMRGX_ERR_ARG, "left sector %d has size %d", i, SL.size[i]);
    for (int i = 0; i < SR.nsec; ++i) if (SR.size[i] <= 0) DMRGX_FAIL(DMRGX_ERR_ARG, "right sector %d has size %d", i, SR.size[i]);
    if (d->nblocks <= 0 || !d->block_il || !d->block_ir) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_plan_create: no KronBlocks");
    for (int32_t k = 0; k < d->nblocks; ++k) {
        const int32_t il = d->block_il[k], ir = d->block_ir[k];
        if (il < 0 || il >= SL.nsec || ir < 0 || ir >= SR.nsec) DMRGX_FAIL(DMRGX_ERR_OUTOFRANGE, "KronBlock %d = (%d,%d) out of range", k, il, ir);
        if (!in.kmap.emplace(std::make_pair(il, ir), k).second) DMRGX_FAIL(DMRGX_ERR_ARG, "KronBlock (%d,%d) listed twice", il, ir);
    }
    if (d->n_left_ops < 0 || d->n_right_ops < 0 || d->nterms < 0) DMRGX_FAIL(DMRGX_ERR_ARG, "negative count");
    in.Lops.resize(d->n_left_ops); in.Rops.resize(d->n_right_ops);
    for (int32_t i = 0; i < d->n_left_ops; ++i) DMRGX_CHK(normalise_op(&d->left_ops[i], SL, "left op", in.Lops[i]));
    for (int32_t i = 0; i < d->n_right_ops; ++i) DMRGX_CHK(normalise_op(&d->right_ops[i], SR, "right op", in.Rops[i]));
    if (d->h_left) { if (d->h_left->shift != 0) DMRGX_FAIL(DMRGX_ERR_ARG, "H_L must have shift 0"); DMRGX_CHK(normalise_op(d->h_left, SL, "H_L", in.HL)); }
    if (d->h_right) { if (d->h_right->shift != 0) DMRGX_FAIL(DMRGX_ERR_ARG, "H_R must have shift 0"); DMRGX_CHK(normalise_op(d->h_right, SR, "H_R", in.HR)); }
    for (int32_t t = 0; t < d->nterms; ++t) {
        const dmrgx_term& T = d->terms[t];
        if (T.left_op < 0 || T.left_op >= d->n_left_ops || T.right_op < 0 || T.right_op >= d->n_right_ops)
            DMRGX_FAIL(DMRGX_ERR_OUTOFRANGE, "term %d references operator (%d,%d) out of range", t, T.left_op, T.right_op);
        if (d->left_ops[T.left_op].shift + d->right_ops[T.right_op].shift != 0)
            DMRGX_FAIL(DMRGX_ERR_ARG, "term %d does not conserve Sz (shifts %d,%d)", t, d->left_ops[T.left_op].shift, d->right_ops[T.right_op].shift);
    }
    return DMRGX_OK;
}

// ---- planning: host code only, no HIP call ----------------------------------------------------------------------------------------
// Where every KronBlock sits in the reference vector and in the striped one.  Columns [cbeg(k,w), cend(k,w)) of block k belong to
// rank w (stripe (w + k) mod W: see stripe_of_rank); rank w's segment of a full vector holds its panels of all blocks back to back.
struct Layout {
    int32_t W = 1, me = 0, nb = 0;
    const int32_t *il = nullptr, *ir = nullptr;     // the descriptor's KronBlock list
    std::vector<int32_t> nL, nR;                    // rows and columns of block k
    std::vector<int32_t> cuts;                      // nb x (W + 1): the column cuts of block k, by stripe
    std::vector<int64_t> ref_off;                   // nb + 1: block k in the reference vector
    std::vector<int64_t> seg_off;                   // W x (nb + 1): rank w's panel of block k inside its segment
    int64_t N = 0, seg_stride = 0;
    explicit Layout(const dmrgx_kron_desc* d)
        : W(world_of(d)), me(d->rank), nb(d->nblocks), il(d->block_il), ir(d->block_ir), nL(nb), nR(nb), cuts((size_t)nb * (W + 1)), ref_off(nb + 1, 0), seg_off((size_t)W * (nb + 1), 0)
    {
        for (int32_t k = 0; k < nb; ++k) {
            nL[k] = d->left.size[il[k]]; nR[k] = d->right.size[ir[k]];
            ref_off[k + 1] = ref_off[k] + (int64_t)nL[k] * nR[k];
            for (int32_t s = 0; s <= W; ++s) cuts[(size_t)k * (W + 1) + s] = stripe_cut(nR[k], W, s);
        }
        N = ref_off[nb];
        int64_t max_seg = 0;
        for (int32_t w = 0; w < W; ++w) {
            for (int32_t k = 0; k < nb; ++k) seg_off[(size_t)w * (nb + 1) + k + 1] = seg(k, w) + (int64_t)nL[k] * panel_ld(k, w);
            max_seg = std::max(max_seg, seg(nb, w));
        }
        seg_stride = (W == 1) ? N : ((max_seg + 63) / 64) * 64;
    }
    int32_t cbeg(int32_t k, int32_t w) const { return cuts[(size_t)k * (W + 1) + stripe_of_rank(W, w, k)]; }
    int32_t cend(int32_t k, int32_t w) const { return cuts[(size_t)k * (W + 1) + stripe_of_rank(W, w, k) + 1]; }
    int32_t panel_ld(int32_t k, int32_t w) const { return cend(k, w) - cbeg(k, w); }
    int64_t seg(int32_t k, int32_t w) const { return seg_off[(size_t)w * (nb + 1) + k]; }
    int64_t panel_off(int32_t k, int32_t w) const { return (int64_t)w * seg_stride + seg(k, w); }      // in a full vector
};

// Term groups = a minimum vertex cover of the bipartite graph (distinct left operators) -- terms -- (distinct right operators):
// a covered right operator B_j keys the group  (sum_t a_t A_t) (x) B_j  of its terms (left operators merged, the map the
// reference builds at src/DMRGKron.cpp:955-960), a covered left operator A_i the group  A_i (x) (sum_t a_t B_t).  Merging on
// one side only costs min(#left, #right) groups; at a cut in the middle of a column of the J1-J2 cylinder that is 9-10 sites
// per operator type against a cover of 8 (Koenig: maximum matching, alternating paths from the unmatched left vertices).
struct Cover { std::vector<char> L, R; };
Cover vertex_cover(const dmrgx_kron_desc* d)
{
    const int32_t nl = d->n_left_ops, nr = d->n_right_ops;
    std::vector<std::vector<int32_t>> adj(nl);
    for (int32_t t = 0; t < d->nterms; ++t) if (d->terms[t].a != 0.0) adj[d->terms[t].left_op].push_back(d->terms[t].right_op);
    std::vector<int32_t> matchR(nr, -1), matchL(nl, -1);
    std::vector<char> seen;
    auto augment = [&](auto&& self, int32_t l) -> bool {
        for (int32_t r : adj[l]) {
            if (seen[r]) continue;
            seen[r] = 1;
            if (matchR[r] < 0 || self(self, matchR[r])) { matchR[r] = l; matchL[l] = r; return true; }
        }
        return false;
    };
    for (int32_t l = 0; l < nl; ++l) if (!adj[l].empty()) { seen.assign(nr, 0); augment(augment, l); }
    // Z = vertices reachable from unmatched left vertices along alternating paths; cover = (L \ Z) u (R n Z)
    std::vector<char> zL(nl, 0), zR(nr, 0);
    std::vector<int32_t> stack;
    for (int32_t l = 0; l < nl; ++l) if (!adj[l].empty() && matchL[l] < 0) { zL[l] = 1; stack.push_back(l); }
    while (!stack.empty()) {
        const int32_t l = stack.back(); stack.pop_back();
        for (int32_t r : adj[l]) {
            if (zR[r] || matchL[l] == r) continue;
            zR[r] = 1;
            const int32_t l2 = matchR[r];
            if (l2 >= 0 && !zL[l2]) { zL[l2] = 1; stack.push_back(l2); }
        }
    }
    Cover c{std::vector<char>(nl, 0), zR};
    for (int32_t l = 0; l < nl; ++l) c.L[l] = !adj[l].empty() && !zL[l];
    return c;
}

// The plan's own operators: one merged cell list per side of every term group, H_L and H_R^T, and the operator part of the arena
// that holds their dense cells, filled at plan creation by `copies`.
struct Group {
    int32_t sA, sB;
    std::vector<PCell> left, rightT;    // rightT: cells of Bhat^T
    std::vector<int32_t> ksrc;          // [k]: the source block k' = (IL + sA, IR + sB) of KronBlock k, -1 where it does not exist
    std::vector<int64_t> toff;          // [k]: arena offset of T_{g,k}
};
struct Operators {
    std::vector<Group> G;
    std::vector<PCell> HL, HRT;
    std::vector<CopyTask> copies;
    int64_t elems = 0;                  // arena elements taken by the dense cells
    std::vector<int64_t> TRoff;         // [k]: arena offset of T_R,k, -1 without H_R
};
using Contrib = std::vector<std::pair<double, const std::vector<NCell>*>>;

// merged (or raw) cell list for one side: sum_t coeff_t * op_t ; transpose_out => store cells transposed
void build_side(const Contrib& contrib, bool transpose_out, std::vector<PCell>& dst, Operators& O)
{
    std::map<std::tuple<int32_t, int32_t, int32_t, int32_t, int32_t, int32_t>, int32_t> index;   // key -> dst idx
    std::map<int32_t, int32_t> rounds;
    for (auto& ct : contrib) {
        for (const NCell& c : *ct.second) {
            auto key = std::make_tuple(c.q, c.r0, c.c0, c.nr, c.nc, c.kind);
            auto it = index.find(key);
            int32_t di;
            if (it == index.end()) {
                PCell pc{c.q, c.r0, c.c0, c.nr, c.nc, c.kind, 0.0, -1};
                if (transpose_out) { std::swap(pc.r0, pc.c0); std::swap(pc.nr, pc.nc); }      // q stays the ROW sector of the un-transposed op
                if (c.kind == DMRGX_CELL_DENSE) { pc.off = O.elems; O.elems += (int64_t)pc.nr * pc.nc; }
                dst.push_back(pc);
                di = (int32_t)dst.size() - 1;
                index.emplace(key, di);
            } else di = it->second;
            if (c.kind == DMRGX_CELL_IDENT) dst[di].scale += ct.first * c.scale;
            else O.copies.push_back(CopyTask{dst[di].off, c.data, c.ld, dst[di].nr, dst[di].nc, dst[di].nc, (c.tr != transpose_out) ? 1 : 0, ct.first, rounds[di]++});
        }
    }
}

// term groups: merge on the side with MORE distinct operators, keyed by the operator on the other side
dmrgx_status merge_operators(const dmrgx_kron_desc* d, const Checked& in, const Cover& cover, Operators& O)
{
    std::map<std::pair<int32_t, int32_t>, std::vector<int32_t>> by_key;   // (side: 1 = keyed by right op, 0 = by left op; op) -> term indices
    for (int32_t t = 0; t < d->nterms; ++t) {
        const dmrgx_term& T = d->terms[t];
        if (T.a == 0.0) continue;
        if (cover.R[T.right_op]) by_key[{1, T.right_op}].push_back(t);
        else if (cover.L[T.left_op]) by_key[{0, T.left_op}].push_back(t);
        else DMRGX_FAIL(DMRGX_ERR_INTERNAL, "kron_plan_create: term %d is not covered", t);
    }
    for (auto& kv : by_key) {
        const bool by_right = kv.first.first == 1;
        const int32_t op = kv.first.second;
        Group g;
        g.sB = by_right ? d->right_ops[op].shift : -d->left_ops[op].shift; g.sA = -g.sB;
        Contrib keyed{{1.0, by_right ? &in.Rops[op] : &in.Lops[op]}}, merged;
        for (int32_t t : kv.second) merged.push_back({d->terms[t].a, by_right ? &in.Lops[d->terms[t].left_op] : &in.Rops[d->terms[t].right_op]});
        build_side(by_right ? merged : keyed, false, g.left, O);
        build_side(by_right ? keyed : merged, true, g.rightT, O);
        O.G.push_back(std::move(g));
    }
    build_side({{1.0, &in.HL}}, false, O.HL, O);
    build_side({{1.0, &in.HR}}, true, O.HRT, O);
    return DMRGX_OK;
}

// The intermediates behind the operators in the arena: T_{g,k} (n_L(IL') x my stripe of IR) and T_R,k (n_L x my stripe) -> their elements
int64_t place_intermediates(const Layout& L, const Checked& in, Operators& O)
{
    int64_t elems = 0;
    auto place = [&](int32_t k, int32_t ksrc) { const int64_t off = O.elems + elems; elems += (int64_t)L.nL[ksrc] * L.panel_ld(k, L.me); return off; };
    for (Group& g : O.G) {
        g.ksrc.assign(L.nb, -1); g.toff.assign(L.nb, -1);
        for (int32_t k = 0; k < L.nb; ++k) {
            auto it = in.kmap.find({L.il[k] + g.sA, L.ir[k] + g.sB});
            if (it != in.kmap.end()) { g.ksrc[k] = it->second; g.toff[k] = place(k, it->second); }
        }
    }
    O.TRoff.assign(L.nb, -1);
    if (!O.HRT.empty()) for (int32_t k = 0; k < L.nb; ++k) O.TRoff[k] = place(k, k);
    return elems;
}

// The task tables of both stages, the zero rectangles of the intermediates and the split-K fix-up.
struct Tables {
    std::vector<RelProd> prods;
    std::vector<RelGroup> groups;
    std::vector<GTile> tiles1, tiles2;      // 64 x 64 tiles per stage (128 x 128 tiles for the 128-aligned cores in launches of their own measured equal: rounds 2-4)
    int32_t stage2_begin = 0, stage2_end = 0;   // the groups opened by stage2(), before split-K appends its own
    std::vector<ZeroRect> zero_rects;
    double flops_alg = 0, flops_exec = 0;
    int32_t ksteps(int32_t g) const {      // cost of one tile of group g in k-steps of the GEMM stream
        int32_t c = 0;
        for (int32_t p = groups[g].prod_begin; p < groups[g].prod_end; ++p) c += prods[p].kind == GPROD_GEMM ? ggemm_ksteps(prods[p].K) : 1;
        return c;
    }

    // open a group; products are appended afterwards with add_*; close() sorts AXPY first
    int32_t open(int32_t c_base, int64_t c_off, int32_t ldc, int32_t M, int32_t N, int32_t accumulate) {
        groups.push_back(RelGroup{c_off, c_base, ldc, M, N, (int32_t)prods.size(), (int32_t)prods.size(), 0, accumulate});
        return (int32_t)groups.size() - 1;
    }
    void add_gemm(int32_t a_base, int64_t a_off, int32_t lda, int32_t b_base, int64_t b_off, int32_t ldb, int32_t K) {
        prods.push_back(RelProd{a_off, b_off, lda, ldb, K, GPROD_GEMM, 1.0, a_base, b_base});
    }
    void add_axpy(int32_t s_base, int64_t s_off, int32_t lds, double alpha) {
        prods.push_back(RelProd{0, s_off, 0, lds, 0, GPROD_AXPY, alpha, BASE_ARENA, s_base});
    }
    void close(int32_t g) {
        RelGroup& G = groups[g];
        G.prod_end = (int32_t)prods.size();
        std::stable_sort(prods.begin() + G.prod_begin, prods.end(), [](const RelProd& a, const RelProd& b) { return a.kind > b.kind; });
        G.n_axpy = 0;
        for (int32_t p = G.prod_begin; p < G.prod_end; ++p) {
            const double mn = (double)G.M * G.N;
            if (prods[p].kind == GPROD_AXPY) { G.n_axpy++; flops_alg += 2.0 * mn; }
            else {
                flops_alg += 2.0 * mn * prods[p].K;
                // MFMA work actually issued: 16 x 16 accumulator blocks that intersect the output, k in units of 4
                const double tm = (G.M + 15) / 16, tn = (G.N + 15) / 16;
                flops_exec += 2.0 * tm * tn * 256.0 * (double)(((prods[p].K + 3) / 4) * 4);
            }
        }
    }

    // Stage 1:  T[:, cols] = sum over the transposed right cells of block (IR -> IR') that reach those columns of
    //           X_src[:, contraction range of the cell] * cellT.  A merged right operator may hold several cells with the
    //           same output columns (e.g. O (x) 1 cell (2,2) and the new site's identity cell (2,1)), so groups are built
    //           per output-column SEGMENT with a product list -- never one overwriting group per cell.
    // T (at toff, this rank's stripe of block k) is read from the source block ksrc of x; only its rows [row0, row0 + M) are built.
    void stage1(const Layout& L, const std::vector<PCell>& cellsT, int32_t k, int32_t ksrc, int64_t toff, int32_t row0, int32_t M) {
        const int32_t ir = L.ir[k], cs = L.cbeg(k, L.me), ce = L.cend(k, L.me), w = ce - cs;
        if (w <= 0 || M <= 0) return;
        toff += (int64_t)row0 * w;
        std::set<int32_t> cuts = {cs, ce};
        auto clampc = [&](int32_t v) { return std::min(std::max(v, cs), ce); };
        for (const PCell& c : cellsT) {
            if (c.q != ir) continue;
            cuts.insert(clampc(c.c0)); cuts.insert(clampc(c.c0 + c.nc));
            if (c.kind == DMRGX_CELL_IDENT)        // a scaled copy must read ONE source panel: cut at panel borders too
                for (int32_t p = 0; p < L.W; ++p) { const int32_t sc = L.cbeg(ksrc, p); if (sc > c.r0 && sc < c.r0 + c.nr) cuts.insert(clampc(c.c0 + (sc - c.r0))); }
        }
        for (auto it = cuts.begin(); std::next(it) != cuts.end(); ++it) {
            const int32_t o0 = *it, o1 = *std::next(it);
            bool any = false;
            for (const PCell& c : cellsT) if (c.q == ir && c.c0 <= o0 && c.c0 + c.nc >= o1) { any = true; break; }
            if (!any) { zero_rects.push_back(ZeroRect{toff + (o0 - cs), w, M, o1 - o0, 0}); continue; }      // T is zero there: zero_rects_kernel at plan creation
            const int32_t g = open(BASE_ARENA, toff + (o0 - cs), w, M, o1 - o0, 0);
            for (const PCell& c : cellsT) {
                if (c.q != ir || c.c0 > o0 || c.c0 + c.nc < o1) continue;
                if (c.kind == DMRGX_CELL_DENSE) {
                    for (int32_t p = 0; p < L.W; ++p) {          // contraction index r' in [c.r0, c.r0+c.nr) split over source panels
                        const int32_t k0 = std::max(c.r0, L.cbeg(ksrc, p)), k1 = std::min(c.r0 + c.nr, L.cend(ksrc, p));
                        if (k0 >= k1) continue;
                        add_gemm(BASE_X, L.panel_off(ksrc, p) + (int64_t)row0 * L.panel_ld(ksrc, p) + (k0 - L.cbeg(ksrc, p)), L.panel_ld(ksrc, p),
                                 BASE_ARENA, c.off + (int64_t)(k0 - c.r0) * c.nc + (o0 - c.c0), c.nc, k1 - k0);
                    }
                } else {                                         // identity cell: T[:, o] += scale * X_src[:, c.r0 + (o - c.c0)]
                    const int32_t s0 = c.r0 + (o0 - c.c0);
                    int32_t p = 0;
                    for (int32_t pp = 0; pp < L.W; ++pp) if (L.cbeg(ksrc, pp) <= s0 && s0 < L.cend(ksrc, pp)) p = pp;
                    add_axpy(BASE_X, L.panel_off(ksrc, p) + (int64_t)row0 * L.panel_ld(ksrc, p) + (s0 - L.cbeg(ksrc, p)), L.panel_ld(ksrc, p), c.scale);
                }
            }
            close(g);
            ggemm_append_tiles(tiles1, g, groups[g].M, groups[g].N, ksteps(g));
        }
    }

    // The products of the left cells of sector il that cover rows [ra, rb) of an open stage-2 group; the B operand (ld = w) starts at b_base + b_off
    void add_left_cells(const std::vector<PCell>& cells, int32_t il, int32_t ra, int32_t rb, int32_t b_base, int64_t b_off, int32_t w) {
        for (const PCell& c : cells) {
            if (c.q != il || c.r0 > ra || c.r0 + c.nr < rb) continue;
            if (c.kind == DMRGX_CELL_DENSE) add_gemm(BASE_ARENA, c.off + (int64_t)(ra - c.r0) * c.nc, c.nc, b_base, b_off + (int64_t)c.c0 * w, w, c.nc);
            else add_axpy(b_base, b_off + (int64_t)(c.c0 + (ra - c.r0)) * w, w, c.scale);
        }
    }
    // Stage 2:  Y_k[rows, stripe] = sum over left cells covering `rows`
    void stage2(const Layout& L, const Operators& O) {
        stage2_begin = (int32_t)groups.size();
        for (int32_t k = 0; k < L.nb; ++k) {
            const int32_t il = L.il[k], w = L.panel_ld(k, L.me), nl = L.nL[k];
            if (w <= 0) continue;
            std::set<int32_t> cuts = {0, nl};
            for (const Group& g : O.G) if (g.ksrc[k] >= 0) for (const PCell& c : g.left) if (c.q == il) { cuts.insert(c.r0); cuts.insert(c.r0 + c.nr); }
            for (const PCell& c : O.HL) if (c.q == il) { cuts.insert(c.r0); cuts.insert(c.r0 + c.nr); }
            for (auto it = cuts.begin(); std::next(it) != cuts.end(); ++it) {
                const int32_t ra = *it, rb = *std::next(it);
                const int32_t grp = open(BASE_Y, L.seg(k, L.me) + (int64_t)ra * w, w, rb - ra, w, 0);
                for (const Group& g : O.G) if (g.ksrc[k] >= 0) add_left_cells(g.left, il, ra, rb, BASE_ARENA, g.toff[k], w);
                add_left_cells(O.HL, il, ra, rb, BASE_X, L.panel_off(k, L.me), w);             // H_L (x) 1 : B operand is this rank's own panel of X_k
                if (O.TRoff[k] >= 0) add_axpy(BASE_ARENA, O.TRoff[k] + (int64_t)ra * w, w, 1.0);   // 1 (x) H_R
                close(grp);
            }
        }
        stage2_end = (int32_t)groups.size();
    }

    // Stage-2 output tiles carry the whole operator list of a KronBlock (K ~ 10^4 at m = 2048) and there are fewer
    // of them than workgroup slots, so long product lists are cut on product boundaries into contiguous segments of
    // about equal length ("split-K"): enough (tile, segment) units that the scheduler can balance the XCDs, long enough
    // that the 32 KB partial-tile write is amortised.  Segment 0 writes y, segment s >= 1 writes a compact slab in the
    // arena; slab_reduce_kernel adds them in fixed order, so the result stays bit-reproducible (no atomics).
    std::vector<RedTask> red_tasks;
    std::vector<RedTile> red_tiles;
    int64_t slab_elems = 0;
    void finalize_stage2(int64_t slab_base) {
        double total = 0;
        for (int32_t g = stage2_begin; g < stage2_end; ++g) {
            const RelGroup& G = groups[g];
            total += (double)ksteps(g) * ((G.M + GG_BM - 1) / GG_BM) * ((G.N + GG_BN - 1) / GG_BN);
        }
        constexpr double units = 8192.0;      // (4 k - 32 k units, a floor of 8 - 32 k-steps and a tapered last segment all measured within +-1 %: round 2)
        // Shortest segment worth its 32 KB slab: 16 k-steps when the launch has work for every workgroup slot anyway; a small
        // superblock (m <= 512: a few thousand tile-k-steps in all) is latency-bound by its longest segment instead, so the
        // floor drops until about 1024 units exist (4 k-steps at least).
        const double min_seg = std::min(16.0, std::max(4.0, total / 1024.0));
        const double seg_target = std::max(total / units, min_seg);
        for (int32_t g = stage2_begin; g < stage2_end; ++g) {
            const int32_t axpy_begin = groups[g].prod_begin, gemm_begin = groups[g].prod_begin + groups[g].n_axpy, gemm_end = groups[g].prod_end;
            int32_t gcost = 0;
            for (int32_t p = gemm_begin; p < gemm_end; ++p) gcost += ggemm_ksteps(prods[p].K);
            // S equal segments of ~seg_target k-steps, cut at gcost * s / S (distinct: S <= gcost).  Cuts may fall inside a
            // product: a product is just (pointers, K), so it is split at a multiple of GG_BK.  (Cutting the last
            // segment further into 1/2, 1/4, 1/4 so that every XCD finishes on short units measured neutral to slightly negative.)
            int32_t S = (int32_t)std::min<double>(64.0, std::max(1.0, std::floor(gcost / seg_target + 0.5)));
            if ((int64_t)groups[g].M * groups[g].N >= (int64_t)1 << 31) S = 1;      // slab_reduce_kernel indexes a block with 32 bits
            S = std::min(S, gcost);
            if (S <= 1) { ggemm_append_tiles(tiles2, g, groups[g].M, groups[g].N, ksteps(g)); continue; }
            const int64_t mn = (int64_t)groups[g].M * groups[g].N;
            red_tasks.push_back(RedTask{groups[g].c_off, slab_base + slab_elems, groups[g].ldc, groups[g].M, groups[g].N, S - 1});
            for (int64_t c = 0; c * RED_CHUNK < mn; ++c) red_tiles.push_back(RedTile{(int32_t)red_tasks.size() - 1, (int32_t)c});
            const int32_t n_axpy = groups[g].n_axpy;
            int32_t lo = 0, p = gemm_begin, ps = 0;             // p: the product the stream stands in, ps: its start in k-steps
            for (int32_t sidx = 0; sidx < S; ++sidx) {
                const int32_t hi = (int32_t)(((int64_t)gcost * (sidx + 1)) / S);
                const int32_t nb = (int32_t)prods.size();
                // the scaled-copy products (identity operator cells, 1 (x) H_R) are dealt over the segments: each is a dependent
                // descriptor + tile load of its own, and all of them on segment 0 made that unit the tail of its tile
                int32_t n_axpy_seg = 0;
                for (int32_t q = sidx; q < n_axpy; q += S) { const RelProd ax = prods[axpy_begin + q]; prods.push_back(ax); ++n_axpy_seg; }
                while (p < gemm_end && ps < hi) {
                    const int32_t pe = ps + ggemm_ksteps(prods[p].K), olo = std::max(lo, ps), ohi = std::min(hi, pe);
                    if (olo < ohi) {
                        RelProd sub = prods[p];
                        const int32_t k0 = (olo - ps) * GG_BK, k1 = std::min(prods[p].K, (ohi - ps) * GG_BK);
                        sub.a_off += k0; sub.b_off += (int64_t)k0 * sub.ldb; sub.K = k1 - k0;
                        prods.push_back(sub);
                    }
                    if (pe > hi) break;                         // the rest of the product belongs to the next segment
                    ps = pe; ++p;
                }
                const int32_t ne = (int32_t)prods.size();
                int32_t gs = g;
                if (sidx > 0) {                                  // a group of its own that writes slab sidx - 1
                    RelGroup slab = groups[g];
                    slab.c_base = BASE_ARENA; slab.c_off = slab_base + slab_elems + (int64_t)(sidx - 1) * mn; slab.ldc = slab.N; slab.accumulate = 0;
                    groups.push_back(slab);
                    gs = (int32_t)groups.size() - 1;
                }
                groups[gs].prod_begin = nb; groups[gs].prod_end = ne; groups[gs].n_axpy = n_axpy_seg;
                ggemm_append_tiles(tiles2, gs, groups[gs].M, groups[gs].N, (hi - lo) + n_axpy_seg);
                lo = hi;
            }
            slab_elems += (int64_t)(S - 1) * mn;
        }
    }
};

// Diagonal terms (dmrgx_kron_diag): t = 0: H_L (x) 1, t = 1: 1 (x) H_R, then the shift-0 groups.  Every source adds a run of
// one operator's diagonal (or a constant) into dvec = [dA (terms x NL) | dB (terms x NR)]; sources of one (side, term, sector)
// are added in separate rounds.
DiagTables diag_tables(const dmrgx_kron_desc* d, const Layout& L, const Operators& O)
{
    DiagTables D;
    const dmrgx_sectors* S[2] = {&d->left, &d->right};
    std::vector<int64_t> off[2];                                          // sector offsets, left and right
    for (int side = 0; side < 2; ++side) {
        off[side].assign(S[side]->nsec + 1, 0);
        for (int i = 0; i < S[side]->nsec; ++i) off[side][i + 1] = off[side][i] + S[side]->size[i];
    }
    D.NL = off[0].back(); D.NR = off[1].back();
    D.terms = 2;
    for (auto& g : O.G) if (g.sA == 0 && g.sB == 0) ++D.terms;
    std::map<std::tuple<int32_t, int32_t, int32_t>, int32_t> rounds;      // (side, term, sector) -> sources so far
    auto add = [&](int side, int32_t t, int32_t q, int32_t lo, int32_t n, int64_t src_off, int32_t ld, double scale) {
        const int32_t round = rounds[std::make_tuple(side, t, q)]++;
        D.rounds = std::max(D.rounds, round + 1);
        D.src.push_back(DiagSrc{src_off, ld, n, round, (side == 0 ? (int64_t)t * D.NL : (int64_t)D.terms * D.NL + (int64_t)t * D.NR) + off[side][q] + lo, scale});
    };
    auto add_cells = [&](const std::vector<PCell>& cells, int side, int32_t t) {
        for (const PCell& c : cells) {
            // block (q -> q): the diagonal crosses the cell where r0 + i == c0 + j (transposed storage swaps the roles, same set)
            const int32_t lo = std::max(c.r0, c.c0), hi = std::min(c.r0 + c.nr, c.c0 + c.nc);
            if (lo >= hi) continue;
            if (c.kind != DMRGX_CELL_DENSE && c.r0 != c.c0) continue;      // an identity cell maps row r0 + i to column c0 + i: on the diagonal only when r0 == c0
            add(side, t, c.q, lo, hi - lo, c.kind == DMRGX_CELL_DENSE ? c.off + (int64_t)(lo - c.r0) * c.nc + (lo - c.c0) : -1, c.nc, c.scale);
        }
    };
    auto add_ones = [&](int side, int32_t t) { for (int32_t q = 0; q < S[side]->nsec; ++q) add(side, t, q, 0, S[side]->size[q], -1, 0, 1.0); };
    add_cells(O.HL, 0, 0); add_ones(1, 0);
    add_ones(0, 1); add_cells(O.HRT, 1, 1);
    int32_t t = 2;
    for (auto& g : O.G) {
        if (g.sA != 0 || g.sB != 0) continue;
        add_cells(g.left, 0, t); add_cells(g.rightT, 1, t);
        ++t;
    }
    for (int32_t k = 0; k < L.nb; ++k) {
        if (L.panel_ld(k, L.me) <= 0) continue;
        D.segs.push_back(DiagSeg{L.seg(k, L.me), L.nL[k], L.panel_ld(k, L.me), off[0][L.il[k]], off[1][L.ir[k]] + L.cbeg(k, L.me)});
    }
    return D;
}

// Everything the device step and the later calls need.
struct HostPlan {
    Tables tab;                                         // relative products and groups, the two scheduled tile lists, zero rectangles, reduction
    std::vector<CopyTask> copies;                       // operator copies; contributions to one cell go in rounds (round 0 writes)
    std::vector<CopyTile> copy_tiles;                   // their 32 x 32 tiles, round after round
    std::vector<std::pair<size_t, size_t>> copy_rounds; // (first tile, tiles) of every round that has any
    std::vector<LayoutSeg> layout;
    DiagTables diag;
    int64_t arena_ops = 0, arena_T = 0, arena_slabs = 0;   // arena extents in elements: operators, intermediates, split-K slabs
    dmrgx_kron_info info{};
};

// rows_read (DMRGX_PLAN_FOLD, default on): stage 1 builds only the rows of T_{g,k} that stage 2 reads -- the rows under a cell of the group's
// left operator in sector IL, for the Sp / Sm operators of a block's new site (one identity cell per sector block) about half of them.  The
// other rows get no group, no tile and no zero rectangle.  Every element of y stays the same sum in the same order: y is bit for bit what
// the plan of whole intermediates gives.
dmrgx_status plan_on_host(const dmrgx_kron_desc* d, const Checked& in, bool rows_read, HostPlan& hp)
{
    const Layout L(d);
    Operators O;
    DMRGX_CHK(merge_operators(d, in, vertex_cover(d), O));
    const int64_t T_elems = place_intermediates(L, in, O);
    Tables& B = hp.tab;
    for (const Group& g : O.G)
        for (int32_t k = 0; k < L.nb; ++k) {
            if (g.ksrc[k] < 0) continue;
            if (!rows_read) { B.stage1(L, g.rightT, k, g.ksrc[k], g.toff[k], 0, L.nL[g.ksrc[k]]); continue; }
            std::vector<std::pair<int32_t, int32_t>> read;             // [c0, c0 + nc) of the left cells of sector IL, merged into disjoint ranges
            for (const PCell& c : g.left) if (c.q == L.il[k]) read.push_back({c.c0, c.c0 + c.nc});
            std::sort(read.begin(), read.end());
            for (size_t i = 0; i < read.size();) {
                const int32_t r0 = read[i].first;
                int32_t r1 = read[i].second;
                for (++i; i < read.size() && read[i].first <= r1; ++i) r1 = std::max(r1, read[i].second);
                B.stage1(L, g.rightT, k, g.ksrc[k], g.toff[k], r0, r1 - r0);
            }
        }
    if (!O.HRT.empty()) for (int32_t k = 0; k < L.nb; ++k) B.stage1(L, O.HRT, k, k, O.TRoff[k], 0, L.nL[k]);
    B.stage2(L, O);
    B.finalize_stage2(O.elems + T_elems);
    ggemm_schedule(B.tiles1, B.groups);
    ggemm_schedule(B.tiles2, B.groups);
    if (B.zero_rects.size() >= ((size_t)1 << 23)) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_plan: %zu zero rectangles exceed the launch grid", B.zero_rects.size());
    hp.arena_ops = O.elems; hp.arena_T = T_elems; hp.arena_slabs = B.slab_elems;
    for (int32_t r = 0;; ++r) {                         // (a cell's contributions are numbered 0, 1, ...: the first round without a tile is the end)
        const size_t first = hp.copy_tiles.size();
        for (size_t i = 0; i < O.copies.size(); ++i) if (O.copies[i].round == r)
            for (int32_t ti = 0; ti < (O.copies[i].nr + 31) / 32; ++ti)
                for (int32_t tj = 0; tj < (O.copies[i].nc + 31) / 32; ++tj) hp.copy_tiles.push_back(CopyTile{(int32_t)i, ti, tj, 0});
        if (hp.copy_tiles.size() == first) break;
        hp.copy_rounds.push_back({first, hp.copy_tiles.size() - first});
    }
    for (int32_t k = 0; k < L.nb; ++k) for (int32_t w = 0; w < L.W; ++w)      // layout conversion table (reference order <-> rank-major stripes)
        if (L.panel_ld(k, w) > 0) hp.layout.push_back(LayoutSeg{L.ref_off[k] + L.cbeg(k, w), L.panel_off(k, w), L.nL[k], L.panel_ld(k, w), L.nR[k], L.panel_ld(k, w)});
    hp.diag = diag_tables(d, L, O);

    dmrgx_kron_info& I = hp.info;
    I.n_states = L.N; I.vec_len = (L.W == 1) ? L.N : (int64_t)L.W * L.seg_stride; I.local_offset = (int64_t)L.me * L.seg_stride;
    I.local_len = (L.W == 1) ? L.N : L.seg_stride; I.seg_stride = L.seg_stride;
    I.flops_alg = B.flops_alg; I.flops_exec = B.flops_exec;
    I.bytes_alg = 8.0 * (double)O.elems + 8.0 * ((double)L.N + (double)L.seg(L.nb, L.me));      // every dense operator cell once, x, this rank's y
    I.bytes_workspace = 16.0 * (double)T_elems + 16.0 * (double)B.slab_elems;
    I.n_groups = (int32_t)O.G.size(); I.n_tiles_stage1 = (int32_t)B.tiles1.size(); I.n_tiles_stage2 = (int32_t)B.tiles2.size();      // (n_tiles_big, flops_alg_big: 0, the MatMult runs 64 x 64 tiles only)
    hp.copies = std::move(O.copies);
    return DMRGX_OK;
}

// developer aid and test evidence (DMRGX_PLAN_DUMP): scheduled tile lists, one line per tile; then one line per zero rectangle of the
// intermediates ("zr i off ld nr nc") and one per split-K reduction task ("red i dst_off slab_off ldc M N nslab")
void dump_plan(const char* path, const Tables& B)
{
    FILE* f = fopen(path, "w");
    if (!f) return;
    auto put = [&](const char* name, const std::vector<GTile>& tl) {
        for (size_t i = 0; i < tl.size(); ++i) {
            const GTile& t = tl[i];
            if (t.group < 0) { fprintf(f, "%s %zu -1 0 0 0 0 0 0\n", name, i); continue; }
            const RelGroup& G = B.groups[t.group];
            fprintf(f, "%s %zu %d %d %d %d %d %d %d\n", name, i, t.group, t.tm, t.tn, G.M, G.N, B.ksteps(t.group), G.prod_end - G.prod_begin);
        }
    };
    put("s1", B.tiles1); put("s2", B.tiles2);
    size_t i = 0;
    for (const ZeroRect& z : B.zero_rects) fprintf(f, "zr %zu %lld %d %d %d\n", i++, (long long)z.off, z.ld, z.nr, z.nc);
    i = 0;
    for (const RedTask& r : B.red_tasks) fprintf(f, "red %zu %lld %lld %d %d %d %d\n", i++, (long long)r.dst_off, (long long)r.slab_off, r.ldc, r.M, r.N, r.nslab);
    fclose(f);
}

// ---- device step: the arena and the tables of a finished HostPlan -----------------------------------------------------------------
dmrgx_status create_device_objects(HostPlan& hp, hipStream_t st, dmrgx_kron_plan& P)
{
    const Tables& B = hp.tab;
    P.info = hp.info;
    DMRGX_CHK(P.arena.alloc_f64((size_t)std::max<int64_t>(hp.arena_ops + hp.arena_T + hp.arena_slabs, 1), st));
    {   // operator copies, one launch per accumulation round (round 0 writes); the unreached segments of the intermediates are zeroed.
        // Nothing else of the arena is read before it is written: every dense operator cell has a round-0 copy, stage 1 writes the reached
        // segments of every T_{g,k} whole, the split-K segments write their slabs whole.
        DevBuf d_tab;                                   // the copy tasks and the tile lists of all rounds in one upload
        PackedUpload pk;
        const size_t o_tasks = pk.add(hp.copies), o_zero = pk.add(B.zero_rects), o_tiles = pk.add(hp.copy_tiles);
        DMRGX_CHK(pk.upload(d_tab, st));
        if (!B.zero_rects.empty()) {
            int64_t big = 1;
            for (const ZeroRect& r : B.zero_rects) big = std::max(big, (int64_t)r.nr * r.nc);
            hipLaunchKernelGGL(zero_rects_kernel, dim3((unsigned)B.zero_rects.size(), (unsigned)std::min<int64_t>((big + 2047) / 2048, 512)), dim3(256), 0, st,
                               (const ZeroRect*)packed_at<ZeroRect>(d_tab, o_zero), P.arena.as<double>());
            DMRGX_HIP(hipGetLastError());
        }
        for (const auto& r : hp.copy_rounds) {
            hipLaunchKernelGGL(cell_copy_kernel, dim3((unsigned)r.second), dim3(256), 0, st, (const CopyTile*)packed_at<CopyTile>(d_tab, o_tiles) + r.first,
                               (const CopyTask*)packed_at<CopyTask>(d_tab, o_tasks), P.arena.as<double>());
            DMRGX_HIP(hipGetLastError());
        }
    }
    P.nprods = (int32_t)B.prods.size(); P.ngroups = (int32_t)B.groups.size();
    P.ntiles1 = (int32_t)B.tiles1.size(); P.ntiles2 = (int32_t)B.tiles2.size();
    P.n_red_tiles = (int32_t)B.red_tiles.size(); P.nlayout = (int32_t)hp.layout.size();
    PackedUpload pk;                                    // every table of the plan in one copy
    P.o_rprods = pk.add(B.prods); P.o_rgroups = pk.add(B.groups); P.o_tiles1 = pk.add(B.tiles1); P.o_tiles2 = pk.add(B.tiles2);
    P.o_red_tasks = pk.add(B.red_tasks); P.o_red_tiles = pk.add(B.red_tiles); P.o_layout = pk.add(hp.layout);
    DMRGX_CHK(pk.upload(P.d_tables, st));
    P.diag = std::move(hp.diag);
    return DMRGX_OK;
}

}  // namespace

extern "C" dmrgx_status dmrgx_kron_plan_create(const dmrgx_kron_desc* d, void* stream, dmrgx_kron_plan** out)
{
    if (!d || !out) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_plan_create: null argument");
    *out = nullptr;
    Checked in;
    DMRGX_CHK(validate(d, in));
    HostPlan hp;
    const char* rows = getenv("DMRGX_PLAN_FOLD");        // A/B switch, read at plan creation: 0 builds every intermediate whole
    DMRGX_CHK(plan_on_host(d, in, !(rows && atoi(rows) == 0), hp));
    if (const char* dump = getenv("DMRGX_PLAN_DUMP")) dump_plan(dump, hp.tab);
    std::unique_ptr<dmrgx_kron_plan> P(new (std::nothrow) dmrgx_kron_plan());
    if (!P) DMRGX_FAIL(DMRGX_ERR_MEM, "out of host memory");
    DMRGX_CHK(create_device_objects(hp, (hipStream_t)stream, *P));
    *out = P.release();
    return DMRGX_OK;
}

extern "C" dmrgx_status dmrgx_kron_plan_info(const dmrgx_kron_plan* plan, dmrgx_kron_info* info)
{
    if (!plan || !info) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_plan_info: null argument");
    *info = plan->info;
    return DMRGX_OK;
}

// The patched tables of the pair (x, y): from the cache, or patched now on `st` into a new set or, once PATCHED_MAX exist, over the next victim.
static dmrgx_status patched_tables(dmrgx_kron_plan* P, const double* x_full, double* y_local, hipStream_t st, dmrgx_kron_plan::Patched** out)
{
    for (auto& c : P->patched) if (c->x == x_full && c->y == y_local) { *out = c.get(); return DMRGX_OK; }
    dmrgx_kron_plan::Patched* T = nullptr;
    if (P->patched.size() < dmrgx_kron_plan::PATCHED_MAX) {
        std::unique_ptr<dmrgx_kron_plan::Patched> c(new (std::nothrow) dmrgx_kron_plan::Patched());
        if (!c) DMRGX_FAIL(DMRGX_ERR_MEM, "out of host memory");
        DMRGX_CHK(c->prods.alloc(std::max<size_t>((size_t)P->nprods, 1) * sizeof(GProd)));
        DMRGX_CHK(c->groups.alloc(std::max<size_t>((size_t)P->ngroups, 1) * sizeof(GGroup)));
        P->patched.push_back(std::move(c));
        T = P->patched.back().get();
    } else {
        T = P->patched[P->patched_next].get();
        P->patched_next = (P->patched_next + 1) % dmrgx_kron_plan::PATCHED_MAX;
    }
    T->x = x_full; T->y = y_local;
    const int n = std::max(P->nprods, P->ngroups);
    if (n > 0) {
        hipLaunchKernelGGL(patch_tables_kernel, dim3((n + 255) / 256), dim3(256), 0, st,
                           P->table<RelProd>(P->o_rprods), T->prods.as<GProd>(), P->nprods,
                           P->table<RelGroup>(P->o_rgroups), T->groups.as<GGroup>(), P->ngroups,
                           P->arena.as<double>(), x_full, y_local);
        DMRGX_HIP(hipGetLastError());
    }
    *out = T;
    return DMRGX_OK;
}

extern "C" dmrgx_status dmrgx_kron_apply(dmrgx_kron_plan* P, const double* x_full, double* y_local, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!P || !x_full || !y_local) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_apply: null argument");
    dmrgx_kron_plan::Patched* T = nullptr;
    DMRGX_CHK(patched_tables(P, x_full, y_local, st, &T));
    hipEvent_t* e = nullptr;
    if (P->timing && P->ev_used + P->NEV <= P->NEV * P->MAX_TIMED) {
        while (P->ev.size() < P->ev_used + P->NEV) { hipEvent_t x; DMRGX_HIP(hipEventCreate(&x)); P->ev.push_back(x); }
        e = &P->ev[P->ev_used];
        P->ev_used += P->NEV;
    }
    // one launch per stage, bracketed by events
    if (e) DMRGX_HIP(hipEventRecord(e[0], st));
    DMRGX_CHK(ggemm_launch(P->table<GTile>(P->o_tiles1), T->groups.as<GGroup>(), T->prods.as<GProd>(), P->ntiles1, st, 0));
    if (e) DMRGX_HIP(hipEventRecord(e[1], st));
    DMRGX_CHK(ggemm_launch(P->table<GTile>(P->o_tiles2), T->groups.as<GGroup>(), T->prods.as<GProd>(), P->ntiles2, st, 0));
    if (e) DMRGX_HIP(hipEventRecord(e[2], st));
    if (P->n_red_tiles > 0) {
        hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)P->n_red_tiles), dim3(256), 0, st, P->table<RedTile>(P->o_red_tiles), P->table<RedTask>(P->o_red_tasks), y_local, P->arena.as<double>());
        DMRGX_HIP(hipGetLastError());
    }
    return DMRGX_OK;
}

extern "C" dmrgx_status dmrgx_kron_plan_timing(dmrgx_kron_plan* P, int32_t enable)
{
    if (!P) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_plan_timing: null plan");
    if (enable) P->ev_used = 0;
    P->timing = enable != 0;
    return DMRGX_OK;
}

extern "C" dmrgx_status dmrgx_kron_plan_timing_read(dmrgx_kron_plan* P, double* ms, int64_t* n_applies)
{
    if (!P || !ms || !n_applies) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_plan_timing_read: null argument");
    ms[0] = ms[1] = ms[2] = ms[3] = 0.0; *n_applies = (int64_t)(P->ev_used / P->NEV);      // ms[0], ms[2]: the 128 x 128 slots, 0 for the MatMult
    for (size_t i = 0; i + P->NEV <= P->ev_used; i += P->NEV) {
        DMRGX_HIP(hipEventSynchronize(P->ev[i + 2]));
        for (int k = 0; k < 2; ++k) { float t = 0; DMRGX_HIP(hipEventElapsedTime(&t, P->ev[i + k], P->ev[i + k + 1])); ms[2 * k + 1] += t; }
    }
    return DMRGX_OK;
}

extern "C" dmrgx_status dmrgx_kron_plan_destroy(dmrgx_kron_plan* plan)
{
    if (!plan) return DMRGX_OK;
    // no synchronisation: the blocks go back to the pool and are recycled in stream order (pool.hip)
    delete plan;
    return DMRGX_OK;
}

static dmrgx_status layout_copy(const dmrgx_kron_plan* P, const double* src, double* dst, int to_striped, hipStream_t st)
{
    if (!P || !src || !dst) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_vec layout copy: null argument");
    if (P->nlayout == 0) return DMRGX_OK;
    hipLaunchKernelGGL(layout_copy_kernel, dim3(64, (unsigned)P->nlayout), dim3(256), 0, st, P->table<LayoutSeg>(P->o_layout), src, dst, to_striped);
    DMRGX_HIP(hipGetLastError());
    return DMRGX_OK;
}

extern "C" dmrgx_status dmrgx_kron_vec_to_striped(const dmrgx_kron_plan* plan, const double* v_ref_dev, double* v_full_dev, void* stream)
{ return layout_copy(plan, v_ref_dev, v_full_dev, 1, (hipStream_t)stream); }

extern "C" dmrgx_status dmrgx_kron_vec_from_striped(const dmrgx_kron_plan* plan, const double* v_full_dev, double* v_ref_dev, void* stream)
{ return layout_copy(plan, v_full_dev, v_ref_dev, 0, (hipStream_t)stream); }

extern "C" dmrgx_status dmrgx_kron_diag(dmrgx_kron_plan* P, double* d_local, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!P || !d_local) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_diag: null argument");
    const DiagTables& D = P->diag;
    DevBuf dvec, d_src, d_segs;
    const size_t nvec = (size_t)D.terms * (size_t)(D.NL + D.NR);
    DMRGX_CHK(dvec.alloc(std::max<size_t>(nvec, 1) * sizeof(double)));
    DMRGX_HIP(zero_async(dvec.p, dvec.bytes, st));
    DMRGX_HIP(zero_async(d_local, (size_t)P->info.local_len * sizeof(double), st));
    DMRGX_CHK(upload(d_src, D.src, st));
    DMRGX_CHK(upload(d_segs, D.segs, st));
    for (int32_t r = 0; r < D.rounds; ++r) {
        hipLaunchKernelGGL(diag_gather_kernel, dim3((unsigned)D.src.size()), dim3(256), 0, st, d_src.as<DiagSrc>(), (int)D.src.size(), r,
                           (const double*)P->arena.as<double>(), dvec.as<double>());
        DMRGX_HIP(hipGetLastError());
    }
    if (!D.segs.empty()) {
        hipLaunchKernelGGL(diag_fill_kernel, dim3(64, (unsigned)D.segs.size()), dim3(256), 0, st, d_segs.as<DiagSeg>(), (const double*)dvec.as<double>(),
                           (const double*)(dvec.as<double>() + (size_t)D.terms * D.NL), D.terms, D.NL, D.NR, d_local);
        DMRGX_HIP(hipGetLastError());
    }
    return DMRGX_OK;
}

// ---- all-pairs correlators: G = Gram matrix of operator images of psi ---------------------------------------------------------------
// An image v = sum_t c_t (A_t (x) B_t) psi is formed block by block.  A one-sided term is a list of grouped-GEMM products (dense cells)
// and scaled copies (identity cells), exactly like a stage-2 (stage-1) row of the MatMult without the other factor.  A two-sided term
// is the MatMult's two stages: T = X_k B^T goes to pool scratch in a first grouped launch, A T is accumulated into the image by the
// second.  All terms of a vector that land in one image block -- from whichever source KronBlock -- are products of the same groups, so
// they are summed inside the GEMM and every image element is written exactly once.  dmrgx_vec_gram then takes every inner product at
// once.  The images are never held whole: the image blocks are worked off in slices that fit the workspace bound.
//
// The coefficient of a term is applied once: as the scale of a scaled copy, or folded into the one operand of the term that is
// materialised for it (the left one of a two-sided term) -- a GEMM product itself carries none.  For a scaled-identity cell the scale of the
// copy is the rounded product c * scale: exact whenever scale is 1 or c a power of two (every case the engine has: c in {1, 1/2}), one
// rounding more than c * scale * x otherwise.
namespace {
struct UCell { int32_t q, r0, c0, nr, nc, kind; double scale; const double* data; int32_t ld; int64_t trans_off; };      // data: row-major in the shape the NN GEMM reads; trans_off >= 0: materialised there; scale: coefficient included
struct ImgBlock { int32_t a, b; int64_t size, off; int32_t slice; };
enum : int { SIDE_LEFT = 0, SIDE_RIGHT = 1 };

// One contribution to (image block, vector): the cells of an operator (row sector = the image's) applied to a source matrix.
//   left kind:  Y[r0.., :] += cell * S[c0.., :]        S: rows of the operator's column sector x n_R(b), leading dimension lds
//   right kind: Y[:, r0..] += S[:, c0..] * cell^T      S: n_L(a) x columns of the operator's column sector
struct ImgContrib { const std::vector<UCell>* cells; const double* S; int32_t lds; };

struct GramLayout {
    const dmrgx_sectors* SL; const dmrgx_sectors* SR;
    int32_t nblocks; const int32_t* il; const int32_t* ir;
    std::map<std::pair<int32_t, int32_t>, int32_t> kmap;
    std::vector<int64_t> ref_off;
};

// The offsets and the (il, ir) -> index map of a KronBlock list over checked sector tables; `what` names the list in messages.
dmrgx_status block_layout(const char* fn, const char* what, const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks, const int32_t* block_il, const int32_t* block_ir, GramLayout& L)
{
    L.SL = left; L.SR = right; L.nblocks = nblocks; L.il = block_il; L.ir = block_ir;
    L.ref_off.assign((size_t)nblocks + 1, 0);
    for (int32_t k = 0; k < nblocks; ++k) {
        const int32_t il = block_il[k], ir = block_ir[k];
        if (il < 0 || il >= left->nsec || ir < 0 || ir >= right->nsec) DMRGX_FAIL(DMRGX_ERR_OUTOFRANGE, "%s: %s %d = (%d,%d) out of range", fn, what, k, il, ir);
        if (!L.kmap.emplace(std::make_pair(il, ir), k).second) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: %s (%d,%d) listed twice", fn, what, il, ir);
        L.ref_off[k + 1] = L.ref_off[k] + (int64_t)left->size[il] * right->size[ir];
    }
    return DMRGX_OK;
}

// The same after the checks of the sector tables themselves: everything a call can refuse without looking at psi.
dmrgx_status kron_layout(const char* fn, const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks, const int32_t* block_il, const int32_t* block_ir, GramLayout& L)
{
    if (!left || !right || left->nsec <= 0 || right->nsec <= 0 || !left->size || !right->size) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: empty sector table", fn);
    for (int i = 0; i < left->nsec; ++i) if (left->size[i] <= 0) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: left sector %d has size %d", fn, i, left->size[i]);
    for (int i = 0; i < right->nsec; ++i) if (right->size[i] <= 0) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: right sector %d has size %d", fn, i, right->size[i]);
    if (nblocks <= 0 || !block_il || !block_ir) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: no KronBlocks", fn);
    return block_layout(fn, "KronBlock", left, right, nblocks, block_il, block_ir, L);
}

dmrgx_status gram_layout(const char* fn, const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks, const int32_t* block_il, const int32_t* block_ir,
                         const double* psi_dev, GramLayout& L)
{
    if (!psi_dev) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: null psi", fn);
    return kron_layout(fn, left, right, nblocks, block_il, block_ir, L);
}

// The operands of one call.  The NN GEMM reads a left cell as A (row-major nr x nc) and a right cell as B = cell^T (row-major nc x nr): cells
// stored the other way round, and cells that carry a coefficient, are materialised once per call (as the plan's cell_copy writes B^T).
// One entry per (side, operator, coefficient) in use.  Order of use: use_of for every operand, storage for trans_doubles, bind, the two
// tables into the call's PackedUpload, launch_copies ahead of the first GEMM.
struct OperandUses {
    std::map<std::tuple<int, int32_t, uint64_t>, std::vector<UCell>> uses;
    std::vector<CopyTask> copies;
    std::vector<CopyTile> copy_tiles;
    int64_t trans_doubles = 0;
    static uint64_t bits_of(double coeff) { uint64_t bits; memcpy(&bits, &coeff, sizeof bits); return bits; }      // a coefficient as a map key
    // cells: the normalised cells of operator `op` of `side`
    dmrgx_status use_of(const char* fn, int side, int32_t op, double coeff, const std::vector<NCell>& cells, const std::vector<UCell>** out)
    {
        auto ins = uses.emplace(std::make_tuple(side, op, bits_of(coeff)), std::vector<UCell>());
        *out = &ins.first->second;
        if (!ins.second) return DMRGX_OK;
        const bool is_left = side == SIDE_LEFT;
        for (const NCell& c : cells) {
            UCell u{c.q, c.r0, c.c0, c.nr, c.nc, c.kind, c.scale * coeff, c.data, 0, -1};
            if (c.kind == DMRGX_CELL_DENSE) {
                if (c.ld > INT32_MAX) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: %s operator %d: leading dimension %lld of a cell too large", fn, is_left ? "left" : "right", op, (long long)c.ld);
                u.ld = (int32_t)c.ld;
                const bool flip = c.tr == is_left;      // left and stored transposed, or right and stored plainly
                if (flip || coeff != 1.0) {
                    const int32_t dr = is_left ? c.nr : c.nc, dc = is_left ? c.nc : c.nr;
                    copies.push_back(CopyTask{trans_doubles, c.data, c.ld, dr, dc, dc, flip ? 1 : 0, coeff, 0});
                    for (int32_t ti = 0; ti < (dr + 31) / 32; ++ti)
                        for (int32_t tj = 0; tj < (dc + 31) / 32; ++tj) copy_tiles.push_back(CopyTile{(int32_t)copies.size() - 1, ti, tj, 0});
                    u.trans_off = trans_doubles;
                    u.ld = dc;
                    trans_doubles += (int64_t)dr * dc;
                }
            }
            ins.first->second.push_back(u);
        }
        return DMRGX_OK;
    }
    void bind(double* trans) { for (auto& kv : uses) for (UCell& u : kv.second) if (u.trans_off >= 0) u.data = trans + u.trans_off; }
    dmrgx_status launch_copies(const DevBuf& tab, size_t o_tiles, size_t o_tasks, double* trans, hipStream_t st) const
    {
        if (copy_tiles.empty()) return DMRGX_OK;
        hipLaunchKernelGGL(cell_copy_kernel, dim3((unsigned)copy_tiles.size()), dim3(256), 0, st, (const CopyTile*)packed_at<CopyTile>(tab, o_tiles),
                           (const CopyTask*)packed_at<CopyTask>(tab, o_tasks), trans);
        DMRGX_HIP(hipGetLastError());
        return DMRGX_OK;
    }
};

// The groups of one output block Y (nLa x nRb, leading dimension ldc): the rows are cut at the borders of the left-kind cells, the columns
// at the borders of the right-kind cells, and every rectangle of that grid is one group -- scaled copies first, then the GEMM products --
// of the cells that reach it.  A rectangle that no cell reaches is a group without products: zeros.  With contributions of one kind only
// the grid is a list of row (column) segments.
// (the cells of the contributions that live in the block's row sector are picked once per block, as the segments are walked per rectangle)
struct CellHit { const UCell* u; const double* S; int32_t lds; };
struct EmitScratch { std::vector<int32_t> rcuts, ccuts; std::vector<CellHit> lhit, rhit; };
void emit_groups(GemmBatch& gb, GemmSet& set, double* Y, int32_t ldc, int32_t nLa, int32_t nRb, int32_t a, int32_t b,
                 const std::vector<ImgContrib>& lefts, const std::vector<ImgContrib>& rights, EmitScratch& w)
{
    w.rcuts.assign({0, nLa});
    w.ccuts.assign({0, nRb});
    w.lhit.clear(); w.rhit.clear();
    for (const ImgContrib& c : lefts) for (const UCell& u : *c.cells) if (u.q == a) { w.lhit.push_back(CellHit{&u, c.S, c.lds}); w.rcuts.push_back(u.r0); w.rcuts.push_back(u.r0 + u.nr); }
    for (const ImgContrib& c : rights) for (const UCell& u : *c.cells) if (u.q == b) { w.rhit.push_back(CellHit{&u, c.S, c.lds}); w.ccuts.push_back(u.r0); w.ccuts.push_back(u.r0 + u.nr); }
    for (std::vector<int32_t>* cuts : {&w.rcuts, &w.ccuts}) { std::sort(cuts->begin(), cuts->end()); cuts->erase(std::unique(cuts->begin(), cuts->end()), cuts->end()); }
    for (size_t s = 0; s + 1 < w.rcuts.size(); ++s)
        for (size_t t = 0; t + 1 < w.ccuts.size(); ++t) {
            const int32_t p = w.rcuts[s], e = w.rcuts[s + 1], p2 = w.ccuts[t], e2 = w.ccuts[t + 1];
            const int32_t pb = (int32_t)gb.prods.size();
            int32_t cost = 0, n_axpy = 0;
            for (int pass = 0; pass < 2; ++pass) {              // scaled copies first, then the GEMM products
                for (const CellHit& h : w.lhit) {
                    const UCell& u = *h.u;
                    if (u.r0 > p || u.r0 + u.nr < e || (u.kind == DMRGX_CELL_IDENT) != (pass == 0)) continue;
                    const int32_t d = p - u.r0;
                    if (u.kind == DMRGX_CELL_IDENT) {
                        gb.prods.push_back(GProd{nullptr, h.S + (int64_t)(u.c0 + d) * h.lds + p2, 0, h.lds, 0, GPROD_AXPY, u.scale});
                        ++n_axpy; ++cost;
                    } else {
                        gb.prods.push_back(GProd{u.data + (int64_t)d * u.ld, h.S + (int64_t)u.c0 * h.lds + p2, u.ld, h.lds, u.nc, GPROD_GEMM, 1.0});
                        cost += ggemm_ksteps(u.nc);
                    }
                }
                for (const CellHit& h : w.rhit) {
                    const UCell& u = *h.u;
                    if (u.r0 > p2 || u.r0 + u.nr < e2 || (u.kind == DMRGX_CELL_IDENT) != (pass == 0)) continue;
                    const int32_t d = p2 - u.r0;
                    if (u.kind == DMRGX_CELL_IDENT) {
                        gb.prods.push_back(GProd{nullptr, h.S + (int64_t)p * h.lds + u.c0 + d, 0, h.lds, 0, GPROD_AXPY, u.scale});
                        ++n_axpy; ++cost;
                    } else {
                        gb.prods.push_back(GProd{h.S + (int64_t)p * h.lds + u.c0, u.data + d, h.lds, u.ld, u.nc, GPROD_GEMM, 1.0});
                        cost += ggemm_ksteps(u.nc);
                    }
                }
            }
            gb.group(set, GGroup{Y + (int64_t)p * ldc + p2, ldc, e - p, e2 - p2, pb, (int32_t)gb.prods.size(), n_axpy, 0}, std::max(cost, 1));
        }
}

// The builder behind dmrgx_kron_term_gram and dmrgx_kron_term_apply.  `fn` names the caller in messages.
// Output mode (Y_dev != nullptr, dmrgx_kron_term_apply and _apply_to): the images themselves are the result.  The image blocks are then
// the KronBlocks of the output list Out (a second layout over the same sector tables, never null with Y_dev; dmrgx_kron_term_apply passes L itself) at their
// offsets in its reference layout, all in one slice whose "workspace" is the caller's Y (vector stride ldy), and no Gram matrix is
// taken; the sources are looked up in L, and the groups, products and cell copies are emitted exactly as for the Gram matrix.
// Several states (nstates > 1, dmrgx_kron_term_gram_states; never with Y_dev): psi_dev holds nstates rows of stride ldpsi, and the family is
// the nstates * nvec images in state-major order, member s * nvec + v built from row s.  The image blocks of a slice hold the whole family;
// within a slice the states are built one after another, each with its own pair of GEMM sets launched in stream order, so that the
// intermediates T of the two-sided terms are those of one state at a time and the scratch does not grow with nstates.  The operand copies
// are made once.  With (nstates, ldpsi) = (1, 0) every table and launch is what it was before there were states.
dmrgx_status term_gram_build(const char* fn, const GramLayout& L, const double* psi_dev, int32_t nstates, int64_t ldpsi,
                             int32_t n_left_ops, const dmrgx_secop* left_ops, int32_t n_right_ops, const dmrgx_secop* right_ops,
                             int32_t nvec, const int32_t* vec_first, const dmrgx_term* terms,
                             size_t workspace_bytes, double* G_dev, int64_t ldg, dmrgx_gram_report* report, hipStream_t st,
                             double* Y_dev = nullptr, int64_t ldy = 0, const GramLayout* Out = nullptr)
{
    const dmrgx_sectors& SL = *L.SL;
    const dmrgx_sectors& SR = *L.SR;
    const int32_t nterms = vec_first[nvec];
    const int64_t nfam = (int64_t)nstates * nvec;     // the vectors an image block holds
    auto shift_l = [&](const dmrgx_term& t) { return t.left_op < 0 ? 0 : left_ops[t.left_op].shift; };
    auto shift_r = [&](const dmrgx_term& t) { return t.right_op < 0 ? 0 : right_ops[t.right_op].shift; };
    std::vector<std::vector<NCell>> cellsL((size_t)n_left_ops), cellsR((size_t)n_right_ops);
    {
        const std::string wl = std::string(fn) + " left op", wr = std::string(fn) + " right op";
        for (int32_t i = 0; i < n_left_ops; ++i) DMRGX_CHK(normalise_op(&left_ops[i], SL, wl.c_str(), cellsL[i]));
        for (int32_t i = 0; i < n_right_ops; ++i) DMRGX_CHK(normalise_op(&right_ops[i], SR, wr.c_str(), cellsR[i]));
    }

    // image blocks: in KronBlock order, and for each KronBlock in the order the (left, right) shift pairs first appear among the terms
    std::vector<std::pair<int32_t, int32_t>> pairs;
    for (int32_t t = 0; t < nterms; ++t) {
        const auto p = std::make_pair(shift_l(terms[t]), shift_r(terms[t]));
        if (std::find(pairs.begin(), pairs.end(), p) == pairs.end()) pairs.push_back(p);
    }
    std::vector<ImgBlock> imgs;
    std::map<std::pair<int32_t, int32_t>, int32_t> imap;
    std::vector<int64_t> slice_len;
    for (int32_t k = 0; k < L.nblocks; ++k) {
        for (const auto& p : pairs) {
            const int32_t a = L.il[k] - p.first, b = L.ir[k] - p.second;
            if (a < 0 || a >= SL.nsec || b < 0 || b >= SR.nsec) continue;
            if (Y_dev && !Out->kmap.count(std::make_pair(a, b)))
                DMRGX_FAIL(DMRGX_ERR_ARG, "%s: shifts (%d,%d) map KronBlock %d = (%d,%d) to the sector pair (%d,%d), which is not one of the %sKronBlocks", fn, p.first, p.second, k, L.il[k], L.ir[k], a, b, Out == &L ? "" : "output ");
            if (!Y_dev && imap.emplace(std::make_pair(a, b), (int32_t)imgs.size()).second) imgs.push_back(ImgBlock{a, b, (int64_t)SL.size[a] * SR.size[b], 0, 0});
        }
    }
    // output mode: every KronBlock of the output list is an image block where its layout has it, reached or not
    if (Y_dev)
        for (int32_t k = 0; k < Out->nblocks; ++k) imgs.push_back(ImgBlock{Out->il[k], Out->ir[k], Out->ref_off[k + 1] - Out->ref_off[k], Out->ref_off[k], 0});
    if (Y_dev) slice_len.assign(1, ldy);              // one slice: the caller's vectors, stride ldy
    // slices of image blocks that fit the workspace
    const int64_t bound = (int64_t)((workspace_bytes ? workspace_bytes : ((size_t)1 << 30)) / sizeof(double)) / nfam;
    for (ImgBlock& im : imgs) {
        if (Y_dev) break;
        if (im.size > bound)
            DMRGX_FAIL(DMRGX_ERR_ARG, "%s: image block (%d,%d) of %d x %d needs %lld bytes for the %lld vectors, workspace_bytes allows %lld",
                       fn, im.a, im.b, SL.size[im.a], SR.size[im.b], (long long)(im.size * nfam * (int64_t)sizeof(double)), (long long)nfam, (long long)(bound * nfam * (int64_t)sizeof(double)));
        if (slice_len.empty() || slice_len.back() + im.size > bound) slice_len.push_back(0);
        im.slice = (int32_t)slice_len.size() - 1;
        im.off = slice_len.back();
        slice_len.back() += im.size;
    }
    const int32_t nslices = (int32_t)slice_len.size();
    if (nslices == 0) {                               // no shifted sector pair exists: every image is zero
        DMRGX_CHK(dmrgx_vec_gram((int32_t)nfam, (int32_t)nfam, 0, nullptr, 0, nullptr, 0, G_dev, ldg, 0, report, st));
        return DMRGX_OK;
    }
    // the source KronBlock of term t in image block im (-1: none)
    auto source = [&](const dmrgx_term& t, const ImgBlock& im) -> int32_t {
        auto it = L.kmap.find(std::make_pair(im.a + shift_l(t), im.b + shift_r(t)));
        return it == L.kmap.end() ? -1 : it->second;
    };

    // Operands: one entry per (side, operator, coefficient) in use.
    OperandUses ou;
    auto bits_of = OperandUses::bits_of;
    auto use_of = [&](int side, int32_t op, double coeff, const std::vector<UCell>** out) { return ou.use_of(fn, side, op, coeff, (side == SIDE_LEFT ? cellsL : cellsR)[op], out); };
    // identity (x) identity: one scaled-identity cell per left sector, per coefficient
    std::map<uint64_t, std::vector<UCell>> ident_uses;
    auto ident_of = [&](double coeff) -> const std::vector<UCell>* {
        auto ins = ident_uses.emplace(bits_of(coeff), std::vector<UCell>());
        if (ins.second) for (int32_t q = 0; q < SL.nsec; ++q) ins.first->second.push_back(UCell{q, 0, 0, SL.size[q], SL.size[q], DMRGX_CELL_IDENT, coeff, nullptr, 0, -1});
        return &ins.first->second;
    };
    // per term: the cells of its left factor (coefficient included) and, for a two-sided term, of its right factor
    struct TermUse { const std::vector<UCell>* left; const std::vector<UCell>* right; };
    std::vector<TermUse> tuse((size_t)nterms, TermUse{nullptr, nullptr});
    for (int32_t t = 0; t < nterms; ++t) {
        const dmrgx_term& T = terms[t];
        if (T.left_op >= 0) DMRGX_CHK(use_of(SIDE_LEFT, T.left_op, T.a, &tuse[t].left));
        if (T.right_op >= 0) DMRGX_CHK(use_of(SIDE_RIGHT, T.right_op, T.left_op >= 0 ? 1.0 : T.a, &tuse[t].right));
        if (T.left_op < 0 && T.right_op < 0) tuse[t].left = ident_of(T.a);
    }
    // intermediates T = X_k B^T of the two-sided terms, one per (slice, right operator, source KronBlock): n_L(IL_k) x n_R(IR_k - shift)
    std::map<std::tuple<int32_t, int32_t, int32_t>, int64_t> toff;
    std::vector<int64_t> scratch_len((size_t)nslices, 0);
    for (const ImgBlock& im : imgs)
        for (int32_t t = 0; t < nterms; ++t) {
            const dmrgx_term& T = terms[t];
            if (T.left_op < 0 || T.right_op < 0) continue;
            const int32_t k = source(T, im);
            if (k < 0) continue;
            if (toff.emplace(std::make_tuple(im.slice, T.right_op, k), scratch_len[im.slice]).second)
                scratch_len[im.slice] += (int64_t)SL.size[L.il[k]] * SR.size[im.b];
        }

    DevBuf W, trans, scratch, tab;
    if (Y_dev) W.view(Y_dev, (size_t)((nvec - 1) * ldy + Out->ref_off[Out->nblocks]) * sizeof(double));
    else DMRGX_CHK(W.alloc_f64((size_t)(*std::max_element(slice_len.begin(), slice_len.end())) * (size_t)nfam, st));
    if (ou.trans_doubles > 0) DMRGX_CHK(trans.alloc_f64((size_t)ou.trans_doubles, st));
    const int64_t scratch_max = *std::max_element(scratch_len.begin(), scratch_len.end());
    if (scratch_max > 0) DMRGX_CHK(scratch.alloc_f64((size_t)scratch_max, st));
    ou.bind(trans.as<double>());

    GemmBatch gb;
    std::vector<GemmSet> sets1((size_t)nslices * nstates), sets2((size_t)nslices * nstates);      // per (slice, state) -- stage 1: the intermediates; stage 2: the images
    EmitScratch emit;
    std::vector<ImgContrib> lefts, rights;
    for (int32_t s = 0; s < nstates; ++s) {
        const double* psi = psi_dev + (int64_t)s * ldpsi;
        for (const auto& kv : toff) {                              // (ordered by slice, right operator, KronBlock)
            const int32_t sl = std::get<0>(kv.first), r = std::get<1>(kv.first), k = std::get<2>(kv.first);
            const int32_t nl = SL.size[L.il[k]], b = L.ir[k] - right_ops[r].shift, ldx = SR.size[L.ir[k]];
            lefts.clear();
            rights.assign(1, ImgContrib{&ou.uses.at(std::make_tuple((int)SIDE_RIGHT, r, bits_of(1.0))), psi + L.ref_off[k], ldx});
            emit_groups(gb, sets1[(size_t)sl * nstates + s], scratch.as<double>() + kv.second, SR.size[b], nl, SR.size[b], -1, b, lefts, rights, emit);
        }
    }
    for (int32_t s = 0; s < nstates; ++s) {
        const double* psi = psi_dev + (int64_t)s * ldpsi;
        for (const ImgBlock& im : imgs) {
            const int32_t nLa = SL.size[im.a], nRb = SR.size[im.b];
            const int64_t ldw = slice_len[im.slice];
            for (int32_t v = 0; v < nvec; ++v) {
                lefts.clear(); rights.clear();
                for (int32_t t = vec_first[v]; t < vec_first[v + 1]; ++t) {
                    const dmrgx_term& T = terms[t];
                    const int32_t k = source(T, im);
                    if (k < 0) continue;
                    if (T.left_op >= 0 && T.right_op >= 0) lefts.push_back(ImgContrib{tuse[t].left, scratch.as<double>() + toff.at(std::make_tuple(im.slice, T.right_op, k)), nRb});
                    else if (T.right_op >= 0) rights.push_back(ImgContrib{tuse[t].right, psi + L.ref_off[k], SR.size[L.ir[k]]});
                    else lefts.push_back(ImgContrib{tuse[t].left, psi + L.ref_off[k], nRb});
                }
                emit_groups(gb, sets2[(size_t)im.slice * nstates + s], W.as<double>() + ((int64_t)s * nvec + v) * ldw + im.off, nRb, nLa, nRb, im.a, im.b, lefts, rights, emit);
            }
        }
    }
    PackedUpload pk;
    gb.pack(pk);
    for (GemmSet& s : sets1) gb.pack(s, pk);
    for (GemmSet& s : sets2) gb.pack(s, pk);
    const size_t o_tasks = pk.add(ou.copies), o_tiles = pk.add(ou.copy_tiles);
    DMRGX_CHK(pk.upload(tab, st));
    gb.bind(tab);
    DMRGX_CHK(ou.launch_copies(tab, o_tiles, o_tasks, trans.as<double>(), st));
    dmrgx_gram_report total{0, nslices, 0};
    for (int32_t s = 0; s < nslices; ++s) {               // fixed order: slice s is added to the sum of the slices before it
        for (int32_t j = 0; j < nstates; ++j) {           // state j's images read its T: stream order keeps the next state's T behind them
            DMRGX_CHK(gb.launch(sets1[(size_t)s * nstates + j], tab, st));
            DMRGX_CHK(gb.launch(sets2[(size_t)s * nstates + j], tab, st));
        }
        if (Y_dev) continue;
        dmrgx_gram_report r{};
        DMRGX_CHK(dmrgx_vec_gram((int32_t)nfam, (int32_t)nfam, slice_len[s], W.as<double>(), slice_len[s], W.as<double>(), slice_len[s], G_dev, ldg, s > 0 ? 1 : 0, &r, st));
        total.tiles = r.tiles;
        total.slab_doubles = std::max(total.slab_doubles, r.slab_doubles);
    }
    if (report) *report = total;
    return DMRGX_OK;
}
}  // namespace

// The checks dmrgx_kron_term_gram and dmrgx_kron_term_apply share: operator lists, vectors, term indices, one total shift (-> *shift_out).
static dmrgx_status term_list_check(const char* fn, int32_t n_left_ops, const dmrgx_secop* left_ops, int32_t n_right_ops, const dmrgx_secop* right_ops,
                                    int32_t nvec, const int32_t* vec_first, const dmrgx_term* terms, int32_t* shift_out)
{
    if (n_left_ops < 0 || n_right_ops < 0 || (n_left_ops > 0 && !left_ops) || (n_right_ops > 0 && !right_ops))
        DMRGX_FAIL(DMRGX_ERR_ARG, "%s: bad operator lists (%d left, %d right)", fn, n_left_ops, n_right_ops);
    if (nvec < 1 || !vec_first || vec_first[0] != 0) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: no vectors, or vec_first does not start at 0", fn);
    for (int32_t v = 0; v < nvec; ++v)
        if (vec_first[v + 1] <= vec_first[v]) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: vector %d is empty (vec_first %d, %d): every vector has at least one term", fn, v, vec_first[v], vec_first[v + 1]);
    if (!terms) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: null term list", fn);
    int32_t shift = 0;
    for (int32_t v = 0; v < nvec; ++v)
        for (int32_t t = vec_first[v]; t < vec_first[v + 1]; ++t) {
            const dmrgx_term& T = terms[t];
            if (T.left_op < -1 || T.left_op >= n_left_ops || T.right_op < -1 || T.right_op >= n_right_ops)
                DMRGX_FAIL(DMRGX_ERR_OUTOFRANGE, "%s: term %d of vector %d references operator (%d,%d) outside the %d left and %d right operators", fn, t - vec_first[v], v, T.left_op, T.right_op, n_left_ops, n_right_ops);
            const int32_t s = (T.left_op < 0 ? 0 : left_ops[T.left_op].shift) + (T.right_op < 0 ? 0 : right_ops[T.right_op].shift);
            if (t == 0) shift = s;
            else if (s != shift) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: term %d of vector %d has total shift %d, the first term has %d: one call takes one shift", fn, t - vec_first[v], v, s, shift);
        }
    *shift_out = shift;
    return DMRGX_OK;
}

extern "C" dmrgx_status dmrgx_kron_term_gram(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks,
                                             const int32_t* block_il, const int32_t* block_ir, const double* psi_dev,
                                             int32_t n_left_ops, const dmrgx_secop* left_ops, int32_t n_right_ops, const dmrgx_secop* right_ops,
                                             int32_t nvec, const int32_t* vec_first, const dmrgx_term* terms,
                                             size_t workspace_bytes, double* G_dev, int64_t ldg, dmrgx_gram_report* report, void* stream)
{
    const char* fn = "kron_term_gram";
    GramLayout L;
    DMRGX_CHK(gram_layout(fn, left, right, nblocks, block_il, block_ir, psi_dev, L));
    int32_t shift = 0;
    DMRGX_CHK(term_list_check(fn, n_left_ops, left_ops, n_right_ops, right_ops, nvec, vec_first, terms, &shift));
    if (!G_dev || ldg < nvec) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: null G or ldg %lld below the %d vectors", fn, (long long)ldg, nvec);
    return term_gram_build(fn, L, psi_dev, 1, 0, n_left_ops, left_ops, n_right_ops, right_ops, nvec, vec_first, terms, workspace_bytes, G_dev, ldg, report, (hipStream_t)stream);
}

// dmrgx_kron_term_gram_states: the Gram matrix of the images of several states, state-major (the builder's multi-state path).
extern "C" dmrgx_status dmrgx_kron_term_gram_states(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks,
                                                    const int32_t* block_il, const int32_t* block_ir,
                                                    int32_t nstates, const double* Psi_dev, int64_t ldpsi,
                                                    int32_t n_left_ops, const dmrgx_secop* left_ops, int32_t n_right_ops, const dmrgx_secop* right_ops,
                                                    int32_t nvec, const int32_t* vec_first, const dmrgx_term* terms,
                                                    size_t workspace_bytes, double* G_dev, int64_t ldg, dmrgx_gram_report* report, void* stream)
{
    const char* fn = "kron_term_gram_states";
    GramLayout L;
    if (nstates < 1) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: nstates %d: at least one state", fn, nstates);
    DMRGX_CHK(gram_layout(fn, left, right, nblocks, block_il, block_ir, Psi_dev, L));
    if (ldpsi < L.ref_off[nblocks]) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: ldpsi %lld below the %lld states of a row", fn, (long long)ldpsi, (long long)L.ref_off[nblocks]);
    int32_t shift = 0;
    DMRGX_CHK(term_list_check(fn, n_left_ops, left_ops, n_right_ops, right_ops, nvec, vec_first, terms, &shift));
    if ((int64_t)nstates * nvec > INT32_MAX) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: %d states x %d vectors: too many", fn, nstates, nvec);
    if (!G_dev || ldg < (int64_t)nstates * nvec) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: null G or ldg %lld below the %d x %d vectors", fn, (long long)ldg, nstates, nvec);
    return term_gram_build(fn, L, Psi_dev, nstates, ldpsi, n_left_ops, left_ops, n_right_ops, right_ops, nvec, vec_first, terms, workspace_bytes, G_dev, ldg, report, (hipStream_t)stream);
}

// dmrgx_kron_term_apply: the images themselves, written once each into the caller's Y (the builder's output mode).
extern "C" dmrgx_status dmrgx_kron_term_apply(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks,
                                              const int32_t* block_il, const int32_t* block_ir, const double* psi_dev,
                                              int32_t n_left_ops, const dmrgx_secop* left_ops, int32_t n_right_ops, const dmrgx_secop* right_ops,
                                              int32_t nvec, const int32_t* vec_first, const dmrgx_term* terms,
                                              double* Y_dev, int64_t ldy, void* stream)
{
    const char* fn = "kron_term_apply";
    GramLayout L;
    DMRGX_CHK(gram_layout(fn, left, right, nblocks, block_il, block_ir, psi_dev, L));
    int32_t shift = 0;
    DMRGX_CHK(term_list_check(fn, n_left_ops, left_ops, n_right_ops, right_ops, nvec, vec_first, terms, &shift));
    if (shift != 0) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: the terms have total shift %d: an image in the layout of psi needs total shift 0", fn, shift);
    const int64_t N = L.ref_off[nblocks];
    if (!Y_dev || ldy < N) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: null Y or ldy %lld below the %lld states", fn, (long long)ldy, (long long)N);
    if (Y_dev < psi_dev + N && psi_dev < Y_dev + (int64_t)(nvec - 1) * ldy + N) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: Y overlaps psi", fn);
    return term_gram_build(fn, L, psi_dev, 1, 0, n_left_ops, left_ops, n_right_ops, right_ops, nvec, vec_first, terms, 0, nullptr, 0, nullptr, (hipStream_t)stream, Y_dev, ldy, &L);      // output list == input list
}

// dmrgx_kron_term_apply_to: the same images written in the layout of a second KronBlock list (the sector the total shift leads to).
extern "C" dmrgx_status dmrgx_kron_term_apply_to(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks,
                                                 const int32_t* block_il, const int32_t* block_ir, const double* psi_dev,
                                                 int32_t n_left_ops, const dmrgx_secop* left_ops, int32_t n_right_ops, const dmrgx_secop* right_ops,
                                                 int32_t nvec, const int32_t* vec_first, const dmrgx_term* terms,
                                                 int32_t n_out, const int32_t* out_il, const int32_t* out_ir,
                                                 double* Y_dev, int64_t ldy, void* stream)
{
    const char* fn = "kron_term_apply_to";
    GramLayout L, O;
    DMRGX_CHK(gram_layout(fn, left, right, nblocks, block_il, block_ir, psi_dev, L));
    int32_t shift = 0;
    DMRGX_CHK(term_list_check(fn, n_left_ops, left_ops, n_right_ops, right_ops, nvec, vec_first, terms, &shift));
    if (n_out < 0 || (n_out > 0 && (!out_il || !out_ir))) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: bad output KronBlock list (%d blocks)", fn, n_out);
    if (n_out == 0) return DMRGX_OK;
    DMRGX_CHK(block_layout(fn, "output KronBlock", left, right, n_out, out_il, out_ir, O));
    const int64_t N = L.ref_off[nblocks], NO = O.ref_off[n_out];
    if (!Y_dev || ldy < NO) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: null Y or ldy %lld below the %lld output states", fn, (long long)ldy, (long long)NO);
    if (Y_dev < psi_dev + N && psi_dev < Y_dev + (int64_t)(nvec - 1) * ldy + NO) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: Y overlaps psi", fn);
    return term_gram_build(fn, L, psi_dev, 1, 0, n_left_ops, left_ops, n_right_ops, right_ops, nvec, vec_first, terms, 0, nullptr, 0, nullptr, (hipStream_t)stream, Y_dev, ldy, &O);
}

// dmrgx_kron_noise_expand: psi with the images c_a A_a psi of one side's operators set beside it (side 0: as further columns of the
// KronBlock they land in, side 1: as further rows), so that the density matrix of the expansion is White's perturbed one
//   rho'_q = Psi_q Psi_q^T + sum_a c_a^2 sum_k' (A_a Psi_k')(A_a Psi_k')^T        (PRB 72, 180403)
// and the density-matrix solver needs nothing but wider sector tables.  Every panel is one emit_groups call of the term builder -- the
// products and scaled copies of a one-sided term -- with the panel's corner as the output and the expanded leading dimension; the
// coefficient goes into the materialised operand (OperandUses), a zero coefficient makes its panels groups without products.  The
// Psi_k parts are strided device copies: bit for bit.
extern "C" dmrgx_status dmrgx_kron_noise_expand(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks,
                                                const int32_t* block_il, const int32_t* block_ir, const double* psi_dev,
                                                int32_t side, int32_t n_ops, const dmrgx_secop* ops, const double* coef,
                                                int32_t* extent, int64_t* n_out, double* Y_dev, void* stream)
{
    const char* fn = "kron_noise_expand";
    hipStream_t st = (hipStream_t)stream;
    if (side != 0 && side != 1) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: side %d is neither 0 (columns, for rho_L) nor 1 (rows, for rho_R)", fn, side);
    if (n_ops < 0 || (n_ops > 0 && (!ops || !coef))) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: bad operator list (%d operators)", fn, n_ops);
    if (!extent || !n_out) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: null extent or n_out", fn);
    if (Y_dev && !psi_dev) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: null psi", fn);
    GramLayout L;
    DMRGX_CHK(kron_layout(fn, left, right, nblocks, block_il, block_ir, L));
    const dmrgx_sectors& SL = *left;
    const dmrgx_sectors& SR = *right;
    const dmrgx_sectors& SS = side == 0 ? SL : SR;                      // the table the operators live on
    const int32_t* sec_of = side == 0 ? block_il : block_ir;           // a KronBlock's sector on that side
    std::vector<std::vector<NCell>> cells((size_t)n_ops);
    for (int32_t a = 0; a < n_ops; ++a) {
        if (!std::isfinite(coef[a])) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: coefficient %d is not finite", fn, a);
        DMRGX_CHK(normalise_op(&ops[a], SS, side == 0 ? "kron_noise_expand left op" : "kron_noise_expand right op", cells[a]));
    }
    // the panels of every output block: (operator, source KronBlock), operators ascending, sources ascending
    // fixed dimension of block k: n_L(IL_k) rows on side 0, n_R(IR_k) columns on side 1; the expanded one starts with psi's own
    struct Panel { int32_t a, src, at; };                               // at: first column (row) of the panel in its block
    std::vector<std::vector<Panel>> panels((size_t)nblocks);
    std::vector<int64_t> out_off((size_t)nblocks + 1, 0);
    for (int32_t k = 0; k < nblocks; ++k) {
        int64_t ext = side == 0 ? SR.size[block_ir[k]] : SL.size[block_il[k]];
        for (int32_t a = 0; a < n_ops; ++a)
            for (int32_t s = 0; s < nblocks; ++s) {
                if (sec_of[s] - ops[a].shift != sec_of[k]) continue;
                panels[k].push_back(Panel{a, s, (int32_t)ext});
                ext += side == 0 ? SR.size[block_ir[s]] : SL.size[block_il[s]];
                if (ext > INT32_MAX) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: the expansion of KronBlock %d is wider than 2^31 - 1", fn, k);
            }
        extent[k] = (int32_t)ext;
        out_off[k + 1] = out_off[k] + ext * (side == 0 ? SL.size[block_il[k]] : SR.size[block_ir[k]]);
    }
    *n_out = out_off[nblocks];
    if (!Y_dev) return DMRGX_OK;                                        // sizes only: no device call so far
    const int64_t N = L.ref_off[nblocks];
    if (Y_dev < psi_dev + N && psi_dev < Y_dev + *n_out) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: Y overlaps psi", fn);

    OperandUses ou;
    std::vector<const std::vector<UCell>*> use((size_t)n_ops, nullptr);
    for (int32_t k = 0; k < nblocks; ++k)
        for (const Panel& p : panels[k])
            if (coef[p.a] != 0.0 && !use[p.a]) DMRGX_CHK(ou.use_of(fn, side, p.a, coef[p.a], cells[p.a], &use[p.a]));
    DevBuf trans, tab;
    if (ou.trans_doubles > 0) DMRGX_CHK(trans.alloc_f64((size_t)ou.trans_doubles, st));
    ou.bind(trans.as<double>());

    GemmBatch gb;
    GemmSet set;
    EmitScratch emit;
    std::vector<ImgContrib> lefts, rights;
    for (int32_t k = 0; k < nblocks; ++k) {
        const int32_t nl = SL.size[block_il[k]], nr = SR.size[block_ir[k]];
        double* Yk = Y_dev + out_off[k];
        const int32_t ldc = side == 0 ? extent[k] : nr;
        // psi's own block: the leading columns (side 0) or rows (side 1)
        DMRGX_HIP(hipMemcpy2DAsync(Yk, (size_t)ldc * sizeof(double), psi_dev + L.ref_off[k], (size_t)nr * sizeof(double), (size_t)nr * sizeof(double), (size_t)nl,
                                   hipMemcpyDeviceToDevice, st));
        for (const Panel& p : panels[k]) {
            const int32_t sl = SL.size[block_il[p.src]], sr = SR.size[block_ir[p.src]];
            double* Yp = side == 0 ? Yk + p.at : Yk + (int64_t)p.at * ldc;
            const int32_t pm = side == 0 ? nl : sl, pn = side == 0 ? sr : nr;      // the panel: A Psi_src is n_L(IL_k) x n_R(IR_src), Psi_src B^T n_L(IL_src) x n_R(IR_k)
            lefts.clear(); rights.clear();
            if (use[p.a]) (side == 0 ? lefts : rights).push_back(ImgContrib{use[p.a], psi_dev + L.ref_off[p.src], sr});
            // (without a contribution -- a zero coefficient -- the panel is one group without products: zeros)
            emit_groups(gb, set, Yp, ldc, pm, pn, side == 0 ? block_il[k] : -1, side == 0 ? -1 : block_ir[k], lefts, rights, emit);
        }
    }
    PackedUpload pk;
    gb.pack(pk);
    gb.pack(set, pk);
    const size_t o_tasks = pk.add(ou.copies), o_tiles = pk.add(ou.copy_tiles);
    DMRGX_CHK(pk.upload(tab, st));
    gb.bind(tab);
    DMRGX_CHK(ou.launch_copies(tab, o_tiles, o_tasks, trans.as<double>(), st));
    return gb.launch(set, tab, st);
}

// dmrgx_kron_op_gram: one operator per vector, A (x) 1 or 1 (x) B.  It keeps its own builder: the same image blocks, groups and products
// as one one-sided term per vector gives above (the shared parts are normalise_op, the cell copies, GemmBatch and dmrgx_vec_gram), with
// the cells of an operator picked per image block before its segments are walked.
namespace {
struct OpUCell { int32_t r0, c0, nr, nc, kind; double scale; const double* data; int32_t ld; int64_t trans_off; };      // data: row-major in the shape the NN GEMM reads; trans_off >= 0: materialised there
struct OpImgBlock { int32_t a, b, src_left, src_right; int64_t size, off; int32_t slice; };
}  // namespace

extern "C" dmrgx_status dmrgx_kron_op_gram(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks,
                                           const int32_t* block_il, const int32_t* block_ir, const double* psi_dev,
                                           int32_t n_left_ops, const dmrgx_secop* left_ops, int32_t n_right_ops, const dmrgx_secop* right_ops,
                                           size_t workspace_bytes, double* G_dev, int64_t ldg, dmrgx_gram_report* report, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!left || !right || left->nsec <= 0 || right->nsec <= 0 || !left->size || !right->size) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_op_gram: empty sector table");
    const dmrgx_sectors& SL = *left;
    const dmrgx_sectors& SR = *right;
    for (int i = 0; i < SL.nsec; ++i) if (SL.size[i] <= 0) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_op_gram: left sector %d has size %d", i, SL.size[i]);
    for (int i = 0; i < SR.nsec; ++i) if (SR.size[i] <= 0) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_op_gram: right sector %d has size %d", i, SR.size[i]);
    if (nblocks <= 0 || !block_il || !block_ir) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_op_gram: no KronBlocks");
    if (!psi_dev) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_op_gram: null psi");
    if (n_left_ops < 0 || n_right_ops < 0 || n_left_ops + n_right_ops < 1 || (n_left_ops > 0 && !left_ops) || (n_right_ops > 0 && !right_ops))
        DMRGX_FAIL(DMRGX_ERR_ARG, "kron_op_gram: bad operator lists (%d left, %d right)", n_left_ops, n_right_ops);
    const int32_t nops = n_left_ops + n_right_ops;
    if (!G_dev || ldg < nops) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_op_gram: null G or ldg %lld below the %d operators", (long long)ldg, nops);
    std::map<std::pair<int32_t, int32_t>, int32_t> kmap;
    std::vector<int64_t> ref_off(nblocks + 1, 0);
    for (int32_t k = 0; k < nblocks; ++k) {
        const int32_t il = block_il[k], ir = block_ir[k];
        if (il < 0 || il >= SL.nsec || ir < 0 || ir >= SR.nsec) DMRGX_FAIL(DMRGX_ERR_OUTOFRANGE, "kron_op_gram: KronBlock %d = (%d,%d) out of range", k, il, ir);
        if (!kmap.emplace(std::make_pair(il, ir), k).second) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_op_gram: KronBlock (%d,%d) listed twice", il, ir);
        ref_off[k + 1] = ref_off[k] + (int64_t)SL.size[il] * SR.size[ir];
    }
    auto op_at = [&](int32_t v) -> const dmrgx_secop& { return v < n_left_ops ? left_ops[v] : right_ops[v - n_left_ops]; };
    const int32_t shift = op_at(0).shift;
    for (int32_t v = 1; v < nops; ++v)
        if (op_at(v).shift != shift) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_op_gram: operator %d has shift %d, operator 0 has %d: one call takes one shift", v, op_at(v).shift, shift);
    std::vector<std::vector<NCell>> cells(nops);
    for (int32_t v = 0; v < nops; ++v) DMRGX_CHK(normalise_op(&op_at(v), v < n_left_ops ? SL : SR, v < n_left_ops ? "kron_op_gram left op" : "kron_op_gram right op", cells[v]));

    // image blocks, in KronBlock order (left image, then right image of each)
    std::vector<OpImgBlock> imgs;
    std::map<std::pair<int32_t, int32_t>, int32_t> imap;
    auto image = [&](int32_t a, int32_t b) -> OpImgBlock& {
        auto it = imap.emplace(std::make_pair(a, b), (int32_t)imgs.size());
        if (it.second) imgs.push_back(OpImgBlock{a, b, -1, -1, (int64_t)SL.size[a] * SR.size[b], 0, 0});
        return imgs[it.first->second];
    };
    for (int32_t k = 0; k < nblocks; ++k) {
        const int32_t a = block_il[k] - shift, b = block_ir[k] - shift;
        if (n_left_ops > 0 && a >= 0 && a < SL.nsec) image(a, block_ir[k]).src_left = k;
        if (n_right_ops > 0 && b >= 0 && b < SR.nsec) image(block_il[k], b).src_right = k;
    }
    // slices of image blocks that fit the workspace
    const int64_t bound = (int64_t)((workspace_bytes ? workspace_bytes : ((size_t)1 << 30)) / sizeof(double)) / nops;
    std::vector<int64_t> slice_len;
    for (OpImgBlock& im : imgs) {
        if (im.size > bound)
            DMRGX_FAIL(DMRGX_ERR_ARG, "kron_op_gram: image block (%d,%d) of %d x %d needs %lld bytes for the %d operators, workspace_bytes allows %lld",
                       im.a, im.b, SL.size[im.a], SR.size[im.b], (long long)(im.size * nops * (int64_t)sizeof(double)), nops, (long long)(bound * nops * (int64_t)sizeof(double)));
        if (slice_len.empty() || slice_len.back() + im.size > bound) slice_len.push_back(0);
        im.slice = (int32_t)slice_len.size() - 1;
        im.off = slice_len.back();
        slice_len.back() += im.size;
    }
    const int32_t nslices = (int32_t)slice_len.size();
    if (nslices == 0) {                               // no shifted sector exists: every image is zero
        DMRGX_CHK(dmrgx_vec_gram(nops, nops, 0, nullptr, 0, nullptr, 0, G_dev, ldg, 0, report, stream));
        return DMRGX_OK;
    }
    DevBuf W, trans, tab;
    DMRGX_CHK(W.alloc_f64((size_t)(*std::max_element(slice_len.begin(), slice_len.end())) * nops, st));

    // the NN GEMM reads a left cell as A (row-major nr x nc) and a right cell as B = cell^T (row-major nc x nr): cells stored the other
    // way round are materialised once per call (as the plan's cell_copy writes B^T)
    std::vector<std::vector<OpUCell>> ucells(nops);
    std::vector<CopyTask> copies;
    std::vector<CopyTile> copy_tiles;
    int64_t trans_doubles = 0;
    for (int32_t v = 0; v < nops; ++v)
        for (const NCell& c : cells[v]) {
            const bool is_left = v < n_left_ops;
            OpUCell u{c.r0, c.c0, c.nr, c.nc, c.kind, c.scale, c.data, 0, -1};
            if (c.kind == DMRGX_CELL_DENSE) {
                if (c.ld > INT32_MAX) DMRGX_FAIL(DMRGX_ERR_ARG, "kron_op_gram: operator %d: leading dimension %lld of a cell too large", v, (long long)c.ld);
                u.ld = (int32_t)c.ld;
                if (c.tr == is_left) {                  // left and stored transposed, or right and stored plainly
                    const int32_t dr = is_left ? c.nr : c.nc, dc = is_left ? c.nc : c.nr;
                    copies.push_back(CopyTask{trans_doubles, c.data, c.ld, dr, dc, dc, 1, 1.0, 0});
                    for (int32_t ti = 0; ti < (dr + 31) / 32; ++ti)
                        for (int32_t tj = 0; tj < (dc + 31) / 32; ++tj) copy_tiles.push_back(CopyTile{(int32_t)copies.size() - 1, ti, tj, 0});
                    u.trans_off = trans_doubles;
                    u.ld = dc;
                    trans_doubles += (int64_t)dr * dc;
                }
            }
            ucells[v].push_back(u);
        }
    if (trans_doubles > 0) DMRGX_CHK(trans.alloc_f64((size_t)trans_doubles, st));
    for (auto& list : ucells)
        for (OpUCell& u : list)
            if (u.trans_off >= 0) u.data = trans.as<double>() + u.trans_off;

    GemmBatch gb;
    std::vector<GemmSet> sets(nslices);
    std::vector<int32_t> cuts, hit;
    for (const OpImgBlock& im : imgs) {
        const int32_t nLa = SL.size[im.a], nRb = SR.size[im.b];
        const int64_t ldw = slice_len[im.slice];
        for (int32_t v = 0; v < nops; ++v) {
            const bool is_left = v < n_left_ops;
            double* Y = W.as<double>() + (int64_t)v * ldw + im.off;
            const int32_t src = is_left ? im.src_left : im.src_right;
            const int32_t q = is_left ? im.a : im.b, n = is_left ? nLa : nRb;     // the operator's row sector and its size: the index cut in segments
            // segments of that index between the borders of the cells that reach it: every segment gets one group (no products: zeros)
            cuts.assign({0, n});
            hit.clear();
            if (src >= 0)
                for (size_t i = 0; i < cells[v].size(); ++i)
                    if (cells[v][i].q == q) { hit.push_back((int32_t)i); cuts.push_back(cells[v][i].r0); cuts.push_back(cells[v][i].r0 + cells[v][i].nr); }
            std::sort(cuts.begin(), cuts.end());
            cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
            const double* X = src >= 0 ? psi_dev + ref_off[src] : nullptr;
            const int32_t ldx = src >= 0 ? SR.size[block_ir[src]] : 0;
            for (size_t s = 0; s + 1 < cuts.size(); ++s) {
                const int32_t p = cuts[s], e = cuts[s + 1];
                const int32_t pb = (int32_t)gb.prods.size();
                int32_t cost = 0, n_axpy = 0;
                for (int pass = 0; pass < 2; ++pass)            // scaled copies first, then the GEMM products
                    for (int32_t i : hit) {
                        const OpUCell& u = ucells[v][i];
                        if (u.r0 > p || u.r0 + u.nr < e || (u.kind == DMRGX_CELL_IDENT) != (pass == 0)) continue;
                        const int32_t d = p - u.r0;
                        if (u.kind == DMRGX_CELL_IDENT) {
                            gb.prods.push_back(GProd{nullptr, is_left ? X + (int64_t)(u.c0 + d) * ldx : X + u.c0 + d, 0, ldx, 0, GPROD_AXPY, u.scale});
                            ++n_axpy; ++cost;
                        } else if (is_left) {
                            gb.prods.push_back(GProd{u.data + (int64_t)d * u.ld, X + (int64_t)u.c0 * ldx, u.ld, ldx, u.nc, GPROD_GEMM, 1.0});
                            cost += ggemm_ksteps(u.nc);
                        } else {
                            gb.prods.push_back(GProd{X + u.c0, u.data + d, ldx, u.ld, u.nc, GPROD_GEMM, 1.0});
                            cost += ggemm_ksteps(u.nc);
                        }
                    }
                const GGroup g = is_left ? GGroup{Y + (int64_t)p * nRb, nRb, e - p, nRb, pb, (int32_t)gb.prods.size(), n_axpy, 0}
                                         : GGroup{Y + p, nRb, nLa, e - p, pb, (int32_t)gb.prods.size(), n_axpy, 0};
                gb.group(sets[im.slice], g, std::max(cost, 1));
            }
        }
    }
    PackedUpload pk;
    gb.pack(pk);
    for (GemmSet& s : sets) gb.pack(s, pk);
    const size_t o_tasks = pk.add(copies), o_tiles = pk.add(copy_tiles);
    DMRGX_CHK(pk.upload(tab, st));
    gb.bind(tab);
    if (!copy_tiles.empty()) {
        hipLaunchKernelGGL(cell_copy_kernel, dim3((unsigned)copy_tiles.size()), dim3(256), 0, st, (const CopyTile*)packed_at<CopyTile>(tab, o_tiles),
                           (const CopyTask*)packed_at<CopyTask>(tab, o_tasks), trans.as<double>());
        DMRGX_HIP(hipGetLastError());
    }
    dmrgx_gram_report total{0, nslices, 0};
    for (int32_t s = 0; s < nslices; ++s) {               // fixed order: slice s is added to the sum of the slices before it
        DMRGX_CHK(gb.launch(sets[s], tab, st));
        dmrgx_gram_report r{};
        DMRGX_CHK(dmrgx_vec_gram(nops, nops, slice_len[s], W.as<double>(), slice_len[s], W.as<double>(), slice_len[s], G_dev, ldg, s > 0 ? 1 : 0, &r, stream));
        total.tiles = r.tiles;
        total.slab_doubles = std::max(total.slab_doubles, r.slab_doubles);
    }
    if (report) *report = total;
    return DMRGX_OK;
}
