// dmrgx_secop_compose: products of two and three sector operators of ONE block, summed with coefficients, as dense sector blocks.
//
//     C_o = sum over the strings t of output o of  c_t F_{t,1} F_{t,2} [F_{t,3}]
//
// An operator of shift s lives in the blocks (q -> q + s); a product of shifts s1, s2 in (q -> q + s1 + s2) through the middle sector
// q + s1.  This is what a measurement of three site operators needs from a block: S_i . (S_j x S_k) of a triangle inside a block is six
// strings of three factors, and the part of such a string on one side of the cut is a product of two (DimerFrame::BuildBondOperators
// forms the one shift-0 case S_i . S_j through the public grouped GEMM, by hand).
//
// Two grouped-GEMM passes through GemmBatch, the batch builder of every grouped GEMM outside the MatMult:
//   pass 1  the distinct prefixes (c F_1) F_2 of the three-factor strings, one dense block per row sector, into pool scratch -- distinct
//           over the whole call by (F_1, F_2, c): Sz_i Sp_j / 2 is shared by every triangle that holds the ordered pair (i, j);
//   pass 2  every sector block of every output as the groups of its strings: prefix . F_3, (c F_1) F_2, or c F_1 alone.
// The operands are cell lists, so an output block is cut at the cell borders as term_gram's emit_groups cuts an image block: rows at the
// borders of the left operands' cells, columns at those of the right operands', and where a factor is a scaled-identity cell at the
// borders of its partner pulled through the identity.  Every rectangle of that grid is one group -- scaled copies first, then the GEMM
// products -- and a rectangle nothing reaches is a group without products: zeros.  dense . dense is a GEMM product over the part of the
// middle sector both cells cover; identity . dense and dense . identity are scaled copies of the dense cell's rows / columns;
// identity . identity, and a one-factor string that is an identity cell, are scaled copies out of a unit matrix in pool scratch.
// A GEMM product carries no coefficient: c_t is folded into the first factor of its string -- into the scale of an identity cell, or into
// a materialised copy of a dense one.  Dense cells stored transposed (Sm from Sp) are materialised the same way: secop_cell_copy_kernel,
// the only device code of this file.  No atomics, fixed order: two calls give the same bits.
#include "ggemm.h"
#include <cmath>
#include <map>
#include <tuple>

namespace dmrgx {
namespace {

// dst[i*ldd + j] = a * src(i,j), i < nr, j < nc; src(i,j) = src[i*lds + j], or src[j*lds + i] when tr; src == nullptr: a * delta_ij
struct CellCopy { int64_t dst_off; const double* src; int64_t lds; int32_t nr, nc, ldd, tr; double a; };
struct CellCopyTile { int32_t task, ti, tj, pad; };

// one 32 x 32 tile per workgroup; a transposed source is read along its own rows and turned in LDS, so both sides stay coalesced
__global__ void __launch_bounds__(256)
secop_cell_copy_kernel(const CellCopyTile* __restrict__ tiles, const CellCopy* __restrict__ tasks, double* __restrict__ base)
{
    __shared__ double buf[32][33];
    const CellCopyTile t = tiles[blockIdx.x];
    const CellCopy k = tasks[t.task];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const int i0 = t.ti * 32, j0 = t.tj * 32;
    double* dst = base + k.dst_off;
    if (!k.src) {
        for (int r = ty; r < 32; r += 8) {
            const int i = i0 + r, j = j0 + tx;
            if (i < k.nr && j < k.nc) dst[(size_t)i * k.ldd + j] = i == j ? k.a : 0.0;
        }
    } else if (!k.tr) {
        for (int r = ty; r < 32; r += 8) {
            const int i = i0 + r, j = j0 + tx;
            if (i < k.nr && j < k.nc) dst[(size_t)i * k.ldd + j] = k.a * k.src[(size_t)i * k.lds + j];
        }
    } else {
        for (int r = ty; r < 32; r += 8) {
            const int j = j0 + r, i = i0 + tx;
            buf[r][tx] = (i < k.nr && j < k.nc) ? k.src[(size_t)j * k.lds + i] : 0.0;
        }
        __syncthreads();
        for (int r = ty; r < 32; r += 8) {
            const int i = i0 + r, j = j0 + tx;
            if (i < k.nr && j < k.nc) dst[(size_t)i * k.ldd + j] = k.a * buf[tx][r];
        }
    }
}

// A cell as the GEMM reads it: rows r0.., columns c0.. of the block (q -> q + shift), row-major at `data` with leading dimension ld (a
// copy in pool scratch when copy_off >= 0).  scale: of an identity cell, the string's coefficient included.
struct UCell { int32_t q, r0, c0, nr, nc, kind; double scale; const double* data; int32_t ld; int64_t copy_off; };

struct Operands {
    std::map<std::pair<int32_t, uint64_t>, std::vector<UCell>> uses;     // (operator or ~prefix, coefficient bits)
    std::vector<CellCopy> copies;
    std::vector<CellCopyTile> tiles;
    int64_t doubles = 0;
    int32_t eye = 0;                 // order of the unit matrix (0: none needed), at eye_off
    int64_t eye_off = 0;
    static uint64_t bits_of(double c) { uint64_t b; memcpy(&b, &c, sizeof b); return b; }
    void push_copy(const double* src, int64_t lds, int32_t nr, int32_t nc, int32_t tr, double a)
    {
        copies.push_back(CellCopy{doubles, src, lds, nr, nc, nc, tr, a});
        for (int32_t ti = 0; ti < (nr + 31) / 32; ++ti)
            for (int32_t tj = 0; tj < (nc + 31) / 32; ++tj) tiles.push_back(CellCopyTile{(int32_t)copies.size() - 1, ti, tj, 0});
        doubles += (int64_t)nr * nc;
    }
    // the cells of operator `op` (normalised: as used) times coeff
    const std::vector<UCell>* use_of(int32_t op, double coeff, const dmrgx_secop& so)
    {
        auto ins = uses.emplace(std::make_pair(op, bits_of(coeff)), std::vector<UCell>());
        if (!ins.second) return &ins.first->second;
        const bool tr = so.transposed != 0;
        for (int32_t i = 0; i < so.ncells; ++i) {
            const dmrgx_cell& c = so.cells[i];
            UCell u{c.row_sector, c.r0, c.c0, c.nr, c.nc, c.kind, c.scale * coeff, c.data, (int32_t)c.ld, -1};
            if (tr) { u.q -= so.shift; std::swap(u.r0, u.c0); std::swap(u.nr, u.nc); }
            if (c.kind == DMRGX_CELL_DENSE && (tr || coeff != 1.0)) {
                u.copy_off = doubles; u.ld = u.nc;
                push_copy(c.data, c.ld, u.nr, u.nc, tr ? 1 : 0, coeff);
            }
            ins.first->second.push_back(u);
        }
        return &ins.first->second;
    }
    void bind(double* scratch) { for (auto& kv : uses) for (UCell& u : kv.second) if (u.copy_off >= 0) u.data = scratch + u.copy_off; }
};

// One contribution to an output block (rows of sector qa): A's cells of row sector qa times B's cells of row sector qb (the middle
// sector), or, with B == nullptr, A's cells alone.
struct Contrib { const std::vector<UCell>* A; int32_t qa; const std::vector<UCell>* B; int32_t qb; };

inline bool k_overlap(const UCell& a, const UCell& b, int32_t* k0, int32_t* k1)
{
    *k0 = std::max(a.c0, b.r0); *k1 = std::min(a.c0 + a.nc, b.r0 + b.nr);
    return *k0 < *k1;
}

struct EmitWork { std::vector<int32_t> rcuts, ccuts; };

// The groups of one output block C (M x N, leading dimension ldc).  eye: the unit matrix (leading dimension ld_eye), where one is needed.
void emit_block(GemmBatch& gb, GemmSet& set, double* Cp, int32_t ldc, int32_t M, int32_t N, const std::vector<Contrib>& cs,
                const double* eye, int32_t ld_eye, EmitWork& w)
{
    w.rcuts.assign({0, M});
    w.ccuts.assign({0, N});
    for (const Contrib& c : cs)
        for (const UCell& a : *c.A) {
            if (a.q != c.qa) continue;
            w.rcuts.push_back(a.r0); w.rcuts.push_back(a.r0 + a.nr);
            if (!c.B) { w.ccuts.push_back(a.c0); w.ccuts.push_back(a.c0 + a.nc); continue; }
            for (const UCell& b : *c.B) {
                if (b.q != c.qb) continue;
                w.ccuts.push_back(b.c0); w.ccuts.push_back(b.c0 + b.nc);
                int32_t k0, k1;
                if (!k_overlap(a, b, &k0, &k1)) continue;
                if (a.kind == DMRGX_CELL_IDENT) { w.rcuts.push_back(a.r0 + k0 - a.c0); w.rcuts.push_back(a.r0 + k1 - a.c0); }
                if (b.kind == DMRGX_CELL_IDENT) { w.ccuts.push_back(b.c0 + k0 - b.r0); w.ccuts.push_back(b.c0 + k1 - b.r0); }
            }
        }
    for (std::vector<int32_t>* cuts : {&w.rcuts, &w.ccuts}) { std::sort(cuts->begin(), cuts->end()); cuts->erase(std::unique(cuts->begin(), cuts->end()), cuts->end()); }
    for (size_t s = 0; s + 1 < w.rcuts.size(); ++s)
        for (size_t t = 0; t + 1 < w.ccuts.size(); ++t) {
            const int32_t p = w.rcuts[s], e = w.rcuts[s + 1], p2 = w.ccuts[t], e2 = w.ccuts[t + 1];
            const int32_t pb = (int32_t)gb.prods.size();
            int32_t cost = 0, n_axpy = 0;
            auto copy_of = [&](const double* S, int32_t lds, double alpha) { gb.prods.push_back(GProd{nullptr, S, 0, lds, 0, GPROD_AXPY, alpha}); ++n_axpy; ++cost; };
            for (int pass = 0; pass < 2; ++pass)                  // scaled copies first, then the GEMM products
                for (const Contrib& c : cs)
                    for (const UCell& a : *c.A) {
                        if (a.q != c.qa || a.r0 > p || a.r0 + a.nr < e) continue;
                        const bool ai = a.kind == DMRGX_CELL_IDENT;
                        if (!c.B) {
                            if (pass != 0 || a.c0 > p2 || a.c0 + a.nc < e2) continue;
                            if (ai) copy_of(eye + (int64_t)(p - a.r0) * ld_eye + (p2 - a.c0), ld_eye, a.scale);
                            else copy_of(a.data + (int64_t)(p - a.r0) * a.ld + (p2 - a.c0), a.ld, 1.0);
                            continue;
                        }
                        for (const UCell& b : *c.B) {
                            if (b.q != c.qb || b.c0 > p2 || b.c0 + b.nc < e2) continue;
                            const bool bi = b.kind == DMRGX_CELL_IDENT;
                            int32_t k0, k1;
                            if ((ai || bi) != (pass == 0) || !k_overlap(a, b, &k0, &k1)) continue;
                            const int32_t kp = a.c0 + (p - a.r0), kc = b.r0 + (p2 - b.c0);      // where the rectangle's rows / columns sit in the middle sector, through an identity
                            if (ai && (kp < k0 || kp + (e - p) > k1)) continue;
                            if (bi && (kc < k0 || kc + (e2 - p2) > k1)) continue;
                            if (ai && bi) copy_of(eye + (int64_t)(kp - k0) * ld_eye + (kc - k0), ld_eye, a.scale * b.scale);
                            else if (ai) copy_of(b.data + (int64_t)(kp - b.r0) * b.ld + (p2 - b.c0), b.ld, a.scale);
                            else if (bi) copy_of(a.data + (int64_t)(p - a.r0) * a.ld + (kc - a.c0), a.ld, b.scale);
                            else {
                                gb.prods.push_back(GProd{a.data + (int64_t)(p - a.r0) * a.ld + (k0 - a.c0), b.data + (int64_t)(k0 - b.r0) * b.ld + (p2 - b.c0), a.ld, b.ld, k1 - k0, GPROD_GEMM, 1.0});
                                cost += ggemm_ksteps(k1 - k0);
                            }
                        }
                    }
            gb.group(set, GGroup{Cp + (int64_t)p * ldc + p2, ldc, e - p, e2 - p2, pb, (int32_t)gb.prods.size(), n_axpy, 0}, std::max(cost, 1));
        }
}

// the checks of one input operator: normalise_op's of the term builder, on the cells as given
dmrgx_status check_op(const char* fn, int32_t o, const dmrgx_secop& op, const dmrgx_sectors& sec)
{
    if (op.ncells < 0 || (op.ncells > 0 && !op.cells)) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: operator %d: bad cell list", fn, o);
    const int32_t stored = op.transposed ? -op.shift : op.shift;
    for (int32_t i = 0; i < op.ncells; ++i) {
        const dmrgx_cell& c = op.cells[i];
        const int32_t qc = c.row_sector + stored;
        if (c.row_sector < 0 || c.row_sector >= sec.nsec || qc < 0 || qc >= sec.nsec)
            DMRGX_FAIL(DMRGX_ERR_OUTOFRANGE, "%s: operator %d: cell %d sector (%d -> %d) out of range [0,%d)", fn, o, i, c.row_sector, qc, sec.nsec);
        if (c.nr <= 0 || c.nc <= 0 || c.r0 < 0 || c.c0 < 0 || c.r0 + c.nr > sec.size[c.row_sector] || c.c0 + c.nc > sec.size[qc])
            DMRGX_FAIL(DMRGX_ERR_OUTOFRANGE, "%s: operator %d: cell %d rectangle [%d+%d, %d+%d) exceeds block %d x %d", fn, o, i, c.r0, c.nr, c.c0, c.nc, sec.size[c.row_sector], sec.size[qc]);
        if (c.kind == DMRGX_CELL_IDENT) { if (c.nr != c.nc) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: operator %d: identity cell %d not square", fn, o, i); }
        else if (c.kind == DMRGX_CELL_DENSE) {
            if (!c.data || c.ld < c.nc || c.ld > INT32_MAX) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: operator %d: dense cell %d has no data / bad ld", fn, o, i);
        } else DMRGX_FAIL(DMRGX_ERR_ARG, "%s: operator %d: cell %d has unknown kind %d", fn, o, i, c.kind);
    }
    return DMRGX_OK;
}

}  // namespace
}  // namespace dmrgx

using namespace dmrgx;

extern "C" dmrgx_status dmrgx_secop_compose(const dmrgx_sectors* sectors, int32_t n_ops, const dmrgx_secop* ops,
                                            int32_t n_out, const int32_t* out_first, const dmrgx_secop_string* strings,
                                            int32_t* out_shift, int32_t* cell_first, dmrgx_cell* cells,
                                            int64_t* n_doubles, double* arena_dev, void* stream)
{
    const char* fn = "secop_compose";
    hipStream_t st = (hipStream_t)stream;
    if (!sectors || sectors->nsec <= 0 || !sectors->size) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: empty sector table", fn);
    const dmrgx_sectors& S = *sectors;
    const int32_t ns = S.nsec;
    for (int32_t q = 0; q < ns; ++q) if (S.size[q] <= 0) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: sector %d has size %d", fn, q, S.size[q]);
    if (n_ops < 0 || (n_ops > 0 && !ops)) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: bad operator list (%d operators)", fn, n_ops);
    if (n_out < 0 || !out_first || out_first[0] != 0) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: no outputs, or out_first does not start at 0", fn);
    if (!out_shift || !cell_first || !cells || !n_doubles) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: null out_shift, cell_first, cells or n_doubles", fn);
    for (int32_t o = 0; o < n_out; ++o)
        if (out_first[o + 1] <= out_first[o]) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: output %d is empty (out_first %d, %d): every output has at least one string", fn, o, out_first[o], out_first[o + 1]);
    if (n_out > 0 && !strings) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: null string list", fn);
    for (int32_t o = 0; o < n_out; ++o)
        for (int32_t t = out_first[o]; t < out_first[o + 1]; ++t) {
            const dmrgx_secop_string& T = strings[t];
            if (T.nfac < 1 || T.nfac > 3) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: string %d of output %d has %d factors: 1, 2 or 3", fn, t - out_first[o], o, T.nfac);
            if (!std::isfinite(T.coeff)) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: the coefficient of string %d of output %d is not finite", fn, t - out_first[o], o);
            int32_t s = 0;
            for (int32_t f = 0; f < T.nfac; ++f) {
                if (T.fac[f] < 0 || T.fac[f] >= n_ops) DMRGX_FAIL(DMRGX_ERR_OUTOFRANGE, "%s: string %d of output %d references operator %d outside the %d operators", fn, t - out_first[o], o, T.fac[f], n_ops);
                s += ops[T.fac[f]].shift;
            }
            if (t == out_first[o]) out_shift[o] = s;
            else if (s != out_shift[o]) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: string %d of output %d has net shift %d, its first string has %d: one output, one shift", fn, t - out_first[o], o, s, out_shift[o]);
        }
    for (int32_t i = 0; i < n_ops; ++i) DMRGX_CHK(check_op(fn, i, ops[i], S));

    // the cell table: output o dense over every block (q -> q + s_o) whose sectors exist, ascending q, one after the other
    int64_t total = 0;
    int32_t ncell = 0;
    for (int32_t o = 0; o < n_out; ++o) {
        cell_first[o] = ncell;
        for (int32_t q = 0; q < ns; ++q) {
            const int32_t qc = q + out_shift[o];
            if (qc < 0 || qc >= ns) continue;
            cells[ncell++] = dmrgx_cell{q, 0, 0, S.size[q], S.size[qc], DMRGX_CELL_DENSE, 0.0, arena_dev ? arena_dev + total : nullptr, S.size[qc]};
            total += (int64_t)S.size[q] * S.size[qc];
        }
    }
    cell_first[n_out] = ncell;
    *n_doubles = total;
    if (!arena_dev || n_out == 0) return DMRGX_OK;                  // sizes only: no device call so far

    for (int32_t i = 0; i < n_ops; ++i)
        for (int32_t j = 0; j < ops[i].ncells; ++j) {
            const dmrgx_cell& c = ops[i].cells[j];
            if (c.kind != DMRGX_CELL_DENSE) continue;
            const double* end = c.data + (int64_t)(c.nr - 1) * c.ld + c.nc;
            if (arena_dev < end && c.data < arena_dev + total) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: the arena overlaps cell %d of operator %d", fn, j, i);
        }

    // operands: the first factor of a string carries its coefficient; a prefix is numbered ~index in the same table
    Operands ou;
    struct Prefix { int32_t f1, f2; double c; const std::vector<UCell>* A; const std::vector<UCell>* B; };
    std::vector<Prefix> prefixes;
    std::map<std::tuple<int32_t, int32_t, uint64_t>, int32_t> prefix_of;
    const int32_t nstr = out_first[n_out];
    struct StrUse { const std::vector<UCell>* A; const std::vector<UCell>* B; int32_t s_mid, prefix; };     // C-block rows q: A at q, B at q + s_mid
    std::vector<StrUse> suse((size_t)nstr);
    for (int32_t t = 0; t < nstr; ++t) {
        const dmrgx_secop_string& T = strings[t];
        StrUse& u = suse[(size_t)t];
        u = StrUse{nullptr, nullptr, 0, -1};
        if (T.nfac <= 2) {
            u.A = ou.use_of(T.fac[0], T.coeff, ops[T.fac[0]]);
            if (T.nfac == 2) { u.B = ou.use_of(T.fac[1], 1.0, ops[T.fac[1]]); u.s_mid = ops[T.fac[0]].shift; }
        } else {
            auto ins = prefix_of.emplace(std::make_tuple(T.fac[0], T.fac[1], Operands::bits_of(T.coeff)), (int32_t)prefixes.size());
            if (ins.second) prefixes.push_back(Prefix{T.fac[0], T.fac[1], T.coeff, ou.use_of(T.fac[0], T.coeff, ops[T.fac[0]]), ou.use_of(T.fac[1], 1.0, ops[T.fac[1]])});
            u.prefix = ins.first->second;
            u.B = ou.use_of(T.fac[2], 1.0, ops[T.fac[2]]);
            u.s_mid = ops[T.fac[0]].shift + ops[T.fac[1]].shift;
        }
    }
    // the prefixes: one dense block per row sector q whose middle sector q + s1 and column sector q + s1 + s2 exist
    for (size_t x = 0; x < prefixes.size(); ++x) {
        const int32_t s1 = ops[prefixes[x].f1].shift, sp = s1 + ops[prefixes[x].f2].shift;
        std::vector<UCell>& pc = ou.uses[std::make_pair(~(int32_t)x, (uint64_t)0)];
        for (int32_t q = 0; q < ns; ++q) {
            if (q + s1 < 0 || q + s1 >= ns || q + sp < 0 || q + sp >= ns) continue;
            pc.push_back(UCell{q, 0, 0, S.size[q], S.size[q + sp], DMRGX_CELL_DENSE, 1.0, nullptr, S.size[q + sp], ou.doubles});
            ou.doubles += (int64_t)S.size[q] * S.size[q + sp];
        }
    }
    // a unit matrix where a scaled copy has no dense cell to copy from: identity . identity, a one-factor string that is an identity cell
    auto ident_order = [](const std::vector<UCell>* v) { int32_t n = 0; if (v) for (const UCell& u : *v) if (u.kind == DMRGX_CELL_IDENT) n = std::max(n, u.nr); return n; };
    for (int32_t t = 0; t < nstr; ++t) {
        const StrUse& u = suse[(size_t)t];
        if (u.prefix >= 0) continue;
        const int32_t na = ident_order(u.A), nb = ident_order(u.B);
        if (na > 0 && (!u.B || nb > 0)) ou.eye = std::max(ou.eye, std::max(na, nb));
    }
    for (const Prefix& p : prefixes) if (ident_order(p.A) > 0 && ident_order(p.B) > 0) ou.eye = std::max(ou.eye, std::max(ident_order(p.A), ident_order(p.B)));
    if (ou.eye > 0) { ou.eye_off = ou.doubles; ou.push_copy(nullptr, 0, ou.eye, ou.eye, 0, 1.0); }

    DevBuf scratch, tab;
    if (ou.doubles > 0) DMRGX_CHK(scratch.alloc_f64((size_t)ou.doubles, st));
    ou.bind(scratch.as<double>());
    const double* eye = ou.eye > 0 ? scratch.as<double>() + ou.eye_off : nullptr;

    GemmBatch gb;
    GemmSet set1, set2;
    EmitWork work;
    std::vector<Contrib> cs;
    for (size_t x = 0; x < prefixes.size(); ++x) {
        const int32_t s1 = ops[prefixes[x].f1].shift;
        for (const UCell& pc : ou.uses.at(std::make_pair(~(int32_t)x, (uint64_t)0))) {
            cs.assign(1, Contrib{prefixes[x].A, pc.q, prefixes[x].B, pc.q + s1});
            emit_block(gb, set1, const_cast<double*>(pc.data), pc.ld, pc.nr, pc.nc, cs, eye, ou.eye, work);
        }
    }
    for (int32_t o = 0; o < n_out; ++o)
        for (int32_t ci = cell_first[o]; ci < cell_first[o + 1]; ++ci) {
            const dmrgx_cell& c = cells[ci];
            const int32_t q = c.row_sector;
            cs.clear();
            for (int32_t t = out_first[o]; t < out_first[o + 1]; ++t) {
                const StrUse& u = suse[(size_t)t];
                const int32_t qm = q + u.s_mid;
                if (u.B && (qm < 0 || qm >= ns)) continue;             // the middle sector does not exist
                cs.push_back(Contrib{u.prefix >= 0 ? &ou.uses.at(std::make_pair(~u.prefix, (uint64_t)0)) : u.A, q, u.B, qm});
            }
            emit_block(gb, set2, const_cast<double*>(c.data), (int32_t)c.ld, c.nr, c.nc, cs, eye, ou.eye, work);
        }
    PackedUpload pk;
    gb.pack(pk);
    gb.pack(set1, pk);
    gb.pack(set2, pk);
    const size_t o_tasks = pk.add(ou.copies), o_tiles = pk.add(ou.tiles);
    DMRGX_CHK(pk.upload(tab, st));
    gb.bind(tab);
    if (!ou.tiles.empty()) {
        hipLaunchKernelGGL(secop_cell_copy_kernel, dim3((unsigned)ou.tiles.size()), dim3(256), 0, st, (const CellCopyTile*)packed_at<CellCopyTile>(tab, o_tiles),
                           (const CellCopy*)packed_at<CellCopy>(tab, o_tasks), scratch.as<double>());
        DMRGX_HIP(hipGetLastError());
    }
    DMRGX_CHK(gb.launch(set1, tab, st));
    return gb.launch(set2, tab, st);
}
