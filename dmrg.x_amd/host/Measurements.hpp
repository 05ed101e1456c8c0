#ifndef DMRGX_HOST_MEASUREMENTS_HPP
#define DMRGX_HOST_MEASUREMENTS_HPP
/** What the measurements of EngineMeasurements.hpp share.  All of them: the two blocks as the library sees them, the site operators of
    one Gram / term call, the JSON record file; -corr_matrix and -corr_dimer: the bond list and the lattice Fourier sum; -corr_dimer and
    -dsf_dimer (DimerCorrelations::Run, DimerDynamics::Run): DimerFrame, the bond operators as terms, BondsOfOrientation, the bond header.
    The four dynamical ones, -dsf, -dsf_sites, -dsf_cheb and -dsf_cv (DynamicalStructureFactor::Run, DynamicalCorrelations::Run,
    ChebyshevCorrelations::Run, CorrectionVectors::Run): SzFrame, SiteCosineSum, the w0,w1,nw grid, the openings of their records;
    the phase coefficients of -dsf; -dsf_pm (TransverseDynamics::Run): SzFrame over Sp or Sm.  The Chebyshev three, -dsf_cheb, -dsf_pm and
    -dsf_dimer: the window, the moment run (MomentRun), the Jackson-damped grid and the moment part of a record.  host_tool.cpp runs the pure parts without a GPU. */
#include <cmath>
#include <deque>
#include "DMRGKron.hpp"
#include "TridiagQL.hpp"

namespace dmrgx_host {

constexpr double two_pi = 6.283185307179586476925286766559;

/** The left (side 0) and the right (side 1) block of a KronBlocks_t, their sector sizes and the (left, right) sector of every
    KronBlock.  sectors[] points into sizes[]: not copyable.  Site s of the right block is lattice site N - 1 - s, as in SetUpCorrelation. */
struct CentreFrame {
    const char* name = "";                                      /* the measurement, as its messages call it */
    Block::SpinBase* blk[2] = {nullptr, nullptr};
    PetscInt nsites[2] = {0, 0}, N = 0;
    std::vector<int32_t> sizes[2], bil, bir;
    dmrgx_sectors sectors[2] = {{0, nullptr}, {0, nullptr}};
    CentreFrame() = default;
    CentreFrame(const CentreFrame&) = delete;
    PetscErrorCode Init(KronBlocks_t& KronBlocks, PetscInt num_sites, const char* display_name)
    {
        name = display_name; blk[0] = &KronBlocks.LeftBlockRefMod(); blk[1] = &KronBlocks.RightBlockRefMod();
        nsites[0] = blk[0]->NumSites(); nsites[1] = blk[1]->NumSites(); N = num_sites;
        if (nsites[0] + nsites[1] != N) SETERRQ4(PETSC_COMM_SELF, 1, "%s: the blocks hold %lld + %lld sites, the lattice %lld.", name, LLD(nsites[0]), LLD(nsites[1]), LLD(N));
        for (int side = 0; side < 2; ++side) { sizes[side] = blk[side]->Magnetization.Sizes32(); sectors[side] = dmrgx_sectors{(int32_t)sizes[side].size(), sizes[side].data()}; }
        for (PetscInt k = 0; k < KronBlocks.size(); ++k) { bil.push_back((int32_t)KronBlocks.LeftIdx(k)); bir.push_back((int32_t)KronBlocks.RightIdx(k)); }
        return 0;
    }
    PetscInt lattice_site(int side, PetscInt block_site) const { return side == 0 ? block_site : N - 1 - block_site; }
    PetscInt block_site(int side, PetscInt lattice_site) const { return side == 0 ? lattice_site : N - 1 - lattice_site; }
    /** Sz(s) or Sp(s) of a block (Sm is never stored).  A pruned operator must never read as zero. */
    PetscErrorCode resident(int side, Op_t type, PetscInt s, Mat& m) const
    {
        m = type == OpSz ? blk[side]->Sz(s) : blk[side]->Sp(s);
        if (!m) SETERRQ4(PETSC_COMM_SELF, PETSC_ERR_ARG_WRONGSTATE, "%s: operator %s(%lld) of the %s block is not resident (pruned).", name, OpToCStr(type), LLD(s), side == 0 ? "left" : "right");
        return 0;
    }
};

/** The operators of one dmrgx_kron_op_gram / term_apply / term_gram call: ops[0] on the left block, ops[1] on the right, in the order
    they were asked for (the order of the Gram vectors).  The cells behind a dmrgx_secop stay where they are while the table lives. */
class SiteOperators {
public:
    explicit SiteOperators(const CentreFrame& F) : F(F) {}
    SiteOperators(const SiteOperators&) = delete;                /* ops point into store */
    std::vector<dmrgx_secop> ops[2];
    /** idx: where Sz, Sp or Sm of block site s stands in ops[side]; appended at its first use.  Sm(s) is Sp(s) read transposed. */
    PetscErrorCode Site(int side, Op_t type, PetscInt s, int32_t& idx)
    {
        auto it = index.find(std::make_tuple(side, (int)type, s));
        if (it != index.end()) { idx = it->second; return 0; }
        Mat m;
        PetscErrorCode ierr = F.resident(side, type == OpSz ? OpSz : OpSp, s, m); CHKERRQ(ierr);
        index[std::make_tuple(side, (int)type, s)] = idx = Add(side, m, type == OpSm);
        return 0;
    }
    /** A ready operator of the block (a bond operator), or read transposed with sector shift -1 (Sm from Sp). */
    int32_t Add(int side, const Mat& m, bool transposed = false) { dmrgx_secop so; store.emplace_back(); m->to_secop(so, store.back(), transposed, -1); ops[side].push_back(so); return (int32_t)ops[side].size() - 1; }
    /** Sz, Sp or Sm of every site of the left, then of the right block; `lattice` gains the lattice site of each. */
    PetscErrorCode AllSites(Op_t type, std::vector<PetscInt>& lattice)
    {
        for (int side = 0; side < 2; ++side) for (PetscInt s = 0; s < F.nsites[side]; ++s) {
            int32_t idx;
            PetscErrorCode ierr = Site(side, type, s, idx); CHKERRQ(ierr);
            lattice.push_back(F.lattice_site(side, s));
        }
        return 0;
    }
    /** The identity of the block. */
    void AddIdentity(int side)
    {
        const std::vector<int32_t>& sz = F.sizes[side];
        store.emplace_back();
        for (int32_t q = 0; q < (int32_t)sz.size(); ++q) store.back().push_back(dmrgx_cell{q, 0, 0, sz[(size_t)q], sz[(size_t)q], DMRGX_CELL_IDENT, 1.0, nullptr, 0});
        ops[side].push_back(dmrgx_secop{0, 0, (int32_t)store.back().size(), store.back().data()});
    }
private:
    const CentreFrame& F;
    std::deque<std::vector<dmrgx_cell>> store;                  /* a deque: its elements never move */
    std::map<std::tuple<int, int, PetscInt>, int32_t> index;    /* (side, Sz / Sp / Sm, block site) -> index in ops[side] */
};

/** Sz of every site of the centre superblock and the ground state it acts on: the set-up of -dsf, -dsf_sites, -dsf_cheb and -dsf_cv.
    Operator a of the table T is Sz of lattice site site[a], op_of is the inverse; (rx, ry)[s] is where LATTICE site s sits on the
    Lx x Ly lattice of M = Lx Ly sites.  psi: the n states on the device, norm = <psi|psi>; ld = n rounded up to even, the row length
    of a family of vectors (the library streams rows in 16-byte loads).  Init(..., OpSp) or (..., OpSm) gives the same frame over Sp or Sm
    (Sp read transposed) of every site: the set-up of -dsf_pm, whose images live in another sector (Images with out_il, out_ir). */
struct SzFrame {
    CentreFrame F;
    SiteOperators T{F};
    std::vector<PetscInt> site, op_of, rx, ry;
    PetscInt Lx = 0, Ly = 0, M = 0;
    int64_t n = 0, ld = 0;
    const double* psi = nullptr; double norm = 0.0;
    template<class Hamiltonian> PetscErrorCode Init(KronBlocks_t& KronBlocks, PetscInt num_sites, const Hamiltonian& Ham, const Vec& gsv_r, const char* display_name, Op_t type = OpSz)
    {
        PetscErrorCode ierr = F.Init(KronBlocks, num_sites, display_name); CHKERRQ(ierr);
        ierr = T.AllSites(type, site); CHKERRQ(ierr);
        op_of.assign((size_t)F.N, -1); rx.resize((size_t)F.N); ry.resize((size_t)F.N);
        for (PetscInt a = 0; a < F.N; ++a) op_of[(size_t)site[(size_t)a]] = a;
        for (PetscInt s = 0; s < F.N; ++s) {
            if (op_of[(size_t)s] < 0) SETERRQ2(PETSC_COMM_SELF, 1, "%s: site %lld is in neither block.", F.name, LLD(s));
            ierr = Ham.To2D(s, rx[(size_t)s], ry[(size_t)s]); CHKERRQ(ierr);
        }
        Lx = Ham.Lx(); Ly = Ham.Ly(); M = Lx * Ly;
        n = gsv_r->n; ld = n + (n & 1); psi = gsv_r->buf->dev_ro();
        if (dmrgx_dot(n, psi, psi, &norm, nullptr)) SETERRQ1(PETSC_COMM_SELF, 1, "dmrgx_dot: %s", dmrgx_last_error());
        return 0;
    }
    /** coeff times operator a (Sz of its site), as a term of one vector. */
    dmrgx_term term(PetscInt a, double coeff = 1.0) const { return a < F.nsites[0] ? dmrgx_term{coeff, (int32_t)a, -1} : dmrgx_term{coeff, -1, (int32_t)(a - F.nsites[0])}; }
    /** dmrgx_kron_term_apply on psi: vector j = the sum of terms[vec_first[j] .. vec_first[j + 1]), written to dst + j ld_dst. */
    PetscErrorCode Apply(PetscInt nvec, const int32_t* vec_first, const dmrgx_term* terms, double* dst, int64_t ld_dst) const
    {
        if (dmrgx_kron_term_apply(&F.sectors[0], &F.sectors[1], (int32_t)F.bil.size(), F.bil.data(), F.bir.data(), psi, (int32_t)T.ops[0].size(), T.ops[0].data(), (int32_t)T.ops[1].size(), T.ops[1].data(),
                                  (int32_t)nvec, vec_first, terms, dst, ld_dst, nullptr)) SETERRQ1(PETSC_COMM_SELF, 1, "dmrgx_kron_term_apply: %s", dmrgx_last_error());
        return 0;
    }
    /** Images of at most 1 GiB per term_apply (its intermediates grow with its vectors). */
    PetscInt chunk() const { return std::max<PetscInt>(1, std::min<PetscInt>(F.N, (PetscInt)((((int64_t)1 << 30) / (int64_t)sizeof(double)) / ld))); }
    /** dst + j ld_dst = operator ops[j] on psi, j < count, in chunks: in the layout of psi, or, with out_il and out_ir, in the layout of the KronBlocks
        (out_il, out_ir)[0 .. n_out) of the sector the operators lead to (dmrgx_kron_term_apply_to; there a chunk is 1 GiB of rows of ld_dst). */
    PetscErrorCode Images(const PetscInt* ops, PetscInt count, double* dst, int64_t ld_dst, const std::vector<int32_t>* out_il = nullptr, const std::vector<int32_t>* out_ir = nullptr) const
    {
        const PetscInt per = out_il ? std::max<PetscInt>(1, std::min<PetscInt>(F.N, (PetscInt)((((int64_t)1 << 30) / (int64_t)sizeof(double)) / std::max<int64_t>(ld_dst, 1)))) : chunk();
        std::vector<dmrgx_term> terms; std::vector<int32_t> vec_first;
        for (PetscInt j0 = 0; j0 < count; j0 += per) {
            const PetscInt cnt = std::min<PetscInt>(per, count - j0);
            terms.clear(); vec_first.assign(1, 0);
            for (PetscInt j = j0; j < j0 + cnt; ++j) { terms.push_back(term(ops[j])); vec_first.push_back((int32_t)terms.size()); }
            if (!out_il) { PetscErrorCode ierr = Apply(cnt, vec_first.data(), terms.data(), dst + j0 * ld_dst, ld_dst); CHKERRQ(ierr); }
            else if (dmrgx_kron_term_apply_to(&F.sectors[0], &F.sectors[1], (int32_t)F.bil.size(), F.bil.data(), F.bir.data(), psi, (int32_t)T.ops[0].size(), T.ops[0].data(), (int32_t)T.ops[1].size(), T.ops[1].data(),
                                              (int32_t)cnt, vec_first.data(), terms.data(), (int32_t)out_il->size(), out_il->data(), out_ir->data(), dst + j0 * ld_dst, ld_dst, nullptr))
                SETERRQ1(PETSC_COMM_SELF, 1, "dmrgx_kron_term_apply_to: %s", dmrgx_last_error());
        }
        return 0;
    }
    /** U: Images of all N sites, row s = the operator of LATTICE site s on psi, in rows of n_out rounded up to even doubles (n_out = n in
        the layout of psi).  They stay on the device while U lives; PETSC_ERR_MEM if they do not fit. */
    PetscErrorCode AllImages(std::unique_ptr<DevBuffer>& U, int64_t n_out, const std::vector<int32_t>* out_il = nullptr, const std::vector<int32_t>* out_ir = nullptr) const
    {
        const int64_t ld_out = n_out + (n_out & 1);
        try { U.reset(new DevBuffer((size_t)(F.N * ld_out), DevBuffer::device_only_t{})); }
        catch (const std::exception& e) { SETERRQ5(PETSC_COMM_SELF, PETSC_ERR_MEM, "%s: no memory for the images of %lld sites x %lld states (%.3f GB): %s", F.name, LLD(F.N), LLD(n_out), (double)(F.N * ld_out) * 8e-9, e.what()); }
        return Images(op_of.data(), F.N, U->dev_uninitialised(), ld_out, out_il, out_ir);
    }
};

/** S[nx][ny] = (1 / norm) sum_ab cos(q . (r_a - r_b)) T[a][b] over n points r_a = (x[a], y[a]) of the Lx x Ly lattice,
    q = (2 pi nx / Lx, 2 pi ny / Ly); T is n x n, the result Lx x Ly, both row-major. */
inline std::vector<double> LatticeFourier(PetscInt Lx, PetscInt Ly, const PetscInt* x, const PetscInt* y, const double* T, PetscInt n, double norm)
{
    std::vector<double> S((size_t)(Lx * Ly), 0.0);
    for (PetscInt nx = 0; nx < Lx; ++nx) for (PetscInt ny = 0; ny < Ly; ++ny) {
        double acc = 0.0;
        for (PetscInt a = 0; a < n; ++a) for (PetscInt b = 0; b < n; ++b)
            acc += std::cos(two_pi * ((double)(nx * (x[a] - x[b])) / (double)Lx + (double)(ny * (y[a] - y[b])) / (double)Ly)) * T[a * n + b];
        S[(size_t)(nx * Ly + ny)] = acc / norm;
    }
    return S;
}

/** The lattice Fourier sum of one column, from the reference site c:  out[nx Ly + ny][k] = sum_s cos(q . (r_s - r_c)) T[s][k] over
    the N sites r_s = (rx[s], ry[s]); T is N x ncol, the result (Lx Ly) x ncol, both row-major.  Every element is summed over s
    ascending from 0.0: LatticeFourier of the N x N matrix that holds T[:, k] in column c gives the same bits with norm = 1. */
inline std::vector<double> SiteCosineSum(PetscInt Lx, PetscInt Ly, const PetscInt* rx, const PetscInt* ry, PetscInt c, const double* T, PetscInt N, PetscInt ncol)
{
    std::vector<double> out((size_t)(Lx * Ly * ncol), 0.0);
    for (PetscInt nx = 0; nx < Lx; ++nx) for (PetscInt ny = 0; ny < Ly; ++ny) for (PetscInt s = 0; s < N; ++s) {
        const double cq = std::cos(two_pi * ((double)(nx * (rx[s] - rx[c])) / (double)Lx + (double)(ny * (ry[s] - ry[c])) / (double)Ly));
        for (PetscInt k = 0; k < ncol; ++k) out[(size_t)((nx * Ly + ny) * ncol + k)] += cq * T[s * ncol + k];
    }
    return out;
}

/** The single-mode weight of a transition amplitude T_i = < s | O_i | t > over the N sites r_i = (rx[i], ry[i]):
        W[nx Ly + ny] = (1 / N) [ (sum_i cos(q . r_i) T_i)^2 + (sum_i sin(q . r_i) T_i)^2 ] = (1 / N) | sum_i e^(i q . r_i) T_i |^2,
    q = (2 pi nx / Lx, 2 pi ny / Ly); the result is Lx x Ly, row-major.  Both sums run over i ascending from 0.0.  Summed over all Lx Ly
    wave vectors of a lattice whose sites are all different, W gives sum_i T_i^2 (N = Lx Ly). */
inline std::vector<double> TransitionWeight(PetscInt Lx, PetscInt Ly, const PetscInt* rx, const PetscInt* ry, const double* T, PetscInt N)
{
    std::vector<double> W((size_t)(Lx * Ly), 0.0);
    for (PetscInt nx = 0; nx < Lx; ++nx) for (PetscInt ny = 0; ny < Ly; ++ny) {
        double c = 0.0, s = 0.0;
        for (PetscInt i = 0; i < N; ++i) {
            const double phase = two_pi * ((double)(nx * rx[i]) / (double)Lx + (double)(ny * ry[i]) / (double)Ly);
            c += std::cos(phase) * T[i]; s += std::sin(phase) * T[i];
        }
        W[(size_t)(nx * Ly + ny)] = (c * c + s * s) / (double)N;
    }
    return W;
}

/** The frequencies of a w0,w1,nw option: nw >= 1 equidistant points from w0 to w1 (nw = 1: w0 = w1).  false, and no grid, unless
    om[0..count) is three such numbers. */
inline bool OmegaGrid(const double* om, PetscInt count, std::vector<double>& grid)
{
    if (!(count == 3 && std::isfinite(om[0]) && std::isfinite(om[1]) && om[0] <= om[1] && om[2] >= 1.0 && om[2] <= 1e6 && om[2] == std::floor(om[2]) && (om[2] > 1.0 || om[0] == om[1]))) return false;
    grid.resize((size_t)om[2]);
    for (size_t k = 0; k < grid.size(); ++k) grid[k] = grid.size() > 1 ? om[0] + (om[1] - om[0]) * (double)k / (double)(grid.size() - 1) : om[0];
    return true;
}

/** cos (part 0) or sin (part 1) of the exact fraction 2 pi p / M, 0 <= p < M, with the exact zeros taken from p, not from a rounded
    angle: a part of O_q that vanishes by symmetry vanishes in its coefficients too. */
inline double DsfPhaseCoefficient(int part, PetscInt p, PetscInt M)
{
    if (part == 0) return ((4 * p) % M == 0 && (2 * p) % M != 0) ? 0.0 : std::cos(two_pi * (double)p / (double)M);
    return (2 * p) % M == 0 ? 0.0 : std::sin(two_pi * (double)p / (double)M);
}

/** The window [centre - half_width, centre + half_width] = [E_lo, E_hi] of a Chebyshev expansion from `done` steps of a Lanczos run (alpha, beta
    of dmrgx_kron_lanczos_coeffs; the vectors hold the steps asked for, done < alpha.size() is a breakdown).  theta_min, theta_max: the extreme
    eigenvalues of the Lanczos matrix of order `done`; residual_min, residual = beta_{done-1} |last component of the eigenvector|, the bound
    |lambda - theta| <= residual for SOME eigenvalue lambda of H -- 0 after a breakdown, where the Krylov space is invariant.
    ChebyshevWindow, the lowest eigenvalue E0 known (it stands for theta_min, residual_min = 0):  E_hi = theta_max + residual + 0.02 width,
    E_lo = E0 - 0.01 width, width = theta_max - E0.  ChebyshevWindowTwoSided, a sector whose bottom is not known (-dsf_pm: the neighbouring
    total-Sz sector, for which E0 of the target sector is neither an upper nor a lower bound):  E_hi as before, E_lo = theta_min - residual_min -
    0.02 width, width = theta_max - theta_min; a window that is too tight is caught by the guard of dmrgx_kron_chebyshev_moments (StepsDone < Steps).
    ok false: done < 1, the QL iteration failed, or a window of no width.  bound_steps is for who ran the steps (0: a window that was given). */
struct ChebyshevSpectralWindow { double centre = 0.0, half_width = 0.0, theta_min = 0.0, theta_max = 0.0, residual_min = 0.0, residual = 0.0; PetscInt bound_steps = 0; bool ok = false; };
inline ChebyshevSpectralWindow RitzWindow(const double* bottom, const std::vector<double>& alpha, const std::vector<double>& beta, PetscInt done)
{
    ChebyshevSpectralWindow W;
    if (done < 1 || (size_t)done > alpha.size() || beta.size() < alpha.size()) return W;
    std::vector<double> theta(alpha.begin(), alpha.begin() + done), e(beta.begin(), beta.begin() + done), vec;
    if (!TridiagQLVectors(theta, e, vec)) return W;
    PetscInt top = 0, bot = 0;
    for (PetscInt k = 1; k < done; ++k) { if (theta[(size_t)k] > theta[(size_t)top]) top = k; if (theta[(size_t)k] < theta[(size_t)bot]) bot = k; }
    const double last = (size_t)done < alpha.size() ? 0.0 : beta[(size_t)(done - 1)];
    W.theta_max = theta[(size_t)top]; W.residual = last * std::fabs(vec[(size_t)(top * done + done - 1)]);
    W.theta_min = bottom ? *bottom : theta[(size_t)bot]; W.residual_min = bottom ? 0.0 : last * std::fabs(vec[(size_t)(bot * done + done - 1)]);
    const double width = W.theta_max - W.theta_min, hi = W.theta_max + W.residual + 0.02 * width, lo = W.theta_min - W.residual_min - (bottom ? 0.01 : 0.02) * width;
    W.centre = 0.5 * (hi + lo); W.half_width = 0.5 * (hi - lo);
    W.ok = W.half_width > 0.0 && std::isfinite(W.half_width) && std::isfinite(W.centre);
    return W;
}
inline ChebyshevSpectralWindow ChebyshevWindow(double E0, const std::vector<double>& alpha, const std::vector<double>& beta, PetscInt done) { return RitzWindow(&E0, alpha, beta, done); }
inline ChebyshevSpectralWindow ChebyshevWindowTwoSided(const std::vector<double>& alpha, const std::vector<double>& beta, PetscInt done) { return RitzWindow(nullptr, alpha, beta, done); }

/** The Jackson-damped Chebyshev sum of M moments mu[0..M) at x:
        ( g_0 mu_0 + 2 sum_{n=1}^{M-1} g_n mu_n T_n(x) ) / ( pi sqrt(1 - x^2) ),
        g_n = [ (M - n + 1) cos(pi n / (M + 1)) + sin(pi n / (M + 1)) cot(pi / (M + 1)) ] / (M + 1),
    the moments of a positive measure give a non-negative value (the Jackson kernel is positive).  0 for |x| >= 1 or M < 1. */
inline double ChebyshevJackson(const double* mu, PetscInt M, double x)
{
    if (M < 1 || !(std::fabs(x) < 1.0)) return 0.0;
    const double pi = 0.5 * two_pi, a = pi / (double)(M + 1), cot = std::cos(a) / std::sin(a), phi = std::acos(x);
    double sum = 0.0;
    for (PetscInt n = M - 1; n >= 0; --n) {                      /* the small terms first */
        const double g = ((double)(M - n + 1) * std::cos(a * (double)n) + std::sin(a * (double)n) * cot) / (double)(M + 1);
        sum += (n ? 2.0 : 1.0) * g * mu[n] * std::cos((double)n * phi);
    }
    return sum / (pi * std::sqrt(1.0 - x * x));
}

/** One dmrgx_kron_chebyshev_moments run from row c (a site, a bond) of a family of `count` images, as -dsf_cheb, -dsf_pm and -dsf_dimer record
    it: norm2 = <v0, v0>, `done` steps inside the window, diag[m] = mu_m^{cc}, m <= 2 done, mom (count x (done + 1), row-major) the moments against
    every image, momq their lattice sum (the caller's: which rows enter differs), grid of ChebyshevGrid; elastic: -dsf_dimer alone. */
struct MomentRun { PetscInt c = 0; double norm2 = 0.0, elastic = 0.0; int32_t done = 0; std::vector<double> diag, mom, momq, grid; };

/** What the library returned, as the record holds it: diag (2 K + 1 values) cut to 2 done + 1, cross[k * count + s], k <= done,
    transposed into mom[s * (done + 1) + k], both divided by norm = <psi|psi>.  One division per entry. */
inline void ScaleMoments(MomentRun& R, const std::vector<double>& cross, PetscInt count, double norm)
{
    const PetscInt nm = R.done + 1;
    R.diag.resize((size_t)(2 * R.done + 1));
    for (double& x : R.diag) x /= norm;
    R.mom.assign((size_t)(count * nm), 0.0);
    for (PetscInt s = 0; s < count; ++s) for (PetscInt k = 0; k < nm; ++k) R.mom[(size_t)(s * nm + k)] = cross[(size_t)(k * count + s)] / norm;
}
/** K Chebyshev steps of the planned Hamiltonian in the window W from row R.c of the family U (count rows of ld doubles, on the device),
    <u_i, t_n> of all rows taken by the library, then ScaleMoments by norm; `cross` is the callers' scratch, kept between runs.
    *seconds, unless null, gains the time of the run alone (for the log): a stream sync before it, the library's own after. */
inline PetscErrorCode ChebyshevMomentRun(dmrgx_kron_plan* plan, const double* U, int64_t ld, PetscInt count, const ChebyshevSpectralWindow& W, PetscInt K, double norm,
                                         std::vector<double>& cross, MomentRun& R, double* seconds)
{
    R.diag.assign((size_t)(2 * K + 1), 0.0);
    cross.resize((size_t)((K + 1) * count));
    PetscLogDouble tr0 = 0.0, tr1 = 0.0;
    if (seconds) { if (dmrgx_stream_sync(nullptr)) SETERRQ1(PETSC_COMM_SELF, 1, "%s", dmrgx_last_error()); PetscTime(&tr0); }
    if (dmrgx_kron_chebyshev_moments(plan, U + R.c * ld, W.centre, W.half_width, (int32_t)K, (int32_t)count, U, ld, &R.norm2, R.diag.data(), cross.data(), &R.done, nullptr))
        SETERRQ1(PETSC_COMM_SELF, 1, "dmrgx_kron_chebyshev_moments: %s", dmrgx_last_error());
    if (seconds) { PetscTime(&tr1); *seconds += tr1 - tr0; }
    ScaleMoments(R, cross, count, norm);
    return 0;
}

/** grid[q][k] = ChebyshevJackson(momq[q], nm, x_k) / half_width at x_k = (omega[k] + E0 - centre) / half_width, for every row q of momq
    (rows of nm moments): the Jackson-broadened spectral density at the frequencies omega, measured from E0. */
inline std::vector<double> ChebyshevGrid(const std::vector<double>& momq, PetscInt nm, const std::vector<double>& omega, double E0, double centre, double half_width)
{
    const PetscInt M = (PetscInt)momq.size() / nm, nw = (PetscInt)omega.size();
    std::vector<double> grid((size_t)(M * nw), 0.0);
    for (PetscInt q = 0; q < M; ++q) for (PetscInt k = 0; k < nw; ++k)
        grid[(size_t)(q * nw + k)] = ChebyshevJackson(momq.data() + q * nm, nm, (omega[(size_t)k] + E0 - centre) / half_width) / half_width;
    return grid;
}

/** The warning of a run that the library's guard ended before its K steps: "-option[ (channel)]: the run from <noun> c left the window". */
inline void WarnLeftWindow(const char* option, const char* channel, const char* noun, const MomentRun& R, const ChebyshevSpectralWindow& W, PetscInt K)
{
    if (R.done >= K) return;
    printf("  * WARNING: %s%s%s%s: the run from %s %lld left the window [%.6f, %.6f] after %lld of %lld steps; the record holds the moments up to there.\n",
           option, channel ? " (" : "", channel ? channel : "", channel ? ")" : "", noun, LLD(R.c), W.centre - W.half_width, W.centre + W.half_width, LLD(R.done), LLD(K));
}

/** A nearest-neighbour bond of the lattice: sites i < j, the site (ix, jy) from which NearestNeighbors generates it, 'x' if the two
    sites differ in column, else 'y'. */
struct DimerBond { PetscInt i, j, ix, jy; char orient; };
/** The distinct pairs of Ham.NeighborPairs(), in order of first appearance (on Ly = 2 with the periodic y boundary every vertical pair
    appears twice).  The generating site is the one whose "above" (y) or "right" (x) neighbour is the other site; where that holds
    for both -- two sites round a periodic direction -- the lower-numbered one is visited first. */
template<class Hamiltonian> std::vector<DimerBond> DimerBonds(const Hamiltonian& Ham)
{
    std::vector<DimerBond> bonds;
    std::set<std::pair<PetscInt, PetscInt>> seen;
    for (const std::vector<PetscInt>& p : Ham.NeighborPairs()) {
        if (!seen.insert({p[0], p[1]}).second) continue;
        PetscInt x0, y0, x1, y1;
        Ham.To2D(p[0], x0, y0); Ham.To2D(p[1], x1, y1);
        const char orient = x0 != x1 ? 'x' : 'y';
        const bool from_i = orient == 'x' ? (x0 + 1) % Ham.Lx() == x1 : (y0 + 1) % Ham.Ly() == y1;
        bonds.push_back(DimerBond{p[0], p[1], from_i ? x0 : x1, from_i ? y0 : y1, orient});
    }
    return bonds;
}

/** The bonds of one orientation ('x' or 'y'): of[k] = their index in `bonds`, (x[k], y[k]) = their position (ix, jy), in the order of `bonds`. */
struct OrientedBonds { std::vector<PetscInt> of, x, y; };
inline OrientedBonds BondsOfOrientation(const std::vector<DimerBond>& bonds, char orient)
{
    OrientedBonds O;
    for (size_t b = 0; b < bonds.size(); ++b) if (bonds[b].orient == orient) { O.of.push_back((PetscInt)b); O.x.push_back(bonds[b].ix); O.y.push_back(bonds[b].jy); }
    return O;
}

/** D_b = S_i . S_j = Sz_i Sz_j + (Sp_i Sm_j + Sm_i Sp_j) / 2 of every nearest-neighbour bond of the centre superblock, as terms on the
    ground state: the set-up of -corr_dimer and -dsf_dimer.  side_of[b]: 0 / 1 a bond inside the left / right block, 2 across the cut.
    D_b is built from the stored, truncated block operators, the operator of site i first: a bond inside the left block is A_b (x) 1 with
    A_b formed on the device in dense per-sector form (one grouped GEMM per chunk of bonds: every sector block of every bond is one group
    of three products; the site operators are densified once and released when the bond operators exist), a bond inside the right block
    is 1 (x) B_b -- one one-sided term each --, a bond across the cut is three two-sided terms.  Sm is Sp read transposed.  Bond b is
    terms[vec_first[b] .. vec_first[b + 1]) over the operators of T.  The bond operators (bond_doubles doubles) live as long as the frame. */
struct DimerFrame {
    CentreFrame F;
    SiteOperators T{F};
    std::vector<DimerBond> bonds;
    std::vector<int> side_of;
    std::vector<Mat> bond_op;
    std::vector<int32_t> vec_first;
    std::vector<dmrgx_term> terms;
    PetscInt nb = 0;
    int64_t n = 0, bond_doubles = 0;
    const double* psi = nullptr;
    template<class Hamiltonian> PetscErrorCode Init(KronBlocks_t& KronBlocks, PetscInt num_sites, const Hamiltonian& Ham, const Vec& gsv_r, const char* display_name)
    {
        PetscErrorCode ierr = F.Init(KronBlocks, num_sites, display_name); CHKERRQ(ierr);
        bonds = DimerBonds(Ham);
        nb = (PetscInt)bonds.size();
        n = gsv_r->n; psi = gsv_r->buf->dev_ro();
        for (const DimerBond& b : bonds) side_of.push_back(b.j < F.nsites[0] ? 0 : (b.i >= F.nsites[0] ? 1 : 2));
        ierr = BuildBondOperators(); CHKERRQ(ierr);
        vec_first.assign(1, 0);
        for (PetscInt b = 0; b < nb; ++b) {
            const int side = side_of[(size_t)b];
            if (side < 2) {
                const int32_t idx = T.Add(side, bond_op[(size_t)b]);
                terms.push_back(side == 0 ? dmrgx_term{1.0, idx, -1} : dmrgx_term{1.0, -1, idx});
            } else {
                const PetscInt si = bonds[(size_t)b].i, sj = F.block_site(1, bonds[(size_t)b].j);
                const Op_t left_type[3] = {OpSz, OpSp, OpSm}, right_type[3] = {OpSz, OpSm, OpSp};
                const double coeff[3] = {1.0, 0.5, 0.5};
                for (int t = 0; t < 3; ++t) {
                    int32_t il, ir;
                    ierr = T.Site(0, left_type[t], si, il); CHKERRQ(ierr);
                    ierr = T.Site(1, right_type[t], sj, ir); CHKERRQ(ierr);
                    terms.push_back(dmrgx_term{coeff[t], il, ir});
                }
            }
            vec_first.push_back((int32_t)terms.size());
        }
        return 0;
    }
    /** G ((nb + 1) x (nb + 1), row-major, host): the Gram matrix of psi (vector 0) and the images D_b psi (vector 1 + b), ONE dmrgx_kron_term_gram call. */
    PetscErrorCode Gram(std::vector<double>& G) const { return GramOf(0, psi, 0, G); }
    /** The same over the `nstates` rows of Psi (row stride ldpsi), ONE dmrgx_kron_term_gram_states call: G is (nstates (nb + 1))^2, state-major,
        member s (nb + 1) the state s itself and s (nb + 1) + 1 + b the image D_b psi_s.  The frame's own psi is not read. */
    PetscErrorCode GramStates(PetscInt nstates, const double* Psi, int64_t ldpsi, std::vector<double>& G) const { return GramOf(nstates, Psi, ldpsi, G); }
private:
    /** nstates == 0: dmrgx_kron_term_gram on the one vector Psi; else dmrgx_kron_term_gram_states.  The workspace holds at least the largest
        image block of every vector of the family. */
    PetscErrorCode GramOf(PetscInt nstates, const double* Psi, int64_t ldpsi, std::vector<double>& G) const
    {
        const PetscInt nv = nb + 1, nf = std::max<PetscInt>(nstates, 1) * nv;
        std::vector<int32_t> first{0};
        std::vector<dmrgx_term> all;
        all.push_back(dmrgx_term{1.0, -1, -1});
        all.insert(all.end(), terms.begin(), terms.end());
        for (int32_t f : vec_first) first.push_back(f + 1);
        /* the workspace holds at least the largest image block of every vector: the blocks (IL, IR), (IL - 1, IR + 1), (IL + 1, IR - 1) */
        int64_t largest = 1;
        for (size_t k = 0; k < F.bil.size(); ++k)
            for (int32_t d = -1; d <= 1; ++d) {
                const int32_t a = F.bil[k] - d, c = F.bir[k] + d;
                if (a >= 0 && a < (int32_t)F.sizes[0].size() && c >= 0 && c < (int32_t)F.sizes[1].size()) largest = std::max<int64_t>(largest, (int64_t)F.sizes[0][(size_t)a] * F.sizes[1][(size_t)c]);
            }
        const size_t workspace = std::max<size_t>((size_t)1 << 30, (size_t)largest * (size_t)nf * sizeof(double));
        G.assign((size_t)(nf * nf), 0.0);
        DevBuffer g((size_t)(nf * nf), DevBuffer::device_only_t{});
        if (nstates == 0) {
            if (dmrgx_kron_term_gram(&F.sectors[0], &F.sectors[1], (int32_t)F.bil.size(), F.bil.data(), F.bir.data(), Psi, (int32_t)T.ops[0].size(), T.ops[0].data(), (int32_t)T.ops[1].size(), T.ops[1].data(),
                                     (int32_t)nv, first.data(), all.data(), workspace, g.dev_uninitialised(), nv, nullptr, nullptr)) SETERRQ1(PETSC_COMM_SELF, 1, "dmrgx_kron_term_gram: %s", dmrgx_last_error());
        } else if (dmrgx_kron_term_gram_states(&F.sectors[0], &F.sectors[1], (int32_t)F.bil.size(), F.bil.data(), F.bir.data(), (int32_t)nstates, Psi, ldpsi, (int32_t)T.ops[0].size(), T.ops[0].data(), (int32_t)T.ops[1].size(), T.ops[1].data(),
                                               (int32_t)nv, first.data(), all.data(), workspace, g.dev_uninitialised(), nf, nullptr, nullptr)) SETERRQ1(PETSC_COMM_SELF, 1, "dmrgx_kron_term_gram_states: %s", dmrgx_last_error());
        if (dmrgx_memcpy_d2h(G.data(), g.dev_ro(), G.size() * sizeof(double), nullptr)) SETERRQ1(PETSC_COMM_SELF, 1, "%s", dmrgx_last_error());
        return 0;
    }
public:
    /** dst + b ld = D_b psi for all nb bonds, through dmrgx_kron_term_apply in chunks of at most 1 GiB of images (as SzFrame::Images). */
    PetscErrorCode Images(double* dst, int64_t ld) const
    {
        const PetscInt chunk = std::max<PetscInt>(1, std::min<PetscInt>(nb, (PetscInt)((((int64_t)1 << 30) / (int64_t)sizeof(double)) / std::max<int64_t>(ld, 1))));
        std::vector<int32_t> first;
        for (PetscInt b0 = 0; b0 < nb; b0 += chunk) {
            const PetscInt cnt = std::min<PetscInt>(chunk, nb - b0);
            const int32_t t0 = vec_first[(size_t)b0];
            first.clear();
            for (PetscInt b = b0; b <= b0 + cnt; ++b) first.push_back(vec_first[(size_t)b] - t0);
            if (dmrgx_kron_term_apply(&F.sectors[0], &F.sectors[1], (int32_t)F.bil.size(), F.bil.data(), F.bir.data(), psi, (int32_t)T.ops[0].size(), T.ops[0].data(), (int32_t)T.ops[1].size(), T.ops[1].data(),
                                      (int32_t)cnt, first.data(), terms.data() + t0, dst + b0 * ld, ld, nullptr)) SETERRQ1(PETSC_COMM_SELF, 1, "dmrgx_kron_term_apply: %s", dmrgx_last_error());
        }
        return 0;
    }
private:
    /** bond_op[b] of every bond inside a block, dense per sector:
        C[q] = Sz_i[q] Sz_j[q] + (Sp_i / 2)[q -> q+1] Sm_j[q+1 -> q] + (Sm_i / 2)[q -> q-1] Sp_j[q-1 -> q] */
    PetscErrorCode BuildBondOperators()
    {
        PetscErrorCode ierr;
        bond_op.assign((size_t)nb, Mat());
        for (int side = 0; side < 2; ++side) {
            const std::vector<int32_t>& sz = F.sizes[side];
            const int32_t ns = (int32_t)sz.size();
            enum { DSz = 0, DSp = 1, DSm = 2, DHalfSp = 3, DHalfSm = 4 };
            std::map<std::pair<int, PetscInt>, Mat> dense;          /* (kind, block site) -> dense form, for this measurement */
            auto densify = [&](int kind, PetscInt s, Mat& d) -> PetscErrorCode {
                auto it = dense.find({kind, s});
                if (it != dense.end()) { d = it->second; return 0; }
                Mat m;
                PetscErrorCode e = F.resident(side, kind == DSz ? OpSz : OpSp, s, m); CHKERRQ(e);
                if (kind == DSm || kind == DHalfSm) {               /* Sm(s) = Sp(s) read transposed */
                    auto v = std::make_shared<SectorMat>();
                    v->transpose_of = m; v->shift = OpSm; v->sizes = m->sizes;
                    m = v;
                }
                if (SectorMatDensify(m, d, kind >= DHalfSp ? 0.5 : 1.0)) SETERRQ2(PETSC_COMM_SELF, 1, "%s: densifying a site operator: %s", F.name, dmrgx_last_error());
                dense[{kind, s}] = d;
                return 0;
            };
            auto cell_at = [](const Mat& M, int32_t q) -> const MatCell* { for (const MatCell& c : M->cells) if (c.q == q) return &c; return nullptr; };
            std::vector<dmrgx_ggemm_group> groups;
            std::vector<dmrgx_ggemm_prod> prods;
            std::vector<size_t> first_prod;
            int64_t chunk_elems = 0, total = 0;
            for (int32_t q = 0; q < ns; ++q) total += (int64_t)sz[(size_t)q] * sz[(size_t)q];
            const int64_t chunk_limit = (int64_t)1 << 28;           /* 2 GiB of bond operators per grouped launch */
            auto flush = [&]() -> PetscErrorCode {
                for (size_t g = 0; g < groups.size(); ++g) groups[g].prods = prods.data() + first_prod[g];
                if (!groups.empty() && dmrgx_ggemm_groups((int32_t)groups.size(), groups.data(), 0, nullptr, nullptr)) SETERRQ1(PETSC_COMM_SELF, 1, "dmrgx_ggemm_groups: %s", dmrgx_last_error());
                groups.clear(); prods.clear(); first_prod.clear(); chunk_elems = 0;
                return 0;
            };
            for (PetscInt b = 0; b < nb; ++b) {
                if (side_of[(size_t)b] != side) continue;
                const PetscInt si = F.block_site(side, bonds[(size_t)b].i), sj = F.block_site(side, bonds[(size_t)b].j);
                Mat zi, zj, hpi, hmi, pj, mj;
                ierr = densify(DSz, si, zi); CHKERRQ(ierr); ierr = densify(DSz, sj, zj); CHKERRQ(ierr);
                ierr = densify(DHalfSp, si, hpi); CHKERRQ(ierr); ierr = densify(DSm, sj, mj); CHKERRQ(ierr);
                ierr = densify(DHalfSm, si, hmi); CHKERRQ(ierr); ierr = densify(DSp, sj, pj); CHKERRQ(ierr);
                if (chunk_elems + total > chunk_limit) { ierr = flush(); CHKERRQ(ierr); }
                Mat C = std::make_shared<SectorMat>();
                C->shift = 0; C->sizes = sz;
                auto arena = std::make_shared<DevBuffer>((size_t)std::max<int64_t>(total, 1), DevBuffer::device_only_t{});
                int64_t cursor = 0;
                for (int32_t q = 0; q < ns; ++q) {
                    const int32_t nq = sz[(size_t)q];
                    MatCell c;
                    c.q = q; c.nr = c.nc = nq; c.ld = nq; c.buf = arena; c.off = cursor;
                    C->cells.push_back(c);
                    first_prod.push_back(prods.size());
                    int32_t np = 0;
                    auto product = [&](const Mat& A, const Mat& B, int32_t qmid) {        /* A[q -> qmid] B[qmid -> q] */
                        if (qmid < 0 || qmid >= ns) return;
                        const MatCell* a = cell_at(A, q);
                        const MatCell* bb = cell_at(B, qmid);
                        if (!a || !bb) return;
                        prods.push_back(dmrgx_ggemm_prod{0, sz[(size_t)qmid], a->buf->dev_ro() + a->off, a->ld, bb->buf->dev_ro() + bb->off, bb->ld, 1.0});
                        ++np;
                    };
                    product(zi, zj, q); product(hpi, mj, q + 1); product(hmi, pj, q - 1);
                    groups.push_back(dmrgx_ggemm_group{arena->dev_uninitialised() + cursor, nq, nq, nq, 0, np, nullptr});
                    cursor += (int64_t)nq * nq;
                }
                chunk_elems += total;
                bond_doubles += total;
                bond_op[(size_t)b] = C;
            }
            ierr = flush(); CHKERRQ(ierr);
        }                                                           /* (the dense site operators go back to the pool here: stream-ordered) */
        return 0;
    }
};

/** A plaquette of the lattice: the sites a = (x, y), b = (x + 1, y), c = (x + 1, y + 1), d = (x, y + 1) in s[0 .. 4), y + 1 taken round
    the periodic direction, generated from the corner a = (x, y). */
struct ChiralPlaquette { PetscInt s[4], x, y; };
/** The plaquettes all four of whose edges a-b, b-c, c-d, d-a are among the distinct pairs of Ham.NeighborPairs(), in order of (x, y),
    each set of four sites once: on Ly = 2 the plaquette generated at y = 1 is the one of y = 0 again and is dropped, as DimerBonds drops
    the doubled vertical pair. */
template<class Hamiltonian> std::vector<ChiralPlaquette> ChiralPlaquettes(const Hamiltonian& Ham)
{
    std::set<std::pair<PetscInt, PetscInt>> nn;
    for (const std::vector<PetscInt>& p : Ham.NeighborPairs()) nn.insert({std::min(p[0], p[1]), std::max(p[0], p[1])});
    std::vector<ChiralPlaquette> plaq;
    std::set<std::vector<PetscInt>> seen;
    const PetscInt Lx = Ham.Lx(), Ly = Ham.Ly();
    for (PetscInt x = 0; x + 1 < Lx; ++x) for (PetscInt y = 0; y < Ly; ++y) {
        const PetscInt y1 = (y + 1) % Ly;
        const ChiralPlaquette P{{Ham.To1D(x, y), Ham.To1D(x + 1, y), Ham.To1D(x + 1, y1), Ham.To1D(x, y1)}, x, y};
        bool edges = true;
        for (int e = 0; e < 4; ++e) edges = edges && nn.count({std::min(P.s[e], P.s[(e + 1) % 4]), std::max(P.s[e], P.s[(e + 1) % 4])});
        std::vector<PetscInt> key(P.s, P.s + 4);
        std::sort(key.begin(), key.end());
        if (edges && seen.insert(key).second) plaq.push_back(P);
    }
    return plaq;
}

/** A triangle of a plaquette: the ordered, counter-clockwise triple (i, j, k) = three consecutive corners starting at corner `kind` --
    kind 0 .. 3 = (a, b, c), (b, c, d), (c, d, a), (d, a, b) --, its plaquette and that plaquette's position. */
struct ChiralTriangle { PetscInt i, j, k; int kind; PetscInt plaq, x, y; };
inline std::vector<ChiralTriangle> ChiralTriangles(const std::vector<ChiralPlaquette>& plaq)
{
    std::vector<ChiralTriangle> tri;
    for (size_t p = 0; p < plaq.size(); ++p)
        for (int kind = 0; kind < 4; ++kind) tri.push_back(ChiralTriangle{plaq[p].s[kind], plaq[p].s[(kind + 1) % 4], plaq[p].s[(kind + 2) % 4], kind, (PetscInt)p, plaq[p].x, plaq[p].y});
    return tri;
}

/** One string c O_1(s_1) O_2(s_2) O_3(s_3) of three site operators on lattice sites. */
struct ChiralString { double coeff; Op_t type[3]; PetscInt site[3]; };
/** chi_ijk = S_i . (S_j x S_k) = i K_ijk with the real, antisymmetric
      K_ijk = [ Sz_i (Sp_j Sm_k - Sm_j Sp_k) + Sz_j (Sp_k Sm_i - Sm_k Sp_i) + Sz_k (Sp_i Sm_j - Sm_i Sp_j) ] / 2:
    its six strings in this order, the site operators of each in the order written. */
inline std::vector<ChiralString> ChiralStrings(PetscInt i, PetscInt j, PetscInt k)
{
    const PetscInt s[3] = {i, j, k};
    std::vector<ChiralString> out;
    for (int r = 0; r < 3; ++r) {
        const PetscInt a = s[r], b = s[(r + 1) % 3], c = s[(r + 2) % 3];
        out.push_back(ChiralString{+0.5, {OpSz, OpSp, OpSm}, {a, b, c}});
        out.push_back(ChiralString{-0.5, {OpSz, OpSm, OpSp}, {a, b, c}});
    }
    return out;
}

/** The factors of a string that fall on one side of the cut behind the first n_left lattice sites, in their order in the string: (operator,
    BLOCK site) pairs -- site s of the right block is lattice site N - 1 - s.  The two parts of a string have opposite sector shifts. */
typedef std::vector<std::pair<int, PetscInt>> ChiralPart;
inline ChiralPart ChiralStringPart(const ChiralString& S, int side, PetscInt n_left, PetscInt N)
{
    ChiralPart part;
    for (int f = 0; f < 3; ++f)
        if ((S.site[f] < n_left ? 0 : 1) == side) part.push_back({(int)S.type[f], side == 0 ? S.site[f] : N - 1 - S.site[f]});
    return part;
}

/** K_a of every triangle of the lattice as terms on the ground state: the set-up of -corr_chiral.  A string of K_a splits at the cut into
    a left and a right part of 0 to 3 factors, each side's factors in their order in the string.  A part of one factor is the resident site
    operator; a part of two factors is a composed operator -- dmrgx_secop_compose, one per (ordered block sites, operator kinds), shared by
    every triangle that uses it --; a triangle wholly inside a block is ONE composed operator of shift 0, the sum of its six strings, and one
    one-sided term.  A triangle across the cut is six two-sided terms.  Triangle a is terms[vec_first[a] .. vec_first[a + 1]) over the
    operators of T.  side_of[a]: 0 / 1 inside the left / right block, 2: two sites left and one right, 3: one left and two right.
    The composed operators (composed_doubles doubles) live as long as the frame; they are built in chunks of about 2 GiB of operators
    and prefixes per call. */
struct ChiralFrame {
    CentreFrame F;
    SiteOperators T{F};
    std::vector<ChiralPlaquette> plaquettes;
    std::vector<ChiralTriangle> triangles;
    std::vector<int> side_of;
    std::vector<Mat> composed;
    std::vector<int32_t> vec_first;
    std::vector<dmrgx_term> terms;
    PetscInt nt = 0;
    int64_t n = 0, composed_doubles = 0;
    const double* psi = nullptr;
    template<class Hamiltonian> PetscErrorCode Init(KronBlocks_t& KronBlocks, PetscInt num_sites, const Hamiltonian& Ham, const Vec& gsv_r, const char* display_name)
    {
        PetscErrorCode ierr = F.Init(KronBlocks, num_sites, display_name); CHKERRQ(ierr);
        plaquettes = ChiralPlaquettes(Ham);
        triangles = ChiralTriangles(plaquettes);
        nt = (PetscInt)triangles.size();
        n = gsv_r->n; psi = gsv_r->buf->dev_ro();
        /* a term names a part by (composed, index): the index of a site operator in T.ops[side], or of an output in want[side] */
        struct Ref { bool composed; int32_t idx; };
        struct Pending { double coeff; Ref part[2]; };
        std::vector<Pending> pending;
        vec_first.assign(1, 0);
        for (const ChiralTriangle& t : triangles) {
            const PetscInt nl = (t.i < F.nsites[0]) + (t.j < F.nsites[0]) + (t.k < F.nsites[0]);
            const std::vector<ChiralString> strings = ChiralStrings(t.i, t.j, t.k);
            side_of.push_back(nl == 3 ? 0 : (nl == 0 ? 1 : (nl == 2 ? 2 : 3)));
            if (nl == 3 || nl == 0) {
                const int side = nl == 3 ? 0 : 1;
                Output O;
                for (const ChiralString& S : strings) { ierr = AddString(side, S.coeff, ChiralStringPart(S, side, F.nsites[0], F.N), O); CHKERRQ(ierr); }
                want[side].push_back(O);
                Pending P{1.0, {{false, -1}, {false, -1}}};
                P.part[side] = Ref{true, (int32_t)want[side].size() - 1};
                pending.push_back(P);
            } else {
                for (const ChiralString& S : strings) {
                    Pending P{S.coeff, {{false, -1}, {false, -1}}};
                    for (int side = 0; side < 2; ++side) {
                        const ChiralPart part = ChiralStringPart(S, side, F.nsites[0], F.N);
                        if (part.size() == 1) { ierr = T.Site(side, (Op_t)part[0].first, part[0].second, P.part[side].idx); CHKERRQ(ierr); continue; }
                        auto ins = shared[side].emplace(part, (int32_t)want[side].size());
                        if (ins.second) { Output O; ierr = AddString(side, 1.0, part, O); CHKERRQ(ierr); want[side].push_back(O); }
                        P.part[side] = Ref{true, ins.first->second};
                    }
                    pending.push_back(P);
                }
            }
            vec_first.push_back((int32_t)pending.size());
        }
        int32_t first_composed[2] = {0, 0};
        for (int side = 0; side < 2; ++side) { first_composed[side] = (int32_t)T.ops[side].size(); ierr = Compose(side); CHKERRQ(ierr); }
        for (const Pending& P : pending) {
            int32_t idx[2];
            for (int side = 0; side < 2; ++side) idx[side] = P.part[side].composed ? first_composed[side] + P.part[side].idx : P.part[side].idx;
            terms.push_back(dmrgx_term{P.coeff, idx[0], idx[1]});
        }
        for (int side = 0; side < 2; ++side) { want[side].clear(); shared[side].clear(); }
        return 0;
    }
    /** G ((nt + 1) x (nt + 1), row-major, host): the Gram matrix of psi (vector 0) and the images K_a psi (vector 1 + a), ONE dmrgx_kron_term_gram call. */
    PetscErrorCode Gram(std::vector<double>& G) const
    {
        const PetscInt nv = nt + 1;
        std::vector<int32_t> first{0};
        std::vector<dmrgx_term> all;
        all.push_back(dmrgx_term{1.0, -1, -1});
        all.insert(all.end(), terms.begin(), terms.end());
        for (int32_t f : vec_first) first.push_back(f + 1);
        /* the workspace holds at least the largest image block of every vector: a part shifts by at most one sector, the blocks (IL - d, IR + d) */
        int64_t largest = 1;
        for (size_t k = 0; k < F.bil.size(); ++k)
            for (int32_t d = -1; d <= 1; ++d) {
                const int32_t a = F.bil[k] - d, c = F.bir[k] + d;
                if (a >= 0 && a < (int32_t)F.sizes[0].size() && c >= 0 && c < (int32_t)F.sizes[1].size()) largest = std::max<int64_t>(largest, (int64_t)F.sizes[0][(size_t)a] * F.sizes[1][(size_t)c]);
            }
        const size_t workspace = std::max<size_t>((size_t)1 << 30, (size_t)largest * (size_t)nv * sizeof(double));
        G.assign((size_t)(nv * nv), 0.0);
        DevBuffer g((size_t)(nv * nv), DevBuffer::device_only_t{});
        if (dmrgx_kron_term_gram(&F.sectors[0], &F.sectors[1], (int32_t)F.bil.size(), F.bil.data(), F.bir.data(), psi, (int32_t)T.ops[0].size(), T.ops[0].data(), (int32_t)T.ops[1].size(), T.ops[1].data(),
                                 (int32_t)nv, first.data(), all.data(), workspace, g.dev_uninitialised(), nv, nullptr, nullptr)) SETERRQ1(PETSC_COMM_SELF, 1, "dmrgx_kron_term_gram: %s", dmrgx_last_error());
        if (dmrgx_memcpy_d2h(G.data(), g.dev_ro(), G.size() * sizeof(double), nullptr)) SETERRQ1(PETSC_COMM_SELF, 1, "%s", dmrgx_last_error());
        return 0;
    }
    /** dst + a ld = K_a psi for all nt triangles, through dmrgx_kron_term_apply in chunks of at most 1 GiB of images (as DimerFrame::Images). */
    PetscErrorCode Images(double* dst, int64_t ld) const
    {
        const PetscInt chunk = std::max<PetscInt>(1, std::min<PetscInt>(nt, (PetscInt)((((int64_t)1 << 30) / (int64_t)sizeof(double)) / std::max<int64_t>(ld, 1))));
        std::vector<int32_t> first;
        for (PetscInt a0 = 0; a0 < nt; a0 += chunk) {
            const PetscInt cnt = std::min<PetscInt>(chunk, nt - a0);
            const int32_t t0 = vec_first[(size_t)a0];
            first.clear();
            for (PetscInt a = a0; a <= a0 + cnt; ++a) first.push_back(vec_first[(size_t)a] - t0);
            if (dmrgx_kron_term_apply(&F.sectors[0], &F.sectors[1], (int32_t)F.bil.size(), F.bil.data(), F.bir.data(), psi, (int32_t)T.ops[0].size(), T.ops[0].data(), (int32_t)T.ops[1].size(), T.ops[1].data(),
                                      (int32_t)cnt, first.data(), terms.data() + t0, dst + a0 * ld, ld, nullptr)) SETERRQ1(PETSC_COMM_SELF, 1, "dmrgx_kron_term_apply: %s", dmrgx_last_error());
        }
        return 0;
    }
private:
    typedef std::vector<dmrgx_secop_string> Output;             /* the strings of one composed operator, factors by index into T.ops[side] */
    std::vector<Output> want[2];
    std::map<ChiralPart, int32_t> shared[2];                    /* two-factor part -> its output in want[side] */
    PetscErrorCode AddString(int side, double coeff, const ChiralPart& part, Output& O)
    {
        dmrgx_secop_string s{coeff, (int32_t)part.size(), {0, 0, 0}};
        for (size_t f = 0; f < part.size(); ++f) { PetscErrorCode ierr = T.Site(side, (Op_t)part[f].first, part[f].second, s.fac[f]); CHKERRQ(ierr); }
        O.push_back(s);
        return 0;
    }
    /** The outputs of want[side] through dmrgx_secop_compose, appended to T.ops[side] in their order. */
    PetscErrorCode Compose(int side)
    {
        const std::vector<int32_t>& sz = F.sizes[side];
        const int32_t ns = (int32_t)sz.size(), n_in = (int32_t)T.ops[side].size();
        int64_t block = 0;                                          /* an upper bound of one operator or prefix: the largest shift-s table */
        for (int32_t s = -1; s <= 1; ++s) { int64_t b = 0; for (int32_t q = 0; q < ns; ++q) if (q + s >= 0 && q + s < ns) b += (int64_t)sz[(size_t)q] * sz[(size_t)(q + s)]; block = std::max(block, b); }
        const int64_t chunk_limit = (int64_t)1 << 28;
        const std::vector<dmrgx_secop> inputs(T.ops[side].begin(), T.ops[side].begin() + n_in);
        for (size_t o0 = 0; o0 < want[side].size();) {
            std::vector<int32_t> first{0};
            std::vector<dmrgx_secop_string> strings;
            int64_t cost = 0;
            size_t o1 = o0;
            for (; o1 < want[side].size(); ++o1) {
                int64_t c = block;
                for (const dmrgx_secop_string& s : want[side][o1]) if (s.nfac == 3) c += block;
                if (o1 > o0 && cost + c > chunk_limit) break;
                cost += c;
                strings.insert(strings.end(), want[side][o1].begin(), want[side][o1].end());
                first.push_back((int32_t)strings.size());
            }
            const int32_t cnt = (int32_t)(o1 - o0);
            std::vector<int32_t> shift((size_t)cnt), cell_first((size_t)cnt + 1);
            std::vector<dmrgx_cell> cells((size_t)cnt * (size_t)ns);
            int64_t total = 0;
            if (dmrgx_secop_compose(&F.sectors[side], n_in, inputs.data(), cnt, first.data(), strings.data(), shift.data(), cell_first.data(), cells.data(), &total, nullptr, nullptr))
                SETERRQ2(PETSC_COMM_SELF, 1, "%s: dmrgx_secop_compose: %s", F.name, dmrgx_last_error());
            std::shared_ptr<DevBuffer> arena;
            try { arena = std::make_shared<DevBuffer>((size_t)std::max<int64_t>(total, 1), DevBuffer::device_only_t{}); }
            catch (const std::exception& e) { SETERRQ4(PETSC_COMM_SELF, PETSC_ERR_MEM, "%s: no memory for %d composed operators (%.3f GB): %s", F.name, (int)cnt, (double)total * 8e-9, e.what()); }
            double* base = arena->dev_uninitialised();
            if (dmrgx_secop_compose(&F.sectors[side], n_in, inputs.data(), cnt, first.data(), strings.data(), shift.data(), cell_first.data(), cells.data(), &total, base, nullptr))
                SETERRQ2(PETSC_COMM_SELF, 1, "%s: dmrgx_secop_compose: %s", F.name, dmrgx_last_error());
            for (int32_t o = 0; o < cnt; ++o) {
                Mat C = std::make_shared<SectorMat>();
                C->shift = shift[(size_t)o]; C->sizes = sz;
                for (int32_t ci = cell_first[(size_t)o]; ci < cell_first[(size_t)o + 1]; ++ci) {
                    const dmrgx_cell& d = cells[(size_t)ci];
                    MatCell c;
                    c.q = d.row_sector; c.nr = d.nr; c.nc = d.nc; c.ld = d.ld; c.buf = arena; c.off = (int64_t)(d.data - base);
                    C->cells.push_back(c);
                }
                T.Add(side, C);
                composed.push_back(C);
            }
            composed_doubles += total;
            o0 = o1;
        }
        return 0;
    }
};

/** A JSON file that holds one list of records, one per measurement: created by the first Begin(), finished by Close().  The caller
    writes the record itself to fp; numbers of Row() and Table() go through `number`, a printf format for one double. */
struct JsonRecordFile {
    const char* const number;
    FILE* fp = NULL;
    explicit JsonRecordFile(const char* number) : number(number) {}
    JsonRecordFile(const JsonRecordFile&) = delete;
    ~JsonRecordFile() { if (fp) fclose(fp); }                   /* (an error path: the list stays open-ended) */
    /** Start a record: "[\n" in a new file, ",\n" after the record before. */
    PetscErrorCode Begin(const std::string& path)
    {
        const bool first = !fp;
        if (first && !(fp = fopen(path.c_str(), "w"))) SETERRQ1(PETSC_COMM_SELF, PETSC_ERR_FILE_OPEN, "Cannot open %s", path.c_str());
        fprintf(fp, first ? "[\n" : ",\n");
        return 0;
    }
    void Row(const double* v, PetscInt cnt) const { fprintf(fp, "["); for (PetscInt i = 0; i < cnt; ++i) { fprintf(fp, "%s", i ? ", " : ""); fprintf(fp, number, v[i]); } fprintf(fp, "]"); }
    void Row(const std::vector<double>& v) const { Row(v.data(), (PetscInt)v.size()); }
    void Table(const char* name, const std::vector<double>& T, PetscInt nr, PetscInt nc, const char* end) const
    {
        fprintf(fp, "   \"%s\": [\n", name);
        for (PetscInt i = 0; i < nr; ++i) { fprintf(fp, "     "); Row(T.data() + i * nc, nc); fprintf(fp, "%s\n", i + 1 < nr ? "," : ""); }
        fprintf(fp, "   ]%s", end);
    }
    /** Begin() and how the record of a dynamical measurement opens; in it, how the entry of a reference site opens.  The caller goes on with ", ...". */
    PetscErrorCode BeginDynamical(const std::string& path, PetscInt glob_idx, const char* loop_type, double E0, double norm)
    {
        const PetscErrorCode ierr = Begin(path);
        if (!ierr) fprintf(fp, "  {\"GlobIdx\": %lld, \"LoopType\": \"%s\", \"E0\": %.17g, \"Norm\": %.17g", LLD(glob_idx), loop_type, E0, norm);
        return ierr;
    }
    void OpenSite(PetscInt c, PetscInt x, PetscInt y, double norm2) const { fprintf(fp, "   {\"Site\": %lld, \"r\": [%lld, %lld], \"Norm2\": %.17g", LLD(c), LLD(x), LLD(y), norm2); }
    /** The optional "Omega" row in the head of a Chebyshev record. */
    void Omega(const std::vector<double>* omega) const { if (omega) { fprintf(fp, "   \"Omega\": "); Row(*omega); fprintf(fp, ",\n"); } }
    /** The moment part of the entry of one run, after the caller's "..., \"StepsDone\": d": Diag, Moments (rows x (done + 1)), MomentsQ
        (M x (done + 1)) and, where frequencies were asked for, SqwGrid (M x their number); `end` closes the entry. */
    void Moments(const MomentRun& R, PetscInt rows, PetscInt M, const std::vector<double>* omega, const char* end) const
    {
        const PetscInt nm = R.done + 1;
        fprintf(fp, ",\n   \"Diag\": ");
        Row(R.diag); fprintf(fp, ",\n");
        Table("Moments", R.mom, rows, nm, ",\n");
        Table("MomentsQ", R.momq, M, nm, omega ? ",\n" : end);
        if (omega) Table("SqwGrid", R.grid, M, (PetscInt)omega->size(), end);
    }
    /** "Bonds", "Orientation", "Position" of the bonds and "D" = < D_b >, as -corr_dimer and -dsf_dimer write them, each line closed. */
    void BondHeader(const std::vector<DimerBond>& bonds, const std::vector<double>& D) const
    {
        BondList(bonds);
        fprintf(fp, "   \"D\": ");
        Row(D); fprintf(fp, ",\n");
    }
    /** The bond list of BondHeader without "D" (-states_corr, whose D is a table per pair of states). */
    void BondList(const std::vector<DimerBond>& bonds) const
    {
        const size_t nb = bonds.size();
        fprintf(fp, "   \"Bonds\": [");
        for (size_t b = 0; b < nb; ++b) fprintf(fp, "%s[%lld, %lld]", b ? ", " : "", LLD(bonds[b].i), LLD(bonds[b].j));
        fprintf(fp, "],\n   \"Orientation\": [");
        for (size_t b = 0; b < nb; ++b) fprintf(fp, "%s\"%c\"", b ? ", " : "", bonds[b].orient);
        fprintf(fp, "],\n   \"Position\": [");
        for (size_t b = 0; b < nb; ++b) fprintf(fp, "%s[%lld, %lld]", b ? ", " : "", LLD(bonds[b].ix), LLD(bonds[b].jy));
        fprintf(fp, "],\n");
    }
    void Close() { if (fp) { fprintf(fp, "\n]\n"); fclose(fp); fp = NULL; } }
};

}  // namespace dmrgx_host
#endif
