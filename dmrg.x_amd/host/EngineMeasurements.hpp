#ifndef DMRGX_HOST_ENGINEMEASUREMENTS_HPP
#define DMRGX_HOST_ENGINEMEASUREMENTS_HPP
/** The eleven engine-extension measurements of the sweep engine, on top of what they share (Measurements.hpp): -corr_matrix, -corr_dimer,
    -corr_chiral, -dsf, -dsf_sites, -dsf_cheb, -dsf_dimer, -dsf_pm, -dsf_cv, -chi_sites / -chi_bonds and -states_corr.  Each is a struct of its flag, its options, its record
    file, a ReadOptions and a Run; EngineMeasurements holds the eleven as plain members and calls them in a fixed order.  What a Run needs
    from the step comes in a MeasurementContext, the lattice through a template parameter: nothing here depends on the block or the
    container class, so host_tool.cpp reads the options without a GPU (command measopts). */
#include <random>
#include <set>
#include "Measurements.hpp"

namespace dmrgx_host {

/** The states of a step with -nstates k > 1: count rows of stride ld on the device, row s the state s in the layout of psi (row 0 is psi),
    and their energies.  Empty (count 0) with -nstates 1 and in a step whose sector holds one state. */
struct TargetedStatesView { const double* rows = nullptr; int64_t ld = 0; PetscInt count = 0; const double* energies = nullptr; };

/** What a measurement reads of the DMRG step it runs in.  The step fills it once, after the eigensolve. */
struct MeasurementContext {
    KronBlocks_t& KronBlocks;
    const Vec& psi;                                         /* the ground state */
    Mat* H;                                                 /* the step's superblock Hamiltonian; *H is null once its plan is destroyed */
    const std::vector<Hamiltonians::Term>& Terms;
    PetscScalar E0;
    PetscInt num_sites; PetscReal qn_sector; PetscInt GlobIdx; const char* loop_type;      /* loop_type: "LoopType" in a record */
    PetscBool verbose, do_shell;
    MPI_Comm mpi_comm; PetscMPIInt mpi_rank, mpi_size;
    const std::string& data_dir;
    TargetedStatesView states;                              /* -nstates k > 1: all states of the step */
    dmrgx_kron_plan* plan() const { return (*H)->plan; }
};

/** A site-list option (-dsf_sites, -dsf_cheb, -dsf_pm, -dsf_cv c0,c1,...): on when present and not empty; then refused on more than one rank
    (`what` has no collectives), and every site must be one of the `count` lattice sites.  -dsf_dimer: a list of `noun`s out of [0, count). */
inline PetscErrorCode ReadSiteListOption(MPI_Comm comm, PetscMPIInt size, const char* option, const char* what, std::vector<PetscInt>& sites, PetscBool& use,
                                         PetscInt count, const char* noun = "site", const char* range = "the lattice sites in the numbering of To1D")
{
    PetscBool have_sites = PETSC_FALSE;
    PetscInt nc = 4096;
    sites.assign((size_t)nc, 0);
    PetscErrorCode ierr = PetscOptionsGetIntArray(NULL, NULL, option, sites.data(), &nc, &have_sites); CHKERRQ(ierr);
    sites.resize(have_sites ? (size_t)nc : 0);
    use = (have_sites && nc > 0) ? PETSC_TRUE : PETSC_FALSE;
    if (!use) return 0;
    if (size > 1) SETERRQ3(comm, PETSC_ERR_SUP, "%s is not available on more than one rank (got %d): %s has no collectives.", option, (int)size, what);
    for (PetscInt c : sites) if (c < 0 || c >= count) SETERRQ5(comm, PETSC_ERR_ARG_OUTOFRANGE, "%s: %s %lld is outside [0, %lld), %s.", option, noun, LLD(c), LLD(count), range);
    return 0;
}

/** A frequency grid w0,w1,nw (-dsf_cheb_omega, -dsf_dimer_omega, -dsf_cv_omega): `have` if the option is there, then `grid` or the refusal. */
inline PetscErrorCode ReadOmegaGridOption(MPI_Comm comm, const char* option, std::vector<double>& grid, PetscBool& have)
{
    PetscInt no = 3;
    PetscReal om[3] = {0.0, 0.0, 0.0};
    PetscErrorCode ierr = PetscOptionsGetRealArray(NULL, NULL, option, om, &no, &have); CHKERRQ(ierr);
    if (have && !OmegaGrid(om, no, grid)) SETERRQ2(comm, PETSC_ERR_ARG_WRONG, "%s needs w0,w1,nw: nw >= 1 frequencies from w0 to w1 (nw = 1: w0 = w1). Got %lld numbers.", option, LLD(no));
    return 0;
}

/** -dsf_steps and -dsf_breakdown_tol, which -dsf and -dsf_sites share: read by the first of the two that is on. */
struct LanczosStepOptions {
    PetscInt steps = 100;                       /* -dsf_steps: Lanczos steps per run */
    PetscReal breakdown_tol = 0.0;              /* -dsf_breakdown_tol: 0 = the library's default, 1e-7 */
    bool read = false;
    PetscErrorCode ReadOnce(MPI_Comm comm)
    {
        if (read) return 0;
        read = true;
        PetscErrorCode ierr = PetscOptionsGetInt(NULL, NULL, "-dsf_steps", &steps, NULL); CHKERRQ(ierr);
        if (steps < 1) SETERRQ1(comm, PETSC_ERR_ARG_OUTOFRANGE, "-dsf_steps must be at least 1. Got %lld.", LLD(steps));
        ierr = PetscOptionsGetReal(NULL, NULL, "-dsf_breakdown_tol", &breakdown_tol, NULL); CHKERRQ(ierr);
        if (!(breakdown_tol >= 0.0) || breakdown_tol >= 1.0) SETERRQ1(comm, PETSC_ERR_ARG_OUTOFRANGE, "-dsf_breakdown_tol must lie in [0, 1). Got %g.", breakdown_tol);
        return 0;
    }
};

/** The options of the Chebyshev expansion and the window they lead to.  Steps and grid are those of -dsf_cheb and -dsf_pm; the window is
    shared by these two and -dsf_dimer.  Read(): after the lists of all three, the steps before the window (the order of the refusals). */
struct ChebyshevOptions {
    PetscInt steps = 200;                       /* -dsf_cheb_steps: MatMults per run; moments 0 .. steps between sites, 0 .. 2 steps on the diagonal */
    PetscInt bound_steps = 40;                  /* -dsf_cheb_bound_steps: Lanczos steps of the run that finds the top of the spectrum */
    PetscBool have_window = PETSC_FALSE, have_omega = PETSC_FALSE;
    PetscReal window[2] = {0.0, 0.0};           /* -dsf_cheb_window lo,hi: the window given, no bound run */
    std::vector<double> omega;                  /* -dsf_cheb_omega w0,w1,nw: the grid of the Jackson-broadened SqwGrid */
    const std::vector<double>* grid() const { return have_omega ? &omega : nullptr; }

    PetscErrorCode Read(MPI_Comm comm, bool cheb, bool dimer, bool pm)
    {
        PetscErrorCode ierr;
        if (cheb || pm) {
            ierr = PetscOptionsGetInt(NULL, NULL, "-dsf_cheb_steps", &steps, NULL); CHKERRQ(ierr);
            if (steps < 1) SETERRQ1(comm, PETSC_ERR_ARG_OUTOFRANGE, "-dsf_cheb_steps must be at least 1. Got %lld.", LLD(steps));
            ierr = ReadOmegaGridOption(comm, "-dsf_cheb_omega", omega, have_omega); CHKERRQ(ierr);
        }
        if (cheb || dimer || pm) {   /* the window of the Chebyshev expansion, which the three share */
            ierr = PetscOptionsGetInt(NULL, NULL, "-dsf_cheb_bound_steps", &bound_steps, NULL); CHKERRQ(ierr);
            if (bound_steps < 1) SETERRQ1(comm, PETSC_ERR_ARG_OUTOFRANGE, "-dsf_cheb_bound_steps must be at least 1. Got %lld.", LLD(bound_steps));
            PetscInt nw = 2;
            ierr = PetscOptionsGetRealArray(NULL, NULL, "-dsf_cheb_window", window, &nw, &have_window); CHKERRQ(ierr);
            if (have_window && !(nw == 2 && window[0] < window[1] && std::isfinite(window[0]) && std::isfinite(window[1])))
                SETERRQ1(comm, PETSC_ERR_ARG_WRONG, "-dsf_cheb_window needs lo,hi: two finite energies, lo < hi. Got %lld numbers.", LLD(nw));
        }
        return 0;
    }

    /** The window of a Chebyshev expansion on the planned Hamiltonian of n states, for -dsf_cheb, -dsf_dimer and -dsf_pm: -dsf_cheb_window lo,hi as given
        (bound_steps 0, theta_min = lo, theta_max = hi), else from -dsf_cheb_bound_steps Lanczos steps from a fixed pseudo-random vector (BoundRun):
        above the known bottom *E0 (ChebyshevWindow, Measurements.hpp), or, E0 null, a sector whose bottom is not known (ChebyshevWindowTwoSided). */
    PetscErrorCode FindWindow(MPI_Comm comm, dmrgx_kron_plan* plan, int64_t n, const double* E0, const std::string& name, ChebyshevSpectralWindow& W) const
    {
        const double lo = window[0], hi = window[1];
        if (have_window) { W = ChebyshevSpectralWindow{0.5 * (lo + hi), 0.5 * (hi - lo), lo, hi, 0.0, 0.0, 0, true}; return 0; }
        std::vector<double> a, b;
        int32_t done = 0;
        PetscErrorCode ierr = BoundRun(comm, plan, n, a, b, done); CHKERRQ(ierr);
        W = E0 ? ChebyshevWindow(*E0, a, b, done) : ChebyshevWindowTwoSided(a, b, done);
        W.bound_steps = bound_steps;
        if (!W.ok) SETERRQ2(comm, 1, "%s: no spectral window from %d Lanczos steps.", name.c_str(), (int)done);
        return 0;
    }

    /** alpha, beta and the steps done of -dsf_cheb_bound_steps Lanczos steps (dmrgx_kron_lanczos_coeffs) on the planned Hamiltonian of n states from
        a fixed pseudo-random vector: what ChebyshevWindow and ChebyshevWindowTwoSided read. */
    PetscErrorCode BoundRun(MPI_Comm comm, dmrgx_kron_plan* plan, int64_t n, std::vector<double>& a, std::vector<double>& b, int32_t& done) const
    {
        const PetscInt B = bound_steps;
        DevBuffer r((size_t)n);
        {   /* uniform(-1, 1) from a fixed seed, by integer arithmetic on the generator's 64 bits: the same vector everywhere */
            std::mt19937_64 gen(0x63686562ull);
            double* h = r.host();
            for (int64_t e = 0; e < n; ++e) h[e] = (double)(gen() >> 11) * (2.0 / 9007199254740992.0) - 1.0;
        }
        a.assign((size_t)B, 0.0); b.assign((size_t)B, 0.0);
        double r2 = 0.0; done = 0;
        if (dmrgx_kron_lanczos_coeffs(plan, r.dev_ro(), (int32_t)B, 0.0, &r2, a.data(), b.data(), &done, nullptr)) SETERRQ1(comm, 1, "dmrgx_kron_lanczos_coeffs: %s", dmrgx_last_error());
        return 0;
    }
};

/** -corr_matrix 1 (engine extension): the full tables < Sz_i Sz_j >, < Sm_i Sp_j > and < Sp_i Sm_j > over all pairs of lattice sites,
    the spin correlation function < S_i . S_j > and its Fourier transform, the static structure factor, at every measurement point.
    < psi | O_i^T O_j | psi > = < O_i psi , O_j psi >: a table is the Gram matrix of the vectors O_i psi, so each is ONE
    dmrgx_kron_op_gram call -- the identity (which adds < Sz_i > and the norm) and Sz of every site of both blocks, shift 0; Sp of
    every site, shift +1; Sm of every site (Sp read transposed), shift -1 -- instead of a plan, a MatMult and a dot product per pair.
    < Sp_i Sm_j > is a table of its own because two TRUNCATED operators of one block do not commute: it equals < Sm_j Sp_i > only
    across the cut or when nothing was truncated, and the registered correlators multiply the operators in the order they name.
    Site s of the right block is lattice site N - 1 - s, as in SetUpCorrelation.  On several ranks every rank computes the same
    tables from the replicated psi (no collective); rank 0 writes one record per measurement to SpinCorrelations.json. */
struct CorrelationMatrix {
    PetscBool use = PETSC_FALSE;                /* -corr_matrix 1 */
    JsonRecordFile file{"%.15g"};               /* created at the first measurement, rank 0 only */
    PetscErrorCode ReadOptions() { return PetscOptionsGetBool(NULL, NULL, "-corr_matrix", &use, NULL); }

    template<class Hamiltonian> PetscErrorCode Run(const MeasurementContext& ctx, const Hamiltonian& Ham)
    {
        PetscLogDouble t0, t1;
        PetscTime(&t0);
        CentreFrame F;
        PetscErrorCode ierr = F.Init(ctx.KronBlocks, ctx.num_sites, "Correlation matrix"); CHKERRQ(ierr);
        const PetscInt N = F.N;
        std::vector<PetscInt> site;                                 /* lattice site of vector a of a family (identity: -1) */
        std::vector<double> G;
        /* one family: [identity] + the operator of every left site + of every right site; its Gram matrix G, and as a table over lattice sites */
        auto family = [&](Op_t type, bool with_identity, std::vector<double>& table) -> PetscErrorCode {
            SiteOperators T(F);
            site.clear();
            if (with_identity) { T.AddIdentity(0); site.push_back(-1); }
            PetscErrorCode e = T.AllSites(type, site); CHKERRQ(e);
            const PetscInt n = (PetscInt)site.size();
            DevBuffer g((size_t)(n * n), DevBuffer::device_only_t{});
            if (dmrgx_kron_op_gram(&F.sectors[0], &F.sectors[1], (int32_t)F.bil.size(), F.bil.data(), F.bir.data(), ctx.psi->buf->dev_ro(), (int32_t)T.ops[0].size(), T.ops[0].data(), (int32_t)T.ops[1].size(), T.ops[1].data(),
                                   0, g.dev_uninitialised(), n, nullptr, nullptr)) SETERRQ1(ctx.mpi_comm, 1, "dmrgx_kron_op_gram: %s", dmrgx_last_error());
            G.assign((size_t)(n * n), 0.0);
            if (dmrgx_memcpy_d2h(G.data(), g.dev_ro(), G.size() * sizeof(double), nullptr)) SETERRQ1(ctx.mpi_comm, 1, "%s", dmrgx_last_error());
            const PetscInt first = with_identity ? 1 : 0;
            for (PetscInt a = first; a < n; ++a) for (PetscInt b = first; b < n; ++b) table[(size_t)(site[(size_t)a] * N + site[(size_t)b])] = G[(size_t)(a * n + b)];
            return 0;
        };
        std::vector<double> SzSz((size_t)(N * N), 0.0), SmSp((size_t)(N * N), 0.0), SpSm((size_t)(N * N), 0.0), Sz((size_t)N, 0.0);
        ierr = family(OpSz, true, SzSz); CHKERRQ(ierr);
        const double norm = G[0];
        for (PetscInt a = 1; a <= N; ++a) Sz[(size_t)site[(size_t)a]] = G[(size_t)a];     /* < psi , Sz_i psi > */
        ierr = family(OpSp, false, SmSp); CHKERRQ(ierr);
        ierr = family(OpSm, false, SpSm); CHKERRQ(ierr);
        /* S_i . S_j = Sz_i Sz_j + (Sp_i Sm_j + Sm_i Sp_j) / 2: off the diagonal the spins commute and the state is real, so both halves equal
           < Sm_i Sp_j >; on the diagonal Sp Sm = Sm Sp + 2 Sz */
        std::vector<double> SS((size_t)(N * N), 0.0);
        for (PetscInt i = 0; i < N; ++i) for (PetscInt j = 0; j < N; ++j) SS[(size_t)(i * N + j)] = SzSz[(size_t)(i * N + j)] + SmSp[(size_t)(i * N + j)] + (i == j ? Sz[(size_t)i] : 0.0);
        /* S(q) = (1/N) sum_ij cos(q . (r_i - r_j)) SS_ij,  q = (2 pi nx / Lx, 2 pi ny / Ly) */
        const PetscInt Lx = Ham.Lx(), Ly = Ham.Ly();
        std::vector<PetscInt> rx((size_t)N), ry((size_t)N);
        for (PetscInt i = 0; i < N; ++i) { ierr = Ham.To2D(i, rx[(size_t)i], ry[(size_t)i]); CHKERRQ(ierr); }
        const std::vector<double> Sq = LatticeFourier(Lx, Ly, rx.data(), ry.data(), SS.data(), N, (double)N);
        PetscTime(&t1);
        if (!ctx.mpi_rank && ctx.verbose) {
            /* what the two Gram kernels must read: vectors x length of the image space (shift 0: the target sector itself) */
            int64_t len_shifted[2] = {0, 0};                         /* image space of Sp (sector shift +1), of Sm (-1) */
            for (int d = 0; d < 2; ++d) {
                const int32_t sh = d == 0 ? 1 : -1;
                std::set<std::pair<int32_t, int32_t>> img;
                for (size_t k = 0; k < F.bil.size(); ++k) {
                    const int32_t a = F.bil[k] - sh, b = F.bir[k] - sh;
                    if (a >= 0 && a < (int32_t)F.sizes[0].size()) img.insert({a, F.bir[k]});
                    if (b >= 0 && b < (int32_t)F.sizes[1].size()) img.insert({F.bil[k], b});
                }
                for (const auto& ab : img) len_shifted[d] += (int64_t)F.sizes[0][(size_t)ab.first] * F.sizes[1][(size_t)ab.second];
            }
            printf("  * Correlation matrix: %lld x %lld pairs, Gram of %lld vectors x %lld (Sz), %lld x %lld (Sp), %lld x %lld (Sm), tCorrMatrix %.6f s\n", LLD(N), LLD(N), LLD(N + 1), LLD(ctx.psi->n),
                   LLD(N), LLD(len_shifted[0]), LLD(N), LLD(len_shifted[1]), t1 - t0);
        }
        if (ctx.mpi_rank) return 0;
        ierr = file.Begin(ctx.data_dir + "SpinCorrelations.json"); CHKERRQ(ierr);
        fprintf(file.fp, "  {\"GlobIdx\": %lld, \"LoopType\": \"%s\", \"tCorrMatrix\": %.9g, \"Norm\": %.15g,\n   \"Sz\": ", LLD(ctx.GlobIdx), ctx.loop_type, t1 - t0, norm);
        file.Row(Sz);
        fprintf(file.fp, ",\n");
        file.Table("SzSz", SzSz, N, N, ",\n"); file.Table("SmSp", SmSp, N, N, ",\n"); file.Table("SpSm", SpSm, N, N, ",\n"); file.Table("SS", SS, N, N, ",\n"); file.Table("StructureFactor", Sq, Lx, Ly, "}");
        fflush(file.fp);
        return 0;
    }
};

/** -corr_dimer 1 (engine extension): the dimer-dimer table < D_b D_b' > over all pairs of nearest-neighbour bonds, D_b = S_i . S_j
    = Sz_i Sz_j + (Sp_i Sm_j + Sm_i Sp_j) / 2, its connected part and the dimer structure factors of the x and the y bonds, at every
    measurement point.  < psi | D_b^T D_b' | psi > = < D_b psi , D_b' psi >: the whole table is ONE dmrgx_kron_term_gram call over the
    bond images D_b psi -- vector 0 is psi itself (norm and < D_b >), vector 1 + b the image of bond b -- instead of a plan, a MatMult
    and a dot product per pair of bonds.  The bond operators and the term list of every bond are DimerFrame's (Measurements.hpp),
    which -dsf_dimer shares.  Site s of the right block is lattice site N - 1 - s.
    DD[b][b'] is < psi | D_b^T D_b' | psi >: it equals < D_b D_b' > when nothing was truncated or the two bonds sit in different
    blocks -- truncated operators of one block do not commute, the caveat of the SpSm table.  On several ranks every rank
    computes the same table from the replicated psi (no collective); rank 0 writes one record per measurement to
    DimerCorrelations.json. */
struct DimerCorrelations {
    PetscBool use = PETSC_FALSE;                /* -corr_dimer 1 */
    JsonRecordFile file{"%.15g"};               /* created at the first measurement, rank 0 only */
    PetscErrorCode ReadOptions() { return PetscOptionsGetBool(NULL, NULL, "-corr_dimer", &use, NULL); }

    template<class Hamiltonian> PetscErrorCode Run(const MeasurementContext& ctx, const Hamiltonian& Ham)
    {
        PetscLogDouble t0, t1;
        PetscTime(&t0);
        DimerFrame B;
        PetscErrorCode ierr = B.Init(ctx.KronBlocks, ctx.num_sites, Ham, ctx.psi, "Dimer correlations"); CHKERRQ(ierr);
        const std::vector<DimerBond>& bonds = B.bonds;
        const PetscInt nb = B.nb, nv = nb + 1;
        const int64_t bond_doubles = B.bond_doubles;
        /* ---- the vectors: psi, then the image of every bond */
        std::vector<double> G;
        ierr = B.Gram(G); CHKERRQ(ierr);
        const double norm = G[0];
        std::vector<double> D((size_t)nb, 0.0), DD((size_t)(nb * nb), 0.0), Conn((size_t)(nb * nb), 0.0);
        for (PetscInt b = 0; b < nb; ++b) {
            D[(size_t)b] = G[(size_t)(1 + b)];
            for (PetscInt c = 0; c < nb; ++c) DD[(size_t)(b * nb + c)] = G[(size_t)((1 + b) * nv + 1 + c)];
        }
        for (PetscInt b = 0; b < nb; ++b) for (PetscInt c = 0; c < nb; ++c) Conn[(size_t)(b * nb + c)] = DD[(size_t)(b * nb + c)] / norm - D[(size_t)b] * D[(size_t)c] / (norm * norm);
        /* S_a(q) = (1/N_a) sum over the bonds b, b' of orientation a of cos(q . (r_b - r_b')) Connected[b][b'],  q = (2 pi nx / Lx, 2 pi ny / Ly) */
        const PetscInt Lx = Ham.Lx(), Ly = Ham.Ly();
        std::vector<double> Sq[2] = {std::vector<double>((size_t)(Lx * Ly), 0.0), std::vector<double>((size_t)(Lx * Ly), 0.0)};
        for (int o = 0; o < 2; ++o) {
            const OrientedBonds O = BondsOfOrientation(bonds, o == 0 ? 'x' : 'y');
            if (O.of.empty()) continue;
            std::vector<double> C;                                  /* Connected among the bonds of this orientation */
            for (PetscInt b : O.of) for (PetscInt c : O.of) C.push_back(Conn[(size_t)(b * nb + c)]);
            Sq[o] = LatticeFourier(Lx, Ly, O.x.data(), O.y.data(), C.data(), (PetscInt)O.of.size(), (double)O.of.size());
        }
        PetscTime(&t1);
        if (!ctx.mpi_rank && ctx.verbose)
            printf("  * Dimer correlations: %lld bonds, Gram of %lld vectors x %lld, %lld bytes of bond operators held, tDimer %.6f s\n", LLD(nb), LLD(nv), LLD(ctx.psi->n), LLD(bond_doubles * (int64_t)sizeof(double)), t1 - t0);
        if (ctx.mpi_rank) return 0;
        ierr = file.Begin(ctx.data_dir + "DimerCorrelations.json"); CHKERRQ(ierr);
        fprintf(file.fp, "  {\"GlobIdx\": %lld, \"LoopType\": \"%s\", \"tDimer\": %.9g, \"Norm\": %.15g,\n", LLD(ctx.GlobIdx), ctx.loop_type, t1 - t0, norm);
        file.BondHeader(bonds, D);
        file.Table("DD", DD, nb, nb, ",\n"); file.Table("Connected", Conn, nb, nb, ",\n"); file.Table("StructureFactorX", Sq[0], Lx, Ly, ",\n"); file.Table("StructureFactorY", Sq[1], Lx, Ly, "}");
        fflush(file.fp);
        return 0;
    }
};

/** -corr_chiral 1 (engine extension): the table < chi_a chi_b > of the scalar chirality chi_ijk = S_i . (S_j x S_k) over all pairs of
    triangles of the lattice's plaquettes, at every measurement point.  chi = i K with the real, antisymmetric
      K_ijk = [ Sz_i (Sp_j Sm_k - Sm_j Sp_k) + Sz_j (Sp_k Sm_i - Sm_k Sp_i) + Sz_k (Sp_i Sm_j - Sm_i Sp_j) ] / 2,
    so for the real psi < chi_a chi_b > = < K_a psi , K_b psi >: ONE dmrgx_kron_term_gram call over psi (vector 0: the norm and
    K[a] = < psi , K_a psi >, zero in an exact basis and reported as the truncation diagnostic it is) and the images K_a psi.  The
    triangles, their strings, the split at the cut and the composed operators are ChiralFrame's (Measurements.hpp).
    CC[a][b] is < K_a psi , K_b psi >: it equals < chi_a chi_b > when nothing was truncated -- truncated operators of one block do
    not commute, the caveat of the SpSm table.  PlaquetteCC[p][p'] sums CC over the four triangles of p and of p';
    StructureFactor(q) = (1 / N_p) sum_pp' cos(q . (r_p - r_p')) PlaquetteCC[p][p'] / Norm over the plaquette positions.  One rank. */
struct ChiralCorrelations {
    PetscBool use = PETSC_FALSE;                /* -corr_chiral 1 */
    JsonRecordFile file{"%.17g"};               /* created at the first measurement */
    PetscErrorCode ReadOptions(MPI_Comm comm, PetscMPIInt size)
    {
        PetscErrorCode ierr = PetscOptionsGetBool(NULL, NULL, "-corr_chiral", &use, NULL); CHKERRQ(ierr);
        if (use && size > 1) SETERRQ1(comm, PETSC_ERR_SUP, "-corr_chiral 1 is not available on more than one rank (got %d): the triangles are not dealt over the ranks.", (int)size);
        return 0;
    }

    template<class Hamiltonian> PetscErrorCode Run(const MeasurementContext& ctx, const Hamiltonian& Ham)
    {
        PetscLogDouble t0, t1;
        PetscTime(&t0);
        ChiralFrame B;
        PetscErrorCode ierr = B.Init(ctx.KronBlocks, ctx.num_sites, Ham, ctx.psi, "Chiral correlations"); CHKERRQ(ierr);
        const PetscInt nt = B.nt, nv = nt + 1, np = (PetscInt)B.plaquettes.size();
        std::vector<double> G;
        ierr = B.Gram(G); CHKERRQ(ierr);
        const double norm = G[0];
        std::vector<double> K((size_t)nt, 0.0), CC((size_t)(nt * nt), 0.0), PCC((size_t)(np * np), 0.0);
        for (PetscInt a = 0; a < nt; ++a) {
            K[(size_t)a] = G[(size_t)(1 + a)];
            for (PetscInt b = 0; b < nt; ++b) CC[(size_t)(a * nt + b)] = G[(size_t)((1 + a) * nv + 1 + b)];
        }
        for (PetscInt a = 0; a < nt; ++a) for (PetscInt b = 0; b < nt; ++b) PCC[(size_t)(B.triangles[(size_t)a].plaq * np + B.triangles[(size_t)b].plaq)] += CC[(size_t)(a * nt + b)];
        const PetscInt Lx = Ham.Lx(), Ly = Ham.Ly();
        std::vector<PetscInt> px, py;
        for (const ChiralPlaquette& p : B.plaquettes) { px.push_back(p.x); py.push_back(p.y); }
        std::vector<double> Sq((size_t)(Lx * Ly), 0.0);
        if (np > 0) Sq = LatticeFourier(Lx, Ly, px.data(), py.data(), PCC.data(), np, norm * (double)np);
        PetscTime(&t1);
        if (!ctx.mpi_rank && ctx.verbose)
            printf("  * Chiral correlations: %lld triangles, Gram of %lld vectors x %lld, %lld bytes of composed operators held, tChiral %.6f s\n", LLD(nt), LLD(nv), LLD(ctx.psi->n), LLD(B.composed_doubles * (int64_t)sizeof(double)), t1 - t0);
        if (ctx.mpi_rank) return 0;
        ierr = file.Begin(ctx.data_dir + "ChiralCorrelations.json"); CHKERRQ(ierr);
        FILE* fp = file.fp;
        fprintf(fp, "  {\"GlobIdx\": %lld, \"LoopType\": \"%s\", \"tChiral\": %.9g, \"Norm\": %.17g,\n", LLD(ctx.GlobIdx), ctx.loop_type, t1 - t0, norm);
        fprintf(fp, "   \"Triangles\": [");
        for (PetscInt a = 0; a < nt; ++a) fprintf(fp, "%s[%lld, %lld, %lld]", a ? ", " : "", LLD(B.triangles[(size_t)a].i), LLD(B.triangles[(size_t)a].j), LLD(B.triangles[(size_t)a].k));
        fprintf(fp, "],\n   \"Kind\": [");
        for (PetscInt a = 0; a < nt; ++a) fprintf(fp, "%s%d", a ? ", " : "", B.triangles[(size_t)a].kind);
        fprintf(fp, "],\n   \"Position\": [");
        for (PetscInt a = 0; a < nt; ++a) fprintf(fp, "%s[%lld, %lld]", a ? ", " : "", LLD(B.triangles[(size_t)a].x), LLD(B.triangles[(size_t)a].y));
        fprintf(fp, "],\n   \"Side\": [");
        for (PetscInt a = 0; a < nt; ++a) fprintf(fp, "%s%d", a ? ", " : "", B.side_of[(size_t)a]);
        fprintf(fp, "],\n   \"Plaquettes\": [");
        for (PetscInt p = 0; p < np; ++p) fprintf(fp, "%s[%lld, %lld, %lld, %lld]", p ? ", " : "", LLD(B.plaquettes[(size_t)p].s[0]), LLD(B.plaquettes[(size_t)p].s[1]), LLD(B.plaquettes[(size_t)p].s[2]), LLD(B.plaquettes[(size_t)p].s[3]));
        fprintf(fp, "],\n   \"PlaquettePosition\": [");
        for (PetscInt p = 0; p < np; ++p) fprintf(fp, "%s[%lld, %lld]", p ? ", " : "", LLD(B.plaquettes[(size_t)p].x), LLD(B.plaquettes[(size_t)p].y));
        fprintf(fp, "],\n   \"K\": ");
        file.Row(K); fprintf(fp, ",\n");
        file.Table("CC", CC, nt, nt, ",\n"); file.Table("PlaquetteCC", PCC, np, np, ",\n"); file.Table("StructureFactor", Sq, Lx, Ly, "}");
        fflush(fp);
        return 0;
    }
};

/** -dsf 1 (engine extension): the dynamical spin structure factor S^zz(q, w) of the ground state at every measurement point, by the
    Lanczos-vector (continued-fraction) method.  With O_q = N^(-1/2) sum_r e^(-i q.r) Sz_r = C_q - i S_q (cosine and sine part) and a
    real psi,  S^zz(q, w) = sum_n ( |<n|C_q|0>|^2 + |<n|S_q|0>|^2 ) delta(w - E_n + E_0):  two real runs per q.  A run forms
    v = C_q psi with ONE dmrgx_kron_term_apply over Sz of every site of both blocks, then dmrgx_kron_lanczos_coeffs gives |v|^2 and
    the tridiagonal T of H from v without a host round trip per step; T is diagonalised here (TridiagQL.hpp): poles w = theta - E0,
    weights |v|^2 z_k^2 / <psi|psi>.  It runs right after the eigensolve, while the plan of the superblock Hamiltonian still exists.
    The block bases were optimised for the ground state alone (single target): |v|^2 -- the static S^zz(q) -- and the first moments
    are exact in the superblock basis, the line shape is as good as that basis represents the excited states.
    cos and sin are taken of the exact fraction 2 pi p / (Lx Ly) with their exact zeros, so that a part that vanishes by symmetry
    vanishes in the coefficients too; a part whose |v|^2 <= 1e-20 <psi|psi> (rounding of Sz_tot psi at q = 0, for instance) holds no
    weight a double could resolve next to the others and is recorded without a run: StepsDone 0.
    Set-up (operators, site maps, psi): SzFrame, Measurements.hpp.  One rank only (refused at start-up otherwise). */
struct DynamicalStructureFactor {
    PetscBool use = PETSC_FALSE;                /* -dsf 1 */
    std::vector<PetscInt> q;                    /* -dsf_q: nx0, ny0, nx1, ny1, ... */
    static constexpr double no_weight = 1e-20;  /* a part with |v|^2 <= no_weight <psi|psi> (rounding noise, as Sz_tot psi at q = 0) is recorded with StepsDone 0, without a run */
    JsonRecordFile file{"%.17g"};               /* created at the first measurement */
    PetscErrorCode ReadOptions(MPI_Comm comm, PetscMPIInt size, LanczosStepOptions& lanczos)
    {
        PetscErrorCode ierr = PetscOptionsGetBool(NULL, NULL, "-dsf", &use, NULL); CHKERRQ(ierr);
        if (!use) return 0;
        if (size > 1) SETERRQ1(comm, PETSC_ERR_SUP, "-dsf 1 is not available on more than one rank (got %d): the Lanczos run behind S(q,w) has no collectives.", (int)size);
        PetscBool have_q = PETSC_FALSE;
        PetscInt nq = 2048;
        q.assign((size_t)nq, 0);
        ierr = PetscOptionsGetIntArray(NULL, NULL, "-dsf_q", q.data(), &nq, &have_q); CHKERRQ(ierr);
        q.resize((size_t)nq);
        if (!have_q || nq < 2 || nq % 2) SETERRQ1(comm, PETSC_ERR_ARG_WRONG, "-dsf 1 needs -dsf_q nx0,ny0,nx1,ny1,...: pairs of integers, q = (2 pi nx / Lx, 2 pi ny / Ly). Got %lld numbers.", LLD(nq));
        return lanczos.ReadOnce(comm);
    }

    template<class Hamiltonian> PetscErrorCode Run(const MeasurementContext& ctx, const Hamiltonian& Ham, const LanczosStepOptions& lanczos)
    {
        PetscLogDouble t0, t1;
        PetscTime(&t0);
        SzFrame S;
        PetscErrorCode ierr = S.Init(ctx.KronBlocks, ctx.num_sites, Ham, ctx.psi, "Dynamical structure factor"); CHKERRQ(ierr);
        const PetscInt N = S.F.N, Lx = S.Lx, Ly = S.Ly, M = S.M, steps = lanczos.steps;
        const int64_t n = S.n;
        std::vector<dmrgx_term> terms;
        terms.reserve((size_t)N);
        DevBuffer v((size_t)n, DevBuffer::device_only_t{});

        struct Part { double norm2 = 0.0; int32_t done = 0; std::vector<double> alpha, beta, theta, z; };
        struct Point { PetscInt nx, ny; Part part[2]; std::vector<double> poles, weights; double total = 0.0; };
        std::vector<Point> points(q.size() / 2);
        PetscInt matmults = 0;
        for (size_t iq = 0; iq < points.size(); ++iq) {
            Point& P = points[iq];
            P.nx = q[2 * iq]; P.ny = q[2 * iq + 1];
            for (int part = 0; part < 2; ++part) {
                Part& A = P.part[part];
                terms.clear();
                for (PetscInt i = 0; i < N; ++i) {
                    const PetscInt s = S.site[(size_t)i];                /* operator i of the frame is Sz of lattice site s */
                    const PetscInt p = (((P.nx * S.rx[(size_t)s] * Ly + P.ny * S.ry[(size_t)s] * Lx) % M) + M) % M;      /* q . r = 2 pi p / M exactly */
                    const double c = DsfPhaseCoefficient(part, p, M);
                    /* a site whose coefficient is exactly zero takes no part: its Sz cells are neither copied nor multiplied */
                    if (c == 0.0) continue;
                    terms.push_back(S.term(i, c / std::sqrt((double)N)));
                }
                if (terms.empty()) continue;                            /* the part vanishes on the lattice: Norm2 0, no run */
                const int32_t vec_first[2] = {0, (int32_t)terms.size()};
                ierr = S.Apply(1, vec_first, terms.data(), v.dev_uninitialised(), n); CHKERRQ(ierr);
                if (dmrgx_dot(n, v.dev_ro(), v.dev_ro(), &A.norm2, nullptr)) SETERRQ1(ctx.mpi_comm, 1, "dmrgx_dot: %s", dmrgx_last_error());
                if (A.norm2 != A.norm2) SETERRQ3(ctx.mpi_comm, 1, "Dynamical structure factor: the %s part of q = (%lld,%lld) is not a number.", part == 0 ? "cosine" : "sine", LLD(P.nx), LLD(P.ny));
                if (!(A.norm2 > no_weight * S.norm)) continue;        /* no weight: no run */
                A.alpha.assign((size_t)steps, 0.0); A.beta.assign((size_t)steps, 0.0);
                if (dmrgx_kron_lanczos_coeffs(ctx.plan(), v.dev_ro(), (int32_t)steps, lanczos.breakdown_tol, &A.norm2, A.alpha.data(), A.beta.data(), &A.done, nullptr))
                    SETERRQ1(ctx.mpi_comm, 1, "dmrgx_kron_lanczos_coeffs: %s", dmrgx_last_error());
                matmults += steps;
                A.alpha.resize((size_t)A.done); A.beta.resize((size_t)A.done);
                A.theta = A.alpha;
                if (!TridiagQLFirstRow(A.theta, A.beta, A.z)) SETERRQ2(ctx.mpi_comm, 1, "Dynamical structure factor: the QL iteration on the Lanczos matrix of q = (%lld,%lld) did not converge.", LLD(P.nx), LLD(P.ny));
            }
            /* the poles of both parts, ascending */
            std::vector<std::pair<double, double>> pw;
            for (const Part& A : P.part) for (size_t k = 0; k < A.theta.size(); ++k) pw.push_back({A.theta[k] - ctx.E0, A.norm2 * A.z[k] * A.z[k] / S.norm});
            std::sort(pw.begin(), pw.end());
            for (const auto& x : pw) { P.poles.push_back(x.first); P.weights.push_back(x.second); P.total += x.second; }
        }
        PetscTime(&t1);
        if (ctx.verbose) printf("  * Dynamical structure factor: %lld q points, %lld Lanczos steps per run, %lld MatMults on %lld states, tDsf %.6f s\n", LLD(points.size()), LLD(steps), LLD(matmults), LLD(n), t1 - t0);
        ierr = file.BeginDynamical(ctx.data_dir + "DynamicalStructureFactor.json", ctx.GlobIdx, ctx.loop_type, (double)ctx.E0, S.norm); CHKERRQ(ierr);
        FILE* fp_dsf = file.fp;
        fprintf(fp_dsf, ", \"Steps\": %lld, \"tDsf\": %.9g, \"MatMults\": %lld,\n   \"Points\": [\n", LLD(steps), t1 - t0, LLD(matmults));
        for (size_t iq = 0; iq < points.size(); ++iq) {
            const Point& P = points[iq];
            fprintf(fp_dsf, "     {\"q\": [%lld, %lld],\n", LLD(P.nx), LLD(P.ny));
            for (int part = 0; part < 2; ++part) {
                const Part& A = P.part[part];
                fprintf(fp_dsf, "      \"%s\": {\"Norm2\": %.17g, \"StepsDone\": %d, \"Alpha\": ", part == 0 ? "Cos" : "Sin", A.norm2, (int)A.done);
                file.Row(A.alpha); fprintf(fp_dsf, ", \"Beta\": "); file.Row(A.beta); fprintf(fp_dsf, "},\n");
            }
            fprintf(fp_dsf, "      \"Poles\": "); file.Row(P.poles); fprintf(fp_dsf, ",\n      \"Weights\": "); file.Row(P.weights);
            fprintf(fp_dsf, ",\n      \"StaticSzz\": %.17g}%s\n", P.total, iq + 1 < points.size() ? "," : "");
        }
        fprintf(fp_dsf, "   ]}");
        fflush(fp_dsf);
        return 0;
    }
};

/** -dsf_sites c0,c1,... (engine extension): the real-space dynamical correlations of the ground state from every listed site c,
        G_ic(w) = sum_n <0|Sz_i|n> <n|Sz_c|0> delta(w - E_n + E_0)   for ALL sites i,
    from ONE Lanczos run per c, where -dsf needs two runs per wave vector.  dmrgx_kron_lanczos_basis runs the recursion from
    v = Sz_c psi with the basis V kept and fully reorthogonalised, so that T = V H V^T and V V^T = 1 hold to rounding; the overlaps
    M[i][k] = <u_i, q_k> with the images u_i = Sz_i psi (SzFrame::Images, a chunk at a time) are one dmrgx_vec_gram(chunk, V) each.
    With T = S Theta S^T (TridiagQL.hpp, all eigenvectors) the Galerkin approximation of G in the Krylov space of v is
        Poles[n] = theta_n - E0,   Amplitudes[i][n] = (M S)[i][n] |v| S[0][n] / <psi|psi>,
    and Sqw[q][n] = sum_i cos(q . (r_i - r_c)) Amplitudes[i][n] (SiteCosineSum) at all Lx Ly wave vectors q = (2 pi nx / Lx,
    2 pi ny / Ly), row nx Ly + ny: (1/N) sum_c Sqw is S^zz(q, w).  Static[i] = sum_n Amplitudes[i][n] = <Sz_i Sz_c> exactly (S is
    orthogonal), and the moments sum_n Amplitudes[i][n] Poles[n]^p equal <u_i, (H - E0)^p v> for p < steps done.
    The psi component of v is left in: it shows as a pole at w = 0 whose amplitude at i is <Sz_i> <Sz_c>.  Amplitudes[c] are the
    weights |v|^2 S[0][n]^2 >= 0 of the continued fraction of v; for i != c they carry either sign, and Sqw of ONE site is an
    estimator that need not be positive where the lattice is not translation invariant (an open cylinder) -- only the average over c
    is S^zz(q, w).  The block bases were optimised for the ground state alone: the caveat of -dsf applies unchanged.
    Memory: the basis, steps x N_sb doubles on the device for the whole measurement (2.6 GB at 20 x 8, m = 2048, 100 steps), beside
    one chunk of images.  One rank only (refused at start-up otherwise). */
struct DynamicalCorrelations {
    PetscBool use = PETSC_FALSE;                /* -dsf_sites c0,c1,... */
    std::vector<PetscInt> sites;                /* the reference sites c, lattice numbering of To1D; shares -dsf_steps and -dsf_breakdown_tol */
    JsonRecordFile file{"%.17g"};               /* created at the first measurement */
    PetscErrorCode ReadOptions(MPI_Comm comm, PetscMPIInt size, PetscInt num_sites, LanczosStepOptions& lanczos)
    {
        PetscErrorCode ierr = ReadSiteListOption(comm, size, "-dsf_sites", "the Lanczos run behind G_ic(w)", sites, use, num_sites); CHKERRQ(ierr);
        return use ? lanczos.ReadOnce(comm) : 0;
    }

    template<class Hamiltonian> PetscErrorCode Run(const MeasurementContext& ctx, const Hamiltonian& Ham, const LanczosStepOptions& lanczos)
    {
        PetscLogDouble t0, t1;
        PetscTime(&t0);
        SzFrame S;
        PetscErrorCode ierr = S.Init(ctx.KronBlocks, ctx.num_sites, Ham, ctx.psi, "Dynamical correlations"); CHKERRQ(ierr);
        const PetscInt N = S.F.N, M = S.M, K = lanczos.steps, chunk = S.chunk();
        const int64_t n = S.n, ld = S.ld;
        std::vector<PetscInt> ops((size_t)N);                        /* the images are taken in the order of the operators */
        for (PetscInt a = 0; a < N; ++a) ops[(size_t)a] = a;
        std::unique_ptr<DevBuffer> v, V, U, Mdev;
        try {
            v.reset(new DevBuffer((size_t)n, DevBuffer::device_only_t{}));
            V.reset(new DevBuffer((size_t)(K * ld), DevBuffer::device_only_t{}));
            U.reset(new DevBuffer((size_t)(chunk * ld), DevBuffer::device_only_t{}));
            Mdev.reset(new DevBuffer((size_t)(chunk * K), DevBuffer::device_only_t{}));
        } catch (const std::exception& e) { SETERRQ3(ctx.mpi_comm, PETSC_ERR_MEM, "Dynamical correlations: no memory for the basis of %lld steps x %lld states: %s", LLD(K), LLD(n), e.what()); }

        struct Run_t { PetscInt c = 0; double norm2 = 0.0; int32_t done = 0; std::vector<double> alpha, beta, poles, amp, stat, sqw; };
        std::vector<Run_t> runs(sites.size());
        std::vector<double> Mh((size_t)(N * K)), Mchunk((size_t)(chunk * K)), theta, vec;
        PetscInt matmults = 0;
        double t_runs = 0.0;
        for (size_t ir = 0; ir < runs.size(); ++ir) {
            Run_t& R = runs[ir];
            R.c = sites[ir];
            /* v = Sz_c psi, then the run from it */
            ierr = S.Images(&S.op_of[(size_t)R.c], 1, v->dev_uninitialised(), n); CHKERRQ(ierr);
            R.alpha.assign((size_t)K, 0.0); R.beta.assign((size_t)K, 0.0);
            PetscLogDouble tr0 = 0.0, tr1 = 0.0;
            if (ctx.verbose) { if (dmrgx_stream_sync(nullptr)) SETERRQ1(ctx.mpi_comm, 1, "%s", dmrgx_last_error()); PetscTime(&tr0); }      /* the run alone, for the log */
            if (dmrgx_kron_lanczos_basis(ctx.plan(), v->dev_ro(), (int32_t)K, lanczos.breakdown_tol, V->dev_uninitialised(), ld, &R.norm2, R.alpha.data(), R.beta.data(), &R.done, nullptr))
                SETERRQ1(ctx.mpi_comm, 1, "dmrgx_kron_lanczos_basis: %s", dmrgx_last_error());
            if (ctx.verbose) { PetscTime(&tr1); t_runs += tr1 - tr0; }
            matmults += K;
            /* M[s][k] = < Sz_s psi , q_k > for every lattice site s */
            for (PetscInt a0 = 0; a0 < N; a0 += chunk) {
                const PetscInt cnt = std::min<PetscInt>(chunk, N - a0);
                ierr = S.Images(ops.data() + a0, cnt, U->dev_uninitialised(), ld); CHKERRQ(ierr);
                if (dmrgx_vec_gram((int32_t)cnt, (int32_t)K, n, U->dev_ro(), ld, V->dev_ro(), ld, Mdev->dev_uninitialised(), K, 0, nullptr, nullptr)) SETERRQ1(ctx.mpi_comm, 1, "dmrgx_vec_gram: %s", dmrgx_last_error());
                if (dmrgx_memcpy_d2h(Mchunk.data(), Mdev->dev_ro(), (size_t)(cnt * K) * sizeof(double), nullptr)) SETERRQ1(ctx.mpi_comm, 1, "%s", dmrgx_last_error());
                for (PetscInt a = a0; a < a0 + cnt; ++a) std::copy(Mchunk.begin() + (a - a0) * K, Mchunk.begin() + (a - a0 + 1) * K, Mh.begin() + S.site[(size_t)a] * K);
            }
            /* T = S Theta S^T on the host, the poles ascending */
            const PetscInt D = R.done;
            R.alpha.resize((size_t)D); R.beta.resize((size_t)D);
            theta = R.alpha;
            if (!TridiagQLVectors(theta, R.beta, vec)) SETERRQ1(ctx.mpi_comm, 1, "Dynamical correlations: the QL iteration on the Lanczos matrix of site %lld did not converge.", LLD(R.c));
            std::vector<PetscInt> order((size_t)D);
            for (PetscInt k = 0; k < D; ++k) order[(size_t)k] = k;
            std::sort(order.begin(), order.end(), [&](PetscInt a, PetscInt b) { return theta[(size_t)a] < theta[(size_t)b]; });
            const double vnorm = std::sqrt(R.norm2);
            R.poles.resize((size_t)D); R.amp.assign((size_t)(N * D), 0.0); R.stat.assign((size_t)N, 0.0);
            for (PetscInt p = 0; p < D; ++p) {
                const double* z = vec.data() + order[(size_t)p] * D;            /* eigenvector of pole p: z[k] = S[k][n] */
                R.poles[(size_t)p] = theta[(size_t)order[(size_t)p]] - (double)ctx.E0;
                for (PetscInt s = 0; s < N; ++s) {
                    double acc = 0.0;
                    for (PetscInt k = 0; k < D; ++k) acc += Mh[(size_t)(s * K + k)] * z[k];
                    R.amp[(size_t)(s * D + p)] = acc * vnorm * z[0] / S.norm;
                }
            }
            for (PetscInt s = 0; s < N; ++s) for (PetscInt p = 0; p < D; ++p) R.stat[(size_t)s] += R.amp[(size_t)(s * D + p)];
            R.sqw = SiteCosineSum(S.Lx, S.Ly, S.rx.data(), S.ry.data(), R.c, R.amp.data(), N, D);
        }
        PetscTime(&t1);
        if (ctx.verbose) printf("  * Dynamical correlations: %lld reference sites, %lld Lanczos steps per run with the basis kept, %lld MatMults on %lld states, images in chunks of %lld, tDsfSites %.6f s, of it the Lanczos runs %.6f s\n", LLD(runs.size()), LLD(K), LLD(matmults), LLD(n), LLD(chunk), t1 - t0, t_runs);
        ierr = file.BeginDynamical(ctx.data_dir + "DynamicalCorrelations.json", ctx.GlobIdx, ctx.loop_type, (double)ctx.E0, S.norm); CHKERRQ(ierr);
        FILE* fp = file.fp;
        fprintf(fp, ", \"Steps\": %lld, \"tDsfSites\": %.9g, \"MatMults\": %lld,\n   \"Sites\": [\n", LLD(K), t1 - t0, LLD(matmults));
        for (size_t ir = 0; ir < runs.size(); ++ir) {
            const Run_t& R = runs[ir];
            const PetscInt D = R.done;
            file.OpenSite(R.c, S.rx[(size_t)R.c], S.ry[(size_t)R.c], R.norm2);
            fprintf(fp, ", \"StepsDone\": %d,\n   \"Alpha\": ", (int)R.done);
            file.Row(R.alpha); fprintf(fp, ",\n   \"Beta\": "); file.Row(R.beta); fprintf(fp, ",\n   \"Poles\": "); file.Row(R.poles);
            fprintf(fp, ",\n   \"Static\": "); file.Row(R.stat); fprintf(fp, ",\n");
            file.Table("Amplitudes", R.amp, N, D, ",\n"); file.Table("Sqw", R.sqw, M, D, ir + 1 < runs.size() ? "},\n" : "}\n");
        }
        fprintf(fp, "   ]}");
        fflush(fp);
        return 0;
    }
};

/** -dsf_cheb c0,c1,... (engine extension): the Chebyshev moments of the real-space dynamical correlations of the ground state,
        mu_n^{ic} = < Sz_i psi , T_n(Ht) Sz_c psi > / <psi|psi>,   Ht = (H - Centre) / HalfWidth,   for ALL sites i,
    from one dmrgx_kron_chebyshev_moments run per reference site c: the three-term recursion t_{n+1} = 2 Ht t_n - t_{n-1} needs two
    earlier vectors, no kept basis and no reorthogonalisation, so its cost is linear in the number of moments where -dsf_sites
    grows with the square.  The images u_i = Sz_i psi of all N sites (SzFrame::Images, lattice order) stay on the device for
    the whole measurement -- N x N_sb doubles, refused with PETSC_ERR_MEM if they do not fit --; row c is the start vector of run
    c, and the library takes <u_i, t_n> of all i with one Gram call per 16 vectors.
    The window must contain the spectrum of the superblock Hamiltonian.  Unless -dsf_cheb_window lo,hi gives it, it is found once
    per measurement: -dsf_cheb_bound_steps Lanczos steps (dmrgx_kron_lanczos_coeffs) from a fixed pseudo-random vector give the top
    Ritz value and its residual bound, E0 is the bottom (ChebyshevWindow, Measurements.hpp).  Should the window fail to hold, the
    library's guard ends the run: StepsDone < Steps in the record and a warning here, not an error.
    Moments (N x (D + 1), lattice numbering), their lattice Fourier transform MomentsQ[q][n] = sum_i cos(q . (r_i - r_c))
    Moments[i][n] (row nx Ly + ny) and Diag[m] = mu_m^{cc}, m <= 2D (the doubling identities), D = StepsDone.  With -dsf_cheb_omega
    w0,w1,nw also SqwGrid[q][k] = ChebyshevJackson(MomentsQ[q], D + 1, x_k) / HalfWidth at x_k = (w_k + E0 - Centre) / HalfWidth:
    (1/N) sum_c SqwGrid is the Jackson-broadened S^zz(q, w), non-negative and free of ghosts; its resolution is about
    pi HalfWidth / (D + 1).  The caveats of -dsf_sites (one site is an estimator; bases optimised for the ground state) apply.
    One rank only (refused at start-up otherwise). */
struct ChebyshevCorrelations {
    PetscBool use = PETSC_FALSE;                /* -dsf_cheb c0,c1,... */
    std::vector<PetscInt> sites;                /* the reference sites c, lattice numbering of To1D */
    JsonRecordFile file{"%.17g"};               /* created at the first measurement */
    PetscErrorCode ReadOptions(MPI_Comm comm, PetscMPIInt size, PetscInt num_sites) { return ReadSiteListOption(comm, size, "-dsf_cheb", "the Chebyshev recursion", sites, use, num_sites); }

    template<class Hamiltonian> PetscErrorCode Run(const MeasurementContext& ctx, const Hamiltonian& Ham, const ChebyshevOptions& cheb)
    {
        PetscLogDouble t0, t1;
        PetscTime(&t0);
        SzFrame S;
        PetscErrorCode ierr = S.Init(ctx.KronBlocks, ctx.num_sites, Ham, ctx.psi, "Chebyshev correlations"); CHKERRQ(ierr);
        const PetscInt N = S.F.N, M = S.M, K = cheb.steps;
        const int64_t n = S.n, ld = S.ld;
        const std::vector<double>* omega = cheb.grid();
        /* the images of all sites, row s = Sz_s psi */
        std::unique_ptr<DevBuffer> U;
        ierr = S.AllImages(U, n); CHKERRQ(ierr);

        /* the window */
        const double e0 = (double)ctx.E0;
        ChebyshevSpectralWindow W;
        ierr = cheb.FindWindow(ctx.mpi_comm, ctx.plan(), n, &e0, "Chebyshev correlations", W); CHKERRQ(ierr);
        PetscInt matmults = W.bound_steps;

        std::vector<MomentRun> runs(sites.size());
        std::vector<double> cross;
        double t_runs = 0.0;
        for (size_t ir = 0; ir < runs.size(); ++ir) {
            MomentRun& R = runs[ir];
            R.c = sites[ir];
            ierr = ChebyshevMomentRun(ctx.plan(), U->dev_ro(), ld, N, W, K, S.norm, cross, R, ctx.verbose ? &t_runs : nullptr); CHKERRQ(ierr);
            matmults += K;
            WarnLeftWindow("-dsf_cheb", nullptr, "site", R, W, K);
            R.momq = SiteCosineSum(S.Lx, S.Ly, S.rx.data(), S.ry.data(), R.c, R.mom.data(), N, R.done + 1);
            if (omega) R.grid = ChebyshevGrid(R.momq, R.done + 1, *omega, e0, W.centre, W.half_width);
        }
        PetscTime(&t1);
        if (ctx.verbose) printf("  * Chebyshev correlations: %lld reference sites, %lld steps per run, window [%.6f, %.6f] from %lld Lanczos steps, %lld MatMults on %lld states, tDsfCheb %.6f s, of it the Chebyshev runs %.6f s\n",
                                LLD(runs.size()), LLD(K), W.centre - W.half_width, W.centre + W.half_width, LLD(W.bound_steps), LLD(matmults), LLD(n), t1 - t0, t_runs);
        ierr = file.BeginDynamical(ctx.data_dir + "ChebyshevMoments.json", ctx.GlobIdx, ctx.loop_type, e0, S.norm); CHKERRQ(ierr);
        FILE* fp = file.fp;
        fprintf(fp, ", \"Steps\": %lld, \"Centre\": %.17g, \"HalfWidth\": %.17g, \"BoundSteps\": %lld, \"ThetaMax\": %.17g, \"Residual\": %.17g, \"tDsfCheb\": %.9g, \"MatMults\": %lld,\n",
                LLD(K), W.centre, W.half_width, LLD(W.bound_steps), W.theta_max, W.residual, t1 - t0, LLD(matmults));
        file.Omega(omega);
        fprintf(fp, "   \"Sites\": [\n");
        for (size_t ir = 0; ir < runs.size(); ++ir) {
            const MomentRun& R = runs[ir];
            file.OpenSite(R.c, S.rx[(size_t)R.c], S.ry[(size_t)R.c], R.norm2);
            fprintf(fp, ", \"StepsDone\": %d", (int)R.done);
            file.Moments(R, N, M, omega, ir + 1 < runs.size() ? "},\n" : "}\n");
        }
        fprintf(fp, "   ]}");
        fflush(fp);
        return 0;
    }
};

/** -dsf_dimer b0,b1,... (engine extension): the Chebyshev moments of the dynamical dimer correlations of the ground state,
        mu_n^{bc} = < dD_b psi , T_n(Ht) dD_c psi > / <psi|psi>,   dD_b = D_b - <D_b>,   D_b = S_i . S_j,   Ht = (H - Centre) / HalfWidth,
    for ALL nearest-neighbour bonds b, from one dmrgx_kron_chebyshev_moments run per reference bond c (its index in Bonds, the order of
    DimerBonds(Ham) and of DimerCorrelations.json): the singlet channel -- valence-bond order against a spin liquid, what Raman
    scattering sees -- where -dsf_cheb measures the spin channel.  The images D_b psi of all nb bonds (DimerFrame::Images: the bond
    operators and terms of -corr_dimer) are written into one device family, and ONE dmrgx_vec_project_out call removes psi from all
    of them: <D_b> is about -0.3 where <Sz_i> vanishes, and its delta peak at w = 0, far heavier than the inelastic part, would be
    smeared by the Jackson kernel over the window where the singlet gap is.  The coefficients of that call are D[b] = <D_b> =
    <psi|D_b|psi> / <psi|psi>.  Row c of the family is the start vector of run c, the whole family its U.  The window is found as for
    -dsf_cheb (ChebyshevOptions::FindWindow: -dsf_cheb_window, or -dsf_cheb_bound_steps Lanczos steps); a run that leaves it ends with
    StepsDone < Steps and a warning.
    Per reference bond: Norm2 = <dD_c psi, dD_c psi>; Elastic = <psi, dD_c psi> / sqrt(Norm Norm2), what is left of the elastic line
    (rounding); Diag[m] = mu_m^{cc}, m <= 2 StepsDone; Moments (nb x (StepsDone + 1), Moments[:, 0] = Connected[:, c] of -corr_dimer);
    MomentsQ[q][n] = sum over the bonds b of c's orientation of cos(q . (r_b - r_c)) Moments[b][n] at their Positions (row nx Ly + ny);
    with -dsf_dimer_omega w0,w1,nw SqwGrid[q][k] = ChebyshevJackson(MomentsQ[q], StepsDone + 1, x_k) / HalfWidth at
    x_k = (w_k + E0 - Centre) / HalfWidth: averaged over the reference bonds of one orientation the Jackson-broadened dimer structure
    factor S_a(q, w), non-negative.  MatMults = BoundSteps + refs * Steps.
    Memory on the device: the nb images (nb x N_sb doubles, refused with PETSC_ERR_MEM if they do not fit) plus the 34 vectors of the
    moment run.  The block bases are ground-state bases (the caveat of -dsf_sites).  One rank only (refused at start-up otherwise). */
struct DimerDynamics {
    PetscBool use = PETSC_FALSE;                /* -dsf_dimer b0,b1,...; shares -dsf_cheb_window and -dsf_cheb_bound_steps */
    std::vector<PetscInt> bonds;                /* the reference bonds c: their index in DimerBonds(Ham), the Bonds of DimerCorrelations.json */
    PetscInt steps = 200;                       /* -dsf_dimer_steps: MatMults per run */
    PetscBool have_omega = PETSC_FALSE;
    std::vector<double> omega;                  /* -dsf_dimer_omega w0,w1,nw: the grid of the Jackson-broadened SqwGrid */
    JsonRecordFile file{"%.17g"};               /* created at the first measurement */
    PetscErrorCode ReadOptions(MPI_Comm comm, PetscMPIInt size, PetscInt num_bonds)
    {
        PetscErrorCode ierr = ReadSiteListOption(comm, size, "-dsf_dimer", "the Chebyshev recursion", bonds, use, num_bonds, "bond",
                                                 "the nearest-neighbour bonds in the order of Bonds in DimerCorrelations.json"); CHKERRQ(ierr);
        if (!use) return 0;
        ierr = PetscOptionsGetInt(NULL, NULL, "-dsf_dimer_steps", &steps, NULL); CHKERRQ(ierr);
        if (steps < 1) SETERRQ1(comm, PETSC_ERR_ARG_OUTOFRANGE, "-dsf_dimer_steps must be at least 1. Got %lld.", LLD(steps));
        return ReadOmegaGridOption(comm, "-dsf_dimer_omega", omega, have_omega);
    }

    template<class Hamiltonian> PetscErrorCode Run(const MeasurementContext& ctx, const Hamiltonian& Ham, const ChebyshevOptions& cheb)
    {
        PetscLogDouble t0, t1;
        PetscTime(&t0);
        DimerFrame B;
        PetscErrorCode ierr = B.Init(ctx.KronBlocks, ctx.num_sites, Ham, ctx.psi, "Dimer dynamics"); CHKERRQ(ierr);
        const PetscInt nb = B.nb, K = steps, Lx = Ham.Lx(), Ly = Ham.Ly(), M = Lx * Ly;
        const int64_t n = B.n, ld = n + (n & 1);
        /* the images of all bonds, row b = D_b psi, then (D_b - <D_b>) psi */
        std::unique_ptr<DevBuffer> U;
        try { U.reset(new DevBuffer((size_t)(nb * ld), DevBuffer::device_only_t{})); }
        catch (const std::exception& e) { SETERRQ4(ctx.mpi_comm, PETSC_ERR_MEM, "Dimer dynamics: no memory for the images of %lld bonds x %lld states (%.3f GB): %s", LLD(nb), LLD(n), (double)(nb * ld) * 8e-9, e.what()); }
        ierr = B.Images(U->dev_uninitialised(), ld); CHKERRQ(ierr);
        std::vector<double> D((size_t)nb, 0.0);
        double norm = 0.0;
        if (dmrgx_vec_project_out((int32_t)nb, n, U->dev_uninitialised(), ld, B.psi, D.data(), &norm, nullptr)) SETERRQ1(ctx.mpi_comm, 1, "dmrgx_vec_project_out: %s", dmrgx_last_error());
        if (!(norm > 0.0)) SETERRQ(ctx.mpi_comm, 1, "Dimer dynamics: the ground state has no norm.");

        const double e0 = (double)ctx.E0;
        const std::vector<double>* grid = have_omega ? &omega : nullptr;
        ChebyshevSpectralWindow W;
        ierr = cheb.FindWindow(ctx.mpi_comm, ctx.plan(), n, &e0, "Dimer dynamics", W); CHKERRQ(ierr);
        PetscInt matmults = W.bound_steps;

        const OrientedBonds oriented[2] = {BondsOfOrientation(B.bonds, 'x'), BondsOfOrientation(B.bonds, 'y')};
        std::vector<MomentRun> runs(bonds.size());
        std::vector<double> cross;
        double t_runs = 0.0;
        for (size_t ir = 0; ir < runs.size(); ++ir) {
            MomentRun& R = runs[ir];
            R.c = bonds[ir];
            ierr = ChebyshevMomentRun(ctx.plan(), U->dev_ro(), ld, nb, W, K, norm, cross, R, ctx.verbose ? &t_runs : nullptr); CHKERRQ(ierr);
            matmults += K;
            double overlap = 0.0;
            if (dmrgx_dot(n, B.psi, U->dev_ro() + R.c * ld, &overlap, nullptr)) SETERRQ1(ctx.mpi_comm, 1, "dmrgx_dot: %s", dmrgx_last_error());
            R.elastic = R.norm2 > 0.0 ? overlap / std::sqrt(norm * R.norm2) : 0.0;
            WarnLeftWindow("-dsf_dimer", nullptr, "bond", R, W, K);
            /* the cosine sum over the bonds of c's orientation, from c */
            const PetscInt nm = R.done + 1;
            const OrientedBonds& O = oriented[B.bonds[(size_t)R.c].orient == 'x' ? 0 : 1];
            const PetscInt no = (PetscInt)O.of.size(), c_in = (PetscInt)(std::find(O.of.begin(), O.of.end(), R.c) - O.of.begin());
            std::vector<double> sel((size_t)(no * nm));
            for (PetscInt k = 0; k < no; ++k) std::copy(R.mom.begin() + O.of[(size_t)k] * nm, R.mom.begin() + (O.of[(size_t)k] + 1) * nm, sel.begin() + k * nm);
            R.momq = SiteCosineSum(Lx, Ly, O.x.data(), O.y.data(), c_in, sel.data(), no, nm);
            if (grid) R.grid = ChebyshevGrid(R.momq, nm, *grid, e0, W.centre, W.half_width);
        }
        PetscTime(&t1);
        if (ctx.verbose) printf("  * Dimer dynamics: %lld reference bonds of %lld, %lld steps per run, window [%.6f, %.6f] from %lld Lanczos steps, %lld MatMults on %lld states, tDimerDyn %.6f s, of it the Chebyshev runs %.6f s\n",
                                LLD(runs.size()), LLD(nb), LLD(K), W.centre - W.half_width, W.centre + W.half_width, LLD(W.bound_steps), LLD(matmults), LLD(n), t1 - t0, t_runs);
        ierr = file.BeginDynamical(ctx.data_dir + "DimerDynamics.json", ctx.GlobIdx, ctx.loop_type, e0, norm); CHKERRQ(ierr);
        FILE* fp = file.fp;
        fprintf(fp, ", \"Steps\": %lld, \"Centre\": %.17g, \"HalfWidth\": %.17g, \"BoundSteps\": %lld, \"ThetaMax\": %.17g, \"Residual\": %.17g, \"tDimerDyn\": %.9g, \"MatMults\": %lld,\n",
                LLD(K), W.centre, W.half_width, LLD(W.bound_steps), W.theta_max, W.residual, t1 - t0, LLD(matmults));
        file.BondHeader(B.bonds, D);
        file.Omega(grid);
        fprintf(fp, "   \"RefBonds\": [\n");
        for (size_t ir = 0; ir < runs.size(); ++ir) {
            const MomentRun& R = runs[ir];
            const DimerBond& bc = B.bonds[(size_t)R.c];
            fprintf(fp, "   {\"Bond\": %lld, \"Sites\": [%lld, %lld], \"Orientation\": \"%c\", \"Norm2\": %.17g, \"Elastic\": %.17g, \"StepsDone\": %d",
                    LLD(R.c), LLD(bc.i), LLD(bc.j), bc.orient, R.norm2, R.elastic, (int)R.done);
            file.Moments(R, nb, M, grid, ir + 1 < runs.size() ? "},\n" : "}\n");
        }
        fprintf(fp, "   ]}");
        fflush(fp);
        return 0;
    }
};

/** -dsf_pm c0,c1,... (engine extension): the Chebyshev moments of the transverse dynamical correlations of the ground state,
        mu_n^{ic} = < O_i psi , T_n(Ht) O_c psi > / <psi|psi>,   Ht = (H' - Centre) / HalfWidth,   for ALL sites i,
    in two channels: "MinusPlus", O = S^+, the response < S^-_i delta(w - H' + E0) S^+_c >, and "PlusMinus", O = S^- (Sp read
    transposed), < S^+_i ... S^-_c > -- the magnons of an XXZ model or of a magnetised target, which S^zz (-dsf_cheb) does not hold.
    O psi lives in the total-Sz sector qn_sector + 1 (- 1), so H' is the superblock Hamiltonian of THAT sector: per channel a
    KronBlocks_t of the neighbouring sector over the same two blocks, the images of all N sites written in its layout
    (SzFrame::AllImages, dmrgx_kron_term_apply_to) -- N x N_sb' doubles, refused with PETSC_ERR_MEM if they do not fit --, its plan
    (KronSumConstruct with the settings of the ground-state plan), and one dmrgx_kron_chebyshev_moments run per reference site.  The
    measurement runs after the ground-state plan is destroyed and destroys each plan before the next: one plan is resident at a time.
    The window is -dsf_cheb_window lo,hi as given (ThetaMin = lo, ThetaMax = hi), else from -dsf_cheb_bound_steps Lanczos steps on
    H' from the fixed pseudo-random vector of ChebyshevOptions::FindWindow, both ends from the Ritz values (ChebyshevWindowTwoSided: the
    bottom of another sector is not known from E0).  Should the window fail to hold, the library's guard ends the run: StepsDone <
    Steps in the record and a warning here, not an error.  An empty neighbouring sector (a fully polarised target) gives a record
    with States 0, no MatMults and StepsDone 0 for every site.
    One record per measurement and channel in TransverseDynamics.json; Moments, MomentsQ, Diag and SqwGrid as in
    ChebyshevMoments.json, energies measured from E0 of the target sector: (1/N) sum_c SqwGrid is the Jackson-broadened S^-+(q, w)
    (S^+-(q, w)), non-negative.  The caveats of -dsf_sites apply, and one more: the bases of the blocks are optimised for the ONE
    target state, not for the states of the neighbouring sector (single-target DMRG) -- exact while nothing is truncated, an
    approximation that m controls otherwise.  One rank only (refused at start-up otherwise). */
struct TransverseDynamics {
    PetscBool use = PETSC_FALSE;                /* -dsf_pm c0,c1,...; shares the -dsf_cheb_* options */
    std::vector<PetscInt> sites;                /* the reference sites c, lattice numbering of To1D */
    JsonRecordFile file{"%.17g"};               /* created at the first measurement */
    PetscErrorCode ReadOptions(MPI_Comm comm, PetscMPIInt size, PetscInt num_sites) { return ReadSiteListOption(comm, size, "-dsf_pm", "the Chebyshev recursion", sites, use, num_sites); }

    template<class Hamiltonian> PetscErrorCode Run(const MeasurementContext& ctx, const Hamiltonian& Ham, const ChebyshevOptions& cheb)
    {
        PetscErrorCode ierr;
        const PetscInt K = cheb.steps;
        for (int channel = 0; channel < 2; ++channel) {
            PetscLogDouble t0, t1;
            PetscTime(&t0);
            const char* cname = channel == 0 ? "MinusPlus" : "PlusMinus";
            const PetscReal sector = ctx.qn_sector + (channel == 0 ? 1.0 : -1.0);
            SzFrame S;
            ierr = S.Init(ctx.KronBlocks, ctx.num_sites, Ham, ctx.psi, "Transverse dynamics", channel == 0 ? OpSp : OpSm); CHKERRQ(ierr);
            const PetscInt N = S.F.N, M = S.M;
            KronBlocks_t KB1(ctx.KronBlocks.LeftBlockRefMod(), ctx.KronBlocks.RightBlockRefMod(), {sector}, NULL, ctx.GlobIdx);
            const int64_t n1 = KB1.NumStates(), ld1 = n1 + (n1 & 1);

            const std::vector<double>* omega = cheb.grid();
            std::vector<MomentRun> runs(sites.size());
            for (size_t ir = 0; ir < runs.size(); ++ir) runs[ir].c = sites[ir];
            PetscInt matmults = 0;
            ChebyshevSpectralWindow W;
            if (n1 > 0) {
                /* the images of all sites in the layout of KB1, row s = O_s psi */
                std::vector<int32_t> out_il, out_ir;
                for (PetscInt k = 0; k < KB1.size(); ++k) { out_il.push_back((int32_t)KB1.LeftIdx(k)); out_ir.push_back((int32_t)KB1.RightIdx(k)); }
                std::unique_ptr<DevBuffer> U;
                ierr = S.AllImages(U, n1, &out_il, &out_ir); CHKERRQ(ierr);
                /* the plan of the neighbouring sector */
                Mat H1 = nullptr;
                ierr = KB1.KronSumSetRedistribute(PETSC_TRUE); CHKERRQ(ierr);
                ierr = KB1.KronSumSetToleranceFromOptions(); CHKERRQ(ierr);
                ierr = KB1.KronSumSetShellMatrix(ctx.do_shell); CHKERRQ(ierr);
                ierr = KB1.KronSumConstruct(ctx.Terms, H1); CHKERRQ(ierr);
                if (!H1) SETERRQ(ctx.mpi_comm, 1, "Transverse dynamics: H is null.");
                /* the window: the bottom of this sector is not known */
                ierr = cheb.FindWindow(ctx.mpi_comm, H1->plan, n1, nullptr, std::string("Transverse dynamics (") + cname + ")", W); CHKERRQ(ierr);
                matmults = W.bound_steps;
                std::vector<double> cross;
                for (MomentRun& R : runs) {
                    ierr = ChebyshevMomentRun(H1->plan, U->dev_ro(), ld1, N, W, K, S.norm, cross, R, nullptr); CHKERRQ(ierr);
                    matmults += K;
                    if (R.norm2 == 0.0) printf("  * -dsf_pm (%s): the image of site %lld is zero in the bases of the blocks; no run.\n", cname, LLD(R.c));
                    else WarnLeftWindow("-dsf_pm", cname, "site", R, W, K);
                    R.momq = SiteCosineSum(S.Lx, S.Ly, S.rx.data(), S.ry.data(), R.c, R.mom.data(), N, R.done + 1);
                    if (omega) R.grid = ChebyshevGrid(R.momq, R.done + 1, *omega, (double)ctx.E0, W.centre, W.half_width);
                }
                ierr = MatDestroy_KronSumShell(&H1); CHKERRQ(ierr);
                ierr = MatDestroy(&H1); CHKERRQ(ierr);
            }                                                       /* (the images go back to the pool here) */
            PetscTime(&t1);
            if (ctx.verbose) printf("  * Transverse dynamics (%s): sector %g, %lld reference sites, %lld steps per run, window [%.6f, %.6f] from %lld Lanczos steps, %lld MatMults on %lld states, tDsfPm %.6f s\n",
                                    cname, (double)sector, LLD(runs.size()), LLD(K), W.centre - W.half_width, W.centre + W.half_width, LLD(W.bound_steps), LLD(matmults), LLD(n1), t1 - t0);
            ierr = file.BeginDynamical(ctx.data_dir + "TransverseDynamics.json", ctx.GlobIdx, ctx.loop_type, (double)ctx.E0, S.norm); CHKERRQ(ierr);
            FILE* fp = file.fp;
            fprintf(fp, ", \"Channel\": \"%s\", \"Sector\": %.17g, \"States\": %lld, \"Steps\": %lld, \"Centre\": %.17g, \"HalfWidth\": %.17g, \"BoundSteps\": %lld, \"ThetaMin\": %.17g, \"ThetaMax\": %.17g, \"tDsfPm\": %.9g, \"MatMults\": %lld,\n",
                    cname, (double)sector, LLD(n1), LLD(K), W.centre, W.half_width, LLD(W.bound_steps), W.theta_min, W.theta_max, t1 - t0, LLD(matmults));
            file.Omega(omega);
            fprintf(fp, "   \"Sites\": [\n");
            for (size_t ir = 0; ir < runs.size(); ++ir) {
                const MomentRun& R = runs[ir];
                const char* end = ir + 1 < runs.size() ? "},\n" : "}\n";
                file.OpenSite(R.c, S.rx[(size_t)R.c], S.ry[(size_t)R.c], R.norm2);
                fprintf(fp, ", \"StepsDone\": %d", (int)R.done);
                if (n1 == 0) fprintf(fp, "%s", end);                       /* no run: no moments */
                else file.Moments(R, N, M, omega, end);
            }
            fprintf(fp, "   ]}");
            fflush(fp);
        }
        return 0;
    }
};

/** -dsf_cv c0,c1,... (engine extension): the real-space dynamical correlations of the ground state at given complex frequencies,
        G_ic(w_k + i eta) = < Sz_i psi , 1 / (E0 + w_k + i eta - H) Sz_c psi > / <psi|psi>,   for ALL sites i,
    by the correction-vector method: one dmrgx_kron_correction_vector call per reference site c and frequency w_k of -dsf_cv_omega
    solves [(H - sigma)^2 + eta^2] Y = -eta Sz_c psi, sigma = E0 + w_k, by conjugate gradients on the device to the relative residual
    -dsf_cv_tol (at most -dsf_cv_maxit iterations, two MatMults each), forms X = (H - sigma) Y / eta and takes the overlaps of both with
    the images of all sites.  Unlike -dsf, -dsf_sites and -dsf_cheb the error at each frequency is controlled -- |ImG - exact| <=
    |u| |v| Residual / eta -- and the broadening is a true Lorentzian of half width eta.  No warm start between frequencies.
    The images u_i = Sz_i psi of all N sites (SzFrame::Images, lattice order) stay on the device for the whole measurement, as
    for -dsf_cheb; beside them Y, X and the four pool vectors of the solver: N + 6 vectors of N_sb doubles.
    The record: ImG[i][k], ReG[i][k] (the overlaps over <psi|psi>), Aw[i][k] = -ImG / pi, SqwGrid[q][k] = sum_i cos(q . (r_i - r_c))
    Aw[i][k] (SiteCosineSum, row nx Ly + ny; (1/N) sum_c SqwGrid is the Lorentzian-broadened S^zz(q, w)), Iterations[k], Converged[k]
    and Residual[k], the true residual |b - A Y| / |b| of the returned Y.  A frequency that did not converge within -dsf_cv_maxit is
    written as it is, with a warning here.  The caveats of -dsf_sites apply: the block bases are optimised for the ground state alone
    -- no correction vector is targeted in the density matrix.  One rank only (refused at start-up otherwise). */
struct CorrectionVectors {
    PetscBool use = PETSC_FALSE;                /* -dsf_cv c0,c1,... */
    std::vector<PetscInt> sites;                /* the reference sites c, lattice numbering of To1D */
    std::vector<double> omega;                  /* -dsf_cv_omega w0,w1,nw: the frequencies, one solve per site and frequency */
    PetscReal eta = 0.1;                        /* -dsf_cv_eta: half width at half maximum of the Lorentzian */
    PetscReal tol = 1e-8;                       /* -dsf_cv_tol: |r| <= tol |b| ends a solve */
    PetscInt maxit = 2000;                      /* -dsf_cv_maxit: iterations per solve at most */
    JsonRecordFile file{"%.17g"};               /* created at the first measurement */
    PetscErrorCode ReadOptions(MPI_Comm comm, PetscMPIInt size, PetscInt num_sites)
    {
        PetscErrorCode ierr = ReadSiteListOption(comm, size, "-dsf_cv", "the conjugate-gradient run", sites, use, num_sites); CHKERRQ(ierr);
        if (!use) return 0;
        PetscBool have_omega = PETSC_FALSE;
        ierr = ReadOmegaGridOption(comm, "-dsf_cv_omega", omega, have_omega); CHKERRQ(ierr);
        if (!have_omega) SETERRQ(comm, PETSC_ERR_ARG_WRONG, "-dsf_cv needs -dsf_cv_omega w0,w1,nw: the frequencies at which the correction vectors are solved.");
        ierr = PetscOptionsGetReal(NULL, NULL, "-dsf_cv_eta", &eta, NULL); CHKERRQ(ierr);
        if (!(eta > 0.0) || !std::isfinite(eta)) SETERRQ1(comm, PETSC_ERR_ARG_OUTOFRANGE, "-dsf_cv_eta must be positive and finite. Got %g.", eta);
        ierr = PetscOptionsGetReal(NULL, NULL, "-dsf_cv_tol", &tol, NULL); CHKERRQ(ierr);
        if (!(tol > 0.0) || tol >= 1.0) SETERRQ1(comm, PETSC_ERR_ARG_OUTOFRANGE, "-dsf_cv_tol must lie in (0, 1). Got %g.", tol);
        ierr = PetscOptionsGetInt(NULL, NULL, "-dsf_cv_maxit", &maxit, NULL); CHKERRQ(ierr);
        if (maxit < 1) SETERRQ1(comm, PETSC_ERR_ARG_OUTOFRANGE, "-dsf_cv_maxit must be at least 1. Got %lld.", LLD(maxit));
        return 0;
    }

    template<class Hamiltonian> PetscErrorCode Run(const MeasurementContext& ctx, const Hamiltonian& Ham)
    {
        PetscLogDouble t0, t1;
        PetscTime(&t0);
        SzFrame S;
        PetscErrorCode ierr = S.Init(ctx.KronBlocks, ctx.num_sites, Ham, ctx.psi, "Correction vectors"); CHKERRQ(ierr);
        const PetscInt N = S.F.N, M = S.M, nw = (PetscInt)omega.size();
        const int64_t n = S.n, ld = S.ld;
        /* the images of all sites, row s = Sz_s psi, and the two vectors of a solve */
        std::unique_ptr<DevBuffer> U, YX;
        try {
            U.reset(new DevBuffer((size_t)(N * ld), DevBuffer::device_only_t{}));
            YX.reset(new DevBuffer((size_t)(2 * ld), DevBuffer::device_only_t{}));
        }
        catch (const std::exception& e) { SETERRQ3(ctx.mpi_comm, PETSC_ERR_MEM, "Correction vectors: no memory for the images of %lld sites and two vectors of %lld states (%.3f GB): %s", LLD(N), LLD(n), (double)((N + 2) * ld) * 8e-9, e.what()); }
        ierr = S.Images(S.op_of.data(), N, U->dev_uninitialised(), ld); CHKERRQ(ierr);

        struct Run_t { PetscInt c = 0; double norm2 = 0.0; std::vector<double> iterations, converged, residual, im, re, aw, grid; };
        std::vector<Run_t> runs(sites.size());
        std::vector<double> im((size_t)N), re((size_t)N);
        double* Yd = YX->dev_uninitialised();
        double* Xd = Yd + ld;
        PetscInt matmults = 0, iterations = 0;
        for (size_t ir = 0; ir < runs.size(); ++ir) {
            Run_t& R = runs[ir];
            R.c = sites[ir];
            R.iterations.assign((size_t)nw, 0.0); R.converged.assign((size_t)nw, 0.0); R.residual.assign((size_t)nw, 0.0);
            R.im.assign((size_t)(N * nw), 0.0); R.re.assign((size_t)(N * nw), 0.0); R.aw.assign((size_t)(N * nw), 0.0);
            for (PetscInt k = 0; k < nw; ++k) {
                dmrgx_cv_stats cs;
                if (dmrgx_kron_correction_vector(ctx.plan(), U->dev_ro() + R.c * ld, (double)ctx.E0 + omega[(size_t)k], eta, tol, (int32_t)maxit, 0, Yd, Xd,
                                                 (int32_t)N, U->dev_ro(), ld, &R.norm2, im.data(), re.data(), &cs, nullptr))
                    SETERRQ1(ctx.mpi_comm, 1, "dmrgx_kron_correction_vector: %s", dmrgx_last_error());
                matmults += cs.n_matvec; iterations += cs.iterations;
                if (!cs.converged) printf("  * WARNING: -dsf_cv: site %lld, w = %.6f: not converged after %d iterations (residual %.3e, tol %.3e%s); the record holds the last iterate.\n",
                                          LLD(R.c), omega[(size_t)k], (int)cs.iterations, cs.true_residual, tol, cs.dead ? ", the iteration broke down" : "");
                R.iterations[(size_t)k] = (double)cs.iterations; R.converged[(size_t)k] = (double)cs.converged; R.residual[(size_t)k] = cs.true_residual;
                for (PetscInt s = 0; s < N; ++s) {
                    const size_t at = (size_t)(s * nw + k);
                    R.im[at] = im[(size_t)s] / S.norm; R.re[at] = re[(size_t)s] / S.norm; R.aw[at] = -R.im[at] / (0.5 * two_pi);
                }
            }
            R.grid = SiteCosineSum(S.Lx, S.Ly, S.rx.data(), S.ry.data(), R.c, R.aw.data(), N, nw);
        }
        PetscTime(&t1);
        if (ctx.verbose) printf("  * Correction vectors: %lld reference sites x %lld frequencies, eta %.6f, %lld iterations, %lld MatMults on %lld states, tDsfCv %.6f s\n",
                                LLD(runs.size()), LLD(nw), eta, LLD(iterations), LLD(matmults), LLD(n), t1 - t0);
        ierr = file.BeginDynamical(ctx.data_dir + "CorrectionVectors.json", ctx.GlobIdx, ctx.loop_type, (double)ctx.E0, S.norm); CHKERRQ(ierr);
        FILE* fp = file.fp;
        fprintf(fp, ", \"Eta\": %.17g, \"Tol\": %.17g, \"MaxIt\": %lld, \"tDsfCv\": %.9g, \"MatMults\": %lld,\n   \"Omega\": ", eta, tol, LLD(maxit), t1 - t0, LLD(matmults));
        file.Row(omega);
        fprintf(fp, ",\n   \"Sites\": [\n");
        for (size_t ir = 0; ir < runs.size(); ++ir) {
            const Run_t& R = runs[ir];
            file.OpenSite(R.c, S.rx[(size_t)R.c], S.ry[(size_t)R.c], R.norm2);
            fprintf(fp, ",\n   \"Iterations\": ");
            file.Row(R.iterations); fprintf(fp, ",\n   \"Converged\": ");
            file.Row(R.converged); fprintf(fp, ",\n   \"Residual\": ");
            file.Row(R.residual); fprintf(fp, ",\n");
            file.Table("ImG", R.im, N, nw, ",\n");
            file.Table("ReG", R.re, N, nw, ",\n");
            file.Table("Aw", R.aw, N, nw, ",\n");
            file.Table("SqwGrid", R.grid, M, nw, ir + 1 < runs.size() ? "},\n" : "}\n");
        }
        fprintf(fp, "   ]}");
        fflush(fp);
        return 0;
    }
};

/** -chi_sites c0,c1,... and -chi_bonds b0,b1,... (engine extension): the static susceptibilities of the ground state,
        chi_ic = d<O_i>/dh_c = 2 sum_{n>0} <0|O_i|n><n|O_c|0> / (E_n - E0),   for ALL sites (bonds) i,
    O = Sz of a lattice site (-chi_sites, lattice numbering) or O = D_b = S_i . S_j of a nearest-neighbour bond (-chi_bonds, the index in
    DimerBonds(Ham) as for -dsf_dimer): the linear response to a field the Hamiltonian does not have.  One dmrgx_kron_static_response call
    per reference c solves Q (H - E0) Q X = Q O_c psi, Q = 1 - |psi><psi| / <psi|psi>, by conjugate gradients on the device to the
    relative residual -chi_tol (at most -chi_maxit iterations, ONE MatMult each, no eta) and takes the overlaps of X with the images of
    all sites (bonds).  The solver deflates psi itself and returns Mean = <O_c> as its coefficient: no dmrgx_vec_project_out.  The error
    is controlled: |Chi - exact| <= 2 |u| |Q v| Residual / gap.
    The images (SzFrame::Images of all N sites, then DimerFrame::Images of all nb bonds: one family at a time) stay on the device for
    their solves; beside them X and the four pool vectors of the solver: max(N, nb) + 5 vectors of N_sb doubles.
    The record: per reference Norm2 = |Q O_c psi|^2 / Norm, Mean, Iterations, Converged, Residual (the true residual |b - A X| / |b| of
    the returned X), Chi[i] = 2 <u_i, X> / Norm, ChiQ[q] = sum_i cos(q . (r_i - r_c)) Chi[i] (SiteCosineSum, row nx Ly + ny; for a bond
    over the bonds of c's orientation at their Positions, as MomentsQ of -dsf_dimer).  A solve that did not converge within -chi_maxit is
    written as it is, with a warning here.  The caveat of -dsf_sites applies: the block bases are optimised for the ground state alone
    -- X is not targeted in the density matrix, so Chi is exact while nothing is truncated and an approximation that m controls otherwise.
    One rank only (refused at start-up otherwise). */
struct StaticSusceptibility {
    PetscBool use = PETSC_FALSE, use_sites = PETSC_FALSE, use_bonds = PETSC_FALSE;
    std::vector<PetscInt> sites;                /* -chi_sites c0,c1,...: the reference sites, lattice numbering of To1D */
    std::vector<PetscInt> bonds;                /* -chi_bonds b0,b1,...: the reference bonds, their index in DimerBonds(Ham) */
    PetscReal tol = 1e-8;                       /* -chi_tol: |r| <= tol |b| ends a solve */
    PetscInt maxit = 2000;                      /* -chi_maxit: iterations per solve at most */
    JsonRecordFile file{"%.17g"};               /* created at the first measurement */
    PetscErrorCode ReadOptions(MPI_Comm comm, PetscMPIInt size, PetscInt num_sites, PetscInt num_bonds)
    {
        PetscErrorCode ierr = ReadSiteListOption(comm, size, "-chi_sites", "the conjugate-gradient run", sites, use_sites, num_sites); CHKERRQ(ierr);
        ierr = ReadSiteListOption(comm, size, "-chi_bonds", "the conjugate-gradient run", bonds, use_bonds, num_bonds, "bond",
                                  "the nearest-neighbour bonds in the order of Bonds in DimerCorrelations.json"); CHKERRQ(ierr);
        use = (use_sites || use_bonds) ? PETSC_TRUE : PETSC_FALSE;
        if (!use) return 0;
        ierr = PetscOptionsGetReal(NULL, NULL, "-chi_tol", &tol, NULL); CHKERRQ(ierr);
        if (!(tol > 0.0) || tol >= 1.0) SETERRQ1(comm, PETSC_ERR_ARG_OUTOFRANGE, "-chi_tol must lie in (0, 1). Got %g.", tol);
        ierr = PetscOptionsGetInt(NULL, NULL, "-chi_maxit", &maxit, NULL); CHKERRQ(ierr);
        if (maxit < 1) SETERRQ1(comm, PETSC_ERR_ARG_OUTOFRANGE, "-chi_maxit must be at least 1. Got %lld.", LLD(maxit));
        return 0;
    }

    struct Run_t { PetscInt c = 0; double norm2 = 0.0, mean = 0.0, residual = 0.0; int iterations = 0, converged = 0; std::vector<double> chi, chiq; };

    /** The solves of one family of `count` images U (row stride ld): R.c is given, the rest of R is filled. */
    PetscErrorCode Solve(const MeasurementContext& ctx, const char* option, const char* noun, const double* psi, double norm, const double* U, int64_t ld, PetscInt count,
                         double* X, std::vector<Run_t>& runs, PetscInt& matmults, PetscInt& iterations) const
    {
        std::vector<double> chi((size_t)count);
        for (Run_t& R : runs) {
            dmrgx_cv_stats cs;
            if (dmrgx_kron_static_response(ctx.plan(), psi, U + R.c * ld, (double)ctx.E0, tol, (int32_t)maxit, 0, X, (int32_t)count, U, ld, &R.mean, &R.norm2, chi.data(), &cs, nullptr))
                SETERRQ1(ctx.mpi_comm, 1, "dmrgx_kron_static_response: %s", dmrgx_last_error());
            matmults += cs.n_matvec; iterations += cs.iterations;
            if (!cs.converged) printf("  * WARNING: %s: %s %lld: not converged after %d iterations (residual %.3e, tol %.3e%s); the record holds the last iterate.\n",
                                      option, noun, LLD(R.c), (int)cs.iterations, cs.true_residual, tol, cs.dead ? ", the iteration broke down" : "");
            R.norm2 /= norm; R.iterations = (int)cs.iterations; R.converged = (int)cs.converged; R.residual = cs.true_residual;
            R.chi.resize((size_t)count);
            for (PetscInt i = 0; i < count; ++i) R.chi[(size_t)i] = 2.0 * chi[(size_t)i] / norm;
        }
        return 0;
    }

    void WriteTail(const Run_t& R, PetscInt M, const char* end) const
    {
        FILE* fp = file.fp;
        fprintf(fp, ", \"Mean\": %.17g, \"Iterations\": %d, \"Converged\": %d, \"Residual\": %.17g,\n   \"Chi\": ", R.mean, R.iterations, R.converged, R.residual);
        file.Row(R.chi); fprintf(fp, ",\n   \"ChiQ\": ");
        file.Row(R.chiq.data(), M); fprintf(fp, "%s", end);
    }

    template<class Hamiltonian> PetscErrorCode Run(const MeasurementContext& ctx, const Hamiltonian& Ham)
    {
        PetscLogDouble t0, t1;
        PetscTime(&t0);
        PetscErrorCode ierr;
        const PetscInt Lx = Ham.Lx(), Ly = Ham.Ly(), M = Lx * Ly;
        PetscInt matmults = 0, iterations = 0;
        int64_t n = 0;
        double norm = 0.0;
        std::vector<Run_t> site_runs(sites.size()), bond_runs(bonds.size());
        std::vector<PetscInt> site_x, site_y;
        std::vector<DimerBond> all_bonds;
        if (use_sites) {
            SzFrame S;
            ierr = S.Init(ctx.KronBlocks, ctx.num_sites, Ham, ctx.psi, "Static susceptibility"); CHKERRQ(ierr);
            const PetscInt N = S.F.N;
            const int64_t ld = S.ld;
            n = S.n; norm = S.norm;
            /* the images of all sites, row s = Sz_s psi, and the solution of a solve */
            std::unique_ptr<DevBuffer> U, X;
            try {
                U.reset(new DevBuffer((size_t)(N * ld), DevBuffer::device_only_t{}));
                X.reset(new DevBuffer((size_t)ld, DevBuffer::device_only_t{}));
            }
            catch (const std::exception& e) { SETERRQ4(ctx.mpi_comm, PETSC_ERR_MEM, "Static susceptibility: no memory for the images of %lld sites and one vector of %lld states (%.3f GB): %s", LLD(N), LLD(n), (double)((N + 1) * ld) * 8e-9, e.what()); }
            ierr = S.Images(S.op_of.data(), N, U->dev_uninitialised(), ld); CHKERRQ(ierr);
            for (size_t ir = 0; ir < site_runs.size(); ++ir) site_runs[ir].c = sites[ir];
            ierr = Solve(ctx, "-chi_sites", "site", S.psi, norm, U->dev_ro(), ld, N, X->dev_uninitialised(), site_runs, matmults, iterations); CHKERRQ(ierr);
            for (Run_t& R : site_runs) R.chiq = SiteCosineSum(S.Lx, S.Ly, S.rx.data(), S.ry.data(), R.c, R.chi.data(), N, 1);
            site_x = S.rx; site_y = S.ry;
        }
        if (use_bonds) {
            DimerFrame B;
            ierr = B.Init(ctx.KronBlocks, ctx.num_sites, Ham, ctx.psi, "Static susceptibility"); CHKERRQ(ierr);
            const PetscInt nb = B.nb;
            n = B.n;
            const int64_t ld = n + (n & 1);
            if (dmrgx_dot(n, B.psi, B.psi, &norm, nullptr)) SETERRQ1(ctx.mpi_comm, 1, "dmrgx_dot: %s", dmrgx_last_error());
            if (!(norm > 0.0)) SETERRQ(ctx.mpi_comm, 1, "Static susceptibility: the ground state has no norm.");
            /* the images of all bonds, row b = D_b psi, and the solution of a solve */
            std::unique_ptr<DevBuffer> U, X;
            try {
                U.reset(new DevBuffer((size_t)(nb * ld), DevBuffer::device_only_t{}));
                X.reset(new DevBuffer((size_t)ld, DevBuffer::device_only_t{}));
            }
            catch (const std::exception& e) { SETERRQ4(ctx.mpi_comm, PETSC_ERR_MEM, "Static susceptibility: no memory for the images of %lld bonds and one vector of %lld states (%.3f GB): %s", LLD(nb), LLD(n), (double)((nb + 1) * ld) * 8e-9, e.what()); }
            ierr = B.Images(U->dev_uninitialised(), ld); CHKERRQ(ierr);
            for (size_t ir = 0; ir < bond_runs.size(); ++ir) bond_runs[ir].c = bonds[ir];
            ierr = Solve(ctx, "-chi_bonds", "bond", B.psi, norm, U->dev_ro(), ld, nb, X->dev_uninitialised(), bond_runs, matmults, iterations); CHKERRQ(ierr);
            /* the cosine sum over the bonds of c's orientation, from c */
            const OrientedBonds oriented[2] = {BondsOfOrientation(B.bonds, 'x'), BondsOfOrientation(B.bonds, 'y')};
            for (Run_t& R : bond_runs) {
                const OrientedBonds& O = oriented[B.bonds[(size_t)R.c].orient == 'x' ? 0 : 1];
                const PetscInt no = (PetscInt)O.of.size(), c_in = (PetscInt)(std::find(O.of.begin(), O.of.end(), R.c) - O.of.begin());
                std::vector<double> sel((size_t)no);
                for (PetscInt k = 0; k < no; ++k) sel[(size_t)k] = R.chi[(size_t)O.of[(size_t)k]];
                R.chiq = SiteCosineSum(Lx, Ly, O.x.data(), O.y.data(), c_in, sel.data(), no, 1);
            }
            all_bonds = B.bonds;
        }
        PetscTime(&t1);
        if (ctx.verbose) printf("  * Static susceptibility: %lld reference sites, %lld reference bonds, %lld iterations, %lld MatMults on %lld states, tChi %.6f s\n",
                                LLD(site_runs.size()), LLD(bond_runs.size()), LLD(iterations), LLD(matmults), LLD(n), t1 - t0);
        ierr = file.BeginDynamical(ctx.data_dir + "StaticSusceptibility.json", ctx.GlobIdx, ctx.loop_type, (double)ctx.E0, norm); CHKERRQ(ierr);
        FILE* fp = file.fp;
        fprintf(fp, ", \"Tol\": %.17g, \"MaxIt\": %lld, \"tChi\": %.9g, \"MatMults\": %lld,\n   \"Sites\": [\n", tol, LLD(maxit), t1 - t0, LLD(matmults));
        for (size_t ir = 0; ir < site_runs.size(); ++ir) {
            const Run_t& R = site_runs[ir];
            file.OpenSite(R.c, site_x[(size_t)R.c], site_y[(size_t)R.c], R.norm2);
            WriteTail(R, M, ir + 1 < site_runs.size() ? "},\n" : "}\n");
        }
        fprintf(fp, "   ],\n   \"Bonds\": [\n");
        for (size_t ir = 0; ir < bond_runs.size(); ++ir) {
            const Run_t& R = bond_runs[ir];
            const DimerBond& bc = all_bonds[(size_t)R.c];
            fprintf(fp, "   {\"Bond\": %lld, \"Sites\": [%lld, %lld], \"Orientation\": \"%c\", \"r\": [%lld, %lld], \"Norm2\": %.17g", LLD(R.c), LLD(bc.i), LLD(bc.j), bc.orient, LLD(bc.ix), LLD(bc.jy), R.norm2);
            WriteTail(R, M, ir + 1 < bond_runs.size() ? "},\n" : "}\n");
        }
        fprintf(fp, "   ]}");
        fflush(fp);
        return 0;
    }
};

/** -states_corr 1 (engine extension, with -nstates k >= 2): what the k targeted states ARE -- the correlations of every state and the
    transition amplitudes between them, at every measurement point.  Four dmrgx_kron_term_gram_states calls on the k_step states of the
    step (the rows of MeasurementContext::states), each the Gram matrix of a state-major family of images O_a psi_s:
        identity + Sz of every site (shift 0), Sp of every site (+1), Sm of every site (Sp read transposed, -1),
        identity + the bond images D_b = S_i . S_j (DimerFrame's operators and terms, built once; shift 0).
    The block (s, t) of a Gram matrix is < O_a psi_s , O_b psi_t > = < psi_s | O_a^T O_b | psi_t >; its identity row is the one-point
    amplitude < psi_s | O_b | psi_t >.  The record (StateCorrelations.json, one per measurement):
      Energies, Overlaps (k x k, the identity rows of the first family), tStates (seconds), the bond list;
      Sz[s][t] (N numbers, lattice numbering) and D[s][t] (nb numbers) for all s, t: the transition amplitudes;
      TransitionSz[s][t]: the Lx x Ly single-mode weights W(q) = (1/N) |sum_i e^(i q . r_i) Sz[s][t][i]|^2 (TransitionWeight, Measurements.hpp) --
        with E_s - E_t the momentum and the weight of the pole that state s contributes to S^zz(q, w) of state t;
      States[s]: SzSz, SmSp, SpSm, SS, StructureFactor (the tables of -corr_matrix, same formulas, SS with + Sz_i on its diagonal) and DD
        (the table of -corr_dimer), from the diagonal blocks (s, s);
      with -states_corr_cross 1, Cross: per pair s < t the off-diagonal blocks SzSz, SmSp, SpSm, DD.  Of an exactly degenerate pair the
        solver returns an arbitrary rotation: only the whole 2 x 2 block over the pair has meaning, and this is where it is.
    Every table is < psi_s | O_a^T O_b | psi_t > of TRUNCATED block operators: it equals < psi_s | O_a O_b | psi_t > (O^T for Sp: Sm) when
    nothing was truncated or the two operators sit in different blocks -- truncated operators of one block do not commute, the caveat of
    the SpSm table of -corr_matrix.  The signs of nondegenerate states are arbitrary: Sz[s][t] and D[s][t], s != t, carry the product of two.
    Memory: the images of all k_step states of one family at a time (workspace slices of at least the largest image block of every member).
    One rank, no noise: the limits of -nstates. */
struct StateCorrelations {
    PetscBool use = PETSC_FALSE;                /* -states_corr 1 */
    PetscBool cross = PETSC_FALSE;              /* -states_corr_cross 1: the off-diagonal blocks too */
    JsonRecordFile file{"%.17g"};               /* created at the first measurement */
    PetscErrorCode ReadOptions(MPI_Comm comm)
    {
        PetscErrorCode ierr = PetscOptionsGetBool(NULL, NULL, "-states_corr", &use, NULL); CHKERRQ(ierr);
        if (!use) return 0;
        ierr = PetscOptionsGetBool(NULL, NULL, "-states_corr_cross", &cross, NULL); CHKERRQ(ierr);
        PetscInt k = 1;
        PetscBool set = PETSC_FALSE;
        ierr = PetscOptionsGetInt(NULL, NULL, "-nstates", &k, &set); CHKERRQ(ierr);
        if (!set || k < 2) SETERRQ1(comm, PETSC_ERR_ARG_WRONG, "-states_corr 1 needs -nstates k with k >= 2: it measures the targeted states against each other. Got -nstates %lld.", LLD(set ? k : 1));
        return 0;
    }

    template<class Hamiltonian> PetscErrorCode Run(const MeasurementContext& ctx, const Hamiltonian& Ham)
    {
        const TargetedStatesView& V = ctx.states;
        const PetscInt k = V.count;
        if (k < 2) return 0;                                        /* a step whose sector holds one state: nothing between states */
        PetscLogDouble t0, t1;
        PetscTime(&t0);
        PetscErrorCode ierr;
        DimerFrame B;                                               /* (its CentreFrame serves the site families too) */
        ierr = B.Init(ctx.KronBlocks, ctx.num_sites, Ham, ctx.psi, "State correlations"); CHKERRQ(ierr);
        const CentreFrame& F = B.F;
        const PetscInt N = F.N, nb = B.nb, Lx = Ham.Lx(), Ly = Ham.Ly();
        std::vector<PetscInt> site;                                 /* lattice site of vector a of a site family (identity: -1) */
        std::vector<double> G;
        /* one site family over all states: [identity] + the operator of every left site + of every right site; G is (k n)^2, state-major */
        auto family = [&](Op_t type, bool with_identity, PetscInt& n) -> PetscErrorCode {
            SiteOperators T(F);
            site.clear();
            std::vector<dmrgx_term> terms;
            if (with_identity) { terms.push_back(dmrgx_term{1.0, -1, -1}); site.push_back(-1); }
            PetscErrorCode e = T.AllSites(type, site); CHKERRQ(e);
            for (int32_t a = 0; a < (int32_t)T.ops[0].size(); ++a) terms.push_back(dmrgx_term{1.0, a, -1});
            for (int32_t b = 0; b < (int32_t)T.ops[1].size(); ++b) terms.push_back(dmrgx_term{1.0, -1, b});
            n = (PetscInt)terms.size();
            std::vector<int32_t> first((size_t)n + 1);
            for (PetscInt a = 0; a <= n; ++a) first[(size_t)a] = (int32_t)a;
            /* the workspace holds at least the largest image block of every member: (IL - d, IR) and (IL, IR - d) of the family's shift d */
            const int32_t d = type == OpSz ? 0 : (type == OpSp ? 1 : -1);
            int64_t largest = 1;
            for (size_t q = 0; q < F.bil.size(); ++q) {
                const int32_t a = F.bil[q] - d, c = F.bir[q] - d;
                if (a >= 0 && a < (int32_t)F.sizes[0].size()) largest = std::max<int64_t>(largest, (int64_t)F.sizes[0][(size_t)a] * F.sizes[1][(size_t)F.bir[q]]);
                if (c >= 0 && c < (int32_t)F.sizes[1].size()) largest = std::max<int64_t>(largest, (int64_t)F.sizes[0][(size_t)F.bil[q]] * F.sizes[1][(size_t)c]);
            }
            const PetscInt nf = k * n;
            const size_t workspace = std::max<size_t>((size_t)1 << 30, (size_t)largest * (size_t)nf * sizeof(double));
            DevBuffer g((size_t)(nf * nf), DevBuffer::device_only_t{});
            if (dmrgx_kron_term_gram_states(&F.sectors[0], &F.sectors[1], (int32_t)F.bil.size(), F.bil.data(), F.bir.data(), (int32_t)k, V.rows, V.ld, (int32_t)T.ops[0].size(), T.ops[0].data(), (int32_t)T.ops[1].size(), T.ops[1].data(),
                                            (int32_t)n, first.data(), terms.data(), workspace, g.dev_uninitialised(), nf, nullptr, nullptr)) SETERRQ1(ctx.mpi_comm, 1, "dmrgx_kron_term_gram_states: %s", dmrgx_last_error());
            G.assign((size_t)(nf * nf), 0.0);
            if (dmrgx_memcpy_d2h(G.data(), g.dev_ro(), G.size() * sizeof(double), nullptr)) SETERRQ1(ctx.mpi_comm, 1, "%s", dmrgx_last_error());
            return 0;
        };
        /* the block (s, t) of a site family's G as a table over lattice sites */
        auto block = [&](PetscInt s, PetscInt t, PetscInt n, PetscInt first) {
            std::vector<double> table((size_t)(N * N), 0.0);
            for (PetscInt a = first; a < n; ++a) for (PetscInt b = first; b < n; ++b)
                table[(size_t)(site[(size_t)a] * N + site[(size_t)b])] = G[(size_t)((s * n + a) * (k * n) + t * n + b)];
            return table;
        };
        typedef std::vector<std::vector<double>> Blocks;            /* [s * k + t] */
        Blocks SzSz((size_t)(k * k)), SmSp((size_t)(k * k)), SpSm((size_t)(k * k)), DD((size_t)(k * k)), Sz((size_t)(k * k)), D((size_t)(k * k)), W((size_t)(k * k));
        std::vector<double> overlaps((size_t)(k * k), 0.0);
        auto wanted = [&](PetscInt s, PetscInt t) { return s == t || (cross && s < t); };
        PetscInt n = 0;
        ierr = family(OpSz, true, n); CHKERRQ(ierr);
        for (PetscInt s = 0; s < k; ++s) for (PetscInt t = 0; t < k; ++t) {
            overlaps[(size_t)(s * k + t)] = G[(size_t)((s * n) * (k * n) + t * n)];
            Sz[(size_t)(s * k + t)].assign((size_t)N, 0.0);
            for (PetscInt a = 1; a < n; ++a) Sz[(size_t)(s * k + t)][(size_t)site[(size_t)a]] = G[(size_t)((s * n) * (k * n) + t * n + a)];      /* < psi_s , Sz_i psi_t > */
            if (wanted(s, t)) SzSz[(size_t)(s * k + t)] = block(s, t, n, 1);
        }
        ierr = family(OpSp, false, n); CHKERRQ(ierr);
        for (PetscInt s = 0; s < k; ++s) for (PetscInt t = s; t < k; ++t) if (wanted(s, t)) SmSp[(size_t)(s * k + t)] = block(s, t, n, 0);
        ierr = family(OpSm, false, n); CHKERRQ(ierr);
        for (PetscInt s = 0; s < k; ++s) for (PetscInt t = s; t < k; ++t) if (wanted(s, t)) SpSm[(size_t)(s * k + t)] = block(s, t, n, 0);
        ierr = B.GramStates(k, V.rows, V.ld, G); CHKERRQ(ierr);
        const PetscInt nv = nb + 1;
        for (PetscInt s = 0; s < k; ++s) for (PetscInt t = 0; t < k; ++t) {
            std::vector<double>& d = D[(size_t)(s * k + t)];
            d.assign((size_t)nb, 0.0);
            for (PetscInt b = 0; b < nb; ++b) d[(size_t)b] = G[(size_t)((s * nv) * (k * nv) + t * nv + 1 + b)];                               /* < psi_s , D_b psi_t > */
            if (!wanted(s, t)) continue;
            std::vector<double>& dd = DD[(size_t)(s * k + t)];
            dd.assign((size_t)(nb * nb), 0.0);
            for (PetscInt b = 0; b < nb; ++b) for (PetscInt c = 0; c < nb; ++c) dd[(size_t)(b * nb + c)] = G[(size_t)((s * nv + 1 + b) * (k * nv) + t * nv + 1 + c)];
        }
        /* the single-mode weights of every transition, and per state S_i . S_j and S(q) as -corr_matrix forms them */
        std::vector<PetscInt> rx((size_t)N), ry((size_t)N);
        for (PetscInt i = 0; i < N; ++i) { ierr = Ham.To2D(i, rx[(size_t)i], ry[(size_t)i]); CHKERRQ(ierr); }
        for (PetscInt st = 0; st < k * k; ++st) W[(size_t)st] = TransitionWeight(Lx, Ly, rx.data(), ry.data(), Sz[(size_t)st].data(), N);
        Blocks SS((size_t)k), Sq((size_t)k);
        for (PetscInt s = 0; s < k; ++s) {
            const size_t ss = (size_t)(s * k + s);
            SS[(size_t)s].assign((size_t)(N * N), 0.0);
            for (PetscInt i = 0; i < N; ++i) for (PetscInt j = 0; j < N; ++j) SS[(size_t)s][(size_t)(i * N + j)] = SzSz[ss][(size_t)(i * N + j)] + SmSp[ss][(size_t)(i * N + j)] + (i == j ? Sz[ss][(size_t)i] : 0.0);
            Sq[(size_t)s] = LatticeFourier(Lx, Ly, rx.data(), ry.data(), SS[(size_t)s].data(), N, (double)N);
        }
        PetscTime(&t1);
        if (!ctx.mpi_rank && ctx.verbose)
            printf("  * State correlations: %lld states, Gram of %lld vectors x %lld (Sz), %lld (Sp), %lld (Sm), %lld (bonds), tStates %.6f s\n", LLD(k), LLD(k * (N + 1)), LLD(ctx.psi->n), LLD(k * N), LLD(k * N), LLD(k * nv), t1 - t0);
        if (ctx.mpi_rank) return 0;
        ierr = file.Begin(ctx.data_dir + "StateCorrelations.json"); CHKERRQ(ierr);
        FILE* fp = file.fp;
        fprintf(fp, "  {\"GlobIdx\": %lld, \"LoopType\": \"%s\", \"NStates\": %lld, \"tStates\": %.9g,\n   \"Energies\": ", LLD(ctx.GlobIdx), ctx.loop_type, LLD(k), t1 - t0);
        file.Row(V.energies, k); fprintf(fp, ",\n");
        file.Table("Overlaps", overlaps, k, k, ",\n");
        file.BondList(B.bonds);
        /* name[s][t]: a row of `len` numbers, or (rows > 0) a rows x len / rows table, per pair of states */
        auto pairs = [&](const char* name, const Blocks& T, PetscInt len, PetscInt rows) {
            fprintf(fp, "   \"%s\": [\n", name);
            for (PetscInt s = 0; s < k; ++s) {
                fprintf(fp, "     [");
                for (PetscInt t = 0; t < k; ++t) {
                    const double* v = T[(size_t)(s * k + t)].data();
                    fprintf(fp, "%s", t ? ",\n      " : "");
                    if (rows == 0) file.Row(v, len);
                    else { fprintf(fp, "["); for (PetscInt r = 0; r < rows; ++r) { fprintf(fp, "%s", r ? ", " : ""); file.Row(v + r * (len / rows), len / rows); } fprintf(fp, "]"); }
                }
                fprintf(fp, "]%s\n", s + 1 < k ? "," : "");
            }
            fprintf(fp, "   ],\n");
        };
        pairs("Sz", Sz, N, 0); pairs("D", D, nb, 0); pairs("TransitionSz", W, Lx * Ly, Lx);
        fprintf(fp, "   \"States\": [\n");
        for (PetscInt s = 0; s < k; ++s) {
            const size_t ss = (size_t)(s * k + s);
            fprintf(fp, "   {\"State\": %lld, \"Energy\": %.17g,\n", LLD(s), V.energies[s]);
            file.Table("SzSz", SzSz[ss], N, N, ",\n"); file.Table("SmSp", SmSp[ss], N, N, ",\n"); file.Table("SpSm", SpSm[ss], N, N, ",\n"); file.Table("SS", SS[(size_t)s], N, N, ",\n");
            file.Table("StructureFactor", Sq[(size_t)s], Lx, Ly, ",\n"); file.Table("DD", DD[ss], nb, nb, s + 1 < k ? "},\n" : "}\n");
        }
        fprintf(fp, "   ]");
        if (cross) {
            fprintf(fp, ",\n   \"Cross\": [\n");
            for (PetscInt s = 0; s < k; ++s) for (PetscInt t = s + 1; t < k; ++t) {
                const size_t st = (size_t)(s * k + t);
                fprintf(fp, "   {\"s\": %lld, \"t\": %lld,\n", LLD(s), LLD(t));
                file.Table("SzSz", SzSz[st], N, N, ",\n"); file.Table("SmSp", SmSp[st], N, N, ",\n"); file.Table("SpSm", SpSm[st], N, N, ",\n");
                file.Table("DD", DD[st], nb, nb, (s == k - 2 && t == k - 1) ? "}\n" : "},\n");
            }
            fprintf(fp, "   ]");
        }
        fprintf(fp, "}");
        fflush(fp);
        return 0;
    }
};

/** The eleven measurements, the options they share, and the order in which a DMRG step reads and runs them. */
struct EngineMeasurements {
    CorrelationMatrix corr_matrix;
    DimerCorrelations corr_dimer;
    ChiralCorrelations corr_chiral;
    DynamicalStructureFactor dsf;
    DynamicalCorrelations dsf_sites;
    ChebyshevCorrelations dsf_cheb;
    DimerDynamics dsf_dimer;
    TransverseDynamics dsf_pm;
    CorrectionVectors dsf_cv;
    StaticSusceptibility chi;
    StateCorrelations states_corr;
    LanczosStepOptions lanczos;                 /* -dsf, -dsf_sites */
    ChebyshevOptions cheb;                      /* -dsf_cheb, -dsf_pm; its window also -dsf_dimer */

    /** Reads every option in a fixed order: of two mistakes on a command line, the one read first is the one refused.  (No option is read or
        refused by rank; the argument stands for the caller's triple of communicator, rank and size.) */
    template<class Hamiltonian> PetscErrorCode ReadOptions(MPI_Comm comm, PetscMPIInt /* rank */, PetscMPIInt size, PetscInt num_sites, const Hamiltonian& Ham)
    {
        PetscErrorCode ierr;
        ierr = corr_matrix.ReadOptions(); CHKERRQ(ierr);
        ierr = corr_dimer.ReadOptions(); CHKERRQ(ierr);
        ierr = corr_chiral.ReadOptions(comm, size); CHKERRQ(ierr);
        ierr = dsf.ReadOptions(comm, size, lanczos); CHKERRQ(ierr);
        ierr = dsf_sites.ReadOptions(comm, size, num_sites, lanczos); CHKERRQ(ierr);
        ierr = dsf_cheb.ReadOptions(comm, size, num_sites); CHKERRQ(ierr);
        ierr = dsf_dimer.ReadOptions(comm, size, (PetscInt)DimerBonds(Ham).size()); CHKERRQ(ierr);
        ierr = dsf_pm.ReadOptions(comm, size, num_sites); CHKERRQ(ierr);
        ierr = cheb.Read(comm, dsf_cheb.use, dsf_dimer.use, dsf_pm.use); CHKERRQ(ierr);
        ierr = dsf_cv.ReadOptions(comm, size, num_sites); CHKERRQ(ierr);
        ierr = chi.ReadOptions(comm, size, num_sites, (PetscInt)DimerBonds(Ham).size()); CHKERRQ(ierr);
        return states_corr.ReadOptions(comm);
    }
    /** Right after the eigensolve, while the plan of the superblock Hamiltonian exists. */
    template<class Hamiltonian> PetscErrorCode RunWithPlan(const MeasurementContext& ctx, const Hamiltonian& Ham)
    {
        PetscErrorCode ierr;
        if (dsf.use) { ierr = dsf.Run(ctx, Ham, lanczos); CHKERRQ(ierr); }
        if (dsf_sites.use) { ierr = dsf_sites.Run(ctx, Ham, lanczos); CHKERRQ(ierr); }
        if (dsf_cheb.use) { ierr = dsf_cheb.Run(ctx, Ham, cheb); CHKERRQ(ierr); }
        if (dsf_dimer.use) { ierr = dsf_dimer.Run(ctx, Ham, cheb); CHKERRQ(ierr); }
        if (dsf_cv.use) { ierr = dsf_cv.Run(ctx, Ham); CHKERRQ(ierr); }
        if (chi.use) { ierr = chi.Run(ctx, Ham); CHKERRQ(ierr); }
        return 0;
    }
    /** After that plan is destroyed: needs psi, not H -- its plans are of other sectors, one resident at a time. */
    template<class Hamiltonian> PetscErrorCode RunAfterPlan(const MeasurementContext& ctx, const Hamiltonian& Ham) { return dsf_pm.use ? dsf_pm.Run(ctx, Ham, cheb) : 0; }
    /** With the registered correlators, after the truncation. */
    template<class Hamiltonian> PetscErrorCode RunAtCentre(const MeasurementContext& ctx, const Hamiltonian& Ham)
    {
        PetscErrorCode ierr;
        if (corr_matrix.use) { ierr = corr_matrix.Run(ctx, Ham); CHKERRQ(ierr); }
        if (corr_dimer.use) { ierr = corr_dimer.Run(ctx, Ham); CHKERRQ(ierr); }
        if (corr_chiral.use) { ierr = corr_chiral.Run(ctx, Ham); CHKERRQ(ierr); }
        if (states_corr.use) { ierr = states_corr.Run(ctx, Ham); CHKERRQ(ierr); }
        return 0;
    }
    /** Every one of them reads Sz and Sp of every site of both centre blocks, on every rank. */
    bool NeedsAllSiteOperators() const { return corr_matrix.use || corr_dimer.use || corr_chiral.use || dsf.use || dsf_sites.use || dsf_cheb.use || dsf_cv.use || dsf_dimer.use || dsf_pm.use || chi.use || states_corr.use; }
    void Close() { corr_matrix.file.Close(); corr_dimer.file.Close(); corr_chiral.file.Close(); dsf.file.Close(); dsf_sites.file.Close(); dsf_cheb.file.Close(); dsf_cv.file.Close(); dsf_dimer.file.Close(); dsf_pm.file.Close(); chi.file.Close(); states_corr.file.Close(); }
};

}  // namespace dmrgx_host

#endif
