/** @file host_tool.cpp
    Line-oriented test harness over the engine's host classes (QuantumNumbers, Block::SpinBase, KronBlocks_t,
    KronEye_Explicit, Hamiltonians) -- everything here is index/metadata work on host-resident cells, so it runs
    without a GPU.  Used by tests/test_host_engine.py to replay the reference's known-answer tables
    (tests/UnitTests_DMRGKron.cpp, tests/UnitTests_DMRGBlock.cpp) against the C++ engine. */
#include <iostream>
#include <sstream>
#include <map>
#include "DMRGBlock.hpp"
#include "Hamiltonians.hpp"
#include "DMRGKron.hpp"
#include "CorrelatorDealing.hpp"
#include "TridiagQL.hpp"
#include "EngineMeasurements.hpp"
#include "Noise.hpp"
#include "TargetStates.hpp"
#include "SpinPenalty.hpp"

static void dump_mat(const char* tag, PetscInt site, const Mat& m)
{
    if (!m) { printf("op %s %lld null\n", tag, LLD(site)); return; }
    const PetscInt n = m->N();
    printf("op %s %lld %lld\n", tag, LLD(site), LLD(n));
    for (PetscInt r = 0; r < n; ++r) {
        const std::vector<double> row = m->dense_row(r);
        printf("row %lld", LLD(r));
        for (PetscInt c = 0; c < n; ++c) if (row[(size_t)c] != 0.0) printf(" %lld:%.17g", LLD(c), row[(size_t)c]);
        printf("\n");
    }
}

static void print_numbers(const char* tag, const std::vector<double>& v) { printf("%s", tag); for (double x : v) printf(" %.17g", x); printf("\n"); }

int main()
{
    std::map<std::string, Block::SpinBase> blocks;
    Hamiltonians::J1J2XXZModel_SquareLattice ham;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        if (!(is >> cmd) || cmd[0] == '#') continue;
        PetscErrorCode ierr = 0;
        if (cmd == "block") {
            std::string name; PetscInt nsites, nsec;
            is >> name >> nsites >> nsec;
            std::vector<PetscReal> qn((size_t)nsec); std::vector<PetscInt> sz((size_t)nsec);
            for (auto& q : qn) is >> q;
            for (auto& s : sz) is >> s;
            ierr = blocks[name].Initialize(PETSC_COMM_WORLD, nsites, qn, sz);
            printf("rc %d\n", ierr);
        } else if (cmd == "single") {
            std::string name; is >> name;
            ierr = blocks[name].Initialize(PETSC_COMM_WORLD, 1, PETSC_DEFAULT);
            printf("rc %d\n", ierr);
        } else if (cmd == "set") {
            std::string name, op; PetscInt site, row, col; double val;
            is >> name >> op >> site >> row >> col >> val;
            Mat m = (op == "Sz") ? blocks[name].Sz(site) : blocks[name].Sp(site);
            ierr = m->set(row, col, val);
            printf("rc %d\n", ierr);
        } else if (cmd == "copy") {              /* shallow copy: the new block shares the operator handles */
            std::string a, b; is >> a >> b;
            blocks[b] = blocks[a];
            printf("rc 0\n");
        } else if (cmd == "destroy") {
            std::string name; is >> name;
            ierr = blocks[name].Destroy();
            printf("rc %d\n", ierr);
        } else if (cmd == "nnz") {               /* number of stored cells of Sz(site) as seen through this block object */
            std::string name; PetscInt site; is >> name >> site;
            long n = -1;
            try { Mat m = blocks[name].Sz(site); n = m ? (long)m->cells.size() : -1; } catch (const std::exception&) { n = -2; }
            printf("nnz %ld\n", n);
        } else if (cmd == "save") {
            std::string name, dir; is >> name >> dir;
            ierr = blocks[name].SaveToDisk(dir);
            printf("rc %d\n", ierr);
        } else if (cmd == "load") {
            std::string name, dir; int with_sp_tot = 0; is >> name >> dir;
            if (!(is >> with_sp_tot)) with_sp_tot = 0;      /* load name dir 1: the carried total-spin operator too */
            ierr = blocks[name].InitializeFromDisk(PETSC_COMM_WORLD, dir, with_sp_tot != 0);
            printf("rc %d\n", ierr);
        } else if (cmd == "check") {
            std::string name; is >> name;
            ierr = blocks[name].CheckOperatorBlocks();
            printf("rc %d\n", ierr);
        } else if (cmd == "kroneye") {
            std::string l, r, o; is >> l >> r >> o;
            ierr = KronEye_Explicit(blocks[l], blocks[r], {}, blocks[o]);
            printf("rc %d\n", ierr);
        } else if (cmd == "dump") {
            std::string name; is >> name;
            Block::SpinBase& b = blocks[name];
            printf("sectors %lld", LLD(b.Magnetization.NumSectors()));
            for (PetscReal q : b.Magnetization.List()) printf(" %.17g", q);
            for (PetscInt s : b.Magnetization.Sizes()) printf(" %lld", LLD(s));
            printf("\n");
            for (PetscInt i = 0; i < b.NumSites(); ++i) { dump_mat("Sz", i, b.Sz(i)); dump_mat("Sp", i, b.Sp(i)); }
            printf("end\n");
        } else if (cmd == "kronblocks") {
            std::string l, r; is >> l >> r;
            std::vector<PetscReal> qs; PetscReal q;
            while (is >> q) qs.push_back(q);
            KronBlocks_t kb(blocks[l], blocks[r], qs, NULL, 0);
            printf("kronblocks %lld %lld", LLD(kb.size()), LLD(kb.NumStates()));
            for (PetscInt k = 0; k < kb.size(); ++k) printf(" %lld,%lld,%lld,%lld", LLD(kb.LeftIdx(k)), LLD(kb.RightIdx(k)), LLD(kb.Sizes(k)), LLD(kb.Offsets(k)));
            printf("\n");
        } else if (cmd == "iterate") {           /* walk KronBlocksIterator over [istart, iend) of the (sector-filtered) KronBlocks */
            std::string l, r; PetscInt i0, i1; is >> l >> r >> i0 >> i1;
            std::vector<PetscReal> qs; PetscReal q;
            while (is >> q) qs.push_back(q);
            KronBlocks_t kb(blocks[l], blocks[r], qs, NULL, 0);
            if (i1 < 0) i1 = kb.NumStates();
            KronBlocksIterator it(kb, i0, i1);
            printf("iterate %lld %lld\n", LLD(it.IdxStart()), LLD(it.IdxEnd()));
            for (; it.Loop(); ++it)
                printf("it %lld %lld %lld %lld %lld %lld %lld %lld %lld %d %lld %lld %lld\n", LLD(it.Idx()), LLD(it.BlockIdx()), LLD(it.LocIdx()), LLD(it.BlockIdxLeft()),
                       LLD(it.BlockIdxRight()), LLD(it.LocIdxLeft()), LLD(it.LocIdxRight()), LLD(it.GlobalIdxLeft()), LLD(it.GlobalIdxRight()), (int)it.UpdatedBlock(),
                       LLD(it.Steps()), LLD(it.BlockStartIdx(0)), LLD(it.BlockSize(+1)));
            printf("end\n");
        } else if (cmd == "ham") {
            dmrgx_host::Options::Global().Clear();
            std::string k, v;
            while (is >> k >> v) dmrgx_host::Options::Global().Set(k[0] == '-' ? k.substr(1) : k, v == "_" ? "" : v);
            ham = Hamiltonians::J1J2XXZModel_SquareLattice();
            ierr = ham.SetFromOptions();
            printf("rc %d\n", ierr);
        } else if (cmd == "terms") {
            PetscInt n; is >> n;
            const std::vector<Hamiltonians::Term> T = ham.H(n < 0 ? PETSC_DEFAULT : n);
            printf("terms %zu", T.size());
            for (const auto& t : T) printf(" %.17g,%d,%lld,%d,%lld", t.a, (int)t.Iop, LLD(t.Isite), (int)t.Jop, LLD(t.Jsite));
            printf("\n");
        } else if (cmd == "snake") {
            PetscInt ns = ham.NumSites();
            printf("snake");
            for (PetscInt i = 0; i < ns; ++i) { PetscInt ix, jy; ham.To2D(i, ix, jy); printf(" %lld,%lld,%lld", LLD(ix), LLD(jy), LLD(ham.To1D(ix, jy))); }
            printf("\n");
        } else if (cmd == "qnrange") {
            std::string name; PetscInt blk, shift; is >> name >> blk >> shift;
            PetscInt s = 0, e = 0; PetscBool flg = PETSC_FALSE;
            ierr = blocks[name].Magnetization.OpBlockToGlobalRange(blk, shift, s, e, flg);
            printf("rc %d %lld %lld %d\n", ierr, LLD(s), LLD(e), (int)flg);
        } else if (cmd == "deal") {              /* deal N W ncorr, then per correlator: k site_1 .. site_k  ->  owners and carried weights */
            int64_t N; int W; size_t nc;
            is >> N >> W >> nc;
            std::vector<std::vector<int64_t>> sites(nc);
            for (auto& v : sites) { size_t k; is >> k; v.resize(k); for (auto& x : v) is >> x; }
            std::vector<double> carried;
            const std::vector<int> owner = dmrgx_host::DealCorrelators(sites, N, W, &carried);
            printf("owners");
            for (int o : owner) printf(" %d", o);
            printf("\n");
            print_numbers("carried", carried);
        } else if (cmd == "tridiag") {           /* tridiag n d_0 .. d_{n-1} e_0 .. e_{n-2}  ->  eigenvalues and first eigenvector components */
            size_t n; is >> n;
            std::vector<double> d(n), e(n ? n - 1 : 0), z;
            for (double& x : d) is >> x;
            for (double& x : e) is >> x;
            const bool ok = dmrgx_host::TridiagQLFirstRow(d, e, z);
            printf("tridiag %d", (int)ok);
            for (size_t i = 0; i < n; ++i) printf(" %.17g,%.17g", d[i], z[i]);
            printf("\n");
        } else if (cmd == "tridiagvec") {        /* tridiagvec n d_0 .. d_{n-1} e_0 .. e_{n-2}  ->  one line per eigenvalue: the eigenvalue, then its eigenvector */
            size_t n; is >> n;
            std::vector<double> d(n), e(n ? n - 1 : 0), vec;
            for (double& x : d) is >> x;
            for (double& x : e) is >> x;
            const bool ok = dmrgx_host::TridiagQLVectors(d, e, vec);
            printf("tridiagvec %d %zu\n", (int)ok, n);
            for (size_t k = 0; k < n; ++k) {
                printf("eig %.17g", d[k]);
                for (size_t i = 0; i < n; ++i) printf(" %.17g", vec[k * n + i]);
                printf("\n");
            }
        } else if (cmd == "dsfcoef") {           /* dsfcoef Lx Ly nx ny  ->  cosine,sine coefficient of O_q (without 1/sqrt N) at every site, in the order of ham.To2D */
            PetscInt Lx, Ly, nx, ny; is >> Lx >> Ly >> nx >> ny;
            const PetscInt M = Lx * Ly;
            printf("dsfcoef");
            for (PetscInt i = 0; i < M; ++i) {
                PetscInt x, y; ham.To2D(i, x, y);
                const PetscInt p = (((nx * x * Ly + ny * y * Lx) % M) + M) % M;
                printf(" %.17g,%.17g", dmrgx_host::DsfPhaseCoefficient(0, p, M), dmrgx_host::DsfPhaseCoefficient(1, p, M));
            }
            printf("\n");
        } else if (cmd == "bonds") {             /* the nearest-neighbour bonds of ham: i,j,orientation,ix,jy */
            printf("bonds");
            for (const dmrgx_host::DimerBond& b : dmrgx_host::DimerBonds(ham)) printf(" %lld,%lld,%c,%lld,%lld", LLD(b.i), LLD(b.j), b.orient, LLD(b.ix), LLD(b.jy));
            printf("\n");
        } else if (cmd == "bondsof") {           /* bondsof x|y: the bonds of ham of that orientation: index,ix,jy */
            std::string o; is >> o;
            const dmrgx_host::OrientedBonds O = dmrgx_host::BondsOfOrientation(dmrgx_host::DimerBonds(ham), o.empty() ? '?' : o[0]);
            printf("bondsof %zu", O.of.size());
            for (size_t k = 0; k < O.of.size(); ++k) printf(" %lld,%lld,%lld", LLD(O.of[k]), LLD(O.x[k]), LLD(O.y[k]));
            printf("\n");
        } else if (cmd == "plaquettes") {        /* the plaquettes of ham: a,b,c,d,x,y */
            printf("plaquettes");
            for (const dmrgx_host::ChiralPlaquette& p : dmrgx_host::ChiralPlaquettes(ham)) printf(" %lld,%lld,%lld,%lld,%lld,%lld", LLD(p.s[0]), LLD(p.s[1]), LLD(p.s[2]), LLD(p.s[3]), LLD(p.x), LLD(p.y));
            printf("\n");
        } else if (cmd == "triangles") {         /* the triangles of ham's plaquettes: i,j,k,kind,plaquette,x,y */
            printf("triangles");
            for (const dmrgx_host::ChiralTriangle& t : dmrgx_host::ChiralTriangles(dmrgx_host::ChiralPlaquettes(ham))) printf(" %lld,%lld,%lld,%d,%lld,%lld,%lld", LLD(t.i), LLD(t.j), LLD(t.k), t.kind, LLD(t.plaq), LLD(t.x), LLD(t.y));
            printf("\n");
        } else if (cmd == "chiralsplit") {       /* chiralsplit i j k n_left N  ->  per string of K_ijk: coefficient | left part | right part, a part as op:blocksite,... or - */
            PetscInt i, j, k, nl, N; is >> i >> j >> k >> nl >> N;
            printf("chiralsplit");
            for (const dmrgx_host::ChiralString& S : dmrgx_host::ChiralStrings(i, j, k)) {
                printf(" %.17g", S.coeff);
                for (int side = 0; side < 2; ++side) {
                    const dmrgx_host::ChiralPart part = dmrgx_host::ChiralStringPart(S, side, nl, N);
                    printf("|");
                    if (part.empty()) printf("-");
                    for (size_t f = 0; f < part.size(); ++f) printf("%s%d:%lld", f ? "," : "", part[f].first, LLD(part[f].second));
                }
            }
            printf("\n");
        } else if (cmd == "fourier" || cmd == "cossum") {
            /* fourier Lx Ly n x_0 .. x_{n-1} y_0 .. y_{n-1} T_00 .. T_{n-1,n-1} [norm]  ->  the Lx x Ly table of LatticeFourier, norm n unless given
               cossum Lx Ly n c ncol x_0 .. x_{n-1} y_0 .. y_{n-1} T_00 .. T_{n-1,ncol-1}  ->  the (Lx Ly) x ncol table of SiteCosineSum, row by row */
            PetscInt Lx, Ly, n, c = -1, ncol; is >> Lx >> Ly >> n;
            if (cmd == "cossum") is >> c >> ncol; else ncol = n;
            std::vector<PetscInt> x((size_t)n), y((size_t)n);
            std::vector<double> T((size_t)(n * ncol));
            for (PetscInt& v : x) is >> v;
            for (PetscInt& v : y) is >> v;
            for (double& v : T) is >> v;
            double norm;
            if (!(is >> norm)) norm = (double)n;
            print_numbers(cmd.c_str(), c < 0 ? dmrgx_host::LatticeFourier(Lx, Ly, x.data(), y.data(), T.data(), n, norm) : dmrgx_host::SiteCosineSum(Lx, Ly, x.data(), y.data(), c, T.data(), n, ncol));
        } else if (cmd == "transweight") {       /* transweight Lx Ly n x_0 .. x_{n-1} y_0 .. y_{n-1} T_0 .. T_{n-1}  ->  the Lx x Ly table of TransitionWeight */
            PetscInt Lx, Ly, n; is >> Lx >> Ly >> n;
            std::vector<PetscInt> x((size_t)n), y((size_t)n);
            std::vector<double> T((size_t)n);
            for (PetscInt& v : x) is >> v;
            for (PetscInt& v : y) is >> v;
            for (double& v : T) is >> v;
            print_numbers(cmd.c_str(), dmrgx_host::TransitionWeight(Lx, Ly, x.data(), y.data(), T.data(), n));
        } else if (cmd == "omegagrid") {         /* omegagrid w0 w1 nw  ->  1 and the grid, or 0 */
            std::vector<double> om, grid;
            for (double v; is >> v;) om.push_back(v);
            const bool ok = dmrgx_host::OmegaGrid(om.data(), (PetscInt)om.size(), grid);
            print_numbers(ok ? "omegagrid 1" : "omegagrid 0", grid);
        } else if (cmd == "chebwindow" || cmd == "chebwindow2") {
            /* chebwindow E0 nsteps done alpha_0 .. alpha_{nsteps-1} beta_0 .. beta_{nsteps-1}  ->  ok centre half_width theta_max residual
               chebwindow2 nsteps done alpha_0 .. alpha_{nsteps-1} beta_0 .. beta_{nsteps-1}  ->  ok centre half_width theta_min theta_max res_min res_max */
            double E0 = 0.0; size_t nsteps; PetscInt done;
            if (cmd == "chebwindow") is >> E0;
            is >> nsteps >> done;
            std::vector<double> a(nsteps), b(nsteps);
            for (double& x : a) is >> x;
            for (double& x : b) is >> x;
            const dmrgx_host::ChebyshevSpectralWindow W = cmd == "chebwindow" ? dmrgx_host::ChebyshevWindow(E0, a, b, done) : dmrgx_host::ChebyshevWindowTwoSided(a, b, done);
            if (cmd == "chebwindow") printf("chebwindow %d %.17g %.17g %.17g %.17g\n", (int)W.ok, W.centre, W.half_width, W.theta_max, W.residual);
            else printf("chebwindow2 %d %.17g %.17g %.17g %.17g %.17g %.17g\n", (int)W.ok, W.centre, W.half_width, W.theta_min, W.theta_max, W.residual_min, W.residual);
        } else if (cmd == "chebjackson") {      /* chebjackson M nx mu_0 .. mu_{M-1} x_0 .. x_{nx-1}  ->  the damped sum at every x */
            PetscInt M, nx; is >> M >> nx;
            std::vector<double> mu((size_t)M), xs((size_t)nx);
            for (double& v : mu) is >> v;
            for (double& v : xs) is >> v;
            printf("chebjackson");
            for (double x : xs) printf(" %.17g", dmrgx_host::ChebyshevJackson(mu.data(), M, x));
            printf("\n");
        } else if (cmd == "chebmoments") {       /* chebmoments count K done norm diag_0 .. diag_{2K} cross_0 .. cross_{(K+1) count - 1}  ->  two lines: diag, mom of ScaleMoments */
            PetscInt count, K; dmrgx_host::MomentRun R; double norm; is >> count >> K >> R.done >> norm;
            std::vector<double> cross((size_t)((K + 1) * count));
            R.diag.resize((size_t)(2 * K + 1));
            for (double& v : R.diag) is >> v;
            for (double& v : cross) is >> v;
            dmrgx_host::ScaleMoments(R, cross, count, norm);
            print_numbers("diag", R.diag); print_numbers("mom", R.mom);
        } else if (cmd == "chebgrid") {          /* chebgrid M nm nw E0 centre half_width momq_00 .. momq_{M-1,nm-1} omega_0 .. omega_{nw-1}  ->  the M x nw grid of ChebyshevGrid, row by row */
            PetscInt M, nm, nw; double E0, centre, half_width; is >> M >> nm >> nw >> E0 >> centre >> half_width;
            std::vector<double> momq((size_t)(M * nm)), omega((size_t)nw);
            for (double& v : momq) is >> v;
            for (double& v : omega) is >> v;
            print_numbers("chebgrid", dmrgx_host::ChebyshevGrid(momq, nm, omega, E0, centre, half_width));
        } else if (cmd == "momentrec") {         /* momentrec path have_omega nsites: one dynamical record (%.17g) whose entry s is a run of s + 1 steps over 2 rows and 2 q of thirds, then Close() */
            std::string path; int have_omega; PetscInt nsites; is >> path >> have_omega >> nsites;
            dmrgx_host::JsonRecordFile J("%.17g");
            const std::vector<double> grid_omega{1.0 / 3.0, 2.0 / 3.0}, *omega = have_omega ? &grid_omega : nullptr;
            ierr = J.BeginDynamical(path, 7, "Sweep", -1.0 / 3.0, 2.0 / 3.0);
            if (!ierr) { fprintf(J.fp, ",\n"); J.Omega(omega); fprintf(J.fp, "   \"Sites\": [\n"); }
            for (PetscInt s = 0; s < nsites && !ierr; ++s) {
                dmrgx_host::MomentRun R;
                R.c = s; R.done = (int32_t)(s + 1); R.norm2 = (double)(s + 1) / 3.0;
                auto thirds = [s](PetscInt cnt, PetscInt from) { std::vector<double> v; for (PetscInt i = 0; i < cnt; ++i) v.push_back((double)(from + s + i) / 3.0); return v; };
                R.diag = thirds(2 * R.done + 1, 0); R.mom = thirds(2 * (R.done + 1), 10); R.momq = thirds(2 * (R.done + 1), 20); R.grid = thirds(2 * 2, 30);
                J.OpenSite(R.c, s, 0, R.norm2);
                fprintf(J.fp, ", \"StepsDone\": %d", (int)R.done);
                J.Moments(R, 2, 2, omega, s + 1 < nsites ? "},\n" : "}\n");
            }
            if (!ierr) fprintf(J.fp, "   ]}");
            J.Close();
            printf("rc %d\n", ierr);
        } else if (cmd == "jsonrec") {          /* jsonrec path format nrec: nrec records {"K": k, "R": row of 3, "T": 2 x 3 table} of thirds, then Close() */
            std::string path, fmt; PetscInt nrec; is >> path >> fmt >> nrec;
            dmrgx_host::JsonRecordFile J(fmt.c_str());
            for (PetscInt k = 0; k < nrec && !ierr; ++k) {
                std::vector<double> T;
                for (int i = 0; i < 6; ++i) T.push_back((double)(k * 6 + i) / 3.0);
                ierr = J.Begin(path);
                if (ierr) break;
                fprintf(J.fp, "  {\"K\": %lld,\n   \"R\": ", LLD(k));
                J.Row(T.data() + 1, 3);
                fprintf(J.fp, ",\n");
                J.Table("T", T, 2, 3, "}");
            }
            J.Close();
            printf("rc %d\n", ierr);
        } else if (cmd == "noise") {            /* noise <-noise value or "none"> <-noise_warmup value or "none"> nsweeps  ->  rc, then the warm-up's weight and that of every sweep, then the JSON */
            std::string sched, warm; PetscInt nsweeps; is >> sched >> warm >> nsweeps;
            dmrgx_host::Options::Global().Clear();
            if (sched != "none") PetscOptionsSetValue(NULL, "-noise", sched == "empty" ? "" : sched.c_str());
            if (warm != "none") PetscOptionsSetValue(NULL, "-noise_warmup", warm.c_str());
            dmrgx_host::NoiseSchedule S;
            ierr = dmrgx_host::ReadNoiseOptions(PETSC_COMM_WORLD, S);
            printf("rc %d\n", ierr);
            if (!ierr) {
                std::vector<double> v{S.At(true, 0)};
                for (PetscInt s = 0; s < nsweeps; ++s) v.push_back(S.At(false, s));
                print_numbers("noise", v);
                printf("any %d json %s\n", (int)S.Any(), S.Json().c_str());
            }
        } else if (cmd == "spinpenalty") {      /* spinpenalty <-spin_penalty value or "none"> <-spin_penalty_warmup value or "none"> nsweeps ranks  ->  as "noise", read on that many ranks */
            std::string sched, warm; PetscInt nsweeps; PetscMPIInt ranks; is >> sched >> warm >> nsweeps >> ranks;
            dmrgx_host::Options::Global().Clear();
            if (sched != "none") PetscOptionsSetValue(NULL, "-spin_penalty", sched == "empty" ? "" : sched.c_str());
            if (warm != "none") PetscOptionsSetValue(NULL, "-spin_penalty_warmup", warm.c_str());
            dmrgx_host::SpinPenaltySchedule S;
            ierr = dmrgx_host::ReadSpinPenaltyOptions(PETSC_COMM_WORLD, ranks, S);
            printf("rc %d\n", ierr);
            if (!ierr) {
                std::vector<double> v{S.At(true, 0)};
                for (PetscInt s = 0; s < nsweeps; ++s) v.push_back(S.At(false, s));
                print_numbers("spinpenalty", v);
                printf("any %d json %s\n", (int)S.Any(), S.Json().c_str());
            }
        } else if (cmd == "sptot") {            /* sptot name: gives a one-site block its carried total-spin operator */
            std::string name; is >> name;
            ierr = blocks[name].CreateSpTot();
            printf("rc %d\n", ierr);
        } else if (cmd == "dumpsptot") {        /* dumpsptot name: the carried operator, as "dump" prints a site operator */
            std::string name; is >> name;
            dump_mat("SpTot", 0, blocks[name].SpTot);
            printf("end\n");
        } else if (cmd == "targets") {          /* targets <-nstates value or "none"> <-state_weights value or "none"> nstates_of_sector  ->  rc, then k, k_step and the step's normalised weights */
            std::string ns, sw; PetscInt in_sector; is >> ns >> sw >> in_sector;
            dmrgx_host::Options::Global().Clear();
            if (ns != "none") PetscOptionsSetValue(NULL, "-nstates", ns.c_str());
            if (sw != "none") PetscOptionsSetValue(NULL, "-state_weights", sw == "empty" ? "" : sw.c_str());
            dmrgx_host::TargetStates T;
            ierr = dmrgx_host::ReadTargetStatesOptions(PETSC_COMM_WORLD, T);
            printf("rc %d\n", ierr);
            if (!ierr) {
                const std::vector<double> w = T.StepWeights(in_sector);
                printf("k %lld k_step %lld\n", LLD(T.k), LLD((PetscInt)w.size()));
                print_numbers("weights", w);
                print_numbers("all", T.weights);
            }
        } else if (cmd == "measopts") {         /* measopts ranks -option value ...: the model and the measurement options as on the driver's command line ("_": no value)  ->  rc of EngineMeasurements::ReadOptions on that many ranks, then one line per measurement */
            PetscMPIInt ranks; is >> ranks;
            dmrgx_host::Options::Global().Clear();
            std::string k, v;
            while (is >> k >> v) PetscOptionsSetValue(NULL, k.c_str(), v == "_" ? "" : v.c_str());
            ham = Hamiltonians::J1J2XXZModel_SquareLattice();
            ierr = ham.SetFromOptions();
            dmrgx_host::EngineMeasurements E;
            if (!ierr) ierr = E.ReadOptions(PETSC_COMM_WORLD, 0, ranks, ham.NumSites(), ham);
            printf("rc %d\n", ierr);
            if (!ierr) {
                auto ints = [](const std::vector<PetscInt>& a) { std::string s; for (PetscInt x : a) s += (s.empty() ? "" : ",") + std::to_string(x); return s.empty() ? std::string("-") : s; };
                auto reals = [](const std::vector<double>* a) { std::string s; char b[32]; if (a) for (double x : *a) { snprintf(b, sizeof(b), "%.17g", x); s += (s.empty() ? "" : ",") + std::string(b); } return s.empty() ? std::string("-") : s; };
                const std::vector<double> window(E.cheb.window, E.cheb.window + 2);
                const std::string shared = " bound_steps " + std::to_string(E.cheb.bound_steps) + " window " + reals(E.cheb.have_window ? &window : nullptr);
                const std::string cheb = " steps " + std::to_string(E.cheb.steps) + " omega " + reals(E.cheb.grid()) + shared;
                printf("corr_matrix %d\ncorr_dimer %d\ncorr_chiral %d\n", (int)E.corr_matrix.use, (int)E.corr_dimer.use, (int)E.corr_chiral.use);
                printf("dsf %d q %s steps %lld breakdown_tol %.17g\n", (int)E.dsf.use, ints(E.dsf.q).c_str(), LLD(E.lanczos.steps), E.lanczos.breakdown_tol);
                printf("dsf_sites %d sites %s steps %lld breakdown_tol %.17g\n", (int)E.dsf_sites.use, ints(E.dsf_sites.sites).c_str(), LLD(E.lanczos.steps), E.lanczos.breakdown_tol);
                printf("dsf_cheb %d sites %s%s\n", (int)E.dsf_cheb.use, ints(E.dsf_cheb.sites).c_str(), cheb.c_str());
                printf("dsf_dimer %d bonds %s steps %lld omega %s%s\n", (int)E.dsf_dimer.use, ints(E.dsf_dimer.bonds).c_str(), LLD(E.dsf_dimer.steps), reals(E.dsf_dimer.have_omega ? &E.dsf_dimer.omega : nullptr).c_str(), shared.c_str());
                printf("dsf_pm %d sites %s%s\n", (int)E.dsf_pm.use, ints(E.dsf_pm.sites).c_str(), cheb.c_str());
                printf("dsf_cv %d sites %s omega %s eta %.17g tol %.17g maxit %lld\n", (int)E.dsf_cv.use, ints(E.dsf_cv.sites).c_str(), reals(&E.dsf_cv.omega).c_str(), E.dsf_cv.eta, E.dsf_cv.tol, LLD(E.dsf_cv.maxit));
                /* the tenth measurement prints its line when it is on: a run without its options lists the nine above, as before */
                if (E.chi.use) printf("chi 1 sites %s bonds %s tol %.17g maxit %lld\n", ints(E.chi.sites).c_str(), ints(E.chi.bonds).c_str(), E.chi.tol, LLD(E.chi.maxit));
                if (E.states_corr.use) printf("states_corr 1 cross %d\n", (int)E.states_corr.cross);      /* the eleventh: likewise */
            }
        } else if (cmd == "noiseops") {        /* noiseops a n, then n x (shift transposed id): plan operators, id names the stored cell set  ->  the list of NoiseOperators as shift:transposed:id, then the coefficient */
            double a; PetscInt n; is >> a >> n;
            std::vector<dmrgx_cell> sets(64);
            for (size_t i = 0; i < sets.size(); ++i) sets[i] = dmrgx_cell{0, 0, 0, 2, 2, DMRGX_CELL_DENSE, 0.0, reinterpret_cast<const double*>(sets.data()) + i % 32, 2};      /* (addresses never read; set 32 + i is a second descriptor of the blocks of set i) */
            std::vector<dmrgx_secop> plan_ops, ops;
            for (PetscInt i = 0; i < n; ++i) { PetscInt s, t, id; is >> s >> t >> id; plan_ops.push_back(dmrgx_secop{(int32_t)s, (int32_t)t, 1, &sets[(size_t)id]}); }
            std::vector<double> coef;
            dmrgx_host::NoiseOperators(plan_ops, a, ops, coef);
            printf("noiseops");
            for (const dmrgx_secop& o : ops) printf(" %d:%d:%d", o.shift, o.transposed, (int)(o.cells - sets.data()));
            printf("\ncoef %.17g %d\n", coef.empty() ? 0.0 : coef[0], (int)coef.size());
        } else printf("unknown %s\n", cmd.c_str());
        fflush(stdout);
    }
    return 0;
}
