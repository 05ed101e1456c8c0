/* dmrgx.h -- C ABI of the MI355X-native DMRG hot path (libdmrgx_hip.so).
 *
 * This is the drop-in boundary: the host sweep engine (C++, mirrors DMRGBlock / DMRGKron /
 * DMRGBlockContainer of jnvance/DMRG.x) reaches every device computation through these entry points and
 * nothing else.  Plain pointers and sizes only; no C++/torch types; every function returns a dmrgx_status
 * (0 = success), never throws, and records a message retrievable with dmrgx_last_error().
 *
 * What each entry point replaces in the reference (paths relative to the reference tree):
 *   dmrgx_kron_plan_create   <- KronBlocks_t::KronSumConstruct -> KronSumConstructShell
 *                               (src/DMRGKron.cpp:759-841, 1871-1917: term filtering is the caller's job,
 *                               operator fetch 891-989, per-row descriptors 1706-1824)
 *   dmrgx_kron_apply         <- MatMult_KronSumShell (src/DMRGKron.cpp:1827-1869), the MATOP_MULT callback
 *                               registered at src/DMRGKron.cpp:1912-1914
 *   dmrgx_kron_plan_destroy  <- MatDestroy_KronSumShell (src/DMRGKron.cpp:1919-1942)
 *   dmrgx_eigs_lowest        <- EPSSolve(EPS_HEP, EPS_SMALLEST_REAL, nev=1) as configured at
 *                               include/DMRGBlockContainer.hpp:1488-1499 [SLEPc Krylov-Schur, external]
 *   dmrgx_rdm_create         <- the device part of GetTruncation: rho_L, rho_R of every KronBlock and all their eigenpairs
 *   dmrgx_rdm_eigenvalues       (EigRDM_BlockDiag, include/DMRGBlockContainer.hpp:1715-1775, 1962-2003); the global sort and
 *   dmrgx_rdm_eigenvectors      the m-cut stay with the caller; _eigenvectors == FillRotation_BlockDiag (:2006-2057)
 *   dmrgx_rotate_ops         <- Block::SpinBase::RotateOperators (src/DMRGBlock.cpp:677-823)
 *   dmrgx_cells_axpy         <- the explicit KronSum that assembles an enlarged block's H (src/DMRGKron.cpp:612 ->
 *                               KronSumFillMatrix :1440-1446); the site operators of an enlarged block
 *                               (MatKronEyeConstruct, src/DMRGKron.cpp:52-456) are views and need no device call
 *   dmrgx_kron_op_gram       <- all two-site correlators of one kind at once: the per-correlator KronConstruct + MatMult + VecDot
 *   dmrgx_vec_gram              of include/DMRGBlockContainer.hpp:2287-2293, as one Gram matrix of the operator images O_i psi
 *   dmrgx_kron_term_gram     <- the same for images that are sums of terms c A (x) B (bond operators S_i . S_j inside a block or across
 *                               the cut): the whole table < D_b D_b' > of dimer-dimer correlations as one Gram matrix
 *   dmrgx_kron_term_apply    <- nothing in the reference: engine extensions like the Gram calls.  The image vectors sum_t c_t (A_t (x) B_t) psi
 *   dmrgx_kron_lanczos_coeffs   themselves (the Gram calls only hand back their inner products) and the Lanczos coefficients of the planned
 *                               superblock Hamiltonian from such a vector: the continued fraction behind a dynamical structure factor
 *   dmrgx_kron_term_apply_to    the same images written in the layout of another total-Sz sector: S+_i psi as start vectors of that sector's plan (-dsf_pm)
 *   dmrgx_kron_lanczos_basis    (-dsf); the same run with the basis kept and reorthogonalised, for overlaps with it (-dsf_sites)
 *   dmrgx_kron_chebyshev_moments  the Chebyshev recursion on the planned Hamiltonian and its moments with a family of vectors (-dsf_cheb)
 *   dmrgx_kron_correction_vector  the correction vector 1 / (sigma + i eta - H) v0 by a device-resident conjugate-gradient run, and its
 *                               overlaps with a family of vectors: G_ic(w + i eta) under a true Lorentzian (-dsf_cv)
 *   dmrgx_kron_noise_expand     psi with the images of one block's operators beside it: White's density-matrix perturbation as a wider input
 *                               of dmrgx_rdm_create_subset (-noise)
 *   dmrgx_secop_compose         sums of products of two and three operators of one block, dense per sector: the parts of S_i . (S_j x S_k)
 *                               on one side of the cut (-corr_chiral)
 *   dmrgx_vec_project_out       one vector removed from a family of vectors, coefficients returned: (D_b - <D_b>) psi for all bonds (-dsf_dimer)
 *   dmrgx_kron_static_response  the static linear response sum_{n>0} |n><n|v0> / (E_n - E0) by a device-resident conjugate-gradient run on the
 *                               complement of psi, and its overlaps with a family of vectors: chi_ic = d<Sz_i>/dh_c, chi_bc (-chi_sites, -chi_bonds)
 *   dmrgx_eigs_lowest_orth      the lowest eigenpair on the complement of states already found, and dmrgx_kron_states_expand, those states
 *   dmrgx_kron_states_expand    side by side as the input of dmrgx_rdm_create_subset: the k lowest states of a sector under a
 *                               state-averaged density matrix (-nstates)
 *   dmrgx_comm_*             <- the communicator of the reference's MPI path: VecScatter-to-all of x inside every MatMult
 *                               (src/DMRGKron.cpp:1833-1834) and the MPI_Allreduce behind SLEPc's VecDot / VecNorm
 *
 * Data model.  All floating point is f64 real (include/DMRGKron.hpp:395-399).  A block's basis is split in
 * Sz sectors (descending Sz); an operator with sector shift s (Op_t value: Sm=-1, Sz=0, Sp=+1,
 * include/DMRGBlock.hpp:19-27) is non-zero only in blocks (row sector q -> column sector q+s).  On the device
 * an operator is a list of *cells*: dense row-major rectangles (or scaled identities) inside those blocks.
 * The superblock vector of the target sector is the concatenation over KronBlocks k=(IL,IR) of the row-major
 * n_L(IL) x n_R(IR) matrices X_k (include/DMRGKron.hpp:160-209, 603-612).
 *
 * Threading: a plan is used from one host thread at a time; all work is enqueued on the hipStream_t passed as
 * `void* stream` (NULL = default stream).  Device pointers must come from the current HIP device.
 */
#ifndef DMRGX_H
#define DMRGX_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMRGX_ABI_VERSION 3

typedef int32_t dmrgx_status;
enum {
    DMRGX_OK = 0,
    DMRGX_ERR_ARG = 62,          /* = PETSC_ERR_ARG_WRONG: malformed descriptor                     */
    DMRGX_ERR_OUTOFRANGE = 63,   /* = PETSC_ERR_ARG_OUTOFRANGE: index/sector out of range            */
    DMRGX_ERR_MEM = 55,          /* = PETSC_ERR_MEM                                                  */
    DMRGX_ERR_DEVICE = 97,       /* HIP runtime error / no device                                    */
    DMRGX_ERR_NOTCONV = 91,      /* eigensolver did not converge within max_it                       */
    DMRGX_ERR_INTERNAL = 77
};

/* ---- library ---------------------------------------------------------------------------------------- */
int32_t      dmrgx_abi_version(void);
const char*  dmrgx_last_error(void);                 /* thread-local, valid until the next failing call  */
dmrgx_status dmrgx_device_count(int32_t* n);         /* fails loudly (DMRGX_ERR_DEVICE) without a GPU     */

/* ---- communicator: one process per GPU, collectives over RCCL / xGMI ------------------------ */
/* Replaces the reference's MPI traffic on the hot path: the VecScatter-to-all of x inside every MatMult
 * (src/DMRGKron.cpp:1833-1834), the MPI_Allreduce behind SLEPc's VecDot / VecNorm, and the rank-0 RDM solve followed by
 * a broadcast of the rotation (include/DMRGBlockContainer.hpp:1673-1677, 1812-1925).  Every collective is enqueued on the
 * caller's stream and must be called by all ranks in the same order.
 *   launch: rank 0 calls dmrgx_comm_unique_id and hands the 128 bytes to the other ranks by any means (file, socket, the
 *   launcher's store); every rank then calls dmrgx_set_device(local rank) and dmrgx_comm_init.
 * The host-staged back-end (several ranks on ONE GPU exchanging through a POSIX shared-memory segment named by rank 0)
 * exists to rehearse the N > 1 control flow on a one-GPU box; it is not a measurement path. */
typedef struct dmrgx_comm dmrgx_comm;
#define DMRGX_COMM_ID_BYTES 128
enum { DMRGX_COMM_RCCL = 1, DMRGX_COMM_HOST_STAGED = 2 };
dmrgx_status dmrgx_set_device(int32_t device);
dmrgx_status dmrgx_comm_unique_id(uint8_t* id128);
dmrgx_status dmrgx_comm_init(int32_t rank, int32_t world, const uint8_t* id128, dmrgx_comm** out);
dmrgx_status dmrgx_comm_init_host_staged(int32_t rank, int32_t world, const char* shm_name, dmrgx_comm** out);
dmrgx_status dmrgx_comm_info(const dmrgx_comm* comm, int32_t* rank, int32_t* world, int32_t* backend);
/* in place: segment r of full_vec (seg_stride doubles, this rank's = the send buffer) is replicated on every rank */
dmrgx_status dmrgx_comm_allgather(dmrgx_comm* comm, double* full_vec_dev, int64_t seg_stride, void* stream);
dmrgx_status dmrgx_comm_allreduce_sum(dmrgx_comm* comm, double* buf_dev, int64_t count, void* stream);
dmrgx_status dmrgx_comm_bcast(dmrgx_comm* comm, void* buf_dev, size_t bytes, int32_t root, void* stream);
/* host payloads (spectra, counters): recv = concatenation over ranks of bytes_per_rank bytes; synchronises the stream */
dmrgx_status dmrgx_comm_allgather_host(dmrgx_comm* comm, const void* send, void* recv, size_t bytes_per_rank, void* stream);
dmrgx_status dmrgx_comm_barrier(dmrgx_comm* comm, void* stream);      /* all ranks have finished the work queued on `stream` */
dmrgx_status dmrgx_comm_destroy(dmrgx_comm* comm);

/* ---- operator cells --------------------------------------------------------------------------------- */
enum { DMRGX_CELL_DENSE = 1, DMRGX_CELL_IDENT = 2 };

typedef struct {
    int32_t row_sector;   /* q: row sector of the (q -> q+shift) block this cell lives in               */
    int32_t r0, c0;       /* top-left corner inside that block                                          */
    int32_t nr, nc;       /* extent (IDENT: nr == nc)                                                   */
    int32_t kind;         /* DMRGX_CELL_DENSE | DMRGX_CELL_IDENT                                        */
    double  scale;        /* IDENT: the cell equals scale * I.  DENSE: ignored                          */
    const double* data;   /* DENSE: device pointer to element (r0,c0); row-major, leading dimension ld */
    int64_t ld;
} dmrgx_cell;

/* One operator of one block.  `transposed` != 0 means the operator is the transpose of the stored cells
 * (Sm(i) = Sp(i)^T, src/DMRGBlock.cpp:630-632): the cells then describe the stored operator (whose shift is
 * -shift) and are read transposed -- no Sm is ever materialised. */
typedef struct {
    int32_t shift;        /* sector shift of the operator AS USED (after the optional transpose)        */
    int32_t transposed;
    int32_t ncells;
    const dmrgx_cell* cells;   /* host array */
} dmrgx_secop;

/* Sector table of one (enlarged) block: sizes of the Sz sectors in descending-Sz order. */
typedef struct {
    int32_t nsec;
    const int32_t* size;  /* host array [nsec] */
} dmrgx_sectors;

/* ---- K1: superblock plan ---------------------------------------------------------------------------- */
/* One inter-block term a * A(left op) (x) B(right op)  (Hamiltonians::Term after the filtering/reflection of
 * src/DMRGKron.cpp:788-807).  left_op / right_op index into desc->left_ops / desc->right_ops. */
typedef struct {
    double  a;
    int32_t left_op;
    int32_t right_op;
} dmrgx_term;

typedef struct {
    dmrgx_sectors left, right;
    int32_t nblocks;               /* KronBlocks of the target sector, in the reference's order        */
    const int32_t* block_il;       /* [nblocks] left sector index  (include/DMRGKron.hpp:160-171)      */
    const int32_t* block_ir;       /* [nblocks] right sector index                                     */
    int32_t n_left_ops, n_right_ops;
    const dmrgx_secop* left_ops;   /* distinct (op,site) operators of the left block used by terms     */
    const dmrgx_secop* right_ops;
    const dmrgx_secop* h_left;     /* H_L (shift 0), term [H_L (x) 1]  (src/DMRGKron.cpp:939-944); may be NULL */
    const dmrgx_secop* h_right;    /* H_R (shift 0), term [1 (x) H_R]  (src/DMRGKron.cpp:946-951); may be NULL */
    int32_t nterms;
    const dmrgx_term* terms;
    /* striping of the right index over ranks; world_size == 1 -> plain layout */
    int32_t world_size, rank;
} dmrgx_kron_desc;

typedef struct dmrgx_kron_plan dmrgx_kron_plan;

typedef struct {
    int64_t n_states;          /* N_sb = sum_k n_L n_R                                                  */
    int64_t vec_len;           /* length of a full device vector (== n_states when world_size == 1)     */
    int64_t local_offset;      /* this rank's segment inside a full vector                              */
    int64_t local_len;         /* length of this rank's segment (incl. padding)                         */
    int64_t seg_stride;        /* stride between rank segments                                          */
    double  flops_alg;         /* algorithmic flops of ONE apply on THIS rank (SURVEY 8d F_alg)         */
    double  bytes_alg;         /* algorithmic bytes of ONE apply on THIS rank (SURVEY 8d B_alg)         */
    double  flops_exec;        /* flops the tiled kernels actually issue (padding included)             */
    double  bytes_workspace;   /* bytes of intermediates written+read per apply (not part of B_alg)     */
    int32_t n_groups;          /* merged (A,B) operator pairs                                           */
    int32_t n_tiles_stage1, n_tiles_stage2;
    int32_t n_tiles_big;       /* of those, 128x128 macro tiles: 0, the MatMult runs 64x64 tiles only     */
    double  flops_alg_big;     /* part of flops_alg executed by the 128x128 kernel: 0                     */
} dmrgx_kron_info;

dmrgx_status dmrgx_kron_plan_create(const dmrgx_kron_desc* desc, void* stream, dmrgx_kron_plan** out);
dmrgx_status dmrgx_kron_plan_info(const dmrgx_kron_plan* plan, dmrgx_kron_info* info);
/* y_local <- (H x)[this rank's segment].  x_full: full vector (vec_len), y_local: points at the start of this
 * rank's segment of a full vector or at a separate buffer of local_len doubles.  world_size==1: y = H x. */
dmrgx_status dmrgx_kron_apply(dmrgx_kron_plan* plan, const double* x_full, double* y_local, void* stream);
dmrgx_status dmrgx_kron_plan_destroy(dmrgx_kron_plan* plan);
/* d_local[e] <- <e| H |e> for the basis states of this rank's segment (local_len doubles, padding 0): the diagonal of the
 * superblock Hamiltonian, = sum over H_L (x) 1, 1 (x) H_R and the sector-diagonal terms (Sz Sz) of diag(A)[l] diag(B)[r]
 * -- what a diagonally preconditioned eigensolver (SLEPc: -H_eps_type gd, -H_st_pc_type jacobi) asks MatGetDiagonal for; the
 * reference's shell matrix does not implement it (src/DMRGKron.cpp:1912-1914 registers MATOP_MULT only). */
dmrgx_status dmrgx_kron_diag(dmrgx_kron_plan* plan, double* d_local_dev, void* stream);
/* Optional per-launch timing of the two GEMM stages with HIP events recorded on the apply's own stream
 * (the reference's analogue is the -DDMRG_KRON_TIMINGS accumulators, include/MiscTools.hpp:17-59).
 * enable != 0 resets and starts recording (up to 4096 applies), enable == 0 stops. */
dmrgx_status dmrgx_kron_plan_timing(dmrgx_kron_plan* plan, int32_t enable);
/* Synchronises the recorded events (three per apply: before stage 1, between the stages, after stage 2) and returns the
 * summed kernel time in milliseconds of the two GEMM launches of an apply: ms[1] stage 1, ms[3] stage 2.  ms[0] and ms[2]
 * are the slots of 128x128 launches, which the MatMult does not make: always 0. */
dmrgx_status dmrgx_kron_plan_timing_read(dmrgx_kron_plan* plan, double* ms4, int64_t* n_applies);
/* Convert between the reference's vector layout (KronBlocks order, n_states doubles, host or device) and the
 * striped full-vector layout (identity copy when world_size == 1). */
dmrgx_status dmrgx_kron_vec_to_striped(const dmrgx_kron_plan* plan, const double* v_ref_dev, double* v_full_dev, void* stream);
dmrgx_status dmrgx_kron_vec_from_striped(const dmrgx_kron_plan* plan, const double* v_full_dev, double* v_ref_dev, void* stream);

/* Host-only helper (no device needed): columns [*c0, *c1) are stripe number `rank` of a KronBlock whose right sector has n_right
 * states cut for `world_size` ranks -- the cut rule used by every plan (cuts on whole GEMM tiles where possible). */
dmrgx_status dmrgx_stripe_bounds(int32_t n_right, int32_t world_size, int32_t rank, int32_t* c0, int32_t* c1);
/* The columns rank `rank` owns in the KronBlock number `block` (position in desc->block_il/ir): stripe (rank + block) mod world_size
 * of dmrgx_stripe_bounds -- the stripes are dealt round the ranks block by block so that the ragged last stripe moves around. */
dmrgx_status dmrgx_stripe_bounds_of_block(int32_t n_right, int32_t world_size, int32_t rank, int32_t block, int32_t* c0, int32_t* c1);

/* ---- generic grouped f64 GEMM (used by K1/K3/K6; exposed for tests) ---------------------------------- */
/* C[M x N] (row-major, ldc) = A[M x K] (row-major, lda) * B[K x N] (row-major, ldb), device pointers. */
dmrgx_status dmrgx_dgemm_nn(int32_t M, int32_t N, int32_t K, const double* A, int64_t lda,
                            const double* B, int64_t ldb, double* C, int64_t ldc, void* stream);
/* The same for `count` independent products in one grouped launch (operator products per sector block, correlators:
 * the MatMatMult calls of include/DMRGBlockContainer.hpp:2378-2395).  accumulate != 0: C += A*B.  Outputs must not
 * overlap.  Both GEMM entry points are asynchronous on `stream` (the task array itself is consumed before returning). */
typedef struct {
    int32_t M, N, K, accumulate;
    const double* A; int64_t lda;
    const double* B; int64_t ldb;
    double* C; int64_t ldc;
} dmrgx_gemm_task;
dmrgx_status dmrgx_dgemm_batch(int32_t count, const dmrgx_gemm_task* tasks, void* stream);
/* Whole groups of the grouped GEMM, as the MatMult, the density matrices and the rotations build them (tests/test_gpu_ggemm.py):
 *   C[M x N] (=|+=) sum over the GEMM products A[M x K] * B[K x N]  +  sum over the scaled copies alpha * S[M x N]
 * in ONE launch per tile size.  kind 0: GEMM product (a product with K == 0 adds nothing); kind 1: scaled copy, `B` is the source S
 * and `ldb` its leading dimension, A / lda / K are ignored.  A group without products writes C = 0 (or leaves C, accumulating);
 * groups with M == 0 or N == 0 are skipped.  Outputs must not overlap.  tiling 0: 128 x 128 cores and 64 x 64 edges (what every
 * library user gets), 1: 64 x 64 tiles only (as the MatMult tiles).  report (may be NULL): the tiles of the launch, the lengths of
 * the scheduled lists handed to the kernels (padded per XCD queue) and the resident workgroup slots they were scheduled for --
 * a list longer than its slots is worked off by claiming.  Asynchronous on `stream`; the tables are consumed before returning. */
typedef struct {
    int32_t kind, K;
    const double* A; int64_t lda;
    const double* B; int64_t ldb;
    double alpha;
} dmrgx_ggemm_prod;
typedef struct {
    double* C; int64_t ldc;
    int32_t M, N, accumulate, nprods;
    const dmrgx_ggemm_prod* prods;
} dmrgx_ggemm_group;
typedef struct {
    int32_t tiles_big, tiles_small;         /* real tiles: 128 x 128, 64 x 64           */
    int32_t entries_big, entries_small;     /* list lengths handed to the kernels       */
    int32_t slots_big, slots_small;         /* resident workgroups of a full launch     */
} dmrgx_ggemm_report;
dmrgx_status dmrgx_ggemm_groups(int32_t count, const dmrgx_ggemm_group* groups, int32_t tiling, dmrgx_ggemm_report* report, void* stream);

/* ---- K2: lowest eigenpair of the planned superblock Hamiltonian -------------------------------------- */
typedef struct {
    int32_t ncv;        /* Krylov subspace size (0: SLEPc's default for nev=1, 16).  Method 0 uses at most 64 vectors and at
                           least 2 (a one-vector space cannot restart: ncv = 1 is taken as 2), never more than n_states */
    int32_t max_it;     /* maximum number of restarts                                                    */
    double  tol;        /* converged when ||r|| <= tol * |theta|  (SLEPc default criterion, default 1e-8) */
    uint64_t seed;      /* start vector: counter-based uniform(-1,1) stream of this seed, unless ...      */
    int32_t use_initial; /* ... use_initial != 0: psi_full holds the start vector                         */
    int32_t max_matvec;  /* > 0: stop after exactly this many MatMults (status DMRGX_ERR_NOTCONV unless converged
                            earlier); used by benchmarks to time a fixed number of Lanczos steps               */
    /* collective hooks for world_size > 1 (NULL when world_size == 1).  They must be stream-ordered on
     * `stream`: allgather(sendbuf=this rank's segment, full vector) and allreduce_sum(buf, count). */
    dmrgx_status (*allgather)(void* user, double* full_vec, int64_t seg_stride, void* stream);
    dmrgx_status (*allreduce_sum)(void* user, double* buf, int64_t count, void* stream);
    void* user;
    /* native collectives: when `comm` is set (and the hooks are NULL) the solver calls dmrgx_comm_allgather /
     * dmrgx_comm_allreduce_sum itself -- the product path; the hooks remain for harnesses that own their communicator */
    dmrgx_comm* comm;
    /* 0: thick-restart Lanczos (SLEPc's default for this solve, -H_eps_type krylovschur).  1: generalized Davidson with the
     * diagonal of H_sb as preconditioner (-H_eps_type gd with a Jacobi preconditioner): same convergence criterion (true
     * residual), about a quarter fewer MatMults from the engine's transformed start vectors; the projected problem is
     * solved on the device, the host only looks at (|r|, theta) one iteration behind the queue.  Applies when use_initial is set; from a random start the Lanczos
     * path is used (the preconditioned iteration is twice as slow there). */
    int32_t method;
    /* > 0 (with use_initial): the start vector is only trusted if its squared norm is at least this -- the engine's start vectors are
     * projections of a normalised state, so their norm says how much of it survived.  A lighter vector is dropped and the solve runs
     * from the random start vector (stats->start_rejected = 1).  The norm is read with the first coefficients that come back to the
     * host anyway: no extra synchronisation.  0: no check beyond "not zero / NaN". */
    double min_initial_norm2;
    /* method 1: number of lowest Ritz vectors the search space is restarted to, beside the previous iteration's Ritz vector (SLEPc:
     * -eps_gd_minv with -eps_gd_plusk 1).  0: the default, 1.  The search space itself holds `ncv` vectors (0: the default of the
     * method -- 16 for method 0, 8 for method 1). */
    int32_t gd_minv;
    int32_t reserved_;
} dmrgx_eigs_opts;

typedef struct {
    int32_t n_matvec;       /* number of dmrgx_kron_apply calls ("superblock MatMults")                  */
    int32_t n_restart;
    int32_t converged;
    int32_t start_rejected; /* 1: the supplied start vector was dropped (zero / NaN norm, or below min_initial_norm2)  */
    double  residual;       /* final ||H psi - e0 psi||                                                  */
    double  seconds;        /* wall time of the solve (host clock around a stream sync)                  */
} dmrgx_eigs_stats;

dmrgx_status dmrgx_eigs_lowest(dmrgx_kron_plan* plan, const dmrgx_eigs_opts* opts, double* e0,
                               double* psi_full, dmrgx_eigs_stats* stats, void* stream);
/* The lowest eigenpair of P H P on the complement of span(Q), P = 1 - Qt Qt^T: the excited states of one sector, found one after another,
 * each call with the states already found as Q (-nstates).  That resolves exact degeneracies, which a single Krylov sequence cannot.
 * Q_dev: nq rows of n_states doubles, ldq >= n_states, any 8-byte alignment, only read.  The call orthonormalises a private, 16-byte
 * aligned copy Qt of it (CGS2 row by row, in row order).  psi_dev: n_states doubles; with opts->use_initial it holds the start vector,
 * which is projected against Qt first; the run starts from the projected random vector instead (stats->start_rejected = 1) when the
 * projected squared norm is not finite and positive or lies below max(min_initial_norm2, 1e-20 times the unprojected squared norm).
 * nq == 0 forwards to dmrgx_eigs_lowest with the same options: the same bits in e, psi and stats.
 * Read from opts as in dmrgx_eigs_lowest: ncv (0: 16; at most 64, never more than n_states - nq), max_it, tol (0: 1e-8), seed,
 * use_initial, min_initial_norm2.  `method` is ignored for nq > 0.
 * Refused with DMRGX_ERR_ARG before any MatMult: a null plan, opts, e or psi; nq < 0; a null Q or ldq < n_states; nq >= n_states; a row of
 * Q that is zero or not finite; a row whose norm after the projection against the rows before it falls below 1e-10 of its own norm
 * (linearly dependent); a striped plan (world_size > 1); non-null allgather / allreduce_sum / comm; max_matvec > 0.
 * Method: thick-restart Lanczos with the restart rule, the look at the Ritz pair after every step and the convergence test
 * |r| <= tol |theta| of dmrgx_eigs_lowest's Lanczos path.  Every w = H v_j is orthogonalised twice against all rows of [Qt ; v_0 .. v_j];
 * the Krylov space never grows past n_states - nq, where the answer is exact and converged = 1.
 * Outputs: *e = theta; psi of unit norm, projected against Qt once more before the final normalisation (|<qt_i, psi>| <= 1e-13); stats as
 * for dmrgx_eigs_lowest, `residual` that of P H P.  Not reaching tol within max_it restarts gives DMRGX_ERR_NOTCONV with the last iterate.
 * Memory from the pool, with ld = n_states rounded up to even: (nq + ncv + 1) rows of ld doubles in one allocation, two work vectors of
 * ld (the MatMult's input and output), (nq + ncv + 2) (n_states / 2048 + 1) doubles of per-workgroup partial sums, and O(nq + ncv^2)
 * scalars.  No atomics, every sum has a fixed order: two calls give the same bits in e, psi and the stats (seconds apart). */
dmrgx_status dmrgx_eigs_lowest_orth(dmrgx_kron_plan* plan, const dmrgx_eigs_opts* opts, int32_t nq, const double* Q_dev, int64_t ldq,
                                    double* e, double* psi_dev, dmrgx_eigs_stats* stats, void* stream);

/* Distributed solves only: where the MatMults of the solves since the last reset spent their time on this rank -- the all-gather that
 * rebuilds x (the reference's VecScatter-to-all, src/DMRGKron.cpp:1833-1834) and the apply behind it -- from HIP events on the
 * solver's stream (milliseconds, summed over n_matvec MatMults).  reset != 0 clears the totals.  Any pointer may be null. */
dmrgx_status dmrgx_eigs_comm_timing(double* allgather_ms, double* apply_ms, int64_t* n_matvec, int32_t reset);

/* ---- K3/K4: reduced density matrices + full spectra ------------------------------------------------------ */
/* For every KronBlock k of the layout: rho_L = Psi Psi^T, rho_R = Psi^T Psi (Psi = n_L x n_R row-major slice of
 * psi_dev in the reference's vector layout) and ALL eigenpairs of each, largest first -- the device part of
 * GetTruncation / EigRDM_BlockDiag (include/DMRGBlockContainer.hpp:1715-1775, 1962-2003).  The global sort, the
 * m-cut and the sector bookkeeping (:1795, 1850-1892) stay with the caller. side: 0 = left (rho_L), 1 = right. */
typedef struct dmrgx_rdm dmrgx_rdm;
dmrgx_status dmrgx_rdm_create(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks,
                              const int32_t* block_il, const int32_t* block_ir, const double* psi_dev,
                              void* stream, dmrgx_rdm** out);
/* dmrgx_rdm_create_warm is dmrgx_rdm_create with a starting-basis argument that is accepted for compatibility only: v0_rows (NULL, or
 * per matrix 2*k + side NULL or a device pointer to an orthogonal n x n basis) is never dereferenced, and neither the results nor the
 * sweep counts depend on it.  The Householder-QR preconditioning step of the block-Jacobi solver (csrc/hqr.hip) made it redundant,
 * and the direct solver never had a use for it. */
/* Multi-GPU form: only the density matrices selected by side_mask[k] (bit 0: rho_L, bit 1: rho_R of KronBlock k) are built and
 * diagonalised by this rank -- the matrices of a step are dealt over the ranks by their n^3 cost; psi_dev is the
 * whole vector on every rank.  Queries for a matrix that was not selected fail with DMRGX_ERR_ARG. */
dmrgx_status dmrgx_rdm_create_subset(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks,
                                     const int32_t* block_il, const int32_t* block_ir, const double* psi_dev,
                                     const uint8_t* side_mask, void* stream, dmrgx_rdm** out);
dmrgx_status dmrgx_rdm_create_warm(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks,
                                   const int32_t* block_il, const int32_t* block_ir, const double* psi_dev,
                                   const double* const* v0_rows, void* stream, dmrgx_rdm** out);
/* host_out[0..n) = eigenvalues of block k's matrix, descending (n = sector size on that side). */
dmrgx_status dmrgx_rdm_eigenvalues(const dmrgx_rdm* rdm, int32_t side, int32_t k, double* host_out);
/* dst_dev[r*ld + i], r < count: the eigenvector of the r-th largest eigenvalue as a ROW (a row of RotMatT,
 * == FillRotation_BlockDiag, include/DMRGBlockContainer.hpp:2032-2054). */
dmrgx_status dmrgx_rdm_eigenvectors(const dmrgx_rdm* rdm, int32_t side, int32_t k, int32_t count, double* dst_dev, int64_t ld, void* stream);
/* The same for several (density matrix, destination) pairs in one launch (the rotation of a truncation step asks for one block of rows
 * per kept sector: a dozen launches of a few microseconds each at m = 512). */
typedef struct { int32_t side, k, count, pad; double* dst_dev; int64_t ld; } dmrgx_rdm_vec_task;
dmrgx_status dmrgx_rdm_eigenvectors_batch(const dmrgx_rdm* rdm, int32_t ntasks, const dmrgx_rdm_vec_task* tasks, void* stream);
/* Optional second phase between the spectra and the eigenvectors.  dmrgx_rdm_create* returns with every spectrum final but -- with the direct
 * solver -- no eigenvector formed: the m-cut of GetTruncation (include/DMRGBlockContainer.hpp:1795-1875) is taken on the spectra, and only
 * then are the eigenvectors of the KEPT states computed: counts[2*k + side] = number of (largest) eigenvalues of that density matrix whose
 * eigenvectors are wanted (entries of matrices this rank did not build are ignored).  The last merge of the divide and conquer, the
 * back-transformation and the verification then run on half-width matrices when half of the states are kept.  The spectra do not change
 * (dmrgx_rdm_eigenvalues: the solver's own eigenvalues, descending); dmrgx_rdm_eigenvectors serves count <= counts[..].  A caller that never
 * selects gets every eigenvector at its first dmrgx_rdm_eigenvectors call.  `psi_dev` of the create call must stay unchanged until then.
 * Verification: every selected eigenvalue is computed a second time as the Rayleigh quotient |Psi^T u|^2 of its finished eigenvector; the two
 * are compared when the object is destroyed -- dmrgx_rdm_destroy returns DMRGX_ERR_NOTCONV if they disagree (the counterpart of the
 * reference's "all eigenpairs converged" check, include/DMRGBlockContainer.hpp:1987) -- so the comparison costs no synchronisation. */
dmrgx_status dmrgx_rdm_select(dmrgx_rdm* rdm, const int32_t* counts, void* stream);
/* What the solver of this set of density matrices did.  The reference checks "all eigenpairs converged" after every LAPACK call
 * (include/DMRGBlockContainer.hpp:1987); here a failure would not be a wrong result but a silently slower path, so the path is reported:
 * DMRGRun.json counts TridFallbacks / TridLaunchPathCalls from it and bench.py refuses a leg that took an unexpected path. */
typedef struct {
    int32_t n_sweeps;                   /* block-Jacobi solver: outer sweeps (0 for the direct solver)                                   */
    int32_t solver;                     /* 0: Householder tridiagonalisation + divide and conquer (csrc/symeig.hip), 1: block Jacobi    */
    int32_t trid_persistent_matrices;   /* matrices tridiagonalised by the persistent LDS-resident kernel                                */
    int32_t trid_launch_matrices;       /* ... by one launch per column: by design (order > ~1700) or after a time-out                   */
    int32_t max_workgroups_per_matrix;  /* persistent kernel: workgroups that shared the rows of one matrix                              */
    int32_t merge_levels;               /* depth of the divide-and-conquer tree of the largest matrix                                    */
    int32_t wy_blocks_max;              /* compact-WY blocks (64 reflectors) in the back-transformation of the largest matrix            */
    int32_t timed_out;                  /* this call's persistent round timed out (1) / was lapped (2) and was repeated by launches      */
    int32_t process_timeouts;           /* persistent rounds that timed out in this process so far                                       */
    int32_t persistent_off;             /* the persistent kernel is switched off for the rest of the process (time-out, shared GPU)      */
} dmrgx_rdm_report;
dmrgx_status dmrgx_rdm_info(const dmrgx_rdm* rdm, dmrgx_rdm_report* out);
dmrgx_status dmrgx_rdm_destroy(dmrgx_rdm* rdm);

/* ---- K6: operator rotation + dense-cell accumulate ------------------------------------------------------------ */
/* dst[i*ldd + j] += alpha * src(i,j), src(i,j) = src[i*lds + j] or (transposed) src[j*lds + i]; nr x nc is the shape of
 * the DESTINATION rectangle.  Tasks whose destinations may overlap must carry the same dst_base (e.g. the owning
 * sector block): they are then applied in submission order; dst_base == NULL means "no overlap with other tasks".
 * src == NULL adds alpha to the diagonal of a square destination (scaled-identity source cell). */
typedef struct {
    double* dst; const double* dst_base; const double* src;
    int64_t ldd, lds; int32_t nr, nc; int32_t transposed; double alpha;
} dmrgx_axpy_task;
dmrgx_status dmrgx_cells_axpy(int32_t ntasks, const dmrgx_axpy_task* tasks, void* stream);

/* Truncation as a block rotation: new sector a keeps kept[a] states of old sector old_sector[a] (ascending), rows of
 * RotMatT for it are rot_t[a] (kept[a] x n_old, row-major, ld = n_old; device) -- include/DMRGBlockContainer.hpp:2032-2054. */
typedef struct {
    int32_t n_new;
    const int32_t* old_sector;
    const int32_t* kept;
    const double* const* rot_t;
} dmrgx_rotation;
/* For every source operator o (cells in the OLD sector basis): dst_blocks[o][a] <- RT_a . O_{q -> q+shift} . RT_a'^T with
 * q = old_sector[a] and a' the new sector cut from old sector q+shift; dst_blocks[o][a] is a caller-allocated dense
 * kept[a] x kept[a'] row-major block (ignored / may be NULL when a' does not exist).  == RotateOperators
 * (src/DMRGBlock.cpp:763-772) for Sz(i), Sp(i) and H at once.  Identity cells are square (nr == nc); any other identity
 * cell, and any kind other than DENSE or IDENT, is refused with DMRGX_ERR_ARG. */
dmrgx_status dmrgx_rotate_ops(const dmrgx_sectors* old_sectors, const dmrgx_rotation* rot, int32_t nops,
                              const dmrgx_secop* src_ops, double* const* const* dst_blocks, void* stream);

/* ---- device memory (so that the host engine needs no HIP headers) ------------------------------------------ */
/* Blocks come from a size-class pool inside the library: dmrgx_free never synchronises the device, and a freed block is
 * recycled in STREAM ORDER -- work already queued on it may still be running, the next owner's operations are queued
 * behind it on the same stream.  A caller that frees on one stream and reuses on another calls dmrgx_stream_sync in
 * between (the engine and the Python wrappers use a single stream).  DMRGX_POOL=0 makes every free a plain hipFree. */
dmrgx_status dmrgx_malloc(void** dev_ptr, size_t bytes);
dmrgx_status dmrgx_free(void* dev_ptr);
/* device bytes handed out by the pool now, cached for reuse, and the high-water mark of the first (what the reference's
 * disk spill bounds: src/DMRGBlock.cpp:1090-1103); any pointer may be NULL */
dmrgx_status dmrgx_mem_stats(size_t* in_use, size_t* cached, size_t* peak_in_use);
dmrgx_status dmrgx_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes, void* stream);
dmrgx_status dmrgx_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, void* stream);   /* synchronises the stream */
dmrgx_status dmrgx_memcpy_d2d(void* dst_dev, const void* src_dev, size_t bytes, void* stream);
dmrgx_status dmrgx_memset_zero(void* dst_dev, size_t bytes, void* stream);
dmrgx_status dmrgx_stream_sync(void* stream);
/* *host_out = <x, y> (device vectors, fixed summation order); replaces VecDot in the correlator path
 * (include/DMRGBlockContainer.hpp:2287-2293).  Synchronises the stream. */
dmrgx_status dmrgx_dot(int64_t n, const double* x_dev, const double* y_dev, double* host_out, void* stream);
/* The same without the synchronisation: the sum (same summation order) is written to dev_out[0] in stream order -- lets a
 * caller queue many expectation values and fetch them with one dmrgx_memcpy_d2h. */
dmrgx_status dmrgx_dot_async(int64_t n, const double* x_dev, const double* y_dev, double* dev_out, void* stream);
/* Many 2-D (Frobenius) inner products in one launch: dev_out[t.out] = sum over the tasks with that `out` of
 * sum_ij a[i*lda + j] * b[i*ldb + j]; outputs that no task names are left untouched.  Fixed summation order.  With the
 * Gram blocks G_k = X_k X_k^T of the state this evaluates <psi|P (x) 1|psi> = sum_k <P[IL(k)], G_k> for a whole table of
 * system-block correlators at once (the MatMult + VecDot pairs of include/DMRGBlockContainer.hpp:2287-2293). */
typedef struct { const double* a; int64_t lda; const double* b; int64_t ldb; int32_t nr, nc, out, pad; } dmrgx_dot2d_task;
dmrgx_status dmrgx_dot2d_batch(int32_t count, const dmrgx_dot2d_task* tasks, double* dev_out, void* stream);

/* ---- all-pairs correlators: Gram matrices of operator images ------------------------------------------------- */
/* G[i*ldg + j] (= | +=) sum_{n < len} U[i*ldu + n] * V[j*ldv + n],  i < nu, j < nv: the inner products of two families of long
 * vectors (len contiguous) on the f64 MFMA, split over len into slices whose partial tiles are added in slice order -- no atomics,
 * the result repeats bit for bit.  nu, nv >= 1; len >= 0 (len == 0 writes zeros, or leaves G when accumulating); any ld >= len;
 * pointers only 8-byte aligned.  Same family (same pointer, ld and count): G is bitwise symmetric.  G must not overlap U or V.
 * report (may be NULL): output tiles computed (one triangle for the same family), slices of len, doubles of slab workspace. */
typedef struct { int32_t tiles, slices; int64_t slab_doubles; } dmrgx_gram_report;
dmrgx_status dmrgx_vec_gram(int32_t nu, int32_t nv, int64_t len, const double* U_dev, int64_t ldu,
                            const double* V_dev, int64_t ldv, double* G_dev, int64_t ldg,
                            int32_t accumulate, dmrgx_gram_report* report /* may be NULL */, void* stream);
/* G[a*ldg + b] = < O_a psi , O_b psi >  for the n_left + n_right operators (left ones first): O_a = A_a (x) 1 or 1 (x) B_a.
 * All operators carry the same sector shift (as used, after `transposed`).  psi: reference vector layout over the given KronBlocks.
 * With O = Sz(i) this is the whole table <Sz_i Sz_j>, with O = Sp(i) the table <Sm_i Sp_j>, over all sites of both blocks at once:
 * it replaces one KronConstruct + MatMult + VecDot per correlator (include/DMRGBlockContainer.hpp:2287-2293).
 * The images live on the sector pairs reached from a KronBlock (IL, IR) by the shift: (IL - shift, IR) for a left operator,
 * (IL, IR - shift) for a right one; a pair whose shifted sector does not exist contributes nothing.  Every image block is a list of
 * grouped-GEMM products (dense cells) and scaled copies (identity cells).  workspace_bytes bounds the storage of the images (0: 1 GiB):
 * the image blocks are worked off in slices that fit, each accumulated into G in fixed order; an image block that does not fit on
 * its own is refused with DMRGX_ERR_ARG, as are operators of different shifts; a cell outside its sector block gives
 * DMRGX_ERR_OUTOFRANGE.  report (may be NULL): tiles of G, number of workspace slices, largest slab of a slice. */
dmrgx_status dmrgx_kron_op_gram(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks,
                                const int32_t* block_il, const int32_t* block_ir, const double* psi_dev,
                                int32_t n_left_ops, const dmrgx_secop* left_ops, int32_t n_right_ops, const dmrgx_secop* right_ops,
                                size_t workspace_bytes, double* G_dev, int64_t ldg, dmrgx_gram_report* report, void* stream);
/* G[a*ldg + b] = < v_a , v_b >,  v_a = sum over the terms t of vector a of  c_t (A_t (x) B_t) psi,  a, b < nvec.
 * Vector a owns terms[vec_first[a] .. vec_first[a+1]) (vec_first[0] = 0, every vector at least one term); a term names its operators by
 * index into left_ops / right_ops, -1 meaning the identity on that side (both -1: c psi).  Sector tables, KronBlocks, psi, operators
 * (cells, `transposed`), workspace_bytes, G, ldg and report are those of dmrgx_kron_op_gram, which is this function with one one-sided
 * term per vector.  A term with left shift sA and right shift sB maps KronBlock (IL, IR) to the image block (IL - sA, IR - sB); where
 * either shifted sector does not exist it contributes nothing.  Every term of one call must have the same total sA + sB (the identity
 * counts 0), else DMRGX_ERR_ARG; an operator index outside its list gives DMRGX_ERR_OUTOFRANGE, an empty vector or a vec_first that
 * does not grow DMRGX_ERR_ARG.  Terms of one vector that reach the same image block from different KronBlocks are summed there.
 * A one-sided term is built as in dmrgx_kron_op_gram; a two-sided term takes two grouped launches per workspace slice, like the
 * MatMult: T = X_k B^T into scratch, then A T accumulated into the image.  The coefficient is applied once: as the scale of a scaled
 * copy, or folded into a materialised copy of the (left) operand.
 * Memory on top of workspace_bytes, all from the library's pool: (1) the intermediates T of ONE slice, one n_L(IL) x n_R(IR - sB)
 * matrix per distinct (right operator, source KronBlock) of the two-sided terms that reach the slice -- at most, when one slice holds
 * every image block, sum over the distinct right operators r of two-sided terms of sum_k n_L(IL_k) n_R(IR_k - s_r) doubles: about one
 * superblock vector per such operator (the Ly operators next to the cut for nearest-neighbour bonds); (2) one copy of every dense cell that is stored the other way round than the GEMM
 * reads it (left operators used transposed, right operators stored plainly) or that carries a coefficient other than 1.
 * No atomics: the result repeats bit for bit and is bitwise symmetric. */
dmrgx_status dmrgx_kron_term_gram(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks,
                                  const int32_t* block_il, const int32_t* block_ir, const double* psi_dev,
                                  int32_t n_left_ops, const dmrgx_secop* left_ops, int32_t n_right_ops, const dmrgx_secop* right_ops,
                                  int32_t nvec, const int32_t* vec_first, const dmrgx_term* terms,
                                  size_t workspace_bytes, double* G_dev, int64_t ldg, dmrgx_gram_report* report, void* stream);
/* G[(s*nvec + a)*ldg + (t*nvec + b)] = < v_a(psi_s) , v_b(psi_t) >,  s, t < nstates, a, b < nvec:  dmrgx_kron_term_gram over several states
 * at once, with the inner products between the images of different states -- the transition amplitudes <psi_s|O_a^T O_b|psi_t> and, with
 * an identity vector in the family, <psi_s|O_b|psi_t>.  Psi holds the states as rows in the reference vector layout, row s at
 * Psi_dev + s*ldpsi (the convention of dmrgx_kron_states_expand): ldpsi >= n_states, any 8-byte alignment, rows only read, the columns
 * from n_states to ldpsi never touched.  The family is the nstates * nvec images in state-major order, member s*nvec + a the image v_a of
 * dmrgx_kron_term_gram built from psi_s; sector tables, KronBlocks, operators, vectors, terms (the (-1, -1) identity term, the one total
 * shift), workspace_bytes, report and every check are those of dmrgx_kron_term_gram, with the same codes.  ldg >= nstates * nvec.
 * Refused with DMRGX_ERR_ARG besides: nstates < 1, a null Psi, ldpsi < n_states, a null G, ldg < nstates * nvec.  A refused call writes
 * nothing.
 * Memory: the image blocks of a workspace slice hold all nstates * nvec vectors, so workspace_bytes (0: 1 GiB) bounds
 * nstates * nvec * (doubles of a slice), and an image block whose nstates * nvec copies do not fit is refused with DMRGX_ERR_ARG.  Within a
 * slice the states are built one after another, then one dmrgx_vec_gram over the whole family is accumulated into G, slice after
 * slice.  The intermediates T of the two-sided terms are those of ONE state at a time: the pool memory on top of the workspace is (1)
 * and (2) of dmrgx_kron_term_gram and does not grow with nstates; the operand copies (2) are made once per call.
 * No atomics and a fixed summation order: G is bitwise symmetric, two calls give the same bits, and nstates == 1 gives the bits of
 * dmrgx_kron_term_gram on that row. */
dmrgx_status dmrgx_kron_term_gram_states(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks,
                                         const int32_t* block_il, const int32_t* block_ir,
                                         int32_t nstates, const double* Psi_dev, int64_t ldpsi,
                                         int32_t n_left_ops, const dmrgx_secop* left_ops, int32_t n_right_ops, const dmrgx_secop* right_ops,
                                         int32_t nvec, const int32_t* vec_first, const dmrgx_term* terms,
                                         size_t workspace_bytes, double* G_dev, int64_t ldg, dmrgx_gram_report* report, void* stream);
/* Y[a*ldy + n] = v_a[n], n < n_states:  the images v_a = sum_t c_t (A_t (x) B_t) psi of dmrgx_kron_term_gram themselves, in the reference
 * vector layout of the same KronBlocks.  Sector tables, KronBlocks, psi, operators, vectors and terms, and their checks, are those of
 * dmrgx_kron_term_gram; it is the same builder with the caller's Y in place of the workspace and no Gram matrix taken.  The images must
 * live where psi lives: every term has total shift 0 (DMRGX_ERR_ARG otherwise), and a term that maps a KronBlock to an existing sector pair
 * that is not one of the KronBlocks is refused (DMRGX_ERR_ARG), not dropped.  Every element [0, n_states) of every vector is written
 * exactly once -- KronBlocks that no term reaches as zeros --, the columns from n_states to ldy are not touched.  ldy >= n_states; Y must
 * not overlap psi.  Memory from the pool: the intermediates and cell copies of dmrgx_kron_term_gram, (1) and (2) there.  No atomics: two
 * calls give the same bits. */
dmrgx_status dmrgx_kron_term_apply(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks,
                                   const int32_t* block_il, const int32_t* block_ir, const double* psi_dev,
                                   int32_t n_left_ops, const dmrgx_secop* left_ops, int32_t n_right_ops, const dmrgx_secop* right_ops,
                                   int32_t nvec, const int32_t* vec_first, const dmrgx_term* terms,
                                   double* Y_dev, int64_t ldy, void* stream);
/* Y[a*ldy + n] = v_a[n], n < n_out_states:  the same images written in the reference vector layout of a SECOND KronBlock list
 * (n_out, out_il, out_ir) over the same two sector tables -- the nested list order, block j an n_L(out_il[j]) x n_R(out_ir[j]) row-major
 * matrix, n_out_states the sum of those sizes.  This is how S+_i psi becomes a start vector for a plan of the neighbouring total-Sz
 * sector.  Every other argument, and its checks, are those of dmrgx_kron_term_apply, which is this function with the output list equal
 * to the input list (same bits).  Every term of a call has the same total shift s (DMRGX_ERR_ARG otherwise), and s may be any value.  A
 * term with shifts (sA, sB) maps source KronBlock (IL, IR) to (IL - sA, IR - sB); a pair whose shifted sector does not exist contributes
 * nothing, a pair that exists but is not in the output list is refused (DMRGX_ERR_ARG), not dropped.  An output KronBlock out of range
 * gives DMRGX_ERR_OUTOFRANGE, one listed twice DMRGX_ERR_ARG.  Every element [0, n_out_states) of every vector is written exactly once --
 * output blocks that no term reaches as exact zeros --, the columns from n_out_states to ldy are not touched.  ldy >= n_out_states; Y
 * must not overlap psi; a null Y is DMRGX_ERR_ARG.  n_out == 0 is DMRGX_OK with nothing written (out_il, out_ir may then be NULL).
 * Memory from the pool as for dmrgx_kron_term_apply.  No atomics: two calls give the same bits. */
dmrgx_status dmrgx_kron_term_apply_to(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks,
                                      const int32_t* block_il, const int32_t* block_ir, const double* psi_dev,
                                      int32_t n_left_ops, const dmrgx_secop* left_ops, int32_t n_right_ops, const dmrgx_secop* right_ops,
                                      int32_t nvec, const int32_t* vec_first, const dmrgx_term* terms,
                                      int32_t n_out, const int32_t* out_il, const int32_t* out_ir,
                                      double* Y_dev, int64_t ldy, void* stream);

/* ---- density-matrix noise: psi with the images of one block's operators set beside it --------------------------------- */
/* White's perturbation of the reduced density matrix (PRB 72, 180403) without a new density-matrix build.  For the left block and a
 * KronBlock k = (IL, IR), q = IL,
 *   rho'_q = Psi_q Psi_q^T + sum_a coef[a]^2 sum_k' (A_a Psi_k')(A_a Psi_k')^T,      k' over the KronBlocks with IL_k' - shift_a == q,
 * is Psi'_q Psi'_q^T of the column-expanded Psi'_q = [ Psi_q | coef[a] A_a Psi_k' | ... ]; for the right block the rows are stacked,
 * Psi''_k = [ Psi_k ; coef[b] Psi_k' B_b^T ; ... ] and rho'_R = Psi''^T Psi''.  This call writes the expansion; dmrgx_rdm_create_subset
 * then runs on it unchanged, with `extent` as the sector table of the other side (side 0: right table = extent, block_ir'[k] = k, side mask
 * bit 0; side 1: left table = extent, block_il'[k] = k, bit 1).
 * Sector tables, KronBlocks and psi (reference vector layout, only read) as in dmrgx_kron_term_apply.  side: 0 expands columns with
 * operators of the LEFT block, 1 expands rows with operators of the RIGHT block.  ops[a] (cells, `transposed`, any shift, shifts may differ
 * within a call) live on the sector table of that side; coef: host array [n_ops], finite, any sign.  n_ops == 0 copies psi.
 * Output: block k follows block k - 1 (the nested list order of the KronBlocks) and is row-major.
 *   side 0: n_L(IL_k) x extent[k].  Columns [0, n_R(IR_k)) are Psi_k, copied bit for bit.  Then, for every operator a in ascending order and
 *           for every source KronBlock k' in ascending order with IL_k' - shift_a == IL_k, one panel coef[a] * A_a Psi_k' of n_R(IR_k') columns.
 *   side 1: extent[k] x n_R(IR_k).  Rows [0, n_L(IL_k)) are Psi_k.  Then, in the same order, for every k' with IR_k' - shift_b == IR_k, one
 *           panel coef[b] * Psi_k' B_b^T of n_L(IL_k') rows.
 * A source KronBlock whose shifted sector exists but is the sector of no KronBlock contributes nothing, like one whose shifted sector does
 * not exist: the perturbation never creates a sector the target state cannot use.  An operator without cells in a panel's sector block
 * gives a panel of zeros; coef[a] == 0 gives its panels as exact zeros whatever psi and the cells hold.
 * extent (host [nblocks]) and *n_out (host: the doubles of the whole expansion, sum_k extent[k] times the block's other dimension) are
 * always written.  Y_dev == NULL: sizes only -- nothing else is done, no device is touched, psi_dev may be NULL.  Otherwise every element
 * of [0, *n_out) of Y is written exactly once (Y may hold anything on entry).  Y must not overlap psi.
 * Every panel is a list of grouped-GEMM products (dense cells) and scaled copies (identity cells) with the panel's corner as the output and
 * the block's leading dimension, built and launched as the one-sided terms of dmrgx_kron_term_apply are; the coefficient is applied once,
 * as there.  One grouped launch per tile size for all panels, one strided device copy per KronBlock.  Memory from the pool: one copy of every dense cell
 * that is stored the other way round than the GEMM reads it or that carries a coefficient other than 1 (those of coefficient 0: none).
 * Refused (DMRGX_ERR_ARG): a null sector table, KronBlock list, extent or n_out; ops or coef NULL with n_ops > 0; n_ops < 0; a side that
 * is not 0 or 1; a coefficient that is not finite; a null psi with Y given; Y overlapping psi; a KronBlock listed twice; an expanded
 * extent above 2^31 - 1.  DMRGX_ERR_OUTOFRANGE: a KronBlock or a cell's sector outside the tables, a cell outside its sector block.
 * No atomics: two calls give the same bits. */
dmrgx_status dmrgx_kron_noise_expand(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks,
                                     const int32_t* block_il, const int32_t* block_ir, const double* psi_dev,
                                     int32_t side, int32_t n_ops, const dmrgx_secop* ops, const double* coef /* host [n_ops] */,
                                     int32_t* extent /* host [nblocks]: expanded width (side 0) / height (side 1) of block k */,
                                     int64_t* n_out /* host: total doubles of the expansion */,
                                     double* Y_dev /* NULL: sizes only */, void* stream);

/* ---- several target states: the states set side by side as the input of the state-averaged density matrix -------------- */
/* For states Psi_0 .. Psi_{nstates-1} of one sector with weights w_s, the averaged density matrices sum_s w_s rho_L,s and sum_s w_s rho_R,s
 * without a new density-matrix build: for the left block Psi'_k = [ sqrt(w_0) Psi_0,k | sqrt(w_1) Psi_1,k | ... ] has Psi' Psi'^T =
 * sum_s w_s rho_L,s; for the right block the panels are stacked as rows and Psi''^T Psi'' = sum_s w_s rho_R,s.  This call writes the
 * expansion; dmrgx_rdm_create_subset then runs on it unchanged, with `extent` as the sector table of the other side exactly as for
 * dmrgx_kron_noise_expand (side 0: right table = extent, block_ir'[k] = k, side mask bit 0; side 1: left table = extent, block_il'[k] = k,
 * bit 1).
 * Sector tables and KronBlocks as in dmrgx_kron_term_apply.  Psi_dev: nstates rows in the reference vector layout, row s at
 * Psi_dev + s * ldpsi, ldpsi >= n_states, any 8-byte alignment, only read; the columns beyond n_states are neither read nor touched.
 * weight: host array [nstates], non-negative and finite, not all zero; sqrt(w_s) is taken once on the host.
 * Output: block k follows block k - 1 and is row-major.
 *   side 0: n_L(IL_k) x extent[k], extent[k] = nstates * n_R(IR_k); columns [s n_R, (s + 1) n_R) are sqrt(w_s) Psi_s,k.
 *   side 1: extent[k] x n_R(IR_k), extent[k] = nstates * n_L(IL_k); rows [s n_L, (s + 1) n_L) are sqrt(w_s) Psi_s,k.
 * A panel of weight exactly 1 is a bit-for-bit copy; a panel of weight 0 is exact zeros whatever the state holds (it is not read).
 * extent (host [nblocks]) and *n_out (host: nstates * n_states doubles) are always written.  Y_dev == NULL: sizes only -- nothing else is
 * done, no device is touched, Psi_dev may be NULL.  Otherwise every element of [0, *n_out) of Y is written exactly once (Y may hold
 * anything on entry, any 8-byte alignment).  One strided scaled-copy kernel over all blocks and panels, in 16-byte pairs where a panel's
 * rows are 16-byte aligned on both sides.  Memory from the pool: the table of panels.
 * Refused (DMRGX_ERR_ARG): a null sector table, KronBlock list, extent or n_out; nstates < 1 or null weights; ldpsi < n_states; a weight
 * that is negative or not finite; all weights zero; a side that is not 0 or 1; a null Psi with Y given; Y overlapping Psi; a KronBlock
 * listed twice; an expanded extent above 2^31 - 1.  DMRGX_ERR_OUTOFRANGE: a KronBlock outside the tables.
 * No atomics: two calls give the same bits. */
dmrgx_status dmrgx_kron_states_expand(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks,
                                      const int32_t* block_il, const int32_t* block_ir,
                                      int32_t nstates, const double* Psi_dev, int64_t ldpsi, const double* weight /* host [nstates] */,
                                      int32_t side, int32_t* extent /* host [nblocks]: expanded width (side 0) / height (side 1) of block k */,
                                      int64_t* n_out /* host: total doubles of the expansion */,
                                      double* Y_dev /* NULL: sizes only */, void* stream);

/* ---- products of sector operators of one block (observables of three site operators: the scalar chirality) ------------- */
/* C_o = sum over the strings t of output o of  coeff_t * F_{t,1} F_{t,2} [F_{t,3}],  o < n_out:  sums of products of one, two or three
 * operators of ONE block, formed on the device in dense per-sector form.  Nothing in the reference does this: its correlators multiply
 * site operators pair by pair with MatMatMult (include/DMRGBlockContainer.hpp:2378-2395).
 * sectors: the block's sector table.  ops[0 .. n_ops): the input operators (cells, `transposed`, any shift; only read).  Output o owns
 * strings[out_first[o] .. out_first[o + 1]) (out_first[0] = 0, every output at least one string); a string names its 1, 2 or 3 factors by
 * index into ops, and they multiply in the order given -- truncated block operators do not commute, the order is part of the contract.
 * Every string of one output has the same net shift s_o = the sum of its factors' shifts (DMRGX_ERR_ARG otherwise); outputs may differ.
 * With shifts s1, s2, s3 the block (q -> q + s_o) of a string is F_1[q -> q + s1] F_2[q + s1 -> q + s1 + s2] F_3[.. -> q + s_o]: where a
 * middle sector does not exist, or a factor has no cell there, the string contributes nothing.
 * Host outputs, always written: out_shift[o] = s_o; cells[cell_first[o] .. cell_first[o + 1]) = the cells of output o, one DENSE cell per
 * sector block (q -> q + s_o) whose two sectors exist, ascending q, covering the whole block (r0 = c0 = 0, ld = nc = the size of sector
 * q + s_o); `cells` has room for n_out * nsec entries.  Cell c starts where cell c - 1 ends, the first at arena_dev: *n_doubles is the
 * sum of their sizes.  With shift = out_shift[o] and transposed = 0 the cells are a dmrgx_secop for every other call of this header.
 * arena_dev == NULL: sizes only -- the cells' `data` are NULL, no device is touched.  Otherwise every element of [0, *n_doubles) of the
 * arena is written exactly once (it may hold anything on entry), a block that no string reaches as exact zeros.
 * At most two grouped launches per tile size, through the batch builder of dmrgx_kron_term_apply: (1) the distinct two-factor prefixes
 * (coeff F_1) F_2 of the three-factor strings -- distinct over the whole call by (F_1, F_2, coeff) -- into pool scratch; (2) every block of
 * every output as the groups of its strings.  Identity cells become scaled copies, as there; the coefficient is applied once, in the
 * first factor: in the scale of an identity cell or in a materialised copy of a dense one (exact for the +-1/2 of the chirality).
 * Memory from the pool: the prefixes, about one operator each; one copy of every dense cell that is used transposed or as a first factor
 * with a coefficient other than 1; a unit matrix of the order of the largest identity cell where two identity cells meet or a
 * one-factor string is one.
 * Refused (DMRGX_ERR_ARG): a null sector table, operator list (n_ops > 0), out_first, string list or host output; n_ops < 0, n_out < 0;
 * an output without strings; a factor count outside 1..3; strings of one output with different net shifts; a coefficient that is not
 * finite; an arena that overlaps a dense cell of an input.  DMRGX_ERR_OUTOFRANGE: a factor index outside ops; a cell's sector outside
 * the table; a cell outside its sector block.  A refused call leaves the arena untouched.  n_out == 0: DMRGX_OK, nothing written.
 * No atomics, fixed order: two calls give the same bits. */
typedef struct {
    double  coeff;
    int32_t nfac;         /* 1, 2 or 3                                                                    */
    int32_t fac[3];       /* indices into ops, leftmost factor first; entries from nfac on are ignored   */
} dmrgx_secop_string;
dmrgx_status dmrgx_secop_compose(const dmrgx_sectors* sectors, int32_t n_ops, const dmrgx_secop* ops,
                                 int32_t n_out, const int32_t* out_first, const dmrgx_secop_string* strings,
                                 int32_t* out_shift /* host [n_out] */, int32_t* cell_first /* host [n_out + 1] */,
                                 dmrgx_cell* cells /* host [n_out * nsec] */, int64_t* n_doubles /* host */,
                                 double* arena_dev /* NULL: sizes only */, void* stream);

/* ---- Lanczos coefficients from a given start vector (continued fractions: S(q, w)) ------------------------------------ */
/* The plain three-term recursion with q_0 = v0 / |v0| on the planned Hamiltonian (world_size == 1; a striped plan is refused with
 * DMRGX_ERR_ARG):  w = H q_j - beta_{j-1} q_{j-1};  alpha_j = q_j . w;  w -= alpha_j q_j;  beta_j = |w|;  q_{j+1} = w / beta_j.
 * No basis is kept and nothing is reorthogonalised: three vectors of n_states doubles from the pool, v0 (reference layout, n_states
 * doubles) is only read.  All nsteps steps (>= 1, may exceed n_states) are enqueued without looking at the device; the call ends with
 * one copy and one synchronisation.  Host outputs: *norm2 = |v0|^2, alpha[0..nsteps), beta[0..nsteps), *nsteps_done.
 * Breakdown is decided on the device: at the first j with beta_j <= breakdown_tol * max(|alpha_i| (i <= j), beta_i (i < j)) the run is dead,
 * *nsteps_done = j + 1, and T_{j+1} = tridiag(alpha_0..alpha_j; beta_0..beta_{j-1}) is the whole answer.  beta[j] of that step is the small
 * value found; every later vector is exactly zero, every later coefficient 0, and nothing is ever divided by such a beta (the later
 * MatMults run on zero vectors).  Without a breakdown *nsteps_done = nsteps.  breakdown_tol == 0: 1e-7 (genuine betas of the lattices
 * here are O(1), the beta of an exhausted Krylov space is rounding noise of 1e-8 .. 1e-12); values outside [0, 1): DMRGX_ERR_ARG.
 * A start vector whose squared norm is not a positive finite number (zero, NaN, overflow) gives *norm2 = 0, *nsteps_done = 0 and zero
 * coefficients.  A sum that turns NaN or infinite inside step j (overflow, a NaN operator) ends the run before that step counts:
 * *nsteps_done = j, alpha[j], beta[j] and all later coefficients are 0: no output is ever NaN.  Fixed-order sums, no atomics: two runs
 * give the same bits. */
dmrgx_status dmrgx_kron_lanczos_coeffs(dmrgx_kron_plan* plan, const double* v0_dev, int32_t nsteps, double breakdown_tol,
                                       double* norm2, double* alpha /* [nsteps] */, double* beta /* [nsteps] */,
                                       int32_t* nsteps_done, void* stream);
/* The same recursion with the basis kept and fully reorthogonalised: row j of V (V_dev[j*ldv + e], e < n_states; the caller's device
 * memory, nsteps rows, ldv >= n_states) is q_j.  After the three-term step w is orthogonalised against all of q_0..q_j twice by
 * classical Gram-Schmidt (h = V_{0..j} w, w -= V_{0..j}^T h; h stays on the device); alpha_j is the sum of everything removed along
 * q_j, beta_j = |w| after the second pass.  So V V^T = 1 and V H V^T = tridiag(alpha; beta) hold to rounding over all steps done, which
 * the overlaps <u, q_k> of other vectors with the basis need (the real-space dynamical correlations of -dsf_sites), and an exhausted
 * Krylov space is noticed: beta falls to rounding noise and the run breaks down.  Arguments, refusals, the breakdown rule, the treatment
 * of a zero, NaN or overflowing v0 and of a sum that turns non-finite, the host outputs and the single copy and synchronisation at the
 * end are those of dmrgx_kron_lanczos_coeffs; refused in addition (DMRGX_ERR_ARG): V_dev NULL, ldv < n_states, V overlapping v0.
 * Every row [0, nsteps) of V is written, the rows >= *nsteps_done as exact zeros (V may hold anything on entry); the columns from
 * n_states to ldv are not touched.  The rows stream in 16-byte loads when V_dev is 16-byte aligned and ldv even, else in 8-byte loads.
 * The MatMult runs from and into two fixed pool vectors -- the plan sees one (x, y) pair, never a row of V.  Memory from the pool: those
 * two vectors, nsteps * ceil(n_states / 2048) doubles of partial sums, 2 nsteps of h.  Fixed grids, fixed-order sums, no atomics: two
 * runs give the same bits in alpha, beta and V. */
dmrgx_status dmrgx_kron_lanczos_basis(dmrgx_kron_plan* plan, const double* v0_dev, int32_t nsteps, double breakdown_tol,
                                      double* V_dev, int64_t ldv, double* norm2, double* alpha /* [nsteps] */, double* beta /* [nsteps] */,
                                      int32_t* nsteps_done, void* stream);

/* ---- Chebyshev moments from a given start vector (kernel polynomial method: broadened spectra at linear cost) ---------- */
/* With Ht = (H - centre) / half_width on the planned Hamiltonian (world_size == 1; a striped plan is refused with DMRGX_ERR_ARG):
 * t_0 = v0 (not normalised), t_1 = Ht t_0, t_{n+1} = 2 Ht t_n - t_{n-1}; nsteps = K >= 1 MatMults give t_0 .. t_K.  Nothing is
 * normalised or reorthogonalised and no basis is kept: the recursion is stable as long as the spectrum of H lies inside
 * [centre - half_width, centre + half_width].  Host outputs:
 *   *norm2         = mu_0 = <v0, v0>;
 *   mu_diag[m]     = <v0, T_m(Ht) v0>, m = 0 .. 2K, by the doubling identities mu_{2n} = 2 <t_n, t_n> - mu_0 and
 *                    mu_{2n+1} = 2 <t_{n+1}, t_n> - mu_1;
 *   mu_cross[n*nu + i] = <u_i, t_n>, n = 0 .. K, u_i = row i of U (U_dev[i*ldu + e], e < n_states; ldu >= n_states, any 8-byte
 *                    alignment, only read).  nu == 0: no cross moments, U_dev and mu_cross may be NULL.
 * The whole run is enqueued without looking at the device and ends with one copy and one synchronisation.  Per step one fused kernel
 * reads w = H t_n, t_n and t_{n-1}, writes t_{n+1} and leaves the workgroups' partial sums of <t_{n+1}, t_{n+1}> and <t_{n+1}, t_n>; a
 * one-workgroup kernel adds them in block order.  The vectors go through a ring of 32 rows; whenever 16 consecutive t_n are complete (and
 * for the last, partial block) one dmrgx_vec_gram of U against those rows writes their cross moments on the device, so U is read once
 * per 16 steps.
 * The guard, decided on the device: inside the window |t_n|^2 <= mu_0.  At the first n where <t_{n+1}, t_{n+1}> is not a finite number
 * or exceeds (1 + 1e-6) mu_0 the run is dead: *nsteps_done = D = n, the index of the last valid vector; every later vector is exact
 * zeros, mu_diag[m] = 0 for m > 2D and every row n > D of mu_cross is 0.  Without a trip D = K.  A v0 whose squared norm is not a
 * positive finite number gives *norm2 = 0, D = 0 and all moments 0.  With a finite U no output is ever NaN or infinite.
 * Refused (DMRGX_ERR_ARG): a null argument (mu_cross only when nu > 0), K < 1, a half_width that is not a positive finite number, a
 * centre that is not finite, nu < 0, nu > 0 with U_dev NULL or ldu < n_states.
 * Memory from the pool: 2 + 32 vectors of n_states doubles, 2 ceil(n_states / 2048) partial sums, (K + 1) nu + 2K + 1 moments.  Fixed
 * grids, fixed-order sums, no atomics: two runs give the same bits. */
dmrgx_status dmrgx_kron_chebyshev_moments(dmrgx_kron_plan* plan, const double* v0_dev, double centre, double half_width, int32_t nsteps,
                                          int32_t nu, const double* U_dev, int64_t ldu,
                                          double* norm2, double* mu_diag /* host [2 nsteps + 1] */,
                                          double* mu_cross /* host [(nsteps + 1) * nu], row n; may be NULL when nu == 0 */,
                                          int32_t* nsteps_done, void* stream);

/* ---- Correction vector at one complex frequency (Lorentzian-broadened spectra to a stated residual) -------------------- */
/* 1 / (sigma + i eta - H) v0 = X + i Y on the planned Hamiltonian (world_size == 1; a striped plan is refused with DMRGX_ERR_ARG):
 *   Y = -eta [(H - sigma)^2 + eta^2]^-1 v0,   X = (H - sigma) Y / eta,
 * so that for any u  -(1/pi) <u, Y> = (1/pi) sum_n <u|n><n|v0> eta / ((sigma - E_n)^2 + eta^2): the spectral function under a Lorentzian of
 * half width at half maximum eta, and <u, X> its real counterpart.  Y is found by conjugate gradients on the positive definite
 * A = (H - sigma)^2 + eta^2 with b = -eta v0 and y_0 = 0.  Per iteration two MatMults (t = H p, u = H s with s = t - sigma p), p.A p as the sum
 * of squares s.s + eta^2 p.p, three fused vector kernels and two one-workgroup scalar kernels; alpha, beta, r.r, the count and the flags
 * live in a small device array.  Convergence is decided on the device: r.r <= tol^2 b.b (tol == 0: 1e-8; outside [0, 1): DMRGX_ERR_ARG).
 * Iterations are enqueued in blocks of check_every (0: 8); after each block one small copy brings the count and the flags back -- the only
 * place where the host looks at the device.  Once the run has converged, died or counted max_it iterations, the kernels that remain in
 * the block leave every vector alone and count nothing (their MatMults still run): Y, X, im, re, iterations and both residuals do not
 * depend on check_every, bit for bit; only n_matvec = 2 blocks check_every + 2 does.  After the loop two more MatMults give X (written when
 * X_dev is not NULL) and the true residual |b - A Y| / |b| of the returned Y.
 * v0 (reference layout, n_states doubles) is only read.  Y_dev and X_dev are the caller's buffers of n_states doubles, any 8-byte alignment;
 * every element is written.  U, ldu, nu as in dmrgx_kron_chebyshev_moments (only read; columns beyond n_states neither read nor touched);
 * the overlaps im[i] = <u_i, Y> and re[i] = <u_i, X> are two dmrgx_vec_gram calls after the loop.  The MatMult runs between pool vectors
 * only, two fixed (x, y) pairs; it never sees Y, X or U.
 * Not reaching tol within max_it is no error: DMRGX_OK with converged = 0 and the last iterate.  A v0 whose squared norm is not a positive
 * finite number gives *norm2 = 0, Y = X = exact zeros, zero overlaps, iterations = 0, converged = 0, dead = 1.  A partial sum that is not
 * finite, or a p.A p that is not positive and finite, sets dead before that iteration reaches Y: with a finite H and U no output is ever
 * NaN.  (An H that is not finite shows in the closing MatMults: dead = 1 and true_residual = infinity.)
 * Refused (DMRGX_ERR_ARG): a null plan, v0, Y, norm2 or stats; nu > 0 with im NULL, or with X_dev given and re NULL; eta not positive and
 * finite; sigma not finite; max_it < 1; check_every < 0; nu < 0; nu > 0 with U_dev NULL or ldu < n_states; Y or X overlapping v0, U or
 * each other.  Memory from the pool: four vectors of n_states doubles, 2 ceil(n_states / 2048) partial sums, 12 + 2 nu scalars.  Fixed
 * grids, fixed-order sums, no atomics: two runs give the same bits. */
typedef struct {
    int32_t iterations;      /* CG iterations that counted                                              */
    int32_t converged;       /* 1: the recurrence residual reached tol                                  */
    int32_t n_matvec;        /* dmrgx_kron_apply calls enqueued (frozen iterations of the last block included) */
    int32_t dead;            /* 1: a sum turned non-finite or p.A p was not positive: stopped before that update */
    double  residual;        /* |r| / |b| of the recurrence at the last counted iteration               */
    double  true_residual;   /* |b - A Y| / |b| recomputed from the returned Y                          */
} dmrgx_cv_stats;
dmrgx_status dmrgx_kron_correction_vector(dmrgx_kron_plan* plan, const double* v0_dev, double sigma, double eta,
                                          double tol, int32_t max_it, int32_t check_every,
                                          double* Y_dev, double* X_dev /* may be NULL */,
                                          int32_t nu, const double* U_dev, int64_t ldu,
                                          double* norm2, double* im /* host [nu]: <u_i, Y> */,
                                          double* re /* host [nu]: <u_i, X>; NULL iff X_dev NULL or nu == 0 */,
                                          dmrgx_cv_stats* stats, void* stream);

/* ---- One vector projected out of a family of vectors (operators with an expectation value: no elastic line) ------------ */
/* For every row a < nv of V (V_dev[a*ldv + e], e < len):  coef[a] = <v_a, p> / <p, p>,  then  v_a -= coef[a] p;  *p_norm2 = <p, p>.
 * With p = psi and v_b = D_b psi the rows become (D_b - <D_b>) psi and coef the expectation values: the start vectors and images of a
 * dynamical measurement without the delta peak at w = 0 (-dsf_dimer).  Needs no plan: any vectors of one length on the device.
 * Three launches over ranges of 2048 elements: (1) workgroup b keeps its range of p in registers, walks the nv rows and leaves the
 * partial sums of <v_a, p> and of <p, p>; (2) one workgroup adds the partials in block order, divides and writes the nv coefficients
 * to a device array; (3) the same ranges, p again in registers, v_a[e] -= coef[a] p[e].  p is read twice, V is read twice and written
 * once.  The sums are carried as unevaluated pairs of doubles (exact products by fma, TwoSum) through the division: coef[a] is the
 * quotient of the exact sums to a rounding or two whatever len is -- a row stored as 3 p comes back with coef 3.0 and with nothing but
 * the rounding of its own elements left.  The call ends with one copy and one synchronisation.
 * Rows go through 16-byte accesses when V_dev and p_dev are 16-byte aligned and ldv is even, through 8-byte accesses otherwise; the
 * columns from len to ldv are neither read nor written.  p is only read.
 * If <p, p> is not a positive finite number (p = 0, a NaN, overflow) V is left untouched, every coef is 0 and *p_norm2 = 0.  A row
 * whose dot with p is not finite is left untouched with coef 0 while the other rows are done; so is a row whose coef is exactly 0.
 * len == 0: DMRGX_OK, zeros, nothing touched.  Refused (DMRGX_ERR_ARG): a null pointer, nv < 1, len < 0, ldv < len, p overlapping V.
 * Memory from the pool: 2 (nv + 1) ceil(len / 2048) doubles of partial sums, nv + 2 scalars.  Fixed grids, fixed-order sums, no
 * atomics: two calls give the same bits in coef and V. */
dmrgx_status dmrgx_vec_project_out(int32_t nv, int64_t len, double* V_dev, int64_t ldv, const double* p_dev,
                                   double* coef /* host [nv] */, double* p_norm2 /* host */, void* stream);

/* ---- Static linear response on the complement of one vector (susceptibilities without eta and without pinning fields) -- */
/* With Q = 1 - p p^T / <p, p> on the planned Hamiltonian (world_size == 1; a striped plan is refused with DMRGX_ERR_ARG) the call returns
 *   *coef = <p, v0> / <p, p>,   *norm2 = |Q v0|^2,   X with <p, X> = 0 and Q (H - sigma) Q X = Q v0,   chi[i] = <u_i, X>.
 * With p = psi, sigma = E0 and v0 = O_c psi:  coef = <O_c>  and  2 chi[i] = 2 sum_{n>0} <psi|O_i|n><n|O_c|psi> / (E_n - E0) = d<O_i>/dh_c,
 * the static susceptibility, with an error bounded by |u_i| |Q v0| true_residual / gap.  (The correction vector at w = 0 is no substitute:
 * it solves the squared operator, is broadened by eta and turns singular as eta -> 0, psi lying in the null space of H - E0.)
 * X is found by plain conjugate gradients from x = 0 on A = Q (H - sigma) Q, positive definite on the complement of p when p is the lowest
 * eigenvector and sigma its eigenvalue, with b = Q v0.  Per iteration ONE MatMult t = H d, then s = t - sigma d (over t) with the partial
 * sums of d.A d = <d, s> and of <p, s>; r -= delta p + alpha (s - gamma p) with gamma = <p, s> / <p, p> (what H - sigma leaves along p) and
 * delta = <p, r> / <p, p> of the previous update (what rounding left along p), with the partial sums of r . r and <p, r>; x += alpha d,
 * d = r + beta d: three fused vector kernels (9 vector reads, 4 writes) and two one-workgroup scalar kernels; alpha, beta, gamma, delta,
 * r.r, the count and the flags live in a small device array.  Convergence is decided on the device: r.r <= tol^2 b.b (tol == 0: 1e-8;
 * outside [0, 1): DMRGX_ERR_ARG).  Iterations are enqueued in blocks of check_every (0: 8); after each block one small copy brings the
 * count and the flags back -- the only place where the host looks at the device.  Once the run has converged, died or counted max_it
 * iterations, the kernels that remain in the block leave every vector alone and count nothing (their MatMults still run): X, chi,
 * iterations and both residuals do not depend on check_every, bit for bit; only n_matvec = blocks check_every + 1 does.  After the loop
 * <p, X> / <p, p> p is taken out of X once more, and one more MatMult gives the true residual |b - A X| / |b| of the returned X.
 * p and v0 (reference layout, n_states doubles) are only read; p, v0 and X_dev may sit on any 8-byte alignment.  X_dev is the caller's
 * buffer of n_states doubles; every element is written.  U, ldu, nu as in dmrgx_kron_chebyshev_moments (only read; columns beyond
 * n_states neither read nor touched); the overlaps are one dmrgx_vec_gram call after the loop.  The MatMult runs between pool vectors
 * only, one fixed (x, y) pair; it never sees p, X or U.
 * Not reaching tol within max_it is no error: DMRGX_OK with converged = 0 and the last iterate.  *norm2 <= 1e-24 <v0, v0>, or not positive
 * and finite: v0 is a multiple of p to rounding (the projection leaves about eps^2 per element, far below) -- X is exact zeros, chi is 0,
 * iterations = 0, converged = 1, dead = 0.  <p, p> not positive and finite (or a coefficient that is not finite): X and chi are zeros,
 * *coef = *norm2 = 0, converged = 0, dead = 1.  A partial sum that is not finite, or a d.A d that is not positive and finite (sigma above
 * the second eigenvalue), sets dead before that iteration reaches X: with a finite H and U no output is ever NaN.  (An H that is not
 * finite shows in the closing MatMult: dead = 1 and true_residual = infinity.)
 * Refused (DMRGX_ERR_ARG), before any device work: a null plan, p, v0, X, coef, norm2 or stats; sigma not finite; max_it < 1;
 * check_every < 0; nu < 0; nu > 0 with U_dev or chi NULL or ldu < n_states; X overlapping p, v0 or U.  Memory from the pool: four vectors
 * of n_states doubles (r, d, t and an aligned copy of p), 3 ceil(n_states / 2048) partial sums, 18 + nu scalars.  Fixed grids,
 * fixed-order sums, no atomics: two runs give the same bits.  The stats are those of dmrgx_kron_correction_vector, read for this A and X. */
dmrgx_status dmrgx_kron_static_response(dmrgx_kron_plan* plan, const double* p_dev, const double* v0_dev, double sigma,
                                        double tol, int32_t max_it, int32_t check_every,
                                        double* X_dev, int32_t nu, const double* U_dev, int64_t ldu,
                                        double* coef, double* norm2, double* chi /* host [nu]: <u_i, X>; may be NULL when nu == 0 */,
                                        dmrgx_cv_stats* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DMRGX_H */
