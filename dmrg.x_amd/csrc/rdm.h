// What the two translation units of the density-matrix eigendecomposition share: rdm.hip (layout, Gram matrices, the direct solver,
// selection and queries) and rdm_jacobi.hip (the QR-preconditioned block-Jacobi iteration).  Not part of the ABI.
#pragma once
#include "symeig.h"
#include <chrono>

#ifndef DMRGX_JB
#define DMRGX_JB 16
#endif

namespace dmrgx {

// Every matrix is padded to a multiple of the block-Jacobi sub-problem size (JS in rdm_jacobi.hip) and V starts as the identity: both
// are that solver's requirements.  The direct solver gets the same leading dimensions, which its measured speed belongs to.
constexpr int RDM_PAD = 2 * DMRGX_JB;

// Offsets in doubles from the base of dmrgx_rdm::buf.  a_off, v_off: A and V in that arena.  a2_off: the second buffer of A of the
// block-Jacobi solver (a round reads one, writes the other).  It lives in that solver's own workspace and is still counted from the
// base of dmrgx_rdm::buf, because jacobi_round_kernel takes ONE base pointer; only the solver's own copy of the table has it set.
struct MatDesc { int64_t a_off, a2_off, v_off; int32_t n, npad, nb, pad; };
struct TrTile { int64_t src, dst; int32_t nr, nc, ti, tj; };   // dst (nc x nr) = src (nr x nc)^T
void rdm_transpose(const TrTile* d_tiles, size_t count, const double* in, double* out, hipStream_t st);      // enqueues; hipGetLastError is the caller's

// DMRGX_RDM_TRACE (developer aid, read once): wall time of every stage and the convergence history on stderr (synchronising)
bool rdm_trace();
struct RdmStageClock {
    hipStream_t st;
    std::chrono::steady_clock::time_point t_prev = std::chrono::steady_clock::now();
    void operator()(const char* name);
};

// Enqueues W = Psi^T V_L / Psi V_R and the squared column norms (-> the Rayleigh-quotient region) of the LAST cols[mi] columns of every
// selected matrix.  *any: something was enqueued (nothing is when this rank selected no matrix).
dmrgx_status rdm_rayleigh_enqueue(dmrgx_rdm& P, const std::vector<int32_t>& cols, hipStream_t st, bool* any);
dmrgx_status rdm_solve_direct(dmrgx_rdm& P, hipStream_t st);      // the two solvers, on the Gram matrices in P.buf
dmrgx_status rdm_solve_jacobi(dmrgx_rdm& P, hipStream_t st);

}  // namespace dmrgx

struct dmrgx_rdm {
    int32_t nblocks = 0;
    std::vector<dmrgx::MatDesc> mats;          // index 2*k + side
    dmrgx::DevBuf d_tables;                    // the set-up tables in one upload (d_mats is a view into it)
    // buf, in this order: per matrix A and V; Psi^T; diagonals; Rayleigh quotients; W; the direct solver's eigenvalues.  Everything else
    // a solver needs is its own: symeig's workspace sits in `deferred`, block Jacobi's lives and dies inside rdm_solve_jacobi.
    dmrgx::DevBuf buf, d_mats, d_perm;
    std::vector<std::vector<double>> eig;      // per matrix: eigenvalues, descending
    std::vector<std::vector<int32_t>> perm;    // per matrix: column of V for the r-th largest eigenvalue
    std::vector<int64_t> perm_off;
    std::vector<uint8_t> selected;             // per matrix: built and diagonalised by this rank (dmrgx_rdm_create_subset)
    int32_t sweeps = 0;
    int32_t solver = 0;                        // 0: tridiagonalisation + divide and conquer (symeig*.hip), 1: block Jacobi
    dmrgx::SymEigReport symeig;                // what the direct solver did (solver == 0)
    // ---- second phase (dmrgx_rdm_select; direct solver only): the eigenvectors of the kept states are formed once the caller has cut ----
    dmrgx::SymEigDeferred deferred;            // pending: the spectra are final, the eigenvectors are not formed yet
    std::vector<int32_t> have;                 // per matrix: eigenvectors (and Rayleigh quotients) exist for the `have` largest eigenvalues
    const double* psi = nullptr;               // the state the matrices were built from: must stay alive until the selection
    std::vector<int64_t> off, diag_off;        // offsets of the KronBlocks in psi; of every matrix in the per-position arrays
    std::vector<int32_t> nl, nr;               // sector sizes of every KronBlock
    int64_t psiT_off = 0, w_base = 0, rq_base = 0, ew_base = 0, diag_base = 0, dtot = 0;
    // the Rayleigh quotients of the selected states travel to the host behind the launches that follow them and are compared with the
    // solver's own eigenvalues when the object is destroyed (or verified): no synchronisation of their own
    double* rq_host = nullptr;                 // pinned, from pinned_take
    size_t rq_cap = 0;
    std::vector<int32_t> check_cols;
    hipEvent_t check_event = nullptr;          // recorded behind the read-back: the verification waits for IT, not for the stream
    bool check_pending = false;
    dmrgx::RdmStageClock stage{nullptr};       // of the creating call
    ~dmrgx_rdm();
};
