// The second solver of the reduced density matrices (rdm.hip has the first): a batched two-sided block-Jacobi iteration behind one
// Householder-QR preconditioning step (hqr.hip).  Every density matrix of a call goes through it once one sector exceeds SYMEIG_MAX_N,
// or when DMRGX_RDM_SOLVER=jacobi is set.  All matrices of the call are diagonalised TOGETHER (block size JB = 16): per round every
// matrix contributes nb/2 disjoint block pairs; a 32 x 32 sub-problem is solved by scalar Jacobi in LDS, then the rotation is applied
// to the block columns of A and V and to the block rows of A.  The eigenvalues are the Rayleigh quotients of the finished vectors.
#include "ggemm.h"
#include "hqr.h"
#include "rdm.h"
#include <numeric>

namespace dmrgx {
namespace {

constexpr int JB = DMRGX_JB, JS = RDM_PAD;     // block size, sub-problem size.  Every outer round costs ONE launch of pure
                                             // latency (~25 us at any matrix size: the sub-solves of the next round next to the
                                             // updates of this one); 32 x 32 sub-problems (31 dependent rotation rounds on 256
                                             // threads) measured best: JB = 32 halves the rounds but its 63-round, 1024-thread
                                             // solve is > 2x slower (one cyclic sweep per visit: the outer sweeps finish the job)
static_assert(JB == 16 || JB == 32, "sub-problem of 32 or 64 rows: (JS/16)^2 waves per workgroup");
constexpr int JLD = JS + 1;
constexpr int SUB_THREADS = JB * JB;           // sub-solve: one thread per pair of rotation pairs

struct PairRef { int32_t mat, j; };

__device__ __forceinline__ void pair_blocks(int nb, int r, int j, int& I, int& J)
{
    const int m1 = nb - 1;
    if (m1 == 0) { I = 0; J = 0; return; }
    const int rr = r % m1;
    if (j == 0) { I = m1; J = rr; }
    else { I = (rr + j) % m1; J = (rr - j + m1) % m1; }
    if (I > J) { const int t = I; I = J; J = t; }
}

// inverse of pair_blocks: the pair j of round r that block b sits in, and whether it is that pair's first (0) or second (1) block
__device__ __forceinline__ void block_seat(int nb, int r, int b, int& j, int& half)
{
    const int m1 = nb - 1;
    if (m1 == 0) { j = 0; half = 0; return; }
    const int rr = r % m1;
    if (b == m1 || b == rr) j = 0;
    else { const int d = (b - rr + m1) % m1; j = d <= (m1 - 1) / 2 ? d : m1 - d; }
    int I, J;
    pair_blocks(nb, r, j, I, J);
    half = (b == I) ? 0 : 1;
}

// 1/sqrt(x): hardware estimate (v_rsq_f64) + two Newton steps -- the sub-solve is a chain of dependent scalar math on
// one wave per SIMD, so the length of this sequence is what a Jacobi round costs.
__device__ __forceinline__ double fast_rsqrt(double x)
{
    double y = __builtin_amdgcn_rsq(x);
    y = y * (1.5 - 0.5 * x * y * y);
    y = y * (1.5 - 0.5 * x * y * y);
    return y;
}

// Jacobi rotation annihilating a_pq: with d = (a_qq - a_pp)/2 and h = hypot(d, a_pq), tan(theta) = sign(d) a_pq / (|d| + h)
// (the smaller root), c = 1/sqrt(1 + t^2), s = t c.  Division-free and as short as the dependency chain gets (it is what a
// sub-solve round costs): h and 1/(|d| + h) come from the hardware estimates v_rsq_f64 / v_rcp_f64 with one Newton step --
// an error in t only leaves a_pq' = O(eps a_pq) behind, far below what the next sweep removes -- while c gets the two Newton
// steps of full precision, so that c^2 + s^2 = c^2 (1 + t^2) = 1 to round-off and R stays orthogonal.
__device__ __forceinline__ void jacobi_rotation(double apq, double app, double aqq, double& c, double& s)
{
    c = 1.0; s = 0.0;
    const double apq2 = apq * apq;
    if (apq2 > 1e-300 && apq2 > 1e-36 * fabs(app * aqq)) {
        const double d = 0.5 * (aqq - app);
        const double x = d * d + apq2;
        double ih = __builtin_amdgcn_rsq(x);
        ih = ih * (1.5 - 0.5 * x * ih * ih);
        const double den = fabs(d) + x * ih;
        double rd = __builtin_amdgcn_rcp(den);
        rd = rd * (2.0 - den * rd);
        const double t = (d >= 0.0 ? apq : -apq) * rd;
        c = fast_rsqrt(1.0 + t * t);
        s = t * c;
    }
}

// One Jacobi round = ONE launch of jacobi_round_kernel with three kinds of workgroups:
//   [0, n_sub)   sub-solves of round `round_next`: R (row-major JS x JS) with R^T S R diagonal for every block pair -> rbuf_next;
//   the rest     updates of round `round` (rotations in rbuf): kind 0  A_next[P,Q] = R_P^T A_cur[P,Q] R_Q over the upper triangle
//                of pair blocks + mirror;  kind 1  the eigenvectors V[t,Q] <- V[t,Q] R_Q in place.
// The sub-problem (I',J') of the next round does not wait for the update.  Block b of it sits in exactly one pair p(b) of this
// round, so its off-diagonal block is one rotated tile, which the sub-solve workgroup computes itself from A_cur,
//      S'[I',J'] = ( R_p(I')^T . A_cur[p(I'), p(J')] . R_p(J') ) [half(I'), half(J')],
// and its two diagonal blocks are diagonal blocks of the matrices S_p = R_p^T S R_p that the sub-solves of this round ended with:
// they are handed on through dbuf (they differ from the blocks of A_next by the rounding of a different summation order, i.e.
// the rotation angles by a relative 1e-15 -- convergence is judged on A itself).  The dependency chain of a round is therefore
// one launch (~20 us of sub-solve latency) with the updates -- bound by the traffic of A and V through the Infinity Cache --
// beside it, where it used to be a sub-solve launch and an update launch back to back.  A is double-buffered for that (the
// updates write A_next while the sub-solves read A_cur).  The update needs ~7 workgroups per CU in flight to pull its traffic, so
// the sub-solve path is kept as light as the update path: S and R rotate in place (17 KB of LDS), one MFMA tile, <= 72 registers
// (a first fused version with double-buffered S and R and three FMA-rotated tiles, 34 KB / 100 registers, ran the launch in
// 39.5 us; the two kernels on two streams were slower than back to back because of the cross-stream waits).
struct UpdTask { int32_t mat, p, q, kind; };     // p: pair index (kind 0) or row tile (kind 1); q: pair index (both local to mat)
typedef double jd4 __attribute__((ext_vector_type(4)));

// Seat permutation of the round-robin tournament in "neighbours play" form: the JS indices sit in two rows of JB seats, seat
// 2t above seat 2t+1, and seat 2t always plays seat 2t+1.  After a round everybody except seat 0 moves one seat clockwise;
// after JS-1 rounds all pairs have met and everybody is back (period JS-1), so S and R end in their original order.
__device__ __forceinline__ int jacobi_next_seat(int s)
{
    if (s == 0) return 0;
    if (s == 1) return 2;
    if (s & 1) return s - 2;                 // lower row moves left
    return s == JS - 2 ? JS - 1 : s + 2;     // upper row moves right, the last one drops to the lower row
}
// "Cross" form, for a visit that only rotates the pairs BETWEEN the two blocks (the pairs inside a block are rotated once per
// sweep, in the full visits of its first round): block I sits in the upper row (even seats) and stays, block J in the lower row
// moves one seat left per round, and after JB rounds every (i, j) has met once and everybody is back.
__device__ __forceinline__ int jacobi_next_seat_cross(int s) { return (s & 1) ? (s + JS - 2) % JS : s; }
// seat of index j of the sub-problem ([block I; block J]) at the start (and at the end) of a visit
__device__ __forceinline__ int jacobi_seat_of(int j, int cross) { return cross ? (j < JB ? 2 * j : 2 * (j - JB) + 1) : j; }

// acc = R_P^T . M[rows, cols] . R_Q (two_sided) or M[rows, cols] . R_Q for one JS x JS tile, rows = blocks (IP, JP) of JB rows or
// JS consecutive rows from row0 (IP < 0), cols = blocks (IQ, JQ).  256 threads = 2 x 2 waves, each wave owns a 16 x 16 quarter
// of the tile as one v_mfma_f64_16x16x4 accumulator (fragment maps as in ggemm.hip: A[i = l&15][k = l>>4], B[k = l>>4][j = l&15],
// result col = l&15, row = (l>>4) + 4 reg); the tile goes through LDS (X, JS x JLD), R_Q and R_P^T go from global memory
// straight into MFMA fragments.  (The plain-FMA version of these products was LDS-bandwidth bound: the update ran at ~12 TF/s
// and took 70 % of the eigensolve at m = 2048.)  Leaves the once-rotated tile in X; ends without a barrier.
constexpr int JW = JS / 16;                    // the workgroup is a JW x JW grid of waves, one 16 x 16 MFMA block of the tile each
static_assert(SUB_THREADS == 64 * JW * JW, "one thread per pair of rotation pairs == one wave per 16 x 16 block of the tile");
__device__ __forceinline__ jd4 tile_rotate(double* X, const double* __restrict__ M, int npad, int IP, int JP, int row0, int IQ, int JQ,
                                           const double* __restrict__ Rq, const double* __restrict__ Rp, bool two_sided)
{
    constexpr int KG = JS / 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave / JW, wc = wave % JW;
    const int l15 = lane & 15, l4 = lane >> 4;
    auto cq = [&](int j) { return j < JB ? IQ * JB + j : JQ * JB + j - JB; };
    auto rp = [&](int i) { return IP >= 0 ? (i < JB ? IP * JB + i : JP * JB + i - JB) : row0 + i; };
    // fragments: B operand of X . R_Q is R_Q[k][16 wc + l15]; A operand of R_P^T . Y is R_P[k][16 wr + l15]
    double bq[KG], ap[KG];
#pragma unroll
    for (int g = 0; g < KG; ++g) {
        bq[g] = Rq[(4 * g + l4) * JS + 16 * wc + l15];
        ap[g] = two_sided ? Rp[(4 * g + l4) * JS + 16 * wr + l15] : 0.0;
    }
    for (int e = tid; e < JS * JS; e += SUB_THREADS) {
        const int i = e / JS, j = e % JS;
        X[i * JLD + j] = M[(int64_t)rp(i) * npad + cq(j)];
    }
    __syncthreads();
    jd4 acc = (jd4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int g = 0; g < KG; ++g) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(X[(16 * wr + l15) * JLD + 4 * g + l4], bq[g], acc, 0, 0, 0);      // X . R_Q
    if (two_sided) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) X[(16 * wr + l4 + 4 * r) * JLD + 16 * wc + l15] = acc[r];
        __syncthreads();
        acc = (jd4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int g = 0; g < KG; ++g) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[g], X[(4 * g + l4) * JLD + 16 * wc + l15], acc, 0, 0, 0);  // R_P^T . (X . R_Q)
    }
    return acc;
}

//   kind 0 (A, two-sided): block (P,Q), P <= Q, of the pair-block partition:  A_next[P,Q] = R_P^T . A_cur[P,Q] . R_Q, and its
//                          transpose is written to A_next[Q,P] -- every JS x JS block is written by exactly one workgroup, the
//                          column and the row update of the textbook formulation fuse into one pass over the upper
//                          triangle, and A stays symmetric to the last bit;
//   kind 1 (V, one-sided): rows [JS*t, JS*t+JS) x pair-block Q:      V[t,Q] <- V[t,Q] . R_Q
__device__ __forceinline__ void jacobi_update_body(double* X, const MatDesc* __restrict__ mats, const int32_t* __restrict__ pair_start, const UpdTask t,
                                                   double* __restrict__ buf, const double* __restrict__ rbuf, int round, int flip)
{
    const MatDesc m = mats[t.mat];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave / JW, wc = wave % JW, l15 = lane & 15, l4 = lane >> 4;
    int IQ, JQ, IP = -1, JP = -1;
    pair_blocks(m.nb, round, t.q, IQ, JQ);
    if (t.kind == 0) pair_blocks(m.nb, round, t.p, IP, JP);
    const double* Rq = rbuf + (int64_t)(pair_start[t.mat] + t.q) * JS * JS;
    const double* Rp = rbuf + (int64_t)(pair_start[t.mat] + t.p) * JS * JS;
    const double* M = buf + (t.kind == 0 ? (flip ? m.a2_off : m.a_off) : m.v_off);       // A: read the current buffer,
    double* Mo = buf + (t.kind == 0 ? (flip ? m.a_off : m.a2_off) : m.v_off);            //    write the other one; V: in place
    const jd4 acc = tile_rotate(X, M, m.npad, IP, JP, t.p * JS, IQ, JQ, Rq, Rp, t.kind == 0);
    auto cq = [&](int j) { return j < JB ? IQ * JB + j : JQ * JB + j - JB; };
    auto rp = [&](int i) { return t.kind == 0 ? (i < JB ? IP * JB + i : JP * JB + i - JB) : t.p * JS + i; };
#pragma unroll
    for (int r = 0; r < 4; ++r) Mo[(int64_t)rp(16 * wr + l4 + 4 * r) * m.npad + cq(16 * wc + l15)] = acc[r];
    if (t.kind == 0 && t.p != t.q) {                              // mirror: A[Q,P] = (A[P,Q])^T, staged through LDS for row-wise stores
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) X[(16 * wr + l4 + 4 * r) * JLD + 16 * wc + l15] = acc[r];
        __syncthreads();
        for (int e = tid; e < JS * JS; e += SUB_THREADS) {
            const int i = e / JS, j = e % JS;                     // element (i, j) of the transposed block
            Mo[(int64_t)cq(i) * m.npad + rp(j)] = X[j * JLD + i];
        }
    }
}

// The sub-solve is a chain of JS-1 dependent rotation rounds; what a round costs is instructions issued (several sub-problems
// share a CU) plus two LDS round trips.  So the loop carries no index arithmetic at all: thread (k, l) always owns the 2 x 2
// block of seats {2k, 2k+1} x {2l, 2l+1} of S and rows 2k, 2k+1 x columns {2l, 2l+1} of R, reads it from fixed addresses and,
// after the barrier that also hands over the rotations, writes the rotated block to the fixed addresses of the seats its rows /
// columns move to (in place: every read of a round precedes that barrier, every write follows it); the JB rotations of a
// round are computed once, by the first JB lanes of wave 0 from the fixed pivot positions (2t, 2t+1), and handed over through LDS.
//
// flip: which buffer of A is current.  has_prev == 0: no rotation is pending (very first round): S' is A_cur itself and the
// launch holds sub-solves only.  dbuf / dbuf_next: per pair the two JB x JB diagonal blocks of the S it ended with.
__global__ void __launch_bounds__(SUB_THREADS)
jacobi_round_kernel(const MatDesc* __restrict__ mats, const PairRef* __restrict__ pairs, int n_sub, double* __restrict__ buf, int flip,
                    const double* __restrict__ rbuf, const double* __restrict__ dbuf, int round, int has_prev,
                    double* __restrict__ rbuf_next, double* __restrict__ dbuf_next, int round_next, int cross,
                    const UpdTask* __restrict__ tasks, const int32_t* __restrict__ pair_start)
{
    constexpr int BUFSZ = JS * JLD;
    constexpr bool STAGE_IN_R = (JB > 16);            // JB = 32: 33 KB per buffer -- the staging tile shares R's (two workgroups per CU)
    __shared__ double sh[(STAGE_IN_R ? 2 : 3) * BUFSZ];    // S, R and the staging tile of the off-diagonal block (JB = 16: 25 KB, the registers
                                                      // cap the kernel at 6 workgroups per CU anyway)
    __shared__ double rot_c[JB], rot_s[JB];
    if ((int)blockIdx.x >= n_sub) { jacobi_update_body(sh, mats, pair_start, tasks[blockIdx.x - n_sub], buf, rbuf, round, flip); return; }
    double* S = sh;
    double* R = sh + BUFSZ;
    const PairRef pr = pairs[blockIdx.x];
    const MatDesc m = mats[pr.mat];
    int I, J;
    pair_blocks(m.nb, round_next, pr.j, I, J);
    const int tid = threadIdx.x;
    const double* A = buf + (flip ? m.a2_off : m.a_off);
    if (!STAGE_IN_R) for (int e = tid; e < JS * JS; e += SUB_THREADS) R[(e / JS) * JLD + jacobi_seat_of(e % JS, cross)] = (e / JS == e % JS) ? 1.0 : 0.0;
    if (!has_prev) {
        for (int e = tid; e < JS * JS; e += SUB_THREADS) {
            const int i = e / JS, j = e % JS;
            const int gi = (i < JB ? I * JB + i : J * JB + i - JB), gj = (j < JB ? I * JB + j : J * JB + j - JB);
            S[jacobi_seat_of(i, cross) * JLD + jacobi_seat_of(j, cross)] = A[(int64_t)gi * m.npad + gj];
        }
    } else {
        // blocks (I, J) of the coming round, as they are once this round's rotations are applied
        int jp0, hp0, jp1, hp1, PI0, PJ0, PI1, PJ1;
        block_seat(m.nb, round, I, jp0, hp0);
        block_seat(m.nb, round, J, jp1, hp1);
        pair_blocks(m.nb, round, jp0, PI0, PJ0);
        pair_blocks(m.nb, round, jp1, PI1, PJ1);
        const int64_t g0 = pair_start[pr.mat] + jp0, g1 = pair_start[pr.mat] + jp1;
        // diagonal blocks: loads issued before the tile rotation, stored after it
        double dv[2 * JB * JB / SUB_THREADS];
#pragma unroll
        for (int u = 0; u < 2 * JB * JB / SUB_THREADS; ++u)
            dv[u] = dbuf[(u == 0 ? g0 * 2 + hp0 : g1 * 2 + hp1) * (JB * JB) + tid];
        const jd4 acc = tile_rotate(STAGE_IN_R ? R : sh + 2 * BUFSZ, A, m.npad, PI0, PJ0, 0, PI1, PJ1, rbuf + g1 * JS * JS, rbuf + g0 * JS * JS, true);
        const int lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
        // the block (half hp0 of the rows, half hp1 of the columns) of the rotated tile is a JW/2 x JW/2 group of waves
        if ((wave / JW) / (JW / 2) == hp0 && (wave % JW) / (JW / 2) == hp1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int si = jacobi_seat_of(16 * ((wave / JW) % (JW / 2)) + l4 + 4 * r, cross), sj = jacobi_seat_of(JB + 16 * ((wave % JW) % (JW / 2)) + l15, cross);
                S[si * JLD + sj] = acc[r]; S[sj * JLD + si] = acc[r];
            }
        }
#pragma unroll
        for (int u = 0; u < 2 * JB * JB / SUB_THREADS; ++u) S[jacobi_seat_of(u * JB + tid / JB, cross) * JLD + jacobi_seat_of(u * JB + tid % JB, cross)] = dv[u];
    }
    if (STAGE_IN_R) {
        __syncthreads();                                // the staging tile is read no more
        for (int e = tid; e < JS * JS; e += SUB_THREADS) R[(e / JS) * JLD + jacobi_seat_of(e % JS, cross)] = (e / JS == e % JS) ? 1.0 : 0.0;
    }
    __syncthreads();
    {
        // (no convergence test per sub-problem: a launch lasts as long as its slowest sub-solve, rotations of negligible elements are
        //  skipped one by one in jacobi_rotation, and the test itself -- a reduction and two barriers -- cost 0.7 us of every round)
        {
            const int k = tid / JB, l = tid % JB;
            // loop-invariant LDS offsets (elements): the block this thread reads, and where its two rows / columns go
            const int r0 = 2 * k, r1 = 2 * k + 1, c0 = 2 * l, c1 = 2 * l + 1;
            const int nr0 = cross ? jacobi_next_seat_cross(r0) : jacobi_next_seat(r0), nr1 = cross ? jacobi_next_seat_cross(r1) : jacobi_next_seat(r1);
            const int nc0 = cross ? jacobi_next_seat_cross(c0) : jacobi_next_seat(c0), nc1 = cross ? jacobi_next_seat_cross(c1) : jacobi_next_seat(c1);
            const int nrounds = cross ? JB : JS - 1;
            const int in00 = r0 * JLD + c0, in01 = r0 * JLD + c1, in10 = r1 * JLD + c0, in11 = r1 * JLD + c1;
            const int so00 = nr0 * JLD + nc0, so01 = nr0 * JLD + nc1, so10 = nr1 * JLD + nc0, so11 = nr1 * JLD + nc1;     // S: rows and columns move
            const int ro00 = r0 * JLD + nc0, ro01 = r0 * JLD + nc1, ro10 = r1 * JLD + nc0, ro11 = r1 * JLD + nc1;         // R: only columns move
            const int piv = (2 * tid) * JLD + 2 * tid;                                                                  // lane t < JB: pivot block (2t, 2t+1)
#pragma unroll 1
            for (int rr = 0; rr < nrounds; ++rr) {
                if (tid < JB) {                                            // wave 0, JB lanes: one rotation each
                    double c, sn;
                    jacobi_rotation(S[piv + 1], S[piv], S[piv + JLD + 1], c, sn);
                    rot_c[tid] = c; rot_s[tid] = sn;
                }
                const double b00 = S[in00], b01 = S[in01], b10 = S[in10], b11 = S[in11];
                const double q00 = R[in00], q01 = R[in01], q10 = R[in10], q11 = R[in11];
                __syncthreads();
                const double ck = rot_c[k], sk = rot_s[k], cl = rot_c[l], sl = rot_s[l];
                const double t00 = cl * b00 - sl * b01, t01 = sl * b00 + cl * b01;
                const double t10 = cl * b10 - sl * b11, t11 = sl * b10 + cl * b11;
                S[so00] = ck * t00 - sk * t10; S[so01] = ck * t01 - sk * t11;
                S[so10] = sk * t00 + ck * t10; S[so11] = sk * t01 + ck * t11;
                R[ro00] = cl * q00 - sl * q01; R[ro01] = sl * q00 + cl * q01;
                R[ro10] = cl * q10 - sl * q11; R[ro11] = sl * q10 + cl * q11;
                __syncthreads();
            }
        }
    }
    double* Rout = rbuf_next + (int64_t)blockIdx.x * JS * JS;
    for (int e = tid; e < JS * JS; e += SUB_THREADS) Rout[e] = R[(e / JS) * JLD + jacobi_seat_of(e % JS, cross)];
    double* Dout = dbuf_next + (int64_t)blockIdx.x * 2 * JB * JB;
    for (int e = tid; e < 2 * JB * JB; e += SUB_THREADS) {
        const int h = e / (JB * JB), r = (e % (JB * JB)) / JB, c = e % JB;
        Dout[e] = S[jacobi_seat_of(h * JB + r, cross) * JLD + jacobi_seat_of(h * JB + c, cross)];
    }
}

// per matrix and block of the grid: out[(mat*NORM_BLOCKS + b)*2] = partial sum of squares off the diagonal, [..+1] = on it
constexpr int NORM_BLOCKS = 32;
__global__ void __launch_bounds__(256) offnorm_kernel(const MatDesc* __restrict__ mats, const double* __restrict__ buf, double* __restrict__ out, int flip)
{
    __shared__ double r0[4], r1[4];
    MatDesc m = mats[blockIdx.y];
    if (flip) m.a_off = m.a2_off;
    double off = 0.0, dg = 0.0;
    const int64_t tot = (int64_t)m.npad * m.npad;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += 256 * NORM_BLOCKS) {
        const int i = (int)(e / m.npad), j = (int)(e % m.npad);
        const double v = buf[m.a_off + e];
        if (i == j) dg += v * v; else off += v * v;
    }
    for (int o = 32; o > 0; o >>= 1) { off += __shfl_down(off, o, 64); dg += __shfl_down(dg, o, 64); }
    if ((threadIdx.x & 63) == 0) { r0[threadIdx.x >> 6] = off; r1[threadIdx.x >> 6] = dg; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[(blockIdx.y * NORM_BLOCKS + blockIdx.x) * 2] = r0[0] + r0[1] + r0[2] + r0[3];
        out[(blockIdx.y * NORM_BLOCKS + blockIdx.x) * 2 + 1] = r1[0] + r1[1] + r1[2] + r1[3];
    }
}

__global__ void diag_kernel(const MatDesc* __restrict__ mats, const double* buf, double* out, const int64_t* __restrict__ out_off)
{
    const MatDesc m = mats[blockIdx.x];
    for (int i = threadIdx.x; i < m.npad; i += blockDim.x) out[out_off[blockIdx.x] + i] = buf[m.a_off + (int64_t)i * m.npad + i];
}

// Thousands of plane rotations leave the columns of V orthogonal to ~1e-15 but their norms drift by ~1e-13:
// renormalise every column once at the end (64 columns per workgroup, coalesced along the row).
__global__ void __launch_bounds__(256) normalize_columns_kernel(const MatDesc* __restrict__ mats, double* __restrict__ buf)
{
    __shared__ double part[4][64];
    const MatDesc m = mats[blockIdx.y];
    const int c0 = blockIdx.x * 64;
    if (c0 >= m.npad) return;
    const int col = c0 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
    double* V = buf + m.v_off;
    double s = 0.0;
    if (col < m.npad) for (int i = rg; i < m.npad; i += 4) { const double v = V[(int64_t)i * m.npad + col]; s += v * v; }
    part[rg][threadIdx.x & 63] = s;
    __syncthreads();
    const double tot = part[0][threadIdx.x & 63] + part[1][threadIdx.x & 63] + part[2][threadIdx.x & 63] + part[3][threadIdx.x & 63];
    const double inv = tot > 0.0 ? 1.0 / sqrt(tot) : 0.0;
    if (col < m.npad) for (int i = rg; i < m.npad; i += 4) V[(int64_t)i * m.npad + col] *= inv;
}

// Preconditioner input: B = [ P^T A P | I ] (n x 2n) with P the permutation that sorts the diagonal of A downwards
__global__ void __launch_bounds__(256) qr_gather_kernel(const MatDesc* __restrict__ mats, const HqrMat* __restrict__ qm, const int32_t* __restrict__ perm,
                                                         const int64_t* __restrict__ perm_off, double* __restrict__ buf)
{
    const MatDesc m = mats[blockIdx.y];
    const HqrMat q = qm[blockIdx.y];
    const int n = q.n;
    const int32_t* pm = perm + perm_off[blockIdx.y];
    const int64_t tot = (int64_t)n * 2 * n;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (int64_t)gridDim.x * 256) {
        const int i = (int)(e / (2 * n)), j = (int)(e % (2 * n));
        buf[q.b_off + e] = j < n ? buf[m.a_off + (int64_t)pm[i] * m.npad + pm[j]] : (j - n == i ? 1.0 : 0.0);
    }
}

// Preconditioner output: E (n x n, rows = the new basis in the original index order):  E[r][perm[j]] = Q^T[r][j]
__global__ void __launch_bounds__(256) qr_scatter_kernel(const HqrMat* __restrict__ qm, const int32_t* __restrict__ perm, const int64_t* __restrict__ perm_off,
                                                          const int64_t* __restrict__ e_off, double* __restrict__ buf)
{
    const HqrMat q = qm[blockIdx.y];
    const int n = q.n;
    const int32_t* pm = perm + perm_off[blockIdx.y];
    const int64_t tot = (int64_t)n * n;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (int64_t)gridDim.x * 256) {
        const int r = (int)(e / n), j = (int)(e % n);
        buf[e_off[blockIdx.y] + (int64_t)r * n + pm[j]] = buf[q.b_off + (int64_t)r * 2 * n + n + j];
    }
}

}  // namespace

dmrgx_status rdm_solve_jacobi(dmrgx_rdm& P, hipStream_t st)
{
    const int nm = (int)P.mats.size();
    double* buf = P.buf.as<double>();
    // ---- this solver's own tables and workspace (laid out from 0 here, moved behind the allocation below) ---------------------
    std::vector<MatDesc> mats = P.mats;      // + a2_off
    std::vector<PairRef> pairs;
    std::vector<UpdTask> tiles;              // the A updates of a round, then its V updates
    std::vector<int32_t> pair_start(nm);
    int64_t total = 0;
    auto take = [&](int64_t len) { const int64_t o = total; total += len; return o; };
    int max_nb = 2, max_npad = JS;
    for (int mi = 0; mi < nm; ++mi) {
        MatDesc& m = mats[mi];
        m.a2_off = take((int64_t)m.npad * m.npad);
        max_nb = std::max(max_nb, m.nb); max_npad = std::max(max_npad, m.npad);
        pair_start[mi] = (int32_t)pairs.size();
        const int np = m.nb / 2;
        for (int j = 0; j < np; ++j) pairs.push_back(PairRef{mi, j});
        for (int p = 0; p < np; ++p) for (int q = p; q < np; ++q) tiles.push_back(UpdTask{mi, p, q, 0});     // upper triangle; the kernel mirrors
    }
    for (int mi = 0; mi < nm; ++mi) {
        const MatDesc& m = mats[mi];
        for (int t = 0; t < m.npad / JS; ++t) for (int q = 0; q < m.nb / 2; ++q) tiles.push_back(UpdTask{mi, t, q, 1});
    }
    const int64_t rbuf_len = (int64_t)pairs.size() * JS * JS, rbuf_off = take(2 * rbuf_len);          // two slots: round r and r+1
    const int64_t dbuf_len = (int64_t)pairs.size() * 2 * JB * JB, dbuf_off = take(2 * dbuf_len);      // diagonal blocks handed from round to round
    const int64_t norm_off = take(2 * nm * NORM_BLOCKS);
    // QR preconditioner (2 <= n <= HQR_MAX_N): B = [A | I], reflector scratch, the basis E; then W = E A and E^T of the transform
    std::vector<HqrMat> qmats(nm, HqrMat{0, 0, 0, 0, 0});
    std::vector<int64_t> qe_off(nm, 0), qperm_off(nm, 0), tr_w(nm, 0), tr_et(nm, 0);
    int64_t qperm_tot = 0;
    for (int mi = 0; mi < nm; ++mi) {
        const int64_t n = mats[mi].n;
        if (n < 2 || n > HQR_MAX_N) continue;
        qmats[mi] = HqrMat{take(2 * n * n), take(32 * n), take(32 * 32), (int32_t)n, 0};
        qe_off[mi] = take(n * n); tr_w[mi] = take(n * n); tr_et[mi] = take(n * n);
        qperm_off[mi] = qperm_tot; qperm_tot += n;
    }
    DevBuf ws;
    DMRGX_CHK(ws.alloc_f64((size_t)total, st));
    double* w = ws.as<double>();
    const int64_t base = (int64_t)((intptr_t)ws.p - (intptr_t)P.buf.p) / (int64_t)sizeof(double);      // the kernels count from buf (MatDesc, rdm.h)
    for (int mi = 0; mi < nm; ++mi)
        for (int64_t* o : {&mats[mi].a2_off, &qmats[mi].b_off, &qmats[mi].v_off, &qmats[mi].t_off, &qe_off[mi], &tr_w[mi], &tr_et[mi]}) *o += base;
    DevBuf tab, ttab;
    PackedUpload pk, tpk;
    const size_t o_m = pk.add(mats), o_p = pk.add(pairs), o_t = pk.add(tiles), o_ps = pk.add(pair_start), o_d = pk.add(P.diag_off);
    const size_t o_qm = pk.add(qmats), o_qpo = pk.add(qperm_off), o_qeo = pk.add(qe_off);
    DMRGX_CHK(pk.upload(tab, st));
    const MatDesc* dm = packed_at<MatDesc>(tab, o_m);
    const PairRef* d_pairs = packed_at<PairRef>(tab, o_p);
    const UpdTask* d_tiles = packed_at<UpdTask>(tab, o_t);
    const int32_t* d_pstart = packed_at<int32_t>(tab, o_ps);
    if (qperm_tot > 0) {
        // ---- QR step: diagonal of every matrix -> host, sort downwards, gather [P^T A P | I], factor, scatter Q^T back to the original order
        std::vector<double> hd((size_t)P.dtot);
        hipLaunchKernelGGL(diag_kernel, dim3(nm), dim3(256), 0, st, dm, (const double*)buf, buf, (const int64_t*)packed_at<int64_t>(tab, o_d));
        DMRGX_HIP(hipGetLastError());
        DMRGX_HIP(hipMemcpyAsync(hd.data(), buf + P.diag_base, hd.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        DMRGX_HIP(hipStreamSynchronize(st));
        std::vector<int32_t> qperm((size_t)qperm_tot);
        int max_n = 0;
        for (int mi = 0; mi < nm; ++mi) {
            const int n = qmats[mi].n;                      // (0: not preconditioned, nothing to sort)
            max_n = std::max(max_n, n);
            const double* d = hd.data() + (P.diag_off[mi] - P.diag_base);
            int32_t* pm = qperm.data() + qperm_off[mi];
            std::iota(pm, pm + n, 0);
            std::stable_sort(pm, pm + n, [&](int32_t a, int32_t b) { return d[a] > d[b]; });
        }
        DevBuf d_qperm;
        DMRGX_CHK(upload(d_qperm, qperm, st));
        const HqrMat* d_qm = packed_at<HqrMat>(tab, o_qm);
        const int64_t* d_qpoff = packed_at<int64_t>(tab, o_qpo);
        const unsigned gx = (unsigned)std::min<int64_t>(512, ((int64_t)max_n * 2 * max_n + 255) / 256);
        hipLaunchKernelGGL(qr_gather_kernel, dim3(gx, nm), dim3(256), 0, st, dm, d_qm, d_qperm.as<int32_t>(), d_qpoff, buf);
        DMRGX_HIP(hipGetLastError());
        DMRGX_CHK(hqr_batched(qmats, d_qm, buf, st));
        hipLaunchKernelGGL(qr_scatter_kernel, dim3(gx, nm), dim3(256), 0, st, d_qm, d_qperm.as<int32_t>(), d_qpoff, (const int64_t*)packed_at<int64_t>(tab, o_qeo), buf);
        DMRGX_HIP(hipGetLastError());
        P.stage("qr");
        // ---- similarity transform into that basis E (orthogonal, rows): A <- E A E^T, V <- E^T.  It saves the first sweeps; the rest is
        //      the linearly converging tail of near-degenerate small eigenvalues.
        std::vector<TrTile> tt;
        GemmBatch b1, b2;
        GemmSet s1, s2;
        for (int mi = 0; mi < nm; ++mi) {
            const MatDesc& m = mats[mi];
            const int32_t n = qmats[mi].n;
            if (!n) continue;
            for (int ti = 0; ti < (n + 31) / 32; ++ti) for (int tj = 0; tj < (n + 31) / 32; ++tj) tt.push_back(TrTile{qe_off[mi], tr_et[mi], n, n, ti, tj});
            b1.gemm(s1, buf + tr_w[mi], n, n, n, buf + qe_off[mi], n, buf + m.a_off, m.npad, n);         // W = E A
            b2.gemm(s2, buf + m.a_off, m.npad, n, n, buf + tr_w[mi], n, buf + tr_et[mi], n, n);          // A = W E^T
        }
        const size_t o_tt = tpk.add(tt);
        b1.pack(tpk); b1.pack(s1, tpk); b2.pack(tpk); b2.pack(s2, tpk);
        DMRGX_CHK(tpk.upload(ttab, st));
        b1.bind(ttab); b2.bind(ttab);
        rdm_transpose(packed_at<TrTile>(ttab, o_tt), tt.size(), buf, buf, st);
        DMRGX_HIP(hipGetLastError());
        DMRGX_CHK(b1.launch(s1, ttab, st));
        DMRGX_CHK(b2.launch(s2, ttab, st));
        for (int mi = 0; mi < nm; ++mi) {
            const MatDesc& m = mats[mi];
            if (qmats[mi].n) DMRGX_HIP(hipMemcpy2DAsync(buf + m.v_off, (size_t)m.npad * sizeof(double), buf + tr_et[mi], (size_t)m.n * sizeof(double),
                                                        (size_t)m.n * sizeof(double), (size_t)m.n, hipMemcpyDeviceToDevice, st));
        }
        P.stage("transform");
    }
    // ---- the sweeps ------------------------------------------------------------------------------------------------------------
    std::vector<double> norms((size_t)2 * nm * NORM_BLOCKS);
    const int rounds = std::max(1, max_nb - 1);
    int sweep = 0, slot = 0, flip = 0;
    bool have_rot = false;                   // rbuf[slot] / dbuf[slot] hold the rotations of the round about to be applied
    for (; sweep < 30; ++sweep) {
        hipLaunchKernelGGL(offnorm_kernel, dim3(NORM_BLOCKS, nm), dim3(256), 0, st, dm, (const double*)buf, w + norm_off, flip);
        DMRGX_HIP(hipGetLastError());
        DMRGX_HIP(hipMemcpyAsync(norms.data(), w + norm_off, norms.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        DMRGX_HIP(hipStreamSynchronize(st));
        bool conv = true;
        double worst = 0.0;
        // off <= 1e-12 ||A||_F: V is a product of rotations (orthogonal to round-off whatever the convergence) and the
        // eigenvalues are re-evaluated as Rayleigh quotients below, whose error is O(off^2)
        for (int mi = 0; mi < nm; ++mi) {
            double off2 = 0.0, dg2 = 0.0;
            for (int b = 0; b < NORM_BLOCKS; ++b) { off2 += norms[(size_t)(mi * NORM_BLOCKS + b) * 2]; dg2 += norms[(size_t)(mi * NORM_BLOCKS + b) * 2 + 1]; }
            if (off2 > 1e-24 * (off2 + dg2)) conv = false;
            worst = std::max(worst, off2 / std::max(off2 + dg2, 1e-300));
        }
        if (rdm_trace()) fprintf(stderr, "[rdm] sweep %d: max off^2/total^2 = %.3e\n", sweep, worst);
        if (conv) break;
        for (int r = 0; r < rounds; ++r) {
            double *rcur = w + rbuf_off + slot * rbuf_len, *rnext = w + rbuf_off + (slot ^ 1) * rbuf_len;
            double *dcur = w + dbuf_off + slot * dbuf_len, *dnext = w + dbuf_off + (slot ^ 1) * dbuf_len;
            if (!have_rot) {                 // very first round: sub-solves alone, straight from A
                hipLaunchKernelGGL(jacobi_round_kernel, dim3((unsigned)pairs.size()), dim3(SUB_THREADS), 0, st, dm, d_pairs, (int)pairs.size(), buf, flip,
                                   (const double*)rcur, (const double*)dcur, 0, 0, rcur, dcur, r, 0, d_tiles, d_pstart);
                DMRGX_HIP(hipGetLastError());
                have_rot = true;
            }
            // apply round r (A_cur -> A_next, V in place) and, beside it, solve the sub-problems of the round after it
            const int r_next = (r + 1 == rounds) ? 0 : r + 1;
            const int cross_next = r_next != 0 ? 1 : 0;      // the pairs inside a block: once per sweep, in its first round
            hipLaunchKernelGGL(jacobi_round_kernel, dim3((unsigned)(pairs.size() + tiles.size())), dim3(SUB_THREADS), 0, st, dm, d_pairs, (int)pairs.size(), buf, flip,
                               (const double*)rcur, (const double*)dcur, r, 1, rnext, dnext, r_next, cross_next, d_tiles, d_pstart);
            DMRGX_HIP(hipGetLastError());
            slot ^= 1; flip ^= 1;
        }
    }
    P.sweeps = sweep;
    if (sweep >= 30) DMRGX_FAIL(DMRGX_ERR_NOTCONV, "rdm_create: block Jacobi did not converge in 30 sweeps");
    hipLaunchKernelGGL(normalize_columns_kernel, dim3((max_npad + 63) / 64, nm), dim3(256), 0, st, dm, buf);
    DMRGX_HIP(hipGetLastError());
    P.stage("jacobi");
    // ---- eigenvalues: Rayleigh quotients of ALL renormalised columns, in whatever order the iteration left them; sorted descending on the
    //      host, with the column of V remembered for each rank.  The padding is decoupled: the real eigenvectors are the columns [0, n) of V.
    std::vector<int32_t> cols((size_t)nm);
    for (int mi = 0; mi < nm; ++mi) cols[(size_t)mi] = mats[mi].n;
    bool any = false;
    DMRGX_CHK(rdm_rayleigh_enqueue(P, cols, st, &any));
    if (!any) return DMRGX_OK;
    std::vector<double> rq((size_t)P.dtot, 0.0);
    DMRGX_HIP(hipMemcpyAsync(rq.data(), buf + P.rq_base, rq.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    DMRGX_HIP(hipStreamSynchronize(st));
    std::vector<int32_t> allperm;
    for (int mi = 0; mi < nm; ++mi) {
        const int32_t n = mats[mi].n;
        const double* q = rq.data() + (P.diag_off[mi] - P.diag_base);
        std::vector<int32_t>& real = P.perm[mi];
        real.resize(n);
        std::iota(real.begin(), real.end(), 0);
        std::stable_sort(real.begin(), real.end(), [&](int32_t a, int32_t b) { return q[a] > q[b]; });
        P.eig[mi].resize(n);
        for (int32_t r = 0; r < n; ++r) P.eig[mi][r] = q[real[r]];
        P.perm_off[mi] = (int64_t)allperm.size();
        allperm.insert(allperm.end(), real.begin(), real.end());
        P.have[(size_t)mi] = n;
    }
    DMRGX_CHK(upload(P.d_perm, allperm, st));
    P.stage("rayleigh");
    return DMRGX_OK;
}

}  // namespace dmrgx
