// First phase of the batched symmetric eigensolver (symeig.h; driver: symeig.hip): Householder tridiagonalisation  A = Q T Q^T  of all
// matrices of a call, by one of two kernels.
//
//  ONE LAUNCH PER COLUMN (trid_step_kernel).  The eigenproblem of a DMRG step is a
//     latency chain, not a flop count (sum n^3 ~ 3e9 at m = 2048): a column step needs two dependent reductions over the whole
//     column, and the cheapest chip-wide barrier on this machine is a kernel boundary (~1.5 us; an in-kernel all-to-all exchange
//     costs ~3 us).  The classical two phases of a column (y = A v; rank-2 update A -= v w^T + w v^T) are skewed so that one
//     launch does both with one pass over the trailing matrix: every workgroup first finishes, redundantly, the O(n) vector work
//     of the column (w_{j-1} from y_{j-1}; the updated row j -> d_j, e_j, v_j, tau_j), then applies the update of reflector j-1
//     to its rows and multiplies the updated rows by v_j on the way (y_j).  n launches per matrix, all matrices in each launch.
//  ONE PERSISTENT LAUNCH with the matrices resident in LDS (trid_coop_kernel, "1b" below), in rounds that trid_plan lays out: the
//     normal path.  Its status word tells the caller, behind the caller's own synchronisation, whether every workgroup got its partners.
#include "symeig_impl.h"
#include <numeric>

namespace dmrgx {
using namespace symeig_impl;
namespace {

constexpr int TRID_THREADS = 256, TRID_ROWS = 8;      // rows of the trailing matrix per workgroup (two per wave)
constexpr int TRID_PF = 8;                            // chunks of 64 columns requested per row before they are used
struct TridMat {
    double *A, *VT, *y, *d, *e, *tau;                 // VT: row j = reflector v_j (zeros up to column j); y: 2 x n (double-buffered A v)
    int32_t n, lda, ldv, pad;
};
// ---------------------------------------------------------------------------------------------------------------------------
// 1. tridiagonalisation: launch j
// ---------------------------------------------------------------------------------------------------------------------------
// Stored state at the start of launch j: rows / columns >= j of A carry the updates of reflectors 0 .. j-2; y_{j-1} = A v_{j-1}
// (un-scaled) and v_{j-1}, tau_{j-1} are in memory.  Row j is read by everybody and written by nobody (it retires here), rows
// > j are each updated by exactly one wave, so the launch has no write-read race on A.
struct TridArgs { TridMat m[TRID_MAXM]; };            // (TRID_MAXM matrices per launch: a descriptor table in memory costs every workgroup two dependent cold loads
                                                      //  before it can ask for its vectors: ~1.5 us of a ~5 us launch)
__global__ void __launch_bounds__(TRID_THREADS)
trid_step_kernel(const TridArgs args, int j)
{
    extern __shared__ double sh[];                  // w | v_{j-1} | row j, then v_j   (indexed by the absolute column)
    __shared__ double red[TRID_THREADS / 64];
    const TridMat& m = args.m[blockIdx.y];
    const int n = m.n, tid = threadIdx.x, g = blockIdx.x;
    // Workgroup g owns rows [8 g, 8 g + 8) of its matrix in EVERY launch (the grid does not shrink with j: workgroups whose rows have
    // all retired leave at once), so a row is always handled by the same position of the grid.  The last row block also does the
    // bookkeeping of the column (it is never retired before the matrix is done).
    const int glast = (n - 1) / TRID_ROWS;
    if (j >= n || g > glast || (TRID_ROWS * g + TRID_ROWS - 1 <= j && g != glast)) return;
    double* sw = sh;
    double* svp = sh + n;
    double* svj = sh + 2 * n;
    const double tau_p = j > 0 ? m.tau[j - 1] : 0.0;
    const double* yp = m.y + (size_t)((j + 1) & 1) * n;
    double* yc = m.y + (size_t)(j & 1) * n;
    const double* vprow = m.VT + (int64_t)(j > 0 ? j - 1 : 0) * m.ldv;
    const double* arow = m.A + (int64_t)j * m.lda;
    // the rows this wave will update.  Their first TRID_PF chunks of 64 columns are requested now, ahead of the column's vector work
    // (the loads depend on nothing but addresses; the update is latency-bound otherwise)
    const int lane = tid & 63, wave = tid >> 6;
    const int i0 = TRID_ROWS * g + 2 * wave;            // rows i0, i0+1, where they still belong to the trailing matrix (> j)
    const bool r0 = i0 > j && i0 < n, r1 = i0 + 1 > j && i0 + 1 < n;
    double* a0 = m.A + (int64_t)(r0 ? i0 : j) * m.lda;
    double* a1 = m.A + (int64_t)(r1 ? i0 + 1 : j) * m.lda;
    const int kb = j + 1 + lane;
    double pa0[TRID_PF], pa1[TRID_PF];
#pragma unroll
    for (int c = 0; c < TRID_PF; ++c) {
        const int k = kb + 64 * c;
        pa0[c] = (r0 && k < n) ? a0[k] : 0.0;
        pa1[c] = (r1 && k < n) ? a1[k] : 0.0;
    }
    double s = 0.0;
    for (int k = j + tid; k < n; k += TRID_THREADS) {
        const double vp = j > 0 ? vprow[k] : 0.0, y = j > 0 ? yp[k] : 0.0;
        svp[k] = vp; sw[k] = y; svj[k] = arow[k];
        s += y * vp;
    }
    s = block_sum<TRID_THREADS / 64>(s, red, tid);
    const double coef = 0.5 * tau_p * tau_p * s;     // w = tau y - (tau^2 (y.v) / 2) v
    for (int k = j + tid; k < n; k += TRID_THREADS) sw[k] = tau_p * sw[k] - coef * svp[k];
    __syncthreads();
    const double wj = sw[j], vpj = svp[j];
    double sig = 0.0;
    for (int k = j + tid; k < n; k += TRID_THREADS) {     // row j with the update of reflector j-1 applied
        const double r = svj[k] - vpj * sw[k] - wj * svp[k];
        svj[k] = r;
        if (k >= j + 2) sig += r * r;
    }
    sig = block_sum<TRID_THREADS / 64>(sig, red, tid);
    const double dj = svj[j];
    const double alpha = (j + 1 < n) ? svj[j + 1] : 0.0;
    double beta = alpha, tj = 0.0, scale = 0.0;          // dlarfg: H x = beta e_1, H = I - tau v v^T, v_1 = 1
    if (sig > 0.0) {
        const double nrm = sqrt(alpha * alpha + sig);
        beta = alpha >= 0.0 ? -nrm : nrm;
        tj = (beta - alpha) / beta;
        scale = 1.0 / (alpha - beta);
    }
    __syncthreads();                                    // everyone holds d_j and alpha before row j turns into v_j
    for (int k = j + tid; k < n; k += TRID_THREADS)     // a reflector with tau = 0 is stored as the zero vector (H = I)
        svj[k] = (k <= j || tj == 0.0) ? 0.0 : (k == j + 1 ? 1.0 : svj[k] * scale);
    __syncthreads();
    if (g == glast) {
        double* vt = m.VT + (int64_t)j * m.ldv;
        for (int k = tid; k < n; k += TRID_THREADS) vt[k] = k > j ? svj[k] : 0.0;
        if (tid == 0) { m.d[j] = dj; if (j + 1 < n) m.e[j] = beta; m.tau[j] = tj; }
    }
    // ---- own rows: A[i,:] -= v_{j-1}[i] w^T + w[i] v_{j-1}^T, then y_j[i] = A[i,:] . v_j -- two rows per wave
    if (!r0 && !r1) return;
    const double vp0 = r0 ? svp[i0] : 0.0, w0 = r0 ? sw[i0] : 0.0, vp1 = r1 ? svp[i0 + 1] : 0.0, w1 = r1 ? sw[i0 + 1] : 0.0;
    double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
    for (int c = 0; c < TRID_PF; ++c) {
        const int k = kb + 64 * c;
        if (k < n) {
            const double wk = sw[k], vpk = svp[k], vjk = svj[k];
            const double x0 = pa0[c] - (vp0 * wk + w0 * vpk), x1 = pa1[c] - (vp1 * wk + w1 * vpk);
            if (r0) a0[k] = x0;
            if (r1) a1[k] = x1;
            acc0 += x0 * vjk; acc1 += x1 * vjk;
        }
    }
    for (int kc = kb + 64 * TRID_PF; kc < n + lane; kc += 64 * TRID_PF) {     // (kc - lane < n: wave-uniform trip count)
#pragma unroll
        for (int c = 0; c < TRID_PF; ++c) {
            const int k = kc + 64 * c;
            pa0[c] = (r0 && k < n) ? a0[k] : 0.0;
            pa1[c] = (r1 && k < n) ? a1[k] : 0.0;
        }
#pragma unroll
        for (int c = 0; c < TRID_PF; ++c) {
            const int k = kc + 64 * c;
            if (k < n) {
                const double wk = sw[k], vpk = svp[k], vjk = svj[k];
                const double x0 = pa0[c] - (vp0 * wk + w0 * vpk), x1 = pa1[c] - (vp1 * wk + w1 * vpk);
                if (r0) a0[k] = x0;
                if (r1) a1[k] = x1;
                acc0 += x0 * vjk; acc1 += x1 * vjk;
            }
        }
    }
    acc0 = wave_sum(acc0); acc1 = wave_sum(acc1);
    if (lane == 0) { if (r0) yc[i0] = acc0; if (r1) yc[i0 + 1] = acc1; }
}

// ---------------------------------------------------------------------------------------------------------------------------
// 1b. tridiagonalisation with the matrices RESIDENT IN LDS: one persistent launch
// ---------------------------------------------------------------------------------------------------------------------------
// The launch-per-column kernel above pays, per column, a kernel boundary plus a chain of cold loads (~4 us) and streams the whole
// trailing matrix through the fabric twice (read + write-back: ~5 us on average at m = 2048).  Here the rows of a matrix are dealt
// cyclically over G workgroups (one per CU, up to 160 KB of LDS each: 16 rows of a 1037 x 1037 matrix) and never leave the chip;
// per column the workgroups exchange only what the vector work needs -- y_j = A v_j (each publishes the entries of its rows) and
// the next pivot row (published by its owner while it updates it) -- as 8-byte {epoch, half of a double} granules written with
// agent-scope atomic stores and polled with agent-scope atomic loads: the data is the flag, no fence, no ordering assumption
// (cdna_hip_programming.md section 6, Guideline 16, form R2).  Buffers are double-buffered by column parity: a workgroup can be at
// most one column ahead of the slowest one, because publishing column j+1 needs everybody's column j.  Every spin is bounded: a
// workgroup that is not served in time (its partners are not resident -- e.g. another process holds CUs with a persistent kernel of
// its own) sets the status word and leaves; the host then repeats the step with the launch-per-column kernel (A is only read here).
typedef unsigned long long u64;
typedef double dbl2 __attribute__((ext_vector_type(2)));
typedef u64 __attribute__((address_space(1))) gu64;
#define DMRGX_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
constexpr int TC_THREADS = 512, TC_WAVES = TC_THREADS / 64;
constexpr int TC_SPIN_LIMIT = 1 << 19;               // polls of one batch of granules before giving up (~0.5 s)
#ifndef TC_FIRST_SLEEP
#define TC_FIRST_SLEEP 10                            // s_sleep units (64 clocks) before the first poll of a column: the partners' publications are still on their way
#endif                                               // then, and polls that come back empty are traffic in their way: 0 / 6 / 8 / 10 / 12 / 14 -> 752 / 721 / 709 / 701 / 706 / 715 us
#ifndef TC_RETRY_SLEEP                               // per call at m = 512, 4556 / 4309 / 4265 / 4262 / 4291 / 4335 at m = 2048 (profiles/r05_trid_first_poll_delay.txt)
#define TC_RETRY_SLEEP 1                             // between polls of what is still missing (0 / 1 / 2 / 4: 700 / 701 / 706 / 765 us)
#endif
constexpr int TC_KB = 4;                             // columns per thread whose granules are in flight together
constexpr int TC_MB = 4;                             // chunks of 64 columns of the row pass whose LDS reads are in flight together
constexpr int TC_VECS = 4;                           // O(n) vectors every workgroup keeps beside its rows

struct TcMat {
    const double* A; double *VT, *d, *e, *tau;
    u64 *ybuf, *rowbuf;                               // 2 (parity) x n x 2 granules each
    int32_t n, lda, ldv, G, wg0, pad;
};
struct TcArgs { TcMat m[TRID_MAXM]; int32_t* status; long long* prof; int32_t nm, fault; };      // prof: developer aid (phase clocks of one workgroup), else null;
                                                                                                // fault: test hook, one workgroup withholds one publication

__device__ __forceinline__ void put_f64(u64* g, unsigned epoch, double v)
{
    const u64 b = (u64)__double_as_longlong(v), e = (u64)epoch << 32;
    __hip_atomic_store((gu64*)g, e | (b & 0xffffffffull), DMRGX_RLX_AGENT);
    __hip_atomic_store((gu64*)(g + 1), e | (b >> 32), DMRGX_RLX_AGENT);
}

// (Measured and dropped: the rows in REGISTERS instead of LDS -- 256-thread workgroups, one wave per SIMD, 6 rows x 17 chunks per
// lane.  The f64 update of a lane's ~100 elements is then one dependent-issue stream per SIMD: 2.5 us per column against ~1 us for
// eight waves over LDS-resident rows, and the whole column 9.9 us against 4.9.)
__global__ void __launch_bounds__(TC_THREADS)
trid_coop_kernel(const TcArgs args)
{
    extern __shared__ __attribute__((aligned(16))) double shc[];      // y / w (two buffers) | v (two buffers) | the rows of this workgroup
    __shared__ double red_s[TC_WAVES], red_g[TC_WAVES], piv[2];
    __shared__ int sfail;
    const int b = blockIdx.x;
    int mi = 0;
    for (; mi < args.nm; ++mi) if (b >= args.m[mi].wg0 && b < args.m[mi].wg0 + args.m[mi].G) break;
    if (mi == args.nm) return;
    const TcMat& m = args.m[mi];
    const int n = m.n, G = m.G, g = b - m.wg0, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nv = (n + 1) & ~1;                        // even stride: the row pass moves two columns per lane (ds_read_b128 / ds_write_b128)
    double* sw = shc;
    double* sw_next = shc + nv;
    double* svp = shc + 2 * (size_t)nv;
    double* svj = shc + 3 * (size_t)nv;
    double* rows = shc + TC_VECS * (size_t)nv;          // row t of this workgroup = row g + G t of the matrix
    const int cnt = g < n ? (n - g + G - 1) / G : 0;
    // Who runs how long.  A workgroup publishes for as long as it owns a row below the pivot: rows i > j contribute y_j[i], and row j + 1
    // is published by its owner.  The owner of row n - 1 (`glast`) therefore publishes in every column, every other workgroup needs its
    // granule of every column, and it can never fall two columns behind unnoticed -- so it is the one that writes d, e, tau and V^T; a
    // workgroup whose last row has become the pivot (or that has no row at all) LEAVES: it would only consume, nobody would wait for it,
    // and a lagging pure consumer finds its double-buffered slots overwritten by epochs j + 2 / j + 3 and spins to the time-out
    // (round 3 had workgroup 0 do the bookkeeping to the end).
    const int glast = (n - 1) % G, ilast = cnt > 0 ? g + G * (cnt - 1) : -1;
    if (cnt == 0) return;
    for (int t = 0; t < cnt; ++t) {
        const double* src = m.A + (int64_t)(g + G * t) * m.lda;
        for (int k = tid; k < nv; k += TC_THREADS) rows[(size_t)t * nv + k] = k < n ? src[k] : 0.0;
    }
    for (int k = tid; k < nv; k += TC_THREADS) { svj[k] = 0.0; svp[k] = 0.0; sw[k] = 0.0; sw_next[k] = 0.0; }
    if (g == 0) for (int k = tid; k < n; k += TC_THREADS) put_f64(m.rowbuf + 2 * (size_t)k, 1u, m.A[k]);     // row 0, epoch 1
    if (tid == 0) sfail = 0;
    __syncthreads();
    double tau_p = 0.0, out_d = 0.0, out_e = 0.0;
    const bool prof = args.prof && mi == 0 && g == (G > 1 ? 1 : 0) && tid == 0;
    long long pt[4] = {0, 0, 0, 0}, pc = 0;
    for (int j = 0; j < n; ++j) {
        if (g != glast && j >= ilast) {                                // (uniform per workgroup) nothing left to publish: see above
            if (prof) for (int q = 0; q < 4; ++q) args.prof[q] = pt[q] / (j > 0 ? j : 1);      // (developer aid: mean ticks per column of the columns it took part in)
            return;
        }
        if (prof) pc = wall_clock64();
        { double* t = svp; svp = svj; svj = t; }                      // svp = v_{j-1}
        // `glast` (which everybody waits for in every column) writes column j-1's results HERE, where it would otherwise only wait for
        // the partners' publications, instead of in front of its own rows
        if (g == glast && j > 0) {
            double* vt = m.VT + (int64_t)(j - 1) * m.ldv;
            for (int k = tid; k < n; k += TC_THREADS) vt[k] = k > j - 1 ? svp[k] : 0.0;
            if (tid == 0) { m.d[j - 1] = out_d; m.e[j - 1] = out_e; m.tau[j - 1] = tau_p; }
        }
        const u64* rb = m.rowbuf + (size_t)(j & 1) * 2 * n;              // row j, epoch j+1
        const u64* yb = m.ybuf + (size_t)((j + 1) & 1) * 2 * n;          // y_{j-1}, epoch j
        double s = 0.0;
        bool ok = true, lap = false;
        // every granule this thread needs is requested before the first tag is looked at (TC_KB columns x 4 loads in flight), and only
        // the columns that were not there yet are asked for again
#if TC_FIRST_SLEEP > 0
        if (j > 0) __builtin_amdgcn_s_sleep(TC_FIRST_SLEEP);      // the partners' publications are in flight: a poll that leaves now comes back empty and is in their way
#endif
        for (int k0 = j + tid; k0 < n; k0 += TC_THREADS * TC_KB) {
            unsigned pending = 0;
#pragma unroll
            for (int c = 0; c < TC_KB; ++c) if (k0 + c * TC_THREADS < n) pending |= 1u << c;
            for (int spins = 0; pending; ++spins) {
                u64 x[TC_KB][4];
#pragma unroll
                for (int c = 0; c < TC_KB; ++c) {
                    if (!(pending >> c & 1)) continue;
                    const size_t k = (size_t)(k0 + c * TC_THREADS);
                    x[c][0] = __hip_atomic_load((gu64*)(rb + 2 * k), DMRGX_RLX_AGENT);
                    x[c][1] = __hip_atomic_load((gu64*)(rb + 2 * k + 1), DMRGX_RLX_AGENT);
                    if (j > 0) { x[c][2] = __hip_atomic_load((gu64*)(yb + 2 * k), DMRGX_RLX_AGENT); x[c][3] = __hip_atomic_load((gu64*)(yb + 2 * k + 1), DMRGX_RLX_AGENT); }
                }
#pragma unroll
                for (int c = 0; c < TC_KB; ++c) {
                    if (!(pending >> c & 1)) continue;
                    const unsigned er = (unsigned)(j + 1), ey = (unsigned)j;
                    bool ready = (unsigned)(x[c][0] >> 32) == er && (unsigned)(x[c][1] >> 32) == er;
                    // an epoch NEWER than the one waited for is not "not yet": the slot was overwritten, this workgroup has been lapped
                    // -- a protocol error, reported at once instead of after 0.5 s of spinning
                    bool lapped = (unsigned)(x[c][0] >> 32) > er || (unsigned)(x[c][1] >> 32) > er;
                    if (j > 0) {
                        ready = ready && (unsigned)(x[c][2] >> 32) == ey && (unsigned)(x[c][3] >> 32) == ey;
                        lapped = lapped || (unsigned)(x[c][2] >> 32) > ey || (unsigned)(x[c][3] >> 32) > ey;
                    }
                    if (lapped) { ok = false; lap = true; pending = 0; break; }
                    if (!ready) continue;
                    const int k = k0 + c * TC_THREADS;
                    const double a = __longlong_as_double((long long)((x[c][0] & 0xffffffffull) | (x[c][1] << 32)));
                    const double y = j > 0 ? __longlong_as_double((long long)((x[c][2] & 0xffffffffull) | (x[c][3] << 32))) : 0.0;
                    sw[k] = y; svj[k] = a;
                    pending &= ~(1u << c);
                }
                if (pending) {
                    if (spins > TC_SPIN_LIMIT) { ok = false; break; }
                    __builtin_amdgcn_s_sleep(TC_RETRY_SLEEP);
                }
            }
        }
        // INVARIANT: the vector arithmetic of a column is done redundantly by every workgroup of the matrix and must be BIT-IDENTICAL in
        // all of them (same thread -> column map, same summation order): they never exchange v_j or w, so a one-ulp disagreement is
        // never repaired and the recurrence amplifies it (found the hard way: adding y.v in granule-arrival order broke Tr T = Tr A).
        for (int k = j + tid; k < n; k += TC_THREADS) s += sw[k] * svp[k];
        if (prof) { const long long c = wall_clock64(); pt[0] += c - pc; pc = c; }
        if (!ok) sfail = lap ? 2 : 1;
        s = block_sum1<TC_WAVES>(s, red_s, tid);          // (its barrier also publishes the y and the pivot row the other threads just stored)
        if (sfail) { if (tid == 0) __hip_atomic_store(args.status, sfail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }     // 1: timed out, 2: lapped
        const double coef = 0.5 * tau_p * tau_p * s;
        const double vpj = svp[j], wj = tau_p * sw[j] - coef * vpj;     // w_{j-1}[j], straight from y[j]: no barrier between w and the row update
        double sig = 0.0;
        for (int k = j + tid; k < n; k += TC_THREADS) {
            const double vpk = svp[k], wk = tau_p * sw[k] - coef * vpk;
            const double r = svj[k] - vpj * wk - wj * vpk;          // row j with the update of reflector j-1 applied
            sw_next[k] = wk;
            svj[k] = r;
            if (k >= j + 2) sig += r * r;
            if (k == j) piv[0] = r;
            if (k == j + 1) piv[1] = r;
        }
        if (j + 1 >= n && tid == 0) piv[1] = 0.0;
        sig = block_sum1<TC_WAVES>(sig, red_g, tid);
        const double dj = piv[0], alpha = piv[1];
        double beta = alpha, tj = 0.0, scale = 0.0;
        if (sig > 0.0) {
            const double nrm = sqrt(alpha * alpha + sig);
            beta = alpha >= 0.0 ? -nrm : nrm;
            tj = (beta - alpha) / beta;
            scale = 1.0 / (alpha - beta);
        }
        for (int k = j + tid; k < n; k += TC_THREADS) svj[k] = (k <= j || tj == 0.0) ? 0.0 : (k == j + 1 ? 1.0 : svj[k] * scale);     // own columns only
        __syncthreads();
        { double* t = sw; sw = sw_next; sw_next = t; }          // sw = w_{j-1} (the y buffer of this column is the w buffer of the next)
        out_d = dj; out_e = beta;                                // (written out by `glast` at the top of the next column, see there)
        tau_p = tj;
        if (prof) { const long long c = wall_clock64(); pt[1] += c - pc; pc = c; }
        // ---- own rows (in LDS): update with reflector j-1, multiply by v_j; the owner of row j+1 publishes it while it is in hand.
        //      The rows still alive (t >= tmin) are dealt over the waves afresh every column -- wave w takes rows tmin + w and
        //      tmin + w + 8 -- so that retired rows do not leave waves idle; the two rows of a wave share the reads of w, v_{j-1}, v_j.
        u64* rbn = m.rowbuf + (size_t)((j + 1) & 1) * 2 * n;
        u64* ybn = m.ybuf + (size_t)(j & 1) * 2 * n;
        const int tmin = j >= g ? (j - g) / G + 1 : 0;                 // first row of this workgroup below the pivot (row j+1, if it is ours, is this one)
        const int ks = (j + 1) & ~1;                                   // first (even) column of the pass; column j, if included, is dead
        for (int t0 = tmin + wave; t0 < cnt; t0 += 2 * TC_WAVES) {
            const int t1 = t0 + TC_WAVES;
            const int i0 = g + G * t0, i1 = g + G * t1;
            const bool a1 = t1 < cnt;
            double* row0 = rows + (size_t)t0 * nv;
            double* row1 = rows + (size_t)(a1 ? t1 : t0) * nv;
            const double vp0 = svp[i0], w0 = sw[i0], vp1 = a1 ? svp[i1] : 0.0, w1 = a1 ? sw[i1] : 0.0;
            const bool pub0 = i0 == j + 1;
            double acc0 = 0.0, acc1 = 0.0;
            for (int kc = ks + 2 * lane; kc - 2 * lane < n; kc += 128 * TC_MB) {       // (wave-uniform trip count)
                dbl2 wk[TC_MB], vpk[TC_MB], vjk[TC_MB], x0[TC_MB], x1[TC_MB];
#pragma unroll
                for (int c = 0; c < TC_MB; ++c) {
                    const int k = min(kc + 128 * c, nv - 2);
                    wk[c] = *(const dbl2*)(sw + k); vpk[c] = *(const dbl2*)(svp + k); vjk[c] = *(const dbl2*)(svj + k);
                    x0[c] = *(const dbl2*)(row0 + k); x1[c] = *(const dbl2*)(row1 + k);
                }
#pragma unroll
                for (int c = 0; c < TC_MB; ++c) {
                    const int k = kc + 128 * c;
                    if (k < n) {                       // (the pad column of an odd n holds zeros in every vector and row: it stays zero)
                        const dbl2 y0 = x0[c] - (vp0 * wk[c] + w0 * vpk[c]), y1 = x1[c] - (vp1 * wk[c] + w1 * vpk[c]);
                        *(dbl2*)(row0 + k) = y0;
                        acc0 += y0.x * vjk[c].x + y0.y * vjk[c].y;          // (v_j is zero in column j)
                        if (pub0) { if (k > j) put_f64(rbn + 2 * (size_t)k, (unsigned)(j + 2), y0.x); if (k + 1 < n) put_f64(rbn + 2 * (size_t)(k + 1), (unsigned)(j + 2), y0.y); }
                        if (a1) { *(dbl2*)(row1 + k) = y1; acc1 += y1.x * vjk[c].x + y1.y * vjk[c].y; }
                    }
                }
            }
            acc0 = wave_sum_fast(acc0); acc1 = wave_sum_fast(acc1);
            const bool withhold = args.fault && mi == 0 && j == 3 && i0 == n - 1;      // (test hook: the last row's y_3 never arrives -> every partner times out)
            if (lane == 0 && !withhold) { put_f64(ybn + 2 * (size_t)i0, (unsigned)(j + 1), acc0); if (a1) put_f64(ybn + 2 * (size_t)i1, (unsigned)(j + 1), acc1); }
        }
        if (prof) { const long long c = wall_clock64(); pt[2] += c - pc; pc = c; }
        __syncthreads();
        if (prof) { const long long c = wall_clock64(); pt[3] += c - pc; pc = c; }
    }
    if (g == glast && n > 0) {                                     // the last column's results (its reflector is the zero vector)
        double* vt = m.VT + (int64_t)(n - 1) * m.ldv;
        for (int k = tid; k < n; k += TC_THREADS) vt[k] = 0.0;
        if (tid == 0) { m.d[n - 1] = out_d; m.tau[n - 1] = tau_p; }
    }
    if (prof) for (int q = 0; q < 4; ++q) args.prof[q] = pt[q] / (n > 0 ? n : 1);
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------
bool g_coop_disabled = false;                       // set once a persistent round has timed out (process-wide)
int32_t g_coop_timeouts = 0;                        // how often that happened

// the matrices `set` by one launch per column, TRID_MAXM of them per chain of launches
dmrgx_status trid_by_launches(const std::vector<int>& set, const std::vector<SymEigMat>& M, const std::vector<SymEigWs>& ws, double* B, hipStream_t st)
{
    for (size_t c0 = 0; c0 < set.size(); c0 += TRID_MAXM) {
        const int cn = (int)std::min<size_t>(TRID_MAXM, set.size() - c0);
        TridArgs ta;
        int gmax = 0;
        for (int i = 0; i < TRID_MAXM; ++i) {
            if (i < cn) { const int q = set[c0 + i]; ta.m[i] = TridMat{M[q].A, B + ws[q].VT, B + ws[q].y, B + ws[q].d, B + ws[q].e, B + ws[q].tau, M[q].n, M[q].lda, M[q].n, 0}; gmax = std::max(gmax, M[q].n); }
            else ta.m[i] = TridMat{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0};
        }
        const size_t lds = (size_t)3 * gmax * sizeof(double);
        DMRGX_CHK(set_dyn_lds(trid_step_kernel, lds));
        const unsigned gx = (unsigned)((gmax + TRID_ROWS - 1) / TRID_ROWS);
        for (int j = 0; j < gmax; ++j) hipLaunchKernelGGL(trid_step_kernel, dim3(gx, (unsigned)cn), dim3(TRID_THREADS), lds, st, ta, j);
    }
    DMRGX_HIP(hipGetLastError());
    return DMRGX_OK;
}

// The persistent rounds of a call.  Matrices whose rows fit the LDS of at most all CUs go through the persistent kernel, in rounds of
// <= #CUs workgroups and <= TRID_MAXM matrices; larger ones through one launch per column.
struct TridRound { std::vector<int> mats, G; int wgs = 0; };      // the matrices of one launch, the workgroups of each, their sum
struct TridPlan { std::vector<TridRound> rounds; std::vector<int> persistent, by_launch; int max_G = 0; };
// orders: n of every matrix; ncu: CUs of the device; dyn_max: bytes of dynamic LDS a workgroup of trid_coop_kernel may ask for
TridPlan trid_plan(const std::vector<int>& orders, int ncu, int64_t dyn_max)
{
    TridPlan plan;
    const int nm = (int)orders.size(), nmax = *std::max_element(orders.begin(), orders.end());
    std::vector<int> order(nm);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return orders[a] > orders[b]; });
    // Workgroups per matrix: at least what LDS capacity asks for.  CUs that this leaves idle go, one at a time, to the matrix with the
    // longest estimated chain -- n columns x (a fixed part + the workgroup's own row pass, which is proportional to rows per workgroup
    // x row length) -- down to `rows_floor` rows per workgroup: the launch lasts as long as its longest chain, a workgroup's row pass
    // is one link of every column of it, and among few workgroups more partners cost the all-gather almost nothing.  (Small m: a dozen
    // matrices of n <= 300 on 256 CUs go from 75 to 8-16 rows per workgroup: 888 -> 672 us per call at m = 512.)
    constexpr int rows_floor = 8;      // (4 and 2 rows per workgroup measured flat, round 3)
    std::vector<int> Gmin(nm, 0), Gof(nm, 0);
    {
        int64_t used = 0;
        for (int q = 0; q < nm; ++q) {
            const int64_t n = orders[q], nv = (n + 1) & ~(int64_t)1, cap = (dyn_max / 8 - TC_VECS * nv) / nv;      // rows of this matrix one workgroup can hold
            Gmin[q] = cap >= 1 ? (int)((n + cap - 1) / cap) : ncu + 1;
            Gof[q] = Gmin[q];
            if (Gmin[q] <= ncu) used += Gmin[q];
        }
        // estimated chain [us]: per column 2.7 fixed (exchange, vector work, barriers) + 1.35 for 18 rows of 1037 columns (measured, m = 2048)
        auto chain = [&](int q) { const double n = orders[q], rows = std::ceil(n / Gof[q]); return n * (2.7 + 1.35 * (rows / 18.0) * (n / 1037.0)); };
        // Only when the largest matrix is itself small: at m = 2048 (n up to 1037, G = 58 by capacity) more workgroups made the call
        // SLOWER on the same box -- 8.49 ms per truncation with none, 8.60 with the spare CUs on the small matrices, 8.62 with them on
        // the largest -- more partners lengthen the exchange there by more than the shorter row pass saves.
        if (used <= ncu && nmax <= 400) {          // (m = 1024, n up to ~520: no difference either way)
            for (int64_t spare = ncu - used; spare > 0; --spare) {
                int best = -1; double tbest = 0;
                for (int q = 0; q < nm; ++q) {
                    if (Gmin[q] > ncu || (orders[q] + Gof[q] - 1) / Gof[q] <= rows_floor) continue;
                    const double t = chain(q);
                    if (best < 0 || t > tbest) { best = q; tbest = t; }
                }
                if (best < 0) break;
                ++Gof[best];
            }
        }
    }
    for (int q : order) {
        const int G = Gof[q];
        if (G > ncu) { plan.by_launch.push_back(q); continue; }
        TridRound* r = nullptr;
        for (TridRound& c : plan.rounds) if (c.wgs + G <= ncu && (int)c.mats.size() < TRID_MAXM) { r = &c; break; }
        if (!r) { plan.rounds.emplace_back(); r = &plan.rounds.back(); }
        r->mats.push_back(q); r->G.push_back(G); r->wgs += G;
        plan.persistent.push_back(q);
        plan.max_G = std::max(plan.max_G, G);
    }
    return plan;
}

// the granule buffers (zeroed on st) and one launch of trid_coop_kernel per round
dmrgx_status trid_persistent_rounds(const TridPlan& plan, int64_t dyn_max, const std::vector<SymEigMat>& M, const std::vector<SymEigWs>& ws, double* B, hipStream_t st, TridRun& run)
{
    int64_t gtot = 2;                                                        // in u64 words; the status word owns the first 16 bytes
    std::vector<int64_t> goff(M.size(), 0);
    for (int q : plan.persistent) { goff[q] = gtot; gtot += 8 * (int64_t)M[q].n; }   // ybuf, rowbuf: 2 parities x n x 2 granules each
    gtot = (gtot + 1) & ~(int64_t)1;
    DMRGX_CHK(run.gran.alloc((size_t)gtot * sizeof(u64)));
    DMRGX_HIP(hipMemsetAsync(run.gran.p, 0, (size_t)gtot * sizeof(u64), st));     // epochs start at 1: a zeroed granule is "not yet"
    u64* GB = run.gran.as<u64>();
    DMRGX_HIP(hipFuncSetAttribute((const void*)trid_coop_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_max));
    if (getenv("DMRGX_TRID_PROF")) { run.prof = B + ws[plan.persistent[0]].y; run.prof_n = M[plan.persistent[0]].n; }
    for (const TridRound& r : plan.rounds) {
        TcArgs ta;
        ta.status = reinterpret_cast<int32_t*>(GB); ta.nm = (int32_t)r.mats.size();
        // test hook (tests/test_gpu_kron.py: the time-out -> launch-per-column transition, once): the first persistent round of the process
        // loses one publication
        static bool fault_pending = getenv("DMRGX_TRID_FAULT") != nullptr;
        ta.fault = fault_pending ? 1 : 0; fault_pending = false;
        ta.prof = run.prof ? reinterpret_cast<long long*>(B + ws[r.mats[0]].y) : nullptr;      // (the y scratch of the launch path is idle here)
        size_t lds = 0;
        int wg0 = 0;
        for (int i = 0; i < TRID_MAXM; ++i) {
            if (i < (int)r.mats.size()) {
                const int q = r.mats[(size_t)i], n = M[q].n, G = r.G[(size_t)i];
                ta.m[i] = TcMat{M[q].A, B + ws[q].VT, B + ws[q].d, B + ws[q].e, B + ws[q].tau, GB + goff[q], GB + goff[q] + 4 * (int64_t)n, n, M[q].lda, n, G, wg0, 0};
                wg0 += G;
                lds = std::max(lds, (size_t)(TC_VECS + (n + G - 1) / G) * (size_t)((n + 1) & ~1) * sizeof(double));
            } else ta.m[i] = TcMat{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 1 << 30, 0};
        }
        hipLaunchKernelGGL(trid_coop_kernel, dim3((unsigned)wg0), dim3(TC_THREADS), lds, st, ta);
        DMRGX_HIP(hipGetLastError());
    }
    run.persistent = true;
    return DMRGX_OK;
}
}  // namespace

void symeig_set_persistent(bool on) { g_coop_disabled = !on; }
void symeig_note_timeout(int32_t status)
{
    if (!g_coop_disabled) fprintf(stderr, status == 2 ? "[dmrgx] persistent tridiagonalisation: a workgroup was lapped by its partners (protocol error): using one launch per column from now on\n"
                                                       : "[dmrgx] persistent tridiagonalisation timed out waiting for a partner workgroup (GPU shared with another "
                                                         "persistent kernel?): using one launch per column from now on\n");
    g_coop_disabled = true;
    ++g_coop_timeouts;
}
int32_t symeig_deferred_timed_out(const SymEigDeferred& d) { return d.status_host ? *d.status_host : 0; }
void symeig_process_state(int32_t* timeouts, int32_t* persistent_off)
{
    if (timeouts) *timeouts = g_coop_timeouts;
    if (persistent_off) *persistent_off = g_coop_disabled ? 1 : 0;
}

dmrgx_status symeig_impl::trid_enqueue(const std::vector<SymEigMat>& M, const std::vector<SymEigWs>& ws, double* B, hipStream_t st, SymEigReport& rep, TridRun& run)
{
    static const bool coop_wanted = !(getenv("DMRGX_TRID") && std::string(getenv("DMRGX_TRID")) == "launch");     // developer aid / A-B
    TridPlan plan;
    if (coop_wanted && !g_coop_disabled) {
        int dev = 0, ncu = 0, max_lds = 0;
        DMRGX_HIP(hipGetDevice(&dev));
        DMRGX_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
        DMRGX_HIP(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
        const int64_t dyn_max = std::min<int64_t>(max_lds, 160 * 1024) - 256;       // (static LDS of the kernel: a few words)
        std::vector<int> orders;
        for (const SymEigMat& m : M) orders.push_back(m.n);
        plan = trid_plan(orders, ncu, dyn_max);
        if (!plan.rounds.empty()) DMRGX_CHK(trid_persistent_rounds(plan, dyn_max, M, ws, B, st, run));
    } else for (int q = 0; q < (int)M.size(); ++q) plan.by_launch.push_back(q);
    if (!plan.by_launch.empty()) DMRGX_CHK(trid_by_launches(plan.by_launch, M, ws, B, st));
    rep.persistent_matrices = (int32_t)plan.persistent.size(); rep.launch_matrices = (int32_t)plan.by_launch.size();
    rep.max_workgroups_per_matrix = plan.max_G;
    return DMRGX_OK;
}

// The status word travels to pinned memory behind the persistent rounds and is looked at by the CALLER behind its own synchronisation (the
// spectra's) -- symeig_deferred_timed_out -- so that everything else is queued while the tridiagonalisation still runs: the divide and conquer
// starts the moment it ends instead of one host hand-over later.  A time-out (never seen outside the test hook and GPUs shared with another
// persistent kernel) then costs the caller a second call, on the launch path.
dmrgx_status symeig_impl::trid_status_to_pinned(const TridRun& run, hipStream_t st, const int32_t*& status_host)
{
    if (!run.persistent) return DMRGX_OK;
    if (run.prof) {
        long long pr[4];
        DMRGX_HIP(hipMemcpy(pr, run.prof, sizeof(pr), hipMemcpyDeviceToHost));
        fprintf(stderr, "[trid-prof] n=%d: wave 0 of workgroup 1, mean per column [us]: consume %.2f  vector work %.2f  own rows %.2f  end barrier %.2f\n", run.prof_n, pr[0] / 100.0, pr[1] / 100.0, pr[2] / 100.0, pr[3] / 100.0);
    }
    static thread_local int32_t* pin_status = nullptr;
    if (!pin_status) DMRGX_HIP(hipHostMalloc((void**)&pin_status, 64, hipHostMallocDefault));
    *pin_status = 0;
    DMRGX_HIP(hipMemcpyAsync(pin_status, run.gran.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    status_host = pin_status;
    return DMRGX_OK;
}

}  // namespace dmrgx
