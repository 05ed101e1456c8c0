// Second phase of the batched symmetric eigensolver (symeig.h; driver: symeig.hip): the spectra of the tridiagonal matrices, and their
// eigenvectors up to the root merge.
//
//  Tridiagonal divide and conquer (Cuppen; the method of LAPACK's dstedc), level-synchronous: uniform-depth tree, leaves <= DC_LEAF
//     solved by Jacobi in LDS, then per level: deflation (dc_deflate_kernel; the only sequential scan), secular roots by the
//     "middle way" iteration in shifted coordinates (one wave per root), Loewner weights and eigenvector columns, and ONE grouped
//     MFMA GEMM  Q_new = blockdiag(Q1, Q2) . U  in which deflated columns are unit columns of U (no gather / scatter kernels) and
//     the deflation rotations are applied to the ROWS of U.  Density matrices of DMRG states deflate almost completely.
//  The GEMM of the root merge is not part of this phase: symeig_finish runs it for the columns the caller keeps.
#include "symeig_impl.h"

namespace dmrgx {
using namespace symeig_impl;
namespace {
constexpr double DC_EPS = DBL_EPSILON;

struct DcMat {
    double* Q[2];                  // eigenvector buffers (block diagonal while the tree is climbed); level l lives in Q[l & 1]
    double* U;                     // the merge matrices of one level (block diagonal)
    const double *d, *e;           // the tridiagonal matrix (unscaled)
    double *dcur, *scale, *w;      // eigenvalues of the current nodes (scaled); the scale factor; output spectrum
    double *dl, *zl, *tau, *lam, *zhat, *cnorm, *dval, *rc, *rs, *mrho;     // per position of the matrix, length n
    int32_t *org, *pcol, *dcol, *rowpole, *colroot, *pcolmap, *rcp, *rcj, *mk, *mrot;
    int32_t n, ldq[2], ldu;
};
struct DcLeaf { int32_t mat, lo, hi, buf; };
struct DcMerge { int32_t mat, lo, mid, hi, src, pad; };

__global__ void __launch_bounds__(256) dc_scale_kernel(const DcMat* __restrict__ mats)
{
    __shared__ double red[4];
    const DcMat m = mats[blockIdx.x];
    double v = 0.0;
    for (int i = threadIdx.x; i < m.n; i += 256) { v = fmax(v, fabs(m.d[i])); if (i + 1 < m.n) v = fmax(v, fabs(m.e[i])); }
    v = block_max<4>(v, red, threadIdx.x);
    if (threadIdx.x == 0) m.scale[0] = v > 0.0 ? v : 1.0;
}

// Leaf: T[lo:hi] with the rank-one couplings to its neighbours taken off the end diagonals (T = diag(T1', T2') + |beta| u u^T,
// u = e_last(1) + sign(beta) e_first(2)), diagonalised by cyclic Jacobi on the dense 32 x 32 array in LDS.
__global__ void __launch_bounds__(DC_LEAF_THREADS) dc_leaf_kernel(const DcMat* __restrict__ mats, const DcLeaf* __restrict__ leaves)
{
    constexpr int P = DC_LEAF, H = P / 2;
    __shared__ double S[P][P + 1], R[P][P + 1];
    __shared__ double rc[H], rs[H];
    __shared__ double red[4];
    __shared__ int rnk[P];
    const DcLeaf lf = leaves[blockIdx.x];
    const DcMat m = mats[lf.mat];
    const int p = lf.hi - lf.lo, tid = threadIdx.x;
    const double inv = 1.0 / m.scale[0];
    for (int e = tid; e < P * P; e += DC_LEAF_THREADS) { const int i = e / P, c = e % P; S[i][c] = 0.0; R[i][c] = i == c ? 1.0 : 0.0; }
    __syncthreads();
    if (tid < p) {
        const int gi = lf.lo + tid;
        double dv = m.d[gi] * inv;
        if (tid == 0 && lf.lo > 0) dv -= fabs(m.e[lf.lo - 1] * inv);
        if (tid == p - 1 && lf.hi < m.n) dv -= fabs(m.e[lf.hi - 1] * inv);
        S[tid][tid] = dv;
        if (tid + 1 < p) { const double ev = m.e[gi] * inv; S[tid][tid + 1] = ev; S[tid + 1][tid] = ev; }
    }
    __syncthreads();
    // round-robin tournament over pe = p rounded up to even players (a leaf of 17 needs 17 rounds of 9 pairs per sweep, not the 31 x 16
    // of the full 32 x 32 array; the odd player out meets the padding index p, whose row and column are zero: no rotation)
    const int pe = (p + 1) & ~1, hp = pe / 2, pm = pe - 1;
    // (pair, index) of the elements this thread rotates in every round: fixed for the whole solve -- the divisions by the run-time pe
    // and the modulo of the pairing were a third of a round's instructions
    constexpr int NE = (H * P + DC_LEAF_THREADS - 1) / DC_LEAF_THREADS;
    int et[NE], ei[NE];
#pragma unroll
    for (int u = 0; u < NE; ++u) { const int e = tid + u * DC_LEAF_THREADS; et[u] = e < hp * pe ? e / pe : -1; ei[u] = e % pe; }
    for (int sweep = 0; sweep < 20; ++sweep) {
        double off = 0.0, dg = 0.0;
        for (int e = tid; e < P * P; e += DC_LEAF_THREADS) { const int i = e / P, c = e % P; const double v = S[i][c]; if (i == c) dg += v * v; else off += v * v; }
        off = block_sum<DC_LEAF_THREADS / 64>(off, red, tid);
        dg = block_sum<DC_LEAF_THREADS / 64>(dg, red, tid);
        if (off <= 2e-31 * dg || off == 0.0) break;          // off-diagonal norm <= 2 eps |T|; uniform over the workgroup
        for (int r = 0; r < pe - 1; ++r) {
            auto pair_of = [&](int t, int& a, int& bq) {          // 0 <= r < pm, 1 <= t < hp: (r + t) mod pm and (r - t) mod pm by one conditional step
                if (t == 0) { a = pm; bq = r; } else { a = r + t; if (a >= pm) a -= pm; bq = r - t; if (bq < 0) bq += pm; }
                if (a > bq) { const int x = a; a = bq; bq = x; }
            };
            if (tid < hp) {                                  // pair tid of round r
                int a, bq;
                pair_of(tid, a, bq);
                const double apq = S[a][bq], app = S[a][a], aqq = S[bq][bq];
                double c = 1.0, s = 0.0;
                if (apq != 0.0) {
                    const double th = 0.5 * (aqq - app) / apq;
                    const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                    c = 1.0 / sqrt(t * t + 1.0); s = t * c;
                }
                rc[tid] = c; rs[tid] = s;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < NE; ++u) {                                 // columns: S <- S J, R <- R J
                const int t = et[u], i = ei[u];
                if (t < 0) continue;
                int a, bq;
                pair_of(t, a, bq);
                const double c = rc[t], s = rs[t];
                const double sp = S[i][a], sq = S[i][bq];
                S[i][a] = c * sp - s * sq; S[i][bq] = s * sp + c * sq;
                const double rp = R[i][a], rq = R[i][bq];
                R[i][a] = c * rp - s * rq; R[i][bq] = s * rp + c * rq;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < NE; ++u) {                                 // rows: S <- J^T S
                const int t = et[u], i = ei[u];
                if (t < 0) continue;
                int a, bq;
                pair_of(t, a, bq);
                const double c = rc[t], s = rs[t];
                const double sp = S[a][i], sq = S[bq][i];
                S[a][i] = c * sp - s * sq; S[bq][i] = s * sp + c * sq;
            }
            __syncthreads();
        }
    }
    // ascending order; the padding indices >= p never mixed with the real ones (their rows and columns are exactly zero)
    if (tid < p) {
        const double v = S[tid][tid];
        int r = 0;
        for (int q = 0; q < p; ++q) { const double u = S[q][q]; r += (u < v) || (u == v && q < tid); }
        rnk[tid] = r;
        m.dcur[lf.lo + r] = v;
    }
    __syncthreads();
    double* Q = m.Q[lf.buf];
    const int ldq = m.ldq[lf.buf];
    for (int e = tid; e < p * p; e += DC_LEAF_THREADS) { const int i = e / p, c = e % p; Q[(int64_t)(lf.lo + i) * ldq + lf.lo + rnk[c]] = R[i][c]; }
}

// (A one-wave implicit-QL leaf -- no barrier at all, the rotation recurrence redundantly in every lane -- was measured in round 3 and ran
//  the same 250 us per call as the Jacobi leaf above; it is not part of the library.)

// Deflation of one merge (LAPACK dlaed2 in this solver's data flow): z from the children's boundary rows, poles ranked by brute-
// force counting (no sortedness assumed), type-1 (rho |z_i| tiny) and type-2 (two close poles: one Givens rotation moves the
// weight to one of them) deflation in one sequential scan by thread 0 -- the only serial part of the solver.
__global__ void __launch_bounds__(1024) dc_deflate_kernel(const DcMat* __restrict__ mats, const DcMerge* __restrict__ merges, int nlmax)
{
    extern __shared__ double sh[];
    double* D = sh;
    double* z = sh + nlmax;
    double* ds = sh + 2 * (size_t)nlmax;
    double* zs = sh + 3 * (size_t)nlmax;
    int* ord = (int*)(sh + 4 * (size_t)nlmax);
    __shared__ double red[32];
    __shared__ int s_unsorted;
    const DcMerge mg = merges[blockIdx.x];
    const DcMat m = mats[mg.mat];
    const int lo = mg.lo, n1 = mg.mid - mg.lo, nl = mg.hi - mg.lo, tid = threadIdx.x;
    const double beta = m.e[mg.mid - 1] / m.scale[0];
    const double rho = 2.0 * fabs(beta), sgn = beta < 0.0 ? -1.0 : 1.0;
    const double* Qs = m.Q[mg.src];
    const int ldq = m.ldq[mg.src];
    const double* row1 = Qs + (int64_t)(mg.mid - 1) * ldq + lo;      // last row of child 1 (columns lo .. mid-1)
    const double* row2 = Qs + (int64_t)mg.mid * ldq + lo;            // first row of child 2 (columns mid .. hi-1)
    double dmax = 0.0, zmax = 0.0;
    for (int i = tid; i < nl; i += 1024) {
        const double dv = m.dcur[lo + i];
        const double zv = (i < n1 ? row1[i] : sgn * row2[i]) * 0.70710678118654752440;
        D[i] = dv; z[i] = zv;
        dmax = fmax(dmax, fabs(dv)); zmax = fmax(zmax, fabs(zv));
        m.rowpole[lo + i] = -1;
    }
    {   // both maxima behind one pair of barriers
        dmax = wave_max(dmax); zmax = wave_max(zmax);
        if (tid == 0) s_unsorted = 0;
        __syncthreads();
        if ((tid & 63) == 0) { red[tid >> 6] = dmax; red[16 + (tid >> 6)] = zmax; }
        __syncthreads();
        dmax = red[0]; zmax = red[16];
#pragma unroll
        for (int w = 1; w < 16; ++w) { dmax = fmax(dmax, red[w]); zmax = fmax(zmax, red[16 + w]); }
    }
    // Rank of every pole in the union (ties by index).  The children's spectra are sorted ascending -- dc_leaf / dc_norm_rank write them
    // by rank -- so an entry's rank is its own position plus the number of the OTHER child's entries in front of it: a binary search
    // instead of nl comparisons (13 us of a launch at nl = 300, 160 at nl = 1062).  Verified, not assumed: a child that is not
    // sorted sends the merge through the brute-force count.
    for (int i = tid; i + 1 < nl; i += 1024) if (i + 1 != n1 && D[i] > D[i + 1]) s_unsorted = 1;
    __syncthreads();
    if (!s_unsorted) {
        for (int i = tid; i < nl; i += 1024) {
            const double di = D[i];
            int a, b, r;
            if (i < n1) { a = n1; b = nl; while (a < b) { const int c = (a + b) >> 1; if (D[c] < di) a = c + 1; else b = c; } r = i + (a - n1); }       // ties: the other child's index is larger
            else { a = 0; b = n1; while (a < b) { const int c = (a + b) >> 1; if (D[c] <= di) a = c + 1; else b = c; } r = (i - n1) + a; }             // ties: ... is smaller
            ord[r] = i;
        }
    } else {
        for (int i = tid; i < nl; i += 1024) {
            const double di = D[i];
            int r = 0;
            for (int q = 0; q < nl; ++q) { const double dq = D[q]; r += (dq < di) || (dq == di && q < i); }
            ord[r] = i;
        }
    }
    __syncthreads();
    for (int s = tid; s < nl; s += 1024) { const int c = ord[s]; ds[s] = D[c]; zs[s] = z[c]; }
    __syncthreads();
    const double tol = 8.0 * DC_EPS * fmax(dmax, zmax);
    // ---- fast path: no pair of neighbouring poles needs a type-2 rotation (the usual case without exact degeneracies), so the
    //      deflation scan has no sequential dependence: type-1 flags, a prefix count, and every pole / deflated entry written by
    //      its own thread.  One neighbour pair that would rotate sends the whole merge through the sequential scan below.
    int* pre = ord + nlmax;                               // exclusive count of non-deflated entries in front of sorted position s
    int* nf = pre + nlmax;                                // sorted positions of the non-deflated entries, in order
    __shared__ int wtot[16], s_any2, s_k;
    const bool all_defl = rho * zmax <= tol;
    {
        const int per = (nl + 1023) / 1024, s0 = tid * per;
        int c = 0;
        for (int u = 0; u < per; ++u) { const int sp = s0 + u; if (sp < nl && !(all_defl || rho * fabs(zs[sp]) <= tol)) ++c; }
        int inc = c;
        for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o, 64); if ((tid & 63) >= o) inc += v; }
        if ((tid & 63) == 63) wtot[tid >> 6] = inc;
        if (tid == 0) s_any2 = 0;
        __syncthreads();
        int base = 0;
        for (int w = 0; w < (tid >> 6); ++w) base += wtot[w];
        int run = base + inc - c;
        for (int u = 0; u < per; ++u) {
            const int sp = s0 + u;
            if (sp >= nl) break;
            pre[sp] = run;
            if (!(all_defl || rho * fabs(zs[sp]) <= tol)) { nf[run] = sp; ++run; }
        }
        if (tid == 1023) s_k = run;
        __syncthreads();
    }
    const int kfast = s_k;
    for (int p = 1 + tid; p < kfast; p += 1024) {         // would the scan rotate the pair (nf[p-1], nf[p])?
        const int a = nf[p - 1], b = nf[p];
        double s_ = zs[a], c_ = zs[b];
        const double tau = hypot(c_, s_), t = ds[b] - ds[a];
        c_ /= tau; s_ = -s_ / tau;
        if (fabs(t * c_ * s_) <= tol) s_any2 = 1;
    }
    __syncthreads();
    if (!s_any2) {
        for (int sp = tid; sp < nl; sp += 1024) {
            const bool d1 = all_defl || rho * fabs(zs[sp]) <= tol;
            const int c = ord[sp];
            if (d1) { const int t = sp - pre[sp]; m.dval[lo + t] = ds[sp]; m.dcol[lo + t] = c; }
            else { const int kk = pre[sp]; m.dl[lo + kk] = ds[sp]; m.zl[lo + kk] = zs[sp]; m.pcol[lo + kk] = c; m.rowpole[lo + c] = kk; }
        }
        if (tid == 0) { m.mk[lo] = kfast; m.mrot[lo] = 0; m.mrho[lo] = rho; }
        return;
    }
    // ---- sequential scan (thread 0), everything it touches in LDS and the pole it carries in registers: the test
    //      |t c s| <= tol with c = z_jj / tau, s = z_pj / tau is done as |t z_jj z_pj| <= tol tau^2 (no square root, no division
    //      unless the pair really rotates); the lists go to memory in parallel afterwards.
    int* polepos = pre;                                  // (the fast path's arrays are free again)
    int* deflpos = nf;
    int* rcp_s = nf + nlmax;
    int* rcj_s = rcp_s + nlmax;
    double* rc_s = D;                                     // D and z were consumed when ds / zs were built
    double* rs_s = z;
    __shared__ int s_nd, s_nrot;
    if (tid == 0) {
        int k = 0, nd = 0, nrot = 0, pj = -1;
        double zpj = 0.0, dpj = 0.0;
        auto step = [&](int jj, double zj, double dj) {
            if (rho * fabs(zj) <= tol) { deflpos[nd++] = jj; return; }
            if (pj < 0) { pj = jj; zpj = zj; dpj = dj; return; }
            const double tau2 = zj * zj + zpj * zpj, t = dj - dpj;
            if (fabs(t * zj * zpj) <= tol * tau2) {
                const double tau = sqrt(tau2), c_ = zj / tau, s_ = -zpj / tau;
                rcp_s[nrot] = ord[pj]; rcj_s[nrot] = ord[jj]; rc_s[nrot] = c_; rs_s[nrot] = s_; ++nrot;
                const double tt = dpj * c_ * c_ + dj * s_ * s_;
                const double dnew = dpj * s_ * s_ + dj * c_ * c_;
                ds[pj] = tt; zs[pj] = 0.0;
                deflpos[nd++] = pj;
                pj = jj; zpj = tau; dpj = dnew;
                ds[jj] = dnew; zs[jj] = tau;
            } else { polepos[k++] = pj; pj = jj; zpj = zj; dpj = dj; }
        };
        // four entries requested together (the scan only ever writes positions it has passed): one LDS round trip per four entries (eight: no further gain)
        // instead of one per entry -- the scan is a chain of such round trips (~45 ns per entry before)
        int jj = 0;
        for (; jj + 4 <= nl; jj += 4) {
            const double z0 = zs[jj], z1 = zs[jj + 1], z2 = zs[jj + 2], z3 = zs[jj + 3];
            const double d0 = ds[jj], d1 = ds[jj + 1], d2 = ds[jj + 2], d3 = ds[jj + 3];
            step(jj, z0, d0); step(jj + 1, z1, d1); step(jj + 2, z2, d2); step(jj + 3, z3, d3);
        }
        for (; jj < nl; ++jj) step(jj, zs[jj], ds[jj]);
        polepos[k++] = pj;
        s_k = k; s_nd = nd; s_nrot = nrot;
    }
    __syncthreads();
    const int k = s_k, nd = s_nd, nrot = s_nrot;
    for (int p = tid; p < k; p += 1024) { const int sp = polepos[p], c = ord[sp]; m.dl[lo + p] = ds[sp]; m.zl[lo + p] = zs[sp]; m.pcol[lo + p] = c; m.rowpole[lo + c] = p; }
    for (int t = tid; t < nd; t += 1024) { const int sp = deflpos[t]; m.dval[lo + t] = ds[sp]; m.dcol[lo + t] = ord[sp]; }
    for (int t = tid; t < nrot; t += 1024) { m.rcp[lo + t] = rcp_s[t]; m.rcj[lo + t] = rcj_s[t]; m.rc[lo + t] = rc_s[t]; m.rs[lo + t] = rs_s[t]; }
    if (tid == 0) { m.mk[lo] = k; m.mrot[lo] = nrot; m.mrho[lo] = rho; }
}

// Root j of  1 + rho sum_i z_i^2 / (d_i - lambda)  between d_j and d_{j+1} (the last one: right of d_{k-1}), one wave per root.
// The unknown is tau = lambda - d_origin with the origin at the nearer pole; the iteration interpolates the poles left of the
// root by s + a / (p - tau) and the ones right of it by r + b / (q - tau) with value and slope matched ("middle way"), and falls
// back to bisection of the bracket whenever the model's root leaves it.
__global__ void __launch_bounds__(256) dc_secular_kernel(const DcMat* __restrict__ mats, const DcMerge* __restrict__ merges, int nlmax)
{
    extern __shared__ double sh[];
    double* dl = sh;
    double* z2 = sh + nlmax;
    const DcMerge mg = merges[blockIdx.y];
    const DcMat m = mats[mg.mat];
    const int lo = mg.lo, k = m.mk[lo], tid = threadIdx.x, lane = tid & 63;
    if ((int)blockIdx.x * 4 >= k) return;
    for (int i = tid; i < k; i += 256) { dl[i] = m.dl[lo + i]; const double zv = m.zl[lo + i]; z2[i] = zv * zv; }
    __syncthreads();
    const int j = blockIdx.x * 4 + (tid >> 6);
    if (j >= k) return;
    const double rho = m.mrho[lo];
    int o = 0;
    double tau;
    if (k == 1) tau = rho * z2[0];
    else {
        const bool last = j == k - 1;
        int p0, p1;
        double lo_b, hi_b;
        if (last) {
            double s = 0.0;
            for (int i = lane; i < k; i += 64) s += z2[i];
            const double width = rho * wave_sum(s), mid = 0.5 * width;
            o = j; p0 = j - 1; p1 = j;
            const double dorg = dl[o];
            double g = 0.0;
            for (int i = lane; i < k; i += 64) g += z2[i] / ((dl[i] - dorg) - mid);
            g = 1.0 + rho * wave_sum(g);
            if (g <= 0.0) { lo_b = mid; hi_b = width; } else { lo_b = 0.0; hi_b = mid; }
        } else {
            const double width = dl[j + 1] - dl[j], mid = 0.5 * width;
            p0 = j; p1 = j + 1;
            const double dj = dl[j];
            double g = 0.0;
            for (int i = lane; i < k; i += 64) g += z2[i] / ((dl[i] - dj) - mid);
            g = 1.0 + rho * wave_sum(g);
            if (g >= 0.0) { o = j; lo_b = 0.0; hi_b = mid; } else { o = j + 1; lo_b = -mid; hi_b = 0.0; }
        }
        const double dorg = dl[o];
        const double p = dl[p0] - dorg, q = dl[p1] - dorg;
        const int nlft = p0 + 1;
        tau = 0.5 * (lo_b + hi_b);
        for (int it = 0; it < 100; ++it) {
            double sg = 0.0, sa = 0.0, psi = 0.0, dpsi = 0.0, phi = 0.0, dphi = 0.0;
            for (int i = lane; i < k; i += 64) {
                const double den = (dl[i] - dorg) - tau;
                const double t = rho * z2[i] / den, dt = t / den;
                sg += t; sa += fabs(t);
                if (i < nlft) { psi += t; dpsi += dt; } else { phi += t; dphi += dt; }
            }
            sg = wave_sum(sg); sa = wave_sum(sa); psi = wave_sum(psi); dpsi = wave_sum(dpsi); phi = wave_sum(phi); dphi = wave_sum(dphi);
            const double g = 1.0 + sg;
            if (fabs(g) <= DC_EPS * (8.0 * sa + 1.0)) break;
            if (g > 0.0) hi_b = tau; else lo_b = tau;
            if (hi_b - lo_b <= 2.0 * DC_EPS * fmax(fabs(lo_b), fabs(hi_b))) break;
            const double a = dpsi * (p - tau) * (p - tau), sc = psi - dpsi * (p - tau);
            const double b = dphi * (q - tau) * (q - tau), rcst = phi - dphi * (q - tau);
            const double c = 1.0 + sc + rcst;
            const double A2 = c, B2 = -(c * (p + q) + a + b), C2 = c * p * q + a * q + b * p;      // c (p-t)(q-t) + a (q-t) + b (p-t) = 0
            double t1 = 0.5 * (lo_b + hi_b), t2 = t1;
            bool h1 = false, h2 = false;
            if (A2 == 0.0) { if (B2 != 0.0) { t1 = -C2 / B2; h1 = true; } }
            else {
                const double disc = B2 * B2 - 4.0 * A2 * C2;
                if (disc >= 0.0) {
                    const double sq = sqrt(disc), qq = -0.5 * (B2 + (B2 >= 0.0 ? sq : -sq));
                    if (qq != 0.0) { t1 = C2 / qq; h1 = true; }
                    t2 = qq / A2; h2 = true;
                }
            }
            if (h1 && t1 > lo_b && t1 < hi_b) tau = t1;
            else if (h2 && t2 > lo_b && t2 < hi_b) tau = t2;
            else tau = 0.5 * (lo_b + hi_b);
        }
    }
    if (lane == 0) { m.org[lo + j] = o; m.tau[lo + j] = tau; m.lam[lo + j] = dl[o] + tau; }
}

// Loewner weights (Gu / Eisenstat: the z for which the computed roots are the exact eigenvalues -- this is what makes the
// eigenvector columns orthogonal to round-off).  k^2 work per merge: DC_SPLIT workgroups per merge, 16 lanes per pole.
constexpr int DC_SPLIT = 8;
__device__ __forceinline__ double prod16(double v)          // product over the 16 lanes of a row, in every lane
{
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v *= __shfl_xor(v, o, 16);
    return v;
}
__device__ __forceinline__ double sum16(double v)
{
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
    return v;
}
// |zhat_i|^2 of pole i, formed by the 16 lanes q = 0 .. 15 of a group (every lane of the group must call it)
__device__ __forceinline__ double loewner_weight(int i, int k, int q, const double* dl, const double* od, const double* tau)
{
    const double di = dl[i];
    double w = q == 0 ? (di - od[i]) - tau[i] : 1.0;
    for (int j = q; j < k; j += 16) if (j != i) w *= ((di - od[j]) - tau[j]) / (di - dl[j]);
    return prod16(w);
}
__global__ void __launch_bounds__(1024) dc_zhat_kernel(const DcMat* __restrict__ mats, const DcMerge* __restrict__ merges, int nlmax)
{
    extern __shared__ double sh[];
    double* dl = sh;
    double* od = sh + nlmax;                  // d_origin(j)
    double* tau = sh + 2 * (size_t)nlmax;
    const DcMerge mg = merges[blockIdx.y];
    const DcMat m = mats[mg.mat];
    const int lo = mg.lo, k = m.mk[lo], tid = threadIdx.x;
    if ((int)blockIdx.x * 64 >= k) return;
    for (int j = tid; j < k; j += 1024) { dl[j] = m.dl[lo + j]; tau[j] = m.tau[lo + j]; }
    __syncthreads();
    for (int j = tid; j < k; j += 1024) od[j] = dl[m.org[lo + j]];
    __syncthreads();
    const int ps = tid >> 4, q = tid & 15;
    for (int i0 = blockIdx.x * 64; i0 < k; i0 += DC_SPLIT * 64) {     // (uniform trip count: the shuffles below need all 16 lanes of a pole)
        const int i = min(i0 + ps, k - 1);
        const double w = loewner_weight(i, k, q, dl, od, tau);
        if (q == 0 && i0 + ps < k) m.zhat[lo + i] = copysign(sqrt(fabs(w)), m.zl[lo + i]);
    }
}

// column norms of the merge's eigenvector block, and the final order of the node's eigenvalues.
// WITH_ZHAT (small merges, nl <= DC_FUSE_NL: one launch instead of two): every workgroup of the merge forms ALL Loewner weights of the merge
// itself first -- k^2 / 16 divisions per thread group instead of an eighth of them, which is cheaper than the ~10 us a launch costs
// before it computes anything (profiles/r05_rdm_call_kernel_sequence_m2048.txt); same arithmetic, same results as dc_zhat_kernel + this.
constexpr int DC_FUSE_NL = 384;
template <bool WITH_ZHAT>
__global__ void __launch_bounds__(1024) dc_norm_rank_kernel(const DcMat* __restrict__ mats, const DcMerge* __restrict__ merges, int nlmax)
{
    extern __shared__ double sh[];
    double* dl = sh;
    double* zh = sh + nlmax;
    double* val = sh + 2 * (size_t)nlmax;
    double* od = sh + 3 * (size_t)nlmax;      // (WITH_ZHAT only: d_origin(j) and tau_j)
    double* tau = sh + 4 * (size_t)nlmax;
    const DcMerge mg = merges[blockIdx.y];
    const DcMat m = mats[mg.mat];
    const int lo = mg.lo, nl = mg.hi - mg.lo, k = m.mk[lo], tid = threadIdx.x;
    if ((int)blockIdx.x * 64 >= nl) return;
    const int ps = tid >> 4, q = tid & 15;
    for (int j = tid; j < k; j += 1024) { dl[j] = m.dl[lo + j]; if (WITH_ZHAT) tau[j] = m.tau[lo + j]; else zh[j] = m.zhat[lo + j]; }
    for (int x = tid; x < nl; x += 1024) val[x] = x < k ? m.lam[lo + x] : m.dval[lo + x - k];
    __syncthreads();
    if (WITH_ZHAT) {
        for (int j = tid; j < k; j += 1024) od[j] = dl[m.org[lo + j]];
        __syncthreads();
        for (int i0 = 0; i0 < k; i0 += 64) {                           // (uniform trip count: the shuffles need all 16 lanes of a pole)
            const int i = min(i0 + ps, k - 1);
            const double w = loewner_weight(i, k, q, dl, od, tau);
            if (q == 0 && i0 + ps < k) {
                const double zv = copysign(sqrt(fabs(w)), m.zl[lo + i]);
                zh[i] = zv;
                if (blockIdx.x == 0) m.zhat[lo + i] = zv;              // (dc_fill_u reads it)
            }
        }
        __syncthreads();
    }
    for (int j0 = blockIdx.x * 64; j0 < k; j0 += DC_SPLIT * 64) {
        const int j = min(j0 + ps, k - 1);
        const double oj = dl[m.org[lo + j]], tj = m.tau[lo + j];
        double s = 0.0;
        for (int i = q; i < k; i += 16) { const double t = zh[i] / ((dl[i] - oj) - tj); s += t * t; }
        s = sum16(s);
        if (q == 0 && j0 + ps < k) m.cnorm[lo + j] = 1.0 / sqrt(s);
    }
    for (int x0 = blockIdx.x * 64; x0 < nl; x0 += DC_SPLIT * 64) {
        const int x = min(x0 + ps, nl - 1);
        const double v = val[x];
        int r = 0;
        for (int p = q; p < nl; p += 16) { const double u = val[p]; r += (u < v) || (u == v && p < x); }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) r += __shfl_xor(r, o, 16);
        if (q == 0 && x0 + ps < nl) {
            m.dcur[lo + r] = v;
            m.colroot[lo + r] = x < k ? x : -(x - k) - 1;
            if (x >= k) m.pcolmap[lo + m.dcol[lo + x - k]] = r;
        }
    }
}

// U (node block): column of root j = zhat_i / (d_i - lambda_j), normalised, in the rows of the non-deflated poles; column of a
// deflated pole = the unit vector of its old column.  64 x 64 elements per workgroup.
__global__ void __launch_bounds__(256) dc_fill_u_kernel(const DcMat* __restrict__ mats, const DcMerge* __restrict__ merges)
{
    __shared__ int rp[64];
    __shared__ double rz[64], rd[64];
    const DcMerge mg = merges[blockIdx.z];
    const DcMat m = mats[mg.mat];
    const int lo = mg.lo, nl = mg.hi - mg.lo, tid = threadIdx.x;
    const int c = blockIdx.x * 64 + (tid & 63), rbase = blockIdx.y * 64;
    if ((int)blockIdx.x * 64 >= nl || rbase >= nl) return;
    if (tid < 64) {
        const int r = rbase + tid;
        int i = -1;
        if (r < nl) i = m.rowpole[lo + r];
        rp[tid] = i;
        if (i >= 0) { rz[tid] = m.zhat[lo + i]; rd[tid] = m.dl[lo + i]; }
    }
    __syncthreads();
    if (c >= nl) return;
    const int cr = m.colroot[lo + c];
    double od = 0.0, tj = 0.0, cn = 0.0;
    int dcolv = -1;
    if (cr >= 0) { od = m.dl[lo + m.org[lo + cr]]; tj = m.tau[lo + cr]; cn = m.cnorm[lo + cr]; }
    else dcolv = m.dcol[lo - cr - 1];
    for (int rr = tid >> 6; rr < 64; rr += 4) {
        const int r = rbase + rr;
        if (r >= nl) break;
        double v;
        if (cr >= 0) v = rp[rr] >= 0 ? rz[rr] / ((rd[rr] - od) - tj) * cn : 0.0;
        else v = dcolv == r ? 1.0 : 0.0;
        m.U[(int64_t)(lo + r) * m.ldu + lo + c] = v;
    }
}

// The type-2 deflation rotations act on columns of blockdiag(Q1, Q2); Q G U' = Q (G U'), so they are applied to the ROWS of U
// instead, in reverse order, one thread per column of U.  A chain pj_1 -> jj_1 = pj_2 -> jj_2 .. is a register recurrence: the
// row of a deflated pole is still the unit row of its final column when its rotation is reached, so nothing but the survivor's
// row is ever loaded.
__global__ void __launch_bounds__(256) dc_rot_kernel(const DcMat* __restrict__ mats, const DcMerge* __restrict__ merges, int nlmax)
{
    extern __shared__ double sh[];
    double* rc = sh;
    double* rs = sh + nlmax;
    int* rcp = (int*)(sh + 2 * (size_t)nlmax);
    int* rcj = rcp + nlmax;
    int* pmap = rcj + nlmax;
    const DcMerge mg = merges[blockIdx.y];
    const DcMat m = mats[mg.mat];
    const int lo = mg.lo, nl = mg.hi - mg.lo, nrot = m.mrot[lo], tid = threadIdx.x;
    if (nrot == 0 || (int)blockIdx.x * 256 >= nl) return;
    for (int t = tid; t < nrot; t += 256) { rc[t] = m.rc[lo + t]; rs[t] = m.rs[lo + t]; const int cp = m.rcp[lo + t]; rcp[t] = cp; rcj[t] = m.rcj[lo + t]; pmap[t] = m.pcolmap[lo + cp]; }
    __syncthreads();
    const int p = blockIdx.x * 256 + tid;
    if (p >= nl) return;
    double* Ucol = m.U + (int64_t)lo * m.ldu + lo + p;
    int t = nrot - 1;
    while (t >= 0) {
        double R = Ucol[(int64_t)rcj[t] * m.ldu];
        bool cont;
        do {
            const double e = pmap[t] == p ? 1.0 : 0.0, c = rc[t], s = rs[t];
            Ucol[(int64_t)rcj[t] * m.ldu] = s * e + c * R;
            R = c * e - s * R;
            cont = t > 0 && rcj[t - 1] == rcp[t];
            if (!cont) Ucol[(int64_t)rcp[t] * m.ldu] = R;
            --t;
        } while (cont);
    }
}

__global__ void __launch_bounds__(256) dc_out_kernel(const DcMat* __restrict__ mats)
{
    const DcMat m = mats[blockIdx.y];
    const double sc = m.scale[0];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < m.n; i += gridDim.x * 256) m.w[i] = m.dcur[i] * sc;
}
}  // namespace

void symeig_impl::dc_add_tables(const std::vector<SymEigMat>& M, const std::vector<SymEigWs>& ws, double* B, int32_t* I, GemmBatch& gemms, PackedUpload& pk, DcTables& out)
{
    const int nm = (int)M.size();
    std::vector<DcMat> dm(nm);
    std::vector<DcLeaf> leaves;
    int dmax = 0;
    for (int i = 0; i < nm; ++i) {
        const int n = M[i].n, D = ws[i].depth;
        const SymEigWs& w = ws[i];
        dmax = std::max(dmax, D);
        DcMat& q = dm[i];
        q.Q[0] = M[i].X; q.ldq[0] = M[i].ldx;
        q.Q[1] = B + w.Q1; q.ldq[1] = n;
        q.U = B + w.U; q.ldu = n;
        q.d = B + w.d; q.e = B + w.e; q.dcur = B + w.dcur; q.scale = B + w.scale; q.w = M[i].w;
        double* v = B + w.vecs;
        q.dl = v; q.zl = v + n; q.tau = v + 2 * (int64_t)n; q.lam = v + 3 * (int64_t)n; q.zhat = v + 4 * (int64_t)n; q.cnorm = v + 5 * (int64_t)n;
        q.dval = v + 6 * (int64_t)n; q.rc = v + 7 * (int64_t)n; q.rs = v + 8 * (int64_t)n; q.mrho = v + 9 * (int64_t)n;
        int32_t* iv = I + w.ints;
        q.org = iv; q.pcol = iv + n; q.dcol = iv + 2 * (int64_t)n; q.rowpole = iv + 3 * (int64_t)n; q.colroot = iv + 4 * (int64_t)n; q.pcolmap = iv + 5 * (int64_t)n;
        q.rcp = iv + 6 * (int64_t)n; q.rcj = iv + 7 * (int64_t)n; q.mk = iv + 8 * (int64_t)n; q.mrot = iv + 9 * (int64_t)n;
        q.n = n;
        const std::vector<int> b = tree_bounds(n, D);
        for (size_t t = 0; t + 1 < b.size(); ++t) leaves.push_back(DcLeaf{i, b[t], b[t + 1], D & 1});
    }
    out.levels.assign((size_t)dmax, DcLevel());
    std::vector<DcMerge> merges;
    for (int t = 1; t <= dmax; ++t) {
        DcLevel& s = out.levels[(size_t)t - 1];
        s.merge_off = merges.size();
        for (int i = 0; i < nm; ++i) {
            if (ws[i].depth < t) continue;
            const int lev = ws[i].depth - t, n = M[i].n;        // the level being produced; its children live at lev + 1
            const std::vector<int> pb = tree_bounds(n, lev), cb = tree_bounds(n, lev + 1);
            const int src = (lev + 1) & 1, dst = lev & 1;
            for (size_t u = 0; u + 1 < pb.size(); ++u) {
                const int lo = pb[u], mid = cb[2 * u + 1], hi = pb[u + 1];
                merges.push_back(DcMerge{i, lo, mid, hi, src, 0});
                s.nlmax = std::max(s.nlmax, hi - lo);
                if (lev == 0) continue;                             // the root's GEMM: symeig_finish, for the kept columns only
                double* Qd = dm[i].Q[dst]; const int ldd = dm[i].ldq[dst];
                const double* Qs = dm[i].Q[src]; const int lds_ = dm[i].ldq[src];
                const double* U = dm[i].U; const int ldu = dm[i].ldu;
                gemms.gemm(s.gemm, Qd + (int64_t)lo * ldd + lo, ldd, mid - lo, hi - lo, Qs + (int64_t)lo * lds_ + lo, lds_, U + (int64_t)lo * ldu + lo, ldu, mid - lo);
                gemms.gemm(s.gemm, Qd + (int64_t)mid * ldd + lo, ldd, hi - mid, hi - lo, Qs + (int64_t)mid * lds_ + mid, lds_, U + (int64_t)mid * ldu + lo, ldu, hi - mid);
            }
        }
        s.nmerge = (int)(merges.size() - s.merge_off);
        gemms.pack(s.gemm, pk);
    }
    if (merges.empty()) merges.push_back(DcMerge{0, 0, 0, 0, 0, 0});
    out.o_mats = pk.add(dm); out.o_leaves = pk.add(leaves); out.o_merges = pk.add(merges);
    out.nleaves = (int)leaves.size();
}

dmrgx_status symeig_impl::dc_launch(const DcTables& t, int nm, int nmax, const GemmBatch& gemms, const DevBuf& d_tab, hipStream_t st)
{
    const DcMat* ddm = packed_at<DcMat>(d_tab, t.o_mats);
    hipLaunchKernelGGL(dc_scale_kernel, dim3((unsigned)nm), dim3(256), 0, st, ddm);
    hipLaunchKernelGGL(dc_leaf_kernel, dim3((unsigned)t.nleaves), dim3(DC_LEAF_THREADS), 0, st, ddm, packed_at<DcLeaf>(d_tab, t.o_leaves));
    DMRGX_HIP(hipGetLastError());
    for (const DcLevel& s : t.levels) {
        if (s.nmerge == 0) continue;
        const DcMerge* mp = packed_at<DcMerge>(d_tab, t.o_merges) + s.merge_off;
        const int nl = s.nlmax;
        const size_t lds_defl = (size_t)nl * (4 * sizeof(double) + 5 * sizeof(int)) + 16;
        const size_t lds_sec = (size_t)nl * 2 * sizeof(double);
        const size_t lds_wgt = (size_t)nl * 3 * sizeof(double);
        const size_t lds_rot = (size_t)nl * (2 * sizeof(double) + 3 * sizeof(int)) + 16;
        DMRGX_CHK(set_dyn_lds(dc_deflate_kernel, lds_defl)); DMRGX_CHK(set_dyn_lds(dc_secular_kernel, lds_sec));
        const bool fuse_wgt = nl <= DC_FUSE_NL;
        const size_t lds_fused = (size_t)nl * 5 * sizeof(double);
        if (fuse_wgt) DMRGX_CHK(set_dyn_lds(dc_norm_rank_kernel<true>, lds_fused));
        else { DMRGX_CHK(set_dyn_lds(dc_zhat_kernel, lds_wgt)); DMRGX_CHK(set_dyn_lds(dc_norm_rank_kernel<false>, lds_wgt)); }
        DMRGX_CHK(set_dyn_lds(dc_rot_kernel, lds_rot));
        hipLaunchKernelGGL(dc_deflate_kernel, dim3((unsigned)s.nmerge), dim3(1024), lds_defl, st, ddm, mp, nl);
        hipLaunchKernelGGL(dc_secular_kernel, dim3((unsigned)((nl + 3) / 4), (unsigned)s.nmerge), dim3(256), lds_sec, st, ddm, mp, nl);
        if (fuse_wgt) hipLaunchKernelGGL(dc_norm_rank_kernel<true>, dim3(DC_SPLIT, (unsigned)s.nmerge), dim3(1024), lds_fused, st, ddm, mp, nl);
        else {
            hipLaunchKernelGGL(dc_zhat_kernel, dim3(DC_SPLIT, (unsigned)s.nmerge), dim3(1024), lds_wgt, st, ddm, mp, nl);
            hipLaunchKernelGGL(dc_norm_rank_kernel<false>, dim3(DC_SPLIT, (unsigned)s.nmerge), dim3(1024), lds_wgt, st, ddm, mp, nl);
        }
        hipLaunchKernelGGL(dc_fill_u_kernel, dim3((unsigned)((nl + 63) / 64), (unsigned)((nl + 63) / 64), (unsigned)s.nmerge), dim3(256), 0, st, ddm, mp);
        hipLaunchKernelGGL(dc_rot_kernel, dim3((unsigned)((nl + 255) / 256), (unsigned)s.nmerge), dim3(256), lds_rot, st, ddm, mp, nl);
        DMRGX_HIP(hipGetLastError());
        DMRGX_CHK(gemms.launch(s.gemm, d_tab, st));
    }
    hipLaunchKernelGGL(dc_out_kernel, dim3((unsigned)((nmax + 255) / 256), (unsigned)nm), dim3(256), 0, st, ddm);
    DMRGX_HIP(hipGetLastError());
    return DMRGX_OK;
}

}  // namespace dmrgx
