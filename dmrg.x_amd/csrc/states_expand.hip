// dmrgx_kron_states_expand: several states of one sector set side by side, KronBlock by KronBlock, each scaled by the square root of its
// weight, so that the density matrix of the expansion is the state-averaged one,
//   side 0:  Psi'_k = [ sqrt(w_0) Psi_0,k | sqrt(w_1) Psi_1,k | ... ],   Psi' Psi'^T = sum_s w_s rho_L,s
//   side 1:  the panels stacked as rows,                                 Psi''^T Psi'' = sum_s w_s rho_R,s
// and the density-matrix solver needs nothing but wider sector tables (dmrgx_rdm_create_subset, as for dmrgx_kron_noise_expand).
// One strided scaled-copy kernel over all (KronBlock, state) panels: a panel's source is contiguous (a KronBlock slice of one state), its
// destination has the expanded leading dimension.  No atomics, every element written once.
#include "krylov.h"
#include <cmath>
#include <set>

namespace dmrgx {
namespace {

constexpr int SX_THREADS = 256, SX_BLOCKS = 64;

// count = nr * nc doubles at src (row-major, leading dimension nc) to dst (leading dimension ldd), times scale.  vec: nc and ldd are even
// and both corners 16-byte aligned, so every pair of a row is a 16-byte pair on both sides
struct SxPanel { const double* src; double* dst; int64_t ldd, count; int32_t nc, vec; double scale; };

__device__ __forceinline__ double sx_scaled(double v, double scale) { return scale == 1.0 ? v : v * scale; }

// blockIdx.y: the panel.  A scale of exactly 1 copies the bits, a scale of exactly 0 writes zeros and reads nothing.
__global__ void __launch_bounds__(SX_THREADS) sx_copy_kernel(const SxPanel* __restrict__ panels)
{
    const SxPanel p = panels[blockIdx.y];
    const bool zero = p.scale == 0.0;
    const int64_t first = (int64_t)blockIdx.x * SX_THREADS + threadIdx.x, step = (int64_t)gridDim.x * SX_THREADS;
    if (p.vec) {
        const int64_t ncp = p.nc / 2;
        for (int64_t q = first; q < p.count / 2; q += step) {
            const int64_t i = q / ncp, c = 2 * (q - i * ncp);
            double2 v = double2{0.0, 0.0};
            if (!zero) { v = *reinterpret_cast<const double2*>(p.src + 2 * q); v.x = sx_scaled(v.x, p.scale); v.y = sx_scaled(v.y, p.scale); }
            *reinterpret_cast<double2*>(p.dst + i * p.ldd + c) = v;
        }
    } else {
        for (int64_t q = first; q < p.count; q += step) {
            const int64_t i = q / p.nc, c = q - i * p.nc;
            p.dst[i * p.ldd + c] = zero ? 0.0 : sx_scaled(p.src[q], p.scale);
        }
    }
}

}  // namespace
}  // namespace dmrgx

using namespace dmrgx;

extern "C" dmrgx_status dmrgx_kron_states_expand(const dmrgx_sectors* left, const dmrgx_sectors* right, int32_t nblocks,
                                                 const int32_t* block_il, const int32_t* block_ir,
                                                 int32_t nstates, const double* Psi_dev, int64_t ldpsi, const double* weight,
                                                 int32_t side, int32_t* extent, int64_t* n_out, double* Y_dev, void* stream)
{
    const char* fn = "kron_states_expand";
    hipStream_t st = (hipStream_t)stream;
    if (!left || !right || left->nsec <= 0 || right->nsec <= 0 || !left->size || !right->size) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: empty sector table", fn);
    if (nblocks <= 0 || !block_il || !block_ir) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: no KronBlocks", fn);
    if (!extent || !n_out) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: null extent or n_out", fn);
    if (side != 0 && side != 1) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: side %d is neither 0 (columns, for rho_L) nor 1 (rows, for rho_R)", fn, side);
    if (nstates < 1 || !weight) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: nstates %d with %s weights: at least one state and its weight are needed", fn, nstates, weight ? "given" : "null");
    double wsum = 0.0;
    std::vector<double> root((size_t)nstates);
    for (int32_t s = 0; s < nstates; ++s) {
        if (!(weight[s] >= 0.0 && weight[s] < INFINITY)) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: weight %d = %g is negative or not finite", fn, s, weight[s]);
        wsum += weight[s];
        root[s] = std::sqrt(weight[s]);
    }
    if (!(wsum > 0.0)) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: all %d weights are zero", fn, nstates);
    for (int i = 0; i < left->nsec; ++i) if (left->size[i] <= 0) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: left sector %d has size %d", fn, i, left->size[i]);
    for (int i = 0; i < right->nsec; ++i) if (right->size[i] <= 0) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: right sector %d has size %d", fn, i, right->size[i]);
    std::set<std::pair<int32_t, int32_t>> seen;
    std::vector<int64_t> ref_off((size_t)nblocks + 1, 0), out_off((size_t)nblocks + 1, 0);
    for (int32_t k = 0; k < nblocks; ++k) {
        const int32_t il = block_il[k], ir = block_ir[k];
        if (il < 0 || il >= left->nsec || ir < 0 || ir >= right->nsec) DMRGX_FAIL(DMRGX_ERR_OUTOFRANGE, "%s: KronBlock %d = (%d,%d) out of range", fn, k, il, ir);
        if (!seen.emplace(il, ir).second) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: KronBlock (%d,%d) listed twice", fn, il, ir);
        const int64_t nl = left->size[il], nr = right->size[ir], ext = (int64_t)nstates * (side == 0 ? nr : nl);
        if (ext > INT32_MAX) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: the expansion of KronBlock %d is wider than 2^31 - 1", fn, k);
        ref_off[k + 1] = ref_off[k] + nl * nr;
        out_off[k + 1] = out_off[k] + (int64_t)nstates * nl * nr;
    }
    const int64_t N = ref_off[nblocks];
    if (ldpsi < N) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: ldpsi %lld is smaller than n_states %lld", fn, (long long)ldpsi, (long long)N);
    for (int32_t k = 0; k < nblocks; ++k) extent[k] = nstates * (side == 0 ? right->size[block_ir[k]] : left->size[block_il[k]]);
    *n_out = out_off[nblocks];
    if (!Y_dev) return DMRGX_OK;                                        // sizes only: no device call so far
    if (!Psi_dev) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: null Psi", fn);
    if (spans_overlap(Y_dev, (size_t)*n_out, Psi_dev, (size_t)(nstates - 1) * (size_t)ldpsi + (size_t)N)) DMRGX_FAIL(DMRGX_ERR_ARG, "%s: Y overlaps Psi", fn);

    std::vector<SxPanel> panels;
    panels.reserve((size_t)nblocks * nstates);
    int64_t most = 0;
    for (int32_t k = 0; k < nblocks; ++k) {
        const int64_t nl = left->size[block_il[k]], nr = right->size[block_ir[k]];
        for (int32_t s = 0; s < nstates; ++s) {
            SxPanel p;
            p.src = Psi_dev + (int64_t)s * ldpsi + ref_off[k];
            p.dst = Y_dev + out_off[k] + (side == 0 ? (int64_t)s * nr : (int64_t)s * nl * nr);
            p.ldd = side == 0 ? (int64_t)nstates * nr : nr;
            p.count = nl * nr;
            p.nc = (int32_t)nr;
            p.vec = (nr % 2 == 0 && p.ldd % 2 == 0 && ((uintptr_t)p.src & 15) == 0 && ((uintptr_t)p.dst & 15) == 0) ? 1 : 0;
            p.scale = root[s];
            panels.push_back(p);
            most = std::max(most, p.count);
        }
    }
    DevBuf tab;
    DMRGX_CHK(upload(tab, panels, st));
    const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(SX_BLOCKS, (most + SX_THREADS - 1) / SX_THREADS));
    hipLaunchKernelGGL(sx_copy_kernel, dim3(gx, (unsigned)panels.size()), dim3(SX_THREADS), 0, st, (const SxPanel*)tab.as<SxPanel>());
    DMRGX_HIP(hipGetLastError());
    return DMRGX_OK;
}
