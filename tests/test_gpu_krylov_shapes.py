"""The Krylov kernels where the other tests do not reach (-m gpu): odd vector lengths, several workgroups of the basis-keeping Lanczos run,
every basis width of the eigensolver, truncated and exhausted solves, and planted spectra.  Both solver types of dmrgx_eigs_lowest
(csrc/eigs.hip) and both Lanczos runs of csrc/lanczos.hip.

Every reference is numpy.linalg.eigh on the dense Hamiltonian, the Krylov-space Rayleigh-Ritz value of the reorthogonalised numpy
Lanczos (helpers.lanczos_reorth), or a bound derived from the measured residual; there is no host model of the restarted solver.
The inputs come from tests/helpers.py (built once per process, read-only); tests/test_krylov_inputs.py checks, without a GPU, that
each has the property it was built for.

The eigensolver's bounds are those of test_gpu_kron.test_eigs_lowest_vs_dense at tol = 1e-12: converged, |e0 - w0| <= 1e-10 |w0|,
true residual <= 1e-8 |e0| (through plan.apply and through the numpy apply), | |psi| - 1 | < 1e-12, psi finite."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import FactoredH, krylov_input, krylov_superblock, lanczos_basis_invariants, lanczos_reorth, lanczos_tridiag

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
# The restart budget of the runs with a narrow basis.  It is a budget, not a bound: with two vectors a restart keeps one Ritz vector and
# adds one direction, which is steepest descent on the Rayleigh quotient and takes about (w_max - w0) / (w1 - w0) * ln(1 / tol) / 2 steps
# -- 1 700 on the 845-state input (gap ratio 8.3e-3) -- at one restart per MatMult, more than the wrapper's default of 1 000 restarts.
NARROW_MAX_IT = 20000


class _Context:
    def __init__(self, sbm, wl, capi):
        self.sbm, self.wl, self.capi, self._plans, self._big, self._refs = sbm, wl, capi, {}, {}, {}

    def input(self, key):
        """(superblock, dense H, eigenvalues, eigenvectors)"""
        return krylov_input(self.wl, key)

    def big(self, n):
        """(superblock, H as an operator) at 2049 and 4097 states"""
        if n not in self._big:
            sb = krylov_superblock(self.wl, n)
            self._big[n] = (sb, FactoredH(self.wl, sb))
        return self._big[n]

    def plan(self, key):
        if key not in self._plans:
            self._plans[key] = self.sbm.KronPlan(self.big(key)[0] if key in (2049, 4097) else self.input(key)[0])
        return self._plans[key]

    def reference(self, n, v0, K, tag):
        """lanczos_reorth through the numpy apply, once per (size, start vector, steps)"""
        if (n, K, tag) not in self._refs:
            self._refs[(n, K, tag)] = lanczos_reorth(self.big(n)[1], v0, K)
        return self._refs[(n, K, tag)]

    def close(self):
        for p in self._plans.values():
            p.destroy()


@pytest.fixture(scope="module")
def ctx(pkg):
    from dmrgx_amd import superblock, workloads, _capi
    _capi.require_device()
    c = _Context(superblock, workloads, _capi)
    yield c
    c.close()


def _start(n, seed=5):
    return np.random.default_rng(seed).standard_normal(n)


def _check_pair(ctx, key, e0, psi, stats, what):
    """The ordinary bounds.  Returns (psi as numpy, the larger of the two measured true residuals)."""
    sb, H, w, _ = ctx.input(key)
    r = torch.empty_like(psi)
    ctx.plan(key).apply(psi, r)
    res_dev = float((r - e0 * psi).norm())
    x = psi.cpu().numpy()
    res_np = float(np.linalg.norm(ctx.wl.apply_factored_numpy(sb, x) - e0 * x))
    norm = float(psi.norm())
    print(what, "n", sb.n_states, "n_matvec", stats.n_matvec, "n_restart", stats.n_restart, "converged", stats.converged, "e0", e0, "w0", w[0],
          "|e0 - w0| / |w0|", abs(e0 - w[0]) / abs(w[0]), "|r| device", res_dev, "numpy", res_np, "bound", 1e-8 * abs(e0), "| |psi| - 1 |", abs(norm - 1.0))
    assert stats.converged == 1 and stats.n_matvec > 0
    assert np.isfinite(x).all() and np.isfinite(e0)
    assert abs(e0 - w[0]) <= 1e-10 * abs(w[0])
    assert res_dev <= 1e-8 * abs(e0) and res_np <= 1e-8 * abs(e0)
    assert abs(norm - 1.0) < 1e-12 and abs(np.linalg.norm(x) - 1.0) < 1e-12
    return x, max(res_dev, res_np)


def _check_simple_ground_state(ctx, key, x):
    v0 = ctx.input(key)[3][:, 0]
    assert abs(abs(float(x @ v0)) - 1.0) < 1e-8


def _check_eigenspace(ctx, key, x, e0, res, dim):
    """|(1 - P) psi| <= 2 |r| / (w_dim - w0 - |e0 - w0|), P the projector onto eigh's `dim` lowest eigenvectors and r the measured true
    residual: (H - e0) (1 - P) psi = (1 - P) r and H - e0 is at least w_dim - e0 on the range of 1 - P; the factor 2 covers the rounding
    of the check itself."""
    _, _, w, v = ctx.input(key)
    P = v[:, :dim]
    outside = float(np.linalg.norm(x - P @ (P.T @ x)))
    bound = 2.0 * res / (w[dim] - w[0] - abs(e0 - w[0]))
    print(key, "|(1 - P) psi|", outside, "bound", bound, "gap", w[dim] - w[0])
    assert outside <= bound


# ---- eigensolver, Lanczos path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["random", "psi0"])
@pytest.mark.parametrize("key", [845, 1205])
def test_lanczos_odd_length(ctx, key, start):
    """n odd: multi_dot_kernel<false> and axpy_normalise_kernel<false>, which no even-length input runs."""
    n = ctx.input(key)[0].n_states
    assert n % 2 == 1
    kw = dict(seed=9) if start == "random" else dict(psi0=torch.from_numpy(_start(n)).cuda())
    e0, psi, stats = ctx.plan(key).eigs_lowest(tol=TOL, **kw)
    x, _ = _check_pair(ctx, key, e0, psi, stats, "lanczos %s" % start)
    _check_simple_ground_state(ctx, key, x)


@pytest.mark.parametrize("key,ncv", [(845, 2), (845, 3), (845, 24), (845, 25), (845, 40), (845, 64), (845, 200), ("cfg2", 40)])
def test_lanczos_basis_widths(ctx, key, ncv):
    """2: a restart keeps one vector.  24 / 25: the last width whose steps all run the fused axpy_dot_kernel<24>, and the first with an
    unfused step (multi_axpy_kernel, a second multi_dot, c2 <- c1); 40 and 64 run it too, with both parities of n (845 and the 844 of
    cfg2).  200 is clamped to 64 vectors and must give the same run: same MatMults, restarts and bits of e0 (every kernel of the solve
    sums in a fixed order)."""
    e0, psi, stats = ctx.plan(key).eigs_lowest(ncv=ncv, tol=TOL, seed=9, max_it=NARROW_MAX_IT)
    x, _ = _check_pair(ctx, key, e0, psi, stats, "ncv %d" % ncv)
    _check_simple_ground_state(ctx, key, x)
    if ncv == 200:
        e64, _, s64 = ctx.plan(key).eigs_lowest(ncv=64, tol=TOL, seed=9, max_it=NARROW_MAX_IT)
        print("ncv 200 against 64: n_matvec", stats.n_matvec, s64.n_matvec, "n_restart", stats.n_restart, s64.n_restart, "e0", e0, e64)
        assert (stats.n_matvec, stats.n_restart) == (s64.n_matvec, s64.n_restart) and e0 == e64


def test_lanczos_one_vector_basis_is_taken_as_two(ctx):
    """ncv = 1: a one-vector Krylov space cannot restart, so the solver takes it as 2 (n_states > 1).  The ordinary bounds, and the run
    of ncv = 2.  (Before: the restart set k = m = 1, every later cycle ran no MatMult and read the first cycle's beta again, and the call
    returned DMRGX_ERR_NOTCONV after max_it restarts with one MatMult done.)"""
    plan = ctx.plan(845)
    e0, psi, stats = plan.eigs_lowest(ncv=1, tol=TOL, seed=9, max_it=NARROW_MAX_IT)
    x, _ = _check_pair(ctx, 845, e0, psi, stats, "ncv 1")
    _check_simple_ground_state(ctx, 845, x)
    e2, _, s2 = plan.eigs_lowest(ncv=2, tol=TOL, seed=9, max_it=NARROW_MAX_IT)
    assert (stats.n_matvec, stats.n_restart) == (s2.n_matvec, s2.n_restart) and e0 == e2


@pytest.mark.parametrize("k", [1, 2, 7, 16])
def test_max_matvec_inside_one_cycle(ctx, k):
    """max_matvec = k <= ncv = 16 from a supplied psi0: exactly k MatMults, and the answer is the Rayleigh-Ritz pair of the Krylov space
    K_k(H, psi0): e0 = the lowest eigenvalue of the numpy recursion's T_k to 1e-10 |H| (the tolerance of the coefficient tests for the
    same arithmetic), psi of norm 1 with Rayleigh quotient e0 to 1e-10 |H|.  k < 16 is the truncated cycle (jend < m)."""
    sb, H, w, _ = ctx.input(845)
    normH = np.abs(w).max()
    v0 = _start(sb.n_states)
    e0, psi, stats = ctx.plan(845).eigs_lowest(ncv=16, tol=TOL, psi0=torch.from_numpy(v0).cuda(), max_matvec=k)
    _, a, b = lanczos_reorth(H, v0, k)
    want = np.linalg.eigvalsh(lanczos_tridiag(a, b))[0]
    x = psi.cpu().numpy()
    rq = float(x @ (H @ x))
    print("max_matvec", k, "n_matvec", stats.n_matvec, "e0", e0, "T_k", want, "err", abs(e0 - want), "Rayleigh quotient err", abs(rq - e0), "tol", 1e-10 * normH,
          "| |psi| - 1 |", abs(np.linalg.norm(x) - 1.0))
    assert stats.n_matvec == k and stats.start_rejected == 0
    assert np.isfinite(x).all() and abs(np.linalg.norm(x) - 1.0) < 1e-12
    assert abs(e0 - want) <= 1e-10 * normH
    assert abs(rq - e0) <= 1e-10 * normH


def test_max_matvec_across_restarts(ctx):
    """ncv = 4 and max_matvec = 4 (one full cycle), 5 (a restart, then a truncated cycle of one step), 11 (four restarts and a truncated
    cycle): exactly that many MatMults, a Ritz value never below w0, and never rising: the restart keeps the lowest Ritz vector."""
    sb, H, w, _ = ctx.input(845)
    normH = np.abs(w).max()
    psi0 = torch.from_numpy(_start(sb.n_states)).cuda()
    e = {}
    for k in (4, 5, 11):
        e[k], psi, stats = ctx.plan(845).eigs_lowest(ncv=4, tol=TOL, psi0=psi0, max_matvec=k)
        x = psi.cpu().numpy()
        print("ncv 4 max_matvec", k, "n_matvec", stats.n_matvec, "n_restart", stats.n_restart, "e0", e[k], "w0", w[0])
        assert stats.n_matvec == k
        assert np.isfinite(x).all() and abs(np.linalg.norm(x) - 1.0) < 1e-12
        assert e[k] >= w[0] - 1e-10 * normH
        assert abs(float(x @ (H @ x)) - e[k]) <= 1e-10 * normH
    assert e[11] <= e[5] + 1e-12 * normH and e[5] <= e[4] + 1e-12 * normH


def test_max_it_exhausted_returns_the_best_pair_so_far(ctx):
    """ncv = 4, max_it = 2, tol = 1e-14 from a random start: DMRGX_ERR_NOTCONV, the message names the restarts, and psi, e0 are the
    finite, normalised Ritz pair reached (through the C ABI: the wrapper raises)."""
    capi, plan = ctx.capi, ctx.plan(845)
    _, _, w, _ = ctx.input(845)
    opts, stats, e0 = capi.EigsOpts(), capi.EigsStats(), C.c_double(float("nan"))
    opts.ncv, opts.max_it, opts.tol, opts.seed = 4, 2, 1e-14, 9
    psi = torch.full((plan.info.vec_len,), float("nan"), dtype=torch.float64, device="cuda")
    rc = capi.lib().dmrgx_eigs_lowest(plan._handle, C.byref(opts), C.byref(e0), C.c_void_p(psi.data_ptr()), C.byref(stats), plan._stream_ptr(None))
    msg = capi.lib().dmrgx_last_error().decode(errors="replace")
    x = psi.cpu().numpy()
    print("rc", rc, "message", msg, "n_matvec", stats.n_matvec, "n_restart", stats.n_restart, "e0", e0.value, "w0", w[0])
    assert rc == capi.DMRGX_ERR_NOTCONV and stats.converged == 0
    assert stats.n_restart == 2 and "after 2 restarts" in msg
    assert np.isfinite(x).all() and np.isfinite(e0.value)
    assert abs(np.linalg.norm(x) - 1.0) <= 1e-12
    assert e0.value >= w[0] - 1e-10 * np.abs(w).max()
    with pytest.raises(capi.DmrgxError) as e:
        plan.eigs_lowest(ncv=4, max_it=2, tol=1e-14, seed=9)
    assert e.value.code == capi.DMRGX_ERR_NOTCONV


def test_lanczos_positive_definite(ctx):
    """The lowest eigenvalue is +3 and the largest magnitude is at the other end of the spectrum."""
    _, _, w, _ = ctx.input("posdef")
    e0, psi, stats = ctx.plan("posdef").eigs_lowest(tol=TOL, seed=9)
    x, _ = _check_pair(ctx, "posdef", e0, psi, stats, "posdef")
    _check_simple_ground_state(ctx, "posdef", x)
    assert e0 > 0.0 and abs(e0 - 3.0) < abs(e0 - w[-1])


def test_lanczos_degenerate_ground_state(ctx):
    """psi may be any unit vector of the two-dimensional eigenspace."""
    e0, psi, stats = ctx.plan("degenerate").eigs_lowest(tol=TOL, seed=9)
    x, res = _check_pair(ctx, "degenerate", e0, psi, stats, "degenerate")
    _check_eigenspace(ctx, "degenerate", x, e0, res, 2)


def test_lanczos_tiny_gap(ctx):
    """(w1 - w0) / (w_max - w0) = 1e-3, within the wrapper's 1000 restarts."""
    e0, psi, stats = ctx.plan("tinygap").eigs_lowest(tol=TOL, seed=9)
    x, res = _check_pair(ctx, "tinygap", e0, psi, stats, "tinygap")
    _check_eigenspace(ctx, "tinygap", x, e0, res, 1)


# ---- eigensolver, generalized Davidson -----------------------------------------------------------------------------------------------------
def _gd_start(ctx, key, start):
    sb, _, _, v = ctx.input(key)
    rng = np.random.default_rng(1)
    return torch.from_numpy(rng.standard_normal(sb.n_states) if start == "far" else v[:, 0] + 1e-3 * rng.standard_normal(sb.n_states)).cuda()


@pytest.mark.parametrize("start", ["far", "near"])
@pytest.mark.parametrize("ncv", [0, 3, 6])
@pytest.mark.parametrize("key", [845, 1205])
def test_davidson_odd_length(ctx, key, ncv, start):
    """n odd: the work vectors are padded to an even length with a zero (gd_zero_pads_kernel) and every kernel runs its two-per-lane
    form over the pad.  The bounds of test_eigs_generalized_davidson_vs_dense_and_lanczos."""
    e0, psi, stats = ctx.plan(key).eigs_lowest(tol=TOL, method=1, ncv=ncv, psi0=_gd_start(ctx, key, start))
    x, _ = _check_pair(ctx, key, e0, psi, stats, "gd ncv %d %s" % (ncv, start))
    _check_simple_ground_state(ctx, key, x)


@pytest.mark.parametrize("start", ["far", "near"])
def test_davidson_positive_definite(ctx, start):
    _, _, w, _ = ctx.input("posdef")
    e0, psi, stats = ctx.plan("posdef").eigs_lowest(tol=TOL, method=1, psi0=_gd_start(ctx, "posdef", start))
    x, _ = _check_pair(ctx, "posdef", e0, psi, stats, "gd posdef %s" % start)
    _check_simple_ground_state(ctx, "posdef", x)
    assert e0 > 0.0 and abs(e0 - 3.0) < abs(e0 - w[-1])


@pytest.mark.parametrize("start", ["far", "near"])
def test_davidson_degenerate_ground_state(ctx, start):
    e0, psi, stats = ctx.plan("degenerate").eigs_lowest(tol=TOL, method=1, psi0=_gd_start(ctx, "degenerate", start))
    x, res = _check_pair(ctx, "degenerate", e0, psi, stats, "gd degenerate %s" % start)
    _check_eigenspace(ctx, "degenerate", x, e0, res, 2)


# ---- the Lanczos runs at several workgroups and odd lengths --------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 1, 2])
@pytest.mark.parametrize("n", [2049, 4097])
def test_basis_run_over_several_workgroups(ctx, n, pad):
    """dmrgx_kron_lanczos_basis with two (2049: the second holds one element) and three workgroups, 70 steps -- one more than a chunk of
    64 rows -- into NaN-filled storage.  pad 0: ldv = n, odd, the 8-byte loads.  pad 1: rows 16-byte aligned with n odd, the 16-byte
    loads with the scalar tail.  pad 2: odd again with a wider pad.  The pad columns stay NaN.  The invariants of
    test_gpu_lanczos_basis with H applied by numpy and |H| taken as the largest |Ritz value| of the reference, a lower bound."""
    sb, H = ctx.big(n)
    K = 70
    v0 = _start(n, 11)
    store = torch.full((K, n + pad), float("nan"), dtype=torch.float64, device="cuda")
    assert store.data_ptr() % 16 == 0 and store.stride(0) == n + pad
    lanczos_basis_invariants(ctx.plan(n), H, v0, K, V=store[:, :n], ref=ctx.reference(n, v0, K, "random"))
    assert torch.isnan(store[:, n:]).all() and not torch.isnan(store[:, :n]).any()


@pytest.mark.parametrize("where", ["last", "straddle"])
def test_basis_run_from_the_edge_of_the_last_workgroup(ctx, where):
    """2049 states, a start vector that is non-zero only in its last element (all of the second workgroup), or only in elements 2047 and
    2048 on both sides of the workgroup boundary: norm2 exact, alpha_0 = <q0|H|q0> to 1e-10 |H|, the invariants for 8 steps."""
    n, K = 2049, 8
    sb, H = ctx.big(n)
    v0 = np.zeros(n)
    if where == "last":
        v0[2048], exact = 1.5, 2.25
    else:
        v0[2047], v0[2048], exact = 0.75, -1.25, 2.125
    ref = ctx.reference(n, v0, K, where)
    normH = np.abs(np.linalg.eigvalsh(lanczos_tridiag(ref[1], ref[2]))).max()
    store = torch.full((K, n + 1), float("nan"), dtype=torch.float64, device="cuda")
    norm2, alpha, beta = lanczos_basis_invariants(ctx.plan(n), H, v0, K, V=store[:, :n], ref=ref)
    q0 = v0 / np.sqrt(exact)
    want = float(q0 @ (H @ q0))
    print(where, "norm2", norm2, "alpha_0", alpha[0], "want", want, "err", abs(alpha[0] - want), "tol", 1e-10 * normH)
    assert norm2 == exact
    assert abs(alpha[0] - want) <= 1e-10 * normH
    assert torch.isnan(store[:, n:]).all()


@pytest.mark.parametrize("pad", [0, 1])
def test_basis_run_through_a_nearly_invariant_start_vector(ctx, pad):
    """Where the reorthogonalisation of the last element matters.  On a generic input every Gram-Schmidt correction is rounding noise, and a
    run that never stored the corrected last element of an odd-length w (the scalar tail store of lb_multiaxpy_kernel) still keeps
    V V^T = 1 to 1e-15; numpy says so.  Here v0 is a combination of the 5 eigenvectors that are largest in the last element plus 1e-12
    of a random vector: beta_4 is 5e-9 of the scale (breakdown_tol = 1e-10 lets the run go on), the division by it lifts the rounding
    of w to 1e-5 of q_5, and the corrections that take it out again are what keeps V V^T = 1 and V H V^T = T to 1e-12 (|H|).  Without
    the tail store numpy gives 4e-11 for both.  845 states, 12 steps; pad 0: ldv odd, pad 1: 16-byte rows with the scalar tail."""
    sb, H, w, v = ctx.input(845)
    n, K = sb.n_states, 12
    idx = np.sort(np.argsort(np.abs(v[n - 1]))[-5:])
    v0 = v[:, idx] @ np.random.default_rng(13).uniform(0.5, 1.5, 5) + 1e-12 * _start(n, 11)
    v0d = torch.from_numpy(v0).cuda()
    store = torch.full((K, n + pad), float("nan"), dtype=torch.float64, device="cuda")
    plan = ctx.plan(845)
    norm2, alpha, beta, done, V = plan.lanczos_basis(v0d, K, breakdown_tol=1e-10, V=store[:, :n])
    Vh = V.cpu().numpy().copy()
    _, alphab, betab, doneb, Vb = plan.lanczos_basis(v0d, K, breakdown_tol=1e-10)
    scale = max(np.abs(alpha).max(), beta.max())
    orth, galerkin = np.abs(Vh @ Vh.T - np.eye(K)).max(), np.abs(Vh @ (H @ Vh.T) - lanczos_tridiag(alpha, beta)).max()
    normH = np.abs(w).max()
    print("pad", pad, "beta", beta, "beta_4 / scale", beta[4] / scale, "|VV^T - 1|", orth, "|VHV^T - T|", galerkin, "|H|", normH)
    assert done == K == doneb and np.isfinite(alpha).all() and np.isfinite(beta).all() and np.isfinite(Vh).all()
    assert 1e-10 * scale < beta[4] < 1e-7 * scale          # the regime this test is about
    assert orth <= 1e-12
    assert galerkin <= 1e-12 * normH
    assert np.array_equal(alpha.view(np.uint64), alphab.view(np.uint64)) and np.array_equal(beta.view(np.uint64), betab.view(np.uint64))
    assert np.array_equal(Vh.view(np.uint64), Vb.cpu().numpy().view(np.uint64))
    assert torch.isnan(store[:, n:]).all()


@pytest.mark.parametrize("n", [845, 2049, 4097])
def test_coefficients_odd_lengths(ctx, n):
    """dmrgx_kron_lanczos_coeffs as test_gpu_lanczos_coeffs.test_coefficients_against_reorthogonalised_numpy checks it, K = 10."""
    K = 10
    if n == 845:
        sb, plan = ctx.input(n)[0], ctx.plan(n)
        H = FactoredH(ctx.wl, sb)
    else:
        (sb, H), plan = ctx.big(n), ctx.plan(n)
    v0 = _start(n, 11)
    n2, a, b = lanczos_reorth(H, v0, K)
    v0d = torch.from_numpy(v0).cuda()
    norm2, alpha, beta, done = plan.lanczos_coeffs(v0d, K)
    norm2b, alphab, betab, doneb = plan.lanczos_coeffs(v0d, K)
    tol = 1e-10 * np.abs(a).max()
    print("n", n, "norm2 err", abs(norm2 - n2), "alpha err", np.abs(alpha - a).max(), "beta err", np.abs(beta[:K - 1] - b[:K - 1]).max(), "tol", tol)
    assert done == K and np.isfinite(alpha).all() and np.isfinite(beta).all()
    assert abs(norm2 - n2) <= tol
    assert np.abs(alpha - a).max() <= tol and np.abs(beta[:K - 1] - b[:K - 1]).max() <= tol
    assert norm2 == norm2b and done == doneb
    assert np.array_equal(alpha.view(np.uint64), alphab.view(np.uint64)) and np.array_equal(beta.view(np.uint64), betab.view(np.uint64))
    assert np.array_equal(v0d.cpu().numpy().view(np.uint64), v0.view(np.uint64))


# ---- the same on poisoned workspaces -------------------------------------------------------------------------------------------------------
POISONED_NODES = ["tests/test_gpu_krylov_shapes.py::" + name for name in (
    "test_lanczos_odd_length", "test_lanczos_basis_widths", "test_lanczos_one_vector_basis_is_taken_as_two", "test_max_matvec_inside_one_cycle",
    "test_max_matvec_across_restarts", "test_max_it_exhausted_returns_the_best_pair_so_far", "test_lanczos_positive_definite",
    "test_lanczos_degenerate_ground_state", "test_lanczos_tiny_gap", "test_davidson_odd_length", "test_davidson_positive_definite",
    "test_davidson_degenerate_ground_state", "test_basis_run_over_several_workgroups", "test_basis_run_from_the_edge_of_the_last_workgroup",
    "test_basis_run_through_a_nearly_invariant_start_vector",     "test_coefficients_odd_lengths")]


def test_this_file_on_poisoned_workspaces():
    """The tests above, unchanged, in one child process with every f64 pool block handed out NaN-filled (DMRGX_POOL_POISON=1, as
    test_gpu_lanczos_basis.py does): the pads of the odd lengths and the almost empty last workgroup are where an unwritten element
    would hide."""
    env = dict(os.environ, DMRGX_POOL_POISON="1")
    python = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    p = subprocess.run(python + ["-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", *POISONED_NODES], cwd=ROOT, env=env, capture_output=True, text=True, timeout=480)
    tail = p.stdout[-3000:] + p.stderr[-2000:]
    assert p.returncode == 0, tail
    assert " passed" in tail and " failed" not in tail and " skipped" not in tail, tail
