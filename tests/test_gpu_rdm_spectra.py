"""The density-matrix eigensolver (csrc/symeig.hip behind dmrgx_rdm_create / _select / _eigenvectors) where the other tests do not reach
(-m gpu): planted tridiagonals that pass the Householder stage unchanged, merges in which one pole or none survives, clustered and graded
spectra that send the deflation through its sequential scan and rotation chains, every order from 1 to 40 in one call, the orders at the
edges of the tree, of the fused Loewner kernel, of the WY blocks and of the prefetch chunk, more matrices than one launch takes, more
workgroups than the device has CUs, and the launch-per-column path.

The inputs come from tests/helpers.py (built once per process, read-only); tests/test_rdm_inputs.py checks, without a GPU, that each has the
property it was built for and that LAPACK alone meets every bound used here.

One checker for everything (_check_call).  The reference is numpy.linalg.eigh of the float64 rho formed on the host.  For both sides of
every KronBlock:
  eigenvalues     |w - w_ref| <= 3e-15 n max|w_ref| + 1e-17, descending                      (the project's bound)
  orthonormality  |U U^T - 1| <= 1e-13                                                       (the project's bound, n <= 1100)
  residual        max |rho U^T - U^T diag(w)| <= 3e-15 n |rho|_2 + 1e-16                     (the same constant on the eigenvectors)
  verification    destroy() succeeds (the Rayleigh quotients agree with the solver's eigenvalues); the report says direct solver, no
                  time-out, persistent kernel not switched off
Every figure is printed before it is asserted (pytest -s), with LAPACK's own figure beside it.

The other solver, the QR-preconditioned block Jacobi of csrc/rdm_jacobi.hip and csrc/hqr.hip, is what EVERY density matrix of a call goes through
once one of its sectors exceeds SYMEIG_MAX_N = 3072.  The same checker holds it to the same inputs (_check_call with solver=1: the
report says Jacobi, eigenvalues as above, residual <= 1e-11 |rho|_F + 1e-16 -- ten times the solver's stop criterion --, orthonormality
as above, dmrgx_rdm_select a no-op) in a child process with DMRGX_RDM_SOLVER=jacobi (run_jacobi_cases), in the same child on poisoned
workspaces, and once in this process by the automatic switch itself, at order 3073.  Measured on an MI355X:
  case                                          sweeps   worst residual / bound   worst orthogonality
  orders 1 .. 40 (80 matrices)                       6          5.6e-05                 2.2e-15
  orders 255 .. 258                                  8          3.5e-05                 3.9e-15
  orders 511 .. 514                                  9          2.1e-05                 5.5e-15
  orders 1024, 1025                                  9          1.2e-03                 1.1e-14
  clusters_200, graded_pairs_300, glued, diagonal   18          7.5e-03                 8.3e-15
  zero, rank-one, orthogonal / sqrt(48), Gaussian    6          4.4e-03                 2.2e-15
  graded state, without / with ignored bases (7)  7 / 7          6.0e-05                 2.7e-15
  subset (four matrices of order 0 in the call)      7
  3073 x 24 with 1100 x 60, no switch set            6          1.8e-04                 3.2e-14
The same counts and figures came out on poisoned workspaces.  Orthogonality at order 3073: 3.235e-14 for the device, 4.996e-15 for
LAPACK's own eigenvectors of the same rho, so the bound max(1e-13, 10 x LAPACK's) was 1e-13; dmrgx_rdm_create of that call took 0.16 s."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}          # (tag, k, side) -> (rho, eigenvalues descending, LAPACK's eigenvectors as rows): computed once, read-only


@pytest.fixture(scope="module")
def mods(pkg):
    from dmrgx_amd import superblock, _capi
    _capi.require_device()
    return superblock, _capi


def _reference(tag, k, side, Psi):
    if (tag, k, side) not in _REF:
        rho = Psi.T @ Psi if side else Psi @ Psi.T
        w, X = np.linalg.eigh(rho)
        ref = (rho, w[::-1].copy(), X.T[::-1].copy())
        for a in ref:
            a.setflags(write=False)
        _REF[(tag, k, side)] = ref
    return _REF[(tag, k, side)]


def _device_figures(rho, w, U):
    """(max |rho U^T - U^T diag(w)|, max |U U^T - 1|) by float64 matrix products of torch on the device: a checker that shares nothing with
    the code under test, for the one order at which numpy's products on the host do not finish (a null space of 3049 subnormal-ridden
    directions)."""
    R, wd = torch.from_numpy(np.array(rho)).cuda(), torch.from_numpy(np.array(w[:len(U)])).cuda()
    Ud = torch.from_numpy(np.array(U)).cuda() if isinstance(U, np.ndarray) else U
    res = (R @ Ud.T - Ud.T * wd).abs().max().item()
    orth = (Ud @ Ud.T - torch.eye(len(U), dtype=torch.float64, device="cuda")).abs().max().item()
    return res, orth


def _check_call(mods, tag, mats, counts=None, solver=0, layout=None, warm=None, exact=None, max_sweeps=None):
    """One dmrgx_rdm_create over the KronBlocks (i, i) of the matrices `mats` (each Psi of one block), optionally dmrgx_rdm_select(counts)
    (counts[2 k + side]), and the assertions of the module's docstring.  Returns the report as a dict.

    solver: the solver the call is expected to report.  0 (direct): everything as it was.  1 (block Jacobi, csrc/rdm_jacobi.hip + hqr.hip): the
    report says Jacobi and no tridiagonalisation; the eigenvalues -- Rayleigh quotients of the finished vectors -- keep the bound of the
    direct solver; the residual bound is the project's bound for this solver, 1e-11 |rho|_F + 1e-16, ten times the solver's stop criterion
    off^2 <= 1e-24 total^2 (rdm_solve_jacobi), which bounds |rho U^T - U^T diag(w)|_F by 1e-12 |rho|_F before rounding; orthogonality
    1e-13 up to order 1100 and, above, max(1e-13, 10 x LAPACK's own figure for the same rho) (each column sees O(n sweeps) rotations where
    LAPACK applies O(n) reflectors), both figures by _device_figures; dmrgx_rdm_select is a no-op there -- every eigenvector exists from the
    start -- so the row c + 1 is NOT refused, and the first c rows of that request are the kept rows bit for bit.
    layout: (left sizes, right sizes, blocks) where the KronBlocks are not (i, i).  warm: {(side, k): orthogonal n x n} (dmrgx_rdm_create_warm: accepted, never read).
    exact: {2 k + side: spectrum} where the eigenvalues are planted and LAPACK is not the reference.  max_sweeps: the bound on n_sweeps."""
    sbm, capi = mods
    ls, rs, blocks = layout or ([m.shape[0] for m in mats], [m.shape[1] for m in mats], [(i, i) for i in range(len(mats))])
    assert [(ls[a], rs[b]) for a, b in blocks] == [m.shape for m in mats]
    psi = torch.from_numpy(np.concatenate([m.ravel() for m in mats])).cuda()
    hints = {key: torch.from_numpy(np.ascontiguousarray(v)).cuda() for key, v in warm.items()} if warm else None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rdm = sbm.ReducedDensityMatrices(ls, rs, blocks, psi, warm=hints)
    torch.cuda.synchronize()
    rep = {k: getattr(rdm.report, k) for k, _ in rdm.report._fields_}
    print("RDMREPORT %s solver %d n_sweeps %d create %.3f s" % (tag, rep["solver"], rep["n_sweeps"], time.perf_counter() - t0), rep)
    if solver == 0:
        assert rep["solver"] == 0 and rep["timed_out"] == 0 and rep["persistent_off"] == 0, rep
    else:
        assert rep["solver"] == 1 and rep["trid_persistent_matrices"] == 0 and rep["trid_launch_matrices"] == 0 and rep["timed_out"] == 0, rep
        assert max_sweeps is None or rep["n_sweeps"] <= max_sweeps, (tag, rep)
    spectra = [rdm.eigenvalues(mi % 2, mi // 2) for mi in range(2 * len(mats))]
    if counts is not None:
        rdm.select(counts)
    worst = np.zeros(6)
    for mi in range(2 * len(mats)):
        side, k = mi % 2, mi // 2
        rho, w_ref, X = _reference(tag, k, side, mats[k])
        n = rho.shape[0]
        big = n > 1100
        w = rdm.eigenvalues(side, k)
        assert np.array_equal(w, spectra[mi])                                    # the selection leaves the spectrum as it was
        c = n if counts is None else counts[mi]
        w_lapack = w_ref
        if exact is not None and mi in exact:
            w_ref = exact[mi]
        bound_w, bound_r = (helpers.rdm_jacobi_bounds if solver else helpers.rdm_bounds)(rho, w_ref)
        err_w = np.abs(w - w_ref).max()
        if big:
            assert solver == 1 and c == n, (tag, k, side, n)                     # the direct solver has the project's figure up to 1100 only
            Ud = rdm.eigenvectors(side, k, c)
            finite = bool(torch.isfinite(Ud).all())
            res, orth = _device_figures(rho, w, Ud)
            lap_res, lap_orth = _device_figures(rho, w_lapack, X)
            lap = (np.abs(w_lapack - w_ref).max() / bound_w, lap_res / bound_r, lap_orth)
            orth_tol = max(helpers.RDM_ORTH_TOL, 10.0 * lap_orth)
            print("RDM %s block %d side %d n %d: orthogonality %.3e, LAPACK's own %.3e, bound %.3e; LAPACK's eigenvalues / bound %.3e" % (tag, k, side, n, orth, lap_orth, orth_tol, lap[0]))
        else:
            U = rdm.eigenvectors(side, k, c).cpu().numpy() if c else np.zeros((0, n))
            finite = bool(np.isfinite(U).all())
            res = np.abs(rho @ U.T - U.T * w[:c]).max() if c else 0.0
            orth = np.abs(U @ U.T - np.eye(c)).max() if c else 0.0
            lap = helpers.rdm_ratios(rho, w_lapack, X[:c] if c else X[:1], w_ref, jacobi=bool(solver))
            orth_tol = helpers.RDM_ORTH_TOL
        fig = np.array([err_w / bound_w, res / bound_r, orth, 0.0, lap[1], lap[2]])
        worst = np.maximum(worst, fig)
        print("RDM %s block %d side %d n %d kept %d: eigenvalues / bound %.3e  residual / bound %.3e  orthogonality %.3e   LAPACK: residual / bound %.3e  orthogonality %.3e"
              % (tag, k, side, n, c, fig[0], fig[1], fig[2], fig[4], fig[5]))
        assert np.isfinite(w).all() and finite, (tag, k, side)
        assert err_w <= bound_w, (tag, k, side, n, err_w, bound_w)
        assert np.all(np.diff(w) <= 0), (tag, k, side)
        if solver == 0:
            assert n <= 1100 and orth <= helpers.RDM_ORTH_TOL, (tag, k, side, n, orth)
        else:
            assert orth <= orth_tol, (tag, k, side, n, orth, orth_tol)
        assert res <= bound_r, (tag, k, side, n, res, bound_r)
        if c < n and solver == 0:
            with pytest.raises(capi.DmrgxError):
                rdm.eigenvectors(side, k, c + 1)
        elif c < n:
            more = rdm.eigenvectors(side, k, c + 1).cpu().numpy()
            assert more.shape == (c + 1, n) and np.isfinite(more).all() and np.array_equal(more[:c], U), (tag, k, side)
    print("RDMWORST %s matrices %d: device eigenvalues %.3e residual %.3e orthogonality %.3e | LAPACK residual %.3e orthogonality %.3e"
          % (tag, 2 * len(mats), worst[0], worst[1], worst[2], worst[4], worst[5]))
    rdm.destroy()                                                                # raises when the Rayleigh-quotient verification fails
    return rep


def _depth(n):
    return helpers.rdm_tree_bounds(n)[0]


# ---- the cases as plain functions: the tests below call them, and so does the child process of the launch-per-column test ------------------
PLANTED = helpers.RDM_TRIDIAGONALS + ["blockdiag_64"]


def run_planted(mods):
    mats = [helpers.rdm_input(name)[2] for name in PLANTED]
    return _check_call(mods, "planted", mats), 2 * len(mats)


def _gaussian(tag, shapes):
    key = ("gaussian", tag)
    if key not in _REF:
        rng = np.random.default_rng(sum(a * 31 + b for a, b in shapes))
        _REF[key] = [rng.standard_normal(s) for s in shapes]
        for m in _REF[key]:
            m.setflags(write=False)
    return _REF[key]


def run_orders_1_to_40(mods, half=False, solver=0):
    """ls = 1 .. 40 against rs = 40 .. 1: 80 density matrices, every order twice."""
    mats = _gaussian("orders_1_40", [(i, 41 - i) for i in range(1, 41)])
    counts = [n // 2 for m in mats for n in m.shape] if half else None
    return _check_call(mods, "orders_1_40", mats, counts, solver=solver), 2 * len(mats)


def run_edge_orders(mods, orders, solver=0):
    """n x (n // 3) slices: rho_L of order n with a null space of two thirds, rho_R of order n // 3 and full rank."""
    mats = _gaussian("edge_%d" % orders[0], [(n, n // 3) for n in orders])
    rep = _check_call(mods, "edge_%d" % orders[0], mats, solver=solver)
    if solver == 0:                                                              # figures of the direct solver: the Jacobi path reports zeros
        assert rep["merge_levels"] == _depth(max(orders)), (rep, orders)
        assert rep["wy_blocks_max"] == -(-(max(orders) - 2) // helpers.RDM_CONSTANTS["DMRGX_WY_NB"]), (rep, orders)
    return rep, 2 * len(mats)


CLUSTERED = ["clusters_200", "graded_pairs_300", "glued_12_1e-8"]
# counts[2 k + side] for (clusters L, R, graded L, R, glued L, R): inside the 25-fold exactly degenerate cluster, inside the 1e-14 cluster
# (eigenvalues 50 .. 74), inside the exactly equal pairs (0, 1) and (60, 61), inside the 24 glued copies of W21's top pair; 1, n - 1 and 0
CUTS = [[10, 62, 1, 61, 5, 13],
        [199, 0, 299, 0, 251, 1],
        [0, 1, 261, 299, 0, 251]]
# diagonal_100 behind them: inside the eleven eigenvalues 0.0625 (ranks 21 .. 31) and inside the twenty exact zeros (ranks 80 .. 99)
JACOBI_CUT = CUTS[0] + [25, 90]


def run_special_blocks(mods, solver=0):
    """One state with a KronBlock that is exactly zero (every eigenvalue 0, any orthonormal basis), one of rank one, one orthogonal / sqrt(48)
    (rho = 1 / 48: nothing to rotate) and a Gaussian one."""
    mats = [helpers.rdm_input(name)[2] for name in helpers.RDM_SPECIAL]
    return _check_call(mods, "special", mats, solver=solver), 2 * len(mats)


def _graded_mats():
    lsz, rsz, blocks = helpers.RDM_GRADED_LAYOUT
    psi1, mats, off = helpers.rdm_graded_state()[1], [], 0
    for a, b in blocks:
        mats.append(psi1[off:off + lsz[a] * rsz[b]].reshape(lsz[a], rsz[b]))
        off += lsz[a] * rsz[b]
    return mats


def run_subset(mods, solver):
    """dmrgx_rdm_create_subset in the layout of test_gpu_kron.py::test_rdm_subset_matches_full_solve_and_refuses_unselected (block 0: left
    only, block 1: right only, block 2: nothing -- four matrices of order 0 inside the call): a selected matrix gets the spectrum of the full
    solve and of LAPACK within the project's eigenvalue bound (two runs of one solver differ by the rounding of their Rayleigh quotients,
    which that bound covers), its eigenvectors meet the bounds of _check_call, the batched gather returns the rows of the single one bit
    for bit, and an unselected matrix is refused."""
    import ctypes as C
    sbm, capi = mods
    L = capi.lib()
    ls, rs, blocks = [70, 33, 5], [20, 64, 41], [(0, 1), (1, 2), (2, 0)]
    mats = _gaussian("subset", [(ls[a], rs[b]) for a, b in blocks])
    psi = torch.from_numpy(np.concatenate([m.ravel() for m in mats])).cuda()
    full = sbm.ReducedDensityMatrices(ls, rs, blocks, psi)
    lsz, rsz = (C.c_int32 * 3)(*ls), (C.c_int32 * 3)(*rs)
    sl, sr = capi.Sectors(3, lsz), capi.Sectors(3, rsz)
    bil, bir = (C.c_int32 * 3)(*[b[0] for b in blocks]), (C.c_int32 * 3)(*[b[1] for b in blocks])
    mask = (C.c_uint8 * 3)(1, 2, 0)
    sub = sbm.ReducedDensityMatrices.__new__(sbm.ReducedDensityMatrices)          # the wrapper's accessors round a handle made here
    sub.left_sizes, sub.right_sizes, sub.blocks, sub._psi, sub._handle = ls, rs, blocks, psi, C.c_void_p()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    capi.check(L.dmrgx_rdm_create_subset(C.byref(sl), C.byref(sr), 3, bil, bir, C.c_void_p(psi.data_ptr()), C.cast(mask, C.c_void_p), st, C.byref(sub._handle)))
    sub.report = capi.RdmReport()
    capi.check(L.dmrgx_rdm_info(sub._handle, C.byref(sub.report)))
    print("RDMREPORT subset solver %d n_sweeps %d; the full solve: solver %d n_sweeps %d" % (sub.report.solver, sub.report.n_sweeps, full.report.solver, full.report.n_sweeps))
    assert sub.report.solver == full.report.solver == solver
    for k, side in ((0, 0), (1, 1)):
        rho, w_ref, _ = _reference("subset", k, side, mats[k])
        n = rho.shape[0]
        bound_w, bound_r = (helpers.rdm_jacobi_bounds if solver else helpers.rdm_bounds)(rho, w_ref)
        w, w_full = sub.eigenvalues(side, k), full.eigenvalues(side, k)
        U = sub.eigenvectors(side, k, n)
        Uh = U.cpu().numpy()
        res, orth = np.abs(rho @ Uh.T - Uh.T * w).max(), np.abs(Uh @ Uh.T - np.eye(n)).max()
        print("RDM subset block %d side %d n %d: against the full solve / bound %.3e  against LAPACK / bound %.3e  residual / bound %.3e  orthogonality %.3e"
              % (k, side, n, np.abs(w - w_full).max() / bound_w, np.abs(w - w_ref).max() / bound_w, res / bound_r, orth))
        assert np.isfinite(w).all() and np.isfinite(Uh).all() and np.all(np.diff(w) <= 0)
        assert np.abs(w - w_full).max() <= bound_w and np.abs(w - w_ref).max() <= bound_w and np.abs(w_full - w_ref).max() <= bound_w
        assert res <= bound_r and orth <= helpers.RDM_ORTH_TOL
        for c in (n, n // 2, 1):
            (got,) = sub.eigenvectors_batch([(side, k, c)])
            assert torch.equal(got, sub.eigenvectors(side, k, c)) and torch.equal(got, U[:c])
    out = (C.c_double * 70)()
    for k, side in ((0, 1), (1, 0), (2, 0), (2, 1)):
        assert L.dmrgx_rdm_eigenvalues(sub._handle, side, k, out) == capi.DMRGX_ERR_ARG
        with pytest.raises(capi.DmrgxError):
            sub.eigenvectors(side, k, 1)
        with pytest.raises(capi.DmrgxError):
            sub.eigenvectors_batch([(side, k, 1)])
    sub.destroy()
    full.destroy()
    return {k: getattr(sub.report, k) for k, _ in sub.report._fields_}


def run_jacobi_cases(mods):
    """Everything the block-Jacobi solver and its QR preconditioner are held to, for a process started with DMRGX_RDM_SOLVER=jacobi (the
    switch is read once per process).  Returns [(case, solver reported, n_sweeps)].  Only the graded state has a bound on its sweeps -- the
    project's own, test_gpu_kron.py::test_rdm_graded_spectrum_few_sweeps_and_warm_hints, which nowadays runs the direct solver; the sweeps
    of the other inputs are printed: nothing but the code under test could supply a bound for them."""
    out = []

    def note(case, rep):
        out.append((case, rep["solver"], rep["n_sweeps"]))

    # n = 1 (no QR, one padded pair), n = 2, the padding edge 31 / 32 / 33, 80 matrices of different nb in every round launch
    note("orders_1_40", run_orders_1_to_40(mods, solver=1)[0])
    # every size class of the QR panel: registers at 4 / 8 / 16 rows per thread and hqr_panel_kernel
    for orders in helpers.RDM_HQR_EDGE_CALLS:
        note("edge_%d" % orders[0], run_edge_orders(mods, orders, solver=1)[0])
    mats = [helpers.rdm_input(name)[2] for name in CLUSTERED + ["diagonal_100"]]
    note("clustered", _check_call(mods, "clustered", mats, solver=1))
    note("clustered_cut", _check_call(mods, "clustered", mats, JACOBI_CUT, solver=1))
    note("special", run_special_blocks(mods, solver=1)[0])
    junk = helpers.rdm_graded_state()[2]
    note("graded_cold", _check_call(mods, "graded", _graded_mats(), solver=1, layout=helpers.RDM_GRADED_LAYOUT, max_sweeps=7))
    note("graded_junk_hints", _check_call(mods, "graded", _graded_mats(), solver=1, layout=helpers.RDM_GRADED_LAYOUT, warm=junk, max_sweeps=7))
    note("subset", run_subset(mods, solver=1))
    return out


JACOBI_CASES = ["orders_1_40", "edge_255", "edge_511", "edge_1024", "clustered", "clustered_cut", "special", "graded_cold", "graded_junk_hints", "subset"]


# ---- planted tridiagonals ------------------------------------------------------------------------------------------------------------------
def test_planted_tridiagonals(mods):
    """Every bidiagonal and Cholesky input and the block-diagonal one in one call: all reflectors with tau == 0 (whole WY blocks of them),
    exact zero couplings, merges that deflate completely, merges in which one pole survives (the k == 1 branch of the secular kernel), chains
    of rotations.  The persistent kernel takes all twenty matrices."""
    rep, nmat = run_planted(mods)
    assert rep["trid_persistent_matrices"] == nmat and rep["trid_launch_matrices"] == 0, rep
    assert rep["merge_levels"] == _depth(252) == 4, rep


@pytest.mark.parametrize("name", ["k1_20", "k1_40", "diagonal_100"])
def test_closed_form_spectra(mods, name):
    """k1_*: a 2 x 2 block [[1.5625, 1.25], [1.25, 1.5625]] per split point (eigenvalues 2.8125 and 0.3125) and ones; diagonal: the squares
    of the diagonal.  Both sides have the same spectrum (Psi is square)."""
    sbm, _ = mods
    Psi = helpers.rdm_input(name)[2]
    n = Psi.shape[0]
    if name == "diagonal_100":
        exact = np.sort(np.diag(Psi) ** 2)[::-1]
    else:
        splits = len(helpers.rdm_tree_bounds(n)[1]) - 2
        exact = np.sort([2.8125, 0.3125] * splits + [1.0] * (n - 2 * splits))[::-1]
    rdm = sbm.ReducedDensityMatrices([n], [n], [(0, 0)], torch.from_numpy(Psi.ravel().copy()).cuda())
    for side in (0, 1):
        w = rdm.eigenvalues(side, 0)
        err = np.abs(w - exact).max()
        print("RDM closed form", name, "side", side, "error", err, "bound", 3e-15 * n * exact[0] + 1e-17)
        assert err <= 3e-15 * n * exact[0] + 1e-17
        if name == "diagonal_100":
            assert np.array_equal(w, exact)                  # nothing is computed on a diagonal matrix: every merge deflates completely
    rdm.destroy()


# ---- clusters and grading (CLUSTERED and CUTS: above, with the cases) ------------------------------------------------------------------------
def test_clustered_and_graded_spectra(mods):
    mats = [helpers.rdm_input(name)[2] for name in CLUSTERED]
    rep = _check_call(mods, "clustered", mats)
    assert rep["merge_levels"] == _depth(300) == 5, rep


@pytest.mark.parametrize("cut", range(len(CUTS)))
def test_select_cuts_inside_clusters(mods, cut):
    """dmrgx_rdm_select with the cut inside an exactly degenerate pair, inside a cluster of relative width 1e-14, at 1, at n - 1 and at 0:
    the kept rows are orthonormal eigenvectors of rho itself (rho U^T = U^T diag(w[:c])), whatever basis the solver chose inside the
    cluster, and one row more is refused."""
    mats = [helpers.rdm_input(name)[2] for name in CLUSTERED]
    _check_call(mods, "clustered", mats, CUTS[cut])


# ---- every order from 1 to 40; more matrices than one launch takes ---------------------------------------------------------------------------
def test_every_order_from_1_to_40_in_one_call(mods):
    """80 matrices: three launch groups or persistent rounds of at most TRID_MAXM = 32; every leaf edge (15 / 16 / 17, 31 / 32 / 33) and every
    row-block edge of the tridiagonalisation (8 rows per workgroup)."""
    rep, nmat = run_orders_1_to_40(mods)
    assert nmat == 80 and rep["trid_persistent_matrices"] == 80 and rep["trid_launch_matrices"] == 0 and rep["merge_levels"] == _depth(40) == 2, rep


def test_every_order_from_1_to_40_keeps_half(mods):
    run_orders_1_to_40(mods, half=True)


# ---- edge orders ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", range(len(helpers.RDM_EDGE_CALLS)))
def test_edge_orders(mods, call):
    """Orders around the tree's halving, DC_FUSE_NL, the last partial WY block and the prefetch chunk (helpers.RDM_EDGE_ORDERS; why these:
    test_rdm_inputs.test_the_order_lists_still_straddle_the_library_constants)."""
    run_edge_orders(mods, helpers.RDM_EDGE_CALLS[call])


# ---- two persistent rounds by capacity -----------------------------------------------------------------------------------------------------
def test_more_workgroups_than_the_device_has_cus(mods):
    """Six KronBlocks of 700 x 700: twelve matrices whose rows need more workgroups than the device has CUs, so the persistent kernel runs
    in (at least) two rounds.  The workgroups per matrix come from the capacity formula of symeig_batched: cap = (LDS doubles - 4 nv) / nv
    rows per workgroup, nv = n rounded up to even, G = ceil(n / cap)."""
    n = 700
    props = torch.cuda.get_device_properties(torch.cuda.current_device())
    ncu = props.multi_processor_count
    lds = props.shared_memory_per_block
    dyn_max = min(lds, 160 * 1024) - 256
    nv = (n + 1) & ~1
    cap = (dyn_max // 8 - 4 * nv) // nv
    G = -(-n // cap)
    print("RDM capacity: CUs", ncu, "LDS per workgroup", lds, "rows per workgroup", cap, "workgroups per matrix", G, "for 12 matrices", 12 * G)
    assert 1 <= G <= ncu < 12 * G
    mats = _gaussian("capacity", [(n, n)] * 6)
    rep = _check_call(mods, "capacity", mats)
    assert rep["trid_persistent_matrices"] == 12 and rep["trid_launch_matrices"] == 0 and rep["max_workgroups_per_matrix"] == G, rep


# ---- the launch-per-column path ------------------------------------------------------------------------------------------------------------
def test_launch_per_column_path():
    """The planted tridiagonals, the orders 1 .. 40 and 511 .. 514 in one child process with DMRGX_TRID=launch: every matrix is
    tridiagonalised by one launch per column (groups of at most 32 matrices, the 512-column prefetch chunk at its edge)."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r);"
            "from __graft_entry__ import load_package; load_package();"
            "import test_gpu_rdm_spectra as t; from dmrgx_amd import superblock, _capi; _capi.require_device(); mods = (superblock, _capi);"
            "runs = [t.run_planted(mods), t.run_orders_1_to_40(mods), t.run_edge_orders(mods, [511, 512, 513, 514])];"
            "print('launch path', [(r['trid_launch_matrices'], r['trid_persistent_matrices'], n) for r, n in runs])") % (ROOT, os.path.join(ROOT, "tests"))
    python = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    p = subprocess.run(python + ["-c", code], env=dict(os.environ, DMRGX_TRID="launch"), capture_output=True, text=True, timeout=480)
    print(p.stdout[-6000:])
    assert p.returncode == 0 and "launch path" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    got = eval(p.stdout[p.stdout.rindex("launch path") + len("launch path"):].strip())
    assert got == [(20, 0, 20), (80, 0, 80), (8, 0, 8)], got


# ---- zero, rank-one and identity blocks through the default solver ---------------------------------------------------------------------------
def test_zero_rank_one_and_identity_blocks(mods):
    """The state of run_special_blocks through the direct solver: a KronBlock of psi that is exactly zero gives rho = 0 on both sides (the
    bounds are then their absolute terms, 1e-17 and 1e-16), and the verification of destroy() compares Rayleigh quotients with a largest
    eigenvalue of 0."""
    rep, nmat = run_special_blocks(mods)
    assert nmat == 8 and rep["trid_persistent_matrices"] + rep["trid_launch_matrices"] == 8, rep


# ---- the block-Jacobi solver (csrc/rdm_jacobi.hip, csrc/hqr.hip) -----------------------------------------------------------------------------------
def _jacobi_child(extra_env):
    """run_jacobi_cases in a child process with DMRGX_RDM_SOLVER=jacobi; returns its [(case, solver, n_sweeps)]."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r);"
            "from __graft_entry__ import load_package; load_package();"
            "import test_gpu_rdm_spectra as t; from dmrgx_amd import superblock, _capi; _capi.require_device();"
            "print('jacobi path', t.run_jacobi_cases((superblock, _capi)))") % (ROOT, os.path.join(ROOT, "tests"))
    python = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    t0 = time.perf_counter()
    p = subprocess.run(python + ["-c", code], env=dict(os.environ, DMRGX_RDM_SOLVER="jacobi", **extra_env), capture_output=True, text=True, timeout=480)
    print(p.stdout[-20000:])
    print("jacobi child: %.1f s" % (time.perf_counter() - t0))
    assert p.returncode == 0 and "jacobi path" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    got = eval(p.stdout[p.stdout.rindex("jacobi path") + len("jacobi path"):].strip())
    assert [case for case, _, _ in got] == JACOBI_CASES and all(solver == 1 for _, solver, _ in got), got
    assert all(sweeps <= 7 for case, _, sweeps in got if case.startswith("graded")), got
    return got


def test_block_jacobi_solver():
    """The solver that every density matrix of a truncation step goes through once one sector exceeds SYMEIG_MAX_N, held to what the direct
    solver is held to (run_jacobi_cases), in one child process with DMRGX_RDM_SOLVER=jacobi.  Which case reaches which kernel body:
      hqr_panel_regs_kernel, 4 rows per thread (<= 256 rows)   every call; first panel of the orders 2 .. 40, 255, 256, of the 90 / 70 / 48-order blocks
      hqr_panel_regs_kernel, 8 rows per thread (<= 512)        first panel of 257, 258, 300, 511, 512
      hqr_panel_regs_kernel, 16 rows per thread (<= 1024)      first panel of 513, 514, 1024
      hqr_panel_kernel (> 1024 rows, reflector in LDS)         first panel of 1025, which then walks down through the other three
      panels narrower than 32, partial trailing strips         every order that is no multiple of 32
      jacobi_round_kernel: sub-solves, A updates, V updates    every call; one padded pair (n = 1), full and cross visits, up to 33 pairs per matrix
    Measured sweep counts (MI355X): see the table in the module's docstring."""
    _jacobi_child({})


def test_block_jacobi_solver_on_poisoned_workspaces():
    """The same child process with every f64 pool block handed out NaN-filled as well (DMRGX_POOL_POISON=1): the padding of A and V up to a
    multiple of 32, the second buffer of A, the work array [A | I] of the QR, its reflector and T scratch and the rows below a narrow
    panel are where an unwritten element would hide.  The same verdict is required."""
    _jacobi_child({"DMRGX_POOL_POISON": "1"})


def test_an_order_above_symeig_max_n_switches_the_whole_call_to_jacobi(mods):
    """No environment switch: one call with the KronBlocks 3073 x 24 and 1100 x 60.  3073 is the smallest order above SYMEIG_MAX_N, and it
    sends all four density matrices of the call through the block-Jacobi solver; 1100 is beside it so that at the panel steps r0 = 96 .. 1088 one
    matrix is factored by hqr_panel_kernel and the other by hqr_panel_regs_kernel.  The spectrum of the large block is
    planted (Psi = U diag(s) V^T, s = exp(-0.7 i): s^2 and 3049 zeros), its residual and orthogonality come from torch's matrix products
    on the device (_device_figures), and the orthogonality bound above order 1100 is max(1e-13, 10 x LAPACK's own figure).  The choice is
    per call: a small call behind it reports the direct solver again.  (Not among the poisoned nodes below: the Jacobi kernels run
    poisoned in test_block_jacobi_solver_on_poisoned_workspaces, and nothing smaller than this takes the branch.)"""
    assert "DMRGX_RDM_SOLVER" not in os.environ
    mats = [helpers.rdm_input(name)[2] for name in helpers.RDM_SWITCH]
    assert [m.shape for m in mats] == helpers.RDM_SWITCH_SHAPES
    exact = np.concatenate([helpers.RDM_PLANTED_S ** 2, np.zeros(3073 - 24)])
    t0 = time.perf_counter()
    rep = _check_call(mods, "switch", mats, solver=1, exact={0: exact, 1: helpers.RDM_PLANTED_S ** 2})
    print("RDM switch: n_sweeps %d, the whole check %.1f s" % (rep["n_sweeps"], time.perf_counter() - t0))
    rep = _check_call(mods, "after_switch", [helpers.rdm_input("gaussian_40x33")[2]])
    assert rep["solver"] == 0 and rep["trid_persistent_matrices"] == 2, rep


# ---- the same on poisoned workspaces -------------------------------------------------------------------------------------------------------
POISONED_NODES = ["tests/test_gpu_rdm_spectra.py::" + name for name in (
    "test_planted_tridiagonals", "test_closed_form_spectra", "test_clustered_and_graded_spectra", "test_select_cuts_inside_clusters",
    "test_every_order_from_1_to_40_in_one_call", "test_every_order_from_1_to_40_keeps_half", "test_edge_orders",
    "test_more_workgroups_than_the_device_has_cus", "test_launch_per_column_path", "test_zero_rank_one_and_identity_blocks")]


def test_this_file_on_poisoned_workspaces():
    """The tests above, unchanged, in one child process with every f64 pool block handed out NaN-filled (DMRGX_POOL_POISON=1, as
    test_gpu_krylov_shapes.py does): the unit columns of deflated poles, the zero reflectors and the padding of the leaves are where an
    unwritten element would hide."""
    env = dict(os.environ, DMRGX_POOL_POISON="1")
    python = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    p = subprocess.run(python + ["-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", *POISONED_NODES], cwd=ROOT, env=env, capture_output=True, text=True, timeout=480)
    tail = p.stdout[-3000:] + p.stderr[-2000:]
    assert p.returncode == 0, tail
    assert " passed" in tail and " failed" not in tail and " skipped" not in tail, tail
