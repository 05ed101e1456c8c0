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
Every figure is printed before it is asserted (pytest -s), with LAPACK's own figure beside it."""
import os
import subprocess
import sys

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


def _check_call(mods, tag, mats, counts=None):
    """One dmrgx_rdm_create over the KronBlocks (i, i) of the matrices `mats` (each Psi of one block), optionally dmrgx_rdm_select(counts)
    (counts[2 k + side]), and the assertions of the module's docstring.  Returns the report as a dict."""
    sbm, capi = mods
    ls, rs = [m.shape[0] for m in mats], [m.shape[1] for m in mats]
    psi = torch.from_numpy(np.concatenate([m.ravel() for m in mats])).cuda()
    rdm = sbm.ReducedDensityMatrices(ls, rs, [(i, i) for i in range(len(mats))], psi)
    rep = {k: getattr(rdm.report, k) for k, _ in rdm.report._fields_}
    assert rep["solver"] == 0 and rep["timed_out"] == 0 and rep["persistent_off"] == 0, rep
    spectra = [rdm.eigenvalues(mi % 2, mi // 2) for mi in range(2 * len(mats))]
    if counts is not None:
        rdm.select(counts)
    worst = np.zeros(6)
    for mi in range(2 * len(mats)):
        side, k = mi % 2, mi // 2
        rho, w_ref, X = _reference(tag, k, side, mats[k])
        n = rho.shape[0]
        w = rdm.eigenvalues(side, k)
        assert np.array_equal(w, spectra[mi])                                    # the selection leaves the spectrum as it was
        c = n if counts is None else counts[mi]
        U = rdm.eigenvectors(side, k, c).cpu().numpy() if c else np.zeros((0, n))
        bound_w, bound_r = helpers.rdm_bounds(rho, w_ref)
        err_w = np.abs(w - w_ref).max()
        res = np.abs(rho @ U.T - U.T * w[:c]).max() if c else 0.0
        orth = np.abs(U @ U.T - np.eye(c)).max() if c else 0.0
        lap = helpers.rdm_ratios(rho, w_ref, X[:c] if c else X[:1], w_ref)
        fig = np.array([err_w / bound_w, res / bound_r, orth, 0.0, lap[1], lap[2]])
        worst = np.maximum(worst, fig)
        print("RDM %s block %d side %d n %d kept %d: eigenvalues / bound %.3e  residual / bound %.3e  orthogonality %.3e   LAPACK: residual / bound %.3e  orthogonality %.3e"
              % (tag, k, side, n, c, fig[0], fig[1], fig[2], fig[4], fig[5]))
        assert np.isfinite(w).all() and np.isfinite(U).all(), (tag, k, side)
        assert err_w <= bound_w, (tag, k, side, n, err_w, bound_w)
        assert np.all(np.diff(w) <= 0), (tag, k, side)
        assert n <= 1100 and orth <= helpers.RDM_ORTH_TOL, (tag, k, side, n, orth)
        assert res <= bound_r, (tag, k, side, n, res, bound_r)
        if c < n:
            with pytest.raises(capi.DmrgxError):
                rdm.eigenvectors(side, k, c + 1)
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


def run_orders_1_to_40(mods, half=False):
    """ls = 1 .. 40 against rs = 40 .. 1: 80 density matrices, every order twice."""
    mats = _gaussian("orders_1_40", [(i, 41 - i) for i in range(1, 41)])
    counts = [n // 2 for m in mats for n in m.shape] if half else None
    return _check_call(mods, "orders_1_40", mats, counts), 2 * len(mats)


def run_edge_orders(mods, orders):
    """n x (n // 3) slices: rho_L of order n with a null space of two thirds, rho_R of order n // 3 and full rank."""
    mats = _gaussian("edge_%d" % orders[0], [(n, n // 3) for n in orders])
    rep = _check_call(mods, "edge_%d" % orders[0], mats)
    assert rep["merge_levels"] == _depth(max(orders)), (rep, orders)
    assert rep["wy_blocks_max"] == -(-(max(orders) - 2) // helpers.RDM_CONSTANTS["DMRGX_WY_NB"]), (rep, orders)
    return rep, 2 * len(mats)


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


# ---- clusters and grading ------------------------------------------------------------------------------------------------------------------
CLUSTERED = ["clusters_200", "graded_pairs_300", "glued_12_1e-8"]
# counts[2 k + side] for (clusters L, R, graded L, R, glued L, R): inside the 25-fold exactly degenerate cluster, inside the 1e-14 cluster
# (eigenvalues 50 .. 74), inside the exactly equal pairs (0, 1) and (60, 61), inside the 24 glued copies of W21's top pair; 1, n - 1 and 0
CUTS = [[10, 62, 1, 61, 5, 13],
        [199, 0, 299, 0, 251, 1],
        [0, 1, 261, 299, 0, 251]]


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


# ---- the same on poisoned workspaces -------------------------------------------------------------------------------------------------------
POISONED_NODES = ["tests/test_gpu_rdm_spectra.py::" + name for name in (
    "test_planted_tridiagonals", "test_closed_form_spectra", "test_clustered_and_graded_spectra", "test_select_cuts_inside_clusters",
    "test_every_order_from_1_to_40_in_one_call", "test_every_order_from_1_to_40_keeps_half", "test_edge_orders",
    "test_more_workgroups_than_the_device_has_cus", "test_launch_per_column_path")]


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
