"""The inputs of tests/test_gpu_rdm_spectra.py have the properties they were built for (no GPU): a GPU test on an input without its
property proves nothing.  The builders are in tests/helpers.py; every input and its model run are computed once per process.

The merge counts (poles that survive, rotations, chains, fully deflated merges) are those of the project's HOST model of the solver
(tools/proto_trid_dc.py at the library's leaf size), not of the device: the device's tridiagonal and its leaves differ from the model's in
the last bits.  So no property here sits on a knife edge: each is planted by exact arithmetic (dyadic entries, structural zeros, exactly
equal poles) or by a margin of many orders of magnitude against the deflation tolerance of 8 eps."""
import os
import re

import numpy as np
import pytest

import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dmrg.x_amd", "csrc")


def _rho(name):
    Psi = helpers.rdm_input(name)[2]
    return Psi @ Psi.T, Psi.T @ Psi


def _summary(name):
    st = helpers.rdm_named_stats(name)
    m = st["merges"]
    out = dict(n=st["n"], merges=len(m), scanning=sum(r > 0 for _, _, r, _, _ in m), rotations=sum(r for _, _, r, _, _ in m),
               chain=max([c for _, _, _, c, _ in m], default=0), all_deflated=sum(bool(a) for *_, a in m), k=[k for _, k, _, _, _ in m],
               tau_zero=st["tau_zero"], e_zero=st["e_zero"])
    print(name, out)
    return out


@pytest.mark.parametrize("name", helpers.RDM_NAMED + ["gaussian_100x60"])
def test_inputs_are_read_only_and_cached(name):
    rows, cols, Psi = helpers.rdm_input(name)
    assert Psi.shape == (rows, cols) and Psi.dtype == np.float64 and not Psi.flags.writeable and np.isfinite(Psi).all()
    assert helpers.rdm_input(name)[2] is Psi


@pytest.mark.parametrize("name", helpers.RDM_TRIDIAGONALS)
def test_planted_tridiagonals_pass_the_householder_stage_unchanged(name):
    """Bidiagonal and Cholesky inputs: both density matrices are tridiagonal with exact zeros outside, and every reflector of rho_L has
    tau == 0, so the divide and conquer sees the planted tridiagonal itself."""
    rows, cols, Psi = helpers.rdm_input(name)
    assert rows == cols and not np.triu(Psi, 1).any() and not np.tril(Psi, -2).any()
    for rho in _rho(name):
        assert not np.triu(rho, 2).any() and np.array_equal(rho, rho.T)
    s = _summary(name)
    assert s["tau_zero"] == s["n"] == rows
    a, b = np.diag(Psi), np.diag(Psi, -1)
    if not name.startswith("glued"):                                            # dyadic entries: d and e are exact
        rho = _rho(name)[0]
        assert np.array_equal(np.diag(rho), a * a + np.concatenate([[0.0], b * b])) and np.array_equal(np.diag(rho, 1), a[:-1] * b)
        assert np.array_equal(Psi * 1024.0, np.round(Psi * 1024.0)) or name == "diagonal_100"


@pytest.mark.parametrize("name", ["k1_20", "k1_40"])
def test_one_pole_survives_every_merge(name):
    """The k == 1 branch of the secular kernel: d[s-1] == d[s] exactly at every split point, nothing else is coupled."""
    Psi = helpers.rdm_input(name)[2]
    n = Psi.shape[0]
    depth, bounds = helpers.rdm_tree_bounds(n)
    rho = _rho(name)[0]
    for s in bounds[1:-1]:
        assert rho[s - 1, s - 1] == rho[s, s] == 1.5625 and rho[s - 1, s] == 1.25
    assert np.count_nonzero(np.diag(rho, 1)) == len(bounds) - 2
    s = _summary(name)
    assert s["merges"] == len(bounds) - 2 == {20: 1, 40: 3}[n] and all(k == 1 for k in s["k"]) and s["rotations"] == s["merges"]


def test_two_poles_survive_in_the_variant():
    s = _summary("k2_20")
    assert s["k"] == [2] and s["rotations"] == 0


def test_diagonal_input_deflates_every_merge():
    rows, _, Psi = helpers.rdm_input("diagonal_100")
    a = np.diag(Psi)
    assert np.array_equal(Psi, np.diag(a)) and np.sum(a == 0.0) == 20 and len(np.unique(a)) == 3 + 1 + 50 - 2      # (0.5 and 0.25 are in the tail too)
    assert np.any(np.diff(a) > 0) and np.any(np.diff(a) < 0)                      # not sorted
    s = _summary("diagonal_100")
    assert s["e_zero"] == 99 and s["all_deflated"] == s["merges"] == 7 and s["k"] == [0] * 7


def test_zero_couplings_away_from_the_split_points():
    rho = _rho("zero_coupling_50")[0]
    zeros = np.flatnonzero(np.diag(rho, 1) == 0.0) + 1                             # a zero e_j separates rows j and j + 1
    splits = helpers.rdm_tree_bounds(50)[1][1:-1]
    assert list(zeros) == [6, 31] and splits == [12, 25, 37]
    assert _summary("zero_coupling_50")["e_zero"] == 2


def test_block_diagonal_input():
    rho_l, rho_r = _rho("blockdiag_64")
    edges = np.cumsum([0, 7, 16, 17, 1, 23])
    mask = np.zeros((64, 64), bool)
    for lo, hi in zip(edges[:-1], edges[1:]):
        mask[lo:hi, lo:hi] = True
    for rho in (rho_l, rho_r):
        assert not rho[~mask].any() and np.count_nonzero(rho[mask]) == mask.sum()
    assert not set(edges[1:-1]) & set(helpers.rdm_tree_bounds(64)[1])
    s = _summary("blockdiag_64")
    assert s["e_zero"] == 4                                                       # one exact zero coupling per block edge


@pytest.mark.parametrize("name,chain", [("glued_6_1e-8", 2), ("glued_12_1e-8", 2), ("clusters_200", 2), ("toeplitz121_100", 1), ("glued_6_1e-14", 1)])
def test_close_poles_send_the_merges_through_the_sequential_scan(name, chain):
    """At least half of the merges scan, and at least one has a chain of `chain` rotations.  The glue of 1e-14 is the one input whose model
    run has no chain of two: its copies are coupled below the deflation tolerance, so what it adds instead is a merge that deflates
    completely at a coupling that is NOT zero."""
    s = _summary(name)
    assert 2 * s["scanning"] >= s["merges"] and s["chain"] >= chain and s["rotations"] >= s["scanning"]
    if name == "glued_6_1e-14":
        assert s["all_deflated"] >= 1 and s["e_zero"] == 0


def test_gaussian_control_barely_scans():
    """What the new inputs change: the input family of almost every other density-matrix test."""
    s = _summary("gaussian_100x60")
    assert s["scanning"] <= 1 and s["chain"] <= 1 and s["tau_zero"] == 2 and s["e_zero"] == 0 and 1 not in s["k"]


def test_cluster_and_graded_spectra():
    _, _, Psi = helpers.rdm_input("clusters_200")
    w = np.linalg.svd(Psi, compute_uv=False) ** 2
    for c, spread in enumerate([0.0, 1e-16, 1e-14, 1e-12, 1e-10, 1e-8, 1e-6, 1e-4]):
        got = w[25 * c:25 * c + 25] * 2.0 ** c
        assert np.abs(got - 1.0).max() <= spread + 1e-13, (c, np.abs(got - 1.0).max())
    _, _, Psi = helpers.rdm_input("graded_pairs_300")
    s = np.linalg.svd(Psi, compute_uv=False)
    assert np.abs(s[0:260:2] - s[1:260:2]).max() <= 1e-15 and s[260:].max() <= 1e-15 and abs(s[0] - 1.0) <= 1e-14
    W = helpers.rdm_input("glued_12_1e-8")[2]
    w = np.linalg.eigvalsh(W @ W.T)[::-1]
    # W21's two largest eigenvalues agree to 1e-13 and come twelve times each: a cluster of 24 within 1e-7; positive definite
    assert np.abs(w[:24] - w[0]).max() <= 1e-7 and w[24] < w[0] - 0.5 and w[-1] > 0.3


def test_lapack_alone_meets_every_bound():
    """The bounds of tests/test_gpu_rdm_spectra.py are achievable: numpy's eigh meets them on every named input, both sides, with the singular
    values of Psi as the reference of the eigenvalues."""
    worst = {}
    for name in helpers.RDM_NAMED:
        rows, cols, Psi = helpers.rdm_input(name)
        s2 = np.linalg.svd(Psi, compute_uv=False) ** 2
        for side, rho in enumerate(_rho(name)):
            w, X = np.linalg.eigh(rho)
            n = rho.shape[0]
            w_ref = np.concatenate([s2, np.zeros(n - len(s2))])
            re, rr, orth = helpers.rdm_ratios(rho, w[::-1], X.T[::-1], w_ref)
            worst[name] = tuple(max(a, b) for a, b in zip(worst.get(name, (0.0, 0.0, 0.0)), (re, rr, orth)))
            assert re <= 1.0 and rr <= 1.0 and orth <= helpers.RDM_ORTH_TOL, (name, side, re, rr, orth)
    for name, (re, rr, orth) in worst.items():
        print("LAPACK %-18s eigenvalue error / bound %.2e  residual / bound %.2e  orthogonality %.2e" % (name, re, rr, orth))
    print("LAPACK worst: %.2e %.2e %.2e" % tuple(max(v[i] for v in worst.values()) for i in range(3)))


def _graded_blocks(psi):
    lsz, rsz, blocks = helpers.RDM_GRADED_LAYOUT
    out, off = [], 0
    for a, b in blocks:
        out.append(psi[off:off + lsz[a] * rsz[b]].reshape(lsz[a], rsz[b]))
        off += lsz[a] * rsz[b]
    assert off == psi.size
    return out


def test_lapack_alone_meets_every_jacobi_bound():
    """The same for the block-Jacobi cases and their bounds (helpers.rdm_jacobi_bounds): the named inputs, the state with a zero, a rank-one
    and an identity block -- at rho = 0 the bounds are their absolute terms, nothing is divided by a norm --, the graded state, and the
    planted spectrum of order 3073 against eigh (eigenvalues only: numpy's products with eigh's 3049 null vectors do not finish in minutes
    on the host; the GPU test forms them on the device)."""
    inputs = [(name, helpers.rdm_input(name)[2]) for name in helpers.RDM_NAMED + helpers.RDM_SPECIAL + ["gaussian_1100x60"]]
    inputs += [("graded_%d" % k, Psi) for k, Psi in enumerate(_graded_blocks(helpers.rdm_graded_state()[1]))]
    for name, Psi in inputs:
        s2 = np.linalg.svd(Psi, compute_uv=False) ** 2
        for side, rho in enumerate((Psi @ Psi.T, Psi.T @ Psi)):
            w, X = np.linalg.eigh(rho)
            n = rho.shape[0]
            w_ref = np.concatenate([s2, np.zeros(n - len(s2))])
            be, br = helpers.rdm_jacobi_bounds(rho, w_ref)
            assert be > 0.0 and br > 0.0 and np.isfinite([be, br]).all()
            re, rr, orth = helpers.rdm_ratios(rho, w[::-1], X.T[::-1], w_ref, jacobi=True)
            print("LAPACK (Jacobi bounds) %-18s side %d n %4d: eigenvalue error / bound %.2e  residual / bound %.2e  orthogonality %.2e" % (name, side, n, re, rr, orth))
            assert re <= 1.0 and rr <= 1.0 and orth <= helpers.RDM_ORTH_TOL, (name, side, re, rr, orth)
    Psi = helpers.rdm_input("planted_3073x24")[2]
    planted = helpers.RDM_PLANTED_S ** 2
    for side, rho in enumerate((Psi @ Psi.T, Psi.T @ Psi)):
        n = rho.shape[0]
        w_ref = np.concatenate([planted, np.zeros(n - 24)])
        err = np.abs(np.linalg.eigvalsh(rho)[::-1] - w_ref).max()
        be = helpers.rdm_jacobi_bounds(rho, w_ref)[0]
        print("LAPACK planted_3073x24 side %d n %d: eigenvalue error %.3e bound %.3e" % (side, n, err, be))
        assert err <= be


def test_special_blocks_and_the_planted_spectrum():
    """The zero block is zero, the rank-one block has one non-zero singular value, the orthogonal block has 48 equal ones, and the planted
    block has the singular values it was built from."""
    zero, one, orth, gauss = (helpers.rdm_input(name)[2] for name in helpers.RDM_SPECIAL)
    assert zero.shape == one.shape == (90, 70) and not zero.any()
    s = np.linalg.svd(one, compute_uv=False)
    assert s[0] > 1.0 and s[1] <= 1e-14 * s[0]
    assert orth.shape == (48, 48) and np.abs(orth @ orth.T * 48.0 - np.eye(48)).max() <= 1e-14
    assert gauss.shape == (40, 33) and np.linalg.matrix_rank(gauss) == 33
    planted, other = (helpers.rdm_input(name)[2] for name in helpers.RDM_SWITCH)
    assert [planted.shape, other.shape] == helpers.RDM_SWITCH_SHAPES
    s = np.linalg.svd(planted, compute_uv=False)
    assert np.abs(s - helpers.RDM_PLANTED_S).max() <= 1e-14 and helpers.RDM_PLANTED_S[0] == 1.0 and np.all(np.diff(helpers.RDM_PLANTED_S) < 0)


def test_the_graded_state_is_the_one_of_the_warm_hint_test():
    """Schmidt values exp(-0.35 k) u_k with u_k in [0.5, 1] per KronBlock, up to the norm c of the state: the j-th largest of a block then
    lies in c [0.5, 1] exp(-0.35 j) (j + 1 of them are at least the lower end, at most j exceed the upper one).  The perturbed state is
    1e-4 away; the junk hints are orthogonal matrices of the right orders, one per density matrix."""
    psi0, psi1, junk = helpers.rdm_graded_state()
    lsz, rsz, blocks = helpers.RDM_GRADED_LAYOUT
    assert psi0.size == psi1.size == sum(lsz[a] * rsz[b] for a, b in blocks) and not psi0.flags.writeable and helpers.rdm_graded_state()[0] is psi0
    assert abs(np.linalg.norm(psi0) - 1.0) <= 1e-15 and abs(np.linalg.norm(psi1) - 1.0) <= 1e-15
    ratios = []
    for Psi in _graded_blocks(psi0):
        s = np.linalg.svd(Psi, compute_uv=False)
        keep = s > 1e-12 * s[0]                                                   # (below that the computed singular values are rounding)
        assert keep.sum() >= min(len(s), 60), (len(s), keep.sum())
        ratios += list((s / np.exp(-0.35 * np.arange(len(s))))[keep])
    print("graded state: sigma_j / exp(-0.35 j) between", min(ratios), "and", max(ratios))
    assert min(ratios) >= 0.5 * max(ratios) * (1.0 - 1e-3)
    d = np.linalg.norm(psi1 - psi0)
    assert 1e-6 < d < 1e-2
    assert sorted(junk) == sorted((side, k) for k in range(4) for side in (0, 1))
    for (side, k), Q in junk.items():
        n = (lsz[blocks[k][0]], rsz[blocks[k][1]])[side]
        assert Q.shape == (n, n) and np.abs(Q @ Q.T - np.eye(n)).max() <= 1e-13


def test_the_model_meets_every_bound_too():
    """The host model the properties are read from computes the same thing as the library is meant to."""
    for name in helpers.RDM_NAMED:
        st = helpers.rdm_named_stats(name)
        re, rr, orth = helpers.rdm_ratios(_rho(name)[0], st["w"][::-1], st["X"].T[::-1])
        print("model %-18s %.2e %.2e %.2e" % (name, re, rr, orth))
        assert re <= 1.0 and rr <= 1.0 and orth <= helpers.RDM_ORTH_TOL, (name, re, rr, orth)


def _one(pattern, src, what):
    m = re.findall(pattern, src)
    assert len(m) == 1, (what, m)
    return m[0]


def _jacobi_constants():
    """The constants of the block-Jacobi path as csrc/rdm.h (the Jacobi block: it also sets the padding of every matrix) and csrc/hqr.hip
    state them: the Jacobi block, the size classes of hqr_panel_regs_kernel (rows, rows per thread), the panel width where the panels are
    stepped and where they are clipped, the strip of the trailing update."""
    rdm, hqr = open(os.path.join(CSRC, "rdm.h")).read(), open(os.path.join(CSRC, "hqr.hip")).read()
    out = {"DMRGX_JB": int(_one(r"#define\s+DMRGX_JB\s+(\d+)", rdm, "DMRGX_JB")), "HR_MAX_ROWS": int(_one(r"\bHR_MAX_ROWS\s*=\s*(\d+)", hqr, "HR_MAX_ROWS"))}
    classes = re.findall(r"if\s*\(nrem\s*<=\s*(\d+)\)\s*hqr_panel_regs_body<(\d+)>", hqr)
    last = _one(r"else\s+hqr_panel_regs_body<(\d+)>", hqr, "the last size class")
    assert [rr for _, rr in classes] + [last] == ["4", "8", "16"], (classes, last)
    assert all(int(rows) == 64 * int(rr) for rows, rr in classes) and out["HR_MAX_ROWS"] == 64 * int(last)      # 64 row blocks of rr rows each
    out["HQR_REGS_ROWS_4"], out["HQR_REGS_ROWS_8"] = (int(rows) for rows, _ in classes)
    assert _one(r"nrem\s*>\s*(\w+)\)\s*return;", hqr, "the upper end of the register panels") == "HR_MAX_ROWS"
    assert _one(r"m\.n\s*-\s*r0\s*<=\s*(\w+)\)\s*return;", hqr, "the lower end of hqr_panel_kernel") == "HR_MAX_ROWS"
    steps = set(re.findall(r"r0\s*\+=\s*(\d+)", hqr)) | set(re.findall(r"pw\s*=\s*(?:std::)?min\((\d+),\s*nrem\)", hqr))
    assert len(steps) == 1, steps
    out["HQR_PANEL"] = int(steps.pop())
    out["TM_COLS"] = int(_one(r"\bTM_COLS\s*=\s*(\d+)\s*\*\s*TM_NBW", hqr, "TM_COLS")) * int(_one(r"\bTM_NBW\s*=\s*(\d+)", hqr, "TM_NBW"))
    return out


def _constants():
    src = "".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.startswith("symeig") and f.endswith((".hip", ".h")))
    out = _jacobi_constants()
    for name in helpers.RDM_CONSTANTS:
        if name in out:
            continue
        m = re.findall(r"(?:#define\s+%s\s+|constexpr\s+int\s+(?:\w+\s*=\s*\d+\s*,\s*)*%s\s*=\s*)(\d+)" % (name, name), src)
        assert len(m) == 1, (name, m)
        out[name] = int(m[0])
    return out


def test_the_jacobi_order_lists_straddle_the_library_constants():
    """The orders of the block-Jacobi cases sit on the edges of csrc/rdm_jacobi.hip and csrc/hqr.hip as they are today: a retune of the Jacobi block,
    of a size class of the register panels, of the panel width or of the strip of the trailing update must fail here, not silently move an
    edge out of the lists."""
    c = _constants()
    jb, r4, r8, rmax, panel, strip, max_n = (c[k] for k in ("DMRGX_JB", "HQR_REGS_ROWS_4", "HQR_REGS_ROWS_8", "HR_MAX_ROWS", "HQR_PANEL", "TM_COLS", "SYMEIG_MAX_N"))
    assert (jb, r4, r8, rmax, panel, strip) == (16, 256, 512, 1024, 32, 32)
    small, calls = set(range(1, 41)), helpers.RDM_HQR_EDGE_CALLS
    edge = {n for call in calls for n in call}
    assert {1, 2, 2 * jb - 1, 2 * jb, 2 * jb + 1} <= small                        # no QR at n = 1; one padded pair up to 2 JB, two blocks more above
    assert [min(call) <= r <= max(call) - 1 for call, r in zip(calls, (r4, r8, rmax))] == [True] * 3      # one call per edge, both sides in it
    for r in (r4, r8, rmax):
        assert {r, r + 1} <= edge                                                # the first panel in either body
    assert {r4 - 1, r8 - 1} <= edge
    assert max(edge) > rmax and max(edge) - (max(edge) - rmax + panel - 1) // panel * panel > r8      # the largest order walks down through every class
    for div in (panel, strip):                                                   # a last panel narrower than 32; a partial strip of the trailing update
        assert any(n % div for n in edge) and any(n % div == 0 for n in edge)
    assert {n % panel for n in edge | small} >= {0, 1, 2, panel - 1}
    (big, _), (mid, _) = helpers.RDM_SWITCH_SHAPES
    assert big == max_n + 1 and rmax < mid <= 1100                                # the smallest order that switches; the project's orthogonality figure holds up to 1100
    both = [r0 for r0 in range(0, mid, panel) if big - r0 > rmax and 0 < mid - r0 <= rmax]
    assert both, "no panel step at which both kernels of hqr_batched are launched"
    assert max(edge) <= 1100 and max(max(s) for s in helpers.RDM_SWITCH_SHAPES) == big


def test_the_order_lists_still_straddle_the_library_constants():
    """A retune of the leaf size, the fused-kernel threshold, the WY block, the matrices per launch, the prefetch depth or the largest order must
    fail here loudly, not silently uncover an edge."""
    c = _constants()
    assert c == helpers.RDM_CONSTANTS == {"DMRGX_DC_LEAF": 16, "DC_FUSE_NL": 384, "DMRGX_WY_NB": 64, "TRID_MAXM": 32, "TRID_PF": 8, "SYMEIG_MAX_N": 3072,
                                          "DMRGX_JB": 16, "HQR_REGS_ROWS_4": 256, "HQR_REGS_ROWS_8": 512, "HR_MAX_ROWS": 1024, "HQR_PANEL": 32, "TM_COLS": 32}
    leaf, fuse, nb, maxm, pf = c["DMRGX_DC_LEAF"], c["DC_FUSE_NL"], c["DMRGX_WY_NB"], c["TRID_MAXM"], c["TRID_PF"]
    small, edge = list(range(1, 41)), helpers.RDM_EDGE_ORDERS
    assert sorted(o for call in helpers.RDM_EDGE_CALLS for o in call) == edge and max(edge) <= c["SYMEIG_MAX_N"]
    assert {leaf - 1, leaf, leaf + 1, 2 * leaf - 1, 2 * leaf, 2 * leaf + 1} <= set(small)          # one leaf / two leaves; two levels begin at 2 leaf + 1
    for p in (2, 3, 5, 6):                                                       # a level more begins at leaf 2^p + 1
        assert {leaf << p, (leaf << p) + 1} <= set(edge), p
    assert {fuse - 1, fuse, fuse + 1, 2 * fuse, 2 * fuse + 1} <= set(edge)          # the top merge, and the two merges below the top
    assert {0, 1, nb - 1} <= {(n - 2) % nb for n in edge}                         # the last WY block: full, of one reflector, one short of full
    assert {1, 2, 3} <= set(small) and {nb + 1, nb + 2} <= set(edge)              # no reflector at all, the first one; one block short of full, exactly full
    assert {64 * pf - 1, 64 * pf, 64 * pf + 1} <= set(edge)                       # the prefetch chunk of trid_step_kernel
    assert 2 * len(small) > 2 * maxm                                              # 80 matrices: three launch groups / rounds of at most 32
    assert [helpers.rdm_tree_bounds(n)[0] for n in (16, 17, 32, 33, 64, 65, 1024, 1025)] == [0, 1, 1, 2, 2, 3, 6, 7]
