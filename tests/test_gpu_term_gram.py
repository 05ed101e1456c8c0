"""dmrgx_kron_term_gram: the Gram matrix of images that are sums of terms c A (x) B, against dense numpy (-m gpu).

Reference: psi embedded as the n_L x n_R matrix Psi of the full product space, v_a = sum_t c_t (A_t Psi B_t^T).ravel(), G = V V^T.
The bound is test_gpu_gram._check's, 1e-13 max(1, max |want|): the one the project uses for these sizes.

Run as a script (`test_gpu_term_gram.py OUT.npy`) this file is the child of the poisoned-workspace test: it runs one family and saves G."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                      # (the child process: pytest's conftest is not there to set the path)
    sys.path.insert(0, ROOT)

from test_gpu_gram import BLOCKS, LSZ, RSZ, _check, _dense, _embed, _planted  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_OUTOFRANGE = 62, 63


@pytest.fixture(scope="module")
def mods(pkg):
    from dmrgx_amd import superblock, workloads, _capi
    _capi.require_device()
    return superblock, workloads, _capi


def _reference(psi, lsz, rsz, blocks, left_ops, right_ops, vectors):
    Psi = _embed(psi, lsz, rsz, blocks)
    A = [_dense(a, lsz) for a in left_ops]
    B = [_dense(b, rsz) for b in right_ops]
    V = []
    for terms in vectors:
        v = np.zeros_like(Psi)
        for c, l, r in terms:
            X = Psi if l is None else A[l] @ Psi
            v += c * (X if r is None else X @ B[r].T)
        V.append(v.ravel())
    V = np.array(V)
    return V @ V.T


def _planted_case(wl, family):
    """-> (psi, left_ops, right_ops, vectors) on the planted superblock of test_gpu_gram."""
    rng = np.random.default_rng(47)
    o = _planted(wl, rng)
    psi = rng.standard_normal(sum(LSZ[a] * RSZ[b] for a, b in BLOCKS))
    left = [o["L0_partial"], o["L0_ident"], o["L0_ident_off"], o["Lp"], (o["Lm"], True), o["Lp_ident"], (o["Lp"], True)]
    right = [o["R0_partial"], o["R0_ident"], o["R0_ident_off"], o["Rp"], (o["Rm"], True), (o["Rp"], True), o["Rm"]]
    L0p, L0i, L0o, Lp, LmT, Lpi, LpT = range(7)          # LmT, Lp, Lpi: shift +1; LpT: shift -1
    R0p, R0i, R0o, Rp, RmT, RpT, Rm = range(7)           # Rp, RmT: shift +1; RpT, Rm: shift -1
    vectors = {
        # a. one one-sided term per vector (what dmrgx_kron_op_gram builds)
        "one_sided_shift0": [[(1.0, L0p, None)], [(1.0, L0i, None)], [(1.0, L0o, None)], [(1.0, None, R0p)], [(1.0, None, R0i)], [(1.0, None, R0o)]],
        "one_sided_plus": [[(1.0, Lp, None)], [(1.0, LmT, None)], [(1.0, Lpi, None)], [(1.0, None, Rp)], [(1.0, None, RmT)]],
        # b. total shift 0 with two-sided terms
        "two_sided_shift0": [
            [(1.0, None, None)],                                                    # psi itself
            [(0.7, L0p, R0p)],                                                      # c L0 (x) R0
            [(1.0, Lp, RpT)],                                                       # shift +1 (x) shift -1 (a transposed right operator)
            [(-1.3, LmT, Rm)],                                                      # a transposed left operator (x) a stored shift -1
            [(0.5, L0o, R0o), (1.0, Lp, RpT), (-0.25, LmT, Rm)],                    # all of these in one image, from three source blocks
            [(2.0, L0p, None), (0.3, L0i, R0p)],                                    # one-sided + two-sided, both cut the rows
            [(1.5, None, R0p), (0.5, Lpi, RpT), (-0.5, None, None)],                # a right one-sided term beside left-applied ones
            [(0.9, LpT, Rp)],                                                       # shift -1 (x) shift +1
        ],
        # c. total shift +1: KronBlock (0, 2) has no left partner, (2, 0) no right partner
        "two_sided_plus": [
            [(1.0, Lp, R0p), (0.8, L0p, Rp)],
            [(1.0, Lp, None)],
            [(0.6, L0o, RmT), (1.0, None, Rp)],
            [(-2.0, LmT, R0o)],
        ],
    }[family]
    return psi, left, right, vectors


FAMILIES = ["one_sided_shift0", "one_sided_plus", "two_sided_shift0", "two_sided_plus"]


@pytest.mark.parametrize("family", FAMILIES)
def test_term_gram_planted_superblock(mods, family):
    """Sectors [3, 4, 2] x [5, 1, 6] (a one-state sector), KronBlocks (0,2), (1,1), (2,0); operators with partial, overlapping, identity
    and offset-identity cells."""
    sbm, wl, _ = mods
    psi, left, right, vectors = _planted_case(wl, family)
    want = _reference(psi, LSZ, RSZ, BLOCKS, left, right, vectors)
    assert np.abs(want).max() > 0.1
    G, rep = sbm.term_gram((LSZ, RSZ, BLOCKS), psi, left, right, vectors)
    G = G.cpu().numpy()
    _check(G, want)
    assert np.array_equal(G, G.T) and rep.slices == 1
    G2, _ = sbm.term_gram((LSZ, RSZ, BLOCKS), psi, left, right, vectors)
    assert np.array_equal(G.view(np.uint64), G2.cpu().numpy().view(np.uint64))
    if family.startswith("one_sided"):                            # the same operators through dmrgx_kron_op_gram
        lops = [left[t[0][1]] for t in vectors if t[0][1] is not None]
        rops = [right[t[0][2]] for t in vectors if t[0][2] is not None]
        Gop, _ = sbm.op_gram((LSZ, RSZ, BLOCKS), psi, lops, rops)
        _check(G, Gop.cpu().numpy())
    if family == "two_sided_shift0":
        assert abs(G[0, 0] - psi @ psi) <= 1e-13 * (psi @ psi)


def _sliced_case(wl):
    rng = np.random.default_rng(53)
    lsz, rsz, blocks = [90, 40, 30], [60, 70, 50], [(0, 2), (1, 1), (2, 0)]
    D = wl.CELL_DENSE

    def full(sizes, scale):
        return wl.SectorOperator(0, [wl.OpCell(q, 0, 0, n, n, D, 0.0, scale * rng.standard_normal((n, n))) for q, n in enumerate(sizes)])

    def halves(sizes, scale):                                     # two dense cells per sector, as an enlarged block's operators have
        cells = []
        for q, n in enumerate(sizes):
            h = n // 2
            cells += [wl.OpCell(q, 0, 0, h, h, D, 0.0, scale * rng.standard_normal((h, h))),
                      wl.OpCell(q, h, h, n - h, n - h, D, 0.0, scale * rng.standard_normal((n - h, n - h)))]
        return wl.SectorOperator(0, cells)

    left, right = [full(lsz, 0.1), halves(lsz, 0.2)], [full(rsz, 0.1), halves(rsz, 0.2)]
    vectors = [[(1.0, None, None)], [(1.0, 0, None)], [(0.5, 1, 0)], [(1.0, None, 1)], [(0.25, 0, 1), (1.0, 1, None)], [(1.0, None, 0), (-0.5, None, None)]]
    psi = rng.standard_normal(sum(lsz[a] * rsz[b] for a, b in blocks))
    psi /= np.linalg.norm(psi)
    return lsz, rsz, blocks, psi, left, right, vectors


def test_term_gram_workspace_slices_and_refusals(mods):
    """K not a multiple of 16 and a 90-wide extent (more than one 64 tile); a workspace that holds one image block at a time gives three
    slices with the intermediates of the two-sided terms formed per slice; one byte less is refused, and so are mixed total shifts, an
    operator index outside its list and an empty vector."""
    sbm, wl, capi = mods
    lsz, rsz, blocks, psi, left, right, vectors = _sliced_case(wl)
    layout = (lsz, rsz, blocks)
    want = _reference(psi, lsz, rsz, blocks, left, right, vectors)
    assert np.abs(want).max() > 0.1
    largest = max(lsz[a] * rsz[b] for a, b in blocks) * len(vectors) * 8
    G1, rep1 = sbm.term_gram(layout, psi, left, right, vectors)
    G3, rep3 = sbm.term_gram(layout, psi, left, right, vectors, workspace_bytes=largest)
    assert rep1.slices == 1 and rep3.slices >= 3, (rep1.slices, rep3.slices)
    for G in (G1, G3):
        G = G.cpu().numpy()
        _check(G, want)
        assert np.array_equal(G, G.T)
    with pytest.raises(capi.DmrgxError) as e:
        sbm.term_gram(layout, psi, left, right, vectors, workspace_bytes=largest - 1)
    assert e.value.code == ERR_ARG and "workspace" in str(e.value)
    plus = wl.SectorOperator(+1, [wl.OpCell(0, 0, 0, 90, 40, wl.CELL_DENSE, 0.0, np.ones((90, 40)))])
    with pytest.raises(capi.DmrgxError) as e:
        sbm.term_gram(layout, psi, left + [plus], right, vectors + [[(1.0, 2, None)]])
    assert e.value.code == ERR_ARG and "shift" in str(e.value)
    with pytest.raises(capi.DmrgxError) as e:
        sbm.term_gram(layout, psi, left + [plus], right, [[(1.0, 0, 0), (1.0, 2, 1)]])      # inside one vector
    assert e.value.code == ERR_ARG and "shift" in str(e.value)
    for bad in ((1.0, 2, None), (1.0, None, 2), (1.0, -2, 0)):
        with pytest.raises(capi.DmrgxError) as e:
            sbm.term_gram(layout, psi, left, right, vectors + [[bad]])
        assert e.value.code == ERR_OUTOFRANGE, bad
    with pytest.raises(capi.DmrgxError) as e:
        sbm.term_gram(layout, psi, left, right, [vectors[0], [], vectors[1]])
    assert e.value.code == ERR_ARG


POISON_FAMILY = "two_sided_shift0"


def test_poisoned_workspace_gives_the_same_bits(mods, tmp_path):
    """One two-sided family in a child process under DMRGX_POOL_POISON=1 (images, intermediates, materialised operands and the Gram slab
    all come from the pool filled with NaN): the result is finite and bit-identical to the clean run in this process."""
    from test_gpu_poison import _child
    sbm, wl, _ = mods
    psi, left, right, vectors = _planted_case(wl, POISON_FAMILY)
    G, _ = sbm.term_gram((LSZ, RSZ, BLOCKS), psi, left, right, vectors)
    G = G.cpu().numpy()
    out = str(tmp_path / "poisoned.npy")
    p = _child([os.path.join("tests", "test_gpu_term_gram.py"), out], True, 300)
    assert p.returncode == 0 and "term gram child ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    Gp = np.load(out)
    assert np.isfinite(Gp).all() and np.array_equal(G.view(np.uint64), Gp.view(np.uint64))


if __name__ == "__main__":
    from __graft_entry__ import load_package
    load_package()
    from dmrgx_amd import superblock as sbm_child, workloads as wl_child
    assert os.environ.get("DMRGX_POOL_POISON") == "1"
    psi_c, left_c, right_c, vectors_c = _planted_case(wl_child, POISON_FAMILY)
    G_child, _ = sbm_child.term_gram((LSZ, RSZ, BLOCKS), psi_c, left_c, right_c, vectors_c)
    np.save(sys.argv[1], G_child.cpu().numpy())
    print("term gram child ok")
