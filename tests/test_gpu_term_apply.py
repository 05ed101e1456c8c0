"""dmrgx_kron_term_apply: the image vectors v_a = sum_t c_t (A_t (x) B_t) psi themselves, against dense numpy (-m gpu).

Reference: psi embedded as the n_L x n_R matrix Psi of the full product space, v_a = sum_t c_t A_t Psi B_t^T, read back on the KronBlocks.
The planted superblock of test_gpu_gram (sectors [3, 4, 2] x [5, 1, 6], KronBlocks (0,2), (1,1), (2,0)) is the smallest shape that
reaches dense, identity and offset cells, transposed reads and missing shifted sectors.

Run as a script (`test_gpu_term_apply.py OUT.npy`) this file is the child of the poisoned-workspace test: it saves Y."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                      # (the child process: pytest's conftest is not there to set the path)
    sys.path.insert(0, ROOT)

from test_gpu_gram import BLOCKS, LSZ, RSZ, _dense, _embed  # noqa: E402
from test_gpu_term_gram import _planted_case  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_OUTOFRANGE = 62, 63
FAMILY = "two_sided_shift0"      # c psi, one-sided left and right terms, two-sided (+1,-1) and (-1,+1) terms, several per vector
N_STATES = sum(LSZ[a] * RSZ[b] for a, b in BLOCKS)


@pytest.fixture(scope="module")
def mods(pkg):
    from dmrgx_amd import superblock, workloads, _capi
    _capi.require_device()
    return superblock, workloads, _capi


def _extract(M, lsz, rsz, blocks):
    """the n_L x n_R matrix of the full product space -> the vector on the KronBlocks, and what lies outside them"""
    loff, roff = np.concatenate([[0], np.cumsum(lsz)]), np.concatenate([[0], np.cumsum(rsz)])
    rest = M.copy()
    parts = []
    for il, ir in blocks:
        parts.append(M[loff[il]:loff[il + 1], roff[ir]:roff[ir + 1]].ravel())
        rest[loff[il]:loff[il + 1], roff[ir]:roff[ir + 1]] = 0.0
    return np.concatenate(parts), rest


def _reference(psi, lsz, rsz, blocks, left_ops, right_ops, vectors):
    """-> (Y, bound): the dense images on the KronBlocks and, per vector, sum_t |c_t| |A_t| |B_t| |psi| (spectral norms)."""
    Psi = _embed(psi, lsz, rsz, blocks)
    A = [_dense(a, lsz) for a in left_ops]
    B = [_dense(b, rsz) for b in right_ops]
    Y, bound = [], []
    for terms in vectors:
        v, s = np.zeros_like(Psi), 0.0
        for c, l, r in terms:
            X = Psi if l is None else A[l] @ Psi
            v += c * (X if r is None else X @ B[r].T)
            s += abs(c) * (1.0 if l is None else np.linalg.norm(A[l], 2)) * (1.0 if r is None else np.linalg.norm(B[r], 2))
        y, rest = _extract(v, lsz, rsz, blocks)
        assert np.abs(rest).max() == 0.0          # total shift 0: the image lives on the KronBlocks
        Y.append(y)
        bound.append(s * np.linalg.norm(psi))
    return np.array(Y), np.array(bound)


def test_term_apply_planted_superblock(mods):
    """Y against the dense image to 1e-13 sum |c| |A| |B| |psi| per vector; its numpy Gram matrix against dmrgx_kron_term_gram of the same
    vectors to 1e-12 absolute (the images of the two calls are the same products: what differs is the order in which the products of an
    entry are added, on entries of up to a few hundred, whose float64 rounding is a few 1e-14).  Y arrives full of NaN with ldy > n_states:
    every element below n_states comes back finite -- zeros where no term reaches --, the pad stays NaN.  Two calls give the same bits."""
    import torch
    sbm, wl, _ = mods
    psi, left, right, vectors = _planted_case(wl, FAMILY)
    vectors = vectors + [[(1.0, 2, None)]]       # L0_ident_off has no cell in sector 2: KronBlock (2, 0) is reached by nothing
    want, bound = _reference(psi, LSZ, RSZ, BLOCKS, left, right, vectors)
    assert np.abs(want).max() > 0.1 and (want[-1][-LSZ[2] * RSZ[0]:] == 0.0).all() and np.abs(want[-1]).max() > 0.1
    nv, ldy = len(vectors), N_STATES + 5
    Y = torch.full((nv, ldy), float("nan"), dtype=torch.float64, device="cuda")
    out = sbm.term_apply((LSZ, RSZ, BLOCKS), psi, left, right, vectors, out=Y)
    assert out is Y
    got = Y.cpu().numpy()
    assert np.isnan(got[:, N_STATES:]).all()
    got = got[:, :N_STATES]
    assert np.isfinite(got).all()
    err = np.abs(got - want).max(axis=1)
    print("term_apply: max |Y - dense| per vector", err, "bounds", 1e-13 * bound)
    assert (err <= 1e-13 * bound).all(), (err, 1e-13 * bound)
    assert (got[-1][-LSZ[2] * RSZ[0]:] == 0.0).all()
    G, _ = sbm.term_gram((LSZ, RSZ, BLOCKS), psi, left, right, vectors)
    G = G.cpu().numpy()
    gerr = np.abs(got @ got.T - G).max()
    print("term_apply: max |Y Y^T - term_gram|", gerr, "max |G|", np.abs(G).max())
    assert gerr <= 1e-12
    Y2 = sbm.term_apply((LSZ, RSZ, BLOCKS), psi, left, right, vectors)        # default output: ldy == n_states
    assert Y2.shape == (nv, N_STATES)
    assert np.array_equal(Y2.cpu().numpy().view(np.uint64), got.view(np.uint64))


def test_term_apply_refusals(mods):
    """Total shift != 0, an operator index outside its list, an empty vector, ldy < n_states and a Y that overlaps psi are refused; Y is
    left alone."""
    import ctypes as C
    import torch
    sbm, wl, capi = mods
    layout = (LSZ, RSZ, BLOCKS)
    psi, left, right, vectors = _planted_case(wl, FAMILY)
    _, _, _, plus = _planted_case(wl, "two_sided_plus")
    Y = torch.full((len(vectors) + 1, N_STATES), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(capi.DmrgxError) as e:
        sbm.term_apply(layout, psi, left, right, plus, out=Y)                         # every term has total shift +1
    assert e.value.code == ERR_ARG and "shift" in str(e.value)
    with pytest.raises(capi.DmrgxError) as e:
        sbm.term_apply(layout, psi, left, right, vectors + [plus[1]], out=Y)           # one vector of another shift
    assert e.value.code == ERR_ARG and "shift" in str(e.value)
    for bad in ((1.0, 7, None), (1.0, None, 7), (1.0, -2, 0)):
        with pytest.raises(capi.DmrgxError) as e:
            sbm.term_apply(layout, psi, left, right, vectors[:2] + [[bad]], out=Y)
        assert e.value.code == ERR_OUTOFRANGE, bad
    with pytest.raises(capi.DmrgxError) as e:
        sbm.term_apply(layout, psi, left, right, [vectors[0], [], vectors[1]], out=Y)
    assert e.value.code == ERR_ARG
    short = torch.full((2, N_STATES - 1), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(capi.DmrgxError) as e:
        sbm.term_apply(layout, psi, left, right, vectors[:2], out=short)
    assert e.value.code == ERR_ARG and "ldy" in str(e.value)
    # Y overlapping psi: the second vector of a buffer whose tail is psi
    buf = torch.zeros(2 * N_STATES, dtype=torch.float64, device="cuda")
    buf[N_STATES:] = torch.from_numpy(psi).cuda()
    with pytest.raises(capi.DmrgxError) as e:
        sbm.term_apply(layout, buf[N_STATES:], left, right, vectors[:2], out=buf.view(2, N_STATES))
    assert e.value.code == ERR_ARG and "overlap" in str(e.value)
    assert (Y == 7.0).all() and (short == 7.0).all()
    # a null Y
    args, psi_d, keep = sbm._gram_arguments(layout, psi, left, right)
    first, terms = (C.c_int32 * 2)(0, 1), (capi.Term * 1)()
    terms[0].a, terms[0].left_op, terms[0].right_op = 1.0, -1, -1
    assert capi.lib().dmrgx_kron_term_apply(*args, 1, first, terms, None, N_STATES, None) == ERR_ARG


def test_image_outside_the_kronblocks_is_refused(mods):
    """Without KronBlock (1, 1) the (+1, -1) term maps (0, 2) to an existing sector pair that the layout does not hold: refused, not dropped."""
    sbm, wl, capi = mods
    psi, left, right, vectors = _planted_case(wl, FAMILY)
    blocks = [BLOCKS[0], BLOCKS[2]]
    psi2 = np.concatenate([psi[:LSZ[0] * RSZ[2]], psi[-LSZ[2] * RSZ[0]:]])
    with pytest.raises(capi.DmrgxError) as e:
        sbm.term_apply((LSZ, RSZ, blocks), psi2, left, right, [vectors[7]])          # LpT (x) Rp: shift (-1, +1)
    assert e.value.code == ERR_ARG and "KronBlock" in str(e.value)
    Y = sbm.term_apply((LSZ, RSZ, blocks), psi2, left, right, [vectors[1]])           # shift (0, 0) stays inside: fine
    assert np.isfinite(Y.cpu().numpy()).all()


def test_poisoned_workspace_gives_the_same_bits(mods, tmp_path):
    """The same family in a child process under DMRGX_POOL_POISON=1 (intermediates and materialised operands come from the pool filled
    with NaN): Y is finite and bit-identical to the clean run in this process."""
    from test_gpu_poison import _child
    sbm, wl, _ = mods
    psi, left, right, vectors = _planted_case(wl, FAMILY)
    Y = sbm.term_apply((LSZ, RSZ, BLOCKS), psi, left, right, vectors).cpu().numpy()
    out = str(tmp_path / "poisoned.npy")
    p = _child([os.path.join("tests", "test_gpu_term_apply.py"), out], True, 300)
    assert p.returncode == 0 and "term apply child ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    Yp = np.load(out)
    assert np.isfinite(Yp).all() and np.array_equal(Y.view(np.uint64), Yp.view(np.uint64))


if __name__ == "__main__":
    from __graft_entry__ import load_package
    load_package()
    from dmrgx_amd import superblock as sbm_child, workloads as wl_child
    assert os.environ.get("DMRGX_POOL_POISON") == "1"
    psi_c, left_c, right_c, vectors_c = _planted_case(wl_child, FAMILY)
    Y_child = sbm_child.term_apply((LSZ, RSZ, BLOCKS), psi_c, left_c, right_c, vectors_c)
    np.save(sys.argv[1], Y_child.cpu().numpy())
    print("term apply child ok")
