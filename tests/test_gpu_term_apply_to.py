"""dmrgx_kron_term_apply_to: the image vectors v_a = sum_t c_t (A_t (x) B_t) psi written in the layout of ANOTHER KronBlock list -- the
sector the total shift of the terms leads to --, against dense numpy (-m gpu).

Reference, as in test_gpu_term_apply: psi embedded as the n_L x n_R matrix Psi of the full product space, v_a = sum_t c_t A_t Psi B_t^T
(the dense Kronecker product applied to psi), read back on the OUTPUT KronBlocks; what lies outside them must be zero.

The planted superblock: left sectors (3, 70, 1, 5), right sectors (2, 4, 67, 3) -- 70 and 67 cross the 64-wide tile on both sides, one
sector has a single state --, psi on the KronBlocks IL + IR = 3.  A total shift s leads to the KronBlocks IL + IR = 3 - s.

Run as a script (`test_gpu_term_apply_to.py OUT.npy`) this file is the child of the poisoned-workspace test: it saves both Y."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                      # (the child process: pytest's conftest is not there to set the path)
    sys.path.insert(0, ROOT)

from test_gpu_gram import _dense, _embed  # noqa: E402
from test_gpu_term_apply import _extract  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_OUTOFRANGE = 62, 63
LSZ, RSZ = [3, 70, 1, 5], [2, 4, 67, 3]
IN_BLOCKS = [(0, 3), (1, 2), (2, 1), (3, 0)]
OUT_BLOCKS = {+1: [(0, 2), (1, 1), (2, 0)], -1: [(1, 3), (2, 2), (3, 1)], 0: IN_BLOCKS}
N_IN = sum(LSZ[a] * RSZ[b] for a, b in IN_BLOCKS)


def _n_out(s):
    return sum(LSZ[a] * RSZ[b] for a, b in OUT_BLOCKS[s])


@pytest.fixture(scope="module")
def mods(pkg):
    from dmrgx_amd import superblock, workloads, _capi
    _capi.require_device()
    return superblock, workloads, _capi


def _case(wl):
    """-> (psi, left_ops, right_ops, {s: vectors}).  Operators of shift 0, +1, -1 on both sides (and +2, -2 on the right), of dense cells,
    identity cells and identity cells with offsets; the left shift -1 operator is a shift +1 operator stored transposed."""
    rng = np.random.default_rng(101)
    D, I = wl.CELL_DENSE, wl.CELL_IDENT

    def full(sizes, shift, skip=()):
        cells = []
        for q, n in enumerate(sizes):
            if 0 <= q + shift < len(sizes) and q not in skip:
                cells.append(wl.OpCell(q, 0, 0, n, sizes[q + shift], D, 0.0, rng.standard_normal((n, sizes[q + shift])) / np.sqrt(sizes[q + shift])))
        return wl.SectorOperator(shift, cells)

    L0 = wl.SectorOperator(0, [wl.OpCell(0, 0, 0, 3, 3, I, 0.7), wl.OpCell(1, 0, 0, 70, 70, D, 0.0, rng.standard_normal((70, 70)) / 8), wl.OpCell(2, 0, 0, 1, 1, I, -1.1),
                               wl.OpCell(3, 1, 0, 4, 4, I, 0.4)])
    Lp = full(LSZ, +1)                                         # 3 x 70, 70 x 1, 1 x 5
    LmT = (full(LSZ, +1), True)                                # shift -1, read transposed
    Lp_off = wl.SectorOperator(+1, [wl.OpCell(0, 0, 65, 3, 3, I, 0.9), wl.OpCell(2, 0, 2, 1, 1, I, -0.6)])      # sector 1 is reached by no cell
    R0 = wl.SectorOperator(0, [wl.OpCell(0, 0, 0, 2, 2, D, 0.0, rng.standard_normal((2, 2))), wl.OpCell(1, 0, 0, 4, 4, I, 1.3), wl.OpCell(2, 0, 0, 67, 67, D, 0.0, rng.standard_normal((67, 67)) / 8),
                               wl.OpCell(3, 0, 0, 3, 3, I, -0.8)])
    Rp = wl.SectorOperator(+1, [wl.OpCell(0, 0, 0, 2, 4, D, 0.0, rng.standard_normal((2, 4))), wl.OpCell(1, 0, 5, 4, 4, I, 0.8), wl.OpCell(1, 0, 9, 4, 58, D, 0.0, rng.standard_normal((4, 58)) / 8),
                                wl.OpCell(2, 0, 0, 67, 3, D, 0.0, rng.standard_normal((67, 3)))])
    Rm = full(RSZ, -1)
    Rpp, Rmm = full(RSZ, +2), full(RSZ, -2)
    left = [L0, Lp, LmT, Lp_off]
    right = [R0, Rp, Rm, Rpp, Rmm]
    iL0, iLp, iLm, iLo = range(4)
    iR0, iRp, iRm, iRpp, iRmm = range(5)
    vectors = {
        # total shift +1: one-sided terms, (+1, 0), (0, +1) and (-1, +2)
        +1: [[(0.5, iLp, None), (-1.5, None, iRp), (0.9, iLo, None)],
             [(0.7, iLp, iR0), (1.25, iL0, iRp), (-0.3, iLm, iRpp)],
             [(2.0, iLm, iRpp)],                                # reaches (1, 1) and (2, 0) only: (0, 2) stays zero; source (2, 1) -> (3, -1) does not exist
             ],
        # total shift -1: one-sided terms, (-1, 0), (0, -1) and (+1, -2)
        -1: [[(0.5, iLm, None), (-1.5, None, iRm)],
             [(0.7, iLm, iR0), (1.25, iL0, iRm), (-0.3, iLp, iRmm)],
             [(2.0, iLp, iRmm)],                                # reaches (1, 3) and (2, 2) only: (3, 1) stays zero; sources (0, 3), (1, 2) have no image
             ],
        # total shift 0 (the layout of psi): what dmrgx_kron_term_apply does
        0: [[(0.5, None, None), (0.75, iL0, None)], [(0.7, iLp, iRm), (1.25, iL0, iR0)], [(-0.3, iLm, iRp), (1.0, None, iR0)]],
    }
    psi = rng.standard_normal(N_IN)
    return psi, left, right, vectors


def _reference(psi, left_ops, right_ops, vectors, out_blocks):
    """-> (Y, bound): the dense images on the output KronBlocks and, per vector, sum_t |c_t| |A_t| |B_t| |psi| (spectral norms)."""
    Psi = _embed(psi, LSZ, RSZ, IN_BLOCKS)
    A = [_dense(a, LSZ) for a in left_ops]
    B = [_dense(b, RSZ) for b in right_ops]
    Y, bound = [], []
    for terms in vectors:
        v, s = np.zeros_like(Psi), 0.0
        for c, l, r in terms:
            X = Psi if l is None else A[l] @ Psi
            v += c * (X if r is None else X @ B[r].T)
            s += abs(c) * (1.0 if l is None else np.linalg.norm(A[l], 2)) * (1.0 if r is None else np.linalg.norm(B[r], 2))
        y, rest = _extract(v, LSZ, RSZ, out_blocks)
        assert np.abs(rest).max() == 0.0          # the image lives on the output KronBlocks
        Y.append(y)
        bound.append(s * np.linalg.norm(psi))
    return np.array(Y), np.array(bound)


@pytest.fixture(scope="module")
def planted(mods):
    """The case and its dense references, built once and never changed."""
    _, wl, _ = mods
    psi, left, right, vectors = _case(wl)
    ref = {s: _reference(psi, left, right, vectors[s], OUT_BLOCKS[s]) for s in (+1, -1, 0)}
    return psi, left, right, vectors, ref


@pytest.mark.parametrize("s", [+1, -1])
def test_term_apply_to_planted_superblock(mods, planted, s):
    """Y against the dense image to 1e-13 sum |c| |A| |B| |psi| per vector (the bound of test_gpu_term_apply).  Y arrives full of NaN with
    ldy = n_out + 3: every element below n_out comes back finite, the three trailing columns stay NaN.  The output block that the last
    vector does not reach is exact zeros.  Two calls give the same bits."""
    import torch
    sbm, _, _ = mods
    psi, left, right, vectors, ref = planted
    want, bound = ref[s]
    n_out, out = _n_out(s), OUT_BLOCKS[s]
    unreached = out[0] if s > 0 else out[-1]
    o0 = sum(LSZ[a] * RSZ[b] for a, b in out[:out.index(unreached)])
    zero = slice(o0, o0 + LSZ[unreached[0]] * RSZ[unreached[1]])
    assert np.abs(want).max() > 0.1 and (want[2][zero] == 0.0).all() and np.abs(want[2]).max() > 0.1 and np.abs(want[1][zero]).max() > 0.01
    Y = torch.full((3, n_out + 3), float("nan"), dtype=torch.float64, device="cuda")
    ret = sbm.term_apply_to((LSZ, RSZ, IN_BLOCKS), psi, left, right, vectors[s], out, out=Y)
    assert ret is Y
    got = Y.cpu().numpy()
    assert np.isnan(got[:, n_out:]).all()
    got = got[:, :n_out]
    assert np.isfinite(got).all()
    err = np.abs(got - want).max(axis=1)
    print("term_apply_to s=%+d: max |Y - dense| per vector" % s, err, "bounds", 1e-13 * bound)
    assert (err <= 1e-13 * bound).all(), (err, 1e-13 * bound)
    assert (got[2][zero] == 0.0).all()
    Y2 = sbm.term_apply_to((LSZ, RSZ, IN_BLOCKS), psi, left, right, vectors[s], out)        # default output: ldy == n_out
    assert Y2.shape == (3, n_out)
    assert np.array_equal(Y2.cpu().numpy().view(np.uint64), got.view(np.uint64))


def test_same_list_in_and_out_is_term_apply(mods, planted):
    """s = 0 with the output list equal to the input list: the bits of dmrgx_kron_term_apply, and the dense image."""
    sbm, _, _ = mods
    psi, left, right, vectors, ref = planted
    want, bound = ref[0]
    layout = (LSZ, RSZ, IN_BLOCKS)
    Y0 = sbm.term_apply(layout, psi, left, right, vectors[0]).cpu().numpy()
    Y1 = sbm.term_apply_to(layout, psi, left, right, vectors[0], IN_BLOCKS).cpu().numpy()
    assert np.array_equal(Y0.view(np.uint64), Y1.view(np.uint64))
    err = np.abs(Y1 - want).max(axis=1)
    assert (err <= 1e-13 * bound).all(), (err, 1e-13 * bound)
    # the same blocks listed in another order: the same numbers at the offsets of that order
    perm = [IN_BLOCKS[i] for i in (2, 0, 3, 1)]
    Y2 = sbm.term_apply_to(layout, psi, left, right, vectors[0], perm).cpu().numpy()
    off = np.concatenate([[0], np.cumsum([LSZ[a] * RSZ[b] for a, b in IN_BLOCKS])])
    back = np.concatenate([Y1[:, off[i]:off[i + 1]] for i in (2, 0, 3, 1)], axis=1)
    assert np.array_equal(Y2.view(np.uint64), back.view(np.uint64))


def test_term_apply_to_refusals(mods, planted):
    """An image pair that exists but is missing from the output list, mixed total shifts, ldy < n_out, a Y that overlaps psi and a null Y
    are refused with Y left alone; an empty output list is fine and writes nothing."""
    import ctypes as C
    import torch
    sbm, _, capi = mods
    psi, left, right, vectors, _ = planted
    layout = (LSZ, RSZ, IN_BLOCKS)
    out = OUT_BLOCKS[+1]
    n_out = _n_out(+1)
    Y = torch.full((3, n_out), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(capi.DmrgxError) as e:
        sbm.term_apply_to(layout, psi, left, right, vectors[+1], out[1:], out=Y)                 # (0, 2) is reached but not listed
    assert e.value.code == ERR_ARG and "KronBlock" in str(e.value)
    with pytest.raises(capi.DmrgxError) as e:
        sbm.term_apply_to(layout, psi, left, right, vectors[+1], OUT_BLOCKS[-1], out=Y)          # the wrong sector altogether
    assert e.value.code == ERR_ARG
    with pytest.raises(capi.DmrgxError) as e:
        sbm.term_apply_to(layout, psi, left, right, vectors[+1][:2] + [vectors[-1][0]], out, out=Y)
    assert e.value.code == ERR_ARG and "shift" in str(e.value)
    with pytest.raises(capi.DmrgxError) as e:
        sbm.term_apply_to(layout, psi, left, right, vectors[+1], out + [out[0]], out=Y)          # a block listed twice
    assert e.value.code == ERR_ARG
    with pytest.raises(capi.DmrgxError) as e:
        sbm.term_apply_to(layout, psi, left, right, vectors[+1], out + [(4, 0)], out=Y)
    assert e.value.code == ERR_OUTOFRANGE
    short = torch.full((3, n_out - 1), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(capi.DmrgxError) as e:
        sbm.term_apply_to(layout, psi, left, right, vectors[+1], out, out=short)
    assert e.value.code == ERR_ARG and "ldy" in str(e.value)
    # Y overlapping psi: the second vector of a buffer whose tail is psi
    buf = torch.zeros(n_out + N_IN, dtype=torch.float64, device="cuda")
    buf[n_out:] = torch.from_numpy(psi).cuda()
    with pytest.raises(capi.DmrgxError) as e:
        sbm.term_apply_to(layout, buf[n_out:], left, right, vectors[+1][:2], out, out=buf[:2 * n_out].view(2, n_out))
    assert e.value.code == ERR_ARG and "overlap" in str(e.value)
    # a null Y
    args, psi_d, keep = sbm._gram_arguments(layout, psi, left, right)
    first, terms = (C.c_int32 * 2)(0, 1), (capi.Term * 1)()
    terms[0].a, terms[0].left_op, terms[0].right_op = 1.0, 1, -1
    oil, oir = (C.c_int32 * 3)(*[b[0] for b in out]), (C.c_int32 * 3)(*[b[1] for b in out])
    assert capi.lib().dmrgx_kron_term_apply_to(*args, 1, first, terms, 3, oil, oir, None, n_out, None) == ERR_ARG
    # an empty output list: OK, nothing written
    assert capi.lib().dmrgx_kron_term_apply_to(*args, 1, first, terms, 0, None, None, C.c_void_p(Y.data_ptr()), n_out, None) == 0
    ret = sbm.term_apply_to(layout, psi, left, right, vectors[+1], [], out=Y)
    assert ret is Y
    assert (Y == 7.0).all() and (short == 7.0).all()


def _both(sbm, psi, left, right, vectors):
    layout = (LSZ, RSZ, IN_BLOCKS)
    return np.concatenate([sbm.term_apply_to(layout, psi, left, right, vectors[s], OUT_BLOCKS[s]).cpu().numpy().ravel() for s in (+1, -1)])


def test_poisoned_workspace_gives_the_same_bits(mods, planted, tmp_path):
    """Both calls in a child process under DMRGX_POOL_POISON=1 (intermediates and materialised operands come from the pool filled with
    NaN): Y is finite and bit-identical to the clean run in this process."""
    from test_gpu_poison import _child
    sbm, _, _ = mods
    psi, left, right, vectors, _ = planted
    Y = _both(sbm, psi, left, right, vectors)
    out = str(tmp_path / "poisoned.npy")
    p = _child([os.path.join("tests", "test_gpu_term_apply_to.py"), out], True, 300)
    assert p.returncode == 0 and "term apply_to child ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    Yp = np.load(out)
    assert np.isfinite(Yp).all() and np.array_equal(Y.view(np.uint64), Yp.view(np.uint64))


if __name__ == "__main__":
    from __graft_entry__ import load_package
    load_package()
    from dmrgx_amd import superblock as sbm_child, workloads as wl_child
    assert os.environ.get("DMRGX_POOL_POISON") == "1"
    psi_c, left_c, right_c, vectors_c = _case(wl_child)
    np.save(sys.argv[1], _both(sbm_child, psi_c, left_c, right_c, vectors_c))
    print("term apply_to child ok")
