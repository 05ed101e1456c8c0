"""The Gram kernel (csrc/gram.hip) through dmrgx_vec_gram, and the operator-image Gram matrix dmrgx_kron_op_gram built on it (-m gpu).

dmrgx_vec_gram: G[i][j] (=|+=) sum_n U[i][n] V[j][n].  Operands are helpers.GgemmOperand views of larger NaN buffers (a read past the
len edge or past the last row poisons the result), G sits in a band of GGEMM_SENTINEL that must come back bit for bit, and the reference
is numpy in np.longdouble.  The bound is the any-order summation bound (Higham, section 3.1), derived and not measured:

    |G - G_ref|_ij <= (len + 8) 2^-53 (|U| |V|^T)_ij      (+ |G0|_ij 2^-53 when accumulating onto G0)

dmrgx_kron_op_gram: planted superblocks against the dense Kronecker products np.kron(A, 1) psi and np.kron(1, B) psi.

Run as a script (`test_gpu_gram.py OUT.npy`) this file is the child of the poisoned-workspace test: it runs one ladder case and saves G."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                      # (the child process: pytest's conftest is not there to set the path)
    sys.path.insert(0, ROOT)

from helpers import GGEMM_SENTINEL, GgemmOperand, ggemm_values  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_OUTOFRANGE = 62, 63
U53 = 2.0 ** -53

SHAPES = [(1, 1), (3, 17), (16, 16), (17, 33), (64, 64), (65, 70), (161, 161)]
# both sides of the 16-long chunk and of 64, a slice edge inside a chunk (1000 = 62.5 chunks), several slices (4097), and the longest:
# a slice is at least 1024 long, so 70 001 is cut in 69 of them (report.slices >= 2 is asserted; no need to raise it)
LENS = [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 1000, 4097, 70001]
LONGEST = LENS[-1]


class GramCase:
    """U (nu x len) and V (nv x len) as sub-views of NaN buffers, G0 (when accumulating), the long double reference and the bound.
    odd: the parity of U's first element inside the one device buffer (1: U starts an odd number of doubles off 16-byte alignment)."""

    def __init__(self, nu, nv, n, accumulate=False, same=False, odd=None, seed=0):
        rng = np.random.default_rng([nu, nv, n, int(accumulate), int(same), seed])
        self.nu, self.nv, self.n, self.accumulate, self.same, self.odd = nu, nv, n, accumulate, same, odd
        self.U = GgemmOperand(rng, ggemm_values(rng, (nu, n)), np.nan)
        self.V = self.U if same else GgemmOperand(rng, ggemm_values(rng, (nv, n)), np.nan)
        self.G0 = ggemm_values(rng, (nu, nv)) if accumulate else None
        if accumulate and same:
            self.G0 = np.triu(self.G0) + np.triu(self.G0, 1).T          # symmetric: G0 + a symmetric Gram stays symmetric
        self.pad = tuple(int(v) for v in rng.integers(1, 6, size=4))
        Ul, Vl = self.U.view.astype(np.longdouble), self.V.view.astype(np.longdouble)
        self.ref = np.einsum("ik,jk->ij", Ul, Vl)              # (long double has no BLAS: this form is the quickest numpy offers)
        self.bound = (n + 8) * U53 * (np.abs(self.U.view) @ np.abs(self.V.view).T)
        if accumulate:
            self.ref = self.ref + self.G0.astype(np.longdouble)
            self.bound = self.bound + np.abs(self.G0) * U53

    def check(self, G, what=""):
        err = np.abs(G.astype(np.longdouble) - self.ref).astype(np.float64)
        bad = ~(err <= self.bound)
        assert not bad.any(), "%s nu=%d nv=%d len=%d: %d elements outside the bound, first %s: got %r want %r bound %.3e" % (
            what, self.nu, self.nv, self.n, int(bad.sum()), tuple(np.argwhere(bad)[0]), float(G[tuple(np.argwhere(bad)[0])]),
            float(self.ref[tuple(np.argwhere(bad)[0])]), float(self.bound[tuple(np.argwhere(bad)[0])]))


_cases = {}


def case(*key, **kw):
    """Cases are built once (the long double reference of the longest ones takes seconds) and never changed."""
    k = key + tuple(sorted(kw.items()))
    if k not in _cases:
        _cases[k] = GramCase(*key, **kw)
    return _cases[k]


def run_gram(pkg, c, runs=1):
    """dmrgx_vec_gram on the case, `runs` times from the same initial memory -> ([G of every run], report).  U, V and G live in ONE device
    buffer; everything in it except the nu x nv interior of G must come back bit for bit."""
    import ctypes as C
    import torch
    capi = pkg._capi
    L = capi.lib()
    top, bottom, left, right = c.pad
    gbuf = np.full((c.nu + top + bottom, c.nv + left + right), GGEMM_SENTINEL)
    gbuf[top:top + c.nu, left:left + c.nv] = c.G0 if c.accumulate else np.nan
    parts, at, size = [], {}, 0
    for name, buf, first in (("U", c.U.buf, c.U.first), ("V", c.V.buf, c.V.first), ("G", gbuf, 0)):
        if name == "V" and c.same:
            at["V"] = at["U"]
            continue
        if name == "U" and c.odd is not None and (size + first) % 2 != c.odd:
            parts.append(np.full(1, np.nan)); size += 1
        at[name] = size
        parts.append(buf.ravel()); size += buf.size
    host = np.concatenate(parts)
    dev = torch.from_numpy(host).cuda()
    base = dev.data_ptr()
    assert base % 16 == 0
    if c.odd is not None:
        assert ((at["U"] + c.U.first) % 2) == c.odd
    ldg = gbuf.shape[1]
    pu, pv, pg = base + 8 * (at["U"] + c.U.first), base + 8 * (at["V"] + c.V.first), base + 8 * (at["G"] + top * ldg + left)
    outs, rep = [], None
    for r in range(runs):
        if r:
            dev.copy_(torch.from_numpy(host))
        rep = capi.GramReport()
        rc = L.dmrgx_vec_gram(c.nu, c.nv, c.n, C.c_void_p(pu), c.U.ld, C.c_void_p(pv), c.V.ld, C.c_void_p(pg), ldg, int(c.accumulate), C.byref(rep), None)
        assert rc == 0, L.dmrgx_last_error()
        torch.cuda.synchronize()
        got = dev.cpu().numpy()
        G = got[at["G"]:at["G"] + gbuf.size].reshape(gbuf.shape)[top:top + c.nu, left:left + c.nv].copy()
        # nothing but the interior of G changed: operands, their NaN borders, the sentinel band
        want = host.copy()
        want[at["G"]:at["G"] + gbuf.size].reshape(gbuf.shape)[top:top + c.nu, left:left + c.nv] = G
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), "memory outside G's interior changed"
        outs.append(G)
    return outs, rep


# ---- dmrgx_vec_gram -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu,nv", SHAPES)
def test_shape_ladder(pkg, nu, nv):
    """Every (nu, nv) class at every len of the ladder; the longest len is split over len."""
    assert np.finfo(np.longdouble).eps < 1e-18
    for n in LENS:
        c = case(nu, nv, n)
        (G,), rep = run_gram(pkg, c)
        c.check(G, "ladder")
        assert rep.tiles == -(-nu // 64) * -(-nv // 64)
        assert rep.slices == 0 if n == 0 else rep.slices >= 1
        assert rep.slab_doubles == rep.tiles * rep.slices * 64 * 64
        if n == 0:
            assert not G.any()                                            # len = 0 writes zeros
        if n == LONGEST:
            assert rep.slices >= 2, rep.slices


@pytest.mark.parametrize("nu,nv,n", [(3, 17, 15), (17, 33, 17), (17, 33, 1000), (65, 70, 63), (65, 70, 65), (161, 161, 4097), (1, 1, 0), (65, 70, 0)])
def test_accumulate(pkg, nu, nv, n):
    """accumulate = 1 onto random G0 (bound + |G0| 2^-53); len = 0 leaves G0 as it is."""
    c = case(nu, nv, n, accumulate=True)
    (G,), _ = run_gram(pkg, c)
    c.check(G, "accumulate")
    if n == 0:
        assert np.array_equal(G, c.G0)


@pytest.mark.parametrize("odd", [0, 1])
@pytest.mark.parametrize("nu,nv,n", [(3, 17, 17), (65, 70, 1000), (17, 33, 4097)])
def test_leading_dimensions_and_odd_offsets(pkg, nu, nv, n, odd):
    """ld > len for both families (every GgemmOperand has a right border), U starting an even and an odd number of doubles off 16-byte
    alignment: the kernel may assume 8-byte alignment only."""
    c = case(nu, nv, n, odd=odd)
    assert c.U.ld > n and c.V.ld > n
    (G,), _ = run_gram(pkg, c)
    c.check(G, "odd=%d" % odd)


@pytest.mark.parametrize("nu,n,accumulate", [(16, 65, False), (65, 1000, False), (161, 4097, False), (161, 1000, True)])
def test_same_family_is_bitwise_symmetric(pkg, nu, n, accumulate):
    """U and V the same family (pointer, ld, count): one triangle of tiles is computed, G comes back bitwise symmetric (accumulating:
    onto a symmetric G0)."""
    c = case(nu, nu, n, accumulate=accumulate, same=True)
    (G,), rep = run_gram(pkg, c)
    c.check(G, "same family")
    T = -(-nu // 64)
    assert rep.tiles == T * (T + 1) // 2
    assert np.array_equal(G, G.T)


@pytest.mark.parametrize("nu,nv,n", [(17, 33, 1000), (161, 161, 4097)])
def test_two_calls_are_bit_identical(pkg, nu, nv, n):
    c = case(nu, nv, n)
    (G1, G2), rep = run_gram(pkg, c, runs=2)
    assert rep.slices >= 1 and np.array_equal(G1.view(np.uint64), G2.view(np.uint64))


def test_bad_arguments_are_refused(pkg):
    import ctypes as C
    import torch
    L = pkg._capi.lib()
    d = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = C.c_void_p(d.data_ptr())
    for args in ((0, 1, 4, p, 4, p, 4, p, 1), (1, 1, -1, p, 4, p, 4, p, 1), (2, 2, 4, p, 3, p, 4, p, 2), (2, 2, 4, p, 4, p, 4, p, 1),
                 (2, 2, 4, None, 4, p, 4, p, 2), (2, 2, 4, p, 4, p, 4, None, 2)):
        assert L.dmrgx_vec_gram(*args, 0, None, None) == ERR_ARG, args


POISON_CASE = (65, 70, 4097)


def test_poisoned_slab_gives_the_same_bits(pkg, tmp_path):
    """One ladder case in a child process under DMRGX_POOL_POISON=1 (the slab of partial tiles comes from the pool filled with NaN): the
    result is finite and bit-identical to the clean run in this process."""
    from test_gpu_poison import _child
    c = case(*POISON_CASE)
    (G,), rep = run_gram(pkg, c)
    assert rep.slices >= 2
    out = str(tmp_path / "poisoned.npy")
    p = _child([os.path.join("tests", "test_gpu_gram.py"), out], True, 300)
    assert p.returncode == 0 and "gram child ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    Gp = np.load(out)
    assert np.isfinite(Gp).all() and np.array_equal(G.view(np.uint64), Gp.view(np.uint64))


# ---- dmrgx_kron_op_gram against the dense Kronecker product ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mods(pkg):
    from dmrgx_amd import superblock, workloads, _capi
    _capi.require_device()
    return superblock, workloads, _capi


LSZ, RSZ = [3, 4, 2], [5, 1, 6]
BLOCKS = [(0, 2), (1, 1), (2, 0)]


def _embed(psi, lsz, rsz, blocks):
    """psi on the KronBlocks -> the n_L x n_R matrix of the full product space (row-major: the vector of np.kron)."""
    loff, roff = np.concatenate([[0], np.cumsum(lsz)]), np.concatenate([[0], np.cumsum(rsz)])
    Psi, o = np.zeros((loff[-1], roff[-1])), 0
    for il, ir in blocks:
        n = lsz[il] * rsz[ir]
        Psi[loff[il]:loff[il + 1], roff[ir]:roff[ir + 1]] = psi[o:o + n].reshape(lsz[il], rsz[ir])
        o += n
    return Psi


def _dense(op, sizes):
    from test_gpu_kron import _dense_operator
    op, transposed = op if isinstance(op, tuple) else (op, False)
    M = _dense_operator(op, sizes)
    return M.T if transposed else M


def _reference(psi, lsz, rsz, blocks, left_ops, right_ops, kron=True):
    """All inner products of np.kron(A, 1) psi and np.kron(1, B) psi.  kron=False (the larger layout, whose Kronecker matrices would take
    gigabytes): the same vectors as A Psi and Psi B^T on the n_L x n_R matrix Psi."""
    Psi = _embed(psi, lsz, rsz, blocks)
    nl, nr = Psi.shape
    if kron:
        vecs = [np.kron(_dense(a, lsz), np.eye(nr)) @ Psi.ravel() for a in left_ops] + [np.kron(np.eye(nl), _dense(b, rsz)) @ Psi.ravel() for b in right_ops]
    else:
        vecs = [(_dense(a, lsz) @ Psi).ravel() for a in left_ops] + [(Psi @ _dense(b, rsz).T).ravel() for b in right_ops]
    V = np.array(vecs)
    return V @ V.T


def _check(G, want):
    assert np.isfinite(G).all()
    assert np.abs(G - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), np.abs(G - want).max()


def _planted(wl, rng):
    """Operators on LSZ / RSZ: shift 0 with partial and overlapping dense cells, identities, identity cells with offsets; shift +1 given
    directly and as transposed shift -1 cells."""
    D, I = wl.CELL_DENSE, wl.CELL_IDENT

    def dense(q, r0, c0, nr, nc):
        return wl.OpCell(q, r0, c0, nr, nc, D, 0.0, rng.standard_normal((nr, nc)))

    def ident(sizes):
        return wl.SectorOperator(0, [wl.OpCell(q, 0, 0, n, n, I, 1.0) for q, n in enumerate(sizes)])

    ops = {
        # left, shift 0: cells that leave rows of a sector unreached, two cells overlapping in rows 1-2 of sector 1, a full cell
        "L0_partial": wl.SectorOperator(0, [dense(0, 1, 0, 2, 3), dense(1, 0, 0, 3, 2), dense(1, 1, 1, 3, 3), dense(2, 0, 0, 2, 2)]),
        "L0_ident": ident(LSZ),
        # identity cells with offsets (rows 1-2 <- columns 0-1 of sector 0; rows 0-2 <- columns 1-3 of sector 1) beside a dense cell
        "L0_ident_off": wl.SectorOperator(0, [wl.OpCell(0, 1, 0, 2, 2, I, 0.7), wl.OpCell(1, 0, 1, 3, 3, I, -1.3), dense(1, 2, 0, 2, 2)]),
        "R0_partial": wl.SectorOperator(0, [dense(0, 0, 1, 3, 4), dense(0, 2, 0, 3, 2), dense(2, 1, 0, 4, 6)]),
        "R0_ident": ident(RSZ),
        "R0_ident_off": wl.SectorOperator(0, [wl.OpCell(0, 2, 0, 3, 3, I, 0.4), wl.OpCell(2, 0, 3, 3, 3, I, 2.5), dense(1, 0, 0, 1, 1)]),
        # shift +1: row sector q -> column sector q + 1 (no cell in the last sector: its partner does not exist)
        "Lp": wl.SectorOperator(+1, [dense(0, 0, 0, 3, 4), dense(1, 1, 0, 3, 2)]),
        "Lp_ident": wl.SectorOperator(+1, [wl.OpCell(0, 0, 1, 3, 3, I, 0.9), wl.OpCell(1, 2, 0, 2, 2, I, -0.6)]),
        "Rp": wl.SectorOperator(+1, [dense(0, 0, 0, 5, 1), dense(1, 0, 2, 1, 4)]),
        # stored with shift -1 (row sector q -> q - 1), used transposed: shift +1
        "Lm": wl.SectorOperator(-1, [dense(1, 0, 0, 4, 3), dense(2, 0, 1, 2, 3)]),
        "Rm": wl.SectorOperator(-1, [dense(1, 0, 1, 1, 4), dense(2, 1, 0, 4, 1), wl.OpCell(2, 0, 0, 1, 1, I, 1.7)]),
    }
    return ops


@pytest.mark.parametrize("which", ["shift0_mixed", "shift0_left_only", "shift0_right_only", "plus_mixed", "plus_left_only", "plus_right_only"])
def test_op_gram_planted_superblock(mods, which):
    """Three left and three right sectors of unequal sizes, psi random on the target KronBlocks.  With shift +1 KronBlock (0, 2) has no
    left partner (left sector -1) and KronBlock (2, 0) no right partner: they contribute nothing to the images of that side."""
    sbm, wl, _ = mods
    rng = np.random.default_rng(41)
    o = _planted(wl, rng)
    psi = rng.standard_normal(sum(LSZ[a] * RSZ[b] for a, b in BLOCKS))
    L0, R0 = [o["L0_partial"], o["L0_ident"], o["L0_ident_off"]], [o["R0_partial"], o["R0_ident"], o["R0_ident_off"]]
    Lp, Rp = [o["Lp"], (o["Lm"], True), o["Lp_ident"]], [o["Rp"], (o["Rm"], True)]
    left, right = {"shift0_mixed": (L0, R0), "shift0_left_only": (L0, []), "shift0_right_only": ([], R0),
                   "plus_mixed": (Lp, Rp), "plus_left_only": (Lp, []), "plus_right_only": ([], Rp)}[which]
    G, rep = sbm.op_gram((LSZ, RSZ, BLOCKS), psi, left, right)
    want = _reference(psi, LSZ, RSZ, BLOCKS, left, right)
    assert np.abs(want).max() > 0.1
    G = G.cpu().numpy()
    _check(G, want)
    assert np.array_equal(G, G.T) and rep.slices == 1
    if which == "shift0_mixed":                                   # the identity operators give <psi|psi> and <psi|O psi>
        assert abs(G[1, 1] - psi @ psi) <= 1e-13 * (psi @ psi) and abs(G[1, 4] - psi @ psi) <= 1e-13 * (psi @ psi)


def test_op_gram_workspace_slices_and_refusals(mods):
    """A larger layout (sectors about 90 x 60 and 40 x 70) with a workspace that holds one image block at a time: three slices, each
    accumulated into G; one byte less than the largest block needs is refused, and so are mixed shifts and a cell outside its block."""
    sbm, wl, capi = mods
    rng = np.random.default_rng(43)
    lsz, rsz, blocks = [90, 40, 30], [60, 70, 50], [(0, 2), (1, 1), (2, 0)]
    D = wl.CELL_DENSE

    def full(sizes, scale):
        return wl.SectorOperator(0, [wl.OpCell(q, 0, 0, n, n, D, 0.0, scale * rng.standard_normal((n, n))) for q, n in enumerate(sizes)])

    def halves(sizes):                                            # two dense cells per sector, as an enlarged block's operators have
        cells = []
        for q, n in enumerate(sizes):
            h = n // 2
            cells += [wl.OpCell(q, 0, 0, h, h, D, 0.0, rng.standard_normal((h, h))), wl.OpCell(q, h, h, n - h, n - h, D, 0.0, rng.standard_normal((n - h, n - h)))]
        return wl.SectorOperator(0, cells)

    ident = wl.SectorOperator(0, [wl.OpCell(q, 0, 0, n, n, wl.CELL_IDENT, 1.0) for q, n in enumerate(lsz)])
    left, right = [ident, full(lsz, 0.1), halves(lsz)], [full(rsz, 0.1), halves(rsz), halves(rsz)]
    psi = rng.standard_normal(sum(lsz[a] * rsz[b] for a, b in blocks))
    psi /= np.linalg.norm(psi)
    want = _reference(psi, lsz, rsz, blocks, left, right, kron=False)
    largest = max(lsz[a] * rsz[b] for a, b in blocks) * 6 * 8
    G1, rep1 = sbm.op_gram((lsz, rsz, blocks), psi, left, right)
    G3, rep3 = sbm.op_gram((lsz, rsz, blocks), psi, left, right, workspace_bytes=largest)
    assert rep1.slices == 1 and rep3.slices >= 3, (rep1.slices, rep3.slices)
    for G in (G1, G3):
        _check(G.cpu().numpy(), want)
    with pytest.raises(capi.DmrgxError) as e:
        sbm.op_gram((lsz, rsz, blocks), psi, left, right, workspace_bytes=largest - 8)
    assert e.value.code == ERR_ARG and "workspace" in str(e.value)
    plus = wl.SectorOperator(+1, [wl.OpCell(0, 0, 0, 90, 40, D, 0.0, rng.standard_normal((90, 40)))])
    with pytest.raises(capi.DmrgxError) as e:
        sbm.op_gram((lsz, rsz, blocks), psi, [left[1], plus], right)
    assert e.value.code == ERR_ARG and "shift" in str(e.value)
    outside = wl.SectorOperator(0, [wl.OpCell(1, 0, 0, 41, 40, D, 0.0, rng.standard_normal((41, 40)))])
    with pytest.raises(capi.DmrgxError) as e:
        sbm.op_gram((lsz, rsz, blocks), psi, [outside], [])
    assert e.value.code == ERR_OUTOFRANGE


if __name__ == "__main__":
    from __graft_entry__ import load_package
    (G_child,), _ = run_gram(load_package(), GramCase(*POISON_CASE))
    np.save(sys.argv[1], G_child)
    print("gram child ok")
