"""General MatMult descriptors: a plain description of everything include/dmrgx.h lets a dmrgx_kron_desc say, a builder that fills the
ctypes descriptor directly (no superblock.KronPlan in between), a reference from the definition at a chosen precision, and an
element-wise, derived bound (tests/test_kron_general_host.py, tests/test_gpu_kron_general.py).

superblock.KronPlan can only express the Heisenberg-shaped family: shifts -1, 0, +1, `transposed` as "Sm is Sp read transposed",
ld == nc, one operator per (op, site), one term per operator pair.  A GDesc holds any shift, any rectangles (an operator is the sum of
its cells), `transposed` on any operator, ld = nc + ld_pad, data pointers at any element offset, any term list.

Conventions (include/dmrgx.h): a cell of a transposed operator is stored in the orientation of the stored operator, whose shift is
-shift; the operator as used is the transpose of the sum of its stored cells."""
import copy
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from helpers import ggemm_values

CELL_DENSE, CELL_IDENT = 1, 2
SIZES = (1, 2, 15, 16, 17, 33, 63, 64, 65, 129, 130)      # tile edge 64, k-step 16, copy tile 32
SENTINEL = -6.02214076e+123                                # the band round y; must come back bit for bit
EXP_WEAKEST, EXP_BESIDE_WEAKEST = -140, -100               # x of the weakest KronBlock and of the blocks its terms read (powers of two)


@dataclass
class GCell:
    row_sector: int
    r0: int
    c0: int
    nr: int
    nc: int
    kind: int = CELL_DENSE
    scale: float = 0.0
    array: np.ndarray = None      # nr x nc float64, the stored orientation (DENSE only)
    ld_pad: int = 0               # ld = nc + ld_pad
    lead: int = 0                 # element offset of the cell's first element inside its device buffer


@dataclass
class GOp:
    shift: int                    # as used
    transposed: bool = False
    cells: list = field(default_factory=list)

    @property
    def stored_shift(self):
        return -self.shift if self.transposed else self.shift


@dataclass
class GDesc:
    name: str
    left_sizes: list
    right_sizes: list
    blocks: list                  # [(IL, IR)]
    left_ops: list
    right_ops: list
    h_left: GOp = None            # None: NULL in the descriptor
    h_right: GOp = None
    terms: list = field(default_factory=list)      # [(a, left index, right index)]
    world_size: int = 1

    @property
    def n_states(self):
        return sum(self.left_sizes[il] * self.right_sizes[ir] for il, ir in self.blocks)

    def offsets(self):
        off = [0]
        for il, ir in self.blocks:
            off.append(off[-1] + self.left_sizes[il] * self.right_sizes[ir])
        return off


# ---- reference from the definition ---------------------------------------------------------------------------------------------------
def op_blocks(op, sizes, dtype=np.float64, magnitude=False):
    """{row sector as used: dense block} of an operator: the sum of its cells (workloads.operator_to_dense_blocks), `transposed` applied
    afterwards.  magnitude: the sum of the cells' magnitudes instead."""
    if op is None:
        return {}
    s, out = op.stored_shift, {}
    for c in op.cells:
        b = out.setdefault(c.row_sector, np.zeros((sizes[c.row_sector], sizes[c.row_sector + s]), dtype=dtype))
        v = np.asarray(c.array, dtype=np.float64).astype(dtype) if c.kind == CELL_DENSE else dtype(c.scale) * np.eye(c.nr, dtype=dtype)
        b[c.r0:c.r0 + c.nr, c.c0:c.c0 + c.nc] += np.abs(v) if magnitude else v
    if op.transposed:
        out = {q + s: b.T for q, b in out.items()}
    return out


def reference(desc, x, dtype=np.longdouble, only=None):
    """(R, S_abs, n) over the n_states elements of y = H x, from the definition:

        Y_k = H_L[IL] X_k + X_k H_R[IR]^T + sum_t a_t A_t[IL -> IL'] X_k' B_t[IR -> IR']^T,   k' = (IL + shift_A, IR + shift_B),

    a term skipped where k' is no KronBlock.  R at `dtype`; S_abs (float64: a sum of non-negative numbers, good to n eps) the same sum over
    |a|, |A|, |X|, |B|; n the number of roundings an element of block k can see: per term that reaches k the contraction lengths of both
    stages, one per cell of either operator (the merge) and three for the products by a and the hand-over between the stages, n_L and n_R
    and the cells of H_L and H_R, and two.  Over-counted on purpose: it only has to lie above the plan's count.
    only: {(t, k)} -- the terms (t = 'L', 'R' for H_L, H_R) to take, everything else is left out (the parts of a sum, for choosing faults)."""
    ls, rs, off = desc.left_sizes, desc.right_sizes, desc.offsets()
    kmap = {b: k for k, b in enumerate(desc.blocks)}
    x = np.asarray(x, dtype=np.float64)
    X = [x[off[k]:off[k + 1]].reshape(ls[il], rs[ir]).astype(dtype) for k, (il, ir) in enumerate(desc.blocks)]
    XA = [np.abs(x[off[k]:off[k + 1]].reshape(ls[il], rs[ir])) for k, (il, ir) in enumerate(desc.blocks)]
    Y = [np.zeros(v.shape, dtype=dtype) for v in X]
    S = [np.zeros(v.shape) for v in X]
    n = [2] * len(X)
    cache = {}

    def blocks(key, op, sizes):
        if key not in cache:
            cache[key] = (op_blocks(op, sizes, dtype), op_blocks(op, sizes, np.float64, magnitude=True))
        return cache[key]

    hl, hla = blocks("L", desc.h_left, ls)
    hr, hra = blocks("R", desc.h_right, rs)
    for k, (il, ir) in enumerate(desc.blocks):
        if il in hl and (only is None or ("L", k) in only):
            Y[k] += hl[il] @ X[k]
            S[k] += hla[il] @ XA[k]
            n[k] += ls[il] + len(desc.h_left.cells)
        if ir in hr and (only is None or ("R", k) in only):
            Y[k] += X[k] @ hr[ir].T
            S[k] += XA[k] @ hra[ir].T
            n[k] += rs[ir] + len(desc.h_right.cells)
    for t, (a, li, ri) in enumerate(desc.terms):
        A, Aa = blocks(("l", li), desc.left_ops[li], ls)
        B, Ba = blocks(("r", ri), desc.right_ops[ri], rs)
        sa, sb = desc.left_ops[li].shift, desc.right_ops[ri].shift
        for k, (il, ir) in enumerate(desc.blocks):
            ks = kmap.get((il + sa, ir + sb))
            if ks is None or il not in A or ir not in B or (only is not None and (t, k) not in only):
                continue
            Y[k] += dtype(a) * (A[il] @ (X[ks] @ B[ir].T))
            S[k] += abs(a) * (Aa[il] @ (XA[ks] @ Ba[ir].T))
            n[k] += ls[il + sa] + rs[ir + sb] + len(desc.left_ops[li].cells) + len(desc.right_ops[ri].cells) + 3
    R = np.concatenate([v.ravel() for v in Y])
    Sabs = np.concatenate([v.ravel() for v in S])
    nn = np.concatenate([np.full(v.size, float(c)) for v, c in zip(Y, n)])
    return R, Sabs, nn


def reference_diag(desc, dtype=np.longdouble):
    """(D, D_abs, n) of the diagonal <e| H |e>: diag(H_L)[l] + diag(H_R)[r] + sum over the terms of shift 0 of a diag(A)[l] diag(B)[r]."""
    ls, rs = desc.left_sizes, desc.right_sizes
    hl, hla = op_blocks(desc.h_left, ls, dtype), op_blocks(desc.h_left, ls, np.float64, True)
    hr, hra = op_blocks(desc.h_right, rs, dtype), op_blocks(desc.h_right, rs, np.float64, True)
    D, Da, nn = [], [], []
    for (il, ir) in desc.blocks:
        d, da, n = np.zeros((ls[il], rs[ir]), dtype=dtype), np.zeros((ls[il], rs[ir])), 2
        if il in hl:
            d, da, n = d + np.diag(hl[il])[:, None], da + np.diag(hla[il])[:, None], n + len(desc.h_left.cells)
        if ir in hr:
            d, da, n = d + np.diag(hr[ir])[None, :], da + np.diag(hra[ir])[None, :], n + len(desc.h_right.cells)
        for (a, li, ri) in desc.terms:
            A, B = desc.left_ops[li], desc.right_ops[ri]
            if A.shift != 0 or B.shift != 0:
                continue
            Ab, Bb = op_blocks(A, ls, dtype).get(il), op_blocks(B, rs, dtype).get(ir)
            if Ab is None or Bb is None:
                continue
            Aa, Ba = op_blocks(A, ls, np.float64, True)[il], op_blocks(B, rs, np.float64, True)[ir]
            d = d + dtype(a) * np.outer(np.diag(Ab), np.diag(Bb))
            da = da + abs(a) * np.outer(np.diag(Aa), np.diag(Ba))
            n += len(A.cells) + len(B.cells) + 3
        D.append(d.ravel()); Da.append(da.ravel()); nn.append(np.full(d.size, float(n)))
    return np.concatenate(D), np.concatenate(Da), np.concatenate(nn)


# ---- bound and checkers --------------------------------------------------------------------------------------------------------------
def kron_bound(S_abs, n):
    """|got - R| <= 2 (n + 2) eps S_abs, element by element: the statement of helpers.ggemm_bound.  An element of y is a nested sum of
    leaves a A[l, l'] X[l', r'] B[r, r']: the merge adds a_t A_t (or a_t B_t) cell by cell into the group's operator, stage 1 contracts X
    with it over r' (or scales a copy), stage 2 contracts over l' and adds the groups, H_L and H_R and the split-K slabs.  Whatever the
    order and with or without fused multiply-adds, every leaf reaches the result times a product of factors (1 + delta_i), |delta_i| <= u
    = eps / 2, one per rounding on its path: the products by a and in both stages, and the additions it sits under at the three levels.
    The path of a leaf is no longer than n roundings (reference() counts every contraction length and every merged contribution of every
    term that reaches the block), and a product of n such factors stays within gamma_n = n u / (1 - n u) of one (Higham, Accuracy and
    Stability of Numerical Algorithms, lemma 3.1), so |got - exact| <= gamma_n S_abs.  (n + 2) eps lies above gamma_n for every
    n < 2^50; it is taken twice, once for the kernel and once for a float64 reference (the longdouble one needs 2^-11 of it).  Derived, not
    measured."""
    return 2.0 * (np.asarray(n, dtype=np.float64) + 2.0) * np.finfo(np.float64).eps * np.asarray(S_abs, dtype=np.float64)


def kron_violations(got, R, S_abs, n, scale=1.0):
    """Boolean array over every element: outside the bound (a NaN is outside).  The difference is taken at the precision of R."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == R.shape == S_abs.shape, (got.shape, R.shape, S_abs.shape)
    return ~(np.abs(got.astype(R.dtype) - R).astype(np.float64) <= scale * kron_bound(S_abs, n))


def kron_check(got, R, S_abs, n, what="", scale=1.0):
    """Asserts that every element of `got` is within the bound; prints and returns the worst |got - R| / bound (0 for 0 / 0)."""
    bad = kron_violations(got, R, S_abs, n, scale)
    bound = scale * kron_bound(S_abs, n)
    if bad.any():
        i = int(np.argwhere(bad)[0][0])
        raise AssertionError("%s: %d of %d elements outside the bound, first at %d: got %r, want %r, bound %.3e (n = %d)"
                             % (what, int(bad.sum()), bad.size, i, float(np.asarray(got)[i]), float(R[i]), float(bound[i]), int(np.asarray(n)[i])))
    err = np.abs(np.asarray(got, dtype=np.float64).astype(R.dtype) - R).astype(np.float64)
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0))) if err.size else 0.0
    print("%s: worst |got - R| / bound = %.3f over %d elements" % (what, worst, err.size))
    return worst


# ---- graded inputs -------------------------------------------------------------------------------------------------------------------
def dense_cell(rng, q, r0, c0, nr, nc, ld_pad=0, lead=0, exp=None):
    """Magnitudes in [0.5, 1.5] with random signs (ggemm_values) times a power of two in 2^-8 .. 2^8."""
    e = int(rng.integers(-8, 9)) if exp is None else exp
    return GCell(q, r0, c0, nr, nc, CELL_DENSE, 0.0, np.ascontiguousarray(ggemm_values(rng, (nr, nc)) * 2.0 ** e), ld_pad, lead)


def ident_cell(rng, q, r0, c0, n):
    return GCell(q, r0, c0, n, n, CELL_IDENT, float(ggemm_values(rng, ())) * 2.0 ** int(rng.integers(-3, 4)))


def full_op(rng, sizes, shift, transposed=False, pads=(0,), leads=(0,)):
    """One dense cell over every sector block of the operator."""
    op = GOp(shift, transposed)
    s = op.stored_shift
    for q in range(len(sizes)):
        if 0 <= q + s < len(sizes):
            op.cells.append(dense_cell(rng, q, 0, 0, sizes[q], sizes[q + s], int(rng.choice(pads)), int(rng.choice(leads))))
    return op


def block_links(desc):
    """{k: set of k'} -- the KronBlocks a term of non-zero coefficient makes block k read, and the other way round."""
    kmap = {b: k for k, b in enumerate(desc.blocks)}
    ls, rs = desc.left_sizes, desc.right_sizes
    links = {k: set() for k in range(len(desc.blocks))}
    for (a, li, ri) in desc.terms:
        if a == 0.0:
            continue
        A, B = op_blocks(desc.left_ops[li], ls, magnitude=True), op_blocks(desc.right_ops[ri], rs, magnitude=True)
        for k, (il, ir) in enumerate(desc.blocks):
            ks = kmap.get((il + desc.left_ops[li].shift, ir + desc.right_ops[ri].shift))
            if ks is not None and ks != k and il in A and ir in B:
                links[k].add(ks); links[ks].add(k)
    return links


def weakest_block(desc):
    return len(desc.blocks) - 1


def graded_exponents(desc):
    """The power of two of x per KronBlock.  The last block is the weakest, about 2^-140, the blocks a term links it to 2^-100, every other block
    between 2^-40 and 1 with both ends taken: graded over many decades between sectors, as a wave function in a sweep is; with one block
    whose whole sum of magnitudes lies below 1e-13 max |y| (cells reach 2^8 per side), and in which its own x comes in at 2^-40 of what
    its neighbours send -- about the bound, as the x of the block at 2^-40 does in the sums of the block at 1."""
    w, links = weakest_block(desc), block_links(desc)
    far = [k for k in range(len(desc.blocks)) if k != w and k not in links[w]]
    assert far, "%s: every KronBlock is linked to the weakest one" % desc.name
    exps = {w: EXP_WEAKEST}
    exps.update({k: EXP_BESIDE_WEAKEST for k in links[w]})
    exps.update({k: -int(round(40.0 * i / max(len(far) - 1, 1))) for i, k in enumerate(far)})
    if links[w]:
        # ... exactly: the power of two at which the weakest block's own x makes up 2^-33 of the sums of magnitudes of its elements (their
        # median), from the reference's sums alone; the cells' own powers of two move that share by up to 2^32 either way
        off = desc.offsets()
        seg = slice(off[w], off[w + 1])
        own, fed = np.zeros(desc.n_states), np.ones(desc.n_states)
        own[seg], fed[seg] = 2.0 ** EXP_BESIDE_WEAKEST, 0.0
        for k, e in exps.items():
            fed[off[k]:off[k + 1]] *= 2.0 ** e
        S_own, S_fed = reference(desc, own, np.float64)[1][seg], reference(desc, fed, np.float64)[1][seg]
        both = (S_own > 0) & (S_fed > 0)
        if both.any():
            exps[w] = EXP_BESIDE_WEAKEST - 33 - int(round(float(np.median(np.log2(S_own[both] / S_fed[both])))))
    return [exps[k] for k in range(len(desc.blocks))]


def graded_x(desc, seed=0):
    """x with block k scaled by 2^graded_exponents[k]; magnitudes before scaling in [0.5, 1.5], random signs.  Read-only."""
    rng = np.random.default_rng(1000 + seed)
    off, exps = desc.offsets(), graded_exponents(desc)
    x = ggemm_values(rng, (desc.n_states,))
    for k, e in enumerate(exps):
        x[off[k]:off[k + 1]] *= 2.0 ** e
    x.setflags(write=False)
    return x


# ---- named cases ---------------------------------------------------------------------------------------------------------------------
def _antidiagonal(nsec, leave_out=()):
    return [(i, nsec - 1 - i) for i in range(nsec) if i not in leave_out]


def case_shifts():
    rng = np.random.default_rng(101)
    ls, rs = [3, 65, 17, 64, 1], [66, 2, 33, 1, 70]
    d = GDesc("shifts", ls, rs, _antidiagonal(5, leave_out=(2,)), [], [])
    for s in (-2, -1, 0, 1, 2):
        d.left_ops.append(full_op(rng, ls, s, transposed=(s == -2)))
        d.right_ops.append(full_op(rng, rs, -s, transposed=(s == 1)))
        d.terms.append((float(ggemm_values(rng, ())), len(d.left_ops) - 1, len(d.right_ops) - 1))
    d.h_left, d.h_right = full_op(rng, ls, 0), full_op(rng, rs, 0)
    return d


def case_overlap():
    rng = np.random.default_rng(102)
    ls, rs = [65, 130, 64], [33, 17, 16]
    d = GDesc("overlap", ls, rs, _antidiagonal(3), [], [])
    # operator 0, shift 0: the overlapping pair in the 65 x 65 block, an identity cell with r0 != c0 on top of the first, and a
    # 20 x 20 rectangle that operator 1 holds as an identity cell
    a0 = GOp(0, False, [dense_cell(rng, 0, 0, 0, 40, 50), dense_cell(rng, 0, 30, 20, 35, 45), ident_cell(rng, 0, 3, 11, 25),
                        dense_cell(rng, 0, 10, 10, 20, 20), dense_cell(rng, 1, 0, 0, 130, 130), dense_cell(rng, 2, 5, 0, 17, 64)])
    # operator 1, shift 0, transposed: its stored 50 x 40 cell is the rectangle [0:40, 0:50) as used -- one destination, two rounds
    a1 = GOp(0, True, [dense_cell(rng, 0, 0, 0, 50, 40), ident_cell(rng, 0, 10, 10, 20), dense_cell(rng, 1, 64, 0, 66, 64)])
    # operator 2, shift +1: the overlapping pair in the 130 x 64 block (sector 1 -> 2), and a cell of the 65 x 130 block
    a2 = GOp(1, False, [dense_cell(rng, 1, 0, 0, 40, 50), dense_cell(rng, 1, 30, 20, 100, 44), ident_cell(rng, 1, 70, 2, 33),
                        dense_cell(rng, 0, 1, 60, 63, 70)])
    d.left_ops = [a0, a1, a2]
    b0 = full_op(rng, rs, 0)
    b1 = GOp(-1, False, [dense_cell(rng, 1, 0, 0, 17, 33), dense_cell(rng, 1, 4, 16, 9, 17), dense_cell(rng, 2, 0, 0, 16, 17), ident_cell(rng, 2, 2, 0, 14)])
    d.right_ops = [b0, b1]
    d.terms = [(0.75, 0, 0), (-1.25, 1, 0), (0.5, 2, 1)]        # operators 0 and 1 merge under right operator 0
    d.h_left = GOp(0, False, [dense_cell(rng, 0, 0, 0, 65, 65), dense_cell(rng, 1, 0, 0, 130, 64), dense_cell(rng, 1, 0, 60, 130, 70), dense_cell(rng, 2, 0, 0, 64, 64)])
    d.h_right = full_op(rng, rs, 0)
    return d


def case_transposed_ld():
    rng = np.random.default_rng(103)
    ls, rs = [17, 33, 15], [16, 63, 2]
    d = GDesc("transposed_ld", ls, rs, _antidiagonal(3), [], [])
    kw = dict(transposed=True, pads=(1, 3, 7), leads=(1, 3, 5))
    for s in (-1, 0, 1):
        d.left_ops.append(full_op(rng, ls, s, **kw))
        d.right_ops.append(full_op(rng, rs, -s, **kw))
        d.terms.append((float(ggemm_values(rng, ())), len(d.left_ops) - 1, len(d.right_ops) - 1))
    d.h_left, d.h_right = full_op(rng, ls, 0, **kw), full_op(rng, rs, 0, **kw)          # not symmetric
    return d


def case_term_graph():
    rng = np.random.default_rng(104)
    ls, rs = [16, 33], [17, 15]
    d = GDesc("term_graph", ls, rs, [(0, 0), (0, 1), (1, 0), (1, 1)], [], [])
    L = [full_op(rng, ls, 0) for _ in range(5)]
    L[3] = copy.deepcopy(L[2])                                  # two operator entries with identical cells
    L.append(GOp(0, False, []))                                 # 5: no cells, used by a term
    L.append(full_op(rng, ls, 0))                               # 6: no term uses it
    R = [full_op(rng, rs, 0) for _ in range(6)]
    d.left_ops, d.right_ops = L, R
    d.terms = [(0.625, 0, 0), (-1.375, 0, 0),                   # the same pair twice
               (0.0, 1, 1),                                     # a = 0.0: no edge
               (0.9, 5, 0),                                     # the empty operator: with 0 - 0 a star at right operator 0 (right-keyed)
               (1.1, 2, 2), (-0.7, 3, 2), (0.8, 1, 2),          # a star at right operator 2 (right-keyed)
               (0.6, 4, 3), (-1.2, 4, 4), (0.45, 4, 5)]         # a star at left operator 4 (left-keyed)
    d.h_left, d.h_right = full_op(rng, ls, 0), None
    return d


def case_row_ranges():
    rng = np.random.default_rng(105)
    ls, rs = [64, 130, 15], [17, 33, 65]
    d = GDesc("row_ranges", ls, rs, _antidiagonal(3), [], [])
    # shift +1 from sector 0: the columns of these cells are the rows of the 130-row source block that stage 2 reads
    a0 = GOp(1, False, [dense_cell(rng, 0, 0, 0, 10, 5), dense_cell(rng, 0, 10, 40, 30, 30), dense_cell(rng, 0, 20, 60, 44, 40),
                        dense_cell(rng, 1, 0, 0, 130, 15)])
    a1 = GOp(1, False, [dense_cell(rng, 0, 5, 63, 3, 2)])       # another group: rows [63, 65) only
    a2 = GOp(0, False, [dense_cell(rng, 1, 0, 0, 5, 5), dense_cell(rng, 1, 50, 40, 20, 30), dense_cell(rng, 1, 60, 60, 70, 40), dense_cell(rng, 0, 0, 0, 64, 64),
                        dense_cell(rng, 2, 0, 0, 15, 15)])
    d.left_ops = [a0, a1, a2]
    d.right_ops = [full_op(rng, rs, -1), full_op(rng, rs, -1), full_op(rng, rs, -1), full_op(rng, rs, 0), full_op(rng, rs, 0)]
    d.terms = [(0.8, 0, 0), (-1.1, 0, 1), (0.7, 1, 2), (0.55, 1, 0), (1.3, 2, 3), (-0.65, 2, 4)]      # every left operator keys its own group
    d.h_left, d.h_right = full_op(rng, ls, 0), full_op(rng, rs, 0)
    return d


def case_thin():
    rng = np.random.default_rng(106)
    ls, rs = [1, 129, 2], [2, 1, 129]
    d = GDesc("thin", ls, rs, _antidiagonal(3), [], [])
    for s in (-1, 0, 1):
        d.left_ops.append(full_op(rng, ls, s, transposed=(s == 1)))
        d.right_ops.append(full_op(rng, rs, -s))
        d.terms.append((float(ggemm_values(rng, ())), len(d.left_ops) - 1, len(d.right_ops) - 1))
    d.h_left, d.h_right = full_op(rng, ls, 0), full_op(rng, rs, 0)
    return d


def _random_cells(rng, sizes, s, q, allow_pad):
    nr, nc = sizes[q], sizes[q + s]
    cells = []
    for _ in range(int(rng.integers(1, 4))):
        h, w = int(rng.integers(1, nr + 1)), int(rng.integers(1, nc + 1))
        r0, c0 = int(rng.integers(0, nr - h + 1)), int(rng.integers(0, nc - w + 1))
        if rng.random() < 0.3:
            m = min(h, w)
            cells.append(ident_cell(rng, q, r0, c0, m))
        else:
            pad, lead = (int(rng.choice((0, 1, 3, 7))), int(rng.choice((0, 1, 2, 3)))) if allow_pad else (0, 0)
            cells.append(dense_cell(rng, q, r0, c0, h, w, pad, lead))
    return cells


def case_random(seed):
    """Everything above drawn at random: five sectors per side from SIZES (one large one per side at most), the anti-diagonal with one
    interior KronBlock left out, operators of every shift in -2 .. 2 with one to three random cells per sector block, random
    `transposed`, ld_pad and pointer offsets, random terms, then a duplicate term, a zero coefficient and an operator nobody uses."""
    rng = np.random.default_rng(7000 + seed)
    small, large = SIZES[:8], SIZES[8:]

    def sizes():
        v = [int(rng.choice(small)) for _ in range(5)]
        v[int(rng.integers(0, 5))] = int(rng.choice(large))
        return v

    ls, rs = sizes(), sizes()
    d = GDesc("random%d" % seed, ls, rs, _antidiagonal(5, leave_out=(int(rng.integers(1, 4)),)), [], [])
    for side, sz, ops in ((0, ls, d.left_ops), (1, rs, d.right_ops)):
        for s in (-2, -1, 0, 1, 2, int(rng.integers(-2, 3)), 0):
            op = GOp(s if side == 0 else -s, bool(rng.random() < 0.4))
            for q in range(5):
                if 0 <= q + op.stored_shift < 5 and rng.random() < 0.85:
                    op.cells += _random_cells(rng, sz, op.stored_shift, q, True)
            ops.append(op)
    pairs = [(i, j) for i, A in enumerate(d.left_ops[:-1]) for j, B in enumerate(d.right_ops) if A.shift + B.shift == 0]
    for p in rng.permutation(len(pairs))[:9]:
        d.terms.append((float(ggemm_values(rng, ())),) + pairs[p])
    d.terms.append((float(ggemm_values(rng, ())),) + tuple(d.terms[0][1:]))        # a duplicate
    d.terms.append((0.0,) + pairs[int(rng.integers(0, len(pairs)))])               # a zero coefficient; the last left operator stays unused

    def h(sz):
        u = rng.random()
        if u < 0.15:
            return None
        if u < 0.3:
            return GOp(0, False, [])
        op = GOp(0, bool(rng.random() < 0.5))
        for q in range(5):
            op.cells += _random_cells(rng, sz, 0, q, True)
        return op

    d.h_left, d.h_right = h(ls), h(rs)
    return d


NAMED = {"shifts": case_shifts, "overlap": case_overlap, "transposed_ld": case_transposed_ld, "term_graph": case_term_graph,
         "row_ranges": case_row_ranges, "thin": case_thin}
RANDOM_SEEDS = [0, 1, 2, 3, 4, 5]
CASES = list(NAMED) + ["random%d" % s for s in RANDOM_SEEDS]
_CASES, _REFERENCES = {}, {}


def case(name):
    """(descriptor, graded x) of a case; built once per process, to be left unchanged."""
    if name not in _CASES:
        d = NAMED[name]() if name in NAMED else case_random(int(name[len("random"):]))
        assert d.n_states < 40000 and (name == "shifts" or all(s in SIZES for s in d.left_sizes + d.right_sizes)), name      # (shifts: the sizes it was specified with)
        _CASES[name] = (d, graded_x(d, len(_CASES)))
    return _CASES[name]


def case_reference(name, dtype=np.longdouble):
    """(R, S_abs, n) of the case's graded apply at `dtype`, once per process, read-only."""
    key = (name, np.dtype(dtype).name)
    if key not in _REFERENCES:
        d, x = case(name)
        out = reference(d, x, dtype)
        for a in out:
            a.setflags(write=False)
        _REFERENCES[key] = out
    return _REFERENCES[key]


def min_vertex_cover(desc):
    """Size of a minimum vertex cover of the bipartite graph (left operators) -- terms of non-zero coefficient -- (right operators):
    by Koenig's theorem the size of a maximum matching (augmenting paths)."""
    adj = {}
    for (a, li, ri) in desc.terms:
        if a != 0.0:
            adj.setdefault(li, set()).add(ri)
    match = {}

    def augment(l, seen):
        for r in sorted(adj[l]):
            if r in seen:
                continue
            seen.add(r)
            if r not in match or augment(match[r], seen):
                match[r] = l
                return True
        return False

    return sum(augment(l, set()) for l in sorted(adj))


# ---- faults: the reference with a faulty definition -------------------------------------------------------------------------------------
FAULTS = ["term_dropped", "term_twice", "cell_dropped", "cell_untransposed", "cell_one_column_right", "x_from_neighbour", "rows_left_zero"]


def _ops_of(desc):
    """[(where, index, operator)] of every operator a contribution goes through: those of terms with a != 0, H_L, H_R."""
    used_l = sorted({li for (a, li, ri) in desc.terms if a != 0.0})
    used_r = sorted({ri for (a, li, ri) in desc.terms if a != 0.0})
    out = [("left_ops", i, desc.left_ops[i]) for i in used_l] + [("right_ops", i, desc.right_ops[i]) for i in used_r]
    return out + [(w, None, getattr(desc, w)) for w in ("h_left", "h_right") if getattr(desc, w) is not None]


def _with_cell(desc, where, index, ci, new_cell):
    """A copy of desc whose operator (where, index) has cell ci replaced (None: removed); everything else is shared."""
    d = copy.copy(desc)
    op = copy.copy(getattr(desc, where) if index is None else getattr(desc, where)[index])
    op.cells = [c for j, c in enumerate(op.cells) if j != ci] if new_cell is None else [new_cell if j == ci else c for j, c in enumerate(op.cells)]
    if index is None:
        setattr(d, where, op)
    else:
        lst = list(getattr(desc, where))
        lst[index] = op
        setattr(d, where, lst)
    return d


def fault_candidates(desc, x, kind, limit=12):
    """Up to `limit` faults of one kind as (descriptor, x, rows to zero or None), spread over the descriptor."""
    out = []
    live = [t for t, (a, _, _) in enumerate(desc.terms) if a != 0.0]
    if kind in ("term_dropped", "term_twice"):
        for t in live:
            d = copy.copy(desc)
            d.terms = [u for j, u in enumerate(desc.terms) if j != t] if kind == "term_dropped" else list(desc.terms) + [desc.terms[t]]
            out.append((d, x, None))
    elif kind in ("cell_dropped", "cell_untransposed", "cell_one_column_right"):
        for where, index, op in _ops_of(desc):
            for ci, c in enumerate(op.cells):
                if kind == "cell_dropped":
                    out.append((_with_cell(desc, where, index, ci, None), x, None))
                    break
                if c.kind != CELL_DENSE or c.nr * c.nc < 2:
                    continue
                new = copy.copy(c)
                if kind == "cell_untransposed":
                    if min(c.nr, c.nc) < 2:
                        continue
                    # the cell's memory walked in the other orientation: in a transposed operator the stored nr x nc array taken as the
                    # nc x nr cell as used without transposing it, in a plain operator the other way round
                    new.array = np.ascontiguousarray(c.array.reshape(c.nc, c.nr).T)
                else:
                    # every element from one place further on in memory: the next column, at a row's end the first element of the next
                    # row (a leading dimension taken without its pad)
                    flat = c.array.ravel()
                    new.array = np.concatenate([flat[1:], flat[:1]]).reshape(c.nr, c.nc)
                out.append((_with_cell(desc, where, index, ci, new), x, None))
                break
    elif kind == "x_from_neighbour":
        off = desc.offsets()
        for k in range(len(desc.blocks)):
            kn = k + 1 if k + 1 < len(desc.blocks) else k - 1
            x2 = np.array(x)
            x2[off[k]:off[k + 1]] = np.resize(x[off[kn]:off[kn + 1]], off[k + 1] - off[k])
            out.append((desc, x2, None))
    elif kind == "rows_left_zero":
        off = desc.offsets()
        for k, (il, ir) in enumerate(desc.blocks):
            nrow = min(2, desc.left_sizes[il])
            out.append((desc, x, (off[k], off[k] + nrow * desc.right_sizes[ir])))
    else:
        raise KeyError(kind)
    step = max(1, len(out) // limit)
    return out[::step][:limit]


def faulty_result(desc, x, fault, dtype=np.float64):
    d, x2, zero = fault
    y = np.array(reference(d, x2, dtype)[0])
    if zero is not None:
        y[zero[0]:zero[1]] = 0
    return y


VISIBLE = 2.0 ** -36      # of an element's sum of magnitudes: eleven times kron_bound at n = 3000, above the largest n of the cases


def _share(err, S_abs):
    return np.where(S_abs > 0, err / np.where(S_abs > 0, S_abs, 1.0), 0.0)


def subtlest_fault(desc, x, kind, R64, S_abs):
    """The faulty result to show the checker: of every candidate fault the ONE element of y whose error is the smallest share of its sum of
    magnitudes while still reaching VISIBLE, every other element as it should be -- chosen from the float64 references alone, with a
    fixed threshold.  (The checker looks at every element by itself, so it catches the whole fault if it catches this element; a fault
    below the rounding of a correct result cannot be seen by any check, and one of half an element's sum is seen by every check.)
    -> (y, (candidate, element), share), or (None, None, 0.0)."""
    best = (None, None, np.inf)
    for i, f in enumerate(fault_candidates(desc, x, kind)):
        yf = faulty_result(desc, x, f)
        share = _share(np.abs(yf - R64), S_abs)
        share[share < VISIBLE] = np.inf
        e = int(np.argmin(share))
        if share[e] < best[2]:
            y = np.array(R64)
            y[e] = yf[e]
            best = (y, (i, e), float(share[e]))
    return best if best[0] is not None else (None, None, 0.0)


def term_dropped_in_weakest_block(desc, x, R64, S_abs):
    """The float64 result with one term left out of the weakest KronBlock only: the term whose part is the smallest share of an element's
    sum of magnitudes there that still reaches VISIBLE.  -> (y, term, share)"""
    w, off = weakest_block(desc), desc.offsets()
    seg = slice(off[w], off[w + 1])
    best, best_v = None, np.inf
    for t, (a, _, _) in enumerate(desc.terms):
        v = float(_share(reference(desc, x, np.float64, only={(t, w)})[1][seg], S_abs[seg]).max()) if a != 0.0 else 0.0
        if VISIBLE <= v < best_v:
            best, best_v = t, v
    assert best is not None, "%s: no term reaches the weakest KronBlock visibly" % desc.name
    keep = {(t, k) for t in range(len(desc.terms)) for k in range(len(desc.blocks)) if (t, k) != (best, w)}
    keep |= {(s, k) for s in ("L", "R") for k in range(len(desc.blocks))}
    return reference(desc, x, np.float64, only=keep)[0], best, best_v


# ---- raw builder: _capi.KronDesc filled directly --------------------------------------------------------------------------------------
_RAW_CLASS = []


def _raw_class():
    if _RAW_CLASS:
        return _RAW_CLASS[0]
    import torch
    from dmrgx_amd import _capi, superblock

    class RawKronPlan(superblock.KronPlan):
        """A plan created from a GDesc; apply, to_striped, from_striped, destroy and info are superblock.KronPlan's on the handle."""

        def __init__(self, desc, world_size=None, rank=0, device="cuda:0"):
            _capi.require_device()
            self.desc, self.device = desc, torch.device(device)
            self._keep, self._handle = [], C.c_void_p()
            W = desc.world_size if world_size is None else world_size

            def secop(op):
                if op is None:
                    return None
                cells = (_capi.Cell * max(len(op.cells), 1))()
                for i, c in enumerate(op.cells):
                    cells[i].row_sector, cells[i].r0, cells[i].c0, cells[i].nr, cells[i].nc = c.row_sector, c.r0, c.c0, c.nr, c.nc
                    cells[i].kind, cells[i].scale = c.kind, c.scale
                    if c.kind == CELL_DENSE:
                        ld = c.nc + c.ld_pad                    # stored as given, in a NaN-filled array
                        buf = np.full(c.lead + c.nr * ld + 1, np.nan)
                        wide = buf[c.lead:c.lead + c.nr * ld].reshape(c.nr, ld)
                        wide[:, :c.nc] = c.array
                        t = torch.from_numpy(buf).to(self.device)
                        self._keep.append(t)
                        cells[i].data, cells[i].ld = t.data_ptr() + 8 * c.lead, ld
                self._keep.append(cells)
                s = _capi.SecOp()
                s.shift, s.transposed, s.ncells, s.cells = op.shift, (1 if op.transposed else 0), len(op.cells), cells
                return s

            def i32(v):
                arr = (C.c_int32 * max(len(v), 1))(*[int(a) for a in v])
                self._keep.append(arr)
                return arr

            lops, rops = [secop(o) for o in desc.left_ops], [secop(o) for o in desc.right_ops]
            larr, rarr = (_capi.SecOp * max(len(lops), 1))(*lops), (_capi.SecOp * max(len(rops), 1))(*rops)
            terms = (_capi.Term * max(len(desc.terms), 1))()
            for i, (a, li, ri) in enumerate(desc.terms):
                terms[i].a, terms[i].left_op, terms[i].right_op = float(a), int(li), int(ri)
            hl, hr = secop(desc.h_left), secop(desc.h_right)
            d = _capi.KronDesc()
            d.left.nsec, d.left.size = len(desc.left_sizes), i32(desc.left_sizes)
            d.right.nsec, d.right.size = len(desc.right_sizes), i32(desc.right_sizes)
            d.nblocks, d.block_il, d.block_ir = len(desc.blocks), i32([b[0] for b in desc.blocks]), i32([b[1] for b in desc.blocks])
            d.n_left_ops, d.n_right_ops, d.left_ops, d.right_ops = len(lops), len(rops), larr, rarr
            d.h_left = C.pointer(hl) if hl is not None else None
            d.h_right = C.pointer(hr) if hr is not None else None
            d.nterms, d.terms = len(desc.terms), terms
            d.world_size, d.rank = W, rank
            st = self._stream_ptr(None)
            with torch.cuda.device(self.device):
                _capi.check(_capi.lib().dmrgx_kron_plan_create(C.byref(d), st, C.byref(self._handle)))
                torch.cuda.current_stream().synchronize()
            self._keep.clear()              # the plan owns copies of every operator
            self.info = _capi.KronInfo()
            _capi.check(_capi.lib().dmrgx_kron_plan_info(self._handle, C.byref(self.info)))
            self.world_size, self.rank = W, rank

        def diag(self, d_local):
            """d_local <- this rank's segment of the diagonal (dmrgx_kron_diag)."""
            assert d_local.dtype == torch.float64 and d_local.numel() >= self.info.local_len
            _capi.check(_capi.lib().dmrgx_kron_diag(self._handle, C.c_void_p(d_local.data_ptr()), self._stream_ptr(None)))

    _RAW_CLASS.append(RawKronPlan)
    return RawKronPlan


def raw_plan(desc, world_size=None, rank=0):
    """The plan of a GDesc through dmrgx_kron_plan_create: an object with apply, to_striped, from_striped, diag, info and destroy."""
    return _raw_class()(desc, world_size=world_size, rank=rank)
