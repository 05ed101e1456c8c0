"""dmrgx_secop_compose (-m gpu): sums of products of one, two and three sector operators of one block, dense per sector, against numpy on
random operators.  Sector sizes on both sides of the 64-wide tile and the degenerate ones; operators of shift 0, +1 and -1, one read
transposed, one with a missing cell and split cells, two with identity cells; outputs of every factor count and of net shift 0, +-1 and
+2.  The comparison is the forward-error bound of helpers.ggemm_bound on sum |c| |F1| |F2| |F3|, not a fixed tolerance: a block that no
string reaches has bound 0 and must be exact zeros."""
import ctypes as C

import numpy as np
import pytest

from helpers import ggemm_bound

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_OUTOFRANGE = 62, 63
SIZES = (1, 3, 63, 65, 130, 2)
NS = len(SIZES)


@pytest.fixture(scope="module")
def mods(pkg):
    from dmrgx_amd import superblock, workloads, _capi
    _capi.require_device()
    return superblock, workloads, _capi


def _values(rng, shape):
    return rng.uniform(0.5, 1.5, size=shape) * rng.choice((-1.0, 1.0), size=shape)


def _operators(wl):
    """[(SectorOperator, transposed)]: the stored cells and whether the call reads them transposed."""
    rng = np.random.default_rng(20261020)
    D, I = wl.CELL_DENSE, wl.CELL_IDENT

    def dense(q, shift, r0=0, c0=0, nr=None, nc=None):
        nr = SIZES[q] - r0 if nr is None else nr
        nc = SIZES[q + shift] - c0 if nc is None else nc
        return wl.OpCell(q, r0, c0, nr, nc, D, 0.0, np.ascontiguousarray(_values(rng, (nr, nc))))

    ops = []
    ops.append((wl.SectorOperator(0, [dense(q, 0) for q in range(NS)]), False))                                          # 0: shift 0, every block
    ops.append((wl.SectorOperator(1, [dense(q, 1) for q in range(NS - 1)]), False))                                      # 1: shift +1
    ops.append((wl.SectorOperator(1, [dense(q, 1) for q in range(NS - 1)]), True))                                       # 2: shift -1, read transposed
    ops.append((wl.SectorOperator(0, [dense(0, 0), dense(1, 0), dense(2, 0), dense(4, 0, 0, 0, 70, 130), dense(4, 0, 70, 10, 60, 90),
                                      dense(5, 0)]), False))                                                             # 3: no cell in sector 3, two cells in 4
    ops.append((wl.SectorOperator(1, [dense(0, 1), wl.OpCell(2, 0, 2, 40, 40, I, 0.75), dense(2, 1, 40, 0, 23, 65),
                                      wl.OpCell(3, 5, 60, 60, 60, I, -1.5), dense(4, 1)]), False))                       # 4: shift +1, identity cells
    ops.append((wl.SectorOperator(0, [dense(2, 0), wl.OpCell(3, 10, 0, 30, 30, I, 0.5), dense(3, 0, 40, 0, 25, 65),
                                      wl.OpCell(4, 0, 0, 130, 130, I, 2.0), dense(5, 0)]), False))                       # 5: shift 0, identity cells
    ops.append((wl.SectorOperator(-1, [dense(q, -1) for q in range(1, NS)]), False))                                     # 6: shift -1, stored plainly
    ops.append((wl.SectorOperator(1, []), False))                                                                        # 7: shift +1, no cells at all
    return ops


# (coefficient, factors); every output one net shift
OUTPUTS = [
    [(0.5, [1]), (-0.5, [4])],                                             # 0: one factor, shift +1; a dense and an identity-cell operator
    [(0.5, [1, 2]), (-0.5, [2, 1]), (1.0, [5, 5])],                        # 1: two factors, shift 0; middle sector off the table's end (q = 5) and start (q = 0); identity . identity
    [(0.5, [0, 1, 3]), (-0.5, [0, 1, 5])],                                 # 2: three factors, shift +1; the prefix 0 . 1 with both signs
    [(0.5, [0, 1, 2]), (-0.5, [3, 4, 6]), (0.5, [0, 1, 6])],               # 3: three factors, shift 0; shares the prefix (0, 1, +1/2) with output 2
    [(-0.5, [2, 5]), (0.5, [6]), (0.5, [5, 2, 0])],                        # 4: shift -1; one, two and three factors in one output
    [(1.0, [1, 7])],                                                       # 5: no string reaches any block: zeros, shift +2
    [(1.0, [4, 6]), (-0.5, [6, 4])],                                       # 6: identity . dense and dense . identity, shift 0
    [(1.0, [1, 4]), (0.5, [4, 4]), (-0.5, [4, 4, 5])],                     # 7: shift +2; two identity cells that overlap in part of the middle sector
]
SHIFTS = [1, 0, 1, 0, -1, 2, 0, 2]


def _blocks_as_used(op, transposed):
    """(shift as used, {row sector: dense block})."""
    shift = -op.shift if transposed else op.shift
    out = {}
    for c in op.cells:
        q, qc = c.row_sector, c.row_sector + op.shift
        blk = np.zeros((SIZES[q], SIZES[qc]))
        blk[c.r0:c.r0 + c.nr, c.c0:c.c0 + c.nc] = c.array if c.kind == 1 else c.scale * np.eye(c.nr)
        key = qc if transposed else q
        out[key] = out.get(key, 0.0) + (blk.T if transposed else blk)
    return shift, out


@pytest.fixture(scope="module")
def case(mods):
    """The operators and, per output and row sector, (reference block, sum of magnitudes, depth n of the bound); built once, read-only."""
    _, wl, _ = mods
    ops = _operators(wl)
    used = [_blocks_as_used(op, tr) for op, tr in ops]
    want = []
    for strings in OUTPUTS:
        s_o = sum(used[f][0] for f in strings[0][1])
        blocks = {}
        for q in range(NS):
            if not 0 <= q + s_o < NS:
                continue
            R, S, n = np.zeros((SIZES[q], SIZES[q + s_o])), np.zeros((SIZES[q], SIZES[q + s_o])), 0
            for c, fac in strings:
                assert sum(used[f][0] for f in fac) == s_o
                P, A, at, ok = None, None, q, True
                for pos, f in enumerate(fac):
                    shift, blk = used[f]
                    if not 0 <= at + shift < NS or at not in blk:
                        ok = False
                        break
                    n += SIZES[at] if pos else 0                # the depth of a product: the middle sector it sums over
                    P, A, at = (blk[at], np.abs(blk[at]), at + shift) if pos == 0 else (P @ blk[at], A @ np.abs(blk[at]), at + shift)
                if ok:
                    R, S = R + c * P, S + abs(c) * A
                n += 2                                          # the coefficient, the sum over the strings
            for a in (R, S):
                a.setflags(write=False)
            blocks[q] = (R, S, n)
        want.append((s_o, blocks))
    return ops, want


def test_the_inputs_hit_every_path(case):
    ops, want = case
    assert [w[0] for w in want] == SHIFTS
    assert any(tr for _, tr in ops) and 3 not in {c.row_sector for c in ops[3][0].cells}
    assert {c.kind for c in ops[4][0].cells} == {1, 2} and {c.kind for c in ops[5][0].cells} == {1, 2}
    assert {len(f) for o in OUTPUTS for _, f in o} == {1, 2, 3} and {c for o in OUTPUTS for c, _ in o} >= {0.5, -0.5}
    assert all(not S.any() for _, S, _ in want[5][1].values()) and len(want[5][1]) == 4         # the unreached output
    assert sum(1 for o in OUTPUTS for c, f in o if c == 0.5 and f[:2] == [0, 1] and len(f) == 3) == 3      # the shared prefix
    for s_o, blocks in want:
        for q, (R, S, n) in blocks.items():
            assert R.shape == (SIZES[q], SIZES[q + s_o])
    assert max(np.abs(R).max() for _, b in want for R, _, _ in b.values()) > 10.0


def _check(got, blocks_of_output, want, what):
    worst = 0.0
    for o, (s_o, blocks) in enumerate(want):
        assert [b[0] for b in blocks_of_output[o]] == sorted(blocks), (o, blocks_of_output[o])
        for q, off, nr, nc in blocks_of_output[o]:
            R, S, n = blocks[q]
            assert (nr, nc) == R.shape
            g = got[off:off + nr * nc].reshape(nr, nc)
            bound = ggemm_bound(S, n)
            bad = ~(np.abs(g - R) <= bound)
            assert not bad.any(), "%s: output %d sector %d: %d of %d elements outside the bound, worst %.3e" % (what, o, q, bad.sum(), bad.size, np.abs(g - R).max())
            if bound.max() > 0:
                worst = max(worst, float(np.max(np.where(bound > 0, np.abs(g - R) / np.where(bound > 0, bound, 1.0), 0.0))))
            if not S.any():
                assert not g.any()
    return worst


def test_compose_against_numpy(mods, case):
    """Sizes-only mode, then the real call into a NaN-filled arena with three spare elements: every element overwritten, every block
    within its bound, the cells packed in ascending row sector one after the other, and the same bits from a second call."""
    import torch
    sbm, _, capi = mods
    ops, want = case
    args, total, keep = sbm._compose_arguments(SIZES, ops, OUTPUTS)
    assert capi.lib().dmrgx_secop_compose(*args, None, None) == 0
    n_doubles = sum(R.size for _, b in want for R, _, _ in b.values())
    assert total.value == n_doubles
    shift, cell_first, cells = args[6], args[7], args[8]
    assert list(shift[:len(OUTPUTS)]) == SHIFTS
    sizes_only = [(cells[c].row_sector, cells[c].r0, cells[c].c0, cells[c].nr, cells[c].nc, cells[c].kind, cells[c].ld, cells[c].data) for c in range(cell_first[len(OUTPUTS)])]
    assert all(t[1] == t[2] == 0 and t[5] == 1 and t[6] == t[4] and t[7] is None for t in sizes_only)
    arena = torch.full((n_doubles + 3,), float("nan"), dtype=torch.float64, device="cuda")
    out, shifts, blocks = sbm.secop_compose(SIZES, ops, OUTPUTS, out=arena)
    assert out is arena and shifts == SHIFTS
    got = arena.cpu().numpy()
    assert np.isnan(got[n_doubles:]).all() and np.isfinite(got[:n_doubles]).all()
    flat = [b for o in blocks for b in o]
    assert [(b[0], b[2], b[3]) for b in flat] == [(t[0], t[3], t[4]) for t in sizes_only]          # sizes-only mode agrees with the real call
    assert [b[1] for b in flat] == list(np.cumsum([0] + [b[2] * b[3] for b in flat])[:-1])          # packed: each cell starts where the one before ends
    worst = _check(got, blocks, want, "first call")
    print("secop_compose: %d outputs, %d doubles, worst |got - want| / bound %.3f" % (len(OUTPUTS), n_doubles, worst))
    out2, _, _ = sbm.secop_compose(SIZES, ops, OUTPUTS)
    assert np.array_equal(out2.cpu().numpy()[:n_doubles].view(np.uint64), got[:n_doubles].view(np.uint64))


def test_factor_order_is_kept(mods, case):
    """The operators do not commute: A B and B A of two shift-0 operators differ, and each matches its own numpy product."""
    sbm, _, _ = mods
    ops, _ = case
    out, _, blocks = sbm.secop_compose(SIZES, ops, [[(1.0, [0, 3])], [(1.0, [3, 0])]])
    got = out.cpu().numpy()
    A, B = _blocks_as_used(*ops[0])[1], _blocks_as_used(*ops[3])[1]
    for o, (X, Y) in enumerate(((A, B), (B, A))):
        for q, off, nr, nc in blocks[o]:
            g = got[off:off + nr * nc].reshape(nr, nc)
            if q not in X or q not in Y:
                assert not g.any()
                continue
            assert (np.abs(g - X[q] @ Y[q]) <= ggemm_bound(np.abs(X[q]) @ np.abs(Y[q]), SIZES[q] + 2)).all()
    q, off, nr, nc = blocks[0][4]
    off2 = blocks[1][4][1]
    assert np.abs(got[off:off + nr * nc] - got[off2:off2 + nr * nc]).max() > 1.0


def test_compose_refusals(mods, case):
    """Every refusal of the header returns its status and leaves the arena untouched."""
    import torch
    sbm, wl, capi = mods
    L = capi.lib()
    ops, want = case
    call = L.dmrgx_secop_compose
    arena = torch.full((sum(R.size for _, b in want for R, _, _ in b.values()),), 7.0, dtype=torch.float64, device="cuda")
    ap = C.c_void_p(arena.data_ptr())

    def status(outputs, patch=None, operators=ops):
        args, total, keep = sbm._compose_arguments(SIZES, operators, outputs)
        args = list(args)
        if patch:
            patch(args)
        return call(*args, ap, None)

    good = [[(0.5, [0, 1])], [(1.0, [2])]]
    assert status(good) == 0
    arena.fill_(7.0)
    for i in (0, 2, 4, 5, 6, 7, 8, 9):                                     # null sector table, operators, out_first, strings, out_shift, cell_first, cells, n_doubles
        assert status(good, lambda a, i=i: a.__setitem__(i, None)) == ERR_ARG, i
    assert status(good, lambda a: a.__setitem__(1, -1)) == ERR_ARG         # n_ops < 0
    assert status(good, lambda a: a.__setitem__(3, -1)) == ERR_ARG         # n_out < 0
    assert status([[(0.5, [0, 1])], []]) == ERR_ARG and b"empty" in L.dmrgx_last_error()
    assert status([[(0.5, [])]]) == ERR_ARG
    assert status([[(0.5, [0, 0, 0, 0])]]) == ERR_ARG                      # (the wrapper stores three indices and nfac = 4)
    assert status([[(0.5, [0, 1]), (0.5, [0, 2])]]) == ERR_ARG and b"shift" in L.dmrgx_last_error()
    assert status([[(float("nan"), [0])]]) == ERR_ARG and status([[(float("inf"), [0, 1])]]) == ERR_ARG
    assert status([[(1.0, [0, len(ops)])]]) == ERR_OUTOFRANGE and status([[(1.0, [-1])]]) == ERR_OUTOFRANGE
    outside = ops + [(wl.SectorOperator(0, [wl.OpCell(1, 1, 0, 3, 3, wl.CELL_IDENT, 1.0)]), False)]
    assert status(good, operators=outside) == ERR_OUTOFRANGE
    past = ops + [(wl.SectorOperator(1, [wl.OpCell(5, 0, 0, 2, 2, wl.CELL_IDENT, 1.0)]), False)]
    assert status(good, operators=past) == ERR_OUTOFRANGE
    # an arena that overlaps an input: the first cell of operator 0 is made to lie inside it

    def overlap(a):
        a[2][0].cells[0].data = arena.data_ptr() + 8
    assert status(good, overlap) == ERR_ARG and b"overlap" in L.dmrgx_last_error()
    torch.cuda.synchronize()
    assert (arena == 7.0).all()
