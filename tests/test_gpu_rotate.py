"""K6 at its edges (-m gpu): dmrgx_cells_axpy and dmrgx_rotate_ops (csrc/rotate.hip) through the C ABI against plain numpy.

dmrgx_cells_axpy: integer-valued doubles and alpha in {1, -2, 0.5, 0.75}, so every sum is exact in f64 with or without fused
multiply-adds and the comparison is np.array_equal on the WHOLE device array -- destination windows, the frame round each window and
the gaps between the arrays, which are NaN.  Sources sit in a NaN array of their own: a read outside a source poisons the result.

dmrgx_rotate_ops: the reference is RT_a O_{q,q'} RT_a'^T with every operand in np.longdouble, O from workloads.operator_to_dense_blocks.
The bound is derived, not measured: |got - ref| <= gamma_k (|RT_a| |O| |RT_a'|^T) element by element, gamma_k = k u / (1 - k u),
u = 2^-53, k = n_q + n_q' + 2 -- two chained products of inner lengths n_q and n_q' under any summation order (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.5).  Rotations made of unit vectors make every product exact: then array_equal.
Destinations are NaN before the call and sit in one NaN array with gaps that must still be NaN afterwards.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import secop_from

pytestmark = pytest.mark.gpu
ALPHAS = (1.0, -2.0, 0.5, 0.75)
LADDER = [(1, 1), (1, 33), (33, 1), (31, 32), (32, 32), (33, 65), (64, 31), (97, 130)]


@pytest.fixture(scope="module")
def mods(pkg):
    from dmrgx_amd import superblock, workloads, _capi
    _capi.require_device()
    return superblock, workloads, _capi


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class Pool:
    """Matrices laid out one after the other in ONE flat NaN array with NaN gaps of 3 elements (odd offsets, nothing aligned): add() ->
    element offset, upload() -> the device copy, download() -> the device copy back on the host.  `host` keeps the initial content."""

    def __init__(self):
        self.parts, self.n = [], 0

    def add(self, a):
        off = self.n + 3
        self.parts.append((off, np.array(a, dtype=np.float64)))
        self.n = off + self.parts[-1][1].size
        return off

    def upload(self):
        self.host = np.full(self.n + 3, np.nan)
        for off, a in self.parts:
            self.host[off:off + a.size] = a.ravel()
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        return self

    def ptr(self, off):
        return self.dev.data_ptr() + 8 * off

    def download(self):
        torch.cuda.synchronize()
        return self.dev.cpu().numpy()


# ---- A. dmrgx_cells_axpy ---------------------------------------------------------------------------------------------------------------
def _task(doff, soff, ldd, lds, nr, nc, tr=0, alpha=1.0, base=None):
    """dst window at element `doff` of the destination pool (nr x nc, leading dimension ldd), source at `soff` of the source pool (None:
    identity source), base: element offset of dst_base (None: NULL)."""
    return SimpleNamespace(doff=doff, soff=soff, ldd=ldd, lds=lds, nr=nr, nc=nc, tr=tr, alpha=alpha, base=base)


def _view(flat, off, rows, cols, ld):
    assert off >= 0 and off + (rows - 1) * ld + cols <= flat.size
    return np.lib.stride_tricks.as_strided(flat[off:], shape=(rows, cols), strides=(8 * ld, 8))


def _apply_host(dst, src, t):
    """The statement of include/dmrgx.h for one task, in numpy on the flat host arrays."""
    win = _view(dst, t.doff, t.nr, t.nc, t.ldd)
    if t.soff is None:
        win[np.arange(t.nr), np.arange(t.nr)] += t.alpha
    elif t.tr:
        win += t.alpha * _view(src, t.soff, t.nc, t.nr, t.lds).T
    else:
        win += t.alpha * _view(src, t.soff, t.nr, t.nc, t.lds)


def _ctasks(capi, specs, dpool, spool):
    tasks = (capi.AxpyTask * max(len(specs), 1))()
    for k, t in zip(tasks, specs):
        k.dst, k.dst_base = dpool.ptr(t.doff), (None if t.base is None else dpool.ptr(t.base))
        k.src = None if t.soff is None else spool.ptr(t.soff)
        k.ldd, k.lds, k.nr, k.nc, k.transposed, k.alpha = t.ldd, t.lds, t.nr, t.nc, t.tr, t.alpha
    return tasks


def _submit(capi, specs, dpool, spool, ref):
    """One dmrgx_cells_axpy call with `specs`; the same tasks one after the other on the host array `ref`."""
    capi.check(capi.lib().dmrgx_cells_axpy(len(specs), _ctasks(capi, specs, dpool, spool), _stream()))
    for t in specs:
        _apply_host(ref, spool.host, t)


def _framed(window, top=3, left=5, bottom=2, right=4, fill=np.nan):
    """(array, element offset of the window inside it, its leading dimension): `window` at an odd offset inside a larger array."""
    nr, nc = window.shape
    a = np.full((nr + top + bottom, nc + left + right), fill)
    a[top:top + nr, left:left + nc] = window
    return a, top * a.shape[1] + left, a.shape[1]


def _padded(values, pad):
    """values with `pad` NaN columns appended -> (array, leading dimension)."""
    a = np.full((values.shape[0], values.shape[1] + pad), np.nan)
    a[:, :values.shape[1]] = values
    return a, a.shape[1]


def test_cells_axpy_shape_ladder(mods):
    """Plain and transposed at the 32-wide tile edges, one row, one column: 16 tasks in one call with dst_base = NULL, then the two largest
    again, one per call.  Windows at odd offsets (ldd > nc); lds exactly minimal (nc plain, nr transposed) for half of the tasks of each
    mode; arange sources, so that a transposed or mirrored tile cannot pass."""
    _, _, capi = mods
    dpool, spool, specs = Pool(), Pool(), []
    for tr in (0, 1):
        for i, (nr, nc) in enumerate(LADDER):
            window = 1000.0 * (len(specs) + 1) + np.arange(nr * nc, dtype=np.float64).reshape(nr, nc) % 7
            arr, woff, ldd = _framed(window)
            src = 1.0 + np.arange(nr * nc, dtype=np.float64).reshape((nc, nr) if tr else (nr, nc))
            sarr, lds = _padded(src, 0 if (i + tr) % 2 else 3)
            specs.append(_task(dpool.add(arr) + woff, spool.add(sarr), ldd, lds, nr, nc, tr, ALPHAS[(i + tr) % 4]))
    minimal = [t.lds == (t.nr if t.tr else t.nc) for t in specs]
    assert sum(minimal[:8]) == 4 and sum(minimal[8:]) == 4 and all(t.ldd > t.nc for t in specs)
    dpool.upload(), spool.upload()
    ref = dpool.host.copy()
    _submit(capi, specs, dpool, spool, ref)
    got = dpool.download()
    assert np.array_equal(got, ref, equal_nan=True), np.argwhere(_bits(got) != _bits(ref))[:5]
    for t in (specs[7], specs[15]):
        assert (t.nr, t.nc) == (97, 130)
        _submit(capi, [t], dpool, spool, ref)
    got = dpool.download()
    assert np.array_equal(got, ref, equal_nan=True), np.argwhere(_bits(got) != _bits(ref))[:5]
    assert np.isfinite(ref).sum() == sum(nr * nc for nr, nc in LADDER) * 2


def test_cells_axpy_identity_source(mods):
    """src = NULL on an n x n window of a larger matrix: the diagonal gains exactly 0.75, every other element of the matrix is unchanged
    bit for bit."""
    _, _, capi = mods
    dpool, spool, specs = Pool(), Pool().upload(), []
    for n in (1, 31, 32, 33, 70):
        matrix = 1.0 + np.arange((n + 5) * (n + 9), dtype=np.float64).reshape(n + 5, n + 9)
        specs.append(_task(dpool.add(matrix) + 3 * (n + 9) + 5, None, n + 9, 0, n, n, 0, 0.75))
    dpool.upload()
    ref = dpool.host.copy()
    _submit(capi, specs, dpool, spool, ref)
    got = dpool.download()
    assert np.array_equal(_bits(got), _bits(ref))
    assert int((_bits(ref) != _bits(dpool.host)).sum()) == 1 + 31 + 32 + 33 + 70


@pytest.mark.parametrize("n", [1, 40])
def test_cells_axpy_submission_order_by_bits(mods, n):
    """Three tasks with one dst_base add 2^-53, 2^-53 and 1.0 to the same elements, which start at 0: in that order the result is
    1 + 2^-52, with 1.0 earlier it is exactly 1.0 (ties to even) -- the order is visible in the last bit.  All three distinct orders, on a
    single element and on every element of a 40 x 40 window (four tiles)."""
    _, _, capi = mods
    tiny, one = 2.0 ** -53, 1.0
    for order in ((tiny, tiny, one), (tiny, one, tiny), (one, tiny, tiny)):
        dpool, spool = Pool(), Pool()
        arr, woff, ldd = _framed(np.zeros((n, n)))
        d = dpool.add(arr) + woff
        specs = [_task(d, spool.add(_padded(np.full((n, n), v), 2)[0]), ldd, n + 2, n, n, 0, 1.0, base=d) for v in order]
        dpool.upload(), spool.upload()
        ref = dpool.host.copy()
        _submit(capi, specs, dpool, spool, ref)
        want = np.float64(np.float64(np.float64(0.0) + order[0]) + order[1]) + order[2]
        assert want == (1.0 + 2.0 ** -52 if order[2] == one else 1.0) and (_view(ref, d, n, n, ldd) == want).all()
        got = dpool.download()
        assert np.array_equal(_bits(got), _bits(ref)), (order, _view(got, d, n, n, ldd)[0, 0].hex())


def test_cells_axpy_many_overlapping_tasks(mods):
    """24 tasks with one dst_base into a 70 x 70 integer matrix -- dense, transposed and identity sources in turn, as the assembly of an
    enlarged block's Hamiltonian issues them: distinct dst pointers, windows that overlap pairwise -- and 6 tasks with a second dst_base
    into a second matrix, interleaved in submission order.  A lost update between two tasks of one launch changes the exact sum."""
    _, _, capi = mods
    dpool, spool = Pool(), Pool()
    N = 70
    mats = []
    for k in range(2):
        arr, woff, ldd = _framed(100.0 * (k + 1) + np.arange(N * N, dtype=np.float64).reshape(N, N) % 11)
        mats.append((dpool.add(arr) + woff, ldd))

    def make(i, k):
        r0, c0 = i % 24, (7 * i + 3 * k) % 24
        nr, nc = 36 + (5 * i) % 11, 36 + (3 * i) % 11
        base, ldd = mats[k]
        d = base + r0 * ldd + c0
        kind = i % 3
        if kind == 2:
            return _task(d, None, ldd, 0, nr, nr, 0, ALPHAS[i % 4], base=base), (r0, c0, nr, nr)
        a, b = np.meshgrid(np.arange(nc if kind else nr), np.arange(nr if kind else nc), indexing="ij")
        sarr, lds = _padded(((3 * a + 5 * b + i) % 17 - 8).astype(np.float64), 2)
        return _task(d, spool.add(sarr), ldd, lds, nr, nc, kind, ALPHAS[i % 4], base=base), (r0, c0, nr, nc)

    specs, windows = [], []
    for i in range(24):
        t, w = make(i, 0)
        specs.append(t), windows.append(w)
        if i % 4 == 3:
            specs.append(make(i + 1, 1)[0])
    assert len(specs) == 30 and len({t.doff for t in specs}) == 30
    for (r0, c0, nr, nc) in windows:               # every window holds rows and columns 24 .. 35: they overlap pairwise
        assert r0 <= 24 and c0 <= 24 and r0 + nr >= 36 and c0 + nc >= 36 and r0 + nr <= N and c0 + nc <= N
    dpool.upload(), spool.upload()
    ref = dpool.host.copy()
    _submit(capi, specs, dpool, spool, ref)
    got = dpool.download()
    assert np.array_equal(got, ref, equal_nan=True), np.argwhere(_bits(got) != _bits(ref))[:5]


def test_cells_axpy_refusals(mods):
    """Malformed calls return DMRGX_ERR_ARG with a message and touch nothing -- also the well-formed task in front of the malformed one.
    Transposed with nr <= lds < nc is well-formed (lds counts the columns of the SOURCE, which has nr of them); n == 0 is OK."""
    _, _, capi = mods
    L = capi.lib()
    dpool, spool = Pool(), Pool()
    arr, woff, ldd = _framed(np.arange(54, dtype=np.float64).reshape(6, 9))
    d0 = dpool.add(arr) + woff
    d1 = dpool.add(arr) + woff
    s = spool.add(1.0 + np.arange(200, dtype=np.float64).reshape(10, 20))
    dpool.upload(), spool.upload()

    def good():
        return [_task(d0, s, ldd, 20, 6, 9, 0, 2.0), _task(d1, s, ldd, 20, 5, 9, 1, 0.5)]

    def bad(**kw):
        specs = good()
        for k, v in kw.items():
            setattr(specs[1], k, v)
        return len(specs), _ctasks(capi, specs, dpool, spool)

    null_dst = bad()
    null_dst[1][1].dst = None
    cases = {"n < 0": (-1, bad()[1]), "null tasks": (2, None), "dst == NULL": null_dst, "nr == 0": bad(nr=0), "ldd < nc": bad(ldd=8),
             "plain, lds < nc": bad(tr=0, lds=8), "transposed, lds < nr": bad(tr=1, lds=4), "identity source, nr != nc": bad(soff=None, nr=5, nc=6)}
    for what, (n, tasks) in cases.items():
        assert L.dmrgx_cells_axpy(n, tasks, _stream()) == capi.DMRGX_ERR_ARG, what
        assert L.dmrgx_last_error().decode().startswith("cells_axpy"), what
        assert np.array_equal(_bits(dpool.download()), _bits(dpool.host)), what
    assert L.dmrgx_cells_axpy(0, None, _stream()) == capi.DMRGX_OK
    assert np.array_equal(_bits(dpool.download()), _bits(dpool.host))
    ref = dpool.host.copy()
    _submit(capi, [_task(d1, s, ldd, 6, 5, 9, 1, 0.5)], dpool, spool, ref)          # source 9 x 5 with lds = 6: nr <= lds < nc
    assert np.array_equal(dpool.download(), ref, equal_nan=True)
    assert not np.array_equal(_bits(ref), _bits(dpool.host))


# ---- B. dmrgx_rotate_ops ---------------------------------------------------------------------------------------------------------------
def _rotate(capi, sizes, old_sector, kept, RT, ops, ld_pad=0, tweak=None):
    """One dmrgx_rotate_ops call.  RT_a and the NaN destinations live in Pools; `tweak(call)` may damage the ctypes arguments first.
    -> (status, destination pool as it came back, {(operator, new sector): (offset, rows, columns)})."""
    keep = []
    nn = len(old_sector)
    rpool = Pool()
    rt_off = [rpool.add(r) for r in RT]
    rpool.upload()
    new_of_old = {q: a for a, q in enumerate(old_sector)}
    dpool, where = Pool(), {}
    for o, op in enumerate(ops):
        for a, q in enumerate(old_sector):
            ap = new_of_old.get(q + op.shift)
            if ap is not None:
                where[(o, a)] = (dpool.add(np.full((kept[a], kept[ap]), np.nan)), kept[a], kept[ap])
    dpool.upload()
    c = SimpleNamespace()
    c.secops = (capi.SecOp * max(len(ops), 1))(*[secop_from(op, keep, ld_pad) for op in ops])
    c.rows = [(C.c_void_p * nn)() for _ in ops]
    for (o, a), (off, _, _) in where.items():
        c.rows[o][a] = dpool.ptr(off)                   # entries whose a' does not exist stay NULL
    c.dst = (C.POINTER(C.c_void_p) * max(len(ops), 1))(*[C.cast(r, C.POINTER(C.c_void_p)) for r in c.rows])
    c.sizes = (C.c_int32 * len(sizes))(*sizes)
    c.sec = capi.Sectors(len(sizes), c.sizes)
    c.old_sector, c.kept = (C.c_int32 * nn)(*old_sector), (C.c_int32 * nn)(*kept)
    c.rot_t = (C.c_void_p * nn)(*[rpool.ptr(off) for off in rt_off])
    c.rot = capi.Rotation()
    c.rot.n_new, c.rot.old_sector, c.rot.kept, c.rot.rot_t = nn, c.old_sector, c.kept, c.rot_t
    c.nops = len(ops)
    if tweak:
        tweak(c)
    status = capi.lib().dmrgx_rotate_ops(C.byref(c.sec), C.byref(c.rot), c.nops, c.secops, c.dst, _stream())
    out = dpool.download()
    del keep
    return status, out, where


def _gaps_are_nan(out, where):
    covered = np.zeros(out.size, dtype=bool)
    for off, m, mp in where.values():
        covered[off:off + m * mp] = True
    return bool(np.isnan(out[~covered]).all())


def _check_rotation(wl, capi, sizes, old_sector, kept, RT, ops, ld_pad, rows=None):
    """Runs the rotation and compares every destination with the longdouble reference under the derived bound -- or, with `rows` (RT_a =
    the unit vectors rows[a]), exactly with O[rows][:, cols].  -> (worst error / bound, {(operator, new sector): block})."""
    status, out, where = _rotate(capi, sizes, old_sector, kept, RT, ops, ld_pad)
    capi.check(status)
    assert _gaps_are_nan(out, where)
    ld_t, u = np.longdouble, np.longdouble(2.0) ** -53
    worst, blocks = 0.0, {}
    for (o, a), (off, m, mp) in where.items():
        q, qc = old_sector[a], old_sector[a] + ops[o].shift
        ap = old_sector.index(qc)
        got = out[off:off + m * mp].reshape(m, mp)
        blocks[(o, a)] = got
        O = wl.operator_to_dense_blocks(ops[o], sizes).get(q, np.zeros((sizes[q], sizes[qc])))
        if rows is not None:
            assert np.array_equal(got, O[rows[a]][:, rows[ap]]), (o, a)
            continue
        ref = RT[a].astype(ld_t) @ O.astype(ld_t) @ RT[ap].T.astype(ld_t)
        k = sizes[q] + sizes[qc] + 2
        bound = k * u / (1 - k * u) * (np.abs(RT[a]).astype(ld_t) @ np.abs(O).astype(ld_t) @ np.abs(RT[ap]).T.astype(ld_t))
        err = np.abs(got.astype(ld_t) - ref)
        ok = err <= bound
        if ok.all() and bound.max() > 0:
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
        assert ok.all(), (o, a, m, mp, float(err.max()), float(bound.max()), np.argwhere(~ok)[:3])
    print("rotate_ops: %d destinations, worst error / bound %.3g" % (len(where), worst))
    return worst, blocks


def _enlarged_case(wl, seed, integer=False):
    """The operators of an enlarged block kept_profile(24) (x) spin-1/2 -- sizes 1, 3, 6, 14, 14, 6, 3, 1 -- and a truncation that drops the
    interior sector 5 and keeps 1 state, a whole sector and values in between.  integer: integer-valued asymmetric dense cells and
    identity cells of scale 0.75."""
    rng = np.random.default_rng(seed)
    _, sizes, sub = wl.enlarged_sectors(wl.kept_profile(24))
    ops = [wl._old_site_op(rng, 0, sizes, sub), wl._old_site_op(rng, +1, sizes, sub), wl._new_site_op(0, sizes, sub), wl._new_site_op(+1, sizes, sub),
           wl._sym_block_op(rng, sizes)]
    ops.append(wl.SectorOperator(0, wl._old_site_op(rng, 0, sizes, sub).cells + wl._new_site_op(0, sizes, sub).cells))   # dense and identity over one range
    if integer:
        for op in ops:
            for c in op.cells:
                if c.kind == wl.CELL_DENSE:
                    c.array = np.ascontiguousarray(rng.integers(-9, 10, size=(c.nr, c.nc)).astype(np.float64))
                else:
                    c.scale = 0.75
    old_sector = [0, 1, 2, 3, 4, 6, 7]
    kept = [1, 3, 2, 14, 5, 1, 1]
    assert [sizes[q] for q in old_sector] == [1, 3, 6, 14, 14, 3, 1]
    # hole 1 of the old test: an identity cell whose pair (a, a') is cut away is skipped before stage A
    for shift in (0, 1):
        alive = [c for op in ops if op.shift == shift for c in op.cells
                 if c.kind == wl.CELL_IDENT and c.row_sector in old_sector and c.row_sector + shift in old_sector]
        assert alive and (shift == 0 or any(c.r0 != c.c0 for c in alive)), shift
    return rng, sizes, ops, old_sector, kept


def test_rotate_ops_enlarged_block_structure(mods):
    """O (x) 1 and 1 (x) s operators of shift 0 and +1 (identity cells with r0 != c0), a full H and an operator with a dense and an
    identity cell over the same range; every dense cell a view with ld = nc + 3."""
    _, wl, capi = mods
    rng, sizes, ops, old_sector, kept = _enlarged_case(wl, 41)
    RT = [rng.standard_normal((m, sizes[q])) for q, m in zip(old_sector, kept)]
    _check_rotation(wl, capi, sizes, old_sector, kept, RT, ops, 3)


def test_rotate_ops_exact_rotation(mods):
    """Rows of RT_a = distinct unit vectors (a permutation where the whole sector is kept, a selection otherwise), integer cells, identity
    scale 0.75: every product is exact and O' = O[rows][:, cols] -- fails on a transposed UT, a dropped r0 or a dropped c0 * m'."""
    _, wl, capi = mods
    rng, sizes, ops, old_sector, kept = _enlarged_case(wl, 42, integer=True)
    rows = [rng.permutation(sizes[q])[:m] for q, m in zip(old_sector, kept)]
    assert any(m > 1 and not np.array_equal(r, np.sort(r)) for r, m in zip(rows, kept))
    RT = [np.eye(sizes[q])[r] for q, r in zip(old_sector, rows)]
    _check_rotation(wl, capi, sizes, old_sector, kept, RT, ops, 3, rows=rows)


def test_rotate_ops_size_edges(mods):
    """Sector sizes 1, 2, 63, 64, 65, 129 (both sides of the 64-wide GEMM tile and of the 128-wide one) keeping 1, 1, 63, 17, 65, 128:
    operators of shift 0 and +1 with two cells per sector block, split at an odd row (shift 0) or column (shift +1), and a full-block H;
    ld = nc + 1."""
    _, wl, capi = mods
    rng = np.random.default_rng(43)
    sizes, kept = [1, 2, 63, 64, 65, 129], [1, 1, 63, 17, 65, 128]

    def dense(q, r0, c0, nr, nc):
        return wl.OpCell(q, r0, c0, nr, nc, wl.CELL_DENSE, 0.0, np.ascontiguousarray(rng.standard_normal((nr, nc))))

    def odd_cut(n):
        return (n // 2) | 1

    by_rows, by_cols = wl.SectorOperator(0), wl.SectorOperator(+1)
    for q, n in enumerate(sizes):
        r = odd_cut(n)
        by_rows.cells += [dense(q, 0, 0, n, n)] if n == 1 else [dense(q, 0, 0, r, n), dense(q, r, 0, n - r, n)]
        if q + 1 < len(sizes):
            nc = sizes[q + 1]
            c = odd_cut(nc)
            assert 0 < c < nc and c % 2 == 1
            by_cols.cells += [dense(q, 0, 0, n, c), dense(q, 0, c, n, nc - c)]
    ops = [by_rows, by_cols, wl._sym_block_op(rng, sizes)]
    old_sector = list(range(len(sizes)))
    RT = [rng.standard_normal((m, sizes[q])) for q, m in zip(old_sector, kept)]
    _check_rotation(wl, capi, sizes, old_sector, kept, RT, ops, 1)


def test_rotate_ops_truncation_patterns(mods):
    """One five-sector operator set under three rotations that drop the first, the last and a middle sector.  Destinations that exist but
    are reached by no source cell come back all zero (they were NaN), entries of dst_blocks whose a' does not exist are NULL, one
    operator per rotation has every cell cut away; nops == 0 is OK."""
    _, wl, capi = mods
    rng = np.random.default_rng(44)
    sizes = [3, 6, 5, 4, 2]

    def dense(q, r0, c0, nr, nc):
        return wl.OpCell(q, r0, c0, nr, nc, wl.CELL_DENSE, 0.0, np.ascontiguousarray(rng.standard_normal((nr, nc))))

    h = wl._sym_block_op(rng, sizes)
    raise_ = wl.SectorOperator(+1, [dense(0, 1, 2, 2, 3), dense(1, 0, 0, 6, 5), dense(2, 2, 1, 3, 2), dense(3, 0, 0, 4, 2)])
    ident = wl.SectorOperator(+1, [wl.OpCell(0, 1, 3, 2, 2, wl.CELL_IDENT, 0.75), wl.OpCell(1, 2, 0, 4, 4, wl.CELL_IDENT, -0.5),
                                   wl.OpCell(2, 0, 1, 3, 3, wl.CELL_IDENT, 1.25), wl.OpCell(3, 2, 0, 2, 2, wl.CELL_IDENT, 2.0)])
    sparse = wl.SectorOperator(+1, [dense(1, 1, 1, 3, 3)])                 # sectors 0, 2, 3: destinations without a source cell
    for dropped, kept in ((0, [6, 2, 4, 1]), (4, [1, 6, 3, 4]), (2, [3, 4, 2, 2])):
        old_sector = [q for q in range(5) if q != dropped]
        lone = wl.SectorOperator(0, [dense(dropped, 0, 0, sizes[dropped], sizes[dropped])])
        pair = wl.SectorOperator(+1, [dense(dropped - 1, 0, 0, sizes[dropped - 1], sizes[dropped])] if dropped else [dense(0, 0, 0, 3, 6)])
        ops = [h, raise_, ident, sparse, lone, pair]
        RT = [rng.standard_normal((m, sizes[q])) for q, m in zip(old_sector, kept)]
        _, blocks = _check_rotation(wl, capi, sizes, old_sector, kept, RT, ops, 0)
        assert len(blocks) < len(ops) * 4 and all((4, a) in blocks for a in range(4))        # NULL entries; `lone` has all four
        for o in (4, 5):                                                                     # every cell cut away: zeros, not NaN
            mine = [b for (oo, a), b in blocks.items() if oo == o]
            assert mine and all(b.size and not b.any() and np.isfinite(b).all() for b in mine), (dropped, o)
        unreached = [b for (oo, a), b in blocks.items() if oo == 3 and old_sector[a] != 1]
        assert unreached and all(not b.any() and np.isfinite(b).all() for b in unreached), dropped

    def no_ops(c):
        c.nops = 0
    status, out, where = _rotate(capi, sizes, [0, 1, 3, 4], [3, 4, 2, 2], RT, [h], tweak=no_ops)
    assert status == capi.DMRGX_OK and len(where) == 4 and np.isnan(out).all()


def _refusal_case(wl):
    """sizes 3, 4, 5, everything kept in part; operator 0: dense cells of shift 0, operator 1: identity cells of shift +1."""
    rng = np.random.default_rng(45)
    sizes, old_sector, kept = [3, 4, 5], [0, 1, 2], [2, 3, 4]
    ops = [wl._sym_block_op(rng, sizes), wl.SectorOperator(+1, [wl.OpCell(0, 1, 1, 2, 2, wl.CELL_IDENT, 0.75), wl.OpCell(1, 0, 2, 3, 3, wl.CELL_IDENT, 0.75)])]
    RT = [rng.standard_normal((m, sizes[q])) for q, m in zip(old_sector, kept)]
    return sizes, old_sector, kept, RT, ops


def _set_cell(o, i, **kw):
    def tweak(c):
        for k, v in kw.items():
            setattr(c.secops[o].cells[i], k, v)
    return tweak


def _swap_sectors(c):
    c.old_sector[0], c.old_sector[1] = 1, 0


def _set_kept(a, m):
    return lambda c: c.kept.__setitem__(a, m)


ROTATE_REFUSALS = {
    "old_sector_not_ascending": ("DMRGX_ERR_OUTOFRANGE", _swap_sectors),
    "kept_zero": ("DMRGX_ERR_ARG", _set_kept(1, 0)),
    "kept_above_size": ("DMRGX_ERR_ARG", _set_kept(1, 5)),
    "cell_rows_exceed_block": ("DMRGX_ERR_OUTOFRANGE", _set_cell(0, 1, r0=1)),
    "cell_columns_exceed_block": ("DMRGX_ERR_OUTOFRANGE", _set_cell(1, 1, c0=3)),
    "dense_ld_below_nc": ("DMRGX_ERR_ARG", _set_cell(0, 2, ld=4)),
    "dense_null_data": ("DMRGX_ERR_ARG", _set_cell(0, 0, data=None)),
    "transposed_operator": ("DMRGX_ERR_ARG", lambda c: setattr(c.secops[1], "transposed", 1)),
    "missing_destination_of_reachable_pair": ("DMRGX_ERR_ARG", lambda c: c.rows[1].__setitem__(0, None)),
    # the two below were accepted before: stage A copies nc columns of RT_a from r0 on, here columns 1 .. 3 of rows that have 3
    "identity_cell_not_square": ("DMRGX_ERR_ARG", _set_cell(1, 0, nr=2, nc=3)),
    "unknown_cell_kind": ("DMRGX_ERR_ARG", _set_cell(1, 1, kind=3)),
}


@pytest.mark.parametrize("what", list(ROTATE_REFUSALS))
def test_rotate_ops_refusals(mods, what):
    """Each malformed call returns the documented status with a message that names rotate_ops, before any device work: every destination
    is still NaN.  The undamaged call is accepted."""
    _, wl, capi = mods
    sizes, old_sector, kept, RT, ops = _refusal_case(wl)
    code, tweak = ROTATE_REFUSALS[what]
    status, out, where = _rotate(capi, sizes, old_sector, kept, RT, ops, 2, tweak)
    assert status == getattr(capi, code), (what, status)
    message = capi.lib().dmrgx_last_error().decode()
    assert message.startswith("rotate_ops"), (what, message)
    if what in ("identity_cell_not_square", "unknown_cell_kind"):                  # named like the neighbouring checks: operator and cell
        assert "op 1" in message and "cell %d" % (what == "unknown_cell_kind") in message, message
    assert len(where) == 5 and np.isnan(out).all()


def test_rotate_ops_refusal_case_is_accepted_undamaged(mods):
    _, wl, capi = mods
    sizes, old_sector, kept, RT, ops = _refusal_case(wl)
    _check_rotation(wl, capi, sizes, old_sector, kept, RT, ops, 2)
