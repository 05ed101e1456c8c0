"""The grouped GEMM (csrc/ggemm.hip) on its own, through dmrgx_ggemm_groups: whole groups -- product lists, scaled copies, accumulate --
at chosen tile shapes, and the launch regimes (unscheduled, scheduled one workgroup per entry, claiming) of both kernels with a tile
sequence that the test chooses.  Every group is compared element by element with a plain numpy float64 reference under the derived bound
of tests/helpers.py (ggemm_bound); operands sit in NaN buffers and outputs in a sentinel band that must come back bit for bit.
The checker itself is tested on the CPU (the tests without the gpu mark)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from helpers import SCALED_COPY as S
from helpers import GgemmInstance, ggemm_bound, ggemm_check, ggemm_reference, ggemm_violations

ERR_ARG = 62


# ---- the checker, on the CPU ----------------------------------------------------------------------------------------------------------
CHECKER_CASES = [(7, 5, [5], False), (16, 9, [17, 3, 33, 16], False), (9, 20, [S, S, 16], True), (12, 33, [S], False),
                 (6, 7, [12] * 26, True), (20, 18, [1, 1, 1, 1], False)]


def _checker_instances():
    rng = np.random.default_rng(2024)
    return [GgemmInstance(rng, M, N, prods, acc) for M, N, prods, acc in CHECKER_CASES]


def test_checker_float64_reference_is_within_half_the_bound_of_long_double():
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than float64 here: the comparison would say nothing"
    for inst in _checker_instances():
        R_ld, S_ld, n = ggemm_reference(inst, np.longdouble)
        assert n == inst.n and n == sum(p[1] if p[0] == 0 else 1 for p in inst.prods) + int(inst.accumulate)
        assert np.abs(S_ld - inst.S_abs).max() <= 1e-13 * np.abs(S_ld).max()
        err = np.abs(inst.R.astype(np.longdouble) - R_ld)
        assert (err <= 0.5 * ggemm_bound(inst.S_abs, inst.n)).all(), (inst.M, inst.N, inst.n, float(err.max()))
        assert (np.abs(inst.R) <= inst.S_abs).all() and (inst.S_abs >= 0.25 * inst.n).all()      # the magnitude rule


def test_checker_catches_a_dropped_a_doubled_and_a_misplaced_term_at_every_element():
    for inst in _checker_instances():
        assert ggemm_check(inst.R, inst) == 0.0 and not ggemm_violations(inst.R, inst.R, inst.S_abs, inst.n).any()
        terms = []                                                   # single terms of the sum, each M x N
        for kind, K, A, B, alpha in inst.prods:
            if kind == 1:
                terms.append(alpha * B.view)
            else:
                terms += [np.outer(A.view[:, k], B.view[k, :]) for k in sorted({0, K // 2, K - 1})]
        if inst.accumulate:
            terms.append(inst.C0)
        for t in terms:
            assert (np.abs(t) >= 0.25).all()
            for wrong in (inst.R - t, inst.R + t):                   # the term left out; the term added twice
                assert ggemm_violations(wrong, inst.R, inst.S_abs, inst.n).all()
                with pytest.raises(AssertionError):
                    ggemm_check(wrong, inst)
        # the values of the neighbouring tile position (16 columns / 4 rows away: an MFMA block, a lane group) and of the next column
        for shift, axis in ((16 % inst.N or 1, 1), (4 % inst.M or 1, 0), (1, 1)):
            assert ggemm_violations(np.roll(inst.R, shift, axis=axis), inst.R, inst.S_abs, inst.n).all()
        one = inst.R.copy()
        one[2, 3] = inst.R[2, 4]                                     # ONE element from the neighbouring position
        bad = ggemm_violations(one, inst.R, inst.S_abs, inst.n)
        assert bad[2, 3] and bad.sum() == 1
        with pytest.raises(AssertionError):
            ggemm_check(one, inst)
        one = inst.R.copy()
        one[0, 0] = np.nan
        assert ggemm_violations(one, inst.R, inst.S_abs, inst.n)[0, 0]


# ---- launching ------------------------------------------------------------------------------------------------------------------------
def expected_tiles(insts, tiling):
    """(128 x 128 tiles, 64 x 64 tiles) of the groups: cores of whole 128 x 128 blocks (tiling 0 only), the rest in 64 x 64."""
    big = sum((i.M // 128) * (i.N // 128) for i in insts) if tiling == 0 else 0
    return big, sum(-(-i.M // 64) * -(-i.N // 64) for i in insts) - 4 * big


def run_groups(pkg, insts, tiling, runs=1):
    """One dmrgx_ggemm_groups launch of the groups insts[0], insts[1], ... (an instance may appear many times: shared operands, an output
    of its own each time), `runs` times from the same initial memory.  Returns (outs, report): outs[r][g] is the M x N result of group g
    in run r.  All operands and outputs live in ONE device buffer; everything in it except the M x N outputs must come back bit for bit
    (operands, their NaN borders, the sentinel bands round the outputs)."""
    import torch
    capi = pkg._capi
    L = capi.lib()
    parts, size = [], 0

    def put(buf):
        nonlocal size
        off = size
        parts.append(buf.ravel())
        size += buf.size
        return off

    uniq = list({id(i): i for i in insts}.values())
    at = {}
    for inst in uniq:
        for _, _, A, B, _ in inst.prods:
            for op in (A, B):
                if op is not None:
                    at[id(op)] = put(op.buf)
    outs_at = []
    for inst in insts:
        buf, r0, c0 = inst.output_buffer()
        outs_at.append((put(buf), buf.shape[0], buf.shape[1], r0, c0))
    host = np.concatenate(parts)
    del parts
    dev = torch.from_numpy(host).cuda()
    base = dev.data_ptr()

    def ptr(op):
        return base + 8 * (at[id(op)] + op.first)

    P = capi.GgemmProd
    parr = (P * max(1, sum(len(i.prods) for i in uniq)))()
    first, k = {}, 0
    for inst in uniq:
        first[id(inst)] = k
        for kind, K, A, B, alpha in inst.prods:
            parr[k] = P(kind, K, ptr(A) if A is not None else None, A.ld if A is not None else 0, ptr(B), B.ld, alpha)
            k += 1
    garr = (capi.GgemmGroup * len(insts))()
    for g, (inst, (off, rows, ld, r0, c0)) in enumerate(zip(insts, outs_at)):
        plist = C.cast(C.byref(parr, first[id(inst)] * C.sizeof(P)), C.POINTER(P))
        garr[g] = capi.GgemmGroup(base + 8 * (off + r0 * ld + c0), ld, inst.M, inst.N, int(inst.accumulate), len(inst.prods), plist)
    results, rep = [], None
    for r in range(runs):
        if r:
            dev.copy_(torch.from_numpy(host))
        rep = capi.GgemmReport()
        assert L.dmrgx_ggemm_groups(len(insts), garr, tiling, C.byref(rep), None) == 0, L.dmrgx_last_error()
        got = dev.cpu().numpy()
        outs = []
        for inst, (off, rows, ld, r0, c0) in zip(insts, outs_at):
            win = got[off:off + rows * ld].reshape(rows, ld)[r0:r0 + inst.M, c0:c0 + inst.N]
            outs.append(win.copy())
            win[...] = host[off:off + rows * ld].reshape(rows, ld)[r0:r0 + inst.M, c0:c0 + inst.N]
        assert np.array_equal(got.view(np.uint64), host.view(np.uint64)), "memory outside the M x N outputs changed"
        results.append(outs)
    report = {k: getattr(rep, k) for k, _ in capi.GgemmReport._fields_}
    assert (report["tiles_big"], report["tiles_small"]) == expected_tiles(insts, tiling), report
    assert report["entries_big"] >= report["tiles_big"] and report["entries_small"] >= report["tiles_small"], report
    assert report["slots_big"] > 0 and report["slots_small"] > 0, report
    return results, report


def check_all(insts, outs, names):
    worst = 0.0
    for inst, got, name in zip(insts, outs, names):
        worst = max(worst, ggemm_check(got, inst, "%s (M=%d N=%d)" % (name, inst.M, inst.N)))
    print("worst |got - R| / bound over %d groups: %.3f" % (len(insts), worst))


def one_launch(pkg, seed, specs, tiling):
    """specs: (M, N, product list, accumulate); one launch, every group checked."""
    rng = np.random.default_rng(seed)
    insts = [GgemmInstance(rng, M, N, prods, acc) for M, N, prods, acc in specs]
    (outs,), rep = run_groups(pkg, insts, tiling)
    check_all(insts, outs, ["%s%s" % (s[2], " +=" if s[3] else "") for s in specs])
    return insts, outs, rep


SHAPES = [(64, 64, 1), (37, 29, 1), (128, 128, 0)]        # (M, N, tiling): a full 64 x 64 tile, an edge tile, a full 128 x 128 tile
K_LADDER = (1, 3, 4, 15, 16, 17, 31, 32, 33, 48, 49, 65, 80, 81)
K_LISTS = ([5], [5, 5, 5], [16, 1, 16], [1, 1, 1, 1], [17, 3, 33, 16], [15, 17], [32, 32], [12] * 26)


# ---- (a) K ladder, (b) product lists ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,tiling", SHAPES)
def test_k_ladder_one_product(pkg, M, N, tiling):
    """One product of 1 .. 6 k-steps with every K-edge width, the groups of one launch."""
    _, _, rep = one_launch(pkg, 101, [(M, N, [K], False) for K in K_LADDER], tiling)
    assert rep["tiles_big" if M == 128 else "tiles_small"] == len(K_LADDER)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,tiling", SHAPES)
def test_product_lists(pkg, M, N, tiling):
    """Several products in one software-pipelined stream (the K edge in mid-stream; 26 x K = 12: the MatMult's stage 2), every product
    with leading dimensions of its own."""
    insts, _, rep = one_launch(pkg, 102, [(M, N, ks, False) for ks in K_LISTS], tiling)
    assert rep["tiles_big" if M == 128 else "tiles_small"] == len(K_LISTS)
    lds = [(A.ld - K, B.ld - N) for i in insts for _, K, A, B, _ in i.prods]
    assert len(set(lds)) >= 8 and all(a > 0 and b > 0 for a, b in lds)


# ---- (c) scaled copies, (d) accumulate -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,tiling", [(64, 64, 1), (37, 29, 1), (64, 20, 1), (128, 128, 0), (256, 128, 0)])
def test_scaled_copies(pkg, M, N, tiling):
    """1, 2, 3, 5 scaled copies alone and in front of product lists: the pipelined staging-register path (full 64 x 64 tile), the generic
    path (edge tiles) and the 128 x 128 kernel; a group without any product writes zeros, or leaves C when accumulating."""
    specs = [(M, N, [S] * c + tail, False) for c in (1, 2, 3, 5) for tail in ([], [16], [5], [17, 3, 33])]
    specs += [(M, N, [], False), (M, N, [], True), (M, N, [16, S, 3, S], False)]      # (the last: the host moves the copies to the front)
    insts, outs, rep = one_launch(pkg, 103, specs, tiling)
    assert (rep["tiles_big"] > 0) == (tiling == 0) and (rep["tiles_small"] > 0) == (tiling == 1)
    assert not outs[-3].any() and np.array_equal(outs[-2], insts[-2].C0)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,tiling", [(64, 64, 1), (128, 128, 0), (37, 29, 1), (20, 64, 1), (193, 129, 0)])
def test_accumulate(pkg, M, N, tiling):
    """C += on full tiles of both kernels and on edge tiles, with and without scaled copies; C0 follows the magnitude rule."""
    lists = ([16], [5], [17, 3, 33], [80], [S, 16], [S, S, 17, 3], [S, S, S], [1])
    one_launch(pkg, 104, [(M, N, ks, True) for ks in lists] + [(M, N, [33], False)], tiling)


# ---- (e) tile geometry -----------------------------------------------------------------------------------------------------------------
EDGES = (1, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64, 65, 97, 127, 128, 129, 193, 257)


@pytest.mark.gpu
def test_tile_geometry_mixed_tiling(pkg):
    """Every (M, N) of EDGES x EDGES in one launch of the mixed tiling: both re-layouts of thin tiles, every 16-granular block guard, the
    seam between a 128 x 128 core and the 64 x 64 strips round it."""
    _, _, rep = one_launch(pkg, 105, [(M, N, [19], False) for M in EDGES for N in EDGES], 0)
    assert rep["tiles_big"] > 0 and rep["tiles_small"] > 0


@pytest.mark.gpu
def test_tile_geometry_64_only(pkg):
    _, _, rep = one_launch(pkg, 106, [(193, 129, [19], False), (257, 257, [19], False)], 1)
    assert rep["tiles_big"] == 0 and rep["tiles_small"] == 4 * 3 + 5 * 5


# ---- (f), (g) launch regimes -----------------------------------------------------------------------------------------------------------
def cycle_until(insts, tiling, ntiles, not_multiple_of=0):
    """insts[0], insts[1], ... round and round until the launch has at least `ntiles` tiles (of either size)."""
    out, n = [], 0
    for inst in itertools.cycle(insts):
        if n >= ntiles and (not not_multiple_of or n % not_multiple_of):
            return out
        out.append(inst)
        n += sum(expected_tiles([inst], tiling))


def check_regime_launch(pkg, insts, tiling, small_outs, catalogue, runs=1):
    """Every group within the bound, and bit-identical to the same group in the small launch; several runs bit-identical."""
    res, rep = run_groups(pkg, insts, tiling, runs)
    check_all(insts, res[0], ["catalogue entry %d" % catalogue.index(i) for i in insts])
    ref = {id(i): o for i, o in zip(catalogue, small_outs)}
    for g, (inst, got) in enumerate(zip(insts, res[0])):
        assert np.array_equal(got, ref[id(inst)]), "group %d (catalogue entry %d) differs from the same group in the small launch" % (g, catalogue.index(inst))
        for other in res[1:]:
            assert np.array_equal(got, other[g]), "group %d differs between two runs" % g
    return rep


@pytest.mark.gpu
def test_launch_regimes_64(pkg):
    """The three launch regimes of the 64 x 64 kernel over one-tile groups cycling through a fixed catalogue (two sets of operands of
    each entry): at most slots / 4 tiles (unscheduled), up to slots (scheduled and padded, one workgroup per entry), 3 x slots (claiming:
    a workgroup meets full, thin, copy-only, empty and accumulating tiles in the scheduler's order)."""
    rng = np.random.default_rng(107)
    entries = [(64, 64, [80], False), (64, 64, [5], False), (64, 64, [S, S, 17, 3], False), (64, 64, [S, S, S], False), (64, 64, [], False),
               (37, 29, [16, 1, 16], False), (20, 64, [33], False), (64, 20, [17], True), (64, 64, [48], True)]
    catalogue = [GgemmInstance(rng, M, N, ks, acc) for _ in range(2) for M, N, ks, acc in entries]
    (small,), rep = run_groups(pkg, catalogue, 1)
    check_all(catalogue, small, ["catalogue entry %d" % i for i in range(len(catalogue))])
    slots = rep["slots_small"]
    assert rep["tiles_small"] == len(catalogue) <= slots // 4 and rep["entries_small"] == rep["tiles_small"], rep
    # scheduled: eight per-XCD queues padded to one length with group = -1 entries, still one workgroup per entry
    rep = check_regime_launch(pkg, cycle_until(catalogue, 1, slots // 2 + 3, 8), 1, small, catalogue)
    assert slots // 4 < rep["tiles_small"] < rep["entries_small"] <= slots and rep["entries_small"] % 8 == 0, rep
    # claiming
    rep = check_regime_launch(pkg, cycle_until(catalogue, 1, 3 * slots + 5), 1, small, catalogue, runs=2)
    assert rep["tiles_small"] >= 3 * slots and rep["entries_small"] > rep["slots_small"], rep


@pytest.mark.gpu
def test_claiming_128(pkg):
    """The 128 x 128 kernel with more macro tiles than resident workgroups (late claim, prefetch beside the epilogue), with product
    lists, scaled copies and accumulate."""
    rng = np.random.default_rng(108)
    entries = [([80], False), ([16], False), ([5], False), ([17, 3, 33], False), ([S, S, 16], False), ([S, S], False), ([33], True)]
    catalogue = [GgemmInstance(rng, m, m, ks, acc, tight=True) for m in (128, 256) for ks, acc in entries]
    (small,), rep = run_groups(pkg, catalogue, 0)
    check_all(catalogue, small, ["catalogue entry %d" % i for i in range(len(catalogue))])
    slots = rep["slots_big"]
    assert rep["tiles_small"] == 0 and rep["tiles_big"] <= slots // 4 and rep["entries_big"] == rep["tiles_big"], rep
    rep = check_regime_launch(pkg, cycle_until(catalogue, 0, 3 * slots), 0, small, catalogue, runs=2)
    assert rep["tiles_small"] == 0 and rep["tiles_big"] >= 3 * slots and rep["entries_big"] > rep["slots_big"], rep


# ---- (h) refusals (no device is touched by a refused call) ----------------------------------------------------------------------------
def test_ggemm_groups_refuses_bad_arguments(pkg):
    capi = pkg._capi
    L = capi.lib()
    P, G = capi.GgemmProd, capi.GgemmGroup
    p = 1 << 20                                  # stands for a device pointer: a refused call reads none

    def status(group=None, prods=None, count=1, tiling=0, null_groups=False, null_prods=False):
        pr = dict(kind=0, K=16, A=p, lda=16, B=p, ldb=40, alpha=1.0)
        parr = (P * 2)(P(1, 0, None, 0, p, 40, 0.5), P(**dict(pr, **(prods or {}))))
        gr = dict(C=p, ldc=40, M=30, N=40, accumulate=0, nprods=2, prods=None if null_prods else C.cast(parr, C.POINTER(P)))
        garr = (G * 1)(G(**dict(gr, **(group or {}))))
        return L.dmrgx_ggemm_groups(count, None if null_groups else garr, tiling, None, None)

    assert status(count=-1) == ERR_ARG and status(null_groups=True) == ERR_ARG
    assert status(tiling=2) == ERR_ARG and status(tiling=-1) == ERR_ARG
    for bad in (dict(M=-1), dict(N=-1), dict(nprods=-1), dict(C=None), dict(ldc=39), dict(ldc=1 << 31)):
        assert status(group=bad) == ERR_ARG, bad
    assert status(null_prods=True) == ERR_ARG
    for bad in (dict(kind=2), dict(kind=-1), dict(K=-1), dict(A=None), dict(B=None), dict(lda=15), dict(ldb=39), dict(lda=1 << 31),
                dict(kind=1, B=None), dict(kind=1, ldb=39)):
        assert status(prods=bad) == ERR_ARG, bad
    assert b"ggemm_groups" in L.dmrgx_last_error()
    rep = capi.GgemmReport()
    assert L.dmrgx_ggemm_groups(0, None, 0, C.byref(rep), None) == 0                    # nothing to do is no error
    assert rep.tiles_big == 0 and rep.tiles_small == 0 and rep.slots_small == 2 * rep.slots_big > 0
