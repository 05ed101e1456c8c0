"""Kernels on NaN-poisoned device workspaces (-m gpu).

The MatMult arena, the eigensolver vectors and the density-matrix / rotation / tridiagonalisation workspaces are not zeroed: every
location is written before it is read (csrc/kron_plan.hip, csrc/eigs.hip).  Fresh device memory is usually zero, so a missing write
would read the right answer for a pad or an unreached segment and no parity test would notice.  With DMRGX_POOL_POISON=1 every
f64-only block is handed out filled with a quiet NaN (csrc/pool.hip), fresh or recycled: a read before a write turns into a NaN
in the result.  The switch is read once per process, so the poisoned runs are child processes.

The planted-layout tests below build superblocks whose plans reach the paths that rely on that contract -- zero rectangles of the
intermediates, stage-2 rows without products, identity cells across a stripe's panel border, split-K slabs -- prove from
DMRGX_PLAN_DUMP that the plan reached them, and compare with the dense Kronecker product; they run clean here and poisoned in
test_parity_suite_on_poisoned_workspaces.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_kron import _apply, _dense_operator

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON_BITS = 0x7ff8badbadbadbad
OpSz = 0


@pytest.fixture(scope="module")
def mods(pkg):
    from dmrgx_amd import superblock, workloads, _capi
    _capi.require_device()
    return superblock, workloads, _capi


def _child(args, poison, timeout):
    env = dict(os.environ)
    env.pop("DMRGX_POOL_POISON", None)
    if poison:
        env["DMRGX_POOL_POISON"] = "1"
    python = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    return subprocess.run(python + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


# ---- planted layouts --------------------------------------------------------------------------------------------------------------
def _dense_H(sb):
    """The superblock Hamiltonian restricted to the target KronBlocks, from the dense Kronecker products of the sector operators
    (shift-0 terms only: A (x) B with A, B the dense operators)."""
    lsz, rsz = sb.left_sizes, sb.right_sizes
    nl, nr = sum(lsz), sum(rsz)
    full = np.zeros((nl * nr, nl * nr))
    if sb.h_left is not None:
        full += np.kron(_dense_operator(sb.h_left, lsz), np.eye(nr))
    if sb.h_right is not None:
        full += np.kron(np.eye(nl), _dense_operator(sb.h_right, rsz))
    for (a, io, isite, jo, jsite) in sb.terms:
        assert io == OpSz and jo == OpSz
        full += a * np.kron(_dense_operator(sb.left_ops[(io, isite)], lsz), _dense_operator(sb.right_ops[(jo, jsite)], rsz))
    loff, roff = np.concatenate([[0], np.cumsum(lsz)]), np.concatenate([[0], np.cumsum(rsz)])
    idx = [(loff[il] + i) * nr + roff[ir] + j for il, ir in sb.blocks for i in range(lsz[il]) for j in range(rsz[ir])]
    return full[np.ix_(idx, idx)]


def _plan_dump(sbm, sb, path, monkeypatch, **kw):
    """KronPlan built with DMRGX_PLAN_DUMP set -> (plan, {line kind: [int tuples]})."""
    monkeypatch.setenv("DMRGX_PLAN_DUMP", str(path))
    try:
        plan = sbm.KronPlan(sb, **kw)
    finally:
        monkeypatch.delenv("DMRGX_PLAN_DUMP")
    rows = {}
    for line in open(path):
        f = line.split()
        rows.setdefault(f[0], []).append(tuple(int(v) for v in f[1:]))
    return plan, rows


def _groups(rows, *kinds):
    """{group id: (M, N, products)} of the scheduled tiles of the given lists (s1, s1b, s2, s2b)."""
    out = {}
    for kind in kinds:
        for (_, g, _tm, _tn, M, N, _ks, npr) in rows.get(kind, []):
            if g >= 0:
                out[g] = (M, N, npr)
    return out


def _striped_apply(plans, x):
    info = plans[0].info
    xs = torch.zeros(info.vec_len, dtype=torch.float64, device="cuda")
    plans[0].to_striped(torch.from_numpy(x).cuda(), xs)
    ys = torch.full_like(xs, float("nan"))
    for p in plans:
        p.apply(xs, ys[p.info.local_offset:p.info.local_offset + p.info.local_len])
    yd = torch.full((len(x),), float("nan"), dtype=torch.float64, device="cuda")
    plans[0].from_striped(ys, yd)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def _check(y, want):
    assert np.isfinite(y).all()
    assert np.abs(y - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), np.abs(y - want).max()


def _sym(rng, n):
    a = rng.standard_normal((n, n))
    return 0.5 * (a + a.T)


def test_planted_zero_rectangles_and_rows_without_products(mods, tmp_path, monkeypatch):
    """(a) Right-operator cells that leave columns of a sector unreached: those column segments of the intermediates T_{g,k} and T_R,k
    are zero rectangles (the only zeroed part of the arena).  (b) No H_L / H_R at all (NULL in the descriptor) and left cells that cover
    only some rows of a sector: stage-2 row segments with no product, whose rows of y must be written as zeros."""
    sbm, wl, _ = mods
    from dmrgx_amd.workloads import OpCell, SectorOperator, Superblock, CELL_DENSE
    rng = np.random.default_rng(7)
    lsz, rsz = [3, 4], [5, 6]
    qn = [0.5, -0.5]
    blocks = [(0, 1), (1, 0)]

    def dense(q, r0, c0, nr, nc):
        return OpCell(q, r0, c0, nr, nc, CELL_DENSE, 0.0, rng.standard_normal((nr, nc)))

    def full_left():
        return SectorOperator(0, [dense(q, 0, 0, lsz[q], lsz[q]) for q in range(2)])

    # right cells: rows [1, 4) of sector 0 (rows 0 and 4 unreached), rows [0, 3) of sector 1; a second operator reaches other rows
    right0 = SectorOperator(0, [dense(0, 1, 0, 3, 5), dense(1, 0, 0, 3, 6)])
    right1 = SectorOperator(0, [dense(0, 0, 0, 2, 5), dense(1, 4, 0, 2, 6)])
    h_right = SectorOperator(0, [dense(0, 2, 0, 2, 5)])                   # reaches columns 2, 3 of T_R of sector 0 only
    h_left = SectorOperator(0, [OpCell(q, 0, 0, lsz[q], lsz[q], CELL_DENSE, 0.0, _sym(rng, lsz[q])) for q in range(2)])
    terms = [(0.9, OpSz, 0, OpSz, 0), (-0.6, OpSz, 1, OpSz, 1)]
    sb = Superblock("zero_rects", lsz, rsz, qn, qn, blocks, {(OpSz, 0): full_left(), (OpSz, 1): full_left()},
                    {(OpSz, 0): right0, (OpSz, 1): right1}, h_left, h_right, terms, 2, 2)
    plan, rows = _plan_dump(sbm, sb, tmp_path / "a.txt", monkeypatch)
    assert len(rows.get("zr", [])) >= 6, rows.get("zr")                  # gaps of T_{g,k} of both operators and of T_R,k
    H = _dense_H(sb)
    for _ in range(2):
        x = rng.standard_normal(sb.n_states)
        _check(_apply(plan, x), H @ x)
    plan.destroy()

    # (b) no H_L, no H_R; left cells: row 0 of sector 0 and rows [2, 4) of sector 1 (rows 1, 2 of sector 0 and 0, 1 of sector 1: nothing)
    left = SectorOperator(0, [dense(0, 0, 0, 1, 3), dense(1, 2, 0, 2, 4)])
    right = SectorOperator(0, [dense(q, 0, 0, rsz[q], rsz[q]) for q in range(2)])
    sb2 = Superblock("empty_rows", lsz, rsz, qn, qn, blocks, {(OpSz, 0): left}, {(OpSz, 0): right}, None, None, [(1.1, OpSz, 0, OpSz, 0)], 2, 2)
    plan, rows = _plan_dump(sbm, sb2, tmp_path / "b.txt", monkeypatch)
    groups2 = _groups(rows, "s2", "s2b")
    assert sum(npr == 0 for (_, _, npr) in groups2.values()) >= 2, groups2    # a row segment without products in each KronBlock
    H = _dense_H(sb2)
    assert not H.any(axis=1).all()                                          # (the reference has all-zero rows there)
    for _ in range(2):
        x = rng.standard_normal(sb2.n_states)
        _check(_apply(plan, x), H @ x)
    plan.destroy()


@pytest.mark.parametrize("W", [2, 3])
def test_planted_identity_cells_across_panel_borders(mods, tmp_path, monkeypatch, W):
    """Identity cells of the right operator whose source columns cross the border of a source panel (another rank's stripe): stage 1
    reads ONE panel per scaled copy, so the output segment is cut where the source crosses the border.  The dump shows the extra
    segments on each rank; the gathered stripes equal the dense Kronecker product."""
    sbm, wl, _ = mods
    from dmrgx_amd.workloads import OpCell, SectorOperator, Superblock, CELL_DENSE, CELL_IDENT
    rng = np.random.default_rng(11 + W)
    lsz, rsz = [4], [10]
    # cell 1: rows [0, 6) <- columns [2, 8); cell 2: rows [4, 10) <- columns [0, 6).  In the transposed storage of stage 1 the rows are
    # the output columns of T and the columns the source columns of X.
    right = SectorOperator(0, [OpCell(0, 0, 2, 6, 6, CELL_IDENT, 0.7), OpCell(0, 4, 0, 6, 6, CELL_IDENT, -1.3)])
    left = SectorOperator(0, [OpCell(0, 0, 0, 4, 4, CELL_DENSE, 0.0, rng.standard_normal((4, 4)))])
    h_left = SectorOperator(0, [OpCell(0, 0, 0, 4, 4, CELL_DENSE, 0.0, _sym(rng, 4))])
    h_right = SectorOperator(0, [OpCell(0, 0, 0, 10, 10, CELL_DENSE, 0.0, _sym(rng, 10))])
    sb = Superblock("ident_panels", lsz, rsz, [0.0], [0.0], [(0, 0)], {(OpSz, 0): left}, {(OpSz, 0): right}, h_left, h_right,
                    [(0.8, OpSz, 0, OpSz, 0)], 2, 2)
    # sorted widths of the stage-1 column segments per rank (the T_R segment is the whole stripe).  Without the panel cuts they would
    # be W = 2: [1, 4, 5] | [1, 4, 5];  W = 3: [3, 3] | [1, 2, 3] | [4, 4]
    want = {2: [[1, 1, 3, 5], [1, 1, 3, 5]], 3: [[1, 2, 3], [1, 2, 3], [1, 3, 4]]}[W]
    plans = []
    for r in range(W):
        p, rows = _plan_dump(sbm, sb, tmp_path / ("w%d_r%d.txt" % (W, r)), monkeypatch, world_size=W, rank=r)
        plans.append(p)
        assert sorted(N for (M, N, _) in _groups(rows, "s1", "s1b").values()) == want[r], (r, _groups(rows, "s1", "s1b"))
    H = _dense_H(sb)
    for _ in range(2):
        x = rng.standard_normal(sb.n_states)
        _check(_striped_apply(plans, x), H @ x)
    for p in plans:
        p.destroy()


def test_planted_split_k_segments(mods, tmp_path, monkeypatch):
    """A small superblock whose stage-2 groups have long product lists: they are cut into >= 3 split-K segments; segment 0 writes y,
    the others write slabs of the arena that slab_reduce_kernel adds in a fixed order."""
    sbm, wl, _ = mods
    from dmrgx_amd.workloads import OpCell, SectorOperator, Superblock, CELL_DENSE
    rng = np.random.default_rng(3)
    lsz, rsz = [96, 80], [8, 12]
    blocks = [(0, 1), (1, 0)]
    qn = [0.5, -0.5]

    def op(sizes, scale=1.0):
        return SectorOperator(0, [OpCell(q, 0, 0, n, n, CELL_DENSE, 0.0, scale * rng.standard_normal((n, n))) for q, n in enumerate(sizes)])

    nt = 5
    terms = [(0.3 + 0.1 * i, OpSz, i, OpSz, i) for i in range(nt)]
    h_left = SectorOperator(0, [OpCell(q, 0, 0, n, n, CELL_DENSE, 0.0, _sym(rng, n)) for q, n in enumerate(lsz)])
    sb = Superblock("split_k", lsz, rsz, qn, qn, blocks, {(OpSz, i): op(lsz, 0.1) for i in range(nt)}, {(OpSz, i): op(rsz) for i in range(nt)},
                    h_left, None, terms, 2, 2)
    plan, rows = _plan_dump(sbm, sb, tmp_path / "k.txt", monkeypatch)
    red = rows.get("red", [])
    assert red and max(r[6] for r in red) >= 2, red                      # nslab = split-K segments - 1
    H = _dense_H(sb)
    for _ in range(2):
        x = rng.standard_normal(sb.n_states)
        y = _apply(plan, x)
        _check(y, H @ x)
    assert np.array_equal(_apply(plan, x), y)                              # fixed-order reduction: repeatable bit for bit
    plan.destroy()


def test_plan_with_more_than_70000_zero_rectangles(mods, tmp_path, monkeypatch):
    """80 000 unreached column segments spread over 40 operator groups x 100 KronBlocks (right cells that reach every other column):
    more zero rectangles than a launch grid holds in y.  The plan builds and its apply matches the factored CPU statement."""
    sbm, wl, _ = mods
    from dmrgx_amd.workloads import OpCell, SectorOperator, Superblock, CELL_DENSE
    rng = np.random.default_rng(70000)
    ns, nl, nr, nops = 10, 2, 40, 40
    lsz, rsz = [nl] * ns, [nr] * ns
    qn = [0.5 * (ns - 1) - q for q in range(ns)]
    blocks = [(a, b) for a in range(ns) for b in range(ns)]
    left = {(OpSz, i): SectorOperator(0, [OpCell(q, 0, 0, nl, nl, CELL_DENSE, 0.0, rng.standard_normal((nl, nl))) for q in range(ns)])
            for i in range(nops)}
    right = {(OpSz, i): SectorOperator(0, [OpCell(q, 2 * j, 0, 1, nr, CELL_DENSE, 0.0, rng.standard_normal((1, nr)))
                                           for q in range(ns) for j in range(nr // 2)])
             for i in range(nops)}
    hl = SectorOperator(0, [OpCell(q, 0, 0, nl, nl, CELL_DENSE, 0.0, _sym(rng, nl)) for q in range(ns)])
    hr = SectorOperator(0, [OpCell(q, 0, 0, nr, nr, CELL_DENSE, 0.0, _sym(rng, nr)) for q in range(ns)])
    terms = [(float(rng.uniform(-1, 1)), OpSz, i, OpSz, i) for i in range(nops)]
    sb = Superblock("many_zero_rects", lsz, rsz, qn, qn, blocks, left, right, hl, hr, terms, 2, 2)
    plan, rows = _plan_dump(sbm, sb, tmp_path / "z.txt", monkeypatch)
    zr = rows.get("zr", [])
    assert len(zr) == nops * len(blocks) * (nr // 2) and len(zr) > 70000, len(zr)
    assert all(nrows == nl and ncols == 1 for (_, _, _, nrows, ncols) in zr)
    x = rng.standard_normal(sb.n_states)
    y = _apply(plan, x)
    want = wl.apply_factored_numpy(sb, x)
    assert np.isfinite(y).all() and np.abs(y - want).max() <= 1e-13 * np.abs(want).max()
    plan.destroy()


def test_generalized_davidson_odd_and_even_sizes(mods):
    """The Davidson work vectors are padded to an even length and the pads are zeroed only where nothing else writes them: an odd and an
    even number of states against the dense solve, default and smallest search space."""
    sbm, wl, _ = mods
    kept = {0.5: 7, -0.5: 6, 1.5: 3, -1.5: 2}
    sizes = []
    for kw in (dict(m=32, Ly=2, seed=3), dict(Ly=2, seed=3, kept=(kept, kept))):
        sb = wl.synthetic_superblock("cfg2", **kw)
        n = sb.n_states
        sizes.append(n)
        H = np.stack([wl.apply_factored_numpy(sb, e) for e in np.eye(n)], axis=1)
        w, v = np.linalg.eigh(H)
        plan = sbm.KronPlan(sb)
        for ncv in (0, 3):
            psi0 = torch.from_numpy(np.random.default_rng(ncv).standard_normal(n)).cuda()
            e0, psi, stats = plan.eigs_lowest(tol=1e-12, method=1, psi0=psi0, ncv=ncv)
            assert stats.converged == 1 and abs(e0 - w[0]) <= 1e-10 * abs(w[0])
            assert abs(abs(float(psi.cpu().numpy() @ v[:, 0])) - 1.0) < 1e-8
        plan.destroy()
    assert sizes[0] % 2 == 0 and sizes[1] % 2 == 1, sizes


# ---- verification of the density-matrix eigenpairs; lifetime of psi ----------------------------------------------------------------
def test_rdm_verification_catches_a_changed_state(mods):
    """dmrgx_rdm_destroy compares the direct solver's kept eigenvalues with the Rayleigh quotients of its eigenvectors, which
    dmrgx_rdm_select forms from psi.  Scaling one KronBlock's slice of psi in between makes them disagree: the verification must fail
    with DMRGX_ERR_NOTCONV (a disabled check would let a wrong eigenpair through)."""
    sbm, _, capi = mods
    rng = np.random.default_rng(31)
    ls, rs = [90, 40], [60, 70]
    psi = rng.standard_normal(90 * 60 + 40 * 70)
    psi /= np.linalg.norm(psi)
    d = torch.from_numpy(psi).cuda()
    rdm = sbm.ReducedDensityMatrices(ls, rs, [(0, 0), (1, 1)], d)
    d[:90 * 60] *= 1.5
    rdm.select([20, 20, 10, 10])
    with pytest.raises(capi.DmrgxError) as e:
        rdm.destroy()
    assert e.value.code == capi.DMRGX_ERR_NOTCONV, str(e.value)
    # the same calls on the unchanged state pass the verification
    rdm = sbm.ReducedDensityMatrices(ls, rs, [(0, 0), (1, 1)], torch.from_numpy(psi).cuda())
    rdm.select([20, 20, 10, 10])
    rdm.destroy()


def test_rdm_keeps_a_temporary_state_alive(mods):
    """ReducedDensityMatrices built from a temporary psi: the library reads psi again when it forms the eigenvectors, so the wrapper
    holds it until then -- allocations in between must not take its memory."""
    sbm, _, _ = mods
    rng = np.random.default_rng(32)
    ls, rs = [150, 60], [120, 90]
    n = 150 * 120 + 60 * 90
    psi = rng.standard_normal(n)
    psi /= np.linalg.norm(psi)
    rdm = sbm.ReducedDensityMatrices(ls, rs, [(0, 0), (1, 1)], torch.from_numpy(psi).cuda())
    junk = [torch.full((n,), 1e3, dtype=torch.float64, device="cuda") for _ in range(4)]      # would take a released psi block
    counts = [40, 40, 30, 30]
    rdm.select(counts)
    off = 0
    for k, (a, b) in enumerate([(150, 120), (60, 90)]):
        Psi = psi[off:off + a * b].reshape(a, b)
        off += a * b
        for side, rho in ((0, Psi @ Psi.T), (1, Psi.T @ Psi)):
            c = counts[2 * k + side]
            w = rdm.eigenvalues(side, k)
            U = rdm.eigenvectors(side, k, c).cpu().numpy()
            assert np.abs(U @ rho @ U.T - np.diag(w[:c])).max() < 1e-11 * np.linalg.norm(rho) + 1e-16
    rdm.destroy()                                                            # the Rayleigh-quotient verification passes
    del junk


# ---- the pool switch itself, the parity suite poisoned, bit-identity across processes ------------------------------------------------
def test_poison_switch_fills_fresh_and_recycled_blocks():
    """DMRGX_POOL_POISON=1: a block from dmrgx_malloc reads back as the poison pattern, fresh and after it went back to the pool holding
    other values; without the switch the recycled block still holds what was written into it (no fill)."""
    code = ("import sys, ctypes as C, numpy as np; sys.path.insert(0, %r)\n"
            "from __graft_entry__ import load_package; pkg = load_package(); L = pkg._capi.lib()\n"
            "n = 1 << 16; p = C.c_void_p(); out = []\n"
            "for i in range(2):\n"
            "    assert L.dmrgx_malloc(C.byref(p), n * 8) == 0\n"
            "    h = np.zeros(n, dtype=np.uint64); assert L.dmrgx_memcpy_d2h(h.ctypes.data, p, n * 8, None) == 0; out.append(h)\n"
            "    v = np.arange(n, dtype=np.float64); assert L.dmrgx_memcpy_h2d(p, v.ctypes.data, n * 8, None) == 0\n"
            "    assert L.dmrgx_stream_sync(None) == 0 and L.dmrgx_free(p) == 0\n"
            "print('POISON', int((out[0] == %d).all()), int((out[1] == %d).all()), int((out[1].view(np.float64) == np.arange(n)).all()))"
            ) % (ROOT, POISON_BITS, POISON_BITS)
    for poison, want in ((True, "POISON 1 1 0"), (False, "POISON 0 0 1")):
        p = _child(["-c", code], poison, 300)
        assert p.returncode == 0 and want in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


POISONED_NODES = [
    "tests/test_gpu_kron.py::test_dgemm_batch_matches_numpy",
    "tests/test_gpu_kron.py::test_apply_matches_reference_row_loop",
    "tests/test_gpu_kron.py::test_apply_degenerate_layouts_vs_dense_kron",
    "tests/test_gpu_kron.py::test_striped_plans_reassemble_full_apply",
    "tests/test_gpu_kron.py::test_apply_when_one_side_has_fewer_distinct_operators",
    "tests/test_gpu_kron.py::test_kron_diag_matches_dense_diagonal",
    "tests/test_gpu_kron.py::test_eigs_lowest_vs_dense",
    "tests/test_gpu_kron.py::test_eigs_generalized_davidson_vs_dense_and_lanczos",
    "tests/test_gpu_kron.py::test_eigs_tiny_problem_smaller_than_ncv",
    "tests/test_gpu_kron.py::test_rdm_spectra_and_eigenvectors_vs_lapack",
    "tests/test_gpu_kron.py::test_rdm_direct_solver_degenerate_and_boundary_cases",
    "tests/test_gpu_kron.py::test_rdm_direct_solver_large_orders",
    "tests/test_gpu_kron.py::test_rdm_select_forms_only_the_kept_eigenvectors",
    "tests/test_gpu_kron.py::test_rdm_alternative_paths_stay_correct",
    "tests/test_gpu_kron.py::test_rdm_subset_matches_full_solve_and_refuses_unselected",
    "tests/test_gpu_kron.py::test_rdm_graded_spectrum_few_sweeps_and_warm_hints",
    "tests/test_gpu_kron.py::test_rotate_ops_vs_numpy",
    "tests/test_gpu_kron.py::test_cells_axpy_vs_numpy",
    "tests/test_gpu_kron.py::test_device_dot_product",
    "tests/test_gpu_kron.py::test_dot2d_batch_matches_numpy",
    "tests/test_gpu_engine.py::test_two_rank_eigensolve_on_one_gpu",
    "tests/test_gpu_poison.py::test_planted_zero_rectangles_and_rows_without_products",
    "tests/test_gpu_poison.py::test_planted_identity_cells_across_panel_borders",
    "tests/test_gpu_poison.py::test_planted_split_k_segments",
    "tests/test_gpu_poison.py::test_plan_with_more_than_70000_zero_rectangles",
    "tests/test_gpu_poison.py::test_generalized_davidson_odd_and_even_sizes",
    "tests/test_gpu_poison.py::test_rdm_verification_catches_a_changed_state",
    "tests/test_gpu_poison.py::test_rdm_keeps_a_temporary_state_alive",
    "tests/test_gpu_ggemm.py::test_k_ladder_one_product",
    "tests/test_gpu_ggemm.py::test_product_lists",
    "tests/test_gpu_ggemm.py::test_scaled_copies",
    "tests/test_gpu_ggemm.py::test_accumulate",
    "tests/test_gpu_ggemm.py::test_tile_geometry_mixed_tiling",
    "tests/test_gpu_ggemm.py::test_tile_geometry_64_only",
    "tests/test_gpu_ggemm.py::test_launch_regimes_64",
    "tests/test_gpu_ggemm.py::test_claiming_128",
    # rotation workspaces (UT, W of dmrgx_rotate_ops) are fully written before they are read
    "tests/test_gpu_rotate.py::test_cells_axpy_shape_ladder",
    "tests/test_gpu_rotate.py::test_cells_axpy_identity_source",
    "tests/test_gpu_rotate.py::test_cells_axpy_submission_order_by_bits",
    "tests/test_gpu_rotate.py::test_cells_axpy_many_overlapping_tasks",
    "tests/test_gpu_rotate.py::test_rotate_ops_enlarged_block_structure",
    "tests/test_gpu_rotate.py::test_rotate_ops_exact_rotation",
    "tests/test_gpu_rotate.py::test_rotate_ops_size_edges",
    "tests/test_gpu_rotate.py::test_rotate_ops_truncation_patterns",
    "tests/test_gpu_rotate.py::test_rotate_ops_refusal_case_is_accepted_undamaged",
    # general descriptors, element-wise bound: every case, named and drawn, and the patched-table cache
    "tests/test_gpu_kron_general.py::test_apply",
    "tests/test_gpu_kron_general.py::test_gathered_apply",
    "tests/test_gpu_kron_general.py::test_fold_switch",
    "tests/test_gpu_kron_general.py::test_diagonal",
    "tests/test_gpu_kron_general.py::test_repeatability",
    "tests/test_gpu_kron_general.py::test_patched_table_cache_past_its_capacity",
]


def test_parity_suite_on_poisoned_workspaces():
    """The kernel parity tests with every f64 workspace NaN-poisoned, in one child process: their assertions, unchanged, now also show
    that nothing is read before it is written."""
    p = _child(["-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", *POISONED_NODES], True, 480)
    tail = p.stdout[-3000:] + p.stderr[-2000:]
    assert p.returncode == 0, tail
    assert " passed" in tail and " failed" not in tail and " skipped" not in tail, tail


def test_outputs_are_bit_identical_on_poisoned_workspaces(tmp_path):
    """Full-size dmrgx_kron_apply (cfg4real, cfg5) in a clean and in a poisoned process: bit-identical (the apply repeats bit for bit).
    Lanczos, generalized Davidson (odd and even sizes), the density-matrix spectra and eigenvectors and the gathered applies of two
    multi-rank plans (W = 3 and W = 2, both branches of stripe_cut), the other branches of the eigensolver at 845 states (the worker's
    solver_paths group: rejected and accepted start vectors, truncated cycles, an exhausted solve, unfused Davidson and its hand-over to
    Lanczos), and the device-resident Krylov calls with dmrgx_dot at 845 and 4097 states (the worker's krylov group): two clean
    processes agree bit for bit, and so must the poisoned one."""
    worker = os.path.join("tests", "bitwise_worker.py")
    res = {}
    groups = "solvers,solver_paths,striped,krylov"
    for tag, poison, what in (("clean", False, "apply," + groups), ("clean2", False, groups), ("poison", True, "apply," + groups)):
        path = str(tmp_path / (tag + ".npz"))
        p = _child([worker, path, what], poison, 300)
        assert p.returncode == 0 and "bitwise worker ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
        res[tag] = dict(np.load(path))
    clean, clean2, poison = res["clean"], res["clean2"], res["poison"]
    for cfg in ("cfg4real", "cfg5"):
        assert clean["apply_%s_nonfinite" % cfg] == 0 and poison["apply_%s_nonfinite" % cfg] == 0
        assert np.array_equal(clean["apply_%s_sha" % cfg], poison["apply_%s_sha" % cfg]), cfg
    assert clean["n_states_odd"] % 2 == 1 and clean["n_states_even"] % 2 == 0
    differ = [key for key in clean2 if not np.array_equal(clean[key], clean2[key])]
    assert not differ, differ                                               # clean runs repeat bit for bit across processes
    for key in clean2:
        assert np.isfinite(poison[key]).all() and np.array_equal(clean[key], poison[key]), key
