"""The MatMult plan that builds only the rows of the stage-1 intermediates which stage 2 reads (-m gpu; csrc/kron_plan.hip).

The rows of T_{g,k} nobody reads belong to left operators whose cells do not cover their column sector: the identity-only operators of a
block's new site (Sp, Sm: one cell per sector block).  Every case is applied with the default plan and with DMRGX_PLAN_FOLD=0 (every
intermediate whole), each in a fresh plan, and compared with the CPU oracle's row loop at 1e-13 of max|y| -- the comparison of
tests/test_gpu_kron.py -- and with each other bit for bit.  dmrgx_kron_diag of both plans is compared with the diagonal computed from the
dense sector blocks of the operators.  The kept sectors hold 1-40 states; every case has an enlarged sector of more than 64 rows whose
halves have fewer, so that dropping the unread half drops a row of 64 x 64 tiles."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import oracle_shell_from_superblock
from oracle.kron_c import ShellApplyC
from test_gpu_kron import RTOL, _apply

pytestmark = pytest.mark.gpu
OpSm, OpSz, OpSp = -1, 0, +1

KEPT_SMALL = ({1.0: 3, 0.0: 37, -1.0: 34}, {1.0: 2, 0.0: 6, -1.0: 5})                                    # L != R, enlarged edge sectors with dn == 0 / up == 0
KEPT_WIDE = ({1.5: 1, 0.5: 39, -0.5: 32, -1.5: 2}, {1.5: 2, 0.5: 11, -0.5: 8, -1.5: 1})
KEPT_65 = ({1.5: 5, 0.5: 33, -0.5: 32, -1.5: 40, -2.5: 3}, {1.5: 4, 0.5: 32, -0.5: 33, -1.5: 7})          # enlarged sectors of 65 = 33 + 32 and 72 = 32 + 40 rows


@pytest.fixture(scope="module")
def mods(pkg):
    from dmrgx_amd import superblock, workloads, _capi
    _capi.require_device()
    return superblock, workloads, _capi


def _split_h_right(wl, sb, kept_r, rng):
    """H_R as the dd and uu cells of every sector plus the du / ud cells beside them."""
    _, sizes, sub = wl.enlarged_sectors(kept_r)
    assert list(sizes) == list(sb.right_sizes)
    cells = []
    for q, (dn, up) in enumerate(sub):
        a = rng.standard_normal((dn + up, dn + up))
        a = (a + a.T) * 0.5
        for (r0, nr) in ((0, dn), (dn, up)):
            for (c0, nc) in ((0, dn), (dn, up)):
                if nr and nc:
                    cells.append(wl.OpCell(q, r0, c0, nr, nc, wl.CELL_DENSE, 0.0, np.ascontiguousarray(a[r0:r0 + nr, c0:c0 + nc])))
    return wl.SectorOperator(0, cells)


def build_case(wl, name):
    """-> (superblock the plan sees, superblock the oracle sees): the same operator except where the oracle needs an empty H_R in place of none."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "full_hr":           # H_R one full cell per sector: edge sectors with dn == 0 / up == 0;
        # Ly = 3 with next-nearest bonds: every right operator is coupled to the left new site AND to an old left site; Sm is a transposed Sp
        sb = wl.synthetic_superblock("cfg2", Ly=3, seed=11, kept=KEPT_SMALL)
    elif name == "split_hr":        # H_R as dd / uu cells plus off-diagonal cells
        sb = wl.synthetic_superblock("cfg2", Ly=3, seed=12, kept=KEPT_WIDE)
        sb.h_right = _split_h_right(wl, sb, KEPT_WIDE[1], rng)
    elif name == "no_hr":           # no H_R at all
        sb = wl.synthetic_superblock("cfg2", Ly=3, seed=13, kept=KEPT_SMALL)
        sb.h_right = None
    elif name == "no_hl_no_hr":
        sb = wl.synthetic_superblock("cfg2", Ly=2, seed=14, kept=KEPT_WIDE)
        sb.h_left = sb.h_right = None
    elif name == "scales":          # identity scales other than +-1/2 (and not powers of two)
        sb = wl.synthetic_superblock("cfg2", Ly=3, seed=15, kept=KEPT_WIDE)
        for (op, site), o in sb.left_ops.items():
            if site == 2:
                for i, c in enumerate(o.cells):
                    assert c.kind == wl.CELL_IDENT
                    c.scale = (0.7, -0.3, 1.25)[i % 3] if op == OpSz else 1.25
    elif name == "penalty":         # every S-S+ pair across the cut beside the model's bonds, as -spin_penalty adds them (Ly = 4: pairs the model does not couple)
        sb = wl.synthetic_superblock("cfg2", Ly=4, seed=16, kept=KEPT_SMALL)
        lam = 0.37
        sb.terms = list(sb.terms) + [t for i in range(4) for j in range(4) for t in ((lam, OpSm, i, OpSp, j), (lam, OpSp, i, OpSm, j), (2 * lam, OpSz, i, OpSz, j))]
    elif name == "nn_only":         # no next-nearest bonds: the right operators of the new site's groups hold identity cells only
        sb = wl.synthetic_superblock("cfg3", Ly=3, seed=17, kept=KEPT_WIDE)
    elif name == "size65":          # row ranges of 33 + 32 and 32 + 40 rows: a range border inside a 64-row tile, ranges that cross the tile border
        sb = wl.synthetic_superblock("cfg2", Ly=2, seed=18, kept=KEPT_65)
        assert 65 in sb.left_sizes and 65 in sb.right_sizes
    else:
        raise KeyError(name)
    ref = sb
    if sb.h_left is None or sb.h_right is None:
        ref = copy.copy(sb)
        ref.h_left = sb.h_left if sb.h_left is not None else wl.SectorOperator(0, [])
        ref.h_right = sb.h_right if sb.h_right is not None else wl.SectorOperator(0, [])
    return sb, ref


CASES = ["full_hr", "split_hr", "no_hr", "no_hl_no_hr", "scales", "penalty", "nn_only", "size65"]


def _op_blocks(wl, ops, sizes, op, site):
    """{row sector: dense block} of operator (op, site); Sm(i) = Sp(i)^T"""
    if op != OpSm:
        return wl.operator_to_dense_blocks(ops[(op, site)], sizes)
    return {q + 1: b.T for q, b in wl.operator_to_dense_blocks(ops[(OpSp, site)], sizes).items()}


def dense_diagonal(wl, sb):
    """diag(H_sb) in the reference layout from the dense sector blocks: H_L (x) 1 + 1 (x) H_R + the shift-0 terms."""
    hl = wl.operator_to_dense_blocks(sb.h_left, sb.left_sizes) if sb.h_left is not None else {}
    hr = wl.operator_to_dense_blocks(sb.h_right, sb.right_sizes) if sb.h_right is not None else {}
    out = []
    for (il, ir) in sb.blocks:
        nl, nr = sb.left_sizes[il], sb.right_sizes[ir]
        d = np.zeros((nl, nr))
        if il in hl:
            d += np.diag(hl[il])[:, None]
        if ir in hr:
            d += np.diag(hr[ir])[None, :]
        for (a, iop, isite, jop, jsite) in sb.terms:
            if iop != OpSz:
                continue
            A, B = _op_blocks(wl, sb.left_ops, sb.left_sizes, iop, isite).get(il), _op_blocks(wl, sb.right_ops, sb.right_sizes, jop, jsite).get(ir)
            if A is not None and B is not None:
                d += a * np.outer(np.diag(A), np.diag(B))
        out.append(d.ravel())
    return np.concatenate(out)


def unread_row_flops(wl, sb):
    """Stage-1 flops that the plan of whole intermediates spends on rows of the intermediates T_{g,k} of the identity-only left operators which
    stage 2 never reads, from the cell tables: per group and KronBlock, (rows of the source block - rows under an identity cell of sector IL)
    x 2 x (elements of the distinct dense cells of the group's right operators in sector IR, rows of their identity cells)."""
    kmap = {b: k for k, b in enumerate(sb.blocks)}
    total = 0.0
    groups = sorted({(t[1], t[2]) for t in sb.terms if t[0] != 0.0})
    for (iop, isite) in groups:
        src = sb.left_ops[(OpSp if iop != OpSz else OpSz, isite)]
        if not src.cells or any(c.kind != wl.CELL_IDENT for c in src.cells):
            continue
        # normalised identity cells (row sector, first source row, rows)
        cells = [(c.row_sector + 1, c.r0, c.nr) if iop == OpSm else (c.row_sector, c.c0, c.nr) for c in src.cells]
        rights = sorted({(t[3], t[4]) for t in sb.terms if t[0] != 0.0 and (t[1], t[2]) == (iop, isite)})
        for k, (il, ir) in enumerate(sb.blocks):
            ks = kmap.get((il + iop, ir - iop))
            if ks is None:
                continue
            read = np.zeros(sb.left_sizes[sb.blocks[ks][0]], dtype=bool)
            for (q, s0, n) in cells:
                if q == il:
                    read[s0:s0 + n] = True
            geo = set()
            for (jop, jsite) in rights:
                o = sb.right_ops[(OpSp if jop != OpSz else OpSz, jsite)]
                for c in o.cells:
                    q = c.row_sector + 1 if jop == OpSm else c.row_sector
                    if q == ir:             # (an identity cell of n rows is a scaled copy of n columns: 2 n flops per row of T)
                        geo.add(((c.c0, c.r0, c.nc, c.nr) if jop == OpSm else (c.r0, c.c0, c.nr, c.nc)) + (c.kind,))
            total += 2.0 * float((~read).sum()) * sum(g[2] * g[3] if g[4] == wl.CELL_DENSE else g[2] for g in geo)
    return total


def make_plan(sbm, sb, monkeypatch, rows_read, **kw):
    """A fresh plan; the switch is read when the plan is created."""
    if rows_read:
        monkeypatch.delenv("DMRGX_PLAN_FOLD", raising=False)
    else:
        monkeypatch.setenv("DMRGX_PLAN_FOLD", "0")
    try:
        return sbm.KronPlan(sb, **kw)
    finally:
        monkeypatch.delenv("DMRGX_PLAN_FOLD", raising=False)


_REFERENCE = {}


def reference(wl, name):
    """(plan superblock, x, oracle y, dense diagonal) of a case: computed once, read-only."""
    if name not in _REFERENCE:
        sb, ref = build_case(wl, name)
        x = np.random.default_rng(len(name)).standard_normal(sb.n_states)
        y = ShellApplyC(oracle_shell_from_superblock(ref)).apply(x)
        d = dense_diagonal(wl, sb)
        for a in (x, y, d):
            a.setflags(write=False)
        _REFERENCE[name] = (sb, x, y, d)
    return _REFERENCE[name]


def _diag(capi, plan):
    d = torch.full((plan.info.local_len,), float("nan"), dtype=torch.float64, device="cuda")
    capi.check(capi.lib().dmrgx_kron_diag(plan._handle, C.c_void_p(d.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return d.cpu().numpy()


@pytest.mark.parametrize("name", CASES)
def test_both_plans_match_the_oracle_and_each_other(mods, monkeypatch, name):
    sbm, wl, capi = mods
    sb, x, y_ref, d_ref = reference(wl, name)
    info, ys = {}, {}
    for rows_read in (True, False):
        plan = make_plan(sbm, sb, monkeypatch, rows_read)
        y = ys[rows_read] = _apply(plan, np.array(x))
        err = np.abs(y - y_ref).max() / np.abs(y_ref).max()
        d = _diag(capi, plan)
        derr = np.abs(d - d_ref).max() / max(1.0, np.abs(d_ref).max())
        info[rows_read] = (plan.info.n_tiles_stage1, plan.info.flops_alg, plan.info.n_groups)
        print("%s rows_read=%d: apply err %.2e, diag err %.2e, stage-1 tiles %d, flops_alg %.0f, groups %d" % ((name, rows_read, err, derr) + info[rows_read]))
        plan.destroy()
        assert np.isfinite(y).all() and err <= RTOL, (name, rows_read, err)
        assert derr <= 1e-13, (name, rows_read, derr)
    # the rows went: fewer stage-1 tiles and fewer flops, by at least the unread rows of the identity-only groups
    unread = unread_row_flops(wl, sb)
    print("%s: unread-row flops of the identity-only groups %.0f, flops_alg drop %.0f" % (name, unread, info[False][1] - info[True][1]))
    assert unread > 0
    assert info[True][0] < info[False][0], info
    assert info[True][1] < info[False][1] and info[False][1] - info[True][1] >= unread, (info, unread)
    assert info[True][2] == info[False][2]
    # no sum changed: the same y bit for bit
    assert np.array_equal(ys[True], ys[False])


def test_dense_diagonal_is_the_diagonal_of_the_factored_apply(mods):
    """The reference of the diagonal checks above against the numpy statement of the apply, column by column, on the smallest case."""
    _, wl, _ = mods
    sb, _ = build_case(wl, "full_hr")
    H = np.stack([wl.apply_factored_numpy(sb, e) for e in np.eye(sb.n_states)], axis=1)
    assert np.abs(np.diag(H) - dense_diagonal(wl, sb)).max() <= 1e-14 * np.abs(H).max()


@pytest.mark.parametrize("name", ["full_hr", "scales", "no_hr", "size65"])
def test_both_plans_striped_over_two_ranks(mods, monkeypatch, name):
    """Two ranks' plans on one GPU (the rehearsal workers build their own superblocks, so they cannot take these cases): the rows read of a
    source block are taken panel by panel at their row offset, and the gathered stripes equal the oracle with and without the switch."""
    sbm, wl, capi = mods
    sb, x, y_ref, d_ref = reference(wl, name)
    for fold in (True, False):
        plans = [make_plan(sbm, sb, monkeypatch, fold, world_size=2, rank=r) for r in range(2)]
        info = plans[0].info
        xs = torch.zeros(info.vec_len, dtype=torch.float64, device="cuda")
        plans[0].to_striped(torch.from_numpy(np.array(x)).cuda(), xs)
        ys, ds = torch.full_like(xs, float("nan")), torch.zeros_like(xs)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for p in plans:
            p.apply(xs, ys[p.info.local_offset:p.info.local_offset + p.info.local_len])
            capi.check(capi.lib().dmrgx_kron_diag(p._handle, C.c_void_p(ds[p.info.local_offset:].data_ptr()), st))
        y, d = torch.full((sb.n_states,), float("nan"), dtype=torch.float64, device="cuda"), torch.zeros(sb.n_states, dtype=torch.float64, device="cuda")
        plans[0].from_striped(ys, y)
        plans[0].from_striped(ds, d)
        torch.cuda.synchronize()
        for p in plans:
            p.destroy()
        y, d = y.cpu().numpy(), d.cpu().numpy()
        assert np.isfinite(y).all() and np.abs(y - y_ref).max() <= RTOL * np.abs(y_ref).max(), (name, fold)
        assert np.abs(d - d_ref).max() <= 1e-13 * max(1.0, np.abs(d_ref).max()), (name, fold)
