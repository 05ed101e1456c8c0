"""The MatMult plan on general descriptors, checked element by element (-m gpu; csrc/kron_plan.hip).

Every descriptor here is filled field by field (tests/kron_general.py), not through superblock.KronPlan: shifts of -2 .. 2, overlapping
cells, identity cells off the diagonal, `transposed` on any operator and on H_L / H_R, ld > nc, data pointers at odd element offsets,
duplicate and zero-coefficient terms, operators without cells, left-keyed and right-keyed groups in one plan, row ranges of the stage-1
intermediates with gaps and borders inside a tile, sectors of one and two states.  x is graded over 140 binary orders between the
KronBlocks, and every element of y is compared with the longdouble reference from the definition within kron_bound, a derived bound on
the element's own sum of magnitudes: a contribution missing from a weak block cannot hide behind max |y|.

Tile edge 64, k-step 16, copy tile 32: the sector sizes come from kron_general.SIZES."""
import numpy as np
import pytest
import torch

import kron_general as kg

pytestmark = pytest.mark.gpu
BAND = 64


@pytest.fixture(scope="module")
def mods(pkg):
    from dmrgx_amd import _capi
    _capi.require_device()
    return _capi


def _bits(t):
    return t.view(torch.int64)


def apply_in_bands(plan, x_full):
    """One apply with x at an odd element offset inside a NaN buffer and y NaN-prefilled at an odd element offset inside a band of
    SENTINEL; everything outside y must come back bit for bit.  -> y (numpy, local_len)"""
    nx, ny = plan.info.vec_len, plan.info.local_len
    xbuf = torch.full((nx + 8,), float("nan"), dtype=torch.float64, device="cuda")
    xbuf[3:3 + nx] = x_full
    ybuf = torch.full((ny + 2 * BAND + 2,), kg.SENTINEL, dtype=torch.float64, device="cuda")
    ybuf[BAND + 1:BAND + 1 + ny] = float("nan")
    x0, y0 = xbuf.clone(), ybuf.clone()
    plan.apply(xbuf[3:3 + nx], ybuf[BAND + 1:BAND + 1 + ny])
    torch.cuda.synchronize()
    assert torch.equal(_bits(xbuf), _bits(x0)), "x was written"
    assert torch.equal(_bits(ybuf[:BAND + 1]), _bits(y0[:BAND + 1])) and torch.equal(_bits(ybuf[BAND + 1 + ny:]), _bits(y0[BAND + 1 + ny:])), "written outside y"
    return ybuf[BAND + 1:BAND + 1 + ny].cpu().numpy()


def plain_apply(desc, x):
    plan = kg.raw_plan(desc)
    assert plan.info.n_states == desc.n_states == plan.info.vec_len == plan.info.local_len
    y = apply_in_bands(plan, torch.from_numpy(np.array(x)).cuda())
    info = (plan.info.n_groups, plan.info.n_tiles_stage1, plan.info.n_tiles_stage2)
    plan.destroy()
    return y, info


def gathered(desc, W, x=None, diag=False):
    """All W ranks' plans on one GPU: x striped, every rank's segment of y (or of the diagonal) computed by its plan, the stripes gathered
    back into the reference layout."""
    plans = [kg.raw_plan(desc, world_size=W, rank=r) for r in range(W)]
    info = plans[0].info
    out = torch.full((info.vec_len,), float("nan"), dtype=torch.float64, device="cuda")
    if not diag:
        xs = torch.zeros(info.vec_len, dtype=torch.float64, device="cuda")
        plans[0].to_striped(torch.from_numpy(np.array(x)).cuda(), xs)
    for p in plans:
        seg = out[p.info.local_offset:p.info.local_offset + p.info.local_len]
        p.diag(seg) if diag else p.apply(xs, seg)
    y = torch.full((desc.n_states,), float("nan"), dtype=torch.float64, device="cuda")
    plans[0].from_striped(out, y)
    torch.cuda.synchronize()
    for p in plans:
        p.destroy()
    return y.cpu().numpy()


@pytest.mark.parametrize("name", kg.CASES)
def test_apply(mods, name):
    d, x = kg.case(name)
    R, S, n = kg.case_reference(name)
    y, (n_groups, t1, t2) = plain_apply(d, x)
    print("%s: %d states, %d groups, %d + %d tiles" % (name, d.n_states, n_groups, t1, t2))
    assert kg.kron_check(y, R, S, n, name + " apply") <= 1.0
    assert n_groups == kg.min_vertex_cover(d)


@pytest.mark.parametrize("name", kg.CASES)
def test_gathered_apply(mods, name):
    d, x = kg.case(name)
    R, S, n = kg.case_reference(name)
    for W in (2, 3, 5):          # (5 ranks: more than the columns of some blocks, test_kron_general_host.py::test_generator_coverage)
        assert kg.kron_check(gathered(d, W, x), R, S, n, "%s gathered apply W=%d" % (name, W)) <= 1.0


@pytest.mark.parametrize("name", kg.CASES)
def test_fold_switch(mods, monkeypatch, name):
    d, x = kg.case(name)
    R, S, n = kg.case_reference(name)
    monkeypatch.setenv("DMRGX_PLAN_FOLD", "0")
    try:
        y_whole, info_whole = plain_apply(d, x)
    finally:
        monkeypatch.delenv("DMRGX_PLAN_FOLD")
    y, info = plain_apply(d, x)
    kg.kron_check(y_whole, R, S, n, name + " apply, whole intermediates")
    kg.kron_check(y, R, S, n, name + " apply, rows read")
    assert np.array_equal(y.view(np.uint64), y_whole.view(np.uint64))
    print("%s: stage-1 tiles %d (rows read) / %d (whole)" % (name, info[1], info_whole[1]))
    assert info[1] <= info_whole[1] and info[0] == info_whole[0]


@pytest.mark.parametrize("name", kg.CASES)
def test_diagonal(mods, name):
    d, _ = kg.case(name)
    D, Da, nd = kg.reference_diag(d)
    plan = kg.raw_plan(d)
    out = torch.full((plan.info.local_len,), float("nan"), dtype=torch.float64, device="cuda")
    plan.diag(out)
    torch.cuda.synchronize()
    plan.destroy()
    assert kg.kron_check(out.cpu().numpy(), D, Da, nd, name + " diagonal W=1") <= 1.0
    assert kg.kron_check(gathered(d, 2, diag=True), D, Da, nd, name + " diagonal W=2") <= 1.0


@pytest.mark.parametrize("name", kg.CASES)
def test_repeatability(mods, name):
    d, x = kg.case(name)
    xd = torch.from_numpy(np.array(x)).cuda()
    plan = kg.raw_plan(d)
    y1 = apply_in_bands(plan, xd)
    y2 = apply_in_bands(plan, xd)
    plan.destroy()
    y3, _ = plain_apply(d, x)
    assert np.isfinite(y1).all()
    assert np.array_equal(y1.view(np.uint64), y2.view(np.uint64)) and np.array_equal(y1.view(np.uint64), y3.view(np.uint64))


def test_patched_table_cache_past_its_capacity(mods):
    """The plan keeps the patched task tables of PATCHED_MAX = 24 (x, y) pairs and then overwrites them round robin.  30 pairs in order,
    the same 30 in reverse order, then pair 0 with a new x in the same buffer: every result is what a fresh plan gives on that input, bit
    for bit.  All on the current stream."""
    d, _ = kg.case("shifts")
    npairs = 30
    inputs = [np.array(kg.graded_x(d, 50 + i)) for i in range(npairs + 1)]

    def fresh(x):
        p = kg.raw_plan(d)
        y = torch.full((d.n_states,), float("nan"), dtype=torch.float64, device="cuda")
        p.apply(torch.from_numpy(x).cuda(), y)
        torch.cuda.synchronize()
        p.destroy()
        return y.cpu().numpy().view(np.uint64)

    want = [fresh(x) for x in inputs]
    assert len({w.tobytes() for w in want}) == npairs + 1
    xs = [torch.from_numpy(x).cuda() for x in inputs[:npairs]]
    ys = [torch.full((d.n_states,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(npairs)]
    assert len({t.data_ptr() for t in xs}) == npairs and len({t.data_ptr() for t in ys}) == npairs
    plan = kg.raw_plan(d)
    for order in (range(npairs), reversed(range(npairs))):
        for y in ys:
            y.fill_(float("nan"))
        for i in order:
            plan.apply(xs[i], ys[i])
        torch.cuda.synchronize()
        for i in range(npairs):
            assert np.array_equal(ys[i].cpu().numpy().view(np.uint64), want[i]), i
    xs[0].copy_(torch.from_numpy(inputs[npairs]))
    ys[0].fill_(float("nan"))
    plan.apply(xs[0], ys[0])
    torch.cuda.synchronize()
    plan.destroy()
    assert np.array_equal(ys[0].cpu().numpy().view(np.uint64), want[npairs])
