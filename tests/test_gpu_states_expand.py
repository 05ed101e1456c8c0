"""dmrgx_kron_states_expand (-m gpu, csrc/states_expand.hip) on the 845-state layout (4 KronBlocks): the expansion equals numpy's
np.sqrt(w) * psi panels bit for bit, and dmrgx_rdm_create_subset on it gives the spectra of the state-averaged density matrices
sum_s w_s rho_s, which the test builds densely WITHOUT the expansion, within the bounds of tests/test_gpu_noise_rdm.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu
WEIGHTS = {3: [(1.0, 1.0, 1.0), (0.5, 0.0, 0.25)], 2: [(1.0, 1.0), (0.5, 0.0)], 1: [(1.0,)]}
CASES = [(ns, w) for ns in (1, 2, 3) for w in WEIGHTS[ns]]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def mods(pkg):
    from dmrgx_amd import superblock, workloads, _capi
    _capi.require_device()
    return superblock, workloads, _capi


@pytest.fixture(scope="module")
def layout(mods):
    sb = helpers.krylov_superblock(mods[1], 845)
    psi = np.random.default_rng(31).standard_normal((3, 845))
    psi.setflags(write=False)
    return (list(sb.left_sizes), list(sb.right_sizes), list(sb.blocks)), psi


def _blocks_of(lay, v):
    lsz, rsz, blocks = lay
    out, o = [], 0
    for a, b in blocks:
        out.append(v[o:o + lsz[a] * rsz[b]].reshape(lsz[a], rsz[b]))
        o += lsz[a] * rsz[b]
    return out


def _model(lay, psi, weights, side):
    """-> the blocks of the expansion as matrices: numpy's np.sqrt(w) * psi panels, a weight-0 panel as zeros"""
    per_state = [_blocks_of(lay, p) for p in psi]
    mats = []
    for k in range(len(lay[2])):
        parts = [np.zeros_like(per_state[s][k]) if w == 0.0 else np.sqrt(w) * per_state[s][k] for s, w in enumerate(weights)]
        mats.append(np.concatenate(parts, axis=1 if side == 0 else 0))
    return mats


def _psi_store(psi, ns, pad, offset):
    """Psi as a view of a NaN-filled store: row stride n + pad, `offset` doubles into the allocation"""
    n = psi.shape[1]
    store = torch.full((offset + ns * (n + pad) + 1,), float("nan"), dtype=torch.float64, device="cuda")
    P = store[offset:offset + ns * (n + pad)].view(ns, n + pad)[:, :n]
    P.copy_(torch.from_numpy(psi[:ns].copy()))
    assert P.data_ptr() % 16 == (8 * offset) % 16
    return store, P


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("ns,weights", CASES)
def test_expansion_is_numpy_bit_for_bit(mods, layout, ns, weights, side):
    sbm = mods[0]
    lay, psi = layout
    n = psi.shape[1]
    mats = _model(lay, psi[:ns], weights, side)
    want = np.concatenate([m.ravel() for m in mats])
    for pad, offset, yoff in ((0, 0, 0), (3, 1, 0), (3, 1, 1), (2, 0, 1)):
        store, P = _psi_store(psi, ns, pad, offset)
        Ystore = torch.full((yoff + want.size + 2,), float("nan"), dtype=torch.float64, device="cuda")
        Y, extent, n_out = sbm.states_expand(lay, P, weights, side, out=Ystore[yoff:])
        torch.cuda.synchronize()
        got = Ystore.cpu().numpy()
        assert n_out == want.size == ns * n
        assert extent == [ns * (lay[1][b] if side == 0 else lay[0][a]) for a, b in lay[2]]
        assert np.array_equal(_bits(got[yoff:yoff + n_out]), _bits(want)), (pad, offset, yoff)
        assert np.isnan(got[:yoff]).all() and np.isnan(got[yoff + n_out:]).all()
        # Psi is only read: its bits and the NaN around and between its rows are still there
        back = store.cpu().numpy()
        rows = back[offset:offset + ns * (n + pad)].reshape(ns, n + pad)
        assert np.array_equal(_bits(rows[:, :n]), _bits(psi[:ns])) and np.isnan(rows[:, n:]).all() and np.isnan(back[:offset]).all() and np.isnan(back[-1])
    # a weight-1 panel carries identical bits (np.sqrt(1.0) * x is x in numpy too: checked against psi itself)
    for s, w in enumerate(weights):
        if w == 1.0:
            for k, m in enumerate(mats):
                blk = _blocks_of(lay, psi[s])[k]
                panel = m[:, s * blk.shape[1]:(s + 1) * blk.shape[1]] if side == 0 else m[s * blk.shape[0]:(s + 1) * blk.shape[0], :]
                assert np.array_equal(_bits(panel), _bits(blk))


def test_a_weight_zero_panel_is_zeros_whatever_the_state_holds(mods, layout):
    sbm = mods[0]
    lay, psi = layout
    bad = psi.copy()
    bad[1, ::7] = np.nan
    bad[1, 3] = np.inf
    for side in (0, 1):
        Y, _, n_out = sbm.states_expand(lay, torch.from_numpy(bad).cuda(), (0.5, 0.0, 0.25), side)
        want = np.concatenate([m.ravel() for m in _model(lay, psi, (0.5, 0.0, 0.25), side)])
        assert np.array_equal(_bits(Y.cpu().numpy()[:n_out]), _bits(want))


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("ns,weights", [(3, (1.0, 1.0, 1.0)), (3, (0.5, 0.0, 0.25)), (1, (1.0,))])
def test_density_matrices_of_the_expansion_are_the_weighted_average(mods, layout, ns, weights, side):
    sbm = mods[0]
    lay, psi = layout
    Y, extent, n_out = sbm.states_expand(lay, torch.from_numpy(psi[:ns].copy()).cuda(), weights, side)
    lsz, rsz, blocks, mask = sbm.noise_rdm_layout(lay, side, extent)
    rdm = sbm.ReducedDensityMatrices(lsz, rsz, blocks, Y, side_mask=mask)
    jacobi = bool(rdm.report.solver)
    per_state = [_blocks_of(lay, p) for p in psi[:ns]]
    for k in range(len(blocks)):
        rho = sum(w * (X[k] @ X[k].T if side == 0 else X[k].T @ X[k]) for w, X in zip(weights, per_state))
        w_ref = np.linalg.eigvalsh(rho)[::-1]
        w = rdm.eigenvalues(side, k)
        bound_w, _ = (helpers.rdm_jacobi_bounds if jacobi else helpers.rdm_bounds)(rho, w_ref)
        err = np.abs(w - w_ref).max()
        print("states rdm side %d block %d n %d: |w - eigvalsh| %.3e, bound %.3e" % (side, k, len(w), err, bound_w))
        assert w.shape == w_ref.shape and np.isfinite(w).all() and np.all(np.diff(w) <= 0)
        assert err <= bound_w, (k, err, bound_w)
    with pytest.raises(Exception):
        rdm.eigenvalues(1 - side, 0)
    rdm.destroy()                      # raises unless the deferred verification agrees


def test_refusals(mods, layout):
    _, _, capi = mods
    lay, psi = layout
    lsz, rsz, blocks = lay
    n, nb = psi.shape[1], len(blocks)
    lib = capi.lib()
    ARG, RANGE = capi.DMRGX_ERR_ARG, capi.DMRGX_ERR_OUTOFRANGE
    P = torch.from_numpy(psi.copy()).cuda()
    Y = torch.full((3 * n + 4,), float("nan"), dtype=torch.float64, device="cuda")
    i32 = lambda v: (C.c_int32 * len(v))(*v)       # noqa: E731
    ls, rs = i32(lsz), i32(rsz)
    sl, sr = capi.Sectors(len(lsz), ls), capi.Sectors(len(rsz), rs)
    il, ir = i32([b[0] for b in blocks]), i32([b[1] for b in blocks])
    extent, n_out = (C.c_int32 * nb)(*([-7] * nb)), C.c_int64(-7)
    w3 = lambda *v: (C.c_double * len(v))(*v)      # noqa: E731

    def call(left=C.byref(sl), right=C.byref(sr), nblocks=nb, il_=il, ir_=ir, ns=3, psi_=C.c_void_p(P.data_ptr()), ld=n, w=w3(1.0, 1.0, 1.0), side=0,
             ext=extent, nout=C.byref(n_out), y=C.c_void_p(Y.data_ptr())):
        rc = lib.dmrgx_kron_states_expand(left, right, nblocks, il_, ir_, ns, psi_, ld, w, side, ext, nout, y, None)
        return rc, lib.dmrgx_last_error().decode()

    twice, outside = list(blocks), list(blocks)
    twice[2] = twice[0]
    outside[1] = (len(lsz), 0)
    huge_r = i32([2 ** 30] * len(rsz))
    cases = {
        "null left": (dict(left=None), ARG, "sector table"), "null right": (dict(right=None), ARG, "sector table"),
        "null il": (dict(il_=None), ARG, "KronBlocks"), "null ir": (dict(ir_=None), ARG, "KronBlocks"),
        "null extent": (dict(ext=None), ARG, "extent"), "null n_out": (dict(nout=None), ARG, "n_out"),
        "nstates 0": (dict(ns=0), ARG, "nstates"), "null weights": (dict(w=None), ARG, "weights"),
        "ldpsi": (dict(ld=n - 1), ARG, "ldpsi"), "negative weight": (dict(w=w3(1.0, -0.5, 1.0)), ARG, "weight 1"),
        "nan weight": (dict(w=w3(1.0, 1.0, float("nan"))), ARG, "weight 2"), "inf weight": (dict(w=w3(float("inf"), 1.0, 1.0)), ARG, "weight 0"),
        "all zero": (dict(w=w3(0.0, 0.0, 0.0)), ARG, "zero"), "side 2": (dict(side=2), ARG, "side"), "side -1": (dict(side=-1), ARG, "side"),
        "null Psi": (dict(psi_=None), ARG, "null Psi"), "Y is Psi": (dict(y=C.c_void_p(P.data_ptr())), ARG, "overlaps"),
        "Y overlaps the end of Psi": (dict(y=C.c_void_p(P.data_ptr() + 8 * (3 * n - 1))), ARG, "overlaps"),
        "listed twice": (dict(il_=i32([b[0] for b in twice]), ir_=i32([b[1] for b in twice])), ARG, "twice"),
        "extent above 2^31 - 1": (dict(right=C.byref(capi.Sectors(len(rsz), huge_r)), y=None), ARG, "2^31"),
        "outside": (dict(il_=i32([b[0] for b in outside]), ir_=i32([b[1] for b in outside])), RANGE, "out of range"),
    }
    for what, (kw, code, word) in cases.items():
        rc, msg = call(**kw)
        assert rc == code and word in msg, (what, rc, msg)
    assert torch.isnan(Y).all()                                               # every refusal came before any device work
    # sizes only: no device, Psi may be null
    rc, _ = call(psi_=None, y=None)
    assert rc == 0 and n_out.value == 3 * n and list(extent) == [3 * rsz[b] for _, b in blocks]
    rc, _ = call(side=1)
    assert rc == 0 and list(extent) == [3 * lsz[a] for a, _ in blocks]
    torch.cuda.synchronize()
    assert not torch.isnan(Y[:3 * n]).any() and torch.isnan(Y[3 * n:]).all()
