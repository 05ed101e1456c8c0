"""dmrgx_kron_noise_expand: psi with the images coef[a] A_a psi of one block's operators set beside it, against the numpy restatement of
tests/noise_inputs.py (-m gpu).  Both sides; sizes-only call, the Psi_k parts bit for bit, every panel to 1e-13 max |Y| (the project's
MatMult parity bound for products of this depth), exact zeros for coef == 0, a NaN-filled output that comes back finite, the same bits
twice, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import noise_inputs as ni

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_OUTOFRANGE = 62, 63
LAYOUT = (ni.LSZ, ni.RSZ, ni.BLOCKS)


@pytest.fixture(scope="module")
def mods(pkg):
    from dmrgx_amd import superblock, workloads, _capi
    _capi.require_device()
    return superblock, workloads, _capi


@pytest.fixture(scope="module")
def planted(mods):
    """Per side: psi, the operators and the model's expansion; built once, never changed."""
    _, wl, _ = mods
    out = {}
    for side in (0, 1):
        psi, ops = ni.case(wl, side)
        out[side] = (psi, ops) + ni.model_expand(psi, side, ops, ni.COEF)
    return out


def _raw_args(sbm, side, psi, ops):
    args, psi_d, keep = sbm._gram_arguments(LAYOUT, psi, ops if side == 0 else [], ops if side == 1 else [])
    head = args[:6]
    n_ops, arr = (args[6], args[7]) if side == 0 else (args[8], args[9])
    return head, n_ops, arr, psi_d, keep


def _split(Y, side, extent):
    """The flat expansion -> its blocks as matrices."""
    mats, o = [], 0
    for k, (a, b) in enumerate(ni.BLOCKS):
        shape = (ni.LSZ[a], extent[k]) if side == 0 else (extent[k], ni.RSZ[b])
        mats.append(Y[o:o + shape[0] * shape[1]].reshape(shape))
        o += shape[0] * shape[1]
    assert o == Y.size
    return mats


def test_the_inputs_hit_every_path(planted):
    """The planted case has what the header promises to handle: a sector pair without a KronBlock that a shift leads to, a shift off the
    table, an IDENT cell beside a DENSE cell, a transposed operator, and panels on both sides of the 64 tile edge."""
    for side in (0, 1):
        psi, ops, mats, extent, n_out = planted[side]
        sec = [b[side] for b in ni.BLOCKS]
        missing = ({0, 1, 2, 3, 4} - set(sec)).pop()
        assert any(s - ni.shift_of(op) == missing for s in sec for op in ops)               # exists, no KronBlock
        assert any(not 0 <= s - ni.shift_of(op) < 5 for s in sec for op in ops)             # off the table
        assert {c.kind for c in ops[0].cells if c.row_sector == (2, 1)[side]} == {1, 2}
        panels = ni.model_panels(psi, side, ops, ni.COEF)
        assert {a for lst in panels for a, _, _ in lst} == {0, 1, 2, 3, 4}                  # every operator lands somewhere
        assert all(e > (ni.RSZ[b] if side == 0 else ni.LSZ[a]) for e, (a, b) in zip(extent, ni.BLOCKS))
        assert n_out > ni.N_STATES


@pytest.mark.parametrize("side", [0, 1])
def test_expansion_against_the_numpy_model(mods, planted, side):
    import torch
    sbm, _, capi = mods
    psi, ops, want, extent, n_out = planted[side]
    # sizes only: no psi, no Y
    head, n_ops, arr, psi_d, keep = _raw_args(sbm, side, psi, ops)
    cf = (C.c_double * n_ops)(*ni.COEF)
    ext, tot = (C.c_int32 * len(ni.BLOCKS))(), C.c_int64(-1)
    nopsi = head[:5] + (None,)
    assert capi.lib().dmrgx_kron_noise_expand(*nopsi, side, n_ops, arr, cf, ext, C.byref(tot), None, None) == 0
    assert list(ext) == extent and tot.value == n_out
    # the expansion into a NaN-filled buffer with three spare elements
    Y = torch.full((n_out + 3,), float("nan"), dtype=torch.float64, device="cuda")
    ret, ext2, tot2 = sbm.noise_expand(LAYOUT, psi, side, ops, ni.COEF, out=Y)
    assert ret is Y and ext2 == extent and tot2 == n_out
    got = Y.cpu().numpy()
    assert np.isnan(got[n_out:]).all() and np.isfinite(got[:n_out]).all()
    mats = _split(got[:n_out], side, extent)
    scale = max(np.abs(m).max() for m in want)
    X = ni.psi_blocks(psi)
    panels = ni.model_panels(psi, side, ops, ni.COEF)
    worst = 0.0
    for k, (a, b) in enumerate(ni.BLOCKS):
        own = mats[k][:, :ni.RSZ[b]] if side == 0 else mats[k][:ni.LSZ[a], :]
        assert np.array_equal(np.ascontiguousarray(own).view(np.uint64), np.ascontiguousarray(X[k]).view(np.uint64)), k      # Psi_k bit for bit
        at = ni.RSZ[b] if side == 0 else ni.LSZ[a]
        for op_i, ks, p in panels[k]:
            w = p.shape[1 - side]
            g = mats[k][:, at:at + w] if side == 0 else mats[k][at:at + w, :]
            assert g.shape == p.shape
            worst = max(worst, np.abs(g - p).max())
            assert np.abs(g - p).max() <= 1e-13 * scale, (k, op_i, ks, np.abs(g - p).max())
            if op_i == ni.ZERO_OP:
                assert (g == 0.0).all(), (k, ks)
            at += w
        assert at == extent[k]
    print("noise_expand side %d: n_out %d, extents %s, worst |panel - model| %.3e, bound %.3e" % (side, n_out, extent, worst, 1e-13 * scale))
    assert np.abs(np.concatenate([m.ravel() for m in want])).max() > 0.1
    # the same bits from a second call into a fresh buffer; psi untouched
    Y2, _, _ = sbm.noise_expand(LAYOUT, psi_d, side, ops, ni.COEF)
    assert Y2.numel() == n_out
    assert np.array_equal(Y2.cpu().numpy().view(np.uint64), got[:n_out].view(np.uint64))
    assert np.array_equal(psi_d.cpu().numpy().view(np.uint64), np.asarray(psi).view(np.uint64))


def test_no_operators_copies_psi(mods, planted):
    sbm, _, _ = mods
    psi = planted[0][0]
    for side in (0, 1):
        Y, extent, n_out = sbm.noise_expand(LAYOUT, psi, side, [], [])
        assert n_out == ni.N_STATES and extent == [(ni.RSZ[b] if side == 0 else ni.LSZ[a]) for a, b in ni.BLOCKS]
        assert np.array_equal(Y.cpu().numpy().view(np.uint64), np.asarray(psi).view(np.uint64))


def test_noise_expand_refusals(mods, planted):
    """Null pointers, a side that is not 0 or 1, a cell outside its sector block, a KronBlock out of range and a Y that overlaps psi
    return their codes and leave Y alone."""
    import torch
    sbm, wl, capi = mods
    L = capi.lib()
    psi, ops, _, extent, n_out = planted[0]
    head, n_ops, arr, psi_d, keep = _raw_args(sbm, 0, psi, ops)
    cf = (C.c_double * n_ops)(*ni.COEF)
    ext, tot = (C.c_int32 * len(ni.BLOCKS))(), C.c_int64(0)
    Y = torch.full((n_out,), 7.0, dtype=torch.float64, device="cuda")
    yp = C.c_void_p(Y.data_ptr())
    call = L.dmrgx_kron_noise_expand
    assert call(*head, 2, n_ops, arr, cf, ext, C.byref(tot), yp, None) == ERR_ARG and b"side" in L.dmrgx_last_error()
    assert call(*head, -1, n_ops, arr, cf, ext, C.byref(tot), yp, None) == ERR_ARG
    assert call(*head, 0, n_ops, None, cf, ext, C.byref(tot), yp, None) == ERR_ARG
    assert call(*head, 0, n_ops, arr, None, ext, C.byref(tot), yp, None) == ERR_ARG
    assert call(*head, 0, n_ops, arr, cf, None, C.byref(tot), yp, None) == ERR_ARG
    assert call(*head, 0, n_ops, arr, cf, ext, None, yp, None) == ERR_ARG
    assert call(*(head[:5] + (None,)), 0, n_ops, arr, cf, ext, C.byref(tot), yp, None) == ERR_ARG               # psi null with Y given
    assert call(None, *head[1:], 0, n_ops, arr, cf, ext, C.byref(tot), yp, None) == ERR_ARG
    assert call(head[0], None, *head[2:], 0, n_ops, arr, cf, ext, C.byref(tot), yp, None) == ERR_ARG
    assert call(*head[:3], None, *head[4:], 0, n_ops, arr, cf, ext, C.byref(tot), yp, None) == ERR_ARG
    # a left operator handed in as a right one: its cells do not fit the right sector blocks
    assert call(*head, 1, n_ops, arr, cf, ext, C.byref(tot), yp, None) == ERR_OUTOFRANGE
    # a cell one row past its sector block; a KronBlock past the tables
    bad = wl.SectorOperator(0, [wl.OpCell(1, 1, 0, 3, 3, wl.CELL_IDENT, 1.0)])
    with pytest.raises(capi.DmrgxError) as e:
        sbm.noise_expand(LAYOUT, psi_d, 0, [bad], [1.0], out=Y)
    assert e.value.code == ERR_OUTOFRANGE
    past = (C.c_int32 * len(ni.BLOCKS))(0, 1, 2, 5)
    assert call(*head[:3], past, *head[4:], 0, n_ops, arr, cf, ext, C.byref(tot), yp, None) == ERR_OUTOFRANGE
    # Y overlapping psi: psi is the tail of the buffer Y starts in
    buf = torch.zeros(n_out + ni.N_STATES - 1, dtype=torch.float64, device="cuda")
    tail = buf[n_out - 1:]
    head2, _, arr2, _, keep2 = _raw_args(sbm, 0, tail, ops)
    assert call(*head2, 0, n_ops, arr2, cf, ext, C.byref(tot), C.c_void_p(buf.data_ptr()), None) == ERR_ARG and b"overlap" in L.dmrgx_last_error()
    torch.cuda.synchronize()
    assert (Y == 7.0).all() and (buf == 0.0).all()
