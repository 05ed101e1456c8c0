"""dmrgx_vec_project_out (-m gpu, csrc/project_out.hip) through superblock.vec_project_out: coef[a] = <v_a, p> / <p, p>, v_a -= coef[a] p for
a family of rows, against numpy in extended precision.  Every bound is derived (u = 2^-53, |.| the 2-norm), none is measured:
  coefficients       |coef[a] - c_ref[a]| <= (2 len + 2) u |v_a| |p| / |p|^2: the dot contributes len u |v_a| |p|, the norm len u relatively,
                     the division u
  updated rows       |v'_e - (v_e - coef[a] p_e)| <= 2u (|v_e| + |coef[a] p_e|), with the coefficient the device returned: one product, one
                     difference
  remaining overlap  |<v'_a, p>| <= (len + 8) u |v_a| |p|
  planted row        the row stored as 3 p: |coef - 3| <= 4u (one spacing of the doubles at 3) and every element within 4u |p_e| of zero.
                     The row is fl(3 p_e), not 3 p_e: what is left of it is the rounding of its own elements, at most 3u |p_e|, only if the
                     coefficient is 3.0 itself -- one spacing off, it keeps 4u |p_e| of p on top.  The exact quotient of the exact sums is
                     3 (1 + d) with d the p_e^2-weighted mean of those element roundings, |d| <= u: it rounds to 3.0 unless len is 1 or 2.
Lengths at the edges of the 2048-element ranges, row counts on both sides of a wave (33 rows: more than the 16 waves of the coefficient
stage), leading dimensions len, len + 1 (odd or even) and len + 3.

Run as a script (`test_gpu_project_out.py OUT.npz`) this file is the child of the poisoned-workspace test."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                      # (the child process: pytest's conftest is not there to set the path)
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
ERR_ARG = 62
U = 2.0 ** -53
LENS = [1, 2, 7, 2047, 2048, 2049, 4097, 6147]
NVS = [1, 2, 5, 33]
SENTINEL = -6.02214076e+123
LD = np.longdouble
POISON_CASE = (6147, 5)


@pytest.fixture(scope="module")
def mods(pkg):
    from dmrgx_amd import superblock, _capi
    _capi.require_device()
    return superblock, _capi


def _case(n, nv):
    """-> (V [nv][n], p [n], planted row): fixed-seed normal data, row `planted` stored as 3 p."""
    rng = np.random.default_rng(1000 * n + nv)
    p = rng.standard_normal(n)
    V = rng.standard_normal((nv, n))
    planted = nv // 2
    V[planted] = 3.0 * p
    return V, p, planted


def _device(V, p, ldv, v_off=0, p_off=0):
    """The family in a buffer of nv + 1 rows of ldv doubles, v_off doubles into its allocation: columns [n, ldv) and the row after the
    family hold the sentinel.  -> (the whole buffer, the (nv, n) view of it, p on the device p_off doubles into its allocation)"""
    import torch
    nv, n = V.shape
    host = np.full((nv + 1, ldv), SENTINEL)
    host[:nv, :n] = V
    flat = torch.full((v_off + (nv + 1) * ldv,), SENTINEL, dtype=torch.float64, device="cuda")
    flat[v_off:] = torch.from_numpy(host.ravel()).cuda()
    view = torch.as_strided(flat, (nv, n), (ldv, 1), v_off)
    pd = torch.zeros(p_off + n, dtype=torch.float64, device="cuda")
    pd[p_off:] = torch.from_numpy(p).cuda()
    return flat, view, pd[p_off:]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check(V, p, planted, coef, Vout, norm2, rows=None):
    """The four bounds of the module docstring on the rows `rows` (default: all)."""
    nv, n = V.shape
    pl, Vl = p.astype(LD), V.astype(LD)
    pp = pl @ pl
    pn = np.sqrt(pp)
    assert abs(LD(norm2) - pp) <= (n + 1) * U * pp
    for a in (range(nv) if rows is None else rows):
        vn = np.sqrt(Vl[a] @ Vl[a])
        c_ref = (Vl[a] @ pl) / pp
        err_c = abs(LD(coef[a]) - c_ref)
        want = Vl[a] - LD(coef[a]) * pl
        err_v = np.abs(Vout[a].astype(LD) - want) - 2 * U * (np.abs(Vl[a]) + np.abs(LD(coef[a]) * pl))
        overlap = abs(Vout[a].astype(LD) @ pl)
        assert err_c <= (2 * n + 2) * U * vn * pn / pp, (n, nv, a, float(err_c / U))
        assert err_v.max() <= 0.0, (n, nv, a, float(err_v.max() / U))
        assert overlap <= (n + 8) * U * vn * pn, (n, nv, a, float(overlap / U))
    if planted is not None and (rows is None or planted in rows):
        left = np.abs(Vout[planted]) / np.abs(p)
        print("planted row: coef - 3 =", (coef[planted] - 3.0) / U, "u; max |v'_e| / |p_e| =", left.max() / U, "u")
        assert abs(coef[planted] - 3.0) <= 4 * U
        assert (np.abs(Vout[planted]) <= 4 * U * np.abs(p)).all()


@pytest.mark.parametrize("nv", NVS)
@pytest.mark.parametrize("n", LENS)
def test_against_extended_precision(mods, n, nv):
    """ldv = len, len + 1 and len + 3: the bounds, the sentinel columns [len, ldv) and the sentinel row after the family bit for bit, and
    a second call on a copy of the input with the same bits in coef and V."""
    sbm, _ = mods
    V, p, planted = _case(n, nv)
    for ldv in (n, n + 1, n + 3):
        flat, view, pd = _device(V, p, ldv)
        before = flat.cpu().numpy().reshape(nv + 1, ldv)
        coef, norm2 = sbm.vec_project_out(view, pd)
        after = flat.cpu().numpy().reshape(nv + 1, ldv)
        _check(V, p, planted, coef, after[:nv, :n], norm2)
        assert np.array_equal(_bits(after[:nv, n:]), _bits(before[:nv, n:])) and np.array_equal(_bits(after[nv]), _bits(before[nv]))
        assert np.array_equal(pd.cpu().numpy(), p)
        flat2, view2, pd2 = _device(V, p, ldv)
        coef2, norm2_2 = sbm.vec_project_out(view2, pd2)
        assert np.array_equal(_bits(coef), _bits(coef2)) and norm2 == norm2_2
        assert np.array_equal(_bits(flat2.cpu().numpy()), _bits(after.ravel()))


@pytest.mark.parametrize("n,nv", [(2049, 5), (6147, 2), (7, 33)])
def test_unaligned_pointers(mods, n, nv):
    """V and p each one double off a 16-byte boundary, in all four combinations, with an odd ldv: the 8-byte path.  The same bounds (the
    bits need not be those of the aligned case); the double before the family and everything after it stay as they were."""
    sbm, _ = mods
    V, p, planted = _case(n, nv)
    ldv = n + 1 if n % 2 == 0 else n + 2
    assert ldv % 2 == 1
    for v_off in (0, 1):
        for p_off in (0, 1):
            flat, view, pd = _device(V, p, ldv, v_off, p_off)
            assert view.data_ptr() % 16 == 8 * v_off and pd.data_ptr() % 16 == 8 * p_off
            before = flat.cpu().numpy()
            coef, norm2 = sbm.vec_project_out(view, pd)
            after = flat.cpu().numpy()
            rows = after[v_off:].reshape(nv + 1, ldv)
            _check(V, p, planted, coef, rows[:nv, :n], norm2)
            assert np.array_equal(_bits(after[:v_off]), _bits(before[:v_off]))
            assert np.array_equal(_bits(rows[:nv, n:]), _bits(before[v_off:].reshape(nv + 1, ldv)[:nv, n:])) and (rows[nv] == SENTINEL).all()


@pytest.mark.parametrize("n", [7, 4097])
def test_degenerate_p_leaves_everything_alone(mods, n):
    """p = 0 and a p with one NaN: DMRGX_OK, V bit-identical to its input, every coef 0, p_norm2 == 0."""
    sbm, _ = mods
    V, p, _ = _case(n, 5)
    nan_p = p.copy()
    nan_p[n // 2] = np.nan
    for bad in (np.zeros(n), nan_p):
        flat, view, pd = _device(V, bad, n + 1)
        before = flat.cpu().numpy()
        coef, norm2 = sbm.vec_project_out(view, pd)
        assert np.array_equal(_bits(coef), _bits(np.zeros(5))) and norm2 == 0.0
        assert np.array_equal(_bits(flat.cpu().numpy()), _bits(before))


@pytest.mark.parametrize("n", [7, 4097])
def test_a_row_that_is_not_finite_is_left_alone(mods, n):
    """Row 1 holds a NaN, row 3 an infinity: both come back bit for bit with coef 0; rows 0, 2 (planted) and 4 meet the bounds."""
    sbm, _ = mods
    V, p, planted = _case(n, 5)
    assert planted == 2
    V[1, n - 1] = np.nan
    V[3, 0] = np.inf
    flat, view, pd = _device(V, p, n + 3)
    coef, norm2 = sbm.vec_project_out(view, pd)
    out = flat.cpu().numpy().reshape(6, n + 3)[:5, :n]
    assert coef[1] == 0.0 and coef[3] == 0.0
    assert np.array_equal(_bits(out[1]), _bits(V[1])) and np.array_equal(_bits(out[3]), _bits(V[3]))
    _check(V, p, planted, coef, out, norm2, rows=[0, 2, 4])


def test_refusals_and_the_empty_family(mods):
    """DMRGX_ERR_ARG for a null pointer (each of the four), nv < 1, len < 0, ldv < len and p overlapping V (inside a row, and only in the last
    row's last element); len == 0 is DMRGX_OK with zero coefficients, p_norm2 == 0 and nothing touched."""
    import torch
    _, capi = mods
    lib = capi.lib()
    n, nv, ldv = 100, 3, 104
    Vd = torch.full((nv * ldv,), 1.5, dtype=torch.float64, device="cuda")
    pd = torch.full((n,), 2.0, dtype=torch.float64, device="cuda")
    coef, norm2 = (C.c_double * nv)(7.0, 7.0, 7.0), C.c_double(7.0)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + 8 * off)        # noqa: E731

    def call(nv_=nv, n_=n, V_=ptr(Vd), ldv_=ldv, p_=ptr(pd), coef_=coef, norm2_=C.byref(norm2)):
        return lib.dmrgx_vec_project_out(nv_, n_, V_, ldv_, p_, coef_, norm2_, None)

    for bad in (dict(V_=C.c_void_p()), dict(p_=C.c_void_p()), dict(coef_=None), dict(norm2_=None), dict(nv_=0), dict(nv_=-1), dict(n_=-1),
                dict(ldv_=n - 1), dict(p_=ptr(Vd, ldv + 10)), dict(p_=ptr(Vd, 2 * ldv + n - 1)), dict(V_=ptr(pd, n - 1), nv_=1)):
        assert call(**bad) == ERR_ARG, bad
        assert (Vd.cpu().numpy() == 1.5).all()
    # p right behind the last row's elements, inside the family's allocation: no overlap
    assert call(n_=50, p_=ptr(Vd, 2 * ldv + 50)) == 0
    Vd.fill_(1.5)
    assert call(n_=0) == 0
    assert list(coef) == [0.0] * nv and norm2.value == 0.0 and (Vd.cpu().numpy() == 1.5).all() and (pd.cpu().numpy() == 2.0).all()


def _run_poison_case(sbm):
    V, p, planted = _case(*POISON_CASE)
    flat, view, pd = _device(V, p, POISON_CASE[0] + 1)
    coef, norm2 = sbm.vec_project_out(view, pd)
    return V, p, planted, coef, flat.cpu().numpy(), norm2


def test_poisoned_workspace(mods, tmp_path):
    """len 6147, nv 5 in a child process under DMRGX_POOL_POISON=1 (the partial sums and the coefficients come from the pool filled with
    NaN): the same bounds, and the bits of the clean run in this process."""
    from test_gpu_poison import _child
    sbm, _ = mods
    V, p, planted, coef, flat, norm2 = _run_poison_case(sbm)
    out = str(tmp_path / "poisoned.npz")
    pr = _child([os.path.join("tests", "test_gpu_project_out.py"), out], True, 300)
    assert pr.returncode == 0 and "project out child ok" in pr.stdout, pr.stdout[-2000:] + pr.stderr[-2000:]
    got = np.load(out)
    n, nv = POISON_CASE
    _check(V, p, planted, got["coef"], got["flat"].reshape(nv + 1, n + 1)[:nv, :n], float(got["norm2"]))
    assert np.array_equal(_bits(got["coef"]), _bits(coef)) and np.array_equal(_bits(got["flat"]), _bits(flat)) and float(got["norm2"]) == norm2


if __name__ == "__main__":
    from __graft_entry__ import load_package
    load_package()
    from dmrgx_amd import superblock as sbm_child
    assert os.environ.get("DMRGX_POOL_POISON") == "1"
    _, _, _, coef_c, flat_c, norm2_c = _run_poison_case(sbm_child)
    np.savez(sys.argv[1], coef=coef_c, flat=flat_c, norm2=norm2_c)
    print("project out child ok")
