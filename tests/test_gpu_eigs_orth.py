"""dmrgx_eigs_lowest_orth (-m gpu, csrc/eigs_orth.hip): the lowest eigenpair of P H P on the complement of given vectors, at tol 1e-10 and
ncv 16, at one to three workgroups of 2048 elements (845, 1205, 2049 -- the second workgroup holds one element -- and 4097 states).

References and bounds.  845 and 1205 states: the dense eigendecomposition H = V diag(w) V^T (the seven lowest gaps are >= 0.12 and
>= 0.34).  With Q = V[:, :nq] exactly, P H P has the eigenpair (w_nq, V_nq) as its lowest on the complement:
  |e - w_nq| <= tol |e| + 1e-12 ||H||                    (a Ritz value is within its residual of an eigenvalue; the floor is rounding)
  sin angle(psi, V_nq) <= r / delta + 1e-12               (Davis-Kahan; r = |H psi - e psi - Q Q^T H psi| recomputed in numpy, delta the
                                                           distance from e to the rest of the spectrum outside Q)
  |Q psi| <= 1e-12,  stats.residual <= tol |e|.
With Q taken from the library itself (rows found one after another) P is that of an inexact Q: a row q with residual r_q whose level is
g_q away from the nearest other level is within r_q / g_q of an exact eigenvector (a level that other levels approach within 1e-8 counts
with them: any vector of that eigenspace serves), which moves the eigenvalues of P H P by at most 4 ||H|| r_q / g_q:
  |e_k - w_k| <= tol |e_k| + 4 ||H|| sum_{q<k} r_q / g_q + 1e-12 ||H||.
2049 and 4097 states: Q = the plan's own ground state at tol 1e-12, and the residual of P H P recomputed through helpers.FactoredH,
within tol |e| (1 + 1e-6) + 1e-12 ||H||, ||H|| = 1.25 x the largest |Ritz value| of 60 reorthogonalised Lanczos steps."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                      # (the child process: pytest's conftest is not there to set the path)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import FactoredH, krylov_input, krylov_superblock, lanczos_reorth, lanczos_tridiag   # noqa: E402

pytestmark = pytest.mark.gpu
TOL, NCV = 1e-10, 16
DENSE = (845, 1205)
MIN_GAP = {845: 0.12, 1205: 0.34}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class _Context:
    def __init__(self, sbm, wl):
        self.sbm, self.wl, self._plans = sbm, wl, {}

    def plan(self, key):
        if key not in self._plans:
            sb = krylov_superblock(self.wl, key) if key in (2049, 4097) else krylov_input(self.wl, key)[0]
            self._plans[key] = self.sbm.KronPlan(sb)
        return self._plans[key]

    def close(self):
        for p in self._plans.values():
            p.destroy()


@pytest.fixture(scope="module")
def ctx(pkg):
    from dmrgx_amd import superblock, workloads, _capi
    _capi.require_device()
    c = _Context(superblock, workloads)
    yield c
    c.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _padded(Qh, pad, offset):
    """Q as a view of a NaN-filled store: row stride n + pad, first element `offset` doubles into the allocation."""
    nq, n = Qh.shape
    store = torch.full((offset + nq * (n + pad),), float("nan"), dtype=torch.float64, device="cuda")
    Qd = store[offset:].view(nq, n + pad)[:, :n]
    Qd.copy_(torch.from_numpy(Qh.copy()))
    assert Qd.data_ptr() % 16 == (8 * offset) % 16
    return store, Qd


def _php_residual(H, Qh, e, psi):
    """|H psi - e psi - Q Q^T H psi| with the rows of Qh orthonormalised in numpy"""
    Qo = np.linalg.qr(Qh.T)[0]
    hp = H @ psi
    return np.linalg.norm(hp - e * psi - Qo @ (Qo.T @ hp))


def _check_exact_q(w, V, H, nq, e, psi, stats):
    """The bounds of the module docstring for Q = V[:, :nq]"""
    hnorm = np.abs(w).max()
    Qh = V[:, :nq].T
    r = _php_residual(H, Qh, e, psi)
    delta = np.abs(w[nq + 1:] - e).min()
    v = V[:, nq]
    sin = np.linalg.norm(psi - v * (v @ psi))
    print("  nq", nq, "e", e, "w", w[nq], "|e - w|", abs(e - w[nq]), "r", r, "delta", delta, "sin", sin, "|Q psi|", np.abs(Qh @ psi).max(),
          "stats.residual", stats.residual, "matvecs", stats.n_matvec, "restarts", stats.n_restart)
    assert stats.converged == 1 and np.isfinite(psi).all()
    assert abs(e - w[nq]) <= TOL * abs(e) + 1e-12 * hnorm
    assert sin <= r / delta + 1e-12
    assert np.linalg.norm(Qh @ psi) <= 1e-12
    assert abs(np.linalg.norm(psi) - 1.0) <= 1e-13
    assert stats.residual <= TOL * abs(e)


@pytest.mark.parametrize("nq", [1, 3, 7])
@pytest.mark.parametrize("n", DENSE)
def test_exact_lower_states_as_q(ctx, n, nq):
    _, H, w, V = krylov_input(ctx.wl, n)
    assert np.diff(w[:8]).min() >= MIN_GAP[n]
    e, psi, stats = ctx.plan(n).eigs_lowest_orth(_dev(V[:, :nq].T), ncv=NCV, tol=TOL)
    _check_exact_q(w, V, H, nq, e, psi.cpu().numpy()[:n], stats)


def _chain(plan, n, count, seed=1):
    """rows 0 .. count-1 found one after another: eigs_lowest at tol 1e-12, then eigs_lowest_orth with the rows found so far"""
    rows = torch.empty((count, n), dtype=torch.float64, device="cuda")
    es, sts = [], []
    e0, psi, st = plan.eigs_lowest(tol=1e-12, seed=seed)
    rows[0].copy_(psi[:n]); es.append(e0); sts.append(st)
    for k in range(1, count):
        e, psi, st = plan.eigs_lowest_orth(rows[:k], ncv=NCV, tol=TOL, seed=seed + k)
        rows[k].copy_(psi[:n]); es.append(e); sts.append(st)
    return np.array(es), rows, sts


def _chain_bounds(H, w, es, rows):
    """tol |e_k| + 4 ||H|| sum_{q<k} r_q / g_q + 1e-12 ||H|| for every row k"""
    hnorm = np.abs(w).max()
    r = np.array([np.linalg.norm(H @ q - e * q) for e, q in zip(es, rows)])
    g = np.array([np.abs(w[np.abs(w - e) > 1e-8] - e).min() for e in es])
    return np.array([TOL * abs(es[k]) + 4.0 * hnorm * np.sum(r[:k] / g[:k]) + 1e-12 * hnorm for k in range(len(es))]), r, g


@pytest.mark.parametrize("n", DENSE)
def test_q_from_the_library_itself(ctx, n):
    _, H, w, V = krylov_input(ctx.wl, n)
    es, rows, sts = _chain(ctx.plan(n), n, 4)
    R = rows.cpu().numpy()
    bounds, r, g = _chain_bounds(H, w, es, R)
    print("n", n, "e", es, "w", w[:4], "|e - w|", np.abs(es - w[:4]), "bounds", bounds, "r", r, "g", g, "matvecs", [s.n_matvec for s in sts])
    assert all(s.converged == 1 for s in sts)
    assert (np.diff(es) > 0).all()
    assert (np.abs(es - w[:4]) <= bounds).all()
    assert np.abs(R @ R.T - np.eye(4)).max() <= 1e-12


def test_degenerate_ground_state_is_resolved(ctx):
    """'degenerate': a twofold ground state at exactly -3.5, the next level at -1.99973.  Q = the library's first ground vector: -3.5 again,
    orthogonal to it; both as Q: the third level."""
    _, H, w, V = krylov_input(ctx.wl, "degenerate")
    n = H.shape[0]
    assert abs(w[0] + 3.5) <= 1e-12 and abs(w[1] + 3.5) <= 1e-12 and abs(w[2] + 1.99973) <= 1e-5
    es, rows, sts = _chain(ctx.plan("degenerate"), n, 3)
    R = rows.cpu().numpy()
    bounds, r, g = _chain_bounds(H, w, es, R)
    print("e", es, "w", w[:3], "bounds", bounds, "r", r, "g", g, "overlaps", R @ R.T)
    assert all(s.converged == 1 for s in sts)
    assert (np.abs(es - w[:3]) <= bounds).all()
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12
    ground = V[:, :2]
    assert np.linalg.norm(R[1] - ground @ (ground.T @ R[1])) <= r[1] / g[1] + 1e-12      # the second vector lies in the ground space too


def test_tiny_gap_second_call_returns_the_upper_member(ctx):
    """'tinygap': a pair split by 1.2e-2, at -3.50897 and -3.49720"""
    _, H, w, V = krylov_input(ctx.wl, "tinygap")
    n = H.shape[0]
    assert abs(w[0] + 3.50897) <= 1e-5 and abs(w[1] + 3.49720) <= 1e-5
    es, rows, sts = _chain(ctx.plan("tinygap"), n, 2)
    bounds, r, g = _chain_bounds(H, w, es, rows.cpu().numpy())
    print("e", es, "w", w[:2], "bounds", bounds, "r", r, "g", g, "matvecs", [s.n_matvec for s in sts])
    assert sts[1].converged == 1 and abs(es[1] - w[1]) <= bounds[1]


def _range_case(sbm, wl, n):
    """Q = the plan's ground state, in a NaN-filled store with ldq = n + 3, 8 bytes off a 16-byte boundary -> (q, e0, e, psi, stats fields)"""
    plan = sbm.KronPlan(krylov_superblock(wl, n))
    e0, psi0, _ = plan.eigs_lowest(tol=1e-12)
    q = psi0.cpu().numpy()[:n].copy()
    store, Qd = _padded(q[None, :], 3, 1)
    e, psi, st = plan.eigs_lowest_orth(Qd, ncv=NCV, tol=TOL)
    again = plan.eigs_lowest_orth(Qd, ncv=NCV, tol=TOL)
    assert torch.isnan(store[:1]).all() and torch.isnan(store[1 + n:]).all() and np.array_equal(_bits(Qd.cpu().numpy()[0]), _bits(q))
    assert e == again[0] and np.array_equal(_bits(psi.cpu().numpy()), _bits(again[1].cpu().numpy()))
    assert (st.n_matvec, st.n_restart, st.converged, st.residual) == (again[2].n_matvec, again[2].n_restart, again[2].converged, again[2].residual)
    plan.destroy()
    return q, e0, e, psi.cpu().numpy()[:n].copy(), np.array([st.n_matvec, st.n_restart, st.converged, st.start_rejected, st.residual])


def _range_check(wl, n, q, e0, e, psi, scal):
    H = FactoredH(wl, krylov_superblock(wl, n))
    _, a, b = lanczos_reorth(H, np.random.default_rng(100 + n).standard_normal(n), 60)
    hnorm = 1.25 * np.abs(np.linalg.eigvalsh(lanczos_tridiag(a, b))).max()
    res = _php_residual(H, q[None, :], e, psi)
    bound = TOL * abs(e) * (1.0 + 1e-6) + 1e-12 * hnorm
    print("n", n, "e0", e0, "e", e, "residual through FactoredH", res, "bound", bound, "stats", scal, "|q psi|", abs(q @ psi))
    assert scal[2] == 1.0 and np.isfinite(psi).all() and np.isfinite(scal).all()
    assert res <= bound and scal[4] <= TOL * abs(e)
    assert e > e0 and abs(q @ psi) <= 1e-12 and abs(np.linalg.norm(psi) - 1.0) <= 1e-13


@pytest.mark.parametrize("n", [2049, 4097])
def test_ranges_with_a_padded_unaligned_q(ctx, n):
    _range_check(ctx.wl, n, *_range_case(ctx.sbm, ctx.wl, n))


def test_poisoned_workspace(ctx, tmp_path):
    """2049 states in a child process under DMRGX_POOL_POISON=1 (the basis, the work vectors, the partial sums and the coefficients come
    from the pool filled with NaN): converged, nothing NaN, the residual within its bound, and the bits of the clean run in this process."""
    from test_gpu_poison import _child
    q, e0, e, psi, scal = _range_case(ctx.sbm, ctx.wl, 2049)
    out = str(tmp_path / "poisoned.npz")
    pr = _child([os.path.join("tests", "test_gpu_eigs_orth.py"), out], True, 300)
    assert pr.returncode == 0 and "eigs orth child ok" in pr.stdout, pr.stdout[-2000:] + pr.stderr[-2000:]
    got = np.load(out)
    _range_check(ctx.wl, 2049, got["q"], float(got["e0"]), float(got["e"]), got["psi"], got["scal"])
    assert float(got["e"]) == e and np.array_equal(_bits(got["psi"]), _bits(psi)) and np.array_equal(_bits(got["scal"]), _bits(scal))


def test_no_row_forwards_to_eigs_lowest(ctx):
    plan, n = ctx.plan(845), 845
    e0, psi0, st0 = plan.eigs_lowest(ncv=NCV, tol=TOL, seed=5)
    e1, psi1, st1 = plan.eigs_lowest_orth(None, ncv=NCV, tol=TOL, seed=5)
    assert e0 == e1 and np.array_equal(_bits(psi0.cpu().numpy()), _bits(psi1.cpu().numpy()))
    assert (st0.n_matvec, st0.n_restart, st0.converged, st0.start_rejected, st0.residual) == (st1.n_matvec, st1.n_restart, st1.converged, st1.start_rejected, st1.residual)
    g = psi0 + 1e-3 * torch.from_numpy(np.random.default_rng(3).standard_normal(n)).cuda()
    a, b = plan.eigs_lowest(ncv=NCV, tol=TOL, psi0=g, method=0), plan.eigs_lowest_orth(None, ncv=NCV, tol=TOL, psi0=g)
    assert a[0] == b[0] and np.array_equal(_bits(a[1].cpu().numpy()), _bits(b[1].cpu().numpy())) and a[2].n_matvec == b[2].n_matvec


def test_two_runs_give_the_same_bits(ctx):
    _, H, w, V = krylov_input(ctx.wl, 1205)
    Qd = _dev(V[:, :3].T)
    a, b = ctx.plan(1205).eigs_lowest_orth(Qd, ncv=NCV, tol=TOL, seed=9), ctx.plan(1205).eigs_lowest_orth(Qd, ncv=NCV, tol=TOL, seed=9)
    assert a[0] == b[0] and np.array_equal(_bits(a[1].cpu().numpy()), _bits(b[1].cpu().numpy()))
    assert (a[2].n_matvec, a[2].n_restart, a[2].converged, a[2].residual) == (b[2].n_matvec, b[2].n_restart, b[2].converged, b[2].residual)


def test_start_vectors(ctx):
    """A start vector inside span(Q) is rejected and the run is that of the random start, bit for bit; a start vector close to the answer
    is used (fewer MatMults); min_initial_norm2 above the projected norm rejects."""
    n, nq = 845, 3
    _, H, w, V = krylov_input(ctx.wl, n)
    plan, Qd = ctx.plan(n), _dev(V[:, :nq].T)
    rnd = plan.eigs_lowest_orth(Qd, ncv=NCV, tol=TOL, seed=4)
    inside = plan.eigs_lowest_orth(Qd, ncv=NCV, tol=TOL, seed=4, psi0=_dev(0.6 * V[:, 0] - 0.8 * V[:, 2]))
    assert rnd[2].start_rejected == 0 and inside[2].start_rejected == 1
    assert inside[0] == rnd[0] and np.array_equal(_bits(inside[1].cpu().numpy()), _bits(rnd[1].cpu().numpy()))
    _check_exact_q(w, V, H, nq, inside[0], inside[1].cpu().numpy()[:n], inside[2])
    guess = V[:, nq] + 1e-3 * np.random.default_rng(8).standard_normal(n) + 0.5 * V[:, 1]
    near = plan.eigs_lowest_orth(Qd, ncv=NCV, tol=TOL, seed=4, psi0=_dev(guess))
    print("matvecs: random start", rnd[2].n_matvec, "near start", near[2].n_matvec)
    assert near[2].start_rejected == 0 and near[2].n_matvec < rnd[2].n_matvec
    _check_exact_q(w, V, H, nq, near[0], near[1].cpu().numpy()[:n], near[2])
    light = plan.eigs_lowest_orth(Qd, ncv=NCV, tol=TOL, seed=4, psi0=_dev(guess), min_initial_norm2=10.0)
    assert light[2].start_rejected == 1 and light[0] == rnd[0]
    for bad in (np.zeros(n), np.full(n, np.nan)):
        out = plan.eigs_lowest_orth(Qd, ncv=NCV, tol=TOL, seed=4, psi0=_dev(bad))
        assert out[2].start_rejected == 1 and out[0] == rnd[0]


def test_krylov_space_ends_at_the_complement(ctx):
    """nq = n_states - 3 on the 845 input: ncv 16 is cut to 3, the answer is exact after three MatMults and converged"""
    n = 845
    _, H, w, V = krylov_input(ctx.wl, n)
    nq = n - 3
    e, psi, stats = ctx.plan(n).eigs_lowest_orth(_dev(V[:, :nq].T), ncv=NCV, tol=TOL)
    psi = psi.cpu().numpy()[:n]
    v = V[:, nq]
    print("e", e, "w", w[nq], "matvecs", stats.n_matvec, "sin", np.linalg.norm(psi - v * (v @ psi)), "|Q psi|", np.linalg.norm(V[:, :nq].T @ psi))
    assert stats.converged == 1 and stats.n_matvec <= 3
    # 842 rows orthonormalised on the device: the floors are those of the sums over 842 rows, 1e-12 ||H|| and 1e-11 for the angle
    assert abs(e - w[nq]) <= 1e-12 * np.abs(w).max()
    assert np.linalg.norm(psi - v * (v @ psi)) <= 1e-11 / np.diff(w[nq:]).min()
    assert np.linalg.norm(V[:, :nq].T @ psi) <= 1e-12


def test_not_converged_returns_the_last_iterate(ctx):
    from dmrgx_amd import _capi as capi
    n = 1205
    _, H, w, V = krylov_input(ctx.wl, n)
    plan, Qd = ctx.plan(n), _dev(V[:, :2].T)
    opts = capi.EigsOpts()
    opts.ncv, opts.max_it, opts.tol, opts.seed = 4, 1, 1e-14, 1
    e, stats = C.c_double(0.0), capi.EigsStats()
    psi = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    rc = capi.lib().dmrgx_eigs_lowest_orth(plan._handle, C.byref(opts), 2, C.c_void_p(Qd.data_ptr()), n, C.byref(e), C.c_void_p(psi.data_ptr()), C.byref(stats), plan._stream_ptr(None))
    ph = psi.cpu().numpy()
    assert rc == capi.DMRGX_ERR_NOTCONV and "not converged" in capi.lib().dmrgx_last_error().decode()
    assert stats.converged == 0 and stats.n_matvec == 4 and stats.n_restart == 1 and np.isfinite(ph).all()
    assert abs(np.linalg.norm(ph) - 1.0) <= 1e-13 and np.linalg.norm(V[:, :2].T @ ph) <= 1e-12 and e.value >= w[2] - 1e-12 * np.abs(w).max()


def test_refusals(ctx):
    from dmrgx_amd import _capi as capi
    ERR_ARG = capi.DMRGX_ERR_ARG
    n = 845
    _, H, w, V = krylov_input(ctx.wl, n)
    plan = ctx.plan(n)
    lib, st = capi.lib(), plan._stream_ptr(None)
    good = _dev(V[:, :3].T)
    psi = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    e, stats = C.c_double(7.0), capi.EigsStats()
    null = C.c_void_p()

    def call(plan_=plan._handle, nq=3, Q=None, ldq=n, e_=C.byref(e), psi_=C.c_void_p(psi.data_ptr()), **kw):
        opts = capi.EigsOpts()
        opts.ncv, opts.tol = NCV, TOL
        for k, v in kw.items():
            setattr(opts, k, v)
        rc = lib.dmrgx_eigs_lowest_orth(plan_, C.byref(opts), nq, C.c_void_p((good if Q is None else Q).data_ptr()) if Q is not False else null, ldq, e_, psi_, C.byref(stats), st)
        return rc, lib.dmrgx_last_error().decode()

    zero_row, nan_row, dep = V[:, :3].T.copy(), V[:, :3].T.copy(), V[:, :3].T.copy()
    zero_row[1] = 0.0
    nan_row[2, 77] = np.nan
    dep[2] = 0.3 * dep[0] - 2.0 * dep[1] + 1e-12 * V[:, 5]
    hook = capi.ALLGATHER_FN(lambda *a: 0)
    cases = {
        "null plan": (dict(plan_=null), "null"), "null e": (dict(e_=C.POINTER(C.c_double)()), "null"), "null psi": (dict(psi_=null), "null"),
        "negative nq": (dict(nq=-1), "nq"), "null Q": (dict(Q=False), "Q is null"), "ldq": (dict(ldq=n - 1), "ldq"),
        "zero row": (dict(Q=_dev(zero_row)), "row 1 of Q is zero"), "nan row": (dict(Q=_dev(nan_row)), "row 2 of Q is zero or not finite"),
        "dependent row": (dict(Q=_dev(dep)), "row 2 of Q is linearly dependent"),
        "nq = n": (dict(nq=n, Q=torch.zeros((n, n), dtype=torch.float64, device="cuda")), "no complement"),
        "allgather": (dict(allgather=hook), "collectives"), "allreduce": (dict(allreduce_sum=capi.ALLREDUCE_FN(lambda *a: 0)), "collectives"),
        "comm": (dict(comm=8), "collectives"), "max_matvec": (dict(max_matvec=5), "max_matvec"),
    }
    for what, (kw, word) in cases.items():
        rc, msg = call(**kw)
        assert rc == ERR_ARG and word in msg, (what, rc, msg)
    assert torch.isnan(psi).all() and e.value == 7.0                        # nothing was written
    rc, msg = lib.dmrgx_eigs_lowest_orth(plan._handle, None, 3, C.c_void_p(good.data_ptr()), n, C.byref(e), C.c_void_p(psi.data_ptr()), C.byref(stats), st), lib.dmrgx_last_error().decode()
    assert rc == ERR_ARG and "null" in msg
    assert call()[0] == 0 and abs(e.value - w[3]) <= TOL * abs(w[3]) + 1e-12 * np.abs(w).max()      # `method` is ignored: method 1 too
    assert call(method=1)[0] == 0
    striped = ctx.sbm.KronPlan(krylov_input(ctx.wl, 845)[0], world_size=2, rank=0)
    rc, msg = call(plan_=striped._handle)
    assert rc == ERR_ARG and "striped" in msg
    striped.destroy()


if __name__ == "__main__":
    from __graft_entry__ import load_package
    load_package()
    from dmrgx_amd import superblock as sbm_child, workloads as wl_child
    assert os.environ.get("DMRGX_POOL_POISON") == "1"
    q_c, e0_c, e_c, psi_c, scal_c = _range_case(sbm_child, wl_child, 2049)
    np.savez(sys.argv[1], q=q_c, e0=e0_c, e=e_c, psi=psi_c, scal=scal_c)
    print("eigs orth child ok")
