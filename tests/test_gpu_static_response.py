"""dmrgx_kron_static_response (-m gpu, csrc/response.hip): X with <p, X> = 0 and Q (H - sigma) Q X = Q v0, Q = 1 - p p^T / <p, p>, by a
device-resident conjugate-gradient run on the complement of p, at one to three workgroups of 2048 elements (845, 1205, 2049 -- the second
workgroup holds one element -- and 4097 states), with nu = 0, 1 and 13 vectors u_i (u_0 = v0) for the overlaps chi_i = <u_i, X>.

References.  845 and 1205 states: the dense eigendecomposition H = V diag(w) V^T, p = V[:, 0], sigma = w_0, gives
x* = sum_{n>0} V_n <V_n, v0> / (w_n - w_0).  2049 and 4097 states: p and sigma from the plan's own lowest eigenpair at tol 1e-12, and the
residual |Q v0 - Q (H - sigma) Q X| / |Q v0| of the returned X recomputed in numpy through helpers.FactoredH.

Bounds, from lambda_min(A) >= gap = w_1 - w_0 on the complement of p, with rho = true_residual, the call's own |b - A X| / |b|:
X - x* = A^-1 (A X - b) gives |X - x*| <= |Q v0| rho / gap and |chi_i - <u_i, x*>| <= |u_i| |Q v0| rho / gap; a floor of 1e-10 |Q v0| / gap
(times |u_i|) is added for the rounding of the reference and of the sums.  |<p, X>| <= 1e-12 |p| |X|; chi against U @ X of the returned X:
1e-12 |u| |X| -- the Gram kernel's summation order over at most 4097 terms; coef and norm2 to 1e-12 relative.  The factored residual:
tol (1 + 1e-6) + 1e-12 (||H|| + |sigma|) |X| / |Q v0|, ||H|| = 1.25 x the largest |Ritz value| of 60 reorthogonalised Lanczos steps.

Iteration counts of a numpy restatement at tol 1e-10: 64, 33 (dense), 54, 67 (dense H of the factored inputs, p = V[:, 0]); the counts
here are printed, not pinned -- they move by a few with the summation order."""
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
NU_MAX = 13
TOL, MAX_IT = 1e-10, 600
DENSE = (845, 1205)
SIZES = (845, 1205, 2049, 4097)
POISON_CASE = (2049, 5)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class _Context:
    """Per size: the plan, p, sigma, v0 and U (u_0 = v0), the gap (dense) and ||H|| -- all built once, read-only."""

    def __init__(self, sbm, wl):
        self.sbm, self.wl, self._plans, self._cases = sbm, wl, {}, {}

    def plan(self, n):
        if n not in self._plans:
            self._plans[n] = self.sbm.KronPlan(krylov_input(self.wl, n)[0] if n in DENSE else krylov_superblock(self.wl, n))
        return self._plans[n]

    def case(self, n):
        if n in self._cases:
            return self._cases[n]
        rng = np.random.default_rng(100 + n)
        v0 = rng.standard_normal(n)
        U = rng.standard_normal((NU_MAX, n))
        U[0] = v0
        if n in DENSE:
            _, H, w, V = krylov_input(self.wl, n)
            p, sigma, gap, hnorm = np.array(V[:, 0]), float(w[0]), float(w[1] - w[0]), np.abs(w).max()
        else:
            H = FactoredH(self.wl, krylov_superblock(self.wl, n))
            e0, psi, stats = self.plan(n).eigs_lowest(tol=1e-12)
            p, sigma, gap, w, V = psi.cpu().numpy()[:n].copy(), float(e0), None, None, None
            _, a, b = lanczos_reorth(H, v0, 60)
            hnorm = 1.25 * np.abs(np.linalg.eigvalsh(lanczos_tridiag(a, b))).max()
        out = dict(v0=v0, U=U, H=H, w=w, V=V, p=p, sigma=sigma, gap=gap, hnorm=hnorm)
        for a in (v0, U, p):
            a.setflags(write=False)
        self._cases[n] = out
        return out

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


def _padded(Uh, n, pad, offset):
    """U as a view of a NaN-filled store: row stride n + pad, first element `offset` doubles into the allocation."""
    nu = Uh.shape[0]
    store = torch.full((offset + nu * (n + pad),), float("nan"), dtype=torch.float64, device="cuda")
    Ud = store[offset:].view(nu, n + pad)[:, :n]
    Ud.copy_(torch.from_numpy(Uh.copy()))
    assert Ud.data_ptr() % 16 == (8 * offset) % 16 and Ud.stride(0) == n + pad
    return store, Ud


def _odd(h):
    """-> (store, view): the vector 8 bytes into a 16-byte aligned NaN-filled allocation, one NaN behind it"""
    n = len(h)
    store = torch.full((n + 2,), float("nan"), dtype=torch.float64, device="cuda")
    view = store[1:n + 1]
    view.copy_(torch.from_numpy(np.array(h)))
    assert view.data_ptr() % 16 == 8
    return store, view


def _blocks(iterations, check_every):
    return max(1, -(-iterations // check_every))


def _same_bits(a, b):
    assert np.array_equal(_bits(a["X"].cpu().numpy()), _bits(b["X"].cpu().numpy())), "X"
    assert np.array_equal(_bits(a["chi"]), _bits(b["chi"])), "chi"
    for k in ("coef", "norm2", "iterations", "converged", "dead", "residual", "true_residual"):
        assert a[k] == b[k], (k, a[k], b[k])


def _project(p, v):
    return v - (p @ v) / (p @ p) * p


def _residual(H, p, X, v0, sigma):
    """|Q v0 - Q (H - sigma) Q X| / |Q v0| in numpy"""
    b, x = _project(p, v0), _project(p, X)
    return np.linalg.norm(b - _project(p, H @ x - sigma * x)) / np.linalg.norm(b)


def _exact(cs, v0):
    """x* = sum_{n>0} V_n <V_n, v0> / (w_n - w_0) of a dense case"""
    w, V = cs["w"], cs["V"]
    return V[:, 1:] @ ((V[:, 1:].T @ v0) / (w[1:] - w[0]))


@pytest.mark.parametrize("nu", [0, 1, 13], ids=lambda nu: "nu%d" % nu)
@pytest.mark.parametrize("n", SIZES, ids=lambda n: "n%d" % n)
def test_response_to_a_random_vector(ctx, n, nu):
    """Every case converges within 600 iterations to tol 1e-10; X, chi, coef and norm2 within the bounds of the module docstring; n_matvec =
    blocks 8 + 1; the same call twice gives the same bits; p, v0 and U are bitwise unchanged and the NaN store round U is still NaN
    (nu = 13: ldu = n + 1 and U 8 bytes into a 16-byte aligned allocation; at n = 2049 X and p sit 8 bytes into theirs as well, and the
    doubles before and behind them keep their NaN)."""
    cs, plan = ctx.case(n), ctx.plan(n)
    v0, Uh, H, p, sigma = cs["v0"], cs["U"][:nu], cs["H"], cs["p"], cs["sigma"]
    pad = offset = 1 if nu == 13 else 0
    odd = nu == 13 and n == 2049
    v0d = torch.from_numpy(v0.copy()).cuda()
    pstore, pd = _odd(p) if odd else (None, torch.from_numpy(p.copy()).cuda())
    store, Ud = _padded(Uh, n, pad, offset) if nu else (None, None)
    xstore = [torch.full((n + 2,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2)] if odd else None
    out = plan.static_response(pd, v0d, sigma, tol=TOL, max_it=MAX_IT, U=Ud, X=xstore[0][1:n + 1] if odd else None)
    again = plan.static_response(pd, v0d, sigma, tol=TOL, max_it=MAX_IT, U=Ud, X=xstore[1][1:n + 1] if odd else None)
    X = out["X"].cpu().numpy()
    b = _project(p, v0)
    nb, nX, nuU = np.linalg.norm(b), np.linalg.norm(X), np.linalg.norm(Uh, axis=1)
    rho = out["true_residual"]
    print("n", n, "nu", nu, "iterations", out["iterations"], "n_matvec", out["n_matvec"], "residual", out["residual"], "true_residual", rho)
    assert out["converged"] == 1 and out["dead"] == 0 and 1 <= out["iterations"] <= MAX_IT
    assert out["n_matvec"] == _blocks(out["iterations"], 8) * 8 + 1
    assert out["residual"] <= TOL * (1.0 + 1e-12) and np.isfinite(rho)
    want_coef = (p @ v0) / (p @ p)
    print("  coef", out["coef"], want_coef, "norm2", out["norm2"], b @ b)
    assert abs(out["coef"] - want_coef) <= 1e-12 * abs(want_coef)
    assert abs(out["norm2"] - b @ b) <= 1e-12 * (b @ b)
    assert np.isfinite(X).all() and out["chi"].shape == (nu,)
    print("  <p, X> / |p| |X|", abs(p @ X) / (np.linalg.norm(p) * nX))
    assert abs(p @ X) <= 1e-12 * np.linalg.norm(p) * nX
    if n in DENSE:
        xs = _exact(cs, v0)
        bound = nb * rho / cs["gap"] + 1e-10 * nb / cs["gap"]
        print("  |X - x*|", np.linalg.norm(X - xs), "bound", bound)
        assert np.linalg.norm(X - xs) <= bound
        if nu:
            ob = nuU * nb * rho / cs["gap"] + 1e-10 * nuU * nb / cs["gap"]
            assert (np.abs(out["chi"] - Uh @ xs) <= ob).all(), np.abs(out["chi"] - Uh @ xs) / ob
    else:
        res = _residual(H, p, X, v0, sigma)
        bound = TOL * (1.0 + 1e-6) + 1e-12 * (cs["hnorm"] + abs(sigma)) * nX / nb
        print("  |Q v0 - Q (H - sigma) Q X| / |Q v0| through FactoredH", res, "bound", bound)
        assert res <= bound
    if nu:
        assert (np.abs(out["chi"] - Uh @ X) <= 1e-12 * nuU * nX).all()
        assert np.array_equal(_bits(Ud.cpu().numpy()), _bits(Uh))
        assert torch.isnan(store[:offset]).all() and (pad == 0 or torch.isnan(store[offset:].view(nu, n + pad)[:, n:]).all())
    assert np.array_equal(_bits(v0d.cpu().numpy()), _bits(v0)) and np.array_equal(_bits(pd.cpu().numpy()), _bits(p))
    if odd:
        assert torch.isnan(pstore[[0, n + 1]]).all() and all(torch.isnan(s[[0, n + 1]]).all() for s in xstore)
        aligned = plan.static_response(torch.from_numpy(p.copy()).cuda(), v0d, sigma, tol=TOL, max_it=MAX_IT, U=Ud)
        _same_bits(out, aligned)                                             # the 8-byte path of the direction kernel: the bits of the aligned call
    _same_bits(out, again)


@pytest.mark.parametrize("n", [845, 2049], ids=lambda n: "n%d" % n)
def test_results_do_not_depend_on_check_every(ctx, n):
    """check_every 1 (the host looks after every iteration), 8 and 50 (frozen iterations follow convergence) give the same bits in X, chi,
    coef, norm2, iterations and both residuals; only n_matvec differs, blocks check_every + 1."""
    cs, plan = ctx.case(n), ctx.plan(n)
    pd, v0d, Ud = torch.from_numpy(cs["p"].copy()).cuda(), torch.from_numpy(cs["v0"].copy()).cuda(), torch.from_numpy(cs["U"][:3].copy()).cuda()
    outs = {ce: plan.static_response(pd, v0d, cs["sigma"], tol=TOL, max_it=MAX_IT, check_every=ce, U=Ud) for ce in (1, 8, 50)}
    for ce, o in outs.items():
        print("n", n, "check_every", ce, "iterations", o["iterations"], "n_matvec", o["n_matvec"])
        assert o["converged"] == 1 and o["n_matvec"] == _blocks(o["iterations"], ce) * ce + 1
        _same_bits(outs[8], o)
    assert outs[1]["n_matvec"] == outs[1]["iterations"] + 1
    default = plan.static_response(pd, v0d, cs["sigma"], tol=TOL, max_it=MAX_IT, U=Ud)      # check_every 0 is 8
    assert default["n_matvec"] == outs[8]["n_matvec"]
    _same_bits(outs[8], default)


def test_a_component_along_p_is_returned_as_the_coefficient(ctx):
    """v0 = 3 p + 1e-3 z with z orthogonal to p (845 states): coef = 3 to 1e-13, norm2 = 1e-6 |z|^2 to 1e-9 relative (what the rounding of
    3 p leaves), and X equals the solve from 1e-3 z alone within the sum of the two bounds |Q v0| rho / gap, floors included."""
    n = 845
    cs, plan = ctx.case(n), ctx.plan(n)
    p = cs["p"]
    z = _project(p, cs["U"][1])
    z = _project(p, z)
    pd = torch.from_numpy(p.copy()).cuda()
    a = plan.static_response(pd, torch.from_numpy(3.0 * p + 1e-3 * z).cuda(), cs["sigma"], tol=TOL, max_it=MAX_IT)
    b = plan.static_response(pd, torch.from_numpy(1e-3 * z).cuda(), cs["sigma"], tol=TOL, max_it=MAX_IT)
    nz = 1e-3 * np.linalg.norm(z)
    bound = nz * (a["true_residual"] + b["true_residual"] + 2e-10) / cs["gap"]
    diff = np.linalg.norm(a["X"].cpu().numpy() - b["X"].cpu().numpy())
    print("coef", a["coef"], "coef of z alone", b["coef"], "norm2", a["norm2"], nz * nz, "|X_a - X_b|", diff, "bound", bound, "iterations", a["iterations"], b["iterations"])
    assert a["converged"] == 1 and b["converged"] == 1
    assert abs(a["coef"] - 3.0) <= 1e-13 and abs(b["coef"]) <= 1e-13
    assert abs(a["norm2"] - nz * nz) <= 1e-9 * nz * nz
    assert diff <= bound
    assert np.linalg.norm(a["X"].cpu().numpy() - 1e-3 * _exact(cs, z)) <= nz * (a["true_residual"] + 1e-10) / cs["gap"]


def test_multiples_of_p_and_a_zero_p(ctx):
    """v0 = p and v0 = -2.5 p: norm2 <= 1e-24 <v0, v0>, X -- NaN on entry -- exact zeros, chi 0, iterations 0, converged 1, dead 0, coef 1
    (exactly: the two sums are the same sum) and -2.5 to 1e-14 (two sums of 2049 terms through at most 20 additions each, 40 u x 2.5).  p = 0, and a p with one NaN: dead 1, converged 0, coef = norm2 = 0,
    zeros, nothing NaN.  One frozen block and the closing MatMult: n_matvec 9."""
    n = 2049
    cs, plan = ctx.case(n), ctx.plan(n)
    p = cs["p"]
    Ud = torch.from_numpy(cs["U"][:3].copy()).cuda()
    pd = torch.from_numpy(p.copy()).cuda()
    for scale in (1.0, -2.5):
        for U in (None, Ud):
            X = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            out = plan.static_response(pd, torch.from_numpy(scale * p).cuda(), cs["sigma"], U=U, X=X)
            print("v0 =", scale, "p: coef", out["coef"], "norm2", out["norm2"])
            assert (out["iterations"], out["converged"], out["dead"], out["n_matvec"]) == (0, 1, 0, 9)
            assert (out["coef"] == 1.0 if scale == 1.0 else abs(out["coef"] - scale) <= 1e-14) and 0.0 <= out["norm2"] <= 1e-24 * scale * scale * (p @ p)
            assert (X == 0.0).all() and (out["chi"] == 0.0).all() and out["residual"] == 0.0 and out["true_residual"] == 0.0
    bad = p.copy()
    bad[1500] = np.nan
    v0d = torch.from_numpy(cs["v0"].copy()).cuda()
    for ph in (np.zeros(n), bad):
        for U in (None, Ud):
            X = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            out = plan.static_response(torch.from_numpy(ph).cuda(), v0d, cs["sigma"], U=U, X=X)
            assert (out["iterations"], out["converged"], out["dead"], out["n_matvec"]) == (0, 0, 1, 9)
            assert out["coef"] == 0.0 and out["norm2"] == 0.0 and out["residual"] == 0.0 and out["true_residual"] == 0.0
            assert (X == 0.0).all() and (out["chi"] == 0.0).all()


def test_sigma_inside_the_spectrum_breaks_down_cleanly(ctx):
    """sigma in the middle of the dense spectrum (845 states), p = V[:, 0]: Q (H - sigma) Q is indefinite, d.A d of the first direction is
    negative in numpy.  The run must say so -- dead = 1 or converged = 0 -- and every output is finite."""
    cs, plan = ctx.case(845), ctx.plan(845)
    w = cs["w"]
    pd, v0d, Ud = torch.from_numpy(cs["p"].copy()).cuda(), torch.from_numpy(cs["v0"].copy()).cuda(), torch.from_numpy(cs["U"][:3].copy()).cuda()
    out = plan.static_response(pd, v0d, 0.5 * (w[0] + w[-1]), tol=TOL, max_it=100, U=Ud)
    print("iterations", out["iterations"], "converged", out["converged"], "dead", out["dead"], "residual", out["residual"], "true_residual", out["true_residual"])
    assert out["dead"] == 1 or out["converged"] == 0
    assert np.isfinite(out["X"].cpu().numpy()).all() and np.isfinite(out["chi"]).all()
    assert all(np.isfinite(out[k]) for k in ("coef", "norm2", "residual", "true_residual"))


def test_a_run_that_does_not_converge_returns_the_last_iterate(ctx):
    """max_it = 3 at 4097 states: status OK, converged 0, dead 0, iterations 3 exactly (the block of 8 is frozen after its third iteration),
    everything finite, true_residual equal to the numpy residual of the returned X to 1e-10, <p, X> = 0."""
    n = 4097
    cs, plan = ctx.case(n), ctx.plan(n)
    p = cs["p"]
    pd, v0d, Ud = torch.from_numpy(p.copy()).cuda(), torch.from_numpy(cs["v0"].copy()).cuda(), torch.from_numpy(cs["U"][:3].copy()).cuda()
    out = plan.static_response(pd, v0d, cs["sigma"], tol=TOL, max_it=3, U=Ud)
    X = out["X"].cpu().numpy()
    res = _residual(cs["H"], p, X, cs["v0"], cs["sigma"])
    print("iterations", out["iterations"], "residual", out["residual"], "true_residual", out["true_residual"], "numpy", res)
    assert out["converged"] == 0 and out["dead"] == 0 and out["iterations"] == 3 and out["n_matvec"] == 9
    assert np.isfinite(X).all() and np.isfinite(out["chi"]).all() and np.isfinite(out["residual"]) and out["residual"] > TOL
    assert abs(out["true_residual"] - res) <= 1e-10
    assert abs(p @ X) <= 1e-12 * np.linalg.norm(p) * np.linalg.norm(X)


def test_refusals(ctx):
    from dmrgx_amd import _capi as capi
    ERR_ARG = capi.DMRGX_ERR_ARG
    n = 845
    plan = ctx.plan(n)
    ok = torch.ones(n, dtype=torch.float64, device="cuda")
    pp = torch.full((n,), 0.5, dtype=torch.float64, device="cuda")
    U = torch.ones((2, n), dtype=torch.float64, device="cuda")
    for kw, word in (({"tol": -1e-3}, "tol"), ({"tol": 1.0}, "tol"), ({"tol": float("nan")}, "tol"), ({"sigma": float("inf")}, "sigma"), ({"sigma": float("nan")}, "sigma"),
                     ({"max_it": 0}, "max_it"), ({"max_it": -5}, "max_it"), ({"check_every": -1}, "check_every")):
        args = dict(sigma=0.0)
        args.update(kw)
        with pytest.raises(capi.DmrgxError) as e:
            plan.static_response(pp, ok, **args)
        assert e.value.code == ERR_ARG and word in str(e.value), kw
    with pytest.raises(capi.DmrgxError) as e:                               # ldu < n_states
        plan.static_response(pp, ok, 0.0, U=torch.ones((2, 2 * n), dtype=torch.float64, device="cuda")[:, :n].as_strided((2, n), (n - 1, 1)))
    assert e.value.code == ERR_ARG and "ldu" in str(e.value)
    # through the C ABI: null pointers, a negative nu, overlapping buffers
    lib, st = capi.lib(), plan._stream_ptr(None)
    coef, norm2, stats = C.c_double(0.0), C.c_double(0.0), capi.CvStats()
    chi = (C.c_double * 2)()
    big = torch.full((2 * n,), float("nan"), dtype=torch.float64, device="cuda")
    at = lambda k: C.c_void_p(big.data_ptr() + 8 * k)                        # noqa: E731
    pv, v, u, null, nd = C.c_void_p(pp.data_ptr()), C.c_void_p(ok.data_ptr()), C.c_void_p(U.data_ptr()), C.c_void_p(), C.POINTER(C.c_double)()

    def call(plan_=plan._handle, p_=pv, v0=v, X_=at(0), nu=2, U_=u, ldu=n, coef_=C.byref(coef), norm2_=C.byref(norm2), chi_=chi, stats_=C.byref(stats)):
        return lib.dmrgx_kron_static_response(plan_, p_, v0, 0.0, 0.0, 4, 0, X_, nu, U_, ldu, coef_, norm2_, chi_, stats_, st)

    calls = {
        "plan": dict(plan_=null), "p": dict(p_=null), "v0": dict(v0=null), "X": dict(X_=null), "coef": dict(coef_=nd), "norm2": dict(norm2_=nd),
        "stats": dict(stats_=C.POINTER(capi.CvStats)()), "chi": dict(chi_=nd), "U": dict(U_=null), "nu": dict(nu=-1), "ldu": dict(ldu=n - 1),
        "X is p": dict(X_=pv), "X is v0": dict(X_=v), "X overlaps the end of v0": dict(X_=C.c_void_p(ok.data_ptr() + 8 * (n - 1))),
        "X inside U": dict(X_=C.c_void_p(U.data_ptr() + 8 * (2 * n - 1))), "X is U": dict(X_=u),
    }
    for what, kw in calls.items():
        assert call(**kw) == ERR_ARG, what
    assert torch.isnan(big).all()                                            # every refusal came before any device work
    # allowed: no U (chi is then not needed); p = v0 (both only read)
    assert call(nu=0, U_=null, ldu=0, chi_=nd) == 0
    assert call(v0=pv) == 0 and stats.converged == 1 and stats.iterations == 0 and coef.value == 1.0
    assert call() == 0 and coef.value == 2.0 and not torch.isnan(big[:n]).any() and torch.isnan(big[n:]).all()
    striped = ctx.sbm.KronPlan(krylov_input(ctx.wl, 845)[0], world_size=2, rank=0)
    full = torch.ones(striped.info.vec_len, dtype=torch.float64, device="cuda")
    with pytest.raises(capi.DmrgxError) as e:
        striped.static_response(full, full, 0.0)
    assert e.value.code == ERR_ARG and "striped" in str(e.value)
    striped.destroy()


# ---- the same on a poisoned workspace ------------------------------------------------------------------------------------------------------
def _run_poison_case(sbm, wl):
    """n = 2049, nu = 5, p a fixed normal vector and sigma far below the spectrum (no eigensolve: the operator is positive definite on every
    complement): -> (outputs as arrays, X)"""
    n, nu = POISON_CASE
    rng = np.random.default_rng(77)
    p, v0, U = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal((nu, n))
    plan = sbm.KronPlan(krylov_superblock(wl, n))
    out = plan.static_response(torch.from_numpy(p).cuda(), torch.from_numpy(v0).cuda(), -500.0, tol=TOL, max_it=MAX_IT, U=torch.from_numpy(U).cuda())
    X = out["X"].cpu().numpy()
    plan.destroy()
    scal = np.array([out[k] for k in ("coef", "norm2", "iterations", "converged", "dead", "n_matvec", "residual", "true_residual")], dtype=np.float64)
    return p, v0, U, scal, out["chi"], X


def test_poisoned_workspace(ctx, tmp_path):
    """2049 states, nu 5 in a child process under DMRGX_POOL_POISON=1 (r, d, t, the copy of p and the partial sums come from the pool filled
    with NaN: a kernel that read t before it was written, a frozen iteration that let it into the state, or a ragged tail left unwritten
    would turn the outputs NaN): converged, nothing NaN, the residual recomputed in numpy within tol, and the bits of the clean run in
    this process."""
    from test_gpu_poison import _child
    p, v0, U, scal, chi, X = _run_poison_case(ctx.sbm, ctx.wl)
    out = str(tmp_path / "poisoned.npz")
    pr = _child([os.path.join("tests", "test_gpu_static_response.py"), out], True, 300)
    assert pr.returncode == 0 and "static response child ok" in pr.stdout, pr.stdout[-2000:] + pr.stderr[-2000:]
    got = np.load(out)
    assert np.isfinite(got["X"]).all() and np.isfinite(got["chi"]).all() and np.isfinite(got["scal"]).all()
    assert got["scal"][3] == 1.0 and got["scal"][4] == 0.0
    H = FactoredH(ctx.wl, krylov_superblock(ctx.wl, POISON_CASE[0]))
    res = _residual(H, p, got["X"], v0, -500.0)
    print("iterations", got["scal"][2], "residual through FactoredH", res)
    assert res <= TOL * (1.0 + 1e-6) + 1e-12 * (ctx.case(2049)["hnorm"] + 500.0) * np.linalg.norm(got["X"]) / np.linalg.norm(_project(p, v0))
    assert np.array_equal(_bits(got["X"]), _bits(X)) and np.array_equal(_bits(got["chi"]), _bits(chi)) and np.array_equal(_bits(got["scal"]), _bits(scal))


if __name__ == "__main__":
    from __graft_entry__ import load_package
    load_package()
    from dmrgx_amd import superblock as sbm_child, workloads as wl_child
    assert os.environ.get("DMRGX_POOL_POISON") == "1"
    _, _, _, scal_c, chi_c, X_c = _run_poison_case(sbm_child, wl_child)
    np.savez(sys.argv[1], scal=scal_c, chi=chi_c, X=X_c)
    print("static response child ok")
