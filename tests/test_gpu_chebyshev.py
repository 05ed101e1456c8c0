"""dmrgx_kron_chebyshev_moments (-m gpu, csrc/lanczos.hip): the Chebyshev recursion t_{n+1} = 2 Ht t_n - t_{n-1} on the device, its diagonal
moments by the doubling identities and its cross moments through the Gram kernel, at one to three workgroups of 2048 elements (845, 1205,
2049 -- the second workgroup holds one element -- and 4097 states), at block counts of the 16-row ring that end full, one short and
with a partial block (K + 1 = 2, 16, 17, 38), with and without U.

References.  845 and 1205 states: the dense eigendecomposition H = V diag(w) V^T, mu_m = sum_k c_k^2 T_m(x_k) with c = V^T v0,
x_k = (w_k - centre) / half_width, and <u_i, t_n> = sum_k (V^T u_i)_k c_k T_n(x_k); the window is [w_min, w_max] with 1 % of the width
added on both sides.  2049 and 4097 states: the same recursion in numpy through helpers.FactoredH (2 K steps, mu_m = <v0, t_m>); the
window is +-1.25 x the largest |Ritz value| of 60 reorthogonalised Lanczos steps, and every test asserts D == K, which fails if that window
does not hold.

Bounds.  mu_diag to 1e-10 mu_0 and mu_cross[n][i] to 1e-10 |u_i| |v0|: |mu| <= |u| |v| inside the window, a numpy restatement of the
recursion agrees with the eigendecomposition to 7e-15 relative over 200 steps (checked on the CPU at 845 and 2049 states), the margin
is for the summation order; it is the relative scale of the Lanczos coefficient tests."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import FactoredH, krylov_input, krylov_superblock, lanczos_reorth, lanczos_tridiag

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMAX = 37
NU_MAX = 13


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def cheb_T(m, x):
    """T_m(x) for any real x (outside [-1, 1] by cosh), m an integer array or scalar"""
    x = np.asarray(x, dtype=np.float64)
    inside = np.abs(x) <= 1.0
    xi = np.where(inside, x, 0.0)
    xo = np.where(inside, 1.0, np.abs(x))
    sign = np.where((x < 0) & (np.asarray(m) % 2 == 1), -1.0, 1.0)
    return np.where(inside, np.cos(m * np.arccos(xi)), sign * np.cosh(m * np.arccosh(xo)))


class _Context:
    """Per size: the plan, the window, v0 and U (u_0 = v0), and the reference moments for K <= KMAX -- all built once, read-only."""

    def __init__(self, sbm, wl):
        self.sbm, self.wl, self._plans, self._cases = sbm, wl, {}, {}

    def plan(self, n):
        if n not in self._plans:
            self._plans[n] = self.sbm.KronPlan(krylov_input(self.wl, n)[0] if n in (845, 1205) else krylov_superblock(self.wl, n))
        return self._plans[n]

    def case(self, n):
        if n in self._cases:
            return self._cases[n]
        rng = np.random.default_rng(100 + n)
        v0 = rng.standard_normal(n)
        U = rng.standard_normal((NU_MAX, n))
        U[0] = v0
        if n in (845, 1205):
            _, H, w, V = krylov_input(self.wl, n)
            width = w[-1] - w[0]
            lo, hi = w[0] - 0.01 * width, w[-1] + 0.01 * width
            centre, hw = 0.5 * (hi + lo), 0.5 * (hi - lo)
            x = (w - centre) / hw
            c, cu = V.T @ v0, U @ V
            m = np.arange(2 * KMAX + 1)
            Tm = cheb_T(m[:, None], x[None, :])                       # [m][k]
            diag = Tm @ (c * c)
            cross = (Tm[:KMAX + 1] * c[None, :]) @ cu.T                # [n][i]
        else:
            H = FactoredH(self.wl, krylov_superblock(self.wl, n))
            _, a, b = lanczos_reorth(H, v0, 60)
            centre, hw = 0.0, 1.25 * np.abs(np.linalg.eigvalsh(lanczos_tridiag(a, b))).max()
            t = [v0, (H @ v0 - centre * v0) / hw]
            for _ in range(2, 2 * KMAX + 1):
                t.append(2.0 * (H @ t[-1] - centre * t[-1]) / hw - t[-2])
            t = np.array(t)
            diag = t @ v0
            cross = t[:KMAX + 1] @ U.T
        out = dict(v0=v0, U=U, centre=centre, hw=hw, diag=diag, cross=cross)
        for a in (v0, U, diag, cross):
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


def _check_moments(ctx, n, K, nu, pad=0, offset=0):
    """One run, twice.  U is a view of a NaN-filled buffer: row stride n + pad, first element `offset` doubles into the allocation."""
    cs, plan = ctx.case(n), ctx.plan(n)
    v0, Uh = cs["v0"], cs["U"][:nu]
    v0d = torch.from_numpy(v0.copy()).cuda()
    Ud = None
    if nu:
        store = torch.full((offset + nu * (n + pad),), float("nan"), dtype=torch.float64, device="cuda")
        Ud = store[offset:].view(nu, n + pad)[:, :n]
        Ud.copy_(torch.from_numpy(Uh.copy()))
        assert Ud.data_ptr() % 16 == (8 * offset) % 16 and Ud.stride(0) == n + pad
    norm2, diag, cross, done = plan.chebyshev_moments(v0d, cs["centre"], cs["hw"], K, U=Ud)
    norm2b, diagb, crossb, doneb = plan.chebyshev_moments(v0d, cs["centre"], cs["hw"], K, U=Ud)
    mu0 = float(v0 @ v0)
    want_d, want_c = cs["diag"][:2 * K + 1], cs["cross"][:K + 1, :nu]
    scale_c = np.linalg.norm(Uh, axis=1) * np.sqrt(mu0) if nu else np.zeros(0)
    err_d = np.abs(diag - want_d).max() / mu0
    err_c = (np.abs(cross - want_c) / scale_c[None, :]).max() if nu else 0.0
    tie = np.abs(cross[:, 0] - diag[:K + 1]).max() / mu0 if nu else 0.0
    print("n", n, "K", K, "nu", nu, "pad", pad, "offset", offset, "done", done, "norm2 err", abs(norm2 - mu0) / mu0, "diag err / mu0", err_d,
          "cross err / |u||v|", err_c, "|cross[:, 0] - diag| / mu0", tie)
    assert done == K == doneb
    assert diag.shape == (2 * K + 1,) and cross.shape == (K + 1, nu)
    assert np.isfinite(diag).all() and np.isfinite(cross).all()
    assert norm2 == diag[0] and abs(norm2 - mu0) <= 1e-10 * mu0
    assert err_d <= 1e-10
    assert err_c <= 1e-10
    assert tie <= 1e-12                                               # the doubling path against the Gram path (u_0 = v0)
    assert norm2 == norm2b and np.array_equal(_bits(diag), _bits(diagb)) and np.array_equal(_bits(cross), _bits(crossb))
    assert np.array_equal(_bits(v0d.cpu().numpy()), _bits(v0))
    if nu:
        assert np.array_equal(_bits(Ud.cpu().numpy()), _bits(Uh))
        assert torch.isnan(store[:offset]).all() and (pad == 0 or torch.isnan(store[offset:].view(nu, n + pad)[:, n:]).all())


@pytest.mark.parametrize("nu", [0, 1, 13])
@pytest.mark.parametrize("K", [1, 15, 16, 37])
@pytest.mark.parametrize("n", [845, 1205, 2049, 4097])
def test_moments_of_a_random_vector(ctx, n, K, nu):
    """K + 1 = 2 (one partial block), 16 (exactly one block, no partial call), 17 (a block and one vector), 38 (both halves of the ring and
    a partial block of 6); nu = 0 (no Gram call), 1, 13."""
    _check_moments(ctx, n, K, nu)


@pytest.mark.parametrize("n", [845, 2049])
def test_moments_with_a_padded_and_offset_U(ctx, n):
    """ldu = n_states + 1 and a U pointer 8 bytes into a 16-byte aligned allocation: rows alternate between the two alignments; the pad
    column and the element before U stay NaN."""
    _check_moments(ctx, n, 20, 13, pad=1, offset=1)


def test_planted_eigenvector_shows_no_drift(ctx):
    """v0 = 1.5 x eigenvector k of the 845-state H, K = 300: mu_diag[m] = |v0|^2 cos(m arccos x_k) to 1e-10 |v0|^2 for all m <= 600 and
    D = 300 -- the recursion does not drift and the guard does not trip on a vector whose norm sits at the bound for every n where
    |T_n(x_k)| = 1."""
    cs, plan = ctx.case(845), ctx.plan(845)
    _, _, w, V = krylov_input(ctx.wl, 845)
    k, K = 300, 300
    v0 = 1.5 * V[:, k]
    xk = (w[k] - cs["centre"]) / cs["hw"]
    norm2, diag, cross, done = plan.chebyshev_moments(torch.from_numpy(v0.copy()).cuda(), cs["centre"], cs["hw"], K)
    mu0 = float(v0 @ v0)
    want = mu0 * np.cos(np.arange(2 * K + 1) * np.arccos(xk))
    print("x_k", xk, "done", done, "max err / mu0", np.abs(diag - want).max() / mu0)
    assert done == K and cross.shape == (K + 1, 0)
    assert np.abs(diag - want).max() <= 1e-10 * mu0


@pytest.mark.parametrize("nu", [0, 13])
def test_guard_ends_a_run_whose_window_is_too_narrow(ctx, nu):
    """half_width half the true one: the spectrum reaches |x| = 2, T_n grows like e^(1.3 n), the guard trips at some D < K = 40.  Every
    output is finite, mu_diag[m] = 0 for m > 2 D and row n of mu_cross = 0 for n > D exactly, and what was valid still is the polynomial
    T_m((H - centre) / half_width): mu_diag[0 .. min(2 D, 2)] to 1e-10 mu_0 and the rows <= D of mu_cross."""
    cs, plan = ctx.case(845), ctx.plan(845)
    _, _, w, V = krylov_input(ctx.wl, 845)
    K, hw = 40, 0.5 * cs["hw"]
    v0, Uh = cs["v0"], cs["U"][:nu]
    Ud = torch.from_numpy(Uh.copy()).cuda() if nu else None
    norm2, diag, cross, done = plan.chebyshev_moments(torch.from_numpy(v0.copy()).cuda(), cs["centre"], hw, K, U=Ud)
    mu0 = float(v0 @ v0)
    x, c = (w - cs["centre"]) / hw, V.T @ v0
    want = np.array([np.sum(c * c * cheb_T(m, x)) for m in range(3)])
    print("nu", nu, "done", done, "max |x|", np.abs(x).max(), "diag[:5]", diag[:5], "want[:3]", want)
    assert 0 <= done < K
    assert np.isfinite(diag).all() and np.isfinite(cross).all() and abs(norm2 - mu0) <= 1e-10 * mu0
    assert (diag[2 * done + 1:] == 0.0).all() and (cross[done + 1:] == 0.0).all()
    top = min(2 * done, 2)
    assert np.abs(diag[:top + 1] - want[:top + 1]).max() <= 1e-10 * mu0
    if nu:
        cu = Uh @ V
        for n in range(done + 1):
            ref = cu @ (c * cheb_T(n, x))
            assert (np.abs(cross[n] - ref) <= 1e-10 * np.linalg.norm(Uh, axis=1) * np.sqrt(mu0)).all(), n
    # the guard is at |t_{D+1}|^2 > (1 + 1e-6) mu_0: the vectors up to D obey the bound, the next one does not
    norms = np.array([np.sum(c * c * cheb_T(n, x) ** 2) for n in range(done + 2)])
    assert (norms[:done + 1] <= (1 + 1e-6) * mu0 * (1 + 1e-9)).all() and norms[done + 1] > (1 + 1e-6) * mu0 * (1 - 1e-9)


def test_zero_and_nan_start_vectors(ctx):
    plan, n = ctx.plan(845), 845
    U = torch.from_numpy(ctx.case(845)["U"][:3].copy()).cuda()
    for fill in (0.0, float("nan")):
        v0 = torch.full((n,), fill, dtype=torch.float64, device="cuda")
        for u in (None, U):
            norm2, diag, cross, done = plan.chebyshev_moments(v0, 0.0, 10.0, 17, U=u)
            assert norm2 == 0.0 and done == 0 and (diag == 0.0).all() and (cross == 0.0).all(), (fill, norm2, done, diag, cross)
            assert diag.shape == (35,) and cross.shape == (18, 0 if u is None else 3)


def test_refusals(ctx):
    from dmrgx_amd import _capi as capi
    ERR_ARG = capi.DMRGX_ERR_ARG
    plan, n = ctx.plan(845), 845
    ok = torch.ones(n, dtype=torch.float64, device="cuda")
    U = torch.ones((2, n), dtype=torch.float64, device="cuda")
    for K in (0, -3):
        with pytest.raises(capi.DmrgxError) as e:
            plan.chebyshev_moments(ok, 0.0, 10.0, K)
        assert e.value.code == ERR_ARG and "nsteps" in str(e.value)
    for hw in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(capi.DmrgxError) as e:
            plan.chebyshev_moments(ok, 0.0, hw, 4)
        assert e.value.code == ERR_ARG and "half width" in str(e.value)
    for centre in (float("inf"), float("-inf"), float("nan")):
        with pytest.raises(capi.DmrgxError) as e:
            plan.chebyshev_moments(ok, centre, 10.0, 4)
        assert e.value.code == ERR_ARG and "centre" in str(e.value)
    with pytest.raises(capi.DmrgxError) as e:                               # ldu < n_states
        plan.chebyshev_moments(ok, 0.0, 10.0, 4, U=torch.ones((2, 2 * n), dtype=torch.float64, device="cuda")[:, :n].as_strided((2, n), (n - 1, 1)))
    assert e.value.code == ERR_ARG and "ldu" in str(e.value)
    # through the C ABI: null pointers and a negative nu
    lib, st = capi.lib(), plan._stream_ptr(None)
    norm2, done = C.c_double(0.0), C.c_int32(0)
    diag, cross = (C.c_double * 9)(), (C.c_double * 10)()
    v, u, null = C.c_void_p(ok.data_ptr()), C.c_void_p(U.data_ptr()), C.c_void_p()
    nd = C.POINTER(C.c_double)()
    calls = {
        "plan": (null, v, 0.0, 10.0, 4, 2, u, n, C.byref(norm2), diag, cross, C.byref(done), st),
        "v0": (plan._handle, null, 0.0, 10.0, 4, 2, u, n, C.byref(norm2), diag, cross, C.byref(done), st),
        "norm2": (plan._handle, v, 0.0, 10.0, 4, 2, u, n, nd, diag, cross, C.byref(done), st),
        "mu_diag": (plan._handle, v, 0.0, 10.0, 4, 2, u, n, C.byref(norm2), nd, cross, C.byref(done), st),
        "mu_cross": (plan._handle, v, 0.0, 10.0, 4, 2, u, n, C.byref(norm2), diag, nd, C.byref(done), st),
        "nsteps_done": (plan._handle, v, 0.0, 10.0, 4, 2, u, n, C.byref(norm2), diag, cross, C.POINTER(C.c_int32)(), st),
        "U": (plan._handle, v, 0.0, 10.0, 4, 2, null, n, C.byref(norm2), diag, cross, C.byref(done), st),
        "nu": (plan._handle, v, 0.0, 10.0, 4, -1, u, n, C.byref(norm2), diag, cross, C.byref(done), st),
    }
    for what, args in calls.items():
        assert lib.dmrgx_kron_chebyshev_moments(*args) == ERR_ARG, what
    # nu == 0: U and mu_cross may be null
    assert lib.dmrgx_kron_chebyshev_moments(plan._handle, v, 0.0, 1000.0, 4, 0, null, 0, C.byref(norm2), diag, nd, C.byref(done), st) == 0
    assert norm2.value == float(n) and done.value == 4
    striped = ctx.sbm.KronPlan(krylov_input(ctx.wl, 845)[0], world_size=2, rank=0)
    full = torch.ones(striped.info.vec_len, dtype=torch.float64, device="cuda")
    with pytest.raises(capi.DmrgxError) as e:
        striped.chebyshev_moments(full, 0.0, 10.0, 4)
    assert e.value.code == ERR_ARG and "striped" in str(e.value)
    striped.destroy()


# ---- the same on poisoned workspaces -------------------------------------------------------------------------------------------------------
POISONED_NODES = ["tests/test_gpu_chebyshev.py::" + name for name in (
    "test_moments_of_a_random_vector", "test_moments_with_a_padded_and_offset_U", "test_guard_ends_a_run_whose_window_is_too_narrow",
    "test_zero_and_nan_start_vectors")]


def test_moments_on_poisoned_workspaces():
    """The moment tests above, unchanged, in one child process with every f64 pool block handed out NaN-filled (DMRGX_POOL_POISON=1, the
    way test_gpu_krylov_shapes.py does): the ring rows are poisoned memory, so a first step that read the row of t_{-1}, a Gram call on a
    row not yet written, or a ragged tail left unwritten would turn the moments NaN."""
    env = dict(os.environ, DMRGX_POOL_POISON="1")
    python = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    p = subprocess.run(python + ["-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", *POISONED_NODES], cwd=ROOT, env=env, capture_output=True, text=True, timeout=480)
    tail = p.stdout[-3000:] + p.stderr[-2000:]
    assert p.returncode == 0, tail
    assert " passed" in tail and " failed" not in tail and " skipped" not in tail, tail
