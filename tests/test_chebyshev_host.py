"""host/Measurements.hpp (no GPU): the two host parts of -dsf_cheb through the host tool -- ChebyshevWindow, the spectral window from
the coefficients of a short Lanczos run, and ChebyshevJackson, the Jackson-damped Chebyshev sum -- against numpy."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dmrg.x_amd", "dmrgx-host-tool")


def _tool(line):
    out = subprocess.run([TOOL], input=line + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.split()


def _window(E0, alpha, beta, done):
    tok = _tool("chebwindow %.17g %d %d %s %s" % (E0, len(alpha), done, " ".join("%.17g" % x for x in alpha), " ".join("%.17g" % x for x in beta)))
    assert tok[0] == "chebwindow" and len(tok) == 6
    return int(tok[1]), [float(x) for x in tok[2:]]


def _lanczos(H, v0, K):
    """plain numpy Lanczos with full reorthogonalisation: alpha[K], beta[K] (beta[j] = |w| of step j)"""
    Q = [v0 / np.linalg.norm(v0)]
    a, b = [], []
    for j in range(K):
        x = H @ Q[j]
        a.append(Q[j] @ x)
        for _ in range(2):
            for q in Q:
                x = x - (q @ x) * q
        b.append(np.linalg.norm(x))
        Q.append(x / b[j] if b[j] > 1e-300 else x)
    return np.array(a), np.array(b)


def _window_reference(E0, alpha, beta, done, broke):
    T = np.diag(alpha[:done]) + np.diag(beta[:done - 1], 1) + np.diag(beta[:done - 1], -1)
    th, S = np.linalg.eigh(T)
    rho = 0.0 if broke else beta[done - 1] * abs(S[-1, -1])
    hi, lo = th[-1] + rho + 0.02 * (th[-1] - E0), E0 - 0.01 * (th[-1] - E0)
    return [(hi + lo) / 2, (hi - lo) / 2, th[-1], rho]


@pytest.fixture(scope="module")
def planted():
    """A 60 x 60 symmetric matrix with eigenvalues -7 .. 5 and an isolated top eigenvalue 9, a random start vector."""
    rng = np.random.default_rng(3)
    lam = np.concatenate([np.linspace(-7.0, 5.0, 59), [9.0]])
    q, _ = np.linalg.qr(rng.standard_normal((60, 60)))
    return (q * lam) @ q.T, lam, q, rng.standard_normal(60)


def test_window_from_a_converged_top_ritz_value(planted):
    """40 steps: the isolated top eigenvalue 9 has converged, the residual is far below the margins, the window holds the spectrum."""
    H, lam, _, v0 = planted
    a, b = _lanczos(H, v0, 40)
    ok, got = _window(lam[0], a, b, 40)
    want = _window_reference(lam[0], a, b, 40, False)
    print("got", got, "want", want)
    assert ok == 1
    assert np.abs(np.array(got) - np.array(want)).max() <= 1e-12 * 16.0
    assert abs(got[2] - 9.0) <= 1e-9 and got[3] <= 1e-4
    assert got[0] - got[1] < lam[0] and got[0] + got[1] > lam[-1]


def test_window_from_an_unconverged_top_ritz_value(planted):
    """4 steps: theta_max is well below 9 and the residual bound is what closes the gap: some eigenvalue lies within the residual of
    theta_max, and the formula is numpy's."""
    H, lam, _, v0 = planted
    a, b = _lanczos(H, v0, 4)
    ok, got = _window(lam[0], a, b, 4)
    want = _window_reference(lam[0], a, b, 4, False)
    print("got", got, "want", want)
    assert ok == 1
    assert np.abs(np.array(got) - np.array(want)).max() <= 1e-12 * 16.0
    assert got[3] > 1e-2 and got[2] < 9.0 - 1e-3
    assert np.abs(lam - got[2]).min() <= got[3] * (1 + 1e-12)


def test_window_after_a_breakdown(planted):
    """A start vector inside a 3-dimensional invariant subspace: the run breaks down after 3 of 10 steps asked for (the later
    coefficients are zeros, as the library leaves them), the Ritz values are exact and the residual is 0."""
    H, lam, q, _ = planted
    v0 = q[:, [2, 30, 59]] @ np.array([1.0, -0.5, 0.25])
    a, b = _lanczos(H, v0, 3)
    assert b[2] < 1e-10
    alpha, beta = np.concatenate([a, np.zeros(7)]), np.concatenate([b, np.zeros(7)])
    ok, got = _window(lam[0], alpha, beta, 3)
    want = _window_reference(lam[0], alpha, beta, 3, True)
    print("got", got, "want", want)
    assert ok == 1 and got[3] == 0.0
    assert np.abs(np.array(got) - np.array(want)).max() <= 1e-12 * 16.0
    assert abs(got[2] - 9.0) <= 1e-10
    ok0, _ = _window(lam[0], alpha, beta, 0)
    assert ok0 == 0


def _jackson(mu, xs):
    tok = _tool("chebjackson %d %d %s %s" % (len(mu), len(xs), " ".join("%.17g" % m for m in mu), " ".join("%.17g" % x for x in xs)))
    assert tok[0] == "chebjackson" and len(tok) == 1 + len(xs)
    return np.array([float(t) for t in tok[1:]])


def _jackson_reference(mu, x):
    M = len(mu)
    n = np.arange(M)
    g = ((M - n + 1) * np.cos(np.pi * n / (M + 1)) + np.sin(np.pi * n / (M + 1)) / np.tan(np.pi / (M + 1))) / (M + 1)
    w = np.where(n == 0, 1.0, 2.0)
    return float(np.sum(w * g * mu * np.cos(n * np.arccos(x)))) / (np.pi * np.sqrt(1.0 - x * x))


@pytest.mark.parametrize("M", [1, 2, 61])
def test_jackson_sum_against_numpy(M):
    """Interior x against the formula in numpy to 1e-13 of sum |mu| / sqrt(1 - x^2) (M terms of size <= 2 |mu_n|, each with a cosine
    good to a few ulp of its argument n arccos x <= 61 pi); exactly 0 at |x| >= 1."""
    rng = np.random.default_rng(M)
    mu = rng.uniform(-1.0, 1.0, M)
    xs = np.array([-0.999, -0.7, -1e-3, 0.0, 0.31, 0.95, 0.999999])
    got = _jackson(mu, xs)
    want = np.array([_jackson_reference(mu, x) for x in xs])
    tol = 1e-13 * np.abs(mu).sum() / np.sqrt(1.0 - xs * xs)
    print("M", M, "err", np.abs(got - want), "tol", tol)
    assert (np.abs(got - want) <= tol).all()
    outside = _jackson(mu, [1.0, -1.0, 1.5, -7.0])
    assert (outside == 0.0).all()
    if M == 1:
        assert np.abs(got - mu[0] / (np.pi * np.sqrt(1.0 - xs * xs))).max() <= 1e-15 * abs(mu[0]) * 2e3      # g_0 = 1


@pytest.mark.parametrize("M", [1, 2, 61])
def test_jackson_sum_of_a_positive_measure_is_not_negative(M):
    """mu_n = sum_k w_k T_n(x_k) with w_k > 0: five delta peaks.  The Jackson kernel is positive, so the damped sum is >= 0 everywhere
    (to rounding: 1e-14 of sum w / sqrt(1 - x^2)), where the undamped sum of 61 moments swings to -2."""
    xk, wk = np.array([-0.9, -0.2, 0.1, 0.4, 0.97]), np.array([0.5, 1.0, 0.25, 2.0, 0.125])
    mu = np.array([np.sum(wk * np.cos(n * np.arccos(xk))) for n in range(M)])
    xs = np.linspace(-0.9995, 0.9995, 401)
    got = _jackson(mu, xs)
    print("M", M, "min", got.min(), "max", got.max())
    assert (got >= -1e-14 * wk.sum() / np.sqrt(1.0 - xs * xs)).all()
    if M == 61:
        plain = np.array([(mu[0] + 2 * np.sum(mu[1:] * np.cos(np.arange(1, M) * np.arccos(x)))) / (np.pi * np.sqrt(1 - x * x)) for x in xs])
        assert plain.min() < -1.0 and got.max() > 5.0
