"""host/Measurements.hpp (no GPU): ChebyshevWindowTwoSided, the spectral window of -dsf_pm in a sector whose bottom is not known, from both
extreme Ritz values of a short Lanczos run and their residual bounds -- through the host tool against numpy, on the planted matrix and
the three cases of test_chebyshev_host.py."""
import numpy as np

from test_chebyshev_host import _lanczos, _tool, planted  # noqa: F401  (planted: a module-scoped fixture)


def _window2(alpha, beta, done):
    tok = _tool("chebwindow2 %d %d %s %s" % (len(alpha), done, " ".join("%.17g" % x for x in alpha), " ".join("%.17g" % x for x in beta)))
    assert tok[0] == "chebwindow2" and len(tok) == 8
    return int(tok[1]), [float(x) for x in tok[2:]]


def _reference(alpha, beta, done, broke):
    """-> [centre, half_width, theta_min, theta_max, res_min, res_max]"""
    T = np.diag(alpha[:done]) + np.diag(beta[:done - 1], 1) + np.diag(beta[:done - 1], -1)
    th, S = np.linalg.eigh(T)
    rlo, rhi = (0.0, 0.0) if broke else (beta[done - 1] * abs(S[-1, 0]), beta[done - 1] * abs(S[-1, -1]))
    width = th[-1] - th[0]
    lo, hi = th[0] - rlo - 0.02 * width, th[-1] + rhi + 0.02 * width
    return [(hi + lo) / 2, (hi - lo) / 2, th[0], th[-1], rlo, rhi]


def test_window_from_converged_ritz_values(planted):
    """40 steps on the 60 x 60 matrix with spectrum -7 .. 5 and 9: both ends have converged, the residuals are far below the margins,
    the window holds the planted spectrum."""
    H, lam, _, v0 = planted
    a, b = _lanczos(H, v0, 40)
    ok, got = _window2(a, b, 40)
    want = _reference(a, b, 40, False)
    print("got", got, "want", want)
    assert ok == 1
    assert np.abs(np.array(got) - np.array(want)).max() <= 1e-12 * 16.0
    assert abs(got[3] - 9.0) <= 1e-9 and abs(got[2] + 7.0) <= 1e-6 and got[4] <= 1e-2 and got[5] <= 1e-4
    assert got[0] - got[1] < lam[0] and got[0] + got[1] > lam[-1]


def test_window_from_unconverged_ritz_values(planted):
    """4 steps: neither end has converged and the residual bounds are what the window adds beyond the Ritz values; some eigenvalue lies
    within the residual of each, and the formula is numpy's.  (The window need not hold the spectrum here: the guard of the Chebyshev
    run reports that, the window does not promise it.)"""
    H, lam, _, v0 = planted
    a, b = _lanczos(H, v0, 4)
    ok, got = _window2(a, b, 4)
    want = _reference(a, b, 4, False)
    print("got", got, "want", want)
    assert ok == 1
    assert np.abs(np.array(got) - np.array(want)).max() <= 1e-12 * 16.0
    assert got[4] > 1e-2 and got[5] > 1e-2 and got[3] < 9.0 - 1e-3 and got[2] > -7.0 + 1e-3
    assert np.abs(lam - got[3]).min() <= got[5] * (1 + 1e-12) and np.abs(lam - got[2]).min() <= got[4] * (1 + 1e-12)
    assert got[0] - got[1] < got[2] - got[4] and got[0] + got[1] > got[3] + got[5]


def test_window_after_a_breakdown(planted):
    """A start vector inside a 3-dimensional invariant subspace (eigenvalues lam[2], lam[30], 9): the run breaks down after 3 of 10 steps,
    the Ritz values are exact, both residuals are 0, and the window holds the spectrum of that subspace with the 2 % margins."""
    H, lam, q, _ = planted
    v0 = q[:, [2, 30, 59]] @ np.array([1.0, -0.5, 0.25])
    a, b = _lanczos(H, v0, 3)
    assert b[2] < 1e-10
    alpha, beta = np.concatenate([a, np.zeros(7)]), np.concatenate([b, np.zeros(7)])
    ok, got = _window2(alpha, beta, 3)
    want = _reference(alpha, beta, 3, True)
    print("got", got, "want", want)
    assert ok == 1 and got[4] == 0.0 and got[5] == 0.0
    assert np.abs(np.array(got) - np.array(want)).max() <= 1e-12 * 16.0
    assert abs(got[3] - 9.0) <= 1e-10 and abs(got[2] - lam[2]) <= 1e-10
    assert got[0] - got[1] < lam[2] and got[0] + got[1] > 9.0
    assert abs((got[0] - got[1]) - (lam[2] - 0.02 * (9.0 - lam[2]))) <= 1e-9
    ok0, _ = _window2(alpha, beta, 0)
    assert ok0 == 0
    ok1, one = _window2(alpha[:1], beta[:1], 1)       # one step: theta_min = theta_max, the residual alone opens the window
    assert ok1 == 1 and one[2] == one[3] == alpha[0] and abs(one[1] - beta[0]) <= 1e-12 * 16.0
