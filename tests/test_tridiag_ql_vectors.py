"""host/TridiagQL.hpp, TridiagQLVectors (no GPU): all eigenvectors of a symmetric tridiagonal matrix -- what -dsf_sites needs from the
Lanczos matrix of a kept basis -- against numpy.linalg.eigh, through the host tool."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dmrg.x_amd", "dmrgx-host-tool")


def _ql_vectors(d, e):
    line = "tridiagvec %d %s" % (len(d), " ".join(repr(float(x)) for x in list(d) + list(e)))
    out = subprocess.run([TOOL], input=line + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert lines[0].split() == ["tridiagvec", "1", str(len(d))], lines[0][:200]
    rows = np.array([[float(x) for x in ln.split()[1:]] for ln in lines[1:]]).reshape(len(d), len(d) + 1)
    return rows[:, 0], rows[:, 1:]              # eigenvalues (unsorted), vec[k] = eigenvector of eigenvalue k


@pytest.mark.parametrize("n", [1, 2, 40, 300])
def test_all_eigenvectors_against_numpy(n):
    """Well-separated spectra: a diagonal that climbs by 1 per row (jittered by 0.2) with couplings in [0.2, 0.4], so every gap is at
    least ~0.3 and an eigenvector is defined to eps |T| / gap.  Eigenvalues and the |S| entries to 1e-12 |T| (|T|: largest absolute row
    sum); S orthogonal and T S = S Theta to the same bound."""
    rng = np.random.default_rng(300 + n)
    d = np.arange(n) + 0.2 * rng.uniform(-1, 1, n)
    e = rng.uniform(0.2, 0.4, max(n - 1, 0))
    T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    w, S = np.linalg.eigh(T)
    assert n == 1 or np.diff(w).min() > 0.25
    th, vec = _ql_vectors(d, e)
    o = np.argsort(th)
    th, Sq = th[o], vec[o].T                    # Sq[i][k]: component i of eigenvector k, ascending
    scale = np.abs(T).sum(axis=1).max()
    tol = 1e-12 * scale
    print(n, "eigenvalue err", np.abs(th - w).max(), "|S| err", np.abs(np.abs(Sq) - np.abs(S)).max(), "tol", tol)
    assert np.abs(th - w).max() <= tol
    assert np.abs(np.abs(Sq) - np.abs(S)).max() <= tol
    assert np.abs(Sq.T @ Sq - np.eye(n)).max() <= tol
    assert np.abs(T @ Sq - Sq * th).max() <= tol


def test_first_row_agrees_with_the_first_row_function():
    """The two functions run the same iteration: the first components are the same numbers."""
    rng = np.random.default_rng(9)
    n = 25
    d, e = 3.0 * rng.standard_normal(n), 0.3 + np.abs(rng.standard_normal(n - 1))
    th, vec = _ql_vectors(d, e)
    line = "tridiag %d %s" % (n, " ".join(repr(float(x)) for x in list(d) + list(e)))
    out = subprocess.run([TOOL], input=line + "\n", capture_output=True, text=True, timeout=60)
    pairs = np.array([[float(x) for x in t.split(",")] for t in out.stdout.split()[2:]]).reshape(-1, 2)
    assert np.array_equal(pairs[:, 0], th) and np.array_equal(pairs[:, 1], vec[:, 0])
