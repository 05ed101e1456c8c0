"""host/TridiagQL.hpp (no GPU): eigenvalues and first eigenvector components of symmetric tridiagonal matrices -- all that the
continued fraction of -dsf needs from the Lanczos matrix -- against numpy's dense solver, through the host tool."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dmrg.x_amd", "dmrgx-host-tool")


def _ql(d, e):
    line = "tridiag %d %s" % (len(d), " ".join(repr(float(x)) for x in list(d) + list(e)))
    out = subprocess.run([TOOL], input=line + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    tok = out.stdout.split()
    assert tok[0] == "tridiag" and tok[1] == "1", out.stdout[:200]
    pairs = np.array([[float(x) for x in t.split(",")] for t in tok[2:]]).reshape(-1, 2)
    return pairs[:, 0], pairs[:, 1]


@pytest.mark.parametrize("n,kind", [(1, "random"), (2, "random"), (5, "random"), (40, "random"), (100, "random"), (40, "split"), (30, "clustered"), (12, "breakdown")])
def test_eigenvalues_and_first_components_against_numpy(n, kind):
    """Bound: 50 eps |T| for the eigenvalues (a backward-stable QL iteration moves each by a few eps |T|), and the same relative to 1
    for the spectral weights z^2 summed over each cluster of eigenvalues closer than 1e-8 |T| (inside a cluster only the sum is defined)."""
    rng = np.random.default_rng(100 + n)
    d, e = 3.0 * rng.standard_normal(n), 0.3 + np.abs(rng.standard_normal(max(n - 1, 0)))
    if kind == "split":
        e[n // 2] = 0.0                                   # two independent blocks: the second one carries no weight
    if kind == "clustered":
        d[:] = 1.0
        e[:] = 1e-9 * (1 + np.arange(n - 1))
    if kind == "breakdown":
        e[-1] = 1e-13                                     # the tiny beta a breakdown leaves behind in front of nothing
    T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    w, V = np.linalg.eigh(T)
    th, z = _ql(d, e)
    o = np.argsort(th)
    th, z = th[o], z[o]
    scale = max(np.abs(T).sum(axis=1).max(), 1e-300)
    tol = 50 * np.finfo(float).eps
    assert np.abs(th - w).max() <= tol * scale
    assert abs((z ** 2).sum() - 1.0) <= tol
    start = 0
    for i in range(1, n + 1):                             # clusters of the reference spectrum
        if i == n or w[i] - w[i - 1] > 1e-8 * scale:
            assert abs((z[start:i] ** 2).sum() - (V[0, start:i] ** 2).sum()) <= 20 * tol, (kind, start, i)
            start = i
