"""host/Measurements.hpp (no GPU): what the measurements share on the host -- the exact-zero phase coefficients of -dsf, the bond list,
the lattice Fourier sum, the one-column cosine sum and the frequency grid of the site-based dynamical measurements and the JSON record
file -- through the host tool."""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle.hamiltonian import J1J2XXZModel_SquareLattice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dmrg.x_amd", "dmrgx-host-tool")


def _tool(lines):
    out = subprocess.run([TOOL], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.splitlines(), out.stderr


def _ham_line(opts):
    return "ham " + " ".join(f"-{k} {'_' if v is True else v}" for k, v in opts.items())


def _dsfcoef(Lx, Ly, nx, ny):
    out, _ = _tool([_ham_line(dict(Lx=Lx, Ly=Ly, heisenberg=1.0)), f"dsfcoef {Lx} {Ly} {nx} {ny}"])
    tok = out[1].split()
    assert out[0] == "rc 0" and tok[0] == "dsfcoef" and len(tok) == 1 + Lx * Ly
    return np.array([[float(x) for x in t.split(",")] for t in tok[1:]])


@pytest.mark.parametrize("Lx,Ly,nx,ny", [(6, 2, 3, 1), (6, 2, 1, 0), (6, 2, 2, 1), (6, 2, 0, 0), (4, 4, 1, 0)])
def test_dsf_phase_coefficients_have_exact_zeros(Lx, Ly, nx, ny):
    """q . r = 2 pi p / M with the integer p = (nx x Ly + ny y Lx) mod M, M = Lx Ly.  A coefficient is exactly 0.0 where integer
    arithmetic on p says the sine (2p = 0 mod M) or the cosine (4p = 0 and 2p != 0 mod M) vanishes; elsewhere it is numpy's cos / sin
    of the same double 2 pi p / M to 4 ulp (both libraries are accurate to below 1 ulp)."""
    ham = J1J2XXZModel_SquareLattice(Lx=Lx, Ly=Ly, heisenberg=1.0)
    M = Lx * Ly
    got = _dsfcoef(Lx, Ly, nx, ny)
    for s in range(M):
        x, y = ham.To2D(s)
        p = (nx * x * Ly + ny * y * Lx) % M
        for part, fn, zero in ((0, np.cos, (4 * p) % M == 0 and (2 * p) % M != 0), (1, np.sin, (2 * p) % M == 0)):
            c = got[s, part]
            if zero:
                assert c == 0.0, (s, part, p, c)
            else:
                ref = fn(2 * np.pi * p / M)
                assert c != 0.0 and abs(c - ref) <= 4 * np.spacing(abs(ref)), (s, part, p, c, ref)


def test_dsf_sine_part_vanishes_at_6x2_q31():
    """tests/test_gpu_dsf.py relies on it: at q = (3, 1) of the 6 x 2 lattice every sine coefficient is an exact zero, and no cosine
    coefficient is."""
    got = _dsfcoef(6, 2, 3, 1)
    assert not got[:, 1].any() and (np.abs(got[:, 0]) == 1.0).all()


@pytest.mark.parametrize("opts,npairs,nbonds", [(dict(Lx=4, Ly=2, heisenberg=1.0), 14, 10), (dict(Lx=6, Ly=2, heisenberg=1.0), 22, 16),
                                                (dict(Lx=4, Ly=4, heisenberg=1.0), 28, 28), (dict(Lx=6, Ly=1, heisenberg=1.0), 5, 5),
                                                # both ends of the generating-site rule: round a periodic x direction the HIGHER site generates
                                                # the bond (4 x 2), on two columns both sites do and the lower one counts (2 x 2)
                                                (dict(Lx=4, Ly=2, heisenberg=1.0, BCperiodic=True), 16, 12), (dict(Lx=2, Ly=2, heisenberg=1.0, BCperiodic=True), 8, 4)])
def test_bonds_are_the_distinct_neighbour_pairs(opts, npairs, nbonds):
    """DimerBonds: the distinct pairs of the oracle's NeighborPairs() in order of first appearance (on Ly = 2 every vertical pair
    appears twice in the list, once in the bonds); 'x' if the two sites differ in column, else 'y'; the generating site is the one
    whose right (x) or above (y) neighbour is the other site, the lower-numbered one where that holds for both."""
    ham = J1J2XXZModel_SquareLattice(**opts)
    Lx, Ly = ham.Lx(), ham.Ly()
    pairs = ham.NeighborPairs()
    want = []
    for k, (i, j) in enumerate(pairs):
        if [i, j] in pairs[:k]:
            continue
        (x0, y0), (x1, y1) = ham.To2D(i), ham.To2D(j)
        orient = "x" if x0 != x1 else "y"
        from_i = (x0 + 1) % Lx == x1 if orient == "x" else (y0 + 1) % Ly == y1
        from_j = (x1 + 1) % Lx == x0 if orient == "x" else (y1 + 1) % Ly == y0
        assert i < j and (from_i or from_j)
        want.append((i, j, orient) + (ham.To2D(i) if from_i else ham.To2D(j)))
    assert len(pairs) == npairs and len(want) == nbonds
    out, _ = _tool([_ham_line(opts), "bonds"])
    tok = out[1].split()
    assert out[0] == "rc 0" and tok[0] == "bonds"
    got = [tuple(f if n == 2 else int(f) for n, f in enumerate(t.split(","))) for t in tok[1:]]
    assert got == want


@pytest.mark.parametrize("Lx,Ly,n", [(4, 2, 8), (3, 2, 5)])
def test_lattice_fourier_against_numpy(Lx, Ly, n):
    """S[nx][ny] = (1/n) sum_ab cos(2 pi (nx dx / Lx + ny dy / Ly)) T[a][b] on a random T; n = Lx Ly as for the spin table, n != Lx Ly
    as for the bonds of one orientation.  Bound 1e-13 sum|T| / n: n^2 <= 64 terms, each with a few eps of rounding in the angle and
    the product -- a margin of about ten."""
    rng = np.random.default_rng(10 * Lx + n)
    sites = rng.permutation(Lx * Ly)[:n]
    x, y = sites // Ly, sites % Ly
    T = rng.standard_normal((n, n))
    line = "fourier %d %d %d %s %s %s" % (Lx, Ly, n, " ".join(map(str, x)), " ".join(map(str, y)), " ".join(repr(float(v)) for v in T.ravel()))
    out, _ = _tool([line])
    tok = out[0].split()
    assert tok[0] == "fourier" and len(tok) == 1 + Lx * Ly
    got = np.array([float(v) for v in tok[1:]]).reshape(Lx, Ly)
    dx, dy = x[:, None] - x[None, :], y[:, None] - y[None, :]
    want = np.array([[(np.cos(2 * np.pi * (nx * dx / Lx + ny * dy / Ly)) * T).sum() / n for ny in range(Ly)] for nx in range(Lx)])
    assert abs(got[0, 0] - T.sum() / n) <= 1e-13 * np.abs(T).sum() / n
    assert np.abs(got - want).max() <= 1e-13 * np.abs(T).sum() / n, np.abs(got - want).max()


def _lattice(Lx, Ly):
    ham = J1J2XXZModel_SquareLattice(Lx=Lx, Ly=Ly, heisenberg=1.0)
    xy = np.array([ham.To2D(s) for s in range(Lx * Ly)])
    return xy[:, 0], xy[:, 1]


def _numbers(*arrays):
    return " ".join(repr(v) for a in arrays for v in np.asarray(a).ravel().tolist())


def _cossum(Lx, Ly, c, T):
    """SiteCosineSum of the n x ncol table T over all sites of the Lx x Ly lattice, reference site c: the (Lx Ly) x ncol table."""
    x, y = _lattice(Lx, Ly)
    n, ncol = T.shape
    out, _ = _tool([f"cossum {Lx} {Ly} {n} {c} {ncol} " + _numbers(x, y, T)])
    tok = out[0].split()
    assert tok[0] == "cossum" and len(tok) == 1 + Lx * Ly * ncol
    return np.array([float(v) for v in tok[1:]]).reshape(Lx * Ly, ncol)


def _cossum_numpy(Lx, Ly, c, T):
    """The same sum with the cosine argument formed by the same expression, 2 pi (nx dx / Lx + ny dy / Ly) from integer nx dx, ny dy."""
    x, y = _lattice(Lx, Ly)
    return np.array([(np.cos(2 * np.pi * ((nx * (x - x[c])) / Lx + (ny * (y - y[c])) / Ly))[:, None] * T).sum(axis=0) for nx in range(Lx) for ny in range(Ly)])


@pytest.fixture(scope="module")
def table_6x2():
    """12 x 3, entries in [-1, 1]: as many rows as the 6 x 2 lattice has sites."""
    return np.random.default_rng(20261019).uniform(-1.0, 1.0, (12, 3))


@pytest.mark.parametrize("c", [0, 7])
def test_cosine_sum_is_lattice_fourier_of_one_column(table_6x2, c):
    """The path -dsf_cv took before SiteCosineSum: LatticeFourier with norm 1 of the 12 x 12 matrix that is zero except for column c.
    The zeros add nothing and the other terms come in the same order, so every double is the same.  The tool's fourier command
    divides by n unless a norm follows the matrix: it is given 1.0 here, so that nothing is scaled back."""
    x, y = _lattice(6, 2)
    got = _cossum(6, 2, c, table_6x2)
    for k in range(3):
        Z = np.zeros((12, 12))
        Z[:, c] = table_6x2[:, k]
        out, _ = _tool(["fourier 6 2 12 " + _numbers(x, y, Z) + " 1.0"])
        tok = out[0].split()
        assert tok[0] == "fourier" and len(tok) == 1 + 12
        assert (got[:, k] == np.array([float(v) for v in tok[1:]])).all(), (c, k)


@pytest.mark.parametrize("c", [0, 7])
def test_cosine_sum_against_numpy(table_6x2, c):
    """1e-13, the bound tests/test_gpu_dsf_cv.py puts on SqwGrid at N = 12 and |T| <= 1."""
    err = np.abs(_cossum(6, 2, c, table_6x2) - _cossum_numpy(6, 2, c, table_6x2)).max()
    assert err <= 1e-13, err


def test_cosine_sum_on_4x4():
    """q = (0, 0): every cosine is cos(0) = 1, so row 0 is the plain sum of the column over s ascending -- the same doubles.  The other
    rows against numpy to 1e-13: 16 terms with |T| <= 1, each a few eps off through the angle (below 4 pi) and the product."""
    T = np.random.default_rng(44).uniform(-1.0, 1.0, (16, 1))
    got = _cossum(4, 4, 5, T)
    acc = 0.0
    for v in T[:, 0].tolist():
        acc += v
    assert got.shape == (16, 1) and got[0, 0] == acc
    assert np.abs(got - _cossum_numpy(4, 4, 5, T)).max() <= 1e-13


@pytest.mark.parametrize("w0,w1,nw", [(0.0, 4.0, 9), (0.3, 0.3, 1), (-1.0, 2.0, 4)])
def test_omega_grid(w0, w1, nw):
    """w0 + (w1 - w0) k / (nw - 1) in this order of operations, w0 alone for nw = 1: the same doubles as Python's."""
    out, _ = _tool([f"omegagrid {w0!r} {w1!r} {nw}"])
    tok = out[0].split()
    assert tok[:2] == ["omegagrid", "1"]
    assert [float(v) for v in tok[2:]] == ([w0 + (w1 - w0) * k / (nw - 1) for k in range(nw)] if nw > 1 else [w0])


@pytest.mark.parametrize("line", ["0 4 0", "0 4", "4 0 3", "0 4 2.5", "0 4 1"])
def test_omega_grid_refuses_malformed_input(line):
    """nw = 0, two numbers, w0 > w1, a fractional nw, nw = 1 with w0 != w1: a failure and no grid."""
    out, _ = _tool(["omegagrid " + line])
    assert out == ["omegagrid 0"]


# two records of the tool's jsonrec command, number format %.15g: record k holds the row R = T[1:4] and the 2 x 3 table T of the six
# numbers (6 k + i) / 3.  The framing is that of the engine's SpinCorrelations.json and DimerCorrelations.json.
JSONREC_15G = """[
  {"K": 0,
   "R": [0.333333333333333, 0.666666666666667, 1],
   "T": [
     [0, 0.333333333333333, 0.666666666666667],
     [1, 1.33333333333333, 1.66666666666667]
   ]},
  {"K": 1,
   "R": [2.33333333333333, 2.66666666666667, 3],
   "T": [
     [2, 2.33333333333333, 2.66666666666667],
     [3, 3.33333333333333, 3.66666666666667]
   ]}
]
"""


def test_json_record_file_bytes(tmp_path):
    path = str(tmp_path / "rec.json")
    out, _ = _tool([f"jsonrec {path} %.15g 2"])
    assert out == ["rc 0"]
    assert open(path, "rb").read() == JSONREC_15G.encode()


@pytest.mark.parametrize("fmt,rel", [("%.15g", 5e-15), ("%.17g", 0.0)])
def test_json_record_file_loads(tmp_path, fmt, rel):
    """json.load returns the numbers: exactly with 17 significant digits, to half a unit of the 15th digit with 15."""
    path = str(tmp_path / "rec.json")
    out, _ = _tool([f"jsonrec {path} {fmt} 2"])
    assert out == ["rc 0"]
    recs = json.load(open(path))
    assert [r["K"] for r in recs] == [0, 1]
    for k, r in enumerate(recs):
        T = np.array([(6 * k + i) / 3.0 for i in range(6)])
        assert set(r) == {"K", "R", "T"} and np.array(r["T"]).shape == (2, 3)
        assert (np.abs(np.array(r["T"]).ravel() - T) <= rel * np.abs(T)).all()
        assert (np.abs(np.array(r["R"]) - T[1:4]) <= rel * np.abs(T[1:4])).all()


def test_json_record_file_without_a_record_creates_no_file(tmp_path):
    path = str(tmp_path / "none.json")
    out, _ = _tool([f"jsonrec {path} %.15g 0"])
    assert out == ["rc 0"] and not os.path.exists(path)


def test_json_record_file_that_cannot_be_opened(tmp_path):
    """PETSC_ERR_FILE_OPEN (65) and the engine's message."""
    path = str(tmp_path / "missing" / "rec.json")
    out, err = _tool([f"jsonrec {path} %.15g 1"])
    assert out == ["rc 65"] and ("Cannot open " + path) in err
