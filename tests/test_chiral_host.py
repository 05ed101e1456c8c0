"""host/Measurements.hpp, the scalar-chirality part (no GPU): the plaquettes and triangles of a lattice, the six strings of K_ijk and how a
string splits at the cut into a left and a right part, through the host tool -- against a restatement from the oracle Hamiltonian, and
the six strings against S_i . (S_j x S_k) of three spins 1/2 written out densely."""
import os
import subprocess

import numpy as np
import pytest

from oracle.hamiltonian import J1J2XXZModel_SquareLattice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dmrg.x_amd", "dmrgx-host-tool")
OP_SM, OP_SZ, OP_SP = -1, 0, 1


def _tool(lines):
    out = subprocess.run([TOOL], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.splitlines()


def _ham_line(opts):
    return "ham " + " ".join(f"-{k} {'_' if v is True else v}" for k, v in opts.items())


def _plaquettes(ham):
    """a = (x, y), b = (x + 1, y), c = (x + 1, y + 1), d = (x, y + 1), y + 1 round the periodic direction; every edge a nearest-neighbour
    pair; in order of (x, y); every site set once."""
    Lx, Ly = ham.Lx(), ham.Ly()
    site = {tuple(ham.To2D(s)): s for s in range(ham.NumSites())}
    nn = {(min(p), max(p)) for p in ham.NeighborPairs()}
    out, seen = [], set()
    for x in range(Lx - 1):
        for y in range(Ly):
            c = [site[(x, y)], site[(x + 1, y)], site[(x + 1, (y + 1) % Ly)], site[(x, (y + 1) % Ly)]]
            if all((min(u, v), max(u, v)) in nn for u, v in zip(c, c[1:] + c[:1])) and frozenset(c) not in seen:
                seen.add(frozenset(c))
                out.append(tuple(c) + (x, y))
    return out


@pytest.mark.parametrize("opts,nplaq", [(dict(Lx=4, Ly=2, heisenberg=1.0), 3), (dict(Lx=6, Ly=2, heisenberg=1.0), 5), (dict(Lx=4, Ly=4, heisenberg=1.0), 12),
                                        (dict(Lx=3, Ly=3, heisenberg=1.0), 6), (dict(Lx=6, Ly=1, heisenberg=1.0), 0),
                                        (dict(Lx=4, Ly=2, heisenberg=1.0, BCperiodic=True), 3), (dict(Lx=4, Ly=3, heisenberg=1.0, BCopen=True), 6)])
def test_plaquettes_and_triangles(opts, nplaq):
    """On Ly = 2 the plaquette generated at y = 1 is the one of y = 0 again and is dropped; with three or more rows the last row closes
    round the cylinder; a chain has none; under open boundaries the wrapping row has no vertical edge and goes; x is never wrapped.
    Each plaquette gives its four triangles, three consecutive corners from corner `kind`, at the plaquette's position."""
    ham = J1J2XXZModel_SquareLattice(**opts)
    want = _plaquettes(ham)
    assert len(want) == nplaq
    out = _tool([_ham_line(opts), "plaquettes", "triangles"])
    assert out[0] == "rc 0"
    tok = out[1].split()
    assert tok[0] == "plaquettes" and [tuple(int(v) for v in t.split(",")) for t in tok[1:]] == want
    tok = out[2].split()
    tri = [(p[k], p[(k + 1) % 4], p[(k + 2) % 4], k, n, p[4], p[5]) for n, p in enumerate(want) for k in range(4)]
    assert tok[0] == "triangles" and [tuple(int(v) for v in t.split(",")) for t in tok[1:]] == tri
    for i, j, k, *_ in tri:
        assert len({i, j, k}) == 3


def _split(i, j, k, n_left, N):
    out = _tool([f"chiralsplit {i} {j} {k} {n_left} {N}"])
    tok = out[0].split()
    assert tok[0] == "chiralsplit" and len(tok) == 7
    strings = []
    for t in tok[1:]:
        c, left, right = t.split("|")
        strings.append((float(c), *[[] if p == "-" else [tuple(int(v) for v in f.split(":")) for f in p.split(",")] for p in (left, right)]))
    return strings


def test_the_six_strings_are_the_scalar_chirality():
    """With everything on the left (block site = lattice site) the six strings, multiplied out for three spins 1/2, give the real
    antisymmetric K with i K = S_0 . (S_1 x S_2), and chi^2 = 3/32 - (S_0.S_1 + S_1.S_2 + S_2.S_0) / 8."""
    sz, sp = np.array([[0.5, 0.0], [0.0, -0.5]]), np.array([[0.0, 1.0], [0.0, 0.0]])
    one = {OP_SZ: sz, OP_SP: sp, OP_SM: sp.T}

    def at(m, s):
        return np.kron(np.kron(m if s == 0 else np.eye(2), m if s == 1 else np.eye(2)), m if s == 2 else np.eye(2))
    K = np.zeros((8, 8))
    for c, left, right in _split(0, 1, 2, 3, 3):
        assert right == [] and len(left) == 3 and abs(c) == 0.5
        K += c * at(one[left[0][0]], left[0][1]) @ at(one[left[1][0]], left[1][1]) @ at(one[left[2][0]], left[2][1])
    sx, sy = 0.5 * (sp + sp.T), -0.5j * (sp - sp.T)
    S = [[at(m, s) for m in (sx, sy, sz)] for s in range(3)]
    cross = [S[1][1] @ S[2][2] - S[1][2] @ S[2][1], S[1][2] @ S[2][0] - S[1][0] @ S[2][2], S[1][0] @ S[2][1] - S[1][1] @ S[2][0]]
    chi = sum(S[0][a] @ cross[a] for a in range(3))
    assert np.abs(1j * K - chi).max() <= 1e-15 and np.array_equal(K.T, -K)
    dot = lambda a, b: sum(S[a][c] @ S[b][c] for c in range(3))          # noqa: E731
    assert np.abs(chi @ chi - (3.0 / 32.0 * np.eye(8) - (dot(0, 1) + dot(1, 2) + dot(2, 0)) / 8.0)).max() <= 1e-15


@pytest.mark.parametrize("tri,n_left,N", [((3, 4, 5), 4, 8), ((5, 2, 3), 4, 8), ((2, 1, 0), 4, 8), ((6, 5, 4), 4, 8), ((7, 8, 9), 6, 12), ((5, 6, 7), 6, 12)])
def test_strings_split_at_the_cut(tri, n_left, N):
    """Each side keeps its factors in their order in the string; a right factor names block site N - 1 - s; the parts together hold one
    Sz, one Sp and one Sm, so their sector shifts are opposite; a triangle inside one block leaves the other part empty."""
    i, j, k = tri
    rot = [(i, j, k), (i, j, k), (j, k, i), (j, k, i), (k, i, j), (k, i, j)]
    kinds = [(OP_SZ, OP_SP, OP_SM), (OP_SZ, OP_SM, OP_SP)] * 3
    for (c, left, right), sites, ops, sign in zip(_split(i, j, k, n_left, N), rot, kinds, [0.5, -0.5] * 3):
        assert c == sign
        want_left = [(o, s) for o, s in zip(ops, sites) if s < n_left]
        want_right = [(o, N - 1 - s) for o, s in zip(ops, sites) if s >= n_left]
        assert left == want_left and right == want_right
        assert sum(o for o, _ in left) == -sum(o for o, _ in right)
    n_in = sum(s < n_left for s in tri)
    assert all(len(left) == n_in for _, left, _ in _split(i, j, k, n_left, N))
