"""What -dsf_dimer adds that needs no GPU: BondsOfOrientation of host/Measurements.hpp through the host tool, and dmrgx_vec_project_out in
the three places an ABI call has to appear (the header, the ctypes table)."""
import os
import re

import pytest

from oracle.hamiltonian import J1J2XXZModel_SquareLattice
from test_measurements_host import _ham_line, _tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bonds(ham):
    """The distinct pairs of NeighborPairs() in order of first appearance -> [(i, j, orientation, ix, jy)]: 'x' if the sites differ in
    column; (ix, jy) is the site whose right (x) or above (y) neighbour is the other one, the first of the pair where both are."""
    out, seen = [], set()
    for i, j in ham.NeighborPairs():
        if (i, j) in seen:
            continue
        seen.add((i, j))
        (x0, y0), (x1, y1) = ham.To2D(i), ham.To2D(j)
        o = "x" if x0 != x1 else "y"
        from_i = (x0 + 1) % ham.Lx() == x1 if o == "x" else (y0 + 1) % ham.Ly() == y1
        out.append((i, j, o) + ((x0, y0) if from_i else (x1, y1)))
    return out


@pytest.mark.parametrize("Lx,Ly,nbonds", [(4, 2, 10), (6, 2, 16), (6, 4, 44)])        # x bonds (Lx - 1) Ly, y bonds Lx Ly / 2 on Ly = 2 and Lx Ly on Ly = 4
def test_bonds_of_orientation(Lx, Ly, nbonds):
    """bondsof x / bondsof y: the indices of the bonds of that orientation in the order of the bond list, with their positions; the two
    lists are disjoint and cover every bond; any other letter selects nothing.  The restatement's bond list is the tool's own."""
    opts = dict(Lx=Lx, Ly=Ly, heisenberg=1.0)
    ham = J1J2XXZModel_SquareLattice(**opts)
    out, _ = _tool([_ham_line(opts), "bonds", "bondsof x", "bondsof y", "bondsof z"])
    assert out[0] == "rc 0"
    bonds = _bonds(ham)
    assert len(bonds) == nbonds
    assert out[1].split()[1:] == ["%d,%d,%s,%d,%d" % b for b in bonds]
    got = {}
    for line, o in zip(out[2:5], "xyz"):
        tok = line.split()
        assert tok[0] == "bondsof" and int(tok[1]) == len(tok) - 2
        got[o] = [tuple(int(v) for v in t.split(",")) for t in tok[2:]]
        assert got[o] == [(k, b[3], b[4]) for k, b in enumerate(bonds) if b[2] == o]
    assert got["z"] == [] and got["x"] and got["y"]
    assert sorted(k for o in "xy" for k, _, _ in got[o]) == list(range(nbonds))


def test_project_out_is_declared_bound_and_documented(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmrgx.h")).read(), flags=re.S)
    m = re.search(r"dmrgx_status\s+dmrgx_vec_project_out\s*\(([^)]*)\)", hdr)
    assert m and m.group(1).count(",") + 1 == 8
    res, args = pkg._capi.SIGNATURES["dmrgx_vec_project_out"]
    assert len(args) == 8
    assert hasattr(pkg._capi.lib(), "dmrgx_vec_project_out")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    calls = re.findall(r"\bdmrgx_vec_project_out\(([^()]*)\)", doc)
    assert calls and all(c.count(",") + 1 == 8 for c in calls)
    from dmrgx_amd import superblock
    assert callable(superblock.vec_project_out)
