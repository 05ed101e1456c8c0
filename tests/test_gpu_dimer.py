"""-corr_dimer 1 (-m gpu): the engine's dimer-dimer table < D_b D_b' > over all pairs of nearest-neighbour bonds, D_b = S_i . S_j
(DimerCorrelations.json, one dmrgx_kron_term_gram call per measurement) against exact diagonalisation of the lattice, against the
all-pairs spin tables of the same run, and against the inequalities a Gram matrix obeys under truncation."""
import json
import os

import numpy as np
import pytest

from oracle.hamiltonian import J1J2XXZModel_SquareLattice
from oracle.qn import OpSm, OpSp, OpSz
from helpers import lattice_ground_state
from test_gpu_engine import run_engine

pytestmark = pytest.mark.gpu

HEIS_4x2 = ["-Lx", 4, "-Ly", 2, "-heisenberg", 1, "-mwarmup", 64, "-nsweeps", 1, "-H_eps_tol", 1e-13]
# (next-nearest terms exist only when both -J2 and -Jz2 are non-zero: the model's documented quirk)
J1J2_6x2 = ["-Lx", 6, "-Ly", 2, "-J1", 1, "-Jz1", 1, "-J2", 0.5, "-Jz2", 0.5, "-mwarmup", 24, "-nsweeps", 1, "-H_eps_tol", 1e-12]


def _records(d, name="DimerCorrelations.json"):
    recs = json.load(open(str(d) + "/" + name))
    return [{k: (np.array(v, dtype=float) if isinstance(v, list) and k not in ("Orientation",) else v) for k, v in r.items()} for r in recs]


def _bonds(ham):
    """The distinct nearest-neighbour pairs in order of first appearance -> ([[i, j]], [orientation], [[ix, jy] of the site that generates it])."""
    bonds, orient, pos = [], [], []
    for s in range(ham.NumSites()):
        ix, jy = ham.To2D(s)
        for n in ham._nn(ix, jy, ham.NumSites()):
            p = [min(n, s), max(n, s)]
            if p in bonds:
                continue
            bonds.append(p)
            orient.append("x" if ham.To2D(n)[0] != ix else "y")
            pos.append([ix, jy])
    assert bonds == [p for k, p in enumerate(ham.NeighborPairs()) if p not in ham.NeighborPairs()[:k]]
    return bonds, orient, pos


_exact = {}


def _exact_tables(key, ham, spin="1/2"):
    """(D [nb], DD [nb][nb]) of the lattice ground state from dense ED, D_b = Sz_i Sz_j + (Sp_i Sm_j + Sm_i Sp_j) / 2 from the site
    operators of helpers.lattice_ground_state; computed once per lattice."""
    if key not in _exact:
        _, psi, site_op = lattice_ground_state(ham, spin=spin)
        V = np.array([site_op(OpSz, i) @ (site_op(OpSz, j) @ psi) + 0.5 * (site_op(OpSp, i) @ (site_op(OpSm, j) @ psi) + site_op(OpSm, i) @ (site_op(OpSp, j) @ psi))
                      for i, j in _bonds(ham)[0]])
        _exact[key] = (V @ psi, V @ V.T)
    return _exact[key]


def _structure_factor(ham, rec, which):
    Lx, Ly = ham.Lx(), ham.Ly()
    sel = [b for b, o in enumerate(rec["Orientation"]) if o == which]
    S = np.zeros((Lx, Ly))
    if not sel:
        return S
    r = rec["Position"][sel]
    C = rec["Connected"][np.ix_(sel, sel)]
    for nx in range(Lx):
        for ny in range(Ly):
            ph = r @ (2.0 * np.pi * np.array([nx / Lx, ny / Ly]))
            S[nx, ny] = (np.cos(ph[:, None] - ph[None, :]) * C).sum() / len(sel)
    return S


def _check_record_shape(ham, rec, connected_tol=None):
    """Bonds, orientations, positions and shapes; Connected = DD / Norm - D D^T / Norm^2 and both structure factors recomputed from the
    record.  connected_tol None: the bound that follows from the 15 significant digits the record is written with -- every number read
    back is within 5e-15 of itself relatively, Norm enters DD / Norm once and D D^T / Norm^2 twice, D twice."""
    bonds, orient, pos = _bonds(ham)
    nb = len(bonds)
    assert rec["Bonds"].astype(int).tolist() == bonds and rec["Orientation"] == orient and rec["Position"].astype(int).tolist() == pos
    assert rec["D"].shape == (nb,) and rec["DD"].shape == rec["Connected"].shape == (nb, nb)
    assert rec["StructureFactorX"].shape == rec["StructureFactorY"].shape == (ham.Lx(), ham.Ly())
    assert rec["tDimer"] > 0.0
    dd, outer = rec["DD"] / rec["Norm"], np.outer(rec["D"], rec["D"]) / rec["Norm"] ** 2
    if connected_tol is None:
        connected_tol = 5e-15 * (np.abs(rec["Connected"]) + 2.0 * np.abs(dd) + 4.0 * np.abs(outer)) + 4.0 * np.finfo(float).eps * (np.abs(dd) + np.abs(outer))
    assert (np.abs(rec["Connected"] - (dd - outer)) <= connected_tol).all(), np.abs(rec["Connected"] - (dd - outer)).max()
    for which in "xy":
        assert np.abs(rec["StructureFactor" + which.upper()] - _structure_factor(ham, rec, which)).max() <= 1e-12


@pytest.mark.parametrize("ranks", [1, 2])
def test_heisenberg_4x2_against_exact_diagonalisation(tmp_path, ranks):
    """m = 64 keeps everything: D and DD of the last record are exact ground-state expectation values (1e-10, as for the spin tables).
    The ten bonds are the distinct pairs of the fourteen NeighborPairs() (Ly = 2, periodic: every vertical pair twice).  Without the
    option no DimerCorrelations.json appears, and Correlations.json and SpinCorrelations.json carry the same values with it."""
    run_engine(tmp_path / "off", *HEIS_4x2, "-corr_matrix", 1, ranks=ranks)
    run_engine(tmp_path / "on", *HEIS_4x2, "-corr_matrix", 1, "-corr_dimer", 1, ranks=ranks)
    assert not os.path.exists(str(tmp_path / "off") + "/DimerCorrelations.json")
    ham = J1J2XXZModel_SquareLattice(Lx=4, Ly=2, heisenberg=1.0)
    assert len(ham.NeighborPairs()) == 14 and len(_bonds(ham)[0]) == 10
    D, DD = _exact_tables("heis4x2", ham)
    conn = DD - np.outer(D, D)
    off_diag = np.abs(conn - np.diag(np.diag(conn)))
    # what the comparison is worth: the ED values themselves
    assert abs(D.min() + 0.687) <= 1e-3 and abs(D.max() + 0.219) <= 1e-3 and abs(off_diag.max() - 0.229) <= 1e-3 and off_diag.max() > 0.2
    recs = _records(tmp_path / "on")
    corr_on, corr_off = (json.load(open(str(tmp_path / d) + "/Correlations.json")) for d in ("on", "off"))
    assert len(recs) == len(corr_on["values"]) == 2                          # one record per measurement: warm-up, sweep
    rec = recs[-1]
    _check_record_shape(ham, rec, connected_tol=1e-14)
    assert np.abs(rec["D"] - D).max() <= 1e-10 and np.abs(rec["DD"] - DD).max() <= 1e-10
    assert abs(rec["Norm"] - 1.0) <= 1e-12
    assert corr_on == corr_off
    spin_on, spin_off = (_records(tmp_path / d, "SpinCorrelations.json") for d in ("on", "off"))
    assert len(spin_on) == len(spin_off) == 2
    for a, b in zip(spin_on, spin_off):
        assert set(a) == set(b)
        for k in a:
            if k != "tCorrMatrix":
                assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("sector", [(), ("-qn_sector", 1)])
def test_j1j2_6x2_truncated_against_the_spin_tables(tmp_path, sector):
    """A run whose basis is cut to m = 24 states: D_b multiplies the same truncated operators in the same order as the all-pairs spin
    tables, so < D_b > = SzSz[i][j] + (SpSm[i][j] + SmSp[i][j]) / 2 of the same measurement (1e-12), for bonds inside a block and across
    the cut alike.  DD is a Gram matrix whatever was truncated: bitwise symmetric, positive semi-definite, and Cauchy-Schwarz against
    psi bounds its diagonal from below."""
    rows, _, _ = run_engine(tmp_path, *J1J2_6x2, *sector, "-corr_matrix", 1, "-corr_dimer", 1)
    assert any(r["NStates_SysRot"] < r["NStates_SysEnl"] for r in rows)        # m = 24 cuts the basis
    ham = J1J2XXZModel_SquareLattice(Lx=6, Ly=2, J1=1, Jz1=1, J2=0.5, Jz2=0.5)
    recs, spins = _records(tmp_path), _records(tmp_path, "SpinCorrelations.json")
    corr = json.load(open(str(tmp_path) + "/Correlations.json"))
    assert len(recs) == len(spins) == len(corr["values"]) == 2
    for rec, spin in zip(recs, spins):
        assert rec["GlobIdx"] == spin["GlobIdx"]
        _check_record_shape(ham, rec)
        for b, (i, j) in enumerate(rec["Bonds"].astype(int)):
            want = spin["SzSz"][i, j] + 0.5 * (spin["SpSm"][i, j] + spin["SmSp"][i, j])
            assert abs(rec["D"][b] - want) <= 1e-12, (b, i, j, rec["D"][b], want)
        assert np.abs(rec["D"]).max() > 0.2
        assert np.array_equal(rec["DD"], rec["DD"].T)
        assert np.linalg.eigvalsh(rec["DD"]).min() >= -1e-12
        assert (np.diag(rec["DD"]) * rec["Norm"] >= rec["D"] ** 2 - 1e-12).all()


@pytest.mark.parametrize("name,opts,spin,lx,lo,hi", [
    ("chain8", ["-Lx", 8, "-Ly", 1, "-heisenberg", 1, "-mwarmup", 64], "1/2", 8, -0.661, -0.284),
    ("spin1", ["-spin", 1, "-Lx", 6, "-Ly", 1, "-heisenberg", 1, "-mwarmup", 100], "1", 6, -1.689, -1.229)])
def test_open_chains_against_exact_diagonalisation(tmp_path, name, opts, spin, lx, lo, hi):
    """Open chains, nothing truncated (spin 1/2 and spin 1): every bond is an x bond, the y structure factor an Lx x 1 table of zeros."""
    run_engine(tmp_path, *opts, "-nsweeps", 1, "-H_eps_tol", 1e-13, "-corr_dimer", 1)
    ham = J1J2XXZModel_SquareLattice(Lx=lx, Ly=1, heisenberg=1.0)
    D, DD = _exact_tables(name, ham, spin=spin)
    assert abs(D.min() - lo) <= 1e-3 and abs(D.max() - hi) <= 1e-3
    rec = _records(tmp_path)[-1]
    _check_record_shape(ham, rec)
    assert np.abs(rec["D"] - D).max() <= 1e-10 and np.abs(rec["DD"] - DD).max() <= 1e-10
    assert rec["Orientation"] == ["x"] * (lx - 1)
    assert rec["StructureFactorY"].shape == (lx, 1) and not rec["StructureFactorY"].any()
    assert not os.path.exists(str(tmp_path) + "/SpinCorrelations.json")
