"""-chi_sites c0,c1,... and -chi_bonds b0,b1,... (-m gpu): the engine's static susceptibilities chi_ic = d<O_i>/dh_c
(StaticSusceptibility.json: the images Sz_i psi of all sites, D_b psi of all bonds, one dmrgx_kron_static_response solve per reference)
against exact diagonalisation of the 6 x 2 Heisenberg lattice, against -corr_dimer of the same run, and under truncation.

ED from the fixtures of test_gpu_dsf_sites.py (w, V, psi and the diagonals of Sz_i in the Sz = 0 sector, 924 states) and of
test_gpu_dsf_dimer.py (the components of D_b psi and of (D_b - <D_b>) psi along the eigenvectors):
    chi_ic = 2 sum_{n>0} <u_i|n><n|v> / (E_n - E0),   u_i = O_i psi,  v = O_c psi.
-mwarmup 64 keeps every state of a 6 x 2 lattice, so the engine's last superblock is the lattice itself.  The bound: the solver's
X - x* = A^-1 (A X - b) with lambda_min(A) >= gap_ED on the complement of psi gives |Chi - ED| <= 2 |u| |Q v| Residual / gap_ED; 1e-10 is
added for ED's own rounding."""
import json
import os

import numpy as np
import pytest

from test_gpu_engine import run_engine
from test_gpu_dsf import HEIS_6x2, _no_nan
from test_gpu_dsf_sites import heis_ed            # noqa: F401  (module-scoped fixtures, built once here)
from test_gpu_dsf_dimer import dimer_ed, _cosines, _same            # noqa: F401

pytestmark = pytest.mark.gpu
N, LX, LY, NB = 12, 6, 2, 16
TOL = 1e-8                                          # the default of -chi_tol


def _records(d, name="StaticSusceptibility.json"):
    return json.load(open(str(d) + "/" + name))


def _matmults(entries):
    """sum of n_matvec = blocks 8 + 1 over the solves, blocks = ceil(Iterations / 8), at least one"""
    return sum(max(1, -(-s["Iterations"] // 8)) * 8 + 1 for s in entries)


def _site_cosines(ham, c):
    """[q = nx Ly + ny][i] = cos(q . (r_i - r_c))"""
    r = np.array([ham.To2D(i) for i in range(N)], dtype=float)
    out = np.zeros((LX * LY, N))
    for nx in range(LX):
        for ny in range(LY):
            out[nx * LY + ny] = np.cos(2 * np.pi * (nx * (r[:, 0] - r[c, 0]) / LX + ny * (r[:, 1] - r[c, 1]) / LY))
    return out


def test_sites_and_bonds_against_exact_diagonalisation(tmp_path, heis_ed, dimer_ed):
    """-chi_sites 6,0 -chi_bonds <the first x bond, the first y bond>, nothing truncated, last record.  Chi against ED within the bound of
    the module docstring; Mean of a site 0 to 1e-10, of a bond D / Norm of -corr_dimer in the same run to 1e-10; ChiQ the cosine sum of
    Chi to 1e-13; ChiQ[q = 0] of a site 0 to 1e-10 (Sz_tot psi = 0 exactly in the sector basis); Chi[c][c] > 0; every solve converged
    with Residual <= 2 tol; MatMults = sum of n_matvec."""
    ed = dimer_ed
    refs = [ed["orient"].index("x"), ed["orient"].index("y")]
    run_engine(tmp_path, *HEIS_6x2, "-mwarmup", 64, "-chi_sites", "6,0", "-chi_bonds", ",".join(str(b) for b in refs), "-corr_dimer", 1)
    rec, dim = _records(tmp_path)[-1], _records(tmp_path, "DimerCorrelations.json")[-1]
    assert rec["GlobIdx"] == dim["GlobIdx"]
    assert _no_nan(rec) and rec["Tol"] == TOL and rec["MaxIt"] == 2000 and rec["tChi"] > 0.0
    assert abs(rec["Norm"] - 1.0) <= 1e-12 and abs(rec["E0"] - heis_ed["E0"]) <= 1e-10
    assert [s["Site"] for s in rec["Sites"]] == [6, 0] and [s["Bond"] for s in rec["Bonds"]] == refs
    assert rec["MatMults"] == _matmults(rec["Sites"] + rec["Bonds"])
    psi, szd, w, V = heis_ed["psi"], heis_ed["szd"], heis_ed["w"], heis_ed["V"]
    gap = w[1] - w[0]
    assert gap > 0.1
    inv = 1.0 / (w[1:] - w[0])
    Uv = (szd * psi[None, :]) @ V                                       # the components of Sz_i psi along the eigenvectors
    assert np.abs(Uv[:, 0]).max() <= 1e-10                              # <Sz_i> = 0
    for s in rec["Sites"]:
        c = s["Site"]
        chi, chiq = np.array(s["Chi"]), np.array(s["ChiQ"])
        assert s["r"] == list(heis_ed["ham"].To2D(c)) and chi.shape == (N,) and chiq.shape == (LX * LY,)
        want = 2.0 * (Uv[:, 1:] * inv[None, :]) @ Uv[c, 1:]
        nu, nqv = np.linalg.norm(Uv, axis=1), np.linalg.norm(Uv[c, 1:])
        bound = 2.0 * nu * nqv * s["Residual"] / gap + 1e-10
        print("site", c, "iterations", s["Iterations"], "Residual", s["Residual"], "Chi err", np.abs(chi - want).max(), "bound", bound.min(), "Chi[c]", chi[c], "ChiQ[0]", chiq[0])
        assert s["Converged"] == 1 and s["Residual"] <= 2.0 * TOL
        assert (np.abs(chi - want) <= bound).all()
        assert abs(s["Mean"]) <= 1e-10 and abs(s["Norm2"] - nqv ** 2) <= 1e-10
        assert np.abs(chiq - _site_cosines(heis_ed["ham"], c) @ chi).max() <= 1e-13
        assert abs(chiq[0]) <= 1e-10
        assert chi[c] > 0.0
    dU, rawU = ed["dU"], ed["rawU"]
    for s in rec["Bonds"]:
        c = s["Bond"]
        chi, chiq = np.array(s["Chi"]), np.array(s["ChiQ"])
        assert s["Sites"] == ed["bonds"][c] and s["Orientation"] == ed["orient"][c] and s["r"] == ed["pos"][c].astype(int).tolist()
        assert chi.shape == (NB,) and chiq.shape == (LX * LY,)
        want = 2.0 * (dU[:, 1:] * inv[None, :]) @ dU[c, 1:]
        nu, nqv = np.linalg.norm(rawU, axis=1), np.linalg.norm(dU[c, 1:])
        bound = 2.0 * nu * nqv * s["Residual"] / gap + 1e-10
        sel = _same(ed, c)
        print("bond", c, "iterations", s["Iterations"], "Residual", s["Residual"], "Chi err", np.abs(chi - want).max(), "bound", bound.min(), "Chi[c]", chi[c], "Mean", s["Mean"])
        assert s["Converged"] == 1 and s["Residual"] <= 2.0 * TOL
        assert (np.abs(chi - want) <= bound).all()
        assert abs(s["Mean"] - dim["D"][c] / dim["Norm"]) <= 1e-10 and abs(s["Mean"] - ed["D"][c]) <= 1e-10
        assert abs(s["Norm2"] - nqv ** 2) <= 1e-10
        assert np.abs(chiq - _cosines(ed["pos"], sel, c) @ chi[sel]).max() <= 1e-13
        assert chi[c] > 0.0


@pytest.fixture(scope="module")
def truncated_runs(tmp_path_factory):
    """-mwarmup 16: once alone, once with -chi_sites 6,0 -chi_bonds 0,7."""
    d = tmp_path_factory.mktemp("chi")
    rows_off, _, _ = run_engine(d / "off", *HEIS_6x2, "-mwarmup", 16)
    rows_on, _, _ = run_engine(d / "on", *HEIS_6x2, "-mwarmup", 16, "-chi_sites", "6,0", "-chi_bonds", "0,7")
    return d / "off", d / "on", rows_off, rows_on


def test_truncated_run(truncated_runs, heis_ed):
    """m = 16 cuts the basis: every solve of every record ends with Residual <= 2 tol, the q = 0 row of every site is still 0 to 1e-9
    (Sz_tot of the truncated operators still annihilates a state of the Sz = 0 sector), Chi[c][c] > 0, nothing is non-finite, ChiQ is the
    cosine sum of Chi, and MatMults = sum of n_matvec."""
    _, on, _, rows = truncated_runs
    assert any(r["NStates_SysRot"] < r["NStates_SysEnl"] for r in rows)
    recs = _records(on)
    assert len(recs) >= 1
    for rec in recs:
        assert _no_nan(rec) and [s["Site"] for s in rec["Sites"]] == [6, 0] and [s["Bond"] for s in rec["Bonds"]] == [0, 7]
        assert rec["MatMults"] == _matmults(rec["Sites"] + rec["Bonds"])
        for s in rec["Sites"] + rec["Bonds"]:
            print(rec["GlobIdx"], "site" if "Site" in s else "bond", s.get("Site", s.get("Bond")), "iterations", s["Iterations"], "Residual", s["Residual"], "ChiQ[0]", s["ChiQ"][0])
            assert s["Converged"] == 1 and s["Residual"] <= 2.0 * TOL
        for s in rec["Sites"]:
            chi = np.array(s["Chi"])
            assert abs(s["ChiQ"][0]) <= 1e-9 and chi[s["Site"]] > 0.0
            assert np.abs(np.array(s["ChiQ"]) - _site_cosines(heis_ed["ham"], s["Site"]) @ chi).max() <= 1e-13
        for s in rec["Bonds"]:
            assert np.array(s["Chi"])[s["Bond"]] > 0.0


def test_option_off_changes_nothing(truncated_runs):
    """Without the options the file does not appear, and the energies of DMRGSteps.json are the same bits: the measurement only reads."""
    off, on, rows_off, rows_on = truncated_runs
    assert not os.path.exists(str(off) + "/StaticSusceptibility.json") and os.path.exists(str(on) + "/StaticSusceptibility.json")
    assert len(rows_off) == len(rows_on) > 4
    assert [r["GSEnergy"] for r in rows_off] == [r["GSEnergy"] for r in rows_on]
    assert [r["TruncErr_Sys"] for r in rows_off] == [r["TruncErr_Sys"] for r in rows_on]
