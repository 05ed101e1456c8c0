"""-corr_matrix 1 (-m gpu): the engine's all-pairs tables <Sz_i Sz_j>, <Sm_i Sp_j>, <Sp_i Sm_j>, <S_i . S_j> and the structure factor
(SpinCorrelations.json, one dmrgx_kron_op_gram call per table and measurement) against exact diagonalisation of the lattice, against the
registered correlators of the same run, and against the sum rules that hold under truncation."""
import json
import os

import numpy as np
import pytest

from oracle.hamiltonian import J1J2XXZModel_SquareLattice
from oracle.qn import OpSm, OpSp, OpSz
from helpers import lattice_ground_state, parse_desc2
from test_gpu_engine import run_engine

pytestmark = pytest.mark.gpu

HEIS_4x2 = ["-Lx", 4, "-Ly", 2, "-heisenberg", 1, "-mwarmup", 64, "-nsweeps", 1, "-H_eps_tol", 1e-13]
J1J2_6x2 = ["-Lx", 6, "-Ly", 2, "-J1", 1, "-Jz1", 1, "-J2", 0.5, "-Jz2", 0.5, "-mwarmup", 24, "-nsweeps", 1, "-H_eps_tol", 1e-12]


def _records(d):
    recs = json.load(open(str(d) + "/SpinCorrelations.json"))
    return [{k: (np.array(v, dtype=float) if isinstance(v, list) else v) for k, v in r.items()} for r in recs]


def _exact_tables(ham, spin="1/2"):
    """(Sz [N], SzSz, SmSp, SpSm [N][N]) of the lattice ground state from dense ED: <Sm_i Sp_j> = <Sp_i psi, Sp_j psi>,
    <Sp_i Sm_j> = <Sm_i psi, Sm_j psi>."""
    _, psi, site_op = lattice_ground_state(ham, spin=spin)
    N = ham.NumSites()
    vz = np.array([site_op(OpSz, i) @ psi for i in range(N)])
    vp = np.array([site_op(OpSp, i) @ psi for i in range(N)])
    vm = np.array([site_op(OpSm, i) @ psi for i in range(N)])
    return vz @ psi, vz @ vz.T, vp @ vp.T, vm @ vm.T


def _structure_factor(ham, SS):
    Lx, Ly, N = ham.Lx(), ham.Ly(), ham.NumSites()
    r = np.array([ham.To2D(i) for i in range(N)], dtype=float)
    S = np.zeros((Lx, Ly))
    for nx in range(Lx):
        for ny in range(Ly):
            q = 2.0 * np.pi * np.array([nx / Lx, ny / Ly])
            ph = r @ q
            S[nx, ny] = (np.cos(ph[:, None] - ph[None, :]) * SS).sum() / N
    return S


@pytest.mark.parametrize("ranks", [1, 2])
def test_heisenberg_4x2_against_exact_diagonalisation(tmp_path, ranks):
    """m = 64 keeps everything: every entry of Sz, SzSz and SmSp of the last record is an exact ground-state expectation value (1e-10,
    as for the registered correlators); the norm, the structure factor recomputed from SS, the singlet sum rule sum_ij SS_ij = S(S+1) = 0
    and sum_q S(q) = sum_i SS_ii.  Without the option no SpinCorrelations.json appears, and Correlations.json is the same with it."""
    run_engine(tmp_path / "off", *HEIS_4x2, ranks=ranks)
    run_engine(tmp_path / "on", *HEIS_4x2, "-corr_matrix", 1, ranks=ranks)
    assert not os.path.exists(str(tmp_path / "off") + "/SpinCorrelations.json")
    ham = J1J2XXZModel_SquareLattice(Lx=4, Ly=2, heisenberg=1.0)
    N = ham.NumSites()
    sz, szsz, smsp, spsm = _exact_tables(ham)
    recs = _records(tmp_path / "on")
    corr_on, corr_off = (json.load(open(str(tmp_path / d) + "/Correlations.json")) for d in ("on", "off"))
    assert len(recs) == len(corr_on["values"]) == 2                          # one record per measurement: warm-up, sweep
    rec = recs[-1]
    assert rec["SzSz"].shape == rec["SmSp"].shape == rec["SS"].shape == (N, N) and rec["Sz"].shape == (N,) and rec["StructureFactor"].shape == (4, 2)
    assert np.abs(rec["Sz"] - sz).max() <= 1e-10 and np.abs(rec["SzSz"] - szsz).max() <= 1e-10 and np.abs(rec["SmSp"] - smsp).max() <= 1e-10
    assert np.abs(rec["SpSm"] - spsm).max() <= 1e-10
    assert np.abs(szsz).max() > 0.2 and np.abs(smsp).max() > 0.4
    assert abs(rec["Norm"] - 1.0) <= 1e-12
    want_ss = rec["SzSz"] + rec["SmSp"] + np.diag(rec["Sz"])
    assert np.abs(rec["SS"] - want_ss).max() <= 1e-14
    assert np.abs(rec["StructureFactor"] - _structure_factor(ham, rec["SS"])).max() <= 1e-12
    assert abs(rec["SS"].sum()) <= 1e-9
    assert abs(rec["StructureFactor"].sum() - np.trace(rec["SS"])) <= 1e-12
    assert abs(np.trace(rec["SS"]) - 0.75 * N) <= 1e-10                      # S(S+1) per site
    assert corr_on == corr_off


def _measured_ops(desc3, N):
    """'< ( Sz_{5} Sz_{4} ) (x) ( 1 ) >' -> [(OpSz, 5), (OpSz, 4)] in lattice sites: the operators a registered correlator is really
    measured with -- left-block sites as they are, right-block site s as lattice site N - 1 - s.  A correlator whose sites all lie in
    the right half is measured on the LEFT block at the mirrored sites (SetUpCorrelation: reflection symmetry), which is the same number
    only for a reflection-symmetric state; desc3 says what was done."""
    sys_part, env_part = desc3.split("(x)")
    return parse_desc2(sys_part) + [(op, N - 1 - s) for op, s in parse_desc2(env_part)]


def _matrix_entry(rec, ops):
    """The entry of the record's tables that equals the correlator of `ops` (one Sz, or a pair on different sites, in this order)."""
    if len(ops) == 1 and ops[0][0] == OpSz:
        return rec["Sz"][ops[0][1]]
    (a, i), (b, j) = ops
    assert i != j
    if (a, b) == (OpSz, OpSz):
        return rec["SzSz"][i, j]
    if (a, b) == (OpSm, OpSp):
        return rec["SmSp"][i, j]
    if (a, b) == (OpSp, OpSm):                                               # (not SmSp[j, i]: truncated operators of one block do not commute)
        return rec["SpSm"][i, j]
    raise AssertionError(ops)


@pytest.mark.parametrize("sector,sz_tot", [((), 0.0), (("-qn_sector", 1), 1.0)])
def test_j1j2_6x2_truncated_against_the_registered_correlators(tmp_path, sector, sz_tot):
    """A run whose basis is cut to m = 24 states: the tables use the same truncated operators as the registered
    correlators, so every NearestNeighbor... and Magnetization(i) value of Correlations.json equals its matrix entry (1e-12), and
    sum_ij SzSz_ij = Sz_tot^2 exactly: the site Sz operators of a block add up to the sector's Sz whatever was truncated."""
    rows, _, _ = run_engine(tmp_path, *J1J2_6x2, *sector, "-corr_matrix", 1)
    assert any(r["NStates_SysRot"] < r["NStates_SysEnl"] for r in rows)        # m = 24 cuts the basis
    recs = _records(tmp_path)
    corr = json.load(open(str(tmp_path) + "/Correlations.json"))
    assert len(recs) == len(corr["values"]) == 2
    checked = 0
    for rec, values in zip(recs, corr["values"]):
        for c, v in zip(corr["info"], values):
            if c["name"].startswith("NearestNeighbor") or c["name"].startswith("Magnetization("):
                got = _matrix_entry(rec, _measured_ops(c["desc3"], 12))
                assert abs(got - v) <= 1e-12, (c["name"], got, v)
                checked += 1
        assert abs(rec["SzSz"].sum() - sz_tot ** 2) <= 1e-11, rec["SzSz"].sum()
        assert abs(rec["Sz"].sum() - sz_tot) <= 1e-11
    ham = J1J2XXZModel_SquareLattice(Lx=6, Ly=2, J1=1, Jz1=1, J2=0.5, Jz2=0.5)
    assert checked == 2 * (6 + 3 * len(ham.NeighborPairs()))


def test_spin_one_chain_against_exact_diagonalisation(tmp_path):
    """-spin 1, six sites, nothing truncated: SzSz and SmSp against dense ED of the 3^6 lattice."""
    run_engine(tmp_path, "-spin", 1, "-Lx", 6, "-Ly", 1, "-heisenberg", 1, "-mwarmup", 100, "-nsweeps", 1, "-H_eps_tol", 1e-13, "-corr_matrix", 1)
    ham = J1J2XXZModel_SquareLattice(Lx=6, Ly=1, heisenberg=1.0)
    sz, szsz, smsp, spsm = _exact_tables(ham, spin="1")
    rec = _records(tmp_path)[-1]
    assert np.abs(rec["SzSz"] - szsz).max() <= 1e-10 and np.abs(rec["SmSp"] - smsp).max() <= 1e-10 and np.abs(rec["Sz"] - sz).max() <= 1e-10
    assert np.abs(rec["SpSm"] - spsm).max() <= 1e-10
    assert abs(np.trace(rec["SS"]) - 2.0 * 6) <= 1e-9                         # S(S+1) = 2 per site
