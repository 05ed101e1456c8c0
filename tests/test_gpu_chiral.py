"""-corr_chiral 1 (-m gpu): the engine's table < chi_a chi_b > of the scalar chirality chi_ijk = S_i . (S_j x S_k) = i K_ijk over all pairs of
triangles of the lattice's plaquettes (ChiralCorrelations.json: dmrgx_secop_compose for the operator products inside a block, one
dmrgx_kron_term_gram call per measurement) against exact diagonalisation of the lattice, against the operator identity
chi^2 = 3/32 - (S_i.S_j + S_j.S_k + S_k.S_i) / 8 on the spin tables of the same run, and against the inequalities a Gram matrix obeys
under truncation."""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle.hamiltonian import J1J2XXZModel_SquareLattice
from oracle.qn import OpSm, OpSp, OpSz
from helpers import lattice_ground_state
from test_gpu_engine import EXE, run_engine

pytestmark = pytest.mark.gpu

HEIS_4x2 = ["-Lx", 4, "-Ly", 2, "-heisenberg", 1, "-mwarmup", 64, "-nsweeps", 1, "-H_eps_tol", 1e-13]
# (next-nearest terms exist only when both -J2 and -Jz2 are non-zero: the model's documented quirk)
J1J2_6x2 = ["-Lx", 6, "-Ly", 2, "-J1", 1, "-Jz1", 1, "-J2", 0.5, "-Jz2", 0.5, "-nsweeps", 1, "-H_eps_tol", 1e-12]


def plaquettes_and_triangles(ham):
    """The convention, restated from the oracle Hamiltonian: a plaquette is a = (x, y), b = (x + 1, y), c = (x + 1, y + 1), d = (x, y + 1)
    with y + 1 round the periodic direction, all four edges among the distinct nearest-neighbour pairs, in order of (x, y), each site set
    once; its triangles are kind 0 .. 3 = (a, b, c), (b, c, d), (c, d, a), (d, a, b) at the position of a.
    -> (plaquettes [[a, b, c, d]], their positions [[x, y]], triangles [[i, j, k]], kinds, positions, plaquette of every triangle)."""
    Lx, Ly = ham.Lx(), ham.Ly()
    site = {tuple(ham.To2D(s)): s for s in range(ham.NumSites())}
    nn = {(min(p), max(p)) for p in ham.NeighborPairs()}
    plaq, ppos, seen = [], [], set()
    for x in range(Lx - 1):
        for y in range(Ly):
            corners = [site[(x, y)], site[(x + 1, y)], site[(x + 1, (y + 1) % Ly)], site[(x, (y + 1) % Ly)]]
            edges = [(min(u, v), max(u, v)) for u, v in zip(corners, corners[1:] + corners[:1])]
            if all(e in nn for e in edges) and frozenset(corners) not in seen:
                seen.add(frozenset(corners))
                plaq.append(corners)
                ppos.append([x, y])
    tri = [[p[k], p[(k + 1) % 4], p[(k + 2) % 4]] for p in plaq for k in range(4)]
    kind = [k for _ in plaq for k in range(4)]
    tpos = [xy for xy in ppos for _ in range(4)]
    of = [n for n in range(len(plaq)) for _ in range(4)]
    return plaq, ppos, tri, kind, tpos, of


def K_images(site_op, psi, triangles):
    """Rows K_a psi,  K_ijk = [ Sz_i (P_j M_k - M_j P_k) + Sz_j (P_k M_i - M_k P_i) + Sz_k (P_i M_j - M_i P_j) ] / 2."""
    def pm(a, b, c):
        return site_op(OpSz, a) @ (site_op(OpSp, b) @ (site_op(OpSm, c) @ psi) - site_op(OpSm, b) @ (site_op(OpSp, c) @ psi))
    return np.array([0.5 * (pm(i, j, k) + pm(j, k, i) + pm(k, i, j)) for i, j, k in triangles])


_exact = {}


def exact_table(key, ham):
    """(K [nt], CC [nt][nt]) of the lattice ground state from dense ED; computed once per lattice, read-only."""
    if key not in _exact:
        _, psi, site_op = lattice_ground_state(ham)
        V = K_images(site_op, psi, plaquettes_and_triangles(ham)[2])
        K, CC = V @ psi, V @ V.T
        for a in (K, CC):
            a.setflags(write=False)
        _exact[key] = (K, CC)
    return _exact[key]


def _records(d, name="ChiralCorrelations.json"):
    recs = json.load(open(str(d) + "/" + name))
    return [{k: (np.array(v, dtype=float) if isinstance(v, list) and k != "Orientation" else v) for k, v in r.items()} for r in recs]


def _check_record(ham, rec, nplaq):
    """Triangles, kinds, positions, plaquettes and shapes against the restated convention; CC a Gram matrix -- bitwise symmetric, positive
    semi-definite, Cauchy-Schwarz against psi --; PlaquetteCC and StructureFactor recomputed from the record."""
    plaq, ppos, tri, kind, tpos, of = plaquettes_and_triangles(ham)
    nt = len(tri)
    assert len(plaq) == nplaq and nt == 4 * nplaq
    assert rec["Triangles"].astype(int).tolist() == tri and rec["Kind"].astype(int).tolist() == kind and rec["Position"].astype(int).tolist() == tpos
    assert rec["Plaquettes"].astype(int).tolist() == plaq and rec["PlaquettePosition"].astype(int).tolist() == ppos
    assert rec["K"].shape == (nt,) and rec["CC"].shape == (nt, nt) and rec["PlaquetteCC"].shape == (nplaq, nplaq)
    assert rec["StructureFactor"].shape == (ham.Lx(), ham.Ly()) and rec["tChiral"] > 0.0
    CC = rec["CC"]
    assert np.array_equal(CC, CC.T)
    assert np.linalg.eigvalsh(CC).min() >= -1e-12
    assert (np.diag(CC) * rec["Norm"] >= rec["K"] ** 2 - 1e-12).all()
    sel = np.zeros((nplaq, nt))
    sel[of, np.arange(nt)] = 1.0
    pcc = sel @ CC @ sel.T
    assert np.abs(rec["PlaquetteCC"] - pcc).max() <= 1e-12
    r = np.array(ppos, dtype=float)
    S = np.zeros((ham.Lx(), ham.Ly()))
    for nx in range(ham.Lx()):
        for ny in range(ham.Ly()):
            ph = r @ (2.0 * np.pi * np.array([nx / ham.Lx(), ny / ham.Ly()]))
            S[nx, ny] = (np.cos(ph[:, None] - ph[None, :]) * pcc).sum() / rec["Norm"] / nplaq
    assert np.abs(rec["StructureFactor"] - S).max() <= 1e-12


def _sides(ham, triangles):
    """Where a triangle sits at the centre cut (the left block holds the first half of the sites): 0 / 1 inside the left / right block,
    2: two sites left, 3: one site left."""
    half = ham.NumSites() // 2
    return [{3: 0, 0: 1, 2: 2, 1: 3}[sum(s < half for s in t)] for t in triangles]


def _same_bits(a, b, skip):
    assert set(a) == set(b)
    for k in a:
        if k not in skip:
            assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name,opts,model,nplaq,offdiag", [
    ("heis4x2", HEIS_4x2, dict(Lx=4, Ly=2, heisenberg=1.0), 3, 0.180),
    ("j1j2_6x2", J1J2_6x2 + ["-mwarmup", 64], dict(Lx=6, Ly=2, J1=1, Jz1=1, J2=0.5, Jz2=0.5), 5, 0.1875)])
def test_untruncated_lattices_against_exact_diagonalisation(tmp_path, name, opts, model, nplaq, offdiag):
    """m = 64 keeps everything (2^3 and 2^6 states per block): CC of the last record is the exact ground-state table (1e-10, as for the
    spin tables), K vanishes, and CC[a][a] / Norm obeys chi^2 = 3/32 - (S_i.S_j + S_j.S_k + S_k.S_i) / 8 on SpinCorrelations.json of the
    same run.  Without the option no ChiralCorrelations.json appears and the other records carry the same bits with it."""
    run_engine(tmp_path / "off", *opts, "-corr_matrix", 1, "-corr_dimer", 1)
    run_engine(tmp_path / "on", *opts, "-corr_matrix", 1, "-corr_dimer", 1, "-corr_chiral", 1)
    assert not os.path.exists(str(tmp_path / "off") + "/ChiralCorrelations.json")
    ham = J1J2XXZModel_SquareLattice(**model)
    K, CC = exact_table(name, ham)
    off = np.abs(CC - np.diag(np.diag(CC)))
    # what the comparison is worth: the ED values themselves
    print(name, "ED: largest off-diagonal |CC|", off.max(), "diagonal", np.diag(CC).min(), np.diag(CC).max(), "|K|", np.abs(K).max())
    assert abs(off.max() - offdiag) <= 1e-3 and off.max() > 0.01 and np.abs(K).max() <= 1e-12
    recs = _records(tmp_path / "on")
    corr_on, corr_off = (json.load(open(str(tmp_path / d) + "/Correlations.json")) for d in ("on", "off"))
    assert len(recs) == len(corr_on["values"]) == 2                          # one record per measurement: warm-up, sweep
    rec = recs[-1]
    _check_record(ham, rec, nplaq)
    print(name, "engine: |CC - ED|", np.abs(rec["CC"] - CC).max(), "|K|", np.abs(rec["K"]).max(), "tChiral", [r["tChiral"] for r in recs])
    assert np.abs(rec["CC"] - CC).max() <= 1e-10
    assert np.abs(rec["K"]).max() <= 1e-10
    assert abs(rec["Norm"] - 1.0) <= 1e-12
    spin = _records(tmp_path / "on", "SpinCorrelations.json")[-1]
    assert spin["GlobIdx"] == rec["GlobIdx"]
    SS = spin["SS"]                                                          # < S_i . S_j >, not yet divided by the norm
    for a, (i, j, k) in enumerate(rec["Triangles"].astype(int)):
        want = 3.0 / 32.0 - (SS[i, j] + SS[j, k] + SS[k, i]) / spin["Norm"] / 8.0
        assert abs(rec["CC"][a, a] / rec["Norm"] - want) <= 1e-10, (a, i, j, k, rec["CC"][a, a], want)
    sides = _sides(ham, rec["Triangles"].astype(int).tolist())
    assert rec["Side"].astype(int).tolist() == sides
    if name == "j1j2_6x2":
        assert set(sides) == {0, 1, 2, 3}                                     # wholly left, wholly right, 2 + 1 and 1 + 2 across the cut
    # the other records: bit for bit what the run without the option wrote
    assert corr_on == corr_off
    for other, clock in (("SpinCorrelations.json", "tCorrMatrix"), ("DimerCorrelations.json", "tDimer")):
        on, offr = _records(tmp_path / "on", other), _records(tmp_path / "off", other)
        assert len(on) == len(offr) == 2
        for a, b in zip(on, offr):
            _same_bits(a, b, (clock,))


def test_j1j2_6x2_truncated_is_a_gram_matrix(tmp_path):
    """A run whose basis is cut to m = 24 states: CC is a Gram matrix whatever was truncated.  K, the expectation value of an antisymmetric
    operator, is zero only as far as the truncated operators still are antisymmetric: it is recorded, not bounded."""
    rows, _, _ = run_engine(tmp_path, *J1J2_6x2, "-mwarmup", 24, "-corr_chiral", 1, "-corr_dimer", 1)
    assert any(r["NStates_SysRot"] < r["NStates_SysEnl"] for r in rows)        # m = 24 cuts the basis
    ham = J1J2XXZModel_SquareLattice(Lx=6, Ly=2, J1=1, Jz1=1, J2=0.5, Jz2=0.5)
    recs, dimer = _records(tmp_path), _records(tmp_path, "DimerCorrelations.json")
    assert len(recs) == len(dimer) == 2
    for rec, dim in zip(recs, dimer):
        assert rec["GlobIdx"] == dim["GlobIdx"]
        _check_record(ham, rec, 5)
        assert np.diag(rec["CC"]).min() > 0.01
        print("6x2 m=24: |K| max", np.abs(rec["K"]).max(), "tChiral", rec["tChiral"], "tDimer", dim["tDimer"])


def test_4x4_periodic_wrap(tmp_path):
    """Four rows: the plaquettes of the last row close round the cylinder (y + 1 = 0) and are plaquettes of their own, 3 columns x 4 rows."""
    run_engine(tmp_path, "-Lx", 4, "-Ly", 4, "-heisenberg", 1, "-mwarmup", 16, "-nsweeps", 1, "-corr_chiral", 1, "-corr_dimer", 1)
    ham = J1J2XXZModel_SquareLattice(Lx=4, Ly=4, heisenberg=1.0)
    plaq, ppos = plaquettes_and_triangles(ham)[:2]
    assert len(plaq) == 12 and [p for p in ppos if p[1] == 3] == [[0, 3], [1, 3], [2, 3]]
    recs, dimer = _records(tmp_path), _records(tmp_path, "DimerCorrelations.json")
    for rec, dim in zip(recs, dimer):
        _check_record(ham, rec, 12)
        print("4x4 m=16: |K| max", np.abs(rec["K"]).max(), "tChiral", rec["tChiral"], "tDimer", dim["tDimer"])
    assert set(recs[-1]["Side"].astype(int).tolist()) == {0, 1, 2, 3}


def test_two_ranks_are_refused_at_start_up(tmp_path):
    """-corr_chiral 1 on two ranks ends with the refusal message on every rank: no hang, no output of a half-run."""
    d = str(tmp_path) + "/"
    cmd = [EXE, *[str(o) for o in HEIS_4x2], "-corr_chiral", "1", "-data_dir", d]
    name = "dmrgx_test_chiral_%d" % os.getpid()
    procs = [subprocess.Popen(cmd, env=dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", DMRGX_COMM="shm", DMRGX_SHM_NAME=name, DMRGX_SHM_MB="64"),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    try:
        outs = [pr.communicate(timeout=120)[0] for pr in procs]
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    for pr, o in zip(procs, outs):
        assert pr.returncode not in (0, None) and pr.returncode > 0, o[-2000:]
        assert "-corr_chiral 1 is not available on more than one rank" in o, o[-2000:]
    assert not os.path.exists(d + "ChiralCorrelations.json")
