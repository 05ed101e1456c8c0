"""-dsf_dimer b0,b1,... (-m gpu): the engine's Chebyshev moments of the dynamical dimer correlations (DimerDynamics.json: the images
D_b psi of all bonds through DimerFrame, psi removed from all of them by one dmrgx_vec_project_out, one dmrgx_kron_chebyshev_moments run
per reference bond) against exact diagonalisation of the 6 x 2 Heisenberg lattice, against -corr_dimer of the same run, and under
truncation.  ED from helpers.lattice_ground_state as in test_gpu_dimer._exact_tables, restricted to the Sz = 0 sector (924 states);
-mwarmup 64 keeps every state, so the engine's last superblock is the lattice itself."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from oracle.hamiltonian import J1J2XXZModel_SquareLattice
from oracle.qn import OpSm, OpSp, OpSz
from helpers import lattice_ground_state
from test_gpu_engine import EXE, run_engine
from test_gpu_dsf import HEIS_6x2, Q_OPT, _no_nan
from test_gpu_dsf_cheb import jackson
from test_gpu_dimer import _bonds

pytestmark = pytest.mark.gpu
N, LX, LY, NB = 12, 6, 2, 16
U = 2.0 ** -53


def _records(d, name="DimerDynamics.json"):
    return json.load(open(str(d) + "/" + name))


@pytest.fixture(scope="module")
def dimer_ed():
    """Heisenberg 6 x 2 by dense ED, once: w, V of H in the Sz = 0 sector, psi, the dense images D_b psi of the 16 bonds, <D_b>, and the
    components of (D_b - <D_b>) psi (`dU`) and of D_b psi (`rawU`) along the eigenvectors."""
    ham = J1J2XXZModel_SquareLattice(Lx=LX, Ly=LY, heisenberg=1.0)
    E0, psi_full, site_op = lattice_ground_state(ham)
    sector = np.array([i for i in range(2 ** N) if bin(i).count("1") == N // 2])
    H = None
    for t in ham.H(N):
        h = t.a * (site_op(t.Iop, t.Isite) @ site_op(t.Jop, t.Jsite))
        H = h if H is None else H + h
    H = H.tocsr()[sector][:, sector].toarray()
    bonds, orient, pos = _bonds(ham)
    assert len(bonds) == NB
    img = np.array([site_op(OpSz, i) @ (site_op(OpSz, j) @ psi_full) + 0.5 * (site_op(OpSp, i) @ (site_op(OpSm, j) @ psi_full) + site_op(OpSm, i) @ (site_op(OpSp, j) @ psi_full))
                    for i, j in bonds])
    assert np.abs(np.delete(img, sector, axis=1)).max() <= 1e-12     # D_b conserves Sz (psi of the full eigh lies in the sector to rounding)
    img, psi = img[:, sector], psi_full[sector]
    assert abs(psi @ psi - 1.0) < 1e-12 and np.abs(H @ psi - E0 * psi).max() < 1e-10
    w, V = np.linalg.eigh(H)
    D = img @ psi
    out = {"E0": E0, "psi": psi, "w": w, "V": V, "D": D, "dU": (img - np.outer(D, psi)) @ V, "rawU": img @ V, "ham": ham,
           "bonds": bonds, "orient": orient, "pos": np.array(pos, dtype=float)}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _ed_moments(ed, centre, hw, c, nmom, key="dU"):
    """[b][n] = < u_b, T_n((H - centre) / hw) u_c >, n < nmom, u = the projected (dU) or the raw (rawU) images"""
    Tn = np.cos(np.arange(nmom)[:, None] * np.arccos((ed["w"] - centre) / hw)[None, :])
    return (ed[key] * ed[key][c][None, :]) @ Tn.T


def _cosines(pos, sel, c):
    """[q = nx Ly + ny][k] = cos(q . (r_sel[k] - r_c))"""
    out = np.zeros((LX * LY, len(sel)))
    for nx in range(LX):
        for ny in range(LY):
            out[nx * LY + ny] = np.cos(2 * np.pi * (nx * (pos[sel, 0] - pos[c, 0]) / LX + ny * (pos[sel, 1] - pos[c, 1]) / LY))
    return out


def _same(ed, c):
    return [b for b in range(NB) if ed["orient"][b] == ed["orient"][c]]


def _pick_four(bonds, orient, nl):
    """One y bond inside the left block, the first bond across the cut, one x bond inside the right block, one x bond inside the left one."""
    left = [b for b, (i, j) in enumerate(bonds) if j < nl]
    right = [b for b, (i, j) in enumerate(bonds) if i >= nl]
    across = [b for b, (i, j) in enumerate(bonds) if i < nl <= j]
    return [next(b for b in left if orient[b] == "y"), across[0], next(b for b in right if orient[b] == "x"), next(b for b in left if orient[b] == "x")]


def test_four_bonds_against_exact_diagonalisation(tmp_path, dimer_ed):
    """Four reference bonds -- both orientations; inside the left block, across the cut, inside the right block: asserted from the record's
    Bonds and the step's NSites --, 60 steps, nothing truncated, last record.  Moments against < dD_b psi, T_n(Ht) dD_c psi > of ED in the
    record's own window to 1e-10 (the tolerance of the -dsf_cheb ED test: the same recursion at the same length); Diag against ED to
    1e-10 for all n <= 120 and against Moments[c] to 1e-12 for n <= 60; Moments[:, 0] against Connected[:, c] of -corr_dimer in the same
    run to 1e-12 (15 digits of values O(0.1)); D / Norm against ED's <D_b> to 1e-10; MomentsQ the cosine sum of the rows of c's
    orientation to 1e-13; |Elastic| <= 64 u; StepsDone 60; MatMults 40 + 4 * 60; the window contains the ED spectrum."""
    ed = dimer_ed
    refs = _pick_four(ed["bonds"], ed["orient"], N // 2)
    K = 60
    rows, _, _ = run_engine(tmp_path, *HEIS_6x2, "-mwarmup", 64, "-dsf_dimer", ",".join(str(b) for b in refs), "-dsf_dimer_steps", K, "-corr_dimer", 1)
    rec, dim = _records(tmp_path)[-1], _records(tmp_path, "DimerCorrelations.json")[-1]
    assert rec["GlobIdx"] == dim["GlobIdx"]
    (step,) = [r for r in rows if r["GlobIdx"] == rec["GlobIdx"]]
    nl = step["NSites_SysEnl"]
    assert nl == step["NSites_Sys"] + 1 and nl + step["NSites_EnvEnl"] == N
    assert rec["Bonds"] == ed["bonds"] == dim["Bonds"] and rec["Orientation"] == ed["orient"] and rec["Position"] == ed["pos"].astype(int).tolist()
    sides = [0 if j < nl else (1 if i >= nl else 2) for i, j in (rec["Bonds"][b] for b in refs)]
    assert sorted(sides) == [0, 0, 1, 2] and {rec["Orientation"][b] for b in refs} == {"x", "y"}, (refs, sides, nl)
    assert _no_nan(rec) and rec["Steps"] == K and rec["BoundSteps"] == 40 and rec["MatMults"] == 40 + 4 * K and "Omega" not in rec
    assert abs(rec["Norm"] - 1.0) <= 1e-12 and abs(rec["E0"] - ed["E0"]) <= 1e-10 and rec["tDimerDyn"] > 0.0
    centre, hw = rec["Centre"], rec["HalfWidth"]
    print("window", centre - hw, centre + hw, "ED", ed["w"][0], ed["w"][-1], "ThetaMax", rec["ThetaMax"], "Residual", rec["Residual"])
    assert centre - hw < ed["w"][0] and centre + hw > ed["w"][-1]
    errD = np.abs(np.array(rec["D"]) / rec["Norm"] - ed["D"]).max()
    print("D", errD, "ED <D_b> from", ed["D"].min(), "to", ed["D"].max())
    assert errD <= 1e-10 and ed["D"].max() < -0.2
    conn = np.array(dim["Connected"])
    assert [s["Bond"] for s in rec["RefBonds"]] == refs
    for s in rec["RefBonds"]:
        c = s["Bond"]
        assert s["Sites"] == ed["bonds"][c] and s["Orientation"] == ed["orient"][c] and s["StepsDone"] == K and "SqwGrid" not in s
        mom, momq, diag = np.array(s["Moments"]), np.array(s["MomentsQ"]), np.array(s["Diag"])
        assert mom.shape == (NB, K + 1) and momq.shape == (LX * LY, K + 1) and diag.shape == (2 * K + 1,)
        sel = _same(ed, c)
        errs = {"ED": np.abs(mom - _ed_moments(ed, centre, hw, c, K + 1)).max(), "Diag ED": np.abs(diag - _ed_moments(ed, centre, hw, c, 2 * K + 1)[c]).max(),
                "Diag Moments": np.abs(diag[:K + 1] - mom[c]).max(), "Connected": np.abs(mom[:, 0] - conn[:, c]).max(),
                "MomentsQ": np.abs(momq - _cosines(ed["pos"], sel, c) @ mom[sel]).max(), "Elastic": abs(s["Elastic"]) / U,
                "Norm2": abs(diag[0] * rec["Norm"] - s["Norm2"])}
        print("bond", c, errs)
        assert errs["ED"] <= 1e-10
        assert errs["Diag ED"] <= 1e-10
        assert errs["Diag Moments"] <= 1e-12
        assert errs["Connected"] <= 1e-12
        assert errs["MomentsQ"] <= 1e-13
        assert errs["Elastic"] <= 64
        assert errs["Norm2"] <= 1e-15


@pytest.fixture(scope="module")
def runs_with_and_without(tmp_path_factory):
    """-corr_dimer 1 and -dsf 1 (40 steps): once alone, once with -dsf_dimer over all sixteen bonds, 60 steps, and a grid."""
    d = tmp_path_factory.mktemp("dsf_dimer")
    common = [*HEIS_6x2, "-mwarmup", 64, "-corr_dimer", 1, "-dsf", 1, "-dsf_q", Q_OPT, "-dsf_steps", 40]
    run_engine(d / "off", *common)
    run_engine(d / "on", *common, "-dsf_dimer", ",".join(str(b) for b in range(NB)), "-dsf_dimer_steps", 60, "-dsf_dimer_omega", "0,6,241")
    return d / "off", d / "on"


def _orientation_average(rec, ed, which):
    """(1 / N_a) sum over the reference bonds of orientation a of SqwGrid -> [q][k]"""
    sel = [s for s in rec["RefBonds"] if s["Orientation"] == which]
    return sum(np.array(s["SqwGrid"]) for s in sel) / len(sel)


def _ed_grid(ed, rec, which, key="dU", nmom=61):
    """The same average from ED moments in the record's window: jackson of (1 / N_a) sum_{b, c in a} cos(q . (r_b - r_c)) mu_n^{bc} -> [q][k]"""
    centre, hw = rec["Centre"], rec["HalfWidth"]
    sel = [b for b in range(NB) if ed["orient"][b] == which]
    momq = np.zeros((LX * LY, nmom))
    for c in sel:
        momq += _cosines(ed["pos"], sel, c) @ _ed_moments(ed, centre, hw, c, nmom, key)[sel] / len(sel)
    x = (np.array(rec["Omega"]) + rec["E0"] - centre) / hw
    return jackson(momq, x) / hw


def test_all_bonds_average_to_a_positive_broadened_dimer_structure_factor(runs_with_and_without, dimer_ed):
    """All sixteen bonds as references, grid 0,6,241.  Per orientation a: (1 / N_a) sum_{c in a} MomentsQ[q][0] = StructureFactorX / Y of
    -corr_dimer in the same run to 1e-10; SqwGrid = the numpy Jackson formula on the record's MomentsQ to 1e-12; the orientation average
    of SqwGrid is >= -1e-12 everywhere -- sum_bc cos(q . (r_b - r_c)) G_bc is the sum of two squared forms, a positive measure under a
    positive kernel -- and equals the Jackson sum of the ED moments in the same window to 1e-9."""
    _, on = runs_with_and_without
    ed = dimer_ed
    rec, dim = _records(on)[-1], _records(on, "DimerCorrelations.json")[-1]
    assert rec["GlobIdx"] == dim["GlobIdx"]
    assert _no_nan(rec) and rec["MatMults"] == 40 + NB * 60 and [s["Bond"] for s in rec["RefBonds"]] == list(range(NB))
    omega = np.array(rec["Omega"])
    assert omega.shape == (241,) and np.abs(omega - np.linspace(0.0, 6.0, 241)).max() <= 1e-14
    x = (omega + rec["E0"] - rec["Centre"]) / rec["HalfWidth"]
    for s in rec["RefBonds"]:
        assert s["StepsDone"] == 60
        grid = np.array(s["SqwGrid"])
        want = jackson(np.array(s["MomentsQ"]), x) / rec["HalfWidth"]
        assert grid.shape == (LX * LY, 241)
        assert np.abs(grid - want).max() <= 1e-12, (s["Bond"], np.abs(grid - want).max())
    for which in "xy":
        sel = [s for s in rec["RefBonds"] if s["Orientation"] == which]
        assert len(sel) == ed["orient"].count(which)
        static = sum(np.array(s["MomentsQ"])[:, 0] for s in sel) / len(sel)
        sf = np.array(dim["StructureFactor" + which.upper()]).reshape(LX * LY)
        avg = _orientation_average(rec, ed, which)
        want = _ed_grid(ed, rec, which)
        print(which, "static err", np.abs(static - sf).max(), "min of the average", avg.min(), "max", avg.max(), "ED err", np.abs(avg - want).max())
        assert np.abs(static - sf).max() <= 1e-10
        assert avg.min() >= -1e-12
        assert np.abs(avg - want).max() <= 1e-9


def test_the_elastic_line_is_gone(runs_with_and_without, dimer_ed):
    """The x-bond average of SqwGrid at q = 0 and w = 0 (grid point 0), 60 steps (61 moments): below 1e-3 of what the unprojected images
    D_b psi give at the same point -- computed here from ED moments in the record's window --, and equal to the projected ED value to 1e-9.
    From ED alone, in the window [E0 - 0.01 W, w_max + 0.02 W] the engine finds to 1e-6 W (W = w_max - E0): unprojected 2.6004, projected
    1.8087e-05 (the Jackson tail of the lowest singlet pole, 3.10 above E0), ratio 7.0e-06: no other grid point or step count was needed."""
    _, on = runs_with_and_without
    ed = dimer_ed
    rec = _records(on)[-1]
    got = _orientation_average(rec, ed, "x")[0][0]
    raw, projected = _ed_grid(ed, rec, "x", "rawU")[0][0], _ed_grid(ed, rec, "x")[0][0]
    print("q = 0, w = 0, x bonds: engine", got, "ED projected", projected, "ED unprojected", raw, "ratio", got / raw)
    assert rec["Omega"][0] == 0.0 and raw > 1.0
    assert got < 1e-3 * raw
    assert abs(got - projected) <= 1e-9


def test_option_off_changes_nothing(runs_with_and_without):
    """Without -dsf_dimer the file does not appear, and the other outputs of the run -- DimerCorrelations.json through the same DimerFrame
    among them -- are the same bytes once the timing fields tDsf and tDimer are blanked."""
    off, on = runs_with_and_without
    assert not os.path.exists(str(off) + "/DimerDynamics.json") and os.path.exists(str(on) + "/DimerDynamics.json")
    for name in ("Correlations.json", "DMRGSteps.json", "DynamicalStructureFactor.json", "DimerCorrelations.json"):
        a, b = (re.sub(rb'"(tDsf|tDimer)": [^,]*,', rb'"\1": 0,', open(str(d) + "/" + name, "rb").read()) for d in (off, on))
        assert a == b, name
        assert len(a) > 100


def test_truncated_run_static_sum_rule(tmp_path):
    """m = 24 cuts the basis: Moments[:, 0] of every record equals Connected[:, c] of the same run's DimerCorrelations.json (1e-12) -- the
    same truncated operators on the same state --, nothing is non-finite, and the window found from the truncated superblock Hamiltonian
    holds: StepsDone = Steps."""
    rows, _, _ = run_engine(tmp_path, *HEIS_6x2, "-mwarmup", 24, "-corr_dimer", 1, "-dsf_dimer", "0,7,15", "-dsf_dimer_steps", 40)
    assert any(r["NStates_SysRot"] < r["NStates_SysEnl"] for r in rows)
    recs, dims = _records(tmp_path), _records(tmp_path, "DimerCorrelations.json")
    assert len(recs) == len(dims) >= 1
    for rec, dim in zip(recs, dims):
        assert _no_nan(rec) and rec["GlobIdx"] == dim["GlobIdx"] and rec["Steps"] == 40
        conn = np.array(dim["Connected"])
        assert [s["Bond"] for s in rec["RefBonds"]] == [0, 7, 15]
        for s in rec["RefBonds"]:
            err = np.abs(np.array(s["Moments"])[:, 0] - conn[:, s["Bond"]]).max()
            print(rec["GlobIdx"], s["Bond"], "StepsDone", s["StepsDone"], "Moments[:, 0] err", err, "Elastic", s["Elastic"] / U, "u")
            assert err <= 1e-12
            assert s["StepsDone"] == 40


def test_given_window_runs_no_bound_run(tmp_path, dimer_ed):
    """-dsf_cheb_window -11,6, which -dsf_dimer shares: Centre = -2.5 and HalfWidth = 8.5 exactly, no Lanczos run for the bound (BoundSteps
    0, MatMults = refs * K), and the moments against ED in that window to 1e-10."""
    ed = dimer_ed
    run_engine(tmp_path, *HEIS_6x2, "-mwarmup", 64, "-dsf_dimer", "3,8", "-dsf_dimer_steps", 30, "-dsf_cheb_window", "-11,6")
    rec = _records(tmp_path)[-1]
    assert _no_nan(rec) and rec["Centre"] == -2.5 and rec["HalfWidth"] == 8.5 and rec["BoundSteps"] == 0 and rec["MatMults"] == 2 * 30 and "Omega" not in rec
    assert -11.0 < ed["w"][0] and ed["w"][-1] < 6.0
    assert not os.path.exists(str(tmp_path) + "/ChebyshevMoments.json")
    assert [s["Bond"] for s in rec["RefBonds"]] == [3, 8]
    for s in rec["RefBonds"]:
        err = np.abs(np.array(s["Moments"]) - _ed_moments(ed, -2.5, 8.5, s["Bond"], 31)).max()
        print("given window: bond", s["Bond"], "StepsDone", s["StepsDone"], "err", err)
        assert s["StepsDone"] == 30 and "SqwGrid" not in s
        assert err <= 1e-10


def test_two_ranks_are_refused_at_start_up(tmp_path):
    d = str(tmp_path) + "/"
    cmd = [EXE, *[str(o) for o in HEIS_6x2], "-mwarmup", "8", "-dsf_dimer", "6", "-data_dir", d]
    name = "dmrgx_test_dsfd_%d" % os.getpid()
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
        assert "-dsf_dimer is not available on more than one rank" in o, o[-2000:]
    assert not os.path.exists(d + "DimerDynamics.json")


def test_bond_outside_the_list_is_refused_at_start_up(tmp_path):
    out = subprocess.run([EXE, *[str(o) for o in HEIS_6x2], "-mwarmup", "8", "-dsf_dimer", "3,16", "-data_dir", str(tmp_path) + "/"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "-dsf_dimer: bond 16 is outside [0, 16)" in out.stderr
    assert not os.listdir(str(tmp_path))
