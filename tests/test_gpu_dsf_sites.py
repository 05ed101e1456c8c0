"""-dsf_sites c0,c1,... (-m gpu): the engine's real-space dynamical correlations G_ic(w) (DynamicalCorrelations.json: one
dmrgx_kron_lanczos_basis run per reference site, the overlaps of all site images with the kept basis through dmrgx_vec_gram) against
exact diagonalisation of the 6 x 2 Heisenberg lattice, against -dsf and -corr_matrix of the same run, and under truncation.

ED as in test_gpu_dsf.py: the Sz = 0 sector (924 states), Sz_i diagonal in the site basis.  -mwarmup 64 keeps every state of a 6 x 2
lattice, so the engine's superblock is the lattice itself."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from oracle.hamiltonian import J1J2XXZModel_SquareLattice
from oracle.qn import OpSz
from helpers import lattice_ground_state
from test_gpu_engine import EXE, run_engine
from test_gpu_dsf import HEIS_6x2, Q, Q_OPT, _no_nan

pytestmark = pytest.mark.gpu
N = 12


def _records(d, name="DynamicalCorrelations.json"):
    return json.load(open(str(d) + "/" + name))


@pytest.fixture(scope="module")
def heis_ed():
    """Heisenberg 6 x 2 by dense ED, once: H in the Sz = 0 sector, psi, the diagonals of Sz_i."""
    ham = J1J2XXZModel_SquareLattice(Lx=6, Ly=2, heisenberg=1.0)
    E0, psi, site_op = lattice_ground_state(ham)
    sector = np.array([i for i in range(2 ** N) if bin(i).count("1") == N // 2])
    H = None
    for t in ham.H(N):
        h = t.a * (site_op(t.Iop, t.Isite) @ site_op(t.Jop, t.Jsite))
        H = h if H is None else H + h
    H = H.tocsr()[sector][:, sector].toarray()
    psi = psi[sector]
    assert abs(psi @ psi - 1.0) < 1e-12 and np.abs(H @ psi - E0 * psi).max() < 1e-10
    w, V = np.linalg.eigh(H)
    szd = np.array([site_op(OpSz, i).diagonal()[sector] for i in range(N)])
    out = {"E0": E0, "H": H, "psi": psi, "szd": szd, "w": w, "V": V, "ham": ham}
    for a in (H, psi, szd, w, V):
        a.setflags(write=False)
    return out


def test_two_sites_against_exact_diagonalisation(tmp_path, heis_ed):
    """-dsf_sites 6,0, 100 steps, nothing truncated, last record, both sites: Static against ED (1e-10) and against SzSz of the same run
    (1e-12); the moments sum_n Amplitudes[i][n] Poles[n]^p against <u_i, (H - E0)^p v> of ED to 1e-10 W^p, p = 1..5; Amplitudes[c] are
    the continued-fraction weights Norm2 S[0][n]^2 >= 0; the lowest pole with weight is ED's 1.4170703...; Norm2 = 1/4; 200 MatMults."""
    run_engine(tmp_path, *HEIS_6x2, "-mwarmup", 64, "-dsf_sites", "6,0", "-dsf_steps", 100, "-corr_matrix", 1)
    rec = _records(tmp_path)[-1]
    spin = _records(tmp_path, "SpinCorrelations.json")[-1]
    assert rec["GlobIdx"] == spin["GlobIdx"]
    assert _no_nan(rec) and rec["Steps"] == 100 and rec["MatMults"] == 200 and abs(rec["Norm"] - 1.0) <= 1e-12 and abs(rec["E0"] - heis_ed["E0"]) <= 1e-10
    assert [s["Site"] for s in rec["Sites"]] == [6, 0]
    H, psi, szd, w, E0 = heis_ed["H"], heis_ed["psi"], heis_ed["szd"], heis_ed["w"], heis_ed["E0"]
    W = w[-1] - E0
    A = H - E0 * np.eye(len(w))
    szsz = np.array(spin["SzSz"])
    for s in rec["Sites"]:
        c = s["Site"]
        assert s["r"] == list(heis_ed["ham"].To2D(c))
        poles, amp, static = np.array(s["Poles"]), np.array(s["Amplitudes"]), np.array(s["Static"])
        alpha, beta = np.array(s["Alpha"]), np.array(s["Beta"])
        assert s["StepsDone"] == 100 and amp.shape == (N, 100) and len(poles) == len(alpha) == len(beta) == 100 and np.array(s["Sqw"]).shape == (N, 100)
        assert abs(s["Norm2"] - 0.25) <= 1e-10
        v = szd[c] * psi
        U = szd * psi[None, :]
        ed_static = U @ v
        print("site", c, "Static err ED", np.abs(static - ed_static).max(), "err SzSz", np.abs(static - szsz[:, c] / spin["Norm"]).max())
        assert np.abs(static - ed_static).max() <= 1e-10
        assert np.abs(static - szsz[:, c] / spin["Norm"]).max() <= 1e-12
        assert np.abs(static - amp.sum(axis=1)).max() <= 1e-14
        x = v.copy()
        for p in range(1, 6):
            x = A @ x
            err = np.abs(amp @ poles ** p - U @ x).max()
            print("   moment", p, "err", err, "bound", 1e-10 * W ** p)
            assert err <= 1e-10 * W ** p
        th, z = np.linalg.eigh(np.diag(alpha) + np.diag(beta[:-1], 1) + np.diag(beta[:-1], -1))
        assert (np.diff(poles) >= 0).all() and np.abs(poles - (th - rec["E0"])).max() <= 1e-10
        print("   min Amplitudes[c]", amp[c].min(), "err against Norm2 S[0]^2", np.abs(amp[c] - s["Norm2"] * z[0] ** 2).max())
        assert amp[c].min() >= -1e-14
        assert np.abs(amp[c] - s["Norm2"] * z[0] ** 2).max() <= 1e-12
        amp2 = (heis_ed["V"].T @ v) ** 2
        ed_low = w[np.nonzero(amp2 > 1e-9 * amp2.sum())[0]]
        ed_low = ed_low[ed_low - E0 > 1e-6][0] - E0                        # (<Sz_c> = 0: no weight at w = 0)
        low = poles[amp[c] > 1e-9 * s["Norm2"]][0]
        print("   lowest pole", low, "ED", ed_low)
        assert abs(ed_low - 1.4170703) <= 1e-6 and abs(low - ed_low) <= 1e-8


@pytest.fixture(scope="module")
def runs_with_and_without(tmp_path_factory):
    """-dsf 1 at the four q of test_gpu_dsf.py, 40 steps: once alone, once with -dsf_sites over all twelve sites."""
    d = tmp_path_factory.mktemp("dsf_sites")
    common = [*HEIS_6x2, "-mwarmup", 64, "-dsf", 1, "-dsf_q", Q_OPT, "-dsf_steps", 40]
    run_engine(d / "off", *common)
    run_engine(d / "on", *common, "-dsf_sites", ",".join(str(c) for c in range(N)))
    return d / "off", d / "on"


def test_all_sites_average_to_the_structure_factor_of_dsf(runs_with_and_without):
    """For each q of -dsf: (1/12) sum_c sum_n Sqw_c[q][n] equals its StaticSzz and (1/12) sum_c sum_n Sqw_c[q][n] Poles_c[n] its
    sum Weights * Poles, to 1e-10: identities for any number of steps >= 2."""
    _, on = runs_with_and_without
    rec, dsf = _records(on)[-1], _records(on, "DynamicalStructureFactor.json")[-1]
    assert _no_nan(rec) and rec["MatMults"] == 12 * 40 and sorted(s["Site"] for s in rec["Sites"]) == list(range(N))
    Ly = 2
    for p in dsf["Points"]:
        nx, ny = p["q"]
        m0 = sum(np.array(s["Sqw"])[nx * Ly + ny].sum() for s in rec["Sites"]) / N
        m1 = sum(np.array(s["Sqw"])[nx * Ly + ny] @ np.array(s["Poles"]) for s in rec["Sites"]) / N
        want1 = float(np.array(p["Weights"]) @ np.array(p["Poles"])) if p["Poles"] else 0.0
        print(p["q"], "static", m0, p["StaticSzz"], "first moment", m1, want1)
        assert abs(m0 - p["StaticSzz"]) <= 1e-10
        assert abs(m1 - want1) <= 1e-10
    assert [tuple(p["q"]) for p in dsf["Points"]] == Q


def test_option_off_changes_nothing(runs_with_and_without):
    """Without -dsf_sites the file does not appear, and the other outputs of the run are the same bytes (timing fields blanked)."""
    off, on = runs_with_and_without
    assert not os.path.exists(str(off) + "/DynamicalCorrelations.json") and os.path.exists(str(on) + "/DynamicalCorrelations.json")
    for name in ("Correlations.json", "DMRGSteps.json", "DynamicalStructureFactor.json"):
        a, b = (re.sub(rb'"tDsf": [^,]*,', b'"tDsf": 0,', open(str(d) + "/" + name, "rb").read()) for d in (off, on))
        assert a == b, name


def test_truncated_run_static_sum_rule(tmp_path):
    """m = 24 cuts the basis: Static of every record equals SzSz[:, c] / Norm of the same run's SpinCorrelations.json (1e-12) -- the
    same truncated operators on the same state --, and nothing is non-finite."""
    rows, _, _ = run_engine(tmp_path, *HEIS_6x2, "-mwarmup", 24, "-corr_matrix", 1, "-dsf_sites", "6,0", "-dsf_steps", 40)
    assert any(r["NStates_SysRot"] < r["NStates_SysEnl"] for r in rows)
    recs, spin = _records(tmp_path), _records(tmp_path, "SpinCorrelations.json")
    assert len(recs) == len(spin) >= 1
    for rec, srec in zip(recs, spin):
        assert _no_nan(rec) and rec["GlobIdx"] == srec["GlobIdx"]
        szsz = np.array(srec["SzSz"])
        for s in rec["Sites"]:
            err = np.abs(np.array(s["Static"]) - szsz[:, s["Site"]] / srec["Norm"]).max()
            print(rec["GlobIdx"], s["Site"], "StepsDone", s["StepsDone"], "Static err", err)
            assert err <= 1e-12


def test_two_ranks_are_refused_at_start_up(tmp_path):
    d = str(tmp_path) + "/"
    cmd = [EXE, *[str(o) for o in HEIS_6x2], "-mwarmup", "8", "-dsf_sites", "6", "-data_dir", d]
    name = "dmrgx_test_dsfs_%d" % os.getpid()
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
        assert "-dsf_sites is not available on more than one rank" in o, o[-2000:]
    assert not os.path.exists(d + "DynamicalCorrelations.json")


def test_site_outside_the_lattice_is_refused_at_start_up(tmp_path):
    out = subprocess.run([EXE, *[str(o) for o in HEIS_6x2], "-mwarmup", "8", "-dsf_sites", "3,12", "-data_dir", str(tmp_path) + "/"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "-dsf_sites: site 12 is outside [0, 12)" in out.stderr
    assert not os.path.exists(str(tmp_path) + "/DynamicalCorrelations.json")
