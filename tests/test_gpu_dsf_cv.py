"""-dsf_cv c0,c1,... (-m gpu): the engine's correction vectors of the real-space dynamical correlations (CorrectionVectors.json: one
dmrgx_kron_correction_vector solve per reference site and frequency, the images of all sites held on the device) against exact
diagonalisation of the 6 x 2 Heisenberg lattice, and under truncation.  ED as in test_gpu_dsf_sites.py: the Sz = 0 sector (924 states);
-mwarmup 64 keeps every state, so the engine's last superblock is the lattice itself.

With u_i = Sz_i psi, v = Sz_c psi (|u| = |v| = 1/2), sigma = E0 + w and the eigenpairs (E_n, |n>) of ED:
    Aw[i][k]  = -ImG / pi = (1 / pi) sum_n <u_i|n><n|v> eta / ((sigma_k - E_n)^2 + eta^2),
    ReG[i][k] =                      sum_n <u_i|n><n|v> (sigma_k - E_n) / ((sigma_k - E_n)^2 + eta^2).
Bounds from lambda_min((H - sigma)^2 + eta^2) >= eta^2 with the record's own Residual[k] = |b - A Y| / |b| (test_gpu_corrvec.py):
|ImG - exact| <= |u| |v| Residual / eta + 1e-10 |u| |v| / eta, half of that for ReG, and 1 / pi of it for Aw."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_engine import EXE, run_engine
from test_gpu_dsf import HEIS_6x2, Q_OPT, _no_nan
from test_gpu_dsf_sites import heis_ed      # noqa: F401  (a module-scoped fixture)

pytestmark = pytest.mark.gpu
N, LX, LY = 12, 6, 2


def _records(d, name="CorrectionVectors.json"):
    return json.load(open(str(d) + "/" + name))


def _cosines(ham, c):
    """[q = nx Ly + ny][i] = cos(q . (r_i - r_c))"""
    r = np.array([ham.To2D(i) for i in range(N)], dtype=float)
    out = np.zeros((LX * LY, N))
    for nx in range(LX):
        for ny in range(LY):
            out[nx * LY + ny] = np.cos(2 * np.pi * (nx * (r[:, 0] - r[c, 0]) / LX + ny * (r[:, 1] - r[c, 1]) / LY))
    return out


def _matmults(rec):
    """sum of n_matvec = 2 blocks 8 + 2 over the solves of a record, from its Iterations"""
    return sum(2 * 8 * max(1, -(-int(it) // 8)) + 2 for s in rec["Sites"] for it in s["Iterations"])


def _im_bound(residual, eta):
    return 0.25 * np.asarray(residual) / eta + 1e-10 * 0.25 / eta


def test_two_sites_against_exact_diagonalisation(tmp_path, heis_ed):
    """-dsf_cv 6,0 at w = 0, 0.5, .., 4, eta = 0.1, nothing truncated, last record: every solve converges (the numpy restatement needs
    57 - 256 iterations at tol 1e-8); Aw and ReG against the Lorentzian sums over ED's eigenpairs within the bounds of the module
    docstring; SqwGrid is the cosine sum of Aw to 1e-13; Aw[c][k] > 0; Norm2 = 1/4; MatMults = sum of n_matvec."""
    run_engine(tmp_path, *HEIS_6x2, "-mwarmup", 64, "-dsf_cv", "6,0", "-dsf_cv_omega", "0,4,9", "-dsf_cv_eta", 0.1, "-corr_matrix", 1)
    rec, spin = _records(tmp_path)[-1], _records(tmp_path, "SpinCorrelations.json")[-1]
    assert rec["GlobIdx"] == spin["GlobIdx"]
    psi, szd, w, V, E0 = heis_ed["psi"], heis_ed["szd"], heis_ed["w"], heis_ed["V"], heis_ed["E0"]
    eta, nw = 0.1, 9
    assert _no_nan(rec) and rec["Eta"] == eta and rec["Tol"] == 1e-8 and rec["MaxIt"] == 2000
    assert abs(rec["Norm"] - 1.0) <= 1e-12 and abs(rec["E0"] - E0) <= 1e-10
    omega = np.array(rec["Omega"])
    assert omega.shape == (nw,) and np.abs(omega - np.linspace(0.0, 4.0, nw)).max() <= 1e-14
    assert [s["Site"] for s in rec["Sites"]] == [6, 0]
    assert rec["MatMults"] == _matmults(rec)
    Uc = (szd * psi[None, :]) @ V                                          # [i][n]
    x = (omega + E0)[None, :] - w[:, None]                                 # [n][k] = sigma_k - E_n
    lor, disp = eta / (x * x + eta * eta), x / (x * x + eta * eta)
    for s in rec["Sites"]:
        c = s["Site"]
        assert s["r"] == list(heis_ed["ham"].To2D(c)) and abs(s["Norm2"] - 0.25) <= 1e-10
        it, conv, res = np.array(s["Iterations"]), np.array(s["Converged"]), np.array(s["Residual"])
        im, rg, aw, grid = np.array(s["ImG"]), np.array(s["ReG"]), np.array(s["Aw"]), np.array(s["SqwGrid"])
        assert it.shape == conv.shape == res.shape == (nw,) and im.shape == rg.shape == aw.shape == (N, nw) and grid.shape == (LX * LY, nw)
        print("site", c, "iterations", it, "residual max", res.max())
        assert (conv == 1).all() and (it >= 1).all() and (it <= 2000).all() and (res <= 2e-8).all()
        ed_aw = (Uc * Uc[c][None, :]) @ lor / np.pi
        ed_re = (Uc * Uc[c][None, :]) @ disp
        bound = _im_bound(res, eta)[None, :]
        errs = {"Aw": (np.abs(aw - ed_aw) / (bound / np.pi)).max(), "ReG": (np.abs(rg - ed_re) / (0.5 * bound)).max(),
                "Aw from ImG": np.abs(aw + im / np.pi).max(), "SqwGrid": np.abs(grid - _cosines(heis_ed["ham"], c) @ aw).max()}
        print("site", c, "errors (Aw, ReG: in units of the bound)", errs)
        assert errs["Aw"] <= 1.0
        assert errs["ReG"] <= 1.0
        assert errs["Aw from ImG"] <= 1e-15
        assert errs["SqwGrid"] <= 1e-13
        assert (aw[c] > 0.0).all()


@pytest.fixture(scope="module")
def runs_with_and_without(tmp_path_factory):
    """-dsf 1 at the four q of test_gpu_dsf.py, 40 steps: once alone, once with -dsf_cv over all twelve sites at five frequencies."""
    d = tmp_path_factory.mktemp("dsf_cv")
    common = [*HEIS_6x2, "-mwarmup", 64, "-dsf", 1, "-dsf_q", Q_OPT, "-dsf_steps", 40]
    run_engine(d / "off", *common)
    run_engine(d / "on", *common, "-dsf_cv", ",".join(str(c) for c in range(N)), "-dsf_cv_omega", "0,4,5", "-dsf_cv_eta", 0.2)
    return d / "off", d / "on"


def test_all_sites_average_to_the_lorentzian_structure_factor(runs_with_and_without, heis_ed):
    """Over all twelve reference sites, eta = 0.2, w = 0, 1, .., 4: (1/12) sum_c SqwGrid[q][k] against
    sum_n |<n| O_q |0>|^2 L_eta(w_k - w_n) of ED, O_q = N^-1/2 sum_i e^(i q . r_i) Sz_i: every Aw[i][k] is within its bound, the average
    over c of a sum over twelve i with |cos| <= 1 within twelve times the bound at the largest Residual; it is >= -1e-9 everywhere;
    the row q = 0 is <= 1e-6 in magnitude, for every site and so for the average, because Sz_tot psi = 0."""
    _, on = runs_with_and_without
    rec = _records(on)[-1]
    psi, szd, w, V, E0, ham = heis_ed["psi"], heis_ed["szd"], heis_ed["w"], heis_ed["V"], heis_ed["E0"], heis_ed["ham"]
    eta, nw = 0.2, 5
    assert _no_nan(rec) and rec["Eta"] == eta and sorted(s["Site"] for s in rec["Sites"]) == list(range(N)) and rec["MatMults"] == _matmults(rec)
    omega = np.array(rec["Omega"])
    assert np.abs(omega - np.linspace(0.0, 4.0, nw)).max() <= 1e-14
    avg, worst = np.zeros((LX * LY, nw)), 0.0
    for s in rec["Sites"]:
        assert (np.array(s["Converged"]) == 1).all()
        grid = np.array(s["SqwGrid"])
        assert grid.shape == (LX * LY, nw) and np.abs(grid[0]).max() <= 1e-6, (s["Site"], np.abs(grid[0]).max())
        avg += grid / N
        worst = max(worst, max(s["Residual"]))
    Uc = (szd * psi[None, :]) @ V                                          # [i][n]
    r = np.array([ham.To2D(i) for i in range(N)], dtype=float)
    x = (omega + E0)[None, :] - w[:, None]
    lor = eta / (x * x + eta * eta) / np.pi                                # [n][k]
    ed = np.zeros((LX * LY, nw))
    for nx in range(LX):
        for ny in range(LY):
            ph = np.exp(2j * np.pi * (nx * r[:, 0] / LX + ny * r[:, 1] / LY)) / np.sqrt(N)
            ed[nx * LY + ny] = (np.abs(ph @ Uc) ** 2) @ lor
    bound = N * _im_bound(worst, eta) / np.pi
    print("largest Residual", worst, "max |avg - ED|", np.abs(avg - ed).max(), "bound", bound, "min", avg.min(), "max |q = 0 row|", np.abs(avg[0]).max())
    assert np.abs(avg - ed).max() <= bound
    assert avg.min() >= -1e-9
    assert np.abs(avg[0]).max() <= 1e-6


def test_option_off_changes_nothing(runs_with_and_without):
    """Without -dsf_cv the file does not appear, and DMRGSteps.json and the -dsf record of the run are the same bytes (timing field blanked)."""
    off, on = runs_with_and_without
    assert not os.path.exists(str(off) + "/CorrectionVectors.json") and os.path.exists(str(on) + "/CorrectionVectors.json")
    for name in ("Correlations.json", "DMRGSteps.json", "DynamicalStructureFactor.json"):
        a, b = (re.sub(rb'"tDsf": [^,]*,', b'"tDsf": 0,', open(str(d) + "/" + name, "rb").read()) for d in (off, on))
        assert a == b, name


def test_truncated_run(tmp_path):
    """m = 24 cuts the basis.  In every record: nothing non-finite; every frequency converges within MaxIt with Residual <= 2 Tol;
    Aw[c][k] > 0 (a positive sum whatever the basis); the q = 0 row of SqwGrid <= 1e-6 in magnitude -- Sz_tot psi = 0 is exact in any
    Sz-preserving basis."""
    rows, _, _ = run_engine(tmp_path, *HEIS_6x2, "-mwarmup", 24, "-dsf_cv", "6,0", "-dsf_cv_omega", "0,4,5", "-dsf_cv_eta", 0.2)
    assert any(r["NStates_SysRot"] < r["NStates_SysEnl"] for r in rows)
    recs = _records(tmp_path)
    assert len(recs) >= 1
    for rec in recs:
        assert _no_nan(rec) and rec["MatMults"] == _matmults(rec)
        for s in rec["Sites"]:
            it, res, aw, grid = np.array(s["Iterations"]), np.array(s["Residual"]), np.array(s["Aw"]), np.array(s["SqwGrid"])
            print(rec["GlobIdx"], s["Site"], "iterations", it, "residual max", res.max(), "max |q = 0 row|", np.abs(grid[0]).max())
            assert (np.array(s["Converged"]) == 1).all() and (it <= rec["MaxIt"]).all()
            assert (res <= 2.0 * rec["Tol"]).all()
            assert (aw[s["Site"]] > 0.0).all()
            assert np.abs(grid[0]).max() <= 1e-6


def test_two_ranks_are_refused_at_start_up(tmp_path):
    d = str(tmp_path) + "/"
    cmd = [EXE, *[str(o) for o in HEIS_6x2], "-mwarmup", "8", "-dsf_cv", "6", "-dsf_cv_omega", "0,4,5", "-data_dir", d]
    name = "dmrgx_test_dsfv_%d" % os.getpid()
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
        assert "-dsf_cv is not available on more than one rank" in o, o[-2000:]
    assert not os.path.exists(d + "CorrectionVectors.json")


@pytest.mark.parametrize("opts,message", [
    (["-dsf_cv", "3,12", "-dsf_cv_omega", "0,4,5"], "-dsf_cv: site 12 is outside [0, 12)"),
    (["-dsf_cv", "3"], "-dsf_cv needs -dsf_cv_omega w0,w1,nw"),
    (["-dsf_cv", "3", "-dsf_cv_omega", "0,4"], "-dsf_cv_omega needs w0,w1,nw"),
    (["-dsf_cv", "3", "-dsf_cv_omega", "0,4,5", "-dsf_cv_eta", "0"], "-dsf_cv_eta must be positive"),
    (["-dsf_cv", "3", "-dsf_cv_omega", "0,4,5", "-dsf_cv_eta", "-0.1"], "-dsf_cv_eta must be positive"),
    (["-dsf_cv", "3", "-dsf_cv_omega", "0,4,5", "-dsf_cv_maxit", "0"], "-dsf_cv_maxit must be at least 1"),
], ids=["site", "no omega", "short omega", "eta 0", "eta negative", "maxit 0"])
def test_bad_options_are_refused_at_start_up(tmp_path, opts, message):
    out = subprocess.run([EXE, *[str(o) for o in HEIS_6x2], "-mwarmup", "8", *opts, "-data_dir", str(tmp_path) + "/"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and message in out.stderr, out.stderr[-2000:]
    assert not os.path.exists(str(tmp_path) + "/CorrectionVectors.json")
