"""-dsf_cheb c0,c1,... (-m gpu): the engine's Chebyshev moments of the real-space dynamical correlations (ChebyshevMoments.json: one
dmrgx_kron_chebyshev_moments run per reference site, the images of all sites held on the device, the window from a short Lanczos run)
against exact diagonalisation of the 6 x 2 Heisenberg lattice, against -corr_matrix, -dsf and -dsf_sites of the same run, and under
truncation.  ED as in test_gpu_dsf_sites.py: the Sz = 0 sector (924 states); -mwarmup 64 keeps every state, so the engine's last
superblock is the lattice itself."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_engine import EXE, run_engine
from test_gpu_dsf import HEIS_6x2, Q, Q_OPT, _no_nan
from test_gpu_dsf_sites import heis_ed      # noqa: F401  (a module-scoped fixture)

pytestmark = pytest.mark.gpu
N, LX, LY = 12, 6, 2


def _records(d, name="ChebyshevMoments.json"):
    return json.load(open(str(d) + "/" + name))


def _cosines(ham, c):
    """[q = nx Ly + ny][i] = cos(q . (r_i - r_c))"""
    r = np.array([ham.To2D(i) for i in range(N)], dtype=float)
    out = np.zeros((LX * LY, N))
    for nx in range(LX):
        for ny in range(LY):
            out[nx * LY + ny] = np.cos(2 * np.pi * (nx * (r[:, 0] - r[c, 0]) / LX + ny * (r[:, 1] - r[c, 1]) / LY))
    return out


def jackson(mu, x):
    """The Jackson-damped sum of the moments mu[..., M] at the points x[nw] -> [..., nw]; 0 at |x| >= 1."""
    mu, x = np.asarray(mu, dtype=float), np.asarray(x, dtype=float)
    M = mu.shape[-1]
    n = np.arange(M)
    g = ((M - n + 1) * np.cos(np.pi * n / (M + 1)) + np.sin(np.pi * n / (M + 1)) / np.tan(np.pi / (M + 1))) / (M + 1)
    inside = np.abs(x) < 1.0
    xi = np.where(inside, x, 0.0)
    Tn = np.cos(n[:, None] * np.arccos(xi)[None, :])                  # [n][w]
    s = (mu * (g * np.where(n == 0, 1.0, 2.0))) @ Tn
    return np.where(inside, s / (np.pi * np.sqrt(1.0 - xi * xi)), 0.0)


def test_two_sites_against_exact_diagonalisation(tmp_path, heis_ed):
    """-dsf_cheb 6,0, 60 steps, nothing truncated, last record.  The window found from 40 Lanczos steps contains the ED spectrum (forty
    random-start steps reach w_max to 1e-6 of the width on this lattice: checked on the CPU over five seeds); StepsDone = 60 and
    MatMults = 40 + 2 * 60; Moments against < u_i, T_n(Ht) v > of ED with the record's own Centre and HalfWidth to 1e-10; Moments[:, 0]
    against SzSz[:, c] / Norm of the same run to 1e-12; Moments[i][1] against the first moment of the -dsf_sites record of the same run,
    sum_n Amplitudes[i][n] (Poles[n] + E0 - Centre) / HalfWidth, to 1e-10; MomentsQ is the cosine sum of Moments to 1e-13; Diag[n] =
    Moments[c][n] to 1e-12 for n <= 60 (the doubling path against the Gram path), Diag against ED to 1e-10 for all n <= 120, and
    Diag[0] Norm = Norm2."""
    run_engine(tmp_path, *HEIS_6x2, "-mwarmup", 64, "-dsf_cheb", "6,0", "-dsf_cheb_steps", 60, "-corr_matrix", 1, "-dsf_sites", "6,0", "-dsf_steps", 100)
    rec, spin, dyn = _records(tmp_path)[-1], _records(tmp_path, "SpinCorrelations.json")[-1], _records(tmp_path, "DynamicalCorrelations.json")[-1]
    assert rec["GlobIdx"] == spin["GlobIdx"] == dyn["GlobIdx"]
    psi, szd, w, V, E0 = heis_ed["psi"], heis_ed["szd"], heis_ed["w"], heis_ed["V"], heis_ed["E0"]
    K = 60
    assert _no_nan(rec) and rec["Steps"] == K and rec["BoundSteps"] == 40 and rec["MatMults"] == 40 + 2 * K
    assert abs(rec["Norm"] - 1.0) <= 1e-12 and abs(rec["E0"] - E0) <= 1e-10
    centre, hw = rec["Centre"], rec["HalfWidth"]
    print("window", centre - hw, centre + hw, "ED", w[0], w[-1], "ThetaMax", rec["ThetaMax"], "Residual", rec["Residual"])
    assert centre - hw < w[0] and centre + hw > w[-1]
    assert rec["ThetaMax"] <= w[-1] + 1e-10 and rec["Residual"] >= 0.0
    assert [s["Site"] for s in rec["Sites"]] == [6, 0] and [s["Site"] for s in dyn["Sites"]] == [6, 0]
    x = (w - centre) / hw
    Tn = np.cos(np.arange(2 * K + 1)[:, None] * np.arccos(x)[None, :])      # [n][k]
    Uc = (szd * psi[None, :]) @ V                                          # [i][k]
    szsz = np.array(spin["SzSz"])
    for s, sd in zip(rec["Sites"], dyn["Sites"]):
        c = s["Site"]
        assert s["r"] == list(heis_ed["ham"].To2D(c)) and s["StepsDone"] == K
        mom, momq, diag = np.array(s["Moments"]), np.array(s["MomentsQ"]), np.array(s["Diag"])
        assert mom.shape == (N, K + 1) and momq.shape == (LX * LY, K + 1) and diag.shape == (2 * K + 1,)
        vc = Uc[c]
        ed = (Uc * vc[None, :]) @ Tn[:K + 1].T                              # [i][n]
        ed_diag = Tn @ (vc * vc)
        amp, poles = np.array(sd["Amplitudes"]), np.array(sd["Poles"])
        first = amp @ ((poles + rec["E0"] - centre) / hw)
        errs = {"ED": np.abs(mom - ed).max(), "SzSz": np.abs(mom[:, 0] - szsz[:, c] / spin["Norm"]).max(), "first moment": np.abs(mom[:, 1] - first).max(),
                "MomentsQ": np.abs(momq - _cosines(heis_ed["ham"], c) @ mom).max(), "Diag Moments": np.abs(diag[:K + 1] - mom[c]).max(),
                "Diag ED": np.abs(diag - ed_diag).max(), "Norm2": abs(diag[0] * rec["Norm"] - s["Norm2"])}
        print("site", c, errs)
        assert errs["ED"] <= 1e-10
        assert errs["SzSz"] <= 1e-12
        assert errs["first moment"] <= 1e-10
        assert errs["MomentsQ"] <= 1e-13
        assert errs["Diag Moments"] <= 1e-12
        assert errs["Diag ED"] <= 1e-10
        assert errs["Norm2"] <= 1e-15 and abs(s["Norm2"] - 0.25) <= 1e-10


@pytest.fixture(scope="module")
def runs_with_and_without(tmp_path_factory):
    """-dsf 1 at the four q of test_gpu_dsf.py, 40 steps: once alone, once with -dsf_cheb over all twelve sites, 60 steps, and a grid."""
    d = tmp_path_factory.mktemp("dsf_cheb")
    common = [*HEIS_6x2, "-mwarmup", 64, "-dsf", 1, "-dsf_q", Q_OPT, "-dsf_steps", 40]
    run_engine(d / "off", *common)
    run_engine(d / "on", *common, "-dsf_cheb", ",".join(str(c) for c in range(N)), "-dsf_cheb_steps", 60, "-dsf_cheb_omega", "0,6,241")
    return d / "off", d / "on"


def test_all_sites_average_to_a_positive_broadened_structure_factor(runs_with_and_without):
    """Over all twelve reference sites: (1/12) sum_c MomentsQ[q][0] = StaticSzz of -dsf to 1e-10; (1/12) sum_c SqwGrid[q] >= -1e-12
    everywhere -- in exact arithmetic a positive measure under a positive kernel, the CPU restatement gives -9e-17 --; its maximum at
    q = (pi, pi) lies within one grid step (0.025) of w = 1.40 (ED's lowest pole is 1.4170703, the restatement peaks at 1.40 with height
    1.27); SqwGrid equals the numpy Jackson formula applied to the record's MomentsQ to 1e-12."""
    _, on = runs_with_and_without
    rec, dsf = _records(on)[-1], _records(on, "DynamicalStructureFactor.json")[-1]
    assert _no_nan(rec) and rec["MatMults"] == 40 + 12 * 60 and sorted(s["Site"] for s in rec["Sites"]) == list(range(N))
    omega = np.array(rec["Omega"])
    assert omega.shape == (241,) and np.abs(omega - np.linspace(0.0, 6.0, 241)).max() <= 1e-14
    x = (omega + rec["E0"] - rec["Centre"]) / rec["HalfWidth"]
    avg = np.zeros((LX * LY, 241))
    for s in rec["Sites"]:
        assert s["StepsDone"] == 60
        grid = np.array(s["SqwGrid"])
        want = jackson(np.array(s["MomentsQ"]), x) / rec["HalfWidth"]
        assert grid.shape == (LX * LY, 241)
        assert np.abs(grid - want).max() <= 1e-12, (s["Site"], np.abs(grid - want).max())
        avg += grid / N
    for p in dsf["Points"]:
        nx, ny = p["q"]
        m0 = sum(np.array(s["MomentsQ"])[nx * LY + ny][0] for s in rec["Sites"]) / N
        print(p["q"], "static", m0, p["StaticSzz"])
        assert abs(m0 - p["StaticSzz"]) <= 1e-10
    assert [tuple(p["q"]) for p in dsf["Points"]] == Q
    pipi = avg[3 * LY + 1]
    print("min of the average", avg.min(), "peak at (pi, pi)", omega[pipi.argmax()], "height", pipi.max())
    assert avg.min() >= -1e-12
    assert abs(omega[pipi.argmax()] - 1.40) <= 0.025 + 1e-12


def test_option_off_changes_nothing(runs_with_and_without):
    """Without -dsf_cheb the file does not appear, and the other outputs of the run are the same bytes (timing fields blanked)."""
    off, on = runs_with_and_without
    assert not os.path.exists(str(off) + "/ChebyshevMoments.json") and os.path.exists(str(on) + "/ChebyshevMoments.json")
    for name in ("Correlations.json", "DMRGSteps.json", "DynamicalStructureFactor.json"):
        a, b = (re.sub(rb'"tDsf": [^,]*,', b'"tDsf": 0,', open(str(d) + "/" + name, "rb").read()) for d in (off, on))
        assert a == b, name


def test_truncated_run_static_sum_rule(tmp_path):
    """m = 24 cuts the basis: Moments[:, 0] of every record equals SzSz[:, c] / Norm of the same run's SpinCorrelations.json (1e-12) --
    the same truncated operators on the same state --, nothing is non-finite, and the window found from the truncated superblock
    Hamiltonian holds: StepsDone = Steps."""
    rows, _, _ = run_engine(tmp_path, *HEIS_6x2, "-mwarmup", 24, "-corr_matrix", 1, "-dsf_cheb", "6,0", "-dsf_cheb_steps", 40)
    assert any(r["NStates_SysRot"] < r["NStates_SysEnl"] for r in rows)
    recs, spin = _records(tmp_path), _records(tmp_path, "SpinCorrelations.json")
    assert len(recs) == len(spin) >= 1
    for rec, srec in zip(recs, spin):
        assert _no_nan(rec) and rec["GlobIdx"] == srec["GlobIdx"] and rec["Steps"] == 40
        szsz = np.array(srec["SzSz"])
        for s in rec["Sites"]:
            err = np.abs(np.array(s["Moments"])[:, 0] - szsz[:, s["Site"]] / srec["Norm"]).max()
            print(rec["GlobIdx"], s["Site"], "StepsDone", s["StepsDone"], "Moments[:, 0] err", err)
            assert err <= 1e-12
            assert s["StepsDone"] == 40


def test_given_window_runs_no_bound_run(tmp_path, heis_ed):
    """-dsf_cheb_window -11,6 (a negative number first: a value, not an option name): Centre = -2.5 and HalfWidth = 8.5 exactly, no Lanczos
    run for the bound (BoundSteps 0, MatMults = 30), and the moments against ED in that window to 1e-10."""
    run_engine(tmp_path, *HEIS_6x2, "-mwarmup", 64, "-dsf_cheb", "3", "-dsf_cheb_steps", 30, "-dsf_cheb_window", "-11,6")
    rec = _records(tmp_path)[-1]
    assert _no_nan(rec) and rec["Centre"] == -2.5 and rec["HalfWidth"] == 8.5 and rec["BoundSteps"] == 0 and rec["MatMults"] == 30 and "Omega" not in rec
    psi, szd, w, V = heis_ed["psi"], heis_ed["szd"], heis_ed["w"], heis_ed["V"]
    assert -11.0 < w[0] and w[-1] < 6.0
    (s,) = rec["Sites"]
    Uc = (szd * psi[None, :]) @ V
    Tn = np.cos(np.arange(31)[:, None] * np.arccos((w + 2.5) / 8.5)[None, :])
    err = np.abs(np.array(s["Moments"]) - (Uc * Uc[3][None, :]) @ Tn.T).max()
    print("given window: StepsDone", s["StepsDone"], "err", err)
    assert s["Site"] == 3 and s["StepsDone"] == 30 and "SqwGrid" not in s
    assert err <= 1e-10


def test_two_ranks_are_refused_at_start_up(tmp_path):
    d = str(tmp_path) + "/"
    cmd = [EXE, *[str(o) for o in HEIS_6x2], "-mwarmup", "8", "-dsf_cheb", "6", "-data_dir", d]
    name = "dmrgx_test_dsfc_%d" % os.getpid()
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
        assert "-dsf_cheb is not available on more than one rank" in o, o[-2000:]
    assert not os.path.exists(d + "ChebyshevMoments.json")


def test_site_outside_the_lattice_is_refused_at_start_up(tmp_path):
    out = subprocess.run([EXE, *[str(o) for o in HEIS_6x2], "-mwarmup", "8", "-dsf_cheb", "3,12", "-data_dir", str(tmp_path) + "/"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "-dsf_cheb: site 12 is outside [0, 12)" in out.stderr
    assert not os.path.exists(str(tmp_path) + "/ChebyshevMoments.json")
