"""-dsf_pm c0,c1,... (-m gpu): the engine's Chebyshev moments of the transverse dynamical correlations (TransverseDynamics.json: per
channel a plan of the neighbouring total-Sz sector, the images S+_i psi / S-_i psi of all sites written in its layout by
dmrgx_kron_term_apply_to, one dmrgx_kron_chebyshev_moments run per reference site) against the SU(2) identity with -dsf_cheb on the
Heisenberg 6 x 2 lattice, against dense exact diagonalisation (spin 1/2 and spin 1, zero and finite magnetisation, a fully polarised
target), against -corr_matrix under truncation, and with the option off.

ED: the whole lattice in the site basis (site 0 the most significant factor, as helpers.lattice_ground_state), cut to the sectors of
total Sz; nothing is truncated in the runs compared with it, so the engine's last superblock is the lattice itself."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from oracle.hamiltonian import J1J2XXZModel_SquareLattice
from oracle.qn import OpSm, OpSp, OpSz
from test_gpu_engine import EXE, run_engine
from test_gpu_dsf import HEIS_6x2, _no_nan

pytestmark = pytest.mark.gpu
CHANNELS = ("MinusPlus", "PlusMinus")


def _records(d, name="TransverseDynamics.json"):
    return json.load(open(str(d) + "/" + name))


def _last(d):
    """{channel: record} of the last measurement"""
    recs = _records(d)
    assert len(recs) >= 2 and [r["Channel"] for r in recs[-2:]] == list(CHANNELS) and recs[-1]["GlobIdx"] == recs[-2]["GlobIdx"]
    return {r["Channel"]: r for r in recs[-2:]}


def sector_ed(ham, spin, sz_target):
    """Dense ED by sectors of total Sz: the ground state of sector sz_target and, per channel, the spectrum w of the sector sz_target + 1
    (MinusPlus) or - 1 (PlusMinus) and C[i][k] = < k | O_i | psi >, O = S+ (S-), in its eigenbasis; None for a sector without states."""
    import scipy.sparse as sp
    N = ham.NumSites()
    if spin == "1":
        szd, spl = np.array([1.0, 0.0, -1.0]), np.sqrt(2.0) * np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
    else:
        szd, spl = np.array([0.5, -0.5]), np.array([[0.0, 1.0], [0.0, 0.0]])
    d = len(szd)
    single = {OpSz: sp.csr_matrix(np.diag(szd)), OpSp: sp.csr_matrix(spl), OpSm: sp.csr_matrix(spl.T)}

    def site_op(op, i):
        m = sp.identity(1, format="csr")
        for s in range(N):
            m = sp.kron(m, single[op] if s == i else sp.identity(d, format="csr"), format="csr")
        return m

    H = sp.csr_matrix((d ** N, d ** N))
    for t in ham.H(N):
        H = H + t.a * (site_op(t.Iop, t.Isite) @ site_op(t.Jop, t.Jsite))
    H = H.tocsr()
    sz_tot = np.zeros(d ** N)
    for i in range(N):
        sz_tot += site_op(OpSz, i).diagonal()
    sec0 = np.where(np.abs(sz_tot - sz_target) < 1e-9)[0]
    w0, V0 = np.linalg.eigh(H[sec0][:, sec0].toarray())
    psi = V0[:, 0]
    assert len(w0) == 1 or w0[1] - w0[0] > 1e-6                                 # a unique ground state
    out = {"E0": float(w0[0]), "w0": w0, "N": N}
    for name, sign, op in (("MinusPlus", +1, OpSp), ("PlusMinus", -1, OpSm)):
        sec1 = np.where(np.abs(sz_tot - (sz_target + sign)) < 1e-9)[0]
        if len(sec1) == 0:
            out[name] = None
            continue
        w1, V1 = np.linalg.eigh(H[sec1][:, sec1].toarray())
        U = np.array([site_op(op, i).tocsr()[sec1][:, sec0] @ psi for i in range(N)])
        out[name] = (w1, U @ V1)
    return out


def ed_moments(ed, channel, c, centre, hw, K):
    """[i][n] = < O_i psi , T_n((H' - centre) / hw) O_c psi >, n <= K"""
    w1, C = ed[channel]
    Tn = np.cos(np.arange(K + 1)[:, None] * np.arccos((w1 - centre) / hw)[None, :])
    return (C * C[c][None, :]) @ Tn.T


def _check_against_ed(rec, ed, K, tol=1e-10):
    """Every site of a record against ED in the record's own window; -> the largest error"""
    N = ed["N"]
    centre, hw = rec["Centre"], rec["HalfWidth"]
    w1, C = ed[rec["Channel"]]
    assert rec["States"] == len(w1) and centre - hw < w1[0] and centre + hw > w1[-1], (rec["Channel"], centre - hw, centre + hw, w1[0], w1[-1])
    worst = 0.0
    for s in rec["Sites"]:
        assert s["StepsDone"] == K
        mom, diag = np.array(s["Moments"]), np.array(s["Diag"])
        assert mom.shape == (N, K + 1) and diag.shape == (2 * K + 1,)
        want = ed_moments(ed, rec["Channel"], s["Site"], centre, hw, 2 * K)
        errs = {"ED": np.abs(mom - want[:, :K + 1]).max(), "Diag ED": np.abs(diag - want[s["Site"]]).max(), "Norm2": abs(diag[0] * rec["Norm"] - s["Norm2"])}
        print(rec["Channel"], "site", s["Site"], errs)
        assert errs["ED"] <= tol and errs["Diag ED"] <= tol and errs["Norm2"] <= 1e-15
        worst = max(worst, errs["ED"])
    return worst


# ---- Heisenberg 6 x 2: a singlet ground state ---------------------------------------------------------------------------------------
HEIS_STEPS = 30
HEIS_COMMON = [*HEIS_6x2, "-mwarmup", 64, "-corr_matrix", 1, "-dsf_cheb", "6,0", "-dsf_cheb_steps", HEIS_STEPS, "-dsf_cheb_window", "-11,6"]


@pytest.fixture(scope="module")
def runs_with_and_without(tmp_path_factory):
    """-corr_matrix 1 and -dsf_cheb 6,0 in the given window [-11, 6], 30 steps, nothing truncated: once alone, once with -dsf_pm 6,0."""
    d = tmp_path_factory.mktemp("dsf_pm")
    run_engine(d / "off", *HEIS_COMMON)
    run_engine(d / "on", *HEIS_COMMON, "-dsf_pm", "6,0")
    return d / "off", d / "on"


@pytest.fixture(scope="module")
def heis_sector_ed():
    return sector_ed(J1J2XXZModel_SquareLattice(Lx=6, Ly=2, heisenberg=1.0), "1/2", 0.0)


def test_singlet_ground_state_su2_identity(runs_with_and_without):
    """The ground state is a singlet, so < S-_i f(H) S+_c > = < S+_i f(H) S-_c > = 2 < Sz_i f(H) Sz_c >: Moments of both channels equal
    2 x Moments of ChebyshevMoments.json of the same run (same window, same steps) entry by entry, and each other, to 1e-10 -- the
    tolerance of test_gpu_dsf_cheb.py against ED for these moments."""
    _, on = runs_with_and_without
    pm, zz = _last(on), _records(on, "ChebyshevMoments.json")[-1]
    K = HEIS_STEPS
    for ch in CHANNELS:
        rec = pm[ch]
        assert _no_nan(rec) and rec["GlobIdx"] == zz["GlobIdx"] and rec["Steps"] == K and rec["BoundSteps"] == 0 and rec["MatMults"] == 2 * K
        assert rec["Centre"] == -2.5 and rec["HalfWidth"] == 8.5 and rec["ThetaMin"] == -11.0 and rec["ThetaMax"] == 6.0 and rec["E0"] == zz["E0"] and rec["Norm"] == zz["Norm"]
        assert rec["Sector"] == (1.0 if ch == "MinusPlus" else -1.0) and rec["States"] == 792 and "Omega" not in rec
        assert [s["Site"] for s in rec["Sites"]] == [6, 0] == [s["Site"] for s in zz["Sites"]]
    for a, b, z in zip(pm["MinusPlus"]["Sites"], pm["PlusMinus"]["Sites"], zz["Sites"]):
        assert a["StepsDone"] == b["StepsDone"] == z["StepsDone"] == K and a["r"] == z["r"] and "SqwGrid" not in a
        ma, mb, mz = np.array(a["Moments"]), np.array(b["Moments"]), np.array(z["Moments"])
        errs = {"-+ vs 2 zz": np.abs(ma - 2 * mz).max(), "+- vs 2 zz": np.abs(mb - 2 * mz).max(), "-+ vs +-": np.abs(ma - mb).max(),
                "Diag": np.abs(np.array(a["Diag"]) - 2 * np.array(z["Diag"])).max(), "MomentsQ": np.abs(np.array(a["MomentsQ"]) - 2 * np.array(z["MomentsQ"])).max()}
        print("site", a["Site"], errs, "max |Moments|", np.abs(ma).max())
        assert ma.shape == mz.shape == (12, K + 1) and np.abs(ma).max() > 0.4
        assert errs["-+ vs 2 zz"] <= 1e-10 and errs["+- vs 2 zz"] <= 1e-10 and errs["-+ vs +-"] <= 1e-10
        assert errs["Diag"] <= 1e-10 and errs["MomentsQ"] <= 12e-10
        assert abs(a["Norm2"] - 0.5) <= 1e-10 and abs(b["Norm2"] - 0.5) <= 1e-10


def test_heisenberg_against_exact_diagonalisation(runs_with_and_without, heis_sector_ed):
    """The same run against < 0 | S-_i T_n((H - Centre) / HalfWidth) S+_c | 0 > from dense ED of the 12 sites in the Sz = 1 sector (and
    the Sz = -1 sector for PlusMinus), Centre and HalfWidth read from the record, to 1e-10."""
    _, on = runs_with_and_without
    pm = _last(on)
    assert abs(pm["MinusPlus"]["E0"] - heis_sector_ed["E0"]) <= 1e-10
    for ch in CHANNELS:
        _check_against_ed(pm[ch], heis_sector_ed, HEIS_STEPS)


def test_option_off_changes_nothing(runs_with_and_without):
    """Without -dsf_pm the file does not appear, and every other output file of the run holds the same bytes once the timing fields are
    blanked.  Timings.json holds nothing but timings; DMRGRun.json also reports the device memory in use, which the measurement raises."""
    off, on = runs_with_and_without
    assert not os.path.exists(str(off) + "/TransverseDynamics.json") and os.path.exists(str(on) + "/TransverseDynamics.json")
    blank = rb'"(tDsfCheb|tCorrMatrix|eigs_seconds|LastSweepSeconds|EigensolveSeconds|DeviceBytes[A-Za-z]*|ms_stage1|ms_stage2)": [^,}\n]*'
    files = lambda d: sorted(f for f in os.listdir(str(d)) if os.path.isfile(os.path.join(str(d), f)))       # noqa: E731
    names = [f for f in files(on) if f != "TransverseDynamics.json"]
    assert names == files(off) and {"Correlations.json", "DMRGSteps.json", "ChebyshevMoments.json", "SpinCorrelations.json", "EntanglementSpectra.json", "KronStats.json", "DMRGRun.json"} <= set(names)
    for name in names:
        if name == "Timings.json":
            continue
        a, b = (re.sub(blank, b'"\\1": 0', open(str(d) + "/" + name, "rb").read()) for d in (off, on))
        assert a == b, name


# ---- channels that differ: an XXZ chain at finite magnetisation ---------------------------------------------------------------------
def test_xxz_chain_at_finite_magnetisation(tmp_path):
    """8 x 1, Jz1 != J1, -qn_sector 1, nothing truncated, the window from the bound run (40 Lanczos steps, both ends from Ritz values):
    both channels against dense ED (sectors Sz = 2 and Sz = 0) to 1e-10, StepsDone = Steps, the window holds the ED spectrum of its
    sector.  The channels differ from each other and from 2 x zz (-dsf_cheb of the same run, column 0: T_0 = 1 whatever the window) by
    more than 1e-2: on site < S- S+ > = 1/2 - < Sz >, < S+ S- > = 1/2 + < Sz >, 2 < Sz Sz > = 1/2."""
    K = 30
    run_engine(tmp_path, "-Lx", 8, "-Ly", 1, "-J1", 1, "-Jz1", 0.5, "-J2", 0.4, "-Jz2", 0.2, "-qn_sector", 1, "-mwarmup", 64, "-nsweeps", 1, "-H_eps_tol", 1e-13,
               "-dsf_pm", "3,0", "-dsf_cheb", "3,0", "-dsf_cheb_steps", K)
    ed = sector_ed(J1J2XXZModel_SquareLattice(Lx=8, Ly=1, J1=1.0, Jz1=0.5, J2=0.4, Jz2=0.2), "1/2", 1.0)
    pm, zz = _last(tmp_path), _records(tmp_path, "ChebyshevMoments.json")[-1]
    assert abs(pm["MinusPlus"]["E0"] - ed["E0"]) <= 1e-10
    for ch, sector, states in (("MinusPlus", 2.0, 28), ("PlusMinus", 0.0, 70)):
        rec = pm[ch]
        assert _no_nan(rec) and rec["Sector"] == sector and rec["States"] == states and rec["Steps"] == K and rec["BoundSteps"] == 40 and rec["MatMults"] == 40 + 2 * K
        w1 = ed[ch][0]
        print(ch, "window", rec["Centre"] - rec["HalfWidth"], rec["Centre"] + rec["HalfWidth"], "ED", w1[0], w1[-1], "Ritz", rec["ThetaMin"], rec["ThetaMax"])
        assert w1[0] - 1e-9 <= rec["ThetaMin"] and rec["ThetaMax"] <= w1[-1] + 1e-9
        _check_against_ed(rec, ed, K)
    for a, b, z in zip(pm["MinusPlus"]["Sites"], pm["PlusMinus"]["Sites"], zz["Sites"]):
        assert a["Site"] == b["Site"] == z["Site"]
        ma, mb, mz = np.array(a["Moments"]), np.array(b["Moments"]), np.array(z["Moments"])
        gaps = {"-+ vs +-": np.abs(ma[:, 0] - mb[:, 0]).max(), "-+ vs 2 zz": np.abs(ma[:, 0] - 2 * mz[:, 0]).max(), "+- vs 2 zz": np.abs(mb[:, 0] - 2 * mz[:, 0]).max()}
        print("site", a["Site"], gaps)
        assert min(gaps.values()) > 1e-2


def test_spin_one_chain_against_exact_diagonalisation(tmp_path):
    """-spin 1, 6 x 1, nothing truncated: both channels against ED of the 3^6 lattice (S+ = sqrt 2 (|1><0| + |0><-1|)) to 1e-10."""
    K = 30
    run_engine(tmp_path, "-spin", 1, "-Lx", 6, "-Ly", 1, "-heisenberg", 1, "-mwarmup", 100, "-nsweeps", 1, "-H_eps_tol", 1e-13, "-dsf_pm", "2,5", "-dsf_cheb_steps", K)
    ed = sector_ed(J1J2XXZModel_SquareLattice(Lx=6, Ly=1, heisenberg=1.0), "1", 0.0)
    pm = _last(tmp_path)
    assert abs(pm["MinusPlus"]["E0"] - ed["E0"]) <= 1e-10
    for ch in CHANNELS:
        assert _no_nan(pm[ch]) and pm[ch]["BoundSteps"] == 40
        _check_against_ed(pm[ch], ed, K)


# ---- a fully polarised target: the neighbouring sector above it has no states ---------------------------------------------------------
POLARISED = ["-Lx", 6, "-Ly", 1, "-heisenberg", 1, "-qn_sector", 3, "-mwarmup", 16, "-nsweeps", 1, "-H_eps_tol", 1e-13]


def test_fully_polarised_target(tmp_path):
    """6 x 1, -qn_sector 3 (all spins up; the run completes without the option too): MinusPlus has States 0, no MatMults, StepsDone 0 and
    no tables for every site -- a record, not an error -- at every measurement; PlusMinus gives the one-magnon moments against ED to
    1e-10 at the measurement of the warm-up, whose two blocks are the exact three-site blocks (6 states in the sector).  The blocks of
    the sweep keep only the sectors the target state lives in -- one state each for a polarised target --, so its measurement sees a
    magnon on the two centre sites only (2 states; S- of site 5, inside a block, has no image: Norm2 0 and no step): the single-target
    caveat in its plainest form, checked here as such."""
    K = 12
    run_engine(tmp_path / "plain", *POLARISED)
    run_engine(tmp_path / "pm", *POLARISED, "-dsf_pm", "2,5", "-dsf_cheb_steps", K)
    ed = sector_ed(J1J2XXZModel_SquareLattice(Lx=6, Ly=1, heisenberg=1.0), "1/2", 3.0)
    recs = _records(tmp_path / "pm")
    assert len(recs) == 4 and [r["Channel"] for r in recs] == 2 * list(CHANNELS) and [r["LoopType"] for r in recs] == ["Warmup", "Warmup", "Sweep", "Sweep"]
    for up in (recs[0], recs[2]):
        assert ed["MinusPlus"] is None and _no_nan(up) and up["Sector"] == 4.0 and up["States"] == 0 and up["MatMults"] == 0 and up["BoundSteps"] == 0
        assert [s["Site"] for s in up["Sites"]] == [2, 5] and all(s["StepsDone"] == 0 and s["Norm2"] == 0.0 and "Moments" not in s and "Diag" not in s for s in up["Sites"])
    down = recs[1]
    assert _no_nan(down) and down["Sector"] == 2.0 and down["States"] == 6 and abs(down["E0"] - ed["E0"]) <= 1e-10
    _check_against_ed(down, ed, K)
    assert _no_nan(recs[3]) and recs[3]["Sector"] == 2.0 and recs[3]["States"] == 2
    for s in down["Sites"] + recs[3]["Sites"][:1]:
        assert s["StepsDone"] == K and abs(s["Norm2"] - 1.0) <= 1e-12      # < S+ S- > = 1 on an up spin
    inner = recs[3]["Sites"][1]
    assert inner["Site"] == 5 and inner["Norm2"] == 0.0 and inner["StepsDone"] == 0 and np.abs(np.array(inner["Moments"])).max() == 0.0


# ---- under truncation ---------------------------------------------------------------------------------------------------------------
def test_truncated_run_static_sum_rule_and_positive_average(tmp_path):
    """m = 24 cuts the basis (the lattice and m of test_gpu_dsf_cheb.py::test_truncated_run_static_sum_rule), all twelve reference sites:
    Moments[:, 0] of MinusPlus equals column c of SmSp / Norm of the same run's SpinCorrelations.json, of PlusMinus column c of SpSm /
    Norm (1e-12): inner products of the same images of the same truncated operators.  Nothing is non-finite; the windows found on the
    truncated superblock Hamiltonians hold (StepsDone = Steps); and the average of SqwGrid over all c -- a positive measure under a
    positive kernel -- is >= -1e-12 of its maximum."""
    K = 30
    rows, _, _ = run_engine(tmp_path, *HEIS_6x2, "-mwarmup", 24, "-corr_matrix", 1, "-dsf_pm", ",".join(str(c) for c in range(12)), "-dsf_cheb_steps", K, "-dsf_cheb_omega", "0,6,61")
    assert any(r["NStates_SysRot"] < r["NStates_SysEnl"] for r in rows)
    recs, spin = _records(tmp_path), _records(tmp_path, "SpinCorrelations.json")
    assert len(recs) == 2 * len(spin) >= 2
    for k, srec in enumerate(spin):
        for rec, table in ((recs[2 * k], "SmSp"), (recs[2 * k + 1], "SpSm")):
            assert _no_nan(rec) and rec["GlobIdx"] == srec["GlobIdx"] and rec["Channel"] == ("MinusPlus" if table == "SmSp" else "PlusMinus")
            assert rec["Steps"] == K and rec["MatMults"] == 40 + 12 * K and sorted(s["Site"] for s in rec["Sites"]) == list(range(12))
            tab = np.array(srec[table])
            omega = np.array(rec["Omega"])
            avg = np.zeros((12, len(omega)))
            for s in rec["Sites"]:
                err = np.abs(np.array(s["Moments"])[:, 0] - tab[:, s["Site"]] / srec["Norm"]).max()
                assert err <= 1e-12, (rec["GlobIdx"], table, s["Site"], err)
                assert s["StepsDone"] == K
                grid = np.array(s["SqwGrid"])
                assert grid.shape == (12, 61)
                avg += grid / 12
            print(rec["GlobIdx"], rec["Channel"], "min of the average", avg.min(), "max", avg.max())
            assert avg.max() > 0.1 and avg.min() >= -1e-12 * avg.max()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_two_ranks_are_refused_at_start_up(tmp_path):
    d = str(tmp_path) + "/"
    cmd = [EXE, *[str(o) for o in HEIS_6x2], "-mwarmup", "8", "-dsf_pm", "6", "-data_dir", d]
    name = "dmrgx_test_dsfpm_%d" % os.getpid()
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
        assert "-dsf_pm is not available on more than one rank" in o, o[-2000:]
    assert not os.path.exists(d + "TransverseDynamics.json")


def test_site_outside_the_lattice_is_refused_at_start_up(tmp_path):
    out = subprocess.run([EXE, *[str(o) for o in HEIS_6x2], "-mwarmup", "8", "-dsf_pm", "3,12", "-data_dir", str(tmp_path) + "/"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "-dsf_pm: site 12 is outside [0, 12)" in out.stderr
    assert not os.path.exists(str(tmp_path) + "/TransverseDynamics.json")
