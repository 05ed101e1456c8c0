"""-nstates k / -state_weights w0,...: the k lowest states of the target sector in the sweep engine (-m gpu), found one after another by
dmrgx_eigs_lowest_orth and truncated with the state-averaged density matrix, against exact diagonalisation of the 6 x 2 and the 3 x 4
Heisenberg lattice (12 sites, Sz = 0: 924 states).  -mwarmup 64 keeps every state of a 12-site lattice, so the engine's superblock is
the lattice itself.

ED: 6 x 2: E = -10.10564932, -8.68857893, -8.33800372, -7.89301581 (gaps >= 0.35), S(S+1) = 0, 2, 2, 2.  3 x 4 (Lx 3, Ly 4): -7.53013717,
-6.87172423, -5.83766888, -5.63937931, -5.57195959, then an exactly degenerate pair at -5.43059835: states 5 and 6 of -nstates 7.
(The 4 x 3 lattice, whose pair sits at states 1 and 2 -- -6.44271488, -5.74011378 twice, -5.56803858 --, cannot be run: with Ly = 3 the
warm-up's exact blocks already reach half of the 12 sites, and the engine refuses a warm-up without a step, as the reference does.)

Energy bound: a Ritz value lies within its residual of an eigenvalue of P H P, and P is that of the inexact states below -- a state with
residual r_q whose level is g_q away from the other levels is within r_q / g_q of an eigenvector, which moves the eigenvalues of P H P by
at most 4 ||H|| r_q / g_q:  |E_s - w_s| <= r_s + 4 ||H|| sum_{q<s} r_q / g_q + 1e-10, ||H|| = max |w|.  For a degenerate pair g is the
distance to the levels outside the pair (any vector of the pair's space serves)."""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle.hamiltonian import J1J2XXZModel_SquareLattice
from helpers import lattice_ground_state
from test_gpu_engine import EXE, run_engine
from test_gpu_dsf import HEIS_6x2
from test_gpu_dsf_sites import heis_ed            # noqa: F401  (module-scoped fixture, built once here)

pytestmark = pytest.mark.gpu
N = 12
HEIS_3x4 = ["-Lx", 3, "-Ly", 4, "-heisenberg", 1]


def _records(d):
    return json.load(open(str(d) + "/TargetedStates.json"))


@pytest.fixture(scope="module")
def heis34_w():
    """The spectrum of the 3 x 4 Heisenberg lattice in the Sz = 0 sector, written the way heis_ed does it"""
    ham = J1J2XXZModel_SquareLattice(Lx=3, Ly=4, heisenberg=1.0)
    _, _, site_op = lattice_ground_state(ham)
    sector = np.array([i for i in range(2 ** N) if bin(i).count("1") == N // 2])
    H = None
    for t in ham.H(N):
        h = t.a * (site_op(t.Iop, t.Isite) @ site_op(t.Jop, t.Jsite))
        H = h if H is None else H + h
    w = np.linalg.eigvalsh(H.tocsr()[sector][:, sector].toarray())
    w.setflags(write=False)
    return w


def _energy_bounds(w, rec, pair_tol=1e-6):
    """r_s + 4 ||H|| sum_{q<s} r_q / g_q + 1e-10 per state; g_q: the distance of w_q to the levels further than pair_tol from it"""
    hnorm = np.abs(w).max()
    r = np.array(rec["Residuals"])
    g = np.array([np.abs(w[np.abs(w - w[q]) > pair_tol] - w[q]).min() for q in range(len(r))])
    return np.array([r[s] + 4.0 * hnorm * np.sum(r[:s] / g[:s]) + 1e-10 for s in range(len(r))]), g


def _throughput(timings):
    """steps per second of a run, from the Total column of Timings.json"""
    total = sum(row[1] for row in timings["table"])
    return len(timings["table"]) / total


def _untruncated(tmp_path_factory, lattice, name, k=4, extra=()):
    d = tmp_path_factory.mktemp(name)
    rows, run, timings = run_engine(d, *lattice, "-mwarmup", 64, *extra, "-nstates", k)
    _, run1, timings1 = run_engine(tmp_path_factory.mktemp(name + "_one"), *lattice, "-mwarmup", 64, *extra, "-nstates", 1)
    recs = _records(d)
    print("%s -nstates k: per-state MatMults %s Seconds %s of the last step; %d steps, %.2f sites/s (MatMults %d); -nstates 1: %.2f sites/s (MatMults %d)"
          % (name, recs[-1]["MatMults"], ["%.4f" % s for s in recs[-1]["Seconds"]], len(rows), _throughput(timings), run["MatMults"], _throughput(timings1), run1["MatMults"]))
    print("  per-state totals over the run: MatMults %s Seconds %s" % (
        [sum(r["MatMults"][s] for r in recs if len(r["MatMults"]) > s) for s in range(k)],
        ["%.4f" % sum(r["Seconds"][s] for r in recs if len(r["Seconds"]) > s) for s in range(k)]))
    return rows, run, recs


@pytest.fixture(scope="module")
def run_6x2(tmp_path_factory):
    return _untruncated(tmp_path_factory, HEIS_6x2, "targets_6x2")


@pytest.fixture(scope="module")
def run_3x4(tmp_path_factory):
    # (with Ly = 4 the warm-up ends on a superblock of 8 sites: one sweep brings the whole lattice, and its last step is a measurement)
    return _untruncated(tmp_path_factory, HEIS_3x4, "targets_3x4", k=7, extra=("-nsweeps", 1))


def _common_checks(rows, run, recs, w):
    rec = recs[-1]
    E = np.array(rec["Energies"])
    bounds, g = _energy_bounds(w, rec)
    print("E", E, "ED", w[:4], "|E - w|", np.abs(E - w[:4]), "bounds", bounds, "g", g, "residuals", rec["Residuals"], "S(S+1)", rec["TotalSpin2"])
    assert rec["NStates"] == 4 and rec["Weights"] == [0.25] * 4 and all(c == 1 for c in rec["Converged"])
    assert (np.abs(E - w[:4]) <= bounds).all()
    assert np.abs(np.array(rec["Overlaps"]) - np.eye(4)).max() <= 1e-10
    assert np.abs(np.array(rec["TotalSpin2"]) - np.array([0.0, 2.0, 2.0, 2.0])).max() <= 1e-8
    step = [r for r in rows if r["GlobIdx"] == rec["GlobIdx"]]
    assert len(step) == 1 and step[0]["GSEnergy"] == float("%.12g" % E[0])          # (DMRGSteps.json prints GSEnergy with 12 digits)
    assert sum(sum(r["MatMults"]) for r in recs) == run["MatMults"]
    assert [r["GlobIdx"] for r in recs] == [r["GlobIdx"] for r in rows]
    for r in recs:                      # small superblocks hold fewer states: weights dropped and renormalised
        k = r["NStates"]
        assert 1 <= k <= 4 and all(len(r[key]) == k for key in ("Weights", "Energies", "Residuals", "Converged", "MatMults", "Seconds", "StartTransformed", "StartRejected"))
        assert abs(sum(r["Weights"]) - 1.0) <= 1e-15 and ("TotalSpin2" in r) == ("Overlaps" in r)
    assert run["TargetStates"] == 4 and run["TargetWeights"] == [0.25] * 4


def test_6x2_four_states_against_exact_diagonalisation(run_6x2, heis_ed):
    w = heis_ed["w"]
    assert np.abs(w[:4] - np.array([-10.10564932, -8.68857893, -8.33800372, -7.89301581])).max() <= 1e-8 and np.diff(w[:5]).min() >= 0.35
    _common_checks(*run_6x2, w)


def test_3x4_degenerate_pair_is_resolved(run_3x4, heis34_w):
    """-nstates 7 on the 3 x 4 lattice: states 5 and 6 are an exactly degenerate pair, which one Krylov sequence cannot resolve"""
    w = heis34_w
    assert np.abs(w[:7] - np.array([-7.53013717, -6.87172423, -5.83766888, -5.63937931, -5.57195959, -5.43059835, -5.43059835])).max() <= 1e-8 and abs(w[5] - w[6]) <= 1e-12
    rows, run, recs = run_3x4
    rec = recs[-1]
    assert rows[-1]["NSites_SysEnl"] + rows[-1]["NSites_EnvEnl"] == N and rows[-1]["GlobIdx"] == rec["GlobIdx"]
    E = np.array(rec["Energies"])
    bounds, g = _energy_bounds(w, rec)
    print("E", E, "ED", w[:7], "|E - w|", np.abs(E - w[:7]), "bounds", bounds, "g", g, "S(S+1)", rec["TotalSpin2"])
    assert rec["NStates"] == 7 and all(c == 1 for c in rec["Converged"])
    assert (np.abs(E - w[:7]) <= bounds).all()
    assert abs(E[5] - E[6]) <= 1e-9
    assert np.abs(np.array(rec["Overlaps"]) - np.eye(7)).max() <= 1e-10
    spin2 = np.array(rec["TotalSpin2"])
    assert np.abs(spin2[:5] - np.round(spin2[:5])).max() <= 1e-8 and abs(spin2[0]) <= 1e-8      # S(S+1) of the non-degenerate states is that of a definite spin
    assert sum(sum(r["MatMults"]) for r in recs) == run["MatMults"]


@pytest.fixture(scope="module")
def truncated_runs(tmp_path_factory):
    out = {}
    for name, extra in (("equal", ()), ("ground_only", ("-state_weights", "1,0,0"))):
        d = tmp_path_factory.mktemp("targets_cut_" + name)
        rows, run, _ = run_engine(d, *HEIS_6x2, "-mwarmup", 16, "-nsweeps", 2, "-nstates", 3, *extra)
        out[name] = (rows, run, _records(d))
    return out


def test_truncated_run(truncated_runs, heis_ed):
    w = heis_ed["w"]
    rows, run, recs = truncated_runs["equal"]
    full = {r["GlobIdx"] for r in rows if r["NSites_SysEnl"] + r["NSites_EnvEnl"] == N}
    assert len(full) >= 2 * (N - 4)
    for rec in recs:
        assert np.isfinite(np.array([rec[k] for k in ("Energies", "Residuals", "Seconds", "Weights")], dtype=float)).all()
        if rec["GlobIdx"] not in full:
            continue
        E = np.array(rec["Energies"])
        assert rec["NStates"] == 3 and (E >= w[:3] - 1e-10).all(), (rec["GlobIdx"], E - w[:3])      # Ritz values interlace
        assert (np.diff(E) > 0).all() and all(c == 1 for c in rec["Converged"])
    for r in rows:
        assert np.isfinite([r["GSEnergy"], r["TruncErr_Sys"], r["TruncErr_Env"]]).all()
        assert -1e-14 <= r["TruncErr_Sys"] <= 1.0 and -1e-14 <= r["TruncErr_Env"] <= 1.0
    assert any(r["TruncErr_Sys"] > 1e-10 for r in rows if r["GlobIdx"] in full)                     # the cut truncates


def test_weights_reach_the_truncation(truncated_runs, heis_ed):
    """The same run with -state_weights 1,0,0 optimises the blocks for the ground state alone: the first excited state, computed in that
    basis, is the poorer one."""
    w = heis_ed["w"]
    err = {name: truncated_runs[name][2][-1]["Energies"][1] - w[1] for name in ("equal", "ground_only")}
    print("last step, Energies[1] - w[1]: equal weights %.3e, weights 1,0,0 %.3e" % (err["equal"], err["ground_only"]))
    assert truncated_runs["ground_only"][2][-1]["Weights"] == [1.0, 0.0, 0.0]
    assert err["equal"] < err["ground_only"]


def test_option_off_is_the_present_run(tmp_path):
    common = [*HEIS_6x2, "-mwarmup", 16, "-nsweeps", 1]
    a_rows, a_run, _ = run_engine(tmp_path / "plain", *common)
    b_rows, b_run, _ = run_engine(tmp_path / "one", *common, "-nstates", 1)
    assert not os.path.exists(str(tmp_path / "plain" / "TargetedStates.json")) and not os.path.exists(str(tmp_path / "one" / "TargetedStates.json"))
    assert len(a_rows) == len(b_rows)
    for a, b in zip(a_rows, b_rows):
        assert (a["GSEnergy"], a["TruncErr_Sys"], a["TruncErr_Env"]) == (b["GSEnergy"], b["TruncErr_Sys"], b["TruncErr_Env"])
    assert list(a_run.keys()) == list(b_run.keys()) and "TargetStates" not in a_run and "TargetWeights" not in a_run
    assert a_run["MatMults"] == b_run["MatMults"]


def test_refusals_at_start_up(tmp_path):
    def refused(*opts):
        out = subprocess.run([EXE, *[str(o) for o in HEIS_6x2], "-mwarmup", "8", *[str(o) for o in opts], "-data_dir", str(tmp_path) + "/"], capture_output=True, text=True, timeout=120)
        assert out.returncode != 0
        return out.stdout + out.stderr

    assert "cannot be combined with -noise" in refused("-nstates", 2, "-noise", "1e-4")
    assert "cannot be combined with -noise" in refused("-nstates", 2, "-noise_warmup", "1e-4")
    assert "-nstates takes a number of states from 1 to 8. Got 9." in refused("-nstates", 9)
    assert "-state_weights" in refused("-nstates", 2, "-state_weights", "1,1,1")
    cmd = [EXE, *[str(o) for o in HEIS_6x2], "-mwarmup", "8", "-nsweeps", "1", "-nstates", "2", "-data_dir", str(tmp_path) + "/"]
    name = "dmrgx_test_targets_%d" % os.getpid()
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
        assert "-nstates 2 is not available on more than one rank" in o, o[-2000:]
