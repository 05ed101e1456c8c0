"""-spin_penalty l0,l1,... / -spin_penalty_warmup l in the sweep engine (-m gpu): the superblock solves H' = H + l S-_tot S+_tot, which in
the sector Sz = M moves every level of spin S by l [S (S + 1) - M (M + 1)] and leaves S = |M| alone, so that -nstates k finds the k lowest
levels of that spin.  Against exact diagonalisation with the spin resolved (tests/spin_penalty_ed.py) of the 6 x 2 Heisenberg lattice
(12 sites; Sz = 0: 924 states), whose lowest levels are the tower S = 0, 1, 1, 1 at -10.10564932, -8.68857893, -8.33800372, -7.89301581
and whose lowest singlets are -10.10564932, -7.00244885, -6.74602273.  -mwarmup 64 keeps every state of a 12-site lattice, so every step
of a sweep solves the lattice itself.

The model options: -heisenberg 1 is J (Sz Sz + (S+ S- + S- S+) / 2) on nearest neighbours; in the J1-J2 form the engine multiplies
S+ S- + S- S+ by J1 and J2 as given, so the spin-rotation invariant model with J2 / J1 = 0.5 is -J1 0.5 -Jz1 1 -J2 0.25 -Jz2 0.5."""
import json
import os

import numpy as np
import pytest

from oracle.hamiltonian import J1J2XXZModel_SquareLattice
import spin_penalty_ed as ed
from test_gpu_engine import run_engine

pytestmark = pytest.mark.gpu
HEIS_6x2 = ["-Lx", 6, "-Ly", 2, "-heisenberg", 1]
J1J2_6x2 = ["-Lx", 6, "-Ly", 2, "-J1", 0.5, "-Jz1", 1, "-J2", 0.25, "-Jz2", 0.5]
EXACT = ["-mwarmup", 64, "-nsweeps", 1, "-H_eps_tol", 1e-13]
N = 12


def _records(d, name="SpinPenalty.json"):
    return json.load(open(str(d) + "/" + name))


@pytest.fixture(scope="module")
def ed_sz0():
    return ed.levels(J1J2XXZModel_SquareLattice(Lx=6, Ly=2, heisenberg=1.0), 0)


@pytest.fixture(scope="module")
def singlets(ed_sz0):
    return ed.lowest_of_spin(ed_sz0, 0, 3)


@pytest.fixture(scope="module")
def exact_runs(tmp_path_factory):
    """6 x 2 Heisenberg, nothing truncated, -nstates 3, one sweep: with -spin_penalty 2 and without"""
    out = {}
    for name, extra in (("penalty", ("-spin_penalty", 2)), ("plain", ())):
        d = tmp_path_factory.mktemp("spin_penalty_exact_" + name)
        rows, run, _ = run_engine(d, *HEIS_6x2, *EXACT, "-nstates", 3, *extra)
        out[name] = (d, rows, run)
    return out


def _check_records(recs, rows, k):
    """one record per step, every one with the three identities as reported"""
    assert [r["GlobIdx"] for r in recs] == [r["GlobIdx"] for r in rows]
    for r in recs:
        n = len(r["Eigenvalue"])
        assert 1 <= n <= k and all(len(r[key]) == n for key in ("RaisedNorm2", "Energy", "TotalSpin2"))


def test_three_lowest_singlets_of_the_exact_lattice(exact_runs, ed_sz0, singlets):
    """-nstates 3 -spin_penalty 2: the triplets are 4 higher, the quintets 12, so the three lowest states of H' are the three lowest singlets.
    Energy against ED to 1e-9, TotalSpin2 < 1e-8.  Without the option the same run holds a triplet among its three states -- the second
    Sz = 0 level of this lattice is one (checked on the ED side here, and in tests/test_spin_penalty_host.py without a GPU)."""
    order = np.argsort(ed_sz0["energy"])
    assert abs(ed_sz0["spin2"][order][1] - 2.0) <= 1e-10 and abs(ed_sz0["spin2"][order][0]) <= 1e-10      # the second level is a triplet
    assert singlets[2] < ed_sz0["energy"][order][1] + 2.0 * 2.0 - 0.5                                    # ... and stays above the singlets at weight 2
    d, rows, run = exact_runs["penalty"]
    recs = _records(d)
    _check_records(recs, rows, 3)
    rec = recs[-1]
    assert rec["LoopType"] == "Sweep" and rec["Lambda"] == 2.0 and rows[-1]["NSites_SysEnl"] + rows[-1]["NSites_EnvEnl"] == N
    E, spin2, raised, eig = (np.array(rec[k]) for k in ("Energy", "TotalSpin2", "RaisedNorm2", "Eigenvalue"))
    print("Energy", E, "ED singlets", singlets, "|diff|", np.abs(E - singlets), "TotalSpin2", spin2)
    assert len(E) == 3 and np.abs(E - singlets).max() <= 1e-9
    assert np.abs(spin2).max() < 1e-8 and raised.min() >= 0.0
    assert np.array_equal(E, eig - 2.0 * raised) and np.array_equal(spin2, raised)                       # M = 0
    assert rows[-1]["GSEnergy"] == float("%.12g" % eig[0])                                               # GSEnergy stays the solver's eigenvalue
    assert [r["Lambda"] for r in recs if r["LoopType"] == "Warmup"] == [0.0] * sum(r["LoopType"] == "Warmup" for r in recs)
    assert run["SpinPenalty"] == [2.0] and run["SpinPenaltyWarmup"] == 0.0
    # the independent all-sites route of TargetedStates.json agrees: three singlets, with the eigenvalues of H' as its Energies
    trec = _records(d, "TargetedStates.json")[-1]
    assert trec["GlobIdx"] == rec["GlobIdx"] and np.abs(np.array(trec["TotalSpin2"])).max() < 1e-8 and trec["Energies"] == rec["Eigenvalue"]
    # without the option: the tower -- a triplet among the three
    dp, _, runp = exact_runs["plain"]
    assert not os.path.exists(str(dp) + "/SpinPenalty.json") and "SpinPenalty" not in runp and "SpinPenaltyWarmup" not in runp
    plain = _records(dp, "TargetedStates.json")[-1]
    print("without the option: Energies", plain["Energies"], "TotalSpin2", plain["TotalSpin2"])
    assert any(abs(s - 2.0) <= 1e-8 for s in plain["TotalSpin2"])
    assert np.abs(np.array(plain["Energies"]) - ed_sz0["energy"][order][:3]).max() <= 1e-9


def test_sector_m_equal_one(tmp_path):
    """-qn_sector 1 -nstates 2 -spin_penalty 2: S = 1 is the lowest spin of the sector and is not moved -- Eigenvalue - Energy < 1e-9,
    TotalSpin2 = 2 --, and the second state follows ED of H' itself (to 1e-9: eigenvalue, energy and spin)."""
    lv = ed.levels(J1J2XXZModel_SquareLattice(Lx=6, Ly=2, heisenberg=1.0), 1, 2.0)
    rows, run, _ = run_engine(tmp_path, *HEIS_6x2, *EXACT, "-qn_sector", 1, "-nstates", 2, "-spin_penalty", 2)
    recs = _records(tmp_path)
    _check_records(recs, rows, 2)
    rec = recs[-1]
    E, spin2, raised, eig = (np.array(rec[k]) for k in ("Energy", "TotalSpin2", "RaisedNorm2", "Eigenvalue"))
    print("Eigenvalue", eig, "ED of H'", lv["eigenvalue"][:2], "Energy", E, "ED", lv["energy"][:2], "TotalSpin2", spin2, "ED", lv["spin2"][:2])
    assert rec["Lambda"] == 2.0 and len(eig) == 2
    assert abs(eig[0] - E[0]) < 1e-9 and abs(spin2[0] - 2.0) <= 1e-8 and abs(E[0] - lv["energy"][0]) <= 1e-9
    assert abs(eig[1] - lv["eigenvalue"][1]) <= 1e-9 and abs(E[1] - lv["energy"][1]) <= 1e-9 and abs(spin2[1] - lv["spin2"][1]) <= 1e-8
    assert np.array_equal(spin2, raised + 2.0) and raised.min() >= 0.0


# the two lattices of the truncated runs: the issue's J2 / J1 = 0.5 -- whose ground state on this two-leg lattice is the exact product of
# rung singlets at E = -4.5, so m = 16 cuts nothing off it -- and J2 = 0, which m = 16 does truncate
CUT_MODELS = {"j2_0.5": (J1J2_6x2, dict(J1=0.5, Jz1=1.0, J2=0.25, Jz2=0.5)), "j2_0": (HEIS_6x2, dict(heisenberg=1.0))}
# E - E_ED at the last step of the truncated runs, (-spin_penalty 2, no option), measured once on an MI355X (docstring of the test)
CUT_MEASURED = {"j2_0.5": (-3.553e-13, -8.882e-15), "j2_0": (4.463e-07, 4.463e-07)}
# what the eigensolver adds to either energy at -H_eps_tol 1e-12: the residual bound tol * |E| with |E| <= 11, rounded up
SOLVER_FLOOR = 2e-11


@pytest.fixture(scope="module")
def truncated_runs(tmp_path_factory):
    """6 x 2 at m = 16, one sweep, per lattice: -spin_penalty 2 and no option; for J2 = 0 also -spin_penalty 0"""
    out = {}
    for model, (opts, _) in CUT_MODELS.items():
        for name, extra in (("penalty", ("-spin_penalty", 2)), ("plain", ())) + ((("zero", ("-spin_penalty", 0)),) if model == "j2_0" else ()):
            d = tmp_path_factory.mktemp("spin_penalty_cut_%s_%s" % (model.replace(".", ""), name))
            rows, run, _ = run_engine(d, *opts, "-mwarmup", 16, "-nsweeps", 1, "-H_eps_tol", 1e-12, *extra)
            out[model, name] = (d, rows, run)
    return out


@pytest.mark.parametrize("model", list(CUT_MODELS))
def test_identities_hold_under_truncation(truncated_runs, model):
    """m = 16: RaisedNorm2 >= 0 and TotalSpin2 = RaisedNorm2 + M (M + 1) to 1e-12 in every record, as reported; Energy = Eigenvalue -
    lambda RaisedNorm2 likewise.  Energy of state 0 at the last step against the ground-state energy of the same run without the option:
    both are variational energies of H in truncated bases that differ, so they agree at the scale of their own errors against ED -- the
    bound is twice the larger of the two errors, measured once, plus what the eigensolver's tolerance allows either energy.
    Measured on an MI355X, E - E_ED of (-spin_penalty 2, no option):
      J2 / J1 = 0.5 (nothing truncated: the rung-singlet product): -3.553e-13, -8.882e-15 (E_ED = -9 exactly); the two runs differ by 3.46e-13
      J2 = 0 (largest TruncErr_Sys 2.35e-08): 4.463e-07, 4.463e-07 (E_ED = -10.105649318403); the two runs differ by 2.45e-13,
        RaisedNorm2 of the penalised state 2.49e-11"""
    d, rows, run = truncated_runs[model, "penalty"]
    recs = _records(d)
    _check_records(recs, rows, 1)
    print(model, "largest TruncErr_Sys", max(r["TruncErr_Sys"] for r in rows))
    if model == "j2_0":
        assert any(r["TruncErr_Sys"] > 1e-10 for r in rows)                                            # the cut truncates
    for r in recs:
        raised, spin2, E, eig = r["RaisedNorm2"][0], r["TotalSpin2"][0], r["Energy"][0], r["Eigenvalue"][0]
        assert raised >= 0.0 and abs(spin2 - raised) <= 1e-12 and abs(E - (eig - r["Lambda"] * raised)) <= 1e-12
    lv = ed.levels(J1J2XXZModel_SquareLattice(Lx=6, Ly=2, **CUT_MODELS[model][1]), 0)
    e_ed = lv["energy"].min()
    assert abs(lv["spin2"][np.argmin(lv["energy"])]) <= 1e-10                                          # the ground state is a singlet: the penalty leaves it alone
    _, rows_plain, _ = truncated_runs[model, "plain"]
    e_pen, e_plain = recs[-1]["Energy"][0], rows_plain[-1]["GSEnergy"]
    print("%s: ED %.12f; -spin_penalty 2: Energy %.12f (err %.3e, RaisedNorm2 %.3e, Eigenvalue %.12f); plain: GSEnergy %.12f (err %.3e); difference %.3e"
          % (model, e_ed, e_pen, e_pen - e_ed, recs[-1]["RaisedNorm2"][0], recs[-1]["Eigenvalue"][0], e_plain, e_plain - e_ed, e_pen - e_plain))
    assert rows[-1]["NSites_SysEnl"] + rows[-1]["NSites_EnvEnl"] == N and e_pen >= e_ed - 1e-10 and e_plain >= e_ed - 1e-10
    assert abs(e_pen - e_plain) <= 2.0 * max(abs(x) for x in CUT_MEASURED[model]) + SOLVER_FLOOR


def test_zero_weight_is_the_run_without_the_option(truncated_runs):
    """-spin_penalty 0 writes DMRGSteps.json byte for byte as a run without the option and no SpinPenalty.json"""
    dz, _, runz = truncated_runs["j2_0", "zero"]
    dp, _, runp = truncated_runs["j2_0", "plain"]
    assert open(str(dz) + "/DMRGSteps.json", "rb").read() == open(str(dp) + "/DMRGSteps.json", "rb").read()
    assert not os.path.exists(str(dz) + "/SpinPenalty.json") and not os.path.exists(str(dp) + "/SpinPenalty.json")
    assert list(runz.keys()) == list(runp.keys()) and "SpinPenalty" not in runz and runz["MatMults"] == runp["MatMults"]


@pytest.mark.parametrize("extra", [("-H_eps_type", "gd"), ("-prune_ops", 0)], ids=["gd", "prune_ops_0"])
def test_solver_types_and_unpruned_operators_give_the_same_singlets(tmp_path, extra, singlets):
    rows, run, _ = run_engine(tmp_path, *HEIS_6x2, *EXACT, "-nstates", 3, "-spin_penalty", 2, *extra)
    rec = _records(tmp_path)[-1]
    E = np.array(rec["Energy"])
    print(extra, "Energy", E, "|diff|", np.abs(E - singlets), "TotalSpin2", rec["TotalSpin2"])
    assert np.abs(E - singlets).max() <= 1e-9 and np.abs(np.array(rec["TotalSpin2"])).max() < 1e-8


def test_with_density_matrix_noise(tmp_path):
    """-noise 1e-4,0 beside -spin_penalty 2 at m = 16: the perturbation is built from the operators of the Hamiltonian's terms, as many as
    without the penalty (the carried operators are not among them); the records keep their identities; after the clean second sweep the
    energy is variational and within the scale the truncation sets -- 10 x the largest truncation error of that sweep x |E|, the form
    test_gpu_engine.py uses between its pruned and unpruned runs."""
    common = [*HEIS_6x2, "-mwarmup", 16, "-nsweeps", 2, "-H_eps_tol", 1e-12, "-noise", "1e-4,0"]
    rows, run, _ = run_engine(tmp_path / "penalty", *common, "-spin_penalty", 2)
    _, run_plain, _ = run_engine(tmp_path / "plain", *common)
    assert run["NoiseExpansions"] > 0 and (run["NoiseOperatorsLeft"], run["NoiseOperatorsRight"]) == (run_plain["NoiseOperatorsLeft"], run_plain["NoiseOperatorsRight"])
    recs = _records(tmp_path / "penalty")
    _check_records(recs, rows, 1)
    for r in recs:
        assert r["RaisedNorm2"][0] >= 0.0 and r["TotalSpin2"][0] == r["RaisedNorm2"][0] and abs(r["Energy"][0] - (r["Eigenvalue"][0] - r["Lambda"] * r["RaisedNorm2"][0])) <= 1e-12
    e_ed = -10.105649318403
    clean = [r for r in rows if r["Noise"] == 0.0 and r["LoopIdx"] == rows[-1]["LoopIdx"]]
    trunc = max(r["TruncErr_Sys"] for r in clean)
    err = recs[-1]["Energy"][0] - e_ed
    print("after -noise 1e-4,0 under -spin_penalty 2: E - E_ED = %.3e, largest TruncErr_Sys of the clean sweep %.3e, RaisedNorm2 %.3e" % (err, trunc, recs[-1]["RaisedNorm2"][0]))
    assert len(clean) == N - 4 and trunc > 1e-10 and -1e-10 <= err <= 10.0 * trunc * abs(e_ed)


def test_restart_continues_a_penalised_run(tmp_path):
    """As test_gpu_engine.py::test_checkpoint_restart_continues_the_run, under -spin_penalty 1.5,0.75: one sweep + restart + one sweep is
    the two-sweep run bit for bit, in DMRGSteps.json and in SpinPenalty.json -- the carried operator comes back from SpTot_000000000.mat of
    every block, the restarted sweep takes the second weight."""
    model = [*J1J2_6x2, "-mwarmup", 24, "-H_eps_tol", 1e-12, "-wavefunction_guess", 0, "-spin_penalty", "1.5,0.75"]
    rows_a, run_a, _ = run_engine(tmp_path / "a", *model, "-nsweeps", 2)
    rows_b1, _, _ = run_engine(tmp_path / "b1", *model, "-nsweeps", 1, "-scratch_dir", str(tmp_path / "scratch1"))
    last = tmp_path / "scratch1" / "Sweep_000000001"
    for ib in range(6):
        assert (last / ("Sys_%09d" % ib) / "SpTot_000000000.mat").exists(), ib
    assert "-spin_penalty 1.5,0.75" in open(last / "PetscOptions.dat").read()
    rows_b2, run_b2, _ = run_engine(tmp_path / "b2", "-mwarmup", 24, "-H_eps_tol", 1e-12, "-nsweeps", 1, "-wavefunction_guess", 0, "-spin_penalty", "1.5,0.75",
                                    "-restart_dir", str(tmp_path / "scratch1"))
    n1 = len(rows_b1)
    assert rows_a[:n1] == rows_b1 and len(rows_b2) == len(rows_a) - n1 == N - 4
    assert rows_b2 == rows_a[n1:]
    rec_a, rec_b2 = _records(tmp_path / "a"), _records(tmp_path / "b2")
    assert rec_b2 == rec_a[n1:] and all(r["Lambda"] == 0.75 for r in rec_b2) and all(r["Lambda"] == 1.5 for r in rec_a[:n1] if r["LoopType"] == "Sweep")
    assert run_b2["GSEnergy"] == run_a["GSEnergy"]
    # a checkpoint written without the option has no carried operator to go on with
    run_engine(tmp_path / "c1", *J1J2_6x2, "-mwarmup", 24, "-scratch_dir", str(tmp_path / "scratch_plain"))
    with pytest.raises(AssertionError, match="needs a checkpoint that was written with it"):
        run_engine(tmp_path / "c2", "-mwarmup", 24, "-nsweeps", 1, "-spin_penalty", 1, "-restart_dir", str(tmp_path / "scratch_plain"))


def test_carried_operator_against_the_sum_over_sites(tmp_path):
    """4 x 2 Heisenberg, nothing truncated, -nstates 3 with a weight of 0.05 in the warm-up (the tower stays: singlet, triplet, triplet): at
    the warm-up's last step, a measurement step, |S+_tot psi|^2 from the two carried block operators equals the value that TotalSpin2 of
    TargetedStates.json takes from Sp of all eight sites, to 1e-12, state by state."""
    lv = ed.levels(J1J2XXZModel_SquareLattice(Lx=4, Ly=2, heisenberg=1.0), 0, 0.05)
    rows, _, _ = run_engine(tmp_path, "-Lx", 4, "-Ly", 2, "-heisenberg", 1, "-mwarmup", 64, "-H_eps_tol", 1e-13, "-nstates", 3, "-spin_penalty_warmup", 0.05)
    rec, trec = _records(tmp_path)[-1], _records(tmp_path, "TargetedStates.json")[-1]
    assert rec["GlobIdx"] == trec["GlobIdx"] == rows[-1]["GlobIdx"] and rec["LoopType"] == "Warmup" and rec["Lambda"] == 0.05
    assert rows[-1]["NSites_SysEnl"] + rows[-1]["NSites_EnvEnl"] == 8
    carried, sites = np.array(rec["TotalSpin2"]), np.array(trec["TotalSpin2"])
    print("TotalSpin2 carried", carried, "all sites", sites, "|diff|", np.abs(carried - sites), "ED", lv["spin2"][:3])
    assert len(carried) == 3 and np.abs(carried - sites).max() <= 1e-12
    assert np.abs(carried - lv["spin2"][:3]).max() <= 1e-8 and carried.max() > 1.9          # (a triplet is among them: the comparison is not 0 = 0)
    assert np.abs(np.array(rec["Eigenvalue"]) - lv["eigenvalue"][:3]).max() <= 1e-9
