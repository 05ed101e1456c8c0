"""-noise a0,a1,...: White's density-matrix perturbation in the sweep engine (-m gpu).  The 4 x 2 Heisenberg lattice, the smallest 2-D
lattice whose exact-diagonalisation energy the engine tests use: at m = 32 nothing is cut and the run must still end on the ED energy;
at m = 8 the cut truncates, and the option must reach it."""
import os
import subprocess

import pytest

from test_gpu_engine import ED, EXE, run_engine

pytestmark = pytest.mark.gpu
LATTICE, M_ED, E_ED = ED[0]
assert LATTICE == ["-Lx", 4, "-Ly", 2, "-heisenberg", 1]
SCHEDULE = [1e-4, 1e-6, 0.0]
M_CUT = 8


@pytest.fixture(scope="module")
def noisy_ed_run(tmp_path_factory):
    return run_engine(tmp_path_factory.mktemp("noise_ed"), *LATTICE, "-mwarmup", M_ED, "-nsweeps", 3, "-H_eps_tol", 1e-12, "-noise", "1e-4,1e-6,0")


@pytest.fixture(scope="module")
def cut_runs(tmp_path_factory):
    """At m = 8: without the option, with an all-zero schedule, with the schedule."""
    base = (*LATTICE, "-mwarmup", M_CUT, "-nsweeps", 3, "-H_eps_tol", 1e-12)
    return {name: run_engine(tmp_path_factory.mktemp("noise_" + name), *base, *extra)
            for name, extra in (("plain", ()), ("zeros", ("-noise", "0,0,0")), ("noisy", ("-noise", "1e-4,1e-6,0")))}


def test_noisy_schedule_ends_on_the_exact_energy(noisy_ed_run):
    """(a) the tolerance of test_ground_state_energy_matches_exact_diagonalisation; (b) noise changes the basis, never the variational
    property: no step lies below the ED energy."""
    rows, run, _ = noisy_ed_run
    nsites = rows[-1]["NSites_SysEnl"] + rows[-1]["NSites_EnvEnl"]
    full = [r["GSEnergy"] for r in rows if r["NSites_SysEnl"] + r["NSites_EnvEnl"] == nsites]
    print("noisy run: min E %.13f, ED %.13f, last step %.13f" % (min(full), E_ED, rows[-1]["GSEnergy"]))
    assert abs(min(full) - E_ED) <= 1e-10 * abs(E_ED)
    assert abs(rows[-1]["GSEnergy"] - E_ED) <= 1e-10 * abs(E_ED)          # and it ENDS there, after the noise-free sweep
    assert all(r["GSEnergy"] >= E_ED - 1e-10 for r in rows)
    assert len([r for r in rows if r["LoopType"] == "Sweep"]) == 3 * (nsites - 4)


def test_noise_column_follows_the_schedule(noisy_ed_run):
    """(c) DMRGSteps.json: 0 in the warm-up, then the value of the sweep; DMRGRun.json: the schedule as given and what it cost."""
    rows, run, _ = noisy_ed_run
    for r in rows:
        want = 0.0 if r["LoopType"] == "Warmup" else SCHEDULE[r["LoopIdx"] - 1]
        assert r["Noise"] == want, r
    assert {r["LoopIdx"] for r in rows if r["LoopType"] == "Sweep"} == {1, 2, 3}
    assert run["Noise"] == SCHEDULE and run["NoiseWarmup"] == 0.0
    assert run["NoiseExpansions"] > 0 and run["NoiseMaxExpansionBytes"] > 0 and run["NoiseOperatorsLeft"] > 0 and run["NoiseOperatorsRight"] > 0


def test_all_zero_schedule_is_the_run_without_the_option(cut_runs):
    """(d) compared exactly as read from the JSON."""
    plain, zeros = cut_runs["plain"][0], cut_runs["zeros"][0]
    assert len(plain) == len(zeros)
    for a, b in zip(plain, zeros):
        assert a == b
    assert all(r["Noise"] == 0.0 for r in plain)
    assert cut_runs["plain"][1]["Noise"] == [] and cut_runs["zeros"][1]["Noise"] == [0.0, 0.0, 0.0]
    assert cut_runs["plain"][1]["NoiseExpansions"] == 0 and cut_runs["zeros"][1]["NoiseExpansions"] == 0


def test_the_option_reaches_the_cut(cut_runs):
    """(e) at m = 8 the cut truncates, and in the noisy sweeps at least one step keeps another number of states or reports another
    truncation error than the run without noise -- while the steps of the warm-up, which no noise touched, are the same."""
    plain, noisy = cut_runs["plain"][0], cut_runs["noisy"][0]
    assert len(plain) == len(noisy)
    assert any(r["TruncErr_Sys"] > 1e-8 for r in plain if r["LoopType"] == "Sweep")            # the cut truncates
    keys = ("NStates_SysRot", "NStates_EnvRot", "TruncErr_Sys", "TruncErr_Env")
    for a, b in zip(plain, noisy):
        if a["LoopType"] == "Warmup":
            assert a == b
    differ = [a["GlobIdx"] for a, b in zip(plain, noisy) if b["Noise"] > 0 and any(a[k] != b[k] for k in keys)]
    print("steps whose cut differs under noise:", differ)
    assert differ
    e_ed = E_ED
    assert all(r["GSEnergy"] >= e_ed - 1e-10 for r in noisy)


def test_two_ranks_are_refused_at_start_up(tmp_path):
    """(f) the launcher of the two-rank refusals of the dynamical options."""
    d = str(tmp_path) + "/"
    cmd = [EXE, *[str(o) for o in LATTICE], "-mwarmup", "8", "-nsweeps", "1", "-noise", "1e-4", "-data_dir", d]
    name = "dmrgx_test_noise_%d" % os.getpid()
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
        assert "-noise is not available on more than one rank" in o, o[-2000:]
