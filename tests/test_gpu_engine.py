"""End-to-end parity (-m gpu): the C++ sweep engine on the MI355X (dmrg.x_amd/dmrgx-square-lattice, every
computation through the C ABI) against exact diagonalisation and against the CPU oracle's DMRG step by step."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from oracle.dmrg import DMRGOracle
from oracle.hamiltonian import J1J2XXZModel_SquareLattice
from helpers import lattice_ground_state, parse_desc2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dmrg.x_amd", "dmrgx-square-lattice")


def run_engine(tmp_path, *opts, ranks=1, timeout=600):
    """ranks > 1: that many engine processes share cuda:0 and talk through the host-staged communicator (DMRGX_COMM=shm) --
    the multi-GPU control flow (striped plan, native collectives inside the eigensolve, density matrices dealt over the
    ranks, broadcast rotations) rehearsed on the one-GPU test box; rank 0 writes the output files."""
    d = str(tmp_path) + "/"
    os.makedirs(d, exist_ok=True)
    cmd = [EXE, *[str(o) for o in opts], "-data_dir", d]
    if ranks == 1:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    else:
        name = "dmrgx_test_%d_%s" % (os.getpid(), os.path.basename(os.path.normpath(d)))
        procs = []
        for r in range(ranks):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(ranks), LOCAL_RANK="0", DMRGX_COMM="shm", DMRGX_SHM_NAME=name, DMRGX_SHM_MB="64")
            procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        outs = []
        try:
            for pr in procs:
                outs.append(pr.communicate(timeout=timeout)[0])
        finally:
            for pr in procs:
                if pr.poll() is None:
                    pr.kill()
        for r, (pr, o) in enumerate(zip(procs, outs)):
            assert pr.returncode == 0, "rank %d: %s" % (r, o[-3000:])
            open(d + "rank%d.log" % r, "w").write(o)
    steps = json.load(open(d + "DMRGSteps.json"))
    rows = [dict(zip(steps["headers"], r)) for r in steps["table"]]
    run = json.load(open(d + "DMRGRun.json"))
    timings = json.load(open(d + "Timings.json"))
    return rows, run, timings


ED = [  # SURVEY.md section 6 (independent exact diagonalisation in the Sz=0 sector)
    (["-Lx", 4, "-Ly", 2, "-heisenberg", 1], 32, -6.6682766346354),
    (["-Lx", 16, "-Ly", 1, "-heisenberg", 1], 64, -6.9117371455751),        # BASELINE config 1
    (["-Lx", 4, "-Ly", 4, "-heisenberg", 1], 128, -10.2642896209788),
    (["-Lx", 4, "-Ly", 4, "-J1", 1, "-Jz1", 1, "-J2", 0.5, "-Jz2", 0.5], 128, -13.8884952588612),
    (["-Lx", 4, "-Ly", 4], 128, -16.0335482295327),                          # defaults: NNN dropped (reference quirk)
]


@pytest.mark.parametrize("opts,m,e_ed", ED)
def test_ground_state_energy_matches_exact_diagonalisation(tmp_path, opts, m, e_ed):
    rows, run, _ = run_engine(tmp_path, *opts, "-mwarmup", m, "-nsweeps", 2, "-H_eps_tol", 1e-12)
    nsites = rows[-1]["NSites_SysEnl"] + rows[-1]["NSites_EnvEnl"]
    full = [r["GSEnergy"] for r in rows if r["NSites_SysEnl"] + r["NSites_EnvEnl"] == nsites]
    assert abs(min(full) - e_ed) <= 1e-10 * abs(e_ed)                     # north-star tolerance
    sweep_rows = [r for r in rows if r["LoopType"] == "Sweep"]
    assert len(sweep_rows) == 2 * (nsites - 4)                           # N-4 steps per sweep
    assert all(-1e-12 <= r["TruncErr_Sys"] < 1e-6 for r in rows)


def test_step_by_step_parity_with_oracle_under_truncation(tmp_path):
    """16x1 XXZ chain (Jz/J = 0.7/0.5), target sector Sz=1, m=4: a run with REAL truncation (TruncErr ~1e-3) in which
    every m-cut falls into a spectral gap.  Every step's sizes, ground-state energy and truncation error are compared
    with the CPU restatement of the reference algorithm at the north-star tolerance (1e-10 relative).

    Why this case: parity of the kept subspace is only defined when the cut is non-degenerate.  In the Sz=0 sector of a
    spin-flip symmetric model the +q/-q RDM spectra are exactly degenerate, and with larger m the early steps keep
    numerically-zero eigenvalues of rank-deficient RDMs -- in both situations the surviving states are picked by
    rounding noise in ANY implementation (the reference's LAPACK path included).  The oracle
    records the eigenvalues on both sides of every cut and the test first asserts that the case is well-defined."""
    H = J1J2XXZModel_SquareLattice(Lx=16, Ly=1, heisenberg=0.7)
    orc = DMRGOracle(H, 4, qn_sector=1.0)
    orc.Warmup()
    orc.Sweeps(nsweeps=2)
    for o in orc.steps:
        for lam_kept, lam_dropped in (o["cut_Sys"], o["cut_Env"]):
            assert lam_kept > 1e-6 and (lam_dropped == 0.0 or (lam_kept - lam_dropped) / lam_kept > 1e-2), "parity case is not well-defined"
    rows, run, timings = run_engine(tmp_path, "-Lx", 16, "-Ly", 1, "-heisenberg", 0.7, "-qn_sector", 1, "-mwarmup", 4, "-nsweeps", 2, "-H_eps_tol", 1e-13)
    assert len(rows) == len(orc.steps) == 6 + 2 * 12
    for r, o in zip(rows, orc.steps):
        for key in ("NSites_Sys", "NSites_Env", "NStates_SysEnl", "NStates_EnvEnl", "NumStates_H", "NStates_SysRot", "NStates_EnvRot"):
            assert r[key] == o[key], (r["GlobIdx"], key)
        assert abs(r["GSEnergy"] - o["GSEnergy"]) <= 1e-10 * abs(o["GSEnergy"]), r["GlobIdx"]
        # TruncErr = 1 - (sum of kept eigenvalues) is first-order sensitive to the ground-state vector: the engine's Lanczos
        # stops at ||r|| <= 1e-13 |E| while the oracle diagonalises densely, so |d psi| ~ 1e-12 moves TruncErr by
        # ~ |d psi| sqrt(TruncErr) ~ 1e-13 in absolute terms, on top of the 1e-10 relative bar
        for side in ("TruncErr_Sys", "TruncErr_Env"):
            assert abs(r[side] - o[side]) <= 1e-10 * abs(o[side]) + 1e-13, (r["GlobIdx"], side, r[side], o[side])
    assert max(o["TruncErr_Sys"] for o in orc.steps) > 1e-4               # the truncation was real
    # Timings.json: the reference's seven columns first (include/DMRGBlockContainer.hpp:2568-2583), the engine's own after them
    assert run["MatMults"] > 0 and timings["headers"] == ["GlobIdx", "Total", "Enlr", "Kron", "Diag", "Rdms", "Rotb", "MatMults", "RotOps", "AllGatherMs", "ApplyMs"]
    assert all(len(r) == len(timings["headers"]) for r in timings["table"])
    # correlators: same measurement steps, same values as the oracle's restatement
    corr = json.load(open(str(tmp_path) + "/Correlations.json"))
    orc2 = DMRGOracle(H, 4, qn_sector=1.0)
    for c in corr["info"]:
        orc2.SetUpCorrelation(parse_desc2(c["desc2"]))
    orc2.Warmup()
    orc2.Sweeps(nsweeps=2)
    assert len(corr["values"]) == len(orc2.corr_values) == 3              # end of warm-up + one per sweep
    nonzero = 0
    for got, want in zip(corr["values"], orc2.corr_values):
        assert len(got) == len(want) == len(corr["info"])
        for c, g, w in zip(corr["info"], got, want):
            assert abs(g - w) <= 1e-10 * max(abs(w), 1e-2), (c["name"], g, w)
            nonzero += abs(w) > 1e-3
    assert nonzero > 20                                                    # Sz = 1 sector: magnetisations do not vanish


TRUNCATING_2D = [
    # (Lx, Ly, J1, Jz1, J2, Jz2, Sz sector): J1-J2 lattices with next-nearest-neighbour terms, every one truncating hard at m = 4
    # (TruncErr 1e-4 .. 1e-1) with every m-cut inside a spectral gap (scanned with the oracle; asserted below)
    (6, 2, 0.7, 1.0, 0.4, 0.6, 1),      # Ly = 2: periodic-y doubles the vertical and the diagonal bonds
    (8, 2, 0.7, 1.0, 0.4, 0.6, 1),
    (4, 4, 1.0, 1.0, 0.5, 0.5, 1),      # BASELINE's couplings (J2 = Jz2 = 0.5), mid-column cuts of a width-4 cylinder
    (6, 4, 1.0, 0.8, 0.5, 0.3, 1),      # 24 sites, 48 steps
]


@pytest.mark.parametrize("ranks", [1, 2])
@pytest.mark.parametrize("Lx,Ly,J1,Jz1,J2,Jz2,sz", TRUNCATING_2D)
def test_step_by_step_parity_with_oracle_under_truncation_2d(tmp_path, Lx, Ly, J1, Jz1, J2, Jz2, sz, ranks):
    """The step-by-step comparison of the chain test on two-dimensional J1-J2 lattices where the m-cut bites: NNN terms,
    the doubled bonds of Ly = 2, cuts in the middle of a column (one side holds fewer distinct operators than the other,
    which flips the plan's operator-merge direction), the operator pruning of the sweep schedule.  Per step: sizes,
    ground-state energy and both truncation errors at 1e-10 relative against the CPU restatement of the reference
    (include/DMRGBlockContainer.hpp:1656-1959, src/Hamiltonians.cpp:93-112); then every correlator row."""
    H = J1J2XXZModel_SquareLattice(Lx=Lx, Ly=Ly, J1=J1, Jz1=Jz1, J2=J2, Jz2=Jz2)
    m = 4
    if ranks > 1 and Lx * Ly > 16:
        pytest.skip("the two-rank rehearsal runs the two smaller lattices")
    rows, run, _ = run_engine(tmp_path, "-Lx", Lx, "-Ly", Ly, "-J1", J1, "-Jz1", Jz1, "-J2", J2, "-Jz2", Jz2, "-qn_sector", sz, "-mwarmup", m,
                              "-nsweeps", 2, "-H_eps_tol", 1e-13, ranks=ranks)
    corr = json.load(open(str(tmp_path) + "/Correlations.json"))
    orc = DMRGOracle(H, m, qn_sector=float(sz))
    for c in corr["info"]:
        orc.SetUpCorrelation(parse_desc2(c["desc2"]))
    orc.Warmup()
    orc.Sweeps(nsweeps=2)
    for o in orc.steps:
        for lam_kept, lam_dropped in (o["cut_Sys"], o["cut_Env"]):
            assert lam_kept > 1e-9 and (lam_dropped == 0.0 or (lam_kept - lam_dropped) / lam_kept > 1e-2), "parity case is not well-defined"
    assert any(t.Isite != t.Jsite and abs(t.a) in (J2, Jz2) for t in H.H(Lx * Ly))        # the NNN terms are there
    assert len(rows) == len(orc.steps)
    for r, o in zip(rows, orc.steps):
        for key in ("NSites_Sys", "NSites_Env", "NStates_SysEnl", "NStates_EnvEnl", "NumStates_H", "NStates_SysRot", "NStates_EnvRot"):
            assert r[key] == o[key], (r["GlobIdx"], key)
        assert abs(r["GSEnergy"] - o["GSEnergy"]) <= 1e-10 * abs(o["GSEnergy"]), (r["GlobIdx"], r["GSEnergy"], o["GSEnergy"])
        for side in ("TruncErr_Sys", "TruncErr_Env"):      # same absolute slack as the chain test (Lanczos residual 1e-13 vs dense eigh)
            assert abs(r[side] - o[side]) <= 1e-10 * abs(o[side]) + 1e-13, (r["GlobIdx"], side, r[side], o[side])
    assert max(o["TruncErr_Sys"] for o in orc.steps) > 5e-5
    assert len(corr["values"]) == len(orc.corr_values) == 3
    nonzero = 0
    for got, want in zip(corr["values"], orc.corr_values):
        assert len(got) == len(want) == len(corr["info"])
        for c, g, w in zip(corr["info"], got, want):
            assert abs(g - w) <= 1e-10 * max(abs(w), 1e-2), (c["name"], g, w)
            nonzero += abs(w) > 1e-3
    assert nonzero > 20


def _big_golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "engine_big_lattices.json")))


@pytest.mark.parametrize("name,ranks", [("cfg4_j1j2_20x8", 1), ("cfg4_j1j2_20x8", 2), ("cfg3_heisenberg_16x6", 1), ("cfg5_xy_32x8", 1)])
def test_headline_lattices_step_by_step_against_the_oracle(tmp_path, name, ranks):
    """The geometries BASELINE's numbers are quoted on -- J1-J2 20x8 (configs[3]; also on two ranks), Heisenberg 16x6 (configs[2]),
    XY 32x8 with the NNN bonds dropped at Jz2 = 0 (configs[4]) -- at reduced m, step by step against the CPU oracle's DMRG
    (tests/golden/engine_big_lattices.json, generated by tests/golden/make_engine_golden.py from oracle/dmrg.py: minutes of
    single-threaded Python per lattice).  Up to and including the first step whose m-cut is ill-defined (degenerate or round-off
    eigenvalues at the cut: the kept subspace is then decided by rounding noise in any implementation) the superblock sizes and
    the ground-state energy must agree at 1e-10 relative, and before it the truncation errors and the rotated sizes too; after
    it, energies agree at the scale of the truncation error.  Match: src/Hamiltonians.cpp:70-122 (74-, 20- and 18-term cuts of
    the width-8 / width-6 cylinders), src/DMRGKron.cpp:1842-1864, include/DMRGBlockContainer.hpp:1656-1959."""
    g = _big_golden()[name]
    o = g["options"]
    rows, run, _ = run_engine(tmp_path, "-Lx", o["Lx"], "-Ly", o["Ly"], "-J1", o["J1"], "-Jz1", o["Jz1"], "-J2", o["J2"], "-Jz2", o["Jz2"], "-qn_sector", g["qn_sector"],
                              "-mwarmup", g["m"], "-nsweeps", g["nsweeps"], "-H_eps_tol", 1e-13, ranks=ranks)
    steps = g["steps"]
    assert len(rows) == len(steps) and run["Ranks"] == ranks
    first_ill = next((i for i, st in enumerate(steps) if not st["well_defined"]), len(steps))
    assert first_ill >= 2                                                     # the strict part is not empty
    trunc = max(st["TruncErr_Sys"] for st in steps)
    for i, (r, st) in enumerate(zip(rows, steps)):
        for key in ("NSites_Sys", "NSites_Env"):
            assert r[key] == st[key], (i, key)
        if i <= first_ill:
            for key in ("NStates_SysEnl", "NStates_EnvEnl", "NumStates_H"):
                assert r[key] == st[key], (i, key)
            assert abs(r["GSEnergy"] - st["GSEnergy"]) <= 1e-10 * abs(st["GSEnergy"]), (i, r["GSEnergy"], st["GSEnergy"])
        else:
            assert abs(r["GSEnergy"] - st["GSEnergy"]) <= 4.0 * trunc * abs(st["GSEnergy"]), (i, r["GSEnergy"], st["GSEnergy"])
        if i < first_ill:
            for key in ("NStates_SysRot", "NStates_EnvRot"):
                assert r[key] == st[key], (i, key)
            for side in ("TruncErr_Sys", "TruncErr_Env"):
                assert abs(r[side] - st[side]) <= 1e-10 * abs(st[side]) + 1e-13, (i, side, r[side], st[side])
    assert trunc > 1e-4                                                       # the truncation was real


def test_unsupported_reference_options_are_refused(tmp_path):
    """Options of the reference's driver that select code this engine does not build are refused with PETSC_ERR_SUP (56), not
    accepted and ignored: -no_symm (include/DMRGBlockContainer.hpp:243 of the reference refuses it too) and -do_shell 0 (the explicit
    MATMPIAIJ superblock Hamiltonian, src/DMRGKron.cpp:759-841)."""
    for opt in (["-do_shell", 0], ["-no_symm", 1]):
        d = str(tmp_path / opt[0].strip("-")) + "/"
        os.makedirs(d, exist_ok=True)
        out = subprocess.run([EXE, *[str(o) for o in ("-Lx", 4, "-Ly", 2, "-mwarmup", 8, "-nsweeps", 1, *opt, "-data_dir", d)]], capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and "Unsupported option" in (out.stdout + out.stderr), out.stdout[-500:] + out.stderr[-500:]


def test_rdm_warm_start_option_gives_the_same_run(tmp_path):
    """-rdm_warm_start is still a recognised option and does nothing (neither density-matrix solver reads a starting basis; the engine
    says so at start-up): energies and truncation errors of a warm-up + two sweeps equal the run without it."""
    model = ["-Lx", 6, "-Ly", 2, "-J1", 1, "-Jz1", 0.9, "-J2", 0.5, "-Jz2", 0.4, "-qn_sector", 1, "-mwarmup", 12, "-nsweeps", 2, "-H_eps_tol", 1e-12]
    r0, _, _ = run_engine(tmp_path / "cold", *model, "-rdm_warm_start", 0)
    r1, _, _ = run_engine(tmp_path / "warm", *model, "-rdm_warm_start", 1)
    assert len(r0) == len(r1) >= 20
    for a, b in zip(r0, r1):
        assert abs(a["GSEnergy"] - b["GSEnergy"]) <= 1e-10 * abs(a["GSEnergy"]), (a["GlobIdx"], a["GSEnergy"], b["GSEnergy"])
        assert abs(a["TruncErr_Sys"] - b["TruncErr_Sys"]) <= 1e-9 * abs(a["TruncErr_Sys"]) + 1e-13


def _medium_golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "engine_medium_m.json")))


@pytest.mark.parametrize("name,ranks,extra", [("j1j2_10x4_sz1", 1, ()), ("j1j2_8x4_sz1", 1, ()), ("j1j2_8x4_sz1", 2, ()), ("xxz_8x6_sz1", 1, ()), ("j1j2_6x4_sz1", 1, ()),
                                              ("j1j2_6x4_sz1", 3, ()), ("j1j2_6x4_sz1", 1, ("-rdm_warm_start", 1)), ("j1j2_6x4_sz1", 1, ("-H_eps_type", "gd")),
                                              ("j1j2_10x4_sz1", 1, ("-H_eps_type", "gd")), ("j1j2_8x4_sz1", 2, ("-H_eps_type", "gd")), ("xxz_8x6_sz1", 2, ())])
def test_medium_m_step_by_step_against_the_oracle(tmp_path, name, ranks, extra):
    """The engine against the CPU oracle's DMRG step by step at m = 24 ... 48, where the code paths of the production sizes run inside
    the engine: enlarged sectors of 20-35 states are diagonalised by divide and conquer with real merges and deflation
    (csrc/symeig.hip, leaves of 16), back-transformed through WY blocks, and every GEMM tile spans several 16 x 16 MFMA blocks
    (the m = 4-8 cases above never leave one leaf / one block).  tests/golden/engine_medium_m.json is made by
    tests/golden/make_engine_golden_medium_m.py (minutes of single-threaded Python per lattice); its docstring says why the runs warm
    up small, grow m sweep by sweep and turn round `-min_block` sites before the edge: only then is every m-cut decided by the spectrum
    and not by round-off.  Up to the first ill-defined cut -- 70-180 steps into a run, in its last sweep -- sizes, energies and both
    truncation errors agree at 1e-10; across the four runs that is more than 150 steps at m >= 24.  After it, energies agree at the
    truncation-error scale.  The smallest run is repeated on three ranks (density matrices dealt over the ranks, striped solve), with
    -rdm_warm_start 1 (an option that no longer does anything) and with the generalized-Davidson solver type.  Match: include/DMRGBlockContainer.hpp:1656-2057, src/DMRGBlock.cpp:766-771."""
    g = _medium_golden()[name]
    o = g["options"]
    rows, run, _ = run_engine(tmp_path, "-Lx", o["Lx"], "-Ly", o["Ly"], "-J1", o["J1"], "-Jz1", o["Jz1"], "-J2", o["J2"], "-Jz2", o["Jz2"], "-qn_sector", g["qn_sector"],
                              "-mwarmup", g["mwarmup"], "-msweeps", ",".join(str(m) for m in g["msweeps"]), "-min_block", g["min_block"], "-H_eps_tol", 1e-13, *extra, ranks=ranks)
    steps = g["steps"]
    assert len(rows) == len(steps) and run["Ranks"] == ranks
    first_ill = next((i for i, st in enumerate(steps) if not st["well_defined"]), len(steps))
    assert first_ill == g["first_ill"] and g["strict_steps_m24"] >= 20
    assert max(st["max_sector"] for st in steps[:first_ill]) > 16                 # merges of the divide-and-conquer tree happen in the strict part
    trunc = max(st["TruncErr_Sys"] for st in steps)
    for i, (r, st) in enumerate(zip(rows, steps)):
        for key in ("NSites_Sys", "NSites_Env"):
            assert r[key] == st[key], (i, key)
        if i <= first_ill:
            for key in ("NStates_SysEnl", "NStates_EnvEnl", "NumStates_H"):
                assert r[key] == st[key], (i, key)
            assert abs(r["GSEnergy"] - st["GSEnergy"]) <= 1e-10 * abs(st["GSEnergy"]), (i, st["m"], r["GSEnergy"], st["GSEnergy"])
        else:
            assert abs(r["GSEnergy"] - st["GSEnergy"]) <= 4.0 * trunc * abs(st["GSEnergy"]), (i, r["GSEnergy"], st["GSEnergy"])
        if i < first_ill:
            for key in ("NStates_SysRot", "NStates_EnvRot"):
                assert r[key] == st[key], (i, key)
            for side in ("TruncErr_Sys", "TruncErr_Env"):
                assert abs(r[side] - st[side]) <= 1e-10 * abs(st[side]) + 1e-13, (i, st["m"], side, r[side], st[side])


@pytest.mark.parametrize("ranks,extra", [(1, ()), (1, ("-H_eps_type", "gd")), (2, ())])
def test_large_m_step_by_step_against_the_oracle(tmp_path, ranks, extra):
    """The engine against the CPU oracle step by step where the PRODUCTION paths of the density-matrix solver run inside a sweep (VERDICT
    round 4, item 4): J1-J2 4 x 8 cylinder, Sz = 1, m grown to 480 -- enlarged sectors of up to 260 states (the rows of one matrix dealt
    over several workgroups of the persistent tridiagonalisation, >= 3 divide-and-conquer merge levels, several compact-WY blocks; all
    asserted from DMRGRun.json, which carries dmrgx_rdm_info's report) and superblocks of up to 1.8 x 10^5 states (thousands of GEMM tiles per
    MatMult).  tests/golden/engine_large_m.json is made by tests/golden/make_engine_golden_large_m.py, whose docstring says why the
    lattice is 4 x 8 with `-min_block` 8, why every m is even and why "well-defined cut" is an absolute gap here.  Every step whose cuts
    are well-defined -- all 176 are, the 42 steps of the sweeps at m = 252, 366 and 480 among them -- must agree at 1e-10 in sizes, energy and both truncation
    errors.  One rank (both solver types) and two ranks (density matrices dealt over the ranks; the host-staged rehearsal back-end uses one
    launch per column instead of the persistent kernel).  Match: include/DMRGBlockContainer.hpp:1656-2057, src/DMRGBlock.cpp:766-771."""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "engine_large_m.json")))["j1j2_4x8_sz1_large_m"]
    o = g["options"]
    rows, run, _ = run_engine(tmp_path, "-Lx", o["Lx"], "-Ly", o["Ly"], "-J1", o["J1"], "-Jz1", o["Jz1"], "-J2", o["J2"], "-Jz2", o["Jz2"], "-qn_sector", g["qn_sector"],
                              "-mwarmup", g["mwarmup"], "-msweeps", ",".join(str(m) for m in g["msweeps"]), "-min_block", g["min_block"], "-H_eps_tol", 1e-13, *extra, ranks=ranks,
                              timeout=900)
    steps = g["steps"]
    assert len(rows) == len(steps) and run["Ranks"] == ranks
    first_ill = g["first_ill"]
    strict_large = [st for st in steps[:first_ill] if st["m"] >= 250]
    assert len(strict_large) >= 20 and max(st["max_sector"] for st in strict_large) >= 150 and max(st["NumStates_H"] for st in strict_large) >= 100000
    trunc = max(st["TruncErr_Sys"] for st in steps)
    for i, (r, st) in enumerate(zip(rows, steps)):
        for key in ("NSites_Sys", "NSites_Env"):
            assert r[key] == st[key], (i, key)
        if i <= first_ill:
            for key in ("NStates_SysEnl", "NStates_EnvEnl", "NumStates_H"):
                assert r[key] == st[key], (i, key)
            assert abs(r["GSEnergy"] - st["GSEnergy"]) <= 1e-10 * abs(st["GSEnergy"]), (i, st["m"], r["GSEnergy"], st["GSEnergy"])
        else:
            assert abs(r["GSEnergy"] - st["GSEnergy"]) <= 4.0 * trunc * abs(st["GSEnergy"]), (i, r["GSEnergy"], st["GSEnergy"])
        if i < first_ill:
            for key in ("NStates_SysRot", "NStates_EnvRot"):
                assert r[key] == st[key], (i, key)
            for side in ("TruncErr_Sys", "TruncErr_Env"):
                assert abs(r[side] - st[side]) <= 1e-10 * abs(st[side]) + 1e-13, (i, st["m"], side, r[side], st[side])
    # the code paths this run is for did run (dmrgx_rdm_info -> DMRGRun.json)
    assert run["RdmBlockJacobiCalls"] == 0 and run["TridFallbacks"] == 0 and run["RdmMaxMergeLevels"] >= 3 and run["RdmMaxWyBlocks"] >= 2, run
    if ranks == 1:
        assert run["TridPersistentCalls"] == run["RdmCalls"] and run["TridLaunchPathCalls"] == 0 and run["TridMaxWorkgroupsPerMatrix"] >= 2, run
    else:
        assert run["TridLaunchPathCalls"] == run["RdmCalls"] and run["TridPersistentCalls"] == 0, run      # (ranks sharing one GPU: no persistent kernel)


def _assert_run_is_finite(tmp_path):
    """Every number of DMRGRun.json is finite (no NaN / Infinity constant, no non-finite float)."""
    bad = []
    run = json.load(open(os.path.join(str(tmp_path), "DMRGRun.json")), parse_constant=lambda c: bad.append(c) or 0.0)

    def walk(v):
        if isinstance(v, dict):
            for x in v.values():
                walk(x)
        elif isinstance(v, list):
            for x in v:
                walk(x)
        elif isinstance(v, float) and not np.isfinite(v):
            bad.append(v)
    walk(run)
    assert not bad, bad


@pytest.mark.parametrize("ranks", [1, 2])
def test_medium_m_step_by_step_on_poisoned_workspaces(tmp_path, monkeypatch, ranks):
    """The step-by-step comparison with the oracle with every f64 workspace of the engine processes NaN-poisoned (DMRGX_POOL_POISON=1:
    csrc/pool.hip), so that a kernel reading a location nobody wrote shows as a wrong or non-finite step instead of a lucky zero."""
    monkeypatch.setenv("DMRGX_POOL_POISON", "1")
    test_medium_m_step_by_step_against_the_oracle(tmp_path, "j1j2_8x4_sz1", ranks, ())
    _assert_run_is_finite(tmp_path)


def test_large_m_step_by_step_on_poisoned_workspaces(tmp_path, monkeypatch):
    """The production-size density-matrix paths and the generalized-Davidson solver inside a sweep, on poisoned workspaces."""
    monkeypatch.setenv("DMRGX_POOL_POISON", "1")
    test_large_m_step_by_step_against_the_oracle(tmp_path, 1, ("-H_eps_type", "gd"))
    _assert_run_is_finite(tmp_path)


def test_medium_m_tables_cover_the_sizes_they_are_for():
    """(no GPU needed, but kept beside its test) >= 100 strictly compared steps at m >= 24, one run with sectors above 32"""
    g = _medium_golden()
    assert sum(c["strict_steps_m24"] for c in g.values()) >= 100
    assert max(st["max_sector"] for c in g.values() for st in c["steps"][:c["first_ill"]]) > 32


def test_baseline_config1_energy_against_the_oracle_at_reduced_m(tmp_path):
    """BASELINE configs[1] (J1-J2 8x4 cylinder, J2 = 0.5) is too large for exact diagonalisation and, at m = 512, for the CPU
    oracle.  In the Sz = 0 sector the +q/-q spectra are degenerate, so the kept subspaces of two implementations may differ by
    the states at the cut and energies agree only at the truncation-error level: the engine at m = 48
    must reproduce the oracle's m = 48 energy within 2 x (largest truncation error) x |E|, and the energy bench.py quotes at
    m = 512 must lie below both and within the same scale of them (DMRG is variational in m)."""
    H = J1J2XXZModel_SquareLattice(Lx=8, Ly=4, J1=1.0, Jz1=1.0, J2=0.5, Jz2=0.5)
    orc = DMRGOracle(H, 48)
    orc.Warmup()
    orc.Sweeps(nsweeps=1)
    trunc = max(o["TruncErr_Sys"] for o in orc.steps)
    assert 1e-7 < trunc < 1e-4
    model = ["-Lx", 8, "-Ly", 4, "-J1", 1, "-Jz1", 1, "-J2", 0.5, "-Jz2", 0.5, "-nsweeps", 1, "-H_eps_tol", 1e-12]
    _, run48, _ = run_engine(tmp_path / "m48", *model, "-mwarmup", 48)
    _, run512, _ = run_engine(tmp_path / "m512", *model, "-mwarmup", 512)
    e_o, e48, e512 = orc.gse, run48["GSEnergy"], run512["GSEnergy"]
    assert abs(e48 - e_o) <= 2.0 * trunc * abs(e_o), (e48, e_o, trunc)
    assert e512 < min(e48, e_o) and min(e48, e_o) - e512 <= 20.0 * trunc * abs(e_o), (e512, e48, e_o)
    assert abs(e512 - (-27.92734251200497)) <= 1e-7 * abs(e512)          # the value bench.py's sweep leg printed in round 1


def test_multi_rank_engine_sweep_reproduces_the_single_rank_run(tmp_path):
    """A whole engine run on 3 ranks (striped Hamiltonian plan, RDMs dealt by n^3, rotations from broadcast eigenvectors) against
    the same run on one rank, J1-J2 6x4 at m = 40 in the Sz = 1 sector: the first step at 1e-10 relative, every later energy
    within the scale of the truncation error (at m = 40 the early warm-up steps and the edge steps of a sweep keep
    numerically-zero states of rank-deficient density matrices, whose choice -- made by rounding noise, here by the summation
    order of the reductions -- changes sector tables and shifts later energies at the truncation-error level in any
    implementation; the m = 4 parity cases above have no such steps and agree with the oracle to 1e-10 on two ranks as well)."""
    model = ["-Lx", 6, "-Ly", 4, "-J1", 1, "-Jz1", 0.8, "-J2", 0.5, "-Jz2", 0.3, "-qn_sector", 1, "-mwarmup", 40, "-nsweeps", 1, "-H_eps_tol", 1e-12]
    r1, run1, _ = run_engine(tmp_path / "w1", *model)
    r3, run3, _ = run_engine(tmp_path / "w3", *model, ranks=3)
    assert len(r1) == len(r3) == 8 + 20
    trunc = max(max(r["TruncErr_Sys"] for r in r1), 1e-12)
    for a, b in zip(r1, r3):
        if a["GlobIdx"] == 0:        # exact input blocks: the first superblock is the same problem on any number of ranks
            assert a["NumStates_H"] == b["NumStates_H"] and abs(a["GSEnergy"] - b["GSEnergy"]) <= 1e-10 * abs(a["GSEnergy"]), a["GlobIdx"]
        assert abs(a["GSEnergy"] - b["GSEnergy"]) <= 10.0 * trunc * abs(a["GSEnergy"]), (a["GlobIdx"], a["GSEnergy"], b["GSEnergy"])
    assert abs(run1["GSEnergy"] - run3["GSEnergy"]) <= 10.0 * trunc * abs(run1["GSEnergy"])
    c1, c3 = (json.load(open(str(tmp_path / d) + "/Correlations.json")) for d in ("w1", "w3"))
    assert len(c1["values"]) == len(c3["values"]) == 2


def test_correlators_dealt_over_the_ranks_carry_fewer_operators(tmp_path):
    """On W ranks every rank measures only its share of the correlators (values summed at the measurement), so on the way back to
    the centre a rank rotates only the site operators ITS correlators read: the per-step operator counts of rank 0 (Timings.json,
    column RotOps) drop against the one-rank run while Correlations.json stays the same table."""
    # (a long, narrow lattice: most sites of a block are correlator-only there; on 6x4 nearly every site is a coupling site)
    model = ["-Lx", 24, "-Ly", 2, "-J1", 0.7, "-Jz1", 1.0, "-J2", 0.4, "-Jz2", 0.6, "-qn_sector", 1, "-mwarmup", 4, "-nsweeps", 1, "-H_eps_tol", 1e-13]
    _, _, t1 = run_engine(tmp_path / "w1", *model)
    _, _, t3 = run_engine(tmp_path / "w3", *model, ranks=3)
    c1, c3 = (json.load(open(str(tmp_path / d) + "/Correlations.json")) for d in ("w1", "w3"))
    assert len(c1["values"]) == len(c3["values"]) == 2
    for a, b in zip(c1["values"], c3["values"]):
        assert np.abs(np.array(a) - np.array(b)).max() <= 1e-8      # (truncating run: the three-rank reductions sum in another order)
    col = t1["headers"].index("RotOps")
    r1, r3 = [row[col] for row in t1["table"]], [row[col] for row in t3["table"]]
    assert len(r1) == len(r3) and all(b <= a for a, b in zip(r1, r3))
    nsweep = 48 - 4
    one = sum(r1[-nsweep:])
    per_rank = [int(re.search(r"\[rank %d\] SWEEP rotated operators = (\d+)" % r, open(str(tmp_path / "w3") + "/rank%d.log" % r).read()).group(1)) for r in range(3)]
    assert per_rank[0] == sum(r3[-nsweep:])
    # the way out of the centre (left-only masks) is the same on every rank; of the way back each rank carries its run of sites
    assert max(per_rank) < 0.8 * one, (one, per_rank)


def test_engine_with_generalized_davidson_solver(tmp_path):
    """-H_eps_type gd (the option name SLEPc users of the reference have): ED energy of the 4x4 J1-J2 lattice and the oracle's
    per-step energies of a well-defined truncating 2-D case at the north-star tolerance, on one rank and on two."""
    rows, run, _ = run_engine(tmp_path / "ed", "-Lx", 4, "-Ly", 4, "-J1", 1, "-Jz1", 1, "-J2", 0.5, "-Jz2", 0.5, "-mwarmup", 128, "-nsweeps", 2,
                              "-H_eps_tol", 1e-12, "-H_eps_type", "gd")
    assert abs(min(r["GSEnergy"] for r in rows if r["NSites_SysEnl"] + r["NSites_EnvEnl"] == 16) - (-13.8884952588612)) <= 1e-10 * 13.89
    H = J1J2XXZModel_SquareLattice(Lx=6, Ly=2, J1=0.7, Jz1=1.0, J2=0.4, Jz2=0.6)
    orc = DMRGOracle(H, 4, qn_sector=1.0)
    orc.Warmup()
    orc.Sweeps(nsweeps=2)
    for ranks in (1, 2):
        rows, _, _ = run_engine(tmp_path / ("gd%d" % ranks), "-Lx", 6, "-Ly", 2, "-J1", 0.7, "-Jz1", 1.0, "-J2", 0.4, "-Jz2", 0.6, "-qn_sector", 1,
                                "-mwarmup", 4, "-nsweeps", 2, "-H_eps_tol", 1e-13, "-H_eps_type", "gd", ranks=ranks)
        assert len(rows) == len(orc.steps)
        for r, o in zip(rows, orc.steps):
            assert r["NumStates_H"] == o["NumStates_H"] and abs(r["GSEnergy"] - o["GSEnergy"]) <= 1e-10 * abs(o["GSEnergy"]), r["GlobIdx"]
            assert abs(r["TruncErr_Sys"] - o["TruncErr_Sys"]) <= 1e-10 * abs(o["TruncErr_Sys"]) + 1e-13


def test_pruned_and_unpruned_operator_sets_agree(tmp_path):
    """-prune_ops 0 rotates and keeps every Sz(i)/Sp(i) of every block and diagonalises both density matrices of every KronBlock,
    as the reference does; the default keeps the sites a later inter-block term or a registered correlator can touch, does not
    rotate the blocks no later step reads and takes their spectrum from the other side of the KronBlock.  On a parity case with
    well-defined cuts (4x4 J1-J2, Sz = 1, m = 4; pinned to the oracle above in the default mode) every step agrees at the
    north-star tolerance; on a larger run (6x4, m = 48, where edge steps keep numerically-zero states picked by rounding noise)
    energies agree at the truncation-error scale and the rotation work drops."""
    small = ["-Lx", 4, "-Ly", 4, "-J1", 1, "-Jz1", 1, "-J2", 0.5, "-Jz2", 0.5, "-qn_sector", 1, "-mwarmup", 4, "-nsweeps", 2, "-H_eps_tol", 1e-13]
    ra, _, _ = run_engine(tmp_path / "a", *small)
    rb, _, _ = run_engine(tmp_path / "b", *small, "-prune_ops", 0)
    assert len(ra) == len(rb) == 4 + 2 * 12
    for a, b in zip(ra, rb):
        assert {k: v for k, v in a.items() if k not in ("TruncErr_Sys", "TruncErr_Env", "GSEnergy")} == {k: v for k, v in b.items() if k not in ("TruncErr_Sys", "TruncErr_Env", "GSEnergy")}
        assert abs(a["GSEnergy"] - b["GSEnergy"]) <= 1e-10 * abs(b["GSEnergy"])
        for k in ("TruncErr_Sys", "TruncErr_Env"):
            assert abs(a[k] - b[k]) <= 1e-10 * abs(b[k]) + 1e-13, (a["GlobIdx"], k, a[k], b[k])
    ca, cb = (json.load(open(str(tmp_path / d) + "/Correlations.json")) for d in ("a", "b"))
    assert np.abs(np.array(ca["values"]) - np.array(cb["values"])).max() <= 1e-10
    model = ["-Lx", 6, "-Ly", 4, "-J1", 1, "-Jz1", 1, "-J2", 0.5, "-Jz2", 0.5, "-mwarmup", 48, "-nsweeps", 2]
    rc, _, tc = run_engine(tmp_path / "c", *model)
    rd, _, td = run_engine(tmp_path / "d", *model, "-prune_ops", 0)
    assert len(rc) == len(rd) == 8 + 2 * 20
    trunc = max(r["TruncErr_Sys"] for r in rd)
    assert trunc > 1e-8
    for a, b in zip(rc, rd):
        assert abs(a["GSEnergy"] - b["GSEnergy"]) <= 10.0 * trunc * abs(b["GSEnergy"]), (a["GlobIdx"], a["GSEnergy"], b["GSEnergy"])


def test_correlators_match_exact_diagonalisation(tmp_path):
    """Every correlator the driver registers (magnetisations, the three bond correlators of every nearest-neighbour
    pair, the Sz strings) on the 4x2 Heisenberg lattice against dense ED of the lattice: m = 64 keeps everything, so
    the values are exact ground-state expectation values; the J-weighted bond correlators add up to E0."""
    rows, run, _ = run_engine(tmp_path, "-Lx", 4, "-Ly", 2, "-heisenberg", 1, "-mwarmup", 64, "-nsweeps", 1, "-H_eps_tol", 1e-13)
    ham = J1J2XXZModel_SquareLattice(Lx=4, Ly=2, heisenberg=1.0)
    e0, psi, site_op = lattice_ground_state(ham)
    corr = json.load(open(str(tmp_path) + "/Correlations.json"))
    names = [c["name"] for c in corr["info"]]
    assert "Magnetization(3)" in names and "MagnetizationRowX1" in names and "Polyakov" in names and "Polyakov2" in names
    assert sum(n.startswith("NearestNeighbor") for n in names) == 3 * len(ham.NeighborPairs())
    assert len(corr["values"]) == 2
    vals = {}
    for c, v in zip(corr["info"], corr["values"][-1]):
        ops = parse_desc2(c["desc2"])
        P = None
        for (op, i) in ops:
            P = site_op(op, i) if P is None else P @ site_op(op, i)
        exact = float(psi @ (P @ psi))
        assert abs(v - exact) <= 1e-10, (c["name"], v, exact)
        vals[tuple(ops)] = v
    bond = sum(t.a * vals[((t.Iop, t.Isite), (t.Jop, t.Jsite))] for t in ham.H(8))
    assert abs(bond - e0) <= 1e-10 * abs(e0) and abs(run["GSEnergy"] - e0) <= 1e-10 * abs(e0)


def test_batched_correlators_equal_the_per_correlator_route(tmp_path):
    """The Gram-block batch (<psi|P (x) 1|psi> = sum_k <P, X_k X_k^T>, default) and the reference's route (one MatMult + dot per
    correlator, -corr_batch 0) give the same table on a J1-J2 lattice whose warm-up truncates (6x2, m = 24)."""
    model = ["-Lx", 6, "-Ly", 2, "-J1", 1, "-Jz1", 1, "-J2", 0.5, "-Jz2", 0.5, "-mwarmup", 24, "-nsweeps", 1, "-H_eps_tol", 1e-12]
    run_engine(tmp_path / "a", *model)
    run_engine(tmp_path / "b", *model, "-corr_batch", 0)
    ca, cb = (json.load(open(str(tmp_path / d) + "/Correlations.json")) for d in ("a", "b"))
    assert [c["name"] for c in ca["info"]] == [c["name"] for c in cb["info"]] and len(ca["values"]) == len(cb["values"]) == 2
    va, vb = np.array(ca["values"], dtype=float), np.array(cb["values"], dtype=float)
    assert np.abs(va).max() > 0.1 and np.abs(va - vb).max() <= 1e-12


def test_checkpoint_restart_continues_the_run(tmp_path):
    """one sweep + restart from its checkpoint + one sweep reproduces, step for step and bit for bit, the
    second sweep of an uninterrupted two-sweep run (blocks are restored exactly, the eigensolver's start vectors depend
    only on the restored global step index).  The checkpoint has the reference's directory layout."""
    # -wavefunction_guess 0: with the reference's random start vectors every step depends only on the restored blocks and the
    # global step index, so the continuation is bit-identical (a transformed start vector would need the previous step's
    # ground state, which a checkpoint does not carry: the first step after a restart then starts from a random vector;
    # -rdm_warm_start no longer does anything, with either value)
    model = ["-Lx", 6, "-Ly", 2, "-J1", 1, "-Jz1", 1, "-J2", 0.5, "-Jz2", 0.5, "-mwarmup", 24, "-H_eps_tol", 1e-12, "-wavefunction_guess", 0, "-rdm_warm_start", 0]
    (tmp_path / "a").mkdir(); (tmp_path / "b1").mkdir(); (tmp_path / "b2").mkdir()
    rows_a, run_a, _ = run_engine(tmp_path / "a", *model, "-nsweeps", 2)
    rows_b1, _, _ = run_engine(tmp_path / "b1", *model, "-nsweeps", 1, "-scratch_dir", str(tmp_path / "scratch1"))
    sdir = tmp_path / "scratch1"
    assert sorted(p.name for p in sdir.iterdir()) == ["Sweep_000000000", "Sweep_000000001"]        # warm-up, sweep 1
    last = sdir / "Sweep_000000001"
    for name in ("Hamiltonian.dat", "PetscOptions.dat", "Sweep.dat", "Sys_000000000/BlockInfo.dat", "Sys_000000005/QuantumNumbers.dat",
                 "Sys_000000005/Sp_000000005.mat", "Sys_000000005/H_000000000.mat"):
        assert (last / name).exists(), name
    assert not (last / "Sys_000000006").exists()                                                    # only the first N/2 blocks
    sweep = dict(ln.split() for ln in open(last / "Sweep.dat") if ln.strip())
    assert int(sweep["LoopIdx"]) == 1 and int(sweep["sys_ninit"]) == 6 and int(sweep["num_sites"]) == 12
    # restart: the model comes from Hamiltonian.dat (a deliberately wrong -Lx on the command line is overridden)
    rows_b2, run_b2, _ = run_engine(tmp_path / "b2", "-Lx", 2, "-Ly", 2, "-mwarmup", 24, "-H_eps_tol", 1e-12, "-nsweeps", 1, "-wavefunction_guess", 0, "-rdm_warm_start", 0,
                                    "-restart_dir", str(sdir), "-scratch_dir", str(tmp_path / "scratch2"))
    n1 = len(rows_b1)
    assert rows_a[:n1] and [r["GSEnergy"] for r in rows_a[:n1]] == [r["GSEnergy"] for r in rows_b1]
    second = rows_a[n1:]
    assert len(rows_b2) == len(second) == 12 - 4
    for r, o in zip(rows_b2, second):
        for key in ("GlobIdx", "LoopIdx", "NSites_Sys", "NSites_Env", "NumStates_H", "NStates_SysRot", "GSEnergy", "TruncErr_Sys", "TruncErr_Env"):
            assert r[key] == o[key], (key, r[key], o[key])
    assert run_b2["GSEnergy"] == run_a["GSEnergy"]
    assert (tmp_path / "scratch2" / "Sweep_000000002" / "Sweep.dat").exists()                       # the restarted run checkpoints on
    # a restart directory without checkpoints is refused
    (tmp_path / "empty").mkdir()
    out = subprocess.run([EXE, "-restart_dir", str(tmp_path / "empty"), "-mwarmup", "8", "-data_dir", str(tmp_path / "c") + "/"], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "No Sweep directory" in out.stderr


def test_transformed_start_vector_saves_matmults_not_accuracy(tmp_path):
    """The start vector of every eigensolve is the previous step's ground state carried into the new basis (on by default;
    the reference starts from a random vector): the converged energies and truncation errors are the same, the number of
    superblock MatMults drops several-fold."""
    model = ["-Lx", 8, "-Ly", 2, "-J1", 1, "-Jz1", 1, "-J2", 0.5, "-Jz2", 0.5, "-mwarmup", 48, "-nsweeps", 2, "-H_eps_tol", 1e-12]
    (tmp_path / "r").mkdir(); (tmp_path / "g").mkdir()
    rows_r, run_r, _ = run_engine(tmp_path / "r", *model, "-wavefunction_guess", 0)
    rows_g, run_g, _ = run_engine(tmp_path / "g", *model)
    assert len(rows_r) == len(rows_g)
    for r, g in zip(rows_r, rows_g):
        assert abs(r["GSEnergy"] - g["GSEnergy"]) <= 1e-10 * abs(r["GSEnergy"]), r["GlobIdx"]
        assert abs(r["TruncErr_Sys"] - g["TruncErr_Sys"]) <= 1e-8 * abs(r["TruncErr_Sys"]) + 1e-13, r["GlobIdx"]
    assert run_g["LastSweepMatMults"] * 2 < run_r["LastSweepMatMults"], (run_g["LastSweepMatMults"], run_r["LastSweepMatMults"])


def test_start_vectors_of_the_first_sweep_go_through_basis_overlaps(tmp_path):
    """The warm-up re-derives the environment blocks in decreasing order (the reference's order), so in the first sweep a stored
    block is usually the child of a version of its predecessor that has been overwritten since, and the stored rotation cannot
    carry the wavefunction into the current basis.  The engine carries the overlap of the two versions' bases along and projects the
    previous ground state through it (round 2 fell back to a random start vector there): same energies and truncation errors step by
    step, and the first sweep needs markedly fewer MatMults; the second sweep (consistent chain of bases) is untouched."""
    model = ["-Lx", 12, "-Ly", 4, "-J1", 1, "-Jz1", 1, "-J2", 0.5, "-Jz2", 0.5, "-mwarmup", 128, "-nsweeps", 2, "-H_eps_tol", 1e-12, "-H_eps_type", "gd"]
    rows_0, run_0, t_0 = run_engine(tmp_path / "off", *model, "-wavefunction_guess_overlap", 0)
    rows_1, run_1, t_1 = run_engine(tmp_path / "on", *model)
    assert len(rows_0) == len(rows_1)
    # (two converged runs that differ in their start vectors: equal up to what near-ties at a truncation cut amplify -- the oracle
    #  tests use sectors with gapped cuts for 1e-10; this lattice at m = 128 has cuts with gaps of 1e-9)
    for r, g in zip(rows_0, rows_1):
        assert abs(r["GSEnergy"] - g["GSEnergy"]) <= 1e-8 * abs(r["GSEnergy"]), r["GlobIdx"]
        assert abs(r["TruncErr_Sys"] - g["TruncErr_Sys"]) <= 1e-3 * abs(r["TruncErr_Sys"]) + 1e-12, r["GlobIdx"]
    assert abs(run_0["GSEnergy"] - run_1["GSEnergy"]) <= 1e-9 * abs(run_0["GSEnergy"])
    assert run_0["StartVectorsThroughOverlap"] == 0 and run_1["StartVectorsThroughOverlap"] >= 5
    col = t_0["headers"].index("MatMults")
    def per_loop(rows, t):
        out = {}
        for r, tr in zip(rows, t["table"]):
            out[r["LoopIdx"]] = out.get(r["LoopIdx"], 0) + tr[col]
        return out
    m0, m1 = per_loop(rows_0, t_0), per_loop(rows_1, t_1)
    assert m1[1] < 0.8 * m0[1], (m0, m1)
    assert abs(m1[2] - m0[2]) <= 0.05 * m0[2], (m0, m1)


@pytest.mark.parametrize("flag,kw", [("-BCopen", dict(BCopen=True)), ("-BCperiodic", dict(BCperiodic=True))])
def test_boundary_condition_options_match_exact_diagonalisation(tmp_path, flag, kw):
    """-BCopen / -BCperiodic (src/Hamiltonians.cpp:28-45; the default is the cylinder): 4x2 J1-J2 lattice with all four
    couplings, exact at m = 32, against dense ED built from the same option set."""
    rows, run, _ = run_engine(tmp_path, "-Lx", 4, "-Ly", 2, "-J1", 1, "-Jz1", 0.8, "-J2", 0.4, "-Jz2", 0.3, flag, 1,
                              "-mwarmup", 32, "-nsweeps", 1, "-H_eps_tol", 1e-13)
    ham = J1J2XXZModel_SquareLattice(Lx=4, Ly=2, J1=1, Jz1=0.8, J2=0.4, Jz2=0.3, **kw)
    e0, _, _ = lattice_ground_state(ham)
    assert abs(run["GSEnergy"] - e0) <= 1e-10 * abs(e0), (run["GSEnergy"], e0)


def test_container_smoke_of_the_reference(tmp_path):
    """tests/UnitTests_DMRGBlockContainer.cpp:11-26 of the reference: the default 4x4 lattice with
    -mwarmup 20 -msweeps 20,30,40 -maxnsweeps 3,3,3 must run through (the reference checks no value); here also: the
    energy never rises when m grows and every file of the run is valid JSON."""
    rows, run, timings = run_engine(tmp_path, "-mwarmup", 20, "-msweeps", "20,30,40", "-maxnsweeps", "3,3,3")
    assert run["Sweeps"] and run["Sweeps"][0] == 20 and run["Sweeps"][-1] == 40 and 3 <= len(run["Sweeps"]) <= 9
    centre = [r["GSEnergy"] for r in rows if r["NSites_Sys"] == r["NSites_Env"] and r["LoopType"] == "Sweep"]
    assert len(centre) == len(run["Sweeps"])
    by_m = {}
    for m, e in zip(run["Sweeps"], centre):
        by_m[m] = min(e, by_m.get(m, 0.0))
    assert by_m[40] <= by_m[30] + 1e-9 <= by_m[20] + 2e-9
    for name in ("EntanglementSpectra.json", "Correlations.json", "Timings.json"):
        json.load(open(str(tmp_path) + "/" + name))
    # the spectra are written by a background writer: one record per step, in step order, both sides, normalised spectra
    spec = json.load(open(str(tmp_path) + "/EntanglementSpectra.json"))
    assert [r["GlobIdx"] for r in spec] == [r["GlobIdx"] for r in rows]
    for r in spec:
        for side in ("Sys", "Env"):
            tot = sum(sum(s["vals"]) for s in r[side])
            assert r[side] and abs(tot - 1.0) <= 1e-5, (r["GlobIdx"], side, tot)


def test_spin_one_chain_matches_exact_diagonalisation(tmp_path):
    """-spin 1 (three states per site, Sz = diag(1,0,-1), S+ = sqrt(2)(|0><1| + |1><2|): src/DMRGBlock.cpp:1141-1156,1200-1215)
    on a 6-site Heisenberg chain, m large enough to be exact: energy and correlators against dense ED of the 3^6 lattice."""
    rows, run, _ = run_engine(tmp_path, "-spin", 1, "-Lx", 6, "-Ly", 1, "-heisenberg", 1, "-mwarmup", 100, "-nsweeps", 1, "-H_eps_tol", 1e-13)
    ham = J1J2XXZModel_SquareLattice(Lx=6, Ly=1, heisenberg=1.0)
    e0, psi, site_op = lattice_ground_state(ham, spin="1")
    assert abs(run["GSEnergy"] - e0) <= 1e-10 * abs(e0), (run["GSEnergy"], e0)
    corr = json.load(open(str(tmp_path) + "/Correlations.json"))
    for c, v in zip(corr["info"], corr["values"][-1]):
        P = None
        for (op, i) in parse_desc2(c["desc2"]):
            P = site_op(op, i) if P is None else P @ site_op(op, i)
        assert abs(v - float(psi @ (P @ psi))) <= 1e-9, c["name"]


def test_driver_fails_loudly_on_bad_options(tmp_path):
    out = subprocess.run([EXE, "-Lx", "3", "-Ly", "1", "-mwarmup", "8", "-data_dir", str(tmp_path) + "/"], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "must be even" in out.stderr


def test_two_rank_eigensolve_on_one_gpu():
    """N>1 path end to end on one GPU: two processes, striped plans (world_size 2), host-staged gloo collectives."""
    import sys
    script = os.path.join(ROOT, "tests", "dist_eigs_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29641", PYTHONPATH=ROOT)
    procs = [subprocess.Popen([sys.executable, script, str(r), "2"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)[-3000:]
    assert "two-rank eigensolve ok" in outs[0]


def test_native_communicator_rccl_single_rank():
    """csrc/comm.hip, RCCL back-end on the one GPU of the box (world 1): librccl.so resolves, the communicator initialises and
    the in-place collective call forms run; the eigensolver accepts opts.comm."""
    import sys
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "comm_worker.py"), "rccl1"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0 and "native rccl communicator ok" in p.stdout.decode(), p.stdout.decode()[-3000:]


@pytest.mark.parametrize("world", [2, 3])
def test_native_communicator_host_staged_ranks_on_one_gpu(world):
    """The same entry points through the host-staged back-end, `world` processes sharing cuda:0: all-gather / all-reduce /
    broadcast / host all-gather semantics, then the striped eigensolve issuing its own collectives (no Python callback in the
    Lanczos loop) against the one-rank solve (energy 1e-10 relative, eigenvector overlap)."""
    import sys
    name = "dmrgx_commtest_%d_%d" % (os.getpid(), world)
    env = dict(os.environ, PYTHONPATH=ROOT, DMRGX_SHM_MB="64")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "comm_worker.py"), "shm", str(r), str(world), name], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)[-3000:]
    assert "native %d-rank eigensolve ok" % world in outs[0]


def test_engine_starts_rccl_communicator(tmp_path):
    """The C++ engine's own start-up of the RCCL back-end (petsc_compat.hpp::CommBootstrap: device selection, id through the
    rendezvous file, ncclCommInitRank from a process without torch), with the one rank the test box can give it."""
    d = str(tmp_path) + "/"
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", DMRGX_FORCE_COMM="1", DMRGX_RDZV_FILE=d + "rdzv", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([EXE] + [str(o) for o in ("-Lx", 4, "-Ly", 2, "-heisenberg", 1, "-mwarmup", 32, "-nsweeps", 1, "-H_eps_tol", 1e-12, "-data_dir", d)],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    run = json.load(open(d + "DMRGRun.json"))
    assert abs(run["GSEnergy"] - (-6.6682766346354)) <= 1e-10 * 6.67 and run["Ranks"] == 1 and not os.path.exists(d + "rdzv")


def test_rccl_hooks_single_rank():
    """The torch.distributed form of the eigensolver's collective hooks (collectives.torch_hooks: the harness alternative to the
    native communicator), on a one-rank nccl group."""
    import sys
    script = os.path.join(ROOT, "tests", "nccl_hooks_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29643", PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0 and "rccl hooks ok" in out, out[-3000:]


def test_bench_multi_rank_control_flow_rehearsal():
    """`python bench.py --gpus 2` as a PLAIN command (the driver's form: bench.py starts its own rank processes), rehearsed with two
    ranks on the one GPU and the host-staged back-end of the native communicator: striped plans, the solver's own collectives,
    barrier + max-over-ranks timing, one JSON line from rank 0 with whole-job throughput, n_gpus read back from the library's
    communicator, and the engine legs on two ranks (configs[3]'s and configs[2]'s control flow on small lattices)."""
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env.update(DMRGX_BENCH_REHEARSAL="1", PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "24", "--warmup", "8", "--workload", "cfg2", "--full"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 24 and d["warmup"] == 8 and d["scaling"] == "strong" and d["unit"] == "MatMults/s"
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 1e-9
    assert d["cpu_baseline"] is None and d["roofline"]["achieved"] > 0
    assert "2 GPU" in d["config"]["parallelism"] and d["communicator"]["world"] == 2
    sw = d["sweep"]
    assert "error" not in sw and sw["ranks"] == 2 and sw["sites_per_s"] > 0, sw
    assert "error" not in sw["configs_2"] and sw["configs_2"]["ranks"] == 2 and sw["configs_2"]["sites_per_s"] > 0, sw["configs_2"]
    # the N > 1 line explains itself: where a step of the last sweep went on rank 0, the distributed MatMult split into its all-gather and
    # its apply by HIP events (dmrgx_eigs_comm_timing)
    bd = sw["step_breakdown_ms"]
    assert bd["t_allgather_ms"] > 0 and bd["t_apply_ms"] > 0 and bd["t_rdm_ms"] > 0 and bd["t_replicated_ms"] > 0, bd
    assert bd["t_allgather_ms"] + bd["t_apply_ms"] <= 1.05 * bd["t_solve_ms"] and bd["t_solve_ms"] + bd["t_rdm_ms"] <= 1.001 * bd["t_step_ms"], bd


def test_bench_plain_run_and_dumped_outputs(tmp_path, pkg):
    """`python bench.py` without --full: one JSON line from the timed steps alone (no CPU baselines, isolated MatMult or engine legs),
    and --dump-outputs writes what the timed eigensolve returned, checked against the CPU oracle's MatMult: psi is a unit vector in the
    reference's layout, e0 its Rayleigh quotient and `residual` the norm of H psi - e0 psi."""
    import sys
    from dmrgx_amd.workloads import synthetic_superblock
    from oracle.kron_factored import FactoredApplyCPU
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    d = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "4", "--workload", "cfg2", "--dump-outputs", str(d)]
    p = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["steps"] == 40 and r["warmup"] == 4 and r["n_gpus"] == 1 and r["unit"] == "MatMults/s" and r["dtype"] == "f64" and r["higher_is_better"] is True
    assert r["value"] > 0 and abs(r["value"] * r["ms_per_step"] / 1e3 - 1.0) < 1e-9 and r["roofline"]["achieved"] > 0
    assert r["cpu_baseline"] is None and r["matmult_isolated_per_s"] is None and "sweep" not in r
    assert sorted(os.listdir(d)) == ["e0.npy", "psi.npy", "residual.npy"]
    e0, res, psi = (np.load(d / (n + ".npy")) for n in ("e0", "residual", "psi"))
    assert e0.dtype == res.dtype == psi.dtype == np.float64 and e0.shape == res.shape == (1,)
    sb = synthetic_superblock("cfg2")
    assert psi.shape == (sb.n_states,) and abs(np.linalg.norm(psi) - 1.0) < 1e-12
    hpsi = FactoredApplyCPU(sb).apply(psi)
    e0, res = float(e0[0]), float(res[0])
    assert abs(float(psi @ hpsi) - e0) <= 1e-10 * abs(e0)
    assert abs(float(np.linalg.norm(hpsi - e0 * psi)) - res) <= 1e-8 * abs(e0) + 1e-6 * res
