"""-spin_penalty without a GPU: the schedule of -spin_penalty / -spin_penalty_warmup (host/SpinPenalty.hpp, through the host tool), the
carried total-spin operator of a one-site block and its checkpoint file, and the exact diagonalisation with total spin resolved
(tests/spin_penalty_ed.py) that the GPU tests compare the engine with."""
import json
import os

import numpy as np
import pytest

from oracle.hamiltonian import J1J2XXZModel_SquareLattice
import spin_penalty_ed as ed
from test_measurements_host import _tool


def _schedule(sched, warm, nsweeps, ranks=1):
    out, err = _tool(["spinpenalty %s %s %d %d" % (sched, warm, nsweeps, ranks)])
    rc = int(out[0].split()[1])
    if rc:
        return rc, err, None, None
    vals = [float(x) for x in out[1].split()[1:]]
    any_, js = out[2].split(" json ")
    return rc, vals[0], vals[1:], (int(any_.split()[1]), json.loads(js))


def test_schedule_is_a_list_whose_last_value_holds():
    rc, warm, sweeps, (any_, js) = _schedule("2,0.5,0", "none", 5)
    assert rc == 0 and warm == 0.0 and sweeps == [2.0, 0.5, 0.0, 0.0, 0.0] and any_ == 1 and js == [2.0, 0.5, 0.0]
    rc, warm, sweeps, (any_, js) = _schedule("1.25", "none", 3)
    assert rc == 0 and sweeps == [1.25] * 3 and js == [1.25]
    rc, warm, sweeps, (any_, js) = _schedule("0,3", "0.125", 4)
    assert rc == 0 and warm == 0.125 and sweeps == [0.0, 3.0, 3.0, 3.0] and any_ == 1


def test_without_the_option_and_with_zeros_nothing_is_on():
    rc, warm, sweeps, (any_, js) = _schedule("none", "none", 3)
    assert rc == 0 and warm == 0.0 and sweeps == [0.0] * 3 and any_ == 0 and js == []
    rc, warm, sweeps, (any_, js) = _schedule("0,0", "0", 3)
    assert rc == 0 and warm == 0.0 and sweeps == [0.0] * 3 and any_ == 0 and js == [0.0, 0.0]
    rc, warm, sweeps, (any_, js) = _schedule("none", "0.5", 2)           # the warm-up alone
    assert rc == 0 and warm == 0.5 and sweeps == [0.0, 0.0] and any_ == 1


@pytest.mark.parametrize("sched,warm", [("1,-2", "none"), ("1,x", "none"), ("1,,2", "none"), ("nan", "none"), ("inf", "none"), ("empty", "none"), ("1", "-1"), ("1", "inf")])
def test_negative_and_non_finite_values_are_refused(sched, warm):
    rc, err, _, _ = _schedule(sched, warm, 2)
    assert rc == 63 and "-spin_penalty" in err                            # PETSC_ERR_ARG_OUTOFRANGE


def test_more_than_one_rank_is_refused_unless_every_weight_is_zero():
    rc, err, _, _ = _schedule("2", "none", 2, ranks=2)
    assert rc == 56 and "-spin_penalty is not available on more than one rank (got 2)" in err      # PETSC_ERR_SUP
    rc, err, _, _ = _schedule("none", "1e-3", 2, ranks=4)
    assert rc == 56 and "more than one rank (got 4)" in err
    assert _schedule("0,0", "0", 2, ranks=2)[0] == 0 and _schedule("none", "none", 2, ranks=2)[0] == 0


def _rows(lines, tag):
    """the rows of the operator `tag` of a dump: {row: {col: value}}"""
    i = next(k for k, ln in enumerate(lines) if ln.startswith("op %s " % tag))
    if lines[i].endswith("null"):
        return None
    n = int(lines[i].split()[3])
    return {r: {int(t.split(":")[0]): float(t.split(":")[1]) for t in lines[i + 1 + r].split()[2:]} for r in range(n)}


def test_one_site_block_carries_its_own_sp_and_the_checkpoint_holds_it(tmp_path):
    """CreateSpTot on a one-site block is the site's Sp in cells of its own; a block that was not given one has none; SaveToDisk writes
    SpTot_000000000.mat only where the block carries the operator; InitializeFromDisk reads it when asked and refuses a checkpoint
    without it then."""
    d1, d2 = str(tmp_path / "with"), str(tmp_path / "without")
    os.makedirs(d1), os.makedirs(d2)
    out, _ = _tool(["single A", "dumpsptot A", "sptot A", "dumpsptot A", "dump A", "save A " + d1,
                    "single B", "save B " + d2, "load C %s 1" % d1, "dumpsptot C", "load D " + d1, "dumpsptot D", "load E %s 1" % d2])
    first = out.index("op SpTot 0 null")
    assert first == 1                                                     # before CreateSpTot: nothing
    rest = out[first + 2:]
    sptot, sp = _rows(rest, "SpTot"), _rows(rest, "Sp")
    assert sptot == sp == {0: {1: 1.0}, 1: {}}
    assert os.path.exists(d1 + "/SpTot_000000000.mat") and not os.path.exists(d2 + "/SpTot_000000000.mat")
    loads = [k for k, ln in enumerate(out) if ln.startswith("op SpTot")]
    assert _rows(out[loads[2]:], "SpTot") == {0: {1: 1.0}, 1: {}}      # C: read back
    assert out[loads[3]] == "op SpTot 0 null"                            # D: not asked for, not read
    assert out[-1] not in ("rc 0",) and out[-1].startswith("rc ")        # E: asked for, not there


@pytest.fixture(scope="module")
def heis_6x2_levels():
    return ed.levels(J1J2XXZModel_SquareLattice(Lx=6, Ly=2, heisenberg=1.0), 0)


def test_every_level_of_the_12_site_lattice_has_a_definite_spin(heis_6x2_levels):
    """Sz = 0 of 6 x 2 Heisenberg: 924 states; S^2 = <S- S+> + M (M + 1) of every eigenvector is an integer S (S + 1) to 1e-10, the
    multiplicities are those of 12 spins 1/2 (132 singlets, 297 triplets, 275, 154, 54, 11, 1), and the tower the option is for is there:
    the lowest level is a singlet, the next three are triplets."""
    lv = heis_6x2_levels
    assert len(lv["energy"]) == 924
    S = np.round((-1.0 + np.sqrt(1.0 + 4.0 * np.maximum(lv["spin2"], 0.0))) / 2.0)
    dev = np.abs(lv["spin2"] - S * (S + 1)).max()
    print("largest |S^2 - S (S + 1)|:", dev)
    assert dev <= 1e-10
    assert [int((S == s).sum()) for s in range(7)] == [132, 297, 275, 154, 54, 11, 1]
    assert np.abs(lv["eigenvalue"] - (lv["energy"] + ed.RESOLVE * lv["raised"])).max() <= 1e-10
    order = np.argsort(lv["energy"])
    assert np.abs(lv["energy"][order][:4] - np.array([-10.10564932, -8.68857893, -8.33800372, -7.89301581])).max() <= 1e-8
    assert np.abs(lv["spin2"][order][:4] - np.array([0.0, 2.0, 2.0, 2.0])).max() <= 1e-10
    assert np.abs(ed.lowest_of_spin(lv, 0, 3) - np.array([-10.10564932, -7.00244885, -6.74602273])).max() <= 1e-8


def test_penalty_moves_a_level_of_spin_s_by_lambda_times_its_casimir():
    """H' = H + lam S- S+ in the sectors M = 0 and M = 1 of the 4 x 2 lattice: the same energies <H> as at the resolving weight, every
    eigenvalue moved by lam [S (S + 1) - M (M + 1)], S = |M| not at all."""
    ham = J1J2XXZModel_SquareLattice(Lx=4, Ly=2, heisenberg=1.0)
    for M in (0, 1):
        a, b = ed.levels(ham, M), ed.levels(ham, M, 2.0)
        assert np.abs(np.sort(a["energy"]) - np.sort(b["energy"])).max() <= 1e-10
        assert np.abs(b["eigenvalue"] - (b["energy"] + 2.0 * (b["spin2"] - M * (M + 1)))).max() <= 1e-10
        assert abs(b["spin2"][0] - M * (M + 1)) <= 1e-10 and abs(b["eigenvalue"][0] - b["energy"][0]) <= 1e-10
        assert b["raised"].min() >= -1e-12
