"""host/EngineMeasurements.hpp (no GPU): the option rules of the nine engine measurements, through the host tool's measopts command --
EngineMeasurements::ReadOptions on a given number of ranks, on the options database that the driver reads.  The refusals are the ones
the GPU tests see from the driver (tests/test_gpu_dsf*.py, test_gpu_chiral.py), with their PETSc codes; the rest is what the measurements
share: the Lanczos steps of -dsf and -dsf_sites, the Chebyshev steps, grid and window of -dsf_cheb, -dsf_pm and -dsf_dimer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dmrg.x_amd", "dmrgx-host-tool")
HEIS_6x2 = ["-Lx", 6, "-Ly", 2, "-heisenberg", 1]      # 12 sites, 16 nearest-neighbour bonds
ERR_SUP, ERR_ARG_WRONG, ERR_ARG_OUTOFRANGE = 56, 62, 63


def measopts(opts, ranks=1):
    """(rc, {measurement: {"on": bool, field: text}}, stderr); an empty value goes in as "_"."""
    line = " ".join(["measopts", str(ranks)] + [str(o) if str(o) != "" else "_" for o in [*HEIS_6x2, *opts]])
    out = subprocess.run([TOOL], input=line + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert lines and lines[0].startswith("rc "), out.stdout
    parsed = {}
    for ln in lines[1:]:
        tok = ln.split()
        parsed[tok[0]] = dict(zip(tok[2::2], tok[3::2]), on=tok[1] == "1")
    return int(lines[0].split()[1]), parsed, out.stderr


def test_defaults_with_nothing_on():
    rc, m, _ = measopts([])
    assert rc == 0 and list(m) == ["corr_matrix", "corr_dimer", "corr_chiral", "dsf", "dsf_sites", "dsf_cheb", "dsf_dimer", "dsf_pm", "dsf_cv"]
    assert not any(v["on"] for v in m.values())
    assert m["dsf"]["steps"] == "100" and m["dsf_cheb"]["steps"] == "200" and m["dsf_cheb"]["bound_steps"] == "40" and m["dsf_cheb"]["window"] == "-"
    assert m["dsf_dimer"]["steps"] == "200" and m["dsf_cv"]["maxit"] == "2000" and float(m["dsf_cv"]["eta"]) == 0.1 and float(m["dsf_cv"]["tol"]) == 1e-8


@pytest.mark.parametrize("opts,message", [
    (["-corr_chiral", 1], "-corr_chiral 1 is not available on more than one rank"),
    (["-dsf", 1, "-dsf_q", "3,1"], "-dsf 1 is not available on more than one rank"),
    (["-dsf_sites", 6], "-dsf_sites is not available on more than one rank"),
    (["-dsf_cheb", 6], "-dsf_cheb is not available on more than one rank"),
    (["-dsf_dimer", 6], "-dsf_dimer is not available on more than one rank"),
    (["-dsf_pm", 6], "-dsf_pm is not available on more than one rank"),
    (["-dsf_cv", 6, "-dsf_cv_omega", "0,4,5"], "-dsf_cv is not available on more than one rank"),
], ids=["corr_chiral", "dsf", "dsf_sites", "dsf_cheb", "dsf_dimer", "dsf_pm", "dsf_cv"])
def test_two_ranks_are_refused(opts, message):
    rc, _, err = measopts(opts, ranks=2)
    assert rc == ERR_SUP and message in err and "(got 2)" in err, err
    assert measopts(opts, ranks=1)[0] == 0


def test_two_ranks_keep_the_tables_every_rank_computes():
    rc, m, _ = measopts(["-corr_matrix", 1, "-corr_dimer", 1], ranks=2)
    assert rc == 0 and m["corr_matrix"]["on"] and m["corr_dimer"]["on"] and not m["corr_chiral"]["on"]


@pytest.mark.parametrize("opts,message,code", [
    (["-dsf_cv", "3,12", "-dsf_cv_omega", "0,4,5"], "-dsf_cv: site 12 is outside [0, 12)", ERR_ARG_OUTOFRANGE),
    (["-dsf_cv", "3"], "-dsf_cv needs -dsf_cv_omega w0,w1,nw", ERR_ARG_WRONG),
    (["-dsf_cv", "3", "-dsf_cv_omega", "0,4"], "-dsf_cv_omega needs w0,w1,nw", ERR_ARG_WRONG),
    (["-dsf_cv", "3", "-dsf_cv_omega", "0,4,5", "-dsf_cv_eta", "0"], "-dsf_cv_eta must be positive", ERR_ARG_OUTOFRANGE),
    (["-dsf_cv", "3", "-dsf_cv_omega", "0,4,5", "-dsf_cv_eta", "-0.1"], "-dsf_cv_eta must be positive", ERR_ARG_OUTOFRANGE),
    (["-dsf_cv", "3", "-dsf_cv_omega", "0,4,5", "-dsf_cv_maxit", "0"], "-dsf_cv_maxit must be at least 1", ERR_ARG_OUTOFRANGE),
], ids=["site", "no omega", "short omega", "eta 0", "eta negative", "maxit 0"])
def test_bad_dsf_cv_options_are_refused(opts, message, code):
    rc, _, err = measopts(opts)
    assert rc == code and message in err, err


def test_dsf_cv_values():
    rc, m, _ = measopts(["-dsf_cv", "6,0", "-dsf_cv_omega", "0,4,3", "-dsf_cv_eta", 0.25, "-dsf_cv_tol", 1e-6, "-dsf_cv_maxit", 50])
    cv = m["dsf_cv"]
    assert rc == 0 and cv["on"] and cv["sites"] == "6,0" and cv["omega"] == "0,2,4" and float(cv["eta"]) == 0.25 and float(cv["tol"]) == 1e-6 and cv["maxit"] == "50"


def test_lanczos_steps_reach_dsf_and_dsf_sites():
    """-dsf_steps is read once, by the first of -dsf and -dsf_sites that is on: with both on, and with -dsf_sites alone."""
    rc, m, _ = measopts(["-dsf", 1, "-dsf_q", "3,1,1,0", "-dsf_sites", "6,0", "-dsf_steps", 7, "-dsf_breakdown_tol", 0.5])
    assert rc == 0 and m["dsf"]["on"] and m["dsf"]["q"] == "3,1,1,0" and m["dsf_sites"]["on"] and m["dsf_sites"]["sites"] == "6,0"
    assert m["dsf"]["steps"] == m["dsf_sites"]["steps"] == "7" and float(m["dsf"]["breakdown_tol"]) == float(m["dsf_sites"]["breakdown_tol"]) == 0.5
    rc, m, _ = measopts(["-dsf_sites", "6,0", "-dsf_steps", 7])
    assert rc == 0 and not m["dsf"]["on"] and m["dsf_sites"]["on"] and m["dsf_sites"]["steps"] == "7"
    for on in (["-dsf", 1, "-dsf_q", "3,1"], ["-dsf_sites", 6]):
        rc, _, err = measopts([*on, "-dsf_steps", 0])
        assert rc == ERR_ARG_OUTOFRANGE and "-dsf_steps must be at least 1. Got 0." in err, err
    assert measopts(["-dsf_steps", 0])[0] == 0               # neither is on: not read


def test_dsf_needs_pairs_of_integers():
    for opts, got in ((["-dsf", 1], 0), (["-dsf", 1, "-dsf_q", "3,1,1"], 3)):
        rc, _, err = measopts(opts)
        assert rc == ERR_ARG_WRONG and "-dsf 1 needs -dsf_q nx0,ny0,nx1,ny1,..." in err and "Got %d numbers." % got in err, err


def test_chebyshev_steps_are_read_for_dsf_pm_alone():
    rc, m, _ = measopts(["-dsf_pm", "6,0", "-dsf_cheb_steps", 9, "-dsf_cheb_omega", "0,6,13"])
    assert rc == 0 and m["dsf_pm"]["on"] and not m["dsf_cheb"]["on"] and m["dsf_pm"]["sites"] == "6,0"
    assert m["dsf_pm"]["steps"] == "9" and m["dsf_pm"]["omega"].split(",")[:3] == ["0", "0.5", "1"] and len(m["dsf_pm"]["omega"].split(",")) == 13
    rc, _, err = measopts(["-dsf_pm", 6, "-dsf_cheb_steps", 0])
    assert rc == ERR_ARG_OUTOFRANGE and "-dsf_cheb_steps must be at least 1. Got 0." in err, err
    rc, _, err = measopts(["-dsf_pm", 6, "-dsf_cheb_omega", "0,6"])
    assert rc == ERR_ARG_WRONG and "-dsf_cheb_omega needs w0,w1,nw" in err, err


def test_window_options_are_read_for_dsf_dimer_alone():
    """-dsf_dimer shares the window and the bound steps of -dsf_cheb, not its steps and grid; with none of the three on, none is checked."""
    rc, m, _ = measopts(["-dsf_dimer", "6,0", "-dsf_dimer_steps", 20, "-dsf_dimer_omega", "0,4,3", "-dsf_cheb_bound_steps", 11, "-dsf_cheb_window", "-9.5,3"])
    d = m["dsf_dimer"]
    assert rc == 0 and d["on"] and d["bonds"] == "6,0" and d["steps"] == "20" and d["omega"] == "0,2,4" and d["bound_steps"] == "11" and d["window"] == "-9.5,3"
    rc, _, err = measopts(["-dsf_dimer", 6, "-dsf_cheb_bound_steps", 0])
    assert rc == ERR_ARG_OUTOFRANGE and "-dsf_cheb_bound_steps must be at least 1. Got 0." in err, err
    rc, _, err = measopts(["-dsf_dimer", 6, "-dsf_cheb_window", "3,-9.5"])
    assert rc == ERR_ARG_WRONG and "-dsf_cheb_window needs lo,hi" in err, err
    rc, _, err = measopts(["-dsf_dimer", 6, "-dsf_dimer_steps", 0])
    assert rc == ERR_ARG_OUTOFRANGE and "-dsf_dimer_steps must be at least 1. Got 0." in err, err
    assert measopts(["-dsf_dimer", 6, "-dsf_cheb_steps", 0])[0] == 0                    # the steps are -dsf_cheb's and -dsf_pm's
    assert measopts(["-dsf_cheb_bound_steps", 0, "-dsf_cheb_window", "3,-9.5", "-dsf_cheb_steps", 0, "-dsf_dimer_steps", 0])[0] == 0


def test_lists_are_read_before_the_shared_options():
    """Of two mistakes the one read first is refused: the three lists come before the Chebyshev steps, the steps before the window."""
    rc, _, err = measopts(["-dsf_cheb", 3, "-dsf_cheb_steps", 0, "-dsf_dimer", 99])
    assert rc == ERR_ARG_OUTOFRANGE and "-dsf_dimer: bond 99 is outside [0, 16)" in err and "-dsf_cheb_steps" not in err, err
    rc, _, err = measopts(["-dsf_dimer", 3, "-dsf_cheb_bound_steps", 0, "-dsf_pm", 3, "-dsf_cheb_steps", 0])
    assert rc == ERR_ARG_OUTOFRANGE and "-dsf_cheb_steps must be at least 1" in err and "-dsf_cheb_bound_steps" not in err, err


@pytest.mark.parametrize("option", ["-dsf_sites", "-dsf_cheb", "-dsf_dimer", "-dsf_pm", "-dsf_cv"])
def test_an_empty_list_leaves_the_measurement_off(option):
    rc, m, err = measopts([option, ""])
    assert rc == 0 and not m[option[1:]]["on"], err


@pytest.mark.parametrize("option,count,noun", [("-dsf_sites", 12, "site"), ("-dsf_cheb", 12, "site"), ("-dsf_pm", 12, "site"), ("-dsf_cv", 12, "site"), ("-dsf_dimer", 16, "bond")])
def test_the_first_index_past_the_end_is_refused(option, count, noun):
    extra = ["-dsf_cv_omega", "0,4,3"] if option == "-dsf_cv" else []
    rc, m, _ = measopts([option, "0,%d" % (count - 1), *extra])
    assert rc == 0 and m[option[1:]]["on"]
    rc, _, err = measopts([option, "0,%d" % count, *extra])
    assert rc == ERR_ARG_OUTOFRANGE and "%s: %s %d is outside [0, %d)" % (option, noun, count, count) in err, err
    rc, _, err = measopts([option, "-1", *extra])
    assert rc == ERR_ARG_OUTOFRANGE and "%s: %s -1 is outside [0, %d)" % (option, noun, count) in err, err
