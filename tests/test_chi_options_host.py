"""-chi_sites, -chi_bonds, -chi_tol, -chi_maxit (no GPU): the option rules of the tenth engine measurement, StaticSusceptibility of
host/EngineMeasurements.hpp, through the host tool's measopts command as in test_measurement_options_host.py -- its line is printed when
the measurement is on --, and the entry point behind it: exported, bound, and refusing a null plan without a device."""
import ctypes as C
import os

import pytest

from test_measurement_options_host import ERR_ARG_OUTOFRANGE, ERR_SUP, measopts

NINE = ["corr_matrix", "corr_dimer", "corr_chiral", "dsf", "dsf_sites", "dsf_cheb", "dsf_dimer", "dsf_pm", "dsf_cv"]


def test_off_without_the_options(tmp_path, monkeypatch):
    """Nothing on: the nine lines as before, no line of the tenth, and nothing written where the tool runs; -chi_tol and -chi_maxit alone
    are not read (a bad value passes), and an empty list leaves the measurement off."""
    monkeypatch.chdir(tmp_path)
    rc, m, _ = measopts([])
    assert rc == 0 and list(m) == NINE
    for opts in (["-chi_tol", 2, "-chi_maxit", 0], ["-chi_sites", ""], ["-chi_bonds", ""], ["-chi_sites", "", "-chi_bonds", ""]):
        rc, m, err = measopts(opts)
        assert rc == 0 and list(m) == NINE, err
    assert os.listdir(str(tmp_path)) == []


def test_values_and_defaults():
    rc, m, _ = measopts(["-chi_sites", "6,0"])
    chi = m["chi"]
    assert rc == 0 and list(m) == NINE + ["chi"] and chi["on"] and chi["sites"] == "6,0" and chi["bonds"] == "-" and float(chi["tol"]) == 1e-8 and chi["maxit"] == "2000"
    assert not any(m[k]["on"] for k in NINE)
    rc, m, _ = measopts(["-chi_bonds", "15,3", "-chi_tol", 1e-6, "-chi_maxit", 50])
    chi = m["chi"]
    assert rc == 0 and chi["on"] and chi["sites"] == "-" and chi["bonds"] == "15,3" and float(chi["tol"]) == 1e-6 and chi["maxit"] == "50"
    rc, m, _ = measopts(["-chi_sites", "11", "-chi_bonds", "0"])
    assert rc == 0 and m["chi"]["sites"] == "11" and m["chi"]["bonds"] == "0"


@pytest.mark.parametrize("opts,message", [
    (["-chi_sites", "3,12"], "-chi_sites: site 12 is outside [0, 12)"),
    (["-chi_sites", "-1"], "-chi_sites: site -1 is outside [0, 12)"),
    (["-chi_bonds", "3,16"], "-chi_bonds: bond 16 is outside [0, 16)"),
    (["-chi_bonds", "-1"], "-chi_bonds: bond -1 is outside [0, 16)"),
    (["-chi_sites", "3", "-chi_bonds", "16"], "-chi_bonds: bond 16 is outside [0, 16)"),
    (["-chi_sites", "3", "-chi_tol", "0"], "-chi_tol must lie in (0, 1). Got 0."),
    (["-chi_bonds", "3", "-chi_tol", "1"], "-chi_tol must lie in (0, 1). Got 1."),
    (["-chi_sites", "3", "-chi_tol", "-1e-3"], "-chi_tol must lie in (0, 1)"),
    (["-chi_sites", "3", "-chi_maxit", "0"], "-chi_maxit must be at least 1. Got 0."),
], ids=["site 12", "site -1", "bond 16", "bond -1", "bond beside a good site", "tol 0", "tol 1", "tol negative", "maxit 0"])
def test_bad_options_are_refused(opts, message):
    rc, _, err = measopts(opts)
    assert rc == ERR_ARG_OUTOFRANGE and message in err, err


@pytest.mark.parametrize("opts,option", [(["-chi_sites", 6], "-chi_sites"), (["-chi_bonds", 6], "-chi_bonds"), (["-chi_sites", 6, "-chi_bonds", 6], "-chi_sites")],
                         ids=["sites", "bonds", "both"])
def test_two_ranks_are_refused(opts, option):
    rc, _, err = measopts(opts, ranks=2)
    assert rc == ERR_SUP and option + " is not available on more than one rank" in err and "(got 2)" in err, err
    assert measopts(opts, ranks=1)[0] == 0


def test_the_options_are_read_last():
    """Of two mistakes the one read first is refused: every other measurement's options come before these."""
    rc, _, err = measopts(["-chi_sites", 99, "-dsf_cv", "3"])
    assert rc != 0 and "-dsf_cv needs -dsf_cv_omega" in err and "-chi_sites" not in err, err
    rc, _, err = measopts(["-chi_bonds", 99, "-dsf_dimer", 99])
    assert rc == ERR_ARG_OUTOFRANGE and "-dsf_dimer: bond 99" in err and "-chi_bonds" not in err, err


def test_entry_point_is_exported_and_refuses_a_null_plan(pkg):
    """dmrgx_kron_static_response is in the library and in the ctypes table with the header's sixteen arguments; a null plan is
    DMRGX_ERR_ARG before any device work -- no GPU is needed to be refused -- and the outputs are untouched."""
    capi = pkg._capi
    lib = capi.lib()
    assert hasattr(lib, "dmrgx_kron_static_response") and len(capi.SIGNATURES["dmrgx_kron_static_response"][1]) == 16
    coef, norm2, stats = C.c_double(-7.0), C.c_double(-7.0), capi.CvStats()
    stats.iterations = -7
    fake = C.c_void_p(4096)                                           # never dereferenced: the refusal comes first
    rc = lib.dmrgx_kron_static_response(C.c_void_p(), fake, fake, 0.0, 0.0, 10, 0, fake, 0, C.c_void_p(), 0, C.byref(coef), C.byref(norm2),
                                        C.POINTER(C.c_double)(), C.byref(stats), C.c_void_p())
    assert rc == capi.DMRGX_ERR_ARG and b"null argument" in lib.dmrgx_last_error()
    assert coef.value == -7.0 and norm2.value == -7.0 and stats.iterations == -7
    assert lib.dmrgx_abi_version() == 3
