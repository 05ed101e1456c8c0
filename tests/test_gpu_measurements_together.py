"""The nine engine measurements do not see each other (-m gpu): one run of the 6 x 2 Heisenberg lattice with -corr_matrix, -corr_dimer,
-corr_chiral, -dsf, -dsf_sites, -dsf_cheb, -dsf_dimer, -dsf_pm and -dsf_cv all on, and nine runs with one of them on and the same
values.  The last record a measurement writes alone is the record it writes in company, number for number: the library's reductions are
fixed-order and take no atomics, the window run of the Chebyshev three starts from a fixed seed, and no measurement writes to psi.  Only
the wall time of a measurement differs between two runs; those fields are named here, one per file, and nothing else is left out."""
import json

import pytest

from test_gpu_engine import run_engine
from test_gpu_dsf import HEIS_6x2, _no_nan

pytestmark = pytest.mark.gpu

COMMON = [*HEIS_6x2, "-mwarmup", 24]
LANCZOS = ["-dsf_steps", 20]
CHEB = ["-dsf_cheb_steps", 20, "-dsf_cheb_omega", "0,6,13"]
# option: (its command line, its file, the wall-time field of its records, records per measurement point)
MEASUREMENTS = {
    "corr_matrix": (["-corr_matrix", 1], "SpinCorrelations.json", "tCorrMatrix", 1),
    "corr_dimer": (["-corr_dimer", 1], "DimerCorrelations.json", "tDimer", 1),
    "corr_chiral": (["-corr_chiral", 1], "ChiralCorrelations.json", "tChiral", 1),
    "dsf": (["-dsf", 1, "-dsf_q", "3,1,1,0", *LANCZOS], "DynamicalStructureFactor.json", "tDsf", 1),
    "dsf_sites": (["-dsf_sites", "6,0", *LANCZOS], "DynamicalCorrelations.json", "tDsfSites", 1),
    "dsf_cheb": (["-dsf_cheb", "6,0", *CHEB], "ChebyshevMoments.json", "tDsfCheb", 1),
    "dsf_dimer": (["-dsf_dimer", "6,0", "-dsf_dimer_steps", 20], "DimerDynamics.json", "tDimerDyn", 1),
    "dsf_pm": (["-dsf_pm", "6,0", *CHEB], "TransverseDynamics.json", "tDsfPm", 2),      # one record per channel
    "dsf_cv": (["-dsf_cv", "6,0", "-dsf_cv_omega", "0,4,3"], "CorrectionVectors.json", "tDsfCv", 1),
}


def all_on_options():
    """Every measurement's options once (-dsf and -dsf_sites share the Lanczos steps, -dsf_cheb and -dsf_pm the Chebyshev ones)."""
    opts = list(COMMON)
    for own, _, _, _ in MEASUREMENTS.values():
        for k in range(0, len(own), 2):
            if own[k] not in opts:
                opts += own[k:k + 2]
    return opts


def _last_records(d, name):
    _, file, wall_time, count = MEASUREMENTS[name]
    records = json.load(open(str(d) + "/" + file))
    assert len(records) >= count, (file, len(records))
    out = []
    for rec in records[-count:]:
        assert _no_nan(rec), file
        kept = {k: v for k, v in rec.items() if k != wall_time}
        assert set(rec) - set(kept) == {wall_time}, (file, sorted(rec))      # that field, and only that field, is left out
        out.append(kept)
    return out


@pytest.fixture(scope="module")
def all_on(tmp_path_factory):
    d = tmp_path_factory.mktemp("together")
    run_engine(d, *all_on_options())
    return d


@pytest.mark.parametrize("name", list(MEASUREMENTS))
def test_alone_equals_in_company(tmp_path, all_on, name):
    run_engine(tmp_path, *COMMON, *MEASUREMENTS[name][0])
    alone, company = _last_records(tmp_path, name), _last_records(all_on, name)
    for a, b in zip(alone, company):
        assert a.keys() == b.keys()
        for key in a:
            assert a[key] == b[key], (MEASUREMENTS[name][1], key)
