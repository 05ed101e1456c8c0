"""host/Measurements.hpp (no GPU): what -dsf_cheb, -dsf_pm and -dsf_dimer share after the device call -- ScaleMoments (the cut, the
transpose and the division by the norm), ChebyshevGrid (the Jackson-damped sums at the frequencies asked for) and the moment part of a
record (JsonRecordFile::Omega and ::Moments) -- through the host tool."""
import json

import numpy as np
import pytest

from test_measurements_host import _tool


def _nums(a):
    return " ".join("%.17g" % x for x in np.asarray(a, dtype=float).ravel())


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("K,done", [(1, 1), (1, 0), (5, 5), (5, 2), (5, 0)])
def test_scale_moments_against_numpy(count, K, done):
    """diag is cut to 2 done + 1 entries, cross[k][s] to k <= done and transposed to mom[s][k]; every entry is ONE division by the norm,
    so the comparison is ==.  The entries past the cut are poisoned: none may reach the result."""
    rng = np.random.default_rng(100 * count + 10 * K + done)
    diag, cross, norm = rng.standard_normal(2 * K + 1), rng.standard_normal((K + 1, count)), 0.7 + rng.random()
    diag[2 * done + 1:] = 1e300
    cross[done + 1:] = 1e300
    out, _ = _tool(["chebmoments %d %d %d %.17g %s %s" % (count, K, done, norm, _nums(diag), _nums(cross))])
    got_diag, got_mom = (np.array([float(x) for x in line.split()[1:]]) for line in out)
    assert out[0].split()[0] == "diag" and out[1].split()[0] == "mom"
    want_diag, want_mom = diag[:2 * done + 1] / norm, (cross[:done + 1].T / norm).ravel()
    assert got_diag.shape == want_diag.shape and (got_diag == want_diag).all()
    assert got_mom.shape == want_mom.shape == (count * (done + 1),) and (got_mom == want_mom).all()


@pytest.mark.parametrize("nm", [1, 6])
@pytest.mark.parametrize("nw", [1, 4])
@pytest.mark.parametrize("M", [1, 3])
def test_chebyshev_grid_is_the_jackson_sum_of_every_row(nm, nw, M):
    """grid[q][k] = chebjackson(momq[q], nm, x_k) / half_width at x_k = (w_k + E0 - centre) / half_width: the same function on the same
    doubles, so ==.  With four frequencies the last lies above the window, where the sum is 0."""
    rng = np.random.default_rng(1000 * nm + 10 * nw + M)
    momq = rng.standard_normal((M, nm))
    E0, centre, half_width = -3.25, 1.5, 5.0 + rng.random()
    omega = np.array([0.4] if nw == 1 else [0.0, 1.3, 7.9, 11.0])
    x = (omega + E0 - centre) / half_width
    assert abs(x[0]) < 1.0 and (nw == 1 or x[-1] > 1.0)
    lines = ["chebgrid %d %d %d %.17g %.17g %.17g %s %s" % (M, nm, nw, E0, centre, half_width, _nums(momq), _nums(omega))]
    lines += ["chebjackson %d %d %s %s" % (nm, nw, _nums(momq[q]), _nums(x)) for q in range(M)]
    out, _ = _tool(lines)
    assert out[0].split()[0] == "chebgrid" and all(line.split()[0] == "chebjackson" for line in out[1:]) and len(out) == 1 + M
    got = np.array([float(v) for v in out[0].split()[1:]])
    want = np.array([[float(v) for v in line.split()[1:]] for line in out[1:]]) / half_width
    assert got.shape == (M * nw,) and (got == want.ravel()).all()
    assert got[0] != 0.0 and (nw == 1 or (got.reshape(M, nw)[:, -1] == 0.0).all())


def _row(v):
    return "[" + ", ".join("%.17g" % x for x in v) + "]"


def _table(name, T, end):
    return '   "%s": [\n' % name + ",\n".join("     " + _row(r) for r in T) + "\n   ]" + end


def _moment_record(have_omega, nsites):
    """What `momentrec` must write, from the format rules of ChebyshevMoments.json: entry s is a run of s + 1 steps, its numbers are
    (from + s + i) / 3 with from = 0 (Diag), 10 (Moments, 2 rows), 20 (MomentsQ, 2 rows), 30 (SqwGrid, 2 x 2)."""
    text = '[\n  {"GlobIdx": 7, "LoopType": "Sweep", "E0": %.17g, "Norm": %.17g,\n' % (-1 / 3, 2 / 3)
    if have_omega:
        text += '   "Omega": ' + _row([1 / 3, 2 / 3]) + ",\n"
    text += '   "Sites": [\n'
    for s in range(nsites):
        done, end = s + 1, "},\n" if s + 1 < nsites else "}\n"
        thirds = lambda cnt, start: np.array([(start + s + i) / 3 for i in range(cnt)])  # noqa: E731
        text += '   {"Site": %d, "r": [%d, 0], "Norm2": %.17g, "StepsDone": %d,\n   "Diag": ' % (s, s, (s + 1) / 3, done)
        text += _row(thirds(2 * done + 1, 0)) + ",\n"
        text += _table("Moments", thirds(2 * (done + 1), 10).reshape(2, done + 1), ",\n")
        text += _table("MomentsQ", thirds(2 * (done + 1), 20).reshape(2, done + 1), ",\n" if have_omega else end)
        if have_omega:
            text += _table("SqwGrid", thirds(4, 30).reshape(2, 2), end)
    return text + "   ]}\n]\n"


@pytest.mark.parametrize("have_omega", [0, 1])
@pytest.mark.parametrize("nsites", [1, 2])
def test_moment_record_bytes(tmp_path, have_omega, nsites):
    """The four cases in which the end of an entry changes place: after MomentsQ without frequencies, after SqwGrid with them; "}," between
    two entries, "}" after the last."""
    path = str(tmp_path / "rec.json")
    out, _ = _tool([f"momentrec {path} {have_omega} {nsites}"])
    assert out == ["rc 0"]
    assert open(path, "rb").read() == _moment_record(have_omega, nsites).encode()
    (rec,) = json.load(open(path))
    assert ("Omega" in rec) == bool(have_omega) and [e["StepsDone"] for e in rec["Sites"]] == list(range(1, nsites + 1))
    for e in rec["Sites"]:
        assert ("SqwGrid" in e) == bool(have_omega) and len(e["Diag"]) == 2 * e["StepsDone"] + 1
        assert np.array(e["Moments"]).shape == np.array(e["MomentsQ"]).shape == (2, e["StepsDone"] + 1)
