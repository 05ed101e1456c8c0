"""-states_corr (no GPU): the host side of the eleventh engine measurement, StateCorrelations of host/EngineMeasurements.hpp -- the
single-mode weight of a transition amplitude (TransitionWeight, host/Measurements.hpp) through the host tool's transweight command
against numpy, and the option rules through measopts as in test_measurement_options_host.py."""
import subprocess

import numpy as np
import pytest

from test_measurement_options_host import ERR_ARG_WRONG, TOOL, measopts

NINE = ["corr_matrix", "corr_dimer", "corr_chiral", "dsf", "dsf_sites", "dsf_cheb", "dsf_dimer", "dsf_pm", "dsf_cv"]


def _transweight(Lx, Ly, x, y, T):
    line = " ".join(["transweight", str(Lx), str(Ly), str(len(T))] + [str(int(v)) for v in x] + [str(int(v)) for v in y] + [repr(float(v)) for v in T])
    out = subprocess.run([TOOL], input=line + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    tok = out.stdout.split()
    assert tok[0] == "transweight" and len(tok) == 1 + Lx * Ly, out.stdout
    return np.array([float(t) for t in tok[1:]]).reshape(Lx, Ly)


def _numpy_weight(Lx, Ly, x, y, T):
    nx, ny = np.meshgrid(np.arange(Lx), np.arange(Ly), indexing="ij")
    phase = 2.0 * np.pi * (nx[:, :, None] * x[None, None, :] / Lx + ny[:, :, None] * y[None, None, :] / Ly)
    return np.abs((np.exp(1j * phase) * T[None, None, :]).sum(axis=2)) ** 2 / len(T)


@pytest.mark.parametrize("Lx,Ly,seed", [(6, 2, 5), (3, 4, 6)])
def test_transition_weight_against_numpy(Lx, Ly, seed):
    """Random amplitudes on every site of the grid, the sites in a shuffled order: the table to 1e-14 of its largest entry, and the sum rule
    sum_q W(q) = sum_i T_i^2 of a full grid."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(Lx * Ly)
    x, y = order // Ly, order % Ly
    T = rng.standard_normal(Lx * Ly)
    got, want = _transweight(Lx, Ly, x, y, T), _numpy_weight(Lx, Ly, x, y, T)
    assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max(), np.abs(got - want).max()
    assert abs(got.sum() - T @ T) <= 1e-14 * Lx * Ly * (T @ T)
    assert (got >= 0).all()


def test_transition_weight_of_one_mode():
    """An amplitude cos(q0 . r) has all its weight at +q0 and -q0, a uniform one at q = 0."""
    Lx, Ly = 6, 2
    sites = np.arange(Lx * Ly)
    x, y = sites // Ly, sites % Ly
    W = _transweight(Lx, Ly, x, y, np.cos(2 * np.pi * (2 * x / Lx + 1 * y / Ly)))
    assert abs(W[2, 1] - 3.0) < 1e-13 and abs(W[4, 1] - 3.0) < 1e-13 and abs(W.sum() - 6.0) < 1e-13
    W = _transweight(Lx, Ly, x, y, np.ones(Lx * Ly))
    assert abs(W[0, 0] - 12.0) < 1e-13 and abs(W.sum() - 12.0) < 1e-13


def test_measopts_prints_the_line_when_on():
    rc, m, _ = measopts([])
    assert rc == 0 and list(m) == NINE
    rc, m, _ = measopts(["-nstates", 3, "-states_corr_cross", 1])         # the cross switch alone turns nothing on
    assert rc == 0 and list(m) == NINE
    rc, m, _ = measopts(["-nstates", 3, "-states_corr", 0])
    assert rc == 0 and list(m) == NINE
    rc, m, _ = measopts(["-nstates", 3, "-states_corr", 1])
    assert rc == 0 and list(m) == NINE + ["states_corr"] and m["states_corr"]["on"] and m["states_corr"]["cross"] == "0"
    rc, m, _ = measopts(["-nstates", 2, "-states_corr", 1, "-states_corr_cross", 1])
    assert rc == 0 and m["states_corr"]["on"] and m["states_corr"]["cross"] == "1"
    assert not any(m[k]["on"] for k in NINE)


@pytest.mark.parametrize("opts", [["-states_corr", 1], ["-states_corr", 1, "-nstates", 1]], ids=["no -nstates", "-nstates 1"])
def test_states_corr_needs_two_states(opts):
    rc, _, err = measopts(opts)
    assert rc == ERR_ARG_WRONG and "-states_corr" in err and "-nstates" in err, err
