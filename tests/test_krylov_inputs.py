"""The inputs of tests/test_gpu_krylov_shapes.py have the properties they were built for (no GPU): a GPU test on an input without its
property proves nothing.  The builders are in tests/helpers.py; the dense H and its spectrum are computed once per process."""
import numpy as np
import pytest

import helpers


@pytest.fixture(scope="module")
def wl(pkg):
    from dmrgx_amd import workloads
    return workloads


@pytest.mark.parametrize("n", sorted(helpers.KRYLOV_KEPT))
def test_state_counts_are_odd_and_span_one_two_and_three_workgroups(wl, n):
    sb = helpers.krylov_superblock(wl, n)
    assert sb.n_states == n and n % 2 == 1
    assert -(-n // 2048) == {845: 1, 1205: 1, 2049: 2, 4097: 3}[n]          # workgroups of 2048 elements in the basis-keeping Lanczos run
    x = np.random.default_rng(n).standard_normal(n)
    y = np.random.default_rng(n + 1).standard_normal(n)
    H = helpers.FactoredH(wl, sb)
    hx, hy = H @ x, H @ y
    assert abs(y @ hx - x @ hy) <= 1e-12 * np.linalg.norm(hx) * np.linalg.norm(y)      # symmetric, seen through two vectors
    assert np.array_equal(H @ np.stack([x, y], axis=1), np.stack([hx, hy], axis=1))


@pytest.mark.parametrize("key", [845, 1205, "cfg2", "posdef", "degenerate", "tinygap"])
def test_dense_inputs_are_symmetric(wl, key):
    sb, H, w, v = helpers.krylov_input(wl, key)
    normH = np.abs(w).max()
    assert H.shape == (sb.n_states,) * 2 and sb.n_states == {"cfg2": 844, 1205: 1205}.get(key, 845)
    assert np.abs(H - H.T).max() <= 1e-12 * normH
    assert not H.flags.writeable and not w.flags.writeable and not v.flags.writeable


def test_plain_inputs_have_a_negative_lowest_eigenvalue(wl):
    """What the positive-definite input is there to change."""
    for key in (845, 1205, "cfg2"):
        w = helpers.krylov_input(wl, key)[2]
        assert w[0] < 0.0 < w[-1]


def test_positive_definite_input(wl):
    _, H, w, _ = helpers.krylov_input(wl, "posdef")
    w_plain = helpers.krylov_input(wl, 845)[2]
    print("posdef: w0", w[0], "w_max", w[-1])
    assert w[0] > 0.0 and abs(w[-1]) > 2.0 * abs(w[0])
    assert abs(w[0] - 3.0) <= 1e-12 * np.abs(w).max()
    assert np.abs((w - w[0]) - (w_plain - w_plain[0])).max() <= 1e-12 * np.abs(w).max()      # the whole spectrum shifted


def test_degenerate_input(wl):
    sb, H, w, _ = helpers.krylov_input(wl, "degenerate")
    normH = np.abs(w).max()
    print("degenerate: w0..w2", w[:3], "w1 - w0", w[1] - w[0], "|H|", normH)
    assert sb.terms == []
    assert w[1] - w[0] <= 1e-12 * normH and w[2] - w[0] >= 0.5
    assert abs(w[0] + 3.5) <= 1e-12 * normH


def test_tiny_gap_input(wl):
    sb, H, w, _ = helpers.krylov_input(wl, "tinygap")
    ratio = (w[1] - w[0]) / (w[-1] - w[0])
    print("tinygap: w0, w1", w[:2], "w_max", w[-1], "gap ratio", ratio)
    assert len(sb.terms) == 12 and all(t[0] != 0.0 for t in sb.terms)
    assert 3e-4 <= ratio <= 3e-3
    assert w[2] - w[1] > 100.0 * (w[1] - w[0])          # one close neighbour, not a cluster
