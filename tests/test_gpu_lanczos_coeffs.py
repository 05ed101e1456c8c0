"""dmrgx_kron_lanczos_coeffs: the device-resident three-term recursion against a numpy Lanczos on the dense Hamiltonian (-m gpu).

The three small synthetic superblocks of test_gpu_kron.test_kron_diag_matches_dense_diagonal, H made dense column by column with the
numpy restatement of the factored apply, as the eigensolver tests there do (once per module)."""
import numpy as np
import pytest
import torch

from helpers import lanczos_reorth as _lanczos_reorth

pytestmark = pytest.mark.gpu
ERR_ARG = 62
CASES = {"cfg2": dict(name="cfg2", m=32, Ly=3, seed=3), "cfg1": dict(name="cfg1", m=12, Ly=1, seed=4), "cfg5": dict(name="cfg5", m=40, Ly=2, seed=5)}


@pytest.fixture(scope="module")
def mods(pkg):
    from dmrgx_amd import superblock, workloads, _capi
    _capi.require_device()
    return superblock, workloads, _capi


@pytest.fixture(scope="module")
def dense(mods):
    """name -> (superblock, dense H, eigenvalues, eigenvectors); read-only"""
    _, wl, _ = mods
    out = {}
    for key, kw in CASES.items():
        sb = wl.synthetic_superblock(kw["name"], m=kw["m"], Ly=kw["Ly"], seed=kw["seed"])
        H = np.stack([wl.apply_factored_numpy(sb, e) for e in np.eye(sb.n_states)], axis=1)
        w, v = np.linalg.eigh(H)
        for a in (H, w, v):
            a.setflags(write=False)
        out[key] = (sb, H, w, v)
    return out


@pytest.mark.parametrize("key", list(CASES))
def test_coefficients_against_reorthogonalised_numpy(mods, dense, key):
    """Random v0, K = 10: norm2, alpha_0..9 and beta_0..8 to 1e-10 max |alpha| (plain and reorthogonalised recursions agree to 1e-13 over
    these steps; the margin covers the summation order).  Two runs give the same bits; v0 is unchanged."""
    sbm, _, _ = mods
    sb, H, _, _ = dense[key]
    K = 10
    v0 = np.random.default_rng(11).standard_normal(sb.n_states)
    n2, a, b = _lanczos_reorth(H, v0, K)
    plan = sbm.KronPlan(sb)
    v0d = torch.from_numpy(v0).cuda()
    norm2, alpha, beta, done = plan.lanczos_coeffs(v0d, K)
    norm2b, alphab, betab, doneb = plan.lanczos_coeffs(v0d, K)
    plan.destroy()
    tol = 1e-10 * np.abs(a).max()
    print(key, "n", sb.n_states, "norm2 err", abs(norm2 - n2), "alpha err", np.abs(alpha - a).max(), "beta err", np.abs(beta[:K - 1] - b[:K - 1]).max(), "tol", tol)
    assert done == K and np.isfinite(alpha).all() and np.isfinite(beta).all()
    assert abs(norm2 - n2) <= tol
    assert np.abs(alpha - a).max() <= tol and np.abs(beta[:K - 1] - b[:K - 1]).max() <= tol
    assert norm2 == norm2b and done == doneb
    assert np.array_equal(alpha.view(np.uint64), alphab.view(np.uint64)) and np.array_equal(beta.view(np.uint64), betab.view(np.uint64))
    assert np.array_equal(v0d.cpu().numpy().view(np.uint64), v0.view(np.uint64))


@pytest.mark.parametrize("key", list(CASES))
def test_planted_invariant_subspace_breaks_down_on_the_device(mods, dense, key):
    """v0 a combination of 5 eigenvectors (weights in [0.5, 1.5]), nsteps = 9: the Krylov space is exhausted after 5 steps.  nsteps_done
    is 5, the entries 5..8 are exactly 0, nothing is NaN or Inf, and T_5 holds the 5 eigenvalues and the squared coefficients to 1e-9."""
    sbm, _, _ = mods
    sb, H, w, v = dense[key]
    n = sb.n_states
    idx = np.array([0, n // 5, (2 * n) // 5, (3 * n) // 5, n - 1])
    c = np.random.default_rng(13).uniform(0.5, 1.5, 5)
    v0 = v[:, idx] @ c
    plan = sbm.KronPlan(sb)
    norm2, alpha, beta, done = plan.lanczos_coeffs(torch.from_numpy(v0).cuda(), 9)
    plan.destroy()
    print(key, "done", done, "alpha", alpha, "beta", beta)
    assert done == 5
    assert np.isfinite(alpha).all() and np.isfinite(beta).all()
    assert (alpha[5:] == 0.0).all() and (beta[5:] == 0.0).all()
    assert beta[4] <= 1e-7 * max(np.abs(alpha[:5]).max(), beta[:4].max())          # the beta that broke: kept as measured
    T = np.diag(alpha[:5]) + np.diag(beta[:4], 1) + np.diag(beta[:4], -1)
    th, z = np.linalg.eigh(T)
    assert np.abs(th - w[idx]).max() <= 1e-9, np.abs(th - w[idx]).max()
    assert np.abs(norm2 * z[0] ** 2 - c ** 2).max() <= 1e-9, np.abs(norm2 * z[0] ** 2 - c ** 2).max()


def test_more_steps_than_states(mods, dense):
    """nsteps may exceed n_states.  Without reorthogonalisation the recursion need not notice that the Krylov space is exhausted (rounding
    keeps beta alive): the run is accepted, everything is finite, and whatever lies behind nsteps_done is exactly 0."""
    sbm, wl, _ = mods
    sb = wl.synthetic_superblock("cfg1", m=4, Ly=1, seed=3)
    n = sb.n_states
    plan = sbm.KronPlan(sb)
    v0 = torch.from_numpy(np.random.default_rng(17).standard_normal(n)).cuda()
    norm2, alpha, beta, done = plan.lanczos_coeffs(v0, n + 6)
    plan.destroy()
    assert 1 <= done <= n + 6 and np.isfinite(alpha).all() and np.isfinite(beta).all()
    assert (alpha[done:] == 0.0).all() and (beta[done:] == 0.0).all()


def test_zero_and_nan_start_vectors_and_refusals(mods, dense):
    sbm, _, capi = mods
    sb = dense["cfg1"][0]
    plan = sbm.KronPlan(sb)
    n = sb.n_states
    for fill in (0.0, float("nan")):
        v0 = torch.full((n,), fill, dtype=torch.float64, device="cuda")
        norm2, alpha, beta, done = plan.lanczos_coeffs(v0, 6)
        assert norm2 == 0.0 and done == 0 and (alpha == 0.0).all() and (beta == 0.0).all(), (fill, norm2, done, alpha, beta)
    ok = torch.ones(n, dtype=torch.float64, device="cuda")
    for bad in (0, -3):
        with pytest.raises(capi.DmrgxError) as e:
            plan.lanczos_coeffs(ok, bad)
        assert e.value.code == ERR_ARG
    with pytest.raises(capi.DmrgxError) as e:
        plan.lanczos_coeffs(ok, 4, breakdown_tol=-1.0)
    assert e.value.code == ERR_ARG
    plan.destroy()
    striped = sbm.KronPlan(sb, world_size=2, rank=0)
    full = torch.ones(striped.info.vec_len, dtype=torch.float64, device="cuda")
    with pytest.raises(capi.DmrgxError) as e:
        striped.lanczos_coeffs(full, 4)
    assert e.value.code == ERR_ARG and "striped" in str(e.value)
    striped.destroy()
