"""The density-matrix solver on the expansion of dmrgx_kron_noise_expand (-m gpu): dmrgx_rdm_create_subset with the expanded extents as
the other side's sector table gives the spectra of White's perturbed matrix rho' = Psi Psi^T + sum coef^2 (A Psi')(A Psi')^T, which the
test builds densely per sector WITHOUT the expansion (tests/noise_inputs.py); the two-phase selection, the Rayleigh-quotient
verification at destruction and the kept rows work on it unchanged; and the panels raise the rank of a rank-deficient sector."""
import numpy as np
import pytest

import helpers
import noise_inputs as ni

pytestmark = pytest.mark.gpu
LAYOUT = (ni.LSZ, ni.RSZ, ni.BLOCKS)


@pytest.fixture(scope="module")
def mods(pkg):
    from dmrgx_amd import superblock, workloads, _capi
    _capi.require_device()
    return superblock, workloads, _capi


@pytest.fixture(scope="module")
def planted(mods):
    """Per side: psi, operators, the dense perturbed density matrices and their LAPACK spectra (descending); built once, read-only."""
    _, wl, _ = mods
    out = {}
    for side in (0, 1):
        psi, ops = ni.case(wl, side)
        rho = ni.model_rho(psi, side, ops, ni.COEF)
        w = [np.linalg.eigvalsh(r)[::-1] for r in rho]
        for a in rho + w:
            a.setflags(write=False)
        out[side] = (psi, ops, rho, w)
    return out


@pytest.mark.parametrize("side", [0, 1])
def test_spectra_selection_and_verification_on_the_expansion(mods, planted, side):
    sbm, _, _ = mods
    psi, ops, rho, w_ref = planted[side]
    Y, extent, n_out = sbm.noise_expand(LAYOUT, psi, side, ops, ni.COEF)
    lsz, rsz, blocks, mask = sbm.noise_rdm_layout(LAYOUT, side, extent)
    rdm = sbm.ReducedDensityMatrices(lsz, rsz, blocks, Y, side_mask=mask)
    jacobi = bool(rdm.report.solver)
    spectra = []
    for k in range(len(blocks)):
        w = rdm.eigenvalues(side, k)
        spectra.append(w)
        bound_w, _ = (helpers.rdm_jacobi_bounds if jacobi else helpers.rdm_bounds)(rho[k], w_ref[k])
        err = np.abs(w - w_ref[k]).max()
        print("noise rdm side %d block %d n %d: |w - eigvalsh| %.3e, bound %.3e" % (side, k, len(w), err, bound_w))
        assert w.shape == w_ref[k].shape and np.isfinite(w).all() and np.all(np.diff(w) <= 0)
        assert err <= bound_w, (k, err, bound_w)
    # the other side of the expansion was not built
    with pytest.raises(Exception):
        rdm.eigenvalues(1 - side, 0)
    # half of the states kept: the kept rows are orthonormal eigenvectors of rho', and the verification at destruction agrees
    counts = [0] * (2 * len(blocks))
    for k in range(len(blocks)):
        counts[2 * k + side] = (len(spectra[k]) + 1) // 2
    rdm.select(counts)
    rows = rdm.eigenvectors_batch([(side, k, counts[2 * k + side]) for k in range(len(blocks))])
    for k, U in enumerate(rows):
        U = U.cpu().numpy()
        c = counts[2 * k + side]
        _, bound_r = (helpers.rdm_jacobi_bounds if jacobi else helpers.rdm_bounds)(rho[k], w_ref[k])
        orth = np.abs(U @ U.T - np.eye(c)).max()
        res = np.abs(rho[k] @ U.T - U.T * spectra[k][:c]).max()
        print("  block %d: %d rows kept, orthonormal to %.3e, residual %.3e (bound %.3e)" % (k, c, orth, res, bound_r))
        assert np.isfinite(U).all() and orth <= 1e-12, (k, orth)
        assert res <= bound_r, (k, res, bound_r)
    rdm.destroy()                      # raises unless dmrgx_rdm_destroy returns DMRGX_OK: eigenvalues == Rayleigh quotients |Psi'^T u|^2


def test_the_panels_raise_the_rank_of_a_deficient_sector(mods, planted):
    """Left sector 2 has 65 states but Psi of its KronBlock only 5 columns: rho_L has 5 eigenvalues above 1e-14 of the trace, the
    perturbed matrix more -- on the device as in the model."""
    sbm, _, _ = mods
    psi, ops, rho, w_ref = planted[0]
    k = ni.BLOCKS.index((2, 2))
    X = ni.psi_blocks(psi)[k]
    assert X.shape == (65, 5)

    def rank(w):
        return int(np.sum(w > 1e-14 * w.sum()))

    plain = sbm.ReducedDensityMatrices(ni.LSZ, ni.RSZ, ni.BLOCKS, __import__("torch").from_numpy(np.array(psi)).cuda())
    r0 = rank(plain.eigenvalues(0, k))
    plain.destroy()
    Y, extent, _ = sbm.noise_expand(LAYOUT, psi, 0, ops, ni.COEF)
    lsz, rsz, blocks, mask = sbm.noise_rdm_layout(LAYOUT, 0, extent)
    rdm = sbm.ReducedDensityMatrices(lsz, rsz, blocks, Y, side_mask=mask)
    r1 = rank(rdm.eigenvalues(0, k))
    rdm.destroy()
    print("rank of rho_L of sector 2: %d plain, %d perturbed (model: %d)" % (r0, r1, rank(w_ref[k])))
    assert rank(np.linalg.eigvalsh(X @ X.T)) == 5 and rank(w_ref[k]) > 5         # the model: the term does what it is for
    assert r1 > r0                                                               # the device: the count grows
