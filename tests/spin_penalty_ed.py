"""Exact diagonalisation with total spin resolved, for the tests of -spin_penalty (no GPU): a lattice of N spins 1/2 in one Sz sector,
H from the model's own term list, S-_tot S+_tot = S^2 - Sz (Sz + 1) from the site operators.

[H, S^2] = 0, so H' = H + lam S- S+ has the eigenvectors of H with every level of spin S moved by lam [S (S + 1) - M (M + 1)].  A small
irrational lam splits the levels of H in which two spins meet, and the eigenvectors of H' are then states of definite spin: `levels`
returns, per eigenvector, the eigenvalue of H', <H> and <S- S+>.  (Degenerate levels of one spin stay degenerate; their S^2 is definite
all the same.)"""
import numpy as np
import scipy.sparse as sp

from oracle.qn import OpSm, OpSp, OpSz

RESOLVE = np.sqrt(2.0) * 1e-3


def sector_matrices(ham, M=0):
    """(H, S- S+) as dense matrices in the sector Sz = M; site 0 is the most significant factor, a site's first state is up"""
    N = ham.NumSites()
    single = {OpSz: sp.csr_matrix(np.array([[0.5, 0.0], [0.0, -0.5]])), OpSp: sp.csr_matrix(np.array([[0.0, 1.0], [0.0, 0.0]]))}
    single[OpSm] = single[OpSp].T.tocsr()
    cache = {}

    def site_op(op, i):
        if (op, i) not in cache:
            cache[(op, i)] = sp.kron(sp.kron(sp.identity(2 ** i, format="csr"), single[op], format="csr"), sp.identity(2 ** (N - 1 - i), format="csr"), format="csr")
        return cache[(op, i)]

    H = sp.csr_matrix((2 ** N, 2 ** N))
    for t in ham.H(N):
        H = H + t.a * (site_op(t.Iop, t.Isite) @ site_op(t.Jop, t.Jsite))
    up = sp.csr_matrix((2 ** N, 2 ** N))
    for i in range(N):
        up = up + site_op(OpSp, i)
    ndown = N // 2 - int(round(M)) if N % 2 == 0 else None
    assert ndown is not None and abs(M - round(M)) < 1e-12, "an even number of sites and an integer sector"
    sector = np.array([s for s in range(2 ** N) if bin(s).count("1") == ndown])
    raised = (up.T @ up).tocsr()
    return H.tocsr()[sector][:, sector].toarray(), raised[sector][:, sector].toarray()


def levels(ham, M=0, lam=RESOLVE):
    """The eigenvectors of H' = H + lam S- S+ in the sector Sz = M, ascending in the eigenvalue of H':
    dict(eigenvalue=..., energy=<H>, raised=<S- S+>, spin2=raised + M (M + 1)), arrays that cannot be written to"""
    H, R = sector_matrices(ham, M)
    w, V = np.linalg.eigh(H + lam * R)
    out = {"eigenvalue": w, "energy": np.einsum("ik,ik->k", V, H @ V), "raised": np.einsum("ik,ik->k", V, R @ V)}
    out["spin2"] = out["raised"] + M * (M + 1)
    for a in out.values():
        a.setflags(write=False)
    return out


def lowest_of_spin(lv, S, count):
    """the `count` lowest energies of the levels of spin S of `levels` output, ascending"""
    e = np.sort(lv["energy"][np.abs(lv["spin2"] - S * (S + 1)) < 1e-6])
    return e[:count]
