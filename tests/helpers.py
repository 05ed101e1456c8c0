"""Test infrastructure: bridges between the product's Superblock description and the CPU oracle."""
import numpy as np
import scipy.sparse as sp

from oracle.block import Block
from oracle.hamiltonian import Term
from oracle.kron import KronBlocks, ShellCtx
from oracle.qn import QuantumNumbers

CELL_DENSE, CELL_IDENT = 1, 2


def operator_to_csr(op, sizes):
    """SectorOperator (cells) -> scipy CSR of the whole block basis."""
    off = np.concatenate([[0], np.cumsum(sizes)])
    n = int(off[-1])
    R, C, V = [], [], []
    for c in op.cells:
        r0, c0 = off[c.row_sector] + c.r0, off[c.row_sector + op.shift] + c.c0
        if c.kind == CELL_DENSE:
            ii, jj = np.meshgrid(np.arange(c.nr), np.arange(c.nc), indexing="ij")
            R.append((r0 + ii).ravel()); C.append((c0 + jj).ravel()); V.append(np.asarray(c.array).ravel())
        else:
            R.append(r0 + np.arange(c.nr)); C.append(c0 + np.arange(c.nr)); V.append(np.full(c.nr, c.scale))
    if not R:
        return sp.csr_matrix((n, n))
    m = sp.coo_matrix((np.concatenate(V), (np.concatenate(R), np.concatenate(C))), shape=(n, n)).tocsr()
    m.sort_indices()
    return m


def oracle_blocks_from_superblock(sb):
    """Oracle Block objects (CSR Sz(i), Sp(i), H + Magnetization) and the un-reflected reference Term list."""
    def mk(nsites, qn, sizes, ops, h):
        b = Block.with_sectors(nsites, qn, sizes)
        for (op, site), o in ops.items():
            (b.SzData if op == 0 else b.SpData)[site] = operator_to_csr(o, sizes)
        b.H = operator_to_csr(h, sizes)
        return b
    L = mk(sb.n_left_sites, sb.left_qn, sb.left_sizes, sb.left_ops, sb.h_left)
    R = mk(sb.n_right_sites, sb.right_qn, sb.right_sizes, sb.right_ops, sb.h_right)
    nout = sb.n_left_sites + sb.n_right_sites
    # the reference reflects right sites itself (src/DMRGKron.cpp:805-807): hand it global indices
    terms = [Term(a, Iop, Isite, Jop, nout - 1 - Jsite) for (a, Iop, Isite, Jop, Jsite) in sb.terms]
    return L, R, terms


def oracle_shell_from_superblock(sb, target=0.0):
    L, R, terms = oracle_blocks_from_superblock(sb)
    kb = KronBlocks(L, R, (target,))
    assert [(t[1], t[2]) for t in kb.kb] == list(sb.blocks), "KronBlock order differs from the reference's nested loop"
    return ShellCtx(kb, terms)


def secop_from(op, keep, ld_pad=0):
    """ctypes dmrgx_secop for a workloads.SectorOperator; device tensors appended to `keep`.  ld_pad > 0: every dense cell lives in a
    wider NaN-filled device array, ld = nc + ld_pad (in the engine every cell is a view into an arena)."""
    import torch
    from dmrgx_amd import _capi
    cells = (_capi.Cell * max(len(op.cells), 1))()
    for i, c in enumerate(op.cells):
        cells[i].row_sector, cells[i].r0, cells[i].c0, cells[i].nr, cells[i].nc, cells[i].kind, cells[i].scale = c.row_sector, c.r0, c.c0, c.nr, c.nc, c.kind, c.scale
        if c.kind == CELL_DENSE:
            wide = np.full((c.nr, c.nc + ld_pad), np.nan)
            wide[:, :c.nc] = c.array
            t = torch.from_numpy(wide).cuda()
            keep.append(t)
            cells[i].data, cells[i].ld = t.data_ptr(), c.nc + ld_pad
    keep.append(cells)
    s = _capi.SecOp()
    s.shift, s.transposed, s.ncells, s.cells = op.shift, 0, len(op.cells), cells
    return s


# ---- independent exact diagonalisation of the lattice model (correlator known answers) -------------------------------
def lattice_ground_state(ham, spin="1/2"):
    """Dense ED of the whole lattice in the site basis (site 0 = most significant factor), from the model's own term
    list.  Returns (E0, psi, site_op) where site_op(op, i) is the d^N x d^N matrix of a single-site operator
    (single-site matrices of src/DMRGBlock.cpp:1131-1215 for spin 1/2 and spin 1)."""
    import scipy.sparse as sp
    from oracle.qn import OpSm, OpSz, OpSp
    N = ham.NumSites()
    if spin == "1":
        sz = sp.csr_matrix(np.diag([1.0, 0.0, -1.0]))
        spl = sp.csr_matrix(np.sqrt(2.0) * np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]]))
    else:
        sz = sp.csr_matrix(np.array([[0.5, 0.0], [0.0, -0.5]]))
        spl = sp.csr_matrix(np.array([[0.0, 1.0], [0.0, 0.0]]))
    d = sz.shape[0]
    single = {OpSz: sz, OpSp: spl, OpSm: spl.T.tocsr()}
    cache = {}

    def site_op(op, i):
        if (op, i) not in cache:
            m = sp.identity(1, format="csr")
            for s in range(N):
                m = sp.kron(m, single[op] if s == i else sp.identity(d, format="csr"), format="csr")
            cache[(op, i)] = m
        return cache[(op, i)]

    H = sp.csr_matrix((d ** N, d ** N))
    for t in ham.H(N):
        H = H + t.a * (site_op(t.Iop, t.Isite) @ site_op(t.Jop, t.Jsite))
    w, v = np.linalg.eigh(H.toarray())
    return float(w[0]), v[:, 0].copy(), site_op


def parse_desc2(desc2):
    """'< Sz_{3} Sp_{4} >' -> [(OpSz, 3), (OpSp, 4)] (the engine / reference description string of a correlator)."""
    import re
    from oracle.qn import OpSm, OpSz, OpSp
    kinds = {"Sz": OpSz, "Sp": OpSp, "Sm": OpSm}
    return [(kinds[k], int(i)) for k, i in re.findall(r"(S[zpm])_\{(\d+)\}", desc2)]


# ---- grouped GEMM: groups with planted borders, a plain float64 reference and a derived bound (tests/test_gpu_ggemm.py) ---------------
GGEMM_SENTINEL = -6.02214076e+123      # the band round an output; must come back bit for bit
SCALED_COPY = "s"                      # entry of a product list: alpha * S (an int K is a GEMM product A[M x K] B[K x N])


def ggemm_values(rng, shape):
    """Magnitudes in [0.5, 1.5] with random signs: every single term a * b or alpha * s of an output element is >= 0.25 in magnitude."""
    return rng.uniform(0.5, 1.5, size=shape) * rng.choice((-1.0, 1.0), size=shape)


class GgemmOperand:
    """A rows x cols matrix as a sub-view (row and column offset, ld > cols) of a larger buffer filled with `fill`."""

    def __init__(self, rng, values, fill, tight=False):
        rows, cols = values.shape
        top, bottom, left, right = (1, 1, 1, 2) if tight else (int(v) for v in rng.integers(1, 6, size=4))
        self.buf = np.full((rows + top + bottom, cols + left + right), fill, dtype=np.float64)
        self.r0, self.c0, self.rows, self.cols = top, left, rows, cols
        self.view[...] = values

    @property
    def view(self):
        return self.buf[self.r0:self.r0 + self.rows, self.c0:self.c0 + self.cols]

    @property
    def ld(self):
        return self.buf.shape[1]

    @property
    def first(self):          # element offset of view[0, 0] inside buf
        return self.r0 * self.ld + self.c0


class GgemmInstance:
    """One group description with its operands: C[M x N] (=|+=) sum_p A_p B_p + sum_q alpha_q S_q.  `prods` lists K (GEMM product) or
    SCALED_COPY in the caller's order.  A, B and S sit in NaN buffers (a read past the K edge, or outside S, poisons the result); the
    output's initial content is C0 (magnitude rule) when accumulating and NaN otherwise, inside a band of GGEMM_SENTINEL.
    R, S_abs, n: the float64 reference, sum of the magnitudes of the terms and the number of terms of an element."""

    def __init__(self, rng, M, N, prods, accumulate=False, tight=False):
        self.M, self.N, self.accumulate = M, N, bool(accumulate)
        self.prods = []                # (kind, K, A operand or None, B / S operand, alpha)
        for p in prods:
            if p == SCALED_COPY:
                self.prods.append((1, 0, None, GgemmOperand(rng, ggemm_values(rng, (M, N)), np.nan, tight), float(ggemm_values(rng, ()))))
            else:
                K = int(p)
                self.prods.append((0, K, GgemmOperand(rng, ggemm_values(rng, (M, K)), np.nan, tight),
                                   GgemmOperand(rng, ggemm_values(rng, (K, N)), np.nan, tight), 1.0))
        self.C0 = ggemm_values(rng, (M, N)) if accumulate else None
        self.c_pad = (1, 1, 1, 2) if tight else tuple(int(v) for v in rng.integers(1, 6, size=4))
        self.R, self.S_abs, self.n = ggemm_reference(self)

    def output_buffer(self):
        """(buffer, r0, c0): a fresh output buffer in its sentinel band."""
        top, bottom, left, right = self.c_pad
        buf = np.full((self.M + top + bottom, self.N + left + right), GGEMM_SENTINEL, dtype=np.float64)
        buf[top:top + self.M, left:left + self.N] = self.C0 if self.accumulate else np.nan
        return buf, top, left


def ggemm_reference(inst, dtype=np.float64):
    """R = sum_p A_p B_p + sum_q alpha_q S_q (+ C0) in plain numpy at `dtype`, S = the same sum over magnitudes, n = terms per element."""
    R, S, n = np.zeros((inst.M, inst.N), dtype=dtype), np.zeros((inst.M, inst.N), dtype=dtype), 0
    for kind, K, A, B, alpha in inst.prods:
        if kind == 1:
            R = R + dtype(alpha) * B.view.astype(dtype)
            S = S + abs(dtype(alpha)) * np.abs(B.view.astype(dtype))
            n += 1
        else:
            R = R + A.view.astype(dtype) @ B.view.astype(dtype)
            S = S + np.abs(A.view.astype(dtype)) @ np.abs(B.view.astype(dtype))
            n += K
    if inst.accumulate:
        R, S, n = R + inst.C0.astype(dtype), S + np.abs(inst.C0.astype(dtype)), n + 1
    return R, S, n


def ggemm_bound(S_abs, n):
    """|got - R| <= 2 (n + 2) eps S, element by element.  A sum of n products evaluated in ANY order, with or without fused
    multiply-adds, is within gamma_n S of the exact value, gamma_n = n u / (1 - n u) with u = eps / 2 (Higham, Accuracy and Stability of
    Numerical Algorithms, section 3.1); (n + 2) eps lies above gamma_n for every n < 2^50, and it is taken once for the kernel and once
    for the numpy reference.  Derived, not measured."""
    return 2.0 * (n + 2) * np.finfo(np.float64).eps * np.asarray(S_abs, dtype=np.float64)


def ggemm_violations(got, R, S_abs, n):
    """Boolean M x N array: the elements of `got` outside the bound (a NaN is outside)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == R.shape, (got.shape, R.shape)
    return ~(np.abs(got - R) <= ggemm_bound(S_abs, n))


def ggemm_check(got, inst, what=""):
    """Asserts that `got` is the result of `inst` within the bound at every element; returns the worst |got - R| / bound (0 for 0 / 0)."""
    bad = ggemm_violations(got, inst.R, inst.S_abs, inst.n)
    if bad.any():
        i, j = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements outside the bound, first at (%d, %d): got %r, want %r, bound %.3e (M=%d N=%d n=%d)"
                             % (what, int(bad.sum()), bad.size, i, j, float(np.asarray(got)[i, j]), float(inst.R[i, j]),
                                float(ggemm_bound(inst.S_abs, inst.n)[i, j]), inst.M, inst.N, inst.n))
    bound = ggemm_bound(inst.S_abs, inst.n)
    err = np.abs(np.asarray(got, dtype=np.float64) - inst.R)
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0))) if err.size else 0.0


# ---- Krylov kernels: odd lengths, several workgroups, planted spectra (tests/test_krylov_inputs.py, tests/test_gpu_krylov_shapes.py) ----
# kept-sector tables {Sz: states} (left, right) that give these state counts at Ly = 2 (12 terms, 4 KronBlocks)
KRYLOV_KEPT = {845: ({1: 3, 0: 8, -1: 2}, {1: 29, 0: 17, -1: 10}),
               1205: ({1: 35, 0: 2, -1: 6}, {1: 34, 0: 5, -1: 7}),
               2049: ({1: 4, 0: 4, -1: 19}, {1: 18, 0: 27, -1: 38}),          # two 2048-element workgroups of the Lanczos run, the second of one element
               4097: ({1: 3, 0: 35, -1: 26}, {1: 27, 0: 16, -1: 4})}          # three
TINY_GAP_EPS = 5e-3                    # scale of the terms put back on the degenerate input: (w1 - w0) / (w_max - w0) = 1.04e-3


def krylov_superblock(wl, n_states):
    sb = wl.synthetic_superblock("cfg2", Ly=2, seed=7, kept=KRYLOV_KEPT[n_states])
    assert sb.n_states == n_states and len(sb.terms) == 12 and len(sb.blocks) == 4
    return sb


def dense_hamiltonian(wl, sb):
    """(H, eigenvalues, eigenvectors) of a superblock, H column by column through the numpy statement of the factored apply; read-only."""
    H = np.stack([wl.apply_factored_numpy(sb, e) for e in np.eye(sb.n_states)], axis=1)
    w, v = np.linalg.eigh(H)
    for a in (H, w, v):
        a.setflags(write=False)
    return H, w, v


def _planted_block_hamiltonians(wl, terms_scale):
    """The 845-state layout with H_L and H_R replaced by Q diag(lambda) Q^T per sector (Q random orthogonal): lambda in [0, 4] except the
    lowest of the sectors of KronBlocks 1 and 2, which are -2 + -1.5 and -1.25 + -2.25: both sums are -3.5 exactly, every other sum
    lambda_L + lambda_R of a KronBlock is >= -2.25.  The terms are dropped (terms_scale None) or scaled."""
    sb = krylov_superblock(wl, 845)
    rng = np.random.default_rng(23)
    (ia, ja), (ib, jb) = sb.blocks[1], sb.blocks[2]
    low_left, low_right = {ia: -2.0, ib: -1.25}, {ja: -1.5, jb: -2.25}
    for op, sizes, low in ((sb.h_left, sb.left_sizes, low_left), (sb.h_right, sb.right_sizes, low_right)):
        for c in op.cells:
            assert c.kind == CELL_DENSE and c.r0 == 0 and c.c0 == 0 and c.nr == c.nc == sizes[c.row_sector]
            q, _ = np.linalg.qr(rng.standard_normal((c.nr, c.nr)))
            lam = rng.uniform(0.0, 4.0, c.nr)
            lam[0] = low.get(c.row_sector, 0.0)
            a = (q * lam) @ q.T
            c.array = np.ascontiguousarray((a + a.T) * 0.5)
    sb.terms = [] if terms_scale is None else [(terms_scale * t[0],) + tuple(t[1:]) for t in sb.terms]
    return sb


def planted_superblock(wl, kind):
    """'posdef': the 845-state input with c = |w_min| + 3 added to the diagonal of every cell of H_L, which shifts the whole spectrum by c:
    the lowest eigenvalue is +3 and the eigenvalue of largest magnitude is at the top.  'degenerate': no terms, block Hamiltonians with
    planted spectra, a twofold ground state at -3.5 with the third eigenvalue 1.25 above.  'tinygap': the same with the terms put back,
    scaled by TINY_GAP_EPS, which splits the pair by 1e-3 of the spectrum's width."""
    if kind == "posdef":
        sb = krylov_superblock(wl, 845)
        w_min = dense_hamiltonian(wl, sb)[1][0]
        for c in sb.h_left.cells:
            assert c.kind == CELL_DENSE and c.nr == c.nc
            c.array = np.ascontiguousarray(c.array + (abs(w_min) + 3.0) * np.eye(c.nr))
        return sb
    return _planted_block_hamiltonians(wl, {"degenerate": None, "tinygap": TINY_GAP_EPS}[kind])


_KRYLOV_INPUTS = {}


def krylov_input(wl, key):
    """(superblock, dense H, eigenvalues, eigenvectors) of the dense-size inputs, built once per process and read-only: 845, 1205 (odd state
    counts), 'cfg2' (the even 844-state superblock of the Lanczos tests) and the three planted spectra."""
    if key not in _KRYLOV_INPUTS:
        if key == "cfg2":
            sb = wl.synthetic_superblock("cfg2", m=32, Ly=3, seed=3)
        else:
            sb = krylov_superblock(wl, key) if isinstance(key, int) else planted_superblock(wl, key)
        _KRYLOV_INPUTS[key] = (sb,) + dense_hamiltonian(wl, sb)
    return _KRYLOV_INPUTS[key]


class FactoredH:
    """The superblock Hamiltonian as an operator for the sizes at which nobody wants it dense: H @ x for a vector, H @ X for the columns of X."""

    def __init__(self, wl, sb):
        self.wl, self.sb, self.shape = wl, sb, (sb.n_states, sb.n_states)

    def __matmul__(self, x):
        x = np.asarray(x)
        if x.ndim == 1:
            return self.wl.apply_factored_numpy(self.sb, x)
        return np.stack([self.wl.apply_factored_numpy(self.sb, np.ascontiguousarray(c)) for c in x.T], axis=1)


def lanczos_reorth(H, v0, K):
    """Lanczos with full reorthogonalisation (twice) against every earlier vector.  H: anything with H @ vector."""
    Q = [v0 / np.linalg.norm(v0)]
    alpha, beta = [], []
    for j in range(K):
        x = H @ Q[j] - (beta[j - 1] * Q[j - 1] if j else 0.0)
        alpha.append(Q[j] @ x)
        x = x - alpha[j] * Q[j]
        for _ in range(2):
            for q in Q:
                x = x - (q @ x) * q
        beta.append(np.linalg.norm(x))
        Q.append(x / beta[j])
    return v0 @ v0, np.array(alpha), np.array(beta)


def lanczos_tridiag(alpha, beta):
    K = len(alpha)
    return np.diag(alpha) + np.diag(beta[:K - 1], 1) + np.diag(beta[:K - 1], -1)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def lanczos_basis_invariants(plan, H, v0, K, V=None, ref=None):
    """One dmrgx_kron_lanczos_basis run, twice: coefficients against numpy to 1e-10 max |alpha|, V V^T = 1 to 1e-12 and V H V^T = T to
    1e-12 |H|, the same bits from both runs, v0 untouched.  H: the dense matrix, or a FactoredH -- then |H| is the largest |Ritz value|
    of the numpy reference's own T, a lower bound of |H|.  ref: lanczos_reorth(H, v0, K) where the caller has it already.  The second run
    goes into a new contiguous V, whatever the layout of the first.  Returns (norm2, alpha, beta) of the device."""
    import torch
    n = H.shape[0]
    n2, a, b = ref if ref is not None else lanczos_reorth(H, v0, K)
    normH = np.linalg.norm(H, 2) if isinstance(H, np.ndarray) else np.abs(np.linalg.eigvalsh(lanczos_tridiag(a, b))).max()
    v0d = torch.from_numpy(v0).cuda()
    norm2, alpha, beta, done, Vd = plan.lanczos_basis(v0d, K, V=V)
    Vh = Vd.cpu().numpy()[:, :n].copy()
    norm2b, alphab, betab, doneb, Vb = plan.lanczos_basis(v0d, K)
    Vhb = Vb.cpu().numpy()
    tol = 1e-10 * np.abs(a).max()
    T = lanczos_tridiag(alpha, beta)
    orth, galerkin = np.abs(Vh @ Vh.T - np.eye(K)).max(), np.abs(Vh @ (H @ Vh.T) - T).max()
    print("n", n, "K", K, "norm2 err", abs(norm2 - n2), "alpha err", np.abs(alpha - a).max(), "beta err", np.abs(beta[:K - 1] - b[:K - 1]).max(), "tol", tol,
          "|VV^T - 1|", orth, "|VHV^T - T|", galerkin, "|H|", normH)
    assert done == K and np.isfinite(alpha).all() and np.isfinite(beta).all() and np.isfinite(Vh).all()
    assert abs(norm2 - n2) <= tol
    assert np.abs(alpha - a).max() <= tol and np.abs(beta[:K - 1] - b[:K - 1]).max() <= tol
    assert orth <= 1e-12
    assert galerkin <= 1e-12 * normH
    assert norm2 == norm2b and done == doneb
    assert np.array_equal(_bits(alpha), _bits(alphab)) and np.array_equal(_bits(beta), _bits(betab)) and np.array_equal(_bits(Vh), _bits(Vhb))
    assert np.array_equal(_bits(v0d.cpu().numpy()), _bits(v0))
    return norm2, alpha, beta


# ---- density-matrix eigensolver: planted tridiagonals, clusters, edges (tests/test_rdm_inputs.py, tests/test_gpu_rdm_spectra.py) ----
# The constants of csrc/symeig*.hip / symeig*.h the inputs and the order lists were built around; test_rdm_inputs.py parses the sources and
# fails when one of them is retuned.
RDM_CONSTANTS = {"DMRGX_DC_LEAF": 16, "DC_FUSE_NL": 384, "DMRGX_WY_NB": 64, "TRID_MAXM": 32, "TRID_PF": 8, "SYMEIG_MAX_N": 3072,
                 # the block-Jacobi solver of csrc/rdm_jacobi.hip and its QR preconditioner (csrc/hqr.hip): the Jacobi block (matrices are padded to
                 # two of them), the rows up to which a QR panel lives in registers at 4 / 8 / 16 rows per thread (above HR_MAX_ROWS:
                 # hqr_panel_kernel), the panel width and the column strip of the trailing update
                 "DMRGX_JB": 16, "HQR_REGS_ROWS_4": 256, "HQR_REGS_ROWS_8": 512, "HR_MAX_ROWS": 1024, "HQR_PANEL": 32, "TM_COLS": 32}
RDM_LEAF = RDM_CONSTANTS["DMRGX_DC_LEAF"]
# orders above 40 at the edges of the solver: the tree's halving (63 .. 66, 127 .. 131, 511 .. 514, 1024, 1025), the fused / split Loewner
# kernels (a top merge of DC_FUSE_NL = 384 +- 1; 768 and 769: level-1 merges of 384 and 385), the last partial WY block (n - 2 = 64 q + r with
# r = 0, 1, 63) and the 512-column prefetch chunk of the launch-per-column kernel (TRID_PF chunks of 64)
RDM_EDGE_ORDERS = [63, 64, 65, 66, 127, 128, 129, 130, 131, 383, 384, 385, 511, 512, 513, 514, 768, 769, 1024, 1025]
RDM_EDGE_CALLS = [[63, 64, 65, 66, 127, 128, 129, 130, 131, 383, 384, 385], [511, 512, 513, 514], [768, 769], [1024, 1025]]
# the orders at which the QR preconditioner of the block-Jacobi solver changes its panel body (the rows left in the first panel are the
# order itself): registers with 4 / 8 rows per thread at 256, 8 / 16 at 512, registers / hqr_panel_kernel at HR_MAX_ROWS = 1024.  An order
# that is no multiple of 32 ends in a panel narrower than 32 and a partial strip of the trailing update; 1025 walks through all four bodies.
RDM_HQR_EDGE_CALLS = [[255, 256, 257, 258], [511, 512, 513, 514], [1024, 1025]]
# the automatic switch: the smallest order above SYMEIG_MAX_N, and next to it an order between HR_MAX_ROWS and that, so that both panel
# kernels of hqr_batched are launched for the same rows
RDM_SWITCH_SHAPES = [(3073, 24), (1100, 60)]


def rdm_tree_bounds(n, leaf=RDM_LEAF):
    """(depth, node boundaries at that depth) of the divide-and-conquer tree: repeated halving until every leaf is at most `leaf`."""
    depth = 0
    while -(-n // (1 << depth)) > leaf:
        depth += 1
    b = [0, n]
    for _ in range(depth):
        b = [x for lo, hi in zip(b[:-1], b[1:]) for x in (lo, (lo + hi) // 2)] + [n]
    return depth, b


def rdm_bidiag(a, b):
    """The state (flat, row-major) of a layout of one n x n KronBlock whose Psi is lower bidiagonal with diagonal a and subdiagonal b:
    rho_L = Psi Psi^T is tridiagonal with d_i = a_i^2 + b_{i-1}^2, e_i = a_i b_i and structural zeros elsewhere (rho_R = Psi^T Psi: d_i =
    a_i^2 + b_i^2, e_i = a_{i+1} b_i).  With dyadic a, b every entry is exact on any hardware.  Not normalised: the library does not need
    Tr rho = 1."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert b.shape == (len(a) - 1,)
    psi = (np.diag(a) + np.diag(b, -1)).ravel()
    psi.setflags(write=False)
    return psi


def _split_coupled(n, a_low):
    """Couplings only at the tree's split points s: a[s-1] = a_low, a[s] = 0.75, b[s-1] = 1, every other a = 1 and b = 0.  With a_low = 1.25,
    d[s-1] = d[s] = 1.5625 exactly: after Cuppen's rank-one tear both boundary entries are 0.3125, z is non-zero on these two equal poles only,
    one rotation merges them and ONE pole survives (k = 1).  With a_low = 1.5 the two differ (2.25, 1.5625) and two survive."""
    a, b = np.ones(n), np.zeros(n - 1)
    for s in rdm_tree_bounds(n)[1][1:-1]:
        a[s - 1], a[s], b[s - 1] = a_low, 0.75, 1.0
    return a, b


def _tridiag_cholesky(d, e):
    """Lower-bidiagonal Cholesky factor (diagonal, subdiagonal) of the SPD tridiagonal (d, e)."""
    n = len(d)
    a, b = np.zeros(n), np.zeros(n - 1)
    for i in range(n):
        t = d[i] - (b[i - 1] ** 2 if i else 0.0)
        assert t > 0.0
        a[i] = np.sqrt(t)
        if i < n - 1:
            b[i] = e[i] / a[i]
    return a, b


def glued_wilkinson(m, copies, glue, shift=1.5):
    """Psi = the Cholesky factor of `copies` Wilkinson matrices W_{2m+1} (diagonal |-m .. m|, off-diagonal 1) glued by `glue` and shifted by
    `shift` (W21's lowest eigenvalue is -1.125: positive definite): every eigenvalue of W comes `copies` times, split by ~glue, and the large
    ones in pairs that agree to 1e-14 already."""
    w = np.abs(np.arange(-m, m + 1)).astype(np.float64) + shift
    d = np.tile(w, copies)
    e = np.ones(len(d) - 1)
    e[2 * m::2 * m + 1] = glue
    return rdm_bidiag(*_tridiag_cholesky(d, e))


def _orth(rng, n):
    return np.linalg.qr(rng.standard_normal((n, n)))[0]


def _rdm_named(name):
    rng = np.random.default_rng(1729)
    if name in ("k1_20", "k1_40", "k2_20"):
        return rdm_bidiag(*_split_coupled(int(name[3:]), 1.25 if name[1] == "1" else 1.5))
    if name == "toeplitz121_100":
        return rdm_bidiag(np.ones(100), np.ones(99))
    if name == "zero_coupling_50":                       # split points of n = 50: 12, 25, 37; e = 0 behind rows 5 and 30
        i = np.arange(50)
        a, b = 1.0 + (i % 4) / 4.0, 0.5 + (i[:49] % 3) / 8.0
        b[5] = b[30] = 0.0
        return rdm_bidiag(a, b)
    if name == "diagonal_100":                           # 3 x 10 repeated values, 20 exact zeros, a tail of 50 down to 2^-50, shuffled
        a = np.concatenate([np.full(10, 1.0), np.full(10, 0.5), np.full(10, 0.25), np.zeros(20), 2.0 ** -np.arange(1.0, 51.0)])
        return rdm_bidiag(a[rng.permutation(100)], np.zeros(99))
    if name == "blockdiag_64":                           # dense blocks; no block edge (7, 23, 40, 41) is a split point of n = 64 (16, 32, 48)
        Psi, o = np.zeros((64, 64)), 0
        for p in (7, 16, 17, 1, 23):
            Psi[o:o + p, o:o + p] = np.round(rng.standard_normal((p, p)) * 64.0) / 256.0      # dyadic: the zero blocks of rho stay exact
            o += p
        return Psi.ravel()
    if name.startswith("glued_"):
        copies, glue = {"glued_6_1e-8": (6, 1e-8), "glued_6_1e-14": (6, 1e-14), "glued_12_1e-8": (12, 1e-8)}[name]
        return glued_wilkinson(10, copies, glue)
    if name == "clusters_200":                           # eight clusters of 25 eigenvalues of rho at 2^-c (1 + spread u), u in [0, 1)
        spreads = [0.0, 1e-16, 1e-14, 1e-12, 1e-10, 1e-8, 1e-6, 1e-4]
        lam = np.concatenate([2.0 ** -c * (1.0 + sp * np.arange(25) / 25.0) for c, sp in enumerate(spreads)])
        return ((_orth(rng, 200) * np.sqrt(lam)) @ _orth(rng, 200).T).ravel()
    if name == "graded_pairs_300":                       # s = exp(-0.5 i) in exactly equal pairs, rank 260: s down to 1e-56, s^2 to 1e-112
        s = np.exp(-0.5 * np.arange(300.0))
        s[1::2] = s[0::2]
        s[260:] = 0.0
        return ((_orth(rng, 300) * s) @ _orth(rng, 300).T).ravel()
    if name == "gaussian_100x60":                        # the control: what almost every other RDM test uses
        return rng.standard_normal(100 * 60)
    if name == "zero_90x70":                             # a block of the state that is exactly zero: rho = 0, every orthonormal basis is right
        return np.zeros(90 * 70)
    if name == "rank_one_90x70":
        return np.outer(rng.standard_normal(90), rng.standard_normal(70)).ravel()
    if name == "orth_48":                                # rho = 1 / 48 on both sides, up to rounding
        return (_orth(rng, 48) / np.sqrt(48.0)).ravel()
    if name in ("gaussian_40x33", "gaussian_1100x60"):
        rows, cols = (int(v) for v in name[len("gaussian_"):].split("x"))
        return rng.standard_normal(rows * cols)
    if name == "planted_3073x24":                        # Psi = U diag(s) V^T: rho_L has the eigenvalues s^2 = exp(-1.4 i) and 3049 zeros
        U = np.linalg.qr(rng.standard_normal((3073, 24)))[0]
        return ((U * RDM_PLANTED_S) @ _orth(rng, 24).T).ravel()
    raise KeyError(name)


RDM_TRIDIAGONALS = ["k1_20", "k1_40", "k2_20", "toeplitz121_100", "zero_coupling_50", "diagonal_100", "glued_6_1e-8", "glued_6_1e-14", "glued_12_1e-8"]
RDM_NAMED = RDM_TRIDIAGONALS + ["blockdiag_64", "clusters_200", "graded_pairs_300"]
# one state whose KronBlocks are exactly zero, of rank one, orthogonal / sqrt(n) and Gaussian (so that the call is not trivial)
RDM_SPECIAL = ["zero_90x70", "rank_one_90x70", "orth_48", "gaussian_40x33"]
# the call that switches to the block-Jacobi solver by itself (RDM_SWITCH_SHAPES); the singular values planted in its first block
RDM_SWITCH = ["planted_3073x24", "gaussian_1100x60"]
RDM_PLANTED_S = np.exp(-0.7 * np.arange(24.0))
RDM_PLANTED_S.setflags(write=False)
_RDM_INPUTS, _RDM_STATS = {}, {}


def rdm_input(name):
    """(rows, columns, Psi as a read-only matrix) of a named input; built once per process."""
    if name not in _RDM_INPUTS:
        import re
        psi = np.ascontiguousarray(_rdm_named(name), dtype=np.float64)
        shape = re.search(r"_(\d+)x(\d+)$", name)
        rows = int(shape.group(1)) if shape else int(round(np.sqrt(psi.size)))
        Psi = psi.reshape(rows, -1)
        Psi.setflags(write=False)
        _RDM_INPUTS[name] = (rows, Psi.shape[1], Psi)
    return _RDM_INPUTS[name]


def rdm_model_stats(rho, leaf=RDM_LEAF):
    """What the project's numpy model of the solver (tools/proto_trid_dc.py) does with rho: {"merges": [(n, k, rotations, longest rotation chain,
    all deflated), ...] (leaves' level first, the root last), "tau_zero": reflectors with tau == 0 (of n), "e_zero": couplings that are exactly 0
    (of n - 1), "w": the model's eigenvalues (ascending), "X": its eigenvectors (columns)}.  A merge with rotations >= 1 is one that the device
    sends through the sequential scan of dc_deflate_kernel and dc_rot_kernel."""
    import importlib.util
    import os
    import sys
    if "proto_trid_dc" not in sys.modules:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "proto_trid_dc.py")
        spec = importlib.util.spec_from_file_location("proto_trid_dc", path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules["proto_trid_dc"] = mod
        spec.loader.exec_module(mod)
    proto = sys.modules["proto_trid_dc"]
    d, e, VT, tau = proto.trid_pipeline(np.array(rho, dtype=np.float64))
    merges = []
    w, Z, _ = proto.stedc(d, e, leaf=leaf, detail=merges)
    return {"merges": merges, "tau_zero": int(np.sum(tau == 0.0)), "e_zero": int(np.sum(e == 0.0)), "n": len(d),
            "w": w, "X": proto.backtransform(VT, tau, Z, nb=RDM_CONSTANTS["DMRGX_WY_NB"])}


def rdm_named_stats(name):
    """rdm_model_stats of rho_L of a named input, once per process."""
    if name not in _RDM_STATS:
        Psi = rdm_input(name)[2]
        _RDM_STATS[name] = rdm_model_stats(Psi @ Psi.T)
    return _RDM_STATS[name]


def rdm_bounds(rho, w_ref):
    """(eigenvalue bound, residual bound) of a density matrix: the project's backward-stability constant c n eps with c n eps = 3e-15 n, on
    max |w| for the eigenvalues and on |rho|_2 (= max |w|, rho is symmetric) for rho U^T - U^T diag(w)."""
    n = rho.shape[0]
    return 3e-15 * n * np.abs(w_ref).max() + 1e-17, 3e-15 * n * np.abs(w_ref).max() + 1e-16


def rdm_jacobi_bounds(rho, w_ref):
    """The same pair under the block-Jacobi solver (the project's bounds for it, tests/test_gpu_kron.py::_rdm_check): its eigenvalues are
    Rayleigh quotients of the finished vectors and keep the bound of rdm_bounds; the residual is 1e-11 |rho|_F + 1e-16, ten times the
    solver's stop criterion off^2 <= 1e-24 total^2 (rdm_create_impl), which bounds the Frobenius norm of rho U^T - U^T diag(w) by
    1e-12 |rho|_F before rounding.  Both stay positive at rho = 0."""
    n = rho.shape[0]
    return 3e-15 * n * np.abs(w_ref).max() + 1e-17, 1e-11 * np.linalg.norm(rho) + 1e-16


RDM_ORTH_TOL = 1e-13          # rows of the eigenvector matrix, orders up to 1100

RDM_GRADED_LAYOUT = ([40, 130, 77, 5], [64, 33, 150, 9], [(0, 3), (1, 2), (2, 1), (3, 0)])
_RDM_GRADED = []


def rdm_graded_state():
    """(psi0, psi1, junk) of tests/test_gpu_kron.py::test_rdm_graded_spectrum_few_sweeps_and_warm_hints, same seed and sizes, draw by draw:
    a state whose KronBlocks (RDM_GRADED_LAYOUT) have the Schmidt values exp(-0.35 k) u_k, u_k in [0.5, 1] -- like a DMRG ground state --,
    a perturbation of it by 1e-4 max |psi0|, and one random orthogonal matrix per density matrix, {(side, k): n x n}, as a junk warm
    hint.  Built once per process, read-only."""
    if not _RDM_GRADED:
        rng = np.random.default_rng(3)
        lsz, rsz, blocks = RDM_GRADED_LAYOUT
        parts = []
        for a, b in blocks:
            U, _ = np.linalg.qr(rng.standard_normal((lsz[a], lsz[a])))
            V, _ = np.linalg.qr(rng.standard_normal((rsz[b], rsz[b])))
            k = min(lsz[a], rsz[b])
            s = np.exp(-0.35 * np.arange(k)) * rng.uniform(0.5, 1.0, k)
            parts.append((U[:, :k] * s) @ V[:, :k].T)
        psi0 = np.concatenate([p.ravel() for p in parts])
        psi0 /= np.linalg.norm(psi0)
        psi1 = psi0 + 1e-4 * rng.standard_normal(psi0.size) * np.abs(psi0).max()
        psi1 /= np.linalg.norm(psi1)
        sizes = {(side, k): (lsz[a], rsz[b])[side] for k, (a, b) in enumerate(blocks) for side in (0, 1)}      # (the test's order: k, then side)
        junk = {key: np.ascontiguousarray(np.linalg.qr(rng.standard_normal((n, n)))[0]) for key, n in sizes.items()}
        for a in [psi0, psi1] + list(junk.values()):
            a.setflags(write=False)
        _RDM_GRADED.append((psi0, psi1, junk))
    return _RDM_GRADED[0]


def rdm_ratios(rho, w, U, w_ref=None, jacobi=False):
    """(eigenvalue error / its bound, residual / its bound, orthogonality error) of eigenvalues w (descending) and eigenvectors U (rows)
    against numpy's eigvalsh of rho, with the bounds of the direct solver or of the block-Jacobi solver."""
    if w_ref is None:
        w_ref = np.linalg.eigvalsh(rho)[::-1]
    be, br = (rdm_jacobi_bounds if jacobi else rdm_bounds)(rho, w_ref)
    c = U.shape[0]
    return (np.abs(w - w_ref).max() / be, np.abs(rho @ U.T - U.T * w[:c]).max() / br, np.abs(U @ U.T - np.eye(c)).max())
