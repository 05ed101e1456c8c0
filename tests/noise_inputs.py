"""Inputs and the numpy restatement of dmrgx_kron_noise_expand, shared by tests/test_gpu_noise_expand.py and tests/test_gpu_noise_rdm.py.

The restatement is written from the definition in include/dmrgx.h with dense per-sector operator blocks and explicit loops: block k of
the expansion is Psi_k followed, for every operator a in ascending order and every source KronBlock k' in ascending order whose sector
on `side` minus shift_a is that of k, by the panel coef[a] A_a Psi_k' (side 0, further columns) or coef[a] Psi_k' B_a^T (side 1, rows).

The planted superblock: left sectors (1, 3, 65, 7, 2), right sectors (2, 64, 5, 1, 66) -- one sector of a single state, one of exactly
64, and 65 / 66 just across the 64-wide tile --, psi on the KronBlocks IL + IR = 4 WITHOUT (3, 1): left sector 3 and right sector 1
exist but carry no KronBlock, so a source that a shift sends there contributes nothing.  Psi of KronBlock (2, 2) is 65 x 5: rho_L of left
sector 2 has rank 5 before the panels raise it."""
import numpy as np

LSZ, RSZ = [1, 3, 65, 7, 2], [2, 64, 5, 1, 66]
BLOCKS = [(0, 4), (1, 3), (2, 2), (4, 0)]
N_STATES = sum(LSZ[a] * RSZ[b] for a, b in BLOCKS)
COEF = [0.5, 1.25, -0.75, 0.0, 2.0]
ZERO_OP = 3                       # the operator with coef == 0
SIZES = (LSZ, RSZ)


def case(wl, side):
    """-> (psi, ops) of one side: [shift 0 with an IDENT cell beside a DENSE cell in one sector block, shift +1, the same stored cells read
    transposed (shift -1), a shift +1 operator that gets coef 0, shift +4 (from every source but the last sector it falls off the table)].
    The shift +1 operator sends the source in the last sector to the sector without a KronBlock (left) / reaches it from there (right),
    and falls off the table from sector 0."""
    rng = np.random.default_rng(2024 + side)
    D, I = wl.CELL_DENSE, wl.CELL_IDENT
    sz = SIZES[side]

    def dense(q, shift):
        return wl.OpCell(q, 0, 0, sz[q], sz[q + shift], D, 0.0, rng.standard_normal((sz[q], sz[q + shift])) / np.sqrt(sz[q + shift]))

    big = 2 if side == 0 else 1                                   # the sector of 65 (64) states: identity on [0, 33), dense on the rest
    rest = sz[big] - 33
    cells0 = [wl.OpCell(0, 0, 0, sz[0], sz[0], I, -1.1),
              wl.OpCell(big, 0, 0, 33, 33, I, 0.7), wl.OpCell(big, 33, 33, rest, rest, D, 0.0, rng.standard_normal((rest, rest)) / 6.0)]
    cells0 += [dense(q, 0) for q in range(1, 5) if q != big and not (side == 0 and q == 4)]      # (left: the last sector has no cell: a panel of zeros)
    op0 = wl.SectorOperator(0, cells0)
    plus = wl.SectorOperator(+1, [dense(q, +1) for q in range(4)])
    other = wl.SectorOperator(+1, [dense(q, +1) for q in range(4)])
    far = wl.SectorOperator(+4, [dense(0, +4)])
    ops = [op0, plus, (plus, True), other, far]
    psi = rng.standard_normal(N_STATES)
    return psi, ops


def psi_blocks(psi):
    out, o = [], 0
    for a, b in BLOCKS:
        out.append(np.asarray(psi[o:o + LSZ[a] * RSZ[b]]).reshape(LSZ[a], RSZ[b]))
        o += LSZ[a] * RSZ[b]
    return out


def shift_of(op):
    return -op[0].shift if isinstance(op, tuple) else op.shift


def op_block(op, sizes, q):
    """The dense block (row sector q -> column sector q + shift) of an operator AS USED, or None where that column sector does not exist."""
    op, transposed = op if isinstance(op, tuple) else (op, False)
    shift = -op.shift if transposed else op.shift
    if not 0 <= q + shift < len(sizes):
        return None
    M = np.zeros((sizes[q], sizes[q + shift]))
    for c in op.cells:
        cell = c.array if c.kind == 1 else c.scale * np.eye(c.nr)
        if not transposed and c.row_sector == q:
            M[c.r0:c.r0 + c.nr, c.c0:c.c0 + c.nc] += cell
        if transposed and c.row_sector + op.shift == q:               # stored (q' -> q' + s): used as (q' + s -> q')
            M[c.c0:c.c0 + c.nc, c.r0:c.r0 + c.nr] += cell.T
    return M


def model_panels(psi, side, ops, coef):
    """-> per KronBlock k the list [(a, k', panel)] in the order of the definition."""
    X = psi_blocks(psi)
    sec = [b[side] for b in BLOCKS]
    out = []
    for k in range(len(BLOCKS)):
        lst = []
        for a, op in enumerate(ops):
            for ks in range(len(BLOCKS)):
                if sec[ks] - shift_of(op) != sec[k]:
                    continue
                A = op_block(op, SIZES[side], sec[k])
                lst.append((a, ks, coef[a] * (A @ X[ks]) if side == 0 else coef[a] * (X[ks] @ A.T)))
        out.append(lst)
    return out


def model_expand(psi, side, ops, coef):
    """-> (blocks of the expansion as matrices, extent, n_out)."""
    X = psi_blocks(psi)
    mats = []
    for k, lst in enumerate(model_panels(psi, side, ops, coef)):
        parts = [X[k]] + [p for _, _, p in lst]
        mats.append(np.concatenate(parts, axis=1 if side == 0 else 0))
    extent = [m.shape[1 - side] for m in mats]
    return mats, extent, sum(m.size for m in mats)


def model_rho(psi, side, ops, coef):
    """Per KronBlock k the perturbed density matrix of `side`, built WITHOUT the expansion: Psi Psi^T + sum coef^2 (A Psi')(A Psi')^T."""
    X = psi_blocks(psi)
    out = []
    for k, lst in enumerate(model_panels(psi, side, ops, [1.0] * len(ops))):
        rho = X[k] @ X[k].T if side == 0 else X[k].T @ X[k]
        for a, _, img in lst:
            rho = rho + coef[a] ** 2 * (img @ img.T if side == 0 else img.T @ img)
        out.append(rho)
    return out
