"""Host-side handle of the HIP superblock plan, mirroring the reference's shell-matrix life cycle:

    KronBlocks_t::KronSumConstruct(Terms, H)  ->  KronPlan(superblock)          (src/DMRGKron.cpp:759-841,1871-1917)
    MatMult(H, x, y)                          ->  KronPlan.apply(x, y)          (src/DMRGKron.cpp:1827-1869)
    MatDestroy_KronSumShell(&H)               ->  KronPlan.destroy()            (src/DMRGKron.cpp:1919-1942)
    EPSSolve(H) (EPS_HEP, SMALLEST_REAL)      ->  KronPlan.eigs_lowest()        (include/DMRGBlockContainer.hpp:1488-1499)

torch is used only to own device memory and streams; every computation goes through the C ABI (_capi).
"""
import ctypes as C

import numpy as np
import torch

from . import _capi
from .workloads import OpSm, OpSz, OpSp, CELL_DENSE, CELL_IDENT


def _i32(values):
    arr = (C.c_int32 * len(values))(*[int(v) for v in values])
    return arr


def _rows_arg(T, n):
    """(count, pointer, row_stride) of an optional 2-D f64 device tensor of rows of at least n elements with unit stride along the row."""
    if T is None:
        return 0, C.c_void_p(), 0
    assert T.dtype == torch.float64 and T.dim() == 2 and T.shape[1] >= n and (T.shape[1] <= 1 or T.stride(1) == 1)
    return T.shape[0], C.c_void_p(T.data_ptr()), T.stride(0) if T.shape[0] > 1 else max(T.stride(0), T.shape[1])


class KronPlan:
    def __init__(self, sb, device="cuda:0", world_size=1, rank=0, stream=None):
        _capi.require_device()          # fails loudly without a GPU: no CPU fallback
        self.sb = sb
        self.device = torch.device(device)
        self._keep = []                 # ctypes arrays + device tensors that must outlive plan creation
        L = _capi.lib()

        def secop(op, transposed=False, shift=None):
            cells = (_capi.Cell * max(len(op.cells), 1))()
            for i, c in enumerate(op.cells):
                cells[i].row_sector, cells[i].r0, cells[i].c0, cells[i].nr, cells[i].nc = c.row_sector, c.r0, c.c0, c.nr, c.nc
                cells[i].kind, cells[i].scale = c.kind, c.scale
                if c.kind == CELL_DENSE:
                    t = torch.from_numpy(np.ascontiguousarray(c.array, dtype=np.float64)).to(self.device)
                    self._keep.append(t)
                    cells[i].data, cells[i].ld = t.data_ptr(), c.nc
            self._keep.append(cells)
            s = _capi.SecOp()
            s.shift = op.shift if shift is None else shift
            s.transposed = 1 if transposed else 0
            s.ncells = len(op.cells)
            s.cells = cells
            return s

        # distinct (op, site) operators per side in term order; Sm(i) = transposed Sp(i) (never materialised)
        def side(ops, which):
            index, lst = {}, []
            for t in sb.terms:
                key = (t[1], t[2]) if which == 0 else (t[3], t[4])
                if key in index:
                    continue
                op, site = key
                if op == OpSm:
                    lst.append(secop(ops[(OpSp, site)], transposed=True, shift=-1))
                else:
                    lst.append(secop(ops[(op, site)]))
                index[key] = len(lst) - 1
            arr = (_capi.SecOp * max(len(lst), 1))(*lst)
            self._keep.append(arr)
            return index, arr, len(lst)

        li, larr, nl = side(sb.left_ops, 0)
        ri, rarr, nr = side(sb.right_ops, 1)
        terms = (_capi.Term * max(len(sb.terms), 1))()
        for i, t in enumerate(sb.terms):
            terms[i].a, terms[i].left_op, terms[i].right_op = t[0], li[(t[1], t[2])], ri[(t[3], t[4])]
        hl = secop(sb.h_left) if sb.h_left is not None else None          # (None: no H_L / H_R term, a NULL in the descriptor)
        hr = secop(sb.h_right) if sb.h_right is not None else None
        d = _capi.KronDesc()
        ls, rs = _i32(sb.left_sizes), _i32(sb.right_sizes)
        bil, bir = _i32([b[0] for b in sb.blocks]), _i32([b[1] for b in sb.blocks])
        d.left.nsec, d.left.size = len(sb.left_sizes), ls
        d.right.nsec, d.right.size = len(sb.right_sizes), rs
        d.nblocks, d.block_il, d.block_ir = len(sb.blocks), bil, bir
        d.n_left_ops, d.n_right_ops, d.left_ops, d.right_ops = nl, nr, larr, rarr
        d.h_left = C.pointer(hl) if hl is not None else None
        d.h_right = C.pointer(hr) if hr is not None else None
        d.nterms, d.terms = len(sb.terms), terms
        d.world_size, d.rank = world_size, rank
        self._handle = C.c_void_p()
        st = self._stream_ptr(stream)
        with torch.cuda.device(self.device):
            _capi.check(L.dmrgx_kron_plan_create(C.byref(d), st, C.byref(self._handle)))
        self._keep.clear()              # the plan owns copies of every operator
        info = _capi.KronInfo()
        _capi.check(L.dmrgx_kron_plan_info(self._handle, C.byref(info)))
        self.info = info
        self.world_size, self.rank = world_size, rank

    @staticmethod
    def _stream_ptr(stream):
        if stream is None:
            stream = torch.cuda.current_stream()
        return C.c_void_p(stream.cuda_stream)

    def new_vector(self):
        return torch.zeros(self.info.vec_len, dtype=torch.float64, device=self.device)

    def apply(self, x_full, y_local, stream=None):
        """y_local <- (H x_full)[this rank's segment]  ==  MatMult_KronSumShell."""
        assert x_full.dtype == torch.float64 and y_local.dtype == torch.float64
        assert x_full.numel() >= self.info.vec_len and y_local.numel() >= self.info.local_len
        _capi.check(_capi.lib().dmrgx_kron_apply(self._handle, C.c_void_p(x_full.data_ptr()), C.c_void_p(y_local.data_ptr()),
                                                 self._stream_ptr(stream)))

    def to_striped(self, v_ref, v_full, stream=None):
        _capi.check(_capi.lib().dmrgx_kron_vec_to_striped(self._handle, C.c_void_p(v_ref.data_ptr()), C.c_void_p(v_full.data_ptr()),
                                                          self._stream_ptr(stream)))

    def from_striped(self, v_full, v_ref, stream=None):
        _capi.check(_capi.lib().dmrgx_kron_vec_from_striped(self._handle, C.c_void_p(v_full.data_ptr()), C.c_void_p(v_ref.data_ptr()),
                                                            self._stream_ptr(stream)))

    def eigs_lowest(self, ncv=16, max_it=1000, tol=1e-8, seed=1, psi0=None, allgather=None, allreduce=None, stream=None,
                    max_matvec=0, comm=None, method=0, min_initial_norm2=0.0, gd_minv=0):
        """Lowest eigenpair (EPS_HEP / EPS_SMALLEST_REAL / nev=1).  Returns (e0, psi_full tensor, stats).

        max_matvec > 0 (benchmarks): run exactly that many Lanczos steps; non-convergence is then not an error.
        comm: a Communicator -- the solver then issues its RCCL collectives itself (no Python inside the solve); the
        allgather/allreduce callbacks are the harness alternative."""
        opts = _capi.EigsOpts()
        opts.ncv, opts.max_it, opts.tol, opts.seed, opts.max_matvec = ncv, max_it, tol, seed, max_matvec
        psi = self.new_vector()
        if psi0 is not None:
            psi.copy_(psi0)
            opts.use_initial = 1
        self._cb = (_capi.ALLGATHER_FN(allgather) if allgather else _capi.ALLGATHER_FN(),
                    _capi.ALLREDUCE_FN(allreduce) if allreduce else _capi.ALLREDUCE_FN())
        opts.allgather, opts.allreduce_sum = self._cb
        opts.comm = comm.handle if comm is not None else None
        opts.method = method            # 0: thick-restart Lanczos, 1: generalized Davidson (diagonal preconditioner)
        opts.gd_minv = gd_minv          # method 1: Ritz vectors kept at a restart beside the previous Ritz vector (0: default 1)
        opts.min_initial_norm2 = min_initial_norm2      # > 0: psi0 is dropped (stats.start_rejected) when |psi0|^2 is below this
        e0 = C.c_double(0.0)
        stats = _capi.EigsStats()
        rc = _capi.lib().dmrgx_eigs_lowest(self._handle, C.byref(opts), C.byref(e0), C.c_void_p(psi.data_ptr()),
                                           C.byref(stats), self._stream_ptr(stream))
        if not (rc == _capi.DMRGX_ERR_NOTCONV and max_matvec > 0):
            _capi.check(rc)
        return e0.value, psi, stats

    def eigs_lowest_orth(self, Q, ncv=16, max_it=1000, tol=1e-8, seed=1, psi0=None, min_initial_norm2=0.0, stream=None):
        """Lowest eigenpair of P H P on the complement of the rows of Q (dmrgx_eigs_lowest_orth): the next excited state of the sector
        when Q holds the states already found.  Q: None (no row: the call forwards to dmrgx_eigs_lowest), or a 2-D f64 device tensor of
        nq rows with unit stride along the vector (its row stride is the library's ldq), only read.  psi0: a start vector, projected
        against Q by the library.  Returns (e, psi, stats); psi is orthogonal to Q."""
        nq, q_ptr, ldq = _rows_arg(Q, self.info.n_states)
        opts = _capi.EigsOpts()
        opts.ncv, opts.max_it, opts.tol, opts.seed, opts.min_initial_norm2 = ncv, max_it, tol, seed, min_initial_norm2
        psi = self.new_vector()
        if psi0 is not None:
            psi.copy_(psi0)
            opts.use_initial = 1
        e, stats = C.c_double(0.0), _capi.EigsStats()
        _capi.check(_capi.lib().dmrgx_eigs_lowest_orth(self._handle, C.byref(opts), int(nq), q_ptr, int(ldq), C.byref(e), C.c_void_p(psi.data_ptr()),
                                                       C.byref(stats), self._stream_ptr(stream)))
        return e.value, psi, stats

    def lanczos_coeffs(self, v0, nsteps, breakdown_tol=0.0, stream=None):
        """Lanczos coefficients of H from the start vector v0 (dmrgx_kron_lanczos_coeffs): plain three-term recursion, device-resident,
        breakdown decided on the device.  v0: f64 device tensor of n_states (reference layout, only read).  Returns
        (norm2, alpha[nsteps], beta[nsteps], nsteps_done); after a breakdown T of order nsteps_done is the whole answer."""
        assert v0.dtype == torch.float64 and v0.is_contiguous() and v0.numel() >= self.info.n_states
        n = max(int(nsteps), 0)
        norm2, done = C.c_double(0.0), C.c_int32(0)
        alpha, beta = (C.c_double * max(n, 1))(), (C.c_double * max(n, 1))()
        _capi.check(_capi.lib().dmrgx_kron_lanczos_coeffs(self._handle, C.c_void_p(v0.data_ptr()), int(nsteps), float(breakdown_tol),
                                                          C.byref(norm2), alpha, beta, C.byref(done), self._stream_ptr(stream)))
        return norm2.value, np.array(alpha[:n]), np.array(beta[:n]), done.value

    def lanczos_basis(self, v0, nsteps, breakdown_tol=0.0, V=None, stream=None):
        """The Lanczos run of lanczos_coeffs with the basis kept and fully reorthogonalised (dmrgx_kron_lanczos_basis).  Returns
        (norm2, alpha[nsteps], beta[nsteps], nsteps_done, V): row j of V is q_j, the rows from nsteps_done on are zeros.  V: an f64 device
        tensor of nsteps rows whose elements are contiguous (its row stride is the library's ldv), any contents; None: a new nsteps x n_states."""
        assert v0.dtype == torch.float64 and v0.is_contiguous() and v0.numel() >= self.info.n_states
        n = max(int(nsteps), 0)
        if V is None:
            V = torch.empty((max(n, 1), self.info.n_states), dtype=torch.float64, device=v0.device)
        assert V.dtype == torch.float64 and V.dim() == 2 and V.shape[0] >= n and (V.shape[1] <= 1 or V.stride(1) == 1)
        norm2, done = C.c_double(0.0), C.c_int32(0)
        alpha, beta = (C.c_double * max(n, 1))(), (C.c_double * max(n, 1))()
        _capi.check(_capi.lib().dmrgx_kron_lanczos_basis(self._handle, C.c_void_p(v0.data_ptr()), int(nsteps), float(breakdown_tol),
                                                         C.c_void_p(V.data_ptr()), int(V.stride(0)), C.byref(norm2), alpha, beta, C.byref(done),
                                                         self._stream_ptr(stream)))
        return norm2.value, np.array(alpha[:n]), np.array(beta[:n]), done.value, V

    def chebyshev_moments(self, v0, centre, half_width, nsteps, U=None, stream=None):
        """Chebyshev moments of Ht = (H - centre) / half_width from the start vector v0 (dmrgx_kron_chebyshev_moments): t_0 = v0,
        t_1 = Ht t_0, t_{n+1} = 2 Ht t_n - t_{n-1}, device-resident, guarded on the device.  v0: f64 device tensor of n_states, only read.
        U: None, or a 2-D f64 device tensor of nu rows with unit stride along the vector (its row stride is the library's ldu), only read.
        Returns (norm2, mu_diag[2 nsteps + 1], mu_cross[nsteps + 1, nu], nsteps_done): mu_diag[m] = <v0, T_m(Ht) v0>,
        mu_cross[n, i] = <U[i], t_n>; beyond 2 nsteps_done and beyond row nsteps_done everything is zero."""
        assert v0.dtype == torch.float64 and v0.is_contiguous() and v0.numel() >= self.info.n_states
        K = max(int(nsteps), 0)
        nu, u_ptr, ldu = _rows_arg(U, self.info.n_states)
        norm2, done = C.c_double(0.0), C.c_int32(0)
        diag, cross = (C.c_double * (2 * K + 1))(), (C.c_double * max((K + 1) * nu, 1))()
        _capi.check(_capi.lib().dmrgx_kron_chebyshev_moments(self._handle, C.c_void_p(v0.data_ptr()), float(centre), float(half_width), int(nsteps), int(nu), u_ptr,
                                                             int(ldu), C.byref(norm2), diag, cross, C.byref(done), self._stream_ptr(stream)))
        return norm2.value, np.array(diag[:2 * K + 1]), np.array(cross[:(K + 1) * nu]).reshape(K + 1, nu), done.value

    def correction_vector(self, v0, sigma, eta, tol=0.0, max_it=1000, check_every=0, U=None, want_real=True, stream=None):
        """The correction vector 1 / (sigma + i eta - H) v0 = X + i Y (dmrgx_kron_correction_vector): conjugate gradients on
        (H - sigma)^2 + eta^2, device-resident, convergence |r| <= tol |b| decided on the device (tol 0: 1e-8), iterations enqueued in blocks
        of check_every (0: 8).  v0: f64 device tensor of n_states, only read.  U: None, or a 2-D f64 device tensor of nu rows with unit
        stride along the vector (its row stride is the library's ldu), only read.  want_real False: X is not formed.  Returns a dict: Y, X
        (device tensors; X None when not wanted), norm2 = |v0|^2, im[nu] = <U[i], Y>, re[nu] = <U[i], X> (None without X), and the fields of
        dmrgx_cv_stats: iterations, converged, n_matvec, dead, residual, true_residual.  Not converging within max_it is no error."""
        assert v0.dtype == torch.float64 and v0.is_contiguous() and v0.numel() >= self.info.n_states
        n = self.info.n_states
        nu, u_ptr, ldu = _rows_arg(U, n)
        Y = torch.empty(n, dtype=torch.float64, device=v0.device)
        X = torch.empty(n, dtype=torch.float64, device=v0.device) if want_real else None
        norm2, stats = C.c_double(0.0), _capi.CvStats()
        im, re = (C.c_double * max(nu, 1))(), (C.c_double * max(nu, 1))()
        _capi.check(_capi.lib().dmrgx_kron_correction_vector(self._handle, C.c_void_p(v0.data_ptr()), float(sigma), float(eta), float(tol), int(max_it), int(check_every),
                                                             C.c_void_p(Y.data_ptr()), C.c_void_p(X.data_ptr()) if want_real else C.c_void_p(), int(nu), u_ptr, int(ldu),
                                                             C.byref(norm2), im, re if want_real else None, C.byref(stats), self._stream_ptr(stream)))
        out = dict(Y=Y, X=X, norm2=norm2.value, im=np.array(im[:nu]), re=np.array(re[:nu]) if want_real else None)
        out.update({k: getattr(stats, k) for k, _ in _capi.CvStats._fields_})
        return out

    def static_response(self, p, v0, sigma, tol=0.0, max_it=1000, check_every=0, U=None, X=None, stream=None):
        """The static response X of v0 on the complement of p (dmrgx_kron_static_response): <p, X> = 0 and Q (H - sigma) Q X = Q v0 with
        Q = 1 - p p^T / <p, p>, by conjugate gradients with one MatMult per iteration, device-resident, convergence |r| <= tol |Q v0| decided
        on the device (tol 0: 1e-8), iterations enqueued in blocks of check_every (0: 8).  p, v0: f64 device tensors of n_states, only read.
        U: None, or a 2-D f64 device tensor of nu rows with unit stride along the vector (its row stride is the library's ldu), only read.
        X: None (a new tensor), or the contiguous f64 device tensor of n_states to write.  Returns a dict: X, coef = <p, v0> / <p, p>,
        norm2 = |Q v0|^2, chi[nu] = <U[i], X>, and the fields of dmrgx_cv_stats: iterations, converged, n_matvec, dead, residual,
        true_residual.  Not converging within max_it is no error."""
        n = self.info.n_states
        for w in (p, v0):
            assert w.dtype == torch.float64 and w.is_contiguous() and w.numel() >= n
        nu, u_ptr, ldu = _rows_arg(U, n)
        if X is None:
            X = torch.empty(n, dtype=torch.float64, device=v0.device)
        assert X.dtype == torch.float64 and X.is_contiguous() and X.numel() >= n
        coef, norm2, stats = C.c_double(0.0), C.c_double(0.0), _capi.CvStats()
        chi = (C.c_double * max(nu, 1))()
        _capi.check(_capi.lib().dmrgx_kron_static_response(self._handle, C.c_void_p(p.data_ptr()), C.c_void_p(v0.data_ptr()), float(sigma), float(tol), int(max_it),
                                                           int(check_every), C.c_void_p(X.data_ptr()), int(nu), u_ptr, int(ldu), C.byref(coef), C.byref(norm2), chi,
                                                           C.byref(stats), self._stream_ptr(stream)))
        out = dict(X=X, coef=coef.value, norm2=norm2.value, chi=np.array(chi[:nu]))
        out.update({k: getattr(stats, k) for k, _ in _capi.CvStats._fields_})
        return out

    def timing(self, enable):
        _capi.check(_capi.lib().dmrgx_kron_plan_timing(self._handle, 1 if enable else 0))

    def timing_read(self):
        """-> ([0, ms stage 1, 0, ms stage 2], applies recorded): slots 0 and 2 belong to 128 x 128 launches, which the MatMult does not make."""
        ms, n = (C.c_double * 4)(), C.c_int64(0)
        _capi.check(_capi.lib().dmrgx_kron_plan_timing_read(self._handle, ms, C.byref(n)))
        return list(ms), n.value

    def destroy(self):
        if self._handle:
            _capi.check(_capi.lib().dmrgx_kron_plan_destroy(self._handle))
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def dgemm_nn(A, B, out=None):
    """C = A @ B through the MFMA grouped-GEMM kernel (row-major f64 device tensors)."""
    assert A.dtype == torch.float64 and B.dtype == torch.float64 and A.is_contiguous() and B.is_contiguous()
    M, K = A.shape
    K2, N = B.shape
    assert K == K2
    if out is None:
        out = torch.empty((M, N), dtype=torch.float64, device=A.device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(_capi.lib().dmrgx_dgemm_nn(M, N, K, C.c_void_p(A.data_ptr()), K, C.c_void_p(B.data_ptr()), N,
                                           C.c_void_p(out.data_ptr()), N, st))
    return out


def vec_gram(U, V, accumulate=False, out=None):
    """G[i, j] (= | +=) <U[i, :], V[j, :]> through the MFMA Gram kernel (dmrgx_vec_gram).  U, V: 2-D f64 device tensors with unit stride
    along the vector (row stride >= length; views of larger buffers are fine).  Passing the same tensor twice takes the same-family
    path: one triangle computed, G bitwise symmetric.  Returns (G, report); G is `out` (any row stride >= nv) when given."""
    assert U.dtype == torch.float64 and V.dtype == torch.float64 and U.dim() == 2 and V.dim() == 2 and U.shape[1] == V.shape[1]
    (nu, n), nv = U.shape, V.shape[0]
    assert n == 0 or (U.stride(1) == 1 and V.stride(1) == 1)
    if out is None:
        assert not accumulate, "accumulate needs the matrix to add to"
        out = torch.empty((nu, nv), dtype=torch.float64, device=U.device)
    assert out.dtype == torch.float64 and out.shape == (nu, nv) and (nv == 1 or out.stride(1) == 1)
    ldu, ldv = (U.stride(0) if nu > 1 else max(n, 1)), (V.stride(0) if nv > 1 else max(n, 1))
    report = _capi.GramReport()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(_capi.lib().dmrgx_vec_gram(nu, nv, n, C.c_void_p(U.data_ptr()), ldu, C.c_void_p(V.data_ptr()), ldv, C.c_void_p(out.data_ptr()),
                                           out.stride(0) if nu > 1 else max(nv, 1), 1 if accumulate else 0, C.byref(report), st))
    return out, report


def vec_project_out(V, p):
    """V[a, :] -= coef[a] p with coef[a] = <V[a, :], p> / <p, p>, in place (dmrgx_vec_project_out).  V: a 2-D f64 device tensor with unit
    stride along the vector (row stride >= length; views of larger buffers are fine, the columns beyond the length are left alone);
    p: a contiguous 1-D f64 device tensor of that length, only read, not overlapping V.  Returns (coef[nv] as a numpy array, <p, p>);
    a p whose squared norm is not a positive finite number leaves V alone and returns zeros."""
    assert V.dtype == torch.float64 and p.dtype == torch.float64 and V.dim() == 2 and p.dim() == 1 and V.shape[1] == p.shape[0]
    nv, n = V.shape
    assert n <= 1 or (V.stride(1) == 1 and p.stride(0) == 1)
    ldv = V.stride(0) if nv > 1 else max(V.stride(0), n)
    coef, norm2 = (C.c_double * max(nv, 1))(), C.c_double(0.0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(_capi.lib().dmrgx_vec_project_out(nv, n, C.c_void_p(V.data_ptr()), ldv, C.c_void_p(p.data_ptr()), coef, C.byref(norm2), st))
    return np.array(coef[:nv]), norm2.value


def _gram_arguments(sb_or_layout, psi, left_ops, right_ops):
    """The arguments dmrgx_kron_op_gram and dmrgx_kron_term_gram share, as ctypes values: (sectors, sectors, nblocks, il, ir, psi pointer, n_left,
    left operators, n_right, right operators), psi as a device tensor, and the list that keeps every buffer behind them alive."""
    if hasattr(sb_or_layout, "blocks"):
        left_sizes, right_sizes, blocks = sb_or_layout.left_sizes, sb_or_layout.right_sizes, sb_or_layout.blocks
    else:
        left_sizes, right_sizes, blocks = sb_or_layout
    if not torch.is_tensor(psi):
        psi = torch.from_numpy(np.ascontiguousarray(psi, dtype=np.float64)).cuda()
    assert psi.dtype == torch.float64 and psi.is_contiguous()
    assert psi.numel() == sum(left_sizes[il] * right_sizes[ir] for il, ir in blocks)
    keep = []

    def secops(ops):
        lst = []
        for op in ops:
            op, transposed = op if isinstance(op, tuple) else (op, False)
            cells = (_capi.Cell * max(len(op.cells), 1))()
            for i, c in enumerate(op.cells):
                cells[i].row_sector, cells[i].r0, cells[i].c0, cells[i].nr, cells[i].nc = c.row_sector, c.r0, c.c0, c.nr, c.nc
                cells[i].kind, cells[i].scale = c.kind, c.scale
                if c.kind == CELL_DENSE:
                    t = torch.from_numpy(np.ascontiguousarray(c.array, dtype=np.float64)).to(psi.device)
                    keep.append(t)
                    cells[i].data, cells[i].ld = t.data_ptr(), c.nc
            keep.append(cells)
            s = _capi.SecOp()
            s.shift, s.transposed, s.ncells, s.cells = (-op.shift if transposed else op.shift), (1 if transposed else 0), len(op.cells), cells
            lst.append(s)
        arr = (_capi.SecOp * max(len(lst), 1))(*lst)
        keep.append(arr)
        return arr, len(lst)

    larr, nl = secops(left_ops)
    rarr, nr = secops(right_ops)
    ls, rs = _i32(left_sizes), _i32(right_sizes)
    sl, sr = _capi.Sectors(len(left_sizes), ls), _capi.Sectors(len(right_sizes), rs)
    bil, bir = _i32([b[0] for b in blocks]), _i32([b[1] for b in blocks])
    keep += [ls, rs, sl, sr, bil, bir]
    return (C.byref(sl), C.byref(sr), len(blocks), bil, bir, C.c_void_p(psi.data_ptr()), nl, larr, nr, rarr), psi, keep


def op_gram(sb_or_layout, psi, left_ops, right_ops, workspace_bytes=0):
    """G[a, b] = <O_a psi, O_b psi> for O_a = A_a (x) 1 (left_ops) and 1 (x) B_a (right_ops), left ones first (dmrgx_kron_op_gram): with
    Sz(i) of every site the whole table <Sz_i Sz_j>, with Sp(i) the table <Sm_i Sp_j>.  sb_or_layout: a Superblock or
    (left_sizes, right_sizes, blocks); psi: the state in the reference's vector layout (device tensor or numpy array).  An operator is a
    SectorOperator, or (SectorOperator, True) for its transpose (Sm(i) from the stored Sp(i)); all must carry the same shift as used.
    workspace_bytes bounds the storage of the images (0: 1 GiB).  Returns (G, report)."""
    _capi.require_device()
    args, psi, keep = _gram_arguments(sb_or_layout, psi, left_ops, right_ops)
    n = len(left_ops) + len(right_ops)
    G = torch.empty((max(n, 1), max(n, 1)), dtype=torch.float64, device=psi.device)
    report = _capi.GramReport()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(_capi.lib().dmrgx_kron_op_gram(*args, workspace_bytes, C.c_void_p(G.data_ptr()), max(n, 1), C.byref(report), st))
    torch.cuda.current_stream().synchronize()       # the operator copies in `keep` are read by the queued work
    return G, report


def term_gram(sb_or_layout, psi, left_ops, right_ops, vectors, workspace_bytes=0):
    """G[a, b] = <v_a, v_b> for v_a = sum over the terms (c, l, r) of vectors[a] of c * (left_ops[l] (x) right_ops[r]) psi
    (dmrgx_kron_term_gram); l or r None: the identity on that side, both None: c * psi.  With the bond operators S_i . S_j -- one operator
    of a block, or three two-sided terms across the cut -- the whole table of dimer-dimer correlations.  Layout, psi, operators
    (a SectorOperator, or (SectorOperator, True) for its transpose) and workspace_bytes as in op_gram; every term of the call must have
    the same total sector shift.  Returns (G, report)."""
    _capi.require_device()
    args, psi, keep = _gram_arguments(sb_or_layout, psi, left_ops, right_ops)
    n = len(vectors)
    first = _i32(list(np.cumsum([0] + [len(v) for v in vectors])))
    flat = [t for v in vectors for t in v]
    terms = (_capi.Term * max(len(flat), 1))()
    for i, (c, l, r) in enumerate(flat):
        terms[i].a, terms[i].left_op, terms[i].right_op = float(c), (-1 if l is None else int(l)), (-1 if r is None else int(r))
    G = torch.empty((max(n, 1), max(n, 1)), dtype=torch.float64, device=psi.device)
    report = _capi.GramReport()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(_capi.lib().dmrgx_kron_term_gram(*args, n, first, terms, workspace_bytes, C.c_void_p(G.data_ptr()), max(n, 1), C.byref(report), st))
    torch.cuda.current_stream().synchronize()       # the operator copies in `keep` are read by the queued work
    return G, report


def term_gram_states(sb_or_layout, Psi, left_ops, right_ops, vectors, workspace_bytes=0):
    """G[s * n + a, t * n + b] = <v_a(psi_s), v_b(psi_t)> for the rows psi_s of Psi and the n = len(vectors) images of term_gram built from
    each of them (dmrgx_kron_term_gram_states): the family is state-major.  Psi: a 2-D f64 device tensor (or numpy array) of one state
    per row in the reference vector layout, unit stride along the row and a row stride >= n_states whose columns beyond n_states are never
    read.  Layout, operators, vectors and workspace_bytes as in term_gram; the workspace holds the images of every state.
    Returns (G, report)."""
    _capi.require_device()
    if not torch.is_tensor(Psi):
        Psi = torch.from_numpy(np.ascontiguousarray(Psi, dtype=np.float64)).cuda()
    assert Psi.dtype == torch.float64 and Psi.dim() == 2 and Psi.shape[0] >= 1 and (Psi.shape[1] <= 1 or Psi.stride(1) == 1)
    k, ns = Psi.shape
    ldpsi = Psi.stride(0) if k > 1 else max(Psi.stride(0), ns)
    args, _, keep = _gram_arguments(sb_or_layout, Psi[0].contiguous(), left_ops, right_ops)        # (row 0 only sizes and places the operators)
    n = len(vectors)
    first = _i32(list(np.cumsum([0] + [len(v) for v in vectors])))
    flat = [t for v in vectors for t in v]
    terms = (_capi.Term * max(len(flat), 1))()
    for i, (c, l, r) in enumerate(flat):
        terms[i].a, terms[i].left_op, terms[i].right_op = float(c), (-1 if l is None else int(l)), (-1 if r is None else int(r))
    nf = max(k * n, 1)
    G = torch.empty((nf, nf), dtype=torch.float64, device=Psi.device)
    report = _capi.GramReport()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(_capi.lib().dmrgx_kron_term_gram_states(*args[:5], k, C.c_void_p(Psi.data_ptr()), ldpsi, *args[6:], n, first, terms, workspace_bytes,
                                                        C.c_void_p(G.data_ptr()), nf, C.byref(report), st))
    torch.cuda.current_stream().synchronize()       # the operator copies in `keep` are read by the queued work
    return G, report


def term_apply(sb_or_layout, psi, left_ops, right_ops, vectors, out=None):
    """Y[a, :n_states] = v_a = sum over the terms (c, l, r) of vectors[a] of c * (left_ops[l] (x) right_ops[r]) psi, in the layout of psi
    (dmrgx_kron_term_apply).  Arguments as in term_gram; every term must have total sector shift 0.  out: a 2-D f64 device tensor with
    unit stride along the vector and a row stride >= n_states whose columns beyond n_states are left alone; default: a new
    (len(vectors), n_states) tensor.  Returns Y."""
    _capi.require_device()
    args, psi, keep = _gram_arguments(sb_or_layout, psi, left_ops, right_ops)
    n, ns = len(vectors), psi.numel()
    first = _i32(list(np.cumsum([0] + [len(v) for v in vectors])))
    flat = [t for v in vectors for t in v]
    terms = (_capi.Term * max(len(flat), 1))()
    for i, (c, l, r) in enumerate(flat):
        terms[i].a, terms[i].left_op, terms[i].right_op = float(c), (-1 if l is None else int(l)), (-1 if r is None else int(r))
    if out is None:
        out = torch.empty((max(n, 1), ns), dtype=torch.float64, device=psi.device)
    assert out.dtype == torch.float64 and out.dim() == 2 and out.shape[0] >= n and (out.shape[1] <= 1 or out.stride(1) == 1)
    ldy = out.stride(0) if out.shape[0] > 1 else out.shape[1]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(_capi.lib().dmrgx_kron_term_apply(*args, n, first, terms, C.c_void_p(out.data_ptr()), ldy, st))
    torch.cuda.current_stream().synchronize()       # the operator copies in `keep` are read by the queued work
    return out


def term_apply_to(sb_or_layout, psi, left_ops, right_ops, vectors, out_blocks, out=None):
    """Y[a, :n_out_states] = v_a as in term_apply, written in the reference layout of the KronBlock list out_blocks over the same sector
    tables (dmrgx_kron_term_apply_to): the terms share one total sector shift of any value, and every sector pair they reach must be in
    out_blocks.  out: as in term_apply with n_out_states in place of n_states; default: a new (len(vectors), n_out_states) tensor.
    Returns Y."""
    _capi.require_device()
    args, psi, keep = _gram_arguments(sb_or_layout, psi, left_ops, right_ops)
    left_sizes, right_sizes = (sb_or_layout.left_sizes, sb_or_layout.right_sizes) if hasattr(sb_or_layout, "blocks") else sb_or_layout[:2]
    n = len(vectors)
    first = _i32(list(np.cumsum([0] + [len(v) for v in vectors])))
    flat = [t for v in vectors for t in v]
    terms = (_capi.Term * max(len(flat), 1))()
    for i, (c, l, r) in enumerate(flat):
        terms[i].a, terms[i].left_op, terms[i].right_op = float(c), (-1 if l is None else int(l)), (-1 if r is None else int(r))
    oil, oir = _i32([b[0] for b in out_blocks]), _i32([b[1] for b in out_blocks])
    if out is None:
        ns = sum(left_sizes[il] * right_sizes[ir] for il, ir in out_blocks)
        out = torch.empty((max(n, 1), ns), dtype=torch.float64, device=psi.device)
    assert out.dtype == torch.float64 and out.dim() == 2 and out.shape[0] >= n and (out.shape[1] <= 1 or out.stride(1) == 1)
    ldy = out.stride(0) if out.shape[0] > 1 else out.shape[1]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(_capi.lib().dmrgx_kron_term_apply_to(*args, n, first, terms, len(out_blocks), oil, oir, C.c_void_p(out.data_ptr()), ldy, st))
    torch.cuda.current_stream().synchronize()       # the operator copies in `keep` are read by the queued work
    return out


def noise_expand(sb_or_layout, psi, side, ops, coef, out=None):
    """psi with the images coef[a] * ops[a] psi of one block's operators beside it (dmrgx_kron_noise_expand): side 0 expands the columns of
    every KronBlock with operators of the left block, side 1 the rows with operators of the right block, so that the density matrix of
    the expansion on that side is White's perturbed one.  Layout, psi and operators (a SectorOperator, or (SectorOperator, True) for its
    transpose; any shifts) as in op_gram.  out: a contiguous 1-D f64 device tensor of at least n_out elements (elements beyond n_out are
    left alone); default: a new tensor of n_out.  Returns (Y, extent, n_out); `noise_rdm_layout` turns extent into the layout the
    density-matrix solver takes."""
    _capi.require_device()
    args, psi, keep = _gram_arguments(sb_or_layout, psi, ops if side == 0 else [], ops if side != 0 else [])
    head, (nl, larr, nr, rarr) = args[:6], args[6:]
    n_ops, arr = (nl, larr) if side == 0 else (nr, rarr)
    assert len(coef) == n_ops
    cf = (C.c_double * max(n_ops, 1))(*[float(c) for c in coef])
    extent, n_out = (C.c_int32 * head[2])(), C.c_int64(0)
    L = _capi.lib()
    _capi.check(L.dmrgx_kron_noise_expand(*head, side, n_ops, arr, cf, extent, C.byref(n_out), None, None))
    if out is None:
        out = torch.empty(n_out.value, dtype=torch.float64, device=psi.device)
    assert out.dtype == torch.float64 and out.dim() == 1 and out.is_contiguous() and out.numel() >= n_out.value
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(L.dmrgx_kron_noise_expand(*head, side, n_ops, arr, cf, extent, C.byref(n_out), C.c_void_p(out.data_ptr()), st))
    torch.cuda.current_stream().synchronize()       # the operator copies in `keep` are read by the queued work
    return out, list(extent), n_out.value


def states_expand(sb_or_layout, Psi, weights, side, out=None):
    """Several states of one sector side by side, each times the square root of its weight (dmrgx_kron_states_expand): side 0 sets the
    KronBlock slices of the states beside each other as columns, side 1 stacks them as rows, so that the density matrix of the expansion
    on that side is the weighted average of the states'.  sb_or_layout: a Superblock or (left_sizes, right_sizes, blocks); Psi: a 2-D f64
    device tensor of one row per state with unit stride along the vector (its row stride is the library's ldpsi), only read; weights: one
    non-negative number per state.  out: a 1-D f64 device tensor with unit stride of at least n_out elements (elements beyond n_out are left
    alone); default: a new tensor of n_out.  Returns (Y, extent, n_out); `noise_rdm_layout` turns extent into the layout the density-matrix
    solver takes."""
    _capi.require_device()
    left_sizes, right_sizes, blocks = (sb_or_layout.left_sizes, sb_or_layout.right_sizes, sb_or_layout.blocks) if hasattr(sb_or_layout, "blocks") else sb_or_layout
    n = sum(left_sizes[il] * right_sizes[ir] for il, ir in blocks)
    assert Psi.dtype == torch.float64 and Psi.dim() == 2 and Psi.shape[1] >= n and (Psi.shape[1] <= 1 or Psi.stride(1) == 1)
    ns = Psi.shape[0]
    assert len(weights) == ns
    ldpsi = Psi.stride(0) if ns > 1 else max(Psi.stride(0), Psi.shape[1])
    ls, rs = _i32(left_sizes), _i32(right_sizes)
    sl, sr = _capi.Sectors(len(left_sizes), ls), _capi.Sectors(len(right_sizes), rs)
    bil, bir = _i32([b[0] for b in blocks]), _i32([b[1] for b in blocks])
    head = (C.byref(sl), C.byref(sr), len(blocks), bil, bir, ns, C.c_void_p(Psi.data_ptr()), int(ldpsi), (C.c_double * ns)(*[float(w) for w in weights]), int(side))
    extent, n_out = (C.c_int32 * len(blocks))(), C.c_int64(0)
    L = _capi.lib()
    _capi.check(L.dmrgx_kron_states_expand(*head, extent, C.byref(n_out), None, None))
    if out is None:
        out = torch.empty(n_out.value, dtype=torch.float64, device=Psi.device)
    assert out.dtype == torch.float64 and out.dim() == 1 and (out.numel() <= 1 or out.stride(0) == 1) and out.numel() >= n_out.value
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(L.dmrgx_kron_states_expand(*head, extent, C.byref(n_out), C.c_void_p(out.data_ptr()), st))
    return out, list(extent), n_out.value


def _compose_arguments(sizes, ops, outputs, device="cuda"):
    """The arguments of dmrgx_secop_compose up to the arena, as ctypes values, and the list that keeps every buffer behind them alive.
    outputs: a list of outputs, each a list of strings (coeff, [operator indices])."""
    dummy = torch.zeros(sizes[0] * sizes[0], dtype=torch.float64, device=device)
    args, _, keep = _gram_arguments((list(sizes), list(sizes), [(0, 0)]), dummy, ops, [])
    sec, n_ops, arr = args[0], args[6], args[7]
    first = _i32(list(np.cumsum([0] + [len(o) for o in outputs])))
    flat = [s for o in outputs for s in o]
    strings = (_capi.SecOpString * max(len(flat), 1))()
    for i, (c, fac) in enumerate(flat):
        strings[i].coeff, strings[i].nfac = float(c), len(fac)
        for f, idx in enumerate(fac[:3]):
            strings[i].fac[f] = int(idx)
    n = len(outputs)
    shift, cell_first = (C.c_int32 * max(n, 1))(), (C.c_int32 * (n + 1))()
    cells = (_capi.Cell * max(n * len(sizes), 1))()
    total = C.c_int64(-1)
    return (sec, n_ops, arr, n, first, strings, shift, cell_first, cells, C.byref(total)), total, keep


def secop_compose(sizes, ops, outputs, out=None):
    """C_o = sum over the strings (coeff, [i1, i2, i3]) of outputs[o] of coeff * ops[i1] ops[i2] ops[i3] (one to three factors) on the
    block with sector table `sizes` (dmrgx_secop_compose).  ops: SectorOperators, or (SectorOperator, True) for the transpose.  out: a
    contiguous 1-D f64 device tensor of at least n_doubles elements; default: a new one.  Returns (arena, shifts, blocks) with
    blocks[o] = [(row sector, offset into the arena, rows, columns)]: output o dense over its sector blocks, row-major."""
    _capi.require_device()
    args, total, keep = _compose_arguments(sizes, ops, outputs)
    L = _capi.lib()
    _capi.check(L.dmrgx_secop_compose(*args, None, None))
    if out is None:
        out = torch.empty(max(total.value, 1), dtype=torch.float64, device="cuda")
    assert out.dtype == torch.float64 and out.dim() == 1 and out.is_contiguous() and out.numel() >= total.value
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(L.dmrgx_secop_compose(*args, C.c_void_p(out.data_ptr()), st))
    torch.cuda.current_stream().synchronize()       # the operator copies in `keep` are read by the queued work
    shift, cell_first, cells = args[6], args[7], args[8]
    blocks = [[(cells[c].row_sector, (cells[c].data - out.data_ptr()) // 8, cells[c].nr, cells[c].nc) for c in range(cell_first[o], cell_first[o + 1])]
              for o in range(len(outputs))]
    return out, list(shift[:len(outputs)]), blocks


def noise_rdm_layout(sb_or_layout, side, extent):
    """(left_sizes, right_sizes, blocks, side_mask) under which ReducedDensityMatrices reads an expansion of noise_expand: the expanded
    extents are the sector table of the other side, one sector per KronBlock, and only the density matrices of `side` are built."""
    left_sizes, right_sizes, blocks = (sb_or_layout.left_sizes, sb_or_layout.right_sizes, sb_or_layout.blocks) if hasattr(sb_or_layout, "blocks") else sb_or_layout
    if side == 0:
        return list(left_sizes), list(extent), [(b[0], k) for k, b in enumerate(blocks)], [1] * len(blocks)
    return list(extent), list(right_sizes), [(k, b[1]) for k, b in enumerate(blocks)], [2] * len(blocks)


class ReducedDensityMatrices:
    """Device RDM blocks + spectra of a superblock state (GetTruncation's rank-0 loop,
    include/DMRGBlockContainer.hpp:1715-1775).  psi: device tensor in the reference's vector layout."""

    def __init__(self, left_sizes, right_sizes, blocks, psi, warm=None, side_mask=None):
        """warm: optional {(side, k): (n x n) device tensor of eigenvectors as rows from a previous solve} (warm start).
        side_mask: optional per-KronBlock bits (1: rho_L, 2: rho_R) of the density matrices to build (dmrgx_rdm_create_subset)."""
        L = _capi.lib()
        self.left_sizes, self.right_sizes, self.blocks = list(left_sizes), list(right_sizes), list(blocks)
        ls, rs = _i32(left_sizes), _i32(right_sizes)
        sl, sr = _capi.Sectors(len(left_sizes), ls), _capi.Sectors(len(right_sizes), rs)
        bil, bir = _i32([b[0] for b in blocks]), _i32([b[1] for b in blocks])
        self._handle = C.c_void_p()
        # the library keeps only psi's address and reads psi again when the eigenvectors are formed (dmrgx_rdm_select or the first
        # request): a temporary tensor would go back to torch's allocator and be handed out again before then
        self._psi = psi
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if side_mask is not None:
            assert not warm and len(side_mask) == len(blocks)
            mask = (C.c_uint8 * len(blocks))(*[int(b) for b in side_mask])
            _capi.check(L.dmrgx_rdm_create_subset(C.byref(sl), C.byref(sr), len(blocks), bil, bir, C.c_void_p(psi.data_ptr()), C.cast(mask, C.c_void_p), st,
                                                  C.byref(self._handle)))
        elif warm:
            ptrs =(C.c_void_p * (2 * len(blocks)))()
            for (side, k), t in warm.items():
                assert t.is_contiguous() and t.dtype == torch.float64 and t.shape == (self.size(side, k),) * 2
                ptrs[2 * k + side] = t.data_ptr()
            _capi.check(L.dmrgx_rdm_create_warm(C.byref(sl), C.byref(sr), len(blocks), bil, bir, C.c_void_p(psi.data_ptr()),
                                                C.cast(ptrs, C.c_void_p), st, C.byref(self._handle)))
        else:
            _capi.check(L.dmrgx_rdm_create(C.byref(sl), C.byref(sr), len(blocks), bil, bir, C.c_void_p(psi.data_ptr()), st, C.byref(self._handle)))
        self.report = _capi.RdmReport()         # which solver path ran: tridiagonalisation kind, workgroups per matrix, merge levels, time-outs
        _capi.check(L.dmrgx_rdm_info(self._handle, C.byref(self.report)))
        self.sweeps = self.report.n_sweeps

    def size(self, side, k):
        return (self.left_sizes[self.blocks[k][0]], self.right_sizes[self.blocks[k][1]])[side]

    def eigenvalues(self, side, k):
        out = (C.c_double * self.size(side, k))()
        _capi.check(_capi.lib().dmrgx_rdm_eigenvalues(self._handle, side, k, out))
        return np.array(out)

    def select(self, counts):
        """Second phase (dmrgx_rdm_select): form the eigenvectors of the counts[2*k + side] largest eigenvalues of every density matrix only."""
        arr = (C.c_int32 * (2 * len(self.blocks)))(*[int(c) for c in counts])
        _capi.check(_capi.lib().dmrgx_rdm_select(self._handle, arr, None))
        self._psi = None                        # (read by work queued on the stream psi was allocated on: stream-ordered release)

    def eigenvectors_batch(self, requests):
        """requests: [(side, k, count), ...] -> list of (count, n) tensors, all gathered by ONE launch (dmrgx_rdm_eigenvectors_batch)."""
        outs, tasks = [], (_capi.RdmVecTask * max(len(requests), 1))()
        for i, (side, k, count) in enumerate(requests):
            n = self.size(side, k)
            outs.append(torch.empty((count, n), dtype=torch.float64, device="cuda"))
            tasks[i].side, tasks[i].k, tasks[i].count, tasks[i].dst_dev, tasks[i].ld = side, k, count, outs[-1].data_ptr(), n
        _capi.check(_capi.lib().dmrgx_rdm_eigenvectors_batch(self._handle, len(requests), tasks, None))
        self._psi = None
        return outs

    def eigenvectors(self, side, k, count):
        n = self.size(side, k)
        dst = torch.empty((count, n), dtype=torch.float64, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _capi.check(_capi.lib().dmrgx_rdm_eigenvectors(self._handle, side, k, count, C.c_void_p(dst.data_ptr()), n, st))
        if count > 0:                           # (a request of nothing forms nothing)
            self._psi = None
        return dst

    def destroy(self):
        if self._handle:
            h, self._handle = self._handle, C.c_void_p()      # (the object is gone whatever the verdict of its verification)
            self._psi = None
            _capi.check(_capi.lib().dmrgx_rdm_destroy(h))

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Communicator:
    """dmrgx_comm handle: RCCL over xGMI (one process per GPU), or the host-staged rehearsal back-end for several ranks on one
    GPU.  The 128-byte RCCL id is produced by rank 0 (Communicator.unique_id()) and handed to the other ranks by the caller
    (bench.py: one torch.distributed broadcast at start-up; the C++ engine: a rendezvous file)."""

    def __init__(self, rank, world, unique_id=None, host_staged_name=None):
        L = _capi.lib()
        self.handle = C.c_void_p()
        self.rank, self.world = rank, world
        if host_staged_name is not None:
            _capi.check(L.dmrgx_comm_init_host_staged(rank, world, host_staged_name.encode(), C.byref(self.handle)))
        else:
            assert unique_id is not None and len(unique_id) == 128
            buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
            _capi.check(L.dmrgx_comm_init(rank, world, C.cast(buf, C.c_void_p), C.byref(self.handle)))

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        _capi.check(_capi.lib().dmrgx_comm_unique_id(C.cast(buf, C.c_void_p)))
        return bytes(buf)

    @staticmethod
    def _st(stream):
        return C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)

    def allgather(self, full, seg_stride, stream=None):
        _capi.check(_capi.lib().dmrgx_comm_allgather(self.handle, C.c_void_p(full.data_ptr()), seg_stride, self._st(stream)))

    def allreduce_sum(self, buf, stream=None):
        _capi.check(_capi.lib().dmrgx_comm_allreduce_sum(self.handle, C.c_void_p(buf.data_ptr()), buf.numel(), self._st(stream)))

    def bcast(self, buf, root, stream=None):
        _capi.check(_capi.lib().dmrgx_comm_bcast(self.handle, C.c_void_p(buf.data_ptr()), buf.numel() * buf.element_size(), root, self._st(stream)))

    def allgather_host(self, arr, stream=None):
        """arr: C-contiguous numpy array (same shape on every rank) -> array of shape (world,) + arr.shape."""
        arr = np.ascontiguousarray(arr)
        out = np.empty((self.world,) + arr.shape, dtype=arr.dtype)
        _capi.check(_capi.lib().dmrgx_comm_allgather_host(self.handle, arr.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), arr.nbytes, self._st(stream)))
        return out

    def barrier(self, stream=None):
        _capi.check(_capi.lib().dmrgx_comm_barrier(self.handle, self._st(stream)))

    def info(self):
        """(rank, world, backend) as the library's communicator reports them (backend 0 = RCCL, 1 = host-staged)."""
        r, w, b = C.c_int32(), C.c_int32(), C.c_int32()
        _capi.check(_capi.lib().dmrgx_comm_info(self.handle, C.byref(r), C.byref(w), C.byref(b)))
        return r.value, w.value, b.value

    def destroy(self):
        if self.handle:
            _capi.check(_capi.lib().dmrgx_comm_destroy(self.handle))
            self.handle = C.c_void_p()
