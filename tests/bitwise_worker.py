"""Child process of tests/test_gpu_poison.py: runs fixed-input kernels and writes their outputs to an .npz file, so that runs in
separate processes -- clean or with DMRGX_POOL_POISON=1 -- can be compared bit for bit.

    python tests/bitwise_worker.py OUT.npz apply,solvers,solver_paths,striped,krylov
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

load_package()
from dmrgx_amd import superblock as sbm, workloads as wl  # noqa: E402


def full_size_applies(out):
    """dmrgx_kron_apply on the full-size BASELINE superblocks: the digest of y (80 MB at cfg5) and its NaN count."""
    for cfg in ("cfg4real", "cfg5"):
        sb = wl.synthetic_superblock(cfg)
        x = torch.from_numpy(np.random.default_rng(4242).standard_normal(sb.n_states)).cuda()
        y = torch.full_like(x, float("nan"))
        plan = sbm.KronPlan(sb)
        plan.apply(x, y)
        torch.cuda.synchronize()
        h = y.cpu().numpy()
        out["apply_%s_sha" % cfg] = np.frombuffer(hashlib.sha256(h.tobytes()).digest(), dtype=np.uint8)
        out["apply_%s_nonfinite" % cfg] = np.array(int((~np.isfinite(h)).sum()))
        plan.destroy()
        del x, y


def solvers(out):
    """Lanczos and generalized Davidson (an odd and an even number of states) from fixed start vectors, and the density-matrix
    spectra + eigenvectors of a fixed state."""
    kept = {0.5: 7, -0.5: 6, 1.5: 3, -1.5: 2}
    for tag, kw in (("even", dict(m=32, Ly=2, seed=3)), ("odd", dict(Ly=2, seed=3, kept=(kept, kept)))):      # 844 and 341 states
        sb = wl.synthetic_superblock("cfg2", **kw)
        plan = sbm.KronPlan(sb)
        out["n_states_%s" % tag] = np.array(sb.n_states)
        e0, psi, _ = plan.eigs_lowest(tol=1e-12, seed=9)
        out["lanczos_%s_e0" % tag], out["lanczos_%s_psi" % tag] = np.array(e0), psi.cpu().numpy()
        psi0 = torch.from_numpy(np.random.default_rng(1).standard_normal(sb.n_states)).cuda()
        e0, psi, _ = plan.eigs_lowest(tol=1e-12, method=1, psi0=psi0, ncv=6)
        out["gd_%s_e0" % tag], out["gd_%s_psi" % tag] = np.array(e0), psi.cpu().numpy()
        plan.destroy()
    rng = np.random.default_rng(5)
    ls, rs = [300, 77], [120, 260]
    psi = rng.standard_normal(300 * 120 + 77 * 260)
    psi /= np.linalg.norm(psi)
    rdm = sbm.ReducedDensityMatrices(ls, rs, [(0, 0), (1, 1)], torch.from_numpy(psi).cuda())
    for k in range(2):
        for side in (0, 1):
            out["rdm_w_%d_%d" % (k, side)] = rdm.eigenvalues(side, k)
            out["rdm_u_%d_%d" % (k, side)] = rdm.eigenvectors(side, k, rdm.size(side, k)).cpu().numpy()
    rdm.destroy()


def solver_paths(out):
    """The branches of dmrgx_eigs_lowest that `solvers` does not reach, on helpers.krylov_superblock at 845 states (odd): rejected and
    accepted start vectors on both methods, truncated cycles, an exhausted solve, the unfused Davidson iteration and its hand-over to
    the Lanczos path.  Per case e0, psi and every field of the stats but the seconds; each case asserts that it took its branch."""
    import ctypes as C
    from dmrgx_amd import _capi
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import krylov_superblock
    fields = [k for k, _ in _capi.EigsStats._fields_ if k != "seconds"]

    def keep(tag, e0, psi, stats):
        out["paths_%s_e0" % tag], out["paths_%s_psi" % tag] = np.array(e0), psi.cpu().numpy()
        for k in fields:
            out["paths_%s_%s" % (tag, k)] = np.array(getattr(stats, k))
        return stats

    n = 845
    plan = sbm.KronPlan(krylov_superblock(wl, n))
    e0, gs, stats = plan.eigs_lowest(tol=1e-12, seed=9)
    assert keep("plain", e0, gs, stats).converged == 1
    rng = np.random.default_rng(845)
    far = torch.from_numpy(rng.standard_normal(n)).cuda()
    near = gs + 1e-3 * torch.from_numpy(rng.standard_normal(n)).cuda()
    for method in (0, 1):
        s = keep("zero_m%d" % method, *plan.eigs_lowest(tol=1e-10, seed=9, method=method, psi0=torch.zeros_like(gs)))
        assert s.start_rejected == 1 and s.converged == 1, (method, s.start_rejected, s.converged)
        s = keep("light_m%d" % method, *plan.eigs_lowest(tol=1e-10, seed=9, method=method, psi0=0.3 * gs, min_initial_norm2=0.25))
        assert s.start_rejected == 1 and s.converged == 1, (method, s.start_rejected, s.converged)
        s = keep("accepted_m%d" % method, *plan.eigs_lowest(tol=1e-10, seed=9, method=method, psi0=0.6 * gs, min_initial_norm2=0.25))
        assert s.start_rejected == 0 and s.converged == 1, (method, s.start_rejected, s.converged)
    s = keep("truncated", *plan.eigs_lowest(ncv=16, max_matvec=3, psi0=far))
    assert s.n_matvec == 3 and s.n_restart == 1, (s.n_matvec, s.n_restart)
    s = keep("restarts_truncated", *plan.eigs_lowest(ncv=4, max_matvec=11, psi0=far))
    assert s.n_matvec == 11 and s.n_restart == 5, (s.n_matvec, s.n_restart)      # 4 + 2 + 2 + 2 MatMults in full cycles, then 1
    # max_it exhausted, through the C ABI (the wrapper raises): the status and the best pair so far
    opts, stats, e0 = _capi.EigsOpts(), _capi.EigsStats(), C.c_double(float("nan"))
    opts.ncv, opts.max_it, opts.tol, opts.seed = 4, 2, 1e-14, 9
    psi = torch.full((plan.info.vec_len,), float("nan"), dtype=torch.float64, device="cuda")
    rc = _capi.lib().dmrgx_eigs_lowest(plan._handle, C.byref(opts), C.byref(e0), C.c_void_p(psi.data_ptr()), C.byref(stats), plan._stream_ptr(None))
    assert rc == _capi.DMRGX_ERR_NOTCONV and keep("exhausted", e0.value, psi, stats).n_restart == 2 and stats.converged == 0
    out["paths_exhausted_status"] = np.array(rc)
    s = keep("gd_unfused", *plan.eigs_lowest(tol=1e-10, method=1, ncv=12, psi0=near))
    assert s.converged == 1 and s.start_rejected == 0 and s.n_matvec <= 96, (s.converged, s.n_matvec)
    # Davidson from a start vector that is not close: after 96 MatMults the Ritz vector goes to the Lanczos path (112 MatMults in all)
    s = keep("gd_hand_over", *plan.eigs_lowest(tol=1e-10, method=1, psi0=far))
    assert s.n_matvec > 96 and s.converged == 1 and s.start_rejected == 0, (s.n_matvec, s.converged)
    plan.destroy()


def striped(out):
    """Multi-rank plans with every rank emulated in this process: to_striped, each rank's apply into a NaN-filled ys, from_striped.
    m = 60 at W = 3: right sectors [1, 4, 10, 18, 27, 27, 18, 10, 4, 1], every stripe an even split and some of them empty.
    m = 256, Ly = 4 at W = 2 (40 940 states): right sectors of 110 >= 48 W, where stripe_cut snaps to 64, beside 78 < 48 W, the even split."""
    for tag, kw, world in (("m60_w3", dict(m=60, Ly=3, seed=11), 3), ("m256_w2", dict(m=256, Ly=4), 2)):
        sb = wl.synthetic_superblock("cfg2", **kw)
        plans = [sbm.KronPlan(sb, world_size=world, rank=r) for r in range(world)]
        x = torch.from_numpy(np.random.default_rng(77).standard_normal(sb.n_states)).cuda()
        xs = torch.zeros(plans[0].info.vec_len, dtype=torch.float64, device="cuda")
        plans[0].to_striped(x, xs)
        ys = torch.full_like(xs, float("nan"))
        for p in plans:
            p.apply(xs, ys[p.info.local_offset:p.info.local_offset + p.info.local_len])
        y = torch.full_like(x, float("nan"))
        plans[0].from_striped(ys, y)
        torch.cuda.synchronize()
        out["striped_%s" % tag] = y.cpu().numpy()
        for p in plans:
            p.destroy()


def krylov(out):
    """The device-resident Krylov calls and dmrgx_dot on helpers.krylov_superblock at 845 states (odd, inside one 2048-element range) and
    4097 (odd, across two range borders), every input from a fixed seed; every returned array and scalar is kept.  lanczos_basis runs
    into a fresh V (ldv = n, odd: 8-byte loads) and into a view of a wider tensor with an even row stride (16-byte loads); the Chebyshev
    run of 17 steps crosses one Gram block of 16 rows; the correction vector runs with check_every 0 and 3 and into a Y 8 bytes off a
    16-byte boundary (eta and sigma as in test_gpu_corrvec.CASES[0]: 0.5 and the spectrum's lower end, -33.53 and -93.84 to four digits;
    a numpy restatement converges to 1e-10 in 270 and 324 iterations); the static response of v0 on the complement of the ground state runs
    the same three ways, and the deflated solve finds the first excited state from its random start vector."""
    import ctypes as C
    from dmrgx_amd import _capi
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import krylov_superblock
    for n, sigma in ((845, -33.5), (4097, -93.8)):
        plan = sbm.KronPlan(krylov_superblock(wl, n))
        rng = np.random.default_rng(300 + n)
        v0 = torch.from_numpy(rng.standard_normal(n)).cuda()
        U = torch.from_numpy(rng.standard_normal((13, n))).cuda()

        def keep(tag, names, values):
            for name, value in zip(names, values):
                out["krylov_%d_%s_%s" % (n, tag, name)] = value.cpu().numpy() if torch.is_tensor(value) else np.array(value)

        keep("coeffs", ("norm2", "alpha", "beta", "done"), plan.lanczos_coeffs(v0, 12))
        keep("basis_odd", ("norm2", "alpha", "beta", "done", "V"), plan.lanczos_basis(v0, 12))
        wide = torch.full((12, n + 3), float("nan"), dtype=torch.float64, device="cuda")
        assert wide.data_ptr() % 16 == 0 and wide.stride(0) % 2 == 0
        keep("basis_even", ("norm2", "alpha", "beta", "done", "V"), plan.lanczos_basis(v0, 12, V=wide[:, :n]))
        for nu in (0, 13):
            # (both spectra lie inside [-102, 102])
            keep("cheb_nu%d" % nu, ("norm2", "diag", "cross", "done"), plan.chebyshev_moments(v0, 0.0, 128.0, 17, U=U[:nu] if nu else None))
        eta = 0.5
        for ce in (0, 3):
            cv = plan.correction_vector(v0, sigma, eta, tol=1e-10, max_it=600, check_every=ce, U=U)
            keep("cv_ce%d" % ce, sorted(cv), [cv[k] for k in sorted(cv)])
        ys = torch.full((n + 2,), float("nan"), dtype=torch.float64, device="cuda")
        assert ys[1:].data_ptr() % 16 == 8
        norm2, stats, im = C.c_double(0.0), _capi.CvStats(), (C.c_double * 13)()
        _capi.check(_capi.lib().dmrgx_kron_correction_vector(plan._handle, C.c_void_p(v0.data_ptr()), sigma, eta, 1e-10, 600, 0, C.c_void_p(ys[1:].data_ptr()), C.c_void_p(),
                                                             13, C.c_void_p(U.data_ptr()), n, C.byref(norm2), im, None, C.byref(stats), plan._stream_ptr(None)))
        assert torch.isnan(ys[[0, n + 1]]).all()
        keep("cv_offset", ("Y", "norm2", "im"), (ys[1:n + 1], norm2.value, np.array(im[:])))
        keep("cv_offset", [k for k, _ in _capi.CvStats._fields_], [getattr(stats, k) for k, _ in _capi.CvStats._fields_])
        # the static response on the complement of the ground state, as the correction vector above: check_every 0 and 3, and into an
        # X 8 bytes off a 16-byte boundary; then the first excited state by the deflated solve
        e0, p, _ = plan.eigs_lowest(tol=1e-12)
        for ce in (0, 3):
            rs = plan.static_response(p, v0, e0, tol=1e-10, max_it=600, check_every=ce, U=U)
            keep("rs_ce%d" % ce, sorted(rs), [rs[k] for k in sorted(rs)])
        xs = torch.full((n + 2,), float("nan"), dtype=torch.float64, device="cuda")
        assert xs[1:].data_ptr() % 16 == 8
        rs = plan.static_response(p, v0, e0, tol=1e-10, max_it=600, U=U, X=xs[1:n + 1])
        assert torch.isnan(xs[[0, n + 1]]).all()
        keep("rs_offset", sorted(rs), [rs[k] for k in sorted(rs)])
        e1, psi1, s1 = plan.eigs_lowest_orth(Q=p[None, :], tol=1e-10, seed=7)
        keep("orth", ("e", "psi", "n_matvec", "n_restart", "converged", "residual"), (e1, psi1, s1.n_matvec, s1.n_restart, s1.converged, s1.residual))
        dot = C.c_double(0.0)
        _capi.check(_capi.lib().dmrgx_dot(n, C.c_void_p(v0.data_ptr()), C.c_void_p(U[1].data_ptr()), C.byref(dot), None))
        keep("dot", ("v0_u1",), (dot.value,))
        plan.destroy()


if __name__ == "__main__":
    path, what = sys.argv[1], sys.argv[2].split(",")
    res = {}
    if "apply" in what:
        full_size_applies(res)
    if "solvers" in what:
        solvers(res)
    if "solver_paths" in what:
        solver_paths(res)
    if "striped" in what:
        striped(res)
    if "krylov" in what:
        krylov(res)
    np.savez(path, **res)
    print("bitwise worker ok", sorted(res))
