"""-dsf 1 (-m gpu): the engine's dynamical structure factor S^zz(q, w) (DynamicalStructureFactor.json: one dmrgx_kron_term_apply and one
dmrgx_kron_lanczos_coeffs per q and cosine / sine part) against exact diagonalisation of the 6 x 2 lattice, against an exactly known
dimer-product ground state, and against the static table of the same run under truncation.

ED: H from ham.H(N) and the site_op of helpers.lattice_ground_state, restricted to the Sz = 0 sector (924 states); O_q is diagonal in the
site basis.  -mwarmup 64 keeps every state of a 6 x 2 lattice, so the engine's superblock is the lattice itself."""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle.hamiltonian import J1J2XXZModel_SquareLattice
from oracle.qn import OpSz
from helpers import lattice_ground_state
from test_gpu_engine import EXE, run_engine

pytestmark = pytest.mark.gpu

Q = [(3, 1), (1, 0), (2, 1), (0, 0)]
Q_OPT = ",".join("%d,%d" % q for q in Q)
HEIS_6x2 = ["-Lx", 6, "-Ly", 2, "-heisenberg", 1, "-nsweeps", 1, "-H_eps_tol", 1e-13]
J1J2_6x2 = ["-Lx", 6, "-Ly", 2, "-J1", 1, "-Jz1", 1, "-J2", 0.5, "-Jz2", 0.5, "-nsweeps", 1, "-H_eps_tol", 1e-13]


def _records(d):
    return json.load(open(str(d) + "/DynamicalStructureFactor.json"))


def _no_nan(rec):
    def walk(x):
        if isinstance(x, dict):
            return all(walk(v) for v in x.values())
        if isinstance(x, list):
            return all(walk(v) for v in x)
        return not isinstance(x, float) or np.isfinite(x)
    return walk(rec)


def _phases(ham, q):
    Lx, Ly, N = ham.Lx(), ham.Ly(), ham.NumSites()
    r = np.array([ham.To2D(i) for i in range(N)], dtype=float)
    return r @ (2.0 * np.pi * np.array([q[0] / Lx, q[1] / Ly]))


def _lanczos_reorth(H, v0, K):
    Qs, alpha, beta = [v0 / np.linalg.norm(v0)], [], []
    for j in range(K):
        x = H @ Qs[j] - (beta[j - 1] * Qs[j - 1] if j else 0.0)
        alpha.append(Qs[j] @ x)
        x = x - alpha[j] * Qs[j]
        for _ in range(2):
            for u in Qs:
                x = x - (u @ x) * u
        beta.append(np.linalg.norm(x))
        Qs.append(x / beta[j])
    return np.array(alpha), np.array(beta)


@pytest.fixture(scope="module")
def heis_ed():
    """Heisenberg 6 x 2 by dense ED, once: per q the cosine and sine start vectors' norms, their first Lanczos coefficients, the lowest
    pole that carries weight and the first moment, all in the Sz = 0 sector."""
    ham = J1J2XXZModel_SquareLattice(Lx=6, Ly=2, heisenberg=1.0)
    N = ham.NumSites()
    E0, psi, site_op = lattice_ground_state(ham)
    sector = np.array([i for i in range(2 ** N) if bin(i).count("1") == N // 2])
    H = None
    for t in ham.H(N):
        h = t.a * (site_op(t.Iop, t.Isite) @ site_op(t.Jop, t.Jsite))
        H = h if H is None else H + h
    H = H.tocsr()[sector][:, sector].toarray()
    psi = psi[sector]
    assert abs(psi @ psi - 1.0) < 1e-12 and np.abs(H @ psi - E0 * psi).max() < 1e-10      # the ground state lives in the sector
    w, V = np.linalg.eigh(H)
    szd = np.array([site_op(OpSz, i).diagonal()[sector] for i in range(N)])
    out = {"E0": E0}
    for q in Q:
        ph = _phases(ham, q)
        parts, amp2 = [], np.zeros(len(w))
        for f in (np.cos, np.sin):
            v = ((f(ph) / np.sqrt(N)) @ szd) * psi
            n2 = v @ v
            coeffs = _lanczos_reorth(H, v, 10) if n2 > 1e-20 else None
            amp2 += (V.T @ v) ** 2
            parts.append({"norm2": n2, "coeffs": coeffs, "moment": v @ (H @ v) - E0 * n2})
        heavy = np.nonzero(amp2 > 1e-9 * amp2.sum())[0] if amp2.sum() > 1e-20 else []
        out[q] = {"parts": parts, "lowest": (w[heavy[0]] - E0) if len(heavy) else None, "moment": sum(p["moment"] for p in parts)}
    return out


def test_heisenberg_6x2_against_exact_diagonalisation(tmp_path, heis_ed):
    """Nothing truncated, 40 steps, last record: Norm2 of every part to 1e-10, alpha_0..9 and beta_0..8 to 1e-8, the lowest pole with
    weight above 1e-9 Norm2 at (3,1) and (2,1) to 1e-7 (the exact 1.4170703...), sum Weights * pole against the exact first moment to
    1e-8; the sine part at (3,1) and both parts at (0,0) hold no weight and are not run.  With -dsf off the file does not appear, and
    Correlations.json and DMRGSteps.json are the same bytes with it on."""
    run_engine(tmp_path / "off", *HEIS_6x2, "-mwarmup", 64)
    run_engine(tmp_path / "on", *HEIS_6x2, "-mwarmup", 64, "-dsf", 1, "-dsf_q", Q_OPT, "-dsf_steps", 40)
    assert not os.path.exists(str(tmp_path / "off") + "/DynamicalStructureFactor.json")
    for name in ("Correlations.json", "DMRGSteps.json"):
        assert open(str(tmp_path / "on") + "/" + name, "rb").read() == open(str(tmp_path / "off") + "/" + name, "rb").read(), name
    rec = _records(tmp_path / "on")[-1]
    assert _no_nan(rec) and rec["Steps"] == 40 and abs(rec["Norm"] - 1.0) <= 1e-12 and abs(rec["E0"] - heis_ed["E0"]) <= 1e-10
    assert [tuple(p["q"]) for p in rec["Points"]] == Q
    runs = 0
    for p in rec["Points"]:
        q, ed = tuple(p["q"]), heis_ed[tuple(p["q"])]
        poles, weights = np.array(p["Poles"]), np.array(p["Weights"])
        for name, e in zip(("Cos", "Sin"), ed["parts"]):
            part = p[name]
            print(q, name, "Norm2", part["Norm2"], "ED", e["norm2"], "StepsDone", part["StepsDone"])
            assert abs(part["Norm2"] - e["norm2"]) <= 1e-10
            if e["coeffs"] is None:
                assert part["Norm2"] <= 1e-20 and part["StepsDone"] == 0 and part["Alpha"] == [] and part["Beta"] == []
                continue
            runs += 1
            assert part["StepsDone"] == 40                     # 78-156 distinct poles: no breakdown
            a, b = e["coeffs"]
            da, db = np.abs(np.array(part["Alpha"][:10]) - a).max(), np.abs(np.array(part["Beta"][:9]) - b[:9]).max()
            print("   alpha err", da, "beta err", db)
            assert da <= 1e-8 and db <= 1e-8
        norm2 = sum(e["norm2"] for e in ed["parts"])
        assert abs(p["StaticSzz"] - norm2) <= 1e-10 and abs(weights.sum() - p["StaticSzz"]) <= 1e-12
        assert (np.diff(poles) >= 0).all() and (weights >= 0).all()
        if q in ((3, 1), (2, 1)):
            low = poles[weights > 1e-9 * norm2][0]
            print(q, "lowest pole", low, "ED", ed["lowest"])
            assert abs(ed["lowest"] - 1.4170703) <= 1e-6 and abs(low - ed["lowest"]) <= 1e-7
        if q == (0, 0):
            assert len(poles) == 0 and p["StaticSzz"] == 0.0
        else:
            assert abs((weights * poles).sum() - ed["moment"]) <= 1e-8
    assert rec["MatMults"] == 40 * runs and runs == 5
    ps, pss = rec["Points"][0]["Sin"], rec["Points"][3]
    assert ps["StepsDone"] == 0 and pss["Cos"]["StepsDone"] == 0 and pss["Sin"]["StepsDone"] == 0


def test_j1j2_dimer_product_state_breaks_down_after_one_step(tmp_path):
    """J2 = J1 / 2 on 6 x 2: the ground state is an exact dimer product with E0 = -15, and C_q |0> at q = (pi, pi) is an eigenstate: the
    cosine part has Norm2 = 1/2, the run breaks down in its first step, and the one pole sits at w = 4 (1e-8)."""
    rows, _, _ = run_engine(tmp_path, *J1J2_6x2, "-mwarmup", 64, "-dsf", 1, "-dsf_q", "3,1", "-dsf_steps", 12)
    rec = _records(tmp_path)[-1]
    assert _no_nan(rec) and abs(rec["E0"] + 15.0) <= 1e-9
    p = rec["Points"][0]
    print("dimer state: Cos", p["Cos"], "Poles", p["Poles"], "Weights", p["Weights"])
    assert abs(p["Cos"]["Norm2"] - 0.5) <= 1e-10 and p["Cos"]["StepsDone"] == 1 and len(p["Cos"]["Alpha"]) == 1
    assert p["Sin"]["Norm2"] <= 1e-20 and p["Sin"]["StepsDone"] == 0
    assert len(p["Poles"]) == 1 and abs(p["Poles"][0] - 4.0) <= 1e-8 and abs(p["Weights"][0] - 0.5) <= 1e-10
    assert rec["MatMults"] == 12


def test_truncated_run_static_sum_rule(tmp_path):
    """m = 24 cuts the basis: StaticSzz at every q equals (1/N) sum_ij cos(q.(r_i - r_j)) SzSz_ij / Norm of the same run's
    SpinCorrelations.json (1e-12) -- the same truncated operators on the same state --, every weight is >= 0 and every pole >= -1e-7
    (T is a compression of the superblock Hamiltonian, whose lowest eigenvalue is E0)."""
    rows, _, _ = run_engine(tmp_path, *HEIS_6x2, "-mwarmup", 24, "-corr_matrix", 1, "-dsf", 1, "-dsf_q", Q_OPT, "-dsf_steps", 40)
    assert any(r["NStates_SysRot"] < r["NStates_SysEnl"] for r in rows)
    ham = J1J2XXZModel_SquareLattice(Lx=6, Ly=2, heisenberg=1.0)
    N = ham.NumSites()
    dsf, spin = _records(tmp_path), json.load(open(str(tmp_path) + "/SpinCorrelations.json"))
    assert len(dsf) == len(spin) >= 1
    for rec, srec in zip(dsf, spin):
        assert _no_nan(rec) and rec["GlobIdx"] == srec["GlobIdx"]
        szsz = np.array(srec["SzSz"])
        for p in rec["Points"]:
            ph = _phases(ham, p["q"])
            want = (np.cos(ph[:, None] - ph[None, :]) * szsz).sum() / N / srec["Norm"]
            print(p["q"], "StaticSzz", p["StaticSzz"], "from SzSz", want)
            assert abs(p["StaticSzz"] - want) <= 1e-12
            assert all(w >= 0.0 for w in p["Weights"]) and all(x >= -1e-7 for x in p["Poles"])


def test_two_ranks_are_refused_at_start_up(tmp_path):
    """-dsf 1 on two ranks ends with the refusal message on every rank: no hang, no output of a half-run."""
    d = str(tmp_path) + "/"
    cmd = [EXE, *[str(o) for o in HEIS_6x2], "-mwarmup", "8", "-dsf", "1", "-dsf_q", "3,1", "-data_dir", d]
    name = "dmrgx_test_dsf_%d" % os.getpid()
    procs = [subprocess.Popen(cmd, env=dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", DMRGX_COMM="shm", DMRGX_SHM_NAME=name, DMRGX_SHM_MB="64"),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    try:
        outs = [pr.communicate(timeout=120)[0] for pr in procs]
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    for pr, o in zip(procs, outs):
        assert pr.returncode not in (0, None) and pr.returncode > 0, o[-2000:]
        assert "-dsf 1 is not available on more than one rank" in o, o[-2000:]
    assert not os.path.exists(d + "DynamicalStructureFactor.json")


def test_dsf_needs_q_points(tmp_path):
    out = subprocess.run([EXE, *[str(o) for o in HEIS_6x2], "-mwarmup", "8", "-dsf", "1", "-data_dir", str(tmp_path) + "/"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "-dsf_q" in out.stderr
