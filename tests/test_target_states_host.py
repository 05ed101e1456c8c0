"""Several target states without a GPU: the rules of -nstates / -state_weights (host/TargetStates.hpp, through the host tool's `targets`
command), the two entry points behind them in the library and its binding, and their refusals that need no device."""
import ctypes as C
import os
import re

import pytest

from test_measurements_host import _tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _targets(nstates, weights, in_sector):
    out, err = _tool(["targets %s %s %d" % (nstates, weights, in_sector)])
    rc = int(out[0].split()[1])
    if rc:
        return rc, err, None, None, None
    k, k_step = int(out[1].split()[1]), int(out[1].split()[3])
    return rc, k, k_step, [float(x) for x in out[2].split()[1:]], [float(x) for x in out[3].split()[1:]]


def test_defaults():
    assert _targets("none", "none", 100) == (0, 1, 1, [1.0], [1.0])
    assert _targets("1", "none", 100) == (0, 1, 1, [1.0], [1.0])
    rc, k, k_step, w, all_w = _targets("4", "none", 100)
    assert (rc, k, k_step) == (0, 4, 4) and w == [0.25] * 4 and all_w == [0.25] * 4
    assert _targets("8", "none", 100)[1:3] == (8, 8)


def test_weights_are_normalised_to_sum_one():
    rc, k, k_step, w, all_w = _targets("3", "2,1,1", 50)
    assert (rc, k, k_step) == (0, 3, 3) and w == [0.5, 0.25, 0.25] and all_w == w
    rc, k, k_step, w, _ = _targets("3", "1,0,0", 50)
    assert rc == 0 and w == [1.0, 0.0, 0.0]
    rc, k, k_step, w, _ = _targets("2", "1e-3,3e-3", 50)
    assert rc == 0 and w == pytest.approx([0.25, 0.75], abs=1e-16) and sum(w) == pytest.approx(1.0, abs=1e-16)
    assert _targets("1", "7.5", 50)[3] == [1.0]


@pytest.mark.parametrize("nstates,weights,word", [
    ("3", "1,1", "-state_weights"), ("2", "1,1,1", "-state_weights"), ("none", "1,1", "-state_weights"),       # a count mismatch (k defaults to 1)
    ("2", "1,-1", "-state_weights"), ("2", "1,nan", "-state_weights"), ("2", "inf,1", "-state_weights"), ("2", "1,x", "-state_weights"),
    ("2", "1,,1", "-state_weights"), ("2", "empty", "-state_weights"), ("3", "0,0,0", "-state_weights"),
    ("0", "none", "-nstates"), ("9", "none", "-nstates"), ("-2", "none", "-nstates")])
def test_bad_values_are_refused_by_name_and_value(nstates, weights, word):
    rc, err, _, _, _ = _targets(nstates, weights, 10)
    assert rc == 63 and word in err
    shown = nstates if word == "-nstates" else ("" if weights == "empty" else weights)
    assert shown in err


def test_k_step_is_clamped_to_the_sector_and_the_rest_renormalised():
    rc, k, k_step, w, all_w = _targets("4", "4,2,1,1", 2)
    assert (rc, k, k_step) == (0, 4, 2) and all_w == [0.5, 0.25, 0.125, 0.125] and w == pytest.approx([2.0 / 3.0, 1.0 / 3.0], abs=1e-16)
    assert _targets("4", "none", 1)[2:4] == (1, [1.0])
    assert _targets("4", "none", 3)[2:4] == (3, pytest.approx([1.0 / 3.0] * 3, abs=1e-16))
    rc, k, k_step, w, _ = _targets("3", "0,0,1", 2)                 # the states that fit carry no weight: equal weights
    assert (rc, k_step, w) == (0, 2, [0.5, 0.5])


def test_both_entry_points_are_exported_and_bound_with_the_header_argument_counts(pkg):
    hdr = open(os.path.join(ROOT, "include", "dmrgx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = pkg._capi.lib()
    for name in ("dmrgx_eigs_lowest_orth", "dmrgx_kron_states_expand"):
        args = re.search(r"\b%s\s*\(([^()]*)\)" % name, hdr).group(1)
        assert hasattr(lib, name) and name in pkg._capi.SIGNATURES
        assert len(pkg._capi.SIGNATURES[name][1]) == args.count(",") + 1, name
    assert len(pkg._capi.SIGNATURES["dmrgx_eigs_lowest_orth"][1]) == 9 and len(pkg._capi.SIGNATURES["dmrgx_kron_states_expand"][1]) == 14
    from dmrgx_amd import superblock
    assert callable(superblock.KronPlan.eigs_lowest_orth) and callable(superblock.states_expand)


def test_null_plan_and_null_tables_are_refused_without_a_device(pkg):
    capi = pkg._capi
    L = capi.lib()
    opts, e, stats = capi.EigsOpts(), C.c_double(7.0), capi.EigsStats()
    stats.n_matvec = -3
    psi = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    Q = (C.c_double * 4)()
    for nq in (0, 1):
        assert L.dmrgx_eigs_lowest_orth(None, C.byref(opts), nq, Q, 4, C.byref(e), psi, C.byref(stats), None) == capi.DMRGX_ERR_ARG
        assert "null" in L.dmrgx_last_error().decode()
    assert e.value == 7.0 and list(psi) == [1.0, 2.0, 3.0, 4.0] and stats.n_matvec == -3
    ls, rs = (C.c_int32 * 2)(3, 2), (C.c_int32 * 2)(2, 5)
    sl, sr = capi.Sectors(2, ls), capi.Sectors(2, rs)
    il, ir = (C.c_int32 * 2)(0, 1), (C.c_int32 * 2)(1, 0)
    w = (C.c_double * 2)(1.0, 3.0)
    extent, n_out = (C.c_int32 * 2)(-7, -7), C.c_int64(-7)
    for left, right in ((None, C.byref(sr)), (C.byref(sl), None), (None, None)):
        assert L.dmrgx_kron_states_expand(left, right, 2, il, ir, 2, None, 19, w, 0, extent, C.byref(n_out), None, None) == capi.DMRGX_ERR_ARG
        assert "sector table" in L.dmrgx_last_error().decode()
    assert list(extent) == [-7, -7] and n_out.value == -7
    # the sizes-only mode touches no device either: 3 x 5 and 2 x 2 states
    assert L.dmrgx_kron_states_expand(C.byref(sl), C.byref(sr), 2, il, ir, 2, None, 19, w, 0, extent, C.byref(n_out), None, None) == 0
    assert list(extent) == [10, 4] and n_out.value == 2 * 19
    assert L.dmrgx_kron_states_expand(C.byref(sl), C.byref(sr), 2, il, ir, 2, None, 19, w, 1, extent, C.byref(n_out), None, None) == 0
    assert list(extent) == [6, 4] and n_out.value == 2 * 19
    assert L.dmrgx_kron_states_expand(C.byref(sl), C.byref(sr), 2, il, ir, 2, None, 18, w, 0, extent, C.byref(n_out), None, None) == capi.DMRGX_ERR_ARG
