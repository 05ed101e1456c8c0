"""Density-matrix noise without a GPU: the schedule of -noise / -noise_warmup (host/Noise.hpp, through the host tool) and the sizes-only
mode of dmrgx_kron_noise_expand, which touches no device, against the numpy restatement of tests/noise_inputs.py."""
import ctypes as C
import json

import pytest

import noise_inputs as ni
from test_measurements_host import _tool


def _schedule(sched, warm, nsweeps):
    out, err = _tool(["noise %s %s %d" % (sched, warm, nsweeps)])
    rc = int(out[0].split()[1])
    if rc:
        return rc, err, None, None
    vals = [float(x) for x in out[1].split()[1:]]
    any_, js = out[2].split(" json ")
    return rc, vals[0], vals[1:], (int(any_.split()[1]), json.loads(js))


def test_schedule_is_read_like_msweeps_and_the_last_value_holds():
    rc, warm, sweeps, (any_, js) = _schedule("1e-4,1e-6,0", "none", 5)
    assert rc == 0 and warm == 0.0 and sweeps == [1e-4, 1e-6, 0.0, 0.0, 0.0] and any_ == 1 and js == [1e-4, 1e-6, 0.0]
    rc, warm, sweeps, (any_, js) = _schedule("3e-5", "none", 3)
    assert rc == 0 and sweeps == [3e-5] * 3 and js == [3e-5]
    rc, warm, sweeps, (any_, js) = _schedule("0,2.5e-3", "0.125", 4)
    assert rc == 0 and warm == 0.125 and sweeps == [0.0, 2.5e-3, 2.5e-3, 2.5e-3]


def test_without_the_options_and_with_zeros_nothing_is_on():
    rc, warm, sweeps, (any_, js) = _schedule("none", "none", 3)
    assert rc == 0 and warm == 0.0 and sweeps == [0.0] * 3 and any_ == 0 and js == []
    rc, warm, sweeps, (any_, js) = _schedule("0,0,0", "0", 4)
    assert rc == 0 and warm == 0.0 and sweeps == [0.0] * 4 and any_ == 0 and js == [0.0] * 3
    rc, warm, sweeps, (any_, js) = _schedule("none", "1e-3", 2)           # the warm-up alone
    assert rc == 0 and warm == 1e-3 and sweeps == [0.0, 0.0] and any_ == 1


@pytest.mark.parametrize("sched,warm", [("1,-2", "none"), ("1,x", "none"), ("1,,2", "none"), ("nan", "none"), ("empty", "none"), ("1e-4", "-1")])
def test_bad_values_are_refused(sched, warm):
    rc, err, _, _ = _schedule(sched, warm, 2)
    assert rc == 63 and ("-noise" in err)


def test_noise_operators_add_the_missing_transposes_once():
    """NoiseOperators: every distinct plan operator, then the transpose of every operator with a shift unless the list has it -- a Heisenberg
    plan names Sp(i) (shift +1) and Sm(i) (the same blocks, transposed, shift -1), an XY-like list may name Sp alone; coefficient sqrt(a).
    Cell set 32 + i is a second descriptor of the blocks of set i."""
    def ops(a, plan):
        out, _ = _tool(["noiseops %.17g %d %s" % (a, len(plan), " ".join("%d %d %d" % p for p in plan))])
        lst = [tuple(int(x) for x in t.split(":")) for t in out[0].split()[1:]]
        coef, n = out[1].split()[1:]
        return lst, float(coef), int(n)

    # Sz(0), Sp(0), Sm(0) through a second descriptor of Sp(0)'s blocks, Sp(1) alone, Sz(0) named again
    lst, coef, n = ops(0.25, [(0, 0, 0), (1, 0, 1), (-1, 1, 33), (1, 0, 2), (0, 0, 0)])
    assert lst == [(0, 0, 0), (1, 0, 1), (-1, 1, 33), (1, 0, 2), (-1, 1, 2)] and n == 5 and coef == 0.5
    lst, coef, n = ops(1e-4, [(0, 0, 5)])
    assert lst == [(0, 0, 5)] and coef == 1e-4 ** 0.5
    lst, _, n = ops(1.0, [(-1, 1, 7)])                                    # Sm alone: Sp is added
    assert lst == [(-1, 1, 7), (1, 0, 7)]
    assert ops(1.0, [])[0] == []


def test_sizes_only_mode_needs_no_device(pkg):
    """extent and n_out of both sides with Y == NULL and psi == NULL: the library is loaded, no device call is made (the dense cells carry
    a pointer that is never read); refusals of that mode come back as codes."""
    capi, wl = pkg._capi, pkg.workloads
    L = capi.lib()
    keep = []

    def i32(v):
        a = (C.c_int32 * len(v))(*v)
        keep.append(a)
        return a

    ls, rs = i32(ni.LSZ), i32(ni.RSZ)
    sl, sr = capi.Sectors(len(ni.LSZ), ls), capi.Sectors(len(ni.RSZ), rs)
    bil, bir = i32([b[0] for b in ni.BLOCKS]), i32([b[1] for b in ni.BLOCKS])
    for side in (0, 1):
        psi, ops = ni.case(wl, side)
        _, extent, n_out = ni.model_expand(psi, side, ops, ni.COEF)
        arr = (capi.SecOp * len(ops))()
        for i, op in enumerate(ops):
            op, tr = op if isinstance(op, tuple) else (op, False)
            cells = (capi.Cell * len(op.cells))()
            for j, c in enumerate(op.cells):
                cells[j].row_sector, cells[j].r0, cells[j].c0, cells[j].nr, cells[j].nc, cells[j].kind, cells[j].scale = c.row_sector, c.r0, c.c0, c.nr, c.nc, c.kind, c.scale
                if c.kind == capi.CELL_DENSE:
                    cells[j].data, cells[j].ld = 8, c.nc                 # (never dereferenced)
            keep.append(cells)
            arr[i].shift, arr[i].transposed, arr[i].ncells, arr[i].cells = (-op.shift if tr else op.shift), int(tr), len(op.cells), cells
        cf = (C.c_double * len(ops))(*ni.COEF)
        ext, tot = (C.c_int32 * len(ni.BLOCKS))(), C.c_int64(-1)
        args = (C.byref(sl), C.byref(sr), len(ni.BLOCKS), bil, bir, None, side, len(ops), arr, cf, ext, C.byref(tot), None, None)
        assert L.dmrgx_kron_noise_expand(*args) == 0, L.dmrgx_last_error()
        assert list(ext) == extent and tot.value == n_out
        bad = list(args)
        bad[6] = 3
        assert L.dmrgx_kron_noise_expand(*bad) == capi.DMRGX_ERR_ARG
        bad = list(args)
        bad[6] = 1 - side                                                # the operators of the other block: cells outside their sector blocks
        assert L.dmrgx_kron_noise_expand(*bad) == capi.DMRGX_ERR_OUTOFRANGE
        bad = list(args)
        bad[10] = None
        assert L.dmrgx_kron_noise_expand(*bad) == capi.DMRGX_ERR_ARG
