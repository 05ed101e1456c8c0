"""The checker of the general-descriptor MatMult suite, on the CPU (tests/kron_general.py): the float64 reference against the longdouble
one, faulty definitions that the element-wise bound must catch, one of them that the max-norm criterion of the older MatMult tests lets
through, and what the case generator must keep producing."""
import numpy as np
import pytest

import kron_general as kg

RTOL_MAXNORM = 1e-13          # tests/test_gpu_kron.py: max |y - y_ref| <= RTOL max |y_ref|


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 1e-18


@pytest.mark.parametrize("name", kg.CASES)
def test_float64_reference_within_half_the_bound(name):
    assert np.finfo(np.longdouble).eps < 1e-18
    d, x = kg.case(name)
    R, S, n = kg.case_reference(name)
    R64, S64, n64 = kg.case_reference(name, np.float64)
    assert R.dtype == np.longdouble and np.array_equal(S, S64) and np.array_equal(n, n64)
    assert np.isfinite(R.astype(np.float64)).all() and (S > 0).any()
    worst = kg.kron_check(R64, R, S, n, name + " float64 reference", scale=0.5)
    assert worst <= 1.0
    D, Da, nd = kg.reference_diag(d)
    D64 = kg.reference_diag(d, np.float64)[0]
    kg.kron_check(D64, D, Da, nd, name + " float64 diagonal", scale=0.5)


@pytest.mark.parametrize("kind", kg.FAULTS)
@pytest.mark.parametrize("name", kg.CASES)
def test_faulty_definitions_violate_the_bound(name, kind):
    """Of every kind of fault the subtlest element that reaches 2^-36 of its sum of magnitudes (chosen from the references,
    kg.subtlest_fault): outside the bound.  A bound 10^4 times as loose lets them through, but for a row left at zero, which is wrong by
    its whole sum whatever the grading."""
    d, x = kg.case(name)
    R, S, n = kg.case_reference(name)
    assert n.max() <= 3000                                      # (what kg.VISIBLE was sized for)
    y, where, share = kg.subtlest_fault(d, x, kind, kg.case_reference(name, np.float64)[0], S)
    assert y is not None, (name, kind, "no candidate")
    bad = kg.kron_violations(y, R, S, n)
    print("%s %s: candidate %d, element %d, |y - R| / S_abs = %.3e, bound / S_abs = %.3e" % ((name, kind) + where + (share, kg.kron_bound(1.0, n[where[1]]))))
    assert bad[where[1]] and bad.sum() == 1, (name, kind, share)


@pytest.mark.parametrize("name", kg.CASES)
def test_max_norm_criterion_is_blind_to_a_term_dropped_in_the_weakest_block(name):
    """The evidence for the element-wise bound: a term left out of the weakest KronBlock passes max |y - R| <= 1e-13 max |R| and fails
    kron_check."""
    d, x = kg.case(name)
    R, S, n = kg.case_reference(name)
    R64 = kg.case_reference(name, np.float64)[0]
    y, t, share = kg.term_dropped_in_weakest_block(d, x, R64, S)
    off, w = d.offsets(), kg.weakest_block(d)
    assert np.array_equal(y[:off[w]], R64[:off[w]])             # confined to the weakest block, the last one
    diff = np.abs(y - R.astype(np.float64))
    print("%s: term %d dropped in block %d (up to %.3e of S_abs): max-norm error %.3e of max |R| %.3e" % (name, t, w, share, diff.max(), np.abs(R64).max()))
    assert diff.max() <= RTOL_MAXNORM * np.abs(R64).max()
    assert kg.kron_violations(y, R, S, n)[off[w]:off[w + 1]].any()
    with pytest.raises(AssertionError):
        kg.kron_check(y, R, S, n, name)


def test_nan_counts_as_a_violation():
    d, x = kg.case("thin")
    R, S, n = kg.case_reference("thin")
    y = R.astype(np.float64)
    assert not kg.kron_violations(y, R, S, n).any()
    y[5] = np.nan
    assert kg.kron_violations(y, R, S, n).sum() == 1


# ---- what the cases must contain ------------------------------------------------------------------------------------------------------
def _features(d):
    f = set()
    live = [(a, li, ri) for (a, li, ri) in d.terms if a != 0.0]
    used = {("l", li) for _, li, _ in d.terms} | {("r", ri) for _, _, ri in d.terms}
    ops = [("l", i, o) for i, o in enumerate(d.left_ops)] + [("r", i, o) for i, o in enumerate(d.right_ops)]
    for side, i, o in ops + [("h", 0, o) for o in (d.h_left, d.h_right) if o is not None]:
        for a, c in enumerate(o.cells):
            if c.kind == kg.CELL_IDENT and c.r0 != c.c0:
                f.add("off-diagonal identity cell")
            if c.kind == kg.CELL_DENSE and c.ld_pad > 0:
                f.add("ld > nc")
            if c.kind == kg.CELL_DENSE and c.lead % 2 == 1:
                f.add("odd pointer offset")
            for c2 in o.cells[a + 1:]:
                if c2.row_sector == c.row_sector and c.r0 < c2.r0 + c2.nr and c2.r0 < c.r0 + c.nr and c.c0 < c2.c0 + c2.nc and c2.c0 < c.c0 + c.nc:
                    f.add("overlapping cells")
        if side != "h" and (side, i) in used:
            if abs(o.shift) == 2:
                f.add("|shift| = 2")
            if o.transposed and o.shift == 0 and o.cells:
                f.add("transposed shift-0 operator")
            if not o.cells:
                f.add("used operator without cells")
        if side != "h" and (side, i) not in used:
            f.add("unused operator")
        if side == "h" and o.transposed:
            f.add("transposed H_L or H_R")
    if len({(li, ri) for _, li, ri in live}) < len(live):
        f.add("duplicate term")
    if any(a == 0.0 for a, _, _ in d.terms):
        f.add("zero coefficient")
    if d.h_left is None or d.h_right is None:
        f.add("H_L or H_R missing")
    if any((il - 1, ir + 1) in d.blocks and (il + 1, ir - 1) in d.blocks and (il, ir) not in d.blocks
           for il in range(len(d.left_sizes)) for ir in range(len(d.right_sizes))):
        f.add("missing interior KronBlock")
    return f


REQUIRED = ["overlapping cells", "off-diagonal identity cell", "|shift| = 2", "transposed shift-0 operator", "duplicate term", "zero coefficient",
            "unused operator", "missing interior KronBlock"]


def test_generator_coverage():
    named = set().union(*[_features(kg.case(n)[0]) for n in kg.NAMED])
    drawn = set().union(*[_features(kg.case("random%d" % s)[0]) for s in kg.RANDOM_SEEDS])
    for feature in REQUIRED + ["ld > nc", "odd pointer offset", "transposed H_L or H_R"]:
        assert feature in named, feature
        assert feature in drawn, feature
    assert "used operator without cells" in named and "H_L or H_R missing" in named
    # the named cases hold what their names say
    assert {"|shift| = 2", "missing interior KronBlock"} <= _features(kg.case("shifts")[0])
    assert {"overlapping cells", "off-diagonal identity cell"} <= _features(kg.case("overlap")[0])
    assert {"transposed shift-0 operator", "ld > nc", "odd pointer offset", "transposed H_L or H_R"} <= _features(kg.case("transposed_ld")[0])
    assert {"duplicate term", "zero coefficient", "unused operator", "used operator without cells"} <= _features(kg.case("term_graph")[0])
    d = kg.case("transposed_ld")[0]
    assert all(o.transposed for o in d.left_ops + d.right_ops + [d.h_left, d.h_right])
    assert all(c.ld_pad in (1, 3, 7) and c.lead % 2 == 1 for o in d.left_ops + d.right_ops + [d.h_left, d.h_right] for c in o.cells)
    for w in (d.h_left, d.h_right):
        b = kg.op_blocks(w, d.left_sizes if w is d.h_left else d.right_sizes)
        assert any(not np.array_equal(v, v.T) for v in b.values())
    # five ranks are more than the columns of some KronBlock, in the named and in the drawn cases
    for names in (list(kg.NAMED), ["random%d" % s for s in kg.RANDOM_SEEDS]):
        assert any(kg.case(n)[0].right_sizes[ir] < 5 for n in names for _, ir in kg.case(n)[0].blocks)
    assert kg.min_vertex_cover(kg.case("term_graph")[0]) == 3 and kg.min_vertex_cover(kg.case("row_ranges")[0]) == 3


@pytest.mark.parametrize("name", kg.CASES)
def test_graded_inputs(name):
    d, x = kg.case(name)
    off, exps = d.offsets(), kg.graded_exponents(d)
    assert max(exps) == 0 and min(exps) <= -40
    for k, e in enumerate(exps):
        m = np.abs(x[off[k]:off[k + 1]]) * 2.0 ** -e
        assert m.min() >= 0.5 and m.max() <= 1.5
    for o in d.left_ops + d.right_ops + [o for o in (d.h_left, d.h_right) if o is not None]:
        for c in o.cells:
            if c.kind == kg.CELL_DENSE:
                m = np.abs(c.array)
                e = np.floor(np.log2(m.max() / 1.5 * (1 + 1e-12))) if m.max() > 0 else 0
                assert c.array.shape == (c.nr, c.nc) and m.min() >= 0.5 * 2.0 ** -8 and m.max() <= 1.5 * 2.0 ** 8, (name, e)
                assert m.max() / m.min() <= 3.0
    assert name == "shifts" or all(s in kg.SIZES for s in d.left_sizes + d.right_sizes)
