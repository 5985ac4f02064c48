"""CPU: the two-level Strassen plan over a folded side of the H_eff apply (tests/helpers/strassen_levels.py, the NumPy twin of
csrc/engine_apply.hip::strassen_side with level 2): the 49-factor layout, the batch-49 descriptor (run through
tests/helpers/zgemm_ref.py), the 49 -> 7 and 7 -> out combines, against the plain product.

Tolerance 1e-13 relative in the max norm, as for one level (tests/test_strassen_blocks_host.py): operands with entries of
order one, contractions of at most 432 terms; the plain complex128 product is good to a few 1e-16, one level to about
twice and two levels to about four times that.
"""

import numpy as np
import pytest

from helpers import strassen_blocks as sb
from helpers import strassen_levels as sl

TOL = 1e-13

# (dl, d, dr), all sides divisible by 4: quarters 40 / 10; 27 / 9 (odd, no multiple of 16); dl != dr both ways; odd
# quarters 15 / 3 and 5 / 3; the smallest
SHAPES = [(40, 4, 40), (36, 3, 36), (48, 4, 32), (32, 4, 48), (12, 5, 12), (4, 1, 4)]


def _crandn(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("batched", [False, True], ids=["separate", "batched"])
@pytest.mark.parametrize("direct", [False, True], ids=["recursion", "direct"])
@pytest.mark.parametrize("dl,d,dr", SHAPES)
def test_both_sides_against_the_plain_product(dl, d, dr, direct, batched):
    rng = np.random.default_rng(dl * 1000 + d * 100 + dr)
    psi = _crandn(rng, dl, d, dr)
    GL = _crandn(rng, dl * d, dl * d)  # not Hermitian: nothing in the plan may assume it
    GR = _crandn(rng, d * dr, d * dr)
    right = sl.apply_side("R", GR, psi.reshape(dl, d * dr), dl, d, dr, batched=batched, direct=direct)
    want_r = psi.reshape(dl, d * dr) @ GR.T
    assert _rel(right, want_r) < TOL
    # the L side adds to what the R side wrote: only its last pass accumulates
    both = sl.apply_side("L", GL, psi.reshape(dl * d, dr), dl, d, dr, out=right.reshape(dl * d, dr), batched=batched, direct=direct)
    want = want_r.reshape(dl * d, dr) + GL @ psi.reshape(dl * d, dr)
    assert _rel(both, want) < TOL
    alone = sl.apply_side("L", GL, psi.reshape(dl * d, dr), dl, d, dr, batched=batched, direct=direct)
    assert _rel(alone, GL @ psi.reshape(dl * d, dr)) < TOL


@pytest.mark.parametrize("name", ["A", "B", "BT"])
def test_direct_packing_has_the_bits_of_the_recursion(name):
    rng = np.random.default_rng(7)
    S = _crandn(rng, 4 * 9, 4 * 5)
    two = sl.pack_second_level(sb.pack_factors(S, sl.TABLES[name]), 18, 10, sl.TABLES[name])
    assert np.array_equal(sl.pack_direct(S, sl.TABLES[name]), two)


def test_layout_of_the_49_factors():
    """factor (k1, k2) at (7 k1 + k2) quarter-size matrices: (0, 0) of a left operand is (S11 + S22) of (A11 + A22), i.e.
    blocks (0,0) + (2,2) + (1,1) + (3,3) of the 4 x 4 grid; (2, 3) is A22 of A11, block (1,1); for GR stored transposed
    factor (2, 2) is the (S21 - S22) of (GR21 - GR22)"""
    rng = np.random.default_rng(8)
    q = 3
    S = _crandn(rng, 4 * q, 4 * q)
    blk = lambda i, j: S[i * q:(i + 1) * q, j * q:(j + 1) * q]  # noqa: E731
    F = sl.pack_direct(S, sb.FACTORS_A).reshape(49, q, q)
    assert np.array_equal(F[0], (blk(0, 0) + blk(2, 2)) + (blk(1, 1) + blk(3, 3)))
    assert np.array_equal(F[7 * 2 + 3], blk(1, 1))
    assert np.array_equal(F[7 * 6 + 1], (blk(1, 2) - blk(3, 2)) + (blk(1, 3) - blk(3, 3)))  # (A21 + A22) of (A12 - A22)
    T = sl.pack_direct(S, sb.FACTORS_BT).reshape(49, q, q)
    assert np.array_equal(T[7 * 2 + 2], (blk(3, 0) - blk(3, 2)) - (blk(3, 1) - blk(3, 3)))


def test_descriptors():
    """one batch of 49 with uniform strides, the level-2 areas behind the level-1 ones; transB and ldb = qk on the R side"""
    dl, d, dr = 48, 4, 32
    qm, qn, qk = sl.quarters("L", dl, d, dr)
    assert (qm, qn, qk) == (48, 8, 48)
    (b,) = sl.product_descs("L", qm, qn, qk, True, 7 * 96 * 16, 7 * 96 * 16)
    assert b["batch"] == 49 and b["transB"] == 0 and (b["lda"], b["ldb"], b["ldc"]) == (qk, qn, qn)
    assert (b["strideA"], b["strideB"], b["strideC"]) == (qm * qk, qk * qn, qm * qn)
    assert (b["offA"], b["offB"], b["offC"]) == (0, 7 * 96 * 16, 7 * 96 * 16)
    qm, qn, qk = sl.quarters("R", dl, d, dr)
    assert (qm, qn, qk) == (12, 32, 32)
    ds = sl.product_descs("R", qm, qn, qk, False, 7 * 24 * 64, 7 * 24 * 64)
    assert len(ds) == 49 and all(x["transB"] == 1 and x["ldb"] == qk for x in ds)
    assert [x["offB"] for x in ds] == [k * qk * qn for k in range(49)]
    assert [x["offC"] for x in ds] == [7 * 24 * 64 + k * qm * qn for k in range(49)]


@pytest.mark.parametrize("dl,d,dr,l_lvl,r_lvl", [
    (36, 3, 36, 2, 2), (34, 3, 34, 1, 1), (33, 3, 33, 0, 0),
    (34, 2, 36, 2, 1),   # R side: rows 34 = 2 mod 4, level 2 refused, level 1 holds; L side: rows 68, columns 36
    (36, 2, 34, 1, 2),   # L side: columns 34 = 2 mod 4; R side: rows 36, columns 68
    (6, 6, 4, 2, 1)])
def test_levels_and_refusals(dl, d, dr, l_lvl, r_lvl):
    assert sl.level("L", dl, d, dr) == l_lvl and sl.level("R", dl, d, dr) == r_lvl
    assert sl.level("L", dl, d, dr, want=1) == min(l_lvl, 1) and sl.level("R", dl, d, dr, want=0) == 0
    for side, lv in (("L", l_lvl), ("R", r_lvl)):
        if lv != 2:
            with pytest.raises(ValueError):
                sl.quarters(side, dl, d, dr)


def test_a_side_refused_two_levels_still_runs_one():
    """34 x 2 x 36: the R side (rows 34) runs one level, the L side two, and the L side adds to the R side's result"""
    dl, d, dr = 34, 2, 36
    rng = np.random.default_rng(9)
    psi, GL, GR = _crandn(rng, dl, d, dr), _crandn(rng, dl * d, dl * d), _crandn(rng, d * dr, d * dr)
    assert (sl.level("R", dl, d, dr), sl.level("L", dl, d, dr)) == (1, 2)
    right = sb.apply_side("R", GR, psi.reshape(dl, d * dr), dl, d, dr, batched=True)
    both = sl.apply_side("L", GL, psi.reshape(dl * d, dr), dl, d, dr, out=right.reshape(dl * d, dr))
    want = (psi.reshape(dl, d * dr) @ GR.T).reshape(dl * d, dr) + GL @ psi.reshape(dl * d, dr)
    assert _rel(both, want) < TOL
