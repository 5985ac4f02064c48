"""CPU: the block plan of one Strassen level over a folded side of the H_eff apply (tests/helpers/strassen_blocks.py, the
NumPy twin of csrc/engine_apply.hip::strassen_side): quadrant sums, packed factors, the descriptors of the seven products
(run through tests/helpers/zgemm_ref.py) and the combination, against the plain product.

Tolerance 1e-13 relative in the max norm: operands with entries of order one, contractions of at most 400 terms; the
plain complex128 product is good to a few 1e-16 and one Strassen level to a small multiple of that.
"""

import numpy as np
import pytest

from helpers import strassen_blocks as sb

TOL = 1e-13

# (dl, d, dr): even everywhere; halves 51 / 17 (no multiple of 16); dl != dr both ways; the smallest
SHAPES = [(40, 4, 40), (34, 3, 34), (48, 4, 32), (32, 4, 48), (6, 5, 10), (2, 1, 2)]


def _crandn(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("batched", [False, True], ids=["seven", "batched"])
@pytest.mark.parametrize("dl,d,dr", SHAPES)
def test_both_sides_against_the_plain_product(dl, d, dr, batched):
    rng = np.random.default_rng(dl * 1000 + d * 100 + dr)
    psi = _crandn(rng, dl, d, dr)
    GL = _crandn(rng, dl * d, dl * d)  # not Hermitian: nothing in the plan may assume it
    GR = _crandn(rng, d * dr, d * dr)
    right = sb.apply_side("R", GR, psi.reshape(dl, d * dr), dl, d, dr, batched=batched)
    want_r = psi.reshape(dl, d * dr) @ GR.T
    assert _rel(right, want_r) < TOL
    # the L side adds to what the R side wrote
    both = sb.apply_side("L", GL, psi.reshape(dl * d, dr), dl, d, dr, out=right.reshape(dl * d, dr), batched=batched)
    want = want_r.reshape(dl * d, dr) + GL @ psi.reshape(dl * d, dr)
    assert _rel(both, want) < TOL
    alone = sb.apply_side("L", GL, psi.reshape(dl * d, dr), dl, d, dr, batched=batched)
    assert _rel(alone, GL @ psi.reshape(dl * d, dr)) < TOL


def test_fixed_factors_of_the_r_side_are_untransposed_blocks():
    """B = GR^T: B12 - B22 is stored as GR21 - GR22, B21 - B11 as GR12 - GR11, and so on."""
    rng = np.random.default_rng(5)
    h = 7
    GR = _crandn(rng, 2 * h, 2 * h)
    g11, g12, g21, g22 = GR[:h, :h], GR[:h, h:], GR[h:, :h], GR[h:, h:]
    want = [g11 + g22, g11, g21 - g22, g12 - g11, g22, g11 + g21, g12 + g22]
    got = sb.pack_factors(GR, sb.FACTORS_BT).reshape(7, h, h)
    for k in range(7):
        assert np.array_equal(got[k], want[k]), k


def test_descriptors():
    """leading dimensions, transposes and packed offsets of the seven products"""
    dl, d, dr = 48, 4, 32
    hm, hn, hk = sb.halves("L", dl, d, dr)
    assert (hm, hn, hk) == (96, 16, 96)
    ds = sb.product_descs("L", hm, hn, hk, False)
    assert len(ds) == 7 and all(x["transB"] == 0 and x["lda"] == hk and x["ldb"] == hn and x["ldc"] == hn for x in ds)
    assert [x["offA"] for x in ds] == [k * hm * hk for k in range(7)]
    assert [x["offC"] for x in ds] == [k * hm * hn for k in range(7)]
    hm, hn, hk = sb.halves("R", dl, d, dr)
    assert (hm, hn, hk) == (24, 64, 64)
    (b,) = sb.product_descs("R", hm, hn, hk, True)
    assert b["batch"] == 7 and b["transB"] == 1 and b["ldb"] == hk
    assert (b["strideA"], b["strideB"], b["strideC"]) == (hm * hk, hk * hn, hm * hn)


@pytest.mark.parametrize("dl,d,dr,l_ok,r_ok", [(33, 3, 33, False, False), (33, 4, 34, True, False), (34, 4, 33, False, True),
                                               (34, 3, 34, True, True), (3, 3, 3, False, False)])
def test_refusals(dl, d, dr, l_ok, r_ok):
    assert sb.valid("L", dl, d, dr) == l_ok and sb.valid("R", dl, d, dr) == r_ok
    for side, ok in (("L", l_ok), ("R", r_ok)):
        if not ok:
            with pytest.raises(ValueError):
                sb.halves(side, dl, d, dr)
