"""NumPy twin of the block plan of one Strassen level over a folded side of the H_eff apply
(csrc/engine_apply.hip::strassen_side, csrc/vecops.hip::strassen_operands / strassen_combine), written from the comments
in csrc/vecops.h: which quadrants are summed into which of the seven factors, where each factor lies in its packed
buffer, which descriptor each of the seven products gets, and how the products are combined into the output.

    M1 = (A11 + A22)(B11 + B22)  M2 = (A21 + A22) B11  M3 = A11 (B12 - B22)  M4 = A22 (B21 - B11)
    M5 = (A11 + A12) B22  M6 = (A21 - A11)(B11 + B12)  M7 = (A12 - A22)(B21 + B22)
    C11 = M1 + M4 - M5 + M7   C12 = M3 + M5   C21 = M2 + M4   C22 = M1 - M2 + M3 + M6

* L side: sigma[(a,i)][r] (+)= GL psi.  A = GL ((d dl) x (d dl), fixed for a local solve), B = psi ((d dl) x dr).
* R side: sigma[a][(i,r)] = psi GR^T.  A = psi (dl x (d dr)), B = GR^T: the product runs with transB = 1 on GR as stored,
  block (k, l) of B is the transpose of quadrant (l, k) of GR, and the fixed factors are untransposed sums of GR's
  quadrants (GR21 - GR22 for B12 - B22).

Factor k of a (2 hr) x (2 hc) matrix is an hr x hc matrix with leading dimension hc, k * hr * hc elements into its
buffer.  The products are described for tests/helpers/zgemm_ref.py, which multiplies flat buffers by index arithmetic.
"""

from __future__ import annotations

import numpy as np

from . import zgemm_ref as zr

# quadrant index 2 * row half + column half; (first quadrant, second quadrant, sign of the second: 0 = none)
FACTORS_A = [(0, 3, 1), (2, 3, 1), (0, 0, 0), (3, 0, 0), (0, 1, 1), (2, 0, -1), (1, 3, -1)]
FACTORS_B = [(0, 3, 1), (0, 0, 0), (1, 3, -1), (2, 0, -1), (3, 0, 0), (0, 1, 1), (2, 3, 1)]
_SWAP = {0: 0, 1: 2, 2: 1, 3: 3}
FACTORS_BT = [(_SWAP[p], _SWAP[q], s) for p, q, s in FACTORS_B]  # B given transposed: S12 <-> S21


def valid(side: str, dl: int, d: int, dr: int) -> bool:
    """rows, columns and contraction length of the side's product all even"""
    if side == "L":
        return (dl * d) % 2 == 0 and dr % 2 == 0
    return dl % 2 == 0 and (d * dr) % 2 == 0


def halves(side: str, dl: int, d: int, dr: int):
    """(hm, hn, hk) of the half-size products"""
    if not valid(side, dl, d, dr):
        raise ValueError(f"{side} side of {dl} x {d} x {dr}: an odd size, the form is refused")
    return (dl * d // 2, dr // 2, dl * d // 2) if side == "L" else (dl // 2, d * dr // 2, d * dr // 2)


def pack_factors(src: np.ndarray, table) -> np.ndarray:
    """the seven factors of a (2 hr) x (2 hc) matrix, packed flat"""
    hr, hc = src.shape[0] // 2, src.shape[1] // 2
    assert src.shape == (2 * hr, 2 * hc)
    quad = [src[:hr, :hc], src[:hr, hc:], src[hr:, :hc], src[hr:, hc:]]
    out = np.empty(7 * hr * hc, np.complex128)
    for k, (p, q, s) in enumerate(table):
        out[k * hr * hc:(k + 1) * hr * hc] = (quad[p] + s * quad[q] if s else quad[p]).reshape(-1)
    return out


def product_descs(side: str, hm: int, hn: int, hk: int, batched: bool):
    """descriptors of the seven products (one batched descriptor, or seven on offsets into the same packed buffers)"""
    base = dict(m=hm, n=hn, k=hk, lda=hk, ldc=hn)
    if side == "L":
        base.update(transB=0, ldb=hn)
    else:
        base.update(transB=1, ldb=hk)
    if batched:
        return [zr.full(dict(base, batch=7, strideA=hm * hk, strideB=hk * hn, strideC=hm * hn))]
    return [zr.full(dict(base, offA=k * hm * hk, offB=k * hk * hn, offC=k * hm * hn)) for k in range(7)]


def combine(M: np.ndarray, hm: int, hn: int, out: np.ndarray | None) -> np.ndarray:
    m = M.reshape(7, hm, hn)
    c = np.empty((2 * hm, 2 * hn), np.complex128)
    c[:hm, :hn] = ((m[0] + m[3]) - m[4]) + m[6]
    c[:hm, hn:] = m[2] + m[4]
    c[hm:, :hn] = m[1] + m[3]
    c[hm:, hn:] = ((m[0] - m[1]) + m[2]) + m[5]
    return c if out is None else out + c


def apply_side(side: str, G: np.ndarray, psi: np.ndarray, dl: int, d: int, dr: int, out=None, batched=False) -> np.ndarray:
    """The side's product through the plan.  L: G = GL ((d dl) x (d dl)), psi (d dl) x dr; R: G = GR ((d dr) x (d dr), as
    stored: the product is psi GR^T), psi dl x (d dr).  out: what the result is added to (the other side's), or None."""
    hm, hn, hk = halves(side, dl, d, dr)
    if side == "L":
        assert G.shape == (2 * hm, 2 * hk) and psi.shape == (2 * hk, 2 * hn)
        A, B = pack_factors(G, FACTORS_A), pack_factors(psi, FACTORS_B)
    else:
        assert G.shape == (2 * hn, 2 * hk) and psi.shape == (2 * hm, 2 * hk)
        A, B = pack_factors(psi, FACTORS_A), pack_factors(G, FACTORS_BT)
    M = np.full(7 * hm * hn, np.nan + 0j)
    for desc in product_descs(side, hm, hn, hk, batched):
        M = zr.apply(desc, A, B, M)
    return combine(M, hm, hn, out)
