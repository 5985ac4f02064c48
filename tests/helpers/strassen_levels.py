"""NumPy twin of the two-level Strassen plan over a folded side of the H_eff apply (csrc/engine_apply.hip::strassen_side with
level 2, csrc/vecops.hip::strassen_operands with a batch / strassen_operands2 / strassen_combine with a batch), built on
the one-level twin tests/helpers/strassen_blocks.py.

Each of the seven half-size products of level 1 is itself seven quarter-size products, with the same tables at both levels:
FACTORS_A for a left operand, FACTORS_B for a right one, FACTORS_BT for a right operand stored transposed (GR: a level-1
factor of GR is an untransposed sum of GR's quadrants and stands for the transposed B factor, so the recursion stays BT).

Layout: factor (k1, k2) of a (4 qr) x (4 qc) matrix is a qr x qc matrix with leading dimension qc at (7 k1 + k2) qr qc
elements, so one stride serves a batch of 49.  The vector's buffer holds its seven level-1 factors first and its 49
behind them; the products' buffer holds the seven half-size products first (written by the 49 -> 7 combine, leading
dimension 2 qn, never added to) and the 49 quarter-size products behind them.  Only the last 7 -> out pass adds to out.
"""

from __future__ import annotations

import numpy as np

from . import strassen_blocks as sb
from . import zgemm_ref as zr

TABLES = {"A": sb.FACTORS_A, "B": sb.FACTORS_B, "BT": sb.FACTORS_BT}


def level(side: str, dl: int, d: int, dr: int, want: int = 2) -> int:
    """the deepest level <= want the sizes allow: 2 needs rows, columns and contraction length divisible by 4, 1 even"""
    rows, cols, klen = (dl * d, dr, dl * d) if side == "L" else (dl, d * dr, d * dr)
    if want >= 2 and rows % 4 == 0 and cols % 4 == 0 and klen % 4 == 0:
        return 2
    return 1 if want >= 1 and sb.valid(side, dl, d, dr) else 0


def quarters(side: str, dl: int, d: int, dr: int):
    """(qm, qn, qk) of the quarter-size products"""
    if level(side, dl, d, dr) != 2:
        raise ValueError(f"{side} side of {dl} x {d} x {dr}: a size not divisible by 4, two levels are refused")
    hm, hn, hk = sb.halves(side, dl, d, dr)
    return hm // 2, hn // 2, hk // 2


def pack_second_level(f1: np.ndarray, hr: int, hc: int, table) -> np.ndarray:
    """the batched second pass: the seven packed hr x hc factors in, 49 packed quarter-size factors out"""
    qr, qc = hr // 2, hc // 2
    out = np.empty(49 * qr * qc, np.complex128)
    for k1 in range(7):
        out[k1 * 7 * qr * qc:(k1 + 1) * 7 * qr * qc] = sb.pack_factors(f1[k1 * hr * hc:(k1 + 1) * hr * hc].reshape(hr, hc), table)
    return out


def pack_direct(src: np.ndarray, table) -> np.ndarray:
    """the 49 factors straight from the 16 blocks (strassen_operands2): the level-1 sums of blocks first, then their
    level-2 sum, so the bits are those of the recursion"""
    qr, qc = src.shape[0] // 4, src.shape[1] // 4
    assert src.shape == (4 * qr, 4 * qc)

    def block(Q, P):  # block P of quadrant Q
        I, J = 2 * (Q >> 1) + (P >> 1), 2 * (Q & 1) + (P & 1)
        return src[I * qr:(I + 1) * qr, J * qc:(J + 1) * qc]

    out = np.empty(49 * qr * qc, np.complex128)
    for k1, (q1, q2, s1) in enumerate(table):
        for k2, (p1, p2, s2) in enumerate(table):
            def part(P):
                return block(q1, P) + s1 * block(q2, P) if s1 else block(q1, P)
            f = part(p1) + s2 * part(p2) if s2 else part(p1)
            k = 7 * k1 + k2
            out[k * qr * qc:(k + 1) * qr * qc] = f.reshape(-1)
    return out


def product_descs(side: str, qm: int, qn: int, qk: int, batched: bool, off_v: int, off_m: int):
    """descriptors of the 49 products: the operator's factors from the start of their own buffer, the vector's factors
    off_v and the products off_m elements into theirs (behind the level-1 areas)"""
    base = dict(m=qm, n=qn, k=qk, lda=qk, ldc=qn)
    if side == "L":  # A = the operator's factors, B = the vector's
        base.update(transB=0, ldb=qn)
        oa, ob = 0, off_v
    else:  # A = the vector's factors, B = the operator's, transposed
        base.update(transB=1, ldb=qk)
        oa, ob = off_v, 0
    sa, sb_, sc = qm * qk, qk * qn, qm * qn
    if batched:
        return [zr.full(dict(base, batch=49, strideA=sa, strideB=sb_, strideC=sc, offA=oa, offB=ob, offC=off_m))]
    return [zr.full(dict(base, offA=oa + k * sa, offB=ob + k * sb_, offC=off_m + k * sc)) for k in range(49)]


def combine_second_level(Mbuf: np.ndarray, qm: int, qn: int) -> None:
    """49 -> 7: the seven half-size products into the head of the products' buffer, leading dimension 2 qn, written"""
    hm, hn = 2 * qm, 2 * qn
    off = 7 * hm * hn
    for k1 in range(7):
        m7 = Mbuf[off + k1 * 7 * qm * qn:off + (k1 + 1) * 7 * qm * qn]
        Mbuf[k1 * hm * hn:(k1 + 1) * hm * hn] = sb.combine(m7, qm, qn, None).reshape(-1)


def apply_side(side: str, G: np.ndarray, psi: np.ndarray, dl: int, d: int, dr: int, out=None, batched=True, direct=True):
    """The side's product through the two-level plan (arguments as strassen_blocks.apply_side).  direct: the operator's 49
    factors from its 16 blocks, else from its seven level-1 factors.  Every buffer starts as NaN: an element of the 49
    product slots or of the seven half-size products that is read before it is written poisons the result."""
    qm, qn, qk = quarters(side, dl, d, dr)
    hm, hn, hk = 2 * qm, 2 * qn, 2 * qk
    t_op, t_v = ("A", "B") if side == "L" else ("BT", "A")
    vr, vc = (hk, hn) if side == "L" else (hm, hk)  # the vector's level-1 factors
    if side == "L":
        assert G.shape == (4 * qm, 4 * qk) and psi.shape == (4 * qk, 4 * qn)
    else:
        assert G.shape == (4 * qn, 4 * qk) and psi.shape == (4 * qm, 4 * qk)
    opr, opc = G.shape[0] // 2, G.shape[1] // 2
    F = pack_direct(G, TABLES[t_op]) if direct else pack_second_level(sb.pack_factors(G, TABLES[t_op]), opr, opc, TABLES[t_op])
    V = np.full(7 * vr * vc + 49 * (vr // 2) * (vc // 2), np.nan + 0j)
    V[:7 * vr * vc] = sb.pack_factors(psi, TABLES[t_v])
    V[7 * vr * vc:] = pack_second_level(V[:7 * vr * vc], vr, vc, TABLES[t_v])
    M = np.full(7 * hm * hn + 49 * qm * qn, np.nan + 0j)
    for desc in product_descs(side, qm, qn, qk, batched, 7 * vr * vc, 7 * hm * hn):
        A, B = (F, V) if side == "L" else (V, F)
        M = zr.apply(desc, A, B, M)
    assert not np.isnan(M[7 * hm * hn:]).any()  # every element of the 49 slots written before the combine reads it
    assert np.isnan(M[:7 * hm * hn]).all()      # and nothing else
    combine_second_level(M, qm, qn)
    assert not np.isnan(M).any()
    return sb.combine(M[:7 * hm * hn], hm, hn, out)
