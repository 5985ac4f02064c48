"""NumPy model of the reducing product of the MFMA zgemm (``zgemm_reduce``; ``ZgemmDesc::epi_w`` in ``csrc/common.h``),
written from the formula there and not from the kernel:

    C[offC + u su + v sv + i si] (+)= sum_{x < xm, y < yn} W[offW + i ldw + x yn + y] * T[u xm + x][v yn + y],   i < di,
    T = A op(B)   (m x n; A: m x k, rows lda apart; B: k x n, or n x k with transB),   u < m / xm,  v < n / yn

and the table of cases the host and the GPU tests share.  Everything is explicit index arithmetic on flat buffers;
``make_case`` lays the views into canary buffers.

The kernel runs one of thirteen epilogue bodies (numbering: ``csrc/zgemm_reduce_args_check.h``); ``CASES`` names, for every
row, the body it must reach in the default setting, with the unguarded variant off, and with the 4 x 4 x 4 form off.
"""

from __future__ import annotations

import numpy as np

DEFAULTS = dict(
    m=0, n=0, k=0, transB=0, lda=0, ldb=0, offA=0, offB=0, xm=0, yn=0, di=0, acc=0, ldw=0, offW=0, su=0, sv=0, si=0, offC=0,
    mode3m=-1, epi_b4=-1, epi_full=-1)

SENTINEL = 12345.0 + 6789.0j  # what C holds wherever the operation does not own it
PAD_ROWS = 64                 # rows of pad behind the last element of an operand (the kernel's tile is 64 rows)
SETTINGS = {"default": dict(epi_b4=-1, epi_full=-1), "full_off": dict(epi_b4=-1, epi_full=0), "b4_off": dict(epi_b4=0, epi_full=-1)}


def full(args: dict) -> dict:
    unknown = set(args) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **args)


def groups(a: dict):
    return a["m"] // a["xm"], a["n"] // a["yn"]


def index_a(a: dict) -> np.ndarray:
    """[m][k] flat indices of A"""
    return a["offA"] + np.arange(a["m"], dtype=np.int64)[:, None] * a["lda"] + np.arange(a["k"], dtype=np.int64)[None, :]


def index_b(a: dict) -> np.ndarray:
    """[k][n] flat indices of op(B)"""
    k = np.arange(a["k"], dtype=np.int64)[:, None]
    j = np.arange(a["n"], dtype=np.int64)[None, :]
    return a["offB"] + (j * a["ldb"] + k if a["transB"] else k * a["ldb"] + j)


def index_w(a: dict) -> np.ndarray:
    """[di][xm * yn] flat indices of the core"""
    return a["offW"] + np.arange(a["di"], dtype=np.int64)[:, None] * a["ldw"] + np.arange(a["xm"] * a["yn"], dtype=np.int64)[None, :]


def index_c(a: dict) -> np.ndarray:
    """[nu][nv][di] flat indices of the outputs"""
    nu, nv = groups(a)
    u = np.arange(nu, dtype=np.int64)[:, None, None]
    v = np.arange(nv, dtype=np.int64)[None, :, None]
    i = np.arange(a["di"], dtype=np.int64)[None, None, :]
    return a["offC"] + u * a["su"] + v * a["sv"] + i * a["si"]


def owned_c(args: dict) -> np.ndarray:
    """flat indices of every element of C the operation owns"""
    a = full(args)
    if a["m"] == 0 or a["n"] == 0:
        return np.zeros(0, np.int64)
    return index_c(a).reshape(-1)


def last_elements(args: dict) -> dict:
    """largest flat index of each view (what the hook's footprint check compares with the buffer sizes)"""
    a = full(args)
    return {"A": int(index_a(a).max()), "B": int(index_b(a).max()), "W": int(index_w(a).max()), "C": int(index_c(a).max())}


def int_bound(a: dict) -> int:
    """Largest magnitude any partial sum of an 'int' case (parts in [-2, 2]) can reach, in either product form: a part of
    T is at most 8 k (4M) and the 3M sum (ar + ai)(br + bi) at most 16 k; the epilogue multiplies parts of W (3M: sums of
    two, at most 4) with parts of T (3M: sums of two) over xm yn terms, and acc adds a part of C."""
    t = 16 * a["k"]
    return a["xm"] * a["yn"] * 4 * (2 * t) + 2


def apply(args: dict, A, B, W, C, dtype=np.complex128) -> np.ndarray:
    """The expected WHOLE C buffer: owned elements written (acc = 0) or added to (acc = 1), every other element as it came
    in.  ``dtype=np.clongdouble`` forms every product and sum in extended precision and rounds once at the end."""
    a = full(args)
    out = np.array(C, dtype=np.complex128).reshape(-1).copy()
    if a["m"] == 0 or a["n"] == 0:
        return out
    A = np.asarray(A, dtype=np.complex128).reshape(-1)
    B = np.asarray(B, dtype=np.complex128).reshape(-1)
    W = np.asarray(W, dtype=np.complex128).reshape(-1)
    nu, nv = groups(a)
    T = A[index_a(a)].astype(dtype) @ B[index_b(a)].astype(dtype)
    Wm = W[index_w(a)].astype(dtype).reshape(a["di"], a["xm"] * a["yn"])
    # [(u, v)][(x, y)] times [(x, y)][i]
    Tg = T.reshape(nu, a["xm"], nv, a["yn"]).transpose(0, 2, 1, 3).reshape(nu * nv, a["xm"] * a["yn"])
    res = (Tg @ Wm.T).reshape(nu, nv, a["di"])
    ic = index_c(a)
    if a["acc"]:
        res = res + out[ic].astype(dtype)
    out[ic] = res.astype(np.complex128)
    return out


def apply_loops(args: dict, A, B, W, C) -> np.ndarray:
    """the same by a plain Python loop over every index of the formula (small cases only)"""
    a = full(args)
    out = np.array(C, dtype=np.complex128).reshape(-1).copy()
    nu, nv = (groups(a) if a["m"] and a["n"] else (0, 0))
    for u in range(nu):
        for v in range(nv):
            for i in range(a["di"]):
                s = 0.0 + 0.0j
                for x in range(a["xm"]):
                    for y in range(a["yn"]):
                        r, c = u * a["xm"] + x, v * a["yn"] + y
                        t = 0.0 + 0.0j
                        for k in range(a["k"]):
                            b = B[a["offB"] + (c * a["ldb"] + k if a["transB"] else k * a["ldb"] + c)]
                            t += A[a["offA"] + r * a["lda"] + k] * b
                        s += W[a["offW"] + i * a["ldw"] + x * a["yn"] + y] * t
                q = a["offC"] + u * a["su"] + v * a["sv"] + i * a["si"]
                out[q] = out[q] + s if a["acc"] else s
    return out


def layout(xm, yn, di, nu, nv, k, transB=0, acc=0, pad=(0, 0, 0), off=(0, 0, 0, 0), c_layout="engine", **extra) -> dict:
    """Descriptor of nu x nv groups: leading dimensions = the view's row + pad (A, B, W), first elements at ``off`` (A, B,
    W, C).  ``c_layout``: 'engine' = the edge apply's output sigma[u][i][v] (su = di nv, sv = 1, si = nv); 'inner' =
    C[u][v][i] with i innermost (si = 1) and padded rows."""
    m, n = nu * xm, nv * yn
    a = dict(m=m, n=n, k=k, transB=transB, xm=xm, yn=yn, di=di, acc=acc)
    a["lda"] = k + pad[0]
    a["ldb"] = (k if transB else n) + pad[1]
    a["ldw"] = xm * yn + pad[2]
    a["offA"], a["offB"], a["offW"], a["offC"] = off
    if c_layout == "engine":
        a["su"], a["sv"], a["si"] = di * nv, 1, nv
    else:
        a["si"], a["sv"] = 1, di + 3
        a["su"] = nv * a["sv"] + 5
    a.update(extra)
    return full(a)


def draw(rng, shape, kind):
    """'int': real and imaginary parts integers in [-2, 2]; 'gauss': standard normal"""
    if kind == "int":
        return rng.integers(-2, 3, shape).astype(np.float64) + 1j * rng.integers(-2, 3, shape).astype(np.float64)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def make_case(args: dict, rng, kind="int"):
    """Canary buffers for a descriptor: (A, B, W, C) flat complex128.  A, B and W are NaN everywhere except the elements
    of their views (the pad between rows, before the first element and behind the last; for W the columns between xm yn
    and ldw).  C holds SENTINEL everywhere except its owned elements, which hold data (acc = 1) or NaN (acc = 0: the
    kernel must overwrite them without reading).  An 'int' case asserts that no partial sum can leave the exact range."""
    a = full(args)
    nan = complex(np.nan, np.nan)
    last = last_elements(a)
    if kind == "int":
        assert int_bound(a) < 2 ** 53 // 1024, a
    A = np.full(last["A"] + 1 + PAD_ROWS * max(a["lda"], 1), nan, dtype=np.complex128)
    B = np.full(last["B"] + 1 + PAD_ROWS * max(a["ldb"], 1), nan, dtype=np.complex128)
    W = np.full(last["W"] + 1 + 2 * max(a["ldw"], 1), nan, dtype=np.complex128)
    C = np.full(last["C"] + 1 + 257, SENTINEL, dtype=np.complex128)
    ia, ib, iw, ic = index_a(a), index_b(a), index_w(a), index_c(a)
    A[ia] = draw(rng, ia.shape, kind)
    B[ib] = draw(rng, ib.shape, kind)
    W[iw] = draw(rng, iw.shape, kind)
    C[ic] = draw(rng, ic.shape, kind) if a["acc"] else nan
    return A, B, W, C


# --------------------------------------------------------------------------------------------------------- the case table
def row(name, xm, yn, di, transB, default, full_off=None, b4_off=None, c_layout="engine"):
    """one shape and the body it must reach: in the default setting, with the unguarded variant off (default: the same),
    with the 4 x 4 x 4 form off"""
    return dict(name=name, xm=xm, yn=yn, di=di, transB=transB, c_layout=c_layout,
                expect={"default": default, "full_off": default if full_off is None else full_off,
                        "b4_off": default if b4_off is None else b4_off})


def engine_rows(d, M, default, full_off=None, b4_off=None, c_layout="engine"):
    """the two products of the edge apply at local dimension d and MPO bond M: the R side (NT, groups d x M) and the L side
    (NN, groups M x d); both reach the same body"""
    return [row(f"d{d}M{M}-R", d, M, d, 1, default, full_off, b4_off, c_layout),
            row(f"d{d}M{M}-L", M, d, d, 0, default, full_off, b4_off, c_layout)]


CASES = (
    engine_rows(16, 32, 1, full_off=4, b4_off=8)
    + engine_rows(32, 16, 2, full_off=6, b4_off=9)
    + engine_rows(16, 64, 3, b4_off=8)
    + engine_rows(16, 24, 4, b4_off=8, c_layout="inner")
    + engine_rows(32, 32, 5, b4_off=9)
    + engine_rows(24, 16, 6, b4_off=9)
    + engine_rows(4, 16, 7, b4_off=13)
    + engine_rows(16, 16, 8)
    + engine_rows(32, 8, 9, c_layout="inner")
    + engine_rows(64, 64, 10)
    + engine_rows(12, 10, 11)
    + engine_rows(20, 8, 12)
    + engine_rows(8, 8, 13)
    + engine_rows(10, 10, 13, c_layout="inner")  # 36 pairs: three column blocks run as four
    + [
        # di apart from xm and yn, at the borders of the dispatch: di = 4 | 5, 16 | 17, 32 | 33, and 3 rows with 64 pairs
        row("di5-p4", 32, 32, 5, 1, 3, b4_off=8),
        row("di5-p8", 32, 16, 5, 0, 4, b4_off=8),
        row("di4-p8", 16, 32, 4, 1, 7, b4_off=8),
        row("di16-p8-whole", 32, 16, 16, 1, 1, full_off=4, b4_off=8, c_layout="inner"),
        row("di17-p8", 32, 16, 17, 1, 6, b4_off=9),
        row("di17-p4", 32, 32, 17, 0, 5, b4_off=9),
        row("di32-p8-whole", 16, 32, 32, 0, 2, full_off=6, b4_off=9),
        row("di32-p16", 16, 16, 32, 1, 9),
        row("di17-p16", 16, 16, 17, 0, 9),
        row("di33-p16", 16, 16, 33, 1, 10),  # three row blocks run as four
        row("di33-p2", 64, 32, 33, 0, 10),
        row("di3-p64", 8, 8, 3, 1, 7, b4_off=13),
        row("di5-p64", 8, 8, 5, 0, 13),
        row("di16-p64", 8, 8, 16, 1, 13, c_layout="inner"),
        row("di16-p30", 12, 10, 16, 0, 11),
        row("di17-p30", 12, 10, 17, 1, 12),
        row("di32-p30", 10, 12, 32, 0, 12),
        row("di4-p16", 16, 16, 4, 0, 7, b4_off=8),
    ]
)

K_VALUES = (1, 5, 16, 33)  # 33 = three K tiles of 16 with a ragged last one


def geometries(idx: int):
    """The three geometries of row ``idx`` of CASES as ``layout`` arguments: one group; exactly one tile; a partial last
    tile in both directions.  K takes its four values in turn over the rows, the ragged three-tile one in the partial
    geometry of every second row; the last two geometries lie in padded rows at non-zero offsets."""
    r = CASES[idx]
    tu, tv = 64 // r["xm"], 64 // r["yn"]
    ks = [K_VALUES[(idx + g) % 4] for g in range(3)]
    if idx % 2 == 0:
        ks[2] = 33
    base = dict(xm=r["xm"], yn=r["yn"], di=r["di"], transB=r["transB"], c_layout=r["c_layout"])
    return [
        dict(base, nu=1, nv=1, k=ks[0]),
        dict(base, nu=tu, nv=tv, k=ks[1], pad=(3, 1, 5), off=(7, 2, 11, 13)),
        dict(base, nu=tu + 1, nv=2 * tv + 1, k=ks[2], pad=(1, 6, 2), off=(4, 9, 3, 6)),
    ]


def settings_of(r: dict):
    """the settings a row runs under: the default, and each switch that changes its body"""
    return ["default"] + [s for s in ("full_off", "b4_off") if r["expect"][s] != r["expect"]["default"]]
