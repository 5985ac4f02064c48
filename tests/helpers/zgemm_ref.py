"""NumPy model of the descriptor of the MFMA zgemm (``ZgemmDesc`` in ``csrc/common.h``), written from the comments there
and not from the kernel:

    C[b] = alpha * op(A[b]) * op(B[b]) + beta * C[b]     (row-major, complex128), b < batch

* operand b starts ``off + b * stride`` elements into its flat buffer; rows are ``ld`` elements apart;
* ``transA``: A stored [K][M]; ``transB``: B stored [N][K]; ``conj*``: the operand is conjugated;
* ``arow_skip`` (A not transposed): logical row r of A is stored at row ``r + r // (arow_skip - 1) + 1`` -- stored rows
  0, arow_skip, 2 arow_skip, ... are left out;
* ``rowmap_p > 0``: row r of C is stored ``((r + r0) % p) * s1 + ((r + r0) // p) * s2`` elements after the base
  instead of ``r * ldc``;
* ``klist``: for row tile tm of the 64-row tile grid, ``klist[tm * klist_stride]`` = number of 16-wide K tiles of A
  that count, followed by their indices; every other tile of A is zero whatever the buffer holds.

Everything is explicit index arithmetic on flat buffers: gather op(A)_b and op(B)_b, multiply with ``@`` in complex128,
scatter through ldc or the row map.  ``make_case`` lays such views into canary buffers.
"""

from __future__ import annotations

import numpy as np

DEFAULTS = dict(
    m=0, n=0, k=0, batch=1, transA=0, conjA=0, transB=0, conjB=0, lda=0, ldb=0, ldc=0, strideA=0, strideB=0, strideC=0,
    offA=0, offB=0, offC=0, alpha=1.0, beta=0.0, tile_cfg=-1, mode3m=-1, arow_skip=0, rowmap_p=0, rowmap_s1=0, rowmap_s2=0,
    rowmap_r0=0, klist_stride=0)

SENTINEL = 12345.0 + 6789.0j  # what C holds wherever the operation does not own it
TILE_ROWS = 128               # tallest tile of the kernel: the pad after the last element of an operand is 128 rows


def full(args: dict) -> dict:
    unknown = set(args) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **args)


def stored_row_a(a: dict, r):
    """stored row of logical row r of an untransposed A"""
    s = a["arow_skip"]
    return r + r // (s - 1) + 1 if s > 1 else r


def row_offset_c(a: dict, r):
    """element offset of row r of C from the base of its batch"""
    if a["rowmap_p"] > 0:
        rr = r + a["rowmap_r0"]
        return (rr % a["rowmap_p"]) * a["rowmap_s1"] + (rr // a["rowmap_p"]) * a["rowmap_s2"]
    return r * a["ldc"]


def index_a(a: dict, b: int) -> np.ndarray:
    """[M][K] flat indices of op(A)_b (before conjugation)"""
    i = np.arange(a["m"], dtype=np.int64)[:, None]
    k = np.arange(a["k"], dtype=np.int64)[None, :]
    base = a["offA"] + b * a["strideA"]
    return base + (k * a["lda"] + i if a["transA"] else stored_row_a(a, i) * a["lda"] + k)


def index_b(a: dict, b: int) -> np.ndarray:
    """[K][N] flat indices of op(B)_b"""
    k = np.arange(a["k"], dtype=np.int64)[:, None]
    j = np.arange(a["n"], dtype=np.int64)[None, :]
    base = a["offB"] + b * a["strideB"]
    return base + (j * a["ldb"] + k if a["transB"] else k * a["ldb"] + j)


def index_c(a: dict, b: int) -> np.ndarray:
    """[M][N] flat indices of C_b"""
    i = np.arange(a["m"], dtype=np.int64)[:, None]
    j = np.arange(a["n"], dtype=np.int64)[None, :]
    return a["offC"] + b * a["strideC"] + row_offset_c(a, i) + j


def listed_mask(a: dict, klist) -> np.ndarray:
    """[M][K] True where the element of A lies in a listed K tile (all True for a dense call)"""
    mask = np.ones((a["m"], a["k"]), dtype=bool)
    if klist is None:
        return mask
    kl = np.asarray(klist).reshape(-1)
    mask[:] = False
    for tm in range((a["m"] + 63) // 64):
        row = kl[tm * a["klist_stride"]:]
        for q in range(int(row[0])):
            t = int(row[1 + q])
            mask[tm * 64:(tm + 1) * 64, t * 16:(t + 1) * 16] = True
    return mask


def _span(idx_fn, a, nb):
    lo = hi = None
    for b in range(nb):
        ix = idx_fn(a, b)
        if ix.size == 0:
            return None
        lo = int(ix.min()) if lo is None else min(lo, int(ix.min()))
        hi = int(ix.max()) if hi is None else max(hi, int(ix.max()))
    return None if lo is None else (lo, hi)


def footprint(args: dict) -> dict:
    """Smallest and largest flat index the operation may read in A and B and read or write in C, and the extent of the
    list (``ntm`` whole rows of ``klist_stride``); None where nothing is touched.  A and B are taken as dense views: a
    list only ever leaves tiles out."""
    a = full(args)
    if a["m"] == 0 or a["n"] == 0 or a["batch"] == 0:
        return {"A": None, "B": None, "C": None, "klist": None}
    nb = a["batch"]
    ntm = (a["m"] + 63) // 64
    return {
        "A": _span(index_a, a, nb),
        "B": _span(index_b, a, nb),
        "C": _span(index_c, a, nb),
        "klist": (0, ntm * a["klist_stride"] - 1) if a["klist_stride"] > 0 else None,
    }


def footprint_enumerated(args: dict) -> dict:
    """The same by brute force: one Python loop over every (b, i, j, k) of the logical operation (small cases only)."""
    a = full(args)
    sp = {"A": None, "B": None, "C": None}

    def note(key, ix):
        lo, hi = sp[key] if sp[key] else (ix, ix)
        sp[key] = (min(lo, ix), max(hi, ix))

    for b in range(a["batch"]):
        for i in range(a["m"]):
            for j in range(a["n"]):
                rr = i + a["rowmap_r0"]
                off = ((rr % a["rowmap_p"]) * a["rowmap_s1"] + (rr // a["rowmap_p"]) * a["rowmap_s2"]) if a["rowmap_p"] else i * a["ldc"]
                note("C", a["offC"] + b * a["strideC"] + off + j)
                for k in range(a["k"]):
                    si = i + i // (a["arow_skip"] - 1) + 1 if a["arow_skip"] > 1 else i
                    note("A", a["offA"] + b * a["strideA"] + (k * a["lda"] + i if a["transA"] else si * a["lda"] + k))
                    note("B", a["offB"] + b * a["strideB"] + (j * a["ldb"] + k if a["transB"] else k * a["ldb"] + j))
    ntm = (a["m"] + 63) // 64
    sp["klist"] = (0, ntm * a["klist_stride"] - 1) if a["klist_stride"] > 0 and sp["C"] else None
    return sp


def apply(args: dict, A, B, C, klist=None) -> np.ndarray:
    """The expected WHOLE C buffer: owned elements alpha * P + beta * C, every other element as it came in."""
    a = full(args)
    A = np.asarray(A, dtype=np.complex128).reshape(-1)
    B = np.asarray(B, dtype=np.complex128).reshape(-1)
    out = np.array(C, dtype=np.complex128).reshape(-1).copy()
    if a["m"] == 0 or a["n"] == 0 or a["batch"] == 0:
        return out
    alpha, beta = complex(a["alpha"]), complex(a["beta"])
    mask = listed_mask(a, klist)
    for b in range(a["batch"]):
        opa = A[index_a(a, b)]
        opa = np.where(mask, opa, 0.0)  # unlisted tiles of A are zero, whatever lies there
        opb = B[index_b(a, b)]
        if a["conjA"]:
            opa = opa.conj()
        if a["conjB"]:
            opb = opb.conj()
        prod = opa @ opb if a["k"] > 0 else np.zeros((a["m"], a["n"]), np.complex128)
        ic = index_c(a, b)
        res = alpha * prod
        if beta != 0:  # beta == 0: C is overwritten without being read
            res = res + beta * out[ic]
        out[ic] = res
    return out


def owned_c(args: dict) -> np.ndarray:
    """flat indices of every element of C the operation owns"""
    a = full(args)
    if a["m"] == 0 or a["n"] == 0 or a["batch"] == 0:
        return np.zeros(0, np.int64)
    return np.concatenate([index_c(a, b).reshape(-1) for b in range(a["batch"])])


def layout(m, n, k, batch=1, transA=0, conjA=0, transB=0, conjB=0, pad=(0, 0, 0), bpad=(0, 0, 0), shared=(False, False),
           off=(3, 5, 7), **extra) -> dict:
    """Descriptor of plain (un-mapped) views: leading dimensions = logical row + pad[i], batch strides = operand + bpad[i]
    elements (0 for a shared A / B), first elements at ``off``.  ``extra`` overrides any field."""
    a = dict(m=m, n=n, k=k, batch=batch, transA=transA, conjA=conjA, transB=transB, conjB=conjB)
    skip = extra.get("arow_skip", 0)
    rows_a = k if transA else (stored_row_a({"arow_skip": skip}, m - 1) + 1 if m else 0)
    a["lda"] = (m if transA else k) + pad[0]
    a["ldb"] = (k if transB else n) + pad[1]
    a["ldc"] = n + pad[2]
    a["strideA"] = 0 if shared[0] else rows_a * a["lda"] + bpad[0]
    a["strideB"] = 0 if shared[1] else (n if transB else k) * a["ldb"] + bpad[1]
    a["strideC"] = m * a["ldc"] + bpad[2]
    a["offA"], a["offB"], a["offC"] = off
    a.update(extra)
    return full(a)


def draw(rng, shape, kind):
    """'int': real and imaginary parts integers in [-4, 4] (every partial sum of a product is then exact in any order);
    'gauss': standard normal"""
    if kind == "int":
        return rng.integers(-4, 5, shape).astype(np.float64) + 1j * rng.integers(-4, 5, shape).astype(np.float64)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def make_case(args: dict, rng, kind="int", klist=None, unlisted="nan"):
    """Canary buffers for a descriptor: (A, B, C) flat complex128.

    A and B are NaN everywhere except the elements the operation reads (so the pad between rows, between batches, before
    the first element, the stored rows that arow_skip leaves out, and -- ``unlisted='nan'`` -- the K tiles a list leaves
    out, are all NaN; ``unlisted='zero'`` puts exact zeros in those tiles).  C holds SENTINEL everywhere except its owned
    elements, which hold data, or NaN when beta == 0 (the product must overwrite them without reading).  Every buffer
    ends with a pad of at least 128 rows (128 x ld elements) after the last element of its view."""
    a = full(args)
    fp = footprint(a)
    nan = complex(np.nan, np.nan)

    def buf(span, off, ld, fill):
        last = span[1] if span else off
        return np.full(last + 1 + TILE_ROWS * max(int(ld), 1), fill, dtype=np.complex128)

    ldc_eff = max(a["ldc"], a["rowmap_s1"], a["rowmap_s2"], a["n"], 1) if a["rowmap_p"] else a["ldc"]
    A = buf(fp["A"], a["offA"], a["lda"], nan)
    B = buf(fp["B"], a["offB"], a["ldb"], nan)
    C = buf(fp["C"], a["offC"], ldc_eff, SENTINEL)
    if fp["C"] is None:
        return A, B, C
    mask = listed_mask(a, klist)
    for b in range(a["batch"] if a["strideA"] else 1):
        ia = index_a(a, b)
        vals = draw(rng, ia.shape, kind)
        if klist is not None:
            vals = np.where(mask, vals, nan if unlisted == "nan" else 0.0)
        A[ia] = vals
    for b in range(a["batch"] if a["strideB"] else 1):
        ib = index_b(a, b)
        B[ib] = draw(rng, ib.shape, kind)
    has_beta = complex(a["beta"]) != 0
    for b in range(a["batch"]):
        ic = index_c(a, b)
        C[ic] = draw(rng, ic.shape, kind) if has_beta else nan
    return A, B, C


def klist_rows(m: int, k: int, tiles_per_row_tile, stride=None) -> tuple[np.ndarray, int]:
    """The list in the format the engine writes: per 64-row tile a count followed by ascending tile indices, rows of
    ``stride`` (default 1 + K / 16) ints.  ``tiles_per_row_tile[tm]`` = the listed K tiles of row tile tm."""
    nkt, ntm = k // 16, (m + 63) // 64
    stride = (1 + nkt) if stride is None else stride
    assert stride >= 1 + nkt and len(tiles_per_row_tile) == ntm
    kl = np.zeros(ntm * stride, dtype=np.intc)  # unused slots are zero, as the engine leaves them
    for tm, tiles in enumerate(tiles_per_row_tile):
        tiles = sorted(int(t) for t in tiles)
        kl[tm * stride] = len(tiles)
        kl[tm * stride + 1:tm * stride + 1 + len(tiles)] = tiles
    return kl, stride
