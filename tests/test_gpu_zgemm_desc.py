"""GPU: the MFMA zgemm over its whole descriptor (``mitdvp_zgemm_desc``) against the NumPy model ``helpers.zgemm_ref``.

Operands lie as views in canary buffers (``zgemm_ref.make_case``): NaN around A and B, a finite sentinel around C, NaN in
the owned part of C when beta == 0.  Integer-valued cases (parts in [-4, 4], Gaussian-integer alpha and beta) are exact in
any summation order, in the 4M and the 3M product and through the split-K combine (every partial sum is an integer far
below 2^53 for K <= 4096), so the WHOLE returned C buffer must equal the model's bit for bit: owned elements, pads and
skipped rows at once.  One Gaussian case per family is held to the bar of the packed tests (test_gpu_kernels.py):
max|out - ref| < 1e-13 max|ref|, times sqrt(K) on the split-K path, and a second call must be bitwise the first.

Figures of one run on an MI355X: profiles/zgemm_desc_tests.txt.
"""

import math
import time

import numpy as np
import pytest

from helpers import zgemm_ref as zr

pytestmark = pytest.mark.gpu

MODES = (0, 1)
ALL_TILES = (-1, 0, 1, 2)
ALPHA, BETA = 2 - 1j, -1 + 3j
STATS = {}  # family -> [calls, worst Gaussian defect relative to its bar's scale]
T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for fam, (calls, worst) in STATS.items():
        print(f"\n[zgemm_desc] family {fam}: {calls} kernel cases, worst Gaussian defect {worst:.3e}")
    print(f"\n[zgemm_desc] module wall time {time.time() - T0:.1f} s")


def note(fam, calls=0, defect=0.0):
    s = STATS.setdefault(fam, [0, 0.0])
    s[0] += calls
    s[1] = max(s[1], defect)


def expected_splits(a, tile, m3):
    """The dispatch rule of zgemm() restated: number of K slabs the product is split into (1 = not split).  Only the
    short-output rule can fire at these sizes (the long-K rule needs K >= 8192)."""
    a = zr.full(a)
    m, n, k, batch = a["m"], a["n"], a["k"], a["batch"]
    assert k < 8192

    def tiles(bm, bn):
        return -(-m // bm) * -(-n // bn) * batch

    cfg = tile
    if cfg < 0:
        t64 = tiles(64, 64)
        cfg = 1 if (t64 >= 256 or (t64 >= 16 and k >= 1024 and batch == 1)) else 2
    nt = tiles(128, 64 if m3 else 128) if cfg == 0 else tiles(32, 32) if cfg == 2 else tiles(64, 64)
    if a["klist_stride"] or batch != 1 or a["rowmap_p"] or not (nt < 192 and k >= 1024):
        return 1
    splits = min((512 + nt - 1) // nt, k // 256)
    if splits < 2:
        return 1
    kc = -(-k // splits)
    kc = (kc + 15) // 16 * 16
    return -(-k // kc)


def compare(out, ref, a, kind, what, sqrt_k=False):
    """int: the whole buffer bit for bit; gauss: everything the operation does not own bit for bit, the owned part at the
    bar.  Returns the Gaussian defect max|out - ref| / max|ref|."""
    own = zr.owned_c(a)
    assert not np.isnan(out[own]).any(), f"{what}: NaN in the owned part of C -- pad (or a skipped row, or an unlisted tile) was read"
    if kind == "int":
        if not np.array_equal(out, ref):
            bad = np.flatnonzero(out != ref)
            inside = np.isin(bad, own)
            raise AssertionError(f"{what}: {bad.size} elements differ from the model ({(~inside).sum()} of them outside the owned "
                                 f"part), first at flat index {bad[0]}: {out[bad[0]]} vs {ref[bad[0]]}")
        return 0.0
    rest = np.ones(out.size, bool)
    rest[own] = False
    assert np.array_equal(out[rest], ref[rest]), f"{what}: an element outside the owned part of C changed"
    scale = np.abs(ref[own]).max()
    err = np.abs(out[own] - ref[own]).max() / scale
    bar = 1e-13 * (math.sqrt(zr.full(a)["k"]) if sqrt_k else 1.0)
    print(f"[zgemm_desc] {what}: defect {err:.3e} (bar {bar:.1e})")
    assert err < bar, f"{what}: {err:.3e} >= {bar:.1e}"
    return err


def run(fam, a, seed, kind="int", klist=None, tiles=ALL_TILES, modes=MODES, unlisted="nan", split=False, twice=None):
    """one descriptor at every (mode, tile) its path allows, against the model computed once"""
    from pytdscf_amd import engine as E

    rng = np.random.default_rng(seed)
    A, B, C0 = zr.make_case(a, rng, kind, klist, unlisted)
    ref = zr.apply(a, A, B, C0, klist)
    twice = (kind == "gauss") if twice is None else twice
    for mode in modes:
        for tile in tiles:
            what = f"{fam} {a['m']}x{a['n']}x{a['k']} b={a['batch']} t={a['transA']}{a['conjA']}{a['transB']}{a['conjB']} " \
                   f"ld=({a['lda']},{a['ldb']},{a['ldc']}) beta={a['beta']} mode3m={mode} tile={tile} {kind}"
            if split:
                assert expected_splits(a, tile, mode) >= 2, what
            d = dict(a, mode3m=mode, tile_cfg=tile)
            out = E.zgemm_desc(d, A, B, C0, klist)
            err = compare(out, ref, a, kind, what, sqrt_k=split)
            if twice:
                assert np.array_equal(out, E.zgemm_desc(d, A, B, C0, klist)), f"{what}: a second call differs bitwise"
            note(fam, 1, err)


# ---------------------------------------------------------------------------------------------------- 1. views
VIEW_SHAPES = [(150, 77, 45), (33, 65, 130), (1, 5, 300), (64, 64, 16)]
FORMS = {"NN": (0, 0, 0, 0), "NT": (0, 0, 1, 0), "TN": (1, 0, 0, 0), "TT": (1, 0, 1, 0), "NC": (0, 0, 1, 1), "CN": (1, 1, 0, 0),
         "CC": (1, 1, 1, 1)}
LD_PADS = [(0, 0, 0)] + [tuple(p if q == w else 0 for q in range(3)) for p in (1, 7, 67) for w in range(3)] + \
          [(1, 1, 1), (7, 7, 7), (67, 67, 67)]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", VIEW_SHAPES)
def test_views(shape, form):
    """batch 1: every leading dimension packed, +1, +7, +67, one at a time and all together, operands at non-zero offsets;
    K = 45 and K = 130 put pad directly behind column K - 1 of every row of the peeled K tail."""
    tA, cA, tB, cB = FORMS[form]
    for i, pad in enumerate(LD_PADS):
        for beta, tiles in ((BETA, ALL_TILES), (0.0, (-1,))) if i % 2 else ((0.0, ALL_TILES), (BETA, (-1,))):
            a = zr.layout(*shape, transA=tA, conjA=cA, transB=tB, conjB=cB, pad=pad, off=(3 + i, 5, 7 + 2 * i), alpha=ALPHA, beta=beta)
            run("views", a, seed=i, tiles=tiles)


@pytest.mark.parametrize("form", ["NN", "NC", "CN", "TT"])
def test_views_gaussian(form):
    tA, cA, tB, cB = FORMS[form]
    a = zr.layout(150, 77, 45, transA=tA, conjA=cA, transB=tB, conjB=cB, pad=(7, 67, 1), alpha=0.7 - 0.2j, beta=-0.3 + 1.1j)
    run("views", a, seed=11, kind="gauss")


# ---------------------------------------------------------------------------------------------------- 2. batch
@pytest.mark.parametrize("shape", [(150, 77, 45), (33, 9, 20)])
@pytest.mark.parametrize("batch", [2, 3, 17])
def test_batch_strides(shape, batch):
    """packed and padded batch strides, a shared A, a shared B, both shared with distinct C slabs"""
    for i, (bpad, shared) in enumerate([((0, 0, 0), (False, False)), ((5, 11, 3), (False, False)), ((0, 0, 9), (True, False)),
                                        ((4, 0, 0), (False, True)), ((0, 0, 2), (True, True))]):
        tB = i % 2
        a = zr.layout(*shape, batch=batch, transB=tB, conjB=tB, pad=(i, 2 * i, 3 * i), bpad=bpad, shared=shared, alpha=ALPHA,
                      beta=BETA if i % 2 == 0 else 0.0)
        run("batch", a, seed=100 + i)


def test_batch_engine_forms():
    """the descriptors of the call sites, at small sizes"""
    # W stage, dense: A shared, strideB = min * d * ncol, strideC = d * mout * ncol
    d, mout, min_, ncol, nb = 3, 14, 5, 35, 4
    a = zr.layout(d * mout, ncol, min_ * d, batch=nb, shared=(True, False), alpha=1.0, beta=0.0)
    assert a["strideA"] == 0 and a["strideB"] == min_ * d * ncol and a["strideC"] == d * mout * ncol
    run("batch", a, seed=120)
    # site_rdm: rho_a[j][j'] = U_a[j][s] conj(C_a[j'][s])
    dl, d, dr = 6, 4, 9
    a = zr.layout(d, d, dr, batch=dl, transB=1, conjB=1, alpha=1.0, beta=0.0)
    assert (a["ldb"], a["ldc"], a["strideA"], a["strideB"], a["strideC"]) == (dr, d, d * dr, d * dr, d * d)
    run("batch", a, seed=121)
    # qr.hip, the batched pair products: all three strides equal, all three leading dimensions n, operands inside n x n
    n, b = 24, 4
    pairs, stride = n // (2 * b), 2 * b * (n + 1)
    a = zr.full(dict(m=b, n=b, k=b, batch=pairs, lda=n, ldb=n, ldc=n, strideA=stride, strideB=stride, strideC=stride,
                     offA=3 + b, offB=5 + b * (n + 1), offC=7 + b, alpha=-1.0, beta=0.0))
    run("batch", a, seed=122)
    run("batch", dict(a, beta=BETA, alpha=ALPHA), seed=123)


def test_batch_one_leg_reduced_density_loop():
    """T'_(o,j)[s][s'] = sum_a' U_o[a'][j][s] conj(C[a'][j][s']): one batched call per j, operands based at + j dr inside
    rows of d dr, C interleaved across j with strideC = d dr dr -- all j into the same C buffer."""
    from pytdscf_amd import engine as E

    no, dl, d, dr = 3, 5, 4, 6
    rng = np.random.default_rng(130)
    nan = complex(np.nan, np.nan)
    offU, offC, offT = 3, 5, 7
    U = np.full(offU + no * dl * d * dr + 128 * d * dr, nan)
    Cs = np.full(offC + dl * d * dr + 128 * d * dr, nan)
    U[offU:offU + no * dl * d * dr] = zr.draw(rng, no * dl * d * dr, "int")
    Cs[offC:offC + dl * d * dr] = zr.draw(rng, dl * d * dr, "int")
    T0_ = np.full(offT + no * d * dr * dr + 128 * dr, zr.SENTINEL)
    T0_[offT:offT + no * d * dr * dr] = nan  # beta == 0: overwritten without being read
    for mode in MODES:
        for tile in ALL_TILES:
            out, ref = T0_, T0_
            for j in range(d):
                a = zr.full(dict(m=dr, n=dr, k=dl, batch=no, transA=1, conjB=1, lda=d * dr, ldb=d * dr, ldc=dr, strideA=dl * d * dr,
                                 strideB=0, strideC=d * dr * dr, offA=offU + j * dr, offB=offC + j * dr, offC=offT + j * dr * dr,
                                 mode3m=mode, tile_cfg=tile))
                out = E.zgemm_desc(a, U, Cs, out)
                ref = zr.apply(a, U, Cs, ref)
                note("batch", 1)
            assert not np.isnan(out[offT:offT + no * d * dr * dr]).any(), "NaN in T': pad was read, or a slab was not written"
            assert np.array_equal(out, ref), (mode, tile)
    Um, Cm = U[offU:offU + no * dl * d * dr].reshape(no, dl, d, dr), Cs[offC:offC + dl * d * dr].reshape(dl, d, dr)
    assert np.array_equal(ref[offT:offT + no * d * dr * dr].reshape(no, d, dr, dr), np.einsum("oajs,ajt->ojst", Um, Cm.conj()))


def test_batch_65535_of_one_by_one():
    """the largest batch the grid takes (blockIdx.y); the expectation is written out, the model's per-batch loop is slow"""
    from pytdscf_amd import engine as E

    nb = 65535
    rng = np.random.default_rng(140)
    a = zr.layout(1, 1, 1, batch=nb, alpha=ALPHA, beta=BETA)
    assert (a["strideA"], a["strideB"], a["strideC"], a["offA"], a["offB"], a["offC"]) == (1, 1, 1, 3, 5, 7)
    A, B = np.full(3 + nb + 128, complex(np.nan, np.nan)), np.full(5 + nb + 128, complex(np.nan, np.nan))
    C0 = np.full(7 + nb + 128, zr.SENTINEL)
    A[3:3 + nb], B[5:5 + nb], C0[7:7 + nb] = zr.draw(rng, nb, "int"), zr.draw(rng, nb, "int"), zr.draw(rng, nb, "int")
    ref = C0.copy()
    ref[7:7 + nb] = ALPHA * (A[3:3 + nb] * B[5:5 + nb]) + BETA * C0[7:7 + nb]
    for mode in MODES:
        out = E.zgemm_desc(dict(a, mode3m=mode), A, B, C0)
        assert np.array_equal(out, ref), mode
        note("batch", 1)


def test_batch_gaussian():
    a = zr.layout(150, 77, 45, batch=3, transB=1, conjB=1, pad=(7, 1, 67), bpad=(5, 0, 3), shared=(False, True), alpha=0.7 - 0.2j,
                  beta=-0.3 + 1.1j)
    run("batch", a, seed=141, kind="gauss")


# ---------------------------------------------------------------------------------------------------- 3. split-K
SPLIT_SHAPES = [(40, 24, 1029), (40, 24, 1040), (70, 130, 4100), (1, 1, 1024)]


def split_form(form, m, n, k, beta=BETA):
    if form == "NN lda=K+5":
        return zr.layout(m, n, k, pad=(5, 0, 0), alpha=ALPHA, beta=0.0)
    if form == "K_eff":  # A a column window of a wider matrix, B transposed and packed (keff_apply_compact, second stage)
        return zr.layout(m, n, k, transB=1, pad=(3 * n, 0, 0), off=(3 + n, 5, 7), alpha=1.0, beta=0.0)
    if form == "TN lda=M+3":
        return zr.layout(m, n, k, transA=1, conjA=1, pad=(3, 0, 0), alpha=-1.0, beta=beta)
    assert form == "ldc=N+5 beta"
    return zr.layout(m, n, k, pad=(0, 0, 5), alpha=ALPHA, beta=beta)


SPLIT_FORMS = ["NN lda=K+5", "K_eff", "TN lda=M+3", "ldc=N+5 beta"]


@pytest.mark.parametrize("form", SPLIT_FORMS)
@pytest.mark.parametrize("shape", SPLIT_SHAPES)
def test_split_k_with_views(shape, form):
    a = split_form(form, *shape)
    assert a["ldb"] == shape[2] or form != "K_eff"
    run("split-K", a, seed=200, split=True, twice=True)


@pytest.mark.parametrize("form", SPLIT_FORMS)
def test_split_k_gaussian(form):
    a = split_form(form, 40, 24, 1029, beta=0.5 + 0.25j)
    run("split-K", a, seed=201, kind="gauss", split=True)


def test_split_k_with_arow_skip_and_no_row_map():
    """the engine never issues it, zgemm() accepts it: the skipped stored rows (NaN here) stay out of every K slab"""
    for skip in (2, 3, 5):
        a = zr.layout(40, 24, 1029, pad=(5, 0, 3), arow_skip=skip, alpha=ALPHA, beta=BETA)
        run("split-K", a, seed=210 + skip, split=True)


# ---------------------------------------------------------------------------------------------------- 4. row map, row skip
def w_stage_args(d, mout, min_, ncol, nb, r0, m, **kw):
    """a row range [r0, r0 + m) of W2 in the (q, i) row order, Y's rows mapped back to (i, q); A shared by the slabs"""
    k = min_ * d
    assert r0 % d == 0 and m % d == 0 and r0 + m <= d * mout
    return zr.full(dict(m=m, n=ncol, k=k, batch=nb, lda=k, ldb=ncol, ldc=ncol, strideA=0, strideB=min_ * d * ncol,
                        strideC=d * mout * ncol, offA=3 + r0 * k, offB=5, offC=7, rowmap_p=d, rowmap_s1=mout * ncol, rowmap_s2=ncol,
                        rowmap_r0=r0, **kw))


@pytest.mark.parametrize("k_tiles", [9, 208])  # K = 45 and 1040: a mapped product is never split, however long K is
def test_row_map_w_stage(k_tiles):
    d, mout, ncol, nb = 5, 40, 77, 3
    for r0, m, beta in ((15, 150, 0.0), (5, 35, BETA), (0, 200, BETA)):
        a = w_stage_args(d, mout, k_tiles, ncol, nb, r0, m, alpha=ALPHA, beta=beta)
        assert expected_splits(a, -1, 1) == 1
        run("rowmap", a, seed=300 + r0, tiles=(-1, 1, 2) if k_tiles == 9 else (1,))


def trimmed_args(ml, na, row, k, **kw):
    """stage S1 with an identity block in MPO-bond state 0: A = L (na ml stored rows, every ml-th left out), C = X + row"""
    return zr.full(dict(m=na * (ml - 1), n=row, k=k, lda=k, ldb=row, ldc=row, offA=3, offB=5, offC=7 + row, arow_skip=ml,
                        rowmap_p=ml - 1, rowmap_s1=row, rowmap_s2=ml * row, rowmap_r0=0, **kw))


@pytest.mark.parametrize("ml", [2, 3, 4, 5])
def test_trimmed_heff_stage(ml):
    """ml = 4: groups of 3 rows, so the 64-row tile boundary falls inside a group.  The skipped stored rows of A are NaN;
    the rows of C of MPO-bond state 0 hold the sentinel and come back untouched (the whole-buffer comparison)."""
    na, row = 50, 77
    for k, beta in ((50, 0.0), (50, BETA), (1040, BETA)):
        a = trimmed_args(ml, na, row, k, alpha=ALPHA, beta=beta)
        assert expected_splits(a, 1, 1) == 1 and expected_splits(dict(a, rowmap_p=0), 1, 1) >= (2 if k >= 1024 else 1)
        A, B, C0 = zr.make_case(a, np.random.default_rng(0), "int")
        assert np.isnan(A[3:3 + na * ml * k].reshape(na, ml, k)[:, 0]).all() and not np.isnan(A[3:3 + na * ml * k].reshape(na, ml, k)[:, 1:]).any()
        assert np.all(C0[7:7 + na * ml * row].reshape(na, ml, row)[:, 0] == zr.SENTINEL)
        run("rowmap", a, seed=320 + ml, tiles=(1,))


def test_keff_compact_row_map():
    """X[a][ci][s] = Lc[(a, ci)][b] sig[b][s] into rows of ldx > n1 d2"""
    d1, n1, d2, nx = 50, 3, 24, 5
    a = zr.full(dict(m=d1 * n1, n=d2, k=d1, lda=d1, ldb=d2, ldc=d2, offA=3, offB=5, offC=7, rowmap_p=n1, rowmap_s1=d2,
                     rowmap_s2=nx * d2, alpha=ALPHA, beta=0.0))
    run("rowmap", a, seed=340)
    run("rowmap", dict(a, beta=BETA), seed=341)


def test_row_map_gaussian():
    run("rowmap", trimmed_args(4, 50, 77, 50, alpha=0.7 - 0.2j, beta=-0.3 + 1.1j), seed=350, kind="gauss", tiles=(1,))
    run("rowmap", w_stage_args(5, 40, 9, 77, 3, 15, 150, alpha=1.0, beta=0.0), seed=351, kind="gauss", tiles=(-1, 1, 2))


# ---------------------------------------------------------------------------------------------------- 5. block-sparse lists
def lists_for(m, k, rng):
    nkt, ntm = k // 16, (m + 63) // 64

    def half():
        return [sorted(rng.choice(nkt, size=(nkt + 1) // 2, replace=False).tolist()) for _ in range(ntm)]

    some = half()
    some[ntm // 2] = []
    return {
        "all": zr.klist_rows(m, k, [range(nkt)] * ntm),
        "half": zr.klist_rows(m, k, half()),
        "first": zr.klist_rows(m, k, [[0]] * ntm),
        "last": zr.klist_rows(m, k, [[nkt - 1]] * ntm),
        "one row tile empty": zr.klist_rows(m, k, some),
        "wide stride": zr.klist_rows(m, k, half(), stride=1 + nkt + 5),
    }


@pytest.mark.parametrize("n", [64, 77])
@pytest.mark.parametrize("m", [64, 150, 200])
@pytest.mark.parametrize("k", [16, 64, 208])
def test_block_sparse_lists(k, m, n):
    """the unlisted tiles of A hold NaN: the product must equal the model with zeros there; the rows of a row tile with an
    empty list must equal beta * C"""
    rng = np.random.default_rng(k * 1000 + m + n)
    for i, (name, (kl, stride)) in enumerate(lists_for(m, k, rng).items()):
        for beta in (BETA, 0.0) if name == "one row tile empty" else (BETA if i % 2 else 0.0,):
            a = zr.layout(m, n, k, pad=(i % 2, 0, 3 * (i % 3)), klist_stride=stride, alpha=ALPHA, beta=beta)
            run("lists", a, seed=400 + i, klist=kl, tiles=(1,))


def test_block_sparse_w_stage_form():
    """the full form of the W stage: list, row map, r0, three slabs, A shared"""
    d, mout, min_, ncol, nb, r0, m = 5, 40, 16, 77, 3, 15, 150
    rng = np.random.default_rng(450)
    kl, stride = lists_for(m, min_ * d, rng)["one row tile empty"]
    for beta in (0.0, BETA):
        a = w_stage_args(d, mout, min_, ncol, nb, r0, m, klist_stride=stride, alpha=ALPHA, beta=beta)
        run("lists", a, seed=451, klist=kl, tiles=(1,))


def test_block_sparse_gaussian_is_bitwise_the_dense_product():
    """exact zeros in the unlisted tiles: skipping them leaves the product bit-identical to the dense call at the same tile
    and mode (the claim above Engine::w_stage, checked at the kernel)"""
    from pytdscf_amd import engine as E

    m, n, k = 150, 77, 208
    rng = np.random.default_rng(460)
    kl, stride = lists_for(m, k, rng)["one row tile empty"]
    a = zr.layout(m, n, k, pad=(1, 0, 3), klist_stride=stride, alpha=0.7 - 0.2j, beta=-0.3 + 1.1j)
    A, B, C0 = zr.make_case(a, rng, "gauss", kl, unlisted="zero")
    ref = zr.apply(a, A, B, C0, kl)
    for mode in MODES:
        d = dict(a, mode3m=mode, tile_cfg=1)
        out = E.zgemm_desc(d, A, B, C0, kl)
        err = compare(out, ref, a, "gauss", f"lists gaussian mode3m={mode}")
        assert np.array_equal(out, E.zgemm_desc(d, A, B, C0, kl))
        assert np.array_equal(out, E.zgemm_desc(dict(d, klist_stride=0), A, B, C0, None)), "the list form is not bitwise the dense one"
        note("lists", 3, err)


# ---------------------------------------------------------------------------------------------------- 6. degenerate sizes
def test_empty_products_leave_c_alone():
    from pytdscf_amd import engine as E

    base = zr.layout(33, 9, 20, batch=2, pad=(1, 2, 3), alpha=ALPHA, beta=BETA)
    A, B, C0 = zr.make_case(base, np.random.default_rng(500), "int")
    C0[::5] = complex(np.nan, -0.0)  # bitwise: NaN payloads and signed zeros included
    for zero in ("m", "n", "batch"):
        for tile in ALL_TILES:
            out = E.zgemm_desc(dict(base, tile_cfg=tile, **{zero: 0}), A, B, C0)
            assert out.tobytes() == C0.tobytes(), (zero, tile)
            note("degenerate", 1)


def test_k_zero_scales_c_by_beta():
    """K = 0: the K loop of zgemm_kernel runs no tile, its accumulators stay zero and the epilogue stores
    alpha * 0 + beta * C -- C = beta * C, and zero (not what C held) when beta == 0.  A and B are never read."""
    for beta in (BETA, 0.0):
        for batch in (1, 3):
            a = zr.layout(70, 33, 0, batch=batch, pad=(4, 2, 5), bpad=(0, 0, 6), alpha=ALPHA, beta=beta)
            run("degenerate", a, seed=510)
    a = trimmed_args(3, 20, 9, 0, alpha=ALPHA, beta=BETA)
    run("degenerate", a, seed=511, tiles=(1,))
