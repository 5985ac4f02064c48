"""NumPy models of the building blocks of the batched-trajectory kernels (``csrc/batch_site.hip``), the table of cases
the host and GPU tests share, and the checkers that hold a result to its bars.

The blocks are what ``mitdvp_batch_block`` / ``engine.batch_block`` run in one workgroup: the workgroup product (32 x 32
output tiles, K in steps of 16) behind ``bt_matmul``, ``bt_heff``, ``bt_keff``, ``bt_env`` / ``bt_env_fwd`` and the overlap
walk; the Householder thin QR ``bt_qr``; the Jacobi split ``bp_jacobi`` + ``bp_select`` + ``bp_cprime``.

Models work on the PLAIN tensors (an MPO core is ``W[c, i, j, t]`` of shape (ml, d, d, mr)); ``operands`` packs them into
the layouts the kernels see.  ``dtype=np.clongdouble`` accumulates a product in extended precision.

Bars (the project's own for the same arithmetic):

* products   ``max|out - ref| < 1e-12 max|ref|`` (``test_heff_keff_env_vs_numpy``).  The complex128 model itself is held
  to 1e-13 against the extended-precision one in the host test.
* QR         ``max|Q^H Q - 1| < 1e-13``, ``max|Q R - A| <= 2e-13 max|A| sqrt(n)``, strict lower triangle of R exactly 0
  (``test_gpu_qr_gauge_free.py::_check``); Gaussian rows also against LAPACK up to the phases of diag(R), to 1e-11.
* split      see ``check_split``.  The projector bar applies where the row has a gap of at least 2 at r AND the direction
  of sigma_r can be resolved in double precision at all: by Wedin's theorem the projector onto the leading r right singular
  vectors moves by at most 2 |E| / (sigma_r - sigma_(r+1)) under a perturbation E, and any SVD in double precision has
  |E| >= eps |theta|; for LAPACK itself to meet a tenth of the bar, 1e-12, the absolute gap has to be about
  2 eps |theta| / 1e-12 = 4.4e-4 |theta|.  ``PROJ_MIN_GAP`` = 1e-3 |theta|_F is that figure rounded up; the host test
  checks on every flagged row that LAPACK, applied to the double-precision theta, is within 1e-12 of the projector of the
  construction.  (A geometric spectrum of ratio 0.5 has sigma_20 = 2e-6 and sigma_64 = 1e-19: the ratio at r is 2, the
  direction is below what the matrix holds.)  The ratio is taken on LAPACK's values with a relative slack ``GAP_SLACK``
  (a prescribed 2 comes back as 1.9999999999999996); with r = n the projector is the identity and the absolute gap does
  not matter.  ``PROJECTOR_EXEMPT`` names the rows whose prescribed ratio is at least 2 and which the absolute gap takes
  out, ``PROJECTOR_COUNT`` how many rows of each spectrum carry the bar: both tests assert them, so that neither list
  can drift.
"""

import zlib

import numpy as np

BP_TINY = 1e-28  # csrc/batch_site.hip: a row with |row|^2 <= BP_TINY |theta|^2 is rounding noise, not a direction
MAX_SITE, MAX_MPO, MAX_BOND, PAIR_MAX_DIM, MAX_COPIES, MAX_CHAIN = 8192, 16, 64, 128, 16, 6
PRODUCT_BAR, QR_ORTH_BAR, QR_REC_BAR, QR_LAPACK_BAR, QR_ROLES_BAR = 1e-12, 1e-13, 2e-13, 1e-11, 1e-12
SPLIT_ORTH_BAR, SPLIT_SV_RTOL, SPLIT_WEIGHT_BAR, SPLIT_PROJ_BAR, SPLIT_RANK_BAR = 1e-13, 1e-10, 1e-12, 1e-11, 1e-13
PROJ_MIN_GAP = 1e-3
GAP_SLACK = 1e-12  # relative, on the ratio sigma_r / sigma_(r+1) as LAPACK returns it
# prescribed sigma_r > 0 and sigma_r >= 2 sigma_(r+1), r < n, absolute gap below PROJ_MIN_GAP |theta|_F: (gap / |theta|_F)
PROJECTOR_EXEMPT = ("split-graded12-8x8-r4",       # 7e-6
                    "split-graded12-9x60-r9",      # 1e-12
                    "split-geometric-27x27-r20",   # 8e-7
                    "split-graded12-27x27-r20",    # 1e-9
                    "split-geometric-127x65-r64",  # 1e-19: below what the matrix holds
                    "split-geometric-128x128-r64", # 1e-19
                    "split-graded12-5x128-r5")     # 1e-12
# rows of each spectrum that carry the projector bar, of the nine shapes
PROJECTOR_COUNT = {"geometric": 6, "graded12": 3, "degenerate-cut": 5, "cluster": 9, "rank-1": 3, "rank-r-1": 3, "one-entry": 3}
TILE_EDGES = (1, 15, 16, 17, 31, 32, 33, 65)
CORNERS = ((64, 2, 64, 16, 16), (16, 32, 16, 16, 1), (1, 5, 1, 1, 1), (7, 3, 33, 5, 16), (33, 3, 7, 16, 5))


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def gauss(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ---------------------------------------------------------------------------------------------------------------- products
def matmul(A, B, dtype=np.complex128):
    return np.einsum("mk,kn->mn", A.astype(dtype), B.astype(dtype))


def heff(L, W, R, v, scl=1.0, dtype=np.complex128):
    """out[a,i,r] = sum L[a,c,b] W[c,i,j,t] R[r,t,s] (scl v)[b,j,s]"""
    X = np.einsum("acb,bjs->acjs", L.astype(dtype), (scl * v).astype(dtype))
    Y = np.einsum("cijt,acjs->aits", W.astype(dtype), X)
    return np.einsum("aits,rts->air", Y, R.astype(dtype))


def keff(L, R, v, scl=1.0, dtype=np.complex128):
    """out[a,r] = sum L[a,c,b] (scl v)[b,s] R[r,c,s]"""
    X = np.einsum("acb,bs->acs", L.astype(dtype), (scl * v).astype(dtype))
    return np.einsum("acs,rcs->ar", X, R.astype(dtype))


def env_fwd(env, W, bra, ket, dtype=np.complex128):
    """L'[a,q,r] = sum conj(bra[b,i,a]) env[b,p,s] W[p,i,j,q] ket[s,j,r]; bra, ket (din, d, dout), W (min, d, d, mout)"""
    X = np.einsum("bia,bps->iaps", bra.conj().astype(dtype), env.astype(dtype))
    Y = np.einsum("pijq,iaps->aqjs", W.astype(dtype), X)
    return np.einsum("aqjs,sjr->aqr", Y, ket.astype(dtype))


def env_bwd(env, W, bra, ket, dtype=np.complex128):
    """R'[a,c,r] = sum conj(bra[a,i,b]) env[b,t,s] W[c,i,j,t] ket[r,j,s]; bra, ket (dout, d, din), W (mout, d, d, min)"""
    X = np.einsum("aib,bts->iats", bra.conj().astype(dtype), env.astype(dtype))
    Y = np.einsum("cijt,iats->acjs", W.astype(dtype), X)
    return np.einsum("acjs,rjs->acr", Y, ket.astype(dtype))


def overlap(ket, bra, dtype=np.complex128):
    """<bra | ket> of two chains of site tensors (b_p, d, b_(p+1))"""
    T = np.ones((1, 1), dtype)
    for k, b in zip(ket, bra):
        U = np.einsum("mn,njs->mjs", T, k.astype(dtype))
        T = np.einsum("mji,mjs->is", b.conj().astype(dtype), U)
    return T[0, 0]


def pack_w2(W, order):
    """w2l[(i,t)][(c,j)], w2el[(t,j)][(i,c)], w2er[(c,j)][(i,t)] of W[c,i,j,t] (csrc/engine.h), by explicit loops"""
    ml, d, _, mr = W.shape
    shape = {"w2l": (d * mr, ml * d), "w2el": (mr * d, d * ml), "w2er": (ml * d, d * mr)}[order]
    out = np.zeros(shape, np.complex128)
    for c in range(ml):
        for i in range(d):
            for j in range(d):
                for t in range(mr):
                    if order == "w2l":
                        out[i * mr + t, c * d + j] = W[c, i, j, t]
                    elif order == "w2el":
                        out[t * d + j, i * ml + c] = W[c, i, j, t]
                    else:
                        out[c * d + j, i * mr + t] = W[c, i, j, t]
    return out


# ------------------------------------------------------------------------------------------------------------ the case table
def _matmul_cases():
    E = TILE_EDGES
    rows = [(E[i], E[(i + 3) % 8], E[(i + 5) % 8]) for i in range(8)]  # every edge as M, as N and as K
    rows += [(v, v, v) for v in (1, 17, 33, 65)]  # square: all three aliasings apply
    rows += [(33, 17, 17), (17, 33, 17), (65, 16, 16), (31, 65, 31)]  # N = K: dst = A; M = K: dst = B
    return [dict(op="matmul", name=f"matmul-{m}x{n}x{k}", dims=(m, n, k)) for m, n, k in rows]


# composite dimensions on the tile edges: (dl ml, d dr, ml d, d mr, dl dr, mr dr, dl d) reach 15, 17, 25, 31, 33, 65, ...
_MORE = ((5, 3, 5, 3, 5), (13, 5, 13, 5, 5), (17, 1, 17, 1, 1), (31, 1, 33, 1, 1), (33, 1, 31, 1, 1), (16, 2, 16, 1, 16),
         (15, 1, 15, 1, 1), (32, 1, 32, 1, 1), (1, 65, 1, 1, 1))


def _product_cases():
    rows = _matmul_cases()
    for q in CORNERS + _MORE:
        tag = "x".join(map(str, q))
        rows.append(dict(op="heff", name=f"heff-{tag}", dims=q, corner=q in CORNERS))
    for dim in (1, 17, 64):
        for m in (1, 16):
            rows.append(dict(op="keff", name=f"keff-{dim}-{m}", dims=(dim, m)))
    for q in CORNERS + _MORE[:5] + _MORE[7:]:
        dl, d, dr, ml, mr = q
        tag = "x".join(map(str, q))
        for role, variant, dims in (("fwd", 0, (dl, ml, d, dr, mr)), ("mirror", 1, (dr, mr, d, dl, ml)), ("fwdinst", 2, (dl, ml, d, dr, mr))):
            for same in ((True, False) if role != "fwdinst" else (False,)):
                rows.append(dict(op="env", name=f"env-{role}-{'sweep' if same else 'cross'}-{tag}", dims=dims, variant=variant,
                                 same=same, corner=q in CORNERS, plain=q))
    for L, d, bonds in ((1, 5, ()), (2, 32, (16,)), (2, 5, (13,)), (3, 3, (7, 33)), (4, 2, (2, 64, 17)), (6, 2, (2, 4, 8, 4, 2))):
        rows.append(dict(op="overlap", name=f"overlap-L{L}-d{d}-" + "-".join(map(str, bonds)), dims=(L, d) + bonds))
    return rows


QR_SHAPES = ((1, 1), (2, 2), (5, 3), (63, 8), (100, 9), (64, 64), (65, 64), (128, 64), (130, 33), (512, 16))
QR_KINDS = ("gauss", "product", "zerocol", "equalcols", "graded24", "tiny")
SPLIT_SHAPES = ((8, 8, 4), (9, 60, 9), (27, 27, 20), (60, 9, 9), (127, 65, 64), (128, 128, 64), (128, 16, 16), (1, 7, 1), (5, 128, 5))
SPLIT_KINDS = ("geometric", "graded12", "degenerate-cut", "cluster", "rank-1", "rank-r-1", "one-entry")


def _cases():
    rows = _product_cases()
    for m, n in QR_SHAPES:
        for kind in QR_KINDS:
            rows.append(dict(op="qr", name=f"qr-{kind}-{m}x{n}", dims=(m, n), kind=kind))
    for m, n, r in SPLIT_SHAPES:
        for kind in SPLIT_KINDS:
            rows.append(dict(op="split", name=f"split-{kind}-{m}x{n}-r{r}", dims=(m, n, r), kind=kind))
    for row in rows:
        row.setdefault("variant", 0)
    return rows


CASES = _cases()
BY_NAME = {r["name"]: r for r in CASES}


def gemm_dims(row):
    """(M, N, K) of every workgroup product the row's block runs"""
    q = row["dims"]
    if row["op"] == "matmul":
        return [q]
    if row["op"] == "heff":
        dl, d, dr, ml, mr = q
        return [(dl * ml, d * dr, dl), (d * mr, dl * dr, ml * d), (dl * d, dr, mr * dr)]
    if row["op"] == "keff":
        dim, m = q
        return [(dim * m, dim, dim), (dim, dim, m * dim)]
    if row["op"] == "env":
        din, mi, d, dout, mo = q
        return [(d * dout, mi * din, din), (mo * d, dout * din, d * mi), (dout * mo, dout, d * din)]
    if row["op"] == "overlap":
        L, d = q[:2]
        b = (1,) + tuple(q[2:]) + (1,)
        out = []
        for p in range(L):
            out += [(b[p], d * b[p + 1], b[p]), (b[p + 1], b[p + 1], b[p] * d)]
        return out
    return []


# --------------------------------------------------------------------------------------------------------------- the inputs
MPO_PHASE = np.exp(0.7j)  # on every core: a dropped conjugate, or one too many, shows


def split_spectrum(kind, m, n, r):
    """the prescribed singular values, descending, min(m, n) of them"""
    k = min(m, n)
    j = np.arange(k, dtype=float)
    if kind == "geometric":
        return 0.5 ** j
    if kind == "graded12":
        return 10.0 ** (-12.0 * j / max(k - 1, 1))
    if kind == "degenerate-cut":  # sigma_r = sigma_(r+1) exactly; with r = k nothing lies beyond the cut: the last two kept
        s = 0.8 ** j
        hi = min(r, k - 1)
        if hi >= 1:
            s[hi] = s[hi - 1]
            s[hi + 1:] = s[hi] * 0.8 ** np.arange(1, k - hi)
        return s
    if kind == "cluster":  # sigma_1, a cluster of three, a slope down to 0.2 at r, then 0.05 and halving: a gap of 4 at r
        s = np.empty(k)
        s[:r] = np.linspace(0.4, 0.2, r) if r > 1 else 0.2
        s[0] = 1.0 if r > 1 else 0.2
        s[1:min(4, r)] = 0.5
        s[r:] = 0.05 * 0.5 ** np.arange(k - r)
        return s
    if kind in ("rank-1", "rank-r-1"):
        rank = 1 if kind == "rank-1" else max(r - 1, 1)
        s = 0.7 ** j
        s[rank:] = 0.0
        return s
    raise ValueError(kind)


def _unitary(rng, n, k):
    return np.linalg.qr(gauss(rng, n, k))[0]


def split_input(row):
    """theta and, where it was built as U diag(s) V^H, its construction (s, V)"""
    m, n, r = row["dims"]
    rng = _rng(row["name"])
    if row["kind"] == "one-entry":
        theta = np.zeros((m, n), np.complex128)
        theta[m // 2, n // 3] = 0.3 - 0.4j
        return theta, None, None
    s = split_spectrum(row["kind"], m, n, r)
    k = min(m, n)
    U, V = _unitary(rng, m, k), _unitary(rng, n, k)
    return (U * s) @ V.conj().T, s, V


def qr_input(row):
    m, n = row["dims"]
    rng = _rng(row["name"])
    kind = row["kind"]
    A = gauss(rng, m, n)
    if kind == "product":  # a product state padded with zeros to the bond dimension: one non-zero column
        A[:, 1:] = 0.0
    elif kind == "zerocol":
        A[:, n // 2] = 0.0
    elif kind == "equalcols" and n > 1:  # (n = 1 has no second column: the row is then the Gaussian column)
        A[:, n - 1] = A[:, (n - 1) // 2]
    elif kind == "graded24":
        A = A * 10.0 ** (-24.0 * np.arange(n) / max(n - 1, 1))
    elif kind == "tiny":
        A = A * 1e-100
    return np.ascontiguousarray(A)


def product_input(row):
    """the plain tensors of a product row, in the order of the model's arguments"""
    rng = _rng(row["name"])
    q, op = row["dims"], row["op"]
    if op == "matmul":
        return gauss(rng, q[0], q[2]), gauss(rng, q[2], q[1])
    if op == "heff":
        dl, d, dr, ml, mr = q
        return gauss(rng, dl, ml, dl), MPO_PHASE * gauss(rng, ml, d, d, mr), gauss(rng, dr, mr, dr), gauss(rng, dl, d, dr)
    if op == "keff":
        dim, m = q
        return gauss(rng, dim, m, dim), gauss(rng, dim, m, dim), gauss(rng, dim, dim)
    if op == "env":
        din, mi, d, dout, mo = q
        fwd = row["variant"] != 1
        site = (din, d, dout) if fwd else (dout, d, din)
        W = MPO_PHASE * gauss(rng, *((mi, d, d, mo) if fwd else (mo, d, d, mi)))
        bra = gauss(rng, *site)
        ket = bra if row["same"] else gauss(rng, *site)
        return gauss(rng, din, mi, din), W, bra, ket
    if op == "overlap":
        L, d = q[:2]
        b = (1,) + tuple(q[2:]) + (1,)
        return [gauss(rng, b[p], d, b[p + 1]) for p in range(L)], [gauss(rng, b[p], d, b[p + 1]) for p in range(L)]
    raise ValueError(op)


HEFF_SCL = 0.37  # the factor 1 / beta a Krylov step puts on the vector


def model(row, plain, dtype=np.complex128):
    op = row["op"]
    if op == "matmul":
        return matmul(*plain, dtype=dtype)
    if op == "heff":
        return heff(*plain, scl=HEFF_SCL, dtype=dtype)
    if op == "keff":
        return keff(*plain, scl=HEFF_SCL, dtype=dtype)
    if op == "env":
        return (env_bwd if row["variant"] == 1 else env_fwd)(*plain, dtype=dtype)
    if op == "overlap":
        return np.array([overlap(*plain, dtype=dtype)])
    raise ValueError(op)


def operands(row, plain):
    """the four operands of engine.batch_block in the layouts the kernel sees (None: not taken)"""
    op = row["op"]
    if op == "matmul":
        return [plain[0], plain[1]]
    if op == "heff":
        L, W, R, v = plain
        return [L, pack_w2(W, "w2l"), R, v]
    if op == "keff":
        L, R, v = plain
        return [L, None, R, v]
    if op == "env":
        env, W, bra, ket = plain
        return [env, pack_w2(W, "w2er" if row["variant"] == 1 else "w2el"), bra, ket]
    if op == "overlap":
        ket, bra = plain
        return [np.concatenate([t.reshape(-1) for t in ket]), np.concatenate([t.reshape(-1) for t in bra])]
    raise ValueError(op)


def scl_of(row):
    return HEFF_SCL if row["op"] in ("heff", "keff") else 1.0


def footprint(row):
    """complex elements of the four operands and the two results, doubles of the info record, per copy"""
    q, op = row["dims"], row["op"]
    if op == "matmul":
        M, N, K = q
        return dict(ins=[M * K, K * N, 0, 0], out0=M * N, out1=0, info=1)
    if op == "heff":
        dl, d, dr, ml, mr = q
        return dict(ins=[dl * ml * dl, d * mr * ml * d, dr * mr * dr, dl * d * dr], out0=dl * d * dr, out1=0, info=1)
    if op == "keff":
        dim, m = q
        return dict(ins=[dim * m * dim, 0, dim * m * dim, dim * dim], out0=dim * dim, out1=0, info=1)
    if op == "env":
        din, mi, d, dout, mo = q
        return dict(ins=[din * mi * din, mo * d * d * mi, din * d * dout, din * d * dout], out0=dout * mo * dout, out1=0, info=1)
    if op == "overlap":
        L, d = q[:2]
        b = (1,) + tuple(q[2:]) + (1,)
        tot = sum(b[p] * d * b[p + 1] for p in range(L))
        return dict(ins=[tot, tot, 0, 0], out0=1, out1=0, info=1)
    if op == "qr":
        m, n = q
        return dict(ins=[m * n, 0, 0, 0], out0=m * n, out1=n * n, info=1)
    m, n, r = q
    return dict(ins=[m * n, 0, 0, 0], out0=r * n, out1=m * r, info=3 + m)


# ---------------------------------------------------------------------------------------------------------------- checkers
def product_defect(out, ref):
    return float(np.abs(np.asarray(out).reshape(-1) - np.asarray(ref, np.complex128).reshape(-1)).max() / np.abs(ref).max())


def check_qr(A, Q, R, lapack=False, margin=1.0):
    """the QR bars (times margin: the host test holds LAPACK to a tenth of them); returns the figures"""
    m, n = A.shape
    fig = dict(orth=float(np.abs(Q.conj().T @ Q - np.eye(n)).max()), rec=float(np.abs(Q @ R - A).max()),
               rec_bar=margin * QR_REC_BAR * float(np.abs(A).max()) * np.sqrt(n), lower=float(np.abs(np.tril(R, -1)).max()))
    assert fig["orth"] < margin * QR_ORTH_BAR, fig
    assert fig["rec"] <= fig["rec_bar"], fig
    assert fig["lower"] == 0.0, fig
    if lapack:
        q0, r0 = np.linalg.qr(A)
        ph = np.diag(R) / np.abs(np.diag(R))  # R = diag(ph) diag(ph0)^-1 R0, Q = Q0 diag(ph0) diag(ph)^-1
        ph0 = np.diag(r0) / np.abs(np.diag(r0))
        f = ph / ph0
        fig["lapack_q"] = float(np.abs(Q * f - q0).max())
        fig["lapack_r"] = float(np.abs(R / f[:, None] - r0).max() / np.abs(r0).max())
        assert fig["lapack_q"] < QR_LAPACK_BAR and fig["lapack_r"] < QR_LAPACK_BAR, fig
    return fig


def split_claims(row, theta):
    """what LAPACK says of the realised theta: singular values, the projector onto the leading r right singular vectors,
    whether the projector bar applies (see the module docstring)"""
    m, n, r = row["dims"]
    _, sv, vh = np.linalg.svd(theta, full_matrices=False)
    nf = float(np.linalg.norm(theta))
    nxt = sv[r] if r < len(sv) else 0.0
    # the ratio with the slack of LAPACK's own rounding (a prescribed ratio of exactly 2 comes back as 1.9999999999999996);
    # with r = n the projector is the identity whatever the spectrum, and B B^H = 1 already gives B^H B = 1 there
    ratio_ok = sv[r - 1] >= 2.0 * nxt * (1.0 - GAP_SLACK)
    gap_ok = r == n or (ratio_ok and sv[r - 1] - nxt >= PROJ_MIN_GAP * nf)
    P = vh[:r].conj().T @ vh[:r]
    rank = int((sv > 1e-13 * nf).sum())
    return dict(sv=sv, P=P, projector=bool(gap_ok), ratio=bool(ratio_ok), rank=rank, nf=nf)


def check_split(row, theta, B, Cp, info, claims=None, margin=1.0):
    """the split bars on one result: B (r x n), C' (m x r), info = [rc, kept, discarded fraction, sigma^2 descending]

    max|B B^H - 1| < 1e-13 on every row; sqrt(sigma^2) against LAPACK rtol 1e-10, atol 2 sqrt(BP_TINY) |theta|_F; kept
    weight and discarded fraction against LAPACK's sums to 1e-12 |theta|_F^2; | |theta - C' B|_F^2 - discarded | < 1e-12
    |theta|_F^2; with a resolvable gap of at least 2 at r, max|B^H B - P_ref| < 1e-11; with rank < r, max|C' B - theta| <
    1e-13 |theta|_F.  (margin scales every bar: the host test holds LAPACK to a tenth of them.)"""
    m, n, r = row["dims"]
    c = claims or split_claims(row, theta)
    nf, sv = c["nf"], c["sv"]
    assert info[0] == 0.0, f"return code {info[0]}"
    fig = dict(orth=float(np.abs(B @ B.conj().T - np.eye(r)).max()))
    assert fig["orth"] < margin * SPLIT_ORTH_BAR, fig
    got = np.sqrt(np.maximum(info[3:3 + m], 0.0))
    assert np.all(np.diff(info[3:3 + m]) <= 0.0), "the squared row norms are not in descending order"
    want = np.zeros(m)
    want[:len(sv)] = sv
    err = np.abs(got - want) - margin * SPLIT_SV_RTOL * want
    fig["sv"] = float(err.max())
    fig["sv_atol"] = margin * 2.0 * np.sqrt(BP_TINY) * nf
    assert fig["sv"] <= fig["sv_atol"], fig
    kept, disc = float((sv[:r] ** 2).sum()), float((sv[r:] ** 2).sum())
    fig["kept"] = abs(info[1] - kept) / nf**2
    fig["disc"] = abs(info[2] * nf**2 - disc) / nf**2
    assert fig["kept"] < margin * SPLIT_WEIGHT_BAR and fig["disc"] < margin * SPLIT_WEIGHT_BAR, fig
    res = float(np.linalg.norm(theta - Cp @ B) ** 2)
    fig["residual"] = abs(res - info[2] * nf**2) / nf**2
    assert fig["residual"] < margin * SPLIT_WEIGHT_BAR, fig
    if c["projector"]:
        fig["proj"] = float(np.abs(B.conj().T @ B - c["P"]).max())
        assert fig["proj"] < margin * SPLIT_PROJ_BAR, fig
    if c["rank"] < r:
        fig["exact"] = float(np.abs(Cp @ B - theta).max() / nf)
        assert fig["exact"] < margin * SPLIT_RANK_BAR, fig
    return fig


def lapack_split(theta, r):
    """the split LAPACK gives, in the form of the hook's results: B, C', info"""
    m = theta.shape[0]
    _, sv, vh = np.linalg.svd(theta, full_matrices=True)
    B = vh[:r]  # full_matrices: an orthonormal completion where the rank is below r
    info = np.zeros(3 + m)
    s2 = np.zeros(m)
    s2[:len(sv)] = sv**2
    info[3:] = s2
    info[1] = s2[:r].sum()
    info[2] = s2[r:].sum() / s2.sum()
    return B, theta @ B.conj().T, info
