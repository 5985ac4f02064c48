"""Models, bars and the case table of the Krylov vector and layout kernels of ``csrc/vecops.hip``, as the test hook
``mitdvp_vecop`` / ``engine.vecop`` runs them (``tests/test_gpu_vecops.py``, ``tests/test_vecops_host.py``).

Every model is a few lines of NumPy above double precision: ``numpy.longdouble`` where it has a 64-bit mantissa, otherwise
complex128 elementwise with ``math.fsum`` for the sums.  No bar comes from a device run; each stands next to its model, with
u = 2^-53:

* pure movement: the bits of the source, and every element outside the written set keeps the bits it had (the results are
  pre-filled with NaNs of distinct payloads);
* elementwise arithmetic: ``|dev - ref|_i <= c u M_i`` per component, M_i the sum of the moduli of the terms of element i, c the
  roundings on its longest chain plus one for FMA contraction; a scalar that comes from partials adds its own bound
  ``(NPART + 2) u sum|p|`` (a root: that over twice the root, plus one rounding; an inverse: one division) times the modulus
  of what it multiplies (twice that for a complex scalar: both components of its error reach each component);
* reductions: the partial array is summed on the host and compared at ``(n_terms + 4) u sum|terms|``, which holds for any
  order of summation; n_terms counts the REAL terms of one component (2 n for a complex dot or a sum of squares over n
  elements: each element contributes two real products to either component), hence the ``2 * n + 4`` in the code;
  moduli are drawn from [0.5, 2], so that one lost or doubled element moves a sum by 0.25 at least;
* ``ident_deviation``: the bits of the same expression in double (every step is one correctly rounded operation or an
  exact maximum), 1e308 where an element is not finite.

A model returns, per result buffer, a *spec*: ``elem`` (reference, bar and written mask per element; bar 0 = the bits),
``sum`` (k groups of NPART partials against k references) or ``first`` (``[0]`` = value, ``[1..255]`` = +0.0).  ``render``
turns specs into the buffers a device that computed the model would return, so that the host test can show that a mutated
model (``MUTATIONS``) misses the table.
"""

import math

import numpy as np

U = 2.0 ** -53
NPART, MAXK, SMALL_VEC_N, GUARD = 256, 21, 16384, 5
EXTENDED = np.finfo(np.longdouble).eps < 2.0 ** -60
XR = np.longdouble if EXTENDED else np.float64
XC = np.clongdouble if EXTENDED else np.complex128

MUTATIONS = ("drop_last", "p0", "p64", "ld_cols", "no_bs", "no_map2", "swap12", "conj_flip", "no_orthodox", "no_zero_to",
             "no_pos0", "nan_fmax", "slot0")


# ------------------------------------------------------------------------------------------------------------ small tools
def xsum(t, axis=-1):
    """the sum of real or complex terms above double precision"""
    t = np.asarray(t)
    if EXTENDED:
        return np.sum(t.astype(XC if np.iscomplexobj(t) else XR), axis=axis)
    t = np.moveaxis(t, axis, -1)
    flat = t.reshape(-1, t.shape[-1])
    if np.iscomplexobj(t):
        out = np.array([complex(math.fsum(r.real), math.fsum(r.imag)) for r in flat])
    else:
        out = np.array([math.fsum(r) for r in flat])
    return out.reshape(t.shape[:-1])


def sentinel(n, cplx=True, salt=0):
    """n NaNs of distinct payloads (complex: in both components)"""
    m = 2 * n if cplx else n
    b = np.uint64(0x7FF8DEAD00000000) + np.uint64(salt << 24) + np.arange(m, dtype=np.uint64)
    d = b.view(np.float64)
    return d.view(np.complex128) if cplx else d


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def rand_c(rng, *shape, scale=1.0):
    """complex numbers of modulus in [0.5, 2] * scale and any phase"""
    return scale * rng.uniform(0.5, 2.0, shape) * np.exp(2j * np.pi * rng.uniform(size=shape))


def split_c(rng, value):
    """NPART complex partials, none negligible, that sum to value within roundoff"""
    r = rng.standard_normal(NPART) + 1j * rng.standard_normal(NPART)
    return value / NPART + abs(value) * (r - r.mean())


def split_r(rng, value):
    """NPART positive partials that sum to value within roundoff"""
    r = rng.uniform(size=NPART)
    return value / NPART * (1.0 + (r - r.mean()))


def take(p, mut):
    """the partials a consumer sums, and the bound on that sum: (NPART + 2) u sum|p|"""
    q = p[:1] if "p0" in mut else p[:64] if "p64" in mut else p
    return xsum(q), (NPART + 2) * U * float(np.abs(p).sum())


def root(s, es):
    """sqrt(s) and its bound: the sum's over twice the root, plus one rounding"""
    b = np.sqrt(XR(s))
    return b, (es / (2 * float(b)) + U * float(b)) if b > 0 else 0.0


# ------------------------------------------------------------------------------------------------------------------ specs
def elem(init, where=None, ref=None, bar=None):
    """``where``: flat indices written; ref / bar: their values (bar 0 or None = bit equality)"""
    n = init.size
    cplx = np.iscomplexobj(init)
    R = np.zeros(n, XC if cplx else XR)
    B = np.zeros(n)
    W = np.zeros(n, bool)
    if where is not None and np.size(where):
        where = np.asarray(where).reshape(-1)
        W[where] = True
        R[where] = np.asarray(ref).reshape(-1)
        if bar is not None:
            B[where] = np.broadcast_to(np.asarray(bar, dtype=np.float64), np.shape(ref)).reshape(-1)
    return dict(kind="elem", init=init, ref=R, bar=B, written=W)


def sums(init, ref, bar, minterm, kind="sum"):
    ref = np.atleast_1d(ref)
    return dict(kind=kind, init=init, ref=ref, bar=np.atleast_1d(np.asarray(bar, dtype=np.float64)), k=ref.size, minterm=float(minterm))


def dot_spec(init, a, b, mut=(), kind="sum"):
    """partials of sum a_i b_i (a already conjugated where it is), a and b of shape (k, n) or (n,)"""
    t = np.atleast_2d(a).astype(XC) * np.atleast_2d(b).astype(XC)
    if "drop_last" in mut:
        t = t[:, :-1]
    n = t.shape[1]
    m = np.abs(t).astype(np.float64)
    # n_terms = 2 n: either component of the sum has two real products per element
    return sums(init, xsum(t), (2 * n + 4) * U * m.sum(axis=1), m.min() if m.size else 0.0, kind)


def sumsq_spec(init, v, ebar=None, mut=(), kind="sum"):
    """partials of sum |v_i|^2 for elements the device holds within ebar of v"""
    v = np.asarray(v).reshape(-1)
    if "drop_last" in mut:
        v = v[:-1]
        ebar = None if ebar is None else np.asarray(ebar).reshape(-1)[:-1]
    m = np.abs(v).astype(np.float64)
    t = m.astype(XR) ** 2 if not EXTENDED else (np.abs(v.astype(XC)) ** 2)
    bar = (2 * v.size + 4) * U * float(np.sum(m * m))  # n_terms = 2 n real squares
    if ebar is not None:  # | |v + e|^2 - |v|^2 | <= 2 sqrt(2) |v| e + 2 e^2 for a componentwise bound e
        e = np.asarray(ebar, dtype=np.float64).reshape(-1)
        bar += float(np.sum(3 * m * e + 2 * e * e))
    return sums(init, xsum(t), bar, (m * m).min() if m.size else 0.0, kind)


def judge(spec, got):
    """(ok, defect, bar, what): the largest defect of the arithmetic elements with its bar, and what failed"""
    init = spec["init"]
    got = np.asarray(got).reshape(-1)
    cplx = np.iscomplexobj(init)
    per = 2 if cplx else 1
    if spec["kind"] == "elem":
        W, B = spec["written"], spec["bar"]
        keep = ~W
        if not np.array_equal(bits(got).reshape(-1, per)[keep], bits(init).reshape(-1, per)[keep]):
            return False, np.inf, 0.0, "an element outside the written set changed"
        exact = W & (B == 0)
        ref64 = spec["ref"].astype(init.dtype)
        if not np.array_equal(bits(got).reshape(-1, per)[exact], bits(ref64).reshape(-1, per)[exact]):
            return False, np.inf, 0.0, "a moved element has other bits"
        ar = W & (B > 0)
        if not ar.any():
            return True, 0.0, 0.0, ""
        d = got[ar].astype(spec["ref"].dtype) - spec["ref"][ar]
        d = np.maximum(np.abs(d.real), np.abs(d.imag)).astype(np.float64) if cplx else np.abs(d).astype(np.float64)
        d = np.where(np.isnan(d), np.inf, d)
        ratio = d / B[ar]
        j = int(np.argmax(ratio))
        return bool(ratio[j] <= 1.0), float(d[j]), float(B[ar][j]), "" if ratio[j] <= 1.0 else "an element misses its bar"
    k = spec["k"]
    tail = slice(k * NPART, None)
    if not np.array_equal(bits(got[tail]), bits(init[tail])):
        return False, np.inf, 0.0, "a guard element behind the partials changed"
    p = got[: k * NPART].reshape(k, NPART)
    if spec["kind"] == "first" and not np.array_equal(bits(p[:, 1:]), bits(np.zeros_like(p[:, 1:]))):
        return False, np.inf, 0.0, "partials [1..255] are not +0.0"
    d = xsum(p) - spec["ref"]
    d = np.maximum(np.abs(d.real), np.abs(d.imag)).astype(np.float64) if cplx else np.abs(d).astype(np.float64)
    d = np.where(np.isnan(d), np.inf, d)
    ratio = d / spec["bar"]
    j = int(np.argmax(ratio))
    return bool(ratio[j] <= 1.0), float(d[j]), float(spec["bar"][j]), "" if ratio[j] <= 1.0 else "a sum misses its bar"


def render(spec):
    """the buffer a device that computed exactly the model would return"""
    out = spec["init"].copy()
    if spec["kind"] == "elem":
        W = spec["written"]
        out[W] = spec["ref"][W].astype(out.dtype)
        return out
    k = spec["k"]
    out[: k * NPART] = 0
    out[np.arange(k) * NPART] = spec["ref"].astype(out.dtype)
    return out


# ----------------------------------------------------------------------------------------------------------------- inputs
def _rng(row):
    return np.random.default_rng(abs(hash_name(row["name"])) % (1 << 32))


def hash_name(s):
    h = 2166136261
    for ch in s.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


def result(n, data=None, cplx=True, salt=0):
    """a result buffer of n elements and GUARD behind them, all sentinels but ``data`` (flat index -> value pairs)"""
    buf = sentinel(n + GUARD, cplx, salt)
    if data is not None:
        buf[data[0]] = data[1]
    return buf


def mat_idx(rows, cols, ld, off=0):
    return (off + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]).reshape(-1)


def build(row):
    """the buffers and scalars of one row: dict(z, r, idx, mask, zo, ro, a, b, both, eps, coef, f)"""
    rng = _rng(row)
    op, d, s, v = row["op"], row["dims"], row["strides"], row["variant"]
    g = dict(z=[None, None, None], r=None, idx=None, mask=(1 << 64) - 1, zo=[None, None], ro=None, a=1.0, b=0.0, both=0.0,
             eps=row.get("eps", 1e-12), coef=(), f=())
    part = lambda: result(NPART, cplx=False, salt=3)  # noqa: E731
    n = d[0]
    if op == "dot":
        g["z"][:2] = rand_c(rng, n), rand_c(rng, n)
        g["zo"][0] = result(NPART, salt=1)
    elif op == "sumsq":
        g["z"][0] = rand_c(rng, n)
        g["ro"] = part()
    elif op == "lanczos_update":
        g["zo"][0] = result(n, (np.arange(n), rand_c(rng, n, scale=6.0)))
        g["z"][0], g["z"][2] = rand_c(rng, n), split_c(rng, 0.4 * np.exp(1j * rng.uniform(0, 6)))
        if v & 1:
            g["z"][1], g["r"] = rand_c(rng, n), split_r(rng, 0.16)
        g["ro"] = part()
    elif op == "lanczos_update_def":
        l = d[1]
        g["zo"][0] = result(n, (np.arange(n), rand_c(rng, n, scale=10.0)))
        g["z"][0], g["z"][2] = rand_c(rng, n), split_c(rng, 0.4 * np.exp(1j * rng.uniform(0, 6)))
        if v & 1:
            g["z"][1] = rand_c(rng, n)
        nrm = np.full((max(l, 1), NPART), np.nan)  # rows other than l - 1 and l - 2 may not matter
        if l > 0:
            nrm[l - 1] = split_r(rng, 1.5625)
        if l > 1:
            nrm[l - 2] = split_r(rng, 4.0)
        g["r"] = nrm.reshape(-1)
        g["ro"] = part()
    elif op == "lanczos_step_small":
        # alpha = <x | w> is a sum of n terms of modulus 2 .. 8 and would grow like sqrt(n), its bound like n, and alpha vl
        # would swamp w.  So the TERMS t_i = conj(x_i) w_i are drawn and made to cancel -- in pairs to a part in 1e4, the
        # last three of an odd n as a triangle -- and w = t / conj(x): every term still counts, alpha stays below 0.1.
        x, t = rand_c(rng, n), rand_c(rng, n, scale=4.0)
        h = (n - 3 * (n % 2)) // 2
        if h > 0:
            t[h:2 * h] = -t[:h] * (1 + 1e-4 * rng.standard_normal(h))
        if n % 2 and n >= 3:
            t[n - 3:] = t[n - 1] * np.exp(2j * np.pi * np.arange(3) / 3)
        vl = rand_c(rng, n) if v & 2 else x
        if n == 1:  # nothing to cancel with: moduli of 2 keep w - alpha vl away from 0
            x, vl = 2 * x / abs(x), 2 * vl / abs(vl)
        g["zo"][0] = result(n, (np.arange(n), t / np.conj(x)))
        g["z"][0] = vl
        if v & 2:
            g["z"][1] = x
        if v & 1:
            g["z"][2], g["r"] = rand_c(rng, n), split_r(rng, 0.0016)
        g["zo"][1], g["ro"] = result(NPART, salt=2), part()
    elif op == "scale_inv_norm":
        g["zo"][0] = result(n, (np.arange(n), rand_c(rng, n)))
        g["r"] = split_r(rng, row.get("norm2", 6.25))
        if row.get("nan_norm"):
            g["r"][77] = np.nan
    elif op in ("multi_dot", "arnoldi_update", "lincomb"):
        k, ldv = d[1], s[0]
        V = sentinel((k - 1) * ldv + n, salt=5)
        V[mat_idx(k, n, ldv)] = rand_c(rng, k * n)
        g["z"][0] = V
        if op == "multi_dot":
            g["z"][1], g["zo"][0] = rand_c(rng, n), result(k * NPART, salt=1)
        elif op == "arnoldi_update":
            g["z"][1] = np.concatenate([split_c(rng, 0.05 * np.exp(1j * rng.uniform(0, 6))) for _ in range(k)])
            g["zo"][0], g["ro"] = result(n, (np.arange(n), rand_c(rng, n, scale=6.0))), part()
        else:
            g["coef"] = [3.0 * np.exp(1j * rng.uniform(0, 6))] + list(rand_c(rng, k - 1, scale=0.01))
            if v & 1:
                g["zo"][0] = result(n)
            if v & 2:
                g["ro"] = part()
    elif op in ("axpby", "scale"):
        g["zo"][0] = result(n, (np.arange(n), rand_c(rng, n)))
        g["a"], g["b"] = 0.3 - 0.7j, -1.1 + 0.2j
        if op == "axpby":
            g["z"][0] = rand_c(rng, n)
    elif op == "transpose":
        rows, cols, batch = d
        g["z"][0] = rand_c(rng, (batch - 1) * s[2] + (rows - 1) * s[0] + cols)
        g["zo"][0] = result((batch - 1) * s[3] + (cols - 1) * s[1] + rows)
    elif op in ("transpose_rev3", "permute_0213", "copy_raw"):
        tot = int(np.prod(d))
        g["z"][0], g["zo"][0] = rand_c(rng, tot), result(tot)
    elif op == "permute5":
        if v & 1:
            g["idx"] = row["map2"]
        last2 = max(row["map2"]) if v & 1 else d[2] - 1
        g["z"][0] = rand_c(rng, 1 + sum((last2 if k == 2 else d[k] - 1) * s[k] for k in range(5)))
        g["zo"][0] = result(int(np.prod(d)))
    elif op == "phys_diag":
        dl, nn, dr = d
        g["z"][0] = rand_c(rng, dl * nn * nn * dr)
        g["zo"][0] = result(dl * dr if v & 1 else dl * nn * dr)
    elif op == "copy2d":
        rows, cols, zt = d
        w = max(cols, zt)
        g["a"] = row["a"]
        g["z"][0] = rand_c(rng, (rows - 1) * s[1] + cols)
        g["zo"][0] = result((rows - 1) * s[0] + w, (mat_idx(rows, w, s[0]), rand_c(rng, rows * w)))
    elif op == "identity":
        g["zo"][0] = result((d[0] - 1) * s[0] + d[1])
    elif op == "scale_cols":
        rows, cols = d
        g["zo"][0] = result((rows - 1) * s[0] + cols, (mat_idx(rows, cols, s[0]), rand_c(rng, rows * cols)))
        g["r"] = rng.uniform(0.5, 2.0, cols) * rng.choice([-1.0, 1.0], cols)
    elif op == "gather_blocks":
        rows, cols, nbl, n_dst, m_src = d
        g["idx"] = row["blk"]
        g["z"][0], g["zo"][0] = rand_c(rng, rows * m_src * cols), result(rows * n_dst * cols)
    elif op == "fill_scaled_blocks":
        rows, cols, nbl, pos0 = d
        g["f"] = list(rand_c(rng, nbl))
        g["z"][0], g["zo"][0] = rand_c(rng, rows * cols), result((rows - 1) * s[0] + (pos0 + nbl) * cols)
    elif op == "accum_scaled_blocks":
        rows, cols, nbl = d
        g["idx"], g["f"], g["both"] = row["blk"], list(rand_c(rng, nbl)), 0.6 - 0.9j
        w = (max(row["blk"]) + 1 if nbl else 0) * cols
        X = sentinel(max((rows - 1) * s[0] + w, 1), salt=5)
        if w:
            X[mat_idx(rows, w, s[0])] = rand_c(rng, rows * w)
        g["z"][0], g["z"][1] = X, rand_c(rng, rows * cols)
        g["zo"][0] = result(rows * cols, (np.arange(rows * cols), rand_c(rng, rows * cols)))
    elif op in ("col_sumsq", "row_sumsq"):
        g["z"][0] = rand_c(rng, d[0] * d[1])
        g["ro"] = result(d[1] if op == "col_sumsq" else d[0], cplx=False, salt=3)
    elif op == "shell_sumsq":
        g["z"][0], g["ro"] = rand_c(rng, n * n), result(n, cplx=False, salt=3)
    elif op == "ident_dev":
        ld, off = s[0], row.get("off", 0)
        buf = rand_c(rng, off + (n - 1) * ld + n)
        blk = np.eye(n, dtype=complex)
        kind = row["kind"]
        i, j = int(rng.integers(n)), int(rng.integers(n))
        if kind == "off":
            blk[n - 1, 0 if n > 1 else n - 1] += 0.125 - 0.375j
        elif kind == "imag":
            blk[n // 2, n // 2] += 3e-7j
        elif kind in ("nan", "+inf", "-inf"):
            blk[i, j] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[kind] * (1 if (i + j) % 2 else 1j)
        buf[mat_idx(n, n, ld, off)] = blk.reshape(-1)
        g["z"][0], g["ro"] = buf[off:], result(1, cplx=False, salt=3)
    elif op == "ident_dev_multi":
        nn, nblk = d
        ld, bs = s
        buf = rand_c(rng, (nblk - 1) * bs + (nn - 1) * ld + nn)
        for c in range(nblk):
            lam = rand_c(rng, 1)[0]
            blk = lam * np.eye(nn, dtype=complex)
            if c == row["bad"]:
                blk[nn - 1, 0] += 0.25j if nn > 1 else 0.0
                blk[nn // 2, nn // 2] += 0.5
            buf[mat_idx(nn, nn, ld, c * bs)] = blk.reshape(-1)
        g["z"][0], g["mask"] = buf, row["mask"]
        g["zo"][1] = result(nblk, salt=2)
        g["ro"] = result(nblk, cplx=False, salt=3)
        if not v & 1:  # no clear: the maximum with what the buffer held (non-negative)
            g["ro"][:nblk] = np.where(np.arange(nblk) % 2 == 0, 0.0, 0.4)
    else:
        raise ValueError(op)
    return g


# ----------------------------------------------------------------------------------------------------------------- models
def expect(row, g, mut=()):
    """the specs of the result buffers of one row: dict(zo0=, zo1=, ro=), a missing key = a buffer the op does not take"""
    op, d, s, v = row["op"], list(row["dims"]), list(row["strides"]), row["variant"]
    z, zo, ro = g["z"], g["zo"], g["ro"]
    C = lambda x: np.asarray(x).astype(XC)  # noqa: E731
    n = d[0]
    if op == "dot":
        x = z[0] if not (v ^ ("conj_flip" in mut)) else np.conj(z[0])
        return dict(zo0=dot_spec(zo[0], x, z[1], mut))
    if op == "sumsq":
        return dict(ro=sumsq_spec(ro, z[0], None, mut))
    if op == "lanczos_update":
        # x = v - alpha a - bp c per component: two products and a subtraction for alpha a, one product and one
        # subtraction for bp c: 5 roundings, + 1
        alpha, ea = take(z[2], mut)
        vv, a = C(zo[0][:n]), C(z[0])
        x, M = vv - alpha * a, np.abs(vv) + abs(alpha) * np.abs(a)
        bar = 2 * ea * np.abs(a)
        if v & 1:
            bp, eb = root(*take(g["r"], mut))
            c = C(z[1])
            x, M, bar = x - bp * c, M + bp * np.abs(c), bar + eb * np.abs(c)
        bar = (bar + 6 * U * M).astype(np.float64)
        w = np.arange(n - 1 if "drop_last" in mut else n)
        return dict(zo0=elem(zo[0], w, x[w], bar[w]), ro=sumsq_spec(ro, x, bar, mut))
    if op == "lanczos_update_def":
        l, eps, nrm = d[1], g["eps"], g["r"].reshape(-1, NPART)
        invb_l = invb_m = XR(1.0)
        beta = XR(0.0)
        e_beta = r_l = r_m = 0.0  # absolute bound of beta_prev, relative bounds of the two inverses
        if l > 0:
            beta, e_beta = root(*take(nrm[l - 1], mut))
            if beta >= eps:
                invb_l, r_l = 1 / beta, e_beta / float(beta) + U
        if l > 1:
            b2, e2 = root(*take(nrm[l - 2], mut))
            if b2 >= eps:
                invb_m, r_m = 1 / b2, e2 / float(b2) + U
        raw, ea = take(z[2], mut)
        fa = invb_l * invb_l if (v & 2) and "no_orthodox" not in mut else invb_l
        alpha = raw * fa
        ea = 2 * ea * float(fa) + float(abs(alpha)) * (2 * r_l + 3 * U)
        vv, a = C(zo[0][:n]), C(z[0])
        t0, t1 = np.abs(vv) * invb_l, abs(alpha) * np.abs(a) * invb_l
        x, M = vv * invb_l - alpha * (a * invb_l), t0 + t1
        bar = r_l * (t0 + t1) + 2 * ea * np.abs(a) * float(invb_l)
        if v & 1:
            c = C(z[1])
            t2 = beta * np.abs(c) * invb_m
            x, M, bar = x - beta * (c * invb_m), M + t2, bar + (e_beta * float(invb_m) + float(beta) * float(invb_m) * r_m) * np.abs(c)
        # longest chain: the scaling of ul, two products and a subtraction, the subtraction from x, then scaling, product
        # and subtraction of the third term: 7, + 1
        bar = (bar + 8 * U * M).astype(np.float64)
        w = np.arange(n - 1 if "drop_last" in mut else n)
        return dict(zo0=elem(zo[0], w, x[w], bar[w]), ro=sumsq_spec(ro, x, bar, mut))
    if op == "lanczos_step_small":
        m = min(n, 1024) if "slot0" in mut else n - 1 if "drop_last" in mut else n
        w0, vl = C(zo[0][:m]), C(z[0][:m])
        xx = C(z[1][:m]) if v & 2 else vl
        da = dot_spec(zo[1], np.conj(xx), w0, kind="first")
        alpha, ea = da["ref"][0], float(da["bar"][0])
        if "alpha_dev" in g:  # the update and the norm from the alpha the device returned: its bound drops out of both
            alpha, ea = XC(g["alpha_dev"]), 0.0
        x, M, bar = w0 - alpha * vl, np.abs(w0) + abs(alpha) * np.abs(vl), 2 * ea * np.abs(vl)
        if v & 1:
            bp, eb = root(*take(g["r"], mut))
            c = C(z[2][:m])
            x, M, bar = x - bp * c, M + bp * np.abs(c), bar + eb * np.abs(c)
        bar = (bar + 6 * U * M).astype(np.float64)
        ns = sumsq_spec(ro, x, bar, kind="first")
        beta, eb = root(ns["ref"][0], float(ns["bar"][0]))
        if beta >= g["eps"]:  # w = x / beta: the relative bound of the inverse, and one more rounding
            inv = 1 / beta
            bar = bar * float(inv) + np.abs(x).astype(np.float64) * float(inv) * (eb / float(beta) + 2 * U)
            x = x * inv
        return dict(zo0=elem(zo[0], np.arange(m), x, bar), zo1=da, ro=ns)
    if op == "scale_inv_norm":
        sm, es = take(g["r"], mut)
        beta, eb = root(sm, es) if sm == sm else (XR(np.nan), 0.0)
        if not beta >= g["eps"]:
            return dict(zo0=elem(zo[0]))
        x = C(zo[0][:n]) / beta
        w = np.arange(n - 1 if "drop_last" in mut else n)
        return dict(zo0=elem(zo[0], w, x[w], (np.abs(x).astype(np.float64) * (eb / float(beta) + 2 * U))[w]))
    if op in ("multi_dot", "arnoldi_update", "lincomb"):
        k, ldv = d[1], n if "ld_cols" in mut else s[0]
        V = z[0][mat_idx(k, n, ldv)].reshape(k, n)
        if op == "multi_dot":
            return dict(zo0=dot_spec(zo[0], np.conj(V), np.broadcast_to(z[1], (k, n)), mut))
        Vx = C(V)
        if op == "arnoldi_update":
            h = [take(z[1][j * NPART:(j + 1) * NPART], mut) for j in range(k)]
            vv = C(zo[0][:n])
            x, M, bar = vv.copy(), np.abs(vv), np.zeros(n, XR)
            for j in range(k):
                x, M, bar = x - h[j][0] * Vx[j], M + abs(h[j][0]) * np.abs(Vx[j]), bar + 2 * h[j][1] * np.abs(Vx[j])
            bar = (bar + (3 * k + 1) * U * M).astype(np.float64)  # three roundings per vector, + 1
            w = np.arange(n - 1 if "drop_last" in mut else n)
            return dict(zo0=elem(zo[0], w, x[w], bar[w]), ro=sumsq_spec(ro, x, bar, mut))
        c = C(g["coef"])
        x = (c[:, None] * Vx).sum(axis=0)
        bar = ((3 * k + 1) * U * (np.abs(c)[:, None] * np.abs(Vx)).sum(axis=0)).astype(np.float64)
        out = {}
        w = np.arange(n - 1 if "drop_last" in mut else n)
        if v & 1:
            out["zo0"] = elem(zo[0], w, x[w], bar[w])
        if v & 2:
            out["ro"] = sumsq_spec(ro, x, bar, mut)
        return out
    if op == "axpby":  # four products and three additions, the longest chain has 4 roundings, + 1
        a, b, x, y = XC(g["a"]), XC(g["b"]), C(z[0]), C(zo[0][:n])
        w = np.arange(n - 1 if "drop_last" in mut else n)
        return dict(zo0=elem(zo[0], w, (a * x + b * y)[w], (5 * U * (abs(a) * np.abs(x) + abs(b) * np.abs(y))).astype(np.float64)[w]))
    if op == "scale":  # two products and a subtraction, + 1
        a, y = XC(g["a"]), C(zo[0][:n])
        w = np.arange(n - 1 if "drop_last" in mut else n)
        return dict(zo0=elem(zo[0], w, (a * y)[w], (3 * U * abs(a) * np.abs(y)).astype(np.float64)[w]))
    if op == "transpose":
        rows, cols, batch = d
        ldi, ldo, ibs, obs = s[:4]
        if "ld_cols" in mut:
            ldi, ldo = cols, rows
        if "no_bs" in mut:
            ibs = obs = 0
        b, r, c = np.meshgrid(np.arange(batch), np.arange(rows), np.arange(cols), indexing="ij")
        src, dst = (b * ibs + r * ldi + c).reshape(-1), (b * obs + c * ldo + r).reshape(-1)
        if "drop_last" in mut:
            src, dst = src[:-1], dst[:-1]
        return dict(zo0=elem(zo[0], dst, z[0][src]))
    if op in ("transpose_rev3", "permute_0213", "copy_raw", "permute5", "gather_blocks"):
        tot = int(np.prod(d[:5])) if op != "gather_blocks" else 0
        if op == "transpose_rev3":
            src = np.arange(tot).reshape(d[:3]).transpose(2, 1, 0).reshape(-1)
        elif op == "permute_0213":
            src = np.arange(tot).reshape(d[:4])
            src = (src if "swap12" in mut else src.transpose(0, 2, 1, 3)).reshape(-1)
        elif op == "copy_raw":
            src = np.arange(tot)
        elif op == "permute5":
            ix = np.indices(d[:5]).reshape(5, -1)
            if v & 1 and "no_map2" not in mut:
                ix[2] = np.asarray(g["idx"])[ix[2]]
            src = sum(ix[k] * s[k] for k in range(5))
        else:
            rows, cols, nbl, n_dst, m_src = d
            a, k, c = np.meshgrid(np.arange(rows), np.arange(nbl), np.arange(cols), indexing="ij")
            src = ((a * m_src + np.asarray(g["idx"], dtype=int).reshape(-1)[k.reshape(-1)].reshape(k.shape)) * cols + c).reshape(-1) if nbl else np.zeros(0, int)
            dst = ((a * n_dst + k) * cols + c).reshape(-1)
            if "drop_last" in mut:
                src, dst = src[:-1], dst[:-1]
            return dict(zo0=elem(zo[0], dst, z[0][src]))
        dst = np.arange(tot)
        if "drop_last" in mut:
            src, dst = src[:-1], dst[:-1]
        return dict(zo0=elem(zo[0], dst, z[0][src]))
    if op == "phys_diag":
        dl, nn, dr = d
        Cc = z[0].reshape(dl, nn, nn, dr)
        dg = np.stack([Cc[:, c, c, :] for c in range(nn)], axis=1) if nn else np.zeros((dl, 0, dr), complex)
        if v & 1:  # n - 1 additions per component, + 1
            return dict(zo0=elem(zo[0], np.arange(dl * dr), xsum(dg, axis=1).reshape(-1), (nn * U * np.abs(dg).sum(axis=1)).reshape(-1)))
        return dict(zo0=elem(zo[0], np.arange(dl * nn * dr), dg.reshape(-1)))
    if op == "copy2d":
        rows, cols, zt = d
        ldd, lds = s[:2]
        if "no_zero_to" in mut:
            zt = 0
        w = max(cols, zt)
        if "ld_cols" in mut:
            ldd, lds = w, cols
        di, si = mat_idx(rows, cols, ldd), mat_idx(rows, cols, lds)
        a, src = XC(g["a"]), C(z[0][si])
        if g["a"] == 1 and not v & 1:
            val, bar = src, np.zeros(si.size)
        else:  # two products and a subtraction (and the addition of dst), + 1
            val, M = a * src, abs(a) * np.abs(src)
            if v & 1:
                val, M = val + C(zo[0][di]), M + np.abs(zo[0][di])
            bar = ((4 if v & 1 else 3) * U * M).astype(np.float64)
        zi = (np.arange(rows)[:, None] * ldd + np.arange(cols, w)[None, :]).reshape(-1)
        return dict(zo0=elem(zo[0], np.concatenate([di, zi]), np.concatenate([val, np.zeros(zi.size, XC)]),
                             np.concatenate([bar, np.zeros(zi.size)])))
    if op == "identity":
        rows, cols = d
        ld = cols if "ld_cols" in mut else s[0]
        return dict(zo0=elem(zo[0], mat_idx(rows, cols, ld), np.eye(rows, cols, dtype=complex).reshape(-1)))
    if op == "scale_cols":  # one product per component, + 1
        rows, cols = d
        ix = mat_idx(rows, cols, cols if "ld_cols" in mut else s[0])
        sc = np.tile(g["r"], rows)
        return dict(zo0=elem(zo[0], ix, C(zo[0][ix]) * sc.astype(XR), 2 * U * np.abs(zo[0][ix]) * np.abs(sc)))
    if op == "fill_scaled_blocks":  # two products and a subtraction, + 1
        rows, cols, nbl, pos0 = d
        if "no_pos0" in mut:
            pos0 = 0
        a, k, c = np.meshgrid(np.arange(rows), np.arange(nbl), np.arange(cols), indexing="ij")
        dst = (a * s[0] + (pos0 + k) * cols + c).reshape(-1)
        if not nbl:
            return dict(zo0=elem(zo[0]))
        f, sg = C(g["f"])[k.reshape(-1)], C(z[0])[(a * cols + c).reshape(-1)]
        return dict(zo0=elem(zo[0], dst, f * sg, (3 * U * np.abs(f) * np.abs(sg)).astype(np.float64)))
    if op == "accum_scaled_blocks":  # three roundings per term (both sig, then the nbl blocks in order), + 1
        rows, cols, nbl = d
        sg, o = C(z[1]).reshape(rows, cols), C(zo[0][:rows * cols]).reshape(rows, cols)
        val, M = o + XC(g["both"]) * sg, np.abs(o) + abs(g["both"]) * np.abs(sg)
        for k in range(nbl):
            Xk = C(z[0][mat_idx(rows, cols, s[0], g["idx"][k] * cols)]).reshape(rows, cols)
            val, M = val + XC(g["f"][k]) * Xk, M + abs(g["f"][k]) * np.abs(Xk)
        return dict(zo0=elem(zo[0], np.arange(rows * cols), val.reshape(-1), ((3 * (nbl + 1) + 1) * U * M).astype(np.float64).reshape(-1)))
    if op in ("col_sumsq", "row_sumsq", "shell_sumsq"):
        if op == "shell_sumsq":
            x = z[0].reshape(n, n)
            groups = [np.concatenate([x[t, :t + 1], x[:t, t]]) for t in range(n)]
        else:
            x = z[0].reshape(d[0], d[1])
            groups = list(x.T) if op == "col_sumsq" else list(x)
        if "drop_last" in mut:
            groups = [q[:-1] for q in groups]
        m2 = [np.abs(q).astype(np.float64) ** 2 for q in groups]
        ref = [xsum(np.abs(C(q)) ** 2) if q.size else XR(0) for q in groups]
        bar = [(2 * q.size + 4) * U * float(t.sum()) for q, t in zip(groups, m2)]
        sp = elem(ro, np.arange(len(groups)), np.array(ref, XR), np.array(bar))
        sp["minterm"] = min((float(t.min()) for t in m2 if t.size), default=np.inf)
        return dict(ro=sp)
    if op in ("ident_dev", "ident_dev_multi"):
        def dev_of(blk, lam):
            nn = blk.shape[0]
            eye = np.eye(nn, dtype=bool)
            with np.errstate(invalid="ignore"):
                dv = np.where(eye, np.maximum(np.abs(blk.real - lam.real), np.abs(blk.imag - lam.imag)),
                              np.maximum(np.abs(blk.real), np.abs(blk.imag)))
                bad = ~(np.isfinite(blk.real) & np.isfinite(blk.imag)) | np.isnan(dv)
            if "nan_fmax" in mut:
                dv = np.where(bad, 0.0, dv)
            else:
                dv = np.where(bad, 1e308, dv)
            return float(dv.max()) if dv.size else 0.0
        ONE = np.complex128(1.0)
        if op == "ident_dev":
            ld = n if "ld_cols" in mut else s[0]
            return dict(ro=elem(ro, [0], np.array([dev_of(z[0][mat_idx(n, n, ld)].reshape(n, n), ONE)], XR)))
        nn, nblk = d
        ld, bs = s[:2]
        on = [c for c in range(nblk) if (g["mask"] >> c) & 1]
        blks = {c: z[0][mat_idx(nn, nn, ld, c * bs)].reshape(nn, nn) for c in on}
        devs = [max(dev_of(blks[c], blks[c][0, 0]), 0.0 if v & 1 else float(ro[c])) for c in on]
        out = dict(zo1=elem(zo[1], on, np.array([blks[c][0, 0] for c in on], XC)))
        if v & 1:  # clear: the whole array is zeroed first, so a block that was not asked for comes back as +0.0
            val = np.zeros(nblk, XR)
            val[on] = devs
            out["ro"] = elem(ro, np.arange(nblk), val)
        else:
            out["ro"] = elem(ro, on, np.array(devs, XR))
        return out
    raise ValueError(op)


# ------------------------------------------------------------------------------------------------------------- case table
CASES = []


def case(group, op, dims, strides=(), variant=0, tag="", **kw):
    name = f"{op}-{'x'.join(str(q) for q in dims)}" + (f"-s{'x'.join(str(q) for q in strides)}" if strides else "") + f"-v{variant}" + (f"-{tag}" if tag else "")
    CASES.append(dict(name=name, group=group, op=op, dims=tuple(int(q) for q in dims), strides=tuple(int(q) for q in strides),
                      variant=variant, **kw))


NS = (1, 63, 64, 255, 256, 257, 65535, 65536, 65537, 131073)
for _n in NS:
    for _v in (0, 1):
        case("npart-reductions", "dot", (_n,), variant=_v)
        case("npart-updates", "lanczos_update", (_n,), variant=_v)
    case("npart-reductions", "sumsq", (_n,))
    for _k in ((1, 2, 20, 21) if _n <= 4099 else (3,)):
        for _ld in (_n, _n + 3):
            case("npart-reductions", "multi_dot", (_n, _k), (_ld,))
            case("npart-arnoldi", "arnoldi_update", (_n, _k), (_ld,))
            case("npart-lincomb", "lincomb", (_n, _k), (_ld,), variant=2)  # out null
            case("npart-lincomb", "lincomb", (_n, _k), (_ld,), variant=1)  # nrm null
    case("npart-lincomb", "lincomb", (_n, 3), (_n,), variant=3)
    for _l, _v in ((0, 0), (1, 1), (2, 3), (5, 1), (5, 3)):
        case("deferred", "lanczos_update_def", (_n, _l), variant=_v)
for _l in (0, 1, 2, 5):
    for _v in (0, 1, 2, 3):
        case("deferred", "lanczos_update_def", (257, _l), variant=_v, tag="all")
case("deferred", "lanczos_update_def", (257, 5), variant=3, tag="eps1e300", eps=1e300)
case("deferred", "lanczos_update_def", (65537, 2), variant=1, tag="eps1e300", eps=1e300)

SMALL_NS = (1, 64, 1023, 1024, 1025, 2048, 8191, 15360, 15361, 16383, 16384)
for _n in SMALL_NS:
    for _v in (0, 1, 2, 3):  # bit 0: vm2 given, bit 1: x is a vector of its own (otherwise vl itself)
        case("step-small", "lanczos_step_small", (_n,), variant=_v)
case("step-small", "lanczos_step_small", (15361,), variant=3, tag="eps1e300", eps=1e300)
case("step-small", "lanczos_step_small", (1025,), variant=0, tag="eps1e300", eps=1e300)

for _n in (1, 1023, 1024, 1025, 262145):
    case("scale-inv-norm", "scale_inv_norm", (_n,))
    case("vec-blocks", "axpby", (_n,))
    case("vec-blocks", "scale", (_n,))
case("scale-inv-norm", "scale_inv_norm", (1025,), tag="below-eps", norm2=1e-30)
case("scale-inv-norm", "scale_inv_norm", (1025,), tag="nan", nan_norm=True)
case("scale-inv-norm", "scale_inv_norm", (65537,), tag="nan", nan_norm=True)

for _rows, _cols in ((1, 1), (1023, 1), (1, 1024), (205, 5), (1, 262145), (37449, 7)):  # totals 1, 1023, 1024, 1025, 262145, 262143
    for _pad in (0, 3):
        case("vec-blocks", "identity", (_rows, _cols), (_cols + _pad,))
        case("vec-blocks", "scale_cols", (_rows, _cols), (_cols + _pad,))
for _rows in (1, 5, 300):
    for _cols in (1, 7, 64):
        for _zt in (0, _cols, _cols + 3):
            for _a in (1, 0.3 - 0.7j):
                for _acc in (0, 1):
                    case("copy2d", "copy2d", (_rows, _cols, _zt), (max(_cols, _zt) + 2, _cols + 1), variant=_acc, a=_a,
                         tag="a1" if _a == 1 else "az")
for _rows, _cols in ((1, 1), (1, 1023), (1024, 1), (205, 5), (262145, 1)):
    case("copy2d", "copy2d", (_rows, _cols, 0), (_cols, _cols), variant=0, a=0.3 - 0.7j, tag="tight")

_blk_rng = np.random.default_rng(7)
for _nbl in (0, 1, 5, 64):
    for _cols in (1, 7, 32):
        for _rows in (1, 33):
            _m = 9
            # unsorted, with repeats (tests/test_vecops_host.py asserts both from 5 blocks on)
            _blk = (7, 2, 7, 0, 5) if _nbl == 5 else tuple(int(q) for q in _blk_rng.integers(0, _m, _nbl))
            case("block-lists", "gather_blocks", (_rows, _cols, _nbl, _nbl + 2, _m), blk=_blk)
            case("block-lists", "fill_scaled_blocks", (_rows, _cols, _nbl, 3), ((_nbl + 3) * _cols + 5,))
            case("block-lists", "accum_scaled_blocks", (_rows, _cols, _nbl), (_m * _cols + 5,), blk=_blk)
# the vec_blocks totals 1, 1023, 1024, 1025 and 262145: rows * cols for accumulate, rows * bl.n * cols for gather and fill
for _rows, _cols, _nbl in ((1, 1, 1), (11, 31, 3), (8, 32, 4), (41, 5, 5), (52429, 1, 5)):
    _blk = {1: (4,), 3: (6, 1, 6), 4: (5, 0, 8, 5), 5: (3, 8, 3, 1, 6)}[_nbl]
    case("block-lists", "gather_blocks", (_rows, _cols, _nbl, _nbl, 9), blk=_blk, tag="total")
    case("block-lists", "fill_scaled_blocks", (_rows, _cols, _nbl, 0), (_nbl * _cols,), tag="total")
for _rows, _cols in ((1, 1), (11, 93), (32, 32), (41, 25), (52429, 5)):
    _blk = (3, 8, 3, 1, 6)
    case("block-lists", "accum_scaled_blocks", (_rows, _cols, 5), (9 * _cols,), blk=_blk, tag="total")

for _rows, _cols in ((1, 1), (1, 33), (33, 1), (31, 33), (32, 32), (33, 31), (64, 65), (65, 64), (100, 7)):
    for _pad in (0, 3):
        for _batch in (1, 3):
            _ldi, _ldo = _cols + _pad, _rows + 2 * _pad
            case("transpose", "transpose", (_rows, _cols, _batch), (_ldi, _ldo, _rows * _ldi + _pad, _cols * _ldo + _pad))
for _shape in ((1, 1, 1), (33, 3, 31), (5, 4, 65), (64, 2, 64), (2, 7, 1)):
    case("transpose", "transpose_rev3", _shape)
    _na, _nj, _ns = _shape  # the same through the batched wrapper: batches interleaved inside a row stride
    case("transpose", "transpose", (_na, _ns, _nj), (_nj * _ns, _nj * _na, _ns, _na), tag="interleaved")

for _shape in ((1, 1, 1, 1), (3, 5, 7, 2), (4, 33, 3, 1), (2, 3, 4, 65)):
    case("permutes", "permute_0213", _shape)


def c_strides(shape):
    st = [1] * len(shape)
    for k in range(len(shape) - 2, -1, -1):
        st[k] = st[k + 1] * shape[k + 1]
    return st


# the two gathers of Engine::kraus_core at k, K, m, x, n = 3, 2, 5, 2, 7: the site (m, k, x, n) read as (K', m, k, x, n)
# with the Kraus index on a zero stride and the rows of m through map2, and the (k, m, K, x, n) product read back as
# (m, K, k, x, n)
_k, _K, _m, _x, _n = 3, 2, 5, 2, 7
_st = c_strides((_m, _k, _x, _n))
case("permutes", "permute5", (_K, _k, _m, _x, _n), (0, _st[1], _st[0], _st[2], _st[3]), variant=1, map2=(3, 0, 4, 1, 2), tag="kraus-in")
_st = c_strides((_k, _m, _K, _x, _n))
case("permutes", "permute5", (_K, _k, _m, _x, _n), (_st[2], _st[0], _st[1], _st[3], _st[4]), variant=1, map2=(4, 2, 0, 3, 1), tag="kraus-out")
_shape, _order = (3, 4, 2, 5, 6), (3, 0, 4, 1, 2)
_st = c_strides(_shape)
case("permutes", "permute5", tuple(_shape[q] for q in _order), tuple(_st[q] for q in _order), tag="axes")
case("permutes", "permute5", (4, 1, 3, 6, 5), (15, 0, 5, 0, 1), tag="zero-stride")

for _shape in ((1, 1, 1), (3, 2, 5), (7, 4, 1), (1, 3, 260), (33, 3, 33)):
    for _v in (0, 1):
        case("phys-diag", "phys_diag", _shape, variant=_v)
case("phys-diag", "phys_diag", (0, 3, 5), variant=0, tag="zero-size")
case("phys-diag", "phys_diag", (0, 3, 5), variant=1, tag="zero-size")

_CAP = 4096 * 256  # the grids of these four stop at 4096 workgroups: one more element needs a second pass
case("capped", "permute_0213", (1, 1025, 1024, 1))
case("capped", "permute5", (1, 1, 1025, 1, 1024), (0, 0, 0, 0, 1), tag="zero-stride")
case("capped", "phys_diag", (1, 1, _CAP + 1))
case("capped", "copy_raw", (_CAP + 1,))
for _n in (1, 1023, 1025):
    case("capped", "copy_raw", (_n,))

for _rows in (1, 255, 256, 257, 600):
    for _cols in (1, 3, 40):
        case("profiles", "col_sumsq", (_rows, _cols))
        case("profiles", "row_sumsq", (_cols, _rows))
for _n in (1, 2, 255, 256, 257, 300):
    case("profiles", "shell_sumsq", (_n,))

for _n in (1, 2, 45, 46, 64, 129):
    for _ld, _off, _lt in ((_n, 0, "tight"), (_n + 7, 0, "padded"), (3 * _n, _n, "env")):  # env: block c = 1 of an (n, 3, n) block
        for _kind in ("exact", "off", "imag", "nan", "+inf", "-inf"):
            case("ident", "ident_dev", (_n,), (_ld,), tag=f"{_lt}-{_kind}", kind=_kind, off=_off)
for _nblk in (1, 3, 64):
    for _n in (1, 46, 129) if _nblk < 64 else (1, 46):
        _masks = {"all": (1 << _nblk) - 1, "one": 1 << (_nblk // 2), "bit63" if _nblk == 64 else "top": 1 << (_nblk - 1)}
        _masks = {_mt: _mask for _mt, _mask in _masks.items() if list(_masks.values()).index(_mask) == list(_masks).index(_mt)}
        for _mt, _mask in _masks.items():
            for _v in (1, 0):
                case("ident-multi", "ident_dev_multi", (_n, _nblk), (_nblk * _n, _n), variant=_v, tag=_mt, mask=_mask, bad=_nblk // 2)

CASES.sort(key=lambda r: (r["group"], max(int(np.prod(r["dims"], dtype=np.int64)), 0)))
BY_NAME = {r["name"]: r for r in CASES}
assert len(BY_NAME) == len(CASES)
GROUPS = sorted({r["group"] for r in CASES})
REFUSED = dict(op="lanczos_step_small", dims=(SMALL_VEC_N + 1,), strides=(), variant=0)


def footprint(row, g):
    """elements of every buffer as build() sizes them: what the host check must accept"""
    return dict(z=[0 if x is None else x.size for x in g["z"]], r=0 if g["r"] is None else g["r"].size,
                idx=0 if g["idx"] is None else len(g["idx"]), zo=[0 if x is None else x.size for x in g["zo"]],
                ro=0 if g["ro"] is None else g["ro"].size)
