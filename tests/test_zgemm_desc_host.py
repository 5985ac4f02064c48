"""CPU: the descriptor hook of the MFMA zgemm (``mitdvp_zgemm_desc``) and the NumPy model the GPU tests hold it to.

* the model (``helpers.zgemm_ref``) equals the plain product in all eight trans / conj forms, a per-batch Python loop,
  and its footprint equals a brute-force enumeration of every index of the logical operation;
* the hook is declared, exported and mirrored with its argument count;
* the footprint check of the C side runs before any HIP call, so its refusals are pinned here without a GPU: a view one
  element too long in A, B, C or the list, and every combination the kernel does not serve.  (The accepted descriptors
  are sent to device -1: the footprint check passes and the call ends with a HIP error, never EINVAL, on any machine.)
"""

import ctypes as C
import itertools
import os

import numpy as np
import pytest

from helpers import zgemm_ref as zr


def opmat(X, trans, conj):
    X = X.T if trans else X
    return X.conj() if conj else X


@pytest.mark.parametrize("tA,cA,tB,cB", list(itertools.product((0, 1), repeat=4)))
def test_model_equals_the_plain_product_on_packed_operands(tA, cA, tB, cB):
    rng = np.random.default_rng(tA * 8 + cA * 4 + tB * 2 + cB)
    m, n, k = 13, 7, 9
    A = zr.draw(rng, (k, m) if tA else (m, k), "gauss")
    B = zr.draw(rng, (n, k) if tB else (k, n), "gauss")
    C0 = zr.draw(rng, (m, n), "gauss")
    alpha, beta = 0.7 - 0.2j, -0.3 + 1.1j
    a = zr.layout(m, n, k, transA=tA, conjA=cA, transB=tB, conjB=cB, off=(0, 0, 0), alpha=alpha, beta=beta)
    assert (a["lda"], a["ldb"], a["ldc"]) == (m if tA else k, k if tB else n, n)
    out = zr.apply(a, A, B, C0).reshape(m, n)
    assert np.array_equal(out, alpha * (opmat(A, tA, cA) @ opmat(B, tB, cB)) + beta * C0)
    a0 = dict(a, beta=0.0)
    assert np.array_equal(zr.apply(a0, A, B, np.full((m, n), np.nan)).reshape(m, n), alpha * (opmat(A, tA, cA) @ opmat(B, tB, cB)))


@pytest.mark.parametrize("shared", [(False, False), (True, False), (False, True), (True, True)])
def test_model_equals_a_per_batch_loop_and_keeps_what_it_does_not_own(shared):
    rng = np.random.default_rng(5)
    m, n, k, nb = 6, 5, 7, 3
    a = zr.layout(m, n, k, batch=nb, transB=1, conjB=1, pad=(2, 3, 4), bpad=(5, 6, 7), shared=shared, alpha=2 - 1j, beta=-1 + 3j)
    A, B, C0 = zr.make_case(a, rng, "int")
    out = zr.apply(a, A, B, C0)
    exp = C0.copy()
    for b in range(nb):
        Ab = np.array([[A[a["offA"] + b * a["strideA"] + i * a["lda"] + kk] for kk in range(k)] for i in range(m)])
        Bb = np.array([[np.conj(B[a["offB"] + b * a["strideB"] + j * a["ldb"] + kk]) for j in range(n)] for kk in range(k)])
        P = Ab @ Bb
        for i in range(m):
            for j in range(n):
                q = a["offC"] + b * a["strideC"] + i * a["ldc"] + j
                exp[q] = (2 - 1j) * P[i, j] + (-1 + 3j) * C0[q]
    assert np.array_equal(out, exp)
    assert not np.isnan(out).any()  # no pad of A or B reached the product
    rest = np.ones(out.size, bool)
    rest[zr.owned_c(a)] = False
    assert rest.sum() > 128 * a["ldc"] and np.all(out[rest] == zr.SENTINEL)


def test_model_row_map_row_skip_and_list():
    rng = np.random.default_rng(6)
    # trimmed H_eff stage: groups of ml - 1 rows, stored row 0 of every group of ml left out, C rows of state 0 untouched
    ml, na, n, k = 3, 4, 5, 6
    a = zr.full(dict(m=na * (ml - 1), n=n, k=k, lda=k, ldb=n, arow_skip=ml, rowmap_p=ml - 1, rowmap_s1=n, rowmap_s2=ml * n, offC=n))
    Afull, B = zr.draw(rng, (na * ml, k), "int"), zr.draw(rng, (k, n), "int")
    X0 = np.full((na, ml, n), zr.SENTINEL)
    out = zr.apply(a, Afull, B, X0).reshape(na, ml, n)
    ref = (Afull @ B).reshape(na, ml, n)
    assert np.array_equal(out[:, 1:], ref[:, 1:]) and np.all(out[:, 0] == zr.SENTINEL)
    # list: the unlisted tiles count as zero whatever they hold
    m, k = 70, 48
    kl, stride = zr.klist_rows(m, k, [[0, 2], []])
    a = zr.layout(m, 4, k, klist_stride=stride, tile_cfg=1, beta=1.0)
    A, B, C0 = zr.make_case(a, rng, "int", klist=kl)
    Ad = np.nan_to_num(A[zr.index_a(a, 0)], nan=0.0)
    assert np.isnan(A[zr.index_a(a, 0)][:64, 16:32]).all() and np.isnan(A[zr.index_a(a, 0)][64:]).all()
    out = zr.apply(a, A, B, C0, kl)
    ic = zr.index_c(a, 0)
    assert np.array_equal(out[ic], Ad @ B[zr.index_b(a, 0)] + C0[ic])
    assert np.array_equal(out[ic][64:], C0[ic][64:])  # empty list: beta * C


FOOTPRINT_CASES = [
    zr.layout(5, 4, 3),
    zr.layout(5, 4, 3, batch=3, pad=(1, 2, 3), bpad=(4, 5, 6)),
    zr.layout(5, 4, 3, batch=2, transA=1, transB=1, pad=(2, 0, 1), shared=(True, False)),
    zr.layout(6, 4, 3, arow_skip=3, pad=(1, 0, 0)),
    zr.layout(6, 4, 3, batch=2, shared=(True, False), rowmap_p=2, rowmap_s1=3 * 4, rowmap_s2=4, rowmap_r0=2, strideC=40),
    zr.layout(8, 4, 3, arow_skip=3, rowmap_p=2, rowmap_s1=5, rowmap_s2=15, off=(0, 0, 5)),
    zr.layout(70, 3, 16, klist_stride=4, tile_cfg=1),
    zr.layout(4, 3, 0),
    zr.layout(0, 3, 5),
]


@pytest.mark.parametrize("idx", range(len(FOOTPRINT_CASES)))
def test_footprint_equals_the_enumeration(idx):
    a = FOOTPRINT_CASES[idx]
    assert zr.footprint(a) == zr.footprint_enumerated(a)


def test_the_hook_is_declared_exported_and_mirrored():
    import inspect

    from pytdscf_amd import _lib
    from pytdscf_amd import engine as E

    name = "mitdvp_zgemm_desc"
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert name in _lib.declared_symbols() and "typedef struct mitdvp_zgemm_args" in header
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    lib = _lib.load()
    assert len(lib.mitdvp_zgemm_desc.argtypes) == 10
    assert len(lib.mitdvp_zgemm.argtypes) == 16  # the packed hook keeps its signature
    assert [f for f, _ in _lib.ZgemmArgs._fields_] == [
        "m", "n", "k", "batch", "transA", "conjA", "transB", "conjB", "lda", "ldb", "ldc", "strideA", "strideB", "strideC",
        "offA", "offB", "offC", "alpha", "beta", "tile_cfg", "mode3m", "arow_skip", "rowmap_p", "rowmap_s1", "rowmap_s2",
        "rowmap_r0", "klist_stride"]
    assert set(E.ZGEMM_DESC_DEFAULTS) == set(zr.DEFAULTS) == {f for f, _ in _lib.ZgemmArgs._fields_}
    assert list(inspect.signature(E.zgemm_desc).parameters) == ["args", "A", "B", "Cbuf", "klist", "device"]
    assert lib.mitdvp_zgemm_desc(0, None, None, 0, None, 0, None, 0, None, 0) == _lib.EINVAL


def call(a, nA, nB, nC, klist=None, nklist=None):
    """the hook on buffers of exactly nA / nB / nC elements, on device -1: EINVAL = refused by the host check, anything
    else = the check passed (the call then fails at hipSetDevice, before anything is allocated or launched)"""
    from pytdscf_amd import _lib
    from pytdscf_amd import engine as E

    A, B, Cb = np.zeros(max(nA, 1), np.complex128), np.zeros(max(nB, 1), np.complex128), np.zeros(max(nC, 1), np.complex128)
    s = _lib.ZgemmArgs()
    for name, val in zr.full(a).items():
        if name in ("alpha", "beta"):
            setattr(s, name, (C.c_double * 2)(complex(val).real, complex(val).imag))
        else:
            setattr(s, name, int(val))
    kl = None if klist is None else np.ascontiguousarray(klist, dtype=np.intc)
    rc = _lib.load().mitdvp_zgemm_desc(-1, C.byref(s), E._dp(A), nA, E._dp(B), nB, E._dp(Cb), nC,
                                        None if kl is None else kl.ctypes.data_as(C.POINTER(C.c_int)),
                                        0 if kl is None else (kl.size if nklist is None else nklist))
    return rc, _lib.load().mitdvp_last_error(None).decode()


VIEW_CASES = [
    zr.layout(5, 4, 3, batch=3, pad=(1, 2, 3), bpad=(4, 5, 6)),
    zr.layout(5, 4, 3, batch=2, transA=1, transB=1, pad=(2, 0, 1), shared=(True, False)),
    zr.layout(6, 4, 3, arow_skip=3, pad=(1, 0, 0)),
    zr.layout(6, 4, 3, batch=2, shared=(True, False), rowmap_p=2, rowmap_s1=3 * 4, rowmap_s2=4, rowmap_r0=2, strideC=40),
    zr.layout(8, 4, 3, arow_skip=3, rowmap_p=2, rowmap_s1=5, rowmap_s2=15, off=(0, 0, 5)),
]


@pytest.mark.parametrize("idx", range(len(VIEW_CASES)))
def test_a_view_one_element_too_long_is_refused(idx):
    """buffers that end exactly at the model's footprint pass the check; one element shorter, in A, in B or in C, does not"""
    from pytdscf_amd import _lib

    a = VIEW_CASES[idx]
    fp = zr.footprint(a)
    nA, nB, nC = fp["A"][1] + 1, fp["B"][1] + 1, fp["C"][1] + 1
    rc, msg = call(a, nA, nB, nC)
    assert rc not in (_lib.OK, _lib.EINVAL), (rc, msg)
    for short, word in (((nA - 1, nB, nC), "A"), ((nA, nB - 1, nC), "B"), ((nA, nB, nC - 1), "C")):
        rc, msg = call(a, *short)
        assert rc == _lib.EINVAL and f"view of {word} leaves" in msg, (short, rc, msg)


def test_a_list_one_element_too_long_is_refused():
    from pytdscf_amd import _lib

    m, k = 150, 64
    kl, stride = zr.klist_rows(m, k, [[0, 1, 2, 3], [3], []], stride=7)
    a = zr.layout(m, 9, k, klist_stride=stride, tile_cfg=1)
    fp = zr.footprint(a)
    assert fp["klist"] == (0, 3 * 7 - 1) and kl.size == 21
    sizes = (fp["A"][1] + 1, fp["B"][1] + 1, fp["C"][1] + 1)
    rc, msg = call(a, *sizes, klist=kl)
    assert rc not in (_lib.OK, _lib.EINVAL), (rc, msg)
    rc, msg = call(a, *sizes, klist=kl, nklist=20)
    assert rc == _lib.EINVAL and "list leaves" in msg, (rc, msg)
    # what the list says is checked too: a count or an index beyond K / 16, a descending pair, a stride below 1 + K / 16
    for bad in ([[0, 1, 2, 4], [3], []], [[2, 1], [], []]):
        klb, _ = zr.klist_rows(m, k, [[]] * 3, stride=7)
        for tm, t in enumerate(bad):
            klb[tm * 7] = len(t)
            klb[tm * 7 + 1:tm * 7 + 1 + len(t)] = t
        rc, msg = call(a, *sizes, klist=klb)
        assert rc == _lib.EINVAL and "K-tile" in msg, (bad, rc, msg)
    klb = kl.copy()
    klb[7] = 5
    assert call(a, *sizes, klist=klb)[0] == _lib.EINVAL
    assert call(dict(a, klist_stride=4), *sizes, klist=kl)[0] == _lib.EINVAL


def test_what_the_kernel_does_not_serve_is_refused():
    from pytdscf_amd import _lib

    big = 1 << 20
    ok = zr.layout(4, 3, 16, off=(0, 0, 0))
    assert call(ok, big, big, big)[0] not in (_lib.OK, _lib.EINVAL)
    kl, stride = zr.klist_rows(4, 16, [[0]])
    refused = {
        "batch = 65536": (dict(ok, batch=65536, strideA=0, strideB=0, strideC=0), None),
        "arow_skip = 1": (dict(ok, arow_skip=1), None),
        "arow_skip with transA": (dict(ok, arow_skip=2, transA=1), None),
        "arow_skip with a list": (dict(ok, arow_skip=2, tile_cfg=1, klist_stride=stride), kl),
        "list with transB": (dict(ok, transB=1, tile_cfg=1, klist_stride=stride), kl),
        "list with transA": (dict(ok, transA=1, tile_cfg=1, klist_stride=stride), kl),
        "list with K % 16 != 0": (dict(ok, k=24, tile_cfg=1, klist_stride=stride + 1), kl),
        "tile_cfg = 3": (dict(ok, tile_cfg=3), None),
        "tile_cfg = -2": (dict(ok, tile_cfg=-2), None),
        "mode3m = 2": (dict(ok, mode3m=2), None),
        "negative m": (dict(ok, m=-1), None),
        "negative lda": (dict(ok, lda=-16), None),
        "negative offset": (dict(ok, offC=-1), None),
    }
    for what, (a, lst) in refused.items():
        rc, msg = call(a, big, big, big, klist=lst)
        assert rc == _lib.EINVAL and msg.startswith("zgemm_desc:"), (what, rc, msg)
    # batch = 65535 of 1 x 1 x 1 passes the check; so does the list form itself
    assert call(zr.layout(1, 1, 1, batch=65535, off=(0, 0, 0)), big, big, big)[0] not in (_lib.OK, _lib.EINVAL)
    assert call(dict(ok, tile_cfg=1, klist_stride=stride), big, big, big, klist=kl)[0] not in (_lib.OK, _lib.EINVAL)
    # m, n or batch of 0 touch nothing: success without a device, whatever the buffers
    for a in (dict(ok, m=0), dict(ok, n=0), dict(ok, batch=0)):
        rc, msg = call(a, 0, 0, 0)
        assert rc not in (_lib.EINVAL,), (rc, msg)


def test_the_python_wrapper_raises_before_the_device_is_touched():
    from pytdscf_amd import engine as E

    a = zr.layout(5, 4, 3, pad=(1, 2, 3))
    A, B, C0 = zr.make_case(a, np.random.default_rng(0), "int")
    with pytest.raises(ValueError, match="view of C leaves"):
        E.zgemm_desc(a, A, B, C0[: zr.footprint(a)["C"][1]], device=-1)
    with pytest.raises(TypeError):
        E.zgemm_desc(dict(a, ldd=3), A, B, C0, device=-1)
