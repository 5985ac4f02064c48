"""CPU: the test hook of the reducing product of the MFMA zgemm (``mitdvp_zgemm_reduce``), the NumPy model the GPU tests
hold it to (``helpers.zgemm_reduce_ref``) and the table of cases they share.

* the model equals a plain Python loop over the formula, NN and NT, writing and accumulating; its owned set equals a
  brute-force enumeration;
* ``zgemm_reduce_variant`` (csrc/zgemm_reduce_args_check.h, compiled with g++ into a throw-away shim) names, for every row
  of ``CASES`` and each of the three settings, the body the row expects; the rows reach all thirteen bodies in the default
  setting and bodies 8-13 with the 4 x 4 x 4 form off (counted here); over all xm, yn, di <= 64 it equals the dispatch
  table written down a second time in Python, and it names an unguarded body exactly where the condition of
  ``zgemm_reduce_full_ok`` holds;
* the footprint check runs before any HIP call, so its refusals are pinned without a GPU (accepted descriptors are sent to
  device -1: the call then ends with a HIP error, never EINVAL);
* the hook is declared, exported and mirrored with its argument count and struct layout.
"""

import ctypes as C
import inspect
import itertools
import os
import subprocess

import numpy as np
import pytest

from helpers import zgemm_reduce_ref as rr

HERE = os.path.dirname(os.path.abspath(__file__))
B4_FULL = {"default": (1, 1), "full_off": (1, 0), "b4_off": (0, 1)}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    from pytdscf_amd import _lib

    out = tmp_path_factory.mktemp("zr") / "libzr.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "helpers", "zgemm_reduce_shim.cpp"), "-o", str(out)],
                   check=True)
    lib = C.CDLL(str(out))
    lib.zr_check.restype = C.c_char_p
    lib.zr_check.argtypes = [C.POINTER(_lib.ZgemmReduceArgs)] + [C.c_size_t] * 4
    for fn in (lib.zr_shape_ok, lib.zr_full_shape):
        fn.argtypes = [C.c_int] * 3
    lib.zr_variant.argtypes = [C.c_int] * 5
    return lib


# ------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("transB,acc,c_layout", [(0, 0, "engine"), (1, 0, "inner"), (0, 1, "inner"), (1, 1, "engine")])
def test_model_equals_the_formula_looped(transB, acc, c_layout):
    rng = np.random.default_rng(10 * transB + acc)
    a = rr.layout(3, 2, 4, nu=2, nv=3, k=5, transB=transB, acc=acc, pad=(2, 1, 3), off=(3, 5, 2, 7), c_layout=c_layout)
    for kind in ("int", "gauss"):
        A, B, W, C0 = rr.make_case(a, rng, kind)
        out = rr.apply(a, A, B, W, C0)
        ref = rr.apply_loops(a, A, B, W, C0)
        own = rr.owned_c(a)
        assert not np.isnan(out[own]).any()  # no pad of A, B or W reached the result, the NaN in C was overwritten
        if kind == "int":
            assert np.array_equal(out, ref)
        else:
            rest = np.ones(out.size, bool)
            rest[own] = False
            assert np.array_equal(out[rest], ref[rest]) and np.abs(out[own] - ref[own]).max() < 1e-13 * np.abs(ref[own]).max()
            ext = rr.apply(a, A, B, W, C0, dtype=np.clongdouble)
            assert np.abs(ext[own] - ref[own]).max() < 1e-13 * np.abs(ref[own]).max()
        rest = np.ones(out.size, bool)
        rest[own] = False
        assert rest.sum() > 256 and np.all(out[rest] == rr.SENTINEL)
        if acc and kind == "int":  # what was there is added to, not replaced
            shifted = C0.copy()
            shifted[own] += 1.0
            assert np.array_equal(rr.apply(a, A, B, W, shifted)[own], out[own] + 1.0)


def test_owned_set_and_last_elements_equal_the_enumeration():
    for c_layout in ("engine", "inner"):
        a = rr.layout(3, 2, 4, nu=2, nv=3, k=5, transB=1, pad=(2, 1, 3), off=(3, 5, 2, 7), c_layout=c_layout)
        own, last = [], dict(A=0, B=0, W=0)
        for u in range(2):
            for v in range(3):
                for i in range(4):
                    own.append(a["offC"] + u * a["su"] + v * a["sv"] + i * a["si"])
                    for x in range(3):
                        for y in range(2):
                            last["W"] = max(last["W"], a["offW"] + i * a["ldw"] + x * 2 + y)
                            for k in range(5):
                                last["A"] = max(last["A"], a["offA"] + (u * 3 + x) * a["lda"] + k)
                                last["B"] = max(last["B"], a["offB"] + (v * 2 + y) * a["ldb"] + k)
        assert sorted(rr.owned_c(a).tolist()) == sorted(own) and len(set(own)) == len(own)
        assert rr.last_elements(a) == dict(last, C=max(own))
    assert rr.owned_c(rr.layout(3, 2, 4, nu=0, nv=3, k=5)).size == 0


def test_the_geometries_are_what_the_table_promises():
    ks = set()
    for idx, r in enumerate(rr.CASES):
        tu, tv = 64 // r["xm"], 64 // r["yn"]
        g = [rr.layout(**geo) for geo in rr.geometries(idx)]
        assert [(rr.groups(a)) for a in g] == [(1, 1), (tu, tv), (tu + 1, 2 * tv + 1)]
        assert all(a["m"] <= 200 and a["n"] <= 200 and a["k"] <= 33 for a in g)
        assert g[1]["lda"] > g[1]["k"] and g[1]["ldw"] > r["xm"] * r["yn"] and min(g[1][f] for f in ("offA", "offB", "offW", "offC")) > 0
        assert g[2]["ldb"] > (g[2]["k"] if r["transB"] else g[2]["n"])
        for a in g:  # the outputs of different (u, v, i) never share an element
            assert np.unique(rr.owned_c(a)).size == a["m"] // r["xm"] * (a["n"] // r["yn"]) * r["di"]
        ks.update(a["k"] for a in g)
    assert ks == {1, 5, 16, 33}
    assert {r["c_layout"] for r in rr.CASES} == {"engine", "inner"} and {r["transB"] for r in rr.CASES} == {0, 1}
    assert len({r["name"] for r in rr.CASES}) == len(rr.CASES)


# ---------------------------------------------------------------------------------------------------------- the dispatch
def table_body(xm, yn, di, b4, full):
    """The dispatch written down from the table of bodies, not from the kernel's branch: 0 = not served"""
    npair = (64 // xm) * (64 // yn)
    rb, cb = -(-di // 16), -(-npair // 16)
    if not ((cb == 1) or (cb == 2 and rb <= 2) or (cb <= 4 and rb == 1)):
        return 0
    pow2 = lambda v: v & (v - 1) == 0  # noqa: E731
    whole = full and pow2(xm) and pow2(yn) and yn % 4 == 0 and (xm * yn) % 128 == 0
    if b4:
        if di <= 4:
            return 7
        if npair <= 8 and di <= 32:
            if npair == 8 and whole and di in (16, 32):
                return 1 if di == 16 else 2
            return (3 if npair <= 4 else 4) if di <= 16 else (5 if npair <= 4 else 6)
    if npair <= 16:
        return 8 if di <= 16 else 9 if di <= 32 else 10
    if npair <= 32:
        return 11 if di <= 16 else 12
    return 13


def test_every_row_names_its_body_and_the_rows_reach_all_thirteen(shim):
    reached = {s: {} for s in B4_FULL}
    for r in rr.CASES:
        for s, (b4, full) in B4_FULL.items():
            got = shim.zr_variant(r["xm"], r["yn"], r["di"], b4, full)
            assert got == r["expect"][s], (r["name"], s, got)
            reached[s][got] = reached[s].get(got, 0) + 1
        assert shim.zr_shape_ok(r["xm"], r["yn"], r["di"])
    for s in reached:
        print(f"[zgemm_reduce] rows per body, {s}: " + ", ".join(f"{b}: {n}" for b, n in sorted(reached[s].items())))
    assert sorted(reached["default"]) == list(range(1, 14))
    assert sorted(reached["b4_off"]) == list(range(8, 14))
    assert not {1, 2} & set(reached["full_off"]) and sorted(reached["full_off"]) == list(range(3, 14))
    by_name = {r["name"]: r["expect"] for r in rr.CASES}
    for d, M, body, guarded, plain in ((16, 32, 1, 4, 8), (32, 16, 2, 6, 9)):
        for side in "RL":
            assert by_name[f"d{d}M{M}-{side}"] == {"default": body, "full_off": guarded, "b4_off": plain}
    # the shapes the engine can produce: (d, M, d) for its NT side and (M, d, d) for its NN side, all thirteen among them
    eng = [r for r in rr.CASES if r["name"][0] == "d" and r["name"][1].isdigit()]
    assert len(eng) == 28 and all((r["xm"] if r["transB"] else r["yn"]) == r["di"] for r in eng)
    assert sorted({r["expect"]["default"] for r in eng}) == list(range(1, 14))
    # di at both sides of every border of the dispatch, and three output rows with 64 pairs
    assert {4, 5, 16, 17, 32, 33} <= {r["di"] for r in rr.CASES}
    assert any(r["di"] == 3 and (64 // r["xm"]) * (64 // r["yn"]) == 64 for r in rr.CASES)


def test_variant_equals_the_table_and_the_full_condition_over_every_shape(shim):
    n_served = 0
    for xm, yn, di in itertools.product(range(1, 65), repeat=3):
        ok = bool(shim.zr_shape_ok(xm, yn, di))
        n_served += ok
        for b4, full in ((1, 1), (1, 0), (0, 1), (0, 0)):
            v = shim.zr_variant(xm, yn, di, b4, full)
            assert v == table_body(xm, yn, di, b4, full), (xm, yn, di, b4, full, v)
            assert (v == 0) == (not ok)
            if b4 and full and ok:  # an unguarded body exactly where zgemm_reduce_full_ok's condition holds
                assert (v in (1, 2)) == bool(shim.zr_full_shape(xm, yn, di)), (xm, yn, di, v)
            if not (b4 and full):
                assert v not in (1, 2)
            if not b4:
                assert v == 0 or v >= 8
    assert n_served > 0
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (65, 4, 4), (4, 65, 4), (4, 4, 65), (-1, 4, 4), (8, 8, 17), (12, 10, 33)):
        assert shim.zr_variant(*bad, 1, 1) == 0 and not shim.zr_shape_ok(*bad)


# ------------------------------------------------------------------------------------------------------ hook and mirror
def test_the_hook_is_declared_exported_and_mirrored(shim):
    from pytdscf_amd import _lib
    from pytdscf_amd import engine as E

    name = "mitdvp_zgemm_reduce"
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert name in _lib.declared_symbols() and "typedef struct mitdvp_zgemm_reduce_args" in header
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    lib = _lib.load()
    assert len(lib.mitdvp_zgemm_reduce.argtypes) == 11
    assert len(lib.mitdvp_zgemm_desc.argtypes) == 10  # the plain hook keeps its signature
    assert [f for f, _ in _lib.ZgemmReduceArgs._fields_] == [
        "m", "n", "k", "transB", "lda", "ldb", "offA", "offB", "xm", "yn", "di", "acc", "ldw", "offW", "su", "sv", "si", "offC",
        "mode3m", "epi_b4", "epi_full"]
    assert C.sizeof(_lib.ZgemmReduceArgs) == shim.zr_sizeof_args()
    assert _lib.ZgemmReduceArgs.mode3m.offset == shim.zr_offsetof_mode3m()
    assert set(E.ZGEMM_REDUCE_DEFAULTS) == set(rr.DEFAULTS) == {f for f, _ in _lib.ZgemmReduceArgs._fields_}
    assert E.ZGEMM_REDUCE_DEFAULTS == rr.DEFAULTS
    assert list(inspect.signature(E.zgemm_reduce).parameters) == ["args", "A", "B", "W", "Cbuf", "device"]
    assert lib.mitdvp_zgemm_reduce(0, None, None, 0, None, 0, None, 0, None, 0, None) == _lib.EINVAL


def struct_of(a):
    from pytdscf_amd import _lib

    s = _lib.ZgemmReduceArgs()
    for name, val in rr.full(a).items():
        setattr(s, name, int(val))
    return s


def call(a, nA, nB, nW, nC):
    """the hook on buffers of exactly nA / nB / nW / nC elements, on device -1: EINVAL = refused by the host check, anything
    else = the check passed (the call then fails at hipSetDevice, before anything is allocated or launched)"""
    from pytdscf_amd import _lib
    from pytdscf_amd import engine as E

    bufs = [np.zeros(max(n, 1), np.complex128) for n in (nA, nB, nW, nC)]
    v = C.c_int(-7)
    rc = _lib.load().mitdvp_zgemm_reduce(-1, C.byref(struct_of(a)), E._dp(bufs[0]), nA, E._dp(bufs[1]), nB, E._dp(bufs[2]), nW,
                                          E._dp(bufs[3]), nC, C.byref(v))
    return rc, _lib.load().mitdvp_last_error(None).decode(), v.value


VIEW_CASES = [
    rr.layout(16, 8, 4, nu=2, nv=3, k=5, pad=(2, 1, 3), off=(3, 5, 2, 7)),
    rr.layout(12, 10, 12, nu=2, nv=3, k=5, transB=1, pad=(2, 1, 3), off=(3, 5, 2, 7), c_layout="inner"),
    rr.layout(16, 32, 16, nu=5, nv=5, k=33, transB=1, acc=1),
    rr.layout(8, 8, 3, nu=1, nv=1, k=1),
]


@pytest.mark.parametrize("idx", range(len(VIEW_CASES)))
def test_a_view_one_element_too_long_is_refused(idx, shim):
    """buffers that end exactly at the last element of each view pass the check; one element shorter, in A, B, W or C, does
    not -- through the library and through the shim alike"""
    from pytdscf_amd import _lib

    a = VIEW_CASES[idx]
    last = rr.last_elements(a)
    sizes = [last[w] + 1 for w in "ABWC"]
    rc, msg, _ = call(a, *sizes)
    assert rc not in (_lib.OK, _lib.EINVAL), (rc, msg)
    assert shim.zr_check(C.byref(struct_of(a)), *sizes) is None
    for q, word in enumerate("ABWC"):
        short = list(sizes)
        short[q] -= 1
        rc, msg, v = call(a, *short)
        assert rc == _lib.EINVAL and f"view of {word} leaves" in msg and v == -7, (word, rc, msg)
        assert f"view of {word} leaves".encode() in shim.zr_check(C.byref(struct_of(a)), *short)


def test_what_the_kernel_does_not_serve_is_refused():
    from pytdscf_amd import _lib

    big = 1 << 20
    ok = rr.layout(16, 16, 16, nu=2, nv=3, k=7, off=(1, 1, 1, 1))
    assert call(ok, big, big, big, big)[0] not in (_lib.OK, _lib.EINVAL)
    for s in rr.SETTINGS.values():  # switching a form off is accepted
        assert call(dict(ok, **s), big, big, big, big)[0] not in (_lib.OK, _lib.EINVAL)
    refused = {
        "epi_b4 = 1": dict(ok, epi_b4=1),
        "epi_full = 1": dict(ok, epi_full=1),
        "epi_b4 = -2": dict(ok, epi_b4=-2),
        "m no multiple of xm": dict(ok, m=33),
        "n no multiple of yn": dict(ok, n=47),
        "shape not served (64 pairs, 17 rows)": dict(ok, xm=8, yn=8, di=17),
        "shape not served (30 pairs, 33 rows)": dict(ok, xm=12, yn=10, di=33, m=24, n=30),
        "xm = 0": dict(ok, xm=0),
        "yn = 65": dict(ok, yn=65, n=65),
        "di = 0": dict(ok, di=0),
        "negative lda": dict(ok, lda=-7),
        "negative ldb": dict(ok, ldb=-48),
        "negative ldw": dict(ok, ldw=-256),
        "negative su": dict(ok, su=-1),
        "negative sv": dict(ok, sv=-1),
        "negative si": dict(ok, si=-1),
        "negative offA": dict(ok, offA=-1),
        "negative offB": dict(ok, offB=-1),
        "negative offW": dict(ok, offW=-1),
        "negative offC": dict(ok, offC=-1),
        "negative m": dict(ok, m=-16),
        "k = 0": dict(ok, k=0),
        "transB = 2": dict(ok, transB=2),
        "acc = 2": dict(ok, acc=2),
        "mode3m = 2": dict(ok, mode3m=2),
    }
    for what, a in refused.items():
        rc, msg, _ = call(a, big, big, big, big)
        assert rc == _lib.EINVAL and msg.startswith("zgemm_reduce:"), (what, rc, msg)
    # m or n of 0 touch nothing: success without a device, whatever the buffers, and C is left alone
    for a in (dict(ok, m=0), dict(ok, n=0)):
        rc, msg, _ = call(a, 0, 0, 0, 0)
        assert rc == _lib.OK, (rc, msg)


def test_the_python_wrapper_raises_before_the_device_is_touched():
    from pytdscf_amd import engine as E

    a = rr.layout(16, 8, 4, nu=2, nv=3, k=5, pad=(2, 1, 3), off=(3, 5, 2, 7))
    A, B, W, C0 = rr.make_case(a, np.random.default_rng(0), "int")
    with pytest.raises(ValueError, match="view of C leaves"):
        E.zgemm_reduce(a, A, B, W, C0[: rr.last_elements(a)["C"]], device=-1)
    with pytest.raises(ValueError, match="cannot be forced on"):
        E.zgemm_reduce(dict(a, epi_full=1), A, B, W, C0, device=-1)
    with pytest.raises(TypeError):
        E.zgemm_reduce(dict(a, ldc=3), A, B, W, C0, device=-1)
    out, variant = E.zgemm_reduce(dict(a, m=0), A, B, W, C0, device=-1)  # nothing to do: C as it came, no device needed
    assert np.array_equal(out, C0, equal_nan=True) and variant == 0
