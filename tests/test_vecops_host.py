"""CPU: the test hook of the Krylov vector and layout kernels (``mitdvp_vecop`` / ``engine.vecop``), the NumPy models the GPU
tests hold them to (``helpers.vecops_ref``) and the table of cases they share.

* ``csrc/vecop_check.h`` (compiled with g++ into a throw-away shim) accepts every row of ``CASES`` with the footprint the
  table builds its buffers to, refuses every buffer one element short, and refuses each violation by name;
* through the real library the refusals come back as EINVAL without a GPU, an accepted call sent to device -1 ends in a HIP
  error, and a zero-size call returns OK with the results untouched;
* the hook is declared, exported and mirrored with its argument count, struct layout and op numbers;
* each model equals a plain Python loop at a tiny shape;
* the table has power: for each mutated model of ``MUTATIONS`` at least one row misses its bar, or its bit equality, when
  the mutant's output is judged against the true model -- and the true model's own output passes every row;
* the inputs are what the bars assume: every term of a reduction row is at least 0.25 in modulus and the largest bar of a
  reduction lies below that.
"""

import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import vecops_ref as vr

HERE = os.path.dirname(os.path.abspath(__file__))
FOOT = ("zin0", "zin1", "zin2", "rin", "idx", "zio0", "zio1", "rio", "zwr0", "zwr1", "rwr", "empty", "own_return")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    from pytdscf_amd import _lib

    out = tmp_path_factory.mktemp("vo") / "libvo.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(HERE, "helpers", "vecop_shim.cpp"),
                    "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    ip, sp = C.POINTER(C.c_int), C.POINTER(C.c_size_t)
    lib.vo_shape.restype = C.c_char_p
    lib.vo_shape.argtypes = [C.POINTER(_lib.VecopArgs), ip, C.c_size_t, sp]
    lib.vo_check.restype = C.c_char_p
    lib.vo_check.argtypes = [C.POINTER(_lib.VecopArgs), sp, ip, C.c_size_t, C.c_int]
    lib.vo_limits.argtypes = [C.POINTER(C.c_long)]
    return lib


def struct_of(op, dims, strides=(), variant=0):
    from pytdscf_amd import _lib
    from pytdscf_amd import engine as E

    a = _lib.VecopArgs()
    a.op, a.variant = (E.VECOP_OPS[op] if isinstance(op, str) else op), variant
    for k, v in enumerate(dims):
        a.dims[k] = v
    for k, v in enumerate(strides):
        a.strides[k] = v
    return a


def idx_of(idx):
    arr = np.ascontiguousarray(idx if idx is not None else [], dtype=np.intc)
    return arr, arr.ctypes.data_as(C.POINTER(C.c_int)) if arr.size else None, arr.size


def shape(shim, op, dims, strides=(), variant=0, idx=None):
    a = struct_of(op, dims, strides, variant)
    keep, p, n = idx_of(idx)
    out = (C.c_size_t * 13)()
    msg = shim.vo_shape(C.byref(a), p, n, out)
    return msg, dict(zip(FOOT, out))


def check(shim, op, dims, strides, variant, sizes, idx=None, alias=-1):
    """sizes: zin0 zin1 zin2 rin zio0 zio1 rio"""
    a = struct_of(op, dims, strides, variant)
    keep, p, n = idx_of(idx)
    return shim.vo_check(C.byref(a), (C.c_size_t * 7)(*sizes), p, n, alias)


# --------------------------------------------------------------------------------------------------- the table and the check
def test_every_row_is_accepted_at_its_footprint_and_meets_its_own_model(shim):
    worst_bar, least_term, nsum = 0.0, np.inf, 0
    for r in vr.CASES:
        g = vr.build(r)
        built = vr.footprint(r, g)
        msg, f = shape(shim, r["op"], r["dims"], r["strides"], r["variant"], g["idx"])
        assert msg is None, (r["name"], msg)
        need = [f["zin0"], f["zin1"], f["zin2"], f["rin"], f["zio0"], f["zio1"], f["rio"]]
        have = built["z"] + [built["r"]] + built["zo"] + [built["ro"]]
        for k, (nd, hv) in enumerate(zip(need, have)):
            if nd:  # inputs are built to the footprint, results to GUARD elements more
                assert hv == nd + (vr.GUARD if k >= 4 else 0) or (k == 3 and hv >= nd), (r["name"], k, nd, hv)
        assert f["zwr0"] <= f["zio0"] and f["zwr1"] <= f["zio1"] and f["rwr"] <= f["rio"]
        assert check(shim, r["op"], r["dims"], r["strides"], r["variant"], have, g["idx"]) is None, r["name"]
        for k, nd in enumerate(need):
            if nd:
                short = list(have)
                short[k] = nd - 1
                msg = check(shim, r["op"], r["dims"], r["strides"], r["variant"], short, g["idx"])
                assert msg is not None and b"shorter than the operation's footprint" in msg, (r["name"], k, msg)
        specs = vr.expect(r, g)
        assert specs or f["empty"], r["name"]
        for key, spec in specs.items():
            ok, defect, bar, what = vr.judge(spec, vr.render(spec))
            assert ok, (r["name"], key, defect, bar, what)
            # the model writes exactly up to where the header says the op writes
            if spec["kind"] == "elem":
                last = int(np.flatnonzero(spec["written"]).max()) + 1 if spec["written"].any() else 0
            else:
                last = spec["k"] * vr.NPART
            assert last <= f[{"zo0": "zwr0", "zo1": "zwr1", "ro": "rwr"}[key]], (r["name"], key, last)
            if "minterm" in spec:
                nsum += 1
                least_term = min(least_term, spec["minterm"])
                worst_bar = max(worst_bar, float(np.max(spec["bar"])))
    print(f"[vecops] {len(vr.CASES)} rows, {nsum} reductions: least term {least_term:.3f}, largest bar {worst_bar:.2e}")
    assert nsum > 400 and least_term >= 0.25 and worst_bar < 0.25


def test_block_lists_are_unsorted_with_repeats():
    """from 5 blocks on (a list of 0 or 1 has neither property to show)"""
    lists = [r["blk"] for r in vr.CASES if "blk" in r and len(r["blk"]) >= 3]
    assert len(lists) >= 20 and {len(b) for b in lists} >= {5, 64}
    for b in lists:
        assert len(set(b)) < len(b) and list(b) != sorted(b) and list(b) != sorted(b, reverse=True), b
    masks = [(r["dims"], r["variant"], r["mask"]) for r in vr.CASES if r["op"] == "ident_dev_multi"]
    assert len(set(masks)) == len(masks) and any(m == 1 << 63 for _, _, m in masks)  # no row twice; bit 63 is there


def test_the_refused_row_is_refused(shim):
    r = vr.REFUSED
    msg, _ = shape(shim, r["op"], r["dims"], r["strides"], r["variant"])
    assert msg is not None and b"SMALL_VEC_N" in msg
    assert shape(shim, r["op"], (vr.SMALL_VEC_N,), (), 0)[0] is None


VIOLATIONS = {
    "unknown op": dict(op=28, dims=(4,)),
    "unknown op ": dict(op=-1, dims=(4,)),
    "unknown variant": dict(op="dot", dims=(4,), variant=2),
    "unknown variant ": dict(op="sumsq", dims=(4,), variant=1),
    "a negative dimension": dict(op="axpby", dims=(-1,)),
    "a negative stride": dict(op="transpose", dims=(2, 2, 1), strides=(2, -2, 0, 0)),
    "a dimension above 2^28": dict(op="copy_raw", dims=((1 << 28) + 1,)),
    "k > MAXK": dict(op="multi_dot", dims=(4, 22), strides=(4,)),
    "k > MAXK ": dict(op="arnoldi_update", dims=(4, 22), strides=(4,)),
    "k > MAXK  ": dict(op="lincomb", dims=(4, 22), strides=(4,), variant=3),
    "l >= MAXK": dict(op="lanczos_update_def", dims=(4, 21)),
    "n > SMALL_VEC_N": dict(op="lanczos_step_small", dims=(16385,)),
    "batch > 65535": dict(op="transpose", dims=(1, 1, 65536), strides=(1, 1, 1, 1)),
    "batch > 65535 ": dict(op="transpose_rev3", dims=(1, 65536, 1)),
    "more than 64 blocks": dict(op="gather_blocks", dims=(1, 1, 65, 65, 3), idx=[0] * 65),
    "more than 64 blocks ": dict(op="fill_scaled_blocks", dims=(1, 1, 65, 0), strides=(65,)),
    "more than 64 blocks  ": dict(op="accum_scaled_blocks", dims=(1, 1, 65), strides=(65,), idx=[0] * 65),
    "more than 64 blocks   ": dict(op="ident_dev_multi", dims=(2, 65), strides=(2, 4), variant=1),
    "n_dst < bl.n": dict(op="gather_blocks", dims=(1, 1, 3, 2, 3), idx=[0, 1, 2]),
    "a block index outside the source": dict(op="gather_blocks", dims=(1, 1, 2, 2, 3), idx=[0, 3]),
    "a block index outside the source ": dict(op="accum_scaled_blocks", dims=(1, 1, 2), strides=(9,), idx=[0, -1]),
    "a negative entry in map2": dict(op="permute5", dims=(1, 1, 2, 1, 1), strides=(0, 0, 1, 0, 0), variant=1, idx=[0, -1]),
    "the int array is shorter": dict(op="permute5", dims=(1, 1, 3, 1, 1), strides=(0, 0, 1, 0, 0), variant=1, idx=[0, 1]),
    "a leading dimension below the row length": dict(op="transpose", dims=(3, 4, 1), strides=(3, 3, 0, 0)),
    "a leading dimension below the row length ": dict(op="copy2d", dims=(3, 4, 6), strides=(5, 4)),
    "a leading dimension below the row length  ": dict(op="multi_dot", dims=(5, 2), strides=(4,)),
    "the batches of the transpose's destination overlap": dict(op="transpose", dims=(3, 4, 2), strides=(4, 3, 12, 5)),
}


def test_the_check_refuses_each_violation_by_name(shim):
    for what, v in VIOLATIONS.items():
        msg, _ = shape(shim, v["op"], v["dims"], v.get("strides", ()), v.get("variant", 0), v.get("idx"))
        assert msg is not None and what.strip().encode() in msg and msg.startswith(b"vecop:"), (what, msg)
    big = [1 << 16] * 7
    # a source laid over the result (every kernel takes its pointers as __restrict__)
    assert b"a source overlaps a destination" in check(shim, "axpby", (8,), (), 0, big, alias=0)
    assert b"a source overlaps a destination" in check(shim, "transpose", (2, 2, 1), (2, 2, 0, 0), 0, big, alias=0)
    assert check(shim, "axpby", (8,), (), 0, big) is None
    # an input the op does not take may lie anywhere
    assert check(shim, "axpby", (8,), (), 0, big, alias=2) is None
    lim = (C.c_long * 7)()
    shim.vo_limits(lim)
    assert list(lim) == [vr.NPART, vr.MAXK, vr.SMALL_VEC_N, 64, 65535, 1 << 28, 128 << 20]
    n = (128 << 20) // 16 // 2
    assert check(shim, "copy_raw", (n,), (), 0, [n, 0, 0, 0, n, 0, 0]) is None
    assert b"more than 128 MB" in check(shim, "copy_raw", (n,), (), 0, [n, 0, 0, 0, n + 1, 0, 0])
    assert b"more than 128 MB" in check(shim, "copy_raw", (8,), (), 0, [8, 0, 1 << 60, 0, 8, 0, 0])


def test_zero_size_calls_are_empty_and_footprints_follow_the_strides(shim):
    for op, dims, strides, own in (("dot", (0,), (), 0), ("phys_diag", (0, 3, 5), (), 1), ("transpose", (3, 0, 2), (0, 3, 0, 0), 1),
                                   ("copy2d", (0, 4, 6), (6, 4), 1), ("multi_dot", (5, 0), (5,), 0), ("lincomb", (5, 2), (5,), 0),
                                   ("ident_dev_multi", (3, 0), (3, 9), 0), ("shell_sumsq", (0,), (), 0)):
        msg, f = shape(shim, op, dims, strides)
        assert msg is None and f["empty"] == 1 and f["own_return"] == own, (op, msg, f)
        assert all(f[k] == 0 for k in FOOT[:11])
    # no Krylov vector at all: the dots have nothing to write, the update still writes v and its norm, the combination zeros
    assert shape(shim, "multi_dot", (5, 0), (5,))[1]["empty"] == 1
    f = shape(shim, "arnoldi_update", (5, 0), (5,))[1]
    assert (f["empty"], f["zin0"], f["zin1"], f["zwr0"], f["rwr"]) == (0, 0, 0, 5, 256)
    f = shape(shim, "lincomb", (5, 0), (5,), 3)[1]
    assert (f["empty"], f["zin0"], f["zwr0"], f["rwr"]) == (0, 0, 5, 256)
    # the trace over an empty physical index still writes dl * dr zeros
    assert shape(shim, "phys_diag", (4, 0, 5), (), 1)[1]["zwr0"] == 20
    f = shape(shim, "transpose", (3, 4, 2), (6, 5, 40, 50))[1]
    assert (f["zin0"], f["zio0"], f["zwr0"]) == (40 + 2 * 6 + 4, 50 + 3 * 5 + 3, 50 + 3 * 5 + 3)
    f = shape(shim, "transpose", (3, 4, 5), (20, 15, 4, 3))[1]  # interleaved: rev3 of (3, 5, 4)
    assert (f["zin0"], f["zio0"]) == (60, 60)
    f = shape(shim, "permute5", (2, 3, 4, 1, 5), (100, 0, 7, 0, 1), 1, idx=[1, 9, 0, 2])[1]
    assert (f["zin0"], f["zio0"], f["idx"]) == (100 + 9 * 7 + 4 + 1, 120, 4)
    f = shape(shim, "fill_scaled_blocks", (3, 2, 4, 1), (20,))[1]
    assert (f["zin0"], f["zio0"]) == (6, 2 * 20 + 10)
    f = shape(shim, "accum_scaled_blocks", (3, 2, 2), (20,), idx=[5, 1])[1]
    assert (f["zin0"], f["zin1"], f["zio0"]) == (2 * 20 + 12, 6, 6)
    f = shape(shim, "lanczos_update_def", (7, 3), (), 1)[1]
    assert (f["zin0"], f["zin1"], f["zin2"], f["rin"], f["zio0"], f["rio"]) == (7, 7, 256, 768, 7, 256)
    f = shape(shim, "lanczos_step_small", (7,), (), 0)[1]  # x is vl, no vm2: one input
    assert (f["zin0"], f["zin1"], f["zin2"], f["rin"], f["zio1"]) == (7, 0, 0, 0, 256)
    f = shape(shim, "ident_dev_multi", (3, 4), (12, 3), 1)[1]
    assert (f["zin0"], f["rio"], f["zio0"], f["zio1"]) == (9 + 2 * 12 + 3, 4, 0, 4)


# ------------------------------------------------------------------------------------------------------ hook and mirror
def test_the_hook_is_declared_exported_and_mirrored(shim):
    from pytdscf_amd import _lib
    from pytdscf_amd import engine as E

    name = "mitdvp_vecop"
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert name in _lib.declared_symbols() and "typedef struct mitdvp_vecop_args" in header
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    lib = _lib.load()
    assert len(lib.mitdvp_vecop.argtypes) == 19
    assert [f for f, _ in _lib.VecopArgs._fields_] == ["op", "variant", "dims", "strides", "a", "b", "both", "eps", "coef", "f"]
    assert C.sizeof(_lib.VecopArgs) == shim.vo_sizeof_args()
    assert _lib.VecopArgs.strides.offset == shim.vo_offsetof_strides() and _lib.VecopArgs.eps.offset == shim.vo_offsetof_eps()
    assert _lib.VecopArgs.f.offset == shim.vo_offsetof_f()
    defines = re.findall(r"#define MITDVP_VECOP_([A-Z_0-9]+) (\d+)\b", header)
    assert [n.lower() for n, _ in defines] == list(_lib.VECOP_NAMES) and [int(k) for _, k in defines] == list(range(28))
    assert E.VECOP_OPS == {n: k for k, n in enumerate(_lib.VECOP_NAMES)}
    assert {r["op"] for r in vr.CASES} == set(_lib.VECOP_NAMES)  # one op per wrapper, every op in the table
    for n, _ in defines:  # the comment in the header is the op table
        assert re.search(rf"^ \*   {n}\s", header, re.M), n
    assert list(inspect.signature(E.vecop).parameters) == ["op", "dims", "strides", "variant", "z", "r", "idx", "mask", "zo", "ro", "a", "b",
                                                          "both", "eps", "coef", "f", "device"]
    assert lib.mitdvp_vecop(0, None, None, 0, None, 0, None, 0, None, 0, None, 0, 0, None, 0, None, 0, None, 0) == _lib.EINVAL
    with open(os.path.join(os.path.dirname(HERE), "README.md")) as f:
        m = re.search(r"C ABI, (\d+) entry points", f.read())
    assert m and int(m.group(1)) == len(_lib.declared_symbols())


def test_through_the_library_refusals_are_einval_and_accepted_calls_reach_hip():
    from pytdscf_amd import _lib
    from pytdscf_amd import engine as E
    from pytdscf_amd._lib import MitdvpError

    for name in ("dot-257-v1", "lanczos_step_small-1025-v3", "transpose-31x33x3-s36x37x1119x1224-v0", "permute5-2x3x5x2x7-s0x14x42x7x1-v1-kraus-in",
                 "accum_scaled_blocks-33x7x5-s68-v0", "ident_dev_multi-46x3-s138x46-v0-one"):
        r = vr.BY_NAME[name]
        g = vr.build(r)
        kw = dict(variant=r["variant"], z=g["z"], r=g["r"], idx=g["idx"], mask=g["mask"], zo=g["zo"], ro=g["ro"], eps=g["eps"], coef=g["coef"],
                  f=g["f"], device=-1)
        with pytest.raises(MitdvpError):  # accepted: the failure is HIP's
            E.vecop(r["op"], r["dims"], r["strides"], **kw)
        zo = [None if x is None else x[:-vr.GUARD - 1] for x in g["zo"]]
        with pytest.raises(ValueError, match="shorter than the operation's footprint"):
            E.vecop(r["op"], r["dims"], r["strides"], **dict(kw, zo=zo))
    w = np.ones(vr.SMALL_VEC_N + 1, complex)
    with pytest.raises(ValueError, match="n > SMALL_VEC_N"):
        E.vecop("lanczos_step_small", (w.size,), z=[w, None, None], zo=[w.copy(), np.zeros(256, complex)], ro=np.zeros(256), device=-1)
    with pytest.raises(ValueError, match="a source overlaps a destination"):
        _lib.check(_overlapping_call())
    with pytest.raises(ValueError, match="unknown op"):
        E.vecop("randn", (8,), zo=[w], device=-1)
    with pytest.raises(ValueError, match="k > MAXK"):
        E.vecop("multi_dot", (4, 22), (4,), z=[w, w, None], zo=[np.zeros(22 * 256, complex)], device=-1)
    # zero size: success before any HIP call, the results as they were
    keep = vr.sentinel(6)
    for op, dims in (("dot", (0,)), ("axpby", (0,)), ("sumsq", (0,)), ("shell_sumsq", (0,)), ("identity", (0, 4))):
        zo0, _, ro = E.vecop(op, dims, (4,) if op == "identity" else (), z=[w, w, None], zo=[keep, None], ro=keep.view(np.float64), device=-1)
        assert np.array_equal(vr.bits(zo0), vr.bits(keep)) and np.array_equal(vr.bits(ro), vr.bits(keep))


def _overlapping_call():
    """the raw entry point with a source inside the result (engine.vecop copies its results, so it cannot alias them)"""
    from pytdscf_amd import _lib
    from pytdscf_amd import engine as E

    buf = np.ones(16, complex)
    a = struct_of("axpby", (8,))
    p = E._dp(buf)
    q = C.cast(C.addressof(p.contents) + 4 * 16, C.POINTER(C.c_double))
    return _lib.load().mitdvp_vecop(-1, C.byref(a), p, 8, None, 0, None, 0, None, 0, None, 0, 0, q, 8, None, 0, None, 0)


# ------------------------------------------------------------------------------------------------------------- the models
def tiny(op, dims, strides=(), variant=0, **kw):
    r = dict(name=f"tiny-{op}-{variant}", group="tiny", op=op, dims=tuple(dims), strides=tuple(strides), variant=variant, **kw)
    g = vr.build(r)
    out = {k: np.asarray(vr.render(s)) for k, s in vr.expect(r, g).items()}
    return g, out


def close(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return a.shape == b.shape and np.abs(a - b).max() <= 1e-13 * max(1.0, np.abs(b).max())


def psum(p):
    return sum(complex(q) for q in p)


def test_vector_models_equal_plain_loops():
    n = 5
    for conj in (0, 1):
        g, out = tiny("dot", (n,), variant=conj)
        x, y = g["z"][:2]
        assert close(out["zo0"][0], sum((x[i].conjugate() if conj else x[i]) * y[i] for i in range(n)))
        assert not out["zo0"][1:256].any()
    g, out = tiny("sumsq", (n,))
    assert close(out["ro"][0], sum(abs(q) ** 2 for q in g["z"][0]))
    for v in (0, 1):
        g, out = tiny("lanczos_update", (n,), variant=v)
        alpha, bp = psum(g["z"][2]), (sum(g["r"]) ** 0.5 if v else 0.0)
        ref = [g["zo"][0][i] - alpha * g["z"][0][i] - (bp * g["z"][1][i] if v else 0) for i in range(n)]
        assert close(out["zo0"][:n], ref) and close(out["ro"][0], sum(abs(q) ** 2 for q in ref))
    for l, v, eps in ((0, 0, 1e-12), (1, 1, 1e-12), (3, 3, 1e-12), (3, 1, 1e-12), (3, 3, 1e300)):
        g, out = tiny("lanczos_update_def", (n, l), variant=v, eps=eps)
        nrm = g["r"].reshape(-1, 256)
        beta = sum(nrm[l - 1]) ** 0.5 if l > 0 else 0.0
        il = 1 / beta if l > 0 and beta >= eps else 1.0
        im = 1 / sum(nrm[l - 2]) ** 0.5 if l > 1 and sum(nrm[l - 2]) ** 0.5 >= eps else 1.0
        alpha = psum(g["z"][2]) * (il * il if v & 2 else il)
        ref = [g["zo"][0][i] * il - alpha * g["z"][0][i] * il - (beta * g["z"][1][i] * im if v & 1 else 0) for i in range(n)]
        assert close(out["zo0"][:n], ref) and close(out["ro"][0], sum(abs(q) ** 2 for q in ref)), (l, v)
    for v, eps in ((0, 1e-12), (1, 1e-12), (2, 1e-12), (3, 1e-12), (3, 1e300)):
        g, out = tiny("lanczos_step_small", (n,), variant=v, eps=eps)
        w, vl = g["zo"][0][:n], g["z"][0]
        x = g["z"][1] if v & 2 else vl
        alpha = sum(x[i].conjugate() * w[i] for i in range(n))
        bp = sum(g["r"]) ** 0.5 if v & 1 else 0.0
        u = [w[i] - alpha * vl[i] - (bp * g["z"][2][i] if v & 1 else 0) for i in range(n)]
        s = sum(abs(q) ** 2 for q in u)
        ref = [q / s ** 0.5 for q in u] if s ** 0.5 >= eps else u
        assert close(out["zo0"][:n], ref) and close(out["zo1"][0], alpha) and close(out["ro"][0], s), v
        assert not out["zo1"][1:256].any() and not out["ro"][1:256].any()
    g, out = tiny("scale_inv_norm", (n,))
    assert close(out["zo0"][:n], [q / sum(g["r"]) ** 0.5 for q in g["zo"][0][:n]])
    k, ldv = 3, n + 2
    g, out = tiny("multi_dot", (n, k), (ldv,))
    for j in range(k):
        assert close(out["zo0"][j * 256], sum(g["z"][0][j * ldv + i].conjugate() * g["z"][1][i] for i in range(n)))
    g, out = tiny("arnoldi_update", (n, k), (ldv,))
    h = [psum(g["z"][1][j * 256:(j + 1) * 256]) for j in range(k)]
    ref = [g["zo"][0][i] - sum(h[j] * g["z"][0][j * ldv + i] for j in range(k)) for i in range(n)]
    assert close(out["zo0"][:n], ref) and close(out["ro"][0], sum(abs(q) ** 2 for q in ref))
    g, out = tiny("lincomb", (n, k), (ldv,), variant=3)
    ref = [sum(g["coef"][j] * g["z"][0][j * ldv + i] for j in range(k)) for i in range(n)]
    assert close(out["zo0"][:n], ref) and close(out["ro"][0], sum(abs(q) ** 2 for q in ref))
    g, out = tiny("axpby", (n,))
    assert close(out["zo0"][:n], [g["a"] * g["z"][0][i] + g["b"] * g["zo"][0][i] for i in range(n)])
    g, out = tiny("scale", (n,))
    assert close(out["zo0"][:n], [g["a"] * g["zo"][0][i] for i in range(n)])


def test_layout_models_equal_plain_loops():
    rows, cols, batch, ldi, ldo, ibs, obs = 3, 4, 2, 6, 5, 30, 40
    g, out = tiny("transpose", (rows, cols, batch), (ldi, ldo, ibs, obs))
    ref = g["zo"][0].copy()
    for b in range(batch):
        for r in range(rows):
            for c in range(cols):
                ref[b * obs + c * ldo + r] = g["z"][0][b * ibs + r * ldi + c]
    assert np.array_equal(vr.bits(out["zo0"]), vr.bits(ref))
    na, nj, ns = 2, 3, 4
    g, out = tiny("transpose_rev3", (na, nj, ns))
    ref = [g["z"][0][(a * nj + j) * ns + s] for s in range(ns) for j in range(nj) for a in range(na)]
    assert np.array_equal(out["zo0"][:len(ref)], ref)
    d = (2, 3, 4, 2)
    g, out = tiny("permute_0213", d)
    ref = [g["z"][0][((i0 * d[1] + i1) * d[2] + i2) * d[3] + i3] for i0 in range(d[0]) for i2 in range(d[2]) for i1 in range(d[1])
           for i3 in range(d[3])]
    assert np.array_equal(out["zo0"][:len(ref)], ref)
    d, s, m2 = (2, 1, 3, 2, 2), (0, 0, 4, 2, 1), (2, 0, 1)
    g, out = tiny("permute5", d, s, 1, map2=m2)
    ref = [g["z"][0][i0 * s[0] + i1 * s[1] + m2[i2] * s[2] + i3 * s[3] + i4 * s[4]] for i0 in range(d[0]) for i1 in range(d[1])
           for i2 in range(d[2]) for i3 in range(d[3]) for i4 in range(d[4])]
    assert np.array_equal(out["zo0"][:len(ref)], ref)
    dl, n, dr = 2, 3, 2
    for trace in (0, 1):
        g, out = tiny("phys_diag", (dl, n, dr), variant=trace)
        Cc = g["z"][0].reshape(dl, n * n, dr)
        if trace:
            ref = [sum(Cc[b, c * n + c, e] for c in range(n)) for b in range(dl) for e in range(dr)]
            assert close(out["zo0"][:len(ref)], ref)
        else:
            ref = [Cc[b, c * n + c, e] for b in range(dl) for c in range(n) for e in range(dr)]
            assert np.array_equal(out["zo0"][:len(ref)], ref)
    rows, cols, zt, ldd, lds = 2, 3, 5, 7, 4
    for a, acc in ((1, 0), (0.3 - 0.7j, 0), (1, 1), (0.3 - 0.7j, 1)):
        g, out = tiny("copy2d", (rows, cols, zt), (ldd, lds), acc, a=a)
        ref = g["zo"][0].copy()
        for r in range(rows):
            for c in range(zt):
                ref[r * ldd + c] = a * g["z"][0][r * lds + c] + (g["zo"][0][r * ldd + c] if acc else 0) if c < cols else 0
        assert close(np.nan_to_num(out["zo0"]), np.nan_to_num(ref)) and np.array_equal(np.isnan(out["zo0"]), np.isnan(ref))
    g, out = tiny("copy_raw", (6,))
    assert np.array_equal(out["zo0"][:6], g["z"][0])
    g, out = tiny("identity", (3, 4), (6,))
    assert all(out["zo0"][r * 6 + c] == (r == c) for r in range(3) for c in range(4)) and np.isnan(out["zo0"][4])
    g, out = tiny("scale_cols", (3, 4), (6,))
    assert close([out["zo0"][r * 6 + c] for r in range(3) for c in range(4)], [g["zo"][0][r * 6 + c] * g["r"][c] for r in range(3) for c in range(4)])
    rows, cols, blk, n_dst, m_src, ldx, pos0 = 2, 3, (2, 0, 2), 4, 3, 20, 1
    g, out = tiny("gather_blocks", (rows, cols, 3, n_dst, m_src), blk=blk)
    ref = g["zo"][0].copy()
    for a in range(rows):
        for k in range(3):
            for c in range(cols):
                ref[(a * n_dst + k) * cols + c] = g["z"][0][(a * m_src + blk[k]) * cols + c]
    assert np.array_equal(vr.bits(out["zo0"]), vr.bits(ref))
    g, out = tiny("fill_scaled_blocks", (rows, cols, 3, pos0), (ldx,))
    for a in range(rows):
        for k in range(3):
            for c in range(cols):
                assert close(out["zo0"][a * ldx + (pos0 + k) * cols + c], g["f"][k] * g["z"][0][a * cols + c])
    assert np.isnan(out["zo0"][:pos0 * cols]).all() and np.isnan(out["zo0"][(pos0 + 3) * cols:ldx]).all()
    g, out = tiny("accum_scaled_blocks", (rows, cols, 3), (ldx,), blk=blk)
    for a in range(rows):
        for c in range(cols):
            ref = g["zo"][0][a * cols + c] + g["both"] * g["z"][1][a * cols + c] + sum(g["f"][k] * g["z"][0][a * ldx + blk[k] * cols + c] for k in range(3))
            assert close(out["zo0"][a * cols + c], ref)
    g, out = tiny("col_sumsq", (4, 3))
    x = g["z"][0].reshape(4, 3)
    assert close(out["ro"][:3], [sum(abs(x[r, c]) ** 2 for r in range(4)) for c in range(3)])
    g, out = tiny("row_sumsq", (4, 3))
    assert close(out["ro"][:4], [sum(abs(x) ** 2 for x in g["z"][0].reshape(4, 3)[r]) for r in range(4)])
    g, out = tiny("shell_sumsq", (4,))
    x = g["z"][0].reshape(4, 4)
    assert close(out["ro"][:4], [sum(abs(x[i, j]) ** 2 for i in range(4) for j in range(4) if max(i, j) == t) for t in range(4)])
    for D in range(1, 5):
        assert close(sum(out["ro"][:D]), sum(abs(x[i, j]) ** 2 for i in range(D) for j in range(D)))


def test_identity_models_equal_plain_loops():
    for kind, want in (("exact", 0.0), ("off", 0.375), ("imag", 3e-7), ("nan", 1e308), ("+inf", 1e308), ("-inf", 1e308)):
        g, out = tiny("ident_dev", (4,), (6,), kind=kind)
        assert out["ro"][0] == want, kind
    g, out = tiny("ident_dev", (4,), (6,), kind="off")
    m = 0.0
    for r in range(4):
        for c in range(4):
            v = g["z"][0][r * 6 + c]
            m = max(m, abs(v.real - (r == c)), abs(v.imag))
    assert out["ro"][0] == m
    for clear in (1, 0):
        g, out = tiny("ident_dev_multi", (3, 4), (12, 3), clear, mask=0b1101, bad=2)
        for c in range(4):
            on = c != 1
            lam = g["z"][0][c * 3]
            m = 0.0
            for r in range(3):
                for q in range(3):
                    v = g["z"][0][c * 3 + r * 12 + q]
                    m = max(m, abs(v.real - lam.real * (r == q)), abs(v.imag - lam.imag * (r == q)))
            if on:
                assert out["zo1"][c] == lam and out["ro"][c] == (m if clear else max(m, g["ro"][c])), (clear, c)
                assert (m > 0.2) == (c == 2)
            else:
                assert np.isnan(out["zo1"][c]) and (out["ro"][c] == 0.0 if clear else vr.bits(out["ro"])[c] == vr.bits(g["ro"])[c])


# --------------------------------------------------------------------------------------------------- the power of the table
MUTANT_OPS = {
    "drop_last": None,  # every op that has a last element
    "p0": ("lanczos_update", "lanczos_update_def", "scale_inv_norm", "arnoldi_update", "lanczos_step_small"),
    "p64": ("lanczos_update", "lanczos_update_def", "scale_inv_norm", "arnoldi_update", "lanczos_step_small"),
    "ld_cols": ("transpose", "copy2d", "identity", "scale_cols", "multi_dot", "arnoldi_update", "lincomb", "ident_dev"),
    "no_bs": ("transpose",),
    "no_map2": ("permute5",),
    "swap12": ("permute_0213",),
    "conj_flip": ("dot",),
    "no_orthodox": ("lanczos_update_def",),
    "no_zero_to": ("copy2d",),
    "no_pos0": ("fill_scaled_blocks",),
    "nan_fmax": ("ident_dev",),
    "slot0": ("lanczos_step_small",),
}


def misses(r, mut):
    g = vr.build(r)
    true, mutant = vr.expect(r, g), vr.expect(r, g, (mut,))
    return any(not vr.judge(true[k], vr.render(mutant[k]))[0] for k in true)


@pytest.mark.parametrize("mut", vr.MUTATIONS)
def test_a_mutated_model_misses_the_table(mut):
    assert set(MUTANT_OPS) == set(vr.MUTATIONS)
    rows = [r for r in vr.CASES if int(np.prod(r["dims"], dtype=np.int64)) <= 20000 and (MUTANT_OPS[mut] is None or r["op"] in MUTANT_OPS[mut])]
    per_op = {}
    for r in rows:
        if per_op.get(r["op"]) or (mut == "drop_last" and r["op"] in ("identity", "ident_dev", "ident_dev_multi", "fill_scaled_blocks",
                                                                    "accum_scaled_blocks", "copy2d", "scale_cols", "phys_diag")):
            continue  # one missing row per op is enough; drop_last is modelled for the ops that loop over a flat index
        per_op[r["op"]] = per_op.get(r["op"], False) or misses(r, mut)
    print(f"[vecops] mutant {mut}: caught in {sorted(k for k, v in per_op.items() if v)}")
    assert per_op and all(per_op.values()), (mut, {k: v for k, v in per_op.items() if not v})
    if MUTANT_OPS[mut] is not None:
        assert set(per_op) == set(MUTANT_OPS[mut])
