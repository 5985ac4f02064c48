"""CPU: the test hook of the batch kernels' building blocks (``mitdvp_batch_block`` / ``engine.batch_block``), the NumPy
models the GPU tests hold it to (``helpers.batch_blocks_ref``) and the table of cases they share.

* the models equal plain Python loops over the formulas on two tiny shapes per operation, and the packers equal the
  engine's;
* ``csrc/batch_block_check.h`` (compiled with g++ into a throw-away shim) accepts every row of ``CASES`` with the footprint
  the table computes, and refuses each violation of the kernels' envelope by name;
* through the real library the refusals come back as EINVAL without a GPU; an accepted call sent to device -1 ends in a
  HIP error, never in EINVAL;
* the hook is declared, exported and mirrored with its argument count and struct layout;
* the reference alone meets every bar of the GPU test with a factor of 10 to spare (the complex128 models against extended
  precision, ``numpy.linalg.qr`` and ``numpy.linalg.svd`` through the checkers on every row), and the designed inputs have
  the property their row claims.
"""

import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import batch_blocks_ref as rr

HERE = os.path.dirname(os.path.abspath(__file__))
OPS = ("matmul", "heff", "keff", "env", "overlap", "qr", "split")


def rows(op):
    return [r for r in rr.CASES if r["op"] == op]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    from pytdscf_amd import _lib

    out = tmp_path_factory.mktemp("bb") / "libbb.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "helpers", "batch_block_shim.cpp"), "-o", str(out)],
                   check=True)
    lib = C.CDLL(str(out))
    lib.bb_shape.restype = C.c_char_p
    lib.bb_shape.argtypes = [C.POINTER(_lib.BatchBlockArgs), C.POINTER(C.c_size_t)]
    lib.bb_check.restype = C.c_char_p
    lib.bb_check.argtypes = [C.POINTER(_lib.BatchBlockArgs), C.POINTER(C.c_size_t), C.c_size_t, C.c_size_t, C.c_size_t]
    lib.bb_limits.argtypes = [C.POINTER(C.c_long)]
    return lib


def struct_of(op, dims, variant=0, ncopies=1, scl=1.0):
    from pytdscf_amd import _lib
    from pytdscf_amd import engine as E

    a = _lib.BatchBlockArgs()
    a.op = E.BATCH_BLOCK_OPS[op] if isinstance(op, str) else op
    a.variant, a.ncopies, a.scl = variant, ncopies, scl
    for k, v in enumerate(dims):
        a.dims[k] = v
    return a


# ------------------------------------------------------------------------------------------------------------- the models
def test_product_models_equal_the_formulas_looped():
    rng = np.random.default_rng(1)
    for M, N, K in ((2, 3, 4), (3, 1, 2)):
        A, B = rr.gauss(rng, M, K), rr.gauss(rng, K, N)
        ref = np.array([[sum(A[m, k] * B[k, n] for k in range(K)) for n in range(N)] for m in range(M)])
        assert np.abs(rr.matmul(A, B) - ref).max() < 1e-14
    for dl, d, dr, ml, mr in ((2, 2, 3, 2, 1), (1, 3, 2, 2, 3)):
        L, W, R, v = rr.gauss(rng, dl, ml, dl), rr.gauss(rng, ml, d, d, mr), rr.gauss(rng, dr, mr, dr), rr.gauss(rng, dl, d, dr)
        ref = np.zeros((dl, d, dr), complex)
        for a in range(dl):
            for i in range(d):
                for r in range(dr):
                    ref[a, i, r] = sum(L[a, c, b] * W[c, i, j, t] * R[r, t, s] * 0.5 * v[b, j, s] for c in range(ml) for b in range(dl)
                                       for j in range(d) for t in range(mr) for s in range(dr))
        assert np.abs(rr.heff(L, W, R, v, scl=0.5) - ref).max() < 1e-13
    for dim, m in ((2, 3), (3, 1)):
        L, R, v = rr.gauss(rng, dim, m, dim), rr.gauss(rng, dim, m, dim), rr.gauss(rng, dim, dim)
        ref = np.array([[sum(L[a, c, b] * 2.0 * v[b, s] * R[r, c, s] for c in range(m) for b in range(dim) for s in range(dim))
                         for r in range(dim)] for a in range(dim)])
        assert np.abs(rr.keff(L, R, v, scl=2.0) - ref).max() < 1e-13
    for din, mi, d, dout, mo in ((2, 2, 2, 3, 1), (3, 1, 2, 2, 2)):
        env = rr.gauss(rng, din, mi, din)
        # forward: tensors (din, d, dout), core (min, d, d, mout)
        W, bra, ket = rr.gauss(rng, mi, d, d, mo), rr.gauss(rng, din, d, dout), rr.gauss(rng, din, d, dout)
        ref = np.zeros((dout, mo, dout), complex)
        for a in range(dout):
            for q in range(mo):
                for r in range(dout):
                    ref[a, q, r] = sum(np.conj(bra[b, i, a]) * env[b, p, s] * W[p, i, j, q] * ket[s, j, r] for b in range(din)
                                       for i in range(d) for p in range(mi) for s in range(din) for j in range(d))
        assert np.abs(rr.env_fwd(env, W, bra, ket) - ref).max() < 1e-13
        # backward: tensors (dout, d, din), core (mout, d, d, min)
        W, bra, ket = rr.gauss(rng, mo, d, d, mi), rr.gauss(rng, dout, d, din), rr.gauss(rng, dout, d, din)
        for a in range(dout):
            for q in range(mo):
                for r in range(dout):
                    ref[a, q, r] = sum(np.conj(bra[a, i, b]) * env[b, t, s] * W[q, i, j, t] * ket[r, j, s] for b in range(din)
                                       for i in range(d) for t in range(mi) for s in range(din) for j in range(d))
        assert np.abs(rr.env_bwd(env, W, bra, ket) - ref).max() < 1e-13
    for d, bonds in ((2, (1, 3, 2, 1)), (3, (1, 2, 1))):
        ket = [rr.gauss(rng, bonds[p], d, bonds[p + 1]) for p in range(len(bonds) - 1)]
        bra = [rr.gauss(rng, bonds[p], d, bonds[p + 1]) for p in range(len(bonds) - 1)]

        def dense(sites):
            psi = sites[0]
            for t in sites[1:]:
                psi = np.tensordot(psi, t, axes=(psi.ndim - 1, 0))
            return psi.reshape(-1)

        assert abs(rr.overlap(ket, bra) - np.vdot(dense(bra), dense(ket))) < 1e-13 * np.linalg.norm(dense(bra)) * np.linalg.norm(dense(ket))


def test_the_packers_equal_the_engines():
    from pytdscf_amd import engine as E

    W = rr.gauss(np.random.default_rng(2), 3, 2, 2, 5)
    for order in ("w2l", "w2el", "w2er"):
        assert np.array_equal(E.pack_w2(W, order), rr.pack_w2(W, order))
    with pytest.raises(ValueError):
        E.pack_w2(W, "w2r")


# ----------------------------------------------------------------------------------------------------- the table and limits
def test_the_table_holds_what_it_promises():
    assert len({r["name"] for r in rr.CASES}) == len(rr.CASES)
    mm = [r["dims"] for r in rows("matmul")]
    for role in range(3):  # every tile edge as M, as N and as K of the plain product
        assert set(rr.TILE_EDGES) <= {q[role] for q in mm}
    assert any(q[1] == q[2] and q[0] != q[2] for q in mm) and any(q[0] == q[2] and q[1] != q[2] for q in mm)
    assert sum(q[0] == q[1] == q[2] for q in mm) >= 3
    for op in ("heff", "env"):  # the corners; composite dimensions on and around 16 / 32 / 64 in every role
        assert {r.get("plain", r["dims"]) for r in rows(op) if r["corner"]} == set(rr.CORNERS)
        for role in range(3):
            got = {g[role] for r in rows(op) for g in rr.gemm_dims(r)}
            assert {1, 15, 16, 17, 32, 33, 65} <= got, (op, role, sorted(got))
    assert {r["dims"] for r in rows("keff")} == {(dim, m) for dim in (1, 17, 64) for m in (1, 16)}
    env = rows("env")
    assert {(r["variant"], r["same"]) for r in env} == {(0, True), (0, False), (1, True), (1, False), (2, False)}
    assert {(r["dims"], r["kind"]) for r in rows("qr")} == {(s, k) for s in rr.QR_SHAPES for k in rr.QR_KINDS}
    assert {(r["dims"], r["kind"]) for r in rows("split")} == {(s, k) for s in rr.SPLIT_SHAPES for k in rr.SPLIT_KINDS}
    assert any(len(rr.gemm_dims(r)) == 12 for r in rows("overlap"))


def test_the_check_accepts_every_row_with_the_tables_footprint(shim):
    lim = (C.c_long * 6)()
    shim.bb_limits(lim)
    assert tuple(lim) == (rr.MAX_SITE, rr.MAX_MPO, rr.MAX_BOND, rr.PAIR_MAX_DIM, rr.MAX_COPIES, rr.MAX_CHAIN)
    from pytdscf_amd import engine as E

    for r in rr.CASES:
        for nc in (1, 3, 16):
            a = struct_of(r["op"], r["dims"], r["variant"], nc)
            out = (C.c_size_t * 10)()
            assert shim.bb_shape(C.byref(a), out) is None, r["name"]
            f = rr.footprint(r)
            assert list(out[:4]) == f["ins"] and (out[4], out[5], out[6]) == (f["out0"], f["out1"], f["info"]), r["name"]
            assert E.batch_block_footprint(r["op"], r["dims"]) == {k: f[k] for k in ("out0", "out1", "info")}
            nin = (C.c_size_t * 4)(*f["ins"])
            sizes = [nc * f["out0"], nc * f["out1"], nc * f["info"]]
            assert shim.bb_check(C.byref(a), nin, *sizes) is None, r["name"]
            # one element short, in each operand and each result, is refused by name
            for k in range(4):
                if f["ins"][k]:
                    short = (C.c_size_t * 4)(*[v - (q == k) for q, v in enumerate(f["ins"])])
                    assert f"operand {k} is shorter".encode() in shim.bb_check(C.byref(a), short, *sizes)
            for k, word in enumerate((b"result 0 is shorter", b"result 1 is shorter", b"info record is shorter")):
                if sizes[k]:
                    s2 = list(sizes)
                    s2[k] -= 1
                    assert word in shim.bb_check(C.byref(a), nin, *s2), (r["name"], word)


VIOLATIONS = {
    "unknown op": (("bad-op", 7), (1, 1, 1), 0, 1),
    "unknown op ": (("bad-op", -1), (1, 1, 1), 0, 1),
    "unknown variant": ("matmul", (4, 4, 4), 3, 1),
    "unknown variant of this op": ("heff", (2, 2, 2, 1, 1), 1, 1),
    "a dimension below 1": ("matmul", (4, 0, 4), 0, 1),
    "a dimension below 1 ": ("split", (4, 4, -2), 0, 1),
    "ncopies outside": ("matmul", (4, 4, 4), 0, 0),
    "ncopies outside ": ("matmul", (4, 4, 4), 0, 17),
    "dst = A needs N = K": ("matmul", (4, 5, 4), 1, 1),
    "dst = B needs M = K": ("matmul", (5, 4, 4), 2, 1),
    "more than BATCH_MAX_SITE": ("matmul", (128, 65, 3), 0, 1),
    "more than BATCH_MAX_SITE ": ("heff", (64, 3, 64, 1, 1), 0, 1),
    "more than BATCH_MAX_SITE  ": ("env", (64, 1, 3, 64, 1), 0, 1),
    "more than BATCH_MAX_SITE   ": ("qr", (513, 16), 0, 1),
    "a bond above BATCH_MAX_BOND": ("heff", (65, 1, 2, 1, 1), 0, 1),
    "a bond above BATCH_MAX_BOND ": ("keff", (65, 1), 0, 1),
    "a bond above BATCH_MAX_BOND  ": ("env", (2, 1, 1, 65, 1), 2, 1),
    "a bond above BATCH_MAX_BOND   ": ("overlap", (3, 2, 65, 2), 0, 1),
    "a bond above BATCH_MAX_BOND    ": ("qr", (100, 65), 0, 1),
    "an MPO bond above BATCH_MAX_MPO": ("heff", (2, 2, 2, 17, 1), 0, 1),
    "an MPO bond above BATCH_MAX_MPO ": ("keff", (2, 17), 0, 1),
    "an MPO bond above BATCH_MAX_MPO  ": ("env", (2, 1, 2, 2, 17), 1, 1),
    "1 .. 6 sites": ("overlap", (7, 2, 2, 2, 2, 2, 2, 2), 0, 1),
    "a thin QR needs m >= n": ("qr", (8, 9), 1, 1),
    "split m or n above BATCH_PAIR_MAX_DIM": ("split", (129, 8, 8), 0, 1),
    "split m or n above BATCH_PAIR_MAX_DIM ": ("split", (8, 129, 8), 0, 1),
    "split r above min(m, n, BATCH_MAX_BOND)": ("split", (8, 9, 9), 0, 1),
    "split r above min(m, n, BATCH_MAX_BOND) ": ("split", (9, 8, 9), 0, 1),
    "split r above min(m, n, BATCH_MAX_BOND)  ": ("split", (128, 128, 65), 0, 1),
}


def _violation(spec):
    op, dims, variant, nc = spec
    return struct_of(op[1] if isinstance(op, tuple) else op, dims, variant, nc)


def test_the_check_refuses_each_violation_by_name(shim):
    big = 1 << 26
    nin = (C.c_size_t * 4)(big, big, big, big)
    for what, spec in VIOLATIONS.items():
        msg = shim.bb_check(C.byref(_violation(spec)), nin, big, big, big)
        assert msg is not None and what.strip().encode() in msg and msg.startswith(b"batch_block:"), (what, msg)
    assert b"null descriptor" in shim.bb_check(None, nin, big, big, big)
    # the limits themselves are inside
    for op, dims, variant in (("heff", (64, 2, 64, 16, 16), 0), ("qr", (512, 16), 1), ("split", (128, 128, 64), 0), ("keff", (64, 16), 0),
                              ("overlap", (6, 2, 2, 64, 64, 2, 1), 0), ("matmul", (128, 64, 64), 1)):
        assert shim.bb_check(C.byref(struct_of(op, dims, variant, 16)), nin, big, big, big) is None, (op, dims)


# ------------------------------------------------------------------------------------------------------ hook and mirror
def test_the_hook_is_declared_exported_and_mirrored(shim):
    from pytdscf_amd import _lib
    from pytdscf_amd import engine as E

    name = "mitdvp_batch_block"
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert name in _lib.declared_symbols() and "typedef struct mitdvp_batch_block_args" in header
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    lib = _lib.load()
    assert len(lib.mitdvp_batch_block.argtypes) == 16
    assert [f for f, _ in _lib.BatchBlockArgs._fields_] == ["op", "variant", "dims", "ncopies", "scl"]
    assert C.sizeof(_lib.BatchBlockArgs) == shim.bb_sizeof_args()
    assert _lib.BatchBlockArgs.ncopies.offset == shim.bb_offsetof_ncopies() and _lib.BatchBlockArgs.scl.offset == shim.bb_offsetof_scl()
    for k, op in enumerate(("MATMUL", "HEFF", "KEFF", "ENV", "OVERLAP", "QR", "SPLIT")):
        assert re.search(rf"#define MITDVP_BLOCK_{op} {k}\b", header) and getattr(_lib, f"BLOCK_{op}") == k
        assert E.BATCH_BLOCK_OPS[op.lower()] == k
    assert list(inspect.signature(E.batch_block).parameters) == ["op", "dims", "operands", "ncopies", "variant", "scl", "device"]
    assert lib.mitdvp_batch_block(0, None, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0) == _lib.EINVAL
    # the README counts the entry points of the header
    with open(os.path.join(os.path.dirname(HERE), "README.md")) as f:
        m = re.search(r"C ABI, (\d+) entry points", f.read())
    assert m and int(m.group(1)) == len(_lib.declared_symbols())


def call(a, f, nc, short=None):
    """the hook on buffers of exactly the footprint (one element less in ``short``), on device -1: EINVAL = refused by the
    host check, anything else = the check passed (the call then fails at hipSetDevice, before anything is allocated)"""
    from pytdscf_amd import _lib
    from pytdscf_amd import engine as E

    sizes = dict(in0=f["ins"][0], in1=f["ins"][1], in2=f["ins"][2], in3=f["ins"][3], out0=nc * f["out0"], out1=nc * f["out1"])
    if short in sizes:
        sizes[short] -= 1
    ninfo = nc * f["info"] - (short == "info")
    args = []
    for k in ("in0", "in1", "in2", "in3", "out0", "out1"):
        buf = np.zeros(max(sizes[k], 1), np.complex128)
        args += [E._dp(buf) if sizes[k] or k.startswith("out") else None, sizes[k]]
    info = np.zeros(max(ninfo, 1))
    rc = _lib.load().mitdvp_batch_block(-1, C.byref(a), *args, E._dp(info), ninfo)
    return rc, _lib.load().mitdvp_last_error(None).decode()


def test_through_the_library_refusals_are_einval_and_accepted_calls_reach_hip():
    from pytdscf_amd import _lib

    picks = ["matmul-33x33x33", "heff-64x2x64x16x16", "keff-17-16", "env-mirror-cross-7x3x33x5x16", "overlap-L4-d2-2-64-17", "qr-gauss-130x33",
             "split-geometric-127x65-r64"]
    for name in picks:
        r = rr.BY_NAME[name]
        f = rr.footprint(r)
        a = struct_of(r["op"], r["dims"], r["variant"], 3)
        rc, msg = call(a, f, 3)
        assert rc not in (_lib.OK, _lib.EINVAL), (name, rc, msg)
        for short in ("in0", "in1", "in2", "in3", "out0", "out1", "info"):
            if short[2:].isdigit() and not f["ins"][int(short[2])] or short == "out1" and not f["out1"]:
                continue
            rc, msg = call(a, f, 3, short)
            assert rc == _lib.EINVAL and "shorter than the operation's footprint" in msg, (name, short, rc, msg)
    f = dict(ins=[1 << 20] * 4, out0=1 << 20, out1=1 << 20, info=1 << 10)
    for what, spec in VIOLATIONS.items():
        rc, msg = call(_violation(spec), f, 1)
        assert rc == _lib.EINVAL and what.strip() in msg, (what, rc, msg)


def test_the_python_wrapper_raises_before_the_device_is_touched():
    from pytdscf_amd import engine as E
    from pytdscf_amd._lib import MitdvpError

    A = np.ones((4, 4), complex)
    with pytest.raises(ValueError, match="dst = A needs N = K"):
        E.batch_block("matmul", (4, 5, 4), A, np.ones((4, 5), complex), variant=1, device=-1)
    with pytest.raises(ValueError, match="ncopies outside"):
        E.batch_block("matmul", (4, 4, 4), A, A, ncopies=17, device=-1)
    with pytest.raises(ValueError, match="operand 1 is shorter"):
        E.batch_block("matmul", (4, 4, 4), A, A[:3], device=-1)
    with pytest.raises(ValueError, match="split r above"):
        E.batch_block("split", (8, 8, 9), np.ones((8, 8), complex), device=-1)
    with pytest.raises(ValueError, match="unknown op"):
        E.batch_block("svd", (8, 8), A, device=-1)
    with pytest.raises(MitdvpError):  # accepted: the failure is HIP's
        E.batch_block("matmul", (4, 4, 4), A, A, device=-1)


# ------------------------------------------------------------------------------------------- the reference against the bars
@pytest.mark.parametrize("op", ["matmul", "heff", "keff", "env", "overlap"])
def test_the_complex128_models_meet_a_tenth_of_the_product_bar(op):
    worst = 0.0
    for r in rows(op):
        plain = rr.product_input(r)
        worst = max(worst, rr.product_defect(rr.model(r, plain), rr.model(r, plain, dtype=np.clongdouble)))
    print(f"[batch_blocks] {op}: complex128 model against extended precision, worst {worst:.2e} (bar / 10 = {rr.PRODUCT_BAR / 10:.0e})")
    assert worst < rr.PRODUCT_BAR / 10


@pytest.mark.parametrize("kind", rr.QR_KINDS)
def test_lapack_qr_meets_a_tenth_of_the_qr_bars_and_the_inputs_are_what_they_claim(kind):
    for r in rows("qr"):
        if r["kind"] != kind:
            continue
        A = rr.qr_input(r)
        m, n = r["dims"]
        q, rm = np.linalg.qr(A)
        rm = np.triu(rm)
        rr.check_qr(A, q, rm, lapack=False, margin=0.1)
        sv = np.linalg.svd(A, compute_uv=False)
        col = np.linalg.norm(A, axis=0)
        if kind == "product":
            assert (col > 0).sum() == 1 and col[0] > 0
        elif kind == "zerocol":
            assert col[n // 2] == 0.0 and (col > 0).sum() == n - 1
        elif kind == "equalcols" and n > 1:
            assert np.array_equal(A[:, n - 1], A[:, (n - 1) // 2]) and (sv > 1e-12 * sv[0]).sum() == n - 1
        elif kind == "graded24" and n > 1:
            assert 1e23 < col[0] / col[-1] < 1e25 and np.all(np.diff(np.log10(col)) < 0.5)
        elif kind == "tiny":
            assert 1e-101 < np.abs(A).max() < 1e-98
        elif kind == "gauss":
            assert sv[-1] > 1e-6 * sv[0]


@pytest.mark.parametrize("kind", rr.SPLIT_KINDS)
def test_lapack_split_meets_a_tenth_of_the_split_bars_and_the_inputs_are_what_they_claim(kind):
    nproj, exempt = 0, []
    for r in rows("split"):
        if r["kind"] != kind:
            continue
        m, n, rk = r["dims"]
        theta, s, V = rr.split_input(r)
        c = rr.split_claims(r, theta)
        if s is not None:  # the projector flag follows the PRESCRIBED spectrum, not LAPACK's rounding of it
            nxt = s[rk] if rk < len(s) else 0.0
            wide = s[rk - 1] > 0 and s[rk - 1] >= 2 * nxt
            if rk == n or (wide and s[rk - 1] - nxt >= rr.PROJ_MIN_GAP * c["nf"]):
                assert c["projector"], r["name"]
            elif wide:
                assert not c["projector"], r["name"]
                exempt.append(r["name"])
            else:
                assert not c["projector"], r["name"]
        B, Cp, info = rr.lapack_split(theta, rk)
        rr.check_split(r, theta, B, Cp, info, claims=c, margin=0.1)
        k = min(m, n)
        if s is not None:  # LAPACK finds the prescribed values in the realised matrix, down to what double precision holds
            assert np.abs(c["sv"] - s).max() < 1e-14 * c["nf"] * np.sqrt(k)
        if kind == "geometric" and k > 1:
            assert np.allclose(s[:-1] / s[1:], 2.0)
        elif kind == "graded12" and k > 1:
            assert np.isclose(s[0] / s[-1], 1e12)
        elif kind == "degenerate-cut" and k > 1:
            hi = min(rk, k - 1)
            assert s[hi] == s[hi - 1] and abs(c["sv"][hi] - c["sv"][hi - 1]) < 1e-14 * c["nf"]
            assert rk == k or not c["projector"]  # no projector is defined across a degenerate cut
        elif kind == "cluster" and rk >= 4:
            assert s[1] == s[2] == s[3] and s[0] > s[1] and (rk == k or s[rk - 1] >= 2 * s[rk]) and c["projector"]
        elif kind in ("rank-1", "rank-r-1"):
            want = 1 if kind == "rank-1" else max(rk - 1, 1)
            assert c["rank"] == want and (rk == n or not (c["projector"] and want < rk))
        elif kind == "one-entry":
            assert np.count_nonzero(theta) == 1 and c["rank"] == 1 and c["projector"] == (rk == n or rk == 1)
        nproj += c["projector"]
        if c["projector"] and V is not None:  # where the projector bar applies LAPACK itself resolves the directions
            P = V[:, :rk] @ V[:, :rk].conj().T
            assert np.abs(c["P"] - P).max() < rr.SPLIT_PROJ_BAR / 10, r["name"]
    print(f"[batch_blocks] split {kind}: projector bar on {nproj} of {len(rr.SPLIT_SHAPES)} shapes")
    # the rows a ratio of at least 2 would admit and the absolute gap takes out are exactly the listed ones
    assert exempt == [n for n in rr.PROJECTOR_EXEMPT if f"-{kind}-" in n], exempt
    assert nproj == rr.PROJECTOR_COUNT[kind], (kind, nproj)
    if kind == "cluster":  # this spectrum carries the projector bar at every shape, the limits 127 x 65 and 128 x 128 included
        assert rr.PROJECTOR_COUNT[kind] == len(rr.SPLIT_SHAPES)
    if kind == "geometric":
        assert rr.split_claims(rr.BY_NAME["split-geometric-8x8-r4"], rr.split_input(rr.BY_NAME["split-geometric-8x8-r4"])[0])["projector"]
