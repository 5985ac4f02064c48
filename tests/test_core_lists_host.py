"""CPU: the coefficient lists of the two core contractions (csrc/core_lists.h: build_fold_list, build_gram_list), compiled
with g++ into a throw-away shim and compared with a NumPy twin written from the dense kernels' loops
(csrc/vecops.hip::k_fold_env_core, k_gram_env_core): the twin walks the core the way a wave of those kernels does and
writes down what it would multiply with.  The blobs must equal the twin's byte for byte; expanded again they must give the
dense core exactly, and their entries / mask bits must be exactly the non-zero groups / coefficients."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRY = np.dtype([("c", "<i4"), ("pad", "<i4", (3,)), ("f", "<c16", (4,))])  # FoldEntry: 80 bytes


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("cl") / "libcl.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "helpers", "core_lists_shim.cpp"), "-o", str(out)],
                   check=True)
    lib = C.CDLL(str(out))
    vp, st = C.c_void_p, C.c_size_t
    lib.cl_fold_list.restype, lib.cl_fold_list.argtypes = st, [vp, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long, vp, st]
    lib.cl_gram_list.restype, lib.cl_gram_list.argtypes = st, [vp, C.c_int, C.c_int, C.c_int, vp, st]
    for name in ("cl_fold_head", "cl_gram_head", "cl_gram_records"):
        getattr(lib, name).restype = st
    assert lib.cl_fold_entry_bytes() == ENTRY.itemsize == 80
    return lib


def _fold_blob(shim, w, d, m, strides):
    w = np.ascontiguousarray(w)
    n = shim.cl_fold_list(w.ctypes.data, d, m, *strides, None, 0)
    out = np.zeros(n, dtype=np.uint8)
    assert shim.cl_fold_list(w.ctypes.data, d, m, *strides, out.ctypes.data, n) == n
    return out


def _gram_blob(shim, ws, d, m, tu):
    ws = np.ascontiguousarray(ws)
    n = shim.cl_gram_list(ws.ctypes.data, d, m, tu, None, 0)
    out = np.zeros(n, dtype=np.uint8)
    assert shim.cl_gram_list(ws.ctypes.data, d, m, tu, out.ctypes.data, n) == n
    return out


# the two layouts choose_apply_forms folds: w_l[i][c][j] and w_r[i][j][t]; (axes of the array, (wi, wj, wm))
def _layouts(d, m):
    return {"l_icj": ((0, 2, 1), (m * d, 1, d)), "r_ijc": ((0, 1, 2), (d * m, m, 1))}


def _sparse_core(rng, d, m, density):
    """(d, d, m) indexed [i][j][c], most elements exactly zero, one of them a negative zero (which is a zero)"""
    w = (rng.standard_normal((d, d, m)) + 1j * rng.standard_normal((d, d, m))) * (rng.random((d, d, m)) < density)
    w[0, 0, 0] = complex(-0.0, 0.0)
    return w


def _fold_twin(w, d, m):
    """from w[i][j][c]: (offsets, entries) as a wave of k_fold_env_core meets them"""
    njb = (d + 3) // 4
    off, ent = [0], []
    for item in range(d * njb):
        i, j0 = item // njb, (item % njb) * 4
        for c in range(m):
            f = [w[i, min(j0 + u, d - 1), c] for u in range(4)]
            if any(x.real != 0.0 or x.imag != 0.0 for x in f):
                ent.append((c, f))
        off.append(len(ent))
    return off, ent


def _check_fold(shim, w, d, m):
    njb = (d + 3) // 4
    off, ent = _fold_twin(w, d, m)
    for name, (axes, strides) in _layouts(d, m).items():
        stored = np.ascontiguousarray(np.transpose(w, np.argsort(axes)))  # element (i, j, c) at i wi + j wj + c wm
        blob = _fold_blob(shim, stored, d, m, strides)
        head = shim.cl_fold_head(d)
        assert head % 16 == 0 and head >= 4 * (d * njb + 1) and len(blob) == head + 80 * len(ent), name
        got_off = blob[: 4 * (d * njb + 1)].view("<i4")
        got = blob[head:].view(ENTRY)
        assert list(got_off) == off, name
        assert [int(c) for c in got["c"]] == [c for c, _ in ent], name
        want_f = np.array([f for _, f in ent], dtype=np.complex128).reshape(len(ent), 4)
        assert np.array_equal(got["f"].view(np.float64), want_f.view(np.float64)), name  # bits: the sign of a zero too
        assert not blob[4 * (d * njb + 1) : head].any() and not got["pad"].any()
        # expanded again: the dense core, exactly; every c of an item that is no entry is a group of zeros
        back = np.zeros((d, d, m), dtype=np.complex128)
        for item in range(d * njb):
            i, j0 = item // njb, (item % njb) * 4
            cs = got["c"][got_off[item] : got_off[item + 1]]
            assert list(cs) == sorted(set(cs))  # ascending, each once
            for e in got[got_off[item] : got_off[item + 1]]:
                for u in range(4):
                    if j0 + u < d:
                        back[i, j0 + u, e["c"]] = e["f"][u]
                    else:
                        assert e["f"][u] == w[i, d - 1, e["c"]]  # the clamp min(j0 + u, d - 1)
        assert np.array_equal(back, w + 0.0), name  # (+ 0.0: a stored -0.0 in a group of zeros is no entry)


D_CASES = [3, 4, 5, 6, 7, 16]   # j-groups of 3; 4; 4 + 1; 4 + 2; 4 + 3; four whole groups
M_CASES = [1, 6, 17, 32, 33, 64]


@pytest.mark.parametrize("m", M_CASES)
@pytest.mark.parametrize("d", D_CASES)
def test_fold_list_is_what_the_dense_kernel_picks(shim, d, m):
    rng = np.random.default_rng(1000 * d + m)
    _check_fold(shim, _sparse_core(rng, d, m, 0.3), d, m)
    _check_fold(shim, rng.standard_normal((d, d, m)) + 1j * rng.standard_normal((d, d, m)), d, m)  # dense: m entries per item


@pytest.mark.parametrize("d", D_CASES)
def test_fold_list_edge_items(shim, d):
    """an all-zero core; an all-zero item beside full ones; one non-zero c, in the clamped column only; bond state 63"""
    m = 64
    rng = np.random.default_rng(d)
    _check_fold(shim, np.zeros((d, d, m), dtype=np.complex128), d, m)
    w = rng.standard_normal((d, d, m)) + 1j * rng.standard_normal((d, d, m))
    w[1, : min(4, d), :] = 0.0  # item (i = 1, first j-group)
    _check_fold(shim, w, d, m)
    off, ent = _fold_twin(w, d, m)
    njb = (d + 3) // 4
    assert off[njb + 1] == off[njb]
    w = np.zeros((d, d, m), dtype=np.complex128)
    w[d - 1, d - 1, 63] = 2.0 - 1.0j  # last item: u = (d - 1) % 4 and every clamped u carry it
    w[0, 0, 63] = 1.0j               # a purely imaginary coefficient is non-zero
    _check_fold(shim, w, d, m)
    off, ent = _fold_twin(w, d, m)
    assert len(ent) == 2 and [c for c, _ in ent] == [63, 63]


def _gram_twin(ws, d, m, tu):
    uc = min(tu, 8)
    nch = tu // uc
    mask = np.zeros(d * d * 4 * nch, dtype=np.uint32)
    cf = np.zeros((d * d * 4 * nch, uc), dtype=np.complex128)
    for i in range(d):
        for j in range(d):
            for v in range(4):
                for ch in range(nch):
                    rec = ((i * 4 + v) * d + j) * nch + ch
                    for u in range(uc):
                        t = v + 4 * (uc * ch + u)  # the block acc[uc * ch + u] of wave v
                        x = ws[i, j, t] if t < m else 0.0
                        cf[rec, u] = x
                        if x.real != 0.0 or x.imag != 0.0:
                            mask[rec] |= np.uint32(1 << u)
    return mask, cf


def _check_gram(shim, ws, d, m, tu):
    uc, nch = min(tu, 8), tu // min(tu, 8)
    blob = _gram_blob(shim, ws, d, m, tu)
    nrec, head = shim.cl_gram_records(d, tu), shim.cl_gram_head(d, tu)
    assert nrec == d * d * 4 * nch and head % 16 == 0 and head >= 4 * nrec and len(blob) == head + nrec * uc * 16
    mask, cf = _gram_twin(ws, d, m, tu)
    got_mask = blob[: 4 * nrec].view("<u4")
    got_cf = blob[head:].view("<c16").reshape(nrec, uc)
    assert np.array_equal(got_mask, mask)
    assert np.array_equal(got_cf.view(np.float64), cf.view(np.float64))
    # expanded again: the dense core exactly, each coefficient once; the mask bits are exactly the non-zero coefficients
    back = np.zeros((d, d, m), dtype=np.complex128)
    seen = np.zeros((d, d, m), dtype=int)
    for i in range(d):
        for j in range(d):
            for v in range(4):
                for ch in range(nch):
                    rec = ((i * 4 + v) * d + j) * nch + ch
                    for u in range(uc):
                        t = v + 4 * (uc * ch + u)
                        bit = bool((got_mask[rec] >> u) & 1)
                        if t < m:
                            back[i, j, t] = got_cf[rec, u]
                            seen[i, j, t] += 1
                            assert bit == bool(ws[i, j, t] != 0.0)
                        else:
                            assert not bit and got_cf[rec, u] == 0.0
    assert np.array_equal(back.view(np.float64), np.ascontiguousarray(ws).view(np.float64)) and (seen == 1).all()


@pytest.mark.parametrize("m", M_CASES)
@pytest.mark.parametrize("d", D_CASES)
def test_gram_list_is_what_the_dense_kernel_picks(shim, d, m):
    """every instantiation that covers m blocks (4 TU >= m), the launcher's own among them"""
    rng = np.random.default_rng(2000 * d + m)
    own = shim.cl_gram_tu(m)
    assert own == (4 if m <= 16 else 8 if m <= 32 else 16)
    for tu in (4, 8, 16):
        if 4 * tu < m:
            continue
        _check_gram(shim, _sparse_core(rng, d, m, 0.3), d, m, tu)
        _check_gram(shim, rng.standard_normal((d, d, m)) + 1j * rng.standard_normal((d, d, m)), d, m, tu)


def test_gram_list_edge_records(shim):
    """an all-zero core (every mask zero: the kernel reads no slab); one non-zero coefficient; block 63 (wave 3, the last
    bit of the second chunk of <16>); a column of zeros, as ws_reuse has"""
    d, m = 5, 64
    _check_gram(shim, np.zeros((d, d, m), dtype=np.complex128), d, m, 16)
    ws = np.zeros((d, d, m), dtype=np.complex128)
    ws[2, 3, 63] = -1.5j
    _check_gram(shim, ws, d, m, 16)
    mask, _ = _gram_twin(ws, d, m, 16)
    assert np.count_nonzero(mask) == 1 and mask[((2 * 4 + 3) * d + 3) * 2 + 1] == 1 << 7
    rng = np.random.default_rng(7)
    ws = rng.standard_normal((d, d, 32)) + 1j * rng.standard_normal((d, d, 32))
    ws[:, :, 9] = 0.0
    _check_gram(shim, ws, d, 32, 8)
    mask, _ = _gram_twin(ws, d, 32, 8)
    assert all(int(mk) == (0xFF & ~(1 << 2) if v == 1 else 0xFF) for mk, v in zip(mask, [(r // d) % 4 for r in range(len(mask))]))
