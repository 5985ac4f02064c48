"""CPU: excited states of the batched improved relaxation by deflation against stored states (mitdvp_batch_deflate_*,
k_batch_relax_defl in csrc/batch_site.hip) without a GPU -- the method restated in NumPy (helpers/deflate_oracle.py) against
the dense spectrum of the disordered Heisenberg chains of helpers/relax_cases.py; the host arithmetic of
csrc/batch_deflate_plan.h through a g++ shim; the four entry points declared, exported and refusing a null handle.

The bars of test 1 are those of the issue that introduced the feature: |E_k - dense E_k| < 1e-10, mutual overlaps < 1e-10,
fewer than 64 vectors in every local solve (measured on these inputs: 2e-14, 8e-14, k <= 45)."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _full_cases():
    from helpers import deflate_oracle as do

    return do.full_cases()


# ---- 1. the model against the dense spectrum ----
@pytest.mark.parametrize("dims,D,seed", _full_cases())
def test_four_states_of_a_full_bond_chain_match_the_dense_spectrum(dims, D, seed):
    from helpers import deflate_oracle as do
    from helpers import relax_cases as rc

    r = do.heis_states(dims, D, seed)
    exact = rc.dense_spectrum("heis", dims, seed)[: do.NSTATES]
    de = np.abs(r["energies"] - exact)
    ov = np.abs(r["overlaps"] - np.eye(do.NSTATES))
    print(f"{dims} D {D} seed {seed}: |E_k - dense| {de}, largest mutual overlap {ov.max():.2e}, largest k {r['kmax']}")
    assert np.all(de < 1e-10)
    assert ov.max() < 1e-10
    assert r["kmax"] < 64
    # E_n of the kernel's convention: the lowest Ritz value at site 0 is the energy plus the penalties, which vanish here
    assert np.all(np.abs(r["ritz"] - r["energies"]) < 1e-10)


# ---- 2. a weight below the gap ----
def test_a_weight_below_the_gap_falls_back_onto_the_ground_state():
    from helpers import deflate_oracle as do
    from helpers import relax_cases as rc

    dims, D, seed = do.SMALL_GAP
    exact = rc.dense_spectrum("heis", dims, seed)
    gap = exact[1] - exact[0]
    assert abs(gap - 0.508) < 1e-3
    weak = do.run_states(rc.heisenberg_mpo(dims, seed), dims, D, seed, nstates=2, nsteps=2, weight=0.01)
    good = do.heis_states(dims, D, seed)
    print(f"gap {gap:.3f}: weight 0.01 gives E {weak['energies']}, |<0|1>| {abs(weak['overlaps'][0, 1]):.3f}; weight 4 gives "
          f"{good['energies'][:2]}")
    assert abs(weak["energies"][1] - exact[0]) < 1e-3  # the penalty 0.01 |<0|1>|^2 is all that keeps it from E_0
    assert abs(weak["overlaps"][0, 1]) > 0.99
    assert abs(good["energies"][1] - exact[1]) < 1e-10


# ---- 3. the stored state itself is no start ----
def test_a_start_on_the_stored_state_stops_at_once_with_the_energy_plus_the_weight():
    from helpers import deflate_oracle as do
    from helpers import relax_cases as rc

    dims, D, seed = do.SMALL_GAP
    r = do.heis_states(dims, D, seed)
    ground = r["cores"][0]
    m = do.DeflatedRelax(ground, rc.heisenberg_mpo(dims, seed), [(ground, do.WEIGHT)])
    k, theta = m.solve(0)
    print(f"k {k}, Ritz value {theta}, E_0 + w {r['energies'][0] + do.WEIGHT}")
    assert k == 1
    assert abs(theta - (r["energies"][0] + do.WEIGHT)) < 1e-10


# ---- 4. the host arithmetic ----
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("bdp_shim") / "libbdp_shim.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "helpers", "deflate_plan_shim.cpp"), "-o", str(out)],
                   check=True)
    lib = C.CDLL(str(out))
    ip, dp, ull = C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_ulonglong
    lib.bdp_max_bytes.restype = ull
    lib.bdp_room.restype = C.c_char_p
    lib.bdp_room.argtypes = [C.c_int]
    lib.bdp_weights_ok.restype = C.c_char_p
    lib.bdp_weights_ok.argtypes = [dp, C.c_int]
    lib.bdp_plan.restype = None
    lib.bdp_plan.argtypes = [ip, ip, ip, C.c_int, C.c_int, C.POINTER(ull)]
    lib.bdp_fits.restype = C.c_char_p
    lib.bdp_fits.argtypes = [ip, ip, ip, C.c_int, C.c_int, ull]
    return lib


def _shape_args(dims, D):
    from oracle import tdvp_oracle as orc

    bd = orc.bond_dims(list(dims), D)
    L = len(dims)
    arr = lambda v: (C.c_int * L)(*v)  # noqa: E731
    return bd, arr([b[0] for b in bd]), arr(list(dims)), arr([b[1] for b in bd]), L


@pytest.mark.parametrize("dims,D", [((2,) * 4, 4), ((2, 3, 2, 3, 2), 12), ((2,) * 8, 4), ((4,) * 10, 32)])
@pytest.mark.parametrize("slots", [1, 3, 8])
def test_the_work_buffer_of_a_replica(shim, dims, D, slots):
    bd, dl, d, dr, L = _shape_args(dims, D)
    out = (C.c_ulonglong * 4)()
    shim.bdp_plan(dl, d, dr, L, slots, out)
    blk = sum(a * a for a, _ in bd)
    nmax = max(a * dd * b for (a, b), dd in zip(bd, dims))
    assert list(out) == [blk, nmax, slots * blk, slots * (blk + nmax)]


def test_the_set_takes_eight_states(shim):
    assert shim.bdp_max_deflate() == 8
    for count in range(8):
        assert shim.bdp_room(count) is None
    msg = shim.bdp_room(8).decode()
    assert "holds 8 states" in msg and "at most 8" in msg


def test_weights_must_be_finite_and_positive(shim):
    ok = (C.c_double * 3)(4.0, 0.01, 1e300)
    assert shim.bdp_weights_ok(ok, 3) is None
    assert "weights is NULL" in shim.bdp_weights_ok(None, 3).decode()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        w = (C.c_double * 3)(4.0, 4.0, bad)
        msg = shim.bdp_weights_ok(w, 3).decode()
        assert "replica 2" in msg and "finite and > 0" in msg


def test_a_work_buffer_above_4_GiB_is_refused_with_both_figures(shim):
    assert shim.bdp_max_bytes() == 1 << 32
    dims, D = (4,) * 10, 32
    bd, dl, d, dr, L = _shape_args(dims, D)
    per1 = sum(a * a for a, _ in bd) + max(a * dd * b for (a, b), dd in zip(bd, dims))
    nrep = 16384
    fit = (1 << 32) // (16 * per1 * nrep)
    assert 1 <= fit < 8
    for slots in range(1, fit + 1):
        assert shim.bdp_fits(dl, d, dr, L, slots, nrep) is None
    msg = shim.bdp_fits(dl, d, dr, L, fit + 1, nrep).decode()
    assert str(16 * per1 * nrep * (fit + 1)) in msg and str(1 << 32) in msg and f"at most {fit} states fit" in msg
    assert shim.bdp_fits(dl, d, dr, L, 8, 128) is None


# ---- 5. the library ----
def test_the_entry_points_are_declared_exported_and_refuse_a_null_handle():
    from pytdscf_amd import TDVPBatch, _lib

    header = open(os.path.join(ROOT, "include", "mitdvp.h")).read()
    assert "int mitdvp_batch_deflate_push(mitdvp_batch* b, const double* weights);" in header
    assert "int mitdvp_batch_deflate_clear(mitdvp_batch* b);" in header
    assert "int mitdvp_batch_deflate_count(mitdvp_batch* b, int* count);" in header
    assert "int mitdvp_batch_deflate_overlaps(mitdvp_batch* b, double* reim);" in header
    lib = _lib.load()
    w = (C.c_double * 1)(4.0)
    cnt = C.c_int(0)
    calls = {
        "mitdvp_batch_deflate_push": lambda: lib.mitdvp_batch_deflate_push(None, w),
        "mitdvp_batch_deflate_clear": lambda: lib.mitdvp_batch_deflate_clear(None),
        "mitdvp_batch_deflate_count": lambda: lib.mitdvp_batch_deflate_count(None, C.byref(cnt)),
        "mitdvp_batch_deflate_overlaps": lambda: lib.mitdvp_batch_deflate_overlaps(None, None),
    }
    for sym, call in calls.items():
        assert sym in _lib.declared_symbols()
        assert hasattr(C.CDLL(_lib.LIB_PATH), sym)
        assert call() == _lib.EINVAL
        assert f"{sym}: null handle" in lib.mitdvp_last_error(None).decode()
    for name in ("deflate_push", "deflate_clear", "deflate_count", "deflate_overlaps"):
        assert callable(getattr(TDVPBatch, name))
    with open(os.path.join(ROOT, "pytdscf_amd", "csrc", "Makefile")) as f:
        assert "batch_deflate_plan.h" in f.read()
