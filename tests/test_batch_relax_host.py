"""CPU: the batched improved relaxation (TDVPBatch.relax, mitdvp_batch_relax, k_batch_relax) without a GPU -- the case
table of tests/helpers/relax_cases.py against the oracle (the inputs are hard enough, and the reference's own scatter is
far below the bars of the GPU tests); the two entry points declared, exported and loadable; the rule of the Krylov carve
(csrc/batch_relax_plan.h, compiled with g++ into a throw-away shim); and every refusal that needs no GPU."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _parity_cases():
    from helpers import relax_cases as rc

    return [(name, seed) for name, (_, _, seeds) in rc.PARITY.items() for seed in seeds[:3]]


# ---- the case table against the oracle ----
@pytest.mark.parametrize("name,seed", _parity_cases())
def test_parity_cases_need_more_vectors_than_the_exponential_keeps(name, seed):
    """at least one local solve of the first step with k > 21 (the exponential's carve), none above 64 (the cap)"""
    from helpers import relax_cases as rc

    dims, D, _ = rc.PARITY[name]
    _, kmax, first, _ = rc.oracle_relax("heis", dims, D, seed, 3)
    print(name, seed, "largest k per step", kmax, "first step", first)
    assert max(first) > 21
    assert max(first) <= 64
    if name == "L8d2D4":  # the edge sites have N = 4 elements and end at k = N
        assert first[0] <= 4 and first[len(dims) - 1] <= 4


@pytest.mark.parametrize("name,seed", _parity_cases())
def test_parity_cases_have_a_gap_and_the_oracle_descends(name, seed):
    from helpers import relax_cases as rc

    dims, D, _ = rc.PARITY[name]
    w = rc.dense_spectrum("heis", dims, seed)
    assert w[1] - w[0] > 0.1
    energies, _, _, _ = rc.oracle_relax("heis", dims, D, seed, 3)
    for e0, e1 in zip(energies, energies[1:]):
        assert e1 - e0 <= 1e-12 * abs(e0)
    assert energies[-1] >= w[0] - 1e-12 * abs(w[0])  # variational


@pytest.mark.parametrize("name", ["L8d2D4", "L6d3D6"])
def test_the_reference_scatters_far_less_than_the_bars(name):
    """a start perturbed by 1e-13 moves the oracle's final state by less than 1e-12 in fidelity (the GPU bar is 1e-10)"""
    from helpers import relax_cases as rc

    dims, D, seeds = rc.PARITY[name]
    e0, _, _, c0 = rc.oracle_relax("heis", dims, D, seeds[0], 3)
    e1, _, _, c1 = rc.oracle_relax("heis", dims, D, seeds[0], 3, 0.0, 1e-13)
    print(name, "fidelity defect", rc.fidelity_defect(c0, c1), "energy difference", abs(e0[-1] - e1[-1]))
    assert rc.fidelity_defect(c0, c1) < 1e-12
    assert abs(e0[-1] - e1[-1]) < 1e-10 * abs(e0[-1])


def test_the_mpo_builders_give_the_matrices_they_say():
    from helpers import relax_cases as rc

    dims = (2, 3, 2)
    H = rc.dense_from_mpo(rc.heisenberg_mpo(dims, 5))
    assert np.allclose(H, H.conj().T, atol=1e-14)
    ops = [rc.spin_ops(d) for d in dims]
    onsite = rc.heisenberg_fields(dims, 5)

    def kron_at(mats):
        out = np.ones((1, 1))
        for m in mats:
            out = np.kron(out, m)
        return out

    ref = 0
    eyes = [np.eye(d) for d in dims]
    for p in range(3):
        ref = ref + kron_at(eyes[:p] + [onsite[p]] + eyes[p + 1:])
    for p in range(2):
        (sz0, sp0, sm0, _), (sz1, sp1, sm1, _) = ops[p], ops[p + 1]
        for a, b, f in ((sp0, sm1, 0.5), (sm0, sp1, 0.5), (sz0, sz1, 1.0)):
            ref = ref + f * kron_at(eyes[:p] + [a, b] + eyes[p + 2:])
    assert np.allclose(H, ref, atol=1e-13)
    # the field-only chain in both of its MPO forms, and its ground energy
    F = rc.dense_from_mpo(rc.field_mpo(dims, 2))
    assert np.allclose(F, rc.dense_from_mpo(rc.field_mpo_wide(dims, 2)), atol=1e-13)
    assert abs(np.linalg.eigvalsh(F)[0] - rc.field_ground_energy(dims, 2)) < 1e-12
    # spin commutator [S+, S-] = 2 Sz
    for d in (2, 3, 4, 8):
        sz, sp, sm, _ = rc.spin_ops(d)
        assert np.allclose(sp @ sm - sm @ sp, 2 * sz, atol=1e-13)


def test_the_field_only_chain_exhausts_its_krylov_space():
    from helpers import relax_cases as rc

    dims, bonds = rc.FIELD
    for D in bonds:
        energies, kmax, first, _ = rc.oracle_relax("field", dims, D, 0, 2)
        print("field-only D =", D, "largest k per step", kmax)
        assert abs(energies[-1] - rc.field_ground_energy(dims, 0)) < 1e-12
        if D == 1:
            assert set(first[: len(dims)]) == {3}  # k = N at every site


def test_the_tridiagonal_table_covers_what_it_should():
    from helpers import relax_cases as rc

    rows = rc.tridiag_table()
    print(rc.tridiag_table_text())
    assert {r["k"] for r in rows} >= {1, 2, 3, 21, 63, 64}
    assert any(r["name"].startswith("L6d3D6") and r["gap"] < 1e-9 * r["norm1"] for r in rows)  # a ghost copy of the lowest Ritz value
    assert all(r["bar_theta"] >= r["k"] * rc.EPS * r["norm1"] and r["bar_res"] >= r["k"] * rc.EPS * r["norm1"] for r in rows)
    close = [r for r in rows if r["name"].startswith("close-pair")]
    assert close and all(0.5e-9 < r["gap"] / r["norm1"] < 4e-9 and r["bar_vec"] is None for r in close)
    tiny = [r for r in rows if r["name"].startswith("tiny-beta")]
    assert tiny and all(np.min(np.abs(r["beta"])) <= 1.0001e-12 * np.max(np.abs(r["alpha"])) for r in tiny)


# ---- the library ----
def test_the_entry_points_are_declared_and_bound():
    from pytdscf_amd import _lib

    header = open(os.path.join(ROOT, "include", "mitdvp.h")).read()
    assert ("int mitdvp_batch_relax(mitdvp_batch* b, int maxstep, double conv_tol, double* energies, int* steps, double* history, "
            "int* statuses);") in header
    assert ("int mitdvp_batch_trilow(int device, const double* alpha, const double* beta, const int* k, int ncases, double* theta, "
            "double* vec);") in header
    capi = open(os.path.join(ROOT, "pytdscf_amd", "csrc", "capi.hip")).read()
    for sym in ("mitdvp_batch_relax", "mitdvp_batch_trilow"):
        assert sym in _lib.declared_symbols()
        assert sym + "(" in capi
    assert "batch_relax_plan.h" in open(os.path.join(ROOT, "pytdscf_amd", "csrc", "Makefile")).read()
    lib = _lib.load()
    assert hasattr(lib, "mitdvp_batch_relax") and hasattr(lib, "mitdvp_batch_trilow")
    import pytdscf_amd
    from pytdscf_amd import TDVPBatch, engine, trajectories

    assert callable(TDVPBatch.relax) and callable(engine.tridiag_lowest) and callable(trajectories.relax_trajectories)
    assert pytdscf_amd.relax_trajectories is trajectories.relax_trajectories


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("brx_shim") / "libbrx_shim.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "helpers", "relax_plan_shim.cpp"), "-o", str(out)],
                   check=True)
    lib = C.CDLL(str(out))
    lib.brx_carve.restype = C.c_ulonglong
    lib.brx_carve.argtypes = [C.c_long, C.c_long, C.c_int, C.c_int]
    lib.brx_kcap_ok.restype = C.c_char_p
    lib.brx_kcap_ok.argtypes = [C.c_int]
    return lib


def test_the_carve_rule(shim):
    assert shim.brx_max_krylov() == 64 and shim.brx_exp_slots() == 21
    for max_site, max_bond in ((32, 16), (108, 36), (4, 16), (8192, 1024), (3, 1), (1, 1)):
        slot = max(max_site, max_bond)
        for relax in (0, 1):  # byte for byte what it was, whatever max_diag_krylov says
            for mdk in (0, 4, 64):
                assert shim.brx_carve(max_site, max_bond, relax, mdk) == 21 * slot
        assert shim.brx_carve(max_site, max_bond, 2, 0) == (min(max_site, 64) + 1) * slot
        assert shim.brx_carve(max_site, max_bond, 2, 64) == (min(max_site, 64) + 1) * slot
        assert shim.brx_carve(max_site, max_bond, 2, 4) == (min(max_site, 4) + 1) * slot
    # the parity cases need more slots than the exponential's 21
    assert shim.brx_carve(108, 36, 2, 0) == 65 * 108 > 21 * 108


def test_the_cap_of_the_krylov_space(shim):
    for ok in (0, 2, 4, 63, 64, -1):
        assert shim.brx_kcap_ok(ok) is None
    for bad in (1, 65, 3000):
        msg = shim.brx_kcap_ok(bad).decode()
        assert f"max_diag_krylov = {bad}" in msg and "2 to 64" in msg


def test_the_hook_refuses_before_the_gpu_is_touched():
    from pytdscf_amd import _lib, engine

    lib = _lib.load()
    a = np.zeros((2, 64))
    th = np.zeros(2)
    ip = C.POINTER(C.c_int)
    dp = C.POINTER(C.c_double)

    def call(ks, n, alpha=a, vec=a):
        ks = np.asarray(ks, dtype=np.int32)
        rc = lib.mitdvp_batch_trilow(0, None if alpha is None else alpha.ctypes.data_as(dp), a.ctypes.data_as(dp), ks.ctypes.data_as(ip), n,
                                     th.ctypes.data_as(dp), None if vec is None else vec.ctypes.data_as(dp))
        return rc, lib.mitdvp_last_error(None).decode()

    rc, msg = call([3, 65], 2)
    assert rc == _lib.EINVAL and "mitdvp_batch_trilow" in msg and "case 1 has k = 65" in msg and "1 .. 64" in msg
    rc, msg = call([0, 3], 2)
    assert rc == _lib.EINVAL and "case 0 has k = 0" in msg
    rc, msg = call([3, 3], 0)
    assert rc == _lib.EINVAL and "ncases = 0" in msg and "1 .. 65536" in msg
    rc, msg = call([3, 3], 2, alpha=None)
    assert rc == _lib.EINVAL and "null argument" in msg
    with pytest.raises(ValueError, match="3 diagonal and 1 off-diagonal"):
        engine.tridiag_lowest([1.0, 2.0, 3.0], [0.5])
    # mitdvp_batch_block keeps refusing op 7: the hook is an entry point of its own
    assert "mitdvp_batch_trilow" not in open(os.path.join(ROOT, "pytdscf_amd", "csrc", "batch_block_check.h")).read()


def test_relax_refuses_without_a_handle_or_with_bad_arguments():
    from pytdscf_amd import TDVPBatch, _lib

    lib = _lib.load()
    assert lib.mitdvp_batch_relax(None, 3, 0.0, None, None, None, None) == _lib.EINVAL
    assert "mitdvp_batch_relax: null handle" in lib.mitdvp_last_error(None).decode()
    bt = TDVPBatch.from_engines([object()])  # the front end's checks come before any handle is made
    with pytest.raises(ValueError, match="maxstep = 0, it must be >= 1"):
        bt.relax(0)
    with pytest.raises(ValueError, match="conv_tol = -1.0, it must be finite and >= 0"):
        bt.relax(3, -1.0)
    with pytest.raises(ValueError, match="it must be finite and >= 0"):
        bt.relax(3, float("nan"))
    bt.engines = []


def test_relax_trajectories_refuses_before_any_engine_exists():
    from pytdscf_amd import relax_trajectories

    class M:
        nstate, space, m_aux_max = 1, "hilbert", 4

        def __init__(self, dims):
            self.dims = dims

    with pytest.raises(ValueError, match="no model"):
        relax_trajectories([])
    with pytest.raises(ValueError, match="model 1 has dims"):
        relax_trajectories([M([2, 2]), M([2, 3])])
    with pytest.raises(ValueError, match="1 starts for 2 models"):
        relax_trajectories([M([2, 2]), M([2, 2])], starts=[[np.ones(2), np.ones(2)]])
    m = M([2, 2])
    m.nstate = 2
    with pytest.raises(NotImplementedError, match="one electronic state"):
        relax_trajectories(m)
