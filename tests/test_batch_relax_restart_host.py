"""CPU: thick restarts of the batched improved relaxation's local Lanczos solve (mitdvp_batch_set_relax_restarts,
bt_diag in csrc/batch_site.hip) without a GPU -- the algorithm restated in NumPy (helpers/relax_restart_oracle.py) against
the reference oracle's unrestarted solve on the cases of helpers/relax_cases.py; the range check of
csrc/batch_relax_plan.h through a g++ shim; the two entry points declared, exported and refusing a null handle.

The bars are the project's own (tests/test_gpu_batch_relax.py): fidelity defect < 1e-10, energy within 1e-8 |E|.  Restart
counts are printed, never pinned: the solver stops on rounding-level quantities once a site has converged."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

FID, ENE = 1e-10, 1e-8
SETTINGS = [(4, 64), (8, 32), (16, 8)]  # (max_diag_krylov, max_restarts)
MOTIVE = ((4,) * 10, 16, 3)             # dims, D, seed: the oracle's first step has a local solve of more than 64 vectors


def _parity_cases():
    from helpers import relax_cases as rc

    return [(name, seed, kcap, nr) for name in ("L6d3D6", "L8d2D4") for seed in rc.PARITY[name][2][:3] for kcap, nr in SETTINGS]


# ---- 1. the model against the reference oracle ----
@pytest.mark.parametrize("name,seed,kcap,max_restarts", _parity_cases())
def test_the_restarted_solve_reaches_the_oracles_states(name, seed, kcap, max_restarts):
    from helpers import relax_cases as rc
    from helpers import relax_restart_oracle as rro

    dims, D, _ = rc.PARITY[name]
    energies, kmax, _, cores = rc.oracle_relax("heis", dims, D, seed, 3)
    m = rro.model_relax("heis", dims, D, seed, 3, kcap, max_restarts)
    fid = rc.fidelity_defect(cores, m["cores"])
    de = abs(m["energies"][-1] - energies[-1]) / abs(energies[-1])
    print(f"{name} seed {seed} kcap {kcap}: fidelity defect {fid:.2e}, |dE/E| {de:.2e}, restarts {m['total']}, most per step {m['most']}, "
          f"applies {m['applies']}, oracle largest k per step {kmax}")
    assert fid < FID
    assert de < ENE
    if kcap in (4, 8):
        assert m["total"] > 0
    assert max(m["most"]) <= max_restarts


# ---- 2. full bonds: exact after the first step ----
@pytest.mark.parametrize("seed", [0, 1])
def test_full_bond_chains_hit_the_dense_ground_energy_after_every_step(seed):
    from helpers import relax_cases as rc
    from helpers import relax_restart_oracle as rro

    dims, D = rc.FULL_BOND
    e0 = rc.dense_spectrum("heis", dims, seed)[0]
    m = rro.model_relax("heis", dims, D, seed, 4, 6, 200)
    print(f"seed {seed}: |E - E0| per step {[abs(e - e0) for e in m['energies']]}, most restarts per step {m['most']}")
    for e in m["energies"]:
        assert abs(e - e0) < 1e-10
    assert m["total"] > 0


# ---- 3. the motivating case ----
def test_the_default_cap_fails_where_one_restart_succeeds():
    from helpers import relax_cases as rc
    from helpers import relax_restart_oracle as rro

    dims, D, seed = MOTIVE
    energies, kmax, first, cores = rc.oracle_relax("heis", dims, D, seed, 1)
    print("oracle: largest k of the first step", kmax[0])
    assert kmax[0] > 64
    m = rro.model_relax("heis", dims, D, seed, 1, 64, 4)
    fid = rc.fidelity_defect(cores, m["cores"])
    de = abs(m["energies"][-1] - energies[-1]) / abs(energies[-1])
    print(f"model, 64 vectors and up to 4 restarts: restarts {m['total']}, fidelity defect {fid:.2e}, |dE/E| {de:.2e}")
    assert m["total"] >= 1 and max(m["most"]) <= 4
    assert fid < FID and de < ENE
    with pytest.raises(ValueError, match="Lanczos Diagonalization is not converged in 64 basis$"):
        rro.model_relax("heis", dims, D, seed, 1, 64, 0)


# ---- 4. exhaustion ----
def _mixed(r, max_restarts):
    """the replicas of test_easy_replicas_finish_next_to_ones_that_do_not_converge: dims (3,) * 5, D = 4, 4 vectors"""
    from helpers import relax_restart_oracle as rro

    dims, D = (3,) * 5, 4
    if r % 2 == 0:
        return rro.model_relax("field_wide", dims, D, r, 2, 4, max_restarts, "product")
    return rro.model_relax("heis", dims, D, r, 2, 4, max_restarts)


def test_restarts_run_out_for_the_hard_replicas_only():
    from helpers import relax_cases as rc

    dims = (3,) * 5
    for r in (1, 3):
        with pytest.raises(ValueError, match="Lanczos Diagonalization is not converged in 4 basis after 2 restarts$"):
            _mixed(r, 2)
    for r in (0, 2):
        m = _mixed(r, 2)
        assert m["total"] == 0
        assert abs(m["energies"][-1] - rc.field_ground_energy(dims, r)) < 1e-12
    for r in range(4):
        m = _mixed(r, 64)
        print(f"replica {r}: restarts {m['total']}, most per step {m['most']}")
        assert max(m["most"]) <= 64
        if r % 2:
            assert m["total"] > 0


# ---- 5. the range of the setting ----
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("brr_shim") / "libbrr_shim.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "helpers", "relax_restart_shim.cpp"), "-o", str(out)],
                   check=True)
    lib = C.CDLL(str(out))
    lib.brr_restarts_ok.restype = C.c_char_p
    lib.brr_restarts_ok.argtypes = [C.c_int]
    return lib


def test_the_range_of_max_restarts(shim):
    assert shim.brr_max_restarts() == 4096
    for ok in (0, 1, 4096):
        assert shim.brr_restarts_ok(ok) is None
    for bad in (-1, 4097):
        msg = shim.brr_restarts_ok(bad).decode()
        assert f"max_restarts = {bad}" in msg and "0 to 4096" in msg


# ---- 6. the library ----
def test_the_entry_points_are_declared_exported_and_refuse_a_null_handle():
    from pytdscf_amd import TDVPBatch, _lib

    header = open(os.path.join(ROOT, "include", "mitdvp.h")).read()
    assert "int mitdvp_batch_set_relax_restarts(mitdvp_batch* b, int max_restarts);" in header
    assert "int mitdvp_batch_relax_restarts(mitdvp_batch* b, long long* total, int* most);" in header
    for sym in ("mitdvp_batch_set_relax_restarts", "mitdvp_batch_relax_restarts"):
        assert sym in _lib.declared_symbols()
    lib = _lib.load()
    assert lib.mitdvp_batch_set_relax_restarts(None, 4) == _lib.EINVAL
    assert "mitdvp_batch_set_relax_restarts: null handle" in lib.mitdvp_last_error(None).decode()
    assert lib.mitdvp_batch_relax_restarts(None, None, None) == _lib.EINVAL
    assert "mitdvp_batch_relax_restarts: null handle" in lib.mitdvp_last_error(None).decode()
    assert callable(TDVPBatch.set_relax_restarts) and callable(TDVPBatch.relax_restarts)
