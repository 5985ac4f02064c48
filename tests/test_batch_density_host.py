"""CPU: multi-site reduced densities of the batched trajectories -- the two entry points are declared, exported and
mirrored; the Python surface (TDVPBatch.densities, the key parser); and the yardstick of the GPU physics test: the NumPy
oracle's reduced_density on the four spin-bath starts against the dense solution traced to the key."""

import ctypes as C
import inspect
import os

import numpy as np
import pytest

NAMES = {"mitdvp_batch_observe_keys": 11, "mitdvp_batch_run_keys": 15}


def test_the_two_entry_points_are_declared_exported_and_mirrored():
    from pytdscf_amd import _lib

    declared = _lib.declared_symbols()
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    with open(os.path.join(os.path.dirname(_lib.__file__), "_lib.py")) as f:
        binding = f.read()
    for n in NAMES:
        assert n in declared and n in header
        assert f'"{n}"' in binding
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
    lib = _lib.load()
    for n, nargs in NAMES.items():
        assert len(getattr(lib, n).argtypes) == nargs, n
    # the pinned neighbours keep their signatures
    assert len(lib.mitdvp_batch_observe.argtypes) == 7 and len(lib.mitdvp_batch_run.argtypes) == 11
    assert C.sizeof(_lib.BatchOut) == 8 * C.sizeof(C.c_void_p)
    cnt = (C.c_size_t * 4)()
    legs = (C.c_int * 2)(1, 1)
    assert lib.mitdvp_batch_observe_keys(None, None, 0, legs, 1, 0, None, None, None, None, cnt) == _lib.EINVAL
    assert lib.mitdvp_batch_run_keys(None, 0.1, 1, 1, None, 0, legs, 1, 0, None, None, None, None, cnt, None) == _lib.EINVAL
    assert _lib.MAX_DENSITY_KEYS == 64


def test_the_python_surface():
    from pytdscf_amd import TDVPBatch, propagate_trajectories

    assert list(inspect.signature(TDVPBatch.densities).parameters) == ["self", "keys", "weights", "per_replica"]
    sig = inspect.signature(TDVPBatch.densities)
    assert sig.parameters["weights"].default is None and sig.parameters["per_replica"].default is True
    # observe keeps its exact parameter list
    assert [(n, q.default) for n, q in inspect.signature(TDVPBatch.observe).parameters.items()][1:] == [
        ("sites", ()), ("norm", True), ("autocorr", False), ("energy", False), ("weights", None), ("per_replica", True)]
    p = inspect.signature(propagate_trajectories).parameters
    assert "densities" in p and p["densities"].default is None


def test_key_parsing():
    from pytdscf_amd.engine import density_key_legs

    assert density_key_legs((0, 0, 2, 2), 3) == [2, 0, 2]
    assert density_key_legs((0, 1), 2) == [1, 1]
    assert density_key_legs((1, 2, 2), 4) == [0, 1, 2, 0]
    assert density_key_legs([3], 4) == [0, 0, 0, 1]
    for bad, nsite in (((2, 1), 3), ((1, 1, 1), 3), ((), 3), ((0, 3), 3), ((-1, 0), 3), ((0, 0, 1, 0), 3)):
        with pytest.raises(ValueError) as err:
            density_key_legs(bad, nsite)
        assert str(tuple(bad)) in str(err.value), (bad, str(err.value))


class _Stop(Exception):
    pass


def test_propagate_trajectories_checks_the_keys_before_any_engine_is_created(monkeypatch):
    from helpers import spin_bath as sb
    from pytdscf_amd import Exciton, Model
    from pytdscf_amd import trajectories as tr

    def no_engine(*a, **k):
        raise _Stop("an engine was created")

    monkeypatch.setattr(tr, "TDVPBatch", no_engine)
    case = sb.case_trajectories()
    m = Model([Exciton(nstate=d) for d in case["dims"]], operators={"hamiltonian": case["mpo"]}, bond_dim=64)
    args = dict(maxstep=3, stepsize=0.1)
    for bad in ((2, 1), (1, 1, 1), (), (0, 3)):
        with pytest.raises(ValueError) as err:
            tr.propagate_trajectories(m, case["starts"], reduced_density=([], 1), densities=[(0, 0, 1, 1), bad], **args)
        assert str(tuple(bad)) in str(err.value)
    # reduced_density keeps taking one-site keys only, and names a key unless densities does
    with pytest.raises(ValueError, match=r"one-site keys \(s, s\) only"):
        tr.propagate_trajectories(m, case["starts"], reduced_density=([(0, 0, 1, 1)], 1), densities=[(0, 1)], **args)
    with pytest.raises(ValueError, match="names no key"):
        tr.propagate_trajectories(m, case["starts"], reduced_density=([], 1), **args)
    with pytest.raises(ValueError, match="names no key"):
        tr.propagate_trajectories(m, case["starts"], reduced_density=([], 1), densities=[], **args)
    with pytest.raises(_Stop):  # accepted: reaches the engine
        tr.propagate_trajectories(m, case["starts"], reduced_density=([], 1), densities=[(0, 0, 2, 2), (0, 2)], **args)


KEYS = [(0, 0, 1, 1), (0, 0, 2, 2), (0, 2), (0, 1, 1)]


def test_the_oracle_against_the_dense_solution_traced_to_the_key():
    """The yardstick of test_gpu_batch_density.py's physics test: oracle.tdvp_oracle.reduced_density on the four spin-bath
    starts, averaged, against the dense propagator traced to the key.  First record exact, last record 3.6e-12 / 3.9e-12 /
    5.7e-13 / 1.9e-12 for the four keys (the integrator's error: Krylov threshold 1e-9 on the local problems)."""
    from helpers import key_density as kd
    from helpers import spin_bath as sb
    from oracle import tdvp_oracle as orc
    from pytdscf_amd.mps import product_state_cores

    case = sb.case_trajectories()
    L = len(case["dims"])
    exact = kd.exact_trajectory_densities(KEYS)
    acc = {k: 0 for k in KEYS}
    for start in case["starts"]:
        st = orc.OracleMPS(orc.canonicalize_site0(product_state_cores(start, 64, space="hilbert"), scale=1.0), case["mpo"],
                           integrator="arnoldi", conserve_norm=False)
        rows = {k: [] for k in KEYS}
        for _ in range(sb.NSTEPS):
            for k in KEYS:
                rows[k].append(orc.reduced_density(st.cores, kd.legs_of(k, L)))
            st.propagate(sb.DT)
        for k in KEYS:
            acc[k] = acc[k] + np.array(rows[k]) / len(case["starts"])
    for k in KEYS:
        assert acc[k].shape == exact[k].shape
        e0, e1 = np.abs(acc[k][0] - exact[k][0]).max(), np.abs(acc[k][-1] - exact[k][-1]).max()
        print(f"oracle key {k}: max |mean density - dense| first {e0:.2e} last {e1:.2e}")
        assert e0 < 1e-11 and e1 < 1e-11
    # the traced dense solution agrees with the one-site yardstick the other trajectory tests use
    one = kd.exact_trajectory_densities([(1, 1)])[(1, 1)]
    assert np.abs(one - sb.exact_rdms(**case["exact"])).max() < 1e-13
