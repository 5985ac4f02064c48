"""CPU: the C surface of the batched observables (mitdvp_batch_observe / mitdvp_batch_run) is declared, documented and
exported, its ctypes signatures load, and the Python front end refuses what it cannot take before it touches the GPU."""

import ctypes as C
import os

import pytest

NAMES = ["mitdvp_batch_observe", "mitdvp_batch_run"]


def test_observe_symbols_are_declared_in_the_header_and_the_binding():
    from pytdscf_amd import _lib

    declared = _lib.declared_symbols()
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    with open(os.path.join(os.path.dirname(_lib.__file__), "_lib.py")) as f:
        binding = f.read()
    for n in NAMES:
        assert n in declared and n in header
        assert f'"{n}"' in binding
    assert "typedef struct mitdvp_batch_out {" in header
    for bit, value in (("NORM", 1), ("AUTOCORR", 2), ("ENERGY", 4), ("RDM", 8)):
        assert f"#define MITDVP_OBS_{bit} {value}" in header
        assert getattr(_lib, f"OBS_{bit}") == value


def test_built_library_exports_the_observe_symbols_and_the_signatures_load():
    from pytdscf_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
    lib = _lib.load()  # sets every declared signature: AttributeError if one is missing
    assert len(lib.mitdvp_batch_observe.argtypes) == 7
    assert len(lib.mitdvp_batch_run.argtypes) == 11
    # the struct mirrors mitdvp_batch_out: eight pointers, per-replica outputs first
    assert [k for k, _ in _lib.BatchOut._fields_] == ["norm", "autocorr", "energy", "rdm", "mean_norm2", "mean_autocorr",
                                                      "mean_energy", "mean_rdm"]
    assert C.sizeof(_lib.BatchOut) == 8 * C.sizeof(C.c_void_p)
    # a null handle is refused, not dereferenced
    assert lib.mitdvp_batch_observe(None, None, 0, 1, None, None, None) == _lib.EINVAL
    assert lib.mitdvp_batch_run(None, 0.1, 2, 1, None, 0, 1, None, None, None, None) == _lib.EINVAL


def test_the_python_surface_exists():
    import inspect

    import pytdscf_amd as P

    assert "propagate_trajectories" in P.__all__
    sig = inspect.signature(P.TDVPBatch.observe)
    assert list(sig.parameters)[1:] == ["sites", "norm", "autocorr", "energy", "weights", "per_replica"]
    sig = inspect.signature(P.TDVPBatch.propagate)
    assert list(sig.parameters)[1:] == ["dt_au", "nsteps", "observe", "every"]
    assert sig.parameters["observe"].default is None and sig.parameters["every"].default == 1
    with open(os.path.join(os.path.dirname(P.__file__), "trajectories.py")) as f:
        assert "oracle" not in f.read()


def test_the_front_end_takes_one_site_keys_only():
    from pytdscf_amd import Exciton, Model, propagate_trajectories
    from pytdscf_amd import synthetic as syn

    dims = [2, 2, 2]
    model = Model([Exciton(nstate=d) for d in dims], operators={"hamiltonian": syn.synthetic_mpo(3, 2, 3, seed=0)}, bond_dim=4)
    starts = [[[1, 0], [1, 0], [0, 1]]]
    with pytest.raises(ValueError, match=r"\(0, 1\)"):
        propagate_trajectories(model, starts, maxstep=2, stepsize=0.1, reduced_density=([(1, 1), (0, 1)], 1))
    with pytest.raises(ValueError, match=r"\(1,\)"):
        propagate_trajectories(model, starts, maxstep=2, stepsize=0.1, reduced_density=([(1,)], 1))
