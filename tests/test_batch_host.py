"""CPU: the C surface of the batched trajectories (mitdvp_batch_*) is declared, documented and exported, and the Python
class refuses an empty batch before it touches the GPU."""

import ctypes as C
import os

import pytest

NAMES = ["mitdvp_batch_create", "mitdvp_batch_step", "mitdvp_batch_sweep", "mitdvp_batch_destroy"]


def test_batch_symbols_are_declared_in_the_header_and_the_binding():
    from pytdscf_amd import _lib

    declared = _lib.declared_symbols()
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    with open(os.path.join(os.path.dirname(_lib.__file__), "_lib.py")) as f:
        binding = f.read()
    for n in NAMES:
        assert n in declared and n in header
        assert f'"{n}"' in binding
    assert "typedef struct mitdvp_batch mitdvp_batch;" in header


def test_built_library_exports_the_batch_symbols():
    from pytdscf_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
    _lib.load()  # sets every declared signature: AttributeError if one is missing


def test_empty_batch_is_refused_before_the_gpu_is_touched():
    from pytdscf_amd import TDVPBatch

    with pytest.raises(ValueError):
        TDVPBatch(0, 4)
    with pytest.raises(ValueError):
        TDVPBatch.from_engines([])
