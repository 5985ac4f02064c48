"""CPU: expectation values of MPO observables of the batched trajectories -- the C surface is declared, exported and
bound; the operators of the device tests have the MPO bonds they are meant to have; the walk of k_batch_expect, restated
in NumPy, equals the dense pin on every (shape, operator) inside the bar of the device tests; and the Python side refuses a
malformed operator list or an unknown observable name before any engine exists."""

import ctypes as C
import os

import numpy as np
import pytest

NAMES = ["mitdvp_batch_set_expect", "mitdvp_batch_expect", "mitdvp_batch_expect_records"]


def test_expect_symbols_are_declared_exported_and_refuse_a_null_batch():
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
    assert lib.mitdvp_batch_set_expect(None, None, 0) == _lib.EINVAL
    assert b"mitdvp_batch_set_expect" in lib.mitdvp_last_error(None)
    assert lib.mitdvp_batch_expect(None, None, None, None, None) == _lib.EINVAL
    assert b"mitdvp_batch_expect:" in lib.mitdvp_last_error(None)
    assert lib.mitdvp_batch_expect_records(None, None, None, None, None) == _lib.EINVAL
    assert b"mitdvp_batch_expect_records" in lib.mitdvp_last_error(None)


@pytest.mark.parametrize("name", ["mixed", "odd", "wide"])
def test_the_operators_have_the_mpo_bonds_they_are_meant_to_have(name):
    from helpers import expect_cases as ec

    dims, _ = ec.SHAPES[name]
    bonds = {label: ec.max_bond(ec.case(name, label)[2]) for label in ec.LABELS}
    print(f"{name}: MPO bonds {bonds}")
    assert all(1 <= m <= ec.MAX_MPO for m in bonds.values())
    assert bonds["product"] == 1 < bonds["energy"]
    assert bonds["local"] != bonds["energy"]
    assert bonds["longrange"] > bonds["energy"]
    for label in ec.LABELS:
        cores = ec.case(name, label)[2]
        assert cores[0].shape[0] == 1 and cores[-1].shape[3] == 1
        assert [w.shape[1] for w in cores] == list(dims) == [w.shape[2] for w in cores]
    terms, shift, _ = ec.case(name, "complex")
    assert shift.imag != 0 and any(np.abs(m - m.conj().T).max() > 0.1 for _, ops in terms for m in ops.values())


@pytest.mark.parametrize("name", ["mixed", "odd", "wide"])
def test_the_twin_equals_the_dense_pin(name):
    """three random states of different norms; every operator; the defect as a fraction of the device tests' bar
    1e-12 SCALE <psi|psi>"""
    from helpers import expect_cases as ec

    worst = 0.0
    for cores in ec.random_states(name, 3, seed=21):
        n2 = ec.norm2(cores)
        for label in ec.LABELS:
            _, shift, mpo = ec.case(name, label)
            pin, twin = ec.dense_value(cores, mpo, shift), ec.walk(cores, mpo, shift)
            S = ec.scale(name, label) * n2
            assert abs(pin) <= S * (1 + 1e-12), (label, pin, S)  # SCALE bounds the value: the bar is a relative one
            worst = max(worst, abs(twin - pin) / (ec.BAR * S))
    print(f"{name}: worst |twin - dense pin| = {worst:.3e} of 1e-12 SCALE <psi|psi>")
    assert worst < 1


def test_the_pin_applies_the_operator_to_the_vector():
    """apply_mpo against the dense matrix where that is small (243 x 243), and the Hermitian operators give real values"""
    from helpers import expect_cases as ec
    from helpers import jump_oracle as jo

    cores = ec.random_states("odd", 1, seed=5)[0]
    v = jo.dense_state(cores)
    for label in ec.LABELS:
        _, shift, mpo = ec.case("odd", label)
        want = jo.dense_operator(mpo) @ v
        assert np.abs(ec.apply_mpo(mpo, v) - want).max() < 1e-12 * np.abs(want).max()
        val = ec.dense_value(cores, mpo, shift)
        if label != "complex":
            assert abs(val.imag) < 1e-12 * ec.scale("odd", label)
        else:
            assert abs(val.imag) > 1e-3


def test_operator_lists_on_the_python_side():
    from pytdscf_amd.engine import expect_ops

    assert expect_ops([1, 2, 0]) == [1, 2, 0] and expect_ops(range(1, 4)) == [1, 2, 3]
    assert expect_ops(np.arange(2)) == [0, 1] and expect_ops(3) == [3] and expect_ops([]) == []
    for bad in ([0.5], [True], ["1"], [None], [2**40], 1.5, [-1], [1, 1], list(range(65))):
        with pytest.raises(ValueError, match="expect operators"):
            expect_ops(bad)


def test_observable_names_are_checked_before_any_engine_exists(monkeypatch):
    """propagate_trajectories(observables=...) raises on a name the model does not have without constructing a batch"""
    import pytdscf_amd.trajectories as tr

    class _Model:
        dims = [2, 2]
        observables = {"dipole": object(), "bath": object()}

    def _no_batch(*a, **k):
        raise AssertionError("a batch was constructed")

    monkeypatch.setattr(tr, "TDVPBatch", _no_batch)
    assert tr.observable_names(_Model, None) == [] and tr.observable_names(_Model, True) == ["dipole", "bath"]
    assert tr.observable_names(_Model, ["bath"]) == ["bath"] and tr.observable_names(_Model, "dipole") == ["dipole"]
    with pytest.raises(ValueError, match="'current'"):
        tr.observable_names(_Model, ["dipole", "current"])
    with pytest.raises(ValueError, match="listed twice"):
        tr.observable_names(_Model, ["dipole", "dipole"])
    with pytest.raises(ValueError, match="names no observable"):
        tr.observable_names(_Model, [])
    with pytest.raises(ValueError, match="'current'"):
        tr.propagate_trajectories(_Model, [[[1, 0], [1, 0]]], 4, 0.1, ([(0, 0)], 1), observables=["current"])
