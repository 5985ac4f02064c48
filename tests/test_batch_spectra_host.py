"""CPU: bond spectra and entanglement entropies of the batched trajectories -- the C surface is declared, exported and
loads; the walk of k_batch_spectra, restated in NumPy, gives the squared singular values of the dense state at every
bond; the entropy bar of the device tests is derived and holds on perturbed spectra; the bar of the dynamics case holds
for the NumPy oracle against dense expm with a factor to spare; and the Python side's handling of a bond list."""

import ctypes as C
import os

import numpy as np
import pytest

NAMES = ["mitdvp_batch_set_spectra", "mitdvp_batch_spectra", "mitdvp_batch_spectra_records"]


def test_spectra_symbols_are_declared_exported_and_refuse_a_null_batch():
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
    assert lib.mitdvp_batch_set_spectra(None, None, 0) == _lib.EINVAL
    assert b"mitdvp_batch_set_spectra" in lib.mitdvp_last_error(None)
    assert lib.mitdvp_batch_spectra(None, None, None, None, None) == _lib.EINVAL
    assert b"mitdvp_batch_spectra:" in lib.mitdvp_last_error(None)
    assert lib.mitdvp_batch_spectra_records(None, None, None, None, None) == _lib.EINVAL
    assert b"mitdvp_batch_spectra_records" in lib.mitdvp_last_error(None)


@pytest.mark.parametrize("name", ["mixed", "odd", "wide"])
def test_the_walk_gives_the_dense_singular_values(name):
    """every bond of the three device shapes, to 1e-13 |psi|^2; the smallest compared weight is above 1e-13 W, so no two
    zeros are compared; W is the squared norm and the weights come out in descending order"""
    from helpers import spectra_cases as sc

    dims, D = sc.SHAPES[name]
    cores = sc.random_states(dims, D, 2, seed=21)[1]
    L = len(dims)
    recs = sc.walk(cores, range(L - 1))
    assert [len(r) - sc.HEAD for r in recs] == [c.shape[2] for c in cores[:-1]]
    assert max(len(r) for r in recs) - sc.HEAD == D
    worst, least = 0.0, 1.0
    for q, r in enumerate(recs):
        want = sc.dense_weights(cores, q)
        W = want.sum()
        assert abs(W - 0.81) < 1e-12 and abs(r[0] - W) < 1e-13 * W
        got = r[sc.HEAD:]
        assert np.all(np.diff(got) <= 0)
        worst = max(worst, np.abs(got - want).max() / W)
        least = min(least, want.min() / W, got.min() / W)
        assert np.abs(r[1:sc.HEAD] - sc.entropies(want)).max() < sc.entropy_bar(len(want), 1e-13)
    print(f"{name}: worst |walk - dense| = {worst:.2e} W, smallest compared weight {least:.2e} W")
    assert worst < 1e-13 and least > 1e-13
    sub = sc.walk(cores, [1, L - 3])  # a sub-list that stops before the last bond: the same walk, cut short
    assert np.array_equal(sub[0], recs[1]) and np.array_equal(sub[1], recs[L - 3])


def test_the_record_rule_on_ties_zeros_and_known_spectra():
    from helpers import spectra_cases as sc

    r = sc.record([0.5, 0.0, 0.5, 0.0])
    assert np.array_equal(r[sc.HEAD:], [0.5, 0.5, 0.0, 0.0]) and r[0] == 1.0 and r[3] == 0.0
    assert abs(r[1] - np.log(2)) < 1e-15 and abs(r[2] - np.log(2)) < 1e-15
    assert np.array_equal(sc.record([0.0, 0.0]), np.zeros(6))  # W == 0: zeros, no NaN
    r = sc.record([0.1, 0.7, 0.2])
    assert np.array_equal(r[sc.HEAD:], [0.7, 0.2, 0.1]) and abs(r[3] - 0.1) < 1e-16
    # the Bell chain and the padded product, through the walk
    from oracle import tdvp_oracle as orc

    recs = sc.walk(orc.canonicalize_site0(sc.bell_chain(), scale=None), range(5))
    for q, rr in enumerate(recs):
        assert abs(rr[0] - 1) < 1e-14 and abs(rr[1] - (np.log(2) if q % 2 == 0 else 0.0)) < 1e-14, (q, rr)
    recs = sc.walk(orc.canonicalize_site0(sc.product_padded((2, 3, 2, 4, 2), 6), scale=None), range(4))
    for rr in recs:
        assert abs(rr[sc.HEAD] - rr[0]) < 1e-14 * rr[0] and np.all(rr[sc.HEAD + 1:] < 1e-28 * rr[0]) and rr[1] < 1e-10


@pytest.mark.parametrize("chi", [2, 7, 40, 64])
def test_the_entropy_bar_is_derived_and_holds_on_perturbed_spectra(chi):
    """weights within delta = 1e-12 of p: |dS1| <= chi delta (1 + |ln delta|), 1.8e-9 at chi = 64.  Flat, steep and
    rank-deficient spectra, the perturbation with every sign pattern that keeps the weights non-negative."""
    from helpers import spectra_cases as sc

    delta = 1e-12
    bar = sc.entropy_bar(chi, delta)
    if chi == 64:
        assert 1.7e-9 < bar < 1.9e-9
    rng = np.random.default_rng(chi)
    worst = 0.0
    spectra = [np.full(chi, 1.0 / chi), np.exp(-3.0 * np.arange(chi)), np.r_[1.0, np.zeros(chi - 1)], rng.random(chi) ** 8]
    for p in spectra:
        p = p / p.sum()
        for _ in range(8):
            q = np.maximum(p + delta * rng.choice([-1.0, 1.0], chi) * rng.random(chi) ** 0.25, 0.0)  # mostly near +-delta
            assert np.abs(q - p).max() <= delta
            s_p = -sum(x * np.log(x) for x in p if x > 0)  # the bound's own quantity: the weights as they are
            s_q = -sum(x * np.log(x) for x in q if x > 0)
            worst = max(worst, abs(s_q - s_p) / bar)
            assert abs(s_q - s_p) <= bar
            # the model's S1, S2 and pmin: it normalises by its own W, so the amplitude is cut until the NORMALISED
            # weights are within delta
            a = delta / (2.0 * (1.0 + chi * p.max()))
            q = np.maximum(p + a * rng.uniform(-1, 1, chi), 0.0) * rng.uniform(0.5, 2.0)  # any norm
            assert np.abs(q / q.sum() - p).max() <= delta
            got, ref = sc.entropies(q), sc.entropies(p)
            worst = max(worst, np.abs(got - ref).max() / bar)
            assert np.abs(got - ref).max() <= bar
    print(f"chi = {chi}: worst entropy change {worst:.3f} of the bar {bar:.2e}")


def test_the_dynamics_bar_holds_for_the_oracle_with_a_factor_to_spare():
    """L = 6 spin chain at full bond dimension, Arnoldi at thresh 1e-10, 4 steps of 0.3: the oracle's entropies through
    the walk model against dense expm.  The bar (spectra_cases.dyn_bar) is 8 delta (1 + |ln delta|) with delta =
    2 * 4 * 2 * 11 * 1e-10 = 1.8e-8: 2.7e-6; it must hold with a factor of at least 3 before the device is asked."""
    from helpers import spectra_cases as sc

    bar = sc.dyn_bar()
    assert 2.5e-6 < bar < 3e-6
    dense, oracle = sc.dyn_dense(), sc.dyn_oracle()
    assert dense.shape == oracle.shape == (sc.DYN_STEPS + 1, sc.DYN_L - 1)
    dev = np.abs(oracle - dense).max()
    move = np.abs(dense - dense[0]).max()
    print(f"oracle vs dense expm: {dev:.2e} = {dev / bar:.2e} of the bar {bar:.2e}; the entropies move by {move:.3f}")
    assert 3 * dev < bar
    assert move > 0.01  # the entropies are not constants of this motion


def test_bond_lists_on_the_python_side():
    from pytdscf_amd.engine import spectra_bonds

    assert spectra_bonds([0, 2, 3], 5) == [0, 2, 3] and spectra_bonds(range(3), 5) == [0, 1, 2]
    assert spectra_bonds(np.arange(2), 5) == [0, 1] and spectra_bonds(2, 5) == [2] and spectra_bonds([], 5) == []
    assert spectra_bonds([7, -1, 1, 1], 5) == [7, -1, 1, 1]  # range and order are the library's to refuse, with its message
    for bad in ([0.5], [True], ["1"], [None], [2**40], 1.5):
        with pytest.raises(ValueError, match="spectra bonds"):
            spectra_bonds(bad, 5)
