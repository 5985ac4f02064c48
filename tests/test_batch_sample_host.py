"""CPU: sampled configurations of the batched trajectories -- the C surface is declared, exported and loads; the
counter-based uniform; the NumPy twin of k_batch_sample (helpers/sample_cases.py) against the dense probabilities; its fast
form against its shot-by-shot form; the selection rule on its edges; and, from the twin alone, what the device tests rely
on: the margins of every decision of their inputs and the statistical case's bars."""

import ctypes as C
import os

import numpy as np
import pytest

NAMES = ["mitdvp_batch_set_samples", "mitdvp_batch_samples", "mitdvp_batch_samples_records"]


def test_sample_symbols_are_declared_exported_and_refuse_a_null_batch():
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
    assert lib.mitdvp_batch_set_samples(None, 0, 0) == _lib.EINVAL
    assert b"mitdvp_batch_set_samples" in lib.mitdvp_last_error(None)
    assert lib.mitdvp_batch_samples(None, None, None, None, None, None, None) == _lib.EINVAL
    assert b"mitdvp_batch_samples:" in lib.mitdvp_last_error(None)
    assert lib.mitdvp_batch_samples_records(None, None, None, None, None, None, None) == _lib.EINVAL
    assert b"mitdvp_batch_samples_records" in lib.mitdvp_last_error(None)


def test_the_uniform():
    """in [0, 1); another number than the jump channels' for the same (seed, id, step, site); mean and variance of 1e5
    draws within 5 standard errors of 1/2 and 1/12 (standard errors sqrt(1/12 / n) and sqrt(1/180 / n)); the vectorised
    form of the twin gives the same numbers"""
    from helpers import sample_cases as sm
    from pytdscf_amd.trajectories import jump_uniform, sample_uniform

    assert sample_uniform(0, 0, 0, 0, 0) == 0.0  # mix(0) = 0: the one fixed point of the counter scheme, still in [0, 1)
    for args in ((0, 0, 0, 1), (5, 7, 3, 2), (2**64 - 1, 2**63, 10**6, 11)):
        for shot in (0, 1, 63, 64, 65535):
            u = sample_uniform(*args, shot)
            assert 0.0 <= u < 1.0 and u != jump_uniform(*args)
    assert sample_uniform(1, 2, 3, 4, 5) != sample_uniform(1, 2, 3, 5, 4)
    n = 100000
    u = sm.uniforms(9, 4, 2, 10, n // 10)
    assert u.shape == (n // 10, 10) and u.min() >= 0.0 and u.max() < 1.0
    for t, p in ((0, 0), (17, 3), (9999, 9)):
        assert u[t, p] == sample_uniform(9, 4, 2, p, t)
    mean, var = u.mean(), u.var()
    print(f"uniform: mean - 1/2 = {mean - 0.5:.2e}, var - 1/12 = {var - 1 / 12:.2e}")
    assert abs(mean - 0.5) < 5 * np.sqrt(1 / 12 / n) and abs(var - 1 / 12) < 5 * np.sqrt(1 / 180 / n)


@pytest.mark.parametrize("name", ["mixed", "odd", "wide"])
def test_the_twin_draws_with_the_dense_probabilities(name):
    """norm^2 = 0.81 states: prob of every drawn configuration is |psi[config]|^2 / |psi|^2 to 1e-12 relative, and the
    fast form draws the shot-by-shot form's configurations"""
    from helpers import sample_cases as sm

    dims, D = sm.SHAPES[name]
    cores = sm.random_states(dims, D, 2, seed=21)[1]
    nshots = 40
    configs, prob, margins = sm.walk(cores, nshots, seed=3, trajectory_id=1, step=2)
    assert configs.dtype == np.int32 and configs.shape == (nshots, len(dims)) and configs.min() >= 0
    assert np.all(configs < np.array(dims)[None, :])
    P = sm.dense_probs(cores)
    assert abs(P.sum() - 1) < 1e-13
    want = P[tuple(configs.T)]
    worst = np.abs(prob / want - 1).max()
    print(f"{name}: worst |prob / dense - 1| = {worst:.2e}; smallest margin {margins.min():.2e}")
    assert worst < 1e-12
    fast = sm.walk_fast(cores, nshots, seed=3, trajectory_id=1, step=2)
    assert margins.min() > 1e-9 and np.array_equal(fast[0], configs)
    assert np.abs(fast[1] / prob - 1).max() < 1e-12 and np.abs(fast[2] - margins).max() < 1e-12
    assert len({c.tobytes() for c in configs}) > 1


def test_the_selection_rule_on_its_edges():
    """zero-weight outcomes are never drawn; u G on an exact boundary takes the next index; rounding that leaves no
    index takes the last one with weight; G == 0 gives -1 from that site on and prob = 0"""
    from helpers import sample_cases as sm

    g = [0.0, 0.25, 0.0, 0.25, 0.5, 0.0]
    for u in np.linspace(0.0, 1.0, 41, endpoint=False):
        assert sm.pick(g, u)[0] in (1, 3, 4)
    assert sm.pick(g, 0.0)[0] == 1 and sm.pick(g, 0.25)[0] == 3 and sm.pick(g, 0.5)[0] == 4  # run > thr, not >=
    assert sm.pick(g, np.nextafter(0.25, 0))[0] == 1
    assert sm.pick(g, 1.0)[0] == 4  # no running sum exceeds G: the last index with weight (u < 1 can round u G up to G)
    assert sm.pick([0.0, 0.0], 0.3)[0] == -1
    # a product state: every shot is the one configuration with weight, prob 1; a zero site: -1 from there on
    e = lambda d, j: np.eye(d)[j].reshape(1, d, 1).astype(complex)
    cores = [e(2, 1), e(3, 0), e(2, 1), e(4, 3)]
    for walk in (sm.walk, sm.walk_fast):
        configs, prob, _ = walk(cores, 5, 0, 0, 0)
        assert np.array_equal(configs, np.tile([1, 0, 1, 3], (5, 1))) and np.array_equal(prob, np.ones(5))
        configs, prob, _ = walk(cores[:2] + [0 * cores[2], cores[3]], 5, 0, 0, 0)
        assert np.array_equal(configs, np.tile([1, 0, -1, -1], (5, 1))) and np.array_equal(prob, np.zeros(5))


@pytest.mark.parametrize("name", ["mixed", "odd", "wide"])
def test_margins_of_the_device_tests_inputs(name):
    """the device is compared with the twin decision by decision: every decision of the inputs of
    tests/test_gpu_batch_sample.py must be at least 1e-6 away from its boundary, ten orders above the rounding of a g_j"""
    from helpers import sample_cases as sm

    dims, D = sm.SHAPES[name]
    state_seed, seed = sm.CASES[name]
    least = np.inf
    for r, cores in enumerate(sm.random_states(dims, D, sm.B, state_seed)):
        configs, _, margins = sm.walk_fast(cores, sm.NSHOTS, seed, r, 0)
        assert configs.min() >= 0
        least = min(least, margins.min())
    print(f"{name}: smallest margin of {sm.B * sm.NSHOTS * len(dims)} decisions: {least:.2e}")
    assert least >= sm.MARGIN


def test_the_statistical_case_holds_for_the_twin():
    """"mixed", 4096 shots, two states: every one-site frequency and every cell of the (site 1, site 3) table within
    4.5 sigma of the exact value, sigma = sqrt(p (1 - p) / n); and the margins of these inputs"""
    from helpers import sample_cases as sm

    st = sm.STAT
    dims, D = sm.SHAPES[st["name"]]
    for r, cores in enumerate(sm.random_states(dims, D, st["B"], st["state_seed"])):
        configs, _, margins = sm.walk_fast(cores, st["nshots"], st["seed"], r, 0)
        one, two = sm.stat_defects(configs, cores, st["pair"])
        print(f"state {r}: one-site {one:.2f} sigma, pair table {two:.2f} sigma, smallest margin {margins.min():.2e}")
        assert one < st["sigmas"] and two < st["sigmas"] and margins.min() >= sm.MARGIN
        freq = sm.histogram(configs, dims)
        assert all(abs(f.sum() - 1) < 1e-12 for f in freq)


def test_sample_requests_on_the_python_side():
    from pytdscf_amd.engine import sample_request

    assert sample_request(150) == (150, 0) and sample_request(np.int64(5), np.uint64(7)) == (5, 7)
    assert sample_request(0, 2**64 - 1) == (0, 2**64 - 1)
    assert sample_request(-3, 1) == (-3, 1) and sample_request(10**6) == (10**6, 0)  # the range is the library's to refuse
    for bad in ((1.5, 0), (True, 0), ("3", 0), (None, 0), (2**40, 0), (3, -1), (3, 2**64), (3, 0.5)):
        with pytest.raises(ValueError, match="samples request"):
            sample_request(*bad)
