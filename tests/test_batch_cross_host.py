"""CPU: cross overlaps and two-time correlation functions of the batched trajectories -- the C surface is declared,
exported and loads; the walk of k_batch_cross, restated in NumPy, is <psi_a| embed(O) |psi_b> on dense vectors; and the
physics case of tests/test_gpu_batch_cross.py is exact, moves, and is out of the t/2 trick's reach, shown from the NumPy
oracle and dense expm alone."""

import ctypes as C
import os

import numpy as np
import pytest

NAMES = ["mitdvp_batch_snapshot", "mitdvp_batch_set_cross", "mitdvp_batch_cross", "mitdvp_batch_cross_records"]


def test_cross_symbols_are_declared_exported_and_load():
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
    assert lib.mitdvp_batch_snapshot(None) == _lib.EINVAL
    assert b"mitdvp_batch_snapshot" in lib.mitdvp_last_error(None)
    assert lib.mitdvp_batch_set_cross(None, 0, None, None, None, None, None) == _lib.EINVAL
    assert b"mitdvp_batch_set_cross" in lib.mitdvp_last_error(None)
    assert lib.mitdvp_batch_cross(None, None, None, None) == _lib.EINVAL
    assert lib.mitdvp_batch_cross_records(None, None, None, None, None) == _lib.EINVAL
    assert b"mitdvp_batch_cross_records" in lib.mitdvp_last_error(None)


@pytest.mark.parametrize("site", [-1, 0, 2, 3])
def test_the_walk_is_the_dense_matrix_element(site):
    """mixed dims (2, 3, 4, 2), the operator on the first, a middle and the last site, and none: to 1e-13 |a| |b|"""
    from helpers import cross_cases as cc
    from helpers import jump_oracle as jo

    dims = (2, 3, 4, 2)
    a, b = cc.random_states(dims, 5, 2, seed=3)
    va, vb = jo.dense_state(a), jo.dense_state(b)
    na, nb = np.linalg.norm(va), np.linalg.norm(vb)
    assert abs(na - 0.7) < 1e-12 and abs(nb - 0.9) < 1e-12 and abs(cc.norm_of(a) - na) < 1e-13
    O = cc.random_op(dims[site], 9) if site >= 0 else None
    want = np.vdot(va, (jo.embed(O, site, dims) @ vb) if site >= 0 else vb)
    got = cc.walk(a, b, site, O)
    print(f"site {site}: |walk - dense| = {abs(got - want):.2e}")
    assert abs(got - want) < 1e-13 * na * nb
    assert abs(want) > 1e-3  # not a comparison of two zeros
    if site < 0:
        assert abs(cc.walk(b, a) - np.conj(got)) < 1e-13 * na * nb


def test_the_physics_case_is_exact_moves_and_defeats_the_half_time_trick():
    """L = 4 spin chain, D = 4, dt = 0.4, 8 steps, complex product start, B = S_x on site 1, A = S_z on site 2, Arnoldi at
    1e-9.  Figures of this case: the oracle's C(t) is 2.6e-12 from dense expm (bar 5e-12); <psi(0)|psi(t)> 3e-14; the
    t/2-trick value 0.151-0.090j against <psi(0)|psi(2t)> = -0.0016-0.190j, 0.18 apart (bar 0.1).  |B psi(0)| is exactly
    1/2 here, and C(0) = 0: C(t) = <psi(t)| A |phi(t)> with phi(0) = B psi(0) moves by 0.140 over the run, and by 0.281
    per unit norm of phi(0) -- the figure that goes with the bar of 0.2, which is therefore asserted on C(t) / |B psi(0)|
    (the correlation function of the NORMALISED phi); the absolute movement is asserted against the same bar times
    |B psi(0)|.  Both say the same thing: the signal is nowhere near flat."""
    from helpers import cross_cases as cc

    corr, auto, auto2 = cc.dense()
    oc = cc.oracle_corr("arnoldi", 1e-9)
    dev = np.abs(oc - corr).max()
    move = np.abs(corr - corr[0]).max()
    nb = np.linalg.norm(cc.psi_phi_vectors()[1][cc.B_OP[0]])  # |B psi(0)|: the other sites' vectors are normalised
    oa, trick = cc.oracle_auto("arnoldi", 1e-9)
    dev_auto = np.abs(oa - auto).max()
    gap = abs(trick[-1] - auto2[-1])
    print(f"oracle C(t) vs dense expm {dev:.2e}; C(t) moves by {move:.3f}, |B psi(0)| = {nb:.3f}, per unit norm {move / nb:.3f}; "
          f"oracle <psi(0)|psi(t)> vs dense {dev_auto:.2e}; t/2 trick {trick[-1]:.4f} vs <psi(0)|psi(2t)> {auto2[-1]:.4f}: {gap:.3f}")
    assert dev < 5e-12 and dev_auto < 5e-12
    assert abs(nb - 0.5) < 1e-15
    assert move / nb > 0.2 and move > 0.2 * nb
    assert gap > 0.1


def test_correlation_function_checks_its_arguments_before_any_engine(monkeypatch):
    from helpers import cross_cases as cc
    from helpers import spin_bath as sb
    from pytdscf_amd import trajectories as tr

    class _Stop(Exception):
        pass

    def no_engine(*a, **k):
        raise _Stop("an engine was created")

    monkeypatch.setattr(tr, "TDVPBatch", no_engine)
    m = cc.model()
    args = dict(maxstep=3, stepsize=0.1)
    with pytest.raises(ValueError, match="both A and B"):
        tr.correlation_function(m, [cc.START], A=(0, sb.SZ), **args)
    with pytest.raises(ValueError, match="A acts on site 4"):
        tr.correlation_function(m, [cc.START], A=(4, sb.SZ), B=(0, sb.SX), **args)
    with pytest.raises(ValueError, match=r"B has shape \(3, 3\)"):
        tr.correlation_function(m, [cc.START], A=(0, sb.SZ), B=(0, np.eye(3)), **args)
    with pytest.raises(ValueError, match="one per start"):
        tr.correlation_function(m, [cc.START], weights=[0.5, 0.5], **args)
    with pytest.raises(ValueError, match="annihilates start 0"):
        tr.correlation_function(m, [[[1, 0]] * 4], A=(0, sb.SZ), B=(1, np.array([[0, 0], [0, 1]])), **args)
    with pytest.raises(TypeError):
        tr.correlation_function(m, [cc.START], jumps={}, **args)
    with pytest.raises(_Stop):
        tr.correlation_function(m, [cc.START], A=cc.A_OP, B=cc.B_OP, **args)
