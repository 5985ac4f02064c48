"""GPU: the structured environment update with the Gram matrix formed by block rows, upper half only
(csrc/engine_apply.hip::env_update_fold: one TN product per block row i over the blocks j >= i; csrc/vecops.hip::
gram_mirror_lower: the blocks i > j as conjugate transposes of the blocks (j, i); gram_env_core then reads the full
matrix as before), against the oracle's plain contraction (oracle/tdvp_oracle.py::env_update_left / env_update_right)
and, over two time steps, against OracleMPS.

What the shapes pin: the flagship's instantiation; block rows of ragged width with a last 32 x 32 mirror tile of 8 live
rows and columns (D = 40) at odd d; one full 64-wide GEMM tile plus one element on both axes of a transposed block
(D = 65: three mirror tiles per axis, the last with one live row / column); an operator whose reduced core ws[:, :, t] is
not Hermitian (the Liouville generator: mirroring the OUTPUT blocks instead of G would fail it); and complex weights of
the identity states (the conjugation of the mirrored blocks must not reach ws).

Every case asserts the form taken (flag bits of heff_apply_center, the n_env_fold delta) and 1e-12 relative in the max
norm (helpers.fold_seam.TOL: one complex128 contraction with the same summation lengths in another order).
"""

import numpy as np
import pytest

from helpers import edge_mpo as em
from helpers.fold_seam import EDGE, FOLD_L, FOLD_R, check_center, engine_under, solve_update_check, to_site

pytestmark = pytest.mark.gpu

BOTH = EDGE | FOLD_R | FOLD_L
FORCED = {"MITDVP_FOLD_APPLY": "1", "MITDVP_FOLD_ENV": "1", "MITDVP_EDGE_APPLY": "1"}
UNSET = {"MITDVP_FOLD_APPLY": None, "MITDVP_FOLD_ENV": None, "MITDVP_EDGE_APPLY": None}


def _at_site(mpo, d, D, c, variables, seed=1, **kw):
    L = len(mpo)
    eng = engine_under(L, variables, **kw)
    eng.set_mpo(mpo)
    eng.init_random([d] * L, D, seed=seed)
    assert eng.get_site_shape(c)[:3] == (D, d, D)
    to_site(eng, c)
    return eng


def _update(mpo, d, D, c, forward, variables=FORCED, **kw):
    """at the D x d x D site c: the apply's form (flag bits), then a local solve and the update behind it"""
    from oracle import tdvp_oracle as orc

    eng = _at_site(mpo, d, D, c, variables, **kw)
    check_center(orc, eng, mpo, c, np.random.default_rng(11), BOTH)
    solve_update_check(orc, eng, mpo, c, forward, 1)
    eng.close()


def _in_mode(mode, fn):
    from pytdscf_amd import engine as E

    E.set_gemm_mode(mode)
    try:
        fn()
    finally:
        E.set_gemm_mode("3m")


# (name, L, d, M, D, centre)
SHAPES = [
    ("flagship_d16_m32", 6, 16, 32, 64, 2),
    ("ragged_d3", 10, 3, 10, 40, 5),
    ("ragged_d5", 8, 5, 17, 40, 3),
    ("ragged_d7", 8, 7, 17, 40, 3),
    ("tile_plus_one_d4", 10, 4, 16, 65, 5),
]


@pytest.mark.parametrize("forward", [True, False], ids=["fwd", "bwd"])
@pytest.mark.parametrize("mode", ["3m", "4m"])
@pytest.mark.parametrize("name,L,d,M,D,c", SHAPES, ids=[s[0] for s in SHAPES])
def test_block_rows_against_the_oracle(name, L, d, M, D, c, mode, forward):
    """The finite-state-machine chain at the shapes of SHAPES, forced, both complex-product forms, both directions."""
    mpo, _ = em.structure("plain", L, d, M, c)
    _in_mode(mode, lambda: _update(mpo, d, D, c, forward))


@pytest.mark.parametrize("forward", [True, False], ids=["fwd", "bwd"])
@pytest.mark.parametrize("mode", ["3m", "4m"])
def test_liouville_generator_core_is_not_hermitian(mode, forward):
    """d = 4, M = 16 Liouville-space generator at 64 x 4 x 64: three general end states, identity weights -1, and a reduced
    core ws[:, :, t] that is not Hermitian, so neither are the output blocks -- only G may be mirrored."""
    from pytdscf_amd import synthetic as syn

    L, D, c = 10, 64, 5
    mpo = syn.synthetic_liouvillian_mpo(L, 16, seed=0, gamma=0.002)
    w = mpo[c][14, :, :, 15]  # out of the third summand's start state into its end state: identity states of either bond
    assert np.abs(w - w.conj().T).max() > 1e-6
    _in_mode(mode, lambda: _update(mpo, 4, D, c, forward, integrator="arnoldi", conserve_norm=False))


@pytest.mark.parametrize("forward", [True, False], ids=["fwd", "bwd"])
@pytest.mark.parametrize("mode", ["3m", "4m"])
def test_complex_weight_on_an_identity_state(mode, forward):
    """W[0,:,:,0] = 0.9 exp(0.3i) 1, W[M-1,:,:,M-1] = -0.8 1 (helpers/edge_mpo.py "weighted"): the multiples lam_c are complex
    and sit in ws, which the conjugation of the mirrored blocks of G must leave alone."""
    L, d, M, D, c = 8, 4, 12, 64, 4
    mpo, want = em.structure("weighted", L, d, M, c)
    assert abs(np.imag(want["S"][0])) > 0.1
    _in_mode(mode, lambda: _update(mpo, d, D, c, forward, integrator="arnoldi", conserve_norm=False))


def test_two_steps_of_the_ragged_chain_default_rules():
    """The ragged chain d = 5, M = 17, D = 40, L = 8 with no variable set (the library's own rules take the forms: M > d),
    two time steps against OracleMPS: equal Krylov counts, energy / autocorrelation to 1e-8 relative, fidelity to 1e-10,
    norm to 1e-12 (the bounds of tests/test_gpu_fold_range.py::test_forced_folds_two_steps_against_the_oracle)."""
    from oracle import tdvp_oracle as orc

    L, d, D, M, dt = 8, 5, 40, 17, 1.0
    mpo = em.fsm_mpo(L, d, M, seed=0)
    mps = orc.synthetic_mps([d] * L, D, seed=1)
    eng = engine_under(L, UNSET)
    eng.set_mpo(mpo)
    eng.set_mps(mps)
    ref = orc.OracleMPS([c.copy() for c in mps], mpo)
    taken = 0
    for step in range(2):
        eng.propagate(dt)
        ref.propagate(dt)
        cnt = eng.counters()
        print(f"step {step}: structured updates {cnt['n_env_fold']:.0f}, edge applies {cnt['n_heff_edge']:.0f}")
        assert cnt["n_env_fold"] > taken, step
        taken = cnt["n_env_fold"]
        assert eng.krylov_stats() == [ref.kprev[i] for i in range(L)], step
        eg, er = eng.expectation(), ref.expectation()
        ag, ar = eng.autocorr(), ref.autocorr()
        fid = abs(orc.overlap(ref.cores, eng.get_mps()))
        print(f"step {step}: energy {abs(eg - er) / abs(er):.3e} autocorr {abs(ag - ar) / abs(ar):.3e} "
              f"fidelity-1 {abs(fid - 1):.3e} norm-1 {abs(eng.norm() - 1):.3e}")
        assert abs(eg - er) < 1e-8 * abs(er) and abs(ag - ar) < 1e-8 * abs(ar), step
        assert abs(eng.norm() - 1) < 1e-12
        assert abs(fid - 1) < 1e-10, step
    eng.close()
