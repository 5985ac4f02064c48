"""GPU: the folded variant of the edge form of the H_eff apply (csrc/engine.hip::heff_apply_edge with fold_r_ / fold_l_,
csrc/vecops.hip::fold_env_core) against the oracle's plain three-leg contraction (oracle/tdvp_oracle.py::heff_apply).

Where a side's MPO bond is wider than d, the reduced core is contracted into the environment block once per local solve,
    GR[(i,r),(j,s)] = sum_t wr[i,j,t] R[r,t,s],      GL[(a,i),(b,j)] = sum_c wl[i,c,j] L[a,c,b],
and the side's apply is one plain GEMM.  mitdvp_heff_apply_center reports the variant in bits 0x20 (R side) and 0x40
(L side) beside the edge form's 0x10.  MITDVP_FOLD_APPLY (read when the engine is created): 1 = wherever the edge form is
valid, 0 = never, unset = the library's rule (a side is folded when its MPO bond exceeds d).

Tolerance: 1e-12 relative in the max norm over the whole output, as tests/test_gpu_edge_apply.py (complex128, the same
summation lengths: the fold changes the order of the sums, not their number of terms).
"""

import numpy as np
import pytest

from helpers.fold_seam import EDGE, FOLD_L, FOLD_R, engine_under
from helpers.fold_seam import check_center as _check_center
from helpers.fold_seam import crandn as _crandn
from helpers.fold_seam import to_site as _to_site

pytestmark = pytest.mark.gpu


def _engine(L, fold="1", edge="1", **kw):
    """an engine with MITDVP_FOLD_APPLY / MITDVP_EDGE_APPLY set while it is created (None: the variable unset)"""
    return engine_under(L, {"MITDVP_FOLD_APPLY": fold, "MITDVP_EDGE_APPLY": edge}, **kw)


@pytest.mark.parametrize("mode", ["3m", "4m"])
def test_forced_fold_against_the_oracle(mode):
    """MITDVP_FOLD_APPLY=1, both complex-product forms: a finite-state-machine chain d=4, M=10, D=128 at an interior site
    and at a tapering one (64 x 4 x 128: the two operators differ in size); a Liouville-space generator (M=16: several
    start and end states, weights -1); a ragged chain d=3, M=10, D=50 (no bond a multiple of a tile)."""
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import engine as E
    from pytdscf_amd import synthetic as syn

    rng = np.random.default_rng(11)
    both = EDGE | FOLD_R | FOLD_L
    E.set_gemm_mode(mode)
    try:
        L, d, D, M = 10, 4, 128, 10
        mpo = syn.synthetic_mpo(L, d, M, seed=0)
        for c, shape in ((5, (D, d, D)), (3, (64, d, D))):
            eng = _engine(L)
            eng.set_mpo(mpo)
            eng.init_random([d] * L, D, seed=1)
            assert eng.get_site_shape(c)[:3] == shape
            _to_site(eng, c)
            _check_center(orc, eng, mpo, c, rng, both)
            eng.close()

        L, D = 10, 128
        mpo = syn.synthetic_liouvillian_mpo(L, 16, seed=0, gamma=0.002)
        eng = _engine(L, integrator="arnoldi", conserve_norm=False)
        eng.set_mpo(mpo)
        eng.init_random([4] * L, D, seed=3)
        assert eng.get_site_shape(5)[:3] == (D, 4, D)
        _to_site(eng, 5)
        _check_center(orc, eng, mpo, 5, rng, both)
        eng.close()

        L, d, D, M = 10, 3, 50, 10
        mpo = syn.synthetic_mpo(L, d, M, seed=2)
        eng = _engine(L)
        eng.set_mpo(mpo)
        eng.init_random([d] * L, D, seed=4)
        assert eng.get_site_shape(5)[:3] == (D, d, D)
        _to_site(eng, 5)
        _check_center(orc, eng, mpo, 5, rng, both)
        eng.close()
    finally:
        E.set_gemm_mode("3m")


def test_default_rule():
    """MITDVP_FOLD_APPLY unset: d=4, M=16, D=128 folds both sides; d=32, M=16, D=128 (the C3 shape) folds none."""
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import synthetic as syn

    rng = np.random.default_rng(12)
    for L, d, M, c, want in ((10, 4, 16, 5, EDGE | FOLD_R | FOLD_L), (6, 32, 16, 2, EDGE)):
        D = 128
        mpo = syn.synthetic_mpo(L, d, M, seed=0)
        eng = _engine(L, fold=None)
        eng.set_mpo(mpo)
        eng.init_random([d] * L, D, seed=1)
        assert eng.get_site_shape(c)[:3] == (D, d, D)
        _to_site(eng, c)
        _check_center(orc, eng, mpo, c, rng, want)
        eng.close()


def test_a_general_core_is_not_folded():
    """A core with a block between two general states: neither the edge form nor a fold, and the result is right."""
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import synthetic as syn

    L, d, D, M = 8, 4, 64, 10
    rng = np.random.default_rng(13)
    general = syn.synthetic_mpo(L, d, M, seed=2)
    general[4][3, :, :, 4] = 0.01 * _crandn(rng, d, d)
    eng = _engine(L)
    eng.set_mpo(general)
    eng.init_random([d] * L, D, seed=4)
    assert eng.get_site_shape(4)[:3] == (D, d, D)
    _to_site(eng, 4)
    _check_center(orc, eng, general, 4, rng, 0)
    eng.close()


def _one_step(make_mpo, L, d, D, dt, **kw):
    from oracle import tdvp_oracle as orc

    res = {}
    for on in ("1", "0"):
        eng = _engine(L, fold=on, **kw)
        eng.set_mpo(make_mpo())
        eng.init_random([d] * L, D, seed=1)
        eng.propagate(dt)
        res[on] = (eng.expectation(), eng.autocorr(), eng.krylov_stats(), eng.get_mps(), eng.norm())
        eng.close()
    e1, a1, k1, s1, n1 = res["1"]
    e0, a0, k0, s0, n0 = res["0"]
    fid = abs(orc.overlap(s0, s1)) / (n0 * n1)
    print(f"energy {abs(e1 - e0) / abs(e0):.3e} autocorr {abs(a1 - a0) / abs(a0):.3e} fidelity-1 {abs(fid - 1):.3e}")
    assert k1 == k0
    assert abs(e1 - e0) < 1e-10 * abs(e0) and abs(a1 - a0) < 1e-10 * abs(a0)
    assert abs(fid - 1) < 1e-10


def test_time_steps_with_and_without_the_fold_agree():
    """One time step of a 10-site Liouville chain (d=4, M=16, D=64, Arnoldi) and of a Hermitian chain (d=4, M=10,
    Lanczos) with MITDVP_FOLD_APPLY=1 against =0: identical Krylov counts, energy and autocorrelation to 1e-10 relative,
    fidelity to 1e-10."""
    from pytdscf_amd import synthetic as syn

    _one_step(lambda: syn.synthetic_liouvillian_mpo(10, 16, seed=0, gamma=0.002), 10, 4, 64, 0.5,
              integrator="arnoldi", conserve_norm=False)
    _one_step(lambda: syn.synthetic_mpo(10, 4, 10, seed=0), 10, 4, 64, 1.0)
