"""GPU: the structured environment update (csrc/engine.hip::env_update_fold, csrc/vecops.hip::gram_env_core) against the
oracle's plain contraction (oracle/tdvp_oracle.py::env_update_left / env_update_right).

With I the MPO-bond states whose blocks of the consumed environment are multiples of the identity (found by the local
solve's check of exactly that block), the update is the site tensor's Gram matrix contracted with the reduced core of the
states in I, plus, per out state t0 that a general state feeds, T^H (GL_t0 T) with the folded operator GL_t0.  The counter
n_env_fold tells which form an update took.  MITDVP_FOLD_ENV (read when the engine is created): 1 = wherever the form is
valid, 0 = never, unset = the library's rule (consumed bond wider than d and at most 3/4 of the chain's products left).

The engine is moved to an interior site with build_envs / split_center / absorb_bond (those updates have no check behind
them and run the chain), the site is solved (site_exp) or probed (heff_apply_center), which runs the check, and the block
split_center builds next is compared.  Tolerance: 1e-12 relative in the max norm, as tests/test_gpu_edge_apply.py and
tests/test_gpu_fold_apply.py (complex128, the same summation lengths in another order).
"""

import numpy as np
import pytest

from helpers.fold_seam import TOL, engine_under
from helpers.fold_seam import rel as _rel
from helpers.fold_seam import solve_update_check as _solve_update_check
from helpers.fold_seam import split as _split
from helpers.fold_seam import to_site as _to_site

pytestmark = pytest.mark.gpu


def _engine(L, fold_env="1", **kw):
    """an engine with MITDVP_FOLD_ENV set while it is created (None: unset)"""
    return engine_under(L, {"MITDVP_FOLD_ENV": fold_env}, **kw)


@pytest.mark.parametrize("forward", [True, False])
@pytest.mark.parametrize("mode", ["3m", "4m"])
def test_forced_against_the_oracle(mode, forward):
    """MITDVP_FOLD_ENV=1, both complex-product forms, both directions: a finite-state-machine chain d=4, M=10, D=128 at an
    interior site and at a tapering one (64 x 4 x 128: Gram matrix and folded operator differ in size); a Liouville-space
    generator (M=16: three start and three end states, weights -1 -- the form is taken, with one folded operator per
    general end state); a ragged chain d=3, M=10, D=50 (no bond a multiple of a tile)."""
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import engine as E
    from pytdscf_amd import synthetic as syn

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
            _solve_update_check(orc, eng, mpo, c, forward, 1)
            eng.close()

        L, D = 10, 128
        mpo = syn.synthetic_liouvillian_mpo(L, 16, seed=0, gamma=0.002)
        eng = _engine(L, integrator="arnoldi", conserve_norm=False)
        eng.set_mpo(mpo)
        eng.init_random([4] * L, D, seed=3)
        assert eng.get_site_shape(5)[:3] == (D, 4, D)
        _to_site(eng, 5)
        _solve_update_check(orc, eng, mpo, 5, forward, 1)
        eng.close()

        L, d, D, M = 10, 3, 50, 10
        mpo = syn.synthetic_mpo(L, d, M, seed=2)
        eng = _engine(L)
        eng.set_mpo(mpo)
        eng.init_random([d] * L, D, seed=4)
        assert eng.get_site_shape(5)[:3] == (D, d, D)
        _to_site(eng, 5)
        _solve_update_check(orc, eng, mpo, 5, forward, 1)
        eng.close()
    finally:
        E.set_gemm_mode("3m")


@pytest.mark.parametrize("forward", [True, False])
def test_default_rule(forward):
    """MITDVP_FOLD_ENV unset: d=4, M=16, D=128 (a C5-like interior shape) takes the form; d=32, M=16, D=128 (the C3
    shape: the bond is not wider than d) does not."""
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import synthetic as syn

    for L, d, M, c, want in ((10, 4, 16, 5, 1), (6, 32, 16, 2, 0)):
        D = 128
        mpo = syn.synthetic_mpo(L, d, M, seed=0)
        eng = _engine(L, fold_env=None)
        eng.set_mpo(mpo)
        eng.init_random([d] * L, D, seed=1)
        assert eng.get_site_shape(c)[:3] == (D, d, D)
        _to_site(eng, c)
        _solve_update_check(orc, eng, mpo, c, forward, want)
        eng.close()


def test_default_rule_takes_the_liouville_generator():
    """MITDVP_FOLD_ENV unset, the C5 generator (d=4, M=16, three general end states): (1 + 3) d^2 + 3 d = 76 against
    2 M d = 128 units of D^3 products -- taken."""
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import synthetic as syn

    L, D = 10, 128
    mpo = syn.synthetic_liouvillian_mpo(L, 16, seed=0, gamma=0.002)
    eng = _engine(L, fold_env=None, integrator="arnoldi", conserve_norm=False)
    eng.set_mpo(mpo)
    eng.init_random([4] * L, D, seed=3)
    _to_site(eng, 5)
    _solve_update_check(orc, eng, mpo, 5, True, 1)
    eng.close()


def test_not_for_adaptive_ranks():
    """An engine with adaptive bond dimensions (bra tensor != ket tensor in its updates) never takes the form, forced or
    not; the same run without adaptive ranks does."""
    from pytdscf_amd import synthetic as syn

    L, d, D, M = 8, 4, 32, 10
    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    took = {}
    for adaptive in (True, False):
        eng = _engine(L)
        eng.set_mpo(mpo)
        eng.init_random([d] * L, D, seed=1)
        if adaptive:
            eng.set_adaptive(True, Dmax=D + 4, dD=2, p_proj=1e-9)
        eng.propagate(0.2)
        took[adaptive] = eng.counters()["n_env_fold"]
        eng.close()
    print(f"structured updates: adaptive {took[True]:.0f}, fixed ranks {took[False]:.0f}")
    assert took[True] == 0
    assert took[False] > 0


@pytest.mark.parametrize("forward", [True, False])
def test_forced_off_is_the_chain_bit_for_bit(forward):
    """MITDVP_FOLD_ENV=0 after a check gives, bit for bit, the block of an update that had no check behind it (the
    three-stage chain), and the forced form agrees with both to the tolerance."""
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import synthetic as syn

    L, d, D, M, c = 10, 4, 128, 10, 5
    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    out = {}
    for name, fold_env, check in (("off", "0", True), ("nocheck", "1", False), ("on", "1", True)):
        eng = _engine(L, fold_env=fold_env)
        eng.set_mpo(mpo)
        eng.init_random([d] * L, D, seed=1)
        _to_site(eng, c)
        if check:
            eng.heff_apply_center()  # the check of a local solve, the centre tensor untouched
        got, _ = _split(orc, eng, mpo, c, forward)
        out[name] = (got, eng.counters()["n_env_fold"])
        eng.close()
    assert out["off"][1] == 0 and out["nocheck"][1] == 0 and out["on"][1] == 1
    assert np.array_equal(out["off"][0], out["nocheck"][0])
    r = _rel(out["on"][0], out["off"][0])
    print(f"structured against chain: rel err {r:.3e}")
    assert r < TOL


def test_a_stale_check_falls_back():
    """The identity sets belong to the blocks the check looked at: after a check at site c, the update at c may use them
    (once); the update at c + 1, reached without a solve there, consumes another block and must run the chain -- and be
    right."""
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import synthetic as syn

    L, d, D, M, c = 10, 4, 128, 10, 4
    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    eng = _engine(L)
    eng.set_mpo(mpo)
    eng.init_random([d] * L, D, seed=1)
    _to_site(eng, c)
    eng.heff_apply_center()
    got, ref = _split(orc, eng, mpo, c, True)
    assert eng.counters()["n_env_fold"] == 1 and _rel(got, ref) < TOL
    eng.absorb_bond(True)
    got, ref = _split(orc, eng, mpo, c + 1, True)  # no check of envL[c + 1] has run
    assert eng.counters()["n_env_fold"] == 1
    r = _rel(got, ref)
    print(f"update behind a stale check: rel err {r:.3e}")
    assert r < TOL
    # and a check whose update went elsewhere is not kept for later: probe at c + 2, move on without using it at once
    eng.absorb_bond(True)
    eng.heff_apply_center()
    eng.split_center(True)   # uses the check (site c + 2)
    eng.absorb_bond(True)
    got, ref = _split(orc, eng, mpo, c + 3, True)  # site c + 3: nothing checked
    assert eng.counters()["n_env_fold"] == 2
    assert _rel(got, ref) < TOL
    eng.close()
