"""GPU: the folded H_eff apply and the structured environment update over the whole range of their kernels
(csrc/vecops.hip::k_fold_env_core, k_gram_env_core<4 / 8 / 16>) and of the host code that feeds them
(csrc/engine.hip::choose_apply_forms, env_fold_ok, env_update_fold), against the oracle's plain contractions
(oracle/tdvp_oracle.py::heff_apply, env_update_left / env_update_right) and, over whole time steps, against OracleMPS.

tests/test_gpu_fold_apply.py and tests/test_gpu_env_fold.py pin the forms at d in {3, 4}, M in {10, 16} with identity
multiples +-1.  Here: the flagship's own instantiation (d = 16, M = 32: gram<8>, four j-groups per i), the limits of the
range (M = 64: 64 KiB of LDS, bit 63 of the state masks; M = 65: everything back to the chain), every tail of the unrolls
(j-groups of 1, 2, 3 elements, lanes t >= m, q-blocks of 1 and 6 live lanes, bonds below one q-block, the dl >= 32
threshold), and the operator structures choose_apply_forms has branches for (tests/helpers/edge_mpo.py: weighted
identities, exactly zero blocks, a state identity-fed from both sides, two general end states, a block between two general
states).  tests/test_edge_mpo_host.py proves on the host that these operators have the structure assumed, so every case
demands the form (flag bits 0x10 edge, 0x20 R side folded, 0x40 L side folded of heff_apply_center; the n_env_fold counter)
as well as the numbers.

Tolerance: 1e-12 relative in the max norm for single contractions, as the two modules above and
tests/test_gpu_fullsize_oracle.py; the sweep-level tolerances are those of test_time_steps_with_and_without_the_fold_agree
and test_c2_exact_shape_three_steps_against_oracle.
"""

import numpy as np
import pytest

from helpers import edge_mpo as em
from helpers.fold_seam import EDGE, FOLD_L, FOLD_R, check_center, engine_under, solve_update_check, to_site

pytestmark = pytest.mark.gpu

BOTH = EDGE | FOLD_R | FOLD_L
FORCED = {"MITDVP_FOLD_APPLY": "1", "MITDVP_FOLD_ENV": "1", "MITDVP_EDGE_APPLY": "1"}
UNSET = {"MITDVP_FOLD_APPLY": None, "MITDVP_FOLD_ENV": None, "MITDVP_EDGE_APPLY": None}


def _at_site(mpo, d, D, c, shape, variables, seed=1, **kw):
    L = len(mpo)
    eng = engine_under(L, variables, **kw)
    eng.set_mpo(mpo)
    eng.init_random([d] * L, D, seed=seed)
    assert eng.get_site_shape(c)[:3] == shape
    to_site(eng, c)
    return eng


def _apply_and_updates(mpo, d, D, c, shape, want_flags, want_env, variables=FORCED, seed=7, **kw):
    """at site c: the apply (the engine's own centre and a random vector) and the update after a solve, left to right, on
    one engine; the update right to left on a second one"""
    from oracle import tdvp_oracle as orc

    rng = np.random.default_rng(seed)
    eng = _at_site(mpo, d, D, c, shape, variables, **kw)
    check_center(orc, eng, mpo, c, rng, want_flags)
    solve_update_check(orc, eng, mpo, c, True, want_env)
    eng.close()
    eng = _at_site(mpo, d, D, c, shape, variables, **kw)
    solve_update_check(orc, eng, mpo, c, False, want_env)
    eng.close()


# ---- 2. the kernels' range ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["3m", "4m", "unset"])
def test_flagship_instantiation(how):
    """d = 16, M = 32 at a 64 x 16 x 64 site (C4's operator at a short bond): k_gram_env_core<8>, four j-groups per i and
    16 KB slabs in k_fold_env_core.  Forced in both complex-product forms; with all three variables unset the library's
    own rules must take the forms too (M > d; (1 + 1) d^2 + d = 528 against 2 M d = 1024 units of D^3 products)."""
    from pytdscf_amd import engine as E

    L, d, M, D, c = 6, 16, 32, 64, 2
    mpo, _ = em.structure("plain", L, d, M, c)
    E.set_gemm_mode("3m" if how == "unset" else how)
    try:
        _apply_and_updates(mpo, d, D, c, (D, d, D), BOTH, 1, UNSET if how == "unset" else FORCED)
    finally:
        E.set_gemm_mode("3m")


# (name, L, d, M, D, centre, flags wanted, structured updates wanted)
RANGE = [
    # gram<16>, m * 64 * 16 = 64 KiB of LDS in k_fold_env_core, bit 63 of S / E, one ragged q-block (n = 48 < 64)
    ("upper_limit", 7, 4, 64, 48, 3, BOTH, 1),
    # upload_mpo_core keeps no host copy of a core wider than 64: no edge form, no structured update, the chain
    ("just_outside", 7, 4, 65, 48, 3, 0, 0),
    # gram<8> at its lower edge (lanes t >= 17 read zero), a full j-group and one of 1, q-blocks of 64 and 6
    ("gram8_lower_edge", 7, 5, 17, 70, 3, BOTH, 1),
    # gram<16> at its lower edge, a j-group of 2, q-blocks of 64 and 1
    ("gram16_lower_edge", 7, 6, 33, 65, 3, BOTH, 1),
    # a j-group of 3, n = 40 < 64
    ("j_tail_of_3", 6, 7, 12, 40, 2, BOTH, 1),
    # the dl >= 32 threshold of the edge form itself, and one below it
    ("smallest_bond", 7, 4, 10, 32, 3, BOTH, 1),
    ("below_smallest_bond", 7, 4, 10, 31, 3, 0, 0),
]


@pytest.mark.parametrize("name,L,d,M,D,c,flags,env", RANGE, ids=[r[0] for r in RANGE])
def test_kernel_range(name, L, d, M, D, c, flags, env):
    """MITDVP_FOLD_APPLY = MITDVP_FOLD_ENV = MITDVP_EDGE_APPLY = 1, the plain finite-state-machine chain at the corners
    of the two kernels' range (see RANGE)."""
    mpo, _ = em.structure("plain", L, d, M, c)
    _apply_and_updates(mpo, d, D, c, (D, d, D), flags, env)


def test_operator_that_does_not_fit_is_not_folded():
    """d = 12, M = 6 at a 32 x 12 x 32 site, forced.  The folded operators and the Gram matrix live in the chain's
    workspaces X_ / Y_, which size_workspaces gives max over the sites of dl dr d max(ml, mr) elements: here
    32 * 32 * 12 * 6 = 73728 (the two 32 x 12 x 32 sites; every other site is smaller).  An operator is (d D)^2 =
    384^2 = 147456 elements: NEITHER side fits, so the edge form runs with both sides unfolded (flags 0x10 exactly:
    zgemm_reduce_ok holds for the groups 12 x 6 and 6 x 12), and env_fold_ok refuses the structured update, whose Gram
    matrix has the same (d D)^2 elements."""
    L, d, M, D, c = 6, 12, 6, 32, 2
    assert (d * D) ** 2 > D * D * d * M  # the capacity rule, both sides (dl = dr, ml = mr)
    mpo, _ = em.structure("plain", L, d, M, c)
    _apply_and_updates(mpo, d, D, c, (D, d, D), EDGE, 0)


# ---- 3. operator structures -----------------------------------------------------------------------------------------
SL, SD, SM, SDIM = 8, 4, 12, 64  # L, d, M, D of the structure tests: sites 3 and 4 are 64 x 4 x 64


def test_weighted_identities():
    """W[0,:,:,0] = 0.9 exp(0.3i) 1 and W[M-1,:,:,M-1] = -0.8 1: the blocks of state 0 / M-1 are alpha^4 1 / beta^3 1,
    folded into wr / wl (the apply) and ws (the update).  The trimmed chain, which wants the plain identity, must not be
    what ran."""
    c = 4
    mpo, _ = em.structure("weighted", SL, SD, SM, c)
    eng = _at_site(mpo, SD, SDIM, c, (SDIM, SD, SDIM), FORCED, integrator="arnoldi", conserve_norm=False)
    _, flags = eng.heff_apply_center()
    assert flags & 0x73 == BOTH, hex(flags)  # bits 0 / 1: an identity block short-circuited by the chain
    eng.close()
    _apply_and_updates(mpo, SD, SDIM, c, (SDIM, SD, SDIM), BOTH, 1, integrator="arnoldi", conserve_norm=False)


def test_zero_blocks_and_the_next_site():
    """No coupling before site 3: the left blocks of the states 1 .. M-2 are exactly zero there (identity multiples with
    weight 0: their terms vanish).  The same engine solved at site 4, where those blocks are general again, is right
    too."""
    from oracle import tdvp_oracle as orc

    c = 3
    rng = np.random.default_rng(8)
    mpo, _ = em.structure("zero", SL, SD, SM, c)
    eng = _at_site(mpo, SD, SDIM, c, (SDIM, SD, SDIM), FORCED)
    assert not eng.get_env(0, c)[:, 1 : SM - 1, :].any()
    check_center(orc, eng, mpo, c, rng, BOTH)
    solve_update_check(orc, eng, mpo, c, True, 1)
    eng.absorb_bond(True)
    assert eng.get_site_shape(c + 1)[:3] == (SDIM, SD, SDIM)
    assert np.abs(eng.get_env(0, c + 1)[:, 1 : SM - 1, :]).max() > 1e-6
    check_center(orc, eng, mpo, c + 1, rng, BOTH)
    solve_update_check(orc, eng, mpo, c + 1, True, 1)
    eng.close()
    eng = _at_site(mpo, SD, SDIM, c, (SDIM, SD, SDIM), FORCED)
    solve_update_check(orc, eng, mpo, c, False, 1)
    eng.close()


def test_state_identity_fed_from_both_sides():
    """A state fed by 0.7 1 on site 3 and drained by (-0.6 + 0.2i) 1 on site 5: at site 4 it is in S and in E at once."""
    c = 4
    mpo, _ = em.structure("both", SL, SD, SM, c)
    _apply_and_updates(mpo, SD, SDIM, c, (SDIM, SD, SDIM), BOTH, 1, integrator="arnoldi", conserve_norm=False)


def test_two_general_end_states_at_d3():
    """The direct sum of two chains of 6 states at d = 3, D = 50: two folded operators per update (|t0| = 2), forced; and
    with MITDVP_FOLD_ENV unset what the library's rule gives for this shape -- the consumed bond wider than d and
    4 ((1 + |t0|) d^2 D^3 + |t0| d D^3) <= 3 (2 M d D^3), worked out here, not asked of the library."""
    L, d, M, D, c = 10, 3, 12, 50, 5
    mpo, _ = em.structure("sum2", L, d, M, c)
    _apply_and_updates(mpo, d, D, c, (D, d, D), BOTH, 1)
    nt = 2
    fresh = d * d * D**3 + nt * (d * d * D**3 + d * D**3)
    chain = M * d * D**3 + M * d * D**3
    rule = int(M > d and 4 * fresh <= 3 * chain)
    assert rule == 1  # 4 * 33 <= 3 * 72
    _apply_and_updates(mpo, d, D, c, (D, d, D), BOTH, rule, dict(FORCED, MITDVP_FOLD_ENV=None))


def test_pass_through_state_is_refused():
    """A state with a general block on either side of the centre and W[p,:,:,p] = 1 there: a block between two general
    states.  Neither the edge form nor a structured update; the two applies and the solve behind the refusal (edge_skip:
    the structure is not looked at again for a while) are right.  (Bits 0x70 of the flags are what is demanded: the
    apply that meets the refusal runs the chain with the two identity blocks it has just verified trimmed, bits 0 / 1.)"""
    c = 4
    mpo, _ = em.structure("pass", SL, SD, SM, c)
    _apply_and_updates(mpo, SD, SDIM, c, (SDIM, SD, SDIM), 0, 0, integrator="arnoldi", conserve_norm=False)


# ---- 4. whole time steps --------------------------------------------------------------------------------------------
def _one_step(make_mpo, L, d, D, dt, **kw):
    from oracle import tdvp_oracle as orc

    res = {}
    for on in ("1", "0"):
        eng = engine_under(L, {"MITDVP_FOLD_ENV": on, "MITDVP_FOLD_APPLY": None, "MITDVP_EDGE_APPLY": None}, **kw)
        eng.set_mpo(make_mpo())
        eng.init_random([d] * L, D, seed=1)
        eng.propagate(dt)
        res[on] = (eng.expectation(), eng.autocorr(), eng.krylov_stats(), eng.get_mps(), eng.norm(),
                   eng.counters()["n_env_fold"])
        eng.close()
    e1, a1, k1, s1, n1, f1 = res["1"]
    e0, a0, k0, s0, n0, f0 = res["0"]
    fid = abs(orc.overlap(s0, s1)) / (n0 * n1)
    print(f"structured updates {f1:.0f} / {f0:.0f}: energy {abs(e1 - e0) / abs(e0):.3e} autocorr "
          f"{abs(a1 - a0) / abs(a0):.3e} fidelity-1 {abs(fid - 1):.3e}")
    assert f1 > 0 and f0 == 0
    assert k1 == k0
    assert abs(e1 - e0) < 1e-10 * abs(e0) and abs(a1 - a0) < 1e-10 * abs(a0)
    assert abs(fid - 1) < 1e-10


def test_time_steps_with_and_without_the_structured_update_agree():
    """One time step with MITDVP_FOLD_ENV=1 against =0 (MITDVP_FOLD_APPLY at its default in both) of a 10-site Liouville
    chain (d=4, M=16, D=64, Arnoldi), of a Hermitian chain (d=4, M=10, Lanczos) and of the chain with weighted identities
    (d=4, M=12, Arnoldi): identical Krylov counts, energy and autocorrelation to 1e-10 relative, fidelity to 1e-10; the
    structured update taken in the one run and never in the other."""
    from pytdscf_amd import synthetic as syn

    _one_step(lambda: syn.synthetic_liouvillian_mpo(10, 16, seed=0, gamma=0.002), 10, 4, 64, 0.5,
              integrator="arnoldi", conserve_norm=False)
    _one_step(lambda: syn.synthetic_mpo(10, 4, 10, seed=0), 10, 4, 64, 1.0)
    _one_step(lambda: em.fsm_mpo(10, 4, 12, seed=0, alpha=em.ALPHA, beta=em.BETA), 10, 4, 64, 0.5,
              integrator="arnoldi", conserve_norm=False)


def test_forced_folds_two_steps_against_the_oracle():
    """The ragged chain d=5, M=17, D=40, L=8 with every form forced, two time steps against OracleMPS: after each step
    equal Krylov counts, energy / autocorrelation to 1e-8 relative, fidelity to 1e-10, norm to 1e-12.  The second step
    runs on the reduced cores the first one cached per site, and must take the structured update again."""
    from oracle import tdvp_oracle as orc

    L, d, D, M, dt = 8, 5, 40, 17, 1.0
    mpo = em.fsm_mpo(L, d, M, seed=0)
    mps = orc.synthetic_mps([d] * L, D, seed=1)
    eng = engine_under(L, FORCED)
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
