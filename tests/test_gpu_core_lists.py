"""GPU: the two core contractions with their coefficients taken from the lists uploaded beside the reduced cores
(csrc/core_lists.h; csrc/vecops.hip::k_fold_env_core_list, k_gram_env_core_list; built by MpoSite::EdgeCache::rebuild)
against the dense kernels, which read the cores themselves.

MITDVP_CORE_LISTS (read when the engine is created): unset = the list kernels, 0 = the dense ones.  The list kernels form
the dense kernels' products from the same operands in the same order, so everything behind them must be equal bit for bit:
heff_apply_center (both folds feed its operators) and one environment update per direction (the Gram core; the fold of
the general states' operator -- no Strassen level unless a test asks for one -- or, where the solve packed Strassen
factors, the Gram core with ws_reuse).  Each result
is also within TOL = 1e-12 of the oracle's plain contraction.  The forms are forced and asserted: the flag bits of
heff_apply_center (edge, both sides folded) and the n_env_fold / n_env_reuse deltas.
"""

import numpy as np
import pytest

from helpers import edge_mpo as em
from helpers.fold_seam import EDGE, FOLD_L, FOLD_R, TOL, crandn, engine_under, rel, split

pytestmark = pytest.mark.gpu

BOTH = EDGE | FOLD_R | FOLD_L
NON_HERMITIAN = {"weighted", "liouville"}

# name: (d, M, bonds, centre); the centre site is bonds[c] x d x bonds[c + 1]
SHAPES = {
    "40x4x40_m10": (4, 10, [1, 4, 16, 40, 40, 16, 4, 1], 3),
    "48x5x32_m17": (5, 17, [1, 5, 25, 48, 32, 25, 5, 1], 3),              # dl != dr, ragged j-group of one
    "33x3x33_m6": (3, 6, [1, 3, 9, 27, 33, 33, 27, 9, 3, 1], 4),          # one j-group of three, <4>
    "65x6x65_m33": (6, 33, [1, 6, 36, 65, 65, 36, 6, 1], 3),              # one lane past a q-block; m = 33 takes <16>
    "64x16x64_m32": (16, 32, [1, 16, 64, 64, 16, 1], 2),                  # the flagship's instantiation, <8>
    "48x4x48_m64": (4, 64, [1, 4, 16, 48, 48, 16, 4, 1], 3),              # the widest bond: lane 63, t = 63
}


def _vars(lists, strassen):
    return {"MITDVP_FOLD_APPLY": "1", "MITDVP_FOLD_ENV": "1", "MITDVP_EDGE_APPLY": "1", "MITDVP_CORE_LISTS": lists,
            "MITDVP_FOLD_STRASSEN": strassen}


def _engine_at(mpo, d, bonds, c, variables, structure):
    L = len(bonds) - 1
    rng = np.random.default_rng(1)
    cores = [crandn(rng, bonds[i], d, bonds[i + 1]) for i in range(L)]
    kw = dict(integrator="arnoldi", conserve_norm=False) if structure in NON_HERMITIAN else {}
    eng = engine_under(L, variables, **kw)
    eng.set_mpo(mpo)
    eng.set_mps(cores, canonicalize=True, scale=None if structure in NON_HERMITIAN else 1.0)
    eng.build_envs(1)
    for _ in range(c):
        eng.split_center(True)
        eng.absorb_bond(True)
    assert eng.get_site_shape(c)[:3] == (bonds[c], d, bonds[c + 1])
    assert eng.counters()["n_env_fold"] == 0
    return eng


def _run(orc, mpo, d, bonds, c, forward, lists, structure, strassen, want_reuse):
    """apply to the centre and to a random vector, then the update behind that check: (the three arrays, all checked
    against the oracle)"""
    eng = _engine_at(mpo, d, bonds, c, _vars(lists, strassen), structure)
    Lb, Rb, psi = eng.get_env(0, c), eng.get_env(1, c + 1), eng.get_site(c)
    x = crandn(np.random.default_rng(41), *psi.shape)
    a, flags = eng.heff_apply_center()
    assert flags & 0x70 == BOTH, hex(flags)
    b, flags = eng.heff_apply_center(x)  # the check behind this apply is the one the update relies on
    assert flags & 0x70 == BOTH, hex(flags)
    ra, rb = rel(a, orc.heff_apply(Lb, mpo[c], Rb, psi)), rel(b, orc.heff_apply(Lb, mpo[c], Rb, x))
    k0 = eng.counters()
    got, ref = split(orc, eng, mpo, c, forward)
    k1 = eng.counters()
    ru = rel(got, ref)
    print(f"lists {lists}: applies {ra:.3e} {rb:.3e}, update {'->' if forward else '<-'} {ru:.3e}, "
          f"reuse {k1['n_env_reuse'] - k0['n_env_reuse']:.0f}")
    assert k1["n_env_fold"] - k0["n_env_fold"] == 1
    assert k1["n_env_reuse"] - k0["n_env_reuse"] == want_reuse
    assert max(ra, rb, ru) < TOL
    eng.close()
    return a, b, got


def _both_settings(mpo, d, bonds, c, forward, structure="plain", strassen="0", want_reuse=0):
    from oracle import tdvp_oracle as orc

    new = _run(orc, mpo, d, bonds, c, forward, None, structure, strassen, want_reuse)
    old = _run(orc, mpo, d, bonds, c, forward, "0", structure, strassen, want_reuse)
    for name, p, q in zip(("apply to the centre", "apply to a random vector", "updated block"), new, old):
        assert np.array_equal(p, q), (name, float(np.abs(p - q).max()))


@pytest.mark.parametrize("forward", [True, False], ids=["fwd", "bwd"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_bit_for_bit(name, forward):
    d, M, bonds, c = SHAPES[name]
    mpo, _ = em.structure("plain", len(bonds) - 1, d, M, c)
    _both_settings(mpo, d, bonds, c, forward)


@pytest.mark.parametrize("forward", [True, False], ids=["fwd", "bwd"])
def test_liouville_generator_two_general_end_states(forward):
    """d = 4, M = 10 Liouville-space generator, a direct sum: H (x) 1 and 1 (x) H^T each end in a general state, so the
    update folds two cores wg[k], each with its own list; a reduced core that is not Hermitian"""
    from pytdscf_amd import synthetic as syn

    d, M, bonds, c = 4, 10, [1, 4, 16, 40, 40, 16, 4, 1], 3
    mpo = syn.synthetic_liouvillian_mpo(len(bonds) - 1, M, seed=0, gamma=0.002)
    assert mpo[c].shape == (M, d, d, M)
    _both_settings(mpo, d, bonds, c, forward, structure="liouville")


@pytest.mark.parametrize("forward", [True, False], ids=["fwd", "bwd"])
@pytest.mark.parametrize("structure", ["weighted", "zero"])
def test_complex_weights_and_exactly_zero_blocks(structure, forward):
    """weighted: complex multiples of the identity states ride in every list.  zero: the left blocks of the states
    1 .. M-2 are exactly zero, their multiples are zero and whole records of the lists are empty."""
    d, M, bonds, c = SHAPES["40x4x40_m10"]
    mpo, _ = em.structure(structure, len(bonds) - 1, d, M, c)
    _both_settings(mpo, d, bonds, c, forward, structure=structure)


@pytest.mark.parametrize("forward", [True, False], ids=["fwd", "bwd"])
def test_update_reusing_the_solves_factors(forward):
    """Two Strassen levels forced at 40 x 4 x 40: the update takes the solve's packed operator, no fold of wg, and backward
    the Gram core runs on ws_reuse (column c0 zero: a mask bit cleared in every record of that wave)."""
    d, M, bonds, c = SHAPES["40x4x40_m10"]
    mpo, _ = em.structure("plain", len(bonds) - 1, d, M, c)
    _both_settings(mpo, d, bonds, c, forward, strassen="2", want_reuse=1)
