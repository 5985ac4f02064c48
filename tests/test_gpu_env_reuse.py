"""GPU: the structured environment update taking the general states' operator from the Strassen factors the local solve
packed (csrc/engine_apply.hip::env_update_fold with a reuse level; decided by MpoSite::EdgeCache::rebuild, recorded by
choose_apply_forms in EnvChecked::lvl), and the one-launch packing / combining of a level-2 L side
(csrc/vecops.hip::strassen_operands2 for the vector, strassen_combine2; the R side keeps the two-pass kernels).

MITDVP_FOLD_ENV_REUSE (read when the engine is created): 0 = never, unset = whenever the core's index sets allow it
(tests/helpers/env_reuse.py::decide, the host twin) and the solve packed the consumed side at a Strassen level >= 1.
The counter n_env_reuse tells which path an update took.  MITDVP_STRASSEN_FUSE=0 keeps the two-pass kernels.

Every update is compared with the oracle's plain contraction (TOL of helpers/fold_seam.py, 1e-12) and with the block of
an engine under MITDVP_FOLD_ENV_REUSE=0 taken through the same moves (1e-13: the same operator up to a factor, applied
as the solve's applies apply it; on the host the two-level plan is 2e-15 from the plain product).
"""

import numpy as np
import pytest

from helpers import edge_mpo as em
from helpers import env_reuse as er
from helpers.fold_seam import TOL, crandn, engine_under, rel, solve_update_check

pytestmark = pytest.mark.gpu

TOL_OFF = 1e-13
NON_HERMITIAN = {"weighted", "both"}  # complex multiples: the Arnoldi integrator, no norm conservation

# (dl, d, dr, M), bonds, centre, Strassen level of both sides under MITDVP_FOLD_STRASSEN=2
SHAPES = {
    "partial_tiles": ((40, 4, 40, 10), [1, 4, 16, 40, 40, 16, 4, 1], 3, 2),
    "dl_differs_from_dr": ((48, 4, 32, 10), [1, 4, 16, 48, 32, 16, 4, 1], 3, 2),
    "even_only_takes_one_level": ((34, 3, 34, 10), [1, 3, 9, 27, 34, 34, 27, 9, 3, 1], 4, 1),
    "odd_has_no_level": ((33, 3, 33, 10), [1, 3, 9, 27, 33, 33, 27, 9, 3, 1], 4, 0),
}


def _vars(reuse=None, fuse=None):
    return {"MITDVP_FOLD_APPLY": "1", "MITDVP_FOLD_ENV": "1", "MITDVP_EDGE_APPLY": "1", "MITDVP_FOLD_STRASSEN": "2",
            "MITDVP_FOLD_ENV_REUSE": reuse, "MITDVP_STRASSEN_FUSE": fuse}


def _engine_at(mpo, d, bonds, c, variables, structure="plain", seed=1):
    L = len(bonds) - 1
    rng = np.random.default_rng(seed)
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
    return eng


def _solve_update_pair(orc, mpo, d, bonds, c, forward, structure, want_reuse):
    """a solve and the update behind it on an engine with the reuse and on one without: the counters, the oracle, each other"""
    blocks = []
    for reuse in (None, "0"):
        eng = _engine_at(mpo, d, bonds, c, _vars(reuse), structure)
        n0 = eng.counters()["n_env_reuse"]
        solve_update_check(orc, eng, mpo, c, forward, 1)  # structured, and within TOL of the oracle
        took = eng.counters()["n_env_reuse"] - n0
        assert took == (want_reuse if reuse is None else 0), (reuse, took)
        blocks.append(eng.get_env(0, c + 1) if forward else eng.get_env(1, c))
        eng.close()
    r = rel(blocks[0], blocks[1])
    print(f"{structure} {'->' if forward else '<-'}: reuse {want_reuse}, against the update without it {r:.3e}")
    assert r < TOL_OFF


@pytest.mark.parametrize("mode", ["3m", "4m"])
@pytest.mark.parametrize("forward", [True, False], ids=["forward", "backward"])
@pytest.mark.parametrize("structure", ["plain", "weighted", "zero", "both", "sum2"])
def test_structures_take_the_path_the_host_twin_decides(structure, forward, mode):
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import engine as E

    (dl, d, dr, M), bonds, c, level = SHAPES["partial_tiles"]
    mpo, want = em.structure(structure, len(bonds) - 1, d, M, c)
    decision = er.decide(mpo[c], want["S"], want["E"])[0 if forward else 1]["reuse"]
    assert level == 2
    E.set_gemm_mode(mode)
    try:
        _solve_update_pair(orc, mpo, d, bonds, c, forward, structure, int(decision))
    finally:
        E.set_gemm_mode("3m")


@pytest.mark.parametrize("forward", [True, False], ids=["forward", "backward"])
@pytest.mark.parametrize("name", ["dl_differs_from_dr", "even_only_takes_one_level", "odd_has_no_level"])
def test_shapes(name, forward):
    """dl != dr; a side that only takes one level (seven half-size factors reused); a side with odd sizes, which packs
    nothing and so reuses nothing"""
    from oracle import tdvp_oracle as orc

    (dl, d, dr, M), bonds, c, level = SHAPES[name]
    mpo, _ = em.structure("plain", len(bonds) - 1, d, M, c)
    _solve_update_pair(orc, mpo, d, bonds, c, forward, "plain", 1 if level else 0)


def test_a_stale_record_gets_no_reuse():
    """The record belongs to one solve: the update behind a check at site c reuses its factors; the update at c + 1,
    reached without a check there, finds no record (the factors in str_l_ are those of site c's operator) and builds its
    own -- and is right.  A check whose engine then moves away and back is not kept either."""
    from oracle import tdvp_oracle as orc
    from helpers.fold_seam import split

    d, M, bonds, c = 4, 10, [1, 4, 16, 40, 40, 40, 16, 4, 1], 3
    mpo, _ = em.structure("plain", 8, d, M, c)
    eng = _engine_at(mpo, d, bonds, c, _vars())
    eng.heff_apply_center()
    got, ref = split(orc, eng, mpo, c, True)
    k = eng.counters()
    assert (k["n_env_fold"], k["n_env_reuse"]) == (1, 1) and rel(got, ref) < TOL
    eng.absorb_bond(True)
    got, ref = split(orc, eng, mpo, c + 1, True)  # 40 x 4 x 40 again: only the record tells the two operators apart
    k = eng.counters()
    assert (k["n_env_fold"], k["n_env_reuse"]) == (1, 1)
    r = rel(got, ref)
    print(f"update behind a stale record: rel err {r:.3e}")
    assert r < TOL
    # back to site c + 1 as the centre, a check there, then the update the other way: the R side's record, used once
    eng.absorb_bond(False)
    eng.heff_apply_center()
    got, ref = split(orc, eng, mpo, c + 1, False)
    k = eng.counters()
    assert (k["n_env_fold"], k["n_env_reuse"]) == (2, 2) and rel(got, ref) < TOL
    eng.absorb_bond(False)
    got, ref = split(orc, eng, mpo, c, False)  # no check at c since: nothing to reuse
    k = eng.counters()
    assert (k["n_env_fold"], k["n_env_reuse"]) == (2, 2) and rel(got, ref) < TOL
    eng.close()


@pytest.mark.parametrize("mode", ["3m", "4m"])
@pytest.mark.parametrize("name", ["partial_tiles", "dl_differs_from_dr"])
def test_fused_pack_and_combine_are_the_two_passes_bit_for_bit(name, mode):
    """heff_apply_center at every level-2 shape with MITDVP_STRASSEN_FUSE unset and = 0: the centre tensor and a random
    vector; the L side's one-pass combine adds to what the R side wrote (the accumulate path).  The same bits."""
    from pytdscf_amd import engine as E

    (dl, d, dr, M), bonds, c, _ = SHAPES[name]
    mpo, _ = em.structure("plain", len(bonds) - 1, d, M, c)
    x = crandn(np.random.default_rng(41), dl, d, dr)
    E.set_gemm_mode(mode)
    try:
        outs = []
        for fuse in (None, "0"):
            eng = _engine_at(mpo, d, bonds, c, _vars(fuse=fuse))
            n0 = eng.counters()["n_launch"]
            a, flags = eng.heff_apply_center()
            launches = eng.counters()["n_launch"] - n0
            assert flags & 0x7F0 == 0x7F0, hex(flags)  # edge, both sides folded, two levels on both
            b, _ = eng.heff_apply_center(x)
            outs.append((a, b, launches))
            eng.close()
        assert outs[1][2] - outs[0][2] == 2  # two launches fewer on the L side; the R side keeps its two passes
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    finally:
        E.set_gemm_mode("3m")
