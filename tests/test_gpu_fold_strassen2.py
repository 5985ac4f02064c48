"""GPU: a second Strassen level over the folded sides of the H_eff apply (csrc/engine_apply.hip::strassen_side with
ApplyPlan::strassen_r / strassen_l == 2): each of the seven half-size products of a folded side as seven quarter-size
products, 49 in one batched launch, the operator's 49 factors packed once per local solve from its seven.

MITDVP_FOLD_STRASSEN (read when the engine is created): 2 = two levels wherever a folded side's rows, columns and
contraction length are divisible by 4, one level where they are only even; 1 = exactly one level; 0 = never; unset = the
library's rule (the products must still fill the device: never at these sizes).  MITDVP_STRASSEN_BATCH=0 issues the 49
products as 49 launches.  mitdvp_heff_apply_center reports two levels in bits 0x200 (R side) and 0x400 (L side), set
together with 0x80 / 0x100.

Every case demands the bits as well as the numbers:
  * against the oracle's plain three-leg contraction (oracle/tdvp_oracle.py::heff_apply): 1e-12 relative in the max norm
    (TOL of helpers/fold_seam.py);
  * against the plain folded apply (MITDVP_FOLD_STRASSEN=0) of an engine taken through the same moves: 1e-13, the bar of
    one level.  On the host, with operators of this structure, two levels cost 1.5e-15 .. 2.0e-15 against one level's
    1.0e-15 .. 1.2e-15: about fifty times below the bar.

tests/test_strassen_levels_host.py proves the two-level plan itself on the host.
"""

import os

import numpy as np
import pytest

from helpers import edge_mpo as em
from helpers.fold_seam import EDGE, FOLD_L, FOLD_R, TOL, crandn, engine_under, rel, solve_update_check

pytestmark = pytest.mark.gpu

STR_R, STR_L, STR2_R, STR2_L = 0x80, 0x100, 0x200, 0x400
MASK = 0x7F0
FOLDED = EDGE | FOLD_R | FOLD_L
ONE = FOLDED | STR_R | STR_L
TWO = ONE | STR2_R | STR2_L
TOL_PLAIN = 1e-13


def _vars(strassen, batch=None):
    return {"MITDVP_FOLD_APPLY": "1", "MITDVP_FOLD_ENV": "1", "MITDVP_EDGE_APPLY": "1", "MITDVP_FOLD_STRASSEN": strassen,
            "MITDVP_STRASSEN_BATCH": batch}


def _pair_at(mpo, d, bonds, c, seed=1, variables=_vars, shift=0.0, **kw):
    """two engines on the same canonicalised random state with the bonds given, centre moved to site c: two levels
    asked for, and the form switched off"""
    L = len(bonds) - 1
    rng = np.random.default_rng(seed)
    cores = [crandn(rng, bonds[i], d, bonds[i + 1]) for i in range(L)]
    out = []
    for s in ("2", "0"):
        eng = engine_under(L, variables(s), **kw)
        eng.set_mpo(mpo, shift=shift)
        eng.set_mps([x.copy() for x in cores], canonicalize=True, scale=None if kw.get("conserve_norm") is False else 1.0)
        eng.build_envs(1)
        for _ in range(c):
            eng.split_center(True)
            eng.absorb_bond(True)
        assert eng.get_site_shape(c)[:3] == (bonds[c], d, bonds[c + 1])
        out.append(eng)
    return out


def _check(orc, on, off, mpo, c, x, want, shift=0.0):
    """one apply of vector x (None: the centre tensor) on both engines"""
    got, flags = on.heff_apply_center(x)
    ref0, flags0 = off.heff_apply_center(x)
    assert flags & MASK == want, hex(flags)
    assert flags0 & MASK == want & ~(STR_R | STR_L | STR2_R | STR2_L), hex(flags0)
    Lb, Rb = on.get_env(0, c), on.get_env(1, c + 1)
    psi = on.get_site(c) if x is None else x
    r_orc = rel(got, orc.heff_apply(Lb, mpo[c], Rb, psi) + shift * psi)
    r_plain = rel(got, ref0)
    print(f"site {c} shape {psi.shape} flags {flags:#x}: against the oracle {r_orc:.3e}, against the plain folded apply {r_plain:.3e}")
    assert r_orc < TOL
    assert r_plain < TOL_PLAIN


# (dl, d, dr, M), bonds of the chain, centre, flags wanted
SHAPES = {
    "flagship_instantiation": ((64, 16, 64, 32), [1, 16, 64, 64, 16, 1], 2, TWO),                # quarters 256 and 16
    "partial_tiles": ((40, 4, 40, 10), [1, 4, 16, 40, 40, 16, 4, 1], 3, TWO),                    # quarters 40 and 10
    "k_quarter_no_multiple_of_16": ((36, 3, 36, 10), [1, 3, 9, 27, 36, 36, 27, 9, 3, 1], 4, TWO),  # quarters 27 and 9
    "dl_differs_from_dr": ((48, 4, 32, 10), [1, 4, 16, 48, 32, 16, 4, 1], 3, TWO),
    "even_only_takes_one_level": ((34, 3, 34, 10), [1, 3, 9, 27, 34, 34, 27, 9, 3, 1], 4, ONE),
    "odd_is_refused": ((33, 3, 33, 10), [1, 3, 9, 27, 33, 33, 27, 9, 3, 1], 4, FOLDED),
}


@pytest.mark.parametrize("launch", ["batched", "separate"])
@pytest.mark.parametrize("mode", ["3m", "4m"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_against_the_oracle_and_the_plain_fold(name, mode, launch):
    """both complex-product forms; the 49 products as one batched launch (the default) and as 49 launches; the centre
    tensor and a random vector"""
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import engine as E

    (dl, d, dr, M), bonds, c, want = SHAPES[name]
    assert (bonds[c], bonds[c + 1]) == (dl, dr)
    mpo, _ = em.structure("plain", len(bonds) - 1, d, M, c)
    rng = np.random.default_rng(31)
    E.set_gemm_mode(mode)
    try:
        on, off = _pair_at(mpo, d, bonds, c, variables=lambda s: _vars(s, None if launch == "batched" else "0"))
        _check(orc, on, off, mpo, c, None, want)
        _check(orc, on, off, mpo, c, crandn(rng, dl, d, dr), want)
        on.close(); off.close()
    finally:
        E.set_gemm_mode("3m")


def _uneven_fsm(L, d, Ms, seed=0):
    """a finite-state-machine MPO with Ms[b] states on bond b (Ms[0] = Ms[L] = 1): state 0 nothing yet, the last state
    done, the states between one operator placed on the site before; a sum of on-site and nearest-neighbour terms"""
    rng = np.random.default_rng(seed)

    def herm(scale):
        G = crandn(rng, d, d)
        return scale * (G + G.conj().T) / 2

    cores = []
    for p in range(L):
        ml, mr = Ms[p], Ms[p + 1]
        W = np.zeros((ml, d, d, mr), dtype=np.complex128)
        if p != L - 1:
            W[0, :, :, 0] = np.eye(d)
            for k in range(1, mr - 1):
                W[0, :, :, k] = herm(0.01)
        if p != 0:
            W[ml - 1, :, :, mr - 1] = np.eye(d)
            for k in range(1, ml - 1):
                W[k, :, :, mr - 1] = herm(0.01)
        W[0, :, :, mr - 1] += herm(0.05)
        cores.append(W)
    return cores


@pytest.mark.parametrize("side", ["R", "L"])
def test_only_one_side_folded(side):
    """d = 8 at a 64 x 8 x 64 site whose MPO bonds are 8 and 16 wide, MITDVP_FOLD_APPLY unset: the library's rule folds
    only the side whose bond exceeds d.  That side takes two levels; the other runs the reducing epilogue, before (L side
    folded: the last combining pass adds to what it wrote) or after it (R side folded: that pass writes)."""
    from oracle import tdvp_oracle as orc

    d, bonds, c = 8, [1, 8, 64, 64, 8, 1], 2
    Ms = [1, 8, 8, 16, 16, 1] if side == "R" else [1, 16, 16, 8, 8, 1]
    mpo = _uneven_fsm(5, d, Ms)
    want = EDGE | (FOLD_R | STR_R | STR2_R if side == "R" else FOLD_L | STR_L | STR2_L)
    rng = np.random.default_rng(32)
    on, off = _pair_at(mpo, d, bonds, c, variables=lambda s: dict(_vars(s), MITDVP_FOLD_APPLY=None))
    _check(orc, on, off, mpo, c, None, want)
    _check(orc, on, off, mpo, c, crandn(rng, 64, d, 64), want)
    on.close(); off.close()


def test_weighted_identities_with_a_shift():
    """complex multiples of the identity in the blocks, folded into the operators, and a shift of 0.4 - 0.2i, which is
    added after the last combining pass"""
    from oracle import tdvp_oracle as orc

    d, M, bonds, c, shift = 4, 12, [1, 4, 16, 40, 40, 16, 4, 1], 3, 0.4 - 0.2j
    mpo, _ = em.structure("weighted", 7, d, M, c)
    rng = np.random.default_rng(33)
    on, off = _pair_at(mpo, d, bonds, c, shift=shift, integrator="arnoldi", conserve_norm=False)
    _check(orc, on, off, mpo, c, None, TWO, shift)
    _check(orc, on, off, mpo, c, crandn(rng, 40, d, 40), TWO, shift)
    on.close(); off.close()


def test_operands_follow_the_site():
    """Apply at site p (32 x 4 x 40), at site p + 1 (40 x 4 x 48: every buffer of the form grows, the 49 factors are
    packed again from other operators), at p again: each equals its own plain result."""
    from oracle import tdvp_oracle as orc

    d, M, bonds, p = 4, 10, [1, 4, 16, 32, 40, 48, 16, 4, 1], 3
    mpo, _ = em.structure("plain", 8, d, M, p)
    rng = np.random.default_rng(35)
    on, off = _pair_at(mpo, d, bonds, p)
    x_p, x_q = crandn(rng, 32, d, 40), crandn(rng, 40, d, 48)
    _check(orc, on, off, mpo, p, x_p, TWO)
    for e in (on, off):
        e.split_center(True)
        e.absorb_bond(True)
    _check(orc, on, off, mpo, p + 1, x_q, TWO)
    for e in (on, off):
        e.split_center(False)
        e.absorb_bond(False)
    _check(orc, on, off, mpo, p, x_p, TWO)
    _check(orc, on, off, mpo, p, None, TWO)
    on.close(); off.close()


def test_two_solves_in_a_row():
    """A local solve with two levels at a 32 x 4 x 40 site, the QR split with the structured environment update (which
    reuses X_ / Y_), the bond matrix into the next, larger site (40 x 4 x 48), the next solve: the updates against the
    oracle, the solved tensors against those of the plain folded apply to 1e-11 (at most 20 applies of a unit vector at
    1e-13 each, and exp(-i H dt) is unitary)."""
    from oracle import tdvp_oracle as orc

    d, M, bonds, c = 4, 10, [1, 4, 16, 32, 40, 48, 16, 4, 1], 3
    mpo, _ = em.structure("plain", 8, d, M, c)
    on, off = _pair_at(mpo, d, bonds, c)
    for site in (c, c + 1):
        _, flags = on.heff_apply_center()
        assert flags & MASK == TWO, hex(flags)
        solve_update_check(orc, on, mpo, site, True, 1)
        solve_update_check(orc, off, mpo, site, True, 1)
        r = rel(on.get_site(site), off.get_site(site))
        print(f"solved site {site}: forms differ by {r:.3e}")
        assert r < 1e-11
        for e in (on, off):
            e.absorb_bond(True)
    on.close(); off.close()


def _two_steps(orc, L, d, D, M, want_trace, capfd):
    """two time steps with MITDVP_FOLD_STRASSEN=2 against OracleMPS: equal Krylov counts; energy, autocorrelation,
    fidelity and norm to 1e-12"""
    dt = 1.0
    mpo = em.fsm_mpo(L, d, M, seed=0)
    mps = orc.synthetic_mps([d] * L, D, seed=1)
    eng = engine_under(L, _vars("2"))
    eng.set_mpo(mpo)
    eng.set_mps(mps)
    ref = orc.OracleMPS([c.copy() for c in mps], mpo)
    old = os.environ.get("MITDVP_EDGE_TRACE")
    os.environ["MITDVP_EDGE_TRACE"] = "1"
    try:
        for step in range(2):
            eng.propagate(dt)
            ref.propagate(dt)
            err = capfd.readouterr().err
            assert want_trace in err, step
            assert eng.krylov_stats() == [ref.kprev[i] for i in range(L)], step
            eg, er = eng.expectation(), ref.expectation()
            ag, ar = eng.autocorr(), ref.autocorr()
            fid = abs(orc.overlap(ref.cores, eng.get_mps()))
            print(f"step {step}: energy {abs(eg - er) / abs(er):.3e} autocorr {abs(ag - ar) / abs(ar):.3e} "
                  f"fidelity-1 {abs(fid - 1):.3e} norm-1 {abs(eng.norm() - 1):.3e}")
            assert abs(eg - er) < 1e-12 * abs(er) and abs(ag - ar) < 1e-12 * abs(ar), step
            assert abs(eng.norm() - 1) < 1e-12
            assert abs(fid - 1) < 1e-12, step
    finally:
        if old is None:
            os.environ.pop("MITDVP_EDGE_TRACE", None)
        else:
            os.environ["MITDVP_EDGE_TRACE"] = old
    eng.close()


def test_two_time_steps_with_two_levels(capfd):
    """The chain d = 4, M = 10, D = 40, L = 8: its 40 x 4 x 40 sites run 49 quarter-size products on both sides."""
    from oracle import tdvp_oracle as orc

    _two_steps(orc, 8, 4, 40, 10, "R 49 quarter-size products, L 49 quarter-size products", capfd)


def test_two_time_steps_of_the_ragged_chain(capfd):
    """The ragged chain d = 5, M = 17, D = 40, L = 8 (bonds 1, 5, 25, 40, 40, 40, 25, 5, 1) of
    tests/test_gpu_fold_range.py: its short sites take no edge form at all, its 40 x 5 x 40 sites (rows 40 and 200, all
    divisible by 4) run two levels on both sides; nothing regresses against OracleMPS."""
    from oracle import tdvp_oracle as orc

    _two_steps(orc, 8, 5, 40, 17, "R 49 quarter-size products, L 49 quarter-size products", capfd)


def test_default_rule_stays_off_at_small_sizes():
    """MITDVP_FOLD_STRASSEN unset at 64 x 16 x 64 and at 40 x 4 x 40 (far fewer than 256 tiles per product): both sides
    folded, no Strassen bit."""
    for d, M, bonds, c in ((16, 32, [1, 16, 64, 64, 16, 1], 2), (4, 10, [1, 4, 16, 40, 40, 16, 4, 1], 3)):
        mpo, _ = em.structure("plain", len(bonds) - 1, d, M, c)
        on, off = _pair_at(mpo, d, bonds, c, variables=lambda s: _vars(None if s == "2" else "0"))
        _, flags = on.heff_apply_center()
        assert flags & MASK == FOLDED, hex(flags)
        on.close(); off.close()
