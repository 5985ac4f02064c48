"""GPU: one Strassen level over the folded sides of the H_eff apply (csrc/engine_apply.hip::strassen_side with
ApplyPlan::strassen_r / strassen_l, csrc/vecops.hip::strassen_operands / strassen_combine): seven half-size products per
folded side instead of one full-size GEMM, the operator's seven factors packed once per local solve.

MITDVP_FOLD_STRASSEN (read when the engine is created): 1 = wherever a folded side has even rows, columns and contraction
length, 0 = never, unset = the library's rule (the half-size products must still fill the device: never at these sizes).
MITDVP_STRASSEN_BATCH=0 issues the seven products as seven launches instead of one batched launch.
mitdvp_heff_apply_center reports the form in bits 0x80 (R side) and 0x100 (L side) beside 0x10 / 0x20 / 0x40.

Every case demands the bits as well as the numbers:
  * against the oracle's plain three-leg contraction (oracle/tdvp_oracle.py::heff_apply): 1e-12 relative in the max norm,
    as tests/test_gpu_fold_apply.py;
  * against the plain folded apply (MITDVP_FOLD_STRASSEN=0) of an engine taken through the same moves: 1e-13.  One
    Strassen level costs a small multiple of the plain product's rounding (measured on the host with operators of this
    structure: 1.7 to 4.9 times 4e-16 .. 6e-16), three orders below this bar.

tests/test_strassen_blocks_host.py proves the block plan itself on the host.
"""

import os

import numpy as np
import pytest

from helpers import edge_mpo as em
from helpers.fold_seam import EDGE, FOLD_L, FOLD_R, TOL, crandn, engine_under, rel, solve_update_check

pytestmark = pytest.mark.gpu

STR_R, STR_L = 0x80, 0x100
MASK = 0x1F0
ALL = EDGE | FOLD_R | FOLD_L | STR_R | STR_L
TOL_PLAIN = 1e-13


def _vars(strassen, batch=None):
    """batch: MITDVP_STRASSEN_BATCH -- None / "1" the seven products as one batched launch, "0" as seven launches"""
    return {"MITDVP_FOLD_APPLY": "1", "MITDVP_FOLD_ENV": "1", "MITDVP_EDGE_APPLY": "1", "MITDVP_FOLD_STRASSEN": strassen,
            "MITDVP_STRASSEN_BATCH": batch}


def _random_cores(d, bonds, seed):
    rng = np.random.default_rng(seed)
    return [crandn(rng, bonds[i], d, bonds[i + 1]) for i in range(len(bonds) - 1)]


def _pair_at(mpo, d, bonds, c, seed=1, variables=_vars, shift=0.0, **kw):
    """two engines on the same canonicalised random state with the bonds given, centre moved to site c: the form forced,
    and switched off"""
    L = len(bonds) - 1
    cores = _random_cores(d, bonds, seed)
    out = []
    for s in ("1", "0"):
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
    assert flags0 & MASK == want & ~(STR_R | STR_L), hex(flags0)
    Lb, Rb = on.get_env(0, c), on.get_env(1, c + 1)
    psi = on.get_site(c) if x is None else x
    r_orc = rel(got, orc.heff_apply(Lb, mpo[c], Rb, psi) + shift * psi)
    r_plain = rel(got, ref0)
    print(f"site {c} shape {psi.shape} flags {flags:#x}: against the oracle {r_orc:.3e}, against the plain folded apply {r_plain:.3e}")
    assert r_orc < TOL
    assert r_plain < TOL_PLAIN


# (dl, d, dr, M), bonds of the chain, centre, flags wanted
SHAPES = {
    "flagship_instantiation": ((64, 16, 64, 32), [1, 16, 64, 64, 16, 1], 2, ALL),
    "partial_tiles": ((40, 4, 40, 10), [1, 4, 16, 40, 40, 16, 4, 1], 3, ALL),                # halves 80 and 20
    "k_no_multiple_of_16": ((34, 3, 34, 10), [1, 3, 9, 27, 34, 34, 27, 9, 3, 1], 4, ALL),    # halves 51 and 17
    "dl_differs_from_dr": ((48, 4, 32, 10), [1, 4, 16, 48, 32, 16, 4, 1], 3, ALL),
    "odd_is_refused": ((33, 3, 33, 10), [1, 3, 9, 27, 33, 33, 27, 9, 3, 1], 4, EDGE | FOLD_R | FOLD_L),
}


@pytest.mark.parametrize("launch", ["batched", "seven"])
@pytest.mark.parametrize("mode", ["3m", "4m"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_against_the_oracle_and_the_plain_fold(name, mode, launch):
    """both complex-product forms; the seven products as one batched launch (the default) and as seven launches"""
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import engine as E

    (dl, d, dr, M), bonds, c, want = SHAPES[name]
    assert (bonds[c], bonds[c + 1]) == (dl, dr)
    mpo, _ = em.structure("plain", len(bonds) - 1, d, M, c)
    rng = np.random.default_rng(21)
    E.set_gemm_mode(mode)
    try:
        on, off = _pair_at(mpo, d, bonds, c, variables=lambda s: _vars(s, None if launch == "batched" else "0"))
        _check(orc, on, off, mpo, c, None, want)
        _check(orc, on, off, mpo, c, crandn(rng, dl, d, dr), want)
        on.close(); off.close()
    finally:
        E.set_gemm_mode("3m")


def _uneven_fsm(L, d, Ms, seed=0):
    """fsm_mpo's machine with Ms[b] states on bond b (Ms[0] = Ms[L] = 1): state 0 nothing yet, the last state done, the
    states between one operator placed on the site before; a sum of on-site and nearest-neighbour terms"""
    rng = np.random.default_rng(seed)

    def herm(scale):
        G = crandn(rng, d, d)
        return scale * (G + G.conj().T) / 2

    cores = []
    for p in range(L):
        ml, mr = Ms[p], Ms[p + 1]
        W = np.zeros((ml, d, d, mr), dtype=np.complex128)
        first, last = p == 0, p == L - 1
        if not last:
            W[0, :, :, 0] = np.eye(d)
            for k in range(1, mr - 1):
                W[0, :, :, k] = herm(0.01)
        if not first:
            W[ml - 1, :, :, mr - 1] = np.eye(d)
            for k in range(1, ml - 1):
                W[k, :, :, mr - 1] = herm(0.01)
        W[0, :, :, mr - 1] += herm(0.05)
        cores.append(W)
    return cores


@pytest.mark.parametrize("side", ["R", "L"])
def test_only_one_side_folded(side):
    """d = 8 at a 64 x 8 x 64 site whose MPO bonds are 8 and 16 wide, MITDVP_FOLD_APPLY unset: the library's rule folds
    only the side whose bond exceeds d.  That side takes the seven products; the other runs the reducing epilogue, before
    (L side folded: the combining pass adds to it) or after it."""
    from oracle import tdvp_oracle as orc

    d, bonds, c = 8, [1, 8, 64, 64, 8, 1], 2
    Ms = [1, 8, 8, 16, 16, 1] if side == "R" else [1, 16, 16, 8, 8, 1]
    mpo = _uneven_fsm(5, d, Ms)
    want = EDGE | (FOLD_R | STR_R if side == "R" else FOLD_L | STR_L)
    rng = np.random.default_rng(22)
    on, off = _pair_at(mpo, d, bonds, c, variables=lambda s: dict(_vars(s), MITDVP_FOLD_APPLY=None))
    _check(orc, on, off, mpo, c, None, want)
    _check(orc, on, off, mpo, c, crandn(rng, 64, d, 64), want)
    on.close(); off.close()


def test_weighted_identities_with_a_shift():
    """W[0,:,:,0] = 0.9 exp(0.3i) 1 and W[M-1,:,:,M-1] = -0.8 1 (complex multiples of the identity in the blocks, folded
    into the operators) and a shift of 0.4 - 0.2i, which is added after the combining pass."""
    from oracle import tdvp_oracle as orc

    d, M, bonds, c, shift = 4, 12, [1, 4, 16, 40, 40, 16, 4, 1], 3, 0.4 - 0.2j
    mpo, _ = em.structure("weighted", 7, d, M, c)
    rng = np.random.default_rng(23)
    on, off = _pair_at(mpo, d, bonds, c, shift=shift, integrator="arnoldi", conserve_norm=False)
    _check(orc, on, off, mpo, c, None, ALL, shift)
    _check(orc, on, off, mpo, c, crandn(rng, 40, d, 40), ALL, shift)
    on.close(); off.close()


def test_liouville_generator():
    """H (x) 1 - 1 (x) H^T - i Gamma (M = 16, d = 4): the folded operators are not Hermitian."""
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import synthetic as syn

    L, bonds, c = 7, [1, 4, 16, 40, 40, 16, 4, 1], 3
    mpo = syn.synthetic_liouvillian_mpo(L, 16, seed=0, gamma=0.002)
    rng = np.random.default_rng(24)
    on, off = _pair_at(mpo, 4, bonds, c, integrator="arnoldi", conserve_norm=False)
    _check(orc, on, off, mpo, c, None, ALL)
    _check(orc, on, off, mpo, c, crandn(rng, 40, 4, 40), ALL)
    on.close(); off.close()


def test_operands_follow_the_site():
    """Apply at site p, at site q = p + 1 (other blocks, other operators, 40 x 4 x 48 after 32 x 4 x 40: every buffer of
    the form grows), at p again: the packed factors are rebuilt with the operators of every local solve, so each equals
    its own plain result."""
    from oracle import tdvp_oracle as orc

    d, M, bonds, p = 4, 10, [1, 4, 16, 32, 40, 48, 16, 4, 1], 3
    mpo, _ = em.structure("plain", 8, d, M, p)
    rng = np.random.default_rng(25)
    on, off = _pair_at(mpo, d, bonds, p)
    x_p, x_q = crandn(rng, 32, d, 40), crandn(rng, 40, d, 48)
    _check(orc, on, off, mpo, p, x_p, ALL)
    for e in (on, off):
        e.split_center(True)
        e.absorb_bond(True)
    _check(orc, on, off, mpo, p + 1, x_q, ALL)
    for e in (on, off):
        e.split_center(False)
        e.absorb_bond(False)
    _check(orc, on, off, mpo, p, x_p, ALL)
    _check(orc, on, off, mpo, p, None, ALL)
    on.close(); off.close()


def test_solve_update_next_solve():
    """A local solve with the form, the QR split with the structured environment update (which reuses X_ / Y_), the bond
    matrix into the next site, the next solve: the update against the oracle, the solved tensors against those of the
    plain folded apply to 1e-11 (at most 20 applies of a unit vector at 1e-13 each, and exp(-i H dt) is unitary)."""
    from oracle import tdvp_oracle as orc

    d, M, bonds, c = 4, 10, [1, 4, 16, 40, 40, 40, 16, 4, 1], 3
    mpo, _ = em.structure("plain", 8, d, M, c)
    rng = np.random.default_rng(26)
    on, off = _pair_at(mpo, d, bonds, c)
    solve_update_check(orc, on, mpo, c, True, 1)
    solve_update_check(orc, off, mpo, c, True, 1)
    r = rel(on.get_site(c), off.get_site(c))
    print(f"solved site {c}: forms differ by {r:.3e}")
    assert r < 1e-11
    for e in (on, off):
        e.absorb_bond(True)
    assert on.get_site_shape(c + 1)[:3] == (40, d, 40)
    got, flags = on.heff_apply_center()
    assert flags & MASK == ALL, hex(flags)
    Lb, Rb, psi = on.get_env(0, c + 1), on.get_env(1, c + 2), on.get_site(c + 1)
    assert rel(got, orc.heff_apply(Lb, mpo[c + 1], Rb, psi)) < TOL
    x = crandn(rng, 40, d, 40)
    got, _ = on.heff_apply_center(x)
    assert rel(got, orc.heff_apply(Lb, mpo[c + 1], Rb, x)) < TOL
    solve_update_check(orc, on, mpo, c + 1, True, 1)
    solve_update_check(orc, off, mpo, c + 1, True, 1)
    r = rel(on.get_site(c + 1), off.get_site(c + 1))
    print(f"solved site {c + 1}: forms differ by {r:.3e}")
    assert r < 1e-11
    on.close(); off.close()


def test_two_time_steps_against_the_oracle(capfd):
    """The ragged chain d = 4, M = 10, D = 40, L = 8 with every form forced, two time steps against OracleMPS at the bars
    of tests/test_gpu_fold_range.py: equal Krylov counts, energy / autocorrelation to 1e-8 relative, fidelity to 1e-10,
    norm to 1e-12.  MITDVP_EDGE_TRACE names the form of the local solves at the 40 x 4 x 40 sites."""
    from oracle import tdvp_oracle as orc

    L, d, D, M, dt = 8, 4, 40, 10, 1.0
    mpo = em.fsm_mpo(L, d, M, seed=0)
    mps = orc.synthetic_mps([d] * L, D, seed=1)
    eng = engine_under(L, _vars("1"))
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
            assert "R seven half-size products, L seven half-size products" in err, step
            assert eng.krylov_stats() == [ref.kprev[i] for i in range(L)], step
            eg, er = eng.expectation(), ref.expectation()
            ag, ar = eng.autocorr(), ref.autocorr()
            fid = abs(orc.overlap(ref.cores, eng.get_mps()))
            print(f"step {step}: energy {abs(eg - er) / abs(er):.3e} autocorr {abs(ag - ar) / abs(ar):.3e} "
                  f"fidelity-1 {abs(fid - 1):.3e} norm-1 {abs(eng.norm() - 1):.3e}")
            assert abs(eg - er) < 1e-8 * abs(er) and abs(ag - ar) < 1e-8 * abs(ar), step
            assert abs(eng.norm() - 1) < 1e-12
            assert abs(fid - 1) < 1e-10, step
    finally:
        if old is None:
            os.environ.pop("MITDVP_EDGE_TRACE", None)
        else:
            os.environ["MITDVP_EDGE_TRACE"] = old
    eng.close()


def test_default_rule_stays_off_at_small_sizes():
    """MITDVP_FOLD_STRASSEN unset at 64 x 16 x 64 (the half-size products are 16 tiles of 64 x 64): both sides folded,
    neither as seven products."""
    d, bonds, c = 16, [1, 16, 64, 64, 16, 1], 2
    mpo, _ = em.structure("plain", 5, d, 32, c)
    on, off = _pair_at(mpo, d, bonds, c, variables=lambda s: _vars(None if s == "1" else "0"))
    _, flags = on.heff_apply_center()
    assert flags & MASK == EDGE | FOLD_R | FOLD_L, hex(flags)
    on.close(); off.close()
