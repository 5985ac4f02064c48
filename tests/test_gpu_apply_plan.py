"""GPU: the form chosen for one local solve does not reach any other apply (csrc/engine_apply.hip: ApplyPlan is a value
choose_apply_forms returns to the solve that asked; every other caller of heff_apply gets the plain three-stage chain by
construction).

The shape is the smallest at which the edge form can be chosen: its rule needs both bonds of the site >= 32, so d = 2,
D = 32, and an edge-structured MPO of bond 4 (helpers/edge_mpo.py::fsm_mpo), on an engine created under
MITDVP_EDGE_APPLY=1 and MITDVP_FOLD_APPLY=1 (helpers/fold_seam.py::engine_under).  An open chain of four sites of d = 2
has no bond wider than 4, and the expectation value is taken with the centre on site 0 only; so the four sites are one
block of a longer chain (sites 8 .. 11 of 20: every bond 32, the outer ones included) between identity boundary blocks,
brought to the canonical form with the centre on ITS site 0.  There the probe mitdvp_heff_apply_center takes the edge
form, and the apply inside mitdvp_expect runs between blocks of the same size: an apply a stale form would have reached.
(The unit-level mitdvp_heff_apply runs on an engine of its own; it is checked for its value only.)

Tolerance of the unit-level apply: 1e-12 relative in the max norm, as tests/test_gpu_kernels.py.  Everything else is
exact: counters are integers, and the same launches on the same data give the same bits.
"""

import numpy as np
import pytest

from helpers.edge_mpo import fsm_mpo
from helpers.fold_seam import EDGE, crandn, engine_under

pytestmark = pytest.mark.gpu

L, d, D, M = 4, 2, 32, 4


def _block():
    eng = engine_under(L, {"MITDVP_EDGE_APPLY": "1", "MITDVP_FOLD_APPLY": "1"})
    eng.set_mpo(fsm_mpo(L, d, M, seed=0))
    eng.init_random_block([d] * 20, 8, D, seed=1)
    one = np.eye(D, dtype=np.complex128).reshape(D, 1, D)
    eng.set_boundary_env(0, one)
    eng.set_boundary_env(1, one)
    eng.set_bond(L, np.eye(D, dtype=np.complex128))
    eng.absorb_bond(False)
    for _ in range(L - 1):
        eng.split_center(False)
        eng.absorb_bond(False)
    assert eng.get_site_shape(0)[:3] == (D, d, D)
    eng.replace_site(0, eng.get_site(0) / eng.norm(), "Psi")  # the raw block is not normalised; the local solves assume it
    return eng


def _probe(eng):
    """step 2: one apply as a local solve issues it; the edge form was taken, by exactly that one apply"""
    n0 = eng.counters()["n_heff_edge"]
    _, flags = eng.heff_apply_center()
    assert flags & EDGE, hex(flags)
    assert eng.counters()["n_heff_edge"] - n0 == 1


def _unit_level_apply(rng):
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import engine as E

    Lb, Rb = crandn(rng, D, M, D), crandn(rng, D, M, D)
    W, psi = crandn(rng, M, d, d, M), crandn(rng, D, d, D)
    ref = orc.heff_apply(Lb, W, Rb, psi)
    out = E.heff_apply(Lb, W, Rb, psi)
    assert np.abs(out - ref).max() < 1e-12 * np.abs(ref).max()


def test_a_probes_form_stays_with_the_probe():
    eng = _block()
    e1 = eng.expectation()  # step 1
    _probe(eng)  # step 2
    n2 = eng.counters()["n_heff_edge"]
    e3 = eng.expectation()  # step 3
    _unit_level_apply(np.random.default_rng(21))
    assert eng.counters()["n_heff_edge"] == n2
    assert e3 == e1  # bit for bit
    eng.close()


def test_with_a_sweep_step_between():
    """The same with a forward sweep_part of one site between steps 2 and 3: the site solve makes its own plan, its
    environment update takes the identity sets that plan left away (the MPO bond it consumes is 1, so by the rule of
    env_fold_ok it runs the chain), the bond solve gets no compact form (keff_prepare declines below D = 256) and runs
    the plain K_eff applies.  The step moves the state and the centre, so the centre is brought back (split_center /
    absorb_bond) and step 3 is compared with a twin engine that ran the same calls WITHOUT the probe: the probe's form
    and its identity sets must not have reached the solve, the update or the expectation value."""
    got = {}
    for probe in (True, False):
        eng = _block()
        e1 = eng.expectation()
        if probe:
            _probe(eng)
        c2 = eng.counters()
        assert eng.sweep_part(0.05, True, 1) == L - 1
        c3 = eng.counters()
        # every apply of the site solve took the form of its own plan, none of the bond solve's did
        assert c3["n_heff_edge"] - c2["n_heff_edge"] == c3["n_heff"] - c2["n_heff"] > 0
        eng.split_center(False)
        eng.absorb_bond(False)
        n3 = eng.counters()["n_heff_edge"]
        e3 = eng.expectation()
        _unit_level_apply(np.random.default_rng(22))
        assert eng.counters()["n_heff_edge"] == n3
        got[probe] = (e1, e3, c3["n_heff"] - c2["n_heff"], c3["n_env_fold"] - c2["n_env_fold"], eng.get_mps())
        eng.close()
    a, b = got[True], got[False]
    assert a[:4] == b[:4]  # expectation values bit for bit, the same number of applies and structured updates
    assert all(np.array_equal(x, y) for x, y in zip(a[4], b[4]))
