"""CPU: the launch planner and the LDS carve of the one-launch small-bond kernel (csrc/small_chain_plan.h, compiled with
g++ into a throw-away shim) against an independent statement of both (tests/helpers/small_plan.py).

The planner decides whether the grid of k_small_site stays resident and the carve whether its LDS regions overlap; both
are integer arithmetic that no GPU test can see fail except as a wrong number or a hang.  Here: every plan of a sweep over
the three chain kinds is a valid launch layout, every refusal is one an exhaustive search confirms, every region of the
carve is disjoint from the others and long enough for what the kernel indexes, the plans of the benchmark's small shapes
are pinned, and two deliberately broken copies of the header are caught."""

import itertools

import numpy as np
import pytest

from helpers import small_plan as sp

N_CU = (8, 16, 32, 64, 128, 256)
BONDS = (1, 2, 3, 4, 5, 7, 8, 11, 13, 16, 17, 23, 25, 27, 31, 32, 33, 37, 41, 47, 53, 61, 64)


def _shapes(kind):
    """every pair of bond dimensions of BONDS, with d in 2..10 and the MPO bonds in 1..7 walked through beside them (a
    fixed walk, coprime strides: every value meets small and large bonds)"""
    out = []
    for n, (a, b) in enumerate(itertools.product(BONDS, BONDS)):
        d, m1, m2 = 2 + n % 9, 1 + (3 * n) % 7, 1 + (5 * n + 2) % 7
        if kind == "heff":
            out.append((a, d, b, m1, m2))
        elif kind == "keff":
            out.append((a, b, m1))
        else:
            out.append((a, m1, d, b, m2))
    return out


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return sp.Shim(tmp_path_factory.mktemp("ssp_shim"))


def test_the_constants_the_reference_statement_assumes(shim):
    assert (shim.MAXG, shim.MAXK, shim.PAYMAX, shim.LDS_PLAN) == (256, 21, 44, sp.LDS_CAP)
    assert shim.THREADS in (512, 1024) and shim.WAVES == shim.THREADS // 64


@pytest.mark.parametrize("kind", ["heff", "keff", "env"])
def test_extents_are_those_of_the_contraction(shim, kind):
    for dims in _shapes(kind)[::7]:
        assert shim.extents(kind, dims) == sp.extents(kind, dims), (kind, dims)


def _carve_defects(shim, kind, dims, exp_mode, plan):
    """the carve under a plan against what the kernel indexes: regions long enough, disjoint, inside the total"""
    e = sp.extents(kind, dims)
    need = sp.lds_regions(e, plan, exp_mode, shim.THREADS, shim.MAXK)
    off = shim.carve(kind, dims, exp_mode, plan)
    bad = []
    spans = {k: (off[k], off[k] + n) for k, n in need.items() if n > 0}
    for k, (lo, hi) in spans.items():
        if hi > off["total"]:
            bad.append(f"{k} ends at {hi}, past the total {off['total']}")
    alias = off["Sg"] == off["Xs"]
    if alias != bool(sp.sg_may_alias_x(e, plan)):
        bad.append(f"Sg {'aliases' if alias else 'does not alias'} X")
    for (k1, (a0, a1)), (k2, (b0, b1)) in itertools.combinations(spans.items(), 2):
        if {k1, k2} == {"Sg", "Xs"} and alias and sp.sg_may_alias_x(e, plan):
            continue  # the one permitted overlap: identical start, Sg no longer than X
        if a0 < b1 and b0 < a1:
            bad.append(f"{k1} [{a0}, {a1}) overlaps {k2} [{b0}, {b1})")
    return bad, off["total"] * sp.ZC


def _sweep_defects(shim, kind, stop_at=None):
    """(number of plans, number of refusals, defects) over the sweep of one chain kind"""
    nplan = nref = 0
    bad = []
    for dims in _shapes(kind):
        e = sp.extents(kind, dims)
        for exp_mode in (False, True):
            for n_cu in N_CU:
                plan = shim.plan(kind, dims, exp_mode, n_cu)
                where = f"{kind} {dims} {'EXP' if exp_mode else 'APPLY'} n_cu {n_cu}"
                if plan is None:
                    nref += 1
                    # the carve may round its block of scalars up by a few elements: an admissible plan within 16
                    # elements of the cap is not held against a refusal
                    other = [p for p in sp.search(e, exp_mode, n_cu, shim.THREADS, shim.MAXK)
                             if sp.lds_bytes(e, p, exp_mode, shim.THREADS, shim.MAXK) <= sp.LDS_CAP - 16 * sp.ZC]
                    if other:
                        bad.append(f"{where}: refused, but {other[0]} is admissible")
                    continue
                nplan += 1
                defects = sp.plan_defects(e, plan, n_cu)
                cbad, lds = _carve_defects(shim, kind, dims, exp_mode, plan)
                if lds > sp.LDS_CAP:
                    defects.append(f"{lds} bytes of LDS")
                bad += [f"{where}: plan {plan}: {w}" for w in defects + cbad]
                if stop_at and len(bad) >= stop_at:
                    return nplan, nref, bad
    return nplan, nref, bad


@pytest.mark.parametrize("kind", ["heff", "keff", "env"])
def test_every_plan_is_a_launch_layout_and_every_refusal_is_forced(shim, kind):
    nplan, nref, bad = _sweep_defects(shim, kind)
    print(f"{kind}: {nplan} plans, {nref} refusals")
    assert nplan > 2000 and nref >= 10  # the sweep reaches both sides (bond matrices up to 64 x 64 are seldom refused)
    assert not bad, bad[:10]


def test_the_sweep_reaches_every_regime(shim):
    """ragged chunks, short last groups, re-staged A, both Sg placements: the regimes the invariants are about occur"""
    seen = set()
    for kind in ("heff", "keff", "env"):
        for dims in _shapes(kind):
            e = sp.extents(kind, dims)
            for n_cu in N_CU:
                p = shim.plan(kind, dims, False, n_cu)
                if p is None:
                    continue
                nsc, cs, spw, res = p
                seen.add(("nsc", nsc))
                if nsc * cs > e["ns"]:
                    seen.add("ragged chunk")
                if spw > 1:
                    seen.add("resident" if res else "re-staged")
                    if e["na"] % spw:
                        seen.add("short group")
                    if nsc * cs > e["ns"] and e["na"] % spw:
                        seen.add("short group and ragged chunk")
                seen.add("Sg aliases X" if sp.sg_may_alias_x(e, p) else ("Sg apart, W" if e["w"] else "Sg apart, no W"))
    want = {("nsc", 1), ("nsc", 2), ("nsc", 4), ("nsc", 8), "ragged chunk", "resident", "re-staged", "short group",
            "short group and ragged chunk", "Sg aliases X", "Sg apart, W", "Sg apart, no W"}
    assert want <= seen, want - seen


def test_degenerate_chains_are_refused(shim):
    for kind, dims in (("heff", (0, 4, 8, 3, 3)), ("heff", (8, 4, 0, 3, 3)), ("keff", (0, 8, 3)), ("keff", (8, 0, 3)),
                       ("env", (0, 3, 4, 8, 3)), ("env", (8, 3, 4, 0, 3))):
        for n_cu in N_CU:
            assert shim.plan(kind, dims, False, n_cu) is None, (kind, dims)


# ---- the plans of the benchmark's small shapes, pinned: a planner change shows up here as a diff ----
# H_eff (32, 10, 32, 6, 6) with the K_eff chain of its bonds and its environment update; per compute units 256 .. 8:
# (nsc, cs, spw, a_resident) in APPLY mode, then in EXP mode
# (the engine plans environment updates in APPLY mode only; the EXP column of "env" pins the arithmetic all the same)
PINNED = {
    "heff": ((32, 10, 32, 6, 6), {
        256: ((4, 8, 1, 1), (4, 8, 1, 1)), 128: ((4, 8, 1, 1), (4, 8, 1, 1)), 64: ((4, 8, 2, 1), (4, 8, 2, 1)),
        32: ((4, 8, 4, 0), (4, 8, 4, 0)), 16: ((4, 8, 8, 0), (4, 8, 8, 0)), 8: ((4, 8, 16, 0), (4, 8, 16, 0))}),
    "keff": ((32, 32, 6), {
        256: ((1, 32, 1, 1), (2, 16, 1, 1)), 128: ((1, 32, 1, 1), (2, 16, 1, 1)), 64: ((1, 32, 1, 1), (2, 16, 1, 1)),
        32: ((1, 32, 1, 1), (2, 16, 2, 1)), 16: ((1, 32, 2, 1), (2, 16, 4, 1)), 8: ((1, 32, 4, 1), (2, 16, 8, 1))}),
    "env": ((32, 6, 10, 32, 6), {
        256: ((4, 8, 1, 1), (8, 4, 1, 1)), 128: ((4, 8, 1, 1), None), 64: ((4, 8, 2, 0), (8, 4, 4, 0)),
        32: ((4, 8, 4, 0), (8, 4, 8, 0)), 16: ((4, 8, 8, 0), (8, 4, 16, 0)), 8: ((4, 8, 16, 0), (8, 4, 32, 0))}),
}


def test_pinned_plans_of_the_benchmark_shapes(shim):
    got = {k: {n: (shim.plan(k, dims, False, n), shim.plan(k, dims, True, n)) for n in N_CU} for k, (dims, _) in PINNED.items()}
    for k, (dims, table) in PINNED.items():
        print(k, dims, got[k])
        assert got[k] == table, (k, dims)


def test_the_library_plans_as_the_header_does(shim):
    """mitdvp_small_plan (host arithmetic inside the built library, chains built by the engine's own code) against the shim"""
    from pytdscf_amd import engine as E

    for kind, (dims, _) in PINNED.items():
        for more in (dims, tuple(max(1, x - 3) for x in dims), tuple(x + 5 for x in dims)):
            for exp_mode in (False, True):
                for n_cu in N_CU:
                    p = E.small_plan(kind, more, exp_mode, n_cu)
                    s = shim.plan(kind, more, exp_mode, n_cu)
                    if s is None:
                        assert p["ok"] == 0, (kind, more, n_cu)
                        continue
                    e = sp.extents(kind, more)
                    off = shim.carve(kind, more, exp_mode, s)
                    assert (p["ok"], p["nsc"], p["cs"], p["spw"], p["a_resident"]) == (1,) + s, (kind, more, n_cu)
                    assert p["grid"] == sp.grid_of(e, s) and p["lds_bytes"] == off["total"] * sp.ZC
                    assert p["sg_aliases_x"] == int(off["Sg"] == off["Xs"])
    with pytest.raises(ValueError):
        E.small_plan("heff", (0, 4, 8, 3, 3), False, 256)


def test_the_gpu_cases_are_planned_into_the_regimes_they_are_named_after():
    """tests/test_gpu_small_chain.py asserts this again from what the library launched; here without a GPU, so that a
    planner change that moves a case shows up before a GPU run (the whole chip is taken as 256 compute units)"""
    from helpers import small_chain_cases as sc
    from pytdscf_amd import engine as E

    named = []
    for case in sc.APPLY_CASES:
        p = E.small_plan(case.kind, case.dims, False, case.n_cu)
        assert p["ok"] and (p["nsc"], p["cs"], p["spw"], p["a_resident"]) == case.plan, (case.id, p)
        ran = sc.regime_of(case.kind, case.dims, p)
        assert case.regime <= ran, (case.id, case.regime - ran)
        named.append(case.regime)
    for need in sc.REQUIRED:
        assert any(need <= r for r in named), need
    assert any(c.shift and "spw" in c.regime for c in sc.APPLY_CASES) and any(c.shift and c.plan[0] > 1 for c in sc.APPLY_CASES)
    assert any(c.kind == "keff" and c.dims[0] != c.dims[1] and not c.shift for c in sc.APPLY_CASES)
    assert {(c.left) for c in sc.APPLY_CASES if c.kind == "env"} == {True, False}
    assert any(c.kind == "env" and "sg_apart" in c.regime for c in sc.APPLY_CASES)  # a W stage whose Sg is not in X
    assert any(c.kind != "heff" and "restaged" in c.regime for c in sc.APPLY_CASES)
    for case in sc.EXP_SITE + sc.EXP_BOND:
        for cu, plan, regime in case.slices:
            p = E.small_plan(case.kind, case.chain_dims, True, cu or 256)
            assert p["ok"] and (p["nsc"], p["cs"], p["spw"], p["a_resident"]) == plan, (case.id, cu, p)
            assert set(regime) <= sc.regime_of(case.kind, case.chain_dims, p), (case.id, cu)


def test_the_references_of_the_gpu_cases_are_the_oracles():
    """the extended-precision einsum formulas against the oracle's functions at complex128, every APPLY case"""
    from helpers import small_chain_cases as sc

    for case in sc.APPLY_CASES:
        ops = sc.operands(case)
        ref, orc = sc.reference(case, ops, np.complex128), sc.oracle(case, ops)
        assert ref.shape == orc.shape and np.abs(ref - orc).max() < 1e-13 * np.abs(orc).max(), case.id


def _exp_cases():
    from helpers import small_chain_cases as sc

    return [(c, i) for c in sc.EXP_BOND + sc.EXP_SITE for i in c.configs]


@pytest.mark.parametrize("case, cfg_id", _exp_cases(), ids=[f"{c.id}-{i}" for c, i in _exp_cases()])
def test_the_exp_cases_may_be_held_to_the_parity_bar(case, cfg_id):
    """lx.PARITY was established at n = 256.  At the shapes of tests/test_gpu_small_chain.py: the reference's two chained
    solves are well separated from the placed threshold, and the reference with its matvec in np.clongdouble lands within
    PARITY / 10 of the one in complex128 with the same Krylov counts -- or the reference does not converge, which the GPU
    case then asks of the kernel in the same words (one site configuration)."""
    from helpers import local_exp as lx
    from helpers import small_chain_cases as sc

    e = sc.eligibility(case, sc.exp_config(cfg_id))
    print(e)
    if e["raises"]:
        assert case.kind == "heff" and cfg_id == "lanczos-reference-shift100-relax" and "not converged" in e["raises"]
        return
    assert e["separated"], e["margins"]
    assert e["k"] == e["k_ld"]
    assert e["precision"] <= lx.PARITY / 10


# ---- deliberately broken planners are caught ----
BROKEN = {
    "an empty last chunk is allowed": [("      if ((nsc - 1) * cs >= c.ns) continue;  // every chunk must be non-empty\n", ""),
                                       ("      if ((nsc - 1) * cs >= c.ns) continue;\n", "")],
    "As is carved for one slab whatever spw": [("(c.a_resident && c.spw > 1 ? c.spw : 1)", "1")],
}


@pytest.mark.parametrize("what", list(BROKEN))
def test_a_broken_planner_fails_the_sweep(tmp_path, what):
    with open(sp.HEADER) as f:
        text = f.read()
    for old, new in BROKEN[what]:
        assert old in text, f"the header no longer has the line this perturbation edits: {old!r}"
        text = text.replace(old, new)
    broken = tmp_path / "small_chain_plan_broken.h"
    broken.write_text(text)
    bad_shim = sp.Shim(tmp_path, header=str(broken))
    found = []
    for kind in ("heff", "keff", "env"):
        found += _sweep_defects(bad_shim, kind, stop_at=1)[2]
        if found:
            break
    print(what, "->", found[:3])
    assert found, f"{what}: the sweep noticed nothing"
    if "chunk" in what:
        assert any("last one is empty" in w for w in found)
    else:
        assert any("As [" in w and "overlaps" in w for w in found)
