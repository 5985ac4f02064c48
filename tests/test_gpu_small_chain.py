"""GPU: the one-launch small-bond kernel (k_small_site, csrc/small_site.hip) under every launch plan.

The kernel's work layout is chosen at run time (csrc/small_chain_plan.h): chunks over the contracted right index with a
possibly narrower last chunk, several slabs per workgroup with a possibly short last group, A resident in LDS or re-staged
per slab, the chunk partial Sg inside X's LDS or apart.  Each case runs on an engine confined to a slice of the chip chosen
so that the planner lands in the regime the case is named after, and FIRST asserts, from what the library reports it
launched, that it did: a case that silently runs another plan fails.

a. APPLY mode (``engine.small_apply``: Engine::heff_apply / keff_apply / env_update on caller data) against the formulas
   of csrc/small_site.h evaluated with einsum in np.clongdouble; the bar is that of test_heff_keff_env_vs_numpy,
   max|out - ref| < 1e-12 max|ref|.  The oracle's functions are cross-checks of the reference at complex128.
b. EXP mode (the whole local Krylov exponential in one launch) against the statement-level references of
   helpers/local_exp.py, two consecutive solves each, on slices of 8, 16 and 64 compute units and on the whole chip.

Lines starting with "SC" are the record behind profiles/small_chain_tests.txt (run with -s)."""

import numpy as np
import pytest

from helpers import local_exp as lx
from helpers import small_chain_cases as sc

pytestmark = pytest.mark.gpu

APPLY_BAR = 1e-12


def _plan_tuple(p):
    return (p["nsc"], p["cs"], p["spw"], p["a_resident"])


def _device_cus():
    from pytdscf_amd import engine as E

    return E.device_cu_count(0)


# ---------------------------------------------------------------------------------------------------------------------
# a. APPLY
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.APPLY_CASES, ids=lambda c: c.id)
def test_apply(case):
    from pytdscf_amd import engine as E

    n_cu = case.cu or _device_cus()
    want = E.small_plan(case.kind, case.dims, False, n_cu)
    assert want["ok"] and _plan_tuple(want) == case.plan, (want, case.plan)  # the planner puts the case where it is named
    ops = sc.operands(case)
    ref = sc.reference(case, ops)
    orc = sc.oracle(case, ops)
    scale = float(np.abs(ref).max())
    assert np.abs(orc - ref).max() < APPLY_BAR * scale  # the formula above is the oracle's
    out, info = E.small_apply(case.kind, ops, shift=case.shift, cu_count=case.cu, left=case.left)
    # the regime that ran: one launch of the one-launch family, under the plan of the case
    assert info["n_launch"] == 1 and info["plan"]["ok"] == 1, info
    assert _plan_tuple(info["plan"]) == case.plan, info
    assert info["plan"] == want, (info, want)
    ran = sc.regime_of(case.kind, case.dims, info["plan"])
    assert case.regime <= ran, (case.regime - ran, ran)
    err = float(np.abs(out - ref).max())
    print(f"SC | apply | {case.id} | plan {case.plan} grid {info['plan']['grid']} lds {info['plan']['lds_bytes']} "
          f"{'Sg=X' if info['plan']['sg_aliases_x'] else 'Sg apart'} | max|out - ref| / max|ref| {err / scale:.2e} | "
          f"oracle against ref {np.abs(orc - ref).max() / scale:.2e}")
    assert out.shape == ref.shape and np.isfinite(out).all()
    assert err < APPLY_BAR * scale


def test_apply_refuses_what_the_engine_refuses():
    from pytdscf_amd import engine as E

    case = sc.APPLY_CASES[0]
    with pytest.raises(ValueError, match="multiple of 8"):
        E.small_apply(case.kind, sc.operands(case), cu_count=12)
    env = next(c for c in sc.APPLY_CASES if c.kind == "env")
    with pytest.raises(ValueError, match="no shift"):
        E.small_apply("env", sc.operands(env), shift=1.0, cu_count=env.cu, left=env.left)


# ---------------------------------------------------------------------------------------------------------------------
# b. EXP: the whole local exponential in one launch, on every slice, against the statement-level reference
# ---------------------------------------------------------------------------------------------------------------------
# lx.PARITY (1e-11, max norm) was established at n = 256.  For the shapes here (n = 1369 .. 7770) it was checked on the
# CPU before use (helpers.small_chain_cases.eligibility, recorded in profiles/small_chain_tests.txt): every case is
# ``well_separated`` -- asserted again below -- and the reference run with its matvec in np.clongdouble instead of
# complex128 lands within PARITY / 10 of itself with the same Krylov counts, so the bar is not spent on the reference.
def _slice_engine(sm, cu, **kw):
    from pytdscf_amd import TDVPEngine

    if cu:
        kw["cu_range"] = (0, cu)
    return sm.engine(TDVPEngine, small_kernels=True, **kw)


def _assert_exp_regime(case, cu, plan, regime):
    """the plan an engine on this slice gives the case's chain in EXP mode is the one the slice is listed for"""
    from pytdscf_amd import engine as E

    p = E.small_plan(case.kind, case.chain_dims, True, cu or _device_cus())
    assert p["ok"] and _plan_tuple(p) == plan, (case.id, cu, p)
    ran = sc.regime_of(case.kind, case.chain_dims, p)
    assert set(regime) <= ran, (case.id, cu, set(regime) - ran)
    return p


def _across_slices(what, got):
    """the same problem on every slice: equal Krylov counts, states within PARITY of each other"""
    (cu0, a1, ka1, a2, ka2) = got[0]
    worst = 0.0
    for cu, b1, kb1, b2, kb2 in got[1:]:
        assert (ka1, ka2) == (kb1, kb2), (what, cu0, cu)
        worst = max(worst, lx.err(a1, b1), lx.err(a2, b2))
    print(f"SC | exp | {what} | across slices {worst:.2e}")
    assert worst <= lx.PARITY, what


SITE = [(c, i) for c in sc.EXP_SITE for i in c.configs]


@pytest.mark.parametrize("case, cfg_id", SITE, ids=[f"{c.id}-{i}" for c, i in SITE])
def test_exp_site(case, cfg_id):
    import test_gpu_local_exp as tle

    cfg = sc.exp_config(cfg_id)
    r = lx.site_reference(case.shape, cfg, dense=False)
    sm = r.seam
    if not r.raises:
        assert lx.well_separated(r.d1, r.thresh) and lx.well_separated(r.d2, r.thresh), (r.d1, r.d2, r.thresh)
    got = []
    for cu, plan, regime in case.slices:
        p = _assert_exp_regime(case, cu, plan, regime)
        eng = _slice_engine(sm, cu, thresh=r.thresh, **cfg.engine_kw())
        try:
            assert eng.krylov_memory(0) == 0
            if r.raises:  # twenty vectors do not do: the kernel says so in the reference's words, under every plan
                tle._apply_launches(eng, True)
                with pytest.raises(ValueError) as dev_err:
                    eng.site_exp(cfg.dt)
                assert r.raises in str(dev_err.value), (r.raises, str(dev_err.value))
                print(f"SC | exp | {case.id} {cfg.id} | cu {cu or 'all'} plan {plan} grid {p['grid']} | raises as the reference does")
                continue
            y1, k1 = tle._site_solve(eng, cfg, "D", 0, sm.n)  # one launch per solve, no host wait
            e1 = lx.err(y1, r.y1)
            eng.replace_site(0, r.y1, "Psi")  # the second solve starts where the reference's does; the memory stays
            assert eng.krylov_memory(0) == r.k1
            y2, k2 = tle._site_solve(eng, cfg, "D", r.k1, sm.n)
            e2 = lx.err(y2, r.y2)
            assert eng.counters()["n_host_waits"] == 0
            print(f"SC | exp | {case.id} {cfg.id} | cu {cu or 'all'} plan {plan} grid {p['grid']} | parity {max(e1, e2):.2e} | "
                  f"k {[k1, k2]} (reference {[r.k1, r.k2]})")
            assert (k1, k2) == (r.k1, r.k2)
            assert eng.krylov_memory(0) == r.k2
            assert e1 <= lx.PARITY and e2 <= lx.PARITY
            got.append((cu, y1, k1, y2, k2))
        finally:
            eng.close()
    if not r.raises:
        _across_slices(f"{case.id} {cfg.id}", got)


BOND = [(c, i) for c in sc.EXP_BOND for i in c.configs]


@pytest.mark.parametrize("case, cfg_id", BOND, ids=[f"{c.id}-{i}" for c, i in BOND])
def test_exp_bond(case, cfg_id):
    import test_gpu_local_exp as tle
    from helpers import fold_seam

    cfg = sc.exp_config(cfg_id)
    sm, _, _, thresh = sc.bond_problem(case, cfg)
    got = []
    for cu, plan, regime in case.slices:
        p = _assert_exp_regime(case, cu, plan, regime)
        eng = _slice_engine(sm, cu, thresh=thresh, **cfg.engine_kw())
        try:
            eng.split_center(True)
            A, sigma = eng.get_site(0), eng.get_bond()
            assert fold_seam.rel(np.tensordot(A, sigma, axes=(2, 0)), sm.psi) < fold_seam.TOL
            b = sc.bond_reference(sm, cfg, A, sigma, thresh)
            assert fold_seam.rel(eng.get_env(0, 1), b.Lp) < fold_seam.TOL
            assert not b.raises, b.raises
            assert lx.well_separated(b.d1, thresh) and lx.well_separated(b.d2, thresh), (b.d1, b.d2, thresh)
            ys, ks = [], []
            for start, k_prev, ref_y, ref_k in ((None, 0, b.y1, b.k1), (b.y1, b.k1, b.y2, b.k2)):
                if start is not None:
                    eng.set_bond(1, start)  # the second solve starts where the reference's does; the memory stays
                assert eng.krylov_memory(0) == k_prev
                before = tle._counts(eng)
                eng.bond_exp(cfg.dt)
                after = tle._counts(eng)
                assert after[4] - before[4] == 1 and after[0] - before[0] == 1  # one launch per solve
                ys.append(eng.get_bond())
                ks.append(eng.krylov_memory(0))
            assert eng.counters()["n_host_waits"] == 0
            e1, e2 = lx.err(ys[0], b.y1), lx.err(ys[1], b.y2)
            print(f"SC | exp | {case.id} {cfg.id} | cu {cu or 'all'} plan {plan} grid {p['grid']} | parity {max(e1, e2):.2e} | "
                  f"k {ks} (reference {[b.k1, b.k2]})")
            assert ks == [b.k1, b.k2]
            assert e1 <= lx.PARITY and e2 <= lx.PARITY
            # the split's gauge may differ between slices: compare A sigma'
            got.append((cu, np.tensordot(A, ys[0], axes=(2, 0)), ks[0], np.tensordot(A, ys[1], axes=(2, 0)), ks[1]))
        finally:
            eng.close()
    _across_slices(f"{case.id} {cfg.id}", got)
