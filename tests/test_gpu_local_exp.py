"""GPU: the local Krylov exponential x <- exp(s Op) x on all four device paths.

  A  multi-launch Lanczos, one-workgroup vector step (k_lanczos_step_small)      one launch per iteration beside the apply
  B  multi-launch Lanczos, deferred normalisation (dot + k_lanczos_update_def)   two
  C  multi-launch Arnoldi (k_multi_dot, k_arnoldi_update, k_scale_inv_norm)      three
  D  the one-launch persistent solve (small_site.hip; batch_site.hip for TDVPBatch)  one launch per SOLVE

Every engine case asserts the path it ran from the ``n_launch`` counter (``helpers.local_exp.step_launches``) and bit 3
of ``heff_apply_center``'s flags; the ``expm_dense`` cases from the counters ``mitdvp_expm_dense_counted`` hands back
(Lanczos with n <= 16384 is A while the small kernels are on, B with MITDVP_SMALL_KERNELS=0, Arnoldi is C).

Bars, all in the max norm (helpers.local_exp):
  * against the statement-level reference (the oracle for lanczos_variant "reference" and Arnoldi, ``sil_orthodox`` for
    "orthodox"): ``PARITY`` = 1e-11 on the result, the bar of test_unit_golden_krylov, and the same k;
  * against ``exact_exp``: err_device <= err_reference + PARITY (the triangle inequality: as wrong as the algorithm
    is, plus the parity bar, no more);
  * between device paths on the same input: PARITY and the same k.
The thresholds and the input condition behind every asserted k are those of tests/test_local_exp_host.py.  lanczos_variant
"reference" at an exhausted Krylov space is not exact (its T_k is no projection of H): it is compared with the oracle,
as everywhere; that its error against ``exact_exp`` is then the oracle's own is what the second bar says.

Lines starting with "LX" (figures) and "LXV" (verdicts where the reference's is decided by rounding) are the record behind profiles/local_exp_tests.txt (run with -s)."""

import os

import numpy as np
import pytest

from helpers import fold_seam
from helpers import local_exp as lx

pytestmark = pytest.mark.gpu

GRID = lx.grid_cases()
STEP = {"A": 1, "B": 2, "C": 3}


def _record(family, path, parity, excess, ks):
    print(f"LX | {family} | {path} | parity {parity:.2e} | err_device - err_reference {excess:+.2e} | k {ks}")


def _hold(y, k, ref_y, ref_k, exact, ref_err, what):
    """the two bars of one solve; returns (parity defect, err_device - err_reference)"""
    parity = lx.err(y, ref_y)
    excess = lx.err(y, exact) - ref_err
    print(f"{what}: k {k} (reference {ref_k}) parity {parity:.2e} err_device - err_reference {excess:+.2e}")
    assert k == ref_k, what
    assert parity <= lx.PARITY, what
    assert excess <= lx.PARITY, what
    return parity, excess


class _small_kernels_off:
    """MITDVP_SMALL_KERNELS=0 while an engine is created (Engine reads it in its constructor)"""

    def __enter__(self):
        self.old = os.environ.get("MITDVP_SMALL_KERNELS")
        os.environ["MITDVP_SMALL_KERNELS"] = "0"

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("MITDVP_SMALL_KERNELS", None)
        else:
            os.environ["MITDVP_SMALL_KERNELS"] = self.old


def _dense_solve(H, x, case_n, scale, integ, cn, thresh, k_prev, var, path):
    """one expm_dense; asserts the path it took from the launches of its Krylov loop (the operator's GEMM is not
    counted there); returns (y, k)"""
    from pytdscf_amd import engine as E

    y, k, c = E.expm_dense(H, x, scale, integ, cn, thresh, k_prev, variant=var, counters=True)
    iters = lx.iterations_run(k, k_prev, case_n)
    step = lx.step_launches(c["n_launch"], iters, k_prev, case_n, cn, 0)
    assert step == STEP[path], (step, path, c["n_launch"], iters)
    return y, k


def _dense_path(integ, n):
    return "A" if integ == "lanczos" else "C"


# ---------------------------------------------------------------------------------------------------------------------
# a. expm_dense: paths A and C (and B through the environment switch)
# ---------------------------------------------------------------------------------------------------------------------
def _dense(case, integ, var, path):
    r = lx.dense_reference(case, integ, var)
    H, x = case.matrix(), case.vector()
    if case.dense_branch():  # the large-norm branch of the projected exponential is the one exercised
        assert lx.first_column_norm(case.scale, H, x) > 8
    y, k = _dense_solve(H, x, case.n, case.scale, integ, case.cn, r.thresh, case.k_prev, var, path)
    p, e = _hold(y, k, r.y1, r.k1, r.ex1, r.err1, f"{case.id} {integ}/{var} path {path}")
    ks = [k]
    if r.chained:  # a second call on the first's (reference) result with its k as memory, as the golden test does
        y, k = _dense_solve(H, r.y1, case.n, case.scale, integ, case.cn, r.thresh, r.k1, var, path)
        p2, e2 = _hold(y, k, r.y2, r.k2, r.ex2, r.err2, f"{case.id} {integ}/{var} path {path}, second call")
        p, e = max(p, p2), max(e, e2)
        ks.append(k)
    _record(f"dense {case.family} {integ}/{var}", path, p, e, ks)


def _verdict(family, path, verdict, k, error):
    print(f"LXV | {family} | {path} | {verdict} | k {k} | error against exact_exp {error}")


def _dense_unstable(case, integ, var, path):
    """Arnoldi behind a saturated warm-up on the offset operators: the oracle's verdict and k are decided by rounding
    (helpers.local_exp.reference_unstable), so neither its k nor parity with it can be asked of the device.  What can:
    the device raises the reference's message, or it returns the solution -- closing differences below the threshold
    mean an error below the threshold -- and, where the oracle returns as well, it is no further from exact_exp than
    the oracle plus the parity bar.  Which of the two it did, and its k, go into the record."""
    r = lx.unstable_reference(case, integ, var)
    H, x = case.matrix(), case.vector()
    if case.dense_branch():
        assert lx.first_column_norm(case.scale, H, x) > 8
    ref = "the oracle raises" if r.raises else f"the oracle closes at k {r.k1} with error {r.err1:.2e}"
    message = f"Short Iterative {integ.capitalize()} is not converged in 20 basis"
    try:
        y, k = _dense_solve(H, x, case.n, case.scale, integ, case.cn, r.thresh, case.k_prev, var, path)
    except ValueError as dev_err:
        print(f"{case.id} {integ} path {path}: {ref}; the device raises: {dev_err}")
        assert message in str(dev_err), str(dev_err)
        _verdict(f"dense {case.family} {integ}/{var}", path, f"raises ({ref})", "-", "-")
        return
    e = lx.err(y, r.ex1)
    print(f"{case.id} {integ} path {path}: {ref}; the device closes at k {k} with error {e:.2e}")
    _verdict(f"dense {case.family} {integ}/{var}", path, f"closes ({ref})", k, f"{e:.2e}")
    assert np.isfinite(y).all() and 17 <= k <= 20  # first inspection at l = 15, first comparison at l = 16
    assert e < r.thresh
    if not r.raises:
        assert e <= r.err1 + lx.PARITY


DENSE = [(c, i, v) for c in GRID + lx.edge_cases() for i, v in lx.CONFIGS]


@pytest.mark.parametrize("case, integ, var", DENSE, ids=[f"{c.id}-{i}-{v}" for c, i, v in DENSE])
def test_dense(case, integ, var):
    if lx.reference_unstable(case, integ):
        _dense_unstable(case, integ, var, _dense_path(integ, case.n))
    else:
        _dense(case, integ, var, _dense_path(integ, case.n))


@pytest.mark.parametrize("case", [c for c in GRID if c.n == 300 and c.k_prev == 0] + [c for c in lx.edge_cases() if c.n in (2, 5, 21)],
                         ids=lambda c: c.id)
@pytest.mark.parametrize("var", ["reference", "orthodox"])
def test_dense_deferred(case, var):
    """path B at unit level: the same inputs with the one-workgroup step switched off"""
    with _small_kernels_off():
        _dense(case, "lanczos", var, "B")


def test_dense_deferred_agrees_with_the_one_workgroup_step():
    """A against B on the same input, both variants, with and without the large-norm branch"""
    for case in (c for c in GRID if c.n == 300 and c.k_prev == 0 and c.op != "wide"):
        H, x = case.matrix(), case.vector()
        for var in ("reference", "orthodox"):
            t = lx.dense_reference(case, "lanczos", var).thresh
            ya, ka = _dense_solve(H, x, case.n, case.scale, "lanczos", case.cn, t, 0, var, "A")
            with _small_kernels_off():
                yb, kb = _dense_solve(H, x, case.n, case.scale, "lanczos", case.cn, t, 0, var, "B")
            print(f"{case.id} {var}: A against B {lx.err(ya, yb):.2e}, k {ka} {kb}")
            assert ka == kb and lx.err(ya, yb) <= lx.PARITY


@pytest.mark.parametrize("integ, var", lx.CONFIGS, ids=lambda v: v)
def test_dense_edges(integ, var):
    from pytdscf_amd import engine as E

    H = lx.herm(36)
    for cn, norm in ((True, 1.0), (False, 1.7)):  # a start vector that is an eigenvector: beta_0 < eps closes at k = 1
        x = lx.eigen_start(H, 7) * norm
        ref, kr, _ = lx.sil(integ, var, -0.1j, lambda v: H @ v, x, lx.THRESH, 0, cn)
        y, k = _dense_solve(H, x, 36, -0.1j, integ, cn, lx.THRESH, 0, var, _dense_path(integ, 36))
        ex = lx.exact_exp(-0.1j, H, x, cn)
        _hold(y, k, ref, kr, ex, lx.err(ref, ex), f"eigenvector start cn={cn}")
        assert k == 1
    z = np.zeros(36, dtype=np.complex128)
    with pytest.raises(ValueError, match="Initial psi has zero norm."):
        E.expm_dense(H, z, -0.1j, integ, False, lx.THRESH, 0, variant=var)
    ref, kr, _ = lx.sil(integ, var, -0.1j, lambda v: H @ v, z, lx.THRESH, 0, True)
    y, k = _dense_solve(H, z, 36, -0.1j, integ, True, lx.THRESH, 0, var, _dense_path(integ, 36))
    assert k == kr == 1 and np.isnan(ref).all() and np.isnan(y).all()  # 0 / |0|, as the reference
    nc = lx.NOT_CONVERGING
    Hw, xw = nc["gain"] * lx.wide(nc["n"]), lx.start(nc["n"])
    with pytest.raises(ValueError) as ref_err:
        lx.sil(integ, var, nc["scale"], lambda v: Hw @ v, xw, lx.THRESH, 0, True)
    with pytest.raises(ValueError) as dev_err:
        E.expm_dense(Hw, xw, nc["scale"], integ, True, lx.THRESH, 0, variant=var)
    assert str(ref_err.value) in str(dev_err.value), (str(ref_err.value), str(dev_err.value))


# ---------------------------------------------------------------------------------------------------------------------
# b. site solve through the one-site engine seam: D and B at the small shape, A and B at the long one
# ---------------------------------------------------------------------------------------------------------------------
def _counts(eng):
    c = eng.counters()
    return c["n_launch"], c["n_heff"], c["n_keff"], c["n_exp_site"], c["n_exp_bond"]


def _apply_launches(eng, want_small):
    """launches of one H_eff apply as the solve issues it (the second call: a first one may look at the blocks once)"""
    eng.heff_apply_center()
    a = _counts(eng)
    _, flags = eng.heff_apply_center()
    b = _counts(eng)
    assert bool(flags & 8) == want_small, hex(flags)
    assert b[1] - a[1] == 1
    return b[0] - a[0]


def _site_solve(eng, cfg, path, k_prev, n):
    """one site_exp; asserts the path it took; returns (tensor, k)"""
    mv = _apply_launches(eng, path == "D")
    a = _counts(eng)
    eng.site_exp(cfg.dt)
    b = _counts(eng)
    assert b[3] - a[3] == 1
    k = eng.krylov_memory(0)
    if path == "D":
        assert b[0] - a[0] == 1, b[0] - a[0]  # one launch per solve
    else:
        iters = b[1] - a[1]
        assert iters == k
        step = lx.step_launches(b[0] - a[0], iters, k_prev, n, cfg.cn, mv)
        assert step == STEP[path], (step, path, b[0] - a[0], iters, mv)
    return eng.get_site(0), k


def _paths(shape, cfg):
    """(path, small kernels on) of the two engines a shape is solved on"""
    multi = "A" if cfg.integrator == "lanczos" else "C"
    off = "B" if cfg.integrator == "lanczos" else "C"
    return [("D" if shape == lx.SHAPE_SMALL else multi, True), (off, False)]


@pytest.mark.parametrize("shape", [lx.SHAPE_SMALL, lx.SHAPE_LONG], ids=["small", "long"])
@pytest.mark.parametrize("cfg", lx.ENGINE_CONFIGS, ids=lambda c: c.id)
def test_site_solve(shape, cfg):
    from pytdscf_amd import TDVPEngine

    r = lx.site_reference(shape, cfg)
    sm = r.seam
    if cfg.shift:
        assert r.first_column > 8  # the large-norm branch
    got = []
    for path, small in _paths(shape, cfg):
        eng = sm.engine(TDVPEngine, small_kernels=small, thresh=r.thresh, **cfg.engine_kw())
        try:
            assert eng.krylov_memory(0) == 0
            if r.raises:
                _apply_launches(eng, path == "D")
                with pytest.raises(ValueError) as dev_err:
                    eng.site_exp(cfg.dt)
                assert r.raises in str(dev_err.value), (r.raises, str(dev_err.value))
                print(f"{cfg.id} {shape} path {path}: raises as the reference does")
                continue
            y1, k1 = _site_solve(eng, cfg, path, 0, sm.n)
            p1, e1 = _hold(y1, k1, r.y1, r.k1, r.ex1, r.err1, f"{cfg.id} {shape} path {path}")
            eng.replace_site(0, r.y1, "Psi")  # the second solve starts where the reference's does; the memory stays
            assert eng.krylov_memory(0) == r.k1
            y2, k2 = _site_solve(eng, cfg, path, r.k1, sm.n)
            p2, e2 = _hold(y2, k2, r.y2, r.k2, r.ex2, r.err2, f"{cfg.id} {shape} path {path}, second solve")
            assert eng.krylov_memory(0) == r.k2
            _record(f"site {cfg.family} {cfg.integrator}/{cfg.variant}", path, max(p1, p2), max(e1, e2), [k1, k2])
            got.append((path, y1, k1, y2, k2))
        finally:
            eng.close()
    if len(got) == 2:
        (pa, a1, ka1, a2, ka2), (pb, b1, kb1, b2, kb2) = got
        d = max(lx.err(a1, b1), lx.err(a2, b2))
        print(f"{cfg.id} {shape}: path {pa} against path {pb} {d:.2e}")
        assert d <= lx.PARITY and (ka1, ka2) == (kb1, kb2)


@pytest.mark.parametrize("variant", ["reference", "orthodox"])
def test_site_solve_deferred_beyond_the_one_workgroup_step(variant):
    """n = 20736 > 16384: path B with the small kernels ON; too long for a dense reference, compared with the oracle
    through ``oracle.heff_apply`` as matvec"""
    from pytdscf_amd import TDVPEngine

    cfg = next(c for c in lx.ENGINE_CONFIGS if c.id == f"lanczos-{variant}")
    r = lx.site_reference(lx.SHAPE_NATURAL_B, cfg, dense=False)
    sm = r.seam
    assert sm.n > 16384
    eng = sm.engine(TDVPEngine, small_kernels=True, thresh=r.thresh, **cfg.engine_kw())
    try:
        y1, k1 = _site_solve(eng, cfg, "B", 0, sm.n)
        eng.replace_site(0, r.y1, "Psi")
        y2, k2 = _site_solve(eng, cfg, "B", r.k1, sm.n)
    finally:
        eng.close()
    p = max(lx.err(y1, r.y1), lx.err(y2, r.y2))
    print(f"n {sm.n} {variant}: k {k1} {k2} (reference {r.k1} {r.k2}) parity {p:.2e}")
    assert (k1, k2) == (r.k1, r.k2) and p <= lx.PARITY
    _record(f"site n=20736 plain real_time lanczos/{variant}", "B", p, float("nan"), [k1, k2])


# ---------------------------------------------------------------------------------------------------------------------
# c. bond solve behind a forward split, paths D and B (C for Arnoldi)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", lx.ENGINE_CONFIGS, ids=lambda c: c.id)
def test_bond_solve(cfg):
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import TDVPEngine

    shape = lx.SHAPE_SMALL
    sm = lx.seam_for(shape, cfg)
    s = cfg.bond_scale()  # +i dt / 2 (relaxation: +dt / 2)
    A0, sig0 = orc.qr_psi2Asigma(sm.psi)  # the device's QR may pick another gauge: a unitarily equivalent problem
    thresh = lx.placed_thresh(cfg.integrator, cfg.variant, s, sm.keff(sm.keff_blocks(A0)[0]), sig0, 0, cfg.cn)
    for path, small in _paths(shape, cfg):
        eng = sm.engine(TDVPEngine, small_kernels=small, thresh=thresh, **cfg.engine_kw())
        try:
            eng.split_center(True)
            A, sigma = eng.get_site(0), eng.get_bond()
            assert fold_seam.rel(np.tensordot(A, sigma, axes=(2, 0)), sm.psi) < fold_seam.TOL
            b = lx.bond_reference(sm, cfg, A, sigma, 0, thresh)
            assert fold_seam.rel(eng.get_env(0, 1), b.Lp) < fold_seam.TOL
            if cfg.shift:
                assert b.first_column > 8
            before = _counts(eng)
            if b.raises:
                # exp(+(100 + k) / 2): approximants of norm 5e21 whose differences stall where the projected exponential
                # rounds (1e7 through the oracle's eigh, less through the device's scaling and squaring).  Whether twenty
                # vectors "converge" to 1e-9 is decided by that rounding, not by the algorithm: the device either raises
                # the reference's message or returns the normalised solution, whose error is then below the threshold.
                try:
                    eng.bond_exp(cfg.dt)
                except ValueError as dev_err:
                    assert b.raises in str(dev_err), (b.raises, str(dev_err))
                    print(f"{cfg.id} bond path {path}: raises as the reference does")
                    _verdict(f"bond {cfg.family} {cfg.integrator}/{cfg.variant}", path, "raises (the reference raises)", "-", "-")
                else:
                    assert cfg.cn
                    e = lx.err(eng.get_bond(), b.ex)
                    print(f"{cfg.id} bond path {path}: the reference raises, the device closes at k "
                          f"{eng.krylov_memory(0)} with error {e:.2e}")
                    _verdict(f"bond {cfg.family} {cfg.integrator}/{cfg.variant}", path, "closes (the reference raises)",
                             eng.krylov_memory(0), f"{e:.2e}")
                    assert e < thresh
                continue
            assert lx.well_separated(b.d, thresh), (b.d, thresh)
            eng.bond_exp(cfg.dt)
            after = _counts(eng)
            k = eng.krylov_memory(0)
            assert after[4] - before[4] == 1
            if path == "D":
                assert after[0] - before[0] == 1
            else:  # keff_apply_rect: two GEMMs per apply
                iters = after[2] - before[2]
                assert iters == k
                assert lx.step_launches(after[0] - before[0], iters, 0, sigma.size, cfg.cn, 2) == STEP[path]
            p, e = _hold(eng.get_bond(), k, b.y, b.k, b.ex, b.err, f"{cfg.id} bond path {path}")
            _record(f"bond {cfg.family} {cfg.integrator}/{cfg.variant}", path, p, e, [k])
        finally:
            eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# d. batch: k_batch_sweep against serial engines on path B, and those against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant, shift", [("orthodox", 0.0), ("reference", 100.0), ("orthodox", 100.0)])
def test_batch(variant, shift):
    import test_gpu_batch as tb
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import TDVPBatch
    from pytdscf_amd import synthetic as syn

    B, L, d, D, M, dt, nsteps = 4, 3, 3, 6, 4, 0.2, 2
    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    seeds = [11 + r for r in range(B)]
    kw = dict(lanczos_variant=variant)
    bt = TDVPBatch(B, L, **kw)
    for e, sd in zip(bt.engines, seeds):
        e.set_mpo(mpo, shift=shift)
        e.init_random([d] * L, D, seed=sd)
    start = [e.get_mps() for e in bt.engines]
    bt.sweep(dt, True)  # the first step builds the right environments with the engines' own launches
    bt.sweep(dt, False)
    for e in bt.engines:
        e.counters_reset()
    bt.sweep(dt, True)
    bt.sweep(dt, False)
    assert bt.statuses == [0] * B
    c0 = bt[0].counters()
    assert c0["n_launch"] == 2 and bt[1].counters()["n_launch"] == 0  # one launch per half-sweep for the whole batch
    assert c0["n_exp_site"] == 2 * L and c0["n_exp_bond"] == 2 * (L - 1)
    tb._against_serial(bt, mpo, [d] * L, D, seeds, nsteps, dt, shift=shift, **kw)
    cls = lx.OrthodoxOracleMPS if variant == "orthodox" else orc.OracleMPS
    for r in range(B):
        ser = tb._serial(L, mpo, [d] * L, D, seeds[r], nsteps, dt, shift=shift, **kw)
        ref = cls([c.copy() for c in start[r]], mpo, shift=shift)
        for _ in range(nsteps):
            ref.propagate(dt)
        tb._same_state(ref.cores, ser.get_mps(), f"replica {r}: serial path B against the oracle ({variant}, shift {shift})")
        ser.close()
    bt.close()
