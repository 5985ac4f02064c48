"""CPU: the references and the inputs of tests/test_gpu_local_exp.py (tests/helpers/local_exp.py).

What is shown here, for EVERY case whose Krylov count the GPU module asserts and with none left out:
  * the statement-level reference converges (or raises, where the case is about the message), and the differences that
    decide its k lie a factor ``MARGIN`` away from the case's threshold on both sides (``well_separated``; why the
    factor is 3 and not 10 is written at ``MARGIN``);
  * ``sil_orthodox`` solves the operation: its error against ``exact_exp`` is below the threshold, and 1e-13 where the
    Krylov space is exhausted (n = 1, 2, 3, 5) -- the reference variant is NOT exact there (2e-3 at n = 2: its alpha_l
    = <v_0 | H v_l> is not the projection of H), which is the reference's behaviour, so variant 0 is compared with the
    oracle only;
  * the cases meant for the large-norm branch of the projected exponential have |s| (|alpha_0| + beta_0) > 8, all
    others < 8.
The reference's own error against ``exact_exp`` is printed per family (run with -s): it is the first term of the GPU bar."""

import numpy as np
import pytest

from helpers import local_exp as lx
from oracle import tdvp_oracle as orc

GRID = lx.grid_cases()


def _fmt(m):
    return "/".join("-" if x is None else f"{x:.1f}" for x in m)


def test_recording_threshold_leaves_the_oracle_alone():
    H, x = lx.herm(36), lx.start(36)
    for integ, fn in (("lanczos", orc.sil_lanczos), ("arnoldi", orc.sil_arnoldi)):
        y0, k0 = fn(-0.1j, lambda v: H @ v, x, 1e-9, 0, True)
        y1, k1, (before, last) = lx.sil_ref(integ, -0.1j, lambda v: H @ v, x, 1e-9, 0, True)
        assert k0 == k1 and np.array_equal(y0, y1)
        assert last < 1e-9 < before


def test_orthodox_is_the_oracle_but_for_alpha():
    """a start vector whose Krylov space is one-dimensional: <v_0 | H v_0> is the only alpha, both forms agree to the bit;
    and on a generic vector they differ, by less than the threshold each solve was run with"""
    H = lx.herm(36)
    e = lx.eigen_start(H, 5)
    a, ka, _ = lx.sil_orthodox(-0.1j, lambda v: H @ v, e)
    b, kb, _ = lx.sil_ref("lanczos", -0.1j, lambda v: H @ v, e)
    assert ka == kb == 1 and np.array_equal(a, b)
    x = lx.start(36)
    a, ka, _ = lx.sil_orthodox(-0.1j, lambda v: H @ v, x)
    b, kb, _ = lx.sil_ref("lanczos", -0.1j, lambda v: H @ v, x)
    assert 0 < lx.err(a, b) < 1e-9


@pytest.mark.parametrize("case", GRID, ids=lambda c: c.id)
@pytest.mark.parametrize("integ, var", lx.CONFIGS, ids=lambda v: v)
def test_dense_case(case, integ, var):
    if lx.reference_unstable(case, integ):
        H, x = case.matrix(), case.vector()
        try:
            y, k, d = lx.sil(integ, var, case.scale, lambda v: H @ v, x, lx.THRESH, case.k_prev, case.cn)
        except ValueError as e:
            print(f"{case.id} {integ}: the oracle raises: {e}")
            return
        e_arn = lx.err(y, case.exact(x))
        e_lan = lx.err(lx.sil_orthodox(case.scale, lambda v: H @ v, x, lx.THRESH, case.k_prev, case.cn)[0], case.exact(x))
        print(f"{case.id} {integ}: the oracle's error {e_arn:.1e}, orthodox Lanczos on the same input {e_lan:.1e}")
        assert e_arn > 100 * e_lan  # noise, not convergence: four orders above what the same schedule gives Lanczos
        return
    r = lx.dense_reference(case, integ, var)
    print(f"{case.id:42s} {integ[:3]}/{var[:4]} thresh {r.thresh:.1e} k {r.k1}"
          f"{'/' + str(r.k2) if r.chained else ''} margins {_fmt(lx.margins(r.d1, r.thresh))}"
          f"{' ' + _fmt(lx.margins(r.d2, r.thresh)) if r.chained else ''} error {r.err1:.1e}")
    assert not r.exhausted and lx.well_separated(r.d1, r.thresh), (r.d1, r.thresh)
    if r.chained:
        assert lx.well_separated(r.d2, r.thresh), (r.d2, r.thresh)
    if case.k_prev == 20:  # the saturated warm-up: n_warm = 15, first inspection at l = 15, closes at l = 16
        assert r.k1 == 17 and r.d1[0] is None
    if (integ, var) != ("lanczos", "reference"):  # a projection of H: converged means solved
        assert r.err1 < r.thresh
    col0 = lx.first_column_norm(case.scale, case.matrix(), case.vector())
    assert (col0 > 8) == case.dense_branch(), col0


def test_families_for_the_record():
    """worst error of each reference against exact_exp per operator family (printed), and the k values"""
    fam = {}
    for case in GRID:
        for integ, var in lx.CONFIGS:
            if lx.reference_unstable(case, integ):
                continue
            r = lx.dense_reference(case, integ, var)
            f = fam.setdefault((case.family, integ[:3] + "/" + var[:4]), [0.0, set()])
            f[0] = max(f[0], r.err1, r.err2 if r.chained else 0.0)
            f[1].add(r.k1)
    for (name, cfg), (e, ks) in fam.items():
        print(f"{name:32s} {cfg}: k {sorted(ks)} worst error {e:.1e}")
    assert len(fam) > 0


@pytest.mark.parametrize("case", lx.edge_cases(), ids=lambda c: c.id)
def test_exhaustion(case):
    n = case.n
    for integ, var in lx.CONFIGS:
        r = lx.dense_reference(case, integ, var)
        print(f"{case.id} {integ[:3]}/{var[:4]}: thresh {r.thresh:.1e} k {r.k1} differences {r.d1} error {r.err1:.1e}")
        assert lx.well_separated(r.d1, r.thresh, exhausted=r.exhausted)
        if r.chained:
            assert lx.well_separated(r.d2, r.thresh, exhausted=r.k2 == n)
        if n <= 5:
            assert r.k1 == n and r.exhausted  # closed by nsize
            if (integ, var) != ("lanczos", "reference"):
                assert r.err1 < 1e-13
        elif case.k_prev == 20:
            assert r.k1 == min(17, n)
    if n == 2 and case.k_prev == 0:  # the reference variant is no projection of H: wrong at exhaustion, and that is the reference
        assert lx.dense_reference(case, "lanczos", "reference").err1 > 1e-6


def test_eigenvector_start_closes_at_one():
    H = lx.herm(36)
    x = lx.eigen_start(H, 7)
    for integ, var in lx.CONFIGS:
        for cn, norm in ((True, 1.0), (False, 1.7)):
            y, k, d = lx.sil(integ, var, -0.1j, lambda v: H @ v, x * norm, lx.THRESH, 0, cn)
            assert k == 1 and d == (None, None)
            assert lx.err(y, lx.exact_exp(-0.1j, H, x * norm, cn)) < 1e-13


def test_zero_vector_and_no_convergence():
    H = lx.herm(36)
    z = np.zeros(36, dtype=np.complex128)
    nc = lx.NOT_CONVERGING
    Hw, xw = nc["gain"] * lx.wide(nc["n"]), lx.start(nc["n"])
    for integ, var in lx.CONFIGS:
        with pytest.raises(ValueError, match="Initial psi has zero norm."):
            lx.sil(integ, var, -0.1j, lambda v: H @ v, z, lx.THRESH, 0, False)
        y, k, _ = lx.sil(integ, var, -0.1j, lambda v: H @ v, z, lx.THRESH, 0, True)
        assert k == 1 and np.isnan(y).all()  # 0 / |0|: what the reference returns, and so what the device is held to
        with pytest.raises(ValueError, match=f"Short Iterative {integ.capitalize()} is not converged in 20 basis"):
            lx.sil(integ, var, nc["scale"], lambda v: Hw @ v, xw, lx.THRESH, 0, True)


@pytest.mark.parametrize("shape", [lx.SHAPE_SMALL, lx.SHAPE_LONG], ids=["small", "long"])
@pytest.mark.parametrize("cfg", lx.ENGINE_CONFIGS, ids=lambda c: c.id)
def test_engine_case(shape, cfg):
    r = lx.site_reference(shape, cfg)
    sm = r.seam
    H = lx.seam_spectral(sm)[0]
    assert lx.is_hermitian(H)
    x = lx.start(sm.n, 5).reshape(sm.psi.shape)
    assert lx.err(sm.heff(x).reshape(-1), H @ x.reshape(-1) + sm.shift * x.reshape(-1)) < 1e-13  # the dense builder
    assert (r.first_column > 8) == (cfg.shift != 0.0), r.first_column
    if r.raises:
        print(f"{cfg.id} {shape}: the reference raises: {r.raises}")
        assert cfg.shift and cfg.relax  # exp(-(100 + h) / 2) through a T_k that is no projection of it
        return
    print(f"{cfg.id:36s} {shape} thresh {r.thresh:.1e} k {r.k1}/{r.k2} margins {_fmt(lx.margins(r.d1, r.thresh))} "
          f"{_fmt(lx.margins(r.d2, r.thresh))} error {r.err1:.1e} {r.err2:.1e}")
    assert lx.well_separated(r.d1, r.thresh) and lx.well_separated(r.d2, r.thresh)
    if (cfg.integrator, cfg.variant) != ("lanczos", "reference") and not (cfg.shift and cfg.relax):
        assert r.err1 < r.thresh and r.err2 < r.thresh
    if shape != lx.SHAPE_SMALL:
        return
    # the bond solve behind a forward split (the device's QR may pick another gauge: a unitarily equivalent problem)
    A, sig = orc.qr_psi2Asigma(sm.psi)
    Lp, _ = sm.keff_blocks(A)
    t = lx.placed_thresh(cfg.integrator, cfg.variant, cfg.bond_scale(), sm.keff(Lp), sig, 0, cfg.cn)
    b = lx.bond_reference(sm, cfg, A, sig, 0, t)
    assert lx.is_hermitian(lx.Seam.keff_dense(sm, Lp))
    assert (b.first_column > 8) == (cfg.shift != 0.0)
    if b.raises:
        print(f"{cfg.id} bond: the reference raises: {b.raises}")
        assert cfg.shift and cfg.relax  # exp(+(100 + h) / 2): differences of the order e^50
        return
    print(f"{cfg.id:36s} bond thresh {t:.1e} k {b.k} margins {_fmt(lx.margins(b.d, t))} error {b.err:.1e}")
    assert lx.well_separated(b.d, t)


def test_natural_deferred_case():
    for cfg in lx.ENGINE_CONFIGS[:1] + [c for c in lx.ENGINE_CONFIGS if c.id == "lanczos-orthodox"]:
        r = lx.site_reference(lx.SHAPE_NATURAL_B, cfg, dense=False)
        assert r.seam.n > 16384
        print(f"{cfg.id} n {r.seam.n} thresh {r.thresh:.1e} k {r.k1}/{r.k2} margins {_fmt(lx.margins(r.d1, r.thresh))} "
              f"{_fmt(lx.margins(r.d2, r.thresh))}")
        assert lx.well_separated(r.d1, r.thresh) and lx.well_separated(r.d2, r.thresh)


def test_launch_arithmetic():
    # 9 iterations from k_prev = 0 on path B with a 3-launch apply: 9 * (3 + 2) + 2 * 9 inspections + 2
    assert lx.step_launches(9 * 5 + 18 + 2, 9, 0, 256, True, 3) == 2
    # k_prev = 20: iterations 0 .. 14 are not inspected
    assert lx.inspections(17, 20, 256) == 2
    assert lx.step_launches(17 * 2 + 4 + 2 + 2, 17, 20, 256, False, 1) == 1
