"""GPU: the projected eigen-solve of the batched improved relaxation alone (engine.tridiag_lowest, mitdvp_batch_trilow:
the device function k_batch_relax runs after every Lanczos vector, one workgroup per matrix) against
scipy.linalg.eigh_tridiagonal in float64 on the same inputs.

The cases are helpers/relax_cases.tridiag_cases: orders 1, 2, 3, 21, 63, 64; random matrices; matrices graded over 12
decades, both ways; matrices recorded from Lanczos runs on the H_eff of the relaxation's own chains, the 64-vector ones
with ghost copies of the lowest Ritz value; one off-diagonal entry of 1e-12 |T|; a lowest pair split by 1e-9 |T|.  The bars
are not chosen by hand: tridiag_table measures, per case, the reference's own |theta_LAPACK - theta_longdouble| and its
residual, and sets each bar to 8 x that, floored at k eps |T|_1; where the reference's gap exceeds 1e-6 |T|_1 the vector
is held too, to (residual bar) / gap.  profiles/batch_relax_tests.txt has the table."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solved():
    from helpers import relax_cases as rc
    from pytdscf_amd import engine

    rows = rc.tridiag_table()
    theta, vecs = engine.tridiag_lowest([r["alpha"] for r in rows], [r["beta"] for r in rows])
    return rows, theta, vecs


def test_every_case_within_its_bars(solved):
    rows, theta, vecs = solved
    misses = []
    for r, th, c in zip(rows, theta, vecs):
        d_theta = abs(th - r["theta"])
        res = float(np.linalg.norm(r["T"] @ c - th * c))
        d_vec = float(np.linalg.norm(c - r["vec"]))
        print("%-24s k %2d  |dtheta| %.2e (bar %.2e)  resid %.2e (bar %.2e)  |dvec| %.2e (bar %s)  | |c| - 1 | %.1e  c0 %.2e" % (
            r["name"], r["k"], d_theta, r["bar_theta"], res, r["bar_res"], d_vec,
            "-" if r["bar_vec"] is None else "%.2e" % r["bar_vec"], abs(np.linalg.norm(c) - 1), c[0]))
        ok = (len(c) == r["k"] and d_theta <= r["bar_theta"] and res <= r["bar_res"] and abs(np.linalg.norm(c) - 1) <= 4 * r["k"] * 2.3e-16
              and c[0] >= 0 and (r["bar_vec"] is None or d_vec <= r["bar_vec"]))
        if not ok:
            misses.append(r["name"])
    assert not misses


def test_one_call_or_many_gives_the_same_bits(solved):
    """a case alone in its launch gives the bits it gives among the others, and the single form returns plain values"""
    from pytdscf_amd import engine

    rows, theta, vecs = solved
    for q in (0, len(rows) // 2, len(rows) - 1):
        th, c = engine.tridiag_lowest(rows[q]["alpha"], rows[q]["beta"])
        assert th == theta[q] and np.array_equal(c, vecs[q])
