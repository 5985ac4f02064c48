"""GPU: the building blocks of the batched-trajectory kernels, each run alone in one workgroup through the test hook
``mitdvp_batch_block`` / ``engine.batch_block`` and held to the NumPy models of ``helpers.batch_blocks_ref``.

Every batch kernel of ``csrc/batch_site.hip`` is built from these functions, and the tests of those kernels compare whole
time steps with another GPU path at workflow bars; here each function meets a plain reference at the shapes where a tiled
product, a Householder QR or a Jacobi split goes wrong:

* the workgroup product (``bt_matmul``, ``bt_heff``, ``bt_keff``, ``bt_env`` with the forward and the mirror strides and with
  bra != ket, the forward-only instance, the overlap walk): every M, N, K on and around the 32 x 32 x 16 tile, the envelope
  corners 64 x 2 x 64 x 16 x 16 and 16 x 32 x 16 x 16 x 1; ``max|out - ref| < 1e-12 max|ref|``; ``bt_matmul`` gives the same
  bits whatever dst aliases;
* ``bt_qr`` in both stride roles of the sweep, on Gaussian, product-state, zero-column, equal-column, graded and tiny input:
  the bars of ``test_gpu_qr_gauge_free.py::_check``, LAPACK up to the phases of diag(R) on the Gaussian rows, the two roles
  against each other;
* ``bp_jacobi`` + ``bp_select`` + ``bp_cprime`` on theta = U diag(s) V^H with a prescribed spectrum (``rr.check_split`` has
  the bars and where the projector bar applies);
* a result does not depend on the grid: three copies in one launch and a launch of one give the same bits.

The forward-only environment update, the selection and C' = theta B^H run as the hook's own non-inlined instances of the
one text (``bt_env_fwd_blk``, ``bp_select_blk``, ``bp_cprime_blk``): a second caller of the kernels' instances moved the
registers of ``k_batch_cross_mpo`` and ``k_batch_pair`` (profiles/batch_blocks_tests.txt).  So for these three the file
covers the text and a compilation of its own; the instances the production kernels call (``bt_env_fwd``, ``bp_select``,
``bp_cprime``: the same instructions, a few in another order or register) are covered through the tests of those kernels.

What the file found, both in ``bp_jacobi`` at 128 rows, both fixed.  (1) A split whose singular values are graded over 12
decades, or lie 0.8 apart, was ``SS_ENOTCONV``: the cyclic sweeps need 32 there and the limit was 30
(``BATCH_PAIR_MAX_SWEEPS``, now 64).  (2) With a geometric spectrum the singular values missed atol
``2 sqrt(BP_TINY) |theta|_F`` at 127 x 65 and 128 x 128 (2.96e-14 and 2.50e-14 against 2.31e-14): a row was left out of
the rotations as soon as its own norm fell to ``sqrt(BP_TINY) |theta|``, while it could still carry a part of a direction
whose singular value lies just above, and some eighty such rows together hid more than one floor.  Rows now leave the
rotations only at the roundoff of ``|theta|`` (``BP_FREEZE``); ``BP_TINY`` still decides which kept rows the completion
replaces.  The same rows now give 3.4e-16 and 4.0e-16.

Figures of one run on an MI355X: profiles/batch_blocks_tests.txt.
"""

import numpy as np
import pytest

from helpers import batch_blocks_ref as rr

pytestmark = pytest.mark.gpu


def run(row, plain=None, ncopies=1, variant=None):
    from pytdscf_amd import engine as E

    plain = rr.product_input(row) if plain is None else plain
    return E.batch_block(row["op"], row["dims"], *rr.operands(row, plain), ncopies=ncopies,
                         variant=row["variant"] if variant is None else variant, scl=rr.scl_of(row))


PRODUCT_GROUPS = {
    "matmul": lambda r: r["op"] == "matmul",
    "heff-corners": lambda r: r["op"] == "heff" and r["corner"],
    "heff-edges": lambda r: r["op"] == "heff" and not r["corner"],
    "keff": lambda r: r["op"] == "keff",
    "env-forward": lambda r: r["op"] == "env" and r["variant"] == 0,
    "env-mirror": lambda r: r["op"] == "env" and r["variant"] == 1,
    "env-forward-instance": lambda r: r["op"] == "env" and r["variant"] == 2,
    "overlap": lambda r: r["op"] == "overlap",
}


@pytest.mark.parametrize("group", list(PRODUCT_GROUPS))
def test_products_equal_the_model(group):
    rows = [r for r in rr.CASES if PRODUCT_GROUPS[group](r)]
    assert rows
    worst = 0.0
    for r in rows:
        plain = rr.product_input(r)
        out, _, info = run(r, plain)
        defect = rr.product_defect(out[0], rr.model(r, plain))
        print(f"[batch_blocks] {r['name']}: defect {defect:.2e}")
        assert info[0, 0] == 0.0
        assert defect < rr.PRODUCT_BAR, (r["name"], defect)
        worst = max(worst, defect)
    print(f"[batch_blocks] {group}: {len(rows)} rows, worst defect {worst:.2e} (bar {rr.PRODUCT_BAR:.0e})")


def test_matmul_gives_the_same_bits_whatever_dst_aliases():
    n = 0
    for r in rr.CASES:
        if r["op"] != "matmul":
            continue
        M, N, K = r["dims"]
        plain = rr.product_input(r)
        sep = run(r, plain, variant=0)[0]
        if N == K:  # in place of A
            assert np.array_equal(run(r, plain, variant=1)[0], sep), r["name"]
            n += 1
        if M == K:  # in place of B
            assert np.array_equal(run(r, plain, variant=2)[0], sep), r["name"]
            n += 1
    assert n >= 12


def qr_both_roles(A, ncopies=1):
    """(Q, R) through the Psi2Asigma role and through the Psi2sigmaB role on the transposed problem, all copies"""
    from pytdscf_amd import engine as E

    m, n = A.shape
    q0, r0, i0 = E.batch_block("qr", (m, n), A, ncopies=ncopies, variant=0)
    q1, r1, i1 = E.batch_block("qr", (m, n), np.ascontiguousarray(A.T), ncopies=ncopies, variant=1)
    assert not i0.any() and not i1.any()
    fwd = [(q0[b].reshape(m, n), r0[b].reshape(n, n)) for b in range(ncopies)]
    bwd = [(q1[b].reshape(n, m).T, r1[b].reshape(n, n).T) for b in range(ncopies)]
    return fwd, bwd


@pytest.mark.parametrize("kind", rr.QR_KINDS)
def test_qr_in_both_stride_roles(kind):
    for r in rr.CASES:
        if r["op"] != "qr" or r["kind"] != kind:
            continue
        A = rr.qr_input(r)
        fwd, bwd = qr_both_roles(A)
        for role, (Q, R) in (("Psi2Asigma", fwd[0]), ("Psi2sigmaB", bwd[0])):
            fig = rr.check_qr(A, Q, R, lapack=kind == "gauss")
            print(f"[batch_blocks] {r['name']} {role}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
        dq = float(np.abs(fwd[0][0] - bwd[0][0]).max())
        dr = float(np.abs(fwd[0][1] - bwd[0][1]).max())
        print(f"[batch_blocks] {r['name']} roles against each other: Q {dq:.2e}, R {dr:.2e} (max|A| {np.abs(A).max():.2e})")
        assert dq < rr.QR_ROLES_BAR and dr <= rr.QR_ROLES_BAR * np.abs(A).max(), (r["name"], dq, dr)
        if kind in ("product", "zerocol"):  # a zero column takes no reflection: its R column above the diagonal and its
            n = A.shape[1]                   # diagonal entry are what the earlier reflections left of it, exactly 0
            zero = [c for c in range(n) if not A[:, c].any()]
            assert (zero or n == 1) and all(not fwd[0][1][:, c].any() for c in zero)


def split(row, theta, ncopies=1):
    from pytdscf_amd import engine as E

    m, n, r = row["dims"]
    B, Cp, info = E.batch_block("split", (m, n, r), theta, ncopies=ncopies)
    return [(B[b].reshape(r, n), Cp[b].reshape(m, r), info[b]) for b in range(ncopies)]


@pytest.mark.parametrize("kind", rr.SPLIT_KINDS)
def test_split_of_a_prescribed_spectrum(kind):
    nproj, failed = 0, []
    for r in rr.CASES:
        if r["op"] != "split" or r["kind"] != kind:
            continue
        theta, _, _ = rr.split_input(r)
        claims = rr.split_claims(r, theta)
        B, Cp, info = split(r, theta)[0]
        try:
            fig = rr.check_split(r, theta, B, Cp, info, claims=claims)
        except AssertionError as e:  # every row is run and reported before the test fails
            failed.append(f"{r['name']}: {e}")
            print(f"[batch_blocks] {r['name']}: FAILED {e}")
            continue
        assert ("proj" in fig) == claims["projector"]
        nproj += "proj" in fig
        if r["name"] == "split-geometric-8x8-r4":  # the clear gap at r the geometric spectrum is there for
            assert "proj" in fig
        print(f"[batch_blocks] {r['name']}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert not failed, "\n".join(failed)
    assert nproj == rr.PROJECTOR_COUNT[kind], (kind, nproj)


@pytest.mark.parametrize("what", ["product", "qr", "split"])
def test_a_result_does_not_depend_on_the_grid(what):
    if what == "product":
        r = rr.BY_NAME["heff-7x3x33x5x16"]
        plain = rr.product_input(r)
        one, three = run(r, plain)[0], run(r, plain, ncopies=3)[0]
        assert three.shape[0] == 3 and rr.product_defect(one[0], rr.model(r, plain)) < rr.PRODUCT_BAR
        assert all(np.array_equal(three[b], one[0]) for b in range(3))
    elif what == "qr":
        A = rr.qr_input(rr.BY_NAME["qr-gauss-130x33"])
        for one, three in zip(qr_both_roles(A), qr_both_roles(A, ncopies=3)):
            rr.check_qr(A, *one[0])
            assert all(np.array_equal(three[b][0], one[0][0]) and np.array_equal(three[b][1], one[0][1]) for b in range(3))
    else:
        r = rr.BY_NAME["split-graded12-127x65-r64"]
        theta, _, _ = rr.split_input(r)
        one, three = split(r, theta)[0], split(r, theta, ncopies=3)
        rr.check_split(r, theta, *one)
        assert all(np.array_equal(three[b][k], one[k]) for b in range(3) for k in range(3))
