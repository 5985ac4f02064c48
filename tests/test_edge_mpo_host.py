"""Host: the operators of tests/helpers/edge_mpo.py have the structure tests/test_gpu_fold_range.py assumes.

For every structure an oracle MPS is brought to the test's centre site with the oracle's own QR gauge moves, the two
environment blocks are built with env_update_left / env_update_right (complex128), and the blocks that deviate from
blk[0,0] 1 by less than 1e-13 in the max norm -- the library's own test for an identity-fed state -- are compared with the
sets and multiples the helper promises.  That is what entitles the GPU tests to demand the edge form with both sides
folded and a structured environment update, instead of accepting whichever form the library picked.
"""

import numpy as np
import pytest

from helpers import edge_mpo as em


def _blocks_at(orc, mpo, d, D, c, seed=1):
    """(envL[c], envR[c + 1]) of a random MPS in mixed-canonical form around site c"""
    L = len(mpo)
    cores = orc.synthetic_mps([d] * L, D, seed=seed)  # site 0 the centre, the others right-orthonormal
    left = np.ones((1, 1, 1), dtype=np.complex128)
    for p in range(c):
        A, sval = orc.qr_psi2Asigma(cores[p])
        cores[p] = A
        left = orc.env_update_left(left, A, mpo[p])
        cores[p + 1] = np.tensordot(sval, cores[p + 1], axes=(1, 0))
    right = np.ones((1, 1, 1), dtype=np.complex128)
    for p in range(L - 1, c, -1):
        right = orc.env_update_right(right, cores[p], mpo[p])
    return left, right


def _identity_states(blk):
    """{state: multiple} of the blocks blk[:, c, :] within 1e-13 (max norm) of blk[0, c, 0] times the identity"""
    out = {}
    for c in range(blk.shape[1]):
        b = blk[:, c, :]
        if np.abs(b - b[0, 0] * np.eye(b.shape[0])).max() < 1e-13:
            out[c] = b[0, 0]
    return out


# (structure, L, d, M, D, centre): the operator shapes of the GPU module -- the plain chain at the corners of the kernels'
# range, the other structures at the shapes of its part 3
CASES = [
    ("plain", 6, 16, 32, 64, 2),
    ("plain", 7, 4, 64, 48, 3),
    ("plain", 7, 4, 65, 48, 3),
    ("plain", 7, 5, 17, 70, 3),
    ("plain", 7, 6, 33, 65, 3),
    ("plain", 6, 7, 12, 40, 2),
    ("plain", 7, 4, 10, 32, 3),
    ("plain", 7, 4, 10, 31, 3),
    ("plain", 6, 12, 6, 32, 2),
    ("weighted", 8, 4, 12, 64, 4),
    ("zero", 8, 4, 12, 64, 3),
    ("zero", 8, 4, 12, 64, 4),
    ("both", 8, 4, 12, 64, 4),
    ("pass", 8, 4, 12, 64, 4),
    ("sum2", 10, 3, 12, 50, 5),
]


@pytest.mark.parametrize("name,L,d,M,D,c", CASES)
def test_structure_at_the_centre(name, L, d, M, D, c):
    from oracle import tdvp_oracle as orc

    mpo, want = em.structure(name, L, d, M, c, seed=0)
    assert mpo[c].shape == (M, d, d, M)
    left, right = _blocks_at(orc, mpo, d, D, c)
    assert left.shape[1] == M and right.shape[1] == M
    S, E = _identity_states(left), _identity_states(right)
    assert set(S) == set(want["S"]) and set(E) == set(want["E"]), (sorted(S), sorted(E))
    for got, exp in ((S, want["S"]), (E, want["E"])):
        for k, v in exp.items():
            assert abs(got[k] - v) < 1e-13, (k, got[k], v)  # exact zeros included: abs(0 - 0.0)
    if name == "zero":
        assert all(not left[:, k, :].any() for k in range(1, M - 1))  # exactly zero, not merely small
    nz = np.abs(mpo[c]).max(axis=(1, 2)) > 0
    general = [(a, b) for a in range(M) for b in range(M) if nz[a, b] and a not in S and b not in E]
    assert bool(general) == want["general_block"], general
    if name == "pass":
        assert general == [(M - 2, M - 2)]


def test_zero_blocks_end_one_site_further():
    """the "zero" structure solved one site right of its centre: the states 1 .. M-2 are general there"""
    from oracle import tdvp_oracle as orc

    L, d, M, D, c = 8, 4, 12, 64, 3
    mpo, _ = em.structure("zero", L, d, M, c, seed=0)
    left, right = _blocks_at(orc, mpo, d, D, c + 1)
    assert set(_identity_states(left)) == {0} and set(_identity_states(right)) == {M - 1}


def test_plain_is_the_projects_synthetic_chain():
    from pytdscf_amd import synthetic as syn

    for a, b in zip(em.fsm_mpo(6, 3, 7, seed=5), syn.synthetic_mpo(6, 3, 7, seed=5)):
        assert np.array_equal(a, b)


def test_direct_sum_and_added_state_as_dense_operators():
    """on a short chain, as d^L x d^L matrices: the direct sum is the sum; an added state adds feed_op x drain_op (with
    identities in between and outside) and nothing else"""
    L, d = 4, 2
    a, b = em.fsm_mpo(L, d, 4, seed=1, alpha=0.9), em.fsm_mpo(L, d, 5, seed=2, beta=-0.8)
    s = em.direct_sum([a, b])
    assert [w.shape for w in s] == [(1, d, d, 9), (9, d, d, 9), (9, d, d, 9), (9, d, d, 1)]
    assert np.allclose(em.dense(s), em.dense(a) + em.dense(b), rtol=0, atol=1e-15)

    rng = np.random.default_rng(3)
    A, B = rng.standard_normal((d, d)), rng.standard_normal((d, d))
    base = em.fsm_mpo(L, d, 4, seed=1)
    ext, p = em.add_state(base, 1, A, 3, B)
    assert p == 3 and ext[1].shape == (5, d, d, 5)
    term = np.kron(np.kron(np.eye(d), A), np.kron(np.eye(d), B))
    assert np.allclose(em.dense(ext), em.dense(base) + term, rtol=0, atol=1e-15)
    ext, _ = em.add_state(base, 0, A, L - 1, B)
    term = np.kron(np.kron(A, np.eye(d)), np.kron(np.eye(d), B))
    assert np.allclose(em.dense(ext), em.dense(base) + term, rtol=0, atol=1e-15)
