"""Host: the structured environment update taking the general states' operator from the local solve's folded operator
(tests/helpers/env_reuse.py, the NumPy twin of EdgeCache::rebuild's decision and of both formulas of
Engine::env_update_fold), and the one-pass combine of two Strassen levels against the two passes it replaces.

At d = 3, D = 5, M = 6 the twin's update, with the reuse and without it, must equal the oracle's plain contraction
(oracle/tdvp_oracle.py::env_update_left / env_update_right) to 1e-12 relative in the max norm for every structure of
helpers/edge_mpo.structure that takes the edge form, in both directions; the decisions are those of the table below.
The site tensor is a random one, not an isometry: neither formula needs one.
"""

import numpy as np
import pytest

from helpers import edge_mpo as em
from helpers import env_reuse as er
from helpers import strassen_blocks as sb
from helpers import strassen_levels as sl

L_, D_, DIM, M_, C_ = 5, 3, 5, 6, 2
TOL = 1e-12

# structure -> (forward, backward): whether the update reuses the solve's operator
WANT = {"plain": (True, True), "weighted": (True, True), "zero": (True, True), "both": (True, False), "sum2": (False, False)}


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _crandn(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


@pytest.mark.parametrize("name", list(WANT))
def test_decisions_and_formulas_against_the_oracle(name):
    from oracle import tdvp_oracle as orc

    mpo, want = em.structure(name, L_, D_, M_, C_)
    S, E = want["S"], want["E"]
    W = mpo[C_]
    Lb, Rb = er.blocks_at(orc, mpo, D_, DIM, C_)
    assert Lb.shape == (DIM, M_, DIM) and Rb.shape == (DIM, M_, DIM)
    rng = np.random.default_rng(5)
    T = _crandn(rng, DIM, D_, DIM)
    fwd, bwd = er.decide(W, S, E)
    assert (fwd["reuse"], bwd["reuse"]) == WANT[name]
    if name == "weighted":  # the multiples of the out states are not 1, so neither is the factor of the closing product
        assert abs(fwd["alpha"] - 1) > 0.1 and abs(bwd["alpha"] - 1) > 0.1
        assert abs(fwd["alpha"] * E[M_ - 1] - 1) < 1e-15 and abs(bwd["alpha"] * S[0] - 1) < 1e-15
    if bwd["reuse"]:  # the Gram core of the backward reuse: column c0 zero, every other column as it was
        c0 = bwd["t0"][0]
        assert not bwd["ws_reuse"][:, :, c0].any() and np.abs(bwd["ws"][:, :, c0]).max() > 0
        keep = [c for c in range(M_) if c != c0]
        assert np.array_equal(bwd["ws_reuse"][:, :, keep], bwd["ws"][:, :, keep])
    if fwd["reuse"]:
        assert np.array_equal(fwd["ws_reuse"], fwd["ws"])
    ref_f, ref_b = orc.env_update_left(Lb, T, W), orc.env_update_right(Rb, T, W)
    for allow in (True, False):
        got_f, ran_f = er.update_forward(W, Lb, T, S, E, allow)
        got_b, ran_b = er.update_backward(W, Rb, T, S, E, allow)
        assert (ran_f, ran_b) == ((fwd["reuse"], bwd["reuse"]) if allow else (False, False))
        rf, rb = _rel(got_f, ref_f), _rel(got_b, ref_b)
        print(f"{name} reuse allowed {allow}: forward {rf:.3e} (reuse {ran_f}), backward {rb:.3e} (reuse {ran_b})")
        assert rf < TOL and rb < TOL


def test_a_refused_reuse_would_be_wrong():
    """'both', backward: the solve's GR also holds the blocks out of the second identity state of S, so the reuse formula
    applied regardless misses the oracle -- the refusal is needed, not a matter of caution."""
    from oracle import tdvp_oracle as orc

    mpo, want = em.structure("both", L_, D_, M_, C_)
    S, E = want["S"], want["E"]
    W = mpo[C_]
    _, Rb = er.blocks_at(orc, mpo, D_, DIM, C_)
    B = _crandn(np.random.default_rng(6), DIM, D_, DIM)
    rec = er.decide(W, S, E)[1]
    assert not rec["reuse"] and rec["t0"] == [0]
    ws0 = rec["ws"].copy()
    ws0[:, :, 0] = 0
    Bm = B.reshape(DIM, D_ * DIM)
    forced = er._gram_part(np.ascontiguousarray(B.transpose(2, 1, 0)), ws0)
    forced[:, 0, :] += (1.0 / S[0]) * (Bm.conj() @ (Bm @ er.solve_gr(W, Rb, S, E).T).T)
    assert _rel(forced, orc.env_update_right(Rb, B, W)) > 1e-6


@pytest.mark.parametrize("qm,qn", [(1, 1), (3, 5), (10, 7)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_one_pass_combine_is_the_two_passes_bit_for_bit(qm, qn, accumulate):
    """49 random quarter-size products: strassen_combine2's twin against the 49 -> 7 pass into the head of the products'
    buffer followed by the 7 -> out pass (helpers/strassen_levels.combine_second_level, strassen_blocks.combine)"""
    rng = np.random.default_rng(7 + qm)
    hm, hn = 2 * qm, 2 * qn
    M49 = _crandn(rng, 49 * qm * qn)
    out = _crandn(rng, 4 * qm, 4 * qn) if accumulate else None
    buf = np.full(7 * hm * hn + 49 * qm * qn, np.nan + 0j)
    buf[7 * hm * hn:] = M49
    sl.combine_second_level(buf, qm, qn)
    two = sb.combine(buf[:7 * hm * hn], hm, hn, out)
    one = er.combine2(M49, qm, qn, out)
    assert one.shape == two.shape == (4 * qm, 4 * qn)
    assert np.array_equal(one, two)
