"""GPU: nearest-neighbour (pair) gates and jump channels of the batched trajectories (k_batch_pair: the channel walk with
merge, apply and a truncated re-split by a one-sided Jacobi SVD inside the workgroup; TDVPBatch.set_gates / set_jumps with
bond keys, pair_jump_counts, discarded_weight; propagate_trajectories(jumps={(q, q + 1): B})).

The sharp tests are parity with the NumPy trajectory step of tests/helpers/pair_oracle.py ON THE SAME NUMBERS, at the bars
of tests/test_gpu_batch_jump.py: fidelity defect 1 - |<a|b>| / (|a| |b|) < 1e-10, norm to 1e-12, site RDMs to 1e-9, counters
exact.  The inputs are tests/helpers/pair_cases.py; tests/test_batch_pair_host.py shows from the oracle alone that none of
their decisions or truncations sits on an edge."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _batch(case, starts=None, integrator="lanczos", **kw):
    from pytdscf_amd import TDVPBatch

    starts = case["starts"] if starts is None else starts
    if "thresh" in case:
        kw.setdefault("thresh", case["thresh"])
    bt = TDVPBatch(len(starts), len(case["dims"]), integrator=integrator, conserve_norm=False, **kw)
    bt.set_mpo(case["mpo"])
    for e, c in zip(bt.engines, starts):
        e.set_mps(c)
    return bt


def _set(bt, case, **kw):
    from helpers import pair_cases as pc

    gates, jumps = pc.batch_tables(case["channels"])
    if gates:
        bt.set_gates(gates)
    if jumps:
        bt.set_jumps(jumps, seed=case["seed"], **kw)


def _defect(a, b):
    from oracle import tdvp_oracle as orc

    na, nb = np.sqrt(abs(orc.overlap(a, a))), np.sqrt(abs(orc.overlap(b, b)))
    return 1 - abs(orc.overlap(a, b)) / (na * nb), abs(na - nb)


def _bytes(bt, which=None):
    return [[c.tobytes() for c in bt[r].get_mps()] for r in (range(len(bt)) if which is None else which)]


def _right_orthonormal(cores):
    """max |B B^+ - 1| over the sites 1 .. L-1 (the centre is at site 0 after a step)"""
    worst = 0.0
    for c in cores[1:]:
        m = c.reshape(c.shape[0], -1)
        worst = max(worst, np.abs(m @ m.conj().T - np.eye(m.shape[0])).max())
    return worst


def _parity(case, ref, bt, tag):
    from oracle import tdvp_oracle as orc

    L = len(case["dims"])
    for r, (cores, dec, spl) in enumerate(ref):
        got = bt[r].get_mps()
        f, dn = _defect(cores, got)
        drdm = max(np.abs(orc.site_rdm(cores, p) - bt[r].site_rdm(p)).max() for p in range(L))
        orth = _right_orthonormal(got)
        print(f"{tag} replica {r}: fidelity defect {f:.2e} norm {dn:.2e} rdm {drdm:.2e} |B B^+ - 1| {orth:.2e}")
        assert abs(f) < 1e-10 and dn < 1e-12 and drdm < 1e-9
        assert orth < 1e-12


@pytest.mark.parametrize("integrator", ["lanczos", "arnoldi"])
@pytest.mark.parametrize("d_mid", [2, 3])
def test_exact_split(d_mid, integrator):
    """Pair gates on all three bonds of an L = 4 chain with maximal bonds and a one-site gate, 3 steps against the oracle.
    d_mid = 2: dims (2, 2, 2, 2), D = 4.  d_mid = 3: dims (2, 3, 3, 2) -- unequal d0, d1 on the outer bonds -- with D = 6,
    the maximal middle bond, so that the split stays exact (at D = 4 a generic gate on (1, 2) has Schmidt rank 6)."""
    from helpers import pair_cases as pc

    case = pc.exact(d_mid)
    ref = pc.reference("exact", integrator, d_mid)
    bt = _batch(case, integrator=integrator)
    _set(bt, case)
    bt.propagate(case["dt"], case["nsteps"])
    assert bt.statuses == [0] * len(bt)
    disc = bt.discarded_weight()
    nsplit = 3 * case["nsteps"]
    print(f"d_mid {d_mid} {integrator}: discarded weight per replica {disc} over {nsplit} splits each")
    assert disc.shape == (len(bt),) and np.all(disc >= 0) and np.all(disc < 1e-24 * nsplit)  # < 1e-24 per split
    _parity(case, ref, bt, f"d_mid {d_mid} {integrator}")
    assert bt.pair_jump_counts().sum() == 0 and bt.jump_counts().sum() == 0
    bt.close()


def test_truncating_split():
    """L = 6, d = 2, D = 4, a random two-site unitary on (2, 3): an 8 x 8 theta of full rank cut to 4, 2 steps"""
    from helpers import pair_cases as pc

    case = pc.truncating()
    ref = pc.reference("truncating", "lanczos")
    bt = _batch(case)
    _set(bt, case)
    bt.propagate(case["dt"], case["nsteps"])
    assert bt.statuses == [0] * len(bt)
    _parity(case, ref, bt, "truncating")
    disc = bt.discarded_weight()
    for r, (_, _, spl) in enumerate(ref):
        want = sum(s[2] for s in spl)
        print(f"replica {r}: discarded weight {disc[r]:.15e}, oracle {want:.15e}, relative difference {abs(disc[r] - want) / want:.2e}")
        assert want > 1e-6  # the case does truncate
        assert abs(disc[r] - want) <= 1e-10 * want
    bt.close()


@pytest.mark.parametrize("d", [4, 3])
def test_larger_and_odd_shapes(d):
    """L = 6, D = 20, pair gates on (1, 2), (2, 3), (3, 4), one step: d = 4 gives theta of 16 x 80 (two columns per lane),
    64 x 64 cut to 20 (several pairs per wave, several elements per thread) and 80 x 16 (more rows than columns); d = 3
    gives 9 x 60, 27 x 27 cut to 20 and 60 x 9: odd row counts, where a slot of the round-robin rests."""
    from helpers import pair_cases as pc

    case = pc.large(d)
    ref = pc.reference("large", "lanczos", d)
    bt = _batch(case)
    _set(bt, case)
    bt.propagate(case["dt"], case["nsteps"])
    assert bt.statuses == [0] * len(bt)
    _parity(case, ref, bt, f"large d = {d}")
    disc = bt.discarded_weight()
    for r, (_, _, spl) in enumerate(ref):
        want = sum(s[2] for s in spl)
        print(f"replica {r}: discarded weight {disc[r]:.15e}, oracle {want:.15e}")
        assert want > 1e-6 and abs(disc[r] - want) <= 1e-10 * want
    bt.close()


def test_rank_deficient_theta():
    """A product start padded to D = 4 and an entangling gate on (2, 3) at L = 6: theta has rank 2 < 4, so two of the four
    rows of B(3) come from the orthonormal completion.  H has one-site terms only: the state after the step is the dense
    (x)_p exp(-i h_p dt / 2) . G . (x)_p exp(-i h_p dt / 2) |start> whatever completes the null space."""
    from helpers import jump_oracle as jo
    from helpers import pair_cases as pc
    from helpers import pair_oracle as po
    from scipy.linalg import expm

    case = pc.rank_deficient()
    dims, dt = case["dims"], case["dt"]
    U = np.ones((1, 1), dtype=complex)
    for h in case["h"]:
        U = np.kron(U, expm(-0.5j * dt * h))
    G = po.embed_pair(case["channels"][(2, 3)][1], 2, dims)
    bt = _batch(case, integrator="arnoldi")
    _set(bt, case)
    bt.propagate(dt, 1)
    assert bt.statuses == [0] * len(bt)
    assert np.all(bt.discarded_weight() < 1e-24)
    for r, start in enumerate(case["starts"]):
        want = U @ (G @ (U @ jo.dense_state(start)))
        got_cores = bt[r].get_mps()
        got = jo.dense_state(got_cores)
        f = 1 - abs(np.vdot(want, got)) / (np.linalg.norm(want) * np.linalg.norm(got))
        orth = _right_orthonormal(got_cores)
        sv = np.linalg.svd(got.reshape(8, 8), compute_uv=False)
        print(f"replica {r}: defect to the dense state {f:.2e}, norm - 1 {bt[r].norm() - 1:.2e}, |B B^+ - 1| {orth:.2e}, "
              f"Schmidt values across (2|3) {sv[:3] / sv[0]}")
        assert abs(f) < 1e-10
        assert orth < 1e-12
        assert abs(bt[r].norm() - 1) < 1e-12
        assert sv[1] > 0.1 * sv[0] and sv[2] < 1e-9 * sv[0]  # rank 2 in a bond of 4
    bt.propagate(dt, 1)  # the following sweeps keep the norm (the gate is unitary)
    assert bt.statuses == [0] * len(bt)
    for r in range(len(bt)):
        assert abs(bt[r].norm() - 1) < 1e-12, r
        assert _right_orthonormal(bt[r].get_mps()) < 1e-12
    bt.close()


def test_pair_jumps_decision_by_decision():
    """Hopping {sqrt(g) s^- s^+, sqrt(g) s^+ s^-, complement} on (2, 3) of an L = 6 spin chain next to a one-site jump
    channel on site 2, B = 6, 4 steps: both counters equal the oracle's choices exactly."""
    from helpers import pair_cases as pc
    from helpers import pair_oracle as po

    case = pc.hopping()
    ref = pc.reference("hopping", "lanczos")
    L = len(case["dims"])
    bt = _batch(case)
    _set(bt, case)
    bt.propagate(case["dt"], case["nsteps"])
    assert bt.statuses == [0] * len(bt)
    one, pair = bt.jump_counts(), bt.pair_jump_counts()
    assert one.shape == pair.shape == (len(bt), L, 16)
    for r, (_, dec, _) in enumerate(ref):
        want_one, want_pair = po.counts_of(dec, L)
        print(f"replica {r}: choices {[(d[0], d[1]) for d in dec]}")
        assert np.array_equal(one[r], want_one), r
        assert np.array_equal(pair[r], want_pair), r
    assert pair.sum() == one.sum() == len(bt) * case["nsteps"]
    assert pair[:, [0, 1, 3, 4, 5]].sum() == 0
    _parity(case, ref, bt, "hopping")
    disc = bt.discarded_weight()
    for r, (_, _, spl) in enumerate(ref):
        want = sum(s[2] for s in spl)
        assert abs(disc[r] - want) <= 1e-10 * want + 1e-24 * len(spl)
    bt.close()


def test_bits_do_not_depend_on_the_batch():
    from helpers import pair_cases as pc
    from oracle import tdvp_oracle as orc

    case = pc.hopping()
    starts = case["starts"]

    def run(B, where, plan):
        filler = orc.canonicalize_site0(orc.synthetic_mps(list(case["dims"]), case["D"], seed=99), scale=1.0)
        cores = [filler] * B
        ids = [1000 + i for i in range(B)]
        for t, r in enumerate(where):
            cores[r], ids[r] = starts[t], t
        bt = _batch(case, cores)
        _set(bt, case, trajectory_ids=ids)
        for n in plan:
            bt.propagate(case["dt"], n)
        out = _bytes(bt, where), bt.pair_jump_counts()[list(where)], bt.discarded_weight()[list(where)].tobytes()
        bt.close()
        return out

    small = run(6, range(6), (4,))
    big = run(70, (3, 69, 0, 41, 17, 64), (4,))
    assert small[0] == big[0]  # the same trajectory ids anywhere in any batch: the same bytes
    assert np.array_equal(small[1], big[1]) and small[2] == big[2]
    split = run(6, range(6), (2, 2))
    assert small[0] == split[0]  # the step counter and the discarded weights run on across calls
    assert np.array_equal(small[1], split[1]) and small[2] == split[2]
    assert small[1].sum() == 6 * 4


def test_setting_then_removing_a_pair_channel_changes_nothing():
    from helpers import pair_cases as pc

    case = pc.hopping()
    gates, jumps = pc.batch_tables(case["channels"])
    dt = case["dt"]
    plain = _batch(case, case["starts"][:3])
    plain.propagate(dt, 1)
    n0 = plain.launches()
    plain.propagate(dt, 2)
    assert plain.launches() - n0 == 2 * 2

    bt = _batch(case, case["starts"][:3])
    bt.set_jumps({(2, 3): jumps[(2, 3)]}, seed=1)
    bt.set_gates({(0, 1): np.eye(4)})
    bt.set_jumps({(2, 3): None})
    bt.set_gates({(0, 1): None})
    bt.propagate(dt, 1)
    n0 = bt.launches()
    bt.propagate(dt, 2)
    assert bt.launches() - n0 == 2 * 2  # set and removed: the two launches per step of before
    assert _bytes(bt) == _bytes(plain)
    assert bt.pair_jump_counts().sum() == 0 and np.all(bt.discarded_weight() == 0)
    bt.set_jumps({(2, 3): jumps[(2, 3)]}, seed=1)
    n0 = bt.launches()
    bt.propagate(dt, 2)
    assert bt.launches() - n0 == 3 * 2  # with a pair channel: exactly one more per step
    assert bt.pair_jump_counts().sum() == 3 * 2
    assert _bytes(bt) != _bytes(plain)
    bt.set_jumps({2: jumps[2]}, seed=1)  # a one-site channel next to it: still one more
    n0 = bt.launches()
    bt.propagate(dt, 1)
    assert bt.launches() - n0 == 3
    plain.close()
    bt.close()


def test_refusals():
    from helpers import pair_cases as pc
    from oracle import tdvp_oracle as orc

    case = pc.hopping()
    B = pc.hopping_ops()
    bt = _batch(case, case["starts"][:2])
    before = _bytes(bt)
    bt._handle()  # the library's batch object exists: the raw calls below reach the C entry point

    def refused(call, match):
        with pytest.raises(ValueError, match=match):
            call()
        assert _bytes(bt) == before  # the engines are untouched

    refused(lambda: bt.set_gates({(5, 6): np.eye(4)}), r"\(5, 6\).*out of range")
    refused(lambda: bt._push_channel((5, 6), 1, np.eye(4).reshape(1, 2, 2, 2, 2).astype(complex)), r"bond \(5, 6\).*out of range.*6 sites")
    refused(lambda: bt._push_channel((-1, 0), 1, np.eye(4).reshape(1, 2, 2, 2, 2).astype(complex)), r"bond \(-1, 0\).*out of range")
    refused(lambda: bt.set_gates({(2, 3): np.eye(6)}), r"\(2, 3\).*order 6.*2 x 2")
    refused(lambda: bt._push_channel((2, 3), 1, np.eye(6).reshape(1, 2, 3, 2, 3).astype(complex)), r"bond \(2, 3\).*2 x 3.*2 x 2")
    refused(lambda: bt.set_jumps({(2, 3): B[:1]}), r"bond \(2, 3\).*2 to 16.*got 1")
    refused(lambda: bt.set_jumps({(2, 3): np.stack([np.eye(4)] * 17) / np.sqrt(17)}), r"bond \(2, 3\).*2 to 16.*got 17")
    assert not bt._channels
    bt.propagate(case["dt"], 1)  # nothing stuck: no channel is set, the engines still step
    assert bt.statuses == [0, 0] and bt.pair_jump_counts().sum() == 0
    bt.set_jumps({(2, 3): B}, seed=1)
    before = _bytes(bt)
    refused(lambda: bt.sweep(case["dt"], True), "half-sweep")
    refused(lambda: bt.set_jumps({(1, 2): B[:1]}), r"bond \(1, 2\).*2 to 16")  # a refused table changes nothing:
    assert set(bt._channels) == {(2, 3)}
    bt.propagate(case["dt"], 1)
    assert bt.statuses == [0, 0] and bt.pair_jump_counts()[:, 2].sum() == 2
    bt.close()

    cold = _batch(case, case["starts"][:2], relax=True)
    before_cold = _bytes(cold)
    with pytest.raises(ValueError, match=r"bond \(2, 3\).*imaginary time"):
        cold.set_jumps({(2, 3): B})
    with pytest.raises(ValueError, match=r"bond \(2, 3\).*imaginary time"):
        cold.set_gates({(2, 3): np.eye(4)})
    assert _bytes(cold) == before_cold
    cold.close()

    # a shape beyond 128 rows: d = 4, bonds (4, 16, 33, 16, 4): theta of bond (3, 4) is (33 * 4) x (4 * 4)
    from pytdscf_amd import TDVPBatch

    dims = [4] * 6
    wide = TDVPBatch(2, 6, conserve_norm=False)
    wide.set_mpo(orc.synthetic_mpo(6, 4, 3, seed=1))
    for r, e in enumerate(wide.engines):
        e.set_mps(orc.canonicalize_site0(orc.synthetic_mps(dims, 33, seed=5 + r), scale=1.0))
    assert tuple(wide[0].get_site_shape(3)[:3]) == (33, 4, 16)
    before_wide = _bytes(wide)
    with pytest.raises(ValueError, match=r"bond \(3, 4\).*132 x 16.*at most 128"):
        wide.set_gates({(3, 4): np.eye(16)})
    assert _bytes(wide) == before_wide
    wide.propagate(0.1, 1)
    assert wide.statuses == [0, 0]
    wide.close()


def test_an_annihilating_pair_channel_stops_one_replica_only():
    """H diagonal in the product basis, so spins 1 and 2 of replica 1 stay |0>|0> exactly; both operators are multiples of
    |11><11|: W == 0 for that replica, which reports the zero-norm status; the others finish."""
    from helpers import spin_bath as sb
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import TDVPBatch, _lib
    from pytdscf_amd.mps import product_state_cores

    dims = [2, 2, 2, 2]
    sz = np.diag([0.5, -0.5]).astype(complex)
    mpo = sb.sop_mpo([(1.0, {0: sz, 1: sz}), (0.7, {1: sz, 2: sz}), (0.4, {2: sz, 3: sz}), (0.3, {1: sz})], dims)
    P11 = np.diag([0.0, 0.0, 0.0, 1.0]).astype(complex)
    B = np.stack([np.sqrt(0.25) * P11, np.sqrt(0.75) * P11])
    up, dn, mix = [1, 0], [0, 1], [1, 1]
    starts = [[up, dn, mix, up], [mix, up, up, dn], [dn, mix, dn, mix]]
    bt = TDVPBatch(3, 4, integrator="arnoldi")
    bt.set_mpo(mpo)
    for e, s in zip(bt.engines, starts):
        e.set_mps(orc.canonicalize_site0(product_state_cores(s, 4, space="hilbert"), scale=1.0))
    bt.set_jumps({(1, 2): B}, seed=5)
    with pytest.raises(ValueError, match="zero"):
        bt.propagate(0.2, 2)
    assert bt.statuses == [0, _lib.EINVAL, 0]
    assert "zero" in _lib.load().mitdvp_last_error(bt[1]._h).decode()
    counts = bt.pair_jump_counts()
    assert counts[1].sum() == 0 and counts[0].sum() == 2 and counts[2].sum() == 2
    for r in (0, 2):
        assert abs(bt[r].norm() - 1) < 1e-12  # the norm before a jump is kept
        for p in (1, 2):
            assert abs(bt[r].site_rdm(p)[1, 1] - 1) < 1e-12  # after |11><11| both spins are |1>
    with pytest.raises(ValueError):
        bt[1].propagate(0.2)  # stopped in the middle of a step: it must be given its tensors again
    bt.close()


def test_end_to_end_through_propagate_trajectories():
    """The L = 4 spin chain of tests/helpers/pair_cases.py at full bond (nothing is truncated, one-site TDVP is exact up to
    the Krylov threshold) with the hopping channel (gamma = 0.9) on (2, 3), 4 starts x 256 replicas = 1024 trajectories, 3 steps: the
    mean density of site 2 at the last record against the dense map.  Tolerance per real number by Hoeffding, built as
    tests/test_gpu_batch_jump.py builds its own (independent trajectories, entries of a pure-state density of norm <= 1
    lie in [-1, 1]): t = sqrt(2 ln(2 E / 1e-6) / B) with E = 8 compared numbers.  It cannot pass trivially: the dense
    results with and without the channel differ by >= 3 t in one entry, asserted from dense CPU math."""
    from helpers import jump_oracle as jo
    from helpers import pair_cases as pc
    from helpers import pair_oracle as po
    from pytdscf_amd import Exciton, Model, units
    from pytdscf_amd.trajectories import propagate_trajectories

    dims, nsteps, rps, dt = [2, 2, 2, 2], 3, 256, 0.3
    mpo = pc._spin_chain_mpo(4)
    Bh = pc.hopping_ops(0.9)
    H = jo.dense_operator(mpo)
    up, dn = [1, 0], [0, 1]
    starts = [[up, dn, dn, up], [dn, up, dn, up], [up, up, dn, up], [dn, dn, dn, up]]

    def dense(channels):
        acc = 0
        for start in starts:
            v = np.ones(1, dtype=complex)
            for w in start:
                v = np.kron(v, np.asarray(w, dtype=complex) / np.linalg.norm(w))
            rho = np.outer(v, v.conj())
            for _ in range(nsteps):
                rho = po.dense_channel_step(rho, H, dt, channels, dims)
            acc = acc + np.einsum("abcdabed->ce", rho.reshape(2, 2, 2, 2, 2, 2, 2, 2))
        return acc / len(starts)

    def reals(x):
        return np.concatenate([x.real.ravel(), x.imag.ravel()])

    B = rps * len(starts)
    with_ch, without = dense({(2, 3): ("jump", Bh)}), dense({})
    E = reals(with_ch).size
    t = np.sqrt(2 * np.log(2 * E / 1e-6) / B)
    gap = np.abs(reals(with_ch) - reals(without)).max()
    assert E == 8 and gap >= 3 * t, (gap, t)

    model = Model([Exciton(nstate=d) for d in dims], operators={"hamiltonian": mpo}, bond_dim=64)
    out = propagate_trajectories(model, starts, maxstep=nsteps + 1, stepsize=dt * units.au_in_fs,
                                 reduced_density=([(2, 2)], 1), integrator="arnoldi", conserve_norm=False,
                                 jumps={(2, 3): Bh}, seed=11, replicas_per_start=rps)
    mean = out["mean"][(2, 2)]
    assert mean.shape == (nsteps + 1, 2, 2)
    err = np.abs(reals(mean[-1]) - reals(with_ch)).max()
    print(f"B = {B}: max |mean - dense| = {err:.3e} (t = {t:.3f}; with / without the channel differ by {gap:.3f})")
    assert err < t
