"""GPU: MPO matrix elements between the replicas of a batch and their snapshots (TDVPBatch.set_cross_mpo / cross_mpo,
propagate(observe=dict(cross_mpo=True)): k_batch_cross_mpo forms every entry with one launch, one workgroup per entry;
k_batch_mean sums them on the device) and trajectories.correlation_function with operators that are sums over the chain.

The pin is the dense pair of states built from the tensors the engines hand back, with the MPO applied to the ket vector
core by core (helpers/cross_mpo_cases.dense_value): values to 1e-12 SCALE |a| |b|, the relative bar of
tests/test_gpu_batch_cross.py times the operator scale of tests/test_gpu_batch_expect.py; the NumPy twin of the walk is
inside a tenth of it (tests/test_batch_cross_mpo_host.py).  Every case prints its worst defect as a fraction of its bar.
The shapes are those of the spectra tests, the smallest at which each part can go wrong:
  mixed  dims (2, 3, 2, 4, 2), D = 6: ragged physical dimensions, a bond narrower than the tile
  odd    dims (3,) * 5, D = 7: every size odd, a multiple of no tile
  wide   dims (2,) * 12, D = 40: bonds past the 32-wide tile and the 16-deep K step, more than one tile per product
and per shape the five operators of helpers/expect_cases (MPO bonds 1 to 8, one non-Hermitian with a complex shift, and
operator 0 with its shift of 0.1)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = 0.2
B = 3


def _give(e, name):
    from helpers import cross_mpo_cases as xc

    for label in xc.LABELS:
        _, shift, mpo = xc.case(name, label)
        e.set_mpo(mpo, xc.OP_ID[label], shift=shift)


def _batch(name, nrep=B, states=None, seed=30, **kw):
    """replicas with random states of norms 0.7, 0.9, 1.1, ..., every one carrying the five operators; no rescaling in a
    step, so the norms stay apart"""
    from helpers import cross_mpo_cases as xc
    from pytdscf_amd import TDVPBatch

    dims, _ = xc.SHAPES[name]
    kw = dict(dict(integrator="arnoldi", conserve_norm=False), **kw)
    bt = TDVPBatch(nrep, len(dims), **kw)
    for e, cores in zip(bt.engines, states if states is not None else xc.random_states(name, nrep, seed)):
        _give(e, name)
        e.set_mps(cores)
    return bt


def _tensors(bt):
    return [e.get_mps() for e in bt.engines]


def _same_tensors(a, b):
    return all(np.array_equal(x, y) for s, t in zip(a, b) for x, y in zip(s, t))


def _stepped(name):
    """a batch with a snapshot of the start and one step behind it: (batch, state(i) for every state index)"""
    bt = _batch(name)
    old = _tensors(bt)
    bt.snapshot()
    bt.propagate(DT, 1)
    now = _tensors(bt)
    return bt, old, now, (lambda i: now[i] if i < B else old[i - B])


@pytest.mark.parametrize("name", ["mixed", "odd", "wide"])
def test_values_equal_the_dense_pin(name):
    """all five operators; a = b and a != b in both orders; snapshot bras and kets after a step that moved the states; one
    entry, fewer entries than replicas, more entries than replicas"""
    from helpers import cross_cases as cc
    from helpers import cross_mpo_cases as xc

    bt, old, now, state = _stepped(name)
    assert max(c.shape[2] for c in now[0]) == xc.SHAPES[name][1]
    unit = cc.norm_of(old[2]) * cc.norm_of(now[2])
    assert abs(cc.walk(old[2], now[2]) - cc.walk(now[2], now[2])) > 1e-6 * unit  # the step moved the states off their snapshots
    s = bt.snap
    pairs = [(0, 0), (0, 1), (1, 0), (2, 2), (s(2), 1), (2, s(1)), (s(0), 0), (s(1), s(2)), (1, 2)]
    entries = [(a, b, xc.OP_ID[label]) for label in xc.LABELS for a, b in pairs]
    assert len(entries) > B
    norms = {i: xc.norm_of(state(i)) for i in range(2 * B)}
    worst, small = 0.0, np.inf
    for P in (1, 2, len(entries)):
        use = entries[7:7 + P] if P < 3 else entries
        bt.set_cross_mpo(use)
        got = bt.cross_mpo()
        assert got["values"].shape == (len(use),) and got["values"].dtype == np.complex128
        for (a, b, k), v in zip(use, got["values"]):
            label = next(x for x in xc.LABELS if xc.OP_ID[x] == k)
            _, shift, mpo = xc.case(name, label)
            unit = xc.scale(name, label) * norms[a] * norms[b]
            pin = xc.dense_value(state(a), state(b), mpo, shift)
            small = min(small, abs(xc.walk(state(a), state(b), mpo, shift)) / (1e-6 * unit))
            worst = max(worst, abs(v - pin) / (xc.BAR * unit))
        assert abs(got["mean"] - got["values"].mean()) < 1e-13 * np.abs(got["values"]).max()
    print(f"{name}: worst |device - dense pin| = {worst:.3e} of the bar 1e-12 SCALE |a| |b|; smallest |twin value| = {small:.3e} of "
          "1e-6 SCALE |a| |b|")
    assert small > 1  # from the twin alone: nothing here compares two zeros
    assert worst < 1
    v = got["values"]
    w = np.linspace(0.5, 1.5, len(entries))
    assert abs(bt.cross_mpo(weights=w)["mean"] - (w * v).sum()) < 1e-13 * np.abs(v).max() * w.sum()
    bt.close()


@pytest.mark.parametrize("name", ["mixed", "wide"])
def test_diagonal_entries_are_expect_and_conjugate_pairs_conjugate(name):
    """(r, r, k) with the centre at site 0 against expect() of (r, k) within the bar; (a, b, k) against the conjugate of
    (b, a, k) for the Hermitian operators within twice the bar (each is within the bar of the exact value)"""
    from helpers import cross_mpo_cases as xc

    bt, old, now, state = _stepped(name)
    ids = [xc.OP_ID[x] for x in xc.LABELS]
    bt.set_expect(ids)
    ex = bt.expect()["values"]
    bt.set_cross_mpo([(r, r, k) for r in range(B) for k in ids])
    diag = bt.cross_mpo()["values"].reshape(B, len(ids))
    norms = {i: xc.norm_of(state(i)) for i in range(2 * B)}
    worst = 0.0
    for r in range(B):
        for j, label in enumerate(xc.LABELS):
            worst = max(worst, abs(diag[r, j] - ex[r, j]) / (xc.BAR * xc.scale(name, label) * norms[r] ** 2))
    herm = [(a, b, xc.OP_ID[label]) for label in xc.HERMITIAN for a, b in ((0, 1), (2, bt.snap(0)), (bt.snap(1), bt.snap(2)))]
    bt.set_cross_mpo(herm + [(b, a, k) for a, b, k in herm])
    v = bt.cross_mpo()["values"]
    worst_h = 0.0
    for i, (a, b, k) in enumerate(herm):
        label = next(x for x in xc.LABELS if xc.OP_ID[x] == k)
        worst_h = max(worst_h, abs(v[i] - np.conj(v[len(herm) + i])) / (2 * xc.BAR * xc.scale(name, label) * norms[a] * norms[b]))
    bt.set_cross_mpo([(0, 1, xc.OP_ID["complex"]), (1, 0, xc.OP_ID["complex"])])
    c = bt.cross_mpo()["values"]
    assert abs(c[0] - np.conj(c[1])) > 1e-3 * norms[0] * norms[1]  # and not for the non-Hermitian one
    print(f"{name}: |(r, r, k) - expect| {worst:.3e} of the bar; |(a, b, k) - conj (b, a, k)| {worst_h:.3e} of twice the bar")
    assert worst < 1 and worst_h < 1
    bt.close()


def test_a_bond_1_operator_is_the_cross_entry_and_the_shift_adds_the_overlap():
    """a one-site operator given as an MPO of bond 1 equals the set_cross entry (a, b, site, O) within the bar; with a shift
    s the value is the no-shift value of the same cores plus s times the set_cross overlap, within the bar"""
    from helpers import cross_cases as cc
    from helpers import cross_mpo_cases as xc
    from helpers import spin_bath as sb

    name = "mixed"
    dims, _ = xc.SHAPES[name]
    bt, old, now, state = _stepped(name)
    norms = {i: xc.norm_of(state(i)) for i in range(2 * B)}
    pairs = [(0, 1), (1, 0), (2, bt.snap(1)), (bt.snap(0), 2), (1, 1)]
    worst = 0.0
    for site in (0, 2, len(dims) - 1):
        O = cc.random_op(dims[site], 11 + site)
        one = [np.ascontiguousarray(w, dtype=np.complex128) for w in sb.sop_mpo([(1.0, {site: O})], list(dims))]
        assert max(w.shape[3] for w in one) == 1
        for e in bt.engines:
            e.set_mpo(one, 7)
        bt.set_cross_mpo([(a, b, 7) for a, b in pairs])
        bt.set_cross([(a, b, site, O) for a, b in pairs])
        got, ref = bt.cross_mpo()["values"], bt.cross()["values"]
        for (a, b), x, y in zip(pairs, got, ref):
            worst = max(worst, abs(x - y) / (xc.BAR * np.linalg.norm(O, 2) * norms[a] * norms[b]))
            assert abs(y) > 1e-6 * norms[a] * norms[b]
    print(f"bond-1 operator: |cross_mpo - cross| {worst:.3e} of 1e-12 |O| |a| |b|")
    assert worst < 1
    # the shift: operator 8 has the cores of `local` and a complex scalar term, operator 2 the same cores and none
    _, _, mpo = xc.case(name, "local")
    s = 0.4 - 0.3j
    for e in bt.engines:
        e.set_mpo(mpo, 8, shift=s)
    bt.set_cross_mpo([(a, b, 8) for a, b in pairs] + [(a, b, xc.OP_ID["local"]) for a, b in pairs])
    bt.set_cross(pairs)
    v, ov = bt.cross_mpo()["values"], bt.cross()["values"]
    worst = 0.0
    for i, (a, b) in enumerate(pairs):
        unit = (xc.scale(name, "local") + abs(s)) * norms[a] * norms[b]
        worst = max(worst, abs(v[i] - (v[len(pairs) + i] + s * ov[i])) / (xc.BAR * unit))
        assert abs(s * ov[i]) > 1e-6 * unit
    print(f"shift: |value - (no-shift value + s overlap)| {worst:.3e} of the bar")
    assert worst < 1
    bt.close()


def test_bits_depend_on_the_entry_only_and_a_record_is_the_call():
    """the same entry alone, inside a longer list at another position, and in a batch of another B; a record of
    propagate(observe=dict(cross_mpo=True)) is bitwise the cross_mpo() call on the same state"""
    from helpers import cross_mpo_cases as xc

    name = "odd"
    states = xc.random_states(name, 5, seed=60)
    k = xc.OP_ID["complex"]
    big = _batch(name, 5, states=states)
    big.set_cross_mpo([(3, 1, k)])
    alone = big.cross_mpo()["values"][0]
    long = [(0, 0, 1), (1, 3, k), (2, 4, 0), (3, 1, k), (4, 4, 3), (3, 1, 2), (3, 1, k)]
    big.set_cross_mpo(long)
    v = big.cross_mpo()["values"]
    assert v[3] == alone and v[6] == alone and len({x for x in v}) == 6 and abs(alone) > 0
    big.close()
    small = _batch(name, 2, states=[states[1], states[3]])
    small.set_cross_mpo([(0, 0, 2), (1, 0, k)])
    assert small.cross_mpo()["values"][1] == alone
    small.close()
    # a record is the call
    bt = _batch("mixed")
    bt.snapshot()
    req = [(0, 1, 2), (bt.snap(1), 2, 4), (2, 2, 0), (1, bt.snap(0), 3)]
    bt.set_cross_mpo(req)
    rec = bt.propagate(DT, 4, observe=dict(norm=False, cross_mpo=True), every=2)
    assert set(rec) == {"cross_mpo", "mean_cross_mpo"} and rec["cross_mpo"].shape == (3, 4) and rec["mean_cross_mpo"].shape == (3,)
    last = bt.cross_mpo()
    assert np.array_equal(rec["cross_mpo"][-1], last["values"]) and rec["mean_cross_mpo"][-1] == last["mean"]
    by_hand = _batch("mixed")
    by_hand.snapshot()
    by_hand.set_cross_mpo(req)
    for t in range(3):
        now = by_hand.cross_mpo()
        assert np.array_equal(rec["cross_mpo"][t], now["values"]) and rec["mean_cross_mpo"][t] == now["mean"], t
        by_hand.propagate(DT, 2)
    by_hand.close()
    assert not np.array_equal(rec["cross_mpo"][0], rec["cross_mpo"][-1])
    # the records under other weights: one launch over what is still on the device
    w = np.array([0.4, 0.1, 0.3, 0.2])
    n = bt.launches()
    vals, mean = bt._cross_mpo_records(w)
    assert bt.launches() - n == 1 and np.array_equal(vals, rec["cross_mpo"])
    assert np.abs(mean - rec["cross_mpo"] @ w).max() < 1e-15 * np.abs(vals).max() * 4
    n = bt.launches()
    assert np.array_equal(bt._cross_mpo_records(None)[1], rec["mean_cross_mpo"]) and bt.launches() == n
    bt.close()


def test_launch_counts_and_nothing_changes_without_a_request():
    """the call: two launches; a recorded run: one more launch per record and one more mean launch; beside the cross and
    expect requests; setting and removing the request leaves propagate bitwise, and launches(), as without it"""
    req = dict(sites=[1, 3], norm=True, autocorr=True, energy=True, keys=[(0, 0, 2, 2)])
    out = []
    for how in ("never", "set and removed", "set"):
        bt = _batch("mixed")
        bt.propagate(DT, 1)  # the engines build their right blocks with launches of their own on first use
        bt.snapshot()
        bt.set_cross([(0, 1), (bt.snap(1), 2)])
        bt.set_expect([2, 0])
        if how != "never":
            bt.set_cross_mpo([(0, 1, 2), (bt.snap(2), 0, 4), (1, 1, 0)])
        if how == "set and removed":
            bt.set_cross_mpo([])
        n = bt.launches()
        obs = dict(req, cross=True, expect=True)
        rec = bt.propagate(DT, 2, observe=dict(obs, cross_mpo=True) if how == "set" else obs, every=1)
        out.append((rec, _tensors(bt), list(bt.statuses), bt.launches() - n))
        if how == "set":
            before = _tensors(bt)
            n = bt.launches()
            bt.cross_mpo()
            assert bt.launches() - n == 2
            assert _same_tensors(before, _tensors(bt)) and list(bt.statuses) == [0, 0, 0]  # an observation changes nothing
            n = bt.launches()
            alone = bt.propagate(DT, 4, observe=dict(norm=False, cross_mpo=True), every=2)  # the request alone... beside the two others
            assert bt.launches() - n == 2 * 4 + 3 * 3 + 3 and set(alone) == {"cross_mpo", "mean_cross_mpo"}
        else:
            with pytest.raises(ValueError, match="no cross request of MPOs"):
                bt.propagate(DT, 1, observe=dict(norm=True, cross_mpo=True))
            with pytest.raises(ValueError, match="no cross request of MPOs"):
                bt.cross_mpo()
        bt.close()
    (a, ta, sa, na), (b, tb, sb_, nb), (c, tc, sc_, nc) = out
    assert na == nb and nc - na == 3 + 1  # one launch per record and one mean launch, nothing else
    assert _same_tensors(ta, tb) and _same_tensors(ta, tc) and sa == sb_ == sc_ == [0, 0, 0]
    assert set(a) == set(b) and set(c) - set(a) == {"cross_mpo", "mean_cross_mpo"} and c["cross_mpo"].shape == (3, 3)
    for other in (b, c):
        for k in a:
            xs, ys = (a[k], other[k]) if isinstance(a[k], list) else ([a[k]], [other[k]])
            for x, y in zip(xs, ys):
                assert np.array_equal(x, y), k


def test_an_entry_that_names_a_failed_replica_is_zeros():
    """the set-up of test_gpu_batch_observe.py: replica 1 propagates under a Hamiltonian a thousand times larger and stops
    with its status word set; entries that name it are zeros from then on, the others' bits are those of a batch without it"""
    from helpers import cross_cases as cc
    from helpers import spin_bath as sb
    from pytdscf_amd import TDVPBatch, TDVPEngine, _lib
    from pytdscf_amd import synthetic as syn

    L, d, D, M, dt = 4, 3, 6, 3, 0.02
    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    hot = [w.copy() for w in mpo]
    hot[0] = hot[0] * 1e3
    obs = sb.sop_mpo([(0.4, {p: cc.random_op(d, 500 + p, hermitian=True), p + 1: cc.random_op(d, 520 + p, hermitian=True)})
                      for p in range(L - 1)], [d] * L)

    def engines(which):
        out = []
        for r in which:
            e = TDVPEngine(L, max_krylov=8)
            e.set_mpo(hot if r == 1 else mpo)
            e.set_mpo(obs, 1, shift=0.25)
            e.init_random([d] * L, D, seed=50 + r)
            out.append(e)
        return out

    engs = engines((0, 1, 2))
    bt = TDVPBatch.from_engines(engs)
    bt.snapshot()
    bt.set_cross_mpo([(0, 2, 1), (0, 1, 1), (1, 1, 1), (2, 1, 1), (bt.snap(1), 2, 1), (bt.snap(0), 1, 1)])
    with pytest.raises(ValueError, match="Short Iterative Lanczos is not converged"):
        bt.propagate(dt, 2, observe=dict(norm=True, cross_mpo=True), every=1)
    assert bt.statuses == [0, _lib.ENOTCONV, 0]
    got = bt.records["cross_mpo"]
    assert got.shape == (3, 6) and np.all(np.abs(got[0]) > 0)  # observed before it failed
    assert np.all(got[1:, [1, 2, 3, 5]] == 0)
    assert np.all(np.abs(got[1:, 4]) > 0)  # the snapshot of the replica that failed later is still a state
    good = engines((0, 2))
    ok = TDVPBatch.from_engines(good)
    ok.set_cross_mpo([(0, 1, 1)])
    ref = ok.propagate(dt, 2, observe=dict(norm=True, cross_mpo=True), every=1)["cross_mpo"]
    assert np.array_equal(got[:, 0], ref[:, 0])
    bt.close()
    ok.close()
    for e in engs + good:
        e.close()


def test_every_refusal_names_itself_and_changes_nothing():
    from helpers import cross_mpo_cases as xc
    from pytdscf_amd import _lib

    name = "mixed"
    dims, _ = xc.SHAPES[name]
    L = len(dims)
    fresh = _batch(name)
    with pytest.raises(ValueError, match=r"mitdvp_batch_set_cross_mpo: entry 1: bra index 4 names the snapshot of replica 1.*no snapshot"):
        fresh.set_cross_mpo([(0, 1, 0), (fresh.snap(1), 0, 0)])
    assert fresh._lib.mitdvp_batch_set_cross_mpo(fresh._handle(), 0, None, None, None) == 0  # removing nothing is fine
    with pytest.raises(ValueError, match="mitdvp_batch_cross_mpo: no cross request of MPOs"):
        _lib.check(fresh._lib.mitdvp_batch_cross_mpo(fresh._handle(), None, None, None))
    fresh.close()

    bt = _batch(name)
    bt.snapshot()
    bt.propagate(DT, 1)
    good = [(0, 1, 2), (bt.snap(2), 1, 0)]
    bt.set_cross_mpo(good)
    # operators that must be refused: 5 is missing on replica 2 from site 3 on, 6 has other MPO bonds on replica 1, 8 has an
    # MPO bond of 17, 9 and 10 have outer MPO bonds of 2, 12 has neighbouring cores that do not fit
    local, product = xc.case(name, "local")[2], xc.case(name, "product")[2]
    rng = np.random.default_rng(9)
    rnd = lambda ml, d, mr: rng.standard_normal((ml, d, d, mr)) + 0j
    for r, e in enumerate(bt.engines):
        e.set_mpo(local if r < 2 else local[:3], 5)
        e.set_mpo(product if r == 1 else local, 6)
        e.set_mpo([rnd(1 if p == 0 else 17, d, 1 if p == L - 1 else 17) for p, d in enumerate(dims)], 8)
        e.set_mpo([rnd(2 if p == 0 else 3, d, 1 if p == L - 1 else 3) for p, d in enumerate(dims)], 9)
        e.set_mpo([rnd(1 if p == 0 else 3, d, 2 if p == L - 1 else 3) for p, d in enumerate(dims)], 10)
    before, n0, tensors = bt.cross_mpo(), bt.launches(), _tensors(bt)
    bad = [([(0, 2 * B, 0)], r"entry 0: ket index 6 is outside 0 \.\. 5"),
           ([(0, 1, 0), (-1, 0, 0)], r"entry 1: bra index -1 is outside 0 \.\. 5"),
           ([(0, 1, 0), (1, 2, -3)], r"entry 1: operator -3 is negative"),
           ([(0, 1, 11)], r"operator 11 has no core at site 0 of replica 0 \(every replica must carry every listed operator at all 5 sites\)"),
           ([(0, 1, 2), (1, 0, 5)], r"operator 5 has no core at site 3 of replica 2"),
           ([(0, 1, 6)], r"operator 6 has MPO bonds \(1, 1\) at site 0 of replica 1, replica 0 has \(1, \d+\): the core shapes must be equal"),
           ([(0, 1, 0), (2, 2, 8)], r"operator 8, site 0: MPO bonds \(1, 17\): the batched kernel takes MPO bonds of 1 to 16"),
           ([(0, 1, 9)], r"operator 9: the outer MPO bonds are \(2, 1\), they must be 1"),
           ([(0, 1, 10)], r"operator 10: the outer MPO bonds are \(1, 2\), they must be 1"),
           ([(0, 1, 0)] * 65537, r"65537 entries, a request takes at most 65536")]
    for entries, match in bad:
        with pytest.raises(ValueError, match="mitdvp_batch_set_cross_mpo: " + match):
            bt.set_cross_mpo(entries)
    with pytest.raises(ValueError, match="set_cross_mpo: entry 0"):
        bt.set_cross_mpo([(0, 1)])
    with pytest.raises(ValueError, match="one per entry"):
        bt.cross_mpo(weights=[1.0])
    assert bt.launches() == n0
    after = bt.cross_mpo()
    assert np.array_equal(after["values"], before["values"]) and after["mean"] == before["mean"]
    assert _same_tensors(tensors, _tensors(bt))
    # cores that arrive after the request was set are checked again where they are used, and good ones are taken up
    keep = xc.case(name, "local")
    bt[1].set_mpo(product, 2)
    with pytest.raises(ValueError, match=r"mitdvp_batch_cross_mpo: operator 2 has MPO bonds \(1, 1\) at site 0 of replica 1"):
        bt.cross_mpo()
    with pytest.raises(ValueError, match=r"mitdvp_batch_run: operator 2 has MPO bonds"):
        bt.propagate(DT, 1, observe=dict(norm=False, cross_mpo=True))
    bt[1].set_mpo(keep[2], 2, shift=keep[1])
    assert np.array_equal(bt.cross_mpo()["values"], before["values"]) and _same_tensors(tensors, _tensors(bt))
    scaled = [w.copy() for w in keep[2]]
    scaled[1] = scaled[1] * 2.0
    bt[1].set_mpo(scaled, 2, shift=keep[1])  # entry 0 is (0, 1, 2): the ket's owner carries the doubled operator now
    twice = bt.cross_mpo()["values"]
    assert abs(twice[0] - 2 * before["values"][0]) < 1e-12 * abs(before["values"][0]) and twice[1] == before["values"][1]
    bt.sweep(DT, True)  # the centre is at the last site now: the walk takes either end
    assert bt.cross_mpo()["values"].shape == (2,)
    bt.close()


def test_the_buffer_cap_is_refused_with_its_figure():
    """d = 4, L = 6, D = 32 (bonds 1, 4, 16, 32, 16, 4, 1) with an operator of MPO bond 16 across the middle: a carve of
    1 572 864 bytes, so 2730 entries fit in 2^32 bytes"""
    from helpers import cross_cases as cc
    from helpers import spin_bath as sb
    from pytdscf_amd import TDVPBatch

    L, d, D = 6, 4, 32
    dims = [d] * L
    terms = [(0.1 + 0.01 * k, {2: cc.random_op(d, 710 + k), 3: cc.random_op(d, 730 + k)}) for k in range(16)]
    wide = [np.ascontiguousarray(w) for w in sb.sop_mpo(terms, dims)]
    assert wide[2].shape[3] == 16
    ham = sb.sop_mpo([(0.5, {p: cc.random_op(d, 750 + p, hermitian=True)}) for p in range(L)], dims)
    bt = TDVPBatch(2, L, integrator="arnoldi", conserve_norm=False)
    for e, cores in zip(bt.engines, cc.random_states(dims, D, 2, 41)):
        e.set_mpo(ham, 0)
        e.set_mpo(wide, 1)
        e.set_mps(cores)
    carve = 2 * (32 * 16 * 32) + 2 * (16 * 4 * 32 * 16)  # two blocks (chi m chi at the middle bond), X (n ml) and Y (n mr)
    fit = (1 << 32) // (carve * 16)
    assert carve * 16 == 1572864 and fit == 2730
    bt.set_cross_mpo([(0, 1, 1), (1, 0, 0)])
    before, tensors = bt.cross_mpo()["values"], _tensors(bt)
    with pytest.raises(ValueError, match=rf"mitdvp_batch_set_cross_mpo: {fit + 1} entries of {carve * 16} bytes each need a buffer of "
                                         rf"{(fit + 1) * carve * 16} bytes, the limit is 4294967296 bytes: at most {fit} entries fit"):
        bt.set_cross_mpo([(0, 1, 1)] * (fit + 1))
    assert np.array_equal(bt.cross_mpo()["values"], before) and _same_tensors(tensors, _tensors(bt))
    bt.close()


def test_correlation_function_with_operators_that_are_sums_over_the_chain():
    """C(t) = <psi| A(t) B |psi> with A = sum_p SZ_p, B = sum_p SX_p given by their names: against the oracle at the
    project's 1e-8 bar and against dense expm within ten times the oracle's own deviation from it
    (helpers/cross_mpo_cases has the figures); the mixed forms; two weighted starts; and the (site, matrix) form is bitwise
    what the cross request gives when it is set by hand, as before"""
    from helpers import cross_cases as cc
    from helpers import cross_mpo_cases as xc
    from pytdscf_amd import TDVPBatch, units
    from pytdscf_amd.mps import product_state_cores
    from pytdscf_amd.trajectories import correlation_function

    m = xc.model()
    kw = dict(maxstep=cc.NSTEPS + 1, stepsize=cc.DT * units.au_in_fs)
    forms = {("mpo", "mpo"): ("sz_total", "sx_total"), ("site", "mpo"): (cc.A_OP, xc.b_mpo()), ("mpo", "site"): (xc.a_mpo(), cc.B_OP)}
    got = {}
    for key, (A, Bop) in forms.items():
        out = correlation_function(m, [cc.START], A=A, B=Bop, per_trajectory=True, **kw)
        assert out["mean"].shape == (cc.NSTEPS + 1,) and out["trajectories"].shape == (cc.NSTEPS + 1, 1)
        assert np.array_equal(out["mean"], out["trajectories"][:, 0])
        oc, de = xc.oracle_corr(*key), xc.dense_corr(*key)
        d_or, d_de, o_de = np.abs(out["mean"] - oc).max(), np.abs(out["mean"] - de).max(), np.abs(oc - de).max()
        print(f"A {key[0]} / B {key[1]}: device vs oracle {d_or:.2e}, device vs dense {d_de:.2e}, oracle vs dense {o_de:.2e}")
        assert d_or < 1e-8
        assert d_de < 10 * o_de
        got[key] = out["mean"]
    # a name is the observable's MPO as propagate_trajectories prepares it: those cores given as a list are the same bits
    cores = [m.observables[k].as_mpo(m.dims) for k in ("sz_total", "sx_total")]
    assert np.array_equal(correlation_function(m, [cc.START], A=cores[0], B=cores[1], **kw)["mean"], got[("mpo", "mpo")])
    # two starts with weights: the second is the first with another site-0 vector; the mean is the weighted sum
    other = [[0.6, 0.8j]] + cc.START[1:]
    two = correlation_function(m, [cc.START, other], A="sz_total", B="sx_total", weights=[0.25, 0.75], per_trajectory=True, every=2, **kw)
    assert two["trajectories"].shape == (5, 2) and np.array_equal(two["trajectories"][:, 0], got[("mpo", "mpo")][::2])
    assert np.abs(two["trajectories"][:, 1] - two["trajectories"][:, 0]).max() > 1e-3
    assert np.abs(two["mean"] - two["trajectories"] @ [0.25, 0.75]).max() < 1e-15 * 4
    # the (site, matrix) form: the launches and bits of the cross request set by hand
    site = correlation_function(m, [cc.START], A=cc.A_OP, B=cc.B_OP, **kw)["mean"]
    v = np.asarray(cc.START[cc.B_OP[0]], dtype=np.complex128)
    bv = cc.B_OP[1] @ (v / np.linalg.norm(v))
    psi, phi = cc.START, cc.START[:cc.B_OP[0]] + [bv] + cc.START[cc.B_OP[0] + 1:]
    bt = TDVPBatch(2, cc.L, integrator="arnoldi", conserve_norm=False, thresh=1e-9)
    mpo = m.project_mpo(m.hamiltonian.as_mpo(m.dims))
    for e, s, scale in zip(bt.engines, (psi, phi), (1.0, float(np.linalg.norm(bv)))):
        e.set_mpo(mpo, 0, shift=m.hamiltonian.coupleJ[0][0])
        e.set_mps(product_state_cores(s, cc.D), canonicalize=True, scale=scale)
    bt.set_cross([(0, 1, cc.A_OP[0], cc.A_OP[1])])
    by_hand = bt.propagate(kw["stepsize"] / units.au_in_fs, cc.NSTEPS, observe=dict(norm=False, per_replica=False, cross=True, cross_weights=np.ones(1)), every=1)
    bt.close()
    assert np.array_equal(site, by_hand["mean_cross"])
