"""GPU: expectation values of MPO observables of the batched trajectories (TDVPBatch.set_expect / expect,
propagate(observe=dict(expect=True)): k_batch_expect walks every listed operator over every replica with one launch, one
workgroup per (replica, operator); k_batch_mean averages on the device) and propagate_trajectories(observables=...).

The pin is the dense state built from the tensors the engines hand back with the MPO applied to the vector core by core
(helpers/expect_cases.dense_value): values to 1e-12 S, S = (sum_terms |coef| prod ||factor||_2 + |shift|) <psi|psi>, the
relative bar the spectra tests hold against their dense pin; the NumPy twin of the walk is inside it with a factor of
1e4 to spare (tests/test_batch_expect_host.py).  Every case prints its worst defect as a fraction of its bar.  The shapes
are those of the spectra tests, the smallest at which each part can go wrong:
  mixed  dims (2, 3, 2, 4, 2), D = 6: ragged physical dimensions, a bond narrower than the tile
  odd    dims (3,) * 5, D = 7: every size odd, a multiple of no tile
  wide   dims (2,) * 12, D = 40: bonds past the 32-wide tile and the 16-deep K step, more than one tile per product
and per shape five operators (helpers/expect_cases): MPO bonds 1, 4, 4 or 8, 3 (non-Hermitian, complex shift) and
operator 0 itself, so the walk runs with MPO bonds below, beside and above those the sweep's buffers are sized for."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = 0.2
ORDER = ("product", "local", "longrange", "complex", "energy")  # the request of most tests: operators 1, 2, 3, 4, 0


def _give(e, name, labels=ORDER):
    from helpers import expect_cases as ec

    for label in labels:
        _, shift, mpo = ec.case(name, label)
        e.set_mpo(mpo, ec.OP_ID[label], shift=shift)


def _batch(name, B, seed=30, states=None, **kw):
    """B replicas with random states of norms 0.7, 0.9, 1.1, ..., every one carrying the five operators; no rescaling in
    a step, so the norms stay apart"""
    from helpers import expect_cases as ec
    from pytdscf_amd import TDVPBatch

    dims, _ = ec.SHAPES[name]
    kw = dict(dict(integrator="arnoldi", conserve_norm=False), **kw)
    bt = TDVPBatch(B, len(dims), **kw)
    for e, cores in zip(bt.engines, states if states is not None else ec.random_states(name, B, seed)):
        _give(e, name)
        e.set_mps(cores)
    return bt


def _ids(labels=ORDER):
    from helpers import expect_cases as ec

    return [ec.OP_ID[x] for x in labels]


def _tensors(bt):
    return [e.get_mps() for e in bt.engines]


def _same_tensors(a, b):
    return all(np.array_equal(x, y) for s, t in zip(a, b) for x, y in zip(s, t))


@pytest.mark.parametrize("name", ["mixed", "odd", "wide"])
def test_values_equal_the_dense_pin_and_the_engine_routes(name):
    """random states of different norms, one propagation step, all five operators in one launch"""
    from helpers import expect_cases as ec

    B = 3
    bt = _batch(name, B)
    bt.propagate(DT, 1)
    now = _tensors(bt)
    assert max(c.shape[2] for c in now[0]) == ec.SHAPES[name][1]
    bt.set_expect(_ids())
    got = bt.expect()
    assert got["values"].shape == (B, 5) and got["values"].dtype == np.complex128 and got["mean"].shape == (5,)
    energy = bt.observe(energy=True)["energy"]
    worst = worst_eng = worst_obs = 0.0
    for r in range(B):
        n2 = ec.norm2(now[r])
        for k, label in enumerate(ORDER):
            _, shift, mpo = ec.case(name, label)
            pin = ec.dense_value(now[r], mpo, shift)
            worst = max(worst, abs(got["values"][r, k] - pin) / (ec.BAR * ec.scale(name, label) * n2))
            worst_eng = max(worst_eng, abs(got["values"][r, k] - bt[r].expectation(ec.OP_ID[label])) / 1e-8)
        worst_obs = max(worst_obs, abs(got["values"][r, 4] - energy[r]) / 1e-8)
    print(f"{name}: |value - dense pin| {worst:.3e} of 1e-12 S; against TDVPEngine.expectation {worst_eng:.3e} of 1e-8; "
          f"operator 0 against observe(energy=True) {worst_obs:.3e} of 1e-8")
    assert worst < 1 and worst_eng < 1 and worst_obs < 1
    assert np.abs(got["values"][:, 3].imag).min() > 1e-3  # the non-Hermitian operator with its complex shift
    assert np.abs(got["values"]).min() > 1e-6  # nothing here is a zero compared with a zero
    assert set(bt.expect(per_replica=False)) == {"mean"}
    bt.close()


def test_the_edges_of_the_envelope():
    """a chain of one site (no walk: the H_eff apply between the two boundary blocks); two sites of d = 4 with an operator
    of MPO bond 16, the kernel's limit, beside a Hamiltonian of bond 2; and a request of 64 operators, the limit of a list"""
    from helpers import cross_cases as cc
    from helpers import expect_cases as ec
    from helpers import spin_bath as sb
    from pytdscf_amd import TDVPBatch

    # L = 1
    h1, o1 = cc.random_op(5, 700, hermitian=True), cc.random_op(5, 701)
    bt = TDVPBatch(2, 1, integrator="arnoldi", conserve_norm=False)
    for e, cores in zip(bt.engines, ec.sc.random_states((5,), 1, 2, 40)):
        e.set_mpo([h1.reshape(1, 5, 5, 1)], 0, shift=0.2)
        e.set_mpo([o1.reshape(1, 5, 5, 1)], 1, shift=-0.1j)
        e.set_mps(cores)
    bt.propagate(DT, 1)
    bt.set_expect([1, 0])
    got = bt.expect()["values"]
    worst = 0.0
    for r, e in enumerate(bt.engines):
        v = e.get_mps()[0].reshape(-1)
        n2 = np.vdot(v, v).real
        for k, (O, shift) in enumerate(((o1, -0.1j), (h1, 0.2))):
            pin = np.vdot(v, O @ v) + shift * n2
            worst = max(worst, abs(got[r, k] - pin) / (ec.BAR * (np.linalg.norm(O, 2) + abs(shift)) * n2))
    bt.close()
    # L = 2, d = 4: sum of 16 random products has MPO bond 16
    dims = (4, 4)
    terms = [(0.1 + 0.01 * k, {0: cc.random_op(4, 710 + k), 1: cc.random_op(4, 730 + k)}) for k in range(16)]
    wide = [np.ascontiguousarray(w) for w in sb.sop_mpo(terms, list(dims))]
    assert wide[0].shape == (1, 4, 4, 16) and wide[1].shape == (16, 4, 4, 1)
    S = sum(abs(c) * np.prod([np.linalg.norm(m, 2) for m in ops.values()]) for c, ops in terms)
    ham = sb.sop_mpo([(0.5, {0: cc.random_op(4, 750, hermitian=True)}), (0.4, {1: cc.random_op(4, 751, hermitian=True)})], list(dims))
    bt = TDVPBatch(3, 2, integrator="arnoldi", conserve_norm=False)
    for e, cores in zip(bt.engines, ec.sc.random_states(dims, 4, 3, 41)):
        e.set_mpo(ham, 0)
        for k in range(1, 65):
            e.set_mpo(wide, k)
        e.set_mps(cores)
    bt.propagate(DT, 1)
    now = _tensors(bt)
    bt.set_expect(range(1, 65))
    got = bt.expect()["values"]
    assert got.shape == (3, 64)
    assert all(np.array_equal(got[:, k], got[:, 0]) for k in range(64))  # 192 workgroups, the same bits for the same work
    for r in range(3):
        worst = max(worst, abs(got[r, 0] - ec.dense_value(now[r], wide)) / (ec.BAR * S * ec.norm2(now[r])))
    print(f"edges: |value - dense pin| {worst:.3e} of 1e-12 S")
    assert worst < 1
    bt.close()


def test_every_replica_reports_its_own_operator():
    """replica 1 carries other cores of the same shapes under operator 2"""
    from helpers import expect_cases as ec

    name, B = "mixed", 3
    bt = _batch(name, B)
    _, shift, mpo = ec.case(name, "local")
    other = [w.copy() for w in mpo]
    other[0] = other[0] * (0.5 + 0.25j)
    other[2] = other[2] * -0.8
    bt[1].set_mpo(other, ec.OP_ID["local"], shift=0.05j)
    bt.propagate(DT, 1)
    now = _tensors(bt)
    bt.set_expect(_ids())
    got = bt.expect()["values"]
    S = ec.scale(name, "local") + 0.05  # |0.5 + 0.25j| 0.8 < 1: the scale of the original bounds the other one's terms
    worst = 0.0
    for r in range(B):
        pin = ec.dense_value(now[r], other, 0.05j) if r == 1 else ec.dense_value(now[r], mpo, shift)
        worst = max(worst, abs(got[r, 1] - pin) / (ec.BAR * S * ec.norm2(now[r])))
    assert abs(got[1, 1] - ec.dense_value(now[1], mpo, shift)) > 1e-3  # and not the one of replica 0
    print(f"per-replica operators: |value - dense pin| {worst:.3e} of 1e-12 S")
    assert worst < 1
    bt.close()


def test_bits_depend_on_the_replica_and_the_operator_only():
    """a replica's values at B = 1, at B = 5 and at another position; operator 3 alone, inside a list of five and at
    another place of the list"""
    from helpers import expect_cases as ec

    name = "odd"
    states = ec.random_states(name, 5, seed=60)
    recs = []
    for order in ([2], [0, 1, 2, 3, 4], [4, 2, 0, 3, 1]):
        bt = _batch(name, len(order), states=[states[i] for i in order])
        bt.set_expect(_ids())
        vals = bt.expect()["values"]
        recs.append(vals[order.index(2)])
        if len(order) == 5:
            assert len({vals[r].tobytes() for r in range(5)}) == 5  # five different states, five records
            bt.set_expect([3])
            alone = bt.expect()["values"]
            bt.set_expect([3, 0, 4, 1, 2])
            moved = bt.expect()["values"]
            assert alone.shape == (5, 1)
            assert np.array_equal(alone[:, 0], vals[:, 2]) and np.array_equal(moved[:, 0], vals[:, 2])
            assert np.array_equal(moved[:, [3, 4, 0, 2, 1]], vals)
        bt.close()
    assert np.array_equal(recs[0], recs[1]) and np.array_equal(recs[0], recs[2])
    assert recs[0].shape == (5,) and np.all(np.abs(recs[0]) > 0)


def test_means_are_the_weighted_sums_of_the_values():
    bt = _batch("mixed", 3)
    bt.propagate(DT, 1)
    bt.set_expect(_ids())
    worst = 0.0
    for w in (None, np.array([0.5, 0.2, 0.3])):
        got = bt.expect(weights=w)
        ww = np.full(3, 1.0 / 3.0) if w is None else w
        for k in range(5):
            worst = max(worst, abs(got["mean"][k] - ww @ got["values"][:, k]) / (1e-15 * np.abs(got["values"][:, k]).max()))
    print(f"means: |device mean - host sum| {worst:.3f} of 1e-15 max |value|")
    assert worst < 1
    with pytest.raises(ValueError, match="one per replica"):
        bt.expect(weights=[1.0])
    bt.close()


def test_a_recorded_run():
    B = 3
    bt = _batch("mixed", B)
    bt.propagate(DT, 1)  # the engines build their right blocks with launches of their own on first use
    bt.set_expect([2, 0, 3])
    n = bt.launches()
    first = bt.expect()
    assert bt.launches() - n == 2
    start = _tensors(bt)
    n = bt.launches()
    rec = bt.propagate(DT, 4, observe=dict(norm=False, expect=True), every=2)  # the request alone
    assert bt.launches() - n == 2 * 4 + 3 + 1
    last = bt.expect()
    assert set(rec) == {"expect", "mean_expect"}
    assert rec["expect"].shape == (4 // 2 + 1, B, 3) and rec["mean_expect"].shape == (3, 3)
    assert np.array_equal(rec["expect"][0], first["values"]) and np.array_equal(rec["mean_expect"][0], first["mean"])
    assert np.array_equal(rec["expect"][-1], last["values"]) and np.array_equal(rec["mean_expect"][-1], last["mean"])
    assert not np.array_equal(first["values"], last["values"])
    # record t is expect() called at that step: the same states with the same history, stepped by hand
    by_hand = _batch("mixed", B)
    by_hand.propagate(DT, 1)
    assert _same_tensors(start, _tensors(by_hand))
    by_hand.set_expect([2, 0, 3])
    for t in range(3):
        now = by_hand.expect()
        assert np.array_equal(rec["expect"][t], now["values"]) and np.array_equal(rec["mean_expect"][t], now["mean"]), t
        by_hand.propagate(DT, 2)
    by_hand.close()
    # the records under other weights: one launch over what is still on the device
    w = np.array([0.5, 0.2, 0.3])
    n = bt.launches()
    again = bt._expect_records(w)
    assert bt.launches() - n == 1
    assert np.array_equal(again["expect"], rec["expect"])
    worst = np.abs(again["mean_expect"] - np.einsum("r,qrk->qk", w, rec["expect"])).max() / (1e-15 * np.abs(rec["expect"]).max())
    print(f"recorded run: means under other weights {worst:.3f} of 1e-15 max |value|")
    assert worst < 1
    n = bt.launches()
    assert np.array_equal(bt._expect_records(None)["mean_expect"], rec["mean_expect"]) and bt.launches() == n
    n = bt.launches()
    bt.propagate(DT, 4, observe=dict(norm=True, sites=[1, 2], expect=True), every=2)  # with an observation of its own
    assert bt.launches() - n == 2 * 4 + 2 * 3 + 2
    bt.set_spectra([0, 2])
    n = bt.launches()
    both = bt.propagate(DT, 2, observe=dict(norm=True, sites=[1, 2], expect=True, spectra=True), every=1)  # and a spectra request
    assert bt.launches() - n == 2 * 2 + 3 * 3 + 3
    assert both["expect"].shape == (3, B, 3) and both["entropy"].shape == (3, B, 2) and both["mean_norm2"].shape == (3,)
    bt.close()


def test_an_observation_changes_nothing():
    bt = _batch("mixed", 3)
    bt.propagate(DT, 1)
    bt.set_expect(_ids())
    before, statuses = _tensors(bt), list(bt.statuses)
    bt.expect()
    assert _same_tensors(before, _tensors(bt)) and list(bt.statuses) == statuses == [0, 0, 0]
    bt.close()
    req = dict(sites=[1, 3], norm=True, autocorr=True, energy=True, keys=[(0, 0, 2, 2)], spectra=True)
    out = []
    for with_expect in (False, True):
        bt = _batch("mixed", 3)
        bt.set_spectra([0, 2])
        if with_expect:
            bt.set_expect([3, 1])
        n = bt.launches()
        rec = bt.propagate(DT, 2, observe=dict(req, expect=True) if with_expect else req, every=1)
        out.append((rec, _tensors(bt), list(bt.statuses), bt.launches() - n))
        bt.close()
    (a, ta, sa, na), (b, tb, sb_, nb) = out
    assert _same_tensors(ta, tb) and sa == sb_ == [0, 0, 0]
    assert set(b) - set(a) == {"expect", "mean_expect"} and b["expect"].shape == (3, 3, 2)
    assert nb - na == 3 + 1  # one launch per record and one mean launch, nothing else
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for x, y in zip(xs, ys):
            assert np.array_equal(x, y), k
    # with no request: the launches of before (two per step, observe + density + spectra per record, two mean launches);
    # the engines build their right blocks with launches of their own in the same call, which both runs share
    bt = _batch("mixed", 3)
    bt.propagate(DT, 1)
    n = bt.launches()
    bt.propagate(DT, 2, observe=dict(sites=[1, 3], norm=True), every=1)
    assert bt.launches() - n == 2 * 2 + 3 + 1
    with pytest.raises(ValueError, match="no expect request"):
        bt.propagate(DT, 2, observe=dict(norm=True, expect=True))
    bt.close()


def test_a_replica_that_does_not_converge_is_recorded_as_zeros():
    """the set-up of test_gpu_batch_observe.py: replica 1 propagates under a Hamiltonian a thousand times larger and stops
    with its status word set; its later records are zeros, the other replicas' bits are those of a batch without it"""
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

    req = dict(norm=True, expect=True)
    engs = engines((0, 1, 2))
    bt = TDVPBatch.from_engines(engs)
    bt.set_expect([1, 0])
    with pytest.raises(ValueError, match="Short Iterative Lanczos is not converged"):
        bt.propagate(dt, 2, observe=req, every=1)
    assert bt.statuses[1] == _lib.ENOTCONV and bt.statuses[0] == 0 and bt.statuses[2] == 0
    rec = bt.records
    assert rec["expect"].shape == (3, 3, 2)
    assert np.all(rec["expect"][1:, 1] == 0) and np.abs(rec["expect"][0, 1]).min() > 0  # observed before it failed
    good = engines((0, 2))
    ok = TDVPBatch.from_engines(good)
    ok.set_expect([1, 0])
    ref = ok.propagate(dt, 2, observe=req, every=1)
    assert np.array_equal(rec["expect"][:, [0, 2]], ref["expect"]) and np.array_equal(rec["norm"][:, [0, 2]], ref["norm"])
    bt.close()
    ok.close()
    for e in engs + good:
        e.close()


def test_the_request_survives_a_new_handle():
    bt = _batch("mixed", 3)
    bt.set_expect([2, 4])
    a = bt.expect()["values"]
    gone = bt.engines.pop(0)
    b = bt.expect()["values"]  # the list of engines changed: the library's batch object is made anew and gets the request again
    assert b.shape == (2, 2) and np.array_equal(b, a[1:])
    gone.close()
    bt.close()


def test_every_refusal_names_itself_and_changes_nothing():
    from helpers import expect_cases as ec
    from pytdscf_amd import _lib

    name = "mixed"
    dims, _ = ec.SHAPES[name]
    L = len(dims)
    fresh = _batch(name, 2)
    with pytest.raises(ValueError, match="no expect request"):
        fresh.expect()
    with pytest.raises(ValueError, match="mitdvp_batch_expect: no expect request"):
        _lib.check(fresh._lib.mitdvp_batch_expect(fresh._handle(), None, None, None, None))
    assert fresh._lib.mitdvp_batch_set_expect(fresh._handle(), None, 0) == 0  # removing nothing is fine
    fresh.close()

    bt = _batch(name, 3)
    bt.propagate(DT, 1)
    bt.set_expect([2, 0])
    # operators that must be refused: 5 is missing on replica 2 from site 3 on, 6 has other MPO bonds on replica 1, 7 has the
    # physical dimensions of another chain, 8 has an MPO bond of 17, 9 and 10 have outer MPO bonds of 2
    local, product = ec.case(name, "local")[2], ec.case(name, "product")[2]
    rng = np.random.default_rng(9)
    rnd = lambda ml, d, mr: rng.standard_normal((ml, d, d, mr)) + 0j
    for r, e in enumerate(bt.engines):
        e.set_mpo(local if r < 2 else local[:3], 5)
        e.set_mpo(product if r == 1 else local, 6)
        e.set_mpo(ec.case("odd", "product")[2], 7)
        e.set_mpo([rnd(1 if p == 0 else 17, d, 1 if p == L - 1 else 17) for p, d in enumerate(dims)], 8)
        e.set_mpo([rnd(2 if p == 0 else 3, d, 1 if p == L - 1 else 3) for p, d in enumerate(dims)], 9)
        e.set_mpo([rnd(1 if p == 0 else 3, d, 2 if p == L - 1 else 3) for p, d in enumerate(dims)], 10)
    before, n0, tensors = bt.expect(), bt.launches(), _tensors(bt)
    bad = [([11], r"operator 11 has no core at site 0 of replica 0 \(every replica must carry every listed operator at all 5 sites\)"),
           ([2, 5], r"operator 5 has no core at site 3 of replica 2"),
           ([6], r"operator 6 has MPO bonds \(1, 1\) at site 0 of replica 1, replica 0 has \(1, \d+\): the core shapes must be equal"),
           ([7], r"operator 7 has physical dimension 3 at site 0 of replica 0, the site's is 2"),
           ([0, 8], r"operator 8, site 0: MPO bonds \(1, 17\): the batched kernel takes MPO bonds of 1 to 16"),
           ([9], r"operator 9: the outer MPO bonds are \(2, 1\), they must be 1"),
           ([10], r"operator 10: the outer MPO bonds are \(1, 2\), they must be 1")]
    for ops, match in bad:
        with pytest.raises(ValueError, match="mitdvp_batch_set_expect: " + match):
            bt.set_expect(ops)
    raw = [([1, 1], r"operator 1 is listed twice"), ([0, -3], r"operator -3 is negative"),
           (list(range(65)), r"bad list of operators \(65 given; a request takes 0 to 64"), (None, r"bad list of operators \(-1 given")]
    for ops, match in raw:  # what the Python side catches first, asked of the library itself
        arr = (C.c_int * 65)(*(ops or []))
        assert bt._lib.mitdvp_batch_set_expect(bt._handle(), arr, len(ops) if ops is not None else -1) == _lib.EINVAL
        with pytest.raises(ValueError, match="mitdvp_batch_set_expect: " + match):
            _lib.check(_lib.EINVAL)
    with pytest.raises(ValueError, match="expect operators"):
        bt.set_expect([0.5])
    with pytest.raises(ValueError, match="one per replica"):
        bt.expect(weights=[1.0])
    assert bt.launches() == n0
    after = bt.expect()
    assert after["values"].shape == (3, 2) and np.array_equal(after["values"], before["values"])
    assert _same_tensors(tensors, _tensors(bt))
    # cores that arrive after the request was set are checked again where they are used
    good = ec.case(name, "local")
    bt[1].set_mpo(product, 2)
    with pytest.raises(ValueError, match=r"mitdvp_batch_expect: operator 2 has MPO bonds \(1, 1\) at site 0 of replica 1"):
        bt.expect()
    with pytest.raises(ValueError, match=r"mitdvp_batch_run: operator 2 has MPO bonds"):
        bt.propagate(DT, 1, observe=dict(norm=False, expect=True))
    bt[1].set_mpo(good[2], 2, shift=good[1])
    assert np.array_equal(bt.expect()["values"], before["values"]) and _same_tensors(tensors, _tensors(bt))
    bt.sweep(DT, True)  # the centre is at the last site now
    moved = _tensors(bt)
    with pytest.raises(ValueError, match=rf"mitdvp_batch_expect: replica 0 has its centre at site {L - 1}"):
        bt.expect()
    assert _same_tensors(moved, _tensors(bt))
    bt.sweep(DT, False)
    assert bt.expect()["values"].shape == (3, 2)
    bt.set_expect([])  # an empty list removes the request
    with pytest.raises(ValueError, match="no expect request"):
        bt.expect()
    with pytest.raises(ValueError, match="mitdvp_batch_expect: no expect request"):
        _lib.check(bt._lib.mitdvp_batch_expect(bt._handle(), None, None, None, None))
    bt.close()


def test_propagate_trajectories_with_observables():
    """a dephasing-free spin chain of 4 sites at full bond dimension, two product starts, two observables (the total
    z magnetisation, a one-site sum, and the nearest-neighbour x-x correlation): every trajectory against exp(-i H t) of its
    dense start.  At full bond dimension one-site TDVP is exact up to its local exponentials: after k steps the state is
    within eps = k 2 (2 L - 1) thresh_sil of the dense one (spectra_cases.dyn_bar has the argument), so <O> moves by at
    most 2 S eps + S eps^2 with S = sum |coef| prod ||factor||_2 >= ||O||; the bar is 2.02 S eps at thresh_sil = 1e-9."""
    from helpers import jump_oracle as jo
    from helpers import pair_cases as pc
    from helpers import spin_bath as sb
    from pytdscf_amd import Exciton, Model, propagate_trajectories, units
    from scipy.linalg import expm

    L, dt, every, maxstep, thresh = 4, 0.3, 2, 5, 1e-9
    terms = {"magnetisation": [(1.0, {p: sb.SZ}) for p in range(L)],
             "xx": [(0.5 + 0.25 * p, {p: sb.SX, p + 1: sb.SX}) for p in range(L - 1)]}
    mpos = {k: sb.sop_mpo(t, [2] * L) for k, t in terms.items()}
    S = {k: sum(abs(c) * np.prod([np.linalg.norm(m, 2) for m in ops.values()]) for c, ops in t) for k, t in terms.items()}
    model = Model([Exciton(nstate=2) for _ in range(L)], operators=dict(mpos, hamiltonian=pc._spin_chain_mpo(L)), bond_dim=4)
    assert list(model.observables) == ["magnetisation", "xx"]
    starts = [[[1, 0], [0, 1]] * (L // 2), [[1, 1], [1, -1j]] * (L // 2)]
    w = np.array([0.3, 0.7])
    kw = dict(maxstep=maxstep, stepsize=dt * units.au_in_fs, reduced_density=([(1, 1)], every), integrator="arnoldi",
              conserve_norm=False, thresh_sil=thresh, weights=w, per_trajectory=True)
    base = propagate_trajectories(model, starts, **kw)
    out = propagate_trajectories(model, starts, observables=True, **kw)
    assert set(base) == {"time", "mean", "trajectories"}
    assert set(propagate_trajectories(model, starts, observables=None, **kw)) == set(base)
    assert set(out) == set(base) | {"expectations", "expectation_trajectories"}
    assert list(out["expectations"]) == ["magnetisation", "xx"]
    assert np.array_equal(out["time"], base["time"]) and np.array_equal(out["mean"][(1, 1)], base["mean"][(1, 1)])
    assert np.array_equal(out["trajectories"][(1, 1)], base["trajectories"][(1, 1)])
    one = propagate_trajectories(model, starts, observables=["xx"], **dict(kw, per_trajectory=False))
    assert set(one) == {"time", "mean", "expectations"} and list(one["expectations"]) == ["xx"]
    assert np.array_equal(one["expectations"]["xx"], out["expectations"]["xx"])
    # the dense trajectories
    H = jo.dense_operator(pc._spin_chain_mpo(L))
    U = expm(-1j * H * dt * every)
    nrec = (maxstep - 1) // every + 1
    worst = worst_mean = 0.0
    for name, mpo in mpos.items():
        O = jo.dense_operator(mpo)
        dense = np.zeros((nrec, len(starts)), dtype=complex)
        for i, st in enumerate(starts):
            v = np.array([1.0 + 0j])
            for vec in st:
                v = np.kron(v, np.asarray(vec, dtype=complex) / np.linalg.norm(vec))
            for q in range(nrec):
                dense[q, i] = np.vdot(v, O @ v)
                v = U @ v
        assert out["expectation_trajectories"][name].shape == (nrec, 2) and out["expectations"][name].shape == (nrec,)
        assert np.abs(dense[-1] - dense[0]).max() > 1e-3  # the observable is not a constant of this motion
        for q in range(nrec):
            bar = 2.02 * S[name] * max(q * every, 1) * 2 * (2 * L - 1) * thresh  # record 0: one step's worth, for the roundings
            worst = max(worst, np.abs(out["expectation_trajectories"][name][q] - dense[q]).max() / bar)
            worst = max(worst, abs(out["expectations"][name][q] - w @ dense[q]) / bar)
        host = out["expectation_trajectories"][name] @ w
        worst_mean = max(worst_mean, np.abs(out["expectations"][name] - host).max() / (1e-15 * np.abs(out["expectation_trajectories"][name]).max()))
    print(f"front end: |value - dense expm| {worst:.3e} of 2.02 S eps; |device mean - host mean| {worst_mean:.3f} of 1e-15 max |value|")
    assert worst < 1 and worst_mean < 1
    with pytest.raises(ValueError, match="'current'"):
        propagate_trajectories(model, starts, observables=["current"], **kw)
