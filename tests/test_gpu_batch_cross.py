"""GPU: cross overlaps and one-site matrix elements between the replicas of a batch and their snapshots
(TDVPBatch.snapshot / set_cross / cross, propagate(observe=dict(cross=True)): k_batch_cross forms every pair with one
launch, k_batch_mean sums them on the device) and trajectories.correlation_function.  Values are compared with a host
contraction of the tensors the engines hand back at 1e-12 |psi_a| |psi_b| (the rounding of the walk is about
L (dl d) eps < 1e-13 at these shapes; 1e-12 is the project's norm bar); the observed defects are printed."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = 0.2


def _mixed_mpo(dims, seed=4):
    """one-site and nearest-neighbour terms for any physical dimensions"""
    from helpers import cross_cases as cc
    from helpers import spin_bath as sb

    terms = [(0.3 + 0.1 * p, {p: cc.random_op(d, seed + p, hermitian=True)}) for p, d in enumerate(dims)]
    terms += [(0.2, {p: cc.random_op(dims[p], seed + 20 + p, hermitian=True), p + 1: cc.random_op(dims[p + 1], seed + 40 + p, hermitian=True)})
              for p in range(len(dims) - 1)]
    return sb.sop_mpo(terms, list(dims))


def _batch(dims, D, B, mpo, seed=30, **kw):
    """B replicas with random states of norms 0.7, 0.9, 1.1, ...; no rescaling in a step, so the norms stay apart"""
    from helpers import cross_cases as cc
    from pytdscf_amd import TDVPBatch

    kw = dict(dict(integrator="arnoldi", conserve_norm=False), **kw)
    bt = TDVPBatch(B, len(dims), **kw)
    bt.set_mpo(mpo)
    for e, cores in zip(bt.engines, cc.random_states(dims, D, B, seed)):
        e.set_mps(cores)
    return bt


SHAPES = {"mixed": ((2, 3, 2, 4, 2), 6), "wide": ((2,) * 12, 40)}


@pytest.mark.parametrize("name", list(SHAPES))
def test_values_equal_a_host_contraction(name):
    """a = b, a != b, (a, b) and (b, a) conjugate for a Hermitian operator, snapshot bras and kets, a non-Hermitian
    operator on the first, a middle and the last site; P = 1, P < B and P > B.  'wide': bonds 2 .. 40 pass the 32-wide
    tile and the 16-deep K step of the workgroup product and are multiples of neither."""
    from helpers import cross_cases as cc
    from helpers import pair_cases as pc

    dims, D = SHAPES[name]
    L, B = len(dims), 3
    bt = _batch(dims, D, B, _mixed_mpo(dims) if name == "mixed" else pc._spin_chain_mpo(L))
    if name == "wide":
        assert max(c.shape[2] for c in bt[0].get_mps()) == 40
    old = [e.get_mps() for e in bt.engines]
    bt.snapshot()
    bt.propagate(DT, 1)
    now = [e.get_mps() for e in bt.engines]
    state = lambda i: now[i] if i < B else old[i - B]
    mid = L // 2
    H = cc.random_op(dims[mid], 1, hermitian=True)
    N0, N1 = cc.random_op(dims[0], 2), cc.random_op(dims[L - 1], 3)
    entries = [(0, 0), (0, 1), (1, 0), (0, 1, mid, H), (1, 0, mid, H), (bt.snap(2), 1), (2, bt.snap(1)), (bt.snap(0), 0, 0, N0),
               (2, 1, L - 1, N1), (bt.snap(1), bt.snap(2), mid, H), (1, 2, 0, N0)]
    worst = 0.0
    assert len(entries) > B
    for P in (1, 2, len(entries)):  # one pair, fewer than replicas, more than replicas
        bt.set_cross(entries[1:1 + P] if P < 3 else entries)
        got = bt.cross()
        for e, v in zip(entries[1:1 + P] if P < 3 else entries, got["values"]):
            e = tuple(e) + (-1, None) if len(e) == 2 else e
            a, b = state(e[0]), state(e[1])
            bar = 1e-12 * cc.norm_of(a) * cc.norm_of(b)
            want = cc.walk(a, b, e[2], e[3])
            worst = max(worst, abs(v - want) / bar)
            assert abs(v - want) < bar, (name, P, e[:3], v, want)
        assert abs(got["mean"] - got["values"].mean()) < 1e-13 * np.abs(got["values"]).max()
    v = got["values"]
    bar = 2e-12 * cc.norm_of(now[0]) * cc.norm_of(now[1])  # each of the two values is within 1e-12 |a| |b| of the exact one
    assert abs(v[1] - np.conj(v[2])) < bar and abs(v[3] - np.conj(v[4])) < bar * np.linalg.norm(H, 2)
    assert min(abs(v[1]), abs(v[3]), abs(v[8])) > 1e-6  # nothing here compares two zeros
    assert abs(cc.walk(old[2], now[1]) - cc.walk(now[2], now[1])) > 1e-6  # the step moved the states off their snapshots
    w = np.linspace(0.5, 1.5, len(entries))
    assert abs(bt.cross(weights=w)["mean"] - (w * v).sum()) < 1e-13 * np.abs(v).max() * w.sum()
    print(f"{name}: worst |device - host| = {worst:.3f} of the bar 1e-12 |a| |b|")
    bt.close()


def test_a_state_with_itself_is_the_observed_norm():
    dims, D = SHAPES["mixed"]
    bt = _batch(dims, D, 4, _mixed_mpo(dims))
    bt.propagate(DT, 1)
    bt.set_cross([(r, r) for r in range(4)])
    v = bt.cross()["values"]
    n2 = bt.observe()["norm"] ** 2
    assert np.abs(n2 - [0.49, 0.81, 1.21, 1.69]).max() < 1e-6  # different norms, kept by a Hermitian operator
    assert np.all(np.abs(v.real - n2) < 1e-13 * n2) and np.all(np.abs(v.imag) < 1e-13 * n2)
    bt.close()


def test_the_snapshot_pair_is_the_engines_own_reference_overlap():
    dims, D = SHAPES["mixed"]
    bt = _batch(dims, D, 3, _mixed_mpo(dims))
    for e in bt.engines:
        e.save_reference()
    bt.snapshot()
    bt.set_cross([(bt.snap(r), r) for r in range(3)])
    bt.propagate(DT, 2)
    v = bt.cross()["values"]
    own = np.array([e.overlap_reference() for e in bt.engines])
    print(f"snapshot pair against overlap_reference: {np.abs(v - own).max():.2e}")
    assert np.abs(v - own).max() < 1e-8
    assert np.abs(v - [0.49, 0.81, 1.21]).min() > 1e-3  # the state left its snapshot
    bt.close()


def test_bits_do_not_depend_on_the_list_and_a_record_is_the_call():
    from helpers import cross_cases as cc

    dims, D = SHAPES["mixed"]
    bt = _batch(dims, D, 3, _mixed_mpo(dims))
    bt.snapshot()
    bt.propagate(DT, 1)
    O = cc.random_op(dims[3], 5)
    entry = (bt.snap(1), 2, 3, O)
    bt.set_cross([entry])
    alone = bt.cross()["values"][0]
    filler = [(r % 3, (r + 1) % 3, r % 5, cc.random_op(dims[r % 5], r)) if r % 2 else (r % 6, (r + 2) % 6) for r in range(70)]
    filler[37] = entry
    bt.set_cross(filler)
    many = bt.cross()["values"]
    assert many[37] == alone and abs(alone) > 1e-6
    assert len(set(many.tolist())) > 20
    # a recorded run's records are cross() at the same steps
    before = bt.cross()["values"]
    rec = bt.propagate(DT, 2, observe=dict(norm=False, cross=True), every=2)
    after = bt.cross()["values"]
    assert rec["cross"].shape == (2, 70) and rec["mean_cross"].shape == (2,)
    assert np.array_equal(rec["cross"][0], before) and np.array_equal(rec["cross"][1], after)
    assert not np.array_equal(before, after)
    assert np.array_equal(bt.propagate(0.0, 0, observe=dict(norm=False, cross=True))["cross"][0], after)
    w = np.linspace(-1, 1, 70)
    rw = bt.propagate(DT, 0, observe=dict(norm=False, cross=True, cross_weights=w))
    assert abs(rw["mean_cross"][0] - (w * after).sum()) < 1e-13 * np.abs(after).max() * np.abs(w).sum()
    bt.close()


def test_without_a_request_nothing_changes():
    """records and launch counts of a recorded run on a batch that never had a request, and on one whose request was
    set and removed again"""
    dims, D = SHAPES["mixed"]
    req = dict(sites=[1, 3], norm=True, autocorr=True, energy=True, keys=[(0, 0, 2, 2)])
    out = []
    for touched in (False, True):
        bt = _batch(dims, D, 3, _mixed_mpo(dims))
        if touched:
            bt.snapshot()
            bt.set_cross([(0, 1), (bt.snap(2), 0)])
            bt.set_cross([])
            with pytest.raises(ValueError, match="no cross request"):
                bt.cross()
        bt.propagate(DT, 1)  # the engines build their right blocks with launches of their own on first use
        n0 = bt.launches()
        rec = bt.propagate(DT, 2, observe=req, every=1)
        out.append((rec, bt.launches() - n0))
        bt.close()
    (a, na), (b, nb) = out
    assert na == nb == 2 * 2 + 3 * 2 + 1
    assert a.keys() == b.keys() and "cross" not in a
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for x, y in zip(xs, ys):
            assert np.array_equal(x, y), k


def test_launch_counts_with_a_request():
    dims, D = SHAPES["mixed"]
    bt = _batch(dims, D, 3, _mixed_mpo(dims))
    bt.propagate(DT, 1)  # the engines build their right blocks with launches of their own on first use
    n = bt.launches()
    bt.snapshot()
    assert bt.launches() - n == 1
    bt.set_cross([(0, 1), (bt.snap(0), 2), (1, 1)])
    n = bt.launches()
    bt.cross()
    assert bt.launches() - n == 2
    n = bt.launches()
    bt.propagate(DT, 4, observe=dict(norm=True, cross=True), every=2)  # 3 records
    assert bt.launches() - n == 2 * 4 + 2 * 3 + 2
    n = bt.launches()
    bt.propagate(DT, 4, observe=dict(norm=False, cross=True), every=2)  # the request alone
    assert bt.launches() - n == 2 * 4 + 3 + 1
    n = bt.launches()
    bt.propagate(DT, 0, observe=dict(norm=False, cross=True, cross_weights=[1.0, 2.0, 3.0]))  # weights: one more mean launch
    assert bt.launches() - n == 2 + 1
    bt.close()


def test_a_replica_that_does_not_converge_gives_zeros_for_its_pairs():
    """the set-up of test_gpu_batch_observe.py: replica 1 has an operator a thousand times hotter and max_krylov = 8"""
    from pytdscf_amd import TDVPBatch, TDVPEngine, _lib
    from pytdscf_amd import synthetic as syn

    L, d, D, M, dt = 4, 3, 6, 3, 0.02
    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    hot = [w.copy() for w in mpo]
    hot[0] = hot[0] * 1e3

    def engines(which):
        out = []
        for r in which:
            e = TDVPEngine(L, max_krylov=8)
            e.set_mpo(hot if r == 1 else mpo)
            e.init_random([d] * L, D, seed=50 + r)
            out.append(e)
        return out

    bt = TDVPBatch.from_engines(engines((0, 1, 2)))
    bt.snapshot()
    bt.set_cross([(0, 2), (0, 1), (1, 1), (2, 1), (bt.snap(1), 2), (bt.snap(0), 1)])
    with pytest.raises(ValueError, match="Short Iterative Lanczos is not converged"):
        bt.propagate(dt, 2, observe=dict(norm=True, cross=True), every=1)
    assert bt.statuses == [0, _lib.ENOTCONV, 0]
    got = bt.records["cross"]
    assert got.shape == (3, 6) and np.all(np.abs(got[0]) > 0) and abs(got[0, 2] - 1) < 1e-12
    assert np.all(got[1:, [1, 2, 3, 5]] == 0)
    ok = TDVPBatch.from_engines(engines((0, 2)))
    ok.snapshot()
    ok.set_cross([(0, 1)])
    ref = ok.propagate(dt, 2, observe=dict(norm=True, cross=True), every=1)["cross"]
    assert np.array_equal(got[:, 0], ref[:, 0])
    assert np.all(np.abs(got[1:, 4]) > 0)  # the snapshot of the replica that failed later is still a state
    bt.close()
    ok.close()


def test_every_refusal_names_itself_and_changes_nothing():
    from helpers import cross_cases as cc
    from pytdscf_amd import _lib

    dims, D = SHAPES["mixed"]
    L, B = len(dims), 3
    fresh = _batch(dims, D, B, _mixed_mpo(dims))
    with pytest.raises(ValueError, match=r"mitdvp_batch_set_cross: pair 1: bra index 4 names the snapshot of replica 1.*no snapshot"):
        fresh.set_cross([(0, 1), (fresh.snap(1), 0)])
    assert fresh._lib.mitdvp_batch_set_cross(fresh._handle(), 0, None, None, None, None, None) == 0  # removing nothing is fine
    with pytest.raises(ValueError, match="mitdvp_batch_cross: no cross request"):
        _lib.check(fresh._lib.mitdvp_batch_cross(fresh._handle(), None, None, None))
    fresh.close()

    bt = _batch(dims, D, B, _mixed_mpo(dims))
    bt.snapshot()
    good = [(0, 1), (bt.snap(2), 1, 1, cc.random_op(3, 1))]
    bt.set_cross(good)
    before, n0 = bt.cross(), bt.launches()
    tensors = [e.get_mps() for e in bt.engines]
    O2, O3 = cc.random_op(2, 2), cc.random_op(3, 3)
    bad = [([(0, 2 * B)], r"pair 0: ket index 6 is outside 0 \.\. 5"),
           ([(0, 1), (-1, 0)], r"pair 1: bra index -1 is outside 0 \.\. 5"),
           ([(0, 1, L, O2)], rf"pair 0: site {L} is out of range"),
           ([(0, 1, -2, O2)], r"pair 0: site -2 is out of range"),
           ([(0, 1), (1, 2, 1, O2)], r"pair 1: the operator is 2 x 2, the physical dimension of site 1 is 3"),
           ([(0, 1, 0, O3)], r"pair 0: the operator is 3 x 3, the physical dimension of site 0 is 2"),
           ([(0, 1)] * 65537, r"65537 pairs, a request takes at most 65536")]
    for entries, match in bad:
        with pytest.raises(ValueError, match="mitdvp_batch_set_cross: " + match):
            bt.set_cross(entries)
    with pytest.raises(ValueError, match="one per pair"):
        bt.cross(weights=[1.0])
    assert bt.launches() == n0
    after = bt.cross()
    assert np.array_equal(after["values"], before["values"]) and after["mean"] == before["mean"]
    for e, t in zip(bt.engines, tensors):
        assert all(np.array_equal(x, y) for x, y in zip(e.get_mps(), t))
    bt.set_cross([(0, 1)] * 65536)  # the limit itself is taken
    assert bt.cross()["values"].shape == (65536,)
    bt.close()


def test_correlation_function_on_the_physics_case():
    """<psi| A(t) B |psi> and <psi(0)|psi(t)> of the L = 4 spin chain from a complex product start: against the NumPy
    oracle at the project's 1e-8 bar, against dense expm within ten times the oracle's own deviation from it (the oracle:
    2.6e-12 and 3e-14, see tests/test_batch_cross_host.py), and out of the reach of the t/2 trick."""
    from helpers import cross_cases as cc
    from helpers import pair_cases as pc
    from pytdscf_amd import TDVPBatch, units
    from pytdscf_amd.mps import product_state_cores
    from pytdscf_amd.trajectories import correlation_function

    corr, auto, _ = cc.dense()
    oc = cc.oracle_corr("arnoldi", 1e-9)
    oa, _ = cc.oracle_auto("arnoldi", 1e-9)
    dev_oc, dev_oa = np.abs(oc - corr).max(), np.abs(oa - auto).max()
    m = cc.model()
    kw = dict(maxstep=cc.NSTEPS + 1, stepsize=cc.DT * units.au_in_fs)
    got = correlation_function(m, [cc.START], A=cc.A_OP, B=cc.B_OP, per_trajectory=True, **kw)
    assert got["mean"].shape == (cc.NSTEPS + 1,) and got["trajectories"].shape == (cc.NSTEPS + 1, 1)
    assert np.allclose(got["time"], np.arange(cc.NSTEPS + 1) * cc.DT * units.au_in_fs)
    assert np.array_equal(got["mean"], got["trajectories"][:, 0])
    d_or, d_de = np.abs(got["mean"] - oc).max(), np.abs(got["mean"] - corr).max()
    ga = correlation_function(m, [cc.START], **kw)["mean"]
    a_or, a_de = np.abs(ga - oa).max(), np.abs(ga - auto).max()
    print(f"C(t): device vs oracle {d_or:.2e}, device vs dense {d_de:.2e}, oracle vs dense {dev_oc:.2e}; "
          f"<psi(0)|psi(t)>: device vs oracle {a_or:.2e}, device vs dense {a_de:.2e}, oracle vs dense {dev_oa:.2e}")
    # the t/2 trick on the same start: the batch's own autocorr record after 4 steps claims <psi(0)|psi(8 dt)>
    bt = TDVPBatch(1, cc.L, integrator="arnoldi", conserve_norm=False, thresh=1e-9)
    bt.set_mpo(pc._spin_chain_mpo(cc.L))
    bt[0].set_mps(product_state_cores(cc.START, cc.D), canonicalize=True, scale=1.0)
    trick = bt.propagate(cc.DT, 4, observe=dict(norm=False, autocorr=True), every=4)["autocorr"][1, 0]
    bt.close()
    print(f"t/2 trick after 4 steps {trick:.4f}, <psi(0)|psi(8 dt)> {ga[8]:.4f}: {abs(trick - ga[8]):.3f} apart")
    assert d_or < 1e-8 and a_or < 1e-8
    assert d_de < 10 * dev_oc and a_de < 10 * dev_oa
    assert abs(trick - ga[8]) > 0.1
    # two starts with weights: the second is the first with another site-0 vector; the mean is the weighted sum
    other = [[0.6, 0.8j]] + cc.START[1:]
    two = correlation_function(m, [cc.START, other], A=cc.A_OP, B=cc.B_OP, weights=[0.25, 0.75], per_trajectory=True, every=2, **kw)
    assert two["trajectories"].shape == (5, 2) and np.array_equal(two["trajectories"][:, 0], got["mean"][::2])
    assert np.abs(two["mean"] - two["trajectories"] @ [0.25, 0.75]).max() < 1e-15
