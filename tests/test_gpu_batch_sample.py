"""GPU: sampled configurations of the batched trajectories (TDVPBatch.set_samples / samples,
propagate(observe=dict(samples=True)): k_batch_sample draws nshots configurations of every replica with one launch,
k_batch_mean averages the frequencies on the device) and propagate_trajectories(shots=...).

The pin is the NumPy twin (helpers/sample_cases.py), run on the tensors the engines hand back and compared decision by
decision: the inputs are chosen so that every decision is at least 1e-6 away from its boundary (shown from the twin alone
in tests/test_batch_sample_host.py and asserted again here on the tensors handed back), ten orders above the rounding of a
weight, so the configurations must be EQUAL.  The shapes are the smallest at which each part can go wrong:
  mixed  dims (2, 3, 2, 4, 2), D = 6: ragged physical dimensions, bonds narrower than the K step, d dr = 24 below a tile
  odd    dims (3,) * 5, D = 7: every bond odd, d dr = 21; 7 is no multiple of the 8 lanes that share a weight
  wide   dims (2,) * 12, D = 40: K = 40 is three K steps with a remainder, d dr = 80 three N tiles with a partial one
150 shots are two full chunks of 64 and a partial one of 22: partial tiles in M as well."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = 0.2


def _mpo(name, dims):
    from helpers import cross_cases as cc
    from helpers import pair_cases as pc
    from helpers import spin_bath as sb

    if name == "wide":
        return pc._spin_chain_mpo(len(dims))
    terms = [(0.3 + 0.1 * p, {p: cc.random_op(d, 4 + p, hermitian=True)}) for p, d in enumerate(dims)]
    terms += [(0.2, {p: cc.random_op(dims[p], 24 + p, hermitian=True), p + 1: cc.random_op(dims[p + 1], 44 + p, hermitian=True)})
              for p in range(len(dims) - 1)]
    return sb.sop_mpo(terms, list(dims))


def _batch(name, B, seed=30, states=None, **kw):
    from helpers import sample_cases as sm
    from pytdscf_amd import TDVPBatch

    dims, D = sm.SHAPES[name]
    kw = dict(dict(integrator="arnoldi", conserve_norm=False), **kw)
    bt = TDVPBatch(B, len(dims), **kw)
    bt.set_mpo(_mpo(name, dims))
    for e, cores in zip(bt.engines, states if states is not None else sm.random_states(dims, D, B, seed)):
        e.set_mps(cores)
    return bt


def _tensors(bt):
    return [e.get_mps() for e in bt.engines]


def _same_tensors(a, b):
    return all(np.array_equal(x, y) for s, t in zip(a, b) for x, y in zip(s, t))


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        assert len(xs) == len(ys)
        for x, y in zip(xs, ys):
            assert x.dtype == y.dtype and np.array_equal(x, y), k


@pytest.mark.parametrize("name", ["mixed", "odd", "wide"])
def test_the_device_draws_what_the_twin_draws(name):
    from helpers import sample_cases as sm

    dims, D = sm.SHAPES[name]
    L, B, ns = len(dims), sm.B, sm.NSHOTS
    state_seed, seed = sm.CASES[name]
    bt = _batch(name, B, seed=state_seed)
    now = _tensors(bt)
    assert max(c.shape[2] for c in now[0]) == D
    bt.set_samples(ns, seed=seed)
    w = np.array([0.5, 0.2, 0.3])
    got = bt.samples(weights=w)
    assert got["configs"].shape == (B, ns, L) and got["configs"].dtype == np.int32 and got["prob"].shape == (B, ns)
    assert [f.shape for f in got["freq"]] == [(B, d) for d in dims] and [f.shape for f in got["mean_freq"]] == [(d,) for d in dims]
    worst, least = 0.0, np.inf
    for r in range(B):
        configs, prob, margins = sm.walk_fast(now[r], ns, seed, r, 0)
        least = min(least, margins.min())
        assert np.array_equal(got["configs"][r], configs), f"replica {r}: {np.argwhere(got['configs'][r] != configs)[:4]}"
        worst = max(worst, np.abs(got["prob"][r] / prob - 1).max())
        want = sm.dense_probs(now[r])[tuple(configs.T)]
        worst = max(worst, np.abs(got["prob"][r] / want - 1).max())
        for f, h in zip(got["freq"], sm.histogram(got["configs"][r], dims)):
            assert np.array_equal(f[r], h)
    mean_dev = max(np.abs(m - w @ f).max() for m, f in zip(got["mean_freq"], got["freq"]))
    print(f"{name}: prob {worst:.2e} relative (bar 1e-12); mean_freq {mean_dev:.2e} (bar 1e-15); smallest margin {least:.2e}")
    assert least >= sm.MARGIN and worst < 1e-12 and mean_dev < 1e-15
    assert len({got["configs"][r].tobytes() for r in range(B)}) == B
    assert set(bt.samples(per_replica=False)) == {"mean_freq"}
    bt.close()


def test_bits_do_not_depend_on_nshots_on_the_chunk_or_on_the_batch():
    """shot t of nshots = 5 against shot t of nshots = 150 (another chunking of the same shots); trajectory id 7 alone in
    B = 1 against the same id and state at position 3 of B = 5"""
    from helpers import sample_cases as sm

    dims, D = sm.SHAPES["odd"]
    states = sm.random_states(dims, D, 5, seed=60)
    bt = _batch("odd", 5, states=states)
    bt.set_jumps({}, seed=11, trajectory_ids=[3, 4, 5, 7, 9])
    bt.set_samples(150, seed=2)
    big = bt.samples()
    bt.set_samples(5, seed=2)
    small = bt.samples()
    bt.set_samples(70, seed=2)  # shots 64 .. 69 are the head of the second chunk here and of the second chunk there
    mid = bt.samples()
    for k in ("configs", "prob"):
        assert np.array_equal(small[k], big[k][:, :5]) and np.array_equal(mid[k], big[k][:, :70])
    bt.close()
    one = _batch("odd", 1, states=[states[3]])
    one.set_jumps({}, seed=11, trajectory_ids=[7])
    one.set_samples(150, seed=2)
    alone = one.samples()
    one.close()
    assert np.array_equal(alone["configs"][0], big["configs"][3]) and np.array_equal(alone["prob"][0], big["prob"][3])
    assert all(np.array_equal(a[0], b[3]) for a, b in zip(alone["freq"], big["freq"]))
    assert len({big["configs"][r].tobytes() for r in range(5)}) == 5
    # the id enters the draw: the same state under another id draws other shots
    other = _batch("odd", 1, states=[states[3]])
    other.set_samples(150, seed=2)  # id 0
    assert not np.array_equal(other.samples()["configs"][0], alone["configs"][0])
    other.close()


def test_the_statistical_case():
    """"mixed", 4096 shots of two states: every one-site frequency and every cell of the (site 1, site 3) table within
    4.5 sigma of the exact value from the dense state (the bars the twin keeps in tests/test_batch_sample_host.py)"""
    from helpers import sample_cases as sm

    st = sm.STAT
    dims, _ = sm.SHAPES[st["name"]]
    bt = _batch(st["name"], st["B"], seed=st["state_seed"])
    now = _tensors(bt)
    bt.set_samples(st["nshots"], seed=st["seed"])
    got = bt.samples()
    for r in range(st["B"]):
        one, two = sm.stat_defects(got["configs"][r], now[r], st["pair"])
        print(f"state {r}: one-site {one:.2f} sigma, pair table {two:.2f} sigma")
        assert one < st["sigmas"] and two < st["sigmas"]
        configs, _, margins = sm.walk_fast(now[r], st["nshots"], st["seed"], r, 0)
        assert margins.min() >= sm.MARGIN and np.array_equal(got["configs"][r], configs)
    bt.close()


def _jump_batch(B):
    from helpers import pair_cases as pc
    from helpers import sample_cases as sm
    from pytdscf_amd import TDVPBatch

    L, g = 5, 0.3
    deph = np.stack([np.sqrt(1 - g) * np.eye(2), np.sqrt(g) * np.diag([1.0, -1.0])]).astype(complex)
    bt = TDVPBatch(B, L, integrator="arnoldi", conserve_norm=False)
    bt.set_mpo(pc._spin_chain_mpo(L))
    for e, cores in zip(bt.engines, sm.random_states((2,) * L, 4, B, seed=80)):
        e.set_mps(cores)
    bt.set_jumps({2: deph}, seed=5)
    bt.set_samples(70, seed=9)
    return bt


def test_a_recorded_run_is_the_steps_one_by_one():
    """L = 5 spin chain with a jump channel on site 2, samples at every step: every record is bitwise what propagate(dt)
    and samples() give step by step; the batch's step counter enters the draw"""
    from helpers import sample_cases as sm

    B, nsteps = 3, 2
    a, b = _jump_batch(B), _jump_batch(B)
    rec = a.propagate(DT, nsteps, observe=dict(norm=False, samples=True))
    assert rec["configs"].shape == (nsteps + 1, B, 70, 5) and rec["prob"].shape == (nsteps + 1, B, 70)
    assert [f.shape for f in rec["freq"]] == [(nsteps + 1, B, 2)] * 5 and [f.shape for f in rec["mean_freq"]] == [(nsteps + 1, 2)] * 5
    for q in range(nsteps + 1):
        if q:
            b.propagate(DT, 1)
        now = b.samples()
        for k in ("configs", "prob"):
            assert np.array_equal(rec[k][q], now[k]), (k, q)
        for k in ("freq", "mean_freq"):
            assert all(np.array_equal(x[q], y) for x, y in zip(rec[k], now[k])), (k, q)
    assert _same_tensors(_tensors(a), _tensors(b))
    assert not np.array_equal(rec["configs"][0], rec["configs"][1]) and not np.array_equal(rec["configs"][1], rec["configs"][2])
    # the last record was drawn with step = nsteps: the twin at that step on the tensors handed back, and not at step 0
    for r, cores in enumerate(_tensors(a)):
        configs, prob, margins = sm.walk_fast(cores, 70, 9, r, nsteps)
        print(f"replica {r}: smallest margin {margins.min():.2e}")
        assert margins.min() >= 1e-9 and np.array_equal(rec["configs"][-1][r], configs)
        assert np.abs(rec["prob"][-1][r] / prob - 1).max() < 1e-12
        assert not np.array_equal(sm.walk_fast(cores, 70, 9, r, 0)[0], configs)
    assert np.array_equal(a.samples()["configs"], rec["configs"][-1])  # an observation does not advance the counter
    a.close()
    b.close()


def test_an_observation_changes_nothing():
    """the tensors and the status words after samples(); norm, autocorrelation, energy, RDMs and a density key of a
    recorded run, bit for bit, with and without the request"""
    bt = _batch("mixed", 3)
    bt.propagate(DT, 1)
    bt.set_samples(150, seed=4)
    before = _tensors(bt)
    bt.samples()
    assert _same_tensors(before, _tensors(bt))
    bt.propagate(DT, 1)  # every replica still runs
    assert bt.statuses == [0, 0, 0]
    bt.close()
    req = dict(sites=[1, 3], norm=True, autocorr=True, energy=True, keys=[(0, 0, 2, 2)])
    out = []
    for with_samples in (False, True):
        bt = _batch("mixed", 3)
        if with_samples:
            bt.set_samples(70, seed=4)
        rec = bt.propagate(DT, 2, observe=dict(req, samples=True) if with_samples else req, every=1)
        out.append((dict(rec), _tensors(bt), list(bt.statuses)))
        bt.close()
    (a, ta, sa), (b, tb, sb) = out
    assert _same_tensors(ta, tb) and sa == sb == [0, 0, 0]
    assert set(b) - set(a) == {"configs", "prob", "freq", "mean_freq"}
    assert b["configs"].shape == (3, 3, 70, 5) and b["configs"].min() >= 0
    _same(a, {k: b[k] for k in a})


def test_without_a_request_nothing_changes():
    """a batch that never had a request and one whose request was removed: the launches of a recorded run and its bits"""
    out = []
    for removed in (False, True):
        bt = _batch("mixed", 3)
        bt.propagate(DT, 1)
        if removed:
            bt.set_samples(20, seed=1)
            bt.samples()
            bt.set_samples(0)
        n = bt.launches()
        rec = bt.propagate(DT, 2, observe=dict(norm=True, sites=[0, 2]))
        out.append((dict(rec), bt.launches() - n))
        with pytest.raises(ValueError, match="no samples request"):
            bt.samples()
        bt.close()
    assert out[0][1] == out[1][1] == 2 * 2 + 3 + 1
    _same(out[0][0], out[1][0])


def test_launch_counts_and_weights_of_a_recorded_run():
    bt = _batch("mixed", 3)
    bt.propagate(DT, 1)  # the engines build their right blocks with launches of their own on first use
    bt.set_samples(70, seed=6)
    n = bt.launches()
    first = bt.samples()
    assert bt.launches() - n == 2
    n = bt.launches()
    rec = bt.propagate(DT, 4, observe=dict(norm=False, samples=True), every=2)  # the request alone
    assert bt.launches() - n == 2 * 4 + 3 + 1
    assert rec["configs"].shape == (3, 3, 70, 5)
    n = bt.launches()
    bt.propagate(DT, 2, observe=dict(norm=True, sites=[1], samples=True), every=1)  # with an observation of its own
    assert bt.launches() - n == 2 * 2 + 2 * 3 + 2
    n = bt.launches()
    w = np.array([0.5, 0.2, 0.3])
    rw = bt.propagate(DT, 0, observe=dict(norm=False, samples=True, samples_weights=w))  # weights: one more mean launch
    assert bt.launches() - n == 2 + 1
    dev = max(np.abs(m[0] - w @ f[0]).max() for m, f in zip(rw["mean_freq"], rw["freq"]))
    print(f"recorded run: weighted mean_freq {dev:.2e} (bar 1e-15)")
    assert dev < 1e-15
    again = bt.samples(weights=w)
    assert np.array_equal(again["configs"], rw["configs"][0]) and all(np.array_equal(x, y[0]) for x, y in zip(again["mean_freq"], rw["mean_freq"]))
    assert not np.array_equal(first["configs"], again["configs"])
    gone = bt.engines.pop(0)  # the library's batch object is made anew and gets the request again
    fewer = bt.samples()
    assert fewer["configs"].shape == (2, 70, 5)
    gone.close()
    bt.close()


def test_a_replica_that_does_not_converge_writes_minus_one_and_zeros():
    """the set-up of test_gpu_batch_observe.py::test_a_replica_that_does_not_converge_is_recorded_as_zeros, run once"""
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

    req = dict(norm=True, samples=True)
    engs = engines((0, 1, 2))
    bt = TDVPBatch.from_engines(engs)
    bt.set_samples(70, seed=3)
    with pytest.raises(ValueError, match="Short Iterative Lanczos is not converged"):
        bt.propagate(dt, 2, observe=req, every=1)
    assert bt.statuses[1] == _lib.ENOTCONV and bt.statuses[0] == 0 and bt.statuses[2] == 0
    rec = bt.records
    assert rec["configs"].shape == (3, 3, 70, L)
    assert rec["configs"][0, 1].min() >= 0 and np.all(rec["prob"][0, 1] > 0)  # observed before it failed
    assert np.all(rec["configs"][1:, 1] == -1) and np.all(rec["prob"][1:, 1] == 0) and all(np.all(f[1:, 1] == 0) for f in rec["freq"])
    good = engines((0, 2))
    ok = TDVPBatch.from_engines(good)
    ok.set_jumps({}, trajectory_ids=[0, 2])
    ok.set_samples(70, seed=3)
    ref = ok.propagate(dt, 2, observe=req, every=1)
    assert ref["configs"].min() >= 0
    for k in ("configs", "prob"):
        assert np.array_equal(rec[k][:, [0, 2]], ref[k])
    bt.close()
    ok.close()
    for e in engs + good:
        e.close()


def test_every_refusal_names_itself_and_changes_nothing():
    from helpers import sample_cases as sm
    from pytdscf_amd import TDVPBatch, _lib
    from pytdscf_amd.mps import product_state_cores

    dims, _ = sm.SHAPES["mixed"]
    L = len(dims)
    none = [None] * 5
    fresh = _batch("mixed", 2)
    with pytest.raises(ValueError, match="no samples request"):
        fresh.samples()
    with pytest.raises(ValueError, match=r"mitdvp_batch_samples: no samples request is set \(mitdvp_batch_set_samples\)"):
        _lib.check(fresh._lib.mitdvp_batch_samples(fresh._handle(), *none, None))
    assert fresh._lib.mitdvp_batch_set_samples(fresh._handle(), 0, 0) == 0  # removing nothing is fine
    cnt = (C.c_size_t * 5)()
    assert fresh._lib.mitdvp_batch_samples_records(fresh._handle(), *none, cnt) == 0 and list(cnt)[:2] == [0, 2]
    fresh.close()
    assert _lib.load().mitdvp_batch_set_samples(None, 1, 0) == _lib.EINVAL

    bt = _batch("mixed", 3)
    bt.set_samples(70, seed=8)
    run = bt.propagate(DT, 1, observe=dict(norm=False, samples=True))
    before, n0, tensors = bt.samples(), bt.launches(), _tensors(bt)
    for nshots, match in [(-1, r"nshots = -1 is outside 0 \.\. 65536"), (65537, r"nshots = 65537 is outside 0 \.\. 65536")]:
        with pytest.raises(ValueError, match="mitdvp_batch_set_samples: " + match):
            bt.set_samples(nshots, seed=1)
    with pytest.raises(ValueError, match="samples request"):
        bt.set_samples(1.5)
    with pytest.raises(ValueError, match="one per replica"):
        bt.samples(weights=[1.0])
    assert bt.launches() == n0
    cnt4 = (C.c_size_t * 4)()
    assert bt._lib.mitdvp_batch_samples(bt._handle(), *none, cnt4) == 0 and list(cnt4) == [3, 70, L, sum(dims)]  # no launch
    assert bt.launches() == n0
    _same(bt.samples(), before)  # the request is the one of before
    kept = bt._samples_records(None)  # and so are the records of the run
    assert kept["configs"].shape == (2, 3, 70, L)
    _same(kept, {k: run[k] for k in kept})
    assert _same_tensors(tensors, _tensors(bt))
    bt.sweep(DT, True)  # the centre is at the last site now
    moved = _tensors(bt)
    with pytest.raises(ValueError, match=rf"mitdvp_batch_samples: replica 0 has its centre at site {L - 1}"):
        bt.samples()
    assert _same_tensors(moved, _tensors(bt))
    bt.sweep(DT, False)
    assert bt.samples()["configs"].shape == (3, 70, L)
    bt.close()

    # nshots * L above 2^22: 65536 shots of a chain of 65 sites; of 64 sites they are taken.  Nothing is launched.
    for nsite, ok in ((65, False), (64, True)):
        long = TDVPBatch(1, nsite)
        long.set_mpo([np.diag([0.5, -0.5]).astype(complex).reshape(1, 2, 2, 1)] * nsite)
        long[0].set_mps(product_state_cores([[1, 0]] * nsite, 2))
        if ok:
            long.set_samples(65536)
            assert long._lib.mitdvp_batch_samples(long._handle(), *none, cnt4) == 0 and list(cnt4) == [1, 65536, 64, 128]
        else:
            with pytest.raises(ValueError, match=r"mitdvp_batch_set_samples: 65536 shots of 65 sites are 4259840 outcomes per replica, "
                                                 r"a request takes at most 4194304"):
                long.set_samples(65536)
            long.set_samples(64527)  # 64527 * 65 = 4194255
        long.close()


def test_propagate_trajectories_with_shots():
    """the dephasing spin chain: L = 6, D = 4, two product starts x two replicas: the new entries and their shapes, the
    device mean of the frequencies against the host mean of the histograms, and exactly the old dict without the keyword"""
    from helpers import pair_cases as pc
    from helpers import sample_cases as sm
    from pytdscf_amd import Exciton, Model, propagate_trajectories, units

    L, g = 6, 0.1
    deph = np.stack([np.sqrt(1 - g) * np.eye(2), np.sqrt(g) * np.diag([1.0, -1.0])]).astype(complex)
    model = Model([Exciton(nstate=2) for _ in range(L)], operators={"hamiltonian": pc._spin_chain_mpo(L)}, bond_dim=4)
    starts = [[[1, 0], [0, 1]] * (L // 2), [[1, 1], [1, -1]] * (L // 2)]  # Neel states along z and along x
    w = np.array([0.1, 0.2, 0.3, 0.4])
    kw = dict(maxstep=5, stepsize=0.4 * units.au_in_fs, reduced_density=([(1, 1)], 2), integrator="arnoldi", conserve_norm=False,
              jumps={p: deph for p in range(L)}, seed=3, replicas_per_start=2, weights=w, per_trajectory=True)
    base = propagate_trajectories(model, starts, **kw)
    out = propagate_trajectories(model, starts, shots=100, shot_seed=5, **kw)
    assert set(base) == {"time", "mean", "trajectories"} and set(out) == set(base) | {"configurations", "frequencies"}
    assert np.array_equal(out["time"], base["time"])
    assert np.array_equal(out["mean"][(1, 1)], base["mean"][(1, 1)]) and np.array_equal(out["trajectories"][(1, 1)], base["trajectories"][(1, 1)])
    cfg = out["configurations"]
    assert cfg.shape == (3, 4, 100, L) and cfg.dtype == np.int32 and cfg.min() >= 0 and cfg.max() <= 1
    assert [f.shape for f in out["frequencies"]] == [(3, 2)] * L
    assert np.array_equal(cfg[0, 0], np.tile([0, 1] * (L // 2), (100, 1)))  # the z Neel start has one configuration
    for p in range(L):
        host = np.array([sum(w[r] * sm.histogram(cfg[q, r], [2] * L)[p] for r in range(4)) for q in range(3)])
        assert np.abs(out["frequencies"][p] - host).max() < 1e-15
    slim = propagate_trajectories(model, starts, shots=100, shot_seed=5, **dict(kw, per_trajectory=False))
    assert set(slim) == {"time", "mean", "configurations", "frequencies"} and np.array_equal(slim["configurations"], cfg)
    # chunks of an ensemble draw what the whole ensemble draws
    tail = propagate_trajectories(model, starts[1:], shots=100, shot_seed=5, first_trajectory=2, **dict(kw, weights=None))
    assert np.array_equal(tail["configurations"], cfg[:, 2:])
    with pytest.raises(ValueError, match="shots must be >= 1"):
        propagate_trajectories(model, starts, shots=0, **kw)
