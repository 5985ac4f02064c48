"""GPU: multi-site reduced densities of the batched trajectories (TDVPBatch.densities / propagate(observe=dict(keys=...)),
mitdvp_batch_observe_keys / mitdvp_batch_run_keys: k_batch_density forms every key of every replica with one launch,
k_batch_mean averages on the device) and propagate_trajectories(densities=...).  Bars (README, as
tests/test_gpu_batch_observe.py): densities against the engines' own reduced_density 1e-9; device means against the
per-replica output B 2^-52 times the largest magnitude.  The observed defects are printed."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALL = dict(norm=True, autocorr=True, energy=True)


def _batch(B, mpo, dims, D, seeds, **kw):
    from pytdscf_amd import TDVPBatch

    bt = TDVPBatch(B, len(dims), **kw)
    bt.set_mpo(mpo)
    for e, s in zip(bt.engines, seeds):
        e.init_random(dims, D, seed=s)
    return bt


def _nonhermitian(mpo):
    out = [w.copy() for w in mpo]
    out[0] = out[0] * (1.0 - 0.1j)
    return out


def _against_engines(bt, keys, label, which=None, weights=None):
    """one batched observation against every (or the picked) engine's own reduced_density on the same state"""
    from pytdscf_amd.engine import density_key_legs

    L = bt[0].nsite
    o = bt.densities(keys, weights=weights)
    assert len(o["density"]) == len(keys) and len(o["mean_density"]) == len(keys)
    worst = 0.0
    for r in (range(len(bt)) if which is None else which):
        for k, key in enumerate(keys):
            ref = bt[r].reduced_density(density_key_legs(key, L))
            got = o["density"][k][r]
            assert got.shape == ref.shape and o["mean_density"][k].shape == ref.shape, (key, got.shape, ref.shape)
            defect = np.abs(got - ref).max()
            worst = max(worst, defect)
            assert defect < 1e-9, (label, r, key, defect)
    print(f"{label}: worst |density - engine's reduced_density| {worst:.2e}")
    return o


def _means_follow(o, w, B, label):
    eps = B * 2.0 ** -52  # the rounding of a length-B sum of terms bounded by max |density| (sum w = 1)
    for k, per in enumerate(o["density"]):
        ref = np.tensordot(w, per, axes=(0, 0))
        defect, bound = np.abs(o["mean_density"][k] - ref).max(), eps * np.abs(per).max()
        print(f"{label}: device mean of key {k}: defect {defect:.2e} bound {bound:.2e}")
        assert defect <= bound, (label, k, defect, bound)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        assert len(xs) == len(ys)
        for x, y in zip(xs, ys):
            assert np.array_equal(x, y), k


PARITY_KEYS = [(0, 0, 2, 2), (1, 3), (1, 2, 2, 4), (0, 0, 1, 1, 2, 2), (4, 4), (0,)]


@pytest.mark.parametrize("integrator, cn", [("lanczos", True), ("arnoldi", False)])
def test_parity_with_the_engines_own_reduced_density(integrator, cn):
    """a gap site, a diagonal pair, mixed legs with the last site of the chain, 81 open legs, one site, one diagonal"""
    from pytdscf_amd import synthetic as syn

    L, d, D, M, B, dt = 5, 3, 7, 5, 3, 0.4
    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    if not cn:
        mpo = _nonhermitian(mpo)
    bt = _batch(B, mpo, [d] * L, D, [11, 12, 13], integrator=integrator, conserve_norm=cn)
    _against_engines(bt, PARITY_KEYS, f"{integrator} before any step")
    bt.propagate(dt, 2)
    o = _against_engines(bt, PARITY_KEYS, f"{integrator} after two steps")
    assert o["density"][3].shape == (B,) + (d,) * 6 and o["density"][1].shape == (B, d, d)
    for r in range(B):
        defect = np.abs(o["density"][4][r] - bt[r].site_rdm(4)).max()
        assert defect < 1e-9, (r, defect)
    _means_follow(o, np.full(B, 1.0 / B), B, integrator)
    bt.close()


@pytest.mark.parametrize("dims, D, keys", [
    ([2, 3, 2], 4, [(0, 0, 1, 1), (0, 0, 2, 2), (0, 2), (0, 1, 1)]),
    ([8, 8, 8, 8], 3, [(1, 1, 3, 3)]),
    ([5], 1, [(0, 0), (0,)]),
    ([2] * 14, 64, [(6, 6, 7, 7), (0, 13)]),
])
def test_awkward_shapes(dims, D, keys):
    """mixed physical dimensions, 64 open legs on bonds of 3, a one-site chain, and the envelope corner 64 x 2 x 64 with a
    pair in the middle and two open values carried across twelve sites"""
    from helpers import spin_bath as sb
    from pytdscf_amd import synthetic as syn

    L = len(dims)
    kw = {}
    if dims == [2, 3, 2]:
        mpo, kw = sb.sop_mpo(sb.hilbert_terms(0, 1, 2), dims), dict(integrator="arnoldi", conserve_norm=False)
    else:
        mpo = syn.synthetic_mpo(L, dims[0], 3 if L > 4 else 4, seed=2)
    bt = _batch(2, mpo, dims, D, [5, 6], **kw)
    _against_engines(bt, keys, f"{dims[:4]} D={D} before a step")
    bt.propagate(0.1, 1)
    _against_engines(bt, keys, f"{dims[:4]} D={D} after a step")
    bt.close()


def test_a_replicas_densities_do_not_depend_on_the_batch():
    from pytdscf_amd import synthetic as syn

    L, d, D, M, dt = 5, 3, 7, 4, 0.4
    mpo = syn.synthetic_mpo(L, d, M, seed=1)
    seeds = [60 + r for r in range(9)]
    big = _batch(9, mpo, [d] * L, D, seeds)
    one = _batch(1, mpo, [d] * L, D, [seeds[4]])
    big.propagate(dt, 1)
    one.propagate(dt, 1)
    keys = [(0, 0, 2, 2), (1, 2, 2, 4), (1, 3)]
    a, b = big.densities(keys), one.densities(keys)
    for x, y in zip(a["density"], b["density"]):
        assert np.abs(y).max() > 0 and np.array_equal(x[4:5], y)
    big.close()
    one.close()


def test_more_replicas_than_compute_units_and_the_device_mean():
    from pytdscf_amd import synthetic as syn

    L, d, D, M, B, dt = 4, 2, 4, 3, 300, 0.5
    mpo = _nonhermitian(syn.synthetic_mpo(L, d, M, seed=0))
    bt = _batch(B, mpo, [d] * L, D, [100 + r for r in range(B)], integrator="arnoldi", conserve_norm=False)
    bt.propagate(dt)
    w = np.random.default_rng(3).random(B) + 0.1
    w /= w.sum()
    o = _against_engines(bt, [(1, 1, 3, 3)], "B = 300", which=(0, 149, 299), weights=w)
    assert o["density"][0].shape == (B, d, d, d, d)
    _means_follow(o, w, B, "B = 300")
    bt.close()


def test_a_recorded_run_equals_observing_by_hand():
    from pytdscf_amd import synthetic as syn

    L, d, D, M, B, dt = 5, 3, 7, 4, 3, 0.3
    mpo = syn.synthetic_mpo(L, d, M, seed=2)
    seeds = [71, 72, 73]
    a, b, c, e = (_batch(B, mpo, [d] * L, D, seeds) for _ in range(4))
    for bt in (a, b, c, e):
        bt.propagate(dt, 1)  # the engines build their right blocks with their own launches, once
    for eng in a.engines:
        eng.counters_reset()
    keys = [(0, 0, 3, 3), (1, 2, 2), (2, 4)]
    plain = dict(sites=[0, 3, 4], **ALL)
    rec = a.propagate(dt, 4, observe=dict(keys=keys, **plain), every=2)
    nl = a[0].counters()["n_launch"]
    print(f"recorded run with keys: {nl} launches for 4 steps and 3 records")
    assert nl <= 2 * 4 + 2 * 3 + 1 and a[1].counters()["n_launch"] == 0
    assert rec["density"][0].shape == (3, B, d, d, d, d) and rec["mean_density"][1].shape == (3, d, d, d)
    assert rec["density"][2].shape == (3, B, d, d)
    # by hand: the observation of before, then the keys alone
    hand = [dict(b.observe(**plain), **b.densities(keys))]
    for _ in range(2):
        assert b.propagate(dt, 2) is None
        hand.append(dict(b.observe(**plain), **b.densities(keys)))
    for q in range(3):
        _same({k: ([x[q] for x in v] if isinstance(v, list) else v[q]) for k, v in rec.items()}, hand[q])
    # the request without keys: its entries are bitwise what they are with them
    without = c.propagate(dt, 4, observe=plain, every=2)
    assert "density" not in without and "mean_density" not in without
    _same({k: v for k, v in rec.items() if k not in ("density", "mean_density")}, without)
    # the keys alone (k_batch_observe is skipped, k_batch_density zeroes the head of the record)
    for eng in e.engines:
        eng.counters_reset()
    alone = e.propagate(dt, 4, observe=dict(norm=False, keys=keys), every=2)
    assert e[0].counters()["n_launch"] <= 2 * 4 + 3 + 1
    _same(alone, {k: rec[k] for k in ("mean_density", "density")})
    for bt in (a, b, c, e):
        bt.close()


def test_a_replica_that_does_not_converge_has_zero_densities():
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

    req = dict(sites=[0, 2], keys=[(0, 0, 2, 2), (1, 3)], **ALL)
    engs = engines((0, 1, 2))
    bt = TDVPBatch.from_engines(engs)
    with pytest.raises(ValueError, match="Short Iterative Lanczos is not converged"):
        bt.propagate(dt, 2, observe=req, every=1)
    assert bt.statuses[1] == _lib.ENOTCONV and bt.statuses[0] == 0 and bt.statuses[2] == 0
    rec = bt.records
    assert rec["density"][0].shape == (3, 3, d, d, d, d) and rec["density"][1].shape == (3, 3, d, d)
    for x in rec["density"]:
        assert np.all(x[1:, 1] == 0) and np.abs(x[0, 1]).max() > 0  # observed before it failed, zeros from then on
    good = engines((0, 2))
    ok = TDVPBatch.from_engines(good)
    ref = ok.propagate(dt, 2, observe=req, every=1)
    for x, y in zip(rec["density"], ref["density"]):
        assert np.abs(y).max() > 0 and np.array_equal(x[:, [0, 2]], y)
    for x, y in zip(rec["rdm"], ref["rdm"]):
        assert np.array_equal(x[:, [0, 2]], y)
    bt.close()
    ok.close()
    for e in engs + good:
        e.close()


def test_refusals_leave_the_engines_untouched():
    from pytdscf_amd import _lib
    from pytdscf_amd import synthetic as syn

    L, d, D, M, dt = 6, 4, 32, 3, 0.1
    bt = _batch(2, syn.synthetic_mpo(L, d, M, seed=0), [d] * L, D, [1, 2])
    lib = _lib.load()

    def raw(rows):
        """the library itself, past the Python key parser: a validation call with these rows of leg counts"""
        flat = [x for row in rows for x in row]
        cnt = (C.c_size_t * 4)()
        _lib.check(lib.mitdvp_batch_observe_keys(bt._handle(), None, 0, (C.c_int * len(flat))(*flat), len(rows), 0, None, None,
                                                 None, None, cnt))
        return list(cnt)

    def refused(call, match):
        before = [e.get_mps() for e in bt.engines]
        with pytest.raises(ValueError, match=match):
            call()
        for e, b in zip(bt.engines, before):
            for x, y in zip(e.get_mps(), b):
                assert np.array_equal(x, y)

    assert raw([[0, 2, 2, 0, 0, 0], [1, 0, 0, 0, 0, 1]]) == [1, 2, 0, d ** 4 + d * d]
    refused(lambda: raw([[0, 3, 0, 0, 0, 0]]), "must be 0, 1 or 2")
    refused(lambda: raw([[0, 2, 0, 0, 0, 0], [0, 0, -1, 0, 0, 0]]), "density key 1 .*must be 0, 1 or 2")
    refused(lambda: raw([[0, 0, 0, 0, 0, 0]]), "keeps no leg")
    refused(lambda: raw([[1, 0, 0, 0, 0, 0]] * 65), "65 density keys.*at most 64")
    refused(lambda: bt.densities([(0,)] * 65), "at most 64")
    refused(lambda: bt.densities([(1, 1, 1)]), r"\(1, 1, 1\)")
    refused(lambda: bt.densities([()]), r"\(\)")
    refused(lambda: bt.densities([]), "no key")
    # three two-leg sites at d = 4, D = 32: 256 open legs reach a 32 x 16 site
    refused(lambda: bt.densities([(2, 2), (1, 1, 2, 2, 3, 3)]), "density key 1 .*256 open legs reach site 3.*at most 65536")
    refused(lambda: bt.densities([(3, 3, 4, 4, 5, 5)] * 20), "density key 16 .*more than 65536 elements per replica")  # 4096 each
    refused(lambda: bt.densities([(0, 1)], weights=[0.5, 0.25, 0.25]), "weights")
    refused(lambda: bt.propagate(dt, 3, observe=dict(norm=False, keys=[(0, 1)]), every=2), "multiple of every")
    # what the one-site entry points refuse they still refuse, in the same words
    refused(lambda: bt.observe(norm=False), "nothing to observe")
    bt.sweep(dt, True)  # the centre is at the last site now
    refused(lambda: bt.densities([(1, 1, 2, 2)]), "centre")
    bt.sweep(dt, False)
    o = _against_engines(bt, [(2, 2, 3, 3)], "a pair at d = 4, D = 32 (16 x 1024 elements of transfer blocks)")
    assert o["density"][0].shape == (2, d, d, d, d)
    bt.close()


KEYS = [(0, 0, 1, 1), (0, 0, 2, 2), (0, 2)]


def test_the_reference_trajectory_case_with_pair_densities():
    """The four starts of the reference's trajectory case through propagate_trajectories(densities=...) against the dense
    solution traced to the key (helpers/key_density.py).  Bars: first record 1e-12; last record 4e-11, ten times the
    3.9e-12 the NumPy oracle has there (tests/test_batch_density_host.py) -- the error is the integrator's, shared by both
    paths, the factor covers the different rounding of the device products; each trajectory against a serial engine 1e-9."""
    from helpers import key_density as kd
    from helpers import spin_bath as sb
    from pytdscf_amd import Exciton, Model, TDVPEngine, propagate_trajectories, units
    from pytdscf_amd.mps import product_state_cores

    case = sb.case_trajectories()
    L = len(case["dims"])
    model = Model([Exciton(nstate=d) for d in case["dims"]], operators={"hamiltonian": case["mpo"]}, bond_dim=64)
    out = propagate_trajectories(model, case["starts"], maxstep=sb.NSTEPS, stepsize=sb.DT * units.au_in_fs,
                                 reduced_density=([(1, 1)], 1), densities=KEYS, integrator="arnoldi", conserve_norm=False,
                                 per_trajectory=True)
    exact = kd.exact_trajectory_densities(KEYS + [(1, 1)])
    assert np.allclose(out["time"], np.arange(sb.NSTEPS) * sb.DT * units.au_in_fs)
    for key in KEYS + [(1, 1)]:
        mean = out["mean"][key]
        assert mean.shape == exact[key].shape
        err0, err = np.abs(mean[0] - exact[key][0]).max(), np.abs(mean[-1] - exact[key][-1]).max()
        print(f"front end key {key}: max |mean density - dense| first {err0:.2e} last {err:.2e}")
        assert err0 < 1e-12 and err < 4e-11, (key, err0, err)
    only = propagate_trajectories(model, case["starts"], maxstep=3, stepsize=sb.DT * units.au_in_fs, reduced_density=([], 1),
                                  densities=KEYS[:1], integrator="arnoldi", conserve_norm=False)
    assert set(only["mean"]) == {KEYS[0]} and np.array_equal(only["mean"][KEYS[0]], out["mean"][KEYS[0]][:3])
    worst = 0.0
    for r, start in enumerate(case["starts"]):
        e = TDVPEngine(L, integrator="arnoldi", conserve_norm=False)
        e.set_mpo(case["mpo"])
        e.set_mps(product_state_cores(start, 64, space="hilbert"), canonicalize=True, scale=1.0)
        for q in range(sb.NSTEPS):
            for key in KEYS:
                worst = max(worst, np.abs(out["trajectories"][key][q, r] - e.reduced_density(kd.legs_of(key, L))).max())
            e.propagate(sb.DT)
        e.close()
    print(f"front end: worst |trajectory density - serial engine| {worst:.2e}")
    assert worst < 1e-9


def test_with_a_jump_channel_against_the_oracle_on_the_same_numbers():
    """the model, channels, seed and NumPy trajectories of test_gpu_batch_jump.py::test_parity_with_the_oracle_on_the_same_numbers"""
    import test_gpu_batch_jump as tj
    from helpers import key_density as kd
    from oracle import tdvp_oracle as orc

    mpo, jumps, gates, starts = tj._setup()
    ref = tj._reference("lanczos")
    keys = [(0, 0, 2, 2), (1, 3, 3), (2, 4)]
    L = len(tj.DIMS)
    bt = tj._batch(tj.NREP, starts, "lanczos")
    bt.set_gates(gates)
    bt.set_jumps(jumps, seed=tj.SEED)
    rec = bt.propagate(tj.DT, tj.NSTEPS, observe=dict(norm=False, keys=keys), every=tj.NSTEPS)
    assert bt.statuses == [0] * tj.NREP
    worst = np.zeros(2)
    for r in range(tj.NREP):
        for k, key in enumerate(keys):
            legs = kd.legs_of(key, L)
            first = np.abs(rec["density"][k][0, r] - orc.reduced_density(starts[r], legs)).max()
            last = np.abs(rec["density"][k][1, r] - orc.reduced_density(ref[r][0], legs)).max()
            worst = np.maximum(worst, [first, last])
            assert first < 1e-9 and last < 1e-9, (r, key, first, last)
    print(f"jump trajectories: worst |density - oracle| before {worst[0]:.2e} after {tj.NSTEPS} steps {worst[1]:.2e}")
    bt.close()
