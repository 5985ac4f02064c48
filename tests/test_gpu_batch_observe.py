"""GPU: batched observables (TDVPBatch.observe / propagate(observe=...), mitdvp_batch_observe / mitdvp_batch_run:
k_batch_observe observes every replica with one launch, k_batch_mean averages on the device) and the trajectory front end.
Every comparison is against the engines' own observables on the same state at the project's bars: norm 1e-12, site RDM
1e-9, energy and autocorrelation 1e-8 (README); the observed defects are printed."""

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


def _against_engines(bt, sites, label, which=None, weights=None):
    """one batched observation against every (or the picked) engine's own observables on the same state"""
    o = bt.observe(sites=sites, weights=weights, **ALL)
    worst = np.zeros(4)
    for r in (range(len(bt)) if which is None else which):
        e = bt[r]
        dn = abs(o["norm"][r] - e.norm())
        da = abs(o["autocorr"][r] - e.autocorr())
        de = abs(o["energy"][r] - e.expectation(0))
        dr = max(np.abs(o["rdm"][k][r] - e.site_rdm(p)).max() for k, p in enumerate(sites))
        worst = np.maximum(worst, [dn, dr, de, da])
        assert dn < 1e-12 and dr < 1e-9 and de < 1e-8 and da < 1e-8, (label, r, dn, dr, de, da)
    print(f"{label}: worst defects norm {worst[0]:.2e} rdm {worst[1]:.2e} energy {worst[2]:.2e} autocorr {worst[3]:.2e}")
    return o


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for x, y in zip(xs, ys):
            assert np.array_equal(x, y), k


@pytest.mark.parametrize("integrator, cn", [("lanczos", True), ("arnoldi", False)])
def test_parity_with_the_engines_own_observables(integrator, cn):
    from pytdscf_amd import synthetic as syn

    L, d, D, M, B, dt = 5, 3, 7, 5, 3, 0.4
    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    if not cn:
        mpo = _nonhermitian(mpo)
    bt = _batch(B, mpo, [d] * L, D, [11, 12, 13], integrator=integrator, conserve_norm=cn)
    _against_engines(bt, [0, 2, 4], f"{integrator} before any step")  # the right blocks are not built yet
    bt.propagate(dt, 2)
    o = _against_engines(bt, [0, 2, 4], f"{integrator} after two steps")
    if cn:
        assert np.abs(o["norm"] - 1).max() < 1e-12
    else:
        assert np.abs(o["norm"] - 1).max() > 1e-6  # the non-Hermitian operator moved the norm
    # the means are those of the per-replica output
    for name, per in (("mean_norm2", o["norm"] ** 2), ("mean_autocorr", o["autocorr"]), ("mean_energy", o["energy"])):
        assert abs(o[name] - per.mean()) < 1e-13 * max(1, abs(per).max()), name
    for k in range(3):
        assert np.abs(o["mean_rdm"][k] - o["rdm"][k].mean(axis=0)).max() < 1e-13
    bt.close()


@pytest.mark.parametrize("dims, D, sites", [([3, 3], 3, [0, 1]), ([2, 3, 2], 4, [0, 1, 2]), ([8, 8, 8, 8], 3, [1, 3]), ([5], 1, [0]),
                                            ([2] * 14, 64, [7, 13])])
def test_awkward_shapes(dims, D, sites):
    """tiles that are no multiple of 16 or 32, mixed physical dimensions, d^2 = 64 outputs with a short K, a one-site
    chain (nothing in mitdvp_batch_create's checks refuses one), and the envelope corner 64 x 2 x 64 = 8192 with a middle and the last site"""
    from helpers import spin_bath as sb
    from pytdscf_amd import synthetic as syn

    L = len(dims)
    kw = {}
    if dims == [2, 3, 2]:
        mpo, kw = sb.sop_mpo(sb.hilbert_terms(0, 1, 2), dims), dict(integrator="arnoldi", conserve_norm=False)
    else:
        mpo = syn.synthetic_mpo(L, dims[0], 3 if L > 4 else 4, seed=2)
    bt = _batch(2, mpo, dims, D, [5, 6], **kw)
    _against_engines(bt, sites, f"{dims[:4]} D={D} before a step")
    bt.propagate(0.1, 1)
    _against_engines(bt, sites, f"{dims[:4]} D={D} after a step")
    bt.close()


def test_a_replicas_record_does_not_depend_on_the_batch():
    from pytdscf_amd import synthetic as syn

    L, d, D, M, dt = 5, 3, 7, 4, 0.4
    mpo = syn.synthetic_mpo(L, d, M, seed=1)
    seeds = [60 + r for r in range(9)]
    big = _batch(9, mpo, [d] * L, D, seeds)
    one = _batch(1, mpo, [d] * L, D, [seeds[4]])
    big.propagate(dt, 1)
    one.propagate(dt, 1)
    a = big.observe(sites=[1, 4], **ALL)
    b = one.observe(sites=[1, 4], **ALL)
    for k in ("norm", "autocorr", "energy"):
        assert np.array_equal(a[k][4:5], b[k]), k
    for x, y in zip(a["rdm"], b["rdm"]):
        assert np.array_equal(x[4:5], y)
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
    o = _against_engines(bt, [0, 2, 3], "B = 300", which=(0, 149, 299), weights=w)
    eps = B * 2.0 ** -52  # the rounding of a length-B sum of terms bounded by max |record| (sum w = 1)
    pairs = [("mean_norm2", o["norm"] ** 2), ("mean_autocorr", o["autocorr"]), ("mean_energy", o["energy"])]
    pairs += [(k, o["rdm"][k]) for k in range(3)]
    for name, per in pairs:
        got = o["mean_rdm"][name] if isinstance(name, int) else o[name]
        ref = np.tensordot(w, per, axes=(0, 0))
        defect, bound = np.abs(got - ref).max(), eps * np.abs(per).max()
        print(f"device mean {name}: defect {defect:.2e} bound {bound:.2e}")
        assert defect <= bound, (name, defect, bound)
    bt.close()


def test_a_recorded_run_equals_observing_by_hand():
    from pytdscf_amd import synthetic as syn

    L, d, D, M, B, dt = 5, 3, 7, 4, 3, 0.3
    mpo = syn.synthetic_mpo(L, d, M, seed=2)
    seeds = [71, 72, 73]
    a = _batch(B, mpo, [d] * L, D, seeds)
    b = _batch(B, mpo, [d] * L, D, seeds)
    for bt in (a, b):
        bt.propagate(dt, 1)  # the engines build their right blocks with their own launches, once
    for e in a.engines:
        e.counters_reset()
    req = dict(sites=[0, 3, 4], **ALL)
    rec = a.propagate(dt, 4, observe=req, every=2)
    nl = a[0].counters()["n_launch"]
    print(f"recorded run: {nl} launches for 4 steps and 3 records")
    assert nl <= 2 * 4 + 2 * 3 and a[1].counters()["n_launch"] == 0
    assert rec["norm"].shape == (3, B) and rec["rdm"][1].shape == (3, B, d, d) and rec["mean_rdm"][2].shape == (3, d, d)
    hand = [b.observe(**req)]
    for _ in range(2):
        assert b.propagate(dt, 2) is None
        hand.append(b.observe(**req))
    for q in range(3):
        _same({k: ([x[q] for x in v] if isinstance(v, list) else v[q]) for k, v in rec.items()}, hand[q])
    a.close()
    b.close()


def test_the_reference_trajectory_case_through_the_front_end():
    """the four starts of the reference's trajectory case (tests/test_mixedstate.py:239-318) through
    propagate_trajectories; bars of test_gpu_batch.py::test_trajectory_average_against_the_dense_solution"""
    from helpers import spin_bath as sb
    from pytdscf_amd import Exciton, Model, TDVPEngine, propagate_trajectories, units
    from pytdscf_amd.mps import product_state_cores

    case = sb.case_trajectories()
    key = case["key"]
    model = Model([Exciton(nstate=d) for d in case["dims"]], operators={"hamiltonian": case["mpo"]}, bond_dim=64)
    out = propagate_trajectories(model, case["starts"], maxstep=sb.NSTEPS, stepsize=sb.DT * units.au_in_fs,
                                 reduced_density=([key], 1), integrator="arnoldi", conserve_norm=False, per_trajectory=True)
    exact = sb.exact_rdms(**case["exact"])
    mean = out["mean"][key]
    assert mean.shape == (sb.NSTEPS, 3, 3) and np.allclose(out["time"], np.arange(sb.NSTEPS) * sb.DT * units.au_in_fs)
    err0, err = np.abs(mean[0] - exact[0]).max(), np.abs(mean[-1] - exact[sb.NSTEPS - 1]).max()
    print(f"front end: max |mean rdm - exact| first {err0:.2e} last {err:.2e}")
    assert err0 < 1e-12 and err < 1e-11
    legs = sb.legs_of(key, len(case["dims"]))
    worst = 0.0
    for r, start in enumerate(case["starts"]):
        e = TDVPEngine(len(case["dims"]), integrator="arnoldi", conserve_norm=False)
        e.set_mpo(case["mpo"])
        e.set_mps(product_state_cores(start, 64, space="hilbert"), canonicalize=True, scale=1.0)
        for q in range(sb.NSTEPS):
            worst = max(worst, np.abs(out["trajectories"][key][q, r] - e.reduced_density(legs)).max())
            e.propagate(sb.DT)
        e.close()
    print(f"front end: worst |trajectory rdm - serial engine| {worst:.2e}")
    assert worst < 1e-9


def test_refusals_leave_the_engines_untouched():
    from pytdscf_amd import synthetic as syn

    L, d, D, M, dt = 4, 3, 6, 3, 0.1
    bt = _batch(2, syn.synthetic_mpo(L, d, M, seed=0), [d] * L, D, [1, 2])

    def refused(call, match):
        before = [e.get_mps() for e in bt.engines]
        with pytest.raises(ValueError, match=match):
            call()
        for e, b in zip(bt.engines, before):
            for x, y in zip(e.get_mps(), b):
                assert np.array_equal(x, y)

    refused(lambda: bt.observe(sites=[L]), "out of range")
    refused(lambda: bt.observe(sites=[1, 1]), "ascending")
    refused(lambda: bt.observe(sites=[2, 1]), "ascending")
    refused(lambda: bt.observe(norm=False), "nothing to observe")
    refused(lambda: bt.observe(sites=[1], weights=[0.5, 0.25, 0.25]), "weights")
    refused(lambda: bt.propagate(dt, 3, observe=dict(sites=[1]), every=2), "multiple of every")
    bt.sweep(dt, True)  # the centre is at the last site now
    refused(lambda: bt.observe(sites=[1]), "centre")
    bt.sweep(dt, False)
    assert bt.observe(sites=[1])["rdm"][0].shape == (2, d, d)
    bt.close()


def test_a_replica_that_does_not_converge_is_recorded_as_zeros():
    """the set-up of test_gpu_batch.py::test_a_replica_that_does_not_converge, run once"""
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

    req = dict(sites=[0, 2], **ALL)
    engs = engines((0, 1, 2))
    bt = TDVPBatch.from_engines(engs)
    with pytest.raises(ValueError, match="Short Iterative Lanczos is not converged"):
        bt.propagate(dt, 2, observe=req, every=1)
    assert bt.statuses[1] == _lib.ENOTCONV and bt.statuses[0] == 0 and bt.statuses[2] == 0
    rec = bt.records
    assert rec["norm"].shape == (3, 3) and abs(rec["norm"][0, 1] - 1) < 1e-12  # observed before it failed
    for k in ("norm", "autocorr", "energy"):
        assert np.all(rec[k][1:, 1] == 0), k
    for x in rec["rdm"]:
        assert np.all(x[1:, 1] == 0) and np.abs(x[0, 1]).max() > 0
    good = engines((0, 2))
    ok = TDVPBatch.from_engines(good)
    ref = ok.propagate(dt, 2, observe=req, every=1)
    for k in ("norm", "autocorr", "energy"):
        assert np.array_equal(rec[k][:, [0, 2]], ref[k]), k
    for x, y in zip(rec["rdm"], ref["rdm"]):
        assert np.array_equal(x[:, [0, 2]], y)
    bt.close()
    ok.close()
    for e in engs + good:
        e.close()
