"""GPU: batched trajectories (TDVPBatch / mitdvp_batch_*: one workgroup of k_batch_sweep owns one replica, one launch per
half-sweep for the whole batch).  Every property is checked against the same engines stepped one at a time through the
general multi-launch path (TDVPEngine.propagate, small kernels off), at the project's own bars: final-state fidelity
| |<a|b>| - 1 | < 1e-10 (test_gpu_ensemble.py, between differently chunked paths), norm to 1e-12, equal krylov_stats(),
1e-8 on the energy and 1e-9 on a site RDM (README)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _serial(L, mpo, dims, D, seed, nsteps, dt, shift=0.0, **kw):
    from pytdscf_amd import TDVPEngine

    e = TDVPEngine(L, **kw)
    e.set_small_kernels(False)
    e.set_mpo(mpo, shift=shift)
    e.init_random(dims, D, seed=seed)
    for _ in range(nsteps):
        e.propagate(dt)
    return e


def _fid(a, b):
    """| |<a|b>| / (|a| |b|) - 1 |, and the two norms agree to 1e-12 (states under a non-Hermitian operator without
    conserve_norm are not normalised)"""
    from oracle import tdvp_oracle as orc

    na, nb = np.sqrt(abs(orc.overlap(a, a))), np.sqrt(abs(orc.overlap(b, b)))
    assert abs(na - nb) < 1e-12, (na, nb)
    return abs(abs(orc.overlap(a, b)) / (na * nb) - 1)


def _batch(B, L, mpo, dims, D, seeds, **kw):
    from pytdscf_amd import TDVPBatch

    bt = TDVPBatch(B, L, **kw)
    bt.set_mpo(mpo)
    for e, s in zip(bt.engines, seeds):
        e.init_random(dims, D, seed=s)
    return bt


def _same_state(a, b, what):
    """the bar between two paths to one state (module docstring)"""
    f = _fid(a, b)
    print(f"{what}: fidelity defect {f:.2e}")
    assert f < 1e-10, (what, f)


def _against_serial(bt, mpos, dims, D, seeds, nsteps, dt, which=None, **kw):
    L = len(dims)
    for r in (range(len(bt)) if which is None else which):
        ser = _serial(L, mpos[r] if isinstance(mpos, dict) else mpos, dims, D, seeds[r], nsteps, dt, **kw)
        _same_state(ser.get_mps(), bt[r].get_mps(), f"replica {r}, krylov {bt[r].krylov_stats()}")
        assert ser.krylov_stats() == bt[r].krylov_stats(), r
        ser.close()


@pytest.mark.parametrize("integrator, cn", [("lanczos", True), ("arnoldi", False)])
def test_parity_with_engines_stepped_one_at_a_time(integrator, cn):
    from pytdscf_amd import synthetic as syn

    L, d, D, M, B, nsteps, dt = 6, 4, 16, 6, 5, 3, 0.5
    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    seeds = [11 + r for r in range(B)]
    kw = dict(integrator=integrator, conserve_norm=cn)
    bt = _batch(B, L, mpo, [d] * L, D, seeds, **kw)
    bt.propagate(dt, 1)  # builds the right environments with the engines' own launches, once
    for e in bt.engines:
        e.counters_reset()
    bt.propagate(dt, nsteps - 1)
    assert bt.statuses == [0] * B
    c0 = bt[0].counters()
    assert c0["n_launch"] == 2 * (nsteps - 1)  # two launches per time step, whatever B and L
    assert bt[1].counters()["n_launch"] == 0
    assert c0["n_exp_site"] == 2 * (nsteps - 1) * L and c0["n_exp_bond"] == 2 * (nsteps - 1) * (L - 1)
    for r in range(B):
        ser = _serial(L, mpo, [d] * L, D, seeds[r], nsteps, dt, **kw)
        f = _fid(ser.get_mps(), bt[r].get_mps())
        de = abs(ser.expectation(0) - bt[r].expectation(0))
        dn = abs(ser.norm() - bt[r].norm())
        drdm = np.abs(ser.site_rdm(2) - bt[r].site_rdm(2)).max()
        print(f"{integrator} replica {r}: fidelity {f:.2e} energy {de:.2e} norm {dn:.2e} rdm {drdm:.2e}")
        assert f < 1e-10 and de < 1e-8 and dn < 1e-12 and drdm < 1e-9
        if cn:
            assert abs(bt[r].norm() - 1) < 1e-12
        assert ser.krylov_stats() == bt[r].krylov_stats()
        ser.close()
    bt.close()


@pytest.mark.parametrize("dims, D, M", [([3, 3], 3, 4), ([3] * 5, 7, 5), ([8, 8, 8, 8], 3, 4)])
def test_awkward_shapes(dims, D, M):
    """tiles that are no multiple of 4 or 16, ends with bond 1, a physical index wider than the bond"""
    from pytdscf_amd import synthetic as syn

    L = len(dims)
    mpo = syn.synthetic_mpo(L, dims[0], M, seed=2)
    seeds = [5, 6]
    bt = _batch(2, L, mpo, dims, D, seeds)
    bt.propagate(0.3, 2)
    _against_serial(bt, mpo, dims, D, seeds, 2, 0.3)
    bt.close()


def test_awkward_shapes_mixed_physical_dimensions():
    from helpers import spin_bath as sb

    dims = [2, 3, 2]
    mpo = sb.sop_mpo(sb.hilbert_terms(0, 1, 2), dims)
    seeds = [5, 6]
    bt = _batch(2, 3, mpo, dims, 4, seeds, integrator="arnoldi", conserve_norm=False)
    bt.propagate(0.1, 2)
    _against_serial(bt, mpo, dims, 4, seeds, 2, 0.1, integrator="arnoldi", conserve_norm=False)
    bt.close()


def test_two_replicas_against_the_oracle():
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import synthetic as syn

    L, d, D, M, nsteps, dt = 6, 3, 8, 4, 2, 0.4
    mpo = syn.synthetic_mpo(L, d, M, seed=1)
    seeds = [21, 22]
    bt = _batch(2, L, mpo, [d] * L, D, seeds)
    start = [e.get_mps() for e in bt.engines]
    bt.propagate(dt, nsteps)
    for r in range(2):
        st = orc.OracleMPS(start[r], mpo)
        for _ in range(nsteps):
            st.propagate(dt)
        f = _fid(st.cores, bt[r].get_mps())
        print(f"replica {r} against the oracle: fidelity defect {f:.2e}")
        assert f < 1e-10
    bt.close()


def test_more_replicas_than_the_chip_has_compute_units():
    from pytdscf_amd import synthetic as syn

    L, d, D, M, dt = 4, 2, 4, 3, 0.5
    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    B = 300
    seeds = [100 + r for r in range(B)]
    big = _batch(B, L, mpo, [d] * L, D, seeds)
    big.propagate(dt)
    assert big.statuses == [0] * B
    pick = (0, 149, 299)
    _against_serial(big, mpo, [d] * L, D, seeds, 1, dt, which=pick)
    small = _batch(3, L, mpo, [d] * L, D, [seeds[r] for r in pick])
    small.propagate(dt)
    for k, r in enumerate(pick):  # fixed-order reductions, no cross-replica state: the same bits whatever B
        for a, b in zip(big[r].get_mps(), small[k].get_mps()):
            assert np.array_equal(a, b), r
    big.close()
    small.close()


def test_per_replica_mpos():
    from pytdscf_amd import TDVPBatch, TDVPEngine
    from pytdscf_amd import synthetic as syn

    L, d, D, M, B, dt = 5, 3, 8, 4, 4, 0.4
    mpos = {r: syn.synthetic_mpo(L, d, M, seed=r) for r in range(B)}
    engs = []
    for r in range(B):
        e = TDVPEngine(L)
        e.set_mpo(mpos[r])
        e.init_random([d] * L, D, seed=40 + r)
        engs.append(e)
    bt = TDVPBatch.from_engines(engs)
    bt.propagate(dt, 2)
    _against_serial(bt, mpos, [d] * L, D, [40 + r for r in range(B)], 2, dt)
    bt.close()
    assert engs[0].norm() > 0  # from_engines leaves the engines open
    for e in engs:
        e.close()


def test_imaginary_time():
    from pytdscf_amd import synthetic as syn

    L, d, D, M, B, dt = 5, 3, 8, 4, 3, 0.2
    mpo = syn.synthetic_mpo(L, d, M, seed=3)
    seeds = [7, 8, 9]
    bt = _batch(B, L, mpo, [d] * L, D, seeds, relax=True)
    bt.propagate(dt, 3)
    for r in range(B):
        ser = _serial(L, mpo, [d] * L, D, seeds[r], 3, dt, relax=True)
        de = abs(ser.expectation(0) - bt[r].expectation(0))
        print(f"replica {r}: energy difference {de:.2e}")
        assert de < 1e-10
        ser.close()
    bt.close()


def test_trajectory_average_against_the_dense_solution():
    """the four starts of the reference's trajectory case (tests/test_mixedstate.py:239-318) as ONE batch; observables
    before the step, as the reference's loop takes them"""
    from helpers import spin_bath as sb
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import TDVPBatch
    from pytdscf_amd.mps import product_state_cores

    case = sb.case_trajectories()
    L = len(case["dims"])
    bt = TDVPBatch(len(case["starts"]), L, integrator="arnoldi", conserve_norm=False)
    bt.set_mpo(case["mpo"])
    for e, start in zip(bt.engines, case["starts"]):
        e.set_mps(orc.canonicalize_site0(product_state_cores(start, 64, space="hilbert"), scale=1.0))
    legs = sb.legs_of(case["key"], L)
    out = []
    for _ in range(sb.NSTEPS):
        out.append(sum(sb.system_rdm(e.reduced_density(legs), case) for e in bt.engines) / len(bt))
        bt.propagate(sb.DT)
    exact = sb.exact_rdms(**case["exact"])
    err0 = np.abs(out[0] - exact[0]).max()
    err = np.abs(out[-1] - exact[sb.NSTEPS - 1]).max()
    print(f"trajectory average: max |rdm - exact| first {err0:.2e} last {err:.2e}")
    assert err0 < 1e-12 and err < 1e-11
    bt.close()


def test_interleaving_with_ordinary_propagation():
    from pytdscf_amd import synthetic as syn

    L, d, D, M, dt = 5, 3, 8, 4, 0.4
    mpo = syn.synthetic_mpo(L, d, M, seed=4)
    seeds = [31, 32, 33]
    bt = _batch(3, L, mpo, [d] * L, D, seeds)
    bt.propagate(dt)
    bt[1].propagate(dt)
    bt.propagate(dt)
    for r, n in ((0, 2), (1, 3), (2, 2)):
        ser = _serial(L, mpo, [d] * L, D, seeds[r], n, dt)
        f = _fid(ser.get_mps(), bt[r].get_mps())
        print(f"replica {r} after {n} steps: fidelity defect {f:.2e}")
        assert f < 1e-10
        ser.close()
    bt.close()


def _refused(engs, match=None):
    from pytdscf_amd import TDVPBatch

    before = [e.get_mps() for e in engs]
    bt = TDVPBatch.from_engines(engs)
    with pytest.raises(ValueError) as ei:
        bt.propagate(0.1)
    assert str(ei.value).strip()
    if match:
        assert match in str(ei.value), str(ei.value)
    for e, b in zip(engs, before):
        for x, y in zip(e.get_mps(), b):
            assert np.array_equal(x, y)
    bt.close()


def _eng(L, d, D, M, seed, mpo_seed=0, **kw):
    from pytdscf_amd import TDVPEngine
    from pytdscf_amd import synthetic as syn

    e = TDVPEngine(L, **kw)
    e.set_mpo(syn.synthetic_mpo(L, d, M, seed=mpo_seed))
    e.init_random([d] * L, D, seed=seed)
    return e


def test_refusals():
    L, d = 4, 3
    cases = {
        "bond": lambda: [_eng(L, d, 6, 3, 1), _eng(L, d, 5, 3, 2)],
        "MPO": lambda: [_eng(L, d, 6, 3, 1), _eng(L, d, 6, 4, 2)],
        "adaptive": None,
        "compute-unit": lambda: [_eng(L, d, 6, 3, 1), _eng(L, d, 6, 3, 2, cu_range=(0, 64))],
        "thresh": lambda: [_eng(L, d, 6, 3, 1), _eng(L, d, 6, 3, 2, thresh=1e-8)],
        "envelope": lambda: [_eng(6, 10, 32, 3, 1), _eng(6, 10, 32, 3, 2)],  # (32, 10, 32) = 10240 elements in the middle
    }
    for name, make in cases.items():
        if make is None:
            engs = [_eng(L, d, 6, 3, 1), _eng(L, d, 6, 3, 2)]
            engs[1].set_adaptive(True, Dmax=8, dD=1)
        else:
            engs = make()
        _refused(engs, {"bond": "shape of site", "MPO": "MPO bonds", "adaptive": "adaptive", "compute-unit": "compute-unit",
                        "thresh": "thresh", "envelope": "at most"}[name])
        for e in engs:
            e.close()
    e = _eng(L, d, 6, 3, 1)
    _refused([e, e], "twice")
    e.close()


def test_a_replica_that_does_not_converge():
    from pytdscf_amd import TDVPBatch, TDVPEngine, _lib
    from pytdscf_amd import synthetic as syn

    L, d, D, M, dt = 4, 3, 6, 3, 0.02
    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    hot = [w.copy() for w in mpo]
    hot[0] = hot[0] * 1e3
    engs = []
    for r in range(3):
        e = TDVPEngine(L, max_krylov=8)
        e.set_mpo(hot if r == 1 else mpo)
        e.init_random([d] * L, D, seed=50 + r)
        engs.append(e)
    bt = TDVPBatch.from_engines(engs)
    with pytest.raises(ValueError, match="Short Iterative Lanczos is not converged"):
        bt.propagate(dt)
    assert bt.statuses[1] == _lib.ENOTCONV and bt.statuses[0] == 0 and bt.statuses[2] == 0
    # the failed replica's message is on its own handle, and it refuses further use until it is given its tensors again
    msg = _lib.load().mitdvp_last_error(engs[1]._h).decode()
    assert "Short Iterative Lanczos is not converged in 8 basis" in msg, msg
    with pytest.raises(ValueError):
        engs[1].propagate(dt)
    with pytest.raises(ValueError):
        bt.propagate(dt)
    engs[1].set_mpo(mpo)
    engs[1].init_random([d] * L, D, seed=51)
    for r in (0, 2):
        ser = _serial(L, mpo, [d] * L, D, 50 + r, 1, dt, max_krylov=8)
        assert _fid(ser.get_mps(), engs[r].get_mps()) < 1e-10
        assert ser.krylov_stats() == engs[r].krylov_stats()
        ser.close()
    bt.close()
    for e in engs:
        e.close()
