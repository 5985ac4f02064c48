"""GPU: an MPO applied to the replicas of a batch (TDVPBatch.operate, mitdvp_batch_operate: k_batch_operate fits
phi ~ O|psi> / |O|psi>| for every selected replica in ONE launch, one workgroup per replica) and
trajectories.correlation_function with starts given as MPS cores.

The pins are the reference's own result (tests/golden/operate_chain.npz) and oracle.tdvp_oracle.operate.  bt_qr is
gauge-free and the fitted state, as a vector, depends on neither the QR phases nor a global phase, so everything is compared
as DENSE states: |phi_got - phi_pin|_2 <= 1e-9 (both normalised) and the norm within 1e-10 relative -- the bars of
tests/test_gpu_operate.py restated gauge-free (helpers/operate_cases).  tests/test_batch_operate_host.py shows on the CPU
that the bars have room: a 1e-13 relative perturbation of the inputs moves the oracle's result by less than a tenth of them
for every case used here.  The shapes are those of the spectra tests, the smallest at which each part can go wrong:
  mixed  dims (2, 3, 2, 4, 2), D = 6: ragged physical dimensions, a bond narrower than the tile
  odd    dims (3,) * 5, D = 7: every size odd, a multiple of no tile
  wide   dims (2,) * 12, D = 40: bonds past the 32-wide tile and the 16-deep K step, more than one tile per product
and per shape the five operators of helpers/expect_cases (MPO bonds 1 to 8, one non-Hermitian with a complex shift, and
operator 0 with its shift of 0.1)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = 0.2
PSI, GB, GC = 0, 2, -1  # the gauge codes Psi, B and C (no gauge) of get_site_shape


def _give(e, name):
    from helpers import expect_cases as ec

    for label in ec.LABELS:
        _, shift, mpo = ec.case(name, label)
        e.set_mpo(mpo, ec.OP_ID[label], shift=shift)


def _batch(name, states, **kw):
    from helpers import operate_cases as oc
    from pytdscf_amd import TDVPBatch

    dims, _ = oc.SHAPES[name]
    kw = dict(dict(integrator="arnoldi", conserve_norm=False), **kw)
    bt = TDVPBatch(len(states), len(dims), **kw)
    for e, cores in zip(bt.engines, states):
        _give(e, name)
        e.set_mps(cores)
    return bt


def _golden_batch(nrep):
    from helpers import operate_cases as oc
    from pytdscf_amd import TDVPBatch

    mpo, start, _ = oc.golden()
    bt = TDVPBatch(nrep, len(mpo))
    for e in bt.engines:
        e.set_mpo(mpo)
        e.set_mps(start)
    return bt


def _tensors(bt):
    return [e.get_mps() for e in bt.engines]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _gauges(e):
    return [e.get_site_shape(i)[3] for i in range(e.nsite)]


def _dense(cores):
    from helpers import jump_oracle as jo

    return jo.dense_state(cores)


@pytest.mark.parametrize("maxstep", [1, 10])
def test_golden(maxstep):
    """B = 3 replicas holding the fixture's start and MPO: the reference's own norm and state, iterations == maxstep at the
    default tolerance, the three replicas bitwise equal, one launch, gauges Psi B B ..."""
    from helpers import operate_cases as oc

    _, _, res = oc.golden()
    ref_norm, ref_state = res[maxstep]
    bt = _golden_batch(3)
    bt.observe()  # the handle exists and the launches are counted from here
    n0 = bt.launches()
    got = bt.operate(0, maxstep=maxstep)
    assert bt.launches() == n0 + 1
    assert list(got["iterations"]) == [maxstep] * 3 and got["statuses"] == [0, 0, 0]
    ts = _tensors(bt)
    for r in range(3):
        dn = abs(got["norms"][r] - ref_norm) / (oc.BAR_NORM * ref_norm)
        ds = oc.state_defect(_dense(ts[r]), ref_state) / oc.BAR_STATE
        print(f"golden maxstep {maxstep} replica {r}: norm defect {dn:.3e} of its bar, state defect {ds:.3e} of its bar")
        assert dn < 1 and ds < 1
        assert _gauges(bt.engines[r]) == [PSI] + [GB] * (len(ts[r]) - 1)
        assert abs(bt.engines[r].norm() - 1) < 1e-12
    assert _same(ts[0], ts[1]) and _same(ts[0], ts[2])
    bt.close()


@pytest.mark.parametrize("name", ["mixed", "odd", "wide"])
def test_shapes_and_operators_against_the_oracle(name):
    """the five operators on three states of norms 0.7 / 0.9 / 1.1, maxstep = 2, conv_tol = 0"""
    from helpers import expect_cases as ec
    from helpers import operate_cases as oc

    worst = 0.0
    for label in oc.LABELS:
        bt = _batch(name, oc.states(name))
        got = bt.operate(ec.OP_ID[label], maxstep=oc.MAXSTEP, conv_tol=0.0)
        ts = _tensors(bt)
        for r in range(oc.NSTATES):
            nrm, pin, it = oc.oracle_case(name, label, r)
            assert got["iterations"][r] == it == oc.MAXSTEP
            dn = abs(got["norms"][r] - nrm) / (oc.BAR_NORM * nrm)
            ds = oc.state_defect(_dense(ts[r]), pin) / oc.BAR_STATE
            worst = max(worst, dn, ds)
        bt.close()
    print(f"{name}: worst defect against the oracle = {worst:.3e} of its bar (state 1e-9, norm 1e-10 relative)")
    assert worst < 1


def test_selection_and_batch_size_independence():
    """replicas=[2, 0] leaves replica 1 bitwise alone and gives 0 and 2 the bits of the all-replica call; a state's result
    in a batch of 300 is bitwise its result in a batch of 3"""
    from helpers import expect_cases as ec
    from helpers import operate_cases as oc

    name, k = "mixed", ec.OP_ID["local"]
    st = oc.states(name)
    full = _batch(name, st)
    rf = full.operate(k, maxstep=2, conv_tol=0.0)
    tf = _tensors(full)
    full.close()
    part = _batch(name, st)
    before = _tensors(part)
    rp = part.operate(k, maxstep=2, conv_tol=0.0, replicas=[2, 0])
    tp = _tensors(part)
    assert _same(tp[1], before[1]) and not _same(tp[0], before[0])
    assert _same(tp[0], tf[0]) and _same(tp[2], tf[2])
    assert rp["norms"][0] == rf["norms"][0] and rp["norms"][2] == rf["norms"][2] and rp["norms"][1] == 0.0
    assert list(rp["iterations"]) == [2, 0, 2]
    assert _gauges(part.engines[1]) == [PSI] + [GB] * 4
    part.close()
    nbig = 300
    many = [st[1]] * nbig
    many[0], many[149], many[299] = st[0], st[1], st[2]
    big = _batch(name, many)
    rb = big.operate(k, maxstep=2, conv_tol=0.0)
    for i, r in ((0, 0), (149, 1), (299, 2)):
        assert _same(big.engines[i].get_mps(), tf[r]) and rb["norms"][i] == rf["norms"][r]
    big.close()


def test_every_replica_stops_on_its_own():
    """one call whose replicas stop at different sweeps, each at the oracle's count (the cases and their gaps:
    tests/test_batch_operate_host.py), and the golden case with its own tolerance"""
    from helpers import operate_cases as oc
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import TDVPBatch

    cases = oc.stop_cases()
    pair = [cases["mixed_local"], cases["mixed_product_padded"]]
    assert pair[0][3] == pair[1][3]  # one tolerance for the call
    bt = TDVPBatch(2, len(pair[0][0]))
    for e, (cores, mpo, shift, _, _) in zip(bt.engines, pair):
        e.set_mpo(mpo, shift=shift)
        e.set_mps(cores)
    got = bt.operate(0, maxstep=10, conv_tol=pair[0][3])
    for r, (cores, mpo, shift, tol, stop) in enumerate(pair):
        nrm, bra, it = orc.operate(cores, mpo, maxstep=10, conv_tol=tol, shift=shift)
        assert it == stop and got["iterations"][r] == stop
        assert abs(got["norms"][r] - nrm) < oc.BAR_NORM * nrm
        assert oc.state_defect(_dense(bt.engines[r].get_mps()), _dense(bra)) < oc.BAR_STATE
    bt.close()
    cores, mpo, shift, tol, stop = cases["golden"]
    bt = _golden_batch(1)
    assert bt.operate(0, maxstep=10, conv_tol=tol)["iterations"][0] == stop
    bt.close()


def test_bookkeeping_after_the_fit():
    """the state handed back is the state the observations see (stale blocks would show), a step keeps the norm, and a
    cross request, an expect request and a snapshot from before the call still give their values"""
    from helpers import cross_cases as cc
    from helpers import expect_cases as ec
    from helpers import operate_cases as oc

    name = "mixed"
    bt = _batch(name, oc.states(name))
    bt.propagate(DT, 1)  # blocks and Krylov memories exist
    bt.snapshot()
    old = _tensors(bt)
    ops = [ec.OP_ID["energy"], ec.OP_ID["local"], ec.OP_ID["complex"]]
    bt.set_expect(ops)
    bt.set_cross([(bt.snap(0), 1), (2, bt.snap(2))])
    bt.operate(ec.OP_ID["local"], maxstep=2, conv_tol=0.0)
    now = _tensors(bt)
    obs = bt.observe(energy=True)
    exp = bt.expect()
    for r in range(3):
        _, shift, mpo = ec.case(name, "energy")
        pin = ec.dense_value(now[r], mpo, shift)
        assert abs(obs["energy"][r] - pin) < 1e-12 * ec.scale(name, "energy") * ec.norm2(now[r])
        for j, label in enumerate(("energy", "local", "complex")):
            _, shift, mpo = ec.case(name, label)
            pin = ec.dense_value(now[r], mpo, shift)
            assert abs(exp["values"][r, j] - pin) < ec.BAR * ec.scale(name, label) * ec.norm2(now[r])
    cr = bt.cross()["values"]
    for v, (a, b) in zip(cr, ((old[0], now[1]), (now[2], old[2]))):
        assert abs(v - cc.walk(a, b)) < 1e-12 * cc.norm_of(a) * cc.norm_of(b)
    bt.propagate(DT, 1)
    for e in bt.engines:
        assert abs(e.norm() - 1) < 1e-12
    bt.close()


def test_against_the_engine_route():
    """TDVPEngine.operate on the same input: each is within 1e-9 of the oracle, so the two dense states are within 2e-9;
    the iteration counts are equal"""
    from helpers import expect_cases as ec
    from helpers import operate_cases as oc
    from pytdscf_amd import TDVPEngine

    name, label = "mixed", "complex"
    st = oc.states(name)
    bt = _batch(name, st)
    got = bt.operate(ec.OP_ID[label], maxstep=10, conv_tol=1e-8)
    for r in range(oc.NSTATES):
        eng = TDVPEngine(len(st[r]))
        _give(eng, name)
        eng.set_mps(st[r])
        nrm, iters = eng.operate(ec.OP_ID[label], maxstep=10, conv_tol=1e-8)
        assert iters == got["iterations"][r]
        assert abs(nrm - got["norms"][r]) < 2 * oc.BAR_NORM * nrm
        assert oc.state_defect(_dense(eng.get_mps()), _dense(bt.engines[r].get_mps())) < 2 * oc.BAR_STATE
        eng.close()
    bt.close()


def test_an_annihilated_replica_stops_and_the_others_finish():
    """replica 1 populates level 0 of site 0 only and the operator projects site 0 on level 1"""
    from helpers import operate_cases as oc
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import TDVPBatch

    dims, D = oc.SHAPES["odd"]
    st = [[c.copy() for c in s] for s in oc.states("odd")]
    st[1][0][:, 1:, :] = 0.0
    proj = np.zeros((dims[0], dims[0]))
    proj[1, 1] = 1.0
    rng = np.random.default_rng(9)
    mats = [proj] + [rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)) for d in dims[1:]]
    mpo = [m[None, :, :, None].astype(np.complex128) for m in mats]
    bt = TDVPBatch(3, len(dims))
    for e, cores in zip(bt.engines, st):
        e.set_mpo(mpo)
        e.set_mps(cores)
    with pytest.raises(Exception, match="annihilates the state of replica 1"):
        bt.operate(0, maxstep=2, conv_tol=0.0)
    assert bt.statuses[0] == 0 and bt.statuses[2] == 0 and bt.statuses[1] != 0
    assert bt.operated["norms"][1] == 0.0
    assert _gauges(bt.engines[1]) == [GC] * len(dims)
    for r in (0, 2):
        nrm, bra, _ = orc.operate(st[r], mpo, maxstep=2, conv_tol=0.0)
        assert abs(bt.operated["norms"][r] - nrm) < oc.BAR_NORM * nrm
        assert oc.state_defect(_dense(bt.engines[r].get_mps()), _dense(bra)) < oc.BAR_STATE
    bt.close()


def test_refusals_leave_everything_as_it_was():
    from helpers import expect_cases as ec
    from helpers import operate_cases as oc
    from pytdscf_amd import TDVPBatch

    name = "mixed"
    dims, _ = oc.SHAPES[name]
    L = len(dims)
    bt = _batch(name, oc.states(name))
    bt.observe()
    before, n0 = _tensors(bt), bt.launches()
    lib, h = bt._lib, bt._handle()

    def refused(match, op_id=2, maxstep=2, tol=0.0, reps=None):
        import ctypes as C

        from pytdscf_amd import _lib

        arr = None if reps is None else (C.c_int * max(len(reps), 1))(*reps)
        rc = lib.mitdvp_batch_operate(h, op_id, maxstep, tol, arr, 0 if reps is None else len(reps), None, None, None)
        assert rc != 0
        with pytest.raises(Exception, match=match):
            _lib.check(rc)
        assert bt.launches() == n0
        assert all(_same(a, b) for a, b in zip(_tensors(bt), before))

    refused("mitdvp_batch_operate: maxstep = 0", maxstep=0)
    refused("mitdvp_batch_operate: conv_tol", tol=-1.0)
    refused("mitdvp_batch_operate: conv_tol", tol=float("nan"))
    refused("mitdvp_batch_operate: conv_tol", tol=float("inf"))
    refused("replica 3 .*outside 0 .. 2", reps=[0, 3])
    refused("replica 1 is listed twice", reps=[1, 0, 1])
    refused("list of replicas is empty", reps=[])
    refused("operator 9 has no core at site 0 of replica 0", op_id=9)
    # an operator missing on one replica: refused when that replica is selected, fine when it is not
    _, shift, mpo = ec.case(name, "product")
    bt.engines[0].set_mpo(mpo, 7, shift=shift)
    bt.engines[2].set_mpo(mpo, 7, shift=shift)
    refused("operator 7 has no core at site 0 of replica 1", op_id=7)
    # core shapes that differ between the replicas
    _, _, wider = ec.case(name, "local")
    bt.engines[1].set_mpo(wider, 7)
    refused("operator 7 has MPO bonds .* of replica 1, replica 0 has", op_id=7)
    # an MPO bond of 17
    def padded(m):
        out = []
        for p in range(L):
            w = np.zeros((1 if p == 0 else m, dims[p], dims[p], 1 if p == L - 1 else m), dtype=np.complex128)
            w[0, :, :, 0] = np.eye(dims[p])
            out.append(w)
        return out

    for e in bt.engines:
        e.set_mpo(padded(17), 8)
    refused("operator 8, site 0: MPO bonds \\(1, 17\\): the batched kernel takes MPO bonds of 1 to 16", op_id=8)
    # outer bonds that are not 1, neighbouring cores that do not fit
    bad = padded(3)
    bad[-1] = np.zeros((3, dims[-1], dims[-1], 2), dtype=np.complex128)
    for e in bt.engines:
        e.set_mpo(bad, 10)
    refused("operator 10: the outer MPO bonds are \\(1, 2\\), they must be 1", op_id=10)
    bad = padded(3)
    bad[2] = np.zeros((2, dims[2], dims[2], 3), dtype=np.complex128)
    for e in bt.engines:
        e.set_mpo(bad, 11)
    refused("operator 11, site 1: MPO bonds \\(3, 3\\): the core of site 2 has the left MPO bond 2", op_id=11)
    # a centre at L-1 after a forward sweep
    bt.sweep(DT, True)
    before, n0 = _tensors(bt), bt.launches()
    refused(f"replica 0 has its centre at site {L - 1}")
    bt.close()
    # the Python front refuses before any handle exists
    bt = TDVPBatch(2, L)
    with pytest.raises(ValueError, match="maxstep = 0"):
        bt.operate(maxstep=0)
    assert bt._b is None
    bt.close()


def test_a_one_site_chain():
    """L = 1: one apply per half-sweep, no QR"""
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import TDVPBatch

    rng = np.random.default_rng(4)
    d = 5
    ops = [(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))[None, :, :, None] for _ in range(2)]
    vs = [(rng.standard_normal((1, d, 1)) + 1j * rng.standard_normal((1, d, 1))) for _ in range(2)]
    bt = TDVPBatch(2, 1)
    for e, w, v in zip(bt.engines, ops, vs):
        e.set_mpo([w], shift=0.2 - 0.1j)
        e.set_mps([v])
    got = bt.operate(0, maxstep=3)
    for r in range(2):
        nrm, bra, it = orc.operate([vs[r]], [ops[r]], maxstep=3, shift=0.2 - 0.1j)
        assert got["iterations"][r] == it
        assert abs(got["norms"][r] - nrm) < 1e-10 * nrm
        assert np.linalg.norm(bt.engines[r].get_mps()[0] - bra[0]) < 1e-9
    bt.close()


def test_correlation_function_from_a_correlated_start(monkeypatch):
    """cross_cases' L = 4, D = 4 spin chain from the oracle's state after two steps (every bond at its exact limit, so the
    fit is exact): C(t) = <psi| A(t) B |psi>, A = sum_p SZ_p, B = sum_p SX_p and a one-site B, against the oracle route
    (orc.operate, OracleMPS runs, walk_mpo) at the project's 1e-8 bar and against dense expm within ten times the oracle
    route's own deviation from it (tests/test_batch_operate_host.py prints and bounds it); a Hartree-product call next to
    it returns what the cross request set by hand returns, launch for launch and bit for bit"""
    from helpers import cross_cases as cc
    from helpers import cross_mpo_cases as xc
    from helpers import operate_cases as oc
    from pytdscf_amd import TDVPBatch, units
    from pytdscf_amd.mps import product_state_cores
    from pytdscf_amd.trajectories import correlation_function

    m = xc.model()
    kw = dict(maxstep=cc.NSTEPS + 1, stepsize=cc.DT * units.au_in_fs)
    start = oc.corr_start()
    for b_form, Bop in (("mpo", "sx_total"), ("site", cc.B_OP)):
        out = correlation_function(m, [start], A="sz_total", B=Bop, per_trajectory=True, **kw)
        assert out["mean"].shape == (cc.NSTEPS + 1,) and out["trajectories"].shape == (cc.NSTEPS + 1, 1)
        o, de = oc.corr_oracle(b_form), oc.corr_dense(b_form)
        d_or, d_de, o_de = np.abs(out["mean"] - o).max(), np.abs(out["mean"] - de).max(), np.abs(o - de).max()
        print(f"B {b_form}: device vs oracle route {d_or:.2e}, device vs dense {d_de:.2e}, oracle route vs dense {o_de:.2e}")
        assert np.abs(out["mean"] - out["trajectories"][:, 0]).max() < 1e-15
        assert d_or < 1e-8
        assert d_de < 10 * o_de
    # two weighted starts, the second a Hartree product written as cores of bond 1
    thin = [np.asarray(v, dtype=np.complex128).reshape(1, 2, 1) for v in cc.START]
    two = correlation_function(m, [start, thin], A="sz_total", B="sx_total", weights=[0.25, 0.75], per_trajectory=True, **kw)
    assert np.abs(two["trajectories"][:, 0] - oc.corr_dense("mpo")).max() < 10 * np.abs(oc.corr_oracle("mpo") - oc.corr_dense("mpo")).max()
    assert np.abs(two["trajectories"][:, 1] - xc.dense_corr("mpo", "mpo")).max() < 1e-8
    assert np.abs(two["mean"] - two["trajectories"] @ [0.25, 0.75]).max() < 1e-14
    # Hartree products are handled as they were: the launches and bits of the cross request set by hand
    from pytdscf_amd import trajectories as tr

    seen = []

    class Counted(TDVPBatch):  # the batch correlation_function makes, its launches read as it is closed
        def close(self):
            if self._b is not None:
                seen.append(self.launches())
            super().close()

    monkeypatch.setattr(tr, "TDVPBatch", Counted)
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
    assert np.array_equal(site, by_hand["mean_cross"])
    assert seen == [bt.launches()]
    bt.close()
