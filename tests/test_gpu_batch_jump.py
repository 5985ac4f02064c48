"""GPU: one-site gates and quantum-jump channels of the batched trajectories (k_batch_channel: one launch per time step
between the two half-sweeps; TDVPBatch.set_gates / set_jumps / jump_counts, propagate_trajectories(jumps=...)).

The sharp test is parity with the NumPy trajectory step of tests/helpers/jump_oracle.py ON THE SAME NUMBERS (the counter
generator is shipped in Python as pytdscf_amd.trajectories.jump_uniform), at the bars of tests/test_gpu_batch.py: final-state
fidelity defect 1 - |<a|b>| / (|a| |b|) < 1e-10, norm to 1e-12, site RDMs to 1e-9, and the jump counters equal to the
oracle's choices exactly."""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIMS, D, M, NREP, NSTEPS, DT = (2, 3, 4, 3, 2), 8, 4, 6, 3, 0.4
SEED = 2024  # of the jump generator; the oracle alone shows every decision's margin >= 1e-6 for it (asserted below)


def _mixed_mpo(dims, M, seed):
    """oracle.tdvp_oracle.synthetic_mpo with a physical dimension per site: Hermitian, nearest-neighbour-like, bond M"""
    rng = np.random.default_rng(seed)
    L, cores = len(dims), []
    for p, d in enumerate(dims):
        def herm(scale):
            G = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
            return scale * (G + G.conj().T) / 2

        W = np.zeros((M, d, d, M), dtype=np.complex128)
        W[0, :, :, 0] = np.eye(d)
        W[M - 1, :, :, M - 1] = np.eye(d)
        for k in range(1, M - 1):
            W[0, :, :, k] = herm(0.01)
            W[k, :, :, M - 1] = herm(0.01)
        W[0, :, :, M - 1] = herm(0.05)
        if p == 0:
            W = W[0:1]
        if p == L - 1:
            W = W[:, :, :, M - 1:M]
        cores.append(np.ascontiguousarray(W))
    return cores


def _kraus_set(K, d, rng):
    """K random matrices rescaled to sum B^+ B = 1"""
    G = rng.standard_normal((K, d, d)) + 1j * rng.standard_normal((K, d, d))
    w, V = np.linalg.eigh(sum(g.conj().T @ g for g in G))
    B = G @ ((V / np.sqrt(w)) @ V.conj().T)
    assert np.abs(sum(b.conj().T @ b for b in B) - np.eye(d)).max() < 1e-12
    return B


@functools.lru_cache(maxsize=None)
def _setup():
    from oracle import tdvp_oracle as orc

    rng = np.random.default_rng(7)
    mpo = _mixed_mpo(DIMS, M, seed=3)
    jumps = {0: _kraus_set(2, DIMS[0], rng), 2: _kraus_set(3, DIMS[2], rng), 4: _kraus_set(4, DIMS[4], rng)}
    gate = np.eye(3) + 0.3 * (rng.standard_normal((3, 3)) + 1j * rng.standard_normal((3, 3)))  # not unitary
    gate *= np.sqrt(3) / np.linalg.norm(gate)  # mean gain 1: the norms stay of order 1, where the 1e-12 bar is meant
    starts = [orc.canonicalize_site0(orc.synthetic_mps(list(DIMS), D, seed=60 + r), scale=1.0) for r in range(NREP)]
    return mpo, jumps, {3: gate}, starts


def _channels(jumps, gates):
    ch = {p: ("jump", B) for p, B in jumps.items()}
    ch.update({p: ("gate", U) for p, U in gates.items()})
    return ch


@functools.lru_cache(maxsize=None)
def _reference(integrator, nsteps=NSTEPS):
    """the oracle's trajectories 0 .. NREP-1, computed once per integrator and left unchanged"""
    from helpers import jump_oracle as jo
    from pytdscf_amd.trajectories import jump_uniform

    mpo, jumps, gates, starts = _setup()
    out = []
    for r in range(NREP):
        st, dec = jo.run_trajectory(starts[r], mpo, DT, nsteps, _channels(jumps, gates),
                                    lambda t, s, p: jump_uniform(SEED, t, s, p), trajectory=r,
                                    integrator=integrator, conserve_norm=False)
        out.append((st.cores, dec))
    return out


def _batch(B, starts, integrator="lanczos", **kw):
    from pytdscf_amd import TDVPBatch

    mpo = _setup()[0]
    bt = TDVPBatch(B, len(DIMS), integrator=integrator, conserve_norm=False, **kw)
    bt.set_mpo(mpo)
    for e, c in zip(bt.engines, starts):
        e.set_mps(c)
    return bt


def _defect(a, b):
    from oracle import tdvp_oracle as orc

    na, nb = np.sqrt(abs(orc.overlap(a, a))), np.sqrt(abs(orc.overlap(b, b)))
    return 1 - abs(orc.overlap(a, b)) / (na * nb), abs(na - nb)


def _bytes(bt, which=None):
    return [[c.tobytes() for c in bt[r].get_mps()] for r in (range(len(bt)) if which is None else which)]


@pytest.mark.parametrize("integrator", ["lanczos", "arnoldi"])
def test_parity_with_the_oracle_on_the_same_numbers(integrator):
    from helpers import jump_oracle as jo
    from oracle import tdvp_oracle as orc

    mpo, jumps, gates, starts = _setup()
    ref = _reference(integrator)
    margins = [d[2] for _, dec in ref for d in dec]
    assert len(margins) == NREP * NSTEPS * len(jumps)
    print(f"{integrator}: smallest decision margin in the oracle {min(margins):.3e}")
    assert min(margins) >= 1e-6  # no decision sits on an edge that rounding could move

    bt = _batch(NREP, starts, integrator)
    bt.set_gates(gates)
    bt.set_jumps(jumps, seed=SEED)
    bt.propagate(DT, NSTEPS)
    assert bt.statuses == [0] * NREP
    counts = bt.jump_counts()
    assert counts.shape == (NREP, len(DIMS), 16)
    for r in range(NREP):
        cores, dec = ref[r]
        got = bt[r].get_mps()
        f, dn = _defect(cores, got)
        drdm = max(np.abs(orc.site_rdm(cores, p) - bt[r].site_rdm(p)).max() for p in range(len(DIMS)))
        print(f"{integrator} replica {r}: fidelity defect {f:.2e} norm {dn:.2e} rdm {drdm:.2e} choices {[d[1] for d in dec]}")
        assert abs(f) < 1e-10 and dn < 1e-12 and drdm < 1e-9
        assert np.array_equal(counts[r], jo.counts_of(dec, len(DIMS))), r
    assert counts.sum() == NREP * NSTEPS * len(jumps)
    bt.close()


def test_bits_do_not_depend_on_the_batch():
    mpo, jumps, gates, starts = _setup()

    def run(B, where, plan):
        from oracle import tdvp_oracle as orc

        filler = orc.canonicalize_site0(orc.synthetic_mps(list(DIMS), D, seed=99), scale=1.0)
        cores = [filler] * B
        ids = [1000 + i for i in range(B)]
        for t, r in enumerate(where):
            cores[r], ids[r] = starts[t], t
        bt = _batch(B, cores)
        bt.set_gates(gates)
        bt.set_jumps(jumps, seed=SEED, trajectory_ids=ids)
        for n in plan:
            bt.propagate(DT, n)
        out = _bytes(bt, where), bt.jump_counts()[list(where)]
        bt.close()
        return out

    small, c_small = run(NREP, range(NREP), (4,))
    scattered = (3, 69, 0, 41, 17, 64)
    big, c_big = run(70, scattered, (4,))
    assert small == big  # the same trajectory ids anywhere in any batch: the same bytes
    assert np.array_equal(c_small, c_big)
    split, c_split = run(NREP, range(NREP), (2, 2))
    assert small == split  # the step counter runs on across calls
    assert np.array_equal(c_small, c_split)


def test_gates_only_against_the_reference_run_and_a_single_engine(golden):
    """tests/golden/gate_chain.npz (the reference's own run: a full gate on site 1, a diagonal one on site 4), four
    replicas of its start.  Its shapes ((6, 3, 6) at most, MPO bond 4) are inside the batch's envelope.  Compared as
    tests/test_gpu_gates.py::test_gate_chain_golden compares, at its tolerances: Krylov counts, energy before the last
    step and at the end, norm, autocorrelation.  That test also compares the cores element by element, which holds for an
    engine whose QR carries LAPACK's signs; the batched kernel's gauge is free (bt_qr), so the final STATE is compared
    instead, by its fidelity to the reference's cores, at the bar of the parity test above."""
    from pytdscf_amd import TDVPEngine

    g = golden("gate_chain.npz")
    n = int(g["nsite"])
    mpo = [g[f"mpo{i}"] for i in range(n)]
    init = [g[f"init{i}"] for i in range(n)]
    dt = float(g["dt_au"])
    gates = {1: g["U1"], 4: g["U4"]}
    from pytdscf_amd import TDVPBatch

    for ns in (1, 3):
        bt = TDVPBatch(4, n)
        bt.set_mpo(mpo)
        for e in bt.engines:
            e.set_mps(init, canonicalize=True)
        bt.set_gates(gates)
        if ns > 1:
            bt.propagate(dt, ns - 1)
        e_last = [e.expectation() for e in bt.engines]
        bt.propagate(dt, 1)
        eng = TDVPEngine(n)
        eng.set_mpo(mpo)
        eng.set_mps(init, canonicalize=True)
        eng.set_gates(gates)
        for _ in range(ns):
            eng.propagate(dt)
        final = [g[f"n{ns}_final{i}"] for i in range(n)]
        el, ef, ac = float(g[f"n{ns}_energy_last"]), float(g[f"n{ns}_energy_final"].real), complex(g[f"n{ns}_autocorr"])
        for r, e in enumerate(bt.engines):
            assert e.krylov_stats() == list(g[f"n{ns}_krylov"])
            assert abs(e_last[r].real - el) < 1e-8 * abs(el)
            assert abs(e.norm() - float(g[f"n{ns}_norm"])) < 1e-12
            assert abs(e.autocorr() - ac) < 1e-8 * abs(ac)
            assert abs(e.expectation().real - ef) < 1e-8 * abs(ef)
            f, _ = _defect(final, e.get_mps())
            f1, dn1 = _defect(eng.get_mps(), e.get_mps())
            print(f"{ns} steps, replica {r}: defect to the reference run {f:.2e}, to the engine {f1:.2e} (norm {dn1:.2e})")
            assert abs(f) < 1e-10
            assert abs(f1) < 1e-10 and dn1 < 1e-12
        eng.close()
        bt.close()


def test_no_channel_means_no_change():
    mpo, jumps, gates, starts = _setup()
    plain = _batch(3, starts[:3])
    plain.propagate(DT, 1)
    n0 = plain.launches()
    plain.propagate(DT, 2)
    assert plain.launches() - n0 == 2 * 2

    bt = _batch(3, starts[:3])
    bt.set_gates(gates)
    bt.set_jumps({2: jumps[2]}, seed=SEED)
    bt.set_gates({3: None})
    bt.set_jumps({2: None})
    bt.propagate(DT, 1)
    n0 = bt.launches()
    bt.propagate(DT, 2)
    assert bt.launches() - n0 == 2 * 2  # a channel set and removed: the two launches per step of before
    assert _bytes(bt) == _bytes(plain)
    assert bt.jump_counts().sum() == 0
    bt.set_jumps({2: jumps[2]}, seed=SEED)
    n0 = bt.launches()
    bt.propagate(DT, 2)
    assert bt.launches() - n0 == 3 * 2  # with a channel: three
    assert bt.jump_counts().sum() == 3 * 2
    assert _bytes(bt) != _bytes(plain)
    plain.close()
    bt.close()


def test_refusals():
    mpo, jumps, gates, starts = _setup()
    bt = _batch(2, starts[:2])
    before = _bytes(bt)

    def refused(call, match):
        with pytest.raises(ValueError, match=match):
            call()
        assert _bytes(bt) == before  # the engines are untouched

    refused(lambda: bt.set_gates({2: np.eye(3)}), "site 2.*physical dimension is 4")
    refused(lambda: bt.set_jumps({2: jumps[0]}), "site 2.*physical dimension is 4")
    refused(lambda: bt.set_jumps({0: np.stack([np.eye(2)] * 17) / np.sqrt(17)}), "site 0.*2 to 16")
    refused(lambda: bt.set_jumps({0: np.eye(2)[None]}), "site 0.*2 to 16")
    refused(lambda: bt.set_gates({5: np.eye(2)}), "site 5 is out of range")
    bt.propagate(DT, 1)  # nothing stuck: no channel is set
    assert bt.launches() > 0 and bt.jump_counts().sum() == 0
    bt.set_jumps({0: jumps[0]}, seed=1)
    before = _bytes(bt)
    refused(lambda: bt.sweep(DT, True), "half-sweep")
    bt.close()

    cold = _batch(2, starts[:2], relax=True)
    before_cold = _bytes(cold)
    with pytest.raises(ValueError, match="imaginary time"):
        cold.set_jumps({0: jumps[0]})
    with pytest.raises(ValueError, match="imaginary time"):
        cold.set_gates(gates)
    assert _bytes(cold) == before_cold
    cold.close()


def test_a_changed_engine_list_checks_the_ids_and_restarts_the_counters():
    mpo, jumps, gates, starts = _setup()
    bt = _batch(3, starts[:3])
    bt.set_jumps({2: jumps[2]}, seed=SEED, trajectory_ids=[5, 6, 7])
    bt.propagate(DT, 1)
    assert bt.jump_counts().sum() == 3
    spare = bt.engines.pop()  # the library's batch object is made anew at the next call
    before = _bytes(bt)
    with pytest.raises(ValueError, match="2 replicas now, trajectory_ids were given for 3"):
        bt.propagate(DT, 1)
    assert _bytes(bt) == before
    bt.set_jumps({2: jumps[2]}, seed=SEED, trajectory_ids=[5, 6])
    assert bt.jump_counts().sum() == 0
    bt.propagate(DT, 1)
    assert bt.statuses == [0, 0] and bt.jump_counts().sum() == 2
    spare.close()
    bt.close()


def test_a_jump_channel_that_annihilates_one_replica():
    """H diagonal in the product basis, so the middle spin of replica 1 stays |0> exactly; both jump operators are
    multiples of |1><1|: W == 0 for that replica, which reports the zero-norm status, and the others finish."""
    from helpers import spin_bath as sb
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import TDVPBatch, _lib
    from pytdscf_amd.mps import product_state_cores

    dims = [2, 2, 2]
    sz = np.diag([0.5, -0.5]).astype(complex)
    mpo = sb.sop_mpo([(1.0, {0: sz, 1: sz}), (0.7, {1: sz, 2: sz}), (0.3, {1: sz})], dims)
    P1 = np.diag([0.0, 1.0]).astype(complex)
    B = np.stack([np.sqrt(0.25) * P1, np.sqrt(0.75) * P1])
    up, dn, mix = [1, 0], [0, 1], [1, 1]
    starts = [[up, dn, mix], [mix, up, dn], [dn, mix, up]]
    bt = TDVPBatch(3, 3)
    bt.set_mpo(mpo)
    for e, s in zip(bt.engines, starts):
        e.set_mps(orc.canonicalize_site0(product_state_cores(s, 4, space="hilbert"), scale=1.0))
    bt.set_jumps({1: B}, seed=5)
    with pytest.raises(ValueError, match="zero"):
        bt.propagate(0.2, 2)
    assert bt.statuses == [0, _lib.EINVAL, 0]
    msg = _lib.load().mitdvp_last_error(bt[1]._h).decode()
    assert "zero" in msg, msg
    counts = bt.jump_counts()
    assert counts[1].sum() == 0 and counts[0].sum() == 2 and counts[2].sum() == 2
    for r in (0, 2):
        assert abs(bt[r].norm() - 1) < 1e-12  # the norm before a jump is kept
        rho = bt[r].site_rdm(1)
        assert abs(rho[1, 1] - 1) < 1e-12  # after P1 the middle spin is |1>
    with pytest.raises(ValueError):
        bt[1].propagate(0.2)  # stopped in the middle of a step: it must be given its tensors again
    bt.close()


def test_end_to_end_through_propagate_trajectories():
    """The L = 3 spin chain of tests/helpers/spin_bath.py at full bond with its amplitude-damping jump on the middle
    site, 4 starts x 512 replicas = 2048 trajectories, 4 steps: the mean middle-site density at the last record against
    the dense map of tests/test_batch_jump_host.py.  Tolerance per real number by Hoeffding (independent trajectories,
    entries of a pure-state density of norm <= 1 lie in [-1, 1]): t = sqrt(2 ln(2 E / 1e-6) / B) = 0.130 for E = 18
    compared numbers.  This catches gross errors only (the parity test is the sharp one); it cannot pass trivially: the
    dense results with and without the channel differ by 0.826 >= 3 t in one entry, asserted from dense CPU math.
    Measured on an MI355X: max |mean - dense| = 4.3e-3.  Wall time there: 18 s, the one slow test of this file, and none
    of it is the ensemble's propagation (0.2 s for the 4 steps, 0.4 s for the first call's preparation, 0.3 s for MPOs
    and states): 6.6 s go into creating the 2048 engines the batch borrows (a stream, mapped host words and device
    buffers each) and 8.5 s into destroying them."""
    from helpers import jump_oracle as jo
    from helpers import spin_bath as sb
    from pytdscf_amd import Exciton, Model, units
    from pytdscf_amd.kraus import lindblad_to_kraus
    from pytdscf_amd.trajectories import propagate_trajectories

    case = sb.case_trajectories()
    dims, nsteps, rps = case["dims"], 4, 512
    Bk = lindblad_to_kraus([sb.L_AMP], sb.DT)
    H = jo.dense_operator(case["mpo"])

    def dense(jumps):
        acc = 0
        for start in case["starts"]:
            v = np.ones(1, dtype=complex)
            for w in start:
                v = np.kron(v, np.asarray(w, dtype=complex) / np.linalg.norm(w))
            rho = np.outer(v, v.conj())
            for _ in range(nsteps):
                rho = jo.dense_channel_step(rho, H, sb.DT, jumps, dims)
            acc = acc + np.einsum("abcadc->bd", rho.reshape(2, 3, 2, 2, 3, 2))
        return acc / len(case["starts"])

    def reals(x):
        return np.concatenate([x.real.ravel(), x.imag.ravel()])

    B = rps * len(case["starts"])
    with_ch, without = dense({1: Bk}), dense({})
    E = reals(with_ch).size
    t = np.sqrt(2 * np.log(2 * E / 1e-6) / B)
    gap = np.abs(reals(with_ch) - reals(without)).max()
    assert E == 18 and gap >= 3 * t, (gap, t)

    model = Model([Exciton(nstate=d) for d in dims], operators={"hamiltonian": case["mpo"]}, bond_dim=64)
    out = propagate_trajectories(model, case["starts"], maxstep=nsteps + 1, stepsize=sb.DT * units.au_in_fs,
                                 reduced_density=([(1, 1)], 1), integrator="arnoldi", conserve_norm=False,
                                 jumps={1: Bk}, seed=11, replicas_per_start=rps)
    mean = out["mean"][(1, 1)]
    assert mean.shape == (nsteps + 1, 3, 3)
    err = np.abs(reals(mean[-1]) - reals(with_ch)).max()
    print(f"B = {B}: max |mean - dense| = {err:.3e} (t = {t:.3f}; with / without the channel differ by {gap:.3f})")
    assert err < t
