"""GPU: time-dependent one-site fields of the batched trajectories (k_batch_field: one launch per time step between the
forward half-sweep and the channels; TDVPBatch.set_fields / field_values, propagate_trajectories(fields=...)).

The sharp test is parity with the NumPy step of tests/helpers/field_oracle.py ON THE SAME NUMBERS -- the oracle is fed the
amplitudes the device reports, one step at a time -- at the bars of tests/test_gpu_batch_jump.py: final-state fidelity
defect 1 - |<a|b>| / (|a| |b|) < 1e-10, norm to 1e-12, site RDMs to 1e-9.  The amplitudes themselves are held to the Python
restatement of the generator (pytdscf_amd.trajectories.field_noise_path) at 1e-12 (sigma + |table|)."""

import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIMS, D, M, NREP, NSTEPS, DT = (2, 3, 4, 3, 2), 8, 4, 6, 3, 0.4
SEED = 2024  # the seed of tests/test_gpu_batch_jump.py, whose jump decisions have margins >= 1e-6 without fields
SIGMA, TAU = 0.5, 1.0
L = len(DIMS)


def _mixed_mpo(dims, M, seed):
    """oracle.tdvp_oracle.synthetic_mpo with a physical dimension per site: Hermitian, nearest-neighbour-like, bond M"""
    rng = np.random.default_rng(seed)
    n, cores = len(dims), []
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
        if p == n - 1:
            W = W[:, :, :, M - 1:M]
        cores.append(np.ascontiguousarray(W))
    return cores


def _kraus_set(K, d, rng):
    G = rng.standard_normal((K, d, d)) + 1j * rng.standard_normal((K, d, d))
    w, V = np.linalg.eigh(sum(g.conj().T @ g for g in G))
    return G @ ((V / np.sqrt(w)) @ V.conj().T)


def _herm(d, rng):
    G = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    return (G + G.conj().T) / 2


@functools.lru_cache(maxsize=None)
def _setup():
    from oracle import tdvp_oracle as orc

    rng = np.random.default_rng(7)
    mpo = _mixed_mpo(DIMS, M, seed=3)
    jumps = {0: _kraus_set(2, DIMS[0], rng), 2: _kraus_set(3, DIMS[2], rng), 4: _kraus_set(4, DIMS[4], rng)}
    gate = np.eye(3) + 0.3 * (rng.standard_normal((3, 3)) + 1j * rng.standard_normal((3, 3)))  # not unitary
    gate *= np.sqrt(3) / np.linalg.norm(gate)
    starts = [orc.canonicalize_site0(orc.synthetic_mps(list(DIMS), D, seed=60 + r), scale=1.0) for r in range(NREP)]
    G = {p: _herm(d, rng) for p, d in enumerate(DIMS)}
    shared = rng.standard_normal(NSTEPS)              # one table for all replicas, sites 1 and 3
    own = rng.standard_normal((NREP, NSTEPS + 1))      # one row per replica, site 0
    return mpo, jumps, {3: gate}, starts, G, shared, own


def _fields(own_rows=None, shared_len=None):
    """a shared pulse table on sites 1 and 3, a per-replica table on site 0, OU noise on sites 2 and 4"""
    G, shared, own = _setup()[4:]
    own = own if own_rows is None else own_rows
    sh = shared if shared_len is None else shared[:shared_len]
    return {0: dict(G=G[0], pulse=own), 1: dict(G=G[1], pulse=sh), 3: dict(G=G[3], pulse=0.5 * sh),
            2: dict(G=G[2], sigma=SIGMA, tau=TAU), 4: dict(G=G[4], sigma=SIGMA, tau=TAU)}


def _batch(B, starts, integrator="lanczos", **kw):
    from pytdscf_amd import TDVPBatch

    mpo = _setup()[0]
    kw.setdefault("conserve_norm", False)
    bt = TDVPBatch(B, L, integrator=integrator, **kw)
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


def _parity(integrator, channels):
    """the device against field_oracle.field_step fed with the device's own amplitudes, step by step"""
    from helpers import field_oracle as fo
    from helpers import jump_oracle as jo
    from oracle import tdvp_oracle as orc
    from pytdscf_amd.trajectories import jump_uniform

    mpo, jumps, gates, starts, G = _setup()[:5]
    bt = _batch(NREP, starts, integrator)
    oracle_channels = None
    if channels:
        bt.set_gates(gates)
        oracle_channels = {p: ("jump", B) for p, B in jumps.items()}
        oracle_channels.update({p: ("gate", U) for p, U in gates.items()})
    bt.set_jumps(jumps if channels else {}, seed=SEED)
    bt.set_fields(_fields())
    refs = [orc.OracleMPS([np.array(c) for c in starts[r]], mpo, integrator=integrator, conserve_norm=False) for r in range(NREP)]
    decisions = [[] for _ in range(NREP)]
    for s in range(NSTEPS):
        bt.propagate(DT, 1)
        assert bt.statuses == [0] * NREP
        amps = bt.field_values()
        assert amps.shape == (NREP, L) and np.all(amps != 0)  # every site carries a field here
        for r in range(NREP):
            decisions[r] += fo.field_step(refs[r], DT, amps[r], G, oracle_channels, lambda t, st, p: jump_uniform(SEED, t, st, p), r, s)
    counts = bt.jump_counts()
    for r in range(NREP):
        got = bt[r].get_mps()
        f, dn = _defect(refs[r].cores, got)
        drdm = max(np.abs(orc.site_rdm(refs[r].cores, p) - bt[r].site_rdm(p)).max() for p in range(L))
        print(f"{integrator} channels={channels} replica {r}: fidelity defect {f:.2e} norm {dn:.2e} rdm {drdm:.2e}")
        assert abs(f) < 1e-10 and dn < 1e-12 and drdm < 1e-9
        if channels:
            margins = [d[2] for d in decisions[r]]
            assert min(margins) >= 1e-6, min(margins)  # no decision sits on an edge that rounding could move
            assert np.array_equal(counts[r], jo.counts_of(decisions[r], L)), r
    if channels:
        assert counts.sum() == NREP * NSTEPS * len(jumps)
    bt.close()


@pytest.mark.parametrize("integrator", ["lanczos", "arnoldi"])
def test_parity_with_the_oracle_on_the_same_numbers(integrator):
    _parity(integrator, channels=False)


def test_fields_together_with_channels():
    _parity("lanczos", channels=True)


def test_device_amplitudes_equal_the_python_restatement():
    """tables (0 past their end), the OU recursion under a changing dt, trajectory ids, the fresh draw after a new seed
    and after set_fields in the middle of the seed's count.  Bar: 1e-12 (sigma + |table|) -- log1p, cos, exp and the
    fused multiply-add of the recursion may differ in the last places, nothing else may."""
    from pytdscf_amd.trajectories import field_noise_path

    starts, G, shared, own = _setup()[3:]
    ids = [11, 5, 2**40 + 3, 0, 77, 6]
    bt = _batch(NREP, starts)
    bt.set_jumps({}, seed=SEED, trajectory_ids=ids)
    bt.set_fields(_fields(shared_len=2))
    bar = 1e-12 * (SIGMA + max(np.abs(shared).max(), np.abs(own).max()))

    def check(seed, first_step, dts, n_before=0):
        """the steps of lengths dts that follow n_before steps since the field clock's reset at first_step"""
        worst = 0.0
        got = []
        for dt in dts:
            bt.propagate(dt, 1)
            got.append(bt.field_values())
        hist = hist_dts + list(dts)
        for r in range(NREP):
            for p in (2, 4):
                want = field_noise_path(seed, ids[r], p, L, SIGMA, TAU, hist, first_step=first_step)[n_before:]
                worst = max(worst, np.abs(np.array([g[r, p] for g in got]) - want).max())
            for k in range(len(dts)):
                n = n_before + k
                assert got[k][r, 0] == (own[r, n] if n < own.shape[1] else 0.0)
                assert got[k][r, 1] == (shared[n] if n < 2 else 0.0)
                assert got[k][r, 3] == (0.5 * shared[n] if n < 2 else 0.0)
        hist_dts.extend(dts)
        return worst

    hist_dts = []
    w1 = check(SEED, 0, [DT, DT, 0.2, DT, 0.1])  # past the ends of both tables (2 and 4 entries); dt changes twice
    bt.set_jumps({}, seed=SEED + 1, trajectory_ids=ids)  # a new seed: the field clock and the step counter restart
    hist_dts = []
    w2 = check(SEED + 1, 0, [DT, DT])
    bt.set_fields(_fields(shared_len=2))  # the field clock restarts, the seed's step counter (2) runs on
    hist_dts = []
    w3 = check(SEED + 1, 2, [DT, 0.3])
    print(f"max |device - Python| {w1:.2e} {w2:.2e} {w3:.2e} (bar {bar:.2e})")
    assert max(w1, w2, w3) <= bar
    bt.close()


def test_bits_do_not_depend_on_the_batch():
    from oracle import tdvp_oracle as orc

    starts, G, shared, own = _setup()[3:]

    def run(B, where, plan):
        filler = orc.canonicalize_site0(orc.synthetic_mps(list(DIMS), D, seed=99), scale=1.0)
        cores = [filler] * B
        ids = [1000 + i for i in range(B)]
        rows = np.full((B, own.shape[1]), 0.123)
        for t, r in enumerate(where):
            cores[r], ids[r], rows[r] = starts[t], t, own[t]
        bt = _batch(B, cores)
        bt.set_jumps({}, seed=SEED, trajectory_ids=ids)
        bt.set_fields(_fields(own_rows=rows))
        for n in plan:
            bt.propagate(DT, n)
        out = _bytes(bt, where), bt.field_values()[list(where)].tobytes()
        bt.close()
        return out

    small = run(NREP, range(NREP), (4,))
    big = run(70, (3, 69, 0, 41, 17, 64), (4,))
    assert small == big  # the same trajectory ids anywhere in any batch: the same bytes
    split = run(NREP, range(NREP), (2, 2))
    assert small == split  # the field clock and the noise state run on across calls


def test_a_unitary_keeps_the_norm():
    """conserve_norm=False and a Hermitian MPO: nothing rescales, so the norm shows what the field launch does to it.  The
    Krylov threshold is 1e-14 here: at the default 1e-9 the local exponentials alone move the norm by 1e-7, field or not."""
    starts = _setup()[3]
    bt = _batch(NREP, starts, "arnoldi", thresh=1e-14)
    bt.set_jumps({}, seed=SEED)
    bt.set_fields(_fields())
    for s in range(NSTEPS):
        bt.propagate(DT, 1)
        worst = max(abs(e.norm() - 1) for e in bt.engines)
        print(f"step {s}: max |norm - 1| = {worst:.2e}")
        assert worst < 1e-12
    bt.close()


def test_zero_amplitude_and_launches():
    """pulse = zeros: the bytes of the same batch without a field; one more launch per step while a field is set, none
    after set_fields({})"""
    starts, G = _setup()[3:5]
    plain = _batch(3, starts[:3])
    plain.propagate(DT, 1)
    n0 = plain.launches()
    plain.propagate(DT, 2)
    assert plain.launches() - n0 == 2 * 2

    bt = _batch(3, starts[:3])
    bt.set_fields({1: dict(G=G[1], pulse=np.zeros(8)), 4: dict(G=G[4], pulse=np.zeros((3, 8))), 2: dict(G=G[2], sigma=0.0, tau=1.0)})
    bt.propagate(DT, 1)
    n0 = bt.launches()
    bt.propagate(DT, 2)
    assert bt.launches() - n0 == 3 * 2  # with a field: three
    assert _bytes(bt) == _bytes(plain)
    assert np.array_equal(bt.field_values(), np.zeros((3, L)))
    bt.set_fields({})
    n0 = bt.launches()
    bt.propagate(DT, 2)
    plain.propagate(DT, 2)
    assert bt.launches() - n0 == 2 * 2  # the fields removed: the two launches per step of before
    assert _bytes(bt) == _bytes(plain)
    bt.set_fields({1: dict(G=G[1], pulse=[0.3])})
    n0 = bt.launches()
    bt.propagate(DT, 2)
    assert bt.launches() - n0 == 3 * 2
    assert _bytes(bt) != _bytes(plain)
    assert np.array_equal(bt.field_values(), np.zeros((3, L)))  # the second step lies past the table's end
    plain.close()
    bt.close()


def test_driven_chain_against_the_time_ordered_state():
    """The L = 4 driven chain at D = 4 (its full bond), dt = 0.025, 40 steps, against the dense time-ordered state.  Bar:
    1.5 x the error of the NumPy step at that dt (8.95e-5 with this pulse), so the kernel is bounded by the splitting's own
    error, not by a guess."""
    from helpers import field_oracle as fo
    from helpers import jump_oracle as jo
    from pytdscf_amd import TDVPBatch
    from pytdscf_amd.trajectories import pulse_table

    case = fo.driven_chain(D=4)
    dt, n = 0.025, 40
    exact = fo.dense_time_ordered(jo.dense_state(case["start"]), case["H0"], fo.pulse, case["G"], 0.0, fo.T_END)
    own = np.linalg.norm(jo.dense_state(fo.run_numpy(case, dt, n).cores) - exact)
    bt = TDVPBatch(1, 4, integrator="arnoldi", conserve_norm=False, thresh=1e-13)
    bt.set_mpo(case["mpo"])
    bt[0].set_mps(case["start"])
    tab = pulse_table(fo.pulse, dt, n)
    bt.set_fields({p: dict(G=Gp, pulse=tab) for p, Gp in case["fields"].items()})
    bt.propagate(dt, n)
    got = jo.dense_state(bt[0].get_mps())
    err = np.linalg.norm(got - exact)
    print(f"|device - exact| = {err:.3e}, |NumPy step - exact| = {own:.3e}")
    assert err < 1.5 * own
    bt.close()


def test_refusals():
    from pytdscf_amd import TDVPBatch, _lib

    starts, G = _setup()[3:5]
    bt = _batch(2, starts[:2])
    bt.propagate(DT, 1)
    before = _bytes(bt)
    lib, h = bt._lib, bt._handle()
    dp = C.POINTER(C.c_double)
    g2, V2 = np.linalg.eigh(G[0])
    V2 = np.ascontiguousarray(V2, dtype=np.complex128)
    tab = np.ones(3)
    pv, pg, pt = V2.ctypes.data_as(dp), g2.ctypes.data_as(dp), tab.ctypes.data_as(dp)

    def refused(args, match):
        assert lib.mitdvp_batch_set_field(h, *args) == _lib.EINVAL
        msg = lib.mitdvp_last_error(None).decode()
        import re
        assert re.search(match, msg), msg

    refused((5, 2, pv, pg, _lib.FIELD_TABLE, pt, 3, 0, 0.0, 0.0), "site 5 is out of range")
    refused((-1, 2, pv, pg, _lib.FIELD_TABLE, pt, 3, 0, 0.0, 0.0), "site -1 is out of range")
    refused((1, 2, pv, pg, _lib.FIELD_TABLE, pt, 3, 0, 0.0, 0.0), "site 1.*physical dimension is 3")
    refused((0, 2, pv, pg, 3, pt, 3, 0, 0.0, 0.0), "site 0.*kind")
    refused((0, 2, pv, pg, 0, pt, 3, 0, 0.0, 0.0), "site 0.*kind")
    refused((0, 2, pv, pg, _lib.FIELD_TABLE, pt, 0, 0, 0.0, 0.0), "site 0.*at least 1")
    refused((0, 2, pv, pg, _lib.FIELD_TABLE, None, 3, 0, 0.0, 0.0), "site 0.*null table")
    refused((0, 2, pv, pg, _lib.FIELD_OU, None, 0, 0, -0.5, 1.0), "site 0.*sigma and tau")
    refused((0, 2, pv, pg, _lib.FIELD_OU, None, 0, 0, 0.5, float("nan")), "site 0.*sigma and tau")
    refused((0, 2, pv, pg, _lib.FIELD_OU, None, 0, 0, float("inf"), 1.0), "site 0.*sigma and tau")
    n0 = bt.launches()
    bt.propagate(DT, 1)  # nothing changed: no field is set, two launches
    assert bt.launches() - n0 == 2 and np.array_equal(bt.field_values(), np.zeros((2, L)))
    with pytest.raises(ValueError, match="order 2.*dimension is 3"):  # the Python layer refuses first
        bt.set_fields({1: dict(G=G[0], pulse=[1.0])})
    bt.set_fields({3: dict(G=G[3], pulse=[1.0])})
    before = _bytes(bt)
    with pytest.raises(ValueError, match="half-sweep.*fields.*site 3"):
        bt.sweep(DT, True)
    assert _bytes(bt) == before
    bt.close()

    cold = _batch(2, starts[:2], relax=True)
    before = _bytes(cold)
    with pytest.raises(ValueError, match="site 0.*imaginary time"):
        cold.set_fields({0: dict(G=G[0], pulse=[1.0])})
    assert _bytes(cold) == before
    cold.close()

    # a site above the kernel's limit of 64: L = 2, dims (65, 2)
    from oracle import tdvp_oracle as orc

    dims = (65, 2)
    wide = TDVPBatch(1, 2, conserve_norm=False)
    wide.set_mpo(_mixed_mpo(dims, M, seed=4))
    wide[0].set_mps(orc.canonicalize_site0(orc.synthetic_mps(list(dims), 2, seed=1), scale=1.0))
    with pytest.raises(ValueError, match="site 0.*65.*at most 64"):
        wide.set_fields({0: dict(G=np.diag(np.arange(65.0)), pulse=[1.0])})
    wide.set_fields({1: dict(G=G[0], pulse=[0.2])})  # the other site is fine
    wide.propagate(DT, 1)
    assert wide.field_values()[0, 1] == 0.2
    wide.close()


def test_end_to_end_through_propagate_trajectories():
    """propagate_trajectories(fields=...) with a callable pulse, noise (tau in fs) and a jump channel against the same
    run driven step by step through TDVPBatch: the per-trajectory densities of every record to 1e-10 (the same kernels
    on the same numbers; the two read the density by different routes)."""
    from helpers import spin_bath as sb
    from pytdscf_amd import Exciton, Model, TDVPBatch, units
    from pytdscf_amd.kraus import lindblad_to_kraus
    from pytdscf_amd.mps import product_state_cores
    from pytdscf_amd.trajectories import propagate_trajectories, pulse_table

    case = sb.case_trajectories()
    dims, nsteps, rps = case["dims"], 3, 2
    stepsize = sb.DT * units.au_in_fs
    Bk = lindblad_to_kraus([sb.L_AMP], sb.DT)
    pulse = lambda t: 0.8 * np.sin(3.0 * t / stepsize)  # t in fs
    tau_fs = 2.5 * stepsize
    fields = {0: dict(G=2 * sb.SX, pulse=pulse), 2: dict(G=2 * sb.SZ, sigma=0.4, tau=tau_fs)}
    model = Model([Exciton(nstate=d) for d in dims], operators={"hamiltonian": case["mpo"]}, bond_dim=64)
    out = propagate_trajectories(model, case["starts"], maxstep=nsteps + 1, stepsize=stepsize, reduced_density=([(1, 1)], 1),
                                 integrator="arnoldi", conserve_norm=False, jumps={1: Bk}, seed=11, replicas_per_start=rps,
                                 first_trajectory=100, per_trajectory=True, fields=fields)
    traj = out["trajectories"][(1, 1)]
    nrep = rps * len(case["starts"])
    assert traj.shape == (nsteps + 1, nrep, 3, 3)

    mpo = model.project_mpo(model.hamiltonian.as_mpo(model.dims))
    bt = TDVPBatch(nrep, 3, integrator="arnoldi", conserve_norm=False, thresh=1.0e-9)
    for i, e in enumerate(bt.engines):
        e.set_mpo(mpo, 0, shift=model.hamiltonian.coupleJ[0][0])
        e.set_mps(product_state_cores(case["starts"][i // rps], 64, space="hilbert"), canonicalize=True, scale=1.0)
    bt.set_jumps({1: Bk}, seed=11, trajectory_ids=range(100, 100 + nrep))
    bt.set_fields({0: dict(G=2 * sb.SX, pulse=pulse_table(pulse, stepsize, nsteps)),
                   2: dict(G=2 * sb.SZ, sigma=0.4, tau=tau_fs / units.au_in_fs)})
    worst = 0.0
    for s in range(nsteps + 1):
        for r in range(nrep):
            worst = max(worst, np.abs(bt[r].site_rdm(1) - traj[s, r]).max())
        if s < nsteps:
            bt.propagate(sb.DT, 1)
    amps = bt.field_values()
    assert np.all(amps[:, 0] == pulse_table(pulse, stepsize, nsteps)[-1]) and len(set(amps[:, 2])) == nrep and np.all(amps[:, 1] == 0)
    print(f"max |run - step by step| over {nsteps + 1} records = {worst:.2e}")
    assert worst < 1e-10
    bt.close()
