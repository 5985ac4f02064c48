"""GPU: ground states of a batch by improved relaxation (TDVPBatch(relax="improved"), TDVPBatch.relax,
mitdvp_batch_relax: k_batch_relax finds the lowest eigenvector of every local H_eff by a Lanczos solver that stays on the
device, one workgroup per replica) and trajectories.relax_trajectories.

The inputs are the disordered Heisenberg chains and field-only chains of helpers/relax_cases: tests/test_batch_relax_host.py
shows on the CPU that their local solves take more Krylov vectors than the exponential keeps (24 .. 43 against 21), that
they have a gap, and that the oracle's own scatter under a 1e-13 perturbation of the start is below 1e-12 -- far under the
bars, which are the project's own (tests/test_gpu_batch.py, test_gpu_parity.py): fidelity defect < 1e-10, energy within
1e-8 |E|, |norm - 1| < 1e-12.  Krylov dimensions are printed, never asserted: the eigen-solver stops on rounding-level
quantities once a site has converged (tests/test_gpu_combos.py), so they are no parity quantity."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FID, ENE, NRM = 1e-10, 1e-8, 1e-12


def _engine(mpo, cores, shift=0.0, **kw):
    from pytdscf_amd import TDVPEngine

    e = TDVPEngine(len(mpo), relax="improved", **kw)
    e.set_mpo(mpo, shift=shift)
    e.set_mps(cores)
    return e


def _batch(items, **kw):
    """items: [(mpo, cores) or (mpo, cores, shift)], one engine each with its own Hamiltonian"""
    from pytdscf_amd import TDVPBatch

    return TDVPBatch.from_engines([_engine(*it, **kw) for it in items])


def _close(bt):
    engines = list(bt.engines)
    bt.close()
    for e in engines:
        e.close()


def _heis(dims, D, seeds):
    from helpers import relax_cases as rc

    return [(rc.heisenberg_mpo(dims, s), rc.start(dims, D, s)) for s in seeds]


def _tensors(bt):
    return [e.get_mps() for e in bt.engines]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _krylov(e):
    return [e.krylov_memory(p) for p in range(e.nsite)]


def _check_state(got_engine, ref_cores, ref_energy, what):
    from helpers import relax_cases as rc

    fid = rc.fidelity_defect(ref_cores, got_engine.get_mps())
    e = got_engine.expectation().real
    n = got_engine.norm()
    print(f"{what}: fidelity defect {fid:.2e}, energy {e:.12f} against {ref_energy:.12f}, |norm - 1| {abs(n - 1):.2e}, k {_krylov(got_engine)}")
    assert fid < FID
    assert abs(e - ref_energy) < ENE * abs(ref_energy)
    assert abs(n - 1) < NRM


# ---- 1. engines stepped one at a time ----
@pytest.mark.parametrize("name,B", [("L8d2D4", 5), ("L6d3D6", 3)])
def test_against_engines_stepped_one_at_a_time(name, B):
    from helpers import relax_cases as rc

    dims, D, seeds = rc.PARITY[name]
    items = _heis(dims, D, seeds[:B])
    steps = 3
    bt = _batch(items)
    try:
        bt.propagate(0.0, 1)  # builds the right blocks with the engines' own launches, once
        for e in bt.engines:
            e.counters_reset()
        bt.propagate(0.0, steps - 1)
        assert bt.statuses == [0] * B
        c0 = bt[0].counters()
        assert c0["n_launch"] == 2 * (steps - 1)  # two launches per step, whatever B and L
        assert bt[1].counters()["n_launch"] == 0
        for e in bt.engines:
            c = e.counters()
            assert c["n_exp_bond"] == 0  # improved relaxation has no bond step
            assert c["n_exp_site"] == 2 * (steps - 1) * len(dims)
        for r, it in enumerate(items):
            ref = _engine(*it)
            ref.set_small_kernels(False)
            for _ in range(steps):
                ref.propagate(0.0)
            print("engine k", _krylov(ref))
            _check_state(bt[r], ref.get_mps(), ref.expectation().real, f"{name} replica {r}")
            ref.close()
    finally:
        _close(bt)


# ---- 2. the oracle ----
def test_against_the_oracle():
    from helpers import relax_cases as rc

    dims, D, seeds = rc.PARITY["L6d3D6"]
    bt = _batch(_heis(dims, D, seeds[:2]))
    try:
        bt.propagate(0.0, 3)
        for r, s in enumerate(seeds[:2]):
            energies, kmax, _, cores = rc.oracle_relax("heis", dims, D, s, 3)
            print("oracle largest k per step", kmax)
            _check_state(bt[r], cores, energies[-1], f"oracle seed {s}")
    finally:
        _close(bt)


# ---- 3. the reference ----
def test_against_the_reference(golden):
    """tests/golden/chain_improved_relax.npz through a batch of 2 identical replicas, held as
    test_chain_improved_relaxation_golden holds the engine"""
    from helpers import relax_cases as rc

    g = golden("chain_improved_relax.npz")
    n = int(g["nsite"])
    mpo = [g[f"mpo{i}"] for i in range(n)]
    init = [g[f"init{i}"] for i in range(n)]
    for ns in (1, 3):
        engines = []
        for _ in range(2):
            from pytdscf_amd import TDVPEngine

            e = TDVPEngine(n, relax="improved")
            e.set_mpo(mpo)
            e.set_mps(init, canonicalize=True)
            engines.append(e)
        from pytdscf_amd import TDVPBatch

        bt = TDVPBatch.from_engines(engines)
        try:
            e_last = None
            for _ in range(ns):
                e_last = [e.expectation().real for e in bt.engines]
                bt.propagate(0.0, 1)
            ref = [g[f"n{ns}_final{i}"] for i in range(n)]
            for r, e in enumerate(bt.engines):
                assert abs(e_last[r] - float(g[f"n{ns}_energy_last"])) < 1e-8 * abs(float(g[f"n{ns}_energy_last"]))
                assert abs(e.expectation().real - float(g[f"n{ns}_energy_final"])) < 1e-8 * abs(float(g[f"n{ns}_energy_final"]))
                assert abs(e.norm() - 1) < NRM
                fid = rc.fidelity_defect(ref, e.get_mps())
                print(f"n{ns} replica {r}: fidelity defect {fid:.2e}")
                assert fid < 1e-9
            assert _same(bt[0].get_mps(), bt[1].get_mps())
        finally:
            _close(bt)


# ---- 4. awkward shapes ----
@pytest.mark.parametrize("dims,D", [((3, 3), 3), ((2, 3, 2), 4), ((8, 8, 8, 8), 3)])
def test_awkward_shapes(dims, D):
    from helpers import relax_cases as rc

    seeds = (0, 1)
    bt = _batch(_heis(dims, D, seeds))
    try:
        bt.propagate(0.0, 2)
        assert bt.statuses == [0, 0]
        for r, s in enumerate(seeds):
            energies, kmax, _, cores = rc.oracle_relax("heis", dims, D, s, 2)
            print("oracle largest k per step", kmax)
            _check_state(bt[r], cores, energies[-1], f"{dims} D {D} seed {s}")
    finally:
        _close(bt)


# ---- 5. exhausted Krylov space ----
@pytest.mark.parametrize("D", [1, 4])
def test_field_only_chain_exhausts_the_krylov_space(D):
    """k = N at every site of the D = 1 chain, beta < eps at D = 4: both early ends; the energy is the sum of the lowest
    one-site eigenvalues"""
    from helpers import relax_cases as rc

    dims, _ = rc.FIELD
    seeds = (0, 1, 2)
    bt = _batch([(rc.field_mpo(dims, s), rc.start(dims, D, s)) for s in seeds])
    try:
        out = bt.relax(2)
        assert bt.statuses == [0, 0, 0]
        for r, s in enumerate(seeds):
            e0 = rc.field_ground_energy(dims, s)
            print(f"D {D} seed {s}: energy {out['energy'][r]:.15f} against {e0:.15f}, k {_krylov(bt[r])}")
            assert abs(out["energy"][r] - e0) < 1e-12
            assert abs(bt[r].expectation().real - e0) < 1e-12
            assert abs(bt[r].norm() - 1) < NRM
    finally:
        _close(bt)


# ---- 6. a scalar term ----
def test_a_scalar_term_shifts_the_energy_and_nothing_else():
    from helpers import relax_cases as rc

    dims, D, seeds = rc.PARITY["L8d2D4"]
    s = seeds[0]
    mpo, cores = rc.heisenberg_mpo(dims, s), rc.start(dims, D, s)
    bt = _batch([(mpo, cores, 0.4), (mpo, cores, 0.0)])
    try:
        out = bt.relax(3)
        e_shift, e_plain = bt[0].expectation(0).real, bt[1].expectation(0).real
        print("energies", out["energy"], "expectation", e_shift, e_plain)
        assert abs(out["energy"][0] - e_shift) < ENE * abs(e_shift)
        assert abs(out["energy"][1] - e_plain) < ENE * abs(e_plain)
        assert abs(e_shift - e_plain - 0.4) < ENE * abs(e_plain)
        assert rc.fidelity_defect(bt[0].get_mps(), bt[1].get_mps()) < 1e-10
    finally:
        _close(bt)


# ---- 7. one launch ----
def test_relax_is_one_launch_and_bitwise_what_the_steps_give():
    from helpers import relax_cases as rc

    dims, D, seeds = rc.PARITY["L8d2D4"]
    items = _heis(dims, D, seeds[:3])
    a, b, c = _batch(items), _batch(items), _batch(items)
    try:
        a.propagate(0.0, 6)
        out = b.relax(6, 0.0)
        assert list(out["steps"]) == [6, 6, 6]
        assert not np.isnan(out["history"]).any()
        assert np.array_equal(out["history"][:, -1], out["energy"])
        for x, y in zip(_tensors(a), _tensors(b)):
            assert _same(x, y)
        # the first call builds the right blocks with the engines' own launches; from a state that has them the whole
        # relaxation is ONE launch
        c.relax(1)
        n0 = c.launches()
        c.relax(5)
        assert c.launches() - n0 == 1
        for x, y in zip(_tensors(a), _tensors(c)):
            assert _same(x, y)
    finally:
        _close(a)
        _close(b)
        _close(c)


def test_replicas_stop_on_their_own():
    """conv_tol = 1e-9 on five disorder realisations that the oracle converges after 3 to 8 steps: the step counts differ,
    every replica is bitwise what the same number of single steps gives, the history is NaN behind the stop and does not
    rise before it.  (All replicas of a batch share one shape, so the full-bond chain has a batch of its own below.)"""
    from helpers import relax_cases as rc

    dims, D, seeds = rc.PARITY["L8d2D4"]
    items = _heis(dims, D, seeds)
    maxstep = 12
    bt = _batch(items)
    try:
        out = bt.relax(maxstep, 1e-9)
        steps = [int(x) for x in out["steps"]]
        print("steps", steps, "energies", out["energy"])
        assert bt.statuses == [0] * len(items)
        assert len(set(steps)) > 1 and min(steps) >= 2 and max(steps) < maxstep
        for r in range(len(items)):
            h = out["history"][r]
            n = steps[r]
            assert np.isnan(h[n:]).all() and not np.isnan(h[:n]).any()
            assert h[n - 1] == out["energy"][r]
            assert all(h[i + 1] - h[i] <= 1e-12 * abs(h[i]) for i in range(n - 1))
            assert abs(h[n - 1] - h[n - 2]) <= 1e-9 and all(abs(h[i + 1] - h[i]) > 1e-9 for i in range(n - 2))
        got = _tensors(bt)
        for r, it in enumerate(items):
            one = _batch([it])
            try:
                one.propagate(0.0, steps[r])
                assert _same(one[0].get_mps(), got[r])
            finally:
                _close(one)
    finally:
        _close(bt)


def test_full_bond_replicas_reach_the_dense_ground_energy():
    """L = 6, d = 2, D = 8: the bonds hold every state, the first step is exact and the second stops the replica"""
    from helpers import relax_cases as rc

    dims, D = rc.FULL_BOND
    seeds = (0, 1, 2)
    bt = _batch(_heis(dims, D, seeds))
    try:
        out = bt.relax(8, 1e-9)
        print("steps", out["steps"], "energies", out["energy"])
        assert list(out["steps"]) == [2, 2, 2]  # converged after step 2 at the latest, and a stop needs two energies
        for r, s in enumerate(seeds):
            assert abs(out["energy"][r] - rc.dense_spectrum("heis", dims, s)[0]) < 1e-10
            assert np.isnan(out["history"][r, 2:]).all()
    finally:
        _close(bt)


# ---- 8. more replicas than compute units ----
def test_more_replicas_than_compute_units():
    from helpers import relax_cases as rc

    dims, D = rc.MANY
    B = 300
    items = [(rc.heisenberg_mpo(dims, s % 7), rc.start(dims, D, s)) for s in range(B)]
    pick = [0, 149, 299]
    big, small = _batch(items), _batch([items[r] for r in pick])
    try:
        big.relax(2)
        small.relax(2)
        assert big.statuses == [0] * B
        for j, r in enumerate(pick):
            assert _same(big[r].get_mps(), small[j].get_mps())
    finally:
        _close(big)
        _close(small)


# ---- 9. not converged is a status ----
def test_the_cap_must_be_equal_across_replicas():
    from helpers import relax_cases as rc

    dims, D, seeds = rc.PARITY["L6d3D6"]
    items = _heis(dims, D, seeds[:2])
    from pytdscf_amd import TDVPBatch

    bt = TDVPBatch.from_engines([_engine(*items[0]), _engine(*items[1], max_diag_krylov=4)])
    try:
        with pytest.raises(Exception, match=r"replica 1 differs from replica 0 in max_diag_krylov \(4 against 64\)"):
            bt.propagate(0.0, 1)
    finally:
        _close(bt)


def test_not_converged_is_a_status_with_the_engines_message():
    from helpers import relax_cases as rc

    dims, D, seeds = rc.PARITY["L6d3D6"]
    bt = _batch(_heis(dims, D, seeds[:2]), max_diag_krylov=4)
    try:
        with pytest.raises(ValueError, match="Lanczos Diagonalization is not converged in 4 basis"):
            bt.relax(2)
        from pytdscf_amd import _lib

        assert bt.statuses == [_lib.ENOTCONV] * 2
    finally:
        _close(bt)


def test_easy_replicas_finish_next_to_ones_that_do_not_converge():
    """dims (3,) * 5, D = 4, at most 4 Krylov vectors.  Easy: the field-only Hamiltonian (in the bond-5 form, so that it
    shares a batch) from a Hartree product zero-padded to the bonds -- its local Krylov spaces have d = 3 dimensions.
    Hard: the Heisenberg chain from a full-rank start."""
    from helpers import relax_cases as rc
    from pytdscf_amd import _lib

    dims, D = (3,) * 5, 4
    items = []
    for r in range(4):
        if r % 2 == 0:
            items.append((rc.field_mpo_wide(dims, r), rc.product_start(dims, D, r)))
        else:
            items.append((rc.heisenberg_mpo(dims, r), rc.start(dims, D, r)))
    bt = _batch(items, max_diag_krylov=4)
    try:
        with pytest.raises(ValueError, match="Lanczos Diagonalization is not converged in 4 basis"):
            bt.relax(2)
        print("statuses", bt.statuses, "energies", bt.relaxed["energy"])
        assert bt.statuses == [0, _lib.ENOTCONV, 0, _lib.ENOTCONV]
        for r in (0, 2):
            assert abs(bt.relaxed["energy"][r] - rc.field_ground_energy(dims, r)) < 1e-12
            assert bt.relaxed["steps"][r] == 2
    finally:
        _close(bt)


# ---- 10. records during a relaxation ----
def test_records_during_a_relaxation():
    from helpers import relax_cases as rc

    dims, D, seeds = rc.PARITY["L8d2D4"]
    items = _heis(dims, D, seeds[:3])
    a, b = _batch(items), _batch(items)
    try:
        rec = a.propagate(0.0, 4, observe=dict(energy=True))
        out = b.relax(4)
        e = np.real(rec["energy"])  # (5, B): before step 0 and after every step
        print("recorded", e[1:].T, "history", out["history"])
        assert e.shape[0] == 5
        for r in range(3):
            for n in range(4):
                assert abs(e[n + 1, r] - out["history"][r, n]) < ENE * abs(out["history"][r, n])
    finally:
        _close(a)
        _close(b)


# ---- 11. relax_trajectories ----
def test_relax_trajectories_feeds_correlation_function():
    from helpers import relax_cases as rc
    from pytdscf_amd import Exciton, Model, TensorHamiltonian, correlation_function, relax_trajectories

    dims, D = rc.FULL_BOND
    n = len(dims)
    models = []
    for s in (0, 1, 2):
        mpo = rc.heisenberg_mpo(dims, s)
        m = Model([Exciton(nstate=2) for _ in range(n)], operators={"hamiltonian": mpo}, bond_dim=D)
        models.append(m)
    out = relax_trajectories(models, starts=[rc.start(dims, D, s) for s in (0, 1, 2)], maxstep=6, conv_tol=1e-11)
    print("steps", out["steps"], "energies", out["energy"])
    for r, s in enumerate((0, 1, 2)):
        assert abs(out["energy"][r] - rc.dense_spectrum("heis", dims, s)[0]) < 1e-10
    # the default start, each model's own Hartree product padded to the bonds: variational, and a batch like the other
    dflt = relax_trajectories(models, maxstep=6, conv_tol=1e-11)
    print("default starts: steps", dflt["steps"], "energies", dflt["energy"])
    for r, s in enumerate((0, 1, 2)):
        assert dflt["energy"][r] >= rc.dense_spectrum("heis", dims, s)[0] - 1e-10
        assert abs(rc.orc.overlap(dflt["states"][r], dflt["states"][r]) - 1) < 1e-10
    assert len(out["states"]) == 3 and [c.shape for c in out["states"][0]] == [c.shape for c in rc.start(dims, D, 0)]
    cf = correlation_function(models[0], [out["states"][0]], maxstep=2, stepsize=0.01)
    assert abs(cf["mean"][0] - 1.0) < 1e-10
