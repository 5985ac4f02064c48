"""GPU: excited states of a batch by deflation against stored states (TDVPBatch.deflate_push / _clear / _count /
_overlaps, mitdvp_batch_deflate_*: k_batch_relax_defl solves every local problem on H_eff + sum_k w_k |q_k><q_k|, q_k the
stored state k in the replica's site basis, one workgroup per replica) and trajectories.relax_trajectories(nstates=).

The inputs are the disordered Heisenberg chains of helpers/relax_cases with the case table of helpers/deflate_oracle:
tests/test_batch_deflate_host.py shows on the CPU that the method, restated in NumPy, reaches states 0 .. 3 of the
full-bond chains to 2e-14 in two steps with at most 45 vectors per local solve.  The bars: 1e-9 on energies and
overlaps against the dense spectrum (four steps on the device), and for the truncated chain the existing relax bars
(fidelity defect 1e-10, energy 1e-8 |E|) or 100 x the model's own sensitivity to 1e-14 noise on the stored state, where
that is larger.

Measured on an MI355X (profiles/batch_deflate_tests.txt has the run): see that file."""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FID, ENE = 1e-10, 1e-8
W = 4.0


def _engine(mpo, cores, **kw):
    from pytdscf_amd import TDVPEngine

    e = TDVPEngine(len(mpo), relax="improved", **kw)
    e.set_mpo(mpo)
    e.set_mps(cores)
    return e


def _batch(items, **kw):
    """items: [(mpo, cores)], one engine each with its own Hamiltonian"""
    from pytdscf_amd import TDVPBatch

    return TDVPBatch.from_engines([_engine(*it, **kw) for it in items])


def _close(bt):
    engines = list(bt.engines)
    bt.close()
    for e in engines:
        e.close()


def _tensors(bt):
    return [e.get_mps() for e in bt.engines]


def _same(a, b):
    return all(np.array_equal(x, y) for s, t in zip(a, b) for x, y in zip(s, t))


def _fresh(bt, dims, D, seeds, k):
    """the fresh start of state k in every replica"""
    from helpers import deflate_oracle as do

    for e, s in zip(bt.engines, seeds):
        e.set_mps(do.state_start(dims, D, s, k))


def _energies(bt):
    return bt.observe(norm=False, energy=True)["energy"].real


def _states(bt, dims, D, seeds, nstates, maxstep, weights=W, after_ground=None):
    """push / fresh start / relax; returns (energies [k][r], the overlaps with the stored states after every state); what
    after_ground() returns right behind state 0 is appended to the overlaps"""
    seen = []
    energies, overlaps = [], []
    for k in range(nstates):
        if k:
            bt.deflate_push(weights)
            _fresh(bt, dims, D, seeds, k)
        bt.relax(maxstep)
        assert bt.statuses == [0] * len(seeds)
        energies.append(_energies(bt))
        overlaps.append(bt.deflate_overlaps())
        if k == 0 and after_ground is not None:
            seen.append(after_ground())
    return np.array(energies), overlaps + seen


# ---- 1. an empty set is bitwise off ----
def test_an_emptied_set_changes_no_bit_and_no_launch():
    from helpers import relax_cases as rc

    dims, D = rc.FULL_BOND
    seeds = (0, 1, 2)
    items = [(rc.heisenberg_mpo(dims, s), rc.start(dims, D, s)) for s in seeds]
    plain, cleared = _batch(items), _batch(items)
    try:
        cleared.deflate_push(W)
        assert cleared.deflate_count() == 1
        cleared.deflate_clear()
        assert cleared.deflate_count() == 0 and cleared.deflate_overlaps().shape == (0, 3)
        outs, launches = [], []
        for bt in (plain, cleared):
            for e in bt.engines:
                e.counters_reset()
            outs.append(bt.relax(2))
            launches.append([e.counters()["n_launch"] for e in bt.engines])
        assert launches[0] == launches[1]
        assert launches[0][0] == launches[0][1] + 1  # the one launch of the batch beside every engine's own block builds
        assert _same(_tensors(plain), _tensors(cleared))
        for key in ("energy", "steps", "history"):
            assert outs[0][key].tobytes() == outs[1][key].tobytes()
    finally:
        _close(plain)
        _close(cleared)


# ---- 2. the dense spectrum ----
def _full_groups():
    from helpers import deflate_oracle as do

    return [(dims, D, seeds) for dims, D, seeds in do.FULL]


@pytest.mark.parametrize("dims,D,seeds", _full_groups())
def test_four_states_match_the_dense_spectrum(dims, D, seeds):
    from helpers import deflate_oracle as do
    from helpers import relax_cases as rc

    bt = _batch([(rc.heisenberg_mpo(dims, s), rc.start(dims, D, s)) for s in seeds])
    try:
        energies, overlaps = _states(bt, dims, D, seeds, do.NSTATES, 4)
        assert bt.deflate_count() == do.NSTATES - 1
        for r, s in enumerate(seeds):
            exact = rc.dense_spectrum("heis", dims, s)[: do.NSTATES]
            de = np.abs(energies[:, r] - exact)
            ov = max(float(np.abs(o[:, r]).max()) for o in overlaps[1:])
            print(f"{dims} D {D} seed {s}: |<H> - E_k| {de}, largest overlap with a stored state {ov:.2e}")
            assert np.all(de < 1e-9)
            assert ov < 1e-9
        assert overlaps[0].shape == (0, len(seeds)) and overlaps[-1].shape == (do.NSTATES - 1, len(seeds))
    finally:
        _close(bt)


# ---- 3. parity with the NumPy model on a truncated chain ----
@functools.lru_cache(maxsize=None)
def _model_state1(seed, noise):
    from helpers import deflate_oracle as do
    from helpers import relax_cases as rc

    dims, D, _ = do.TRUNCATED
    mpo = rc.heisenberg_mpo(dims, seed)
    ground = do.run_states(mpo, dims, D, seed, nstates=1, nsteps=3)["cores"][0]
    stored = do.noisy(ground, noise) if noise else ground
    m = do.DeflatedRelax(do.state_start(dims, D, seed, 1), mpo, [(stored, W)])
    for _ in range(3):
        m.step()
    return ground, m.cores, m.energy()


def test_state_one_of_a_truncated_chain_against_the_model():
    from helpers import deflate_oracle as do
    from helpers import relax_cases as rc

    dims, D, seeds = do.TRUNCATED
    bt = _batch([(rc.heisenberg_mpo(dims, s), _model_state1(s, 0.0)[0]) for s in seeds])
    try:
        bt.deflate_push(W)
        _fresh(bt, dims, D, seeds, 1)
        bt.relax(3)
        assert bt.statuses == [0] * len(seeds)
        got = _energies(bt)
        for r, s in enumerate(seeds):
            _, cores, energy = _model_state1(s, 0.0)
            _, cores_n, energy_n = _model_state1(s, 1e-14)
            sens_f = rc.fidelity_defect(cores, cores_n)
            sens_e = abs(energy - energy_n) / abs(energy)
            fid = rc.fidelity_defect(cores, bt[r].get_mps())
            de = abs(got[r] - energy) / abs(energy)
            bar_f, bar_e = max(FID, 100 * sens_f), max(ENE, 100 * sens_e)
            print(f"seed {s}: model sensitivity to 1e-14 noise: fidelity {sens_f:.2e}, |dE/E| {sens_e:.2e}; device: fidelity defect "
                  f"{fid:.2e} (bar {bar_f:.2e}), |dE/E| {de:.2e} (bar {bar_e:.2e})")
            assert fid < bar_f
            assert de < bar_e
    finally:
        _close(bt)


# ---- 4. deflate_overlaps ----
def test_overlaps_with_several_slots_of_random_states():
    from helpers import relax_cases as rc
    from oracle import tdvp_oracle as orc

    dims, D = (2, 3, 2, 3, 2), 12
    B, K = 3, 5
    mpo = rc.heisenberg_mpo(dims, 0)
    bt = _batch([(mpo, rc.start(dims, D, r)) for r in range(B)])
    try:
        stored = []
        for k in range(K):
            cores = [rc.start(dims, D, 50 + 7 * k + r) for r in range(B)]
            for e, c in zip(bt.engines, cores):
                e.set_mps(c)
            bt.deflate_push(1.0 + k)
            stored.append(cores)
        now = [rc.start(dims, D, 200 + r) for r in range(B)]
        for e, c in zip(bt.engines, now):
            e.set_mps(c)
        before = _tensors(bt)
        got = bt.deflate_overlaps()
        assert got.shape == (K, B) and _same(before, _tensors(bt))
        ref = np.array([[orc.overlap(stored[k][r], now[r]) for r in range(B)] for k in range(K)])
        print("largest |overlap - reference|", np.abs(got - ref).max(), "largest |overlap|", np.abs(ref).max())
        assert np.abs(got - ref).max() < 1e-12
    finally:
        _close(bt)


# ---- 5. restarts under deflation ----
def test_restarts_under_deflation():
    from helpers import deflate_oracle as do
    from helpers import relax_cases as rc

    dims, D, seeds = do.FULL[1]
    bt = _batch([(rc.heisenberg_mpo(dims, s), rc.start(dims, D, s)) for s in seeds], max_diag_krylov=8)
    try:
        bt.set_relax_restarts(64)
        energies, overlaps = _states(bt, dims, D, seeds, do.NSTATES, 4, after_ground=lambda: bt.relax_restarts()["total"].copy())
        ground, rst = overlaps.pop(), bt.relax_restarts()
        print("restarts of state 0", ground, "of all four states", rst["total"], "most of one solve", rst["most"])
        assert (rst["total"] > ground).all()  # the deflated solves of states 1 .. 3 restart too
        for r, s in enumerate(seeds):
            exact = rc.dense_spectrum("heis", dims, s)[: do.NSTATES]
            de = np.abs(energies[:, r] - exact)
            ov = max(float(np.abs(o[:, r]).max()) for o in overlaps[1:])
            print(f"seed {s}: |<H> - E_k| {de}, largest overlap with a stored state {ov:.2e}")
            assert np.all(de < 1e-9)
            assert ov < 1e-9
    finally:
        _close(bt)


# ---- 6. one launch equals single steps ----
def test_one_launch_equals_single_steps():
    from helpers import deflate_oracle as do
    from helpers import relax_cases as rc

    dims, D, seeds = do.TRUNCATED
    items = [(rc.heisenberg_mpo(dims, s), _model_state1(s, 0.0)[0]) for s in seeds]
    one, single = _batch(items), _batch(items)
    try:
        deltas = []
        for bt in (one, single):
            bt.deflate_push(W)
            _fresh(bt, dims, D, seeds, 1)
            for e in bt.engines:
                e.counters_reset()
            if bt is one:
                bt.relax(3, 0.0)
            else:
                for _ in range(3):
                    bt.propagate(0.0, 1)
            assert bt.statuses == [0] * len(seeds)
            deltas.append([e.counters()["n_launch"] for e in bt.engines])
        builds = deltas[0][1]  # replica 1 counts only its own block builds
        assert deltas[1][1] == builds
        assert deltas[0][0] == builds + 1 and deltas[1][0] == builds + 6
        for r in range(len(seeds)):
            fid = rc.fidelity_defect(one[r].get_mps(), single[r].get_mps())
            print(f"replica {r}: fidelity defect between one launch and six {fid:.2e}")
            assert fid < 1e-12
    finally:
        _close(one)
        _close(single)


# ---- 7. batch independence ----
def test_a_replicas_bits_do_not_depend_on_the_batch():
    from helpers import deflate_oracle as do
    from helpers import relax_cases as rc

    dims, D = rc.MANY
    seeds_of = lambda n: [r % 4 for r in range(n)]  # noqa: E731

    def run(n):
        seeds = seeds_of(n)
        bt = _batch([(rc.heisenberg_mpo(dims, s), rc.start(dims, D, 30 + r)) for r, s in enumerate(seeds)])
        try:
            bt.relax(2)
            bt.deflate_push(W)
            for r, e in enumerate(bt.engines):
                e.set_mps(do.state_start(dims, D, 60 + r, 1))
            bt.relax(2)
            assert bt.statuses == [0] * n
            return _tensors(bt), _energies(bt)
        finally:
            _close(bt)

    small, e_small = run(6)
    big, e_big = run(70)
    assert _same(small, big[:6])
    for r in range(70):
        exact = rc.dense_spectrum("heis", dims, r % 4)[1]
        assert abs(e_big[r] - exact) < 1e-9
    assert e_small.tobytes() == e_big[:6].tobytes()


# ---- 8. weights per replica ----
def test_weights_per_replica():
    from helpers import deflate_oracle as do
    from helpers import relax_cases as rc

    dims, D, seed = do.SMALL_GAP
    exact = rc.dense_spectrum("heis", dims, seed)
    bt = _batch([(rc.heisenberg_mpo(dims, seed), rc.start(dims, D, seed))] * 2)
    try:
        bt.relax(4)
        bt.deflate_push([W, 0.01])
        _fresh(bt, dims, D, (seed, seed), 1)
        bt.relax(4)
        e = _energies(bt)
        ov = np.abs(bt.deflate_overlaps()[0])
        print(f"gap {exact[1] - exact[0]:.3f}: weight 4 reaches {e[0]:.12f} (E_1 {exact[1]:.12f}), weight 0.01 reaches {e[1]:.12f} "
              f"(E_0 {exact[0]:.12f}); overlaps with the stored state {ov}")
        assert abs(e[0] - exact[1]) < 1e-9 and ov[0] < 1e-9
        assert abs(e[1] - exact[0]) < 1e-3 and ov[1] > 0.99
    finally:
        _close(bt)


# ---- 9. refusals ----
def test_refusals_leave_the_set_and_the_replicas_as_they_were():
    from helpers import relax_cases as rc
    from pytdscf_amd import TDVPBatch, TDVPEngine

    dims, D = rc.MANY
    items = [(rc.heisenberg_mpo(dims, s), rc.start(dims, D, s)) for s in (0, 1, 2)]
    bt = _batch(items)
    try:
        before = _tensors(bt)
        for bad, who in (([W, float("nan"), W], "replica 1"), ([W, W, 0.0], "replica 2"), ([-1.0, W, W], "replica 0")):
            with pytest.raises(ValueError, match=f"mitdvp_batch_deflate_push: {who} has weight .* finite and > 0"):
                bt.deflate_push(bad)
            assert bt.deflate_count() == 0 and _same(before, _tensors(bt))
        with pytest.raises(ValueError, match="weights for 3 replicas"):
            bt.deflate_push([W, W])
        assert bt.deflate_count() == 0 and _same(before, _tensors(bt))
        bt.sweep(0.0, True)  # leaves the centre at the last site
        moved = _tensors(bt)
        with pytest.raises(ValueError, match="mitdvp_batch_deflate_push: replica 0 has its centre at site 3"):
            bt.deflate_push(W)
        assert bt.deflate_count() == 0 and _same(moved, _tensors(bt))
        bt.sweep(0.0, False)
        for k in range(8):
            bt.deflate_push(W)
            assert bt.deflate_count() == k + 1
        kept = _tensors(bt)
        with pytest.raises(ValueError, match="mitdvp_batch_deflate_push: the set holds 8 states, a batch keeps at most 8"):
            bt.deflate_push(W)
        assert bt.deflate_count() == 8 and _same(kept, _tensors(bt))
        assert bt.deflate_overlaps().shape == (8, 3)
        bt.deflate_clear()
        assert bt.deflate_count() == 0
    finally:
        _close(bt)
    engines = []
    for mpo, cores in items[:2]:
        e = TDVPEngine(len(mpo))  # real time: relax is not 2
        e.set_mpo(mpo)
        e.set_mps(cores)
        engines.append(e)
    rt = TDVPBatch.from_engines(engines)
    try:
        with pytest.raises(ValueError, match="mitdvp_batch_deflate_push: the replicas have relax = 0.*relax must be 2"):
            rt.deflate_push(W)
        assert rt.deflate_count() == 0 and _same([c for _, c in items[:2]], _tensors(rt))
    finally:
        _close(rt)


# ---- 10. relax_trajectories ----
def test_relax_trajectories_finds_three_states():
    from helpers import relax_cases as rc
    from pytdscf_amd import Exciton, Model, relax_trajectories

    dims, D = rc.FULL_BOND
    seeds = (0, 1, 2)
    models = [Model([Exciton(nstate=2) for _ in range(len(dims))], operators={"hamiltonian": rc.heisenberg_mpo(dims, s)}, bond_dim=D)
              for s in seeds]
    starts = [rc.start(dims, D, s) for s in seeds]
    plain = relax_trajectories(models, starts=starts, maxstep=6, conv_tol=1e-11)
    assert set(plain) == {"energy", "steps", "history", "states"}
    again = relax_trajectories(models, starts=starts, maxstep=6, conv_tol=1e-11, nstates=1)
    for key in ("energy", "steps", "history"):
        assert plain[key].tobytes() == again[key].tobytes()
    assert _same(plain["states"], again["states"])
    with pytest.raises(ValueError, match="nstates > 1 needs penalty"):
        relax_trajectories(models, starts=[starts, None, None], nstates=3)
    out = relax_trajectories(models, starts=[starts, None, None], maxstep=6, conv_tol=1e-12, nstates=3, penalty=4.0, seed=5)
    assert set(out) == {"energy", "steps", "history", "states", "energies", "overlaps"}
    assert out["energies"].shape == (3, 3) and out["overlaps"].shape == (3, 3, 3) and out["overlaps"].dtype == np.complex128
    assert len(out["states"]) == 3 and all(len(s) == 3 for s in out["states"])
    assert all(c.shape == p.shape for c, p in zip(out["states"][2][1], plain["states"][1]))
    for r, s in enumerate(seeds):
        exact = rc.dense_spectrum("heis", dims, s)[:3]
        de = np.abs(out["energies"][:, r] - exact)
        off = np.abs(out["overlaps"][:, :, r] - np.eye(3)).max()
        print(f"seed {s}: |<H> - E_k| {de}, largest |overlap - identity| {off:.2e}")
        assert np.all(de < 1e-9)
        assert off < 1e-9
