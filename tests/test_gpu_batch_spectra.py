"""GPU: bond spectra and entanglement entropies of the batched trajectories (TDVPBatch.set_spectra / spectra,
propagate(observe=dict(spectra=True)): k_batch_spectra forms every requested bond of every replica with one launch,
k_batch_mean averages on the device) and propagate_trajectories(entanglement=[...]).

The pin is the SVD of the dense state built from the tensors the engines hand back: squared Schmidt values to 1e-12 W;
S1, S2 and pmin inside chi delta (1 + |ln delta|) at delta = 1e-12 (helpers/spectra_cases.entropy_bar, derived there and
shown on perturbed spectra in tests/test_batch_spectra_host.py).  Every case prints its worst defect as a fraction of its
bar.  The shapes are the smallest at which each part can go wrong:
  mixed  dims (2, 3, 2, 4, 2), D = 6: bonds 2, 6, 6, 2 -- ragged physical dimensions, a bond narrower than the tile
  odd    dims (3,) * 5, D = 7: bonds 3, 7, 7, 3 -- every bond odd: the resting player of the round-robin Jacobi schedule
  wide   dims (2,) * 12, D = 40: bonds up to 40 -- past the 32-wide tile and the 16-deep K step, a multiple of neither;
         dl d = 80 rows in the QR, more than one wave's worth."""

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
    """B replicas with random states of norms 0.7, 0.9, 1.1, ...; no rescaling in a step, so the norms stay apart"""
    from helpers import spectra_cases as sc
    from pytdscf_amd import TDVPBatch

    dims, D = sc.SHAPES[name]
    kw = dict(dict(integrator="arnoldi", conserve_norm=False), **kw)
    bt = TDVPBatch(B, len(dims), **kw)
    bt.set_mpo(_mpo(name, dims))
    for e, cores in zip(bt.engines, states if states is not None else sc.random_states(dims, D, B, seed)):
        e.set_mps(cores)
    return bt


def _tensors(bt):
    return [e.get_mps() for e in bt.engines]


def _same_tensors(a, b):
    return all(np.array_equal(x, y) for s, t in zip(a, b) for x, y in zip(s, t))


@pytest.mark.parametrize("name", ["mixed", "odd", "wide"])
def test_values_equal_the_dense_svd(name):
    """random states of different norms, one propagation step, all bonds and a sub-list that stops before the last one"""
    from helpers import spectra_cases as sc

    dims, D = sc.SHAPES[name]
    L, B = len(dims), 3
    bt = _batch(name, B)
    bt.propagate(DT, 1)
    now = _tensors(bt)
    assert max(c.shape[2] for c in now[0]) == D
    bt.set_spectra(range(L - 1))
    full = bt.spectra()
    n2 = bt.observe()["norm"] ** 2
    assert full["entropy"].shape == full["renyi2"].shape == full["min_weight"].shape == full["norm2"].shape == (B, L - 1)
    assert full["mean_entropy"].shape == (L - 1,) and len(full["weights"]) == len(full["mean_weights"]) == L - 1
    worst_w = worst_s = worst_n = 0.0
    least = 1.0
    for q in range(L - 1):
        chi = now[0][q].shape[2]
        assert full["weights"][q].shape == (B, chi) and full["mean_weights"][q].shape == (chi,)
        bar = sc.entropy_bar(chi, 1e-12)
        for r in range(B):
            want = sc.dense_weights(now[r], q)
            W = want.sum()
            got = full["weights"][q][r]
            assert np.all(np.diff(got) <= 0)
            worst_w = max(worst_w, np.abs(got - want).max() / (1e-12 * W))
            least = min(least, want.min() / W)
            ent = np.array([full["entropy"][r, q], full["renyi2"][r, q], full["min_weight"][r, q]])
            worst_s = max(worst_s, np.abs(ent - sc.entropies(want)).max() / bar)
            worst_n = max(worst_n, abs(full["norm2"][r, q] - n2[r]) / (1e-12 * n2[r]))
    print(f"{name}: sigma^2 {worst_w:.3f} of 1e-12 W; S1, S2, pmin {worst_s:.3f} of chi delta (1 + |ln delta|); "
          f"W against observe() {worst_n:.3f} of 1e-12; smallest weight compared {least:.1e} W")
    assert worst_w < 1 and worst_s < 1 and worst_n < 1
    assert np.abs(n2 - [0.49, 0.81, 1.21]).max() < 1e-6  # different norms, kept by a Hermitian operator
    assert full["entropy"].min() > 0.01  # nothing here is the entropy of a product state
    for k in ("entropy", "renyi2", "min_weight", "norm2"):
        assert np.abs(full["mean_" + k] - full[k].mean(axis=0)).max() < 1e-13 * np.abs(full[k]).max()
    sub = [1, L - 3]
    bt.set_spectra(sub)
    part = bt.spectra(per_replica=True)
    assert part["entropy"].shape == (B, 2)
    for k, q in enumerate(sub):  # the same walk, cut short: the same bits
        assert np.array_equal(part["weights"][k], full["weights"][q]) and np.array_equal(part["entropy"][:, k], full["entropy"][:, q])
    assert set(bt.spectra(per_replica=False)) == {"mean_norm2", "mean_entropy", "mean_renyi2", "mean_min_weight", "mean_weights"}
    bt.close()


def test_known_answers_bell_pairs_and_a_padded_product():
    """Bell pairs on (0, 1), (2, 3), (4, 5) zero-padded to D = 4: S1 = ln 2 on even bonds and 0 on odd ones; the equal
    singular values make a == b in the rotation.  A Hartree product zero-padded to D (the start propagate_trajectories
    builds): rank 1, zero columns in the QR, rows at the `tiny` rule in the Jacobi: spectrum (W, 0, ...) to 1e-12 W."""
    from helpers import pair_cases as pc
    from helpers import spectra_cases as sc
    from pytdscf_amd import TDVPBatch

    bt = TDVPBatch(2, 6, integrator="arnoldi", conserve_norm=False)
    bt.set_mpo(pc._spin_chain_mpo(6))
    for e, scale in zip(bt.engines, (1.0, 0.6)):
        e.set_mps(sc.bell_chain(6, 4), canonicalize=True, scale=scale)
    assert [c.shape[2] for c in bt[0].get_mps()] == [2, 4, 4, 4, 2, 1]
    bt.set_spectra(range(5))
    got = bt.spectra()
    worst = 0.0
    for q in range(5):
        chi = [2, 4, 4, 4, 2][q]
        want = np.zeros(chi)
        want[:2 if q % 2 == 0 else 1] = 0.5 if q % 2 == 0 else 1.0
        for r, W in enumerate((1.0, 0.36)):
            worst = max(worst, np.abs(got["weights"][q][r] - W * want).max() / (1e-12 * W), abs(got["norm2"][r, q] - W) / (1e-12 * W),
                        abs(got["entropy"][r, q] - (np.log(2) if q % 2 == 0 else 0.0)) / sc.entropy_bar(chi, 1e-12))
    print(f"Bell chain: worst defect {worst:.3f} of its bar")
    assert worst < 1
    bt.close()

    dims, D = sc.SHAPES["mixed"]
    bt = TDVPBatch(2, len(dims), integrator="arnoldi", conserve_norm=False)
    bt.set_mpo(_mpo("mixed", dims))
    for e, scale in zip(bt.engines, (1.0, 1.3)):
        e.set_mps(sc.product_padded(dims, D), canonicalize=True, scale=scale)
    bt.set_spectra(range(len(dims) - 1))
    got = bt.spectra()
    worst = 0.0
    for q in range(len(dims) - 1):
        for r, W in enumerate((1.0, 1.69)):
            w = got["weights"][q][r]
            worst = max(worst, abs(w[0] - W) / (1e-12 * W), np.abs(w[1:]).max() / (1e-12 * W), got["entropy"][r, q] / 1e-10)
            assert got["min_weight"][r, q] < 1e-12
    print(f"padded product: worst defect {worst:.3f} of its bar")
    assert worst < 1
    bt.close()


def test_dynamics_against_dense_expm():
    """L = 6 spin chain at full bond dimension (D = 8, Arnoldi at 1e-10), 4 steps: the entropies of every record against
    the dense expm state, within the bar fixed from thresh_sil and the step count (spectra_cases.dyn_bar: 2.7e-6), which
    the NumPy oracle keeps with a factor of 1e6 to spare (tests/test_batch_spectra_host.py)."""
    from helpers import pair_cases as pc
    from helpers import spectra_cases as sc
    from pytdscf_amd import TDVPBatch

    bt = TDVPBatch(1, sc.DYN_L, integrator="arnoldi", conserve_norm=False, thresh=sc.DYN_THRESH)
    bt.set_mpo(pc._spin_chain_mpo(sc.DYN_L))
    bt[0].set_mps(sc.dyn_start())
    bt.set_spectra(range(sc.DYN_L - 1))
    rec = bt.propagate(sc.DYN_DT, sc.DYN_STEPS, observe=dict(norm=False, spectra=True))
    assert rec["entropy"].shape == (sc.DYN_STEPS + 1, 1, sc.DYN_L - 1)
    dev = np.abs(rec["entropy"][:, 0, :] - sc.dyn_dense()).max()
    print(f"dynamics: max |S1 - dense expm| = {dev:.2e} = {dev / sc.dyn_bar():.2e} of the bar {sc.dyn_bar():.2e}")
    assert dev < sc.dyn_bar()
    assert np.abs(rec["entropy"][-1] - rec["entropy"][0]).max() > 0.01
    bt.close()


def test_an_observation_changes_nothing():
    from helpers import spectra_cases as sc

    dims, _ = sc.SHAPES["mixed"]
    bt = _batch("mixed", 3)
    bt.propagate(DT, 1)
    bt.set_spectra(range(len(dims) - 1))
    before = _tensors(bt)
    bt.spectra()
    assert _same_tensors(before, _tensors(bt))
    bt.close()
    req = dict(sites=[1, 3], norm=True, autocorr=True, energy=True, keys=[(0, 0, 2, 2)])
    out = []
    for with_spectra in (False, True):
        bt = _batch("mixed", 3)
        if with_spectra:
            bt.set_spectra([0, 2])
        rec = bt.propagate(DT, 2, observe=dict(req, spectra=True) if with_spectra else req, every=1)
        out.append((rec, _tensors(bt)))
        bt.close()
    (a, ta), (b, tb) = out
    assert _same_tensors(ta, tb)
    assert set(b) - set(a) == {"entropy", "renyi2", "min_weight", "norm2", "weights", "mean_entropy", "mean_renyi2", "mean_min_weight",
                               "mean_weights"}
    assert b["entropy"].shape == (3, 3, 2)
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for x, y in zip(xs, ys):
            assert np.array_equal(x, y), k


def test_bits_do_not_depend_on_the_batch():
    """a replica's record at B = 1, at B = 5 and at another position in the list"""
    from helpers import spectra_cases as sc

    dims, D = sc.SHAPES["odd"]
    states = sc.random_states(dims, D, 5, seed=60)
    flat = lambda got, r: np.concatenate([got[k][r] for k in ("norm2", "entropy", "renyi2", "min_weight")] + [w[r] for w in got["weights"]])
    recs = []
    for order in ([2], [0, 1, 2, 3, 4], [4, 2, 0, 3, 1]):
        bt = _batch("odd", len(order), states=[states[i] for i in order])
        bt.set_spectra(range(len(dims) - 1))
        recs.append(flat(bt.spectra(), order.index(2)))
        if len(order) == 5:
            assert len({flat(bt.spectra(), r).tobytes() for r in range(5)}) == 5  # five different states, five records
        bt.close()
    assert np.array_equal(recs[0], recs[1]) and np.array_equal(recs[0], recs[2])
    assert recs[0].size == 4 * 4 + 3 + 7 + 7 + 3 and np.all(recs[0] > 0)


def test_a_recorded_run():
    from helpers import cross_cases as cc
    from helpers import spectra_cases as sc

    dims, _ = sc.SHAPES["mixed"]
    B = 3
    bt = _batch("mixed", B)
    bt.propagate(DT, 1)  # the engines build their right blocks with launches of their own on first use
    bt.set_spectra([0, 1, 3])
    n = bt.launches()
    first = bt.spectra()
    assert bt.launches() - n == 2
    n = bt.launches()
    rec = bt.propagate(DT, 4, observe=dict(norm=False, spectra=True), every=2)  # the request alone
    assert bt.launches() - n == 2 * 4 + 3 + 1
    last = bt.spectra()
    assert rec["entropy"].shape == (4 // 2 + 1, B, 3) and rec["mean_entropy"].shape == (3, 3)
    assert [w.shape for w in rec["weights"]] == [(3, B, 2), (3, B, 6), (3, B, 2)]
    for k in ("norm2", "entropy", "renyi2", "min_weight"):
        assert np.array_equal(rec[k][0], first[k]) and np.array_equal(rec[k][-1], last[k]) and np.array_equal(rec["mean_" + k][0], first["mean_" + k])
    assert all(np.array_equal(x[0], y) for x, y in zip(rec["weights"], first["weights"]))
    assert not np.array_equal(first["entropy"], last["entropy"])
    n = bt.launches()
    bt.propagate(DT, 4, observe=dict(norm=True, sites=[1, 2], spectra=True), every=2)  # with an observation of its own
    assert bt.launches() - n == 2 * 4 + 2 * 3 + 2
    bt.set_cross([(0, 1), (1, 2, 1, cc.random_op(3, 1))])
    n = bt.launches()
    both = bt.propagate(DT, 2, observe=dict(norm=True, sites=[1, 2], spectra=True, cross=True), every=1)  # and a cross request
    assert bt.launches() - n == 2 * 2 + 3 * 3 + 3
    assert both["cross"].shape == (3, 2) and both["entropy"].shape == (3, B, 3) and both["mean_norm2"].shape == (3,)
    bt.set_cross([])  # a request that is set rides on every record, asked for or not
    n = bt.launches()
    w = np.array([0.5, 0.2, 0.3])
    rw = bt.propagate(DT, 0, observe=dict(norm=False, spectra=True, spectra_weights=w))  # weights: one more mean launch
    assert bt.launches() - n == 2 + 1
    worst = 0.0
    for k in ("norm2", "entropy", "renyi2", "min_weight"):
        worst = max(worst, np.abs(rw["mean_" + k][0] - w @ rw[k][0]).max() / (1e-13 * np.abs(rw[k]).max()))
    for mw, ww in zip(rw["mean_weights"], rw["weights"]):
        worst = max(worst, np.abs(mw[0] - w @ ww[0]).max() / (1e-13 * np.abs(ww).max()))
    print(f"recorded run: weighted means {worst:.3f} of 1e-13")
    assert worst < 1
    assert np.abs(bt.spectra(weights=w)["mean_entropy"] - rw["mean_entropy"][0]).max() < 1e-13
    bt.close()


def test_the_request_survives_a_new_handle():
    from helpers import spectra_cases as sc

    dims, _ = sc.SHAPES["mixed"]
    bt = _batch("mixed", 3)
    bt.set_spectra([1, 2])
    a = bt.spectra()
    gone = bt.engines.pop(0)
    b = bt.spectra()  # the list of engines changed: the library's batch object is made anew and gets the request again
    assert b["entropy"].shape == (2, 2) and np.array_equal(b["entropy"], a["entropy"][1:])
    assert all(np.array_equal(x, y[1:]) for x, y in zip(b["weights"], a["weights"]))
    gone.close()
    bt.close()


def test_every_refusal_names_itself_and_changes_nothing():
    from helpers import spectra_cases as sc
    from pytdscf_amd import _lib

    dims, _ = sc.SHAPES["mixed"]
    L = len(dims)
    fresh = _batch("mixed", 2)
    with pytest.raises(ValueError, match="no spectra request"):
        fresh.spectra()
    with pytest.raises(ValueError, match="mitdvp_batch_spectra: no spectra request"):
        _lib.check(fresh._lib.mitdvp_batch_spectra(fresh._handle(), None, None, None, None))
    assert fresh._lib.mitdvp_batch_set_spectra(fresh._handle(), None, 0) == 0  # removing nothing is fine
    fresh.close()

    bt = _batch("mixed", 3)
    bt.propagate(DT, 1)
    bt.set_spectra([0, 2])
    before, n0, tensors = bt.spectra(), bt.launches(), _tensors(bt)
    bad = [([L - 1], rf"bond {L - 1} is out of range \(the chain has {L} sites, bonds 0 \.\. {L - 2}"),
           ([-1, 0], r"bond -1 is out of range"),
           ([0, 7], r"bond 7 is out of range"),
           ([2, 1], r"the bonds must be strictly ascending \(bond 1 follows bond 2\)"),
           ([1, 1], r"the bonds must be strictly ascending \(bond 1 follows bond 1\)")]
    for bonds, match in bad:
        with pytest.raises(ValueError, match="mitdvp_batch_set_spectra: " + match):
            bt.set_spectra(bonds)
    with pytest.raises(ValueError, match="spectra bonds"):
        bt.set_spectra([0.5])
    with pytest.raises(ValueError, match="one per replica"):
        bt.spectra(weights=[1.0])
    assert bt.launches() == n0
    after = bt.spectra()
    assert after["entropy"].shape == (3, 2) and np.array_equal(after["entropy"], before["entropy"])
    assert all(np.array_equal(x, y) for x, y in zip(after["weights"], before["weights"]))
    assert _same_tensors(tensors, _tensors(bt))
    bt.sweep(DT, True)  # the centre is at the last site now
    moved = _tensors(bt)
    with pytest.raises(ValueError, match=rf"mitdvp_batch_spectra: replica 0 has its centre at site {L - 1}"):
        bt.spectra()
    assert _same_tensors(moved, _tensors(bt))
    bt.sweep(DT, False)
    assert bt.spectra()["entropy"].shape == (3, 2)
    bt.set_spectra([])  # an empty list removes the request
    with pytest.raises(ValueError, match="no spectra request"):
        bt.spectra()
    with pytest.raises(ValueError, match="mitdvp_batch_spectra: no spectra request"):
        _lib.check(bt._lib.mitdvp_batch_spectra(bt._handle(), None, None, None, None))
    bt.close()


def test_a_record_beyond_the_limit_is_refused():
    """rec_len = sum of 4 + chi_q beyond 65536 doubles: a chain of 975 two-level sites at D = 64 has 65 716 for all of its
    bonds; the first 960 have 65 022 and are taken.  Nothing is launched: the request is only registered."""
    from pytdscf_amd import TDVPBatch
    from pytdscf_amd.mps import product_state_cores

    L, D = 975, 64
    bt = TDVPBatch(1, L)
    bt.set_mpo([np.diag([0.5, -0.5]).astype(complex).reshape(1, 2, 2, 1)] * L)
    bt[0].set_mps(product_state_cores([[1, 0]] * L, D))
    with pytest.raises(ValueError, match=r"mitdvp_batch_set_spectra: a replica's record would have 65716 doubles .* at most 65536"):
        bt.set_spectra(range(L - 1))
    bt.set_spectra(range(960))
    cnt = (C.c_size_t * 2)()
    assert bt._lib.mitdvp_batch_spectra(bt._handle(), None, None, None, cnt) == 0 and list(cnt) == [1, 65022]
    bt.close()


def test_propagate_trajectories_with_entanglement():
    """the dephasing spin chain: L = 6, D = 4, {sqrt(1 - g) 1, sqrt(g) sigma_z} on every site, two product starts x two
    replicas: shapes and times, the trajectory mean against the host mean of the per-trajectory values, and the keys of
    the result with and without the keyword"""
    from helpers import pair_cases as pc
    from pytdscf_amd import Exciton, Model, propagate_trajectories, units

    L, g = 6, 0.1
    deph = np.stack([np.sqrt(1 - g) * np.eye(2), np.sqrt(g) * np.diag([1.0, -1.0])]).astype(complex)
    model = Model([Exciton(nstate=2) for _ in range(L)], operators={"hamiltonian": pc._spin_chain_mpo(L)}, bond_dim=4)
    starts = [[[1, 0], [0, 1]] * (L // 2), [[1, 1], [1, -1]] * (L // 2)]  # Neel states along z and along x
    w = np.array([0.1, 0.2, 0.3, 0.4])
    kw = dict(maxstep=5, stepsize=0.4 * units.au_in_fs, reduced_density=([(1, 1)], 2), integrator="arnoldi", conserve_norm=False,
              jumps={p: deph for p in range(L)}, seed=3, replicas_per_start=2, weights=w, per_trajectory=True)
    base = propagate_trajectories(model, starts, **kw)
    out = propagate_trajectories(model, starts, entanglement=[0, 2, 4], **kw)
    assert set(base) == {"time", "mean", "trajectories"}
    assert set(out) == set(base) | {"entropy", "min_weight", "entropy_trajectories"}
    assert set(propagate_trajectories(model, starts, entanglement=[2], **dict(kw, per_trajectory=False))) == {"time", "mean", "entropy", "min_weight"}
    assert np.array_equal(out["time"], base["time"]) and np.allclose(out["time"], np.arange(3) * 2 * 0.4 * units.au_in_fs)
    assert np.array_equal(out["mean"][(1, 1)], base["mean"][(1, 1)]) and np.array_equal(out["trajectories"][(1, 1)], base["trajectories"][(1, 1)])
    assert out["entropy"].shape == out["min_weight"].shape == (3, 3) and out["entropy_trajectories"].shape == (3, 4, 3)
    dev = np.abs(out["entropy"] - np.einsum("r,qrb->qb", w, out["entropy_trajectories"])).max()
    print(f"front end: |device mean - host mean| = {dev:.2e}")
    assert dev < 1e-13
    assert np.abs(out["entropy_trajectories"][0]).max() < 1e-10  # product starts
    assert out["entropy_trajectories"][-1].min() > 1e-3  # the chain entangles them
    with pytest.raises(ValueError, match="entanglement names no bond"):
        propagate_trajectories(model, starts, entanglement=[], **kw)
