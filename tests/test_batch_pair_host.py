"""CPU: nearest-neighbour (pair) gates and jump channels of the batched trajectories -- the C surface is declared,
exported and loads; the two-site sampling rule with the split is an EXACT unravelling of the channel when nothing is
truncated (every branch enumerated, no statistics); propagate_trajectories parses and refuses pair keys before it creates
an engine; and the inputs of tests/test_gpu_batch_pair.py sit on no edge (decision margins, singular-value gaps), shown
from the NumPy oracle alone."""

import ctypes as C
import os

import numpy as np
import pytest

NAMES = ["mitdvp_batch_set_pair_channel", "mitdvp_batch_pair_jump_counts", "mitdvp_batch_discarded_weight"]


def test_pair_symbols_are_declared_exported_and_load():
    from pytdscf_amd import _lib

    declared = _lib.declared_symbols()
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    with open(os.path.join(os.path.dirname(_lib.__file__), "_lib.py")) as f:
        binding = f.read()
    for n in NAMES:
        assert n in declared and n in header
        assert f'"{n}"' in binding
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
    lib = _lib.load()
    assert lib.mitdvp_batch_set_pair_channel.argtypes[-3:] == [C.c_int] * 3
    assert lib.mitdvp_batch_set_pair_channel(None, 0, _lib.CHANNEL_GATE, None, 1, 2, 2) == _lib.EINVAL
    assert lib.mitdvp_batch_pair_jump_counts(None, None) == _lib.EINVAL
    assert lib.mitdvp_batch_discarded_weight(None, None) == _lib.EINVAL


def test_pair_key():
    from pytdscf_amd.engine import pair_key

    assert pair_key((2, 3), 6) == (2, 3) and pair_key([0, 1], 2) == (0, 1)
    for bad, match in (((3, 2), "ascending"), ((1, 3), "nearest neighbours"), ((2, 2), "nearest neighbours"), ((5, 6), "out of range"),
                       ((-1, 0), "out of range"), ((1, 2, 3), "two neighbouring"), (("a", 1), "invalid literal|tuple")):
        with pytest.raises(ValueError, match=match):
            pair_key(bad, 6)


def test_split_of_the_oracle():
    from helpers import pair_oracle as po

    rng = np.random.default_rng(1)
    theta = rng.standard_normal((3, 2, 3, 2)) + 1j * rng.standard_normal((3, 2, 3, 2))
    for r in (6, 4, 1):
        Cp, B, sv, disc = po.split(theta, r)
        Bm = B.reshape(r, -1)
        assert np.abs(Bm @ Bm.conj().T - np.eye(r)).max() < 1e-13
        err = np.linalg.norm(np.tensordot(Cp, B, axes=(2, 0)) - theta) ** 2 / np.linalg.norm(theta) ** 2
        assert abs(err - disc) < 1e-13 and abs(disc - np.sum(sv[r:] ** 2) / np.sum(sv**2)) < 1e-15
    low = np.einsum("ai,js->aijs", theta[:, :, 0, 0], theta[0, 0])  # rank 1, split at r = 4: completed
    Cp, B, sv, disc = po.split(low, 4)
    Bm = B.reshape(4, -1)
    assert np.abs(Bm @ Bm.conj().T - np.eye(4)).max() < 1e-13 and disc < 1e-28
    assert np.abs(np.tensordot(Cp, B, axes=(2, 0)) - low).max() < 1e-13


def test_two_site_sampling_with_the_split_is_an_exact_unravelling():
    """L = 4, d = 2, bonds (2, 4, 2), all maximal: nothing is truncated and one-site TDVP is exact up to the Krylov
    threshold (set tight).  Every branch of two steps of a pair jump channel on (1, 2) plus a one-site channel on site 1,
    each driven by the mid-points of its cumulative intervals and weighted by the product of its w_k / W:
    sum p |psi><psi| equals the dense map to 1e-12."""
    from helpers import jump_oracle as jo
    from helpers import pair_cases as pc
    from helpers import pair_oracle as po
    from oracle import tdvp_oracle as orc

    dims, nsteps, dt = (2, 2, 2, 2), 2, 0.3
    mpo = pc._spin_chain_mpo(4)
    rng = np.random.default_rng(17)
    Bp, B1 = pc.hopping_ops(), pc.kraus_set(2, 2, rng)
    channels = {(1, 2): ("jump", Bp), 1: ("jump", B1)}
    cores = orc.canonicalize_site0(orc.synthetic_mps(list(dims), 4, seed=8), scale=1.0)
    assert [c.shape for c in cores] == [(1, 2, 2), (2, 2, 4), (4, 2, 2), (2, 2, 1)]
    kw = dict(integrator="arnoldi", conserve_norm=False, thresh=1e-14)

    H = jo.dense_operator(mpo)
    psi0 = jo.dense_state(cores)
    rho = np.outer(psi0, psi0.conj())
    for _ in range(nsteps):
        rho = po.dense_channel_step(rho, H, dt, channels, dims)

    # the decisions of a step in the walk's order: the pair on (1, 2) when the centre is at 2, then site 1
    order = [((1, 2), len(Bp)), (1, len(B1))]
    acc = np.zeros_like(rho)
    leaves, total_p = 0, 0.0

    def step_branches(st, step):
        """every branch of one step from st: [(child, probability)]; a branch is found by driving the step with the
        mid-point of the wanted interval at every decision, the intervals read off a probe run of the same prefix"""
        out = []

        def grow(prefix):  # prefix: mid-points chosen so far, by decision index
            child = orc.OracleMPS([c.copy() for c in st.cores], mpo, **kw)
            child.kprev = dict(st.kprev)
            seen = []

            def uniform(trajectory, step_, site):
                i = len(seen)
                seen.append(site)
                return prefix[i] if i < len(prefix) else 0.5
            dec, spl = po.trajectory_step(child, dt, channels, uniform, 0, step)
            assert [d[0] for d in dec] == [o[0] for o in order]
            assert all(s[2] < 1e-24 for s in spl)  # nothing is truncated
            return child, dec

        def weights_at(prefix):
            """the weights of decision number len(prefix), given the mid-points before it (0.5 drives the rest)"""
            probe = orc.OracleMPS([c.copy() for c in st.cores], mpo, **kw)
            probe.kprev = dict(st.kprev)
            calls, seen = [], []

            def uniform(trajectory, step_, site):
                calls.append(site)
                return prefix[len(calls) - 1] if len(calls) <= len(prefix) else 0.5
            po.trajectory_step(probe, dt, channels, uniform, 0, step, weights_out=seen)
            return seen[len(prefix)]

        def descend(prefix, prob):
            if len(prefix) == len(order):
                child, dec = grow(prefix)
                p = float(np.prod([d[3] for d in dec]))
                assert abs(p - prob) < 1e-12
                out.append((child, p))
                return
            w = weights_at(prefix)
            cum = np.concatenate([[0.0], np.cumsum(w)])
            for k in range(len(w)):
                if w[k] > 1e-300:
                    descend(prefix + [0.5 * (cum[k] + cum[k + 1]) / cum[-1]], prob * w[k] / cum[-1])
        descend([], 1.0)
        return out

    def walk(st, step, prob):
        nonlocal acc, leaves, total_p
        if step == nsteps:
            v = jo.dense_state(st.cores)
            acc = acc + prob * np.outer(v, v.conj())
            leaves += 1
            total_p += prob
            return
        for child, p in step_branches(st, step):
            walk(child, step + 1, prob * p)

    walk(orc.OracleMPS([c.copy() for c in cores], mpo, **kw), 0, 1.0)
    err = np.abs(acc - rho).max()
    print(f"{leaves} branches, total probability {total_p:.15f}, max |sum p psi psi^+ - dense| = {err:.2e}")
    assert leaves > 4 and abs(total_p - 1) < 1e-12
    assert err < 1e-12


class _Stop(Exception):
    pass


def test_propagate_trajectories_parses_and_refuses_pair_keys_before_any_engine(monkeypatch):
    from helpers import pair_cases as pc
    from helpers import spin_bath as sb
    from pytdscf_amd import Exciton, Model
    from pytdscf_amd import trajectories as tr

    def no_engine(*a, **k):
        raise _Stop("an engine was created")

    monkeypatch.setattr(tr, "TDVPBatch", no_engine)
    case = sb.case_trajectories()  # dims (2, 3, 2)
    m = Model([Exciton(nstate=d) for d in case["dims"]], operators={"hamiltonian": case["mpo"]}, bond_dim=64)
    args = dict(maxstep=3, stepsize=0.1, reduced_density=([(1, 1)], 1))
    rng = np.random.default_rng(2)
    B6 = pc.kraus_set(3, 6, rng)

    for key, match in (((1, 0), r"\(1, 0\).*ascending"), ((0, 2), r"\(0, 2\).*nearest neighbours"), ((2, 3), r"\(2, 3\).*out of range"),
                       ((0, 1, 2), r"\(0, 1, 2\).*two neighbouring")):
        with pytest.raises(ValueError, match=match):
            tr.propagate_trajectories(m, case["starts"], jumps={key: B6}, **args)
    with pytest.raises(ValueError, match=r"\(0, 1\).*order 4.*2 x 3"):
        tr.propagate_trajectories(m, case["starts"], jumps={(0, 1): pc.kraus_set(2, 4, rng)}, **args)
    with pytest.raises(ValueError, match=r"\(1, 2\).*2 to 16"):
        tr.propagate_trajectories(m, case["starts"], jumps={(1, 2): B6[:1]}, **args)
    with pytest.raises(ValueError, match=r"\(1, 2\).*shape"):
        tr.propagate_trajectories(m, case["starts"], jumps={(1, 2): B6[0]}, **args)
    # accepted, next to an integer key, in both forms: the run reaches the engine
    B3 = pc.kraus_set(2, 3, rng)
    with pytest.raises(_Stop):
        tr.propagate_trajectories(m, case["starts"], jumps={(0, 1): B6, 1: B3}, **args)
    with pytest.raises(_Stop):
        tr.propagate_trajectories(m, case["starts"], jumps={(1, 2): B6.reshape(3, 3, 2, 3, 2)}, **args)
    table = tr._jump_table({(0, 1): B6.reshape(3, 2, 3, 2, 3), 1: B3}, case["dims"])
    assert set(table) == {(0, 1), 1} and table[(0, 1)].shape == (3, 6, 6)


# (case, its arguments, integrator) as tests/test_gpu_batch_pair.py runs them
CASES = [("exact", (2,), "lanczos"), ("exact", (2,), "arnoldi"), ("exact", (3,), "lanczos"), ("exact", (3,), "arnoldi"),
         ("truncating", (), "lanczos"), ("hopping", (), "lanczos"), ("large", (4,), "lanczos"), ("large", (3,), "lanczos")]


@pytest.mark.parametrize("name,args,integrator", CASES)
def test_inputs_of_the_gpu_tests_sit_on_no_edge(name, args, integrator):
    """From the oracle alone: every jump margin >= 1e-6; at every truncating split (sigma_r - sigma_{r+1}) / sigma_1 >= 1e-3."""
    from helpers import pair_cases as pc
    from helpers import pair_oracle as po

    case = getattr(pc, name)(*args)
    ref = pc.reference(name, integrator, *args)
    margins = [d[2] for _, dec, _ in ref for d in dec]
    gaps = [g for _, _, spl in ref for g in po.split_gaps(spl)]
    nsplit = sum(len(spl) for _, _, spl in ref)
    print(f"{name}{args} {integrator}: {len(margins)} decisions, smallest margin {min(margins, default=np.inf):.3e}; "
          f"{nsplit} splits, {len(gaps)} truncating, smallest gap {min(gaps, default=np.inf):.3e}")
    npair = sum(1 for k in case["channels"] if isinstance(k, tuple))
    assert nsplit == len(case["starts"]) * case["nsteps"] * npair
    assert all(mg >= 1e-6 for mg in margins)
    assert all(g >= 1e-3 for g in gaps)
    if name == "exact":
        assert not gaps and all(s[2] < 1e-24 for _, _, spl in ref for s in spl)
    if name == "truncating":
        assert len(gaps) == nsplit  # every split of this case truncates
    if name == "large":
        assert len(gaps) == len(case["starts"])  # the split of bond (2, 3) truncates, the outer two do not
        assert [c.shape for c in case["starts"][0]][2:4] == [(args[0] ** 2, args[0], 20), (20, args[0], args[0] ** 2)]
    if name == "hopping":
        assert len(margins) == len(case["starts"]) * case["nsteps"] * 2


def test_rank_deficient_case_has_rank_two():
    from helpers import pair_cases as pc
    from helpers import pair_oracle as po

    case = pc.rank_deficient()
    ref = pc.reference("rank_deficient", "arnoldi")
    for _, _, spl in ref:
        (bond, sv, disc, r), = spl
        assert bond == (2, 3) and r == 4 and disc < 1e-24
        assert sv[1] > 0.1 * sv[0] and sv[2] < 1e-13 * sv[0]  # rank 2 < 4
    assert not [g for _, _, spl in ref for g in po.split_gaps(spl)]
    assert len(case["starts"]) == 2
