"""The inputs of the pair-channel tests, shared by tests/test_batch_pair_host.py (which asserts from the oracle alone that
no decision and no truncation of theirs sits on an edge) and tests/test_gpu_batch_pair.py (which runs them on the device).
Every case is a dict: ``dims``, ``mpo``, ``starts`` (site-0-centred cores per replica), ``channels`` (the oracle's form,
tests/helpers/pair_oracle.py), ``nsteps``, ``dt``, ``seed`` (of the jump generator).  NumPy only."""

from __future__ import annotations

import functools

import numpy as np

DT = 0.4
SM = np.array([[0, 1], [0, 0]], dtype=complex)  # sigma^-: |1> -> |0> with |0> = (1, 0)
SP = SM.T.copy()
GAMMA = 0.3


def mixed_mpo(dims, M, seed):
    """Hermitian, nearest-neighbour-like, bond M, a physical dimension per site (as tests/test_gpu_batch_jump.py builds it)"""
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


def unitary(n, rng):
    Q, R = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    return Q * (np.diag(R) / np.abs(np.diag(R)))


def kraus_set(K, d, rng):
    """K random matrices rescaled to sum B^+ B = 1"""
    G = rng.standard_normal((K, d, d)) + 1j * rng.standard_normal((K, d, d))
    w, V = np.linalg.eigh(sum(g.conj().T @ g for g in G))
    return G @ ((V / np.sqrt(w)) @ V.conj().T)


def _starts(dims, D, nrep, seed0):
    from oracle import tdvp_oracle as orc

    return [orc.canonicalize_site0(orc.synthetic_mps(list(dims), D, seed=seed0 + r), scale=1.0) for r in range(nrep)]


@functools.lru_cache(maxsize=None)
def exact(d_mid=2):
    """L = 4, all bonds maximal (2, d_mid^2 capped by the outer sites, 2): pair gates on all three bonds and a one-site
    gate; no split truncates.  d_mid = 3: dims (2, 3, 3, 2), bonds (2, 6, 2) -- unequal d0, d1 on the outer bonds."""
    dims = (2, d_mid, d_mid, 2)
    D = 2 * d_mid
    rng = np.random.default_rng(100 + d_mid)
    ch = {(q, q + 1): ("gate", unitary(dims[q] * dims[q + 1], rng)) for q in range(3)}
    g = np.eye(d_mid) + 0.3 * (rng.standard_normal((d_mid, d_mid)) + 1j * rng.standard_normal((d_mid, d_mid)))  # not unitary
    ch[2] = ("gate", g * np.sqrt(d_mid) / np.linalg.norm(g))
    return dict(dims=dims, D=D, mpo=mixed_mpo(dims, 4, seed=3), starts=_starts(dims, D, 3, 40), channels=ch, nsteps=3, dt=DT, seed=0)


@functools.lru_cache(maxsize=None)
def truncating():
    """L = 6, d = 2, D = 4: a random two-site unitary on (2, 3) makes an 8 x 8 theta of full rank that is cut to 4"""
    dims = (2,) * 6
    rng = np.random.default_rng(200)
    ch = {(2, 3): ("gate", unitary(4, rng))}
    return dict(dims=dims, D=4, mpo=mixed_mpo(dims, 4, seed=5), starts=_starts(dims, 4, 3, 50), channels=ch, nsteps=2, dt=DT, seed=0)


@functools.lru_cache(maxsize=None)
def large(d):
    """L = 6, D = 20, pair gates on (1, 2), (2, 3) and (3, 4): the shapes at which the split takes its other paths.
    d = 4, bonds (4, 16, 20, 16, 4): theta is 16 x 80 (more than 64 columns: two per lane), 64 x 64 cut to 20 (more
    pairs than waves, more elements than threads) and 80 x 16 (more rows than columns).  d = 3, bonds (3, 9, 20, 9, 3):
    9 x 60, 27 x 27 cut to 20 and 60 x 9 -- odd row counts, so a slot of the round-robin rests in every round.
    (The start seeds are those whose truncating split has a relative gap >= 1e-3 in the oracle: the host test asserts it.)"""
    dims = (d,) * 6
    rng = np.random.default_rng(400 + d)
    ch = {(q, q + 1): ("gate", unitary(d * d, rng)) for q in (1, 2, 3)}
    return dict(dims=dims, D=20, mpo=mixed_mpo(dims, 4, seed=6), starts=_starts(dims, 20, 2, 80 if d == 4 else 82), channels=ch, nsteps=1, dt=DT, seed=0)


def _one_site_mpo(dims, seed):
    """H = sum_p h_p, one-site terms only: the exact evolution is a product of one-site unitaries"""
    from helpers import spin_bath as sb

    rng = np.random.default_rng(seed)
    terms, hs = [], []
    for p, d in enumerate(dims):
        G = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
        hs.append((G + G.conj().T) / 2)
        terms.append((1.0, {p: hs[-1]}))
    return sb.sop_mpo(terms, list(dims)), hs


@functools.lru_cache(maxsize=None)
def rank_deficient():
    """L = 6, d = 2: a product start padded to D = 4 and the entangling gate CNOT (H x 1) on (2, 3): theta has rank 2 < 4
    at the first step.  H has one-site terms only, so one-site TDVP is exact whatever completes the null space, and the
    state after a step is the dense U G U |start>."""
    from oracle import tdvp_oracle as orc
    from pytdscf_amd.mps import product_state_cores

    dims = (2,) * 6
    had = np.array([[1, 1], [1, -1]], dtype=complex) / np.sqrt(2)
    cnot = np.eye(4, dtype=complex)[[0, 1, 3, 2]]
    gate = cnot @ np.kron(had, np.eye(2))
    mpo, hs = _one_site_mpo(dims, seed=9)
    vecs = [[[1, 0], [0, 1], [1, 0], [1, 0], [0, 1], [1, 0]], [[1, 1], [1, 0], [0, 1], [1, -1], [1, 0], [1, 2]]]
    starts = [orc.canonicalize_site0(product_state_cores(v, 4, space="hilbert"), scale=1.0) for v in vecs]
    # Arnoldi at a tight threshold: short-iterative Lanczos without re-orthogonalisation exhausts the tiny Krylov spaces of
    # a padded product state and pollutes the null space at the 1e-3 level (the oracle shows the same), which is no
    # longer a rank-deficient theta
    return dict(dims=dims, D=4, mpo=mpo, h=hs, starts=starts, channels={(2, 3): ("gate", gate)}, nsteps=1, dt=DT, seed=0, thresh=1e-14)


def hopping_ops(gamma=GAMMA):
    """{sqrt(g) s^- s^+, sqrt(g) s^+ s^-, complement}: incoherent hopping between two neighbouring two-level sites,
    sum B^+ B = 1"""
    a, b = np.sqrt(gamma) * np.kron(SM, SP), np.sqrt(gamma) * np.kron(SP, SM)
    rest = np.eye(4) - a.conj().T @ a - b.conj().T @ b  # diagonal, entries 1 or 1 - gamma
    B = np.stack([a, b, np.sqrt(rest)])
    assert np.abs(sum(x.conj().T @ x for x in B) - np.eye(4)).max() < 1e-12
    return B


def _spin_chain_mpo(L):
    from helpers import spin_bath as sb

    terms = []
    for p in range(L):
        terms.append((0.3 + 0.1 * p, {p: sb.SZ}))
        terms.append((0.2, {p: sb.SX}))
    for p in range(L - 1):
        for s in (sb.SX, sb.SY, sb.SZ):
            terms.append((0.5, {p: s, p + 1: s}))
    return sb.sop_mpo(terms, [2] * L)


@functools.lru_cache(maxsize=None)
def hopping():
    """L = 6 spin chain, D = 4: the hopping channel on (2, 3) next to a one-site jump channel on site 2; six trajectories"""
    dims = (2,) * 6
    rng = np.random.default_rng(300)
    ch = {(2, 3): ("jump", hopping_ops()), 2: ("jump", kraus_set(2, 2, rng))}
    return dict(dims=dims, D=4, mpo=_spin_chain_mpo(6), starts=_starts(dims, 4, 6, 70), channels=ch, nsteps=4, dt=DT, seed=2025)


def batch_tables(channels):
    """the oracle's channel table as the arguments of TDVPBatch.set_gates / set_jumps"""
    gates = {k: ops for k, (kind, ops) in channels.items() if kind == "gate"}
    jumps = {k: ops for k, (kind, ops) in channels.items() if kind == "jump"}
    return gates, jumps


@functools.lru_cache(maxsize=None)
def reference(name, integrator, *args):
    """the oracle's trajectories of a case, computed once per integrator and left unchanged:
    [(cores, decisions, splits), ...] per replica (trajectory id = replica index)"""
    from helpers import pair_oracle as po
    from pytdscf_amd.trajectories import jump_uniform

    case = globals()[name](*args)
    out = []
    for r, start in enumerate(case["starts"]):
        st, dec, spl = po.run_trajectory(start, case["mpo"], case["dt"], case["nsteps"], case["channels"],
                                         lambda t, s, p: jump_uniform(case["seed"], t, s, p), trajectory=r,
                                         integrator=integrator, conserve_norm=False, thresh=case.get("thresh", 1e-9))
        out.append((st.cores, dec, spl))
    return out
