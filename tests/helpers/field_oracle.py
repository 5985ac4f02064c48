"""A NumPy time step with time-dependent one-site fields out of the oracle's own pieces (``oracle.tdvp_oracle``): the time
step of ``k_batch_field`` -- forward half-sweep, the one-site unitaries ``exp(-i dt a_p G_p)`` applied IN PLACE with the
left blocks rebuilt (no gauge move), the channel walk of ``jump_oracle.trajectory_step`` when channels are set, backward
half-sweep -- and the dense time-ordered evolution that the splitting approximates to O(dt^2).

``fields``: ``{site: G (d, d) Hermitian}``; ``amps``: ``{site: a}`` or a sequence over all sites (sites without a field
are ignored).  ``channels`` as ``jump_oracle`` takes them."""

from __future__ import annotations

import numpy as np

from oracle import tdvp_oracle as orc

from . import jump_oracle as jo


def field_unitary(G, a, dt):
    """exp(-i dt a G) through the decomposition the library is given: G = V diag(g) V^+ by numpy.linalg.eigh"""
    G = np.asarray(G, dtype=np.complex128)
    g, V = np.linalg.eigh(0.5 * (G + G.conj().T))
    return (V * np.exp(-1j * dt * a * g)) @ V.conj().T


def _amp(amps, p):
    return float(amps[p]) if not isinstance(amps, dict) else float(amps.get(p, 0.0))


def apply_fields_in_place(st: orc.OracleMPS, dt, amps, fields):
    """centre at L-1, sites 0 .. L-2 in gauge A: U_p on the physical index of every field site, then L[p+1] for
    p = lo .. L-2.  A unitary on the physical index keeps an isometry an isometry: nothing else moves."""
    if not fields:
        return
    L = st.nsite
    for p in sorted(fields):
        st.cores[p] = np.einsum("abc,db->adc", st.cores[p], field_unitary(fields[p], _amp(amps, p), dt))
    for p in range(min(fields), L - 1):
        st.left[p + 1] = orc.env_update_left(st.left[p], st.cores[p], st.mpo[p])


def channel_walk(st: orc.OracleMPS, channels, uniform, trajectory=0, step=0):
    """the middle part of ``jump_oracle.trajectory_step``: the centre from L-1 down to the lowest channel and back up"""
    L, cores, decisions = st.nsite, st.cores, []
    if not channels:
        return decisions
    lo = min(channels)
    for p in range(L - 1, lo - 1, -1):
        kind, ops = channels.get(p, (None, None))
        if kind == "gate":
            orc.apply_one_gate(cores, p, {p: np.asarray(ops, dtype=np.complex128)})
        elif kind == "jump":
            w, n2 = jo.jump_weights(cores[p], ops)
            k, W, margin = jo.select(w, uniform(trajectory, step, p))
            orc.apply_one_gate(cores, p, {p: np.asarray(ops[k], dtype=np.complex128)})
            cores[p] = cores[p] * np.sqrt(n2 / w[k])
            decisions.append((p, k, margin, w[k] / W))
        elif kind is not None:
            raise ValueError(kind)
        if p > lo:
            sval, B = orc.qr_psi2sigmaB(cores[p])
            cores[p] = np.ascontiguousarray(B)
            cores[p - 1] = np.tensordot(cores[p - 1], sval, axes=(2, 0))
    for p in range(lo, L - 1):
        A, sval = orc.qr_psi2Asigma(cores[p])
        cores[p] = A
        st.left[p + 1] = orc.env_update_left(st.left[p], A, st.mpo[p])
        cores[p + 1] = np.tensordot(sval, cores[p + 1], axes=(1, 0))
    return decisions


def field_step(st: orc.OracleMPS, dt, amps, fields, channels=None, uniform=None, trajectory=0, step=0):
    """One time step in place on ``st`` (centre at site 0 before and after); returns the jump decisions."""
    if len(st.right) < st.nsite:
        st.build_right_envs()
    st.sweep(dt, True)
    apply_fields_in_place(st, dt, amps, fields)
    decisions = channel_walk(st, channels, uniform, trajectory, step)
    st.sweep(dt, False)
    return decisions


def walk_step(st: orc.OracleMPS, dt, amps, fields):
    """the same step with the unitaries as GATES of the existing walk (``jump_oracle.trajectory_step``): two gauge moves
    per site above the lowest field"""
    gates = {p: ("gate", field_unitary(G, _amp(amps, p), dt)) for p, G in fields.items()}
    jo.trajectory_step(st, dt, gates, None)


# ---- the dense time-ordered evolution ----
def _expm_herm(H, t):
    w, V = np.linalg.eigh(H)
    return (V * np.exp(-1j * t * w)) @ V.conj().T


def dense_time_ordered(psi, H0, drive, G, t0, t1, nsub=4096):
    """psi(t1) under H(t) = H0 + drive(t) G from psi(t0): ``nsub`` exponential-midpoint steps.  The midpoint rule is of
    second order, so at nsub = 4096 over a unit of time its own error is some 1e-5 of that of a step of 0.0125: exact for
    what it is compared with."""
    h = (t1 - t0) / nsub
    psi = np.asarray(psi, dtype=np.complex128)
    for n in range(nsub):
        psi = _expm_herm(H0 + drive(t0 + (n + 0.5) * h) * G, h) @ psi
    return psi


# ---- the driven chain of the tests: L = 4 spins 1/2, Heisenberg couplings, a Gaussian pulse on all four sites ----
SX = np.array([[0, 1], [1, 0]], dtype=complex) / 2
SY = np.array([[0, -1j], [1j, 0]]) / 2
SZ = np.array([[1, 0], [0, -1]], dtype=complex) / 2
T_END = 1.0


def pulse(t):
    return 1.5 * np.exp(-0.5 * ((t - 0.5) / 0.2) ** 2)


def driven_chain(D=4, seed=5):
    """dims, MPO and dense matrix of H0, the fields {p: Sx_p}, their dense sum, and a start: a random MPS of bond D
    (D = 4 is the full bond of the chain: one-site TDVP of H0 alone is exact there), centre at site 0, norm 1"""
    from . import spin_bath as sb

    dims = [2, 2, 2, 2]
    terms = [(1.0, {p: s, p + 1: s}) for p in range(3) for s in (SX, SY, SZ)] + [(0.3 * (p + 1), {p: SZ}) for p in range(4)]
    mpo = sb.sop_mpo(terms, dims)
    fields = {p: 2.0 * SX for p in range(4)}
    Gsum = sum(jo.embed(G, p, dims) for p, G in fields.items())
    start = orc.canonicalize_site0(orc.synthetic_mps(dims, D, seed=seed), scale=1.0)
    return dict(dims=dims, mpo=mpo, H0=jo.dense_operator(mpo), fields=fields, G=Gsum, start=start)


def midpoints(dt, nsteps):
    return [pulse((n + 0.5) * dt) for n in range(nsteps)]


def run_numpy(case, dt, nsteps, step=field_step, **oracle_kw):
    """``nsteps`` steps of the driven chain from its start; returns the OracleMPS"""
    kw = dict(integrator="arnoldi", conserve_norm=False, thresh=1e-13)
    kw.update(oracle_kw)
    st = orc.OracleMPS([c.copy() for c in case["start"]], case["mpo"], **kw)
    for a in midpoints(dt, nsteps):
        step(st, dt, [a] * 4, case["fields"])
    return st
