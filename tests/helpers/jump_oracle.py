"""A NumPy quantum-jump trajectory step out of the oracle's own pieces (``oracle.tdvp_oracle``): the time step of
``k_batch_channel`` -- forward half-sweep, the channel walk with the centre moving from site L-1 down to the lowest site
with a channel and back up, backward half-sweep -- with the kernel's selection rule, and the dense one-step map that the
MEAN over trajectories follows.

Pieces used: ``OracleMPS.sweep``, ``qr_psi2sigmaB`` / ``qr_psi2Asigma``, ``env_update_left``, ``apply_one_gate``.

``channels``: ``{site: ("gate", U (d, d)) | ("jump", B (K, d, d))}``."""

from __future__ import annotations

import numpy as np

from oracle import tdvp_oracle as orc


def jump_weights(C, B):
    """w_k = |B_k C|^2 for the centre tensor C (dl, d, dr), and |C|^2"""
    BC = np.einsum("kij,ajs->kais", np.asarray(B, dtype=np.complex128), C)
    return [float(np.vdot(x, x).real) for x in BC], float(np.vdot(C, C).real)


def select(w, u):
    """the smallest k whose running sum (index order) exceeds u W; if rounding leaves none, the last k with w_k > 0.
    Returns (k, W, margin) with margin = min_k |u W - cumsum_k| / W."""
    W = 0.0
    for x in w:
        W += x
    if not W > 0.0:
        raise ZeroDivisionError("every operator of the jump channel gives zero weight")
    thr, run, pick, last, margin = u * W, 0.0, -1, 0, np.inf
    for k, x in enumerate(w):
        run += x
        if x > 0.0:
            last = k
        if pick < 0 and run > thr:
            pick = k
        margin = min(margin, abs(thr - run) / W)
    return (pick if pick >= 0 else last), W, margin


def trajectory_step(st: orc.OracleMPS, dt, channels, uniform, trajectory=0, step=0):
    """One time step of one trajectory, in place on ``st`` (centre at site 0 before and after).
    ``uniform(trajectory, step, site)`` supplies the number in [0, 1) of a jump decision.
    Returns the decisions in the order they were taken: ``[(site, k, margin, w_k / W), ...]``."""
    L = st.nsite
    if len(st.right) < L:
        st.build_right_envs()
    st.sweep(dt, True)
    decisions = []
    if channels:
        lo = min(channels)
        cores = st.cores
        for p in range(L - 1, lo - 1, -1):
            kind, ops = channels.get(p, (None, None))
            if kind == "gate":
                orc.apply_one_gate(cores, p, {p: np.asarray(ops, dtype=np.complex128)})  # p is the centre: no gauge move
            elif kind == "jump":
                w, n2 = jump_weights(cores[p], ops)
                k, W, margin = select(w, uniform(trajectory, step, p))
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
    st.sweep(dt, False)
    return decisions


def run_trajectory(cores, mpo, dt, nsteps, channels, uniform, trajectory=0, first_step=0, **oracle_kw):
    """``nsteps`` steps from ``cores`` (site-0-centred); returns (OracleMPS, decisions of all steps)"""
    st = orc.OracleMPS([np.array(c) for c in cores], mpo, **oracle_kw)
    dec = []
    for s in range(nsteps):
        dec += trajectory_step(st, dt, channels, uniform, trajectory, first_step + s)
    return st, dec


def counts_of(decisions, L, kmax=16):
    c = np.zeros((L, kmax), dtype=np.int64)
    for p, k, _, _ in decisions:
        c[p, k] += 1
    return c


def dense_state(cores):
    """the state vector of an MPS, physical indices in site order"""
    v = np.ones((1, 1), dtype=np.complex128)
    for c in cores:
        v = np.tensordot(v, c, axes=(1, 0)).reshape(-1, c.shape[2])
    return v.reshape(-1)


def dense_operator(mpo, shift=0.0):
    """the matrix of a full-chain MPO (ml, d_out, d_in, mr per site)"""
    M = np.ones((1, 1, 1), dtype=np.complex128)  # (rows, cols, bond)
    for w in mpo:
        M = np.einsum("rcb,bijm->ricjm", M, w).reshape(M.shape[0] * w.shape[1], M.shape[1] * w.shape[2], w.shape[3])
    H = M[:, :, 0]
    return H + shift * np.eye(H.shape[0])


def embed(op, site, dims):
    """a one-site operator on the full space"""
    out = np.ones((1, 1), dtype=np.complex128)
    for p, d in enumerate(dims):
        out = np.kron(out, op if p == site else np.eye(d))
    return out


def dense_channel_step(rho, H, dt, jumps, dims):
    """rho <- U (sum_k B_k (U rho U^+) B_k^+) U^+ with U = exp(-i H dt / 2), site after site from the highest jump site
    down: the time step whose unravelling ``trajectory_step`` samples (H may be non-Hermitian: no renormalisation)"""
    from scipy.linalg import expm

    U = expm(-0.5j * dt * H)
    rho = U @ rho @ U.conj().T
    for site in sorted(jumps, reverse=True):
        full = [embed(b, site, dims) for b in jumps[site]]
        rho = sum(b @ rho @ b.conj().T for b in full)
    return U @ rho @ U.conj().T
