"""A NumPy trajectory step with nearest-neighbour (pair) channels out of the oracle's own pieces: what
``jump_oracle.trajectory_step`` does -- forward half-sweep, the channel walk from site L-1 down to the lowest site a
channel touches and back up, backward half-sweep -- plus, on a bond (p-1, p) that carries a pair channel, in the place of
that step's gauge move: merge, apply, ``numpy.linalg.svd`` split to the bond's dimension r, and for a jump the rescale
to the norm before the jump.  The Python twin of ``k_batch_pair``; and the dense one-step map with embedded two-site
operators that the MEAN over trajectories follows when nothing is truncated.

``channels``: ``{site: ("gate", U (d, d)) | ("jump", B (K, d, d)),
(q, q + 1): ("gate", U (d0 d1, d0 d1)) | ("jump", B (K, d0 d1, d0 d1))}``, two-site operators row-major over (i_q, i_{q+1}).
The uniform of a pair jump on (q, q + 1) is ``uniform(trajectory, step, L + q)``."""

from __future__ import annotations

import numpy as np

from helpers import jump_oracle as jo
from oracle import tdvp_oracle as orc


def merge(A, C):
    """theta[a, i, j, s] = sum_b A[a, i, b] C[b, j, s]"""
    return np.tensordot(A, C, axes=(2, 0))


def apply_pair(op, theta):
    """theta'[a, i, j, s] = sum_(i', j') op[(i, j), (i', j')] theta[a, i', j', s]"""
    dl, d0, d1, dr = theta.shape
    op4 = np.asarray(op, dtype=np.complex128).reshape(d0, d1, d0, d1)
    return np.einsum("ijkl,akls->aijs", op4, theta)


def pair_weights(theta, B):
    """w_k = |B_k theta|^2 and |theta|^2"""
    w = []
    for b in B:
        x = apply_pair(b, theta)
        w.append(float(np.vdot(x, x).real))
    return w, float(np.vdot(theta, theta).real)


def split(theta, r):
    """theta (dl, d0, d1, dr) ~ C' (dl, d0, r) . B (r, d1, dr): B the r leading right singular vectors (orthonormal rows,
    completed by further right singular vectors when the rank is below r -- r <= d1 dr), C' = theta B^+.
    Returns (C', B, singular values (all of them), discarded weight sum_{j>r} s_j^2 / sum_j s_j^2)."""
    dl, d0, d1, dr = theta.shape
    mat = theta.reshape(dl * d0, d1 * dr)
    _, sv, vh = np.linalg.svd(mat, full_matrices=True)  # vh: all d1 dr right vectors, orthonormal rows
    Bm = vh[:r]
    Cp = mat @ Bm.conj().T
    tot = float(np.sum(sv**2))
    disc = float(np.sum(sv[r:] ** 2) / tot) if tot > 0.0 else 0.0
    return Cp.reshape(dl, d0, r), Bm.reshape(r, d1, dr), sv, disc


def trajectory_step(st: orc.OracleMPS, dt, channels, uniform, trajectory=0, step=0, weights_out=None):
    """One time step of one trajectory, in place on ``st`` (centre at site 0 before and after).
    Returns ``(decisions, splits)``: decisions in the order taken, ``[(site or (q, q + 1), k, margin, w_k / W), ...]``;
    splits ``[((q, q + 1), singular values, discarded weight, r), ...]``.  ``weights_out``: a list that receives the
    weights ``[w_0, .., w_{K-1}]`` of every decision, in the same order."""
    L = st.nsite
    if len(st.right) < L:
        st.build_right_envs()
    st.sweep(dt, True)
    decisions, splits = [], []
    if channels:
        lo = min(k if isinstance(k, int) else k[0] for k in channels)
        cores = st.cores
        for p in range(L - 1, lo - 1, -1):
            kind, ops = channels.get(p, (None, None))
            if kind == "gate":
                orc.apply_one_gate(cores, p, {p: np.asarray(ops, dtype=np.complex128)})
            elif kind == "jump":
                w, n2 = jo.jump_weights(cores[p], ops)
                if weights_out is not None:
                    weights_out.append(list(w))
                k, W, margin = jo.select(w, uniform(trajectory, step, p))
                orc.apply_one_gate(cores, p, {p: np.asarray(ops[k], dtype=np.complex128)})
                cores[p] = cores[p] * np.sqrt(n2 / w[k])
                decisions.append((p, k, margin, w[k] / W))
            elif kind is not None:
                raise ValueError(kind)
            if p == lo:
                break
            pkind, pops = channels.get((p - 1, p), (None, None))
            if pkind is None:
                sval, B = orc.qr_psi2sigmaB(cores[p])
                cores[p] = np.ascontiguousarray(B)
                cores[p - 1] = np.tensordot(cores[p - 1], sval, axes=(2, 0))
                continue
            theta = merge(cores[p - 1], cores[p])
            r = cores[p].shape[0]
            if pkind == "gate":
                theta = apply_pair(pops, theta)
                Cp, B, sv, disc = split(theta, r)
            elif pkind == "jump":
                w, n2 = pair_weights(theta, pops)
                if weights_out is not None:
                    weights_out.append(list(w))
                k, W, margin = jo.select(w, uniform(trajectory, step, L + p - 1))
                theta = apply_pair(pops[k], theta)
                Cp, B, sv, disc = split(theta, r)
                Cp = Cp * np.sqrt(n2 / float(np.vdot(Cp, Cp).real))  # the norm after the split = the norm before the jump
                decisions.append(((p - 1, p), k, margin, w[k] / W))
            else:
                raise ValueError(pkind)
            cores[p - 1], cores[p] = np.ascontiguousarray(Cp), np.ascontiguousarray(B)
            splits.append(((p - 1, p), sv, disc, r))
        for p in range(lo, L - 1):
            A, sval = orc.qr_psi2Asigma(cores[p])
            cores[p] = A
            st.left[p + 1] = orc.env_update_left(st.left[p], A, st.mpo[p])
            cores[p + 1] = np.tensordot(sval, cores[p + 1], axes=(1, 0))
    st.sweep(dt, False)
    return decisions, splits


def run_trajectory(cores, mpo, dt, nsteps, channels, uniform, trajectory=0, first_step=0, **oracle_kw):
    """``nsteps`` steps from ``cores`` (site-0-centred); returns (OracleMPS, decisions, splits) of all steps"""
    st = orc.OracleMPS([np.array(c) for c in cores], mpo, **oracle_kw)
    dec, spl = [], []
    for s in range(nsteps):
        d, sp = trajectory_step(st, dt, channels, uniform, trajectory, first_step + s)
        dec += d
        spl += sp
    return st, dec, spl


def counts_of(decisions, L, kmax=16):
    """(one-site counters, pair counters), each (L, kmax); a pair on (q, q + 1) counts in row q"""
    one = np.zeros((L, kmax), dtype=np.int64)
    pair = np.zeros((L, kmax), dtype=np.int64)
    for key, k, _, _ in decisions:
        if isinstance(key, tuple):
            pair[key[0], k] += 1
        else:
            one[key, k] += 1
    return one, pair


def split_gaps(splits):
    """(sigma_r - sigma_{r+1}) / sigma_1 of every truncating split (one with a singular value beyond r above rounding)"""
    gaps = []
    for _, sv, _, r in splits:
        if len(sv) > r and sv[r] > 1e-13 * sv[0]:
            gaps.append(float((sv[r - 1] - sv[r]) / sv[0]))
    return gaps


def embed_pair(op, q, dims):
    """a two-site operator on (q, q + 1), row-major over (i_q, i_{q+1}), on the full space"""
    left = int(np.prod(dims[:q], dtype=np.int64))
    right = int(np.prod(dims[q + 2:], dtype=np.int64))
    return np.kron(np.kron(np.eye(left), np.asarray(op, dtype=np.complex128)), np.eye(right))


def dense_channel_step(rho, H, dt, channels, dims):
    """rho <- U C(U rho U^+) U^+, U = exp(-i H dt / 2), C the channels in the walk's order: from the highest site down, the
    one-site channel of p before the pair channel of (p-1, p).  A gate is rho -> G rho G^+, a jump channel
    rho -> sum_k B_k rho B_k^+ (trace-preserving when sum B^+ B = 1: the trajectories keep their norm)."""
    from scipy.linalg import expm

    U = expm(-0.5j * dt * H)
    rho = U @ rho @ U.conj().T
    L = len(dims)
    for p in range(L - 1, -1, -1):
        for key, emb in ((p, lambda o: jo.embed(o, p, dims)), ((p - 1, p), lambda o: embed_pair(o, p - 1, dims))):
            if key not in channels:
                continue
            kind, ops = channels[key]
            full = [emb(np.asarray(ops, dtype=np.complex128))] if kind == "gate" else [emb(b) for b in ops]
            rho = sum(b @ rho @ b.conj().T for b in full)
    return U @ rho @ U.conj().T
