"""Dense yardstick of the general reduced density: a state vector traced down to a key in the reference's form (a tuple
of site indices, each site once for its diagonal or twice for ket and bra), and the trajectory case of the spin-bath
model (``helpers/spin_bath.py``: four product starts, H - i k_H / 2, no dissipator) solved densely start by start and
averaged.  Nothing here is shared with the code under test: ``scipy.linalg.expm`` and ``numpy.einsum`` only."""

from __future__ import annotations

import numpy as np
from scipy.linalg import expm

from . import spin_bath as sb


def legs_of(key, nsite):
    """legs kept per site, all ``nsite`` of them"""
    return [tuple(key).count(p) for p in range(nsite)]


def dense_key_density(psi, dims, key):
    """|psi><psi| traced to ``key``: kept sites ascending, (ket, bra) per two-leg site, the diagonal of a one-leg site"""
    L = len(dims)
    legs = legs_of(key, L)
    t = np.asarray(psi).reshape(dims)
    bra = [L + p if legs[p] == 2 else p for p in range(L)]
    out = []
    for p in range(L):
        out += [p, L + p] if legs[p] == 2 else ([p] if legs[p] == 1 else [])
    return np.einsum(t, list(range(L)), t.conj(), bra, out)


def product_vector(start):
    v = np.ones(1, dtype=np.complex128)
    for s in start:
        v = np.kron(v, np.asarray(s, dtype=np.complex128))
    return v


def exact_trajectory_densities(keys, nsteps=sb.NSTEPS, dt=sb.DT):
    """{key: (nsteps, ...)}: the mean over the four starts of ``spin_bath.case_trajectories`` at t = 0, dt, ..."""
    case = sb.case_trajectories()
    dims = case["dims"]
    H = sb.hamiltonian_dense() - 0.5j * sb.K_HAB * np.eye(int(np.prod(dims)))
    U = expm(-1j * dt * H)
    out = {tuple(k): [] for k in keys}
    psis = [product_vector(s) for s in case["starts"]]
    for _ in range(nsteps):
        for k in out:
            out[k].append(sum(dense_key_density(v, dims, k) for v in psis) / len(psis))
        psis = [U @ v for v in psis]
    return {k: np.array(v) for k, v in out.items()}
