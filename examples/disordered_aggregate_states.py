#!/usr/bin/env python3
"""The lowest three eigenstates of a disordered exciton chain for a few disorder realisations at once, with the transition
dipoles from the ground state:

    H_r = sum_p (E0 + delta_p^r) n_p + J sum_p (up_p down_{p+1} + h.c.),   mu = sum_p (|e_p><g_p| + |g_p><e_p|)

``relax_trajectories(models, nstates=3, penalty=...)`` finds state 0 of every realisation by improved relaxation in one
batch, stores it with the weight ``penalty`` (``TDVPBatch.deflate_push``), gives every replica a fresh random start and
relaxes again on H + penalty |0><0|, and so on: the penalty method, one workgroup per realisation
(``k_batch_relax_defl``).  The penalty must exceed the largest gap wanted -- here the ground state is the empty chain and
the two states above it are the lowest excitons near E0, so anything well above E0 will do.

The transition dipoles <k| mu |0> are then MPO matrix elements between replicas and their snapshots
(``set_cross_mpo``, ``k_batch_cross_mpo``): the ground states go into the snapshot, the replicas take state k.  In the
one-exciton manifold H_r is an L x L tridiagonal matrix, so energies and dipoles are known; the script prints both.  Runs on
one MI355X.

    python examples/disordered_aggregate_states.py [realisations]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytdscf_amd import Exciton, Model, TDVPBatch  # noqa: E402
from pytdscf_amd.trajectories import relax_trajectories  # noqa: E402

L, D = 6, 8
E0, J, SIGMA = 0.10, -0.004, 0.002  # site energy, coupling and the width of the static disorder (hartree)
PENALTY = 1.0
ID = np.eye(2, dtype=complex)
NUM = np.array([[0, 0], [0, 1]], dtype=complex)  # |e><e|
UP = np.array([[0, 0], [1, 0]], dtype=complex)   # |e><g|
SX = UP + UP.T


def frenkel_mpo(site_energy):
    """(ml, d, d, mr) cores of sum_p site_energy[p] n_p + J sum_p (up_p down_{p+1} + h.c.): a four-state automaton"""
    cores = []
    for p in range(L):
        w = np.zeros((4, 2, 2, 4), dtype=complex)
        w[0, :, :, 0] = w[3, :, :, 3] = ID
        w[0, :, :, 1], w[1, :, :, 3] = UP, J * UP.T
        w[0, :, :, 2], w[2, :, :, 3] = UP.T, J * UP
        w[0, :, :, 3] = site_energy[p] * NUM
        cores.append(w[:1] if p == 0 else w)
    cores[-1] = cores[-1][..., 3:]
    return cores


def dipole_mpo():
    """sum_p (|e_p><g_p| + |g_p><e_p|), padded to the Hamiltonian's bond of 4: one batch, one set of MPO shapes"""
    cores = []
    for p in range(L):
        w = np.zeros((4, 2, 2, 4), dtype=complex)
        w[0, :, :, 0] = w[3, :, :, 3] = ID
        w[0, :, :, 3] = SX
        cores.append(w[:1] if p == 0 else w)
    cores[-1] = cores[-1][..., 3:]
    return cores


def main():
    nreal = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    rng = np.random.default_rng(0)
    energies = E0 + SIGMA * rng.standard_normal((nreal, L))
    models = [Model([Exciton(nstate=2) for _ in range(L)], operators={"hamiltonian": frenkel_mpo(e)}, bond_dim=D) for e in energies]
    rng_start = np.random.default_rng(1)
    start0 = [[rng_start.standard_normal(2) for _ in range(L)] for _ in range(nreal)]  # Hartree products with weight in every sector
    out = relax_trajectories(models, starts=[start0, None, None], nstates=3, penalty=PENALTY, maxstep=12, conv_tol=1e-13)

    # <k| mu |0>: the ground states in the snapshot, state k in the replicas
    bt = TDVPBatch(nreal, L)
    try:
        for r, e in enumerate(bt.engines):
            e.set_mpo(frenkel_mpo(energies[r]), 0)
            e.set_mpo(dipole_mpo(), 1)
            e.set_mps(out["states"][0][r])
        bt.snapshot()
        bt.set_cross_mpo([(r, bt.snap(r), 1) for r in range(nreal)])
        dip = np.zeros((3, nreal))
        for k in (1, 2):
            for r, e in enumerate(bt.engines):
                e.set_mps(out["states"][k][r])
            dip[k] = np.abs(bt.cross_mpo()["values"])
    finally:
        bt.close()

    print("# realisation  state   E (relaxation)     E (exact)      |<k|mu|0>|   exact")
    for r in range(nreal):
        h1 = np.diag(energies[r]) + J * (np.eye(L, k=1) + np.eye(L, k=-1))  # the one-exciton block
        w, v = np.linalg.eigh(h1)
        exact_e = [0.0, w[0], w[1]]
        exact_d = [0.0, abs(v[:, 0].sum()), abs(v[:, 1].sum())]
        for k in range(3):
            print(f"  {r:11d}  {k:5d}   {out['energies'][k, r]:14.10f}  {exact_e[k]:14.10f}   {dip[k, r]:10.6f}  {exact_d[k]:10.6f}")
    off = np.abs(out["overlaps"] - np.eye(3)[:, :, None]).max()
    print(f"# largest |<j|k> - delta_jk| over all realisations: {off:.1e}")


if __name__ == "__main__":
    main()
