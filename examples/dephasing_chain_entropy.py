#!/usr/bin/env python3
"""Trajectory-averaged entanglement entropy of a dephasing Heisenberg chain, and the convergence check of a fixed bond
dimension that goes with it:

    Neel start  ->  quantum-jump trajectories of  H = J sum S_p . S_{p+1} + sum h_p S^z_p  with dephasing on every site
                ->  half-chain von Neumann entropy of EVERY trajectory, averaged  (not a function of the averaged density)

The batch keeps its bond dimension D fixed.  ``min_weight`` is the trajectory mean of the smallest normalised Schmidt
weight across the bond: while it stays near zero the bond has room; once it is a visible fraction of 1 / D the bond is
too narrow and the entropy saturates towards ln D.  The script runs the same ensemble at two bond dimensions and prints
both columns side by side.  Runs on one MI355X.

    python examples/dephasing_chain_entropy.py [nsteps] [trajectories]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytdscf_amd import Exciton, Model, propagate_trajectories, units  # noqa: E402

L, J, GAMMA, DT = 8, 1.0, 0.05, 0.2  # sites, exchange, dephasing probability per site and step, time step (a.u.)
SX = np.array([[0, 1], [1, 0]], dtype=complex) / 2
SY = np.array([[0, -1j], [1j, 0]]) / 2
SZ = np.array([[1, 0], [0, -1]], dtype=complex) / 2
ID = np.eye(2, dtype=complex)


def heisenberg_mpo(fields):
    """(ml, d, d, mr) cores of J sum S_p . S_{p+1} + sum fields[p] S^z_p: the usual five-state automaton"""
    cores = []
    for p, h in enumerate(fields):
        w = np.zeros((5, 2, 2, 5), dtype=complex)
        w[0, :, :, 0] = w[4, :, :, 4] = ID
        for k, s in enumerate((SX, SY, SZ)):
            w[0, :, :, 1 + k] = s
            w[1 + k, :, :, 4] = J * s
        w[0, :, :, 4] = h * SZ
        cores.append(w[:1] if p == 0 else w)
    cores[-1] = cores[-1][..., 4:]
    return cores


def main():
    nsteps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    ntraj = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    mpo = heisenberg_mpo([0.1 * (p - (L - 1) / 2) for p in range(L)])
    dephasing = np.stack([np.sqrt(1 - GAMMA) * ID, np.sqrt(GAMMA) * 2 * SZ])  # sum B^+ B = 1
    neel = [[1, 0], [0, 1]] * (L // 2)
    half = L // 2 - 1  # the bond between sites L/2 - 1 and L/2
    cols = {}
    for D in (4, 16):
        model = Model([Exciton(nstate=2) for _ in range(L)], operators={"hamiltonian": mpo}, bond_dim=D)
        out = propagate_trajectories(model, [neel], maxstep=nsteps + 1, stepsize=DT * units.au_in_fs,
                                     reduced_density=([(half, half)], 2), integrator="arnoldi", conserve_norm=False,
                                     jumps={p: dephasing for p in range(L)}, seed=7, replicas_per_start=ntraj,
                                     entanglement=[half])
        cols[D] = (out["time"], out["entropy"][:, 0], out["min_weight"][:, 0])
    print(f"# {ntraj} trajectories, L = {L}, half-chain bond {half}; ln 4 = {np.log(4):.4f}, ln 16 = {np.log(16):.4f}")
    print("# time/fs   S1(D=4)   pmin(D=4)   S1(D=16)  pmin(D=16)")
    for k, t in enumerate(cols[4][0]):
        print(f"{t:9.4f}  {cols[4][1][k]:8.5f}  {cols[4][2][k]:9.2e}  {cols[16][1][k]:8.5f}  {cols[16][2][k]:9.2e}")
    gap = abs(cols[4][1][-1] - cols[16][1][-1])
    print(f"# the two bond dimensions differ by {gap:.2e} in the last entropy: "
          + ("D = 4 is enough so far" if cols[4][2][-1] < 1e-3 else "D = 4 is too narrow by now (its smallest weight is not small)"))


if __name__ == "__main__":
    main()
