#!/usr/bin/env python3
"""A J-aggregate of two-level molecules driven by a laser pulse of finite length, clean and under pure dephasing:

    H(t) = H_Frenkel + E(t) sum_p mu_p (|e_p><g_p| + h.c.)

E(t) is a Gaussian pulse resonant with the bright k = 1 exciton.  The dipole is a sum of one-site operators with one
time-dependent real amplitude, so ``propagate_trajectories(fields=...)`` applies it inside the batch as one-site
unitaries between the half-sweeps of every step (``k_batch_field``, one more launch per step), and the whole recorded
run waits for the host once.  The second run lets jump channels dephase the same molecules while the pulse acts: an
ensemble of quantum-jump trajectories.  A site takes one field; noise instead of a pulse -- ``dict(G=|e><e|, sigma=s,
tau=t)``, an Ornstein-Uhlenbeck process per molecule and trajectory: Kubo-Anderson dephasing with a memory, which no jump
channel expresses -- goes on sites the pulse does not touch.  Runs on one MI355X.

    python examples/pulse_driven_aggregate.py [ntraj] [dephasing_rate_per_fs]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytdscf_amd import Exciton, Model, units  # noqa: E402
from pytdscf_amd.kraus import lindblad_to_kraus  # noqa: E402
from pytdscf_amd.trajectories import propagate_trajectories  # noqa: E402

L, D = 6, 8
E0, J = 0.10, -0.004  # site energy and nearest-neighbour coupling (hartree); J < 0: a J-aggregate
DT_FS, T_FS = 0.05, 30.0
ID = np.eye(2, dtype=complex)
NUM = np.array([[0, 0], [0, 1]], dtype=complex)  # |e><e|
UP = np.array([[0, 0], [1, 0]], dtype=complex)   # |e><g|
SX = UP + UP.T


def frenkel_mpo():
    """(ml, d, d, mr) cores of sum_p E0 n_p + J sum_p (up_p down_{p+1} + h.c.): a four-state automaton"""
    cores = []
    for p in range(L):
        w = np.zeros((4, 2, 2, 4), dtype=complex)
        w[0, :, :, 0] = w[3, :, :, 3] = ID
        w[0, :, :, 1], w[1, :, :, 3] = UP, J * UP.T
        w[0, :, :, 2], w[2, :, :, 3] = UP.T, J * UP
        w[0, :, :, 3] = E0 * NUM
        cores.append(w[:1] if p == 0 else w)
    cores[-1] = cores[-1][..., 3:]
    return cores


def main():
    ntraj = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    rate = float(sys.argv[2]) if len(sys.argv) > 2 else 0.05  # pure dephasing, 1 / fs
    omega = E0 + 2 * J * np.cos(np.pi / (L + 1))  # the bright k = 1 exciton, hartree
    peak, centre, width = 0.004, 10.0, 3.0        # mu E in hartree; fs; fs

    def pulse(t_fs):  # the amplitude at a time in fs, in the Hamiltonian's unit
        return peak * np.exp(-0.5 * ((t_fs - centre) / width) ** 2) * np.cos(omega * (t_fs - centre) / units.au_in_fs)

    model = Model([Exciton(nstate=2) for _ in range(L)], operators={"hamiltonian": frenkel_mpo()}, bond_dim=D)
    ground = [[1, 0]] * L
    nsteps, every = int(round(T_FS / DT_FS)), 50
    keys = [(p, p) for p in range(L)]
    drive = {p: dict(G=SX, pulse=pulse) for p in range(L)}
    common = dict(maxstep=nsteps + 1, stepsize=DT_FS, reduced_density=(keys, every), integrator="arnoldi", conserve_norm=False,
                  fields=drive)

    clean = propagate_trajectories(model, [ground], **common)
    dt_au = DT_FS / units.au_in_fs
    deph = lindblad_to_kraus([np.sqrt(rate * units.au_in_fs) * NUM], dt_au)  # the rate per atomic unit of time
    noisy = propagate_trajectories(model, [ground], jumps={p: deph for p in range(L)}, replicas_per_start=ntraj, seed=1, **common)

    print(f"# pulse: peak {peak} hartree, centre {centre} fs, width {width} fs, carrier {omega:.5f} hartree (the k = 1 exciton)")
    print(f"# dephasing run: {ntraj} trajectories, rate {rate} / fs on every molecule")
    print("#  t / fs   excited population per molecule, clean aggregate" + " " * 19 + "| sum, clean | sum, dephased")
    for k, t in enumerate(clean["time"]):
        pc = [clean["mean"][key][k][1, 1].real for key in keys]
        pn = [noisy["mean"][key][k][1, 1].real for key in keys]
        print(f"{t:8.2f}   " + " ".join(f"{x:8.5f}" for x in pc) + f"   | {sum(pc):8.5f}   | {sum(pn):8.5f}")


if __name__ == "__main__":
    main()
