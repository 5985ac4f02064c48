#!/usr/bin/env python3
"""Time-resolved joint histogram of a dephasing Heisenberg chain from sampled configurations:

    Neel start  ->  quantum-jump trajectories of  H = J sum S_p . S_{p+1}  with dephasing on every site
                ->  at every record, `shots` configurations of EVERY trajectory (one basis index per site, drawn with the
                    state's own probabilities), i.e. a measurement record of all sites at once

From the configurations the script prints, per record: the distribution of the number of up spins in the left half of
the chain (full counting statistics of a conserved current's integral -- the total is conserved, the half is not), and
the probability of the three most frequent configurations of the whole chain.  Neither is a reduced density of a few
sites: both need the joint distribution of all L outcomes.  Runs on one MI355X.

    python examples/dephasing_chain_histogram.py [nsteps] [trajectories] [shots]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dephasing_chain_entropy import DT, GAMMA, ID, SZ, L, heisenberg_mpo  # noqa: E402
from pytdscf_amd import Exciton, Model, propagate_trajectories, units  # noqa: E402


def main():
    nsteps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    ntraj = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    shots = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    mpo = heisenberg_mpo([0.0] * L)
    dephasing = np.stack([np.sqrt(1 - GAMMA) * ID, np.sqrt(GAMMA) * 2 * SZ])  # sum B^+ B = 1
    neel = [[1, 0], [0, 1]] * (L // 2)
    model = Model([Exciton(nstate=2) for _ in range(L)], operators={"hamiltonian": mpo}, bond_dim=16)
    out = propagate_trajectories(model, [neel], maxstep=nsteps + 1, stepsize=DT * units.au_in_fs,
                                 reduced_density=([(0, 0)], 4), integrator="arnoldi", conserve_norm=False,
                                 jumps={p: dephasing for p in range(L)}, seed=7, replicas_per_start=ntraj,
                                 shots=shots, shot_seed=11)
    cfg = out["configurations"]  # (nrec, ntraj, shots, L); outcome 0 is spin up
    nrec = cfg.shape[0]
    flat = cfg.reshape(nrec, -1, L)
    print(f"# {ntraj} trajectories x {shots} shots, L = {L}; columns: P(n up spins in sites 0 .. {L // 2 - 1}), n = 0 .. {L // 2}")
    for q, t in enumerate(out["time"]):
        n_up = np.sum(flat[q, :, :L // 2] == 0, axis=1)
        hist = np.bincount(n_up, minlength=L // 2 + 1) / n_up.size
        codes, counts = np.unique(flat[q] @ (1 << np.arange(L)[::-1]), return_counts=True)
        top = np.argsort(-counts)[:3]
        names = "  ".join(f"{int(codes[k]):0{L}b}:{counts[k] / flat.shape[1]:.3f}" for k in top)
        print(f"{t:8.4f}  " + " ".join(f"{h:.4f}" for h in hist) + f"   most frequent (0 = up): {names}")
    total_up = np.sum(flat == 0, axis=2)
    print(f"# up spins in the whole chain: {total_up.min()} .. {total_up.max()} over all shots (conserved: {L // 2})")


if __name__ == "__main__":
    main()
