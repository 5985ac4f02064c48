#!/usr/bin/env python3
"""Dipole-dipole correlation function and absorption spectrum of a short exciton chain (a J-aggregate of two-level
molecules), with the total dipole -- a sum over the chain -- on both sides:

    |g ... g>  ->  C(t) = <g| mu(t) mu |g>,   mu = sum_p mu_p (|e_p><g_p| + |g_p><e_p|)
               ->  I(omega) by the windowed transform of pytdscf_amd.spectra

``correlation_function`` takes ``A`` and ``B`` by the name of an entry of ``model.observables``.  ``B psi`` is built on
the host as an exact MPS of the dipole MPO's bond (2), ``A`` is given to every replica as operator 1 and
``<psi(t)| mu |phi(t)>`` is contracted on the device at every step by one launch (``k_batch_cross_mpo``).  In the
one-exciton manifold the aggregate is a tight-binding chain, so the bright states and their oscillator strengths are
known in closed form; the script prints them next to the peaks it finds.  Runs on one MI355X.

    python examples/aggregate_dipole_correlation.py [nsteps] [spectrum.dat]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytdscf_amd import Exciton, Model, spectra, units  # noqa: E402
from pytdscf_amd.trajectories import correlation_function  # noqa: E402

L, D = 6, 8
E0, J = 0.10, -0.004  # site energy and nearest-neighbour coupling (hartree); J < 0: a J-aggregate
DT_FS = 0.05
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


def dipole_mpo(mu):
    """sum_p mu[p] (|e_p><g_p| + |g_p><e_p|): bond 2"""
    cores = []
    for p in range(L):
        w = np.zeros((2, 2, 2, 2), dtype=complex)
        w[0, :, :, 0] = w[1, :, :, 1] = ID
        w[0, :, :, 1] = mu[p] * SX
        cores.append(w[:1] if p == 0 else w)
    cores[-1] = cores[-1][..., 1:]
    return cores


def main():
    nsteps = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
    mu = np.ones(L)
    model = Model([Exciton(nstate=2) for _ in range(L)], operators={"hamiltonian": frenkel_mpo(), "dipole": dipole_mpo(mu)}, bond_dim=D)
    ground = [[1, 0]] * L
    out = correlation_function(model, [ground], maxstep=nsteps + 1, stepsize=DT_FS, A="dipole", B="dipole")
    t, c = out["time"], out["mean"]
    print(f"# C(0) = {c[0].real:.6f} (sum of mu_p^2 = {np.sum(mu ** 2):.6f}); {len(t)} records of {DT_FS} fs")
    wn, inten = spectra.ifft_autocorr(t, c / c[0])
    if len(sys.argv) > 2:
        spectra.export_spectrum(wn, inten, sys.argv[2])
    # the one-exciton states of the open chain: E_k = E0 + 2 J cos(k pi / (L + 1)), strength |sum_p mu_p sin(k pi p / (L + 1))|^2
    k = np.arange(1, L + 1)
    ek = E0 + 2 * J * np.cos(k * np.pi / (L + 1))
    fk = np.array([abs(np.sum(mu * np.sin(kk * np.pi * np.arange(1, L + 1) / (L + 1)))) ** 2 * 2 / (L + 1) for kk in k])
    au_to_cm1 = 219474.6313705
    print("# exact one-exciton lines:  k   wave number / cm-1   oscillator strength / sum mu^2")
    for kk, e, f in zip(k, ek, fk):
        if f > 1e-12:
            print(f"#                          {kk}   {e * au_to_cm1:14.1f}   {f / np.sum(mu ** 2):.4f}")
    peak = wn[int(np.argmax(inten))]
    width = 1.0 / (t[-1] * 1e-15 * 2.99792458e10)  # the window's resolution, 1 / (c T), in cm-1
    print(f"# strongest peak of the spectrum at {peak:.1f} cm-1, the k = 1 line at {ek[0] * au_to_cm1:.1f} cm-1 "
          f"(resolution of {t[-1]:.0f} fs: about {width:.0f} cm-1); a J-aggregate carries most of its strength in k = 1")


if __name__ == "__main__":
    main()
