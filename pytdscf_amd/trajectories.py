"""Trajectory averages in one batch: the reference's trajectory workflows (a loop over start states, each run through
``Simulator.propagate(reduced_density=...)``, the densities averaged afterwards: tests/test_mixedstate.py:239-318) as ONE
``TDVPBatch`` whose observables and ensemble means are formed on the device (``mitdvp_batch_run``).

Nothing falls back: a model the batched kernels do not take raises with the library's message."""

from __future__ import annotations

import numpy as np

from . import units
from .engine import TDVPBatch
from .mps import product_state_cores


def _one_site_keys(keys, nsite):
    sites = []
    for key in keys:
        k = tuple(key)
        if len(k) != 2 or k[0] != k[1]:
            raise ValueError(f"reduced_density key {k}: the batch takes one-site keys (s, s) only")
        s = int(k[0])
        if not 0 <= s < nsite:
            raise ValueError(f"reduced_density key {k}: site out of range")
        sites.append(s)
    return sites


def propagate_trajectories(model, starts, maxstep, stepsize, reduced_density, weights=None, integrator="lanczos",
                           conserve_norm=True, per_trajectory=False, thresh_sil=1.0e-09, device=0):
    """Propagate every Hartree product of ``starts`` under ``model`` and average their one-site reduced densities.

    ``model``: a ``Model`` as the shell takes it (one electronic state, Hilbert space, no gates or Kraus maps);
    ``starts``: a list of Hartree products as ``Model.init_HartreeProduct[0]`` takes them; ``stepsize`` in fs;
    ``reduced_density = ([(s, s), ...], every)`` as ``Simulator.propagate`` takes it.  As there, the state is observed
    BEFORE steps 0, every, 2 every, ... < ``maxstep``; steps after the last observation are not run.
    Returns ``{"time": (nrec,) in fs, "mean": {key: (nrec, d, d)}}`` and, with ``per_trajectory``,
    ``"trajectories": {key: (nrec, len(starts), d, d)}``.  ``weights``: one number per start, default equal weights."""
    if integrator not in ("lanczos", "arnoldi"):
        raise ValueError(f"Invalid integrator: {integrator}")
    keys, every = reduced_density
    keys = [tuple(k) for k in keys]
    every = int(every)
    if every < 1 or maxstep < 1:
        raise ValueError("maxstep and the reduced-density interval must be >= 1")
    nsite = len(model.dims)
    key_sites = _one_site_keys(keys, nsite)
    if not keys:
        raise ValueError("reduced_density names no key")
    if model.nstate != 1 or model.space != "hilbert" or model.one_gate_to_apply is not None or model.kraus_op:
        raise NotImplementedError("propagate_trajectories: one electronic state in Hilbert space without gates or Kraus maps")
    starts = list(starts)
    if not starts:
        raise ValueError("no start states")
    sites = sorted(set(key_sites))
    dt_au = stepsize / units.au_in_fs
    nsteps = (maxstep - 1) // every * every
    D = model.m_aux_max if model.m_aux_max is not None else 10**9
    mpo = model.project_mpo(model.hamiltonian.as_mpo(model.dims))
    bt = TDVPBatch(len(starts), nsite, device=device, integrator=integrator, conserve_norm=conserve_norm, thresh=thresh_sil)
    try:
        for e, start in zip(bt.engines, starts):
            e.set_mpo(mpo, 0, shift=model.hamiltonian.coupleJ[0][0])
            e.set_mps(product_state_cores(start, D, space=model.space), canonicalize=True, scale=1.0)
        rec = bt.propagate(dt_au, nsteps, observe=dict(sites=sites, norm=False, weights=weights, per_replica=per_trajectory),
                           every=every)
    finally:
        bt.close()
    nrec = nsteps // every + 1
    out = {"time": np.arange(nrec) * every * dt_au * units.au_in_fs,
           "mean": {k: rec["mean_rdm"][sites.index(s)] for k, s in zip(keys, key_sites)}}
    if per_trajectory:
        out["trajectories"] = {k: rec["rdm"][sites.index(s)] for k, s in zip(keys, key_sites)}
    return out
