"""Trajectory averages in one batch: the reference's trajectory workflows (a loop over start states, each run through
``Simulator.propagate(reduced_density=...)``, the densities averaged afterwards: tests/test_mixedstate.py:239-318) as ONE
``TDVPBatch`` whose observables and ensemble means are formed on the device (``mitdvp_batch_run``).

One-site gates (``Model(one_gate_to_apply=...)``) and sampled one-site Kraus channels (``jumps=``: quantum-jump
trajectories at Hilbert-space cost) act between the two half-sweeps of every step, inside the batch (``k_batch_channel``);
so do sampled nearest-neighbour channels (``jumps={(q, q + 1): B}``: incoherent hopping, correlated decay), which the batch
applies to the merged two-site tensor and splits again at the bond's dimension (``k_batch_pair``).  Time-dependent one-site
terms (``fields=``: a laser pulse of finite length, Ornstein-Uhlenbeck noise per trajectory and site) act in the same slot
as one-site unitaries applied in place (``k_batch_field``); ``field_normal`` / ``field_noise_path`` restate their generator.

``correlation_function`` relates two states of the batch to each other: the autocorrelation function without the t/2
trick and ``<psi| A(t) B |psi>``, contracted for all trajectories by one launch per record (``k_batch_cross``; ``k_batch_cross_mpo``
when ``A`` is a sum over the chain given as an MPO).

``relax_trajectories`` is the first link of relax -> dipole -> propagate over an ensemble: the ground states of a list of
models (static disorder) by improved relaxation, all in one launch (``k_batch_relax``).

Nothing falls back: a model the batched kernels do not take raises with the library's message."""

from __future__ import annotations

import numpy as np

from . import units
from .engine import TDVPBatch, density_key_legs, operate_request, pair_key, sample_request, spectra_bonds
from .mps import bond_dims, product_state_cores


_M64 = (1 << 64) - 1


def _mix(z: int) -> int:
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return z


def jump_uniform(seed: int, trajectory_id: int, step: int, site: int) -> float:
    """The uniform in [0, 1) that ``k_batch_channel`` draws for the jump channel on ``site`` of trajectory
    ``trajectory_id`` in time step ``step`` (completed steps since the seed was set): counter-based, no state --
    ``key = mix(mix(mix(seed ^ trajectory_id) + step) + site)``, ``u = (key >> 11) * 2**-53`` on 64-bit unsigned integers."""
    seed, trajectory_id, step, site = (int(x) & _M64 for x in (seed, trajectory_id, step, site))
    key = _mix((_mix((_mix(seed ^ trajectory_id) + step) & _M64) + site) & _M64)
    return (key >> 11) * 2.0 ** -53


def sample_uniform(seed: int, trajectory_id: int, step: int, site: int, shot: int) -> float:
    """The uniform in [0, 1) that ``k_batch_sample`` draws at ``site`` for shot ``shot`` of trajectory ``trajectory_id``
    when the batch has completed ``step`` time steps since the seed was set: one more level of ``jump_uniform``'s counter
    scheme, with the samples request's own ``seed`` --
    ``key = mix(mix(mix(mix(seed ^ trajectory_id) + step) + site) + shot)``, ``u = (key >> 11) * 2**-53``."""
    seed, trajectory_id, step, site, shot = (int(x) & _M64 for x in (seed, trajectory_id, step, site, shot))
    key = _mix((_mix((_mix((_mix(seed ^ trajectory_id) + step) & _M64) + site) & _M64) + shot) & _M64)
    return (key >> 11) * 2.0 ** -53


def field_normal(seed: int, trajectory_id: int, step: int, site: int, nsite: int) -> float:
    """The standard normal that ``k_batch_field`` draws for the noise on ``site`` of trajectory ``trajectory_id`` in time
    step ``step`` (completed steps since the seed was set): ``z = sqrt(-2 log1p(-u1)) cos(2 pi u2)`` with
    ``u1 = jump_uniform(seed, id, step, 2 nsite + 2 site)`` and ``u2 = jump_uniform(seed, id, step, 2 nsite + 2 site + 1)``
    -- keys that meet neither the one-site jump keys ``0 .. nsite-1`` nor the pair keys ``nsite .. 2 nsite - 2``."""
    import math

    key = 2 * int(nsite) + 2 * int(site)
    u1, u2 = jump_uniform(seed, trajectory_id, step, key), jump_uniform(seed, trajectory_id, step, key + 1)
    return math.sqrt(-2.0 * math.log1p(-u1)) * math.cos(6.283185307179586 * u2)


def field_noise_path(seed: int, trajectory_id: int, site: int, nsite: int, sigma: float, tau: float, dts, first_step: int = 0):
    """The Ornstein-Uhlenbeck amplitudes ``k_batch_field`` applies on ``site`` of trajectory ``trajectory_id`` in the time
    steps of lengths ``dts`` that follow a reset of the field clock (``set_fields`` or ``set_jumps``) made when the
    batch's step counter stood at ``first_step``: ``xi_0 = sigma z_0``, ``xi_n = a_n xi_{n-1} + sigma sqrt(1 - a_n^2) z_n``
    with ``a_n = exp(-|dt_n| / tau)`` (``tau = 0``: 0, white noise) and ``z_n = field_normal(seed, id, first_step + n, site,
    nsite)``.  ``tau`` in the unit of ``dts``.  Returns an array ``(len(dts),)``."""
    import math

    out, xi = [], 0.0
    for n, dt in enumerate(dts):
        z = field_normal(seed, trajectory_id, first_step + n, site, nsite)
        if n == 0:
            xi = sigma * z
        else:
            a = math.exp(-abs(dt) / tau) if tau > 0.0 else 0.0
            xi = a * xi + (sigma * math.sqrt(1.0 - a * a)) * z
        out.append(xi)
    return np.array(out, dtype=np.float64)


def pulse_table(f, stepsize: float, nsteps: int, t0: float = 0.0):
    """Midpoint samples of a pulse shape for ``TDVPBatch.set_fields``: ``f(t0 + (n + 1/2) stepsize)`` for
    ``n = 0 .. nsteps - 1``, the amplitude the symmetric splitting wants for the step from ``t0 + n stepsize`` on."""
    nsteps = int(nsteps)
    if nsteps < 1:
        raise ValueError("pulse_table: nsteps must be >= 1")
    return np.array([float(f(t0 + (n + 0.5) * stepsize)) for n in range(nsteps)], dtype=np.float64)


def _field_table(fields, dims, nrep, stepsize, nsteps):
    """``fields`` of ``propagate_trajectories`` / ``correlation_function`` as ``TDVPBatch.set_fields`` takes it, checked
    before any engine exists (``engine.field_request``): a callable ``pulse`` becomes its midpoint table over the run
    (time in the unit of ``stepsize``), ``tau`` goes from the unit of ``stepsize`` to atomic units."""
    from .engine import field_request

    table = {}
    for site, spec in dict(fields or {}).items():
        if isinstance(spec, dict):
            spec = dict(spec)
            if callable(spec.get("pulse")):
                spec["pulse"] = pulse_table(spec["pulse"], stepsize, max(nsteps, 1))
            if spec.get("tau") is not None and spec.get("sigma") is not None:
                try:
                    spec["tau"] = float(spec["tau"]) / units.au_in_fs
                except (TypeError, ValueError):
                    pass  # field_request names it
        table[site] = spec
    field_request(table, dims, nrep)
    return table


def _jump_table(jumps, dims):
    """{site: (K, d, d) complex, (q, q + 1): (K, d0 d1, d0 d1) complex} checked against the model's dimensions and the
    kernel's limits, before any engine exists"""
    from ._lib import MAX_JUMP

    table = {}
    for site, B in dict(jumps).items():
        if isinstance(site, (tuple, list)):  # a pair channel on the bond (q, q + 1)
            key = pair_key(site, len(dims))
            d0, d1 = dims[key[0]], dims[key[1]]
            B = np.asarray(B, dtype=np.complex128)
            if B.ndim == 5 and B.shape[1:] == (d0, d1, d0, d1):
                B = B.reshape(B.shape[0], d0 * d1, d0 * d1)
            if B.ndim != 3 or B.shape[1] != B.shape[2]:
                raise ValueError(f"jumps[{key}] must have shape (K, d0 d1, d0 d1) or (K, d0, d1, d0, d1) with d0, d1 = {d0}, {d1}; "
                                 f"got {B.shape}")
            if B.shape[1] != d0 * d1:
                raise ValueError(f"jumps[{key}]: the operators are of order {B.shape[1]}, the sites' dimensions are {d0} x {d1} "
                                 f"(order {d0 * d1})")
            if not 2 <= B.shape[0] <= MAX_JUMP:
                raise ValueError(f"jumps[{key}]: a jump channel has 2 to {MAX_JUMP} operators, got {B.shape[0]}")
            table[key] = B
            continue
        site = int(site)
        if not 0 <= site < len(dims):
            raise ValueError(f"jumps: site {site} is out of range")
        B = np.asarray(B, dtype=np.complex128)
        if B.ndim != 3 or B.shape[1] != B.shape[2]:
            raise ValueError(f"jumps[{site}] must have shape (K, d, d), got {B.shape}")
        if B.shape[1] != dims[site]:
            raise ValueError(f"jumps[{site}]: the operators are {B.shape[1]} x {B.shape[1]}, the site's dimension is {dims[site]}")
        if not 2 <= B.shape[0] <= MAX_JUMP:
            raise ValueError(f"jumps[{site}]: a jump channel has 2 to {MAX_JUMP} operators, got {B.shape[0]}")
        table[site] = B
    return table


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


def _site_operator(name, op, dims):
    site, mat = op
    site = int(site)
    if not 0 <= site < len(dims):
        raise ValueError(f"correlation_function: {name} acts on site {site}, the chain has sites 0 .. {len(dims) - 1}")
    mat = np.asarray(mat, dtype=np.complex128)
    if mat.shape != (dims[site], dims[site]):
        raise ValueError(f"correlation_function: {name} has shape {mat.shape}, site {site} takes ({dims[site]}, {dims[site]})")
    return site, mat


def _operator_form(name, op, model, dims):
    """("site", site, matrix) for ``(site, matrix)``; ("mpo", cores) for the name of an entry of ``model.observables`` or a
    list of MPO cores (ml, d, d, mr per site).  ``ValueError`` naming what is wrong, before any engine exists."""
    if isinstance(op, str):
        have = getattr(model, "observables", None) or {}
        if op not in have:
            raise ValueError(f"correlation_function: {name} = {op!r} is not in model.observables (it has {sorted(have)})")
        cores = have[op].as_mpo(dims)
    elif (isinstance(op, (tuple, list)) and len(op) == 2 and isinstance(op[0], (int, np.integer)) and not isinstance(op[0], bool)):
        return ("site",) + _site_operator(name, op, dims)
    else:
        try:
            cores = list(op)
        except TypeError:
            raise ValueError(f"correlation_function: {name} must be (site, matrix), the name of an entry of model.observables "
                             "or a list of MPO cores") from None
    cores = [np.ascontiguousarray(w, dtype=np.complex128) for w in cores]
    if len(cores) != len(dims):
        raise ValueError(f"correlation_function: {name} has {len(cores)} MPO cores, the chain has {len(dims)} sites")
    left = 1
    for p, (w, d) in enumerate(zip(cores, dims)):
        if w.ndim != 4 or w.shape[1] != d or w.shape[2] != d or w.shape[0] != left:
            raise ValueError(f"correlation_function: {name}: the MPO core of site {p} has shape {w.shape}, expected "
                             f"({left}, {d}, {d}, m)")
        left = w.shape[3]
    if left != 1:
        raise ValueError(f"correlation_function: {name}: the last MPO core ends in a bond of {left}, it must be 1")
    return "mpo", cores


def check_mpo_fits_bonds(name, cores, dims, D):
    """``ValueError`` naming the bond and both figures when the MPO is wider somewhere than the state's bond there: the
    product ``B psi`` is an exact MPS of the MPO's bonds and must fit the bond dimensions of ``model.m_aux_max``."""
    for q, ((_, dr), w) in enumerate(zip(bond_dims(list(dims), D), cores[:-1])):
        if w.shape[3] > dr:
            raise ValueError(f"correlation_function: {name} has MPO bond {w.shape[3]} between sites {q} and {q + 1}, the state's "
                             f"bond there is {dr} (model.m_aux_max): B psi does not fit")


def mpo_on_product(cores, vectors):
    """The cores of ``B psi`` for the MPO ``cores`` and the Hartree product of ``vectors`` (each normalised first):
    ``phi_p[c, i, t] = sum_j W_p[c, i, j, t] v_p[j]``, an exact MPS of the MPO's bonds, with the norm of ``B psi``."""
    out = []
    for w, v in zip(cores, vectors):
        v = np.asarray(v, dtype=np.complex128)
        if v.ndim != 1:
            raise ValueError("correlation_function: an MPO B acts on a start given as per-site vectors")
        out.append(np.einsum("cijt,j->cit", w, v / np.linalg.norm(v)))
    return out


def core_starts(starts, dims, D):
    """``None`` when every start is a Hartree product (one vector per site).  Otherwise every start must be an MPS, one
    ``(dl, d, dr)`` array per site, and the result is the starts as complex cores zero-padded to the bond dimensions of
    ``model.m_aux_max`` (``bond_dims(dims, D)``), the shapes every replica of a batch shares.  ``ValueError`` naming the
    start, the site and the limit for a site that is not of rank 3 (vectors and cores may not be mixed), a physical
    dimension that is not the model's, neighbouring bonds that do not fit, outer bonds that are not 1, and a bond above
    what ``model.m_aux_max`` allows there.  Pure Python: raised before any engine exists."""
    starts = [list(s) for s in starts]
    if all(np.ndim(c) == 1 for s in starts for c in s):
        return None
    full = bond_dims(list(dims), D)
    out = []
    for k, s in enumerate(starts):
        who = f"correlation_function: start {k}"
        if len(s) != len(dims):
            raise ValueError(f"{who} has {len(s)} cores, the chain has {len(dims)} sites")
        left, cores = 1, []
        for p, (c, d) in enumerate(zip(s, dims)):
            c = np.asarray(c, dtype=np.complex128)
            if c.ndim != 3:
                raise ValueError(f"{who}, site {p}: an MPS core is (dl, d, dr), got an array of rank {c.ndim} (shape {c.shape}); "
                                 "a start is cores at every site or vectors at every site, and so are all starts")
            if c.shape[1] != d:
                raise ValueError(f"{who}, site {p}: the core has physical dimension {c.shape[1]}, the model's is {d}")
            if c.shape[0] != left:
                raise ValueError(f"{who}, site {p}: the core has the left bond {c.shape[0]}, expected {left}")
            if c.shape[2] > full[p][1]:
                raise ValueError(f"{who}: bond {c.shape[2]} between sites {p} and {p + 1} is above {full[p][1]}, what "
                                 f"model.m_aux_max = {D} allows there")
            left = c.shape[2]
            z = np.zeros((full[p][0], d, full[p][1]), dtype=np.complex128)
            z[:c.shape[0], :, :c.shape[2]] = c
            cores.append(z)
        if left != 1:
            raise ValueError(f"{who}: the last core ends in a bond of {left}, it must be 1")
        out.append(cores)
    return out


def site_operator_mpo(site, mat, dims):
    """the one-site operator ``mat`` on ``site`` as an MPO of bond 1: identity cores elsewhere"""
    return [(np.asarray(mat, dtype=np.complex128) if p == site else np.eye(d, dtype=np.complex128))[None, :, :, None].copy()
            for p, d in enumerate(dims)]


def _mps_norm(cores):
    T = np.ones((1, 1), dtype=np.complex128)
    for c in cores:
        T = np.einsum("ab,ajs,bjt->st", T, np.conj(c), c)
    return float(np.sqrt(abs(T[0, 0])))


def correlation_function(model, starts, maxstep, stepsize, A=None, B=None, every=1, weights=None, integrator="arnoldi",
                         conserve_norm=False, thresh_sil=1.0e-09, per_trajectory=False, device=0, operate_maxstep=10,
                         operate_tol=1.0e-8, fields=None):
    """Two-time correlation functions of an ensemble of Hartree products in ONE batch, contracted and averaged on the device
    (``k_batch_cross``, ``mitdvp_batch_run``): no t/2 trick, so complex starts and Hamiltonians that are not complex
    symmetric are fine.

    ``A`` and ``B`` each take one of three forms: ``(site, matrix)``, a one-site operator; the name of an entry of
    ``model.observables``; or a list of MPO cores ``(ml, d, d, mr)``, one per site.  A named observable is turned into an
    MPO as ``propagate_trajectories`` prepares it (``op.as_mpo(model.dims)``, no scalar term): the total dipole of an
    aggregate, a current, the Hamiltonian.  An MPO ``A`` is given to every replica as operator 1 and evaluated by
    ``k_batch_cross_mpo`` (``TDVPBatch.set_cross_mpo``), one workgroup per start.  An MPO ``B`` is applied to each Hartree
    product on the host: ``phi_p[c, i, t] = sum_j W_p[c, i, j, t] v_p[j]`` is an exact MPS of the MPO's bonds, zero-padded
    to the bond dimensions of ``model.m_aux_max`` and set with its own norm ``|B psi|``; an MPO bond wider than the state's
    bond there is a ``ValueError`` naming the bond and both figures, as are an unknown name and a start that ``B``
    annihilates, all raised before any engine exists.  The forms may be mixed, and with both
    ``(site, matrix)`` everything is as it was.

    With both given, every start ``s`` gives two replicas, ``psi_s(0)`` = the start and
    ``phi_s(0) = B psi_s(0)`` -- still a Hartree product: ``B`` acts on that site's vector, and the product is set with
    its own norm ``|B psi_s(0)|`` -- and the value is ``C(t) = sum_s w_s <psi_s(t)| A |phi_s(t)>``, i.e.
    ``<psi| A(t) B |psi>`` for a Hamiltonian that generates a unitary propagation.  With both ``None`` there is one
    replica per start and a snapshot at t = 0: ``C(t) = sum_s w_s <psi_s(0)|psi_s(t)>``, the autocorrelation function.
    ``weights``: one number per start, default equal weights.

    A start may also be a correlated state: MPS cores, one ``(dl, d, dr)`` array per site, with bonds inside
    ``model.m_aux_max`` (a relaxed ground state, a propagated state, any MPS; all starts are then given so).  It is
    zero-padded to the model's bond dimensions, brought to canonical form and normalised, as a Hartree product is.  For
    such starts ``B`` in any of its three forms is applied ON THE DEVICE: ``phi_s`` is set as a copy of ``psi_s``, ``B`` is
    given to every replica as operator 2 (a one-site ``B`` as an MPO of bond 1), and one ``TDVPBatch.operate`` over the
    ``phi`` replicas (``k_batch_operate``, one launch) replaces each by the normalised fit of ``B psi_s`` in the bond
    dimensions of ``psi_s``, up to ``operate_maxstep`` double sweeps, stopped per start at ``operate_tol``.  The norms
    ``|B psi_s|`` it returns multiply the weights of the cross entries, and the ``per_trajectory`` values on the host; the
    tensors are not rescaled.  The fit is exact only where ``B psi`` fits the bonds -- there is no ``ValueError`` for an
    MPO wider than the bond here, the state is the best one the bonds hold after those sweeps.  A start that ``B``
    annihilates raises with the library's message, naming the replica.  Everything for Hartree products is as it was.

    ``model``, ``starts``, ``stepsize`` (fs) and the observation convention are those of ``propagate_trajectories``: the
    states are observed BEFORE steps 0, every, 2 every, ... < ``maxstep``; steps after the last observation are not run.
    ``model.one_gate_to_apply`` (one-site gates) acts on both replicas of a start.  The defaults differ on purpose:
    ``conserve_norm=False`` because ``phi`` carries the norm of ``B psi`` and an absorbing Hamiltonian must be allowed to
    shrink both, and ``integrator="arnoldi"`` because a product state padded to the bond dimension has a null space that
    Lanczos' three-term recurrence does not keep out of the Krylov vectors.

    Returns ``{"time": (nrec,) in fs, "mean": (nrec,) complex}`` and, with ``per_trajectory``, ``"trajectories"``
    ``(nrec, len(starts))``.

    ``fields``: time-dependent one-site terms ``H(t) = H0 + sum_p a_p(t) G_p`` as ``propagate_trajectories`` takes them; they
    act on both replicas of a start.  A per-replica ``pulse`` has one row per REPLICA (two per start with ``A`` and ``B``),
    and noise is drawn per replica: ``psi_s`` and ``phi_s`` see different paths, so only a shared ``pulse`` gives
    ``<psi| A(t) B |psi>`` of one driven system.

    There is no ``jumps`` argument: under sampled jump channels ``psi`` and ``phi`` would have to jump together with
    probabilities of the pair, which is a different scheme from the independent sampling of ``propagate_trajectories``.
    A model the batched kernels do not take raises with the library's message; nothing falls back."""
    if integrator not in ("lanczos", "arnoldi"):
        raise ValueError(f"Invalid integrator: {integrator}")
    every = int(every)
    if every < 1 or maxstep < 1:
        raise ValueError("maxstep and every must be >= 1")
    if (A is None) != (B is None):
        raise ValueError("correlation_function: give both A and B, or neither (the autocorrelation function)")
    if model.nstate != 1 or model.space != "hilbert":
        raise NotImplementedError("correlation_function: one electronic state in Hilbert space")
    if model.kraus_op:
        raise NotImplementedError("correlation_function: kraus_op means a purified state (a Kraus leg that grows)")
    dims = list(model.dims)
    nsite = len(dims)
    D = model.m_aux_max if model.m_aux_max is not None else 10**9
    a_mpo = b_mpo = None
    starts = [list(s) for s in starts]
    mps_starts = core_starts(starts, dims, D)  # None: Hartree products, everything below as it was
    if mps_starts is not None:
        operate_request(2 * len(starts), 2, operate_maxstep, operate_tol)  # a bad maxstep or tolerance raises here
    if A is not None:
        fa, fb = _operator_form("A", A, model, dims), _operator_form("B", B, model, dims)
        A = fa[1:] if fa[0] == "site" else None
        B = fb[1:] if fb[0] == "site" else None
        a_mpo = fa[1] if fa[0] == "mpo" else None
        b_mpo = fb[1] if fb[0] == "mpo" else None
        if b_mpo is not None and mps_starts is None:
            check_mpo_fits_bonds("B", b_mpo, dims, D)
    two = A is not None or a_mpo is not None
    if not starts:
        raise ValueError("no start states")
    ns = len(starts)
    w = np.full(ns, 1.0 / ns) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.shape != (ns,):
        raise ValueError(f"weights must be {ns} numbers, one per start (got shape {w.shape})")
    # replica 2 s is psi_s, replica 2 s + 1 is phi_s = B psi_s with its norm
    states, scales = [], []
    on_device = mps_starts is not None and two  # B is applied by TDVPBatch.operate
    if on_device:
        b_cores = b_mpo if b_mpo is not None else site_operator_mpo(B[0], B[1], dims)
    for s in mps_starts or []:  # psi_s and, with A and B, the copy of it that becomes phi_s
        states += [s, s] if two else [s]
    for k, s in enumerate(starts if mps_starts is None else []):
        states.append(s)
        scales.append(1.0)
        if b_mpo is not None:
            phi = mpo_on_product(b_mpo, s)
            # |B psi| <= prod_p |W_p|_F for a normalised product: below 1e-14 of that it is rounding of the MPO's cores
            if _mps_norm(phi) <= 1e-14 * float(np.prod([np.linalg.norm(w) for w in b_mpo])):
                raise ValueError(f"correlation_function: B annihilates start {k}")
            states.append(phi)
            scales.append(None)
        elif B is not None:
            v = np.asarray(s[B[0]], dtype=np.complex128)
            if v.ndim != 1:
                raise ValueError("correlation_function: B acts on a start given as per-site vectors")
            bv = B[1] @ (v / np.linalg.norm(v))
            if np.linalg.norm(bv) == 0.0:
                raise ValueError(f"correlation_function: B annihilates start {k}")
            states.append(s[:B[0]] + [bv] + s[B[0] + 1:])
            scales.append(float(np.linalg.norm(bv)))
    gates = model.one_gate_to_apply.one_site_gates(model.dims) if model.one_gate_to_apply is not None else {}
    dt_au = stepsize / units.au_in_fs
    nsteps = (maxstep - 1) // every * every
    field_table = _field_table(fields, dims, len(states), stepsize, nsteps)
    mpo = model.project_mpo(model.hamiltonian.as_mpo(model.dims))
    bt = TDVPBatch(len(states), nsite, device=device, integrator=integrator, conserve_norm=conserve_norm, thresh=thresh_sil)
    norms = None
    try:
        for i, (e, s) in enumerate(zip(bt.engines, states)):
            e.set_mpo(mpo, 0, shift=model.hamiltonian.coupleJ[0][0])
            if a_mpo is not None:
                e.set_mpo(a_mpo, 1)
            if mps_starts is None:
                e.set_mps(product_state_cores(s, D, space=model.space), canonicalize=True, scale=scales[i])
                continue
            if on_device:
                e.set_mpo(b_cores, 2)
            if not two or i % 2 == 0:  # a start is brought to canonical form once; phi_s gets those very tensors
                e.set_mps(s, canonicalize=True, scale=1.0)
                canonical = e.get_mps()
            else:
                e.set_mps(canonical)
        if gates:
            bt.set_gates(gates)
        if on_device:
            norms = bt.operate(2, operate_maxstep, operate_tol, replicas=range(1, 2 * ns, 2))["norms"][1::2].copy()
            w = w * norms
        key = "cross"
        if a_mpo is not None:
            key = "cross_mpo"
            bt.set_cross_mpo([(2 * k, 2 * k + 1, 1) for k in range(ns)])
        elif two:
            bt.set_cross([(2 * k, 2 * k + 1, A[0], A[1]) for k in range(ns)])
        else:
            bt.snapshot()
            bt.set_cross([(bt.snap(k), k) for k in range(ns)])
        if field_table:  # after operate and the snapshot: the field clock starts with the run
            bt.set_fields(field_table)
        rec = bt.propagate(dt_au, nsteps, observe={"norm": False, "per_replica": False, key: True, key + "_weights": w}, every=every)
    finally:
        bt.close()
    nrec = nsteps // every + 1
    out = {"time": np.arange(nrec) * every * dt_au * units.au_in_fs, "mean": rec["mean_" + key]}
    if per_trajectory:
        out["trajectories"] = rec[key] if norms is None else rec[key] * norms[None, :]
    return out


def relax_trajectories(models, starts=None, maxstep=20, conv_tol=1.0e-10, thresh_sil=1.0e-09, device=0, max_diag_krylov=0,
                       max_restarts=0, nstates=1, penalty=None, seed=0):
    """Ground states of an ensemble by improved relaxation in ONE batch and one launch (``TDVPBatch.relax``,
    ``k_batch_relax``): the reference's ``Simulator.relax(improved=True)`` for every realisation at once.

    ``models``: one model, or a list of models of equal site dimensions, ``m_aux_max`` and MPO bonds -- one replica each
    with its own Hamiltonian (static disorder).  ``starts``: one start per replica, Hartree products (one vector per site)
    or MPS cores as ``core_starts`` takes them (``correlation_function`` explains both); default: each model's own initial
    state, ``init_HartreeProduct`` padded to ``m_aux_max``.  A replica stops on its own once its energy changes by no
    more than ``conv_tol`` from one step to the next, ``maxstep`` steps at the most; ``thresh_sil`` is the threshold of
    the local Lanczos solver.  ``max_diag_krylov``: the most Krylov vectors of one local solve, 2 .. 64 (0: 64);
    ``max_restarts``: the restarts such a solve may take before its replica gives up (``TDVPBatch.set_relax_restarts``;
    0: none).  From random or product starts some realisations need more than 64 vectors at a site: a few restarts let
    them through, and with restarts a small ``max_diag_krylov`` (a scratch area per replica of ``max_diag_krylov + 1``
    site tensors) converges too, at more applies.

    Returns ``{"energy": (B,), "steps": (B,) int, "history": (B, maxstep) with NaN behind a replica's stop, "states":
    [cores of replica 0, ...]}``; the states are normalised MPS cores with the centre at site 0, in the form
    ``correlation_function(starts=...)`` and ``propagate_trajectories`` accept.  The energies contain the Hamiltonian's
    scalar term.  With ``max_restarts > 0`` there is also ``"restarts"``: (B,) int64, the restarts every replica took.
    A model the batch does not take raises with the library's message; nothing falls back.

    ``nstates > 1``: the lowest ``nstates`` eigenstates of every realisation by deflation (``TDVPBatch.deflate_push``,
    ``k_batch_relax_defl``), at most 9.  State 0 relaxes as above; then, for every further state, the states found so far
    are stored with the weight ``penalty``, every replica gets a fresh start, and the batch relaxes again on
    ``H + penalty * sum_j |j><j|``.  ``penalty`` is required then: a scalar, or one value per model.  It must EXCEED the
    largest gap wanted, ``E_(nstates-1) - E_0``: a weight that is too small makes a higher root fall back onto a lower
    state (the ``"overlaps"`` show it).  ``starts`` then holds one entry per state, ``starts[k][replica]`` or ``None``
    for the default of that state: state 0 starts as above and state ``k > 0`` from the engine's ``init_random`` seeded
    from ``(seed, k, replica)`` -- never from the converged lower state, which is an exact eigenvector of the penalised operator
    (eigenvalue ``E + penalty``) on which the Lanczos solve stops at once.  The return value then has the keys above for
    the LAST state (``"energy"`` is its Ritz value, the energy plus the penalties, which vanish at convergence) and
    ``"energies"`` ``(nstates, B)``: ``<psi|H|psi>`` from the batch's energy observable; ``"overlaps"`` ``(nstates,
    nstates, B)``: ``<state j|state k>`` of the final states; ``"states"``: for each state the list of per-replica MPS
    cores.  The deflation set is cleared before the call returns."""
    models = list(models) if isinstance(models, (list, tuple)) else [models]
    if not models:
        raise ValueError("relax_trajectories: no model")
    nstates = int(nstates)
    if nstates < 1 or nstates > 9:
        raise ValueError(f"relax_trajectories: nstates = {nstates}, it must be in 1 .. 9 (the ground state and 8 stored states)")
    if nstates > 1:
        if penalty is None:
            raise ValueError("relax_trajectories: nstates > 1 needs penalty, a weight above the largest gap wanted")
        pen = np.broadcast_to(np.asarray(penalty, dtype=np.float64), (len(models),)).copy()
        if not (np.all(np.isfinite(pen)) and np.all(pen > 0.0)):
            raise ValueError("relax_trajectories: penalty must be finite and > 0")
        state_starts = [None] * nstates if starts is None else [None if s is None else [list(c) for c in s] for s in starts]
        if len(state_starts) != nstates:
            raise ValueError(f"relax_trajectories: {len(state_starts)} entries of starts for {nstates} states (starts[k][replica])")
        for k, sk in enumerate(state_starts):
            if sk is not None and len(sk) != len(models):
                raise ValueError(f"relax_trajectories: {len(sk)} starts of state {k} for {len(models)} models (one start per replica)")
        starts = state_starts[0]
    m0 = models[0]
    dims = list(m0.dims)
    nsite = len(dims)
    D = m0.m_aux_max if m0.m_aux_max is not None else 10**9
    for k, m in enumerate(models):
        if m.nstate != 1 or m.space != "hilbert":
            raise NotImplementedError(f"relax_trajectories: model {k}: one electronic state in Hilbert space")
        if list(m.dims) != dims or m.m_aux_max != m0.m_aux_max:
            raise ValueError(f"relax_trajectories: model {k} has dims {list(m.dims)} and m_aux_max {m.m_aux_max}, model 0 has "
                             f"{dims} and {m0.m_aux_max}: the replicas of a batch share their shapes")
    ns = len(models)
    if starts is not None:
        starts = [list(s) for s in starts]
        if len(starts) != ns:
            raise ValueError(f"relax_trajectories: {len(starts)} starts for {ns} models (one start per replica)")
        mps_starts = core_starts(starts, dims, D)
    kw = {"max_diag_krylov": max_diag_krylov} if max_diag_krylov else {}
    bt = TDVPBatch(ns, nsite, device=device, relax="improved", thresh=thresh_sil, **kw)
    try:
        for k, (e, m) in enumerate(zip(bt.engines, models)):
            e.set_mpo(m.project_mpo(m.hamiltonian.as_mpo(m.dims)), 0, shift=m.hamiltonian.coupleJ[0][0])
            if starts is None:
                cores = m.initial_cores(0)
            elif mps_starts is None:
                cores = product_state_cores(starts[k], D, space=m.space)
            else:
                cores = mps_starts[k]
            e.set_mps(cores, canonicalize=True, scale=1.0)
        if max_restarts:
            bt.set_relax_restarts(max_restarts)
        out = bt.relax(maxstep, conv_tol)
        if nstates == 1:
            if max_restarts:
                out["restarts"] = bt.relax_restarts()["total"]
            out["states"] = [e.get_mps() for e in bt.engines]
            return out
        states = [[e.get_mps() for e in bt.engines]]
        energies = [bt.observe(norm=False, energy=True)["energy"].real]
        overlaps = np.zeros((nstates, nstates, ns), dtype=np.complex128)
        overlaps[0, 0] = [e.norm() ** 2 for e in bt.engines]
        for k in range(1, nstates):
            bt.deflate_push(pen)
            sk = state_starts[k]
            mk = None if sk is None else core_starts(sk, dims, D)
            for r, (e, m) in enumerate(zip(bt.engines, models)):
                if sk is None:
                    e.init_random(dims, int(min(D, 2**31 - 1)), seed=((int(seed) * 1000003 + k) * 1000003 + r + 1) % 2**64)
                else:
                    e.set_mps(product_state_cores(sk[r], D, space=m.space) if mk is None else mk[r], canonicalize=True, scale=1.0)
            out = bt.relax(maxstep, conv_tol)
            states.append([e.get_mps() for e in bt.engines])
            energies.append(bt.observe(norm=False, energy=True)["energy"].real)
            ov = bt.deflate_overlaps()  # <state j | state k>, j < k
            overlaps[:k, k] = ov
            overlaps[k, :k] = ov.conj()
            overlaps[k, k] = [e.norm() ** 2 for e in bt.engines]
        if max_restarts:
            out["restarts"] = bt.relax_restarts()["total"]
        out["states"] = states
        out["energies"] = np.array(energies)
        out["overlaps"] = overlaps
        bt.deflate_clear()
    finally:
        bt.close()
    return out


def observable_names(model, observables) -> list[str]:
    """The names of ``propagate_trajectories(observables=...)``: ``None`` or ``False`` is none, ``True`` every entry of
    ``model.observables`` in its order, otherwise a list of names (a single string is a list of one).  ``ValueError``
    naming a name the model does not have or one listed twice, and for more than 64 names (the request's limit).  Pure
    Python: raised before any engine exists."""
    if observables is None or observables is False:
        return []
    have = getattr(model, "observables", None) or {}
    if observables is True:
        names = list(have)
        if not names:
            raise ValueError("observables=True, but model.observables is empty")
    else:
        names = [observables] if isinstance(observables, str) else list(observables)
        if not names:
            raise ValueError("observables names no observable")
    for i, name in enumerate(names):
        if name not in have:
            raise ValueError(f"observable {name!r} is not in model.observables (it has {sorted(have)})")
        if name in names[:i]:
            raise ValueError(f"observable {name!r} is listed twice")
    if len(names) > 64:
        raise ValueError(f"{len(names)} observables, one run takes at most 64")
    return names


def propagate_trajectories(model, starts, maxstep, stepsize, reduced_density, weights=None, integrator="lanczos",
                           conserve_norm=True, per_trajectory=False, thresh_sil=1.0e-09, device=0, jumps=None, seed=0,
                           replicas_per_start=1, first_trajectory=0, densities=None, entanglement=None, shots=None,
                           shot_seed=0, observables=None, fields=None):
    """Propagate every Hartree product of ``starts`` under ``model`` and average their reduced densities.

    ``model``: a ``Model`` as the shell takes it (one electronic state, Hilbert space); its ``one_gate_to_apply``
    (one-site gates only) becomes gates of the batch, applied between the half-sweeps of every step as the reference
    applies them; ``kraus_op`` is refused (in the reference it means a purified state, not trajectories);
    ``starts``: a list of Hartree products as ``Model.init_HartreeProduct[0]`` takes them; ``stepsize`` in fs;
    ``reduced_density = ([(s, s), ...], every)`` as ``Simulator.propagate`` takes it.  As there, the state is observed
    BEFORE steps 0, every, 2 every, ... < ``maxstep``; steps after the last observation are not run.
    Returns ``{"time": (nrec,) in fs, "mean": {key: (nrec, d, d)}}`` and, with ``per_trajectory``,
    ``"trajectories": {key: (nrec, len(starts), d, d)}``.  ``weights``: one number per start, default equal weights.

    ``densities``: a list of keys in the reference's general form -- a tuple of site indices, non-decreasing, each site
    once (its diagonal) or twice (ket and bra): ``(0, 0, 2, 2)``, ``(0, 1)``, ``(1, 2, 2)`` -- recorded at the interval of
    ``reduced_density`` in the same run (``k_batch_density``, one more launch per record) and returned under the same
    ``"mean"`` / ``"trajectories"`` with their own shapes.  ``reduced_density`` keeps taking one-site keys only and may
    name none when ``densities`` is given.

    ``jumps={site: B (K, d, d)}``: a one-site Kraus channel per listed site (e.g. ``kraus.lindblad_to_kraus(ops, dt)``),
    unravelled into quantum jumps: every trajectory picks one operator per site and step with the state's own
    probabilities and keeps its norm, so the MEAN over many trajectories follows the channel.  ``replicas_per_start``
    repeats every start that often (the trajectory axis and ``weights`` then run over the expanded list, start-major);
    trajectory i of the expanded list draws ``jump_uniform(seed, first_trajectory + i, step, site)``, so an ensemble
    cut into chunks (``first_trajectory`` = the chunk's offset) draws the same numbers as one big batch.

    A key of ``jumps`` may also be a bond ``(q, q + 1)`` with ``B`` of shape ``(K, d_q d_{q+1}, d_q d_{q+1})`` (row-major
    over the two physical indices) or ``(K, d_q, d_{q+1}, d_q, d_{q+1})``: a nearest-neighbour Kraus channel, sampled by the
    same rule with the uniform ``jump_uniform(seed, trajectory, step, nsite + q)``; the bond keeps its dimension, so what
    the re-split truncates is lost (``TDVPBatch.discarded_weight``).  A key that is not an ascending pair of neighbours is
    a ``ValueError`` naming it.  ``model.one_gate_to_apply`` stays one-site.

    ``entanglement``: a strictly ascending list of bonds ``q`` (bond ``q`` lies between sites ``q`` and ``q + 1``).  The
    Schmidt spectrum of each is formed for every trajectory at the interval of ``reduced_density`` in the same run
    (``k_batch_spectra``, one more launch per record), and the result gains ``"entropy"`` of shape ``(nrec, nb)`` -- the
    weighted mean over the trajectories of each trajectory's von Neumann entropy (natural logarithm), which no averaged
    density gives -- and ``"min_weight"`` ``(nrec, nb)``, the mean of the smallest normalised Schmidt weight: the check
    that the bond dimension is wide enough.  With ``per_trajectory`` also ``"entropy_trajectories"`` ``(nrec, ntraj, nb)``.
    The default ``None`` leaves the result as it is without the keyword.

    ``shots``: a number of configurations -- one basis index per site, drawn from every trajectory's state with
    probability ``|<j_0 .. j_{L-1}|psi>|^2 / <psi|psi>`` -- sampled at the interval of ``reduced_density`` in the same run
    (``k_batch_sample``, one more launch per record), trajectory i of the expanded list drawing
    ``sample_uniform(shot_seed, first_trajectory + i, step, site, shot)``.  The result gains ``"configurations"`` of shape
    ``(nrec, ntraj, shots, L)`` (int32): the joint distribution of the site occupations, diagonal correlators of any
    order and full counting statistics are histograms of it; and ``"frequencies"``, a list of ``(nrec, d_p)`` arrays, the
    weighted mean over the trajectories of the fraction of shots with outcome j at site p.  The default ``None`` leaves
    the result as it is without the keyword.

    ``observables``: ``True`` for every entry of ``model.observables``, or a list of their names.  Each is turned into an
    MPO as ``Simulator.propagate(observables=True)`` prepares it (``op.as_mpo(model.dims)``, no scalar term), given to
    every trajectory as operator 1, 2, ... and evaluated at the interval of ``reduced_density`` in the same run
    (``k_batch_expect``, one workgroup per trajectory and observable, one more launch per record).  The result gains
    ``"expectations"``, ``{name: (nrec,) complex}`` -- the weighted mean over the trajectories of ``<psi|O|psi>``, not
    normalised, what ``expectations.dat`` holds for one state -- and, with ``per_trajectory``,
    ``"expectation_trajectories"``, ``{name: (nrec, ntraj)}``.  A name the model does not have is a ``ValueError`` naming
    it.  The default ``None`` leaves the result as it is without the keyword.

    ``fields``: time-dependent one-site terms ``H(t) = H0 + sum_p a_p(t) G_p``, ``{site: dict(G=(d, d) Hermitian,
    pulse=...)}`` or ``{site: dict(G=..., sigma=s, tau=t)}`` as ``TDVPBatch.set_fields`` takes them.  ``pulse`` is a table
    of midpoint amplitudes, ``(n,)`` for all trajectories or ``(ntraj, n)`` (0 once it is used up), or a callable of time,
    sampled at the midpoints of the run's steps (``pulse_table``); ``sigma`` / ``tau`` is Ornstein-Uhlenbeck noise per
    (trajectory, site) -- dynamic disorder -- trajectory i of the expanded list drawing ``field_noise_path(seed,
    first_trajectory + i, site, nsite, ...)``.  Times and ``tau`` are in the unit of ``stepsize`` (fs); amplitude times
    ``G`` is in the Hamiltonian's unit.  Each term acts as ``exp(-i dt a_p G_p)`` between the half-sweeps, before gates and
    jumps (``k_batch_field``, one more launch per step); the step is accurate to O(dt^2)."""
    if integrator not in ("lanczos", "arnoldi"):
        raise ValueError(f"Invalid integrator: {integrator}")
    obs_names = observable_names(model, observables)  # an unknown name raises here, before any engine exists
    if shots is not None:
        shots, shot_seed = sample_request(shots, shot_seed)
        if shots < 1:
            raise ValueError("shots must be >= 1")
    keys, every = reduced_density
    keys = [tuple(k) for k in keys]
    every = int(every)
    if every < 1 or maxstep < 1:
        raise ValueError("maxstep and the reduced-density interval must be >= 1")
    nsite = len(model.dims)
    key_sites = _one_site_keys(keys, nsite)
    bonds = spectra_bonds(entanglement, nsite) if entanglement is not None else []
    if entanglement is not None and not bonds:
        raise ValueError("entanglement names no bond")
    dens_keys = [tuple(k) for k in densities] if densities is not None else []
    for k in dens_keys:
        density_key_legs(k, nsite)  # a malformed key raises here, before any engine exists
    if not keys and not dens_keys:
        raise ValueError("reduced_density names no key")
    if model.nstate != 1 or model.space != "hilbert":
        raise NotImplementedError("propagate_trajectories: one electronic state in Hilbert space")
    if model.kraus_op:
        raise NotImplementedError("propagate_trajectories: kraus_op means a purified state (a Kraus leg that grows); "
                                  "pass a one-site channel as jumps={site: B} to sample it instead")
    gates = model.one_gate_to_apply.one_site_gates(model.dims) if model.one_gate_to_apply is not None else {}
    jump_table = _jump_table(jumps or {}, model.dims)
    both = sorted(set(gates) & set(jump_table))
    if both:
        raise ValueError(f"site {both[0]} has a gate and a jump channel: a site carries one channel")
    replicas_per_start, first_trajectory = int(replicas_per_start), int(first_trajectory)
    if replicas_per_start < 1 or first_trajectory < 0:
        raise ValueError("replicas_per_start must be >= 1 and first_trajectory >= 0")
    starts = list(starts)
    if not starts:
        raise ValueError("no start states")
    nrep = len(starts) * replicas_per_start
    sites = sorted(set(key_sites))
    dt_au = stepsize / units.au_in_fs
    nsteps = (maxstep - 1) // every * every
    field_table = _field_table(fields, list(model.dims), nrep, stepsize, nsteps)
    D = model.m_aux_max if model.m_aux_max is not None else 10**9
    mpo = model.project_mpo(model.hamiltonian.as_mpo(model.dims))
    obs_mpos = [model.observables[name].as_mpo(model.dims) for name in obs_names]
    bt = TDVPBatch(nrep, nsite, device=device, integrator=integrator, conserve_norm=conserve_norm, thresh=thresh_sil)
    try:
        for i, e in enumerate(bt.engines):
            e.set_mpo(mpo, 0, shift=model.hamiltonian.coupleJ[0][0])
            for k, cores in enumerate(obs_mpos, start=1):
                e.set_mpo(cores, k)
            if i % replicas_per_start == 0:  # a start is brought to canonical form once; its repeats get those very tensors
                e.set_mps(product_state_cores(starts[i // replicas_per_start], D, space=model.space), canonicalize=True, scale=1.0)
                canonical = e.get_mps()
            else:
                e.set_mps(canonical)
        if gates:
            bt.set_gates(gates)
        if jump_table:
            bt.set_jumps(jump_table, seed=seed, trajectory_ids=range(first_trajectory, first_trajectory + nrep))
        req = dict(sites=sites, norm=False, weights=weights, per_replica=per_trajectory)
        if dens_keys:
            req["keys"] = dens_keys
        if bonds:
            bt.set_spectra(bonds)
            req.update(spectra=True, spectra_weights=weights)
        if field_table:
            if not jump_table:  # the ids of the noise; with jumps set_jumps has registered these very ids
                bt.set_jumps({}, seed=seed, trajectory_ids=range(first_trajectory, first_trajectory + nrep))
            bt.set_fields(field_table)
        if shots is not None:
            if not jump_table and not field_table:  # the ids of the draws; with jumps set_jumps has registered these very ids
                bt.set_jumps({}, seed=seed, trajectory_ids=range(first_trajectory, first_trajectory + nrep))
            bt.set_samples(shots, shot_seed)
            req.update(samples=True, samples_weights=weights)
        if obs_names:
            bt.set_expect(range(1, len(obs_names) + 1))
            req.update(expect=True, expect_weights=weights)
        rec = bt.propagate(dt_au, nsteps, observe=req, every=every)
        if shots is not None and not per_trajectory:  # the configurations are per trajectory by nature
            rec = dict(rec, configs=bt._samples_records(None, True)["configs"])  # handed out from the host copy: no launch
    finally:
        bt.close()
    nrec = nsteps // every + 1
    out = {"time": np.arange(nrec) * every * dt_au * units.au_in_fs,
           "mean": {k: rec["mean_rdm"][sites.index(s)] for k, s in zip(keys, key_sites)}}
    if per_trajectory:
        out["trajectories"] = {k: rec["rdm"][sites.index(s)] for k, s in zip(keys, key_sites)}
    for i, k in enumerate(dens_keys):  # a key given both ways is the general form's
        out["mean"][k] = rec["mean_density"][i]
        if per_trajectory:
            out["trajectories"][k] = rec["density"][i]
    if bonds:
        out["entropy"], out["min_weight"] = rec["mean_entropy"], rec["mean_min_weight"]
        if per_trajectory:
            out["entropy_trajectories"] = rec["entropy"]
    if shots is not None:
        out["configurations"], out["frequencies"] = rec["configs"], rec["mean_freq"]
    if obs_names:
        out["expectations"] = {name: np.ascontiguousarray(rec["mean_expect"][:, k]) for k, name in enumerate(obs_names)}
        if per_trajectory:
            out["expectation_trajectories"] = {name: np.ascontiguousarray(rec["expect"][:, :, k]) for k, name in enumerate(obs_names)}
    return out
