"""The restarted local Lanczos solve of the batched improved relaxation (bt_diag, csrc/batch_site.hip) restated in NumPy,
and a relaxation sweep around it built from the oracle's public functions.  The cases are those of helpers/relax_cases.

The solve: orthodox Lanczos on a basis kept normalised, slot 0 the start as it came; after every new vector the lowest
eigenpair of T_k (scipy.linalg.eigh_tridiagonal, first component non-negative); converged when |c_k - pad(c_{k-1})| <
thresh, or beta_k < 1e-12, or k == N.  With m = kcap = min(N, max_diag_krylov) vectors, no convergence and restarts left:

    u_0 = sum_j c_j v_j, renormalised          u_1 = v_m
    alpha[0] = theta                           beta[0] = s = beta_{m-1} c_{m-1}   (signed)
    c_prev = e_1                               the recurrence goes on at i = 1 with v_{i-1} = u_0, beta_{i-1} = s

since H u_0 = theta u_0 + s u_1, the projected matrix on [u_0, u_1, ...] is tridiagonal again."""

from __future__ import annotations

import functools

import numpy as np
import scipy.linalg

from helpers import relax_cases as rc
from oracle import tdvp_oracle as orc

EPS_BREAK = 1e-12  # SS_EPS


def lowest_pair(alpha, beta):
    """the lowest eigenpair of the tridiagonal (alpha, beta), beta of either sign; first component non-negative"""
    if len(alpha) == 1:
        return float(alpha[0]), np.ones(1)
    w, v = scipy.linalg.eigh_tridiagonal(np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64))
    c = v[:, 0]
    return float(w[0]), (-c if c[0] < 0 else c)


def restarted_lanczos(matvec, psi, thresh=1e-9, max_diag_krylov=64, max_restarts=0):
    """(the new tensor, theta, info): info = dict(k: vectors of the last cycle, applies, restarts).  ValueError with the
    library's words when the solve is not converged after max_restarts restarts."""
    shape = psi.shape
    v0 = np.array(psi, dtype=np.complex128).reshape(-1)
    N = v0.size
    kcap = min(N, max_diag_krylov)
    U = [v0]
    alpha = np.zeros(kcap)
    beta = np.zeros(kcap)
    cprev = None
    c = None
    theta = 0.0
    napply = nrest = 0
    i = 0
    while i < kcap:
        w = np.array(matvec(U[i].reshape(shape)), dtype=np.complex128).reshape(-1)
        napply += 1
        al = float(np.vdot(U[i], w).real)
        w = w - al * U[i]
        if i > 0:
            w = w - beta[i - 1] * U[i - 1]
        be = float(np.linalg.norm(w))
        if be >= EPS_BREAK:
            w = w / be
        del U[i + 1:]
        U.append(w)
        alpha[i], beta[i] = al, be
        k = i + 1
        theta, c = lowest_pair(alpha[:k], beta[: k - 1])
        done = be < EPS_BREAK or k == N
        if not done and i > 0:
            pad = np.zeros(k)
            pad[: len(cprev)] = cprev
            done = float(np.linalg.norm(c - pad)) < thresh
        if done:
            x = np.zeros(N, dtype=np.complex128)
            for j in range(k):  # the order of the kernel's combination
                x = x + c[j] * U[j]
            x = x / np.linalg.norm(x)
            return x.reshape(shape), theta, dict(k=k, applies=napply, restarts=nrest)
        if k < kcap or nrest >= max_restarts:
            cprev = c
            i += 1
            continue
        u0 = np.zeros(N, dtype=np.complex128)
        for j in range(kcap):
            u0 = u0 + c[j] * U[j]
        s = beta[kcap - 1] * c[kcap - 1]
        U = [u0 / np.linalg.norm(u0), U[kcap]]
        alpha[0], beta[0] = theta, s
        cprev = np.array([1.0])
        nrest += 1
        i = 1
    raise ValueError("Lanczos Diagonalization is not converged in %d basis" % max_diag_krylov +
                     (" after %d restarts" % max_restarts if max_restarts > 0 else ""))


def relax_model(mpo, cores, nsteps, max_diag_krylov=64, max_restarts=0, thresh=1e-9, shift=0.0):
    """nsteps improved-relaxation steps (forward + backward half-sweep) with the restarted solve, centre at site 0 before
    and after.  Returns dict(energies: <H> + shift after every step, ritz: the Ritz value of the last solve of every step,
    most: the most restarts of one solve in every step, total: restarts in all, applies, cores).  The bond matrix is left
    alone, as in the oracle's improved relaxation."""
    mpo = [np.array(w, dtype=np.complex128) for w in mpo]
    cores = [np.array(c, dtype=np.complex128) for c in cores]
    n = len(cores)
    one = np.ones((1, 1, 1), dtype=np.complex128)
    left, right = {0: one}, {n - 1: one}
    for p in range(n - 1, 0, -1):
        right[p - 1] = orc.env_update_right(right[p], cores[p], mpo[p])
    energies, ritz, most = [], [], []
    total = applies = 0

    def solve(p):
        nonlocal total, applies

        def mv(x):
            y = orc.heff_apply(left[p], mpo[p], right[p], x)
            return y + shift * x if shift != 0.0 else y

        new, theta, info = restarted_lanczos(mv, cores[p], thresh, max_diag_krylov, max_restarts)
        cores[p] = new
        total += info["restarts"]
        applies += info["applies"]
        return theta, info["restarts"]

    for _ in range(nsteps):
        worst = 0
        theta = 0.0
        for p in range(n):
            theta, nr = solve(p)
            worst = max(worst, nr)
            if p == n - 1:
                break
            A, sval = orc.qr_psi2Asigma(cores[p])
            cores[p] = A
            left[p + 1] = orc.env_update_left(left[p], A, mpo[p])
            cores[p + 1] = np.tensordot(sval, cores[p + 1], axes=(1, 0))
        for p in range(n - 1, -1, -1):
            theta, nr = solve(p)
            worst = max(worst, nr)
            if p == 0:
                break
            sval, B = orc.qr_psi2sigmaB(cores[p])
            cores[p] = np.ascontiguousarray(B)
            right[p - 1] = orc.env_update_right(right[p], cores[p], mpo[p])
            cores[p - 1] = np.tensordot(cores[p - 1], sval, axes=(2, 0))
        st = orc.OracleMPS([c.copy() for c in cores], mpo, relax="improved", shift=shift)
        energies.append(st.expectation().real)
        ritz.append(theta)
        most.append(worst)
    return dict(energies=energies, ritz=ritz, most=most, total=total, applies=applies, cores=[c.copy() for c in cores])


@functools.lru_cache(maxsize=None)
def model_relax(kind, dims, D, seed, nsteps, max_diag_krylov, max_restarts, start="full"):
    """relax_model on a case of relax_cases: kind "heis" / "field" / "field_wide", start "full" (rc.start) or "product";
    computed once and shared"""
    mpo = {"heis": rc.heisenberg_mpo, "field": rc.field_mpo, "field_wide": rc.field_mpo_wide}[kind](dims, seed)
    cores = rc.start(dims, D, seed) if start == "full" else rc.product_start(dims, D, seed)
    return relax_model(mpo, cores, nsteps, max_diag_krylov, max_restarts)
