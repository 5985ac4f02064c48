"""Inputs of the batched improved relaxation's tests (tests/test_batch_relax_host.py, test_gpu_batch_relax.py,
test_gpu_tridiag_lowest.py): disordered Heisenberg chains, field-only chains, dense matrices from MPO cores, starts, the
oracle's relaxation with its Krylov dimensions, tridiagonal matrices recorded from Lanczos runs, and the table of
tridiagonal cases with the reference's own error and the bars derived from it.

``synthetic_mpo`` chains are no use here: the oracle reaches their ground state to 1e-15 in the first step at every
shape, and every later solve stops at k = 1."""

from __future__ import annotations

import functools

import numpy as np

from oracle import tdvp_oracle as orc

EPS = float(np.finfo(np.float64).eps)


# ---- operators ----
def spin_ops(d):
    """S^z, S^+, S^-, S^x of spin (d - 1) / 2 in the basis m = s, s - 1, ..., -s"""
    s = (d - 1) / 2.0
    m = s - np.arange(d)
    sz = np.diag(m).astype(np.complex128)
    sp = np.zeros((d, d), dtype=np.complex128)
    for k in range(1, d):  # S^+ |m> = sqrt(s(s+1) - m(m+1)) |m+1>
        sp[k - 1, k] = np.sqrt(s * (s + 1) - m[k] * (m[k] + 1))
    sm = sp.conj().T.copy()
    return sz, sp, sm, 0.5 * (sp + sm)


def chain_mpo(dims, onsite, J=1.0):
    """MPO of bond 5 of H = J sum_p [(S+S- + S-S+)/2 + SzSz]_{p,p+1} + sum_p onsite[p]; cores (ml, d, d, mr)"""
    L = len(dims)
    cores = []
    for p, d in enumerate(dims):
        sz, sp, sm, _ = spin_ops(d)
        eye = np.eye(d, dtype=np.complex128)
        w = np.zeros((5, d, d, 5), dtype=np.complex128)
        w[0, :, :, 0] = eye
        w[1, :, :, 0] = sm
        w[2, :, :, 0] = sp
        w[3, :, :, 0] = sz
        w[4, :, :, 0] = onsite[p]
        w[4, :, :, 1] = 0.5 * J * sp
        w[4, :, :, 2] = 0.5 * J * sm
        w[4, :, :, 3] = J * sz
        w[4, :, :, 4] = eye
        if p == 0:
            w = w[4:5]
        if p == L - 1:
            w = w[:, :, :, 0:1]
        cores.append(np.ascontiguousarray(w))
    return cores


def heisenberg_fields(dims, seed):
    """the one-site terms h_p S^z + g_p S^x, h_p ~ U(-1, 1), g_p ~ U(-0.5, 0.5) from default_rng(seed)"""
    rng = np.random.default_rng(seed)
    h = rng.uniform(-1.0, 1.0, len(dims))
    g = rng.uniform(-0.5, 0.5, len(dims))
    out = []
    for p, d in enumerate(dims):
        sz, _, _, sx = spin_ops(d)
        out.append(h[p] * sz + g[p] * sx)
    return out


def heisenberg_mpo(dims, seed):
    """the disordered Heisenberg chain of spin (d_p - 1) / 2, MPO bond 5"""
    dims = list(dims)
    return chain_mpo(dims, heisenberg_fields(dims, seed), 1.0)


def field_terms(dims, seed):
    """random Hermitian one-site terms"""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for d in dims:
        a = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
        out.append(0.5 * (a + a.conj().T))
    return out


def field_mpo(dims, seed):
    """H = sum_p h_p with random Hermitian h_p, MPO bond 2"""
    dims = list(dims)
    L = len(dims)
    cores = []
    for p, (d, h) in enumerate(zip(dims, field_terms(dims, seed))):
        eye = np.eye(d, dtype=np.complex128)
        w = np.zeros((2, d, d, 2), dtype=np.complex128)
        w[0, :, :, 0] = eye
        w[1, :, :, 0] = h
        w[1, :, :, 1] = eye
        if p == 0:
            w = w[1:2]
        if p == L - 1:
            w = w[:, :, :, 0:1]
        cores.append(np.ascontiguousarray(w))
    return cores


def field_mpo_wide(dims, seed):
    """the same Hamiltonian as field_mpo in the bond-5 form of chain_mpo (J = 0): it shares a batch with Heisenberg chains"""
    dims = list(dims)
    return chain_mpo(dims, field_terms(dims, seed), 0.0)


def field_ground_energy(dims, seed):
    return float(sum(np.linalg.eigvalsh(h)[0] for h in field_terms(list(dims), seed)))


def dense_from_mpo(cores):
    """the dense matrix of an MPO, rows and columns over (i_0, ..., i_{L-1}), site 0 slowest"""
    m = np.ones((1, 1, 1), dtype=np.complex128)  # [row, col, bond]
    for w in cores:
        m = np.einsum("rcb,bijt->ricjt", m, w).reshape(m.shape[0] * w.shape[1], m.shape[1] * w.shape[2], w.shape[3])
    return m[:, :, 0]


@functools.lru_cache(maxsize=None)
def dense_spectrum(kind, dims, seed):
    mpo = heisenberg_mpo(dims, seed) if kind == "heis" else field_mpo(dims, seed)
    return np.linalg.eigvalsh(dense_from_mpo(mpo))


# ---- starts ----
def start(dims, D, seed):
    """a full-rank random MPS, centre at site 0, normalised"""
    return orc.synthetic_mps(list(dims), D, seed=100 + seed)


def perturbed(cores, size, seed=7):
    rng = np.random.default_rng(seed)
    out = [c + size * (rng.standard_normal(c.shape) + 1j * rng.standard_normal(c.shape)) for c in cores]
    return orc.canonicalize_site0(out)


def product_start(dims, D, seed):
    """a random Hartree product zero-padded to the bonds of (dims, D), centre at site 0"""
    rng = np.random.default_rng(200 + seed)
    out = []
    for (dl, dr), d in zip(orc.bond_dims(list(dims), D), dims):
        v = rng.standard_normal(d) + 1j * rng.standard_normal(d)
        c = np.zeros((dl, d, dr), dtype=np.complex128)
        c[0, :, 0] = v / np.linalg.norm(v)
        out.append(c)
    return out


def fidelity_defect(a, b):
    return abs(abs(orc.overlap(a, b)) - 1.0)


# ---- the case table ----
# parity cases: (dims, D, seeds); the oracle's first step has a local solve with k > 21 in every one of them
PARITY = {
    "L8d2D4": ((2,) * 8, 4, (0, 1, 2, 3, 4)),
    "L6d3D6": ((3,) * 6, 6, (0, 1, 2)),
}
FULL_BOND = ((2,) * 6, 8)  # exact after the first step
FIELD = ((3,) * 5, (1, 4))  # dims, the bond dimensions
MANY = ((2,) * 4, 4)        # more replicas than compute units


@functools.lru_cache(maxsize=None)
def oracle_relax(kind, dims, D, seed, nsteps, shift=0.0, perturb=0.0):
    """nsteps improved-relaxation steps of the oracle from start(dims, D, seed): (energies after every step, the largest
    Krylov dimension of a local solve in every step, all Krylov dimensions of the first step, the final cores)"""
    mpo = heisenberg_mpo(dims, seed) if kind == "heis" else field_mpo(dims, seed)
    cores = start(dims, D, seed)
    if perturb:
        cores = perturbed(cores, perturb)
    st = orc.OracleMPS([c.copy() for c in cores], mpo, relax="improved", shift=shift)
    st.build_right_envs()
    energies, kmax, first = [], [], []
    for n in range(nsteps):
        ks = []
        for fwd in (True, False):
            st.sweep(0.0, fwd)
            ks += [st.kprev[p] for p in range(len(dims))]
        if n == 0:
            first = list(ks)
        kmax.append(max(ks))
        energies.append(st.expectation().real)
    return energies, kmax, first, [c.copy() for c in st.cores]


# ---- tridiagonal matrices ----
def lanczos_T(matvec, psi, kmax):
    """alpha (k), beta (k) of kmax plain Lanczos steps (no re-orthogonalisation: long runs carry ghost copies)"""
    v = np.array(psi, dtype=np.complex128).reshape(-1)
    v = v / np.linalg.norm(v)
    prev, alpha, beta = None, [], []
    for _ in range(min(kmax, v.size)):
        w = np.array(matvec(v.reshape(psi.shape))).reshape(-1)
        a = np.vdot(v, w).real
        w = w - a * v
        if prev is not None:
            w = w - beta[-1] * prev
        b = float(np.linalg.norm(w))
        alpha.append(a)
        beta.append(b)
        if b < 1e-12:
            break
        prev, v = v, w / b
    return np.array(alpha), np.array(beta)


@functools.lru_cache(maxsize=None)
def recorded_T():
    """T matrices from Lanczos runs on the H_eff of site 2 of the parity cases' starts: short ones, one as long as the
    oracle's longest local solve, and 64-vector runs, which carry ghost copies of the lowest Ritz value"""
    out = []
    for name, (dims, D, seeds) in PARITY.items():
        seed = seeds[0]
        st = orc.OracleMPS(start(dims, D, seed), heisenberg_mpo(dims, seed), relax="improved")
        st.build_right_envs()
        st.sweep(0.0, True)
        st.sweep(0.0, False)
        st.sweep(0.0, True)  # the blocks of a middle site are those its solve in this half-sweep saw
        p = len(dims) // 2
        rng = np.random.default_rng(300 + seed)
        psi = rng.standard_normal(st.cores[p].shape) + 1j * rng.standard_normal(st.cores[p].shape)
        a, b = lanczos_T(st._heff(p), psi, 64)
        for k in (5, 21, 30, len(a)):
            k = min(k, len(a))
            out.append((f"{name}-site{p}-k{k}", a[:k].copy(), b[: k - 1].copy()))
    return out


def _rand_T(k, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(k), np.abs(rng.standard_normal(max(k - 1, 0))) + 0.05


@functools.lru_cache(maxsize=None)
def tridiag_cases():
    """[(name, alpha, beta)]: orders 1, 2, 3, 21, 63, 64; random; graded over 12 decades; recorded Lanczos matrices; one
    beta of 1e-12 |T|; a lowest pair split by 1e-9 |T|"""
    out = []
    for k in (1, 2, 3, 21, 63, 64):
        a, b = _rand_T(k, 10 + k)
        out.append((f"random-k{k}", a, b))
    for k in (3, 21, 64):
        g = np.logspace(0, -12, k)
        a, b = _rand_T(k, 40 + k)
        out.append((f"graded-down-k{k}", a * g, b * np.sqrt(g[:-1] * g[1:])))
        out.append((f"graded-up-k{k}", (a * g)[::-1].copy(), (b * np.sqrt(g[:-1] * g[1:]))[::-1].copy()))
    out += list(recorded_T())
    for k, at in ((21, 9), (64, 40)):  # nearly decoupled: one off-diagonal entry of 1e-12 |T|; the lowest pair lives in the upper block
        a, b = _rand_T(k, 70 + k)
        a, b = a.copy(), b.copy()
        a[: at + 1] -= 3.0
        b[at] = 1e-12 * np.max(np.abs(a))
        out.append((f"tiny-beta-k{k}", a, b))
    for k in (4, 22, 64):  # two mirror-image blocks, the lowest diagonal entries at the junction, coupled so weakly that
        h = k // 2         # the lowest pair splits by 1e-9 |T|_1 (the split grows linearly with the coupling)
        a1, b1 = _rand_T(h, 90 + k)
        a1 = np.sort(a1)[::-1].copy()
        a = np.concatenate([a1, a1[::-1]])
        b = np.concatenate([b1, [1e-9], b1[::-1]])
        for _ in range(6):
            w = np.linalg.eigvalsh(np.diag(a) + np.diag(b, 1) + np.diag(b, -1))
            t1 = np.max(np.abs(a)) + 2 * np.max(np.abs(b))
            b[h - 1] *= 1e-9 * t1 / max(w[1] - w[0], 1e-300)
        out.append((f"close-pair-k{k}", a, b))
    return out


def _sturm_lowest_longdouble(a, b):
    """the lowest eigenvalue by bisection on Sturm counts in longdouble"""
    a = np.asarray(a, dtype=np.longdouble)
    b2 = np.asarray(b, dtype=np.longdouble) ** 2
    r = np.concatenate([[0], np.abs(np.asarray(b, dtype=np.longdouble)), [0]])
    lo = np.min(a - r[:-1] - r[1:])
    hi = np.max(a + r[:-1] + r[1:])
    tiny = np.longdouble(1e-4000) if np.finfo(np.longdouble).tiny < 1e-4000 else np.finfo(np.longdouble).tiny

    def count(x):
        q = a[0] - x
        n = int(q < 0)
        for i in range(1, len(a)):
            if q == 0:
                q = -tiny
            q = (a[i] - x) - b2[i - 1] / q
            n += int(q < 0)
        return n

    lo, hi = lo - 1, hi + 1
    for _ in range(200):
        mid = lo + (hi - lo) / 2
        if mid == lo or mid == hi:
            break
        if count(mid) >= 1:
            hi = mid
        else:
            lo = mid
    return lo + (hi - lo) / 2


@functools.lru_cache(maxsize=None)
def tridiag_table():
    """One row per case: the reference (scipy.linalg.eigh_tridiagonal, float64), its own error, and the bars.
    theta_err = |theta_LAPACK - theta_longdouble|, res = |T c - theta c| of LAPACK's pair; the bars are 8 x those,
    floored at k eps |T|_1; where the reference's gap exceeds 1e-6 |T|_1 the vector bar is (residual bar) / gap."""
    import scipy.linalg

    rows = []
    for name, a, b in tridiag_cases():
        k = len(a)
        T = np.diag(a) + (np.diag(b, 1) + np.diag(b, -1) if k > 1 else 0.0)
        t1 = float(np.max(np.sum(np.abs(T), axis=0)))
        if k == 1:
            w, v = np.array([a[0]]), np.ones((1, 1))
        else:
            w, v = scipy.linalg.eigh_tridiagonal(a, b)
        c = v[:, 0] * (-1.0 if v[0, 0] < 0 else 1.0)
        theta_ld = _sturm_lowest_longdouble(a, b)
        theta_err = float(abs(np.longdouble(w[0]) - theta_ld))
        res = float(np.linalg.norm(T @ c - w[0] * c))
        floor = k * EPS * t1
        gap = float(w[1] - w[0]) if k > 1 else float("inf")
        bar_theta = max(8.0 * theta_err, floor)
        bar_res = max(8.0 * res, floor)
        bar_vec = bar_res / gap if gap > 1e-6 * t1 else None
        rows.append(dict(name=name, k=k, alpha=a, beta=b, T=T, norm1=t1, theta=float(w[0]), vec=c, gap=gap, theta_err=theta_err,
                         res=res, bar_theta=bar_theta, bar_res=bar_res, bar_vec=bar_vec))
    return rows


def tridiag_table_text():
    lines = ["case                      k   |T|_1      gap/|T|_1  ref |dtheta|  ref resid   bar theta   bar resid   bar vec"]
    for r in tridiag_table():
        lines.append("%-24s %3d  %9.3e  %9.3e  %9.3e   %9.3e   %9.3e   %9.3e   %s" % (
            r["name"], r["k"], r["norm1"], r["gap"] / r["norm1"], r["theta_err"], r["res"], r["bar_theta"], r["bar_res"],
            "-" if r["bar_vec"] is None else "%9.3e" % r["bar_vec"]))
    return "\n".join(lines)
