"""Shared inputs of tests/test_batch_cross_host.py and tests/test_gpu_batch_cross.py: a NumPy restatement of the walk of
k_batch_cross, random states of different norms, and the physics case of the two-time correlation function with its
references (the NumPy oracle and dense ``expm``), each computed once."""

import functools

import numpy as np

from oracle import tdvp_oracle as orc

from . import jump_oracle as jo
from . import pair_cases as pc
from . import spin_bath as sb


def walk(bra, ket, site=-1, O=None):
    """<bra| O_site |ket> by the kernel's walk over all sites: T (bra bond, ket bond) starts as 1, U = T K, the operator on
    U's physical index at ``site``, T' = sum conj(Bra) U; the value is the 1 x 1 T behind the last site"""
    T = np.ones((1, 1), dtype=np.complex128)
    for p, (b, k) in enumerate(zip(bra, ket)):
        U = np.einsum("ma,ajs->mjs", T, k)
        if p == site:
            U = np.einsum("ij,mjs->mis", np.asarray(O, dtype=np.complex128), U)
        T = np.einsum("mjt,mjs->ts", np.conj(b), U)
    assert T.shape == (1, 1)
    return complex(T[0, 0])


def norm_of(cores):
    return float(np.sqrt(abs(walk(cores, cores))))


def random_states(dims, D, n, seed):
    """n random complex states, site-0 canonical (what a batch replica takes), with norms 0.7, 0.9, 1.1, ..."""
    return [orc.canonicalize_site0(orc.synthetic_mps(list(dims), D, seed=seed + r), scale=0.7 + 0.2 * r) for r in range(n)]


def random_op(d, seed, hermitian=False):
    rng = np.random.default_rng(seed)
    O = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    return O + O.conj().T if hermitian else O


# ---- the physics case: L = 4 spin chain, complex product start, C(t) = <psi| A(t) B |psi> ----
L, D, DT, NSTEPS = 4, 4, 0.4, 8
START = [[1, 0.5j], [0.3, 1], [1, -1j], [0.2 + 0.1j, 1]]
B_OP = (1, sb.SX)
A_OP = (2, sb.SZ)


def start_vectors():
    return [np.asarray(v, dtype=np.complex128) / np.linalg.norm(v) for v in START]


def _product_cores(vectors):
    """the Hartree product padded to the bond dimensions of D, as the trajectory front end sets it (its norm is kept)"""
    from pytdscf_amd.mps import product_state_cores

    cores = product_state_cores([np.ones(len(v)) for v in vectors], D)
    for c, v in zip(cores, vectors):
        c[0, :, 0] = v
    return orc.canonicalize_site0(cores, scale=None)


def psi_phi_vectors():
    psi = start_vectors()
    phi = [v.copy() for v in psi]
    phi[B_OP[0]] = B_OP[1] @ phi[B_OP[0]]
    return psi, phi


@functools.lru_cache(maxsize=None)
def oracle_runs(integrator="arnoldi", thresh=1e-9):
    """the oracle's states of psi and phi = B psi before steps 0 .. NSTEPS: ([cores of psi], [cores of phi])"""
    mpo = pc._spin_chain_mpo(L)
    out = []
    for vec in psi_phi_vectors():
        st = orc.OracleMPS(_product_cores(vec), mpo, integrator=integrator, thresh=thresh, conserve_norm=False)
        hist = [[c.copy() for c in st.cores]]
        for _ in range(NSTEPS):
            st.propagate(DT)
            hist.append([c.copy() for c in st.cores])
        out.append(hist)
    return tuple(out)


def oracle_corr(integrator="arnoldi", thresh=1e-9):
    psi, phi = oracle_runs(integrator, thresh)
    return np.array([walk(a, b, A_OP[0], A_OP[1]) for a, b in zip(psi, phi)])


def oracle_auto(integrator="arnoldi", thresh=1e-9):
    """<psi(0)|psi(t)> and the t/2-trick value <psi(t)*|psi(t)> of the same run"""
    psi, _ = oracle_runs(integrator, thresh)
    return (np.array([walk(psi[0], a) for a in psi]), np.array([orc.overlap(a, a, conj_bra=False) for a in psi]))


@functools.lru_cache(maxsize=None)
def dense():
    """dense expm on the 16-dimensional space: C(t_k), <psi(0)|psi(t_k)> for k = 0 .. NSTEPS, and <psi(0)|psi(2 t_k)>"""
    from scipy.linalg import expm

    dims = [2] * L
    H = jo.dense_operator(pc._spin_chain_mpo(L))
    psi_v, phi_v = psi_phi_vectors()
    kron = lambda vs: functools.reduce(np.kron, vs)
    psi0, phi0 = kron(psi_v), kron(phi_v)
    Aop = jo.embed(A_OP[1], A_OP[0], dims)
    corr, auto, auto2 = [], [], []
    for k in range(NSTEPS + 1):
        U = expm(-1j * H * DT * k)
        corr.append(np.vdot(U @ psi0, Aop @ (U @ phi0)))
        auto.append(np.vdot(psi0, U @ psi0))
        auto2.append(np.vdot(psi0, U @ (U @ psi0)))
    return np.array(corr), np.array(auto), np.array(auto2)


def model():
    """the case as a Model of the shell, for trajectories.correlation_function"""
    from pytdscf_amd import Exciton, Model

    return Model([Exciton(nstate=2) for _ in range(L)], operators={"hamiltonian": pc._spin_chain_mpo(L)}, bond_dim=D)
