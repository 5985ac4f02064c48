"""Cases, NumPy twin and dense pin of the batched MPO matrix elements between replicas (k_batch_cross_mpo).

Shapes: the three of helpers/spectra_cases.SHAPES (ragged d with a bond narrower than the tile; every bond odd; twelve
sites with bonds to 40, past the 32-wide tile and the 16-deep K step).  Operators: those of helpers/expect_cases.case with
its scale(): product, local, longrange, complex (non-Hermitian, complex shift) and energy (shift 0.1), MPO bonds 1 to 16
at bonds that differ from the Hamiltonian's.  States: cross_cases.random_states, norms 0.7, 0.9, 1.1.

The bar of the device tests is BAR SCALE |a| |b| with BAR = 1e-12: the relative bar of tests/test_gpu_batch_cross.py times
the operator scale of tests/test_gpu_batch_expect.py.  The twin's own defect against the dense pin is asserted to be at
most a tenth of it by tests/test_batch_cross_mpo_host.py; the largest observed there is 5.2e-5 of the bar (at the `odd`
shape, a = b), so the bar stands as stated.

The physics case is cross_cases' L = 4, D = 4 spin chain with A = sum_p SZ_p and B = sum_p SX_p: C(t) = <psi| A(t) B |psi>.
The oracle's C(t) (OracleMPS runs of psi and phi = B psi, then the twin) deviates from dense expm by 9.3e-12 at most
(3.8e-12 with the one-site A of cross_cases, 1.8e-12 with its one-site B; tests/test_batch_cross_mpo_host.py prints and
bounds it); the GPU test holds the device within ten times the deviation it computes from the same two references."""

import functools

import numpy as np

from oracle import tdvp_oracle as orc

from . import cross_cases as cc
from . import expect_cases as ec
from . import jump_oracle as jo
from . import pair_cases as pc
from . import spin_bath as sb

SHAPES = ec.SHAPES
LABELS = ec.LABELS
OP_ID = ec.OP_ID
HERMITIAN = ("product", "local", "longrange", "energy")
BAR = 1e-12
case, scale = ec.case, ec.scale


def random_states(name, n, seed=30):
    dims, D = SHAPES[name]
    return cc.random_states(dims, D, n, seed)


# ---- the NumPy twin of k_batch_cross_mpo's walk ----
def walk_mpo(bra, ket, mpo):
    """T (bra bond, MPO bond, ket bond) = [1]; per site the three stages of bt_env in the forward roles:
    X[(c,a)][(p,s)] = sum_b conj(Bra[b,c,a]) T[b,p,s]; Y[a][(q,t)][s] = sum_(c,p) W[p,c,t,q] X[c,a,p,s];
    T'[a,q,r] = sum_(t,s) Y[a,q,t,s] Ket[s,t,r]; the value is the 1 x 1 x 1 block behind the last site"""
    T = np.ones((1, 1, 1), dtype=np.complex128)
    for b, k, W in zip(bra, ket, mpo):
        X = np.einsum("bca,bps->caps", np.conj(b), T)
        Y = np.einsum("pctq,caps->aqts", W, X)
        T = np.einsum("aqts,str->aqr", Y, k)
    assert T.shape == (1, 1, 1)
    return complex(T[0, 0, 0])


def walk(bra, ket, mpo, shift=0.0):
    """the kernel's value: the MPO walk and, for a non-zero scalar term, shift times k_batch_cross's overlap walk"""
    v = walk_mpo(bra, ket, mpo)
    if shift != 0:
        v += shift * cc.walk(bra, ket)
    return v


# ---- the dense pin ----
def dense_value(bra, ket, mpo, shift=0.0):
    """vdot(dense(a), apply_mpo(mpo, dense(b))) + shift vdot(dense(a), dense(b))"""
    a, b = jo.dense_state(bra), jo.dense_state(ket)
    return np.vdot(a, ec.apply_mpo(mpo, b)) + shift * np.vdot(a, b)


def norm_of(cores):
    v = jo.dense_state(cores)
    return float(np.sqrt(np.vdot(v, v).real))


# ---- the physics case: cross_cases' spin chain, A = sum_p SZ_p, B = sum_p SX_p ----
def total(op):
    return [np.ascontiguousarray(w, dtype=np.complex128) for w in sb.sop_mpo([(1.0, {p: op}) for p in range(cc.L)], [2] * cc.L)]


def a_mpo():
    return total(sb.SZ)


def b_mpo():
    return total(sb.SX)


def phi_cores(mpo=None, vectors=None):
    """B psi for the product start as the front end builds it, padded to the bond dimensions of D, its norm kept"""
    from pytdscf_amd.mps import product_state_cores
    from pytdscf_amd.trajectories import mpo_on_product

    phi = mpo_on_product(b_mpo() if mpo is None else mpo, cc.start_vectors() if vectors is None else vectors)
    return orc.canonicalize_site0(product_state_cores(phi, cc.D), scale=None)


@functools.lru_cache(maxsize=None)
def oracle_runs(b_form="mpo", integrator="arnoldi", thresh=1e-9):
    """the oracle's states of psi and phi = B psi before steps 0 .. NSTEPS; b_form "site": cross_cases' one-site B"""
    if b_form == "site":
        return cc.oracle_runs(integrator, thresh)
    mpo = pc._spin_chain_mpo(cc.L)
    out = []
    for cores in (cc._product_cores(cc.start_vectors()), phi_cores()):
        st = orc.OracleMPS(cores, mpo, integrator=integrator, thresh=thresh, conserve_norm=False)
        hist = [[c.copy() for c in st.cores]]
        for _ in range(cc.NSTEPS):
            st.propagate(cc.DT)
            hist.append([c.copy() for c in st.cores])
        out.append(hist)
    return tuple(out)


def oracle_corr(a_form="mpo", b_form="mpo"):
    psi, phi = oracle_runs(b_form)
    if a_form == "mpo":
        return np.array([walk_mpo(a, b, a_mpo()) for a, b in zip(psi, phi)])
    return np.array([cc.walk(a, b, cc.A_OP[0], cc.A_OP[1]) for a, b in zip(psi, phi)])


@functools.lru_cache(maxsize=None)
def dense_corr(a_form="mpo", b_form="mpo"):
    """dense expm on the 16-dimensional space: C(t_k) for k = 0 .. NSTEPS"""
    from scipy.linalg import expm

    dims = [2] * cc.L
    H = jo.dense_operator(pc._spin_chain_mpo(cc.L))
    psi0 = functools.reduce(np.kron, cc.start_vectors())
    Aop = jo.dense_operator(a_mpo()) if a_form == "mpo" else jo.embed(cc.A_OP[1], cc.A_OP[0], dims)
    Bop = jo.dense_operator(b_mpo()) if b_form == "mpo" else jo.embed(cc.B_OP[1], cc.B_OP[0], dims)
    phi0 = Bop @ psi0
    out = []
    for k in range(cc.NSTEPS + 1):
        U = expm(-1j * H * cc.DT * k)
        out.append(np.vdot(U @ psi0, Aop @ (U @ phi0)))
    return np.array(out)


def model():
    """the case as a Model of the shell with the two sums as observables"""
    from pytdscf_amd import Exciton, Model

    return Model([Exciton(nstate=2) for _ in range(cc.L)],
                 operators={"hamiltonian": pc._spin_chain_mpo(cc.L), "sz_total": a_mpo(), "sx_total": b_mpo()}, bond_dim=cc.D)
