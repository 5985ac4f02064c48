"""Shared inputs of tests/test_batch_spectra_host.py and tests/test_gpu_batch_spectra.py: a NumPy restatement of the walk
of k_batch_spectra and of its record (with the record's summation order), the SVD of the dense state as the pin, state
builders, and the dynamics case with its dense ``expm`` reference, computed once."""

import functools

import numpy as np

from oracle import tdvp_oracle as orc

from . import cross_cases as cc
from . import jump_oracle as jo
from . import pair_cases as pc

HEAD = 4  # W, S1, S2, pmin in front of a bond's weights
TOL2, FREEZE, MAX_SWEEPS = 1.6e-29, 1e-32, 64  # BP_TOL2, BP_FREEZE, BATCH_PAIR_MAX_SWEEPS of batch_site

# the smallest shapes at which each part of the kernel can go wrong (tests/test_gpu_batch_spectra.py names why)
SHAPES = {"mixed": ((2, 3, 2, 4, 2), 6), "odd": ((3,) * 5, 7), "wide": ((2,) * 12, 40)}


def jacobi_rows(R):
    """one-sided Jacobi on the rows of R with the kernel's rotation, threshold and `tiny` rule (cyclic order: the order
    of the pairs changes the unitary that is left on R, not the row norms).  Returns (rotated R, converged)."""
    R = np.array(R, dtype=np.complex128)
    m = R.shape[0]
    tiny = FREEZE * np.sum(np.abs(R) ** 2)
    for _ in range(MAX_SWEEPS):
        any_rot = False
        for i in range(m - 1):
            for j in range(i + 1, m):
                x, y = R[i], R[j]
                a, b, g = np.vdot(x, x).real, np.vdot(y, y).real, np.vdot(y, x)  # g = sum x conj(y)
                g2 = abs(g) ** 2
                if not (g2 > TOL2 * a * b and a > tiny and b > tiny):
                    continue
                ag = np.sqrt(g2)
                zeta = (a - b) / (2.0 * ag)
                t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s, ph = c * t, g / ag
                R[i], R[j] = c * x + s * ph * y, -s * x + c * ph * y
                any_rot = True
        if not any_rot:
            return R, True
    return R, False


def record(nrm):
    """a bond's record from the squared row norms: ranked by counting, ties to the lower index (a stable descending
    sort); W, S1, S2 and pmin summed one after the other in that order; W == 0 gives zeros"""
    nrm = np.asarray(nrm, dtype=np.float64)
    srt = nrm[np.argsort(-nrm, kind="stable")]
    W = 0.0
    for v in srt:
        W += v
    s1 = s2 = pmin = 0.0
    if W > 0.0:
        p2 = 0.0
        for v in srt:
            p = v / W
            if p > 0.0:
                s1 -= p * np.log(p)
            p2 += p * p
        s2, pmin = -np.log(p2), srt[-1] / W
    return np.concatenate([[W, s1, s2, pmin], srt])


def entropies(weights):
    """(S1, S2, pmin) of a list of squared Schmidt values, by the record's rule"""
    return record(weights)[1:HEAD]


def walk(cores, bonds, rotate="jacobi"):
    """the kernel's walk on site-0 canonical cores: X = C_0; per bond q up to the last requested one, R of the thin QR of
    X as (dl d) x dr, Jacobi on its rows, the record of a requested bond, X = R' B_{q+1}.  Returns one record per bond.
    rotate="svd" takes R' = U^H R from LAPACK's SVD in the place of the Jacobi sweeps (the same rows up to phases and
    order): the fast form of the host route, which tools/batch_spectra_probe.py times."""
    bonds = list(bonds)
    out, X = [], np.asarray(cores[0], dtype=np.complex128)
    for q in range(bonds[-1] + 1):
        dl, d, dr = X.shape
        R = np.linalg.qr(X.reshape(dl * d, dr), mode="r")
        if rotate == "svd":
            _, s, vh = np.linalg.svd(R)
            R, ok = s[:, None] * vh, True
        else:
            R, ok = jacobi_rows(R)
        assert ok, f"the Jacobi sweeps of bond {q} did not converge"
        if q in bonds:
            out.append(record(np.sum(np.abs(R) ** 2, axis=1)))
        if q < bonds[-1]:
            X = np.tensordot(R, cores[q + 1], axes=(1, 0))
    return out


def dense_weights(cores, q, vec=None):
    """sigma^2 of bond q, descending, chi_q of them, from the SVD of the dense state reshaped at the bond"""
    dims = [c.shape[1] for c in cores]
    v = jo.dense_state(cores) if vec is None else vec
    s = np.linalg.svd(v.reshape(int(np.prod(dims[:q + 1])), -1), compute_uv=False) ** 2
    chi = cores[q].shape[2]
    return np.concatenate([s, np.zeros(max(chi - len(s), 0))])[:chi]


def entropy_bar(chi, delta=1e-12):
    """|S1(p') - S1(p)| <= chi delta (1 + |ln delta|) when every one of the chi weights moves by at most delta < 1/e: one
    term |x ln x - y ln y| <= |x - y| (1 + |ln |x - y||) (the slope of x ln x is 1 + ln x, steepest towards 0, where the
    term is bounded by -delta ln delta itself).  S2 = -ln sum p^2: sum p^2 >= 1 / chi moves by at most sum 2 p delta +
    chi delta^2, about 2 delta, so S2 moves by about 2 chi delta; pmin moves by delta.  Both are inside the same figure
    (1 + |ln delta| > 2), which the tests therefore use for all three."""
    return chi * delta * (1.0 + abs(np.log(delta)))


def random_states(dims, D, n, seed):
    """n random complex states, site-0 canonical, with norms 0.7, 0.9, 1.1, ..."""
    return cc.random_states(dims, D, n, seed)


def bell_chain(L=6, D=4):
    """Bell pairs on (0, 1), (2, 3), ...: ranks 2, 1, 2, 1, ... zero-padded to the bonds of D, NOT canonical (set it
    with canonicalize=True, or through canonicalize_site0); S1 = ln 2 on even bonds, 0 on odd ones, norm 1"""
    from pytdscf_amd.mps import bond_dims

    cores = []
    for dl, dr in bond_dims([2] * L, D):
        p = len(cores)
        c = np.zeros((dl, 2, dr), dtype=np.complex128)
        if p % 2 == 0:
            c[0, 0, 0] = c[0, 1, 1] = 2.0 ** -0.25  # |0>(0| + |1>(1|: two equal Schmidt values
        else:
            c[0, 0, 0] = c[1, 1, 0] = 2.0 ** -0.25
        cores.append(c)
    return cores


def product_padded(dims, D, seed=5):
    """a random Hartree product zero-padded to D, as propagate_trajectories builds its starts"""
    from pytdscf_amd.mps import product_state_cores

    rng = np.random.default_rng(seed)
    vecs = [rng.standard_normal(d) + 1j * rng.standard_normal(d) for d in dims]
    return product_state_cores(vecs, D, space="hilbert")


# ---- the dynamics case: L = 6 spin chain at full bond dimension, Arnoldi, against dense expm ----
DYN_L, DYN_D, DYN_DT, DYN_STEPS, DYN_THRESH = 6, 8, 0.3, 4, 1e-10


def dyn_start():
    return random_states((2,) * DYN_L, DYN_D, 1, seed=11)[0]


def dyn_bar():
    """At full bond dimension one-site TDVP is exact up to its local exponentials.  A time step has 2 (2 L - 1) of them,
    each stopped when its last correction is below thresh_sil relative to a state of norm |psi|: the state after k steps
    is within eps = k 2 (2 L - 1) thresh |psi| of exp(-i H k dt) psi.  Singular values move by at most eps (Weyl), so a
    normalised weight moves by at most delta = 2 eps / |psi| + O(eps^2), and S1 by entropy_bar(chi, delta) at chi = 8."""
    delta = 2.0 * DYN_STEPS * 2 * (2 * DYN_L - 1) * DYN_THRESH
    return entropy_bar(DYN_D, 1.01 * delta)


@functools.lru_cache(maxsize=None)
def dyn_dense():
    """S1 of every bond before steps 0 .. DYN_STEPS from dense expm: (DYN_STEPS + 1, L - 1)"""
    from scipy.linalg import expm

    start = dyn_start()
    H = jo.dense_operator(pc._spin_chain_mpo(DYN_L))
    v0 = jo.dense_state(start)
    U = expm(-1j * H * DYN_DT)
    out, v = [], v0
    for _ in range(DYN_STEPS + 1):
        out.append([entropies(dense_weights(start, q, vec=v))[0] for q in range(DYN_L - 1)])
        v = U @ v
    return np.array(out)


@functools.lru_cache(maxsize=None)
def dyn_oracle():
    """the same from the NumPy oracle's states and the walk model"""
    st = orc.OracleMPS([c.copy() for c in dyn_start()], pc._spin_chain_mpo(DYN_L), integrator="arnoldi", thresh=DYN_THRESH,
                       conserve_norm=False)
    out = []
    for k in range(DYN_STEPS + 1):
        out.append([r[1] for r in walk(st.cores, range(DYN_L - 1))])
        if k < DYN_STEPS:
            st.propagate(DYN_DT)
    return np.array(out)
