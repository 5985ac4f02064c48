"""Cases, NumPy twin and dense pin of the batched expectation values of MPO observables (k_batch_expect).

Shapes: the three of the spectra tests, for the same reasons (helpers/spectra_cases.SHAPES): ragged physical dimensions
and a bond narrower than the tile; every bond odd; bonds past the 32-wide tile and the 16-deep K step at 12 sites.

Operators per shape, as term lists [(coefficient, {site: matrix}), ...] through spin_bath.sop_mpo, MPO bonds <= 16:
  product    one product over all sites: M = 1, narrower than H
  local      one-site terms plus TWO nearest-neighbour products per bond, random Hermitian factors: M differs from H's
  longrange  sum_{p<q} c_pq A_p B_q with a factor A_p, B_q of its own per site and a full-rank c: M = 2 + the rank of c
             across the cut, above H's; the pair list is thinned until M <= 16 (it is 8 at L = 12 as it stands)
  complex    non-Hermitian factors, complex coefficients and a complex shift
  energy     operator 0, the Hamiltonian the replicas are propagated with (shift 0.1)
`SCALE` of an operator is sum_terms |coef| prod ||factor||_2 + |shift|: |<psi|O|psi> + shift <psi|psi>| <= SCALE <psi|psi>,
the size the relative bars of the tests are set against.

The pin is the dense state (jump_oracle.dense_state) with the MPO applied to the VECTOR core by core; no matrix of the
full space is ever built."""

import functools

import numpy as np

from helpers import cross_cases as cc
from helpers import jump_oracle as jo
from helpers import spectra_cases as sc
from helpers import spin_bath as sb

SHAPES = sc.SHAPES
LABELS = ("product", "local", "longrange", "complex", "energy")
OP_ID = {"energy": 0, "product": 1, "local": 2, "longrange": 3, "complex": 4}
H_SHIFT = 0.1
COMPLEX_SHIFT = 0.3 - 0.2j
MAX_MPO = 16
# The relative bar of the device tests against the dense pin: 1e-12 SCALE <psi|psi>.  The twin's own defect against the pin
# is asserted inside it by tests/test_batch_expect_host.py (largest observed there: 5.3e-5 of the bar, at the `wide` shape), so the bar stands as
# the issue states it.
BAR = 1e-12


def h_terms(name):
    """the Hamiltonians of the spectra tests: a spin chain for `wide`, random Hermitian one-site and nearest-neighbour
    terms otherwise"""
    dims, _ = SHAPES[name]
    L = len(dims)
    if name == "wide":
        terms = []
        for p in range(L):
            terms += [(0.3 + 0.1 * p, {p: sb.SZ}), (0.2, {p: sb.SX})]
        for p in range(L - 1):
            terms += [(0.5, {p: s, p + 1: s}) for s in (sb.SX, sb.SY, sb.SZ)]
        return terms
    terms = [(0.3 + 0.1 * p, {p: cc.random_op(d, 4 + p, hermitian=True)}) for p, d in enumerate(dims)]
    terms += [(0.2, {p: cc.random_op(dims[p], 24 + p, hermitian=True), p + 1: cc.random_op(dims[p + 1], 44 + p, hermitian=True)})
              for p in range(L - 1)]
    return terms


def _longrange_terms(dims, keep):
    L = len(dims)
    rng = np.random.default_rng(77)
    c = rng.uniform(0.1, 0.4, (L, L))
    A = [cc.random_op(d, 300 + p, hermitian=True) for p, d in enumerate(dims)]
    Bq = [cc.random_op(d, 400 + p, hermitian=True) for p, d in enumerate(dims)]
    pairs = [(p, q) for p in range(L) for q in range(p + 1, L)][::keep]
    return [(c[p, q], {p: A[p], q: Bq[q]}) for p, q in pairs]


@functools.lru_cache(maxsize=None)
def case(name, label):
    """(terms, shift, cores) of one operator; the cores are the rounded MPO (ml, d, d, mr per site)"""
    dims, _ = SHAPES[name]
    L = len(dims)
    shift = 0.0
    if label == "energy":
        terms, shift = h_terms(name), H_SHIFT
    elif label == "product":
        terms = [(0.7, {p: cc.random_op(d, 100 + p, hermitian=True) for p, d in enumerate(dims)})]
    elif label == "local":
        terms = [(0.2 + 0.05 * p, {p: cc.random_op(d, 120 + p, hermitian=True)}) for p, d in enumerate(dims)]
        for p in range(L - 1):
            for k in range(2):
                terms.append((0.15 + 0.1 * k, {p: cc.random_op(dims[p], 140 + 2 * p + k, hermitian=True),
                                               p + 1: cc.random_op(dims[p + 1], 180 + 2 * p + k, hermitian=True)}))
    elif label == "longrange":
        keep = 1
        while True:  # thinned until the rounded MPO fits the kernel's envelope
            terms = _longrange_terms(dims, keep)
            if max(w.shape[3] for w in sb.sop_mpo(terms, list(dims))) <= MAX_MPO:
                break
            keep += 1
    elif label == "complex":
        terms = [(0.3 - 0.2j, {p: cc.random_op(d, 220 + p)}) for p, d in enumerate(dims) if p % 2 == 0]
        terms += [(0.1 + 0.25j, {p: cc.random_op(dims[p], 240 + p), p + 1: cc.random_op(dims[p + 1], 260 + p)}) for p in range(L - 1)]
        shift = COMPLEX_SHIFT
    else:
        raise KeyError(label)
    cores = [np.ascontiguousarray(w, dtype=np.complex128) for w in sb.sop_mpo(terms, list(dims))]
    return terms, shift, cores


def max_bond(cores):
    return max(w.shape[3] for w in cores)


def scale(name, label):
    """sum_terms |coef| prod ||factor||_2 + |shift|"""
    terms, shift, _ = case(name, label)
    return sum(abs(c) * np.prod([np.linalg.norm(m, 2) for m in ops.values()]) for c, ops in terms) + abs(shift)


def random_states(name, n, seed=30):
    dims, D = SHAPES[name]
    return sc.random_states(dims, D, n, seed)


# ---- the dense pin ----
def apply_mpo(mpo, v):
    """O v for the state vector v (physical indices in site order), core by core: the intermediate is (MPO bond, sites
    done, sites to go); never a matrix of the full space"""
    x = np.asarray(v, dtype=np.complex128).reshape(1, 1, -1)
    for w in mpo:
        m, done, rest = x.shape
        d = w.shape[2]
        x = np.einsum("cijt,cajr->tair", w, x.reshape(m, done, d, rest // d)).reshape(w.shape[3], done * w.shape[1], rest // d)
    assert x.shape[0] == 1 and x.shape[2] == 1
    return x.reshape(-1)


def dense_value(cores, mpo, shift=0.0):
    """<psi|O|psi> + shift <psi|psi>, not normalised"""
    v = jo.dense_state(cores)
    return np.vdot(v, apply_mpo(mpo, v)) + shift * np.vdot(v, v).real


def norm2(cores):
    v = jo.dense_state(cores)
    return np.vdot(v, v).real


# ---- the NumPy twin of k_batch_expect's walk ----
def walk(cores, mpo, shift=0.0):
    """E = [1]; for p = L-1 .. 1: E'[a,q,r] = sum conj(B[a,i,b]) E[b,p,s] W[q,i,j,p] B[r,j,s] in the three stages of bt_env;
    then H = L W R C at site 0 in the three stages of bt_heff and <C|H> + shift <C|C>.  cores: centre at site 0."""
    E = np.ones((1, 1, 1), dtype=np.complex128)
    for p in range(len(cores) - 1, 0, -1):
        Bp, W = cores[p], mpo[p]
        X = np.einsum("aib,bps->iaps", Bp.conj(), E)        # X[(c,a)][(p,s)]
        Y = np.einsum("qijp,iaps->aqjs", W, X)              # Y[a][(q,t)][s]
        E = np.einsum("aqjs,rjs->aqr", Y, Bp)               # out[(a,q)][r]
    C, W = cores[0], mpo[0]
    Lb = np.ones((1, 1, 1), dtype=np.complex128)
    X = np.einsum("acb,bjs->acjs", Lb, C)
    Y = np.einsum("cijt,acjs->aits", W, X)
    H = np.einsum("aits,rts->air", Y, E)
    return np.vdot(C, H) + shift * np.vdot(C, C).real
