"""References, operators and the case tables of the local Krylov exponential x <- exp(s Op) x
(tests/test_local_exp_host.py on the CPU, tests/test_gpu_local_exp.py on the device).  NumPy / SciPy only.

Three references:
  * ``exact_exp``: the operation itself in double precision (``eigh`` / ``scipy.linalg.expm``);
  * ``sil_ref``: the oracle's ``sil_lanczos`` / ``sil_arnoldi`` (lanczos_variant = "reference", Arnoldi), untouched;
  * ``sil_orthodox``: the oracle's ``sil_lanczos`` with alpha_l = <v_l | H v_l> (lanczos_variant = "orthodox").
Both SIL references also hand back the successive-approximant differences ||psi_l - psi_(l-1)|| they compared with the
threshold, last two: a case whose Krylov count a test asserts must not sit near the threshold (``well_separated``).
"""

from __future__ import annotations

import cmath

import numpy as np
import scipy.linalg

from oracle import tdvp_oracle as orc

EPS = orc.EPS
MAX_KRYLOV = orc.MAX_KRYLOV
THRESH = 1e-9
PARITY = 1e-11  # device against its statement-level reference, max norm: the bar of test_unit_golden_krylov


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
class RecordingThresh(float):
    """A threshold that remembers what it was compared with.  The SIL references test ``float(norm) < thresh``; float
    defers ``<`` to the reflected ``>`` of a subclass on the right, so the oracle's own code records its differences
    without being edited."""

    def __new__(cls, value):
        self = super().__new__(cls, value)
        self.seen = []
        return self

    def __gt__(self, other):
        self.seen.append(float(other))
        return float(other) < float(self)

    def last_two(self):
        s = self.seen
        return (s[-2] if len(s) > 1 else None, s[-1] if s else None)


def sil_ref(integrator, scale, matvec, psi, thresh=THRESH, k_prev=0, conserve_norm=True):
    """the oracle (variant "reference" or Arnoldi): (psi_new, k, (difference before the closing one, closing one))"""
    fn = orc.sil_lanczos if integrator == "lanczos" else orc.sil_arnoldi
    t = RecordingThresh(thresh)
    with np.errstate(invalid="ignore", divide="ignore"):
        y, k = fn(scale, matvec, psi, t, k_prev, conserve_norm)
    return y, k, t.last_two()


def sil_orthodox(scale, matvec, psi, thresh=THRESH, k_prev=0, conserve_norm=True):
    """``oracle.tdvp_oracle.sil_lanczos`` with ONE change: alpha_l = <v_l | H v_l>, kept complex (the textbook
    recurrence; what the kernels do for variant = 1).  Same warm-up, ``beta >= EPS`` rule, projected exponential,
    convergence test, rescale and error messages.  Returns (psi_new, k, (difference before the closing one, closing one))."""
    shape = psi.shape
    v0 = np.array(psi, dtype=np.complex128).reshape(-1)
    size = v0.size
    ndim = min(size, MAX_KRYLOV)
    n_warm = orc._n_warmup(size, k_prev)
    if conserve_norm:
        beta0 = 1.0
    else:
        beta0 = float(np.linalg.norm(v0))
        if beta0 == 0.0:
            raise ValueError("Initial psi has zero norm.")
        v0 = v0 / beta0
    V = [v0]
    alpha: list[complex] = []
    beta: list[float] = []
    alpha_is_real = True
    psi_sv = None
    beta_l = 0.0
    diffs: list[float] = []
    for ldim in range(ndim):
        trial = psi if ldim == 0 else V[-1].reshape(shape)
        v_l = np.array(matvec(trial)).reshape(-1)
        if not conserve_norm and ldim == 0:
            v_l = v_l / beta0
        a_l = complex(np.inner(np.conj(V[-1]), v_l))  # the one change: <v_l | H v_l>, not <v_0 | H v_l>
        alpha.append(a_l)
        v_l = v_l - V[-1] * a_l
        if ldim > 0:
            v_l = v_l - V[-2] * beta_l
        beta_l = float(np.linalg.norm(v_l))
        beta.append(beta_l)
        if beta_l >= EPS:
            v_l = v_l / beta_l
        V.append(v_l)
        is_converged = beta_l < EPS or ldim + 1 == size
        if alpha_is_real and abs(a_l.imag) > 1e-10:
            alpha_is_real = False
        if ldim < n_warm and not is_converged:
            continue
        if ldim == 0:
            psi_next = v0 * cmath.exp(scale * alpha[-1])
        else:
            if alpha_is_real:
                lam, phi = scipy.linalg.eigh_tridiagonal(np.real(alpha), beta[:-1])
                coef = phi @ (np.exp(scale * lam) * np.conjugate(phi).T[:, 0])
            else:
                mat = (np.diag(alpha, 0) + np.diag(beta[:-1], -1).astype(np.complex128)
                       + np.diag(beta[:-1], 1).astype(np.complex128))
                lam, phi = scipy.linalg.eig(mat)
                e0 = np.zeros(ldim + 1, dtype=mat.dtype)
                e0[0] = 1
                coef = phi @ (np.exp(scale * lam) * np.linalg.solve(phi, e0))
            psi_next = np.dot(coef, np.array(V[:-1]))
        done = is_converged
        if not done:
            if psi_sv is not None:
                diffs.append(float(np.linalg.norm(psi_next - psi_sv)))
                if diffs[-1] < thresh:
                    done = True
            psi_sv = psi_next
        if done:
            if conserve_norm:
                with np.errstate(invalid="ignore", divide="ignore"):
                    psi_next = psi_next / float(np.linalg.norm(psi_next))
            else:
                psi_next = psi_next * beta0
            return psi_next.reshape(shape), ldim + 1, (diffs[-2] if len(diffs) > 1 else None, diffs[-1] if diffs else None)
    raise ValueError(f"Short Iterative Lanczos is not converged in {ndim} basis. Try shorter time interval.")


def sil(integrator, variant, scale, matvec, psi, thresh=THRESH, k_prev=0, conserve_norm=True):
    """the statement-level reference of one device configuration"""
    if integrator == "lanczos" and variant == "orthodox":
        return sil_orthodox(scale, matvec, psi, thresh, k_prev, conserve_norm)
    return sil_ref(integrator, scale, matvec, psi, thresh, k_prev, conserve_norm)


def is_hermitian(H):
    return bool(np.abs(H - H.conj().T).max() <= 1e-14 * max(1.0, np.abs(H).max()))


def exact_exp(scale, H, x, conserve_norm=True):
    """exp(scale H) x in double precision: ``eigh`` for a Hermitian H, ``scipy.linalg.expm`` otherwise; normalised when
    ``conserve_norm``"""
    x = np.asarray(x, dtype=np.complex128)
    v = x.reshape(-1)
    if is_hermitian(H):
        lam, U = np.linalg.eigh((H + H.conj().T) / 2)
        y = U @ (np.exp(scale * lam) * (U.conj().T @ v))
    else:
        y = scipy.linalg.expm(scale * H) @ v
    if conserve_norm:
        y = y / np.linalg.norm(y)
    return y.reshape(x.shape)


def err(y, ref):
    """max-norm distance; with ``PARITY`` in the same norm, |dev - exact| <= |ref - exact| + |dev - ref| is the
    triangle inequality, which is where the bar against ``exact_exp`` comes from"""
    return float(np.abs(np.asarray(y) - np.asarray(ref)).max())


# How far from the threshold the two differences that decide k must lie, as a factor.  Successive approximants of a
# short-iterative solve close in on each other by a factor of about 2 m / (|s| rho) per vector (m: Krylov dimension,
# rho: spectral radius): 15 to 25 for ``wide`` at either scale, 40 to 70 for ``herm`` at s = -0.1i, above 100 only for
# ``herm`` at s = -0.05 -- measured on the references, and no seed changes it at n >= 300, where the spectrum is
# self-averaging.  A factor of 10 on BOTH sides of the threshold needs two consecutive differences a factor 100 apart,
# which most of these families never offer; so the threshold of a case is placed at the geometric mean of the reference's
# last two differences (``placed_thresh``) and the condition asks for MARGIN = 3 on each side (sqrt(15) = 3.9 is the least
# any family leaves).  The device's differences deviate from the reference's by rounding (relative 1e-6 at the very most:
# PARITY on vectors of norm 1 against differences of 1e-11 .. 1e-8 between them would be 1e-3 .. 1), far inside a factor 3.
MARGIN = 3.0


def margins(diffs, thresh):
    """(thresh / closing difference, difference before it / thresh); None where the solve made no such comparison"""
    before, last = diffs
    return (None if last is None else thresh / max(last, 1e-300), None if before is None else before / thresh)


def well_separated(diffs, thresh, factor=MARGIN, exhausted=False):
    """the input condition of a case whose k is asserted: the closing difference is < thresh / factor and the one
    before it (when the solve compared more than once) is > factor * thresh, so that no rounding of the device moves k.
    A solve closed at k = 1 compared nothing and is exempt; one closed by ``exhausted`` Krylov space (k = n) must not
    have come near the threshold before: whatever it compared is > factor * thresh."""
    if exhausted:
        return all(d is None or d > factor * thresh for d in diffs)
    m_last, m_before = margins(diffs, thresh)
    return (m_last is None or m_last > factor) and (m_before is None or m_before > factor)


def placed_thresh(integrator, variant, scale, matvec, psi, k_prev=0, conserve_norm=True, chained=False):
    """The threshold of a case.  1e-9 when the reference's solve at 1e-9 does not converge or made fewer than two
    comparisons; else the geometric mean of its last two differences (two significant digits): the same k, as far from
    both as it can be.  ``chained``: a second solve follows, from the first's result with its k as memory; where that one
    ends up close to the threshold, the value in [1e-10, 1e-8] that leaves both solves the widest margin is taken."""

    def run(t):
        y, k, d = sil(integrator, variant, scale, matvec, psi, t, k_prev, conserve_norm)
        return [d] + ([sil(integrator, variant, scale, matvec, y, t, k, conserve_norm)[2]] if chained else [])

    def worst(t):
        try:
            ms = [m for d in run(t) for m in margins(d, t) if m is not None]
        except ValueError:
            return 0.0
        return min(ms) if ms else np.inf

    try:
        before, last = run(THRESH)[0]
        exhausted = sil(integrator, variant, scale, matvec, psi, THRESH, k_prev, conserve_norm)[1] == np.size(psi)
    except ValueError:  # does not converge: the case is about the message
        return THRESH
    if before is None or last is None or exhausted:
        return THRESH
    t = float(f"{np.sqrt(before * last):.1e}")
    if not chained or worst(t) > MARGIN:
        return t
    return max([float(f"{c:.1e}") for c in np.geomspace(1e-10, 1e-8, 17)] + [t], key=worst)


def first_column_norm(scale, H, x):
    """|s| (|alpha_0| + beta_0): the 1-norm of column 0 of s T_k for every k >= 2 and both Lanczos variants (alpha_0 and
    beta_0 do not depend on the variant), a lower bound of |s T_k|_1.  Above 8 the one-wave Taylor form of the projected
    exponential (at most 3 halvings to norm <= 1) is not taken and the dense scaling-and-squaring routine runs."""
    v = np.asarray(x, dtype=np.complex128).reshape(-1)
    v = v / np.linalg.norm(v)
    w = H @ v
    a0 = np.vdot(v, w)
    b0 = np.linalg.norm(w - a0 * v)
    return abs(scale) * (abs(a0) + b0)


# ---------------------------------------------------------------------------------------------------------------------
# operators and start vectors, all seeded
# ---------------------------------------------------------------------------------------------------------------------
def _crandn(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


def herm(n, seed=0):
    """GUE scaled by 1 / sqrt(n): spectrum in about [-2, 2] at any n"""
    a = _crandn(np.random.default_rng(1000 + seed), n, n)
    return (a + a.conj().T) / (2.0 * np.sqrt(n))


def shifted(n, seed=0, e0=100.0):
    """a large diagonal offset (zero-point energy, unshifted electronic origin): the projected exponential's large-norm branch"""
    return herm(n, seed) + e0 * np.eye(n)


def wide(n, seed=0):
    return 4.0 * herm(n, seed)


def nonherm(n, seed=0):
    u = np.random.default_rng(2000 + seed).random(n)
    return herm(n, seed) - 0.3j * np.diag(u)


def eigen_start(H, j):
    lam, U = np.linalg.eigh(H)
    return np.ascontiguousarray(U[:, j])


def start(n, seed=0, norm=1.0):
    v = _crandn(np.random.default_rng(3000 + seed), n)
    return v * (norm / np.linalg.norm(v))


OPERATORS = {"herm": herm, "shifted": shifted, "wide": wide, "nonherm": nonherm}


# ---------------------------------------------------------------------------------------------------------------------
# one-site engine seam: H_eff = sum_c A_c (x) B_c (x) C_c from boundary blocks and a bond-diagonal core
# ---------------------------------------------------------------------------------------------------------------------
class Seam:
    """Hermitian blocks of a one-site problem: L[a,c,b] = A_c[a,b] (dl, m, dl), W[c,:,:,c] = B_c, R[r,t,s] = C_t[r,s]
    (dr, m, dr); ``gain`` scales the operator, ``shift`` is handed to ``set_mpo(..., shift=)`` and added by the
    references as ``shift * x``."""

    def __init__(self, dl, d, dr, m, seed=0, shift=0.0, gain=1.0, norm=1.0):
        self.dl, self.d, self.dr, self.m, self.shift, self.seed = dl, d, dr, m, shift, seed
        self.L = np.zeros((dl, m, dl), dtype=np.complex128)
        self.R = np.zeros((dr, m, dr), dtype=np.complex128)
        self.W = np.zeros((m, d, d, m), dtype=np.complex128)
        for c in range(m):
            self.L[:, c, :] = herm(dl, 10 * seed + c) * gain
            self.W[c, :, :, c] = herm(d, 10 * seed + 3 + c)
            self.R[:, c, :] = herm(dr, 10 * seed + 6 + c)
        self.psi = start(dl * d * dr, seed, norm).reshape(dl, d, dr)

    @property
    def n(self):
        return self.dl * self.d * self.dr

    def heff(self, x):
        y = orc.heff_apply(self.L, self.W, self.R, x)
        return y + self.shift * x if self.shift != 0.0 else y

    def heff_dense(self):
        """the matrix of ``heff`` by the oracle's own contraction of every unit vector (row-major (a, i, r))"""
        n = self.n
        H = np.empty((n, n), dtype=np.complex128)
        e = np.zeros(n, dtype=np.complex128)
        for j in range(n):
            e[j] = 1.0
            H[:, j] = self.heff(e.reshape(self.dl, self.d, self.dr)).reshape(-1)
            e[j] = 0.0
        return H

    def engine(self, TDVPEngine, small_kernels=True, **kw):
        eng = TDVPEngine(1, **kw)
        eng.set_small_kernels(small_kernels)
        eng.set_boundary_env(0, self.L)
        eng.set_boundary_env(1, self.R)
        eng.set_mpo([self.W], shift=self.shift)
        eng.set_site(0, self.psi, "Psi")
        return eng

    # ---- the bond right of the site after a forward split: K_eff = sum_c A'_c (x) C_c --------------------------------
    def keff_blocks(self, A):
        """(L', R) around the bond after the site became the isometry A: the oracle's environment update"""
        return orc.env_update_left(self.L, A, self.W), self.R

    def keff(self, Lp):
        def mv(s):
            y = orc.keff_apply(Lp, self.R, s)
            return y + self.shift * s if self.shift != 0.0 else y

        return mv

    def keff_dense(self, Lp):
        n = self.dr * self.dr
        K = np.empty((n, n), dtype=np.complex128)
        e = np.zeros(n, dtype=np.complex128)
        mv = self.keff(Lp)
        for j in range(n):
            e[j] = 1.0
            K[:, j] = mv(e.reshape(self.dr, self.dr)).reshape(-1)
            e[j] = 0.0
        return K


def iterations_run(k, k_prev, size):
    """iterations Engine::krylov_exp issues for a solve that closes at k: it reads no record before iteration l_sync
    (the first at which the warm-up rule allows convergence), so a solve closed earlier (exhaustion) runs up to there"""
    ndim = min(size, MAX_KRYLOV)
    l_sync = min(orc._n_warmup(size, k_prev) + 1, ndim - 1, size - 1)
    return max(k, l_sync + 1)


def inspections(iters, k_prev, size):
    """how many of the first ``iters`` iterations the schedule inspects: all but those of the warm-up, which are skipped
    unless they exhaust the space (l + 1 = size) or are the last the basis allows (l + 1 = ndim)"""
    n_warm, ndim = orc._n_warmup(size, k_prev), min(size, MAX_KRYLOV)
    return sum(1 for l in range(iters) if not (l < n_warm and l + 1 != size and l + 1 < ndim))


def step_launches(dlaunch, iters, k_prev, size, conserve_norm, mv):
    """Launches per iteration of a multi-launch solve that are NOT the operator's: Engine::krylov_exp issues, per
    iteration, the apply (``mv`` launches) and the vector step -- ONE launch on path A (k_lanczos_step_small), TWO on
    path B (dot + k_lanczos_update_def), THREE on path C (Arnoldi) --, two per inspected iteration (Ritz step and
    difference), two to form the result and two more without conserve_norm (norm of the start vector and its scaling)."""
    rest = dlaunch - 2 * inspections(iters, k_prev, size) - 2 - (0 if conserve_norm else 2) - iters * mv
    assert rest % iters == 0, (dlaunch, iters, mv)
    return rest // iters


# ---------------------------------------------------------------------------------------------------------------------
# batch: the oracle's sweep with the orthodox recurrence in place of its _exp
# ---------------------------------------------------------------------------------------------------------------------
class OrthodoxOracleMPS(orc.OracleMPS):
    def _exp(self, scale, matvec, x, site, size=None):
        out, k, _ = sil_orthodox(scale, matvec, x, self.thresh, self.kprev.get(site, 0), self.conserve_norm)
        self.kprev[site] = k
        return out


# ---------------------------------------------------------------------------------------------------------------------
# the dense cases (mitdvp_expm_dense): one table for the host test and the GPU test
# ---------------------------------------------------------------------------------------------------------------------
CONFIGS = [("lanczos", "reference"), ("lanczos", "orthodox"), ("arnoldi", "reference")]
# scale, conserve_norm, |x| (without conserve_norm the start vector always has norm 1.7)
SCALES = {"real_time": (-0.1j, True, 1.0), "damped": (-0.05 + 0j, False, 1.7), "real_time_open": (-0.1j, False, 1.7)}


class DenseCase:
    def __init__(self, op, n, scale_name, k_prev, seed=0, e0=None):
        self.op, self.n, self.scale_name, self.k_prev, self.seed, self.e0 = op, n, scale_name, k_prev, seed, e0
        self.scale, self.cn, self.norm = SCALES[scale_name]
        self.id = f"{op}{'' if e0 is None else int(e0)}-n{n}-{scale_name}-kprev{k_prev}"
        self.family = f"{op}{'' if e0 is None else int(e0)} {scale_name}{' k_prev=20' if k_prev == 20 else ''}"

    def matrix(self):
        return operator(self.op, self.n, self.seed, self.e0)[0]

    def vector(self):
        return start(self.n, self.seed, self.norm)

    def exact(self, x):
        H, lam, U = operator(self.op, self.n, self.seed, self.e0)
        if lam is None:
            return exact_exp(self.scale, H, x, self.cn)
        y = U @ (np.exp(self.scale * lam) * (U.conj().T @ x))
        return y / np.linalg.norm(y) if self.cn else y

    def dense_branch(self):
        """the cases whose projected exponential must take the large-norm branch: an offset e0 with |s| e0 = 10"""
        return self.op == "shifted" and abs(self.scale) * (100.0 if self.e0 is None else self.e0) > 8


_OPS: dict = {}


def operator(op, n, seed=0, e0=None):
    """(H, eigenvalues, eigenvectors) -- the last two None for a non-Hermitian H; the two most recent are kept"""
    key = (op, n, seed, e0)
    if key not in _OPS:
        while len(_OPS) >= 2:
            _OPS.pop(next(iter(_OPS)))
        H = OPERATORS[op](n, seed) if e0 is None else OPERATORS[op](n, seed, e0)
        lam, U = np.linalg.eigh(H) if is_hermitian(H) else (None, None)
        _OPS[key] = (H, lam, U)
    return _OPS[key]


def grid_cases():
    out = [DenseCase(op, n, sc, kp) for op in ("herm", "shifted", "wide") for n in (36, 300, 1025)
           for sc in ("real_time", "damped") for kp in (0, 20)]
    # |s| e0 = 0.05 * 100 = 5 stays under the branch's threshold of 8: the damped scale reaches the dense branch with
    # an offset of 200 (|s| e0 = 10, as at the real-time scale)
    out += [DenseCase("shifted", n, "damped", kp, e0=200.0) for n in (36, 300) for kp in (0, 20)]
    out += [DenseCase("nonherm", 300, "real_time_open", kp) for kp in (0, 20)]
    return out


def reference_unstable(case, integrator):
    """Arnoldi behind a saturated warm-up on an operator with a large offset: fifteen uninspected classical
    Gram-Schmidt steps on 100 + h lose the basis' orthogonality, and the oracle's ``eig`` + ``solve`` of the Hessenberg
    matrix then returns noise of the order of the threshold -- it raises "not converged" at s = -0.1i and is 1e-11 from
    the exact result at s = -0.05 (test_local_exp_host.py shows both).  Its verdict and its k are decided by rounding:
    the device is held to the verdicts open to it (``unstable_reference``), not to the oracle's k."""
    return integrator == "arnoldi" and case.op == "shifted" and case.k_prev == 20


def unstable_reference(case, integrator, variant):
    """a ``reference_unstable`` case at the plain threshold: ``raises`` (the oracle's message or None), its result, k and
    error where it returns, and the exact result"""
    H, x = case.matrix(), case.vector()
    r = Ref()
    r.thresh, r.raises, r.ex1 = THRESH, None, case.exact(x)
    try:
        r.y1, r.k1, r.d1 = sil(integrator, variant, case.scale, lambda v: H @ v, x, THRESH, case.k_prev, case.cn)
        r.err1 = err(r.y1, r.ex1)
    except ValueError as e:
        r.raises = str(e)
    return r


class Ref:
    """what the statement-level reference and ``exact_exp`` say about one case and configuration: the first solve from
    the case's vector with its k_prev, then (k_prev = 0 only) a second one from the first's result with k_prev = k1"""


_REFS: dict = {}


def dense_reference(case, integrator, variant):
    key = (case.id, case.seed, integrator, variant)
    if key in _REFS:
        return _REFS[key]
    H, x = case.matrix(), case.vector()

    def mv(v):
        return H @ v

    r = Ref()
    r.thresh = placed_thresh(integrator, variant, case.scale, mv, x, case.k_prev, case.cn, chained=case.k_prev == 0)
    r.y1, r.k1, r.d1 = sil(integrator, variant, case.scale, mv, x, r.thresh, case.k_prev, case.cn)
    r.ex1 = case.exact(x)
    r.err1 = err(r.y1, r.ex1)
    r.exhausted = r.k1 == case.n  # closed by the size of the space, not by the threshold
    r.chained = case.k_prev == 0
    if r.chained:
        r.y2, r.k2, r.d2 = sil(integrator, variant, case.scale, mv, r.y1, r.thresh, r.k1, case.cn)
        r.ex2 = case.exact(r.y1)
        r.err2 = err(r.y2, r.ex2)
    _REFS[key] = r
    return r


EXHAUST_N = (1, 2, 3, 5, 20, 21)  # exhaustion of the Krylov space, and nsize = ndim and ndim + 1


def edge_cases():
    return [DenseCase("herm", n, "real_time", kp, seed=1) for n in EXHAUST_N for kp in (0, 20)]


NOT_CONVERGING = dict(n=300, gain=30.0, scale=-0.1j)  # 30 * wide: spectrum +-240, a phase of 24 over the step


# ---------------------------------------------------------------------------------------------------------------------
# the engine cases (site_exp / bond_exp on a one-site engine)
# ---------------------------------------------------------------------------------------------------------------------
SHAPE_SMALL = (8, 4, 8, 3)    # inside the one-launch plan: paths D and B (small kernels off)
SHAPE_LONG = (2, 3, 171, 3)   # n = 1026 <= 16384, but the R block of a chunk (3 x 22 x 171 numbers) overflows the
#                               plan's LDS: path A with small kernels on, path B with them off
SHAPE_NATURAL_B = (72, 4, 72, 3)  # n = 20736 > 16384: path B whatever the switch says


class EngineConfig:
    def __init__(self, integrator, variant, shift=0.0, relax=False, cn=True):
        self.integrator, self.variant, self.shift, self.relax, self.cn = integrator, variant, shift, relax, cn
        self.dt = 1.0 if relax else 0.2  # s = -0.5 (relaxation) or -0.1i for the site, the opposite sign for the bond
        self.norm = 1.0 if cn else 1.7
        self.id = (f"{integrator}-{variant}" if integrator == "lanczos" else "arnoldi") + \
                  ("-shift100" if shift else "") + ("-relax" if relax else "") + ("" if cn else "-open")
        self.family = ("shifted " if shift else "plain ") + ("relax" if relax else "real_time") + ("" if cn else " open")

    def site_scale(self):
        return -self.dt / 2 + 0j if self.relax else -0.5j * self.dt

    def bond_scale(self):
        return -self.site_scale()

    def engine_kw(self):
        return dict(integrator=self.integrator, lanczos_variant=self.variant, relax=self.relax, conserve_norm=self.cn)


ENGINE_CONFIGS = ([EngineConfig("lanczos", v, sh, rx) for v in ("reference", "orthodox") for sh in (0.0, 100.0) for rx in (False, True)]
                  + [EngineConfig("arnoldi", "reference", sh, rx) for sh in (0.0, 100.0) for rx in (False, True)]
                  + [EngineConfig(i, v, cn=False) for i, v in CONFIGS])


GAIN = 0.5  # brings the spectral radius of H_eff = sum_c A_c (x) B_c (x) C_c to about that of ``herm`` (2)
# (shape, config id) -> seed, where seed 0 leaves one of the solves too close to its threshold whatever the threshold
_ENGINE_SEEDS: dict = {((8, 4, 8, 3), "lanczos-reference-relax"): 10, ((2, 3, 171, 3), "lanczos-reference-relax"): 2,
                       ((13, 10, 21, 6), "lanczos-reference-relax"): 2}
# (shape, config id) -> gain, where no seed does at GAIN: the relaxation's approximants of this shape close in by a factor of
# about 10 per vector at GAIN (seeds 0 .. 12 leave a margin below 3 on one of the two solves), by about 15 at 0.25
_ENGINE_GAINS: dict = {((13, 10, 21, 6), "lanczos-reference-relax"): 0.25}

_SPECTRA: dict = {}


def seam_spectral(sm):
    """(H_eff without the shift, its eigenvalues, eigenvectors) of a seam's blocks, computed once per set of blocks"""
    key = (sm.dl, sm.d, sm.dr, sm.m, sm.seed)
    if key not in _SPECTRA:
        shift, sm.shift = sm.shift, 0.0
        try:
            H = sm.heff_dense()
        finally:
            sm.shift = shift
        lam, U = np.linalg.eigh(H)
        _SPECTRA[key] = (H, lam, U)
    return _SPECTRA[key]


def seam_exact(sm, scale, x, cn):
    _, lam, U = seam_spectral(sm)
    y = U @ (np.exp(scale * (lam + sm.shift)) * (U.conj().T @ np.asarray(x).reshape(-1)))
    return (y / np.linalg.norm(y) if cn else y).reshape(np.shape(x))


def seam_for(shape, cfg):
    dl, d, dr, m = shape
    return Seam(dl, d, dr, m, seed=_ENGINE_SEEDS.get((shape, cfg.id), 0), shift=cfg.shift,
                gain=_ENGINE_GAINS.get((shape, cfg.id), GAIN), norm=cfg.norm)


def site_reference(shape, cfg, dense=True):
    """Two site solves in a row by the reference (the second from the first's result with the first's k as memory) and
    the exact results from the dense H_eff.  ``r.raises``: the reference's error message when it does not converge."""
    key = ("site", shape, cfg.id)
    if key in _REFS:
        return _REFS[key]
    sm = seam_for(shape, cfg)
    s = cfg.site_scale()
    r = Ref()
    r.seam, r.raises = sm, None
    try:
        r.thresh = placed_thresh(cfg.integrator, cfg.variant, s, sm.heff, sm.psi, 0, cfg.cn, chained=True)
        r.y1, r.k1, r.d1 = sil(cfg.integrator, cfg.variant, s, sm.heff, sm.psi, r.thresh, 0, cfg.cn)
        r.y2, r.k2, r.d2 = sil(cfg.integrator, cfg.variant, s, sm.heff, r.y1, r.thresh, r.k1, cfg.cn)
    except ValueError as e:
        r.raises, r.thresh = str(e), THRESH
    if dense:
        H0 = seam_spectral(sm)[0]
        v = sm.psi.reshape(-1)
        r.first_column = first_column_norm(s, H0, v) + abs(s) * abs(sm.shift)  # alpha_0 moves by the shift, beta_0 does not
        if not r.raises:
            r.ex1 = seam_exact(sm, s, sm.psi, cfg.cn)
            r.ex2 = seam_exact(sm, s, r.y1, cfg.cn)
            r.err1, r.err2 = err(r.y1, r.ex1), err(r.y2, r.ex2)
    _REFS[key] = r
    return r


def bond_reference(sm, cfg, A, sigma, k_prev, thresh):
    """the bond solve after a forward split that left the isometry A and the bond matrix sigma"""
    Lp, _ = sm.keff_blocks(A)
    s = cfg.bond_scale()
    r = Ref()
    r.Lp, r.raises = Lp, None
    K = sm.keff_dense(Lp)
    r.first_column = first_column_norm(s, K, sigma)
    r.ex = exact_exp(s, K, sigma, cfg.cn)
    try:
        r.y, r.k, r.d = sil(cfg.integrator, cfg.variant, s, sm.keff(Lp), sigma, thresh, k_prev, cfg.cn)
    except ValueError as e:
        r.raises = str(e)
        return r
    r.err = err(r.y, r.ex)
    return r
