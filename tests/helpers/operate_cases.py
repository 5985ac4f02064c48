"""Cases, NumPy twin and pins of the batched operator application (k_batch_operate, TDVPBatch.operate).

The pins are the reference's own result (tests/golden/operate_chain.npz: L = 6, d = 3, M = 3, D = 5) and
``oracle.tdvp_oracle.operate``.  bt_qr is gauge-free, and the fitted state as a vector depends on neither the QR phases nor
on a global phase, so everything is compared as DENSE states or overlaps, never tensor by tensor:
  BAR_STATE  |phi_got - phi_pin|_2 <= 1e-9 (both normalised)       the bars of tests/test_gpu_operate.py, gauge-free
  BAR_NORM   |norm_got - norm_pin| <= 1e-10 norm_pin

Shapes and operators are those of helpers/expect_cases (three shapes, five operators each: MPO bonds 1 to 8, one
non-Hermitian with a complex shift, operator 0 with shift 0.1); the states are cross_cases.random_states with norms
0.7 / 0.9 / 1.1.  Everything the oracle computes is computed once and shared."""

import functools
import os

import numpy as np

from oracle import tdvp_oracle as orc

from . import cross_cases as cc
from . import expect_cases as ec
from . import jump_oracle as jo

BAR_STATE = 1e-9
BAR_NORM = 1e-10
SHAPES = ec.SHAPES
LABELS = ec.LABELS
NSTATES = 3
MAXSTEP = 2  # of the shapes x operators cases, with conv_tol = 0
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "operate_chain.npz")


@functools.lru_cache(maxsize=None)
def golden():
    """(mpo cores, the start canonicalised as the engine does it, {maxstep: (norm, dense state)}) of the reference's run"""
    g = np.load(GOLDEN)
    n = int(g["nsite"])
    mpo = [np.ascontiguousarray(g[f"mpo{i}"]) for i in range(n)]
    start = orc.canonicalize_site0([g[f"init{i}"] for i in range(n)])
    res = {ns: (float(g[f"n{ns}_norm"]), jo.dense_state([g[f"n{ns}_final{i}"] for i in range(n)])) for ns in (1, 10)}
    return mpo, start, res


@functools.lru_cache(maxsize=None)
def states(name):
    return ec.random_states(name, NSTATES)


@functools.lru_cache(maxsize=None)
def oracle_case(name, label, r, maxstep=MAXSTEP, conv_tol=0.0):
    """(norm, dense state, iterations) of oracle.operate on state r of the shape with the operator"""
    _, shift, mpo = ec.case(name, label)
    nrm, bra, it = orc.operate(states(name)[r], mpo, maxstep=maxstep, conv_tol=conv_tol, shift=shift)
    return nrm, jo.dense_state(bra), it


def state_defect(got, pin):
    """|got - pin|_2 of two dense states"""
    return float(np.linalg.norm(np.asarray(got) - np.asarray(pin)))


def defects(cores, mpo, shift, nsweeps):
    """the oracle's defect |1 - |<phi_k | phi_{k-1}>|| after double sweep k = 1 .. nsweeps (phi_0 = the start): what its
    convergence test compares with conv_tol"""
    prev = [np.asarray(c, dtype=np.complex128) for c in cores]
    out = []
    for k in range(1, nsweeps + 1):
        _, bra, _ = orc.operate(cores, mpo, maxstep=k, conv_tol=0.0, shift=shift)
        out.append(abs(1.0 - abs(orc.overlap(bra, prev))))
        prev = bra
    return out


def pad_mpo(cores, like):
    """the same operator with its MPO bonds zero-padded to those of ``like``"""
    out = []
    for w, ref in zip(cores, like):
        z = np.zeros(ref.shape, dtype=np.complex128)
        z[:w.shape[0], :, :, :w.shape[3]] = w
        out.append(z)
    return out


# ---- the iteration-count cases: (cores, mpo, shift, conv_tol, the sweep the oracle stops at) ----
@functools.lru_cache(maxsize=None)
def stop_cases():
    gm, gs, _ = golden()
    _, _, local = ec.case("mixed", "local")
    _, _, prod = ec.case("mixed", "product")
    st = states("mixed")
    return {
        # defects 0.532, 0.0289, 0.00867, 0.00341, 0.00127, 4.8e-4: only between sweeps 1 and 2 is the gap a factor 4
        "golden": (gs, gm, 0.0, 0.1, 2),
        # defects 0.697, 1.1e-3, 9.5e-5
        "mixed_local": (st[1], local, 0.0, 3e-4, 3),
        # a product operator keeps the bonds: exact after one double sweep, defect ~1e-16 at the second; its MPO bonds
        # padded with zeros to those of `local`, so that one call can hold both
        "mixed_product_padded": (st[0], pad_mpo(prod, local), 0.0, 3e-4, 2),
    }


# ---- the NumPy twin of k_batch_operate's walk ----
def _phase_qr(a, rng):
    """thin QR with arbitrary phases on diag(R): a gauge-free QR as bt_qr's"""
    q, r = np.linalg.qr(a)
    ph = np.exp(2j * np.pi * rng.random(r.shape[0]))
    return q * ph[None, :], np.conj(ph)[:, None] * r


def _heff(Lb, W, Rb, v):
    """bt_heff's three stages: X[(a,c)][(j,s)], Y[a][(i,t)][s], out[(a,i)][r]"""
    X = np.einsum("acb,bjs->acjs", Lb, v)
    Y = np.einsum("cijt,acjs->aits", W, X)
    return np.einsum("aits,rts->air", Y, Rb)


def _env_fwd(E, bra, ket, W):
    """bt_env in the forward roles: env (bra, mpo, ket) -> the block right of the site"""
    X = np.einsum("bca,bps->caps", bra.conj(), E)
    Y = np.einsum("pctq,caps->aqts", W, X)
    return np.einsum("aqts,str->aqr", Y, ket)


def _env_bwd(E, bra, ket, W):
    """the mirror image: the block left of the site from the one right of it"""
    X = np.einsum("acb,bps->caps", bra.conj(), E)
    Y = np.einsum("qctp,caps->aqts", W, X)
    return np.einsum("aqts,rts->aqr", Y, ket)


def twin(cores, mpo, shift=0.0, maxstep=10, conv_tol=1e-8, seed=0):
    """(norm, cores of phi, iterations, status) by the kernel's walk: one array of L + 1 blocks for both directions, the
    scalar term through overlap blocks and the identity core, the bra's R dropped, a QR with arbitrary phases"""
    rng = np.random.default_rng(seed)
    L = len(cores)
    ket = [np.array(c, dtype=np.complex128) for c in cores]
    bra = [c.copy() for c in ket]
    mpo = [np.asarray(w, dtype=np.complex128) for w in mpo]
    hs = shift != 0.0
    ident = [np.eye(c.shape[1], dtype=np.complex128)[None, :, :, None] for c in ket]
    one = np.ones((1, 1, 1), dtype=np.complex128)
    mix = [None] * (L + 1)
    ov = [None] * (L + 1)
    mix[0] = mix[L] = ov[0] = ov[L] = one
    for p in range(L - 1, 0, -1):
        mix[p] = _env_bwd(mix[p + 1], bra[p], ket[p], mpo[p])
        if hs:
            ov[p] = _env_bwd(ov[p + 1], bra[p], ket[p], ident[p])

    def apply(p):
        y = _heff(mix[p], mpo[p], mix[p + 1], ket[p])
        if hs:
            y = y + shift * _heff(ov[p], ident[p], ov[p + 1], ket[p])
        nrm = float(np.linalg.norm(y))
        if not nrm > 0.0:
            return nrm
        bra[p] = y / nrm
        return nrm

    nrm, it = 0.0, 1
    while True:
        prev = [c.copy() for c in bra]
        for p in range(L):
            nrm = apply(p)
            if not nrm > 0.0:
                return 0.0, bra, it, 3
            if p == L - 1:
                break
            dl, d, dr = ket[p].shape
            q, _ = _phase_qr(bra[p].reshape(dl * d, dr), rng)
            bra[p] = q.reshape(dl, d, dr)
            q, r = _phase_qr(ket[p].reshape(dl * d, dr), rng)
            ket[p] = q.reshape(dl, d, dr)
            ket[p + 1] = np.tensordot(r, ket[p + 1], axes=(1, 0))
            mix[p + 1] = _env_fwd(mix[p], bra[p], ket[p], mpo[p])
            if hs:
                ov[p + 1] = _env_fwd(ov[p], bra[p], ket[p], ident[p])
        for p in range(L - 1, -1, -1):
            nrm = apply(p)
            if not nrm > 0.0:
                return 0.0, bra, it, 3
            if p == 0:
                break
            dl, d, dr = ket[p].shape
            q, _ = _phase_qr(bra[p].reshape(dl, d * dr).T, rng)
            bra[p] = q.T.reshape(dl, d, dr)
            q, r = _phase_qr(ket[p].reshape(dl, d * dr).T, rng)
            ket[p] = q.T.reshape(dl, d, dr)
            ket[p - 1] = np.tensordot(ket[p - 1], r.T, axes=(2, 0))
            mix[p] = _env_bwd(mix[p + 1], bra[p], ket[p], mpo[p])
            if hs:
                ov[p] = _env_bwd(ov[p + 1], bra[p], ket[p], ident[p])
        if abs(1.0 - abs(cc.walk(bra, prev))) < conv_tol or it == maxstep:
            return nrm, bra, it, 0
        it += 1


# ---- the physics case: cross_cases' spin chain from a CORRELATED start, C(t) = <psi| A(t) B |psi> ----
# The start is the oracle's state of cross_cases' product start after two steps: every bond is at its exact limit (L = 4,
# D = 4), so B psi fits the bonds and the fit is exact.  A = sum_p SZ_p; B = sum_p SX_p ("mpo") or cross_cases' one-site
# B_OP ("site").
@functools.lru_cache(maxsize=None)
def corr_start():
    psi, _ = cc.oracle_runs()
    return orc.canonicalize_site0(psi[2], scale=1.0)


def corr_b(b_form):
    from . import cross_mpo_cases as xc

    if b_form == "mpo":
        return xc.b_mpo()
    return [(cc.B_OP[1] if p == cc.B_OP[0] else np.eye(2))[None, :, :, None].astype(np.complex128) for p in range(cc.L)]


@functools.lru_cache(maxsize=None)
def corr_oracle(b_form="mpo"):
    """the oracle route: orc.operate, then OracleMPS runs of psi and phi, then walk_mpo with A, times |B psi|"""
    from . import cross_mpo_cases as xc
    from . import pair_cases as pc

    nrm, phi, _ = orc.operate(corr_start(), corr_b(b_form), maxstep=10, conv_tol=1e-8)
    mpo = pc._spin_chain_mpo(cc.L)
    runs = [orc.OracleMPS([c.copy() for c in cores], mpo, integrator="arnoldi", thresh=1e-9, conserve_norm=False)
            for cores in (corr_start(), phi)]
    out = []
    for k in range(cc.NSTEPS + 1):
        out.append(nrm * xc.walk_mpo(runs[0].cores, runs[1].cores, xc.a_mpo()))
        if k < cc.NSTEPS:
            for st in runs:
                st.propagate(cc.DT)
    return np.array(out)


@functools.lru_cache(maxsize=None)
def corr_dense(b_form="mpo"):
    """dense expm on the 16-dimensional space"""
    from scipy.linalg import expm

    from . import cross_mpo_cases as xc
    from . import pair_cases as pc

    H = jo.dense_operator(pc._spin_chain_mpo(cc.L))
    psi0 = jo.dense_state(corr_start())
    phi0 = jo.dense_operator(corr_b(b_form)) @ psi0
    Aop = jo.dense_operator(xc.a_mpo())
    out = []
    for k in range(cc.NSTEPS + 1):
        U = expm(-1j * H * cc.DT * k)
        out.append(np.vdot(U @ psi0, Aop @ (U @ phi0)))
    return np.array(out)
