"""The deflated improved relaxation (excited states by the penalty method, k_batch_relax_defl in csrc/batch_site.hip)
restated in NumPy on top of ``oracle.tdvp_oracle``, which is imported and not edited.

Every local solve is the oracle's ``lanczos_ground_state`` on

    H_eff + shift + sum_k w_k |q_k><q_k|,   q_k = OL_k[p] . phi_k[p] . OR_k[p + 1]^T,

``phi_k`` a stored state and ``OL_k[b]`` / ``OR_k[b]`` the overlap blocks <replica's basis | phi_k's basis> of bond ``b``
from the left / right.  The right blocks are built when the model is made; after a gauge move the block of the bond the
centre crossed is rewritten from the new ``A`` (``B``).  The Krylov dimension of every local solve is recorded.

Shared by tests/test_batch_deflate_host.py and tests/test_gpu_batch_deflate.py, with the case table below."""

from __future__ import annotations

import functools

import numpy as np

from helpers import relax_cases as rc
from oracle import tdvp_oracle as orc

WEIGHT = 4.0
NSTATES = 4
# full-bond chains: (dims, D, seeds); the dense spectrum is reached exactly
FULL = (
    ((2,) * 4, 4, (0, 1, 2, 3)),
    ((2,) * 6, 8, (0, 1, 2)),
    ((3,) * 4, 9, (0, 1)),
    ((2, 3, 2, 3, 2), 12, (0, 1)),
)
TRUNCATED = ((2,) * 8, 4, (0, 1))  # variational: parity with this model only
SMALL_GAP = ((2,) * 6, 8, 1)       # dims, D, seed: the gap E_1 - E_0 is 0.508


def state_start(dims, D, seed, k):
    """the fresh start of state k"""
    return rc.start(dims, D, seed + 17 * k)


class DeflatedRelax:
    """improved relaxation of ``cores`` (centre at site 0) under ``mpo`` against ``stored`` = [(cores, weight), ...]"""

    def __init__(self, cores, mpo, stored, thresh=1e-9, shift=0.0):
        self.st = orc.OracleMPS([np.array(c) for c in cores], mpo, relax="improved", thresh=thresh, shift=shift)
        self.st.build_right_envs()
        self.L = len(cores)
        self.phi = [[np.asarray(c, dtype=np.complex128) for c in s] for s, _ in stored]
        self.w = [float(w) for _, w in stored]
        self.kdims = []  # the Krylov dimension of every local solve, in order
        one = np.ones((1, 1), dtype=np.complex128)
        self.OL = [{0: one} for _ in self.phi]
        self.OR = [{self.L: one} for _ in self.phi]
        for k, phi in enumerate(self.phi):
            for p in range(self.L - 1, 0, -1):
                self.OR[k][p] = self._right(self.OR[k][p + 1], self.st.cores[p], phi[p])

    @staticmethod
    def _left(T, A, ket):  # OL'[i][j] = sum conj(A[m,s,i]) T[m][n] ket[n,s,j]
        return np.einsum("msi,mn,nsj->ij", A.conj(), T, ket)

    @staticmethod
    def _right(T, B, ket):  # OR'[r][v] = sum conj(B[r,s,t]) T[t][u] ket[v,s,u]
        return np.einsum("rst,tu,vsu->rv", B.conj(), T, ket)

    def q(self, k, p):
        return np.einsum("ab,bsr,tr->ast", self.OL[k][p], self.phi[k][p], self.OR[k][p + 1])

    def matvec(self, p):
        base = self.st._heff(p)
        qs = [self.q(k, p) for k in range(len(self.phi))]

        def mv(x):
            y = base(x)
            for w, q in zip(self.w, qs):
                y = y + w * q * np.vdot(q, x)
            return y

        return mv

    def solve(self, p):
        """the local solve at site p in place; returns (k, the Ritz value <x|Op|x> of the normalised result)"""
        st = self.st
        mv = self.matvec(p)
        new, k = orc.lanczos_ground_state(mv, st.cores[p], st.thresh)
        st.kprev[p] = k
        self.kdims.append(k)
        st.cores[p] = new / np.linalg.norm(new)
        return k, float(np.vdot(st.cores[p], mv(st.cores[p])).real)

    def half(self, forward):
        st, n = self.st, self.L
        sites = range(n) if forward else range(n - 1, -1, -1)
        end = n - 1 if forward else 0
        theta = None
        for p in sites:
            _, theta = self.solve(p)
            if p == end:
                break
            if forward:
                A, sval = orc.qr_psi2Asigma(st.cores[p])
                st.cores[p] = A
                st.left[p + 1] = orc.env_update_left(st.left[p], A, st.mpo[p])
                for k, phi in enumerate(self.phi):
                    self.OL[k][p + 1] = self._left(self.OL[k][p], A, phi[p])
                st.cores[p + 1] = np.tensordot(sval, st.cores[p + 1], axes=(1, 0))
            else:
                sval, B = orc.qr_psi2sigmaB(st.cores[p])
                st.cores[p] = np.ascontiguousarray(B)
                st.right[p - 1] = orc.env_update_right(st.right[p], st.cores[p], st.mpo[p])
                for k, phi in enumerate(self.phi):
                    self.OR[k][p] = self._right(self.OR[k][p + 1], st.cores[p], phi[p])
                st.cores[p - 1] = np.tensordot(st.cores[p - 1], sval, axes=(2, 0))
        st.center = end
        return theta

    def step(self):
        """a full step; returns E_n, the Ritz value of the solve at site 0 (energy + penalties)"""
        self.half(True)
        return self.half(False)

    def energy(self):
        return float(self.st.expectation().real)

    @property
    def cores(self):
        return [c.copy() for c in self.st.cores]


def run_states(mpo, dims, D, seed, nstates=NSTATES, nsteps=2, weight=WEIGHT, starts=None, shift=0.0):
    """states 0 .. nstates-1 one after the other: state k from ``state_start(.., k)`` (or starts[k]) against the states
    before it with ``weight`` each.  Returns dict(energies [k], ritz [k], cores [k], kmax, overlaps [k][j])"""
    stored, energies, ritz, states, kmax = [], [], [], [], 0
    for k in range(nstates):
        s0 = starts[k] if starts is not None else state_start(dims, D, seed, k)
        m = DeflatedRelax(s0, mpo, stored, shift=shift)
        th = None
        for _ in range(nsteps):
            th = m.step()
        kmax = max(kmax, max(m.kdims))
        energies.append(m.energy())
        ritz.append(th)
        states.append(m.cores)
        stored.append((m.cores, weight))
    ov = np.array([[orc.overlap(states[j], states[k]) for k in range(nstates)] for j in range(nstates)])
    return dict(energies=np.array(energies), ritz=np.array(ritz), cores=states, kmax=kmax, overlaps=ov)


@functools.lru_cache(maxsize=None)
def heis_states(dims, D, seed, nstates=NSTATES, nsteps=2, weight=WEIGHT):
    return run_states(rc.heisenberg_mpo(dims, seed), dims, D, seed, nstates, nsteps, weight)


def full_cases():
    return [(dims, D, seed) for dims, D, seeds in FULL for seed in seeds]


def noisy(cores, rel, seed=11):
    """the cores with relative noise ``rel`` on every element (not re-canonicalised: rel is at rounding level)"""
    rng = np.random.default_rng(seed)
    return [c * (1.0 + rel * rng.standard_normal(c.shape)) for c in cores]
