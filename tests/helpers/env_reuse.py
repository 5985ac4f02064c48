"""NumPy twin of the structured environment update's reuse of the local solve's folded operator (csrc/engine_apply.hip:
MpoSite::EdgeCache::rebuild decides it, Engine::env_update_fold runs it) and of the one-pass combine of two Strassen levels
(csrc/vecops.hip::strassen_combine2), for tests/test_env_reuse_host.py and tests/test_gpu_env_reuse.py.

Index sets as helpers/edge_mpo.structure gives them: S / E = {state: multiple} of the identity-fed states of the bond
left / right of the site.  Direction 0 (forward) consumes the left block L with S, direction 1 (backward) the right block R
with E; "in" is the consumed bond, "out" the other one, t0 the out states a general in state feeds.

The solve's operators (choose_apply_forms):
    GL[(a,i)][(b,j)] = sum_{c not in S} sum_{t in E} mu_t W[c,i,j,t] L[a,c,b]
    GR[(i,r)][(j,s)] = sum_{c in S} lam_c sum_t W[c,i,j,t] R[r,t,s]            (all t: every block out of S goes here)
Forward, one t0: GL = mu_t0 GL_t0, so block t0 += (1 / mu_t0) T^H (GL T) and the Gram core ws is untouched.
Backward, t0 = {c0} and no other state of S with a block: GR / lam_c0 = the update's operator + sum_{t in E} mu_t
W[c0,i,j,t] (x) 1; the second term is column c0 of ws, so the Gram core runs with that column zero and block c0 +=
(1 / lam_c0) conj(B)[a'][(i,r)] Z'[a][(i,r)],  Z' = B GR^T with the unmirrored B[a][(j,s)].
"""

from __future__ import annotations

import numpy as np


def blocks_at(orc, mpo, d, D, c, seed=1):
    """(envL[c], envR[c + 1]) of a random MPS in mixed-canonical form around site c, built with the oracle's own moves"""
    L = len(mpo)
    cores = orc.synthetic_mps([d] * L, D, seed=seed)
    left = np.ones((1, 1, 1), dtype=np.complex128)
    for p in range(c):
        A, sval = orc.qr_psi2Asigma(cores[p])
        left = orc.env_update_left(left, A, mpo[p])
        cores[p + 1] = np.tensordot(sval, cores[p + 1], axes=(1, 0))
    right = np.ones((1, 1, 1), dtype=np.complex128)
    for p in range(L - 1, c, -1):
        right = orc.env_update_right(right, cores[p], mpo[p])
    return left, right


def decide(W, S, E):
    """per direction: dict(t0, ws, reuse, alpha, ws_reuse) -- EdgeCache::rebuild's cores and its decision"""
    ml, d, _, mr = W.shape
    nz = np.abs(W).max(axis=(1, 2)) > 0
    out = []
    for side in (0, 1):
        mi, mo = (ml, mr) if side == 0 else (mr, ml)
        I, O = (S, E) if side == 0 else (E, S)

        def blk(i_, o_):
            return nz[i_, o_] if side == 0 else nz[o_, i_]

        def wel(i_, o_):
            return W[i_, :, :, o_] if side == 0 else W[o_, :, :, i_]

        t0 = [o for o in range(mo) if any(blk(i, o) for i in range(mi) if i not in I)]
        ws = np.zeros((d, d, mo), np.complex128)
        for i, wt in I.items():
            for o in range(mo):
                if blk(i, o):
                    ws[:, :, o] += wt * wel(i, o)
        rec = dict(t0=t0, ws=ws, reuse=False, alpha=None, ws_reuse=None)
        if len(t0) == 1:
            o = t0[0]
            ok = o in O and O[o] != 0
            if ok and side == 1:  # no other state of S may have put a block into GR (a zero multiple put none)
                ok = not any(nz[c, t] for c in S if c != o and S[c] != 0 for t in range(mr))
            if ok:
                rec.update(reuse=True, alpha=1.0 / O[o], ws_reuse=ws.copy())
                if side == 1:
                    rec["ws_reuse"][:, :, o] = 0
        out.append(rec)
    return out


def solve_gl(W, Lb, S, E):
    """the L-side operator of the solve, (dl d) x (dl d), rows (a, i), columns (b, j)"""
    ml, d, _, mr = W.shape
    dl = Lb.shape[0]
    G = np.zeros((dl, d, dl, d), np.complex128)
    for c in range(ml):
        if c in S:
            continue
        for t, mu in E.items():
            G += mu * np.einsum("ij,ab->aibj", W[c, :, :, t], Lb[:, c, :])
    return G.reshape(dl * d, dl * d)


def solve_gr(W, Rb, S, E):
    """the R-side operator of the solve, (d dr) x (d dr), rows (i, r), columns (j, s)"""
    ml, d, _, mr = W.shape
    dr = Rb.shape[0]
    G = np.zeros((d, dr, d, dr), np.complex128)
    for c, lam in S.items():
        for t in range(mr):
            G += lam * np.einsum("ij,rs->irjs", W[c, :, :, t], Rb[:, t, :])
    return G.reshape(d * dr, d * dr)


def _gram_part(T, ws):
    """out[a', t, r] = sum_{i,j} ws[i,j,t] G[(i,a')][(j,r)],  G = the Gram matrix of T (din, d, dout)"""
    G = np.einsum("aip,ajq->ipjq", T.conj(), T)
    return np.einsum("ijt,ipjq->ptq", ws, G)


def update_forward(W, Lb, T, S, E, allow_reuse=True):
    """(new left block (dr, mr, dr), whether the reuse formula ran): T (dl, d, dr)"""
    ml, d, _, mr = W.shape
    dl, _, dr = T.shape
    rec = decide(W, S, E)[0]
    Tm = T.reshape(dl * d, dr)
    if rec["reuse"] and allow_reuse:
        out = _gram_part(T, rec["ws_reuse"])
        Z = solve_gl(W, Lb, S, E) @ Tm
        out[:, rec["t0"][0], :] += rec["alpha"] * (Tm.conj().T @ Z)
        return out, True
    out = _gram_part(T, rec["ws"])
    for t in rec["t0"]:
        G = np.zeros((dl, d, dl, d), np.complex128)
        for c in range(ml):
            if c not in S:
                G += np.einsum("ij,ab->aibj", W[c, :, :, t], Lb[:, c, :])
        out[:, t, :] += Tm.conj().T @ (G.reshape(dl * d, dl * d) @ Tm)
    return out, False


def update_backward(W, Rb, B, S, E, allow_reuse=True):
    """(new right block (dl, ml, dl), whether the reuse formula ran): B (dl, d, dr), unmirrored"""
    ml, d, _, mr = W.shape
    dl, _, dr = B.shape
    rec = decide(W, S, E)[1]
    Bt = np.ascontiguousarray(B.transpose(2, 1, 0))  # the mirrored tensor (dr, d, dl) the update is written for
    if rec["reuse"] and allow_reuse:
        out = _gram_part(Bt, rec["ws_reuse"])
        Bm = B.reshape(dl, d * dr)
        Zp = Bm @ solve_gr(W, Rb, S, E).T  # Z'[a][(i,r)]
        out[:, rec["t0"][0], :] += rec["alpha"] * (Bm.conj() @ Zp.T)
        return out, True
    out = _gram_part(Bt, rec["ws"])
    Btm = Bt.reshape(dr * d, dl)
    for c0 in rec["t0"]:
        G = np.zeros((dr, d, dr, d), np.complex128)
        for t in range(mr):
            if t not in E:
                G += np.einsum("ij,rs->risj", W[c0, :, :, t], Rb[:, t, :])
        out[:, c0, :] += Btm.conj().T @ (G.reshape(dr * d, dr * d) @ Btm)
    return out, False


def combine2(M49: np.ndarray, qm: int, qn: int, out: np.ndarray | None) -> np.ndarray:
    """strassen_combine2: the (4 qm) x (4 qn) result from the 49 packed quarter-size products, product (k1, k2) at
    7 k1 + k2.  The four quadrants of every level-1 product first, then, quadrant by quadrant, the four level-1 sums, each
    in the order of strassen_blocks.combine; out is added to the final sums only."""
    m = M49.reshape(7, 7, qm, qn)
    h = [[((m[k, 0] + m[k, 3]) - m[k, 4]) + m[k, 6], m[k, 2] + m[k, 4], m[k, 1] + m[k, 3], ((m[k, 0] - m[k, 1]) + m[k, 2]) + m[k, 5]]
         for k in range(7)]
    c = np.empty((4 * qm, 4 * qn), np.complex128)
    for u in range(4):
        o = [((h[0][u] + h[3][u]) - h[4][u]) + h[6][u], h[2][u] + h[4][u], h[1][u] + h[3][u], ((h[0][u] - h[1][u]) + h[2][u]) + h[5][u]]
        for U in range(4):
            r0, c0 = (2 * (U >> 1) + (u >> 1)) * qm, (2 * (U & 1) + (u & 1)) * qn
            c[r0:r0 + qm, c0:c0 + qn] = o[U] if out is None else o[U] + out[r0:r0 + qm, c0:c0 + qn]
    return c
