"""The launch plan of the one-launch small-bond kernel (k_small_site) stated independently of csrc/small_chain_plan.h, for
tests/test_small_plan_host.py: the extents of the three chains from the formulas in csrc/small_site.h, what the kernel
keeps in LDS from its use of the pointers (csrc/small_site.hip), the conditions of an admissible plan and an exhaustive
search over them.  Plus the loader of the g++ shim over the header itself.  NumPy-free, no GPU."""

from __future__ import annotations

import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "pytdscf_amd", "csrc", "small_chain_plan.h")

KINDS = {"heff": 0, "keff": 1, "env": 2}
LDS_CAP = 155 * 1024
ZC = 16  # bytes of a complex element


# ---------------------------------------------------------------------------------------------------------------------
# the shim
# ---------------------------------------------------------------------------------------------------------------------
class Shim:
    def __init__(self, out_dir, header=None):
        out = os.path.join(str(out_dir), "libssp_shim.so")
        cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "small_plan_shim.cpp"), "-o", out]
        if header is not None:
            cmd.insert(1, f'-DSSP_HEADER="{header}"')
        subprocess.run(cmd, check=True)
        lib = C.CDLL(out)
        ip = C.POINTER(C.c_int)
        lib.ssp_consts.argtypes = [ip]
        lib.ssp_extents.argtypes = [C.c_int, ip, ip]
        lib.ssp_plan.argtypes = [C.c_int, ip, C.c_int, C.c_int, ip]
        lib.ssp_carve.argtypes = [C.c_int, ip, C.c_int, ip, C.POINTER(C.c_ulonglong)]
        self.lib = lib
        c = (C.c_int * 6)()
        lib.ssp_consts(c)
        self.MAXG, self.THREADS, self.WAVES, self.PAYMAX, self.MAXK, self.LDS_PLAN = list(c)

    @staticmethod
    def _dims(dims):
        return (C.c_int * 5)(*(list(dims) + [0] * (5 - len(dims))))

    def extents(self, kind, dims):
        e = (C.c_int * 8)()
        w = self.lib.ssp_extents(KINDS[kind], self._dims(dims), e)
        assert w >= 0
        return dict(zip(("na", "nb", "nc", "nj", "ni", "nt", "ns", "nr"), e), w=bool(w))

    def plan(self, kind, dims, exp_mode, n_cu):
        """(nsc, cs, spw, a_resident) or None where the planner refuses"""
        p = (C.c_int * 4)()
        ok = self.lib.ssp_plan(KINDS[kind], self._dims(dims), int(exp_mode), n_cu, p)
        assert ok >= 0
        return tuple(p) if ok else None

    def carve(self, kind, dims, exp_mode, plan):
        """offsets in complex elements"""
        o = (C.c_ulonglong * 9)()
        assert self.lib.ssp_carve(KINDS[kind], self._dims(dims), int(exp_mode), (C.c_int * 4)(*plan), o) == 0
        return dict(zip(("As", "Rs", "Ws", "Bs", "Xs", "Ys", "Sg", "misc", "total"), o))


# ---------------------------------------------------------------------------------------------------------------------
# the chains (csrc/small_site.h:  out[a][i][r] = sum_{b,c,j,t,s} A(a;c,b) B(b,j,s) W2[(i,t)][(c,j)] R(r,t,s))
# ---------------------------------------------------------------------------------------------------------------------
def extents(kind, dims):
    """index ranges of the chain, read off the contraction each kind is"""
    if kind == "heff":  # sigma[a,i,r] = sum L[a,c,b] W[c,i,j,t] R[r,t,s] psi[b,j,s]
        dl, d, dr, ml, mr = dims
        return dict(na=dl, nb=dl, nc=ml, nj=d, ni=d, nt=mr, ns=dr, nr=dr, w=True)
    if kind == "keff":  # sigma'[a,r] = sum L[a,c,b] sigma[b,s] R[r,c,s]: no physical index, t = c
        d1, d2, m = dims
        return dict(na=d1, nb=d1, nc=m, nj=1, ni=1, nt=m, ns=d2, nr=d2, w=False)
    # env'[a,q,r] = sum conj(T)[b,c,a] env[b,p,s] W[(q,t),(c,p)] T[s,t,r]: slab = new bra bond, j = old MPO bond p,
    # i = new MPO bond q, c and t the physical indices of bra and ket, b and s the old bra and ket bonds
    din, min_, d, dout, mout = dims
    return dict(na=dout, nb=din, nc=d, nj=min_, ni=mout, nt=d, ns=din, nr=dout, w=True)


def lds_regions(e, plan, exp_mode, threads=512, maxk=21):
    """What a workgroup of k_small_site keeps in LDS under a plan, as {name: complex elements it indexes}, from the
    kernel's own loops:
      As   resident: nc*nb per slab of the group, up to spw of them (t < nAone * nsl); re-staged: one slab's
      Rs   (nt * cs) x nr, padded columns written as zeros (t < kk * nr)
      Ws   (ni * nt) x (nc * nj), only with a W stage
      Bs   nb x (nj * cs); EXP mode also the six maxk x maxk matrices of the projected exponential (Tm .. Qm)
      Xs   stage 1's output nc x (nj * cs)
      Ys   stage 2's output (ni * nt) x cs; without a W stage stage 3 reads X in its place
      Sg   stage 3's output ni x nr
      misc pay / red [paymax], wsh [waves * paymax] doubles, alpha / coef / cprev [maxk], hess [(maxk + 1) * maxk],
           beta [maxk], invb [maxk + 1] doubles, ctl [4] ints, in this order
    """
    nsc, cs, spw, res = plan
    waves, paymax = threads // 64, 2 * maxk + 2
    r = {}
    r["As"] = e["nc"] * e["nb"] * (min(spw, e["na"]) if res else 1)
    r["Rs"] = e["nt"] * cs * e["nr"]
    r["Ws"] = e["ni"] * e["nt"] * e["nc"] * e["nj"] if e["w"] else 0
    r["Bs"] = max(e["nb"] * e["nj"] * cs, 6 * maxk * maxk if exp_mode else 0)
    r["Xs"] = e["nc"] * e["nj"] * cs
    r["Ys"] = e["ni"] * e["nt"] * cs if e["w"] else 0
    r["Sg"] = e["ni"] * e["nr"]
    misc_bytes = 8 * (2 * paymax + waves * paymax) + ZC * (3 * maxk + (maxk + 1) * maxk) + 8 * (maxk + maxk + 1) + 4 * 4
    r["misc"] = -(-misc_bytes // ZC)
    return r


def sg_may_alias_x(e, plan):
    """stage 3 reads Y and R only when there is a W stage, so its output may then overwrite X -- if it fits there"""
    return e["w"] and e["ni"] * e["nr"] <= e["nc"] * e["nj"] * plan[1]


def lds_bytes(e, plan, exp_mode, threads=512, maxk=21):
    r = lds_regions(e, plan, exp_mode, threads, maxk)
    n = sum(r.values()) - (r["Sg"] if sg_may_alias_x(e, plan) else 0)
    # a resident A is carved for spw slabs whatever the last group holds
    if plan[3]:
        n += e["nc"] * e["nb"] * (max(plan[2], 1) - min(plan[2], e["na"]))
    return n * ZC


def grid_of(e, plan):
    return -(-e["na"] // max(plan[2], 1)) * plan[0]


def plan_defects(e, plan, n_cu):
    """what is wrong with a plan as a launch layout (LDS apart), as a list of words"""
    nsc, cs, spw, res = plan
    bad = []
    if not (nsc * cs >= e["ns"] and (nsc - 1) * cs < e["ns"]):
        bad.append("chunks do not tile s or the last one is empty")
    if nsc not in (1, 2, 4, 8):
        bad.append("nsc")
    if nsc > 1 and cs < 4:
        bad.append("chunk narrower than 4")
    if spw < 1 or (-(-e["na"] // spw) - 1) * spw >= e["na"]:
        bad.append("empty slab group")
    elif grid_of(e, plan) > min(n_cu, 256):
        bad.append("grid exceeds the resident bound")
    if spw > 1 and n_cu > 64:
        bad.append("several slabs per workgroup on a large slice")
    if res == 0 and spw <= 1:
        bad.append("re-staged A with one slab per workgroup")
    if res not in (0, 1):
        bad.append("a_resident")
    return bad


def search(e, exp_mode, n_cu, threads=512, maxk=21):
    """every admissible (nsc, cs, spw, a_resident), by brute force"""
    found = []
    if min(e["na"], e["nb"], e["ns"], e["nr"]) < 1:
        return found
    for nsc in (1, 2, 4, 8):
        cs = -(-e["ns"] // nsc)
        for spw in (1, 2, 4, 8, 16, 32, 64):
            for res in (1, 0):
                plan = (nsc, cs, spw, res)
                if plan_defects(e, plan, n_cu):
                    continue
                if lds_bytes(e, plan, exp_mode, threads, maxk) <= LDS_CAP:
                    found.append(plan)
    return found
